"""+ASC (ascertainment-bias correction, phylokernel.h:655-725 and :1124-1187) in the forms that batch solver work: the
batched NNI evaluators on one engine (k_newton_batch), on pattern shards and communicator ranks (5 result rows per task
and Newton step), and the one-submission branch-length sweep.  Each is compared with the one-branch-at-a-time form of the
same engine, with the oracle, and (shards) with the unsharded engine.

The alignments are built as in test_newton_oracle_gpu.py: simulate, drop the constant patterns, append one unobserved
constant pattern per state, nsites = sum of the frequencies.  tests/test_asc_batch_inputs.py checks on the CPU that the
oracle gives a finite lnL and prob_const < 1 for every input used here."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from test_parity_gpu import LNL_RTOL
from test_sweep_gpu import run_both

pytestmark = pytest.mark.gpu

SEQ_OTHER = 3

# n, ncat, seq_type, ntaxa, nsites
NNI1_CASES = [(4, 4, 0, 14, 600), (20, 4, 1, 9, 300), (64, 1, 2, 7, 150),
              (4, 4, 0, 40, 70000),            # several workgroups per task, posted exchange
              (3, 4, SEQ_OTHER, 10, 500)]      # an embedded state count
NNI5_CASES = [(4, 4, 0, 13, 500), (20, 4, 1, 8, 250)]
ORACLE_CASES = [(4, 4, 0, 12, 800), (20, 4, 1, 9, 300)]
ABI_CASE = (4, 4, 0, 16, 6000)
SHARD_CASES = [(4, 4, 0, 11, 1500), (20, 4, 1, 11, 900)]
SWEEP_CASES = [(4, 4, 0, 14, 400), (4, 4, 0, 20, 30000), (20, 4, 1, 12, 1500), (64, 1, 2, 9, 500)]
SWEEP_DIVERGED_CASE = (4, 4, 0, 10, 600)


def asc_inputs(synth, n, ncat, seq_type, ntaxa, nsites):
    """-> (newick, pat, freq, n_unobs, nsites, model) of a variable-sites-only alignment"""
    seed = 8800 + 7 * n + ntaxa + nsites % 89
    if n == 4:
        model = synth.gtr_model(alpha=0.9, ncat=ncat)
    else:
        model = synth.random_reversible_model(n, seed, alpha=0.9 if ncat > 1 else None, ncat=ncat)
    nwk = synth.random_tree_newick(ntaxa, seed + 1, 0.02, 0.15)
    st = synth.simulate_alignment(nwk, model, nsites, seed + 2)
    pat, freq = synth.compress_patterns(st)
    const = np.all(pat == pat[0][None, :], axis=0)
    pat, freq = np.ascontiguousarray(pat[:, ~const]), freq[~const].copy()
    ns = float(freq.sum())
    pat = np.ascontiguousarray(np.concatenate([pat, np.tile(np.arange(n, dtype=np.uint8)[None, :], (ntaxa, 1))], axis=1))
    freq = np.concatenate([freq, np.zeros(n)])
    return nwk, pat, freq, n, ns, model


def asc_tree(pkg, inputs, n, seq_type, mem_mode=0, asc=True, attach=lambda t: t.attach_engine(0)):
    nwk, pat, freq, nun, ns, model = inputs
    t = pkg.PhyloTree(nwk)
    t.set_mem_mode(mem_mode)
    t.set_alignment(n, seq_type, pat, freq)
    if asc:
        t.set_ascertainment(nun, ns)
    else:
        t.set_ascertainment(0, 0.0)
    t.set_model(model)
    t.set_likelihood_kernel(pkg.LK_EIGEN_HIP)
    attach(t)
    return t


def asc_oracle(oracle, inputs, n, seq_type, newick=None):
    nwk, pat, freq, nun, ns, model = inputs
    return oracle.OracleTree(newick or nwk, n, seq_type, pat, freq, None, model, n_unobs=nun, nsites=ns)


# ---------------------------------------------------------------------------------------
# 1. the batch equals the evaluator that goes branch by branch
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,ncat,seq_type,ntaxa,nsites", NNI1_CASES)
def test_asc_batch_matches_branch_by_branch(pkg, synth, oracle, n, ncat, seq_type, ntaxa, nsites):
    inputs = asc_inputs(synth, n, ncat, seq_type, ntaxa, nsites)
    t = asc_tree(pkg, inputs, n, seq_type, mem_mode=pkg.LM_ALL_BRANCH)
    lnl = t.compute_likelihood()
    ref, _ = asc_oracle(oracle, inputs, n, seq_type).likelihood()
    assert abs(lnl - ref) <= LNL_RTOL * abs(ref)
    tree0 = t.tree_string()
    batch = t.evaluate_nnis_batch()
    assert len(batch) == 2 * (ntaxa - 3)
    assert t.tree_string() == tree0
    assert abs(t.compute_likelihood() - lnl) <= 1e-12 * abs(lnl)
    by_branch = {}
    for m in batch:
        by_branch.setdefault((m["node1"], m["node2"]), []).append(m)
    assert all(len(v) == 2 for v in by_branch.values())
    for (a, b), two in list(by_branch.items())[:12]:
        seq = t.nni_for_branch(a, b, nni5=False)
        for c in range(2):
            newloglh, nei1, nei2, lens = seq[c]
            assert (two[c]["node1_nei"], two[c]["node2_nei"]) == (nei1, nei2)
            print("nni1", n, (a, b, c), two[c]["new_len"], lens[0], two[c]["newloglh"], newloglh)
            assert abs(two[c]["new_len"] - lens[0]) <= 1e-9 * max(1e-6, lens[0])
            assert abs(two[c]["newloglh"] - newloglh) <= 1e-10 * abs(newloglh)
    again = t.evaluate_nnis_batch()
    assert [(m["new_len"], m["newloglh"]) for m in again] == [(m["new_len"], m["newloglh"]) for m in batch]


@pytest.mark.parametrize("n,ncat,seq_type,ntaxa,nsites", NNI5_CASES)
def test_asc_nni5_batch_matches_branch_by_branch(pkg, synth, oracle, n, ncat, seq_type, ntaxa, nsites):
    inputs = asc_inputs(synth, n, ncat, seq_type, ntaxa, nsites)
    t = asc_tree(pkg, inputs, n, seq_type, mem_mode=pkg.LM_ALL_BRANCH)
    lnl = t.compute_likelihood()
    tree0 = t.tree_string()
    batch = t.evaluate_nnis5_batch()
    assert len(batch) == 2 * (ntaxa - 3) and t.tree_string() == tree0
    assert abs(t.compute_likelihood() - lnl) <= 1e-12 * abs(lnl)
    for k in range(0, min(len(batch), 24), 2):
        a, b = batch[k]["node1"], batch[k]["node2"]
        seq = t.nni_for_branch(a, b, nni5=True)
        for c in range(2):
            newloglh, nei1, nei2, lens = seq[c]
            m = batch[k + c]
            assert (m["node1_nei"], m["node2_nei"]) == (nei1, nei2)
            print("nni5", n, (a, b, c), m["new_lens"], lens, m["newloglh"], newloglh)
            np.testing.assert_allclose(m["new_lens"], lens, rtol=1e-7, atol=1e-12)
            assert abs(m["newloglh"] - newloglh) <= 1e-9 * abs(newloglh)
    again = t.evaluate_nnis5_batch()
    assert [m["newloglh"] for m in again] == [m["newloglh"] for m in batch]


# ---------------------------------------------------------------------------------------
# 2. the C ABI: iqhip_optimize_branch_batch against iqhip_optimize_branch + iqhip_lnl_from_theta
# ---------------------------------------------------------------------------------------
class Result(C.Structure):
    _fields_ = [("optx", C.c_double), ("d2l", C.c_double), ("lnl", C.c_double), ("nsteps", C.c_int32), ("status", C.c_int32)]


def abi_batch_and_single(pkg, synth, oracle, asc):
    """10, 3, 10 tasks with several workgroups per task; -> (batch results of the three calls, single-branch results)"""
    n, ncat, seq_type, ntaxa, nsites = ABI_CASE
    lib = pkg.libiqhip()

    class Task(C.Structure):
        _fields_ = [("ops", C.c_void_p), ("nops", C.c_int32), ("max_steps", C.c_int32), ("a", pkg.BranchEnd), ("b", pkg.BranchEnd),
                    ("xguess", C.c_double), ("x1", C.c_double), ("x2", C.c_double), ("xacc", C.c_double)]

    dp = C.POINTER(C.c_double)
    lib.iqhip_optimize_branch_batch.argtypes = [C.c_void_p, C.POINTER(Task), C.c_int, dp, C.POINTER(Result)]
    inputs = asc_inputs(synth, n, ncat, seq_type, ntaxa, nsites)
    t = asc_tree(pkg, inputs, n, seq_type, mem_mode=pkg.LM_ALL_BRANCH, asc=asc)
    ot = asc_oracle(oracle, inputs, n, seq_type)
    assert t.nptn > 4 * 256                      # several workgroups per task
    t.compute_likelihood()
    t.compute_all_partial_lh()
    inner = [(x, y) for x in range(t.num_nodes) for y, _ in t.neighbors(x) if x < y and not ot.is_leaf(x) and not ot.is_leaf(y)]
    assert len(inner) >= 10
    ends = [(pkg.key_end(t.neighbor_info(x, y)["key"]), pkg.key_end(t.neighbor_info(y, x)["key"])) for x, y in inner[:10]]
    tasks = [Task(None, 0, 10, a, b, 0.05 + 0.01 * k, 1e-6, 100.0, 1e-6) for k, (a, b) in enumerate(ends)]

    def run(sub):
        res = (Result * len(sub))()
        assert lib.iqhip_optimize_branch_batch(t.engine, (Task * len(sub))(*sub), len(sub), None, res) == 0, lib.iqhip_last_error()
        return [(r.optx, r.d2l, r.lnl, r.nsteps, r.status) for r in res]

    batches = [run(tasks), run(tasks[4:7]), run(tasks)]
    single = []
    for k, (a, b) in enumerate(ends):
        optx, d2l, lnl, ns = C.c_double(), C.c_double(), C.c_double(), C.c_int()
        rc = lib.iqhip_optimize_branch(t.engine, None, 0, a, b, 0.05 + 0.01 * k, 1e-6, 100.0, 1e-6, 10, None, C.byref(optx),
                                       C.byref(d2l), C.byref(ns))
        assert rc == 0, lib.iqhip_last_error()
        assert lib.iqhip_lnl_from_theta(t.engine, optx.value, C.byref(lnl)) == 0, lib.iqhip_last_error()
        single.append((optx.value, d2l.value, lnl.value, ns.value, rc))
    return batches, single


def test_asc_batch_through_the_c_abi(pkg, synth, oracle):
    (first, small, third), single = abi_batch_and_single(pkg, synth, oracle, asc=True)
    for got, want in ((first, single), (third, single), (small, single[4:7])):
        for g, w in zip(got, want):
            print("abi", g, w)
            assert g[3:] == w[3:] == (w[3], 0)                      # same step count, status ok
            np.testing.assert_allclose(g[:3], w[:3], rtol=1e-10)    # optx, d2l, lnl


# ---------------------------------------------------------------------------------------
# 3. the oracle: minimizeNewton over its +ASC derivative on the swapped tree, and that tree's lnL
# ---------------------------------------------------------------------------------------
def oracle_swap(ot, node1, node2, nei1, nei2, new_len):
    """the NNI that exchanges subtree nei1 (at node1) with subtree nei2 (at node2); the pendant lengths move with them"""
    e1 = [e for e in ot.adj[node1] if e[0] == nei1][0]
    e2 = [e for e in ot.adj[node2] if e[0] == nei2][0]
    e1[0], e2[0] = nei2, nei1
    e1[1], e2[1] = e2[1], e1[1]
    [e for e in ot.adj[nei1] if e[0] == node1][0][0] = node2
    [e for e in ot.adj[nei2] if e[0] == node2][0][0] = node1
    ot.set_length(node1, node2, new_len)


NNI_MAX_NR_STEP = 10   # the step limit of the NNI evaluators (phylotree.h), batched and branch by branch alike


def oracle_candidates(make_ot, batch):
    """every candidate of `batch` on the oracle, each on a fresh tree from make_ot():
    [(optimum, evaluated points, lnL of the swapped tree at the batch's length)]"""
    out = []
    for k, m in enumerate(batch):
        ot = make_ot()
        a, b = m["node1"], m["node2"]
        # (the second swap of a branch starts from the length the first swap's solve left: phylotree.cpp:3036-3051)
        start = ot.length(a, b) if k % 2 == 0 else batch[k - 1]["new_len"]
        oracle_swap(ot, a, b, m["node1_nei"], m["node2_nei"], start)
        optx, _, pts, status = ot.minimize_newton(a, b, 1e-6, start, 100.0, 1e-6, NNI_MAX_NR_STEP)
        assert status == "ok"
        ot.set_length(a, b, m["new_len"])
        out.append((optx, pts, ot.branch_lnl(a, b)[0]))
    return out


@pytest.mark.parametrize("n,ncat,seq_type,ntaxa,nsites", ORACLE_CASES)
def test_asc_batch_against_the_oracle(pkg, synth, oracle, n, ncat, seq_type, ntaxa, nsites):
    inputs = asc_inputs(synth, n, ncat, seq_type, ntaxa, nsites)
    t = asc_tree(pkg, inputs, n, seq_type, mem_mode=pkg.LM_ALL_BRANCH)
    t.compute_likelihood()
    c0 = t.num_derv_calls
    batch = t.evaluate_nnis_batch()
    nevals = t.num_derv_calls - c0
    ref = oracle_candidates(lambda: asc_oracle(oracle, inputs, n, seq_type), batch)
    assert all(r[0] <= 0.95 * 100.0 for r in ref)                     # no candidate takes the diverged-solve detour
    best = max(range(len(batch)), key=lambda k: batch[k]["newloglh"])
    optx, pts, lnl = ref[best]
    print("oracle", n, batch[best], optx, len(pts), lnl, nevals, sum(len(r[1]) for r in ref))
    assert abs(batch[best]["new_len"] - optx) <= 1e-9 * max(1.0, abs(optx))
    assert abs(batch[best]["newloglh"] - lnl) <= LNL_RTOL * abs(lnl)
    assert nevals == sum(len(r[1]) for r in ref)                      # derivative evaluations, all candidates together


# ---------------------------------------------------------------------------------------
# 4. pattern shards and communicator ranks: the tasks side by side, 5 rows per task and step
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,ncat,seq_type,ntaxa,nsites", SHARD_CASES)
@pytest.mark.parametrize("setup", ["host2", "comm1", "rccl1"])
def test_asc_batched_tasks_share_one_reduction_on_shards(pkg, synth, oracle, monkeypatch, setup, n, ncat, seq_type, ntaxa, nsites):
    inputs = asc_inputs(synth, n, ncat, seq_type, ntaxa, nsites)
    t = asc_tree(pkg, inputs, n, seq_type, mem_mode=pkg.LM_ALL_BRANCH)
    if setup == "comm1":
        def attach(x):
            x.attach_engine(0)
            x.attach_comm(1, 0, pkg.comm_unique_id())
    elif setup == "rccl1":   # the grouped in-stream all-reduce of 5m doubles, device state machines
        def attach(x):
            x.attach_engine_sharded([0], pkg.REDUCE_RCCL)
    else:
        def attach(x):
            x.attach_engine_sharded([0, 0], pkg.REDUCE_HOST)
    ts = asc_tree(pkg, inputs, n, seq_type, mem_mode=pkg.LM_ALL_BRANCH, attach=attach)
    lnl = t.compute_likelihood()
    assert abs(ts.compute_likelihood() - lnl) <= 1e-12 * abs(lnl)
    plain = t.evaluate_nnis_batch()
    lib = pkg.libiqhip()

    def counted(run):   # -> (result, derivative evaluations, all-reduces of a communicator rank)
        cnt0 = cnt1 = None
        avg, cnt = C.c_double(), C.c_int64()
        if setup == "comm1":
            lib.iqhip_timing_enable(ts.engine, 1)
            lib.iqhip_timing_collective_read(ts.engine, C.byref(avg), C.byref(cnt), 1)
        c0 = ts.num_derv_calls
        out = run()
        nev = ts.num_derv_calls - c0
        if setup == "comm1":
            lib.iqhip_timing_collective_read(ts.engine, C.byref(avg), C.byref(cnt), 1)
            cnt1 = cnt.value
            lib.iqhip_timing_enable(ts.engine, 0)
        return out, nev, cnt1

    monkeypatch.setenv("IQHIP_BATCH_SEQUENTIAL", "1")
    seq, ev_seq, nseq = counted(ts.evaluate_nnis_batch)
    monkeypatch.delenv("IQHIP_BATCH_SEQUENTIAL")
    side, ev_side, nside = counted(ts.evaluate_nnis_batch)
    assert len(plain) == len(seq) == len(side) == 2 * (ntaxa - 3) == 16
    if setup == "comm1":   # 16 tasks: one all-reduce per Newton step of the slowest task instead of one per task and step
        print("collectives", n, nside, nseq)
        assert nside * 6 <= nseq, (nside, nseq)
    assert ev_side == ev_seq                                         # step counts
    for mp, ms, mb in zip(plain, seq, side):
        print("shards", n, setup, mp["new_len"], ms["new_len"], mb["new_len"], mp["newloglh"], ms["newloglh"], mb["newloglh"])
        assert ms["new_len"] == mb["new_len"], (ms, mb)              # same sums in the same order: same iterates
        assert abs(ms["newloglh"] - mb["newloglh"]) <= 1e-12 * abs(ms["newloglh"])
        assert abs(mp["new_len"] - mb["new_len"]) <= 1e-8 * max(mp["new_len"], 1e-6)
        assert abs(mp["newloglh"] - mb["newloglh"]) <= 1e-10 * abs(mp["newloglh"])
    monkeypatch.setenv("IQHIP_BATCH_CHUNK", "3")
    chunked = ts.evaluate_nnis_batch()
    monkeypatch.delenv("IQHIP_BATCH_CHUNK")
    assert [(m["new_len"], m["newloglh"]) for m in chunked] == [(m["new_len"], m["newloglh"]) for m in side]
    five, five_s = t.evaluate_nnis5_batch(), ts.evaluate_nnis5_batch()
    for m, ms in zip(five, five_s):
        assert abs(m["newloglh"] - ms["newloglh"]) <= 1e-9 * abs(m["newloglh"])


# ---------------------------------------------------------------------------------------
# 5. one-submission sweeps
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,ncat,seq_type,ntaxa,nsites", SWEEP_CASES)
def test_asc_sweep_equals_the_per_branch_form(pkg, synth, oracle, n, ncat, seq_type, ntaxa, nsites):
    inputs = asc_inputs(synth, n, ncat, seq_type, ntaxa, nsites)
    out = run_both(lambda: asc_tree(pkg, inputs, n, seq_type), iterations=2, start=0.15)
    (l0, len0, c0, s0, _), (l1, len1, c1, s1, t1) = out[False], out[True]
    assert len0.keys() == len1.keys()
    for k in len0:
        assert len0[k] == len1[k], (k, len0[k], len1[k])
    assert l0 == l1
    assert c0 == c1
    nbranch = len(len0)
    print("sweep", n, nsites, s0, s1, nbranch, t1.path_counts())
    assert s0 - s1 >= nbranch - 1
    pc = t1.path_counts()
    assert pc["sweep_per_step"] > 0 and pc["sweep_sequential"] == 0 and pc["sweep_persistent"] == 0, pc
    ot2 = asc_oracle(oracle, inputs, n, seq_type, newick=t1.tree_string())
    ref, _ = ot2.likelihood()
    assert abs(l1 - ref) <= 1e-8 * abs(ref)


def test_asc_sweep_applies_the_diverged_newton_reset(pkg, synth, oracle):
    """phylotree.cpp:2167-2176 inside the sweep, with -nsites * log(1 - prob_const) in both lnL of the comparison"""
    n, ncat, seq_type, ntaxa, nsites = SWEEP_DIVERGED_CASE
    inputs = asc_inputs(synth, n, ncat, seq_type, ntaxa, nsites)
    out = run_both(lambda: asc_tree(pkg, inputs, n, seq_type), iterations=1, bounds=(1e-6, 0.05))
    (l0, len0, c0, _, _), (l1, len1, c1, _, t1) = out[False], out[True]
    assert len0 == len1 and l0 == l1
    pc = t1.path_counts()
    assert pc["sweep_per_step"] > 0 and pc["sweep_sequential"] == 0, pc
    # a length above 0.95 * max after the sweep is a step whose solve ended there and whose comparison of the two lnL kept
    # it: the rule ran for that step (status 5 in its iqhip_branch_result)
    print("diverged", sorted(len1.values()))
    assert sum(1 for v in len1.values() if v > 0.0475) >= 1 and any(v <= 0.0475 for v in len1.values())


def test_asc_sweep_reports_the_rule_through_the_c_abi(pkg, synth, oracle):
    """iqhip_optimize_sweep itself on a +ASC engine with x2 = 0.05: steps whose solve ends above 0.95 * x2 report status 5,
    and every length equals, bit for bit, iqhip_optimize_branch on the same branch followed by the rule on the host with
    iqhip_lnl_from_theta (which carries the +ASC term) at both lengths."""
    n, ncat, seq_type, ntaxa, nsites = SWEEP_DIVERGED_CASE
    inputs = asc_inputs(synth, n, ncat, seq_type, ntaxa, nsites)
    lib = pkg.libiqhip()

    class Step(C.Structure):
        _fields_ = [("ops", C.c_void_p), ("len_from", C.POINTER(C.c_int32)), ("nops", C.c_int32), ("_pad", C.c_int32),
                    ("a", pkg.BranchEnd), ("b", pkg.BranchEnd), ("xguess", C.c_double)]

    dp = C.POINTER(C.c_double)
    lib.iqhip_optimize_sweep.argtypes = [C.c_void_p, C.POINTER(Step), C.c_int, C.c_double, C.c_double, C.c_double, C.c_int,
                                         C.c_double, dp, C.POINTER(Result)]
    t = asc_tree(pkg, inputs, n, seq_type, mem_mode=pkg.LM_ALL_BRANCH)
    ot = asc_oracle(oracle, inputs, n, seq_type)
    t.compute_likelihood()
    t.compute_all_partial_lh()
    inner = [(x, y) for x in range(t.num_nodes) for y, _ in t.neighbors(x) if x < y and not ot.is_leaf(x) and not ot.is_leaf(y)]
    assert len(inner) >= 5
    x1, x2, xacc, ms, frac = 1e-6, 0.05, 1e-6, 100, 0.95
    steps = (Step * len(inner))()
    for k, (x, y) in enumerate(inner):     # no node updates: every vector is valid and stays as it is
        steps[k].ops, steps[k].nops = None, 0
        steps[k].a = pkg.key_end(t.neighbor_info(x, y)["key"])
        steps[k].b = pkg.key_end(t.neighbor_info(y, x)["key"])
        steps[k].xguess = ot.length(x, y)
    res = (Result * len(inner))()
    assert lib.iqhip_optimize_sweep(t.engine, steps, len(inner), x1, x2, xacc, ms, frac, None, res) == 0, lib.iqhip_last_error()
    pc = t.path_counts()
    assert pc["sweep_per_step"] == 1 and pc["sweep_sequential"] == 0 and pc["sweep_persistent"] == 0, pc
    nrule = 0
    for k in range(len(inner)):
        optx, d2l, ns = C.c_double(), C.c_double(), C.c_int()
        assert lib.iqhip_optimize_branch(t.engine, None, 0, steps[k].a, steps[k].b, steps[k].xguess, x1, x2, xacc, ms, None,
                                         C.byref(optx), C.byref(d2l), C.byref(ns)) == 0, lib.iqhip_last_error()
        want, ran = optx.value, optx.value > frac * x2
        if ran:
            opt_lh, orig_lh = C.c_double(), C.c_double()
            assert lib.iqhip_lnl_from_theta(t.engine, optx.value, C.byref(opt_lh)) == 0
            assert lib.iqhip_lnl_from_theta(t.engine, steps[k].xguess, C.byref(orig_lh)) == 0
            if orig_lh.value > opt_lh.value:
                want = steps[k].xguess
            nrule += 1
        print("abi sweep", inner[k], res[k].optx, want, res[k].nsteps, ns.value, res[k].status)
        assert res[k].optx == want and res[k].nsteps == ns.value
        assert res[k].status == (5 if ran else 0)
    assert nrule >= 1 and any(r.status == 5 for r in res)


# ---------------------------------------------------------------------------------------
# 6. nothing moved: engines without +ASC keep the bits of the commit before this feature
# ---------------------------------------------------------------------------------------
NONASC_SWEEP_CASES = [SWEEP_CASES[0], SWEEP_CASES[2]]   # a 4-state engine (persistent sweep) and a 20-state one (per-step form)
NONASC_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "asc_batch_nonasc.json")


def nonasc_values(pkg, synth, oracle):
    """tests 2 and 5 with set_ascertainment(0, 0): every float as its hex string"""
    batches, single = abi_batch_and_single(pkg, synth, oracle, asc=False)
    out = {"abi_batches": [[[float(v).hex() for v in r[:3]] + [int(r[3]), int(r[4])] for r in b] for b in batches],
           "abi_single": [[float(v).hex() for v in r[:3]] + [int(r[3]), int(r[4])] for r in single], "sweeps": []}
    for (n, ncat, seq_type, ntaxa, nsites) in NONASC_SWEEP_CASES:
        inputs = asc_inputs(synth, n, ncat, seq_type, ntaxa, nsites)
        res = run_both(lambda: asc_tree(pkg, inputs, n, seq_type, asc=False), iterations=2, start=0.15)
        for sweep in (False, True):
            lnl, lens, nev, _, _ = res[sweep]
            out["sweeps"].append({"case": [n, ncat, seq_type, ntaxa, nsites], "sweep": sweep, "lnl": float(lnl).hex(), "nevals": nev,
                                  "lengths": [[a, b, float(v).hex()] for (a, b), v in sorted(lens.items())]})
    return out


def test_engines_without_asc_keep_their_bits(pkg, synth, oracle):
    """tests/golden/asc_batch_nonasc.json was recorded on an MI355X with the library of the commit before +ASC entered
    k_newton_batch, k_newton's lnL pass, the chained derivative kernels and the drivers (nonasc_values above, dumped as
    JSON).  Fixed-order sums on a fixed grid: the values repeat to the last bit."""
    got = nonasc_values(pkg, synth, oracle)
    with open(NONASC_GOLDEN) as f:
        want = json.load(f)
    assert got["abi_batches"] == want["abi_batches"]
    assert got["abi_single"] == want["abi_single"]
    assert got["sweeps"] == want["sweeps"]
    for a, b in zip(got["sweeps"][0::2], got["sweeps"][1::2]):      # and the two sweep forms agree with each other
        assert (a["lnl"], a["nevals"], a["lengths"]) == (b["lnl"], b["nevals"], b["lengths"])
