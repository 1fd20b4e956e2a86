"""A batch of joint branch solves on a partition group (iqhip_partition_optimize_branch_batch, kernels_partnewton.hip):
many independent super-tree branches side by side, each solved jointly over all members.  Checked against the
restatement of tests/partition_ref.py over the CPU oracle with the tolerances of tests/test_partition_gpu.py
(|optx - ref| <= 1e-9 max(1, |ref|), the same number of derivative evaluations, d2l to 1e-6 relative, per-member lnL to
1e-9 relative), and bit for bit against iqhip_partition_newton_branch on the same thetas: the per-item body and both
summation orders are shared between the two calls."""
import ctypes as C
import os

import numpy as np
import pytest

import partition_ref as pr

pytestmark = pytest.mark.gpu

LNL_RTOL = 1e-9   # tests/test_parity_gpu.py
ERR_INVALID = 2
STATUS = {"ok": 0, "nonfinite": 2, "maxsteps": 3}
SCRATCH = 1 << 40   # keys no tree of these tests hands out


def end_of(pkg, t, sup, frm, to):
    """the branch end `to` seen from `frm`: a leaf id, or the key of the subtree vector behind `to`"""
    return pkg.leaf_end(to) if sup.is_leaf(to) else pkg.key_end(t.neighbor_info(frm, to)["key"])


def device_member(pkg, nwk, d):
    """partition_ref.device_member with a buffer for every directed subtree vector (the mode the NNI batches run in)"""
    t = pkg.PhyloTree(pr.scale_newick(nwk, d["rate"]))
    t.set_mem_mode(pkg.LM_ALL_BRANCH)
    t.set_alignment(d["n"], d["seq_type"], d["pat"], d["freq"], d["invar"])
    t.set_model(d["model"])
    t.set_likelihood_kernel(pkg.LK_EIGEN_HIP)
    t.attach_engine(0)
    return t


def make_group(pkg, oracle, nwk, members, rates):
    trees = [device_member(pkg, nwk, d) for d in members]
    for t in trees:
        t.compute_likelihood()
        t.compute_all_partial_lh()
    sup = oracle.OracleTree(nwk, 4, 0, members[0]["pat"], members[0]["freq"], None, members[0]["model"])
    edges = pr.tree_edges(sup, len(sup.adj))
    g = pkg.PartitionGroup(trees)
    g.set_rates(rates)
    return dict(nwk=nwk, members=members, trees=trees, sup=sup, group=g, edges=edges, rates=list(rates))


def plain_task(pkg, G, a, b, x1, xg, x2, xacc, ms):
    t0 = G["trees"][0]
    return pkg.BranchTask(None, 0, ms, end_of(pkg, t0, G["sup"], b, a), end_of(pkg, t0, G["sup"], a, b), xg, x1, x2, xacc)


def single_solve(pkg, G, task):
    """iqhip_compute_theta of the task's branch on every member, then the single joint solve -> (optx, d2l, nsteps, part_lnl)"""
    lib = pkg.libiqhip()
    for t in G["trees"]:
        assert lib.iqhip_compute_theta(t.engine, task.a, task.b) == 0
    return G["group"].newton_branch(task.xguess, task.x1, task.x2, task.xacc, task.max_steps)


def check_against_oracle(res, part, ref, want_lnl, where):
    ref_x, ref_d2l, pts, status = ref
    assert res["status"] == STATUS[status], (where, res, status)
    assert res["nsteps"] == len(pts), (where, res, pts)
    assert abs(res["optx"] - ref_x) <= 1e-9 * max(1.0, abs(ref_x)), (where, res, ref_x)
    assert abs(res["d2l"] - ref_d2l) <= 1e-6 * max(1.0, abs(ref_d2l)), (where, res, ref_d2l)
    np.testing.assert_allclose(part, want_lnl, rtol=LNL_RTOL, atol=0)


def same_bits(res, part, other_res, other_part):
    for r, o in zip(res, other_res):
        assert r == o, (r, o)
    assert np.array_equal(part, other_part)


@pytest.fixture(scope="module")
def mixed(pkg, synth, oracle):
    nwk, members = pr.mixed_group(synth, oracle)
    G = make_group(pkg, oracle, nwk, members, pr.MIXED_RATES)
    G["ots"] = [pr.oracle_member(oracle, nwk, d) for d in members]
    yield G
    G["group"].close()


@pytest.fixture(scope="module")
def batch65(pkg, mixed):
    """all 13 branches x the 5 NEWTON_SETUPS as ONE batch of 65 tasks without node updates: more than one chunk of 64"""
    tasks, where = [], []
    for (a, b) in mixed["edges"]:
        for (x1, xg, x2, xacc, ms) in pr.NEWTON_SETUPS:
            xg = mixed["sup"].length(a, b) if xg is None else xg
            tasks.append(plain_task(pkg, mixed, a, b, x1, xg, x2, xacc, ms))
            where.append((a, b, x1, xg, x2, xacc, ms))
    assert len(tasks) == 65
    arr = (pkg.BranchTask * 65)(*tasks)
    res, part = mixed["group"].optimize_branch_batch(arr)
    return dict(tasks=arr, where=where, res=res, part=part)


def test_oracle_mixed_shapes(mixed, batch65):
    """case 1: DNA +G4 with a partial last 64-tile, DNA with one category on less than a tile, protein +G4 with a partial
    16-tile, binary data on the embedded route, all-unknown rows.
    The step-limit tasks (max_steps = 3): minimizeNewton stops them at `j == max_steps` after exactly 3 derivative
    evaluations and hands back the last accepted iterate -- in the reference, the restatement and the single joint solve
    alike that is status 0 (tests/test_partition_gpu.py asserts "ok" for these very setups), so the status checked here is
    the restatement's, and the test asserts that these tasks were cut short while their neighbours ran on to convergence."""
    pats = [d["pat"].shape[1] for d in mixed["members"]]
    assert 128 < pats[0] < 192 and pats[1] < 64 and pats[2] % 16 != 0, pats
    ots, rates = mixed["ots"], mixed["rates"]
    theta_of = {}
    cut_short = 0
    for k, (a, b, x1, xg, x2, xacc, ms) in enumerate(batch65["where"]):
        if (a, b) not in theta_of:
            theta_of[(a, b)] = [ot.theta(a, b) for ot in ots]
        th = theta_of[(a, b)]
        ref = pr.joint_minimize_newton(ots, rates, a, b, x1, xg, x2, xacc, ms, [t for t, _ in th])
        res = batch65["res"][k]
        want = pr.joint_lnl_from_theta(ots, rates, a, b, res["optx"], th)
        check_against_oracle(res, batch65["part"][k], ref, want, batch65["where"][k])
        # results[t].lnl: the members' values summed in member order on the host
        s = 0.0
        for v in batch65["part"][k]:
            s += v
        assert res["lnl"] == s
        if ms == 3:
            long_run = batch65["res"][k - 3]   # the same branch from a guess of 60 with 100 steps allowed
            assert batch65["where"][k - 3][-1] == 100
            print("step limit", (a, b), "evaluations", res["nsteps"], "neighbour", long_run["nsteps"])
            assert res["nsteps"] == 3
            cut_short += long_run["nsteps"] > 3
    assert cut_short >= 1


def test_same_bits_as_single_solve(pkg, mixed, batch65):
    """case 2: every task against iqhip_partition_newton_branch on the same thetas; chunks of 1 and 7 tasks, one step per
    chunk of steps, and the same call again"""
    for k, task in enumerate(batch65["tasks"]):
        optx, d2l, ns, part = single_solve(pkg, mixed, task)
        r = batch65["res"][k]
        assert (r["optx"], r["d2l"], r["nsteps"], r["status"]) == (optx, d2l, ns, 0), (batch65["where"][k], r, optx, d2l, ns)
        assert np.array_equal(batch65["part"][k], part), (batch65["where"][k], batch65["part"][k], part)
    for t in mixed["trees"]:
        t.reset_theta()
    g = mixed["group"]
    same_bits(*g.optimize_branch_batch(batch65["tasks"]), batch65["res"], batch65["part"])
    for name, value in (("IQHIP_PART_BATCH_CHUNK", "1"), ("IQHIP_PART_BATCH_CHUNK", "7"), ("IQHIP_PART_STEPS", "1")):
        os.environ[name] = value
        try:
            got = g.optimize_branch_batch(batch65["tasks"])
        finally:
            del os.environ[name]
        same_bits(*got, batch65["res"], batch65["part"])
    res, none = g.optimize_branch_batch(batch65["tasks"], want_part_lnl=False)
    assert none is None and res == batch65["res"]


def nni1_ops(pkg, G, a, b, key0, scale=1.0):
    """the two node updates of the first nni1 candidate of internal branch (a, b) (PhyloTree::evaluateNNIsBatch): a's first
    subtree and b's first change places -> (ops, end of a's side, end of b's side)"""
    sup, t0 = G["sup"], G["trees"][0]
    s1 = [v for v, _ in sup.adj[a] if v != b]
    s2 = [v for v, _ in sup.adj[b] if v != a]

    def side(frm, to):
        e = end_of(pkg, t0, sup, frm, to)
        return e.key, e.leaf, sup.length(frm, to) * scale

    ops = (pkg.NodeOp * 2)()
    for k, (dst, (lk, ll, llen), (rk, rl, rlen)) in enumerate([(key0, side(a, s1[0]), side(b, s2[1])),
                                                              (key0 + 1, side(b, s2[0]), side(a, s1[1]))]):
        ops[k] = pkg.NodeOp(dst, lk, rk, ll, rl, llen, rlen, 0, 0)
    return ops, pkg.key_end(key0), pkg.key_end(key0 + 1)


def inner_edges(G):
    return [(a, b) for (a, b) in G["edges"] if not G["sup"].is_leaf(a) and not G["sup"].is_leaf(b)]


def nni1_tasks(pkg, G, key_base):
    keep, tasks = [], []
    for k, (a, b) in enumerate(inner_edges(G)):
        ops, ea, eb = nni1_ops(pkg, G, a, b, key_base + 2 * k)
        keep.append(ops)
        tasks.append(pkg.BranchTask(C.cast(ops, C.c_void_p), 2, 100, ea, eb, G["sup"].length(a, b), 1e-6, 100.0, 1e-6))
    return keep, (pkg.BranchTask * len(tasks))(*tasks)


def test_tasks_with_ops(pkg, mixed):
    """case 3: the two-op tasks of an nni1 candidate on scratch keys, all 5 internal branches, against the same ops run
    member by member through iqhip_update_partials with scaled lengths, then iqhip_compute_theta and the single solve"""
    lib = pkg.libiqhip()
    inner = inner_edges(mixed)
    assert len(inner) == 5
    keep, tasks = nni1_tasks(pkg, mixed, SCRATCH)
    res, part = mixed["group"].optimize_branch_batch(tasks)
    for k, (a, b) in enumerate(inner):
        key0 = SCRATCH + 1000 + 2 * k   # (other keys than the batch wrote)
        for t, r in zip(mixed["trees"], mixed["rates"]):
            ops, ea, eb = nni1_ops(pkg, mixed, a, b, key0, scale=r)
            assert lib.iqhip_update_partials(t.engine, ops, 2, None) == 0
            assert lib.iqhip_compute_theta(t.engine, ea, eb) == 0
        optx, d2l, ns, want = mixed["group"].newton_branch(mixed["sup"].length(a, b), 1e-6, 100.0, 1e-6, 100)
        r = res[k]
        assert (r["optx"], r["d2l"], r["nsteps"], r["status"]) == (optx, d2l, ns, 0), ((a, b), r, optx, d2l, ns)
        assert np.array_equal(part[k], want), ((a, b), part[k], want)
    for t in mixed["trees"]:
        t.reset_theta()


def test_several_work_items_per_member(pkg, synth, oracle):
    """case 4: DNA 12 taxa x 40 000 sites (many work items of 16 tiles) with a 64-state member; 5 tasks against the oracle"""
    nwk = synth.random_tree_newick(12, 31, 0.02, 0.2)
    rates = [0.8, 1.7]
    members = [pr.member_data(synth, oracle, nwk, 4, 4, pr.SEQ_DNA, 40000, 600, rates[0]),
               pr.member_data(synth, oracle, nwk, 64, 1, pr.SEQ_CODON, 600, 610, rates[1])]
    assert members[0]["pat"].shape[1] > 2 * 16 * 64
    G = make_group(pkg, oracle, nwk, members, rates)
    ots = [pr.oracle_member(oracle, nwk, d) for d in members]
    edges = G["edges"][:5]
    tasks = (pkg.BranchTask * 5)(*[plain_task(pkg, G, a, b, 1e-6, G["sup"].length(a, b), 100.0, 1e-6, 100) for (a, b) in edges])
    res, part = G["group"].optimize_branch_batch(tasks)
    for k, (a, b) in enumerate(edges):
        th = [ot.theta(a, b) for ot in ots]
        ref = pr.joint_minimize_newton(ots, rates, a, b, 1e-6, G["sup"].length(a, b), 100.0, 1e-6, 100, [t for t, _ in th])
        check_against_oracle(res[k], part[k], ref, pr.joint_lnl_from_theta(ots, rates, a, b, res[k]["optx"], th), (a, b))
    G["group"].close()


def test_many_members(pkg, synth, oracle):
    """case 5: 70 members, more than the 64 the update kernel takes per round; 3 tasks"""
    nwk = synth.random_tree_newick(8, 41, 0.02, 0.2)
    rng = np.random.default_rng(42)
    rates = list(rng.uniform(0.2, 3.0, 70))
    members = [pr.member_data(synth, oracle, nwk, 4, 4, pr.SEQ_DNA, int(rng.integers(40, 131)), 700 + 3 * k, rates[k])
               for k in range(70)]
    G = make_group(pkg, oracle, nwk, members, rates)
    ots = [pr.oracle_member(oracle, nwk, d) for d in members]
    edges = G["edges"][:3]
    tasks = (pkg.BranchTask * 3)(*[plain_task(pkg, G, a, b, 1e-6, G["sup"].length(a, b), 100.0, 1e-6, 100) for (a, b) in edges])
    res, part = G["group"].optimize_branch_batch(tasks)
    for k, (a, b) in enumerate(edges):
        th = [ot.theta(a, b) for ot in ots]
        ref = pr.joint_minimize_newton(ots, rates, a, b, 1e-6, G["sup"].length(a, b), 100.0, 1e-6, 100, [t for t, _ in th])
        check_against_oracle(res[k], part[k], ref, pr.joint_lnl_from_theta(ots, rates, a, b, res[k]["optx"], th), (a, b))
    tm = G["group"].timing()
    most = max(r["nsteps"] for r in res)
    assert 2 * most + 2 <= tm["launches"] <= 2 * (most + 3) + 2 * 3   # (derivative, update) per evaluation + the lnL passes
    G["group"].close()


def test_nan_member_inside_a_batch(pkg, mixed):
    """case 6: one member's vector at one end of ONE task's branch is NaN (tests/test_partition_gpu.py's construction): that
    task is the restatement's with the member's derivatives at 0, the other two tasks keep their bits"""
    lib = pkg.libiqhip()
    trees, ots, rates, sup = mixed["trees"], mixed["ots"], mixed["rates"], mixed["sup"]
    inner = inner_edges(mixed)
    tasks = (pkg.BranchTask * 3)(*[plain_task(pkg, mixed, a, b, 1e-6, sup.length(a, b), 100.0, 1e-6, 100) for (a, b) in inner[:3]])
    before, before_part = mixed["group"].optimize_branch_batch(tasks)
    a, b = inner[1]
    t = trees[1]
    key_ab = t.neighbor_info(a, b)["key"]
    good = np.ascontiguousarray(t.fetch_partial(a, b))
    sc = np.ascontiguousarray(t.fetch_scale_num(a, b), dtype=np.int16)
    bad = np.full_like(good, np.nan)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int16)
    try:
        assert lib.iqhip_upload_partial(t.engine, key_ab, bad.ctypes.data_as(dp), sc.ctypes.data_as(ip)) == 0
        res, part = mixed["group"].optimize_branch_batch(tasks)
    finally:
        assert lib.iqhip_upload_partial(t.engine, key_ab, good.ctypes.data_as(dp), sc.ctypes.data_as(ip)) == 0
    thetas = [ot.theta(a, b)[0] for ot in ots]
    thetas[1] = np.full_like(thetas[1], np.nan)
    ref_x, ref_d2l, pts, status = pr.joint_minimize_newton(ots, rates, a, b, 1e-6, sup.length(a, b), 100.0, 1e-6, 100, thetas)
    assert status == "ok" and res[1]["status"] == 0 and res[1]["nsteps"] == len(pts)
    assert abs(res[1]["optx"] - ref_x) <= 1e-9 * max(1.0, abs(ref_x))
    assert abs(res[1]["d2l"] - ref_d2l) <= 1e-6 * max(1.0, abs(ref_d2l))
    assert res[1]["optx"] != before[1]["optx"]
    for k in (0, 2):
        assert res[k] == before[k]
        assert np.array_equal(part[k], before_part[k])
    again, again_part = mixed["group"].optimize_branch_batch(tasks)
    same_bits(again, again_part, before, before_part)


def test_state_and_refusals(pkg, synth, oracle, mixed, batch65):
    """case 7"""
    lib = pkg.libiqhip()
    g, sup = mixed["group"], mixed["sup"]
    (a, b) = inner_edges(mixed)[0]
    xg = sup.length(a, b)
    ok = plain_task(pkg, mixed, a, b, 1e-6, xg, 100.0, 1e-6, 100)
    one = (pkg.BranchTask * 1)(ok)
    want, want_part = g.optimize_branch_batch(one)
    res1 = (pkg.BranchResult * 1)()
    call = lib.iqhip_partition_optimize_branch_batch
    assert call(None, one, 1, res1, None) == ERR_INVALID
    assert call(g.h, None, 1, res1, None) == ERR_INVALID
    assert call(g.h, one, 1, None, None) == ERR_INVALID
    assert call(g.h, one, 0, res1, None) == ERR_INVALID
    assert call(g.h, one, -3, res1, None) == ERR_INVALID

    def refused(**change):
        t = pkg.BranchTask(ok.ops, ok.nops, ok.max_steps, ok.a, ok.b, ok.xguess, ok.x1, ok.x2, ok.xacc)
        for name, v in change.items():
            setattr(t, name, v)
        # a good task in front: the whole batch is refused
        assert call(g.h, (pkg.BranchTask * 2)(ok, t), 2, (pkg.BranchResult * 2)(), None) == ERR_INVALID, change
        same_bits(*g.optimize_branch_batch(one), want, want_part)   # the group and its members are usable

    refused(nops=2)                 # ops missing
    refused(nops=-1)
    refused(max_steps=0)            # bounds newton_check_bounds refuses
    refused(x1=2.0, x2=1.0)
    refused(xacc=float("nan"))
    refused(a=pkg.key_end(SCRATCH + 777777))   # a key no member knows
    keep, with_ops = nni1_tasks(pkg, mixed, SCRATCH + 5000)
    ops = C.cast(with_ops[0].ops, C.POINTER(pkg.NodeOp))
    stale = ops[0].left_key, ops[0].left_leaf
    ops[0].left_key, ops[0].left_leaf = SCRATCH + 888888, -1      # an op that reads a vector nobody wrote
    assert call(g.h, with_ops, len(with_ops), (pkg.BranchResult * len(with_ops))(), None) == ERR_INVALID
    ops[0].left_key, ops[0].left_leaf = stale
    same_bits(*g.optimize_branch_batch(one), want, want_part)

    # a group batch, then a member's own batch, then a joint single solve: each as on a group that ran no batch
    def member_batch(G):
        n = 4
        tasks = (pkg.BranchTask * n)(*batch65["tasks"][0:5 * n:5])
        out = (pkg.BranchResult * n)()
        assert lib.iqhip_optimize_branch_batch_rows(G["trees"][2].engine, tasks, n, None, out, None) == 0
        return [(r.optx, r.d2l, r.lnl, r.nsteps, r.status) for r in out]

    def joint_single(G):
        for t in G["trees"]:
            t.reset_theta()
            t.compute_likelihood_derv(a, b)
        return G["group"].newton_branch(xg, 1e-6, 100.0, 1e-6, 100)

    fresh = make_group(pkg, oracle, mixed["nwk"], mixed["members"], mixed["rates"])
    held = joint_single(mixed)            # theta of (a, b) is resident on every member ...
    g.optimize_branch_batch(with_ops)     # ... a batch on scratch vectors leaves it alone, validity included
    again = g.newton_branch(xg, 1e-6, 100.0, 1e-6, 100)
    assert again[:3] == held[:3] and np.array_equal(again[3], held[3])
    assert member_batch(mixed) == member_batch(fresh)
    got, ref = joint_single(mixed), joint_single(fresh)
    assert got[:3] == ref[:3] and np.array_equal(got[3], ref[3])
    for G in (mixed, fresh):
        for t in G["trees"]:
            t.reset_theta()
    fresh["group"].close()
