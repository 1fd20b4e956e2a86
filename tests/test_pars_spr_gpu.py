"""GPU: the parsimony SPR scan (include/iqhip.h "Parsimony SPR scan") and the search on top of it against the numpy
restatement of tests/spr_ref.py -- integer arithmetic throughout, every comparison is exact equality.

Scan: every scored step against the Fitch score, computed from scratch, of the tree with that move applied; states 4 / 20 /
64 (registers / LDS with two lanes per column / LDS with four lanes per column); 4 taxa (the smallest tree with a move) to 40;
caterpillars (the radius cuts the walk), balanced and random trees; 33 sites (one workgroup of mostly idle lanes), 513 (just
across the 16 columns a 64-state workgroup owns), 1025 (just across the 32 columns of a 20-state workgroup) and 2049 (just
across the 64 columns of a 4-state workgroup); radius
1, 2, 6, 10, and on 9 taxa the diameter, so that every SPR of the tree is scored.  Then a hand-built job for the stack rule,
the search round by round, determinism, the refusals, the hand-over to the likelihood kernels and the command line."""
import os
import re
import subprocess

import numpy as np
import pytest

import fitch_ref as F
import spr_ref as S
import test_parsimony_gpu as TP

pytestmark = pytest.mark.gpu

INT_MAX = 0x7fffffff


def balanced_tree(ntaxa):
    """three balanced subtrees around one node, any number of taxa"""
    adj, nxt = {}, [ntaxa]

    def build(lo, hi):
        if hi - lo == 1:
            adj[lo] = []
            return lo
        node = nxt[0]
        nxt[0] += 1
        adj[node] = []
        for a, b in ((lo, (lo + hi) // 2), ((lo + hi) // 2, hi)):
            c = build(a, b)
            adj[node].append(c)
            adj[c].append(node)
        return node

    top = nxt[0]
    nxt[0] += 1
    adj[top] = []
    cuts = [0, ntaxa // 3, 2 * ntaxa // 3, ntaxa]
    for a, b in zip(cuts, cuts[1:]):
        c = build(a, b)
        adj[top].append(c)
        adj[c].append(top)
    assert len(adj) == 2 * ntaxa - 2
    return adj


def tree_of(shape, ntaxa, rng):
    return {"caterpillar": F.caterpillar, "balanced": balanced_tree}[shape](ntaxa) if shape != "random" else F.random_tree(ntaxa, rng)


def prepared(pkg, synth, n, shape, ntaxa, nsites, seed):
    """a tree with every directed vector on the device -> (tree handle, adj, tips, slot_of)"""
    rng = np.random.default_rng(seed)
    states, freq, mask = TP.alignment(n, ntaxa, nsites, rng)   # a mask, zero-frequency tail patterns, 10 % ambiguity codes
    assert (states >= n).any() and (freq[-4:] == 0).all() and 0 < mask.sum() < mask.size
    tips = F.tip_vectors(states, F.site_patterns(freq, mask), n)
    adj = tree_of(shape, ntaxa, rng)
    ops, slot = TP.all_directed_ops(adj, ntaxa)
    t = TP.make_tree(pkg, synth, n, states, freq)
    assert t.pars_init(mask) == nsites
    t.pars_update(ops)
    return t, adj, tips, (lambda u, v: TP.slot_of(slot, u, v, ntaxa))


def check_scan(t, adj, tips, slot_of, ntaxa, radius, cache):
    """one scan of every prune point within `radius`; cache: {(p, s, a, b): score of the rearranged tree from scratch}"""
    jobs = S.collect_jobs(adj, ntaxa, radius)
    jr, sr = S.program(jobs, slot_of)
    score, best_step, best_score, best_job = t.pars_spr_scan(jr, sr)
    now = cache.setdefault("now", F.tree_score(adj, tips))
    want = []
    for job in jobs:
        for st in job["steps"]:
            if not st["scored"]:
                want.append(-1)                              # NO_SCORE steps return -1
            elif st["depth"] == 0:
                want.append(now)                             # the scored root step is the current tree
            else:
                key = (job["p"], job["s"]) + st["move"]
                if key not in cache:
                    cache[key] = F.tree_score(S.apply_move(adj, *key), tips)
                want.append(cache[key])
    assert score.tolist() == want
    bs, bsc, bj = S.first_minima(jr, score)
    assert best_step.tolist() == bs and best_score.tolist() == bsc and best_job == bj
    assert bj >= 0 and bsc[bj] == min(v for v in want if v >= 0)
    none, bs2, bsc2, bj2 = t.pars_spr_scan(jr, sr, want_scores=False)
    assert none is None and bs2.tolist() == bs and bsc2.tolist() == bsc and bj2 == bj
    return jobs, jr, sr, score


SCAN_CASES = [
    # shape, ntaxa, nsites, radii
    ("random", 4, 33, (1, 2)),
    ("random", 5, 33, (1, 2, 6)),
    ("caterpillar", 9, 33, (8,)),          # radius >= the diameter: every SPR of the tree
    ("balanced", 9, 513, (8,)),
    ("random", 9, 2049, (8,)),
    ("caterpillar", 17, 33, (1, 2, 6, 10)),
    ("random", 17, 513, (1, 2, 6)),
    ("balanced", 17, 2049, (2,)),
    ("random", 9, 1025, (2,)),
    ("random", 40, 33, (1, 2)),
]


@pytest.mark.parametrize("shape,ntaxa,nsites,radii", SCAN_CASES)
@pytest.mark.parametrize("n", [4, 20, 64])
def test_scan_scores_equal_the_rearranged_trees(pkg, synth, n, shape, ntaxa, nsites, radii):
    t, adj, tips, slot_of = prepared(pkg, synth, n, shape, ntaxa, nsites, seed=n * 1009 + ntaxa * 31 + nsites)
    cache = {}
    nsteps = []
    for radius in radii:
        jobs, jr, sr, score = check_scan(t, adj, tips, slot_of, ntaxa, radius, cache)
        nsteps.append(len(sr))
        depth = max(st["depth"] for job in jobs for st in job["steps"])
        assert depth <= radius
        if shape == "caterpillar" and ntaxa == 17:
            assert depth == radius                         # the radius cuts the walk
    assert nsteps == sorted(nsteps)
    if ntaxa == 9 and radii[-1] >= 8:
        # every SPR of the tree: from every prune point every branch of the pruned tree but the merged one is a target
        for job in jobs:
            inside = 0
            todo = [(job["s"], job["p"])]
            while todo:
                u, dad = todo.pop()
                inside += 1
                todo.extend((k, u) for k in adj[u] if k != dad)
            targets = {frozenset(st["move"]) for st in job["steps"] if st["depth"] >= 1}
            assert len(targets) == (2 * ntaxa - 3) - inside - 2 == sum(st["depth"] >= 1 for st in job["steps"])
    t.close()


def test_stack_rule_second_subtree_after_a_deep_first_one(pkg, synth):
    """pruning leaf 4 of a 9-taxon caterpillar (internal nodes 9 .. 15 in a chain; node 12 = [11, 4, 13]): the walk from node
    11 goes down to depth 3 before the second depth-1 step, which must find the root's vector at level 0 untouched, and the
    steps under the second root find theirs after level 0 was replaced"""
    ntaxa = 9
    t, adj, tips, slot_of = prepared(pkg, synth, 20, "caterpillar", ntaxa, 65, seed=77)
    assert adj[12] == [11, 4, 13] and adj[11] == [10, 3, 12] and adj[10] == [9, 2, 11] and adj[9] == [0, 1, 10]
    #        parent  side      target    move      scored
    steps = [(-1, (13, 12), (11, 12), (11, 13), True),     # 0  depth 0
             (0, (3, 11), (10, 11), (11, 10), True),       # 1  depth 1
             (1, (2, 10), (9, 10), (10, 9), True),         # 2  depth 2
             (2, (1, 9), (0, 9), (9, 0), True),            # 3  depth 3
             (2, (0, 9), (1, 9), (9, 1), True),            # 4  depth 3
             (1, (9, 10), (2, 10), (10, 2), True),         # 5  depth 2: level 1 after level 2 and 3 were written
             (0, (10, 11), (3, 11), (11, 3), True),        # 6  depth 1: level 0 after everything below was written
             (-1, (11, 12), (13, 12), (13, 11), False),    # 7  depth 0, not scored: replaces level 0
             (7, (14, 13), (5, 13), (13, 5), True),        # 8  depth 1
             (7, (5, 13), (14, 13), (13, 14), True),       # 9  depth 1
             (9, (15, 14), (6, 14), (14, 6), True),        # 10 depth 2
             (9, (6, 14), (15, 14), (14, 15), True),       # 11 depth 2
             (7, (14, 13), (5, 13), (13, 5), True)]        # 12 depth 1 again (a repeat of step 8): level 0 once more
    jr = [(slot_of(4, 12), 0, len(steps))]
    sr = [(p, slot_of(*side), slot_of(*tgt), 0 if scored else S.NO_SCORE) for p, side, tgt, _, scored in steps]
    assert pkg.debug_pars_spr_check(ntaxa, 4 * (ntaxa - 1), jr, sr, np.ones(4 * (ntaxa - 1))).tolist() == [0, 1, 2, 3, 3, 2, 1, 0, 1, 1, 2, 2, 1]
    score, best_step, best_score, best_job = t.pars_spr_scan(jr, sr)
    now = F.tree_score(adj, tips)
    want = [now if k == 0 else -1 if not scored else F.tree_score(S.apply_move(adj, 12, 4, *mv), tips)
            for k, (_, _, _, mv, scored) in enumerate(steps)]
    assert score.tolist() == want and want[12] == want[8]
    assert len(set(want[1:7])) > 1                           # (the positions do differ in score)
    assert (best_step[0], best_score[0], best_job) == (want.index(min(v for v in want if v >= 0)), min(v for v in want if v >= 0), 0)
    t.close()


def test_minima_jobs_without_scores_and_empty_calls(pkg, synth):
    ntaxa = 9
    t, adj, tips, slot_of = prepared(pkg, synth, 4, "random", ntaxa, 200, seed=5)
    jobs = S.collect_jobs(adj, ntaxa, 2)
    jr, sr = S.program(jobs, slot_of)
    full = t.pars_spr_scan(jr, sr)
    # the same program with every step of job 1 unscored, the jobs listed backwards and two steps that belong to no job
    sr2 = np.concatenate([sr, [[5, 0, 0, 0], [-1, 1, 2, 0]]]).astype(np.int32)
    f1, n1 = jr[1][1], jr[1][2]
    sr2[f1:f1 + n1, 3] = S.NO_SCORE
    jr2 = jr[::-1].copy()
    score, best_step, best_score, best_job = t.pars_spr_scan(jr2, sr2)
    want = full[0].copy()
    want[f1:f1 + n1] = -1
    assert score.tolist() == want.tolist() + [-1, -1]
    bs, bsc, bj = S.first_minima(jr2, score)
    assert best_step.tolist() == bs and best_score.tolist() == bsc and best_job == bj
    k = len(jr) - 2                                            # job 1 in the reversed list
    assert best_step[k] == -1 and best_score[k] == INT_MAX
    # ties: the first job in job order
    assert bsc.count(min(bsc)) >= 1 and bj == bsc.index(min(bsc))
    # only unscored steps: nothing to report
    only = t.pars_spr_scan([jr[1]], sr2)
    assert only[1].tolist() == [-1] and only[2].tolist() == [INT_MAX] and only[3] == -1 and (only[0] == -1).all()
    # no jobs: succeeds, launches nothing
    before = t.pars_spr_timing(reset=True)
    empty = t.pars_spr_scan(np.zeros((0, 4), np.int32), sr)
    assert empty[1].size == 0 and empty[3] == -1 and (empty[0] == -1).all()
    assert t.pars_spr_timing()["launches"] == 0 and before["launches"] >= 9
    t.close()


def test_two_identical_calls_return_identical_arrays(pkg, synth):
    ntaxa = 17
    t, adj, tips, slot_of = prepared(pkg, synth, 20, "random", ntaxa, 2049, seed=21)
    jr, sr = S.program(S.collect_jobs(adj, ntaxa, 6), slot_of)
    a = t.pars_spr_scan(jr, sr)
    b = t.pars_spr_scan(jr, sr)
    for x, y in zip(a[:3], b[:3]):
        assert x.tobytes() == y.tobytes()
    assert a[3] == b[3]
    tm = t.pars_spr_timing()
    assert tm["launches"] == 6 and tm["steps_scored"] == 2 * int((sr[:, 3] == 0).sum())
    t.close()


# ---- the search -------------------------------------------------------------------------------------------------------------
def search_case(pkg, synth, ntaxa):
    """data simulated on a random tree, the start a caterpillar in taxon order -- deliberately bad"""
    model = synth.gtr_model(alpha=0.9, ncat=4)
    _, pat, freq = synth.make_workload(ntaxa, 150, model, seed=ntaxa, missing_frac=0.02, state_unknown=18)
    t = pkg.PhyloTree(F.newick(F.caterpillar(ntaxa)))
    t.set_alignment(4, 0, pat, freq)
    t.set_model(model)
    t.set_likelihood_kernel(pkg.LK_EIGEN_HIP)
    t.attach_engine(0)
    tips = F.tip_vectors(pat, F.site_patterns(freq, F.is_informative(pat, 4)), 4)
    return t, tips, pat, freq, model


@pytest.mark.parametrize("ntaxa,radius", [(17, 6), (40, 3)])
def test_optimize_parsimony_spr(pkg, synth, ntaxa, radius):
    t, tips, pat, freq, model = search_case(pkg, synth, ntaxa)
    start = S.mirror_adjacency(t)
    first = t.compute_parsimony()
    assert first == F.tree_score(start, tips)
    want_score, want_adj, want_rounds = S.search(start, tips, ntaxa, radius)
    score, rounds = t.optimize_parsimony_spr(radius, trace=True)
    assert rounds == want_rounds                               # round by round: scores, the chosen job / step / move
    assert len(rounds) >= 3 and not rounds[-1]["applied"] and all(r["applied"] for r in rounds[:-1])
    befores = [r["score_before"] for r in rounds]
    assert befores[0] == first and all(a > b for a, b in zip(befores, befores[1:]))   # strictly decreasing
    assert S.mirror_adjacency(t) == want_adj
    assert score == want_score == befores[-1] == t.compute_parsimony() == F.tree_score(want_adj, tips)
    # no move within the radius improves the final tree
    dv = F.directed_vectors(want_adj, tips)
    assert all(sc is None or sc >= score for job in S.collect_jobs(want_adj, ntaxa, radius) for sc in S.job_scores(job, dv))
    assert t.optimize_parsimony_spr(radius) == score           # again: nothing to do
    # the likelihood kernels take over the improved tree
    assert t.fix_negative_branch(True) == 2 * ntaxa - 3
    t.initialize_all_partial_lh()
    lnl = t.compute_likelihood()
    fresh = pkg.PhyloTree(t.tree_string())
    fresh.set_alignment(4, 0, pat, freq)
    fresh.set_model(model)
    fresh.set_likelihood_kernel(pkg.LK_EIGEN_HIP)
    fresh.attach_engine(0)
    fresh.initialize_all_partial_lh()
    fresh.clear_all_partial_lh()
    ref = fresh.compute_likelihood()
    assert np.isfinite(ref) and abs(lnl - ref) <= 1e-9 * abs(ref), (lnl, ref)   # LNL_RTOL of tests/test_parity_gpu.py
    assert fresh.compute_parsimony() == score
    fresh.close()
    t.close()
    # max_rounds = 1 stops after one move
    t1, _, _, _, _ = search_case(pkg, synth, ntaxa)
    one, r1 = t1.optimize_parsimony_spr(radius, max_rounds=1, trace=True)
    assert r1 == want_rounds[:1] and one == want_rounds[0]["score"] == t1.compute_parsimony()
    assert S.mirror_adjacency(t1) == S.apply_move(start, *want_rounds[0]["move"])
    assert t1.optimize_parsimony_spr(radius, max_rounds=0) == one
    t1.close()


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals(pkg, synth):
    rng = np.random.default_rng(11)
    states, freq, mask = TP.alignment(4, 5, 200, rng, tail=False)
    states = np.concatenate([states] * 8, axis=1)     # (a shard holds at least 64 patterns)
    freq, mask = np.concatenate([freq] * 8), np.concatenate([mask] * 8)
    adj = F.random_tree(5, rng)
    ops, slot = TP.all_directed_ops(adj, 5)
    jr, sr = S.program(S.collect_jobs(adj, 5, 2), lambda u, v: TP.slot_of(slot, u, v, 5))
    INVALID, UNSUPPORTED = pkg.ERR_INVALID, pkg.ERR_UNSUPPORTED
    t = TP.make_tree(pkg, synth, 4, states, freq)
    assert TP.code_of(pkg, t.pars_spr_scan, jr, sr) == INVALID             # before iqhip_pars_init
    t.pars_init(mask)
    assert TP.code_of(pkg, t.pars_spr_scan, jr, sr) == INVALID             # vectors never written
    t.pars_update(ops)
    good = t.pars_spr_scan(jr, sr)
    assert good[3] >= 0
    bad = sr.copy()
    bad[1, 0] = 1                                                          # a forward parent
    assert TP.code_of(pkg, t.pars_spr_scan, jr, bad) == INVALID
    bad = sr.copy()
    bad[0, 1] = 5 + 4 * 4                                                  # a slot out of range
    assert TP.code_of(pkg, t.pars_spr_scan, jr, bad) == INVALID
    bad = sr.copy()
    bad[0, 3] = 4                                                          # an unknown flag
    assert TP.code_of(pkg, t.pars_spr_scan, jr, bad) == INVALID
    assert TP.code_of(pkg, t.pars_spr_scan, np.concatenate([jr, jr[:1]]), sr) == INVALID   # overlapping jobs
    again = t.pars_spr_scan(jr, sr)                                        # a refusal changes nothing
    assert again[0].tolist() == good[0].tolist()
    t.set_ptn_freq(freq * 2)                                               # new frequencies invalidate the state
    assert TP.code_of(pkg, t.pars_spr_scan, jr, sr) == INVALID
    t.close()
    ts = TP.make_tree(pkg, synth, 4, states, freq, sharded=2)              # [0, 0] with REDUCE_HOST
    assert TP.code_of(pkg, ts.pars_spr_scan, jr, sr) == UNSUPPORTED
    ts.close()
    t5 = TP.make_tree(pkg, synth, 5, (states % 5).astype(np.uint8), freq, model=synth.random_reversible_model(5, 4, alpha=0.7, ncat=4))
    assert TP.code_of(pkg, t5.pars_spr_scan, jr, sr) == UNSUPPORTED
    t5.close()


# ---- command line -------------------------------------------------------------------------------------------------------------
def test_sprrad_command_line(pkg, tmp_path):
    here = os.path.dirname(os.path.abspath(__file__))
    binary = os.path.join(os.path.dirname(here), "iq-tree_amd", "lib", "iqhip_lnl")
    example = os.path.join(here, "golden", "example.phy")
    model = "GTR{1.513,2.393,1.769,1.912,2.838}+F{0.249,0.262,0.251,0.238}+G4{0.934}"

    def run(*extra, pre):
        r = subprocess.run([binary, "-s", example, "-m", model, "-seed", "1", "-pre", str(tmp_path / pre)] + list(extra),
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        return r.stdout

    out = run("-parstree", "-sprrad", "2", pre="a")
    lines = out.splitlines()
    k = [i for i, ln in enumerate(lines) if ln.startswith("Parsimony score: ")]
    assert len(k) == 1
    m1 = re.fullmatch(r"Parsimony score: (\d+) \(based on (\d+) informative sites\)", lines[k[0]])
    m2 = re.fullmatch(r"Parsimony score after SPR: (\d+) \((\d+) rounds\)", lines[k[0] + 1])   # right after the existing line
    assert m1 and m2, out
    assert int(m2.group(1)) <= int(m1.group(1)) and int(m2.group(2)) >= 1
    # the written tree scores what was printed
    out2 = run("-te", str(tmp_path / "a.parstree"), "-pars", pre="b")
    m = re.search(r"Parsimony score: (\d+) \(based on (\d+) informative sites\)", out2)
    assert m and m.group(1) == m2.group(1) and m.group(2) == m1.group(2)
    # a given tree: -pars -sprrad improves the stepwise-addition tree to a score no worse, and an SPR optimum stays put
    plain = run("-parstree", pre="c")
    out3 = run("-te", str(tmp_path / "c.parstree"), "-pars", "-sprrad", "2", pre="d")
    m3 = re.search(r"Parsimony score: (\d+) .*\nParsimony score after SPR: (\d+) \((\d+) rounds\)", out3)
    assert m3 and m3.group(1) == m1.group(1) and int(m3.group(2)) <= int(m3.group(1))
    out4 = run("-te", str(tmp_path / "a.parstree"), "-pars", "-sprrad", "2", pre="e")
    m4 = re.search(r"Parsimony score after SPR: (\d+) \((\d+) rounds\)", out4)
    assert m4 and m4.groups() == (m2.group(1), "1")
    # without -sprrad the output is what it was: the same lines as with it, less the SPR line
    assert "SPR" not in plain

    def shape(text, pre):
        return [re.sub(r"-?\d[\d.e+-]*", "#", ln) for ln in text.replace(str(tmp_path / pre), "PRE").splitlines()]

    with_spr = shape(out, "a")
    del with_spr[k[0] + 1]
    assert shape(plain, "c") == with_spr
    assert with_spr[k[0]:k[0] + 2] == ["Parsimony score: # (based on # informative sites)",
                                       "Parsimony tree: # s, printed to PRE.parstree"]
    # -sprrad needs -parstree or -pars, and a radius in 1 .. 10
    for args in (["-te", str(tmp_path / "a.parstree"), "-sprrad", "2"], ["-parstree", "-sprrad", "0"], ["-parstree", "-sprrad", "11"]):
        r = subprocess.run([binary, "-s", example, "-m", model] + args, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and "usage" in r.stderr
