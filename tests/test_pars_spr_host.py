"""CPU: iqhip_debug_pars_spr_check -- the validation iqhip_pars_spr_scan runs before it launches anything -- on what
PhyloTree::collectSprJobs produces and on one mutation of each rule; collectSprJobs / applySprMove of the host mirror against
the restatement of tests/spr_ref.py; and the restatement itself against brute force: every move's insertion-formula score is
the Fitch score of the rearranged tree computed from scratch and its Sankoff minimum."""
import ctypes as C

import numpy as np
import pytest

import fitch_ref as F
import spr_ref as S

IQHIP_ERR_INVALID = 2


def mirror_tree(pkg, adj):
    t = pkg.PhyloTree(F.newick(adj))
    t.set_dry_run(True)
    return t


def refused(pkg, ntaxa, nvec, jobs, steps, valid=None, words=None):
    with pytest.raises(pkg.EngineError) as ei:
        pkg.debug_pars_spr_check(ntaxa, nvec, jobs, steps, valid)
    assert ei.value.code == IQHIP_ERR_INVALID
    if words:
        assert words in str(ei.value), str(ei.value)


# ---- the mirror's jobs ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,ntaxa,radius", [("caterpillar", 4, 1), ("caterpillar", 9, 2), ("caterpillar", 17, 10),
                                                 ("random", 5, 6), ("random", 12, 1), ("random", 12, 3), ("random", 30, 6)])
def test_mirror_jobs_equal_the_restatement_and_pass_the_check(pkg, shape, ntaxa, radius):
    rng = np.random.default_rng(ntaxa * 10 + radius)
    t = mirror_tree(pkg, F.caterpillar(ntaxa) if shape == "caterpillar" else F.random_tree(ntaxa, rng))
    adj = S.mirror_adjacency(t)
    jobs, steps, moves = t.collect_spr_jobs(radius)
    want = S.collect_jobs(adj, ntaxa, radius)
    assert len(jobs) == len(want) and len(steps) == sum(len(j["steps"]) for j in want)
    # the slots name directed vectors: a leaf's is its taxon, every other (node, seen from) has one of its own
    slot = {}
    k = 0
    for jr, job in zip(jobs, want):
        assert jr[1] == k and jr[2] == len(job["steps"])
        slot.setdefault((job["s"], job["p"]), int(jr[0]))
        assert slot[(job["s"], job["p"])] == jr[0]
        for st in job["steps"]:
            parent, side, target, flags = (int(x) for x in steps[k])
            assert parent == st["parent"] and flags == (0 if st["scored"] else S.NO_SCORE)
            for key, got in ((st["side"], side), (st["target"], target)):
                assert slot.setdefault(key, got) == got
                assert got == key[0] if key[0] < ntaxa else got >= ntaxa
            assert tuple(int(x) for x in moves[k]) == (job["p"], job["s"]) + st["move"] + (st["depth"],)
            k += 1
    internal = [v for key, v in slot.items() if key[0] >= ntaxa]
    assert len(set(internal)) == len(internal) and all(ntaxa <= v < ntaxa + 4 * (ntaxa - 1) for v in internal)
    nvec = 4 * (ntaxa - 1)
    depth = pkg.debug_pars_spr_check(ntaxa, nvec, jobs, steps, valid=np.ones(nvec))
    assert depth.tolist() == [st["depth"] for j in want for st in j["steps"]] == moves[:, 4].tolist()
    assert depth.max() <= radius
    if shape == "caterpillar" and ntaxa == 17:
        assert depth.max() == 10                 # the radius cuts the walk
    # every job starts with the scored root step, the other root step is the only unscored one
    for first, n in jobs[:, 1:3]:
        flags = steps[first:first + n, 3]
        assert flags[0] == 0 and flags.sum() == 1 and steps[first, 0] == -1
    t.close()


def test_four_taxa_have_moves_and_three_have_none(pkg):
    t = mirror_tree(pkg, F.caterpillar(4))
    jobs, steps, moves = t.collect_spr_jobs(3)
    # pruning a leaf leaves a three-leaf star plus the merged branch's two neighbours; pruning a cherry leaves nowhere to go
    assert len(jobs) == 4 and all(n == 4 for n in jobs[:, 2]) and (moves[:, 4] <= 1).all()
    t.close()
    t3 = pkg.PhyloTree("(0:0.1,1:0.1,2:0.1);")
    t3.set_dry_run(True)
    jobs, steps, moves = t3.collect_spr_jobs(3)
    assert len(jobs) == 0 and len(steps) == 0
    assert pkg.debug_pars_spr_check(3, 0, jobs, steps).size == 0
    with pytest.raises(pkg.HostError):
        t3.collect_spr_jobs(0)
    with pytest.raises(pkg.HostError):
        t3.collect_spr_jobs(11)
    t3.close()


def test_apply_move_on_the_mirror_equals_the_restatement(pkg):
    rng = np.random.default_rng(3)
    ntaxa = 10
    t = mirror_tree(pkg, F.random_tree(ntaxa, rng))
    for _ in range(12):
        adj = S.mirror_adjacency(t)
        jobs = S.collect_jobs(adj, ntaxa, 4)
        job = jobs[int(rng.integers(len(jobs)))]
        st = [s for s in job["steps"] if s["depth"] >= 1]
        st = st[int(rng.integers(len(st)))]
        t.apply_spr_move(job["p"], job["s"], *st["move"])
        want = S.apply_move(adj, job["p"], job["s"], *st["move"])
        assert S.mirror_adjacency(t) == want
        assert sorted(F.branches(want)) == sorted(t.get_branches())
    # refused: the merged branch itself, a branch inside the pruned subtree, a subtree that does not hang there
    adj = S.mirror_adjacency(t)
    p = ntaxa
    s = adj[p][0]
    q1, q2 = adj[p][1], adj[p][2]
    with pytest.raises(pkg.HostError):
        t.apply_spr_move(p, s, q1, q2)
    with pytest.raises(pkg.HostError):
        t.apply_spr_move(p, [u for u in adj if u not in adj[p] and u != p][0], q1, q2)
    inner = [u for u in adj if u >= ntaxa and u != p and p not in adj[u]]
    far = inner[0]
    # the subtree seen from p that contains `far`: a branch at `far` lies inside it
    def contains(u, dad, x):
        return u == x or any(contains(k, u, x) for k in adj[u] if k != dad)
    side = [k for k in adj[p] if contains(k, p, far)][0]
    nb = [k for k in adj[far] if not contains(k, far, p)][0]
    with pytest.raises(pkg.HostError):
        t.apply_spr_move(p, side, far, nb)
    assert S.mirror_adjacency(t) == adj          # a refused move leaves the tree as it was
    t.close()


# ---- one mutation of each rule ----------------------------------------------------------------------------------------------
def test_every_refusal_of_the_check(pkg):
    T, V = 6, 12
    ok_valid = np.ones(V)
    #          parent side target flags
    steps = [(-1, 1, 2, 0),      # 0  depth 0
             (0, 6, 3, 0),       # 1  depth 1
             (1, 7, 4, 0),       # 2  depth 2
             (0, 8, 5, 0),       # 3  depth 1
             (3, 9, 0, 1)]       # 4  depth 2, not scored
    jobs = [(10, 0, 5)]
    assert pkg.debug_pars_spr_check(T, V, jobs, steps, ok_valid).tolist() == [0, 1, 2, 1, 2]

    def mutate(k, col, value, jb=jobs, valid=ok_valid, words=None):
        st = [list(s) for s in steps]
        st[k][col] = value
        refused(pkg, T, V, jb, st, valid, words)

    mutate(2, 0, 2, words="earlier step")                   # a forward parent: itself ...
    mutate(2, 0, 3, words="earlier step")                   # ... and a later step
    mutate(4, 0, 1, words="most recent")                    # a parent at the wrong depth of the stack: step 1's level was
    #                                                         overwritten by step 3
    st = [list(x) for x in steps]
    st[4][0] = 2                                            # (step 2 is still the most recent step of its depth: legal)
    assert pkg.debug_pars_spr_check(T, V, jobs, st, ok_valid).tolist() == [0, 1, 2, 1, 3]
    mutate(1, 1, T + V, words="outside")                    # an invalid slot: side ...
    mutate(1, 2, -1, words="outside")                       # ... target ...
    refused(pkg, T, V, [(T + V, 0, 5)], steps, ok_valid, words="outside")   # ... the subtree
    unset = ok_valid.copy()
    unset[1] = 0                                            # slot 7: an unset valid flag
    refused(pkg, T, V, jobs, steps, unset, words="never been written")
    refused(pkg, T, V, jobs, steps, None, words="never been written")
    refused(pkg, T, V, [(10, 0, 3), (11, 2, 3)], steps, ok_valid, words="earlier job")   # overlapping jobs
    refused(pkg, T, V, [(10, 3, 3)], steps, ok_valid, words="outside [0, nsteps)")
    refused(pkg, T, V, [(10, -1, 2)], steps, ok_valid, words="outside [0, nsteps)")
    mutate(0, 3, 2, words="unknown flag")
    mutate(0, 3, 3, words="unknown flag")
    # depth 10 is the limit, depth 11 is refused
    chain = [(-1, 1, 2, 0)] + [(k, 1, 2, 0) for k in range(10)]
    assert pkg.debug_pars_spr_check(T, V, [(0, 0, 11)], chain, ok_valid).tolist() == list(range(11))
    refused(pkg, T, V, [(0, 0, 12)], chain + [(10, 1, 2, 0)], ok_valid, words="deeper")
    # steps that belong to no job are not looked at; two disjoint jobs in any order are fine
    assert pkg.debug_pars_spr_check(T, V, [(11, 3, 2), (10, 0, 3)], [steps[0], steps[1], steps[2], (-1, 1, 2, 0), (0, 3, 4, 1)],
                                    ok_valid).tolist() == [0, 1, 2, 0, 1]
    assert pkg.debug_pars_spr_check(T, V, [(10, 1, 1)], [(5, 99, 99, 7), (-1, 1, 2, 0)], ok_valid).tolist() == [-1, 0]


def test_symbols_and_planner_refusals(pkg):
    lib = pkg.libiqhip()
    for s in ("iqhip_pars_spr_scan", "iqhip_debug_pars_spr_check", "iqhip_debug_pars_spr_timing"):
        assert hasattr(lib, s) and s in pkg.IQHIP_SYMBOLS, s
    assert pkg.PARS_SPR_NO_SCORE == S.NO_SCORE == 1 and pkg.PARS_SPR_MAX_RADIUS == 10
    e = C.c_void_p()
    assert lib.iqhip_debug_create_planner(C.byref(e), 4, 4, 100, 5, 256, 18, 1) == 0
    try:
        jobs = np.array([[0, 0, 1, 0]], dtype=np.int32)
        steps = np.array([[-1, 1, 2, 0]], dtype=np.int32)
        out = np.zeros(4, dtype=np.int32)
        p = out.ctypes.data_as(C.POINTER(C.c_int32))
        assert lib.iqhip_pars_spr_scan(e, jobs.ctypes.data_as(C.c_void_p), 1, steps.ctypes.data_as(C.c_void_p), 1, p, p, p, p) == IQHIP_ERR_INVALID
        assert b"planning-only" in lib.iqhip_last_error()
    finally:
        lib.iqhip_destroy(e)


# ---- the restatement against brute force ------------------------------------------------------------------------------------
@pytest.mark.parametrize("ntaxa", [5, 6])
def test_every_move_scores_the_rearranged_tree(ntaxa):
    rng = np.random.default_rng(ntaxa)
    st = F.random_states(ntaxa, 12, 4, rng, amb_frac=0.10)
    assert (st >= 4).any()
    sp = F.site_patterns(np.ones(12))
    tips = F.tip_vectors(st, sp, 4)
    seen = set()
    for adj in (F.caterpillar(ntaxa), F.random_tree(ntaxa, rng)):
        dv = F.directed_vectors(adj, tips)
        now = F.tree_score(adj, tips)
        jobs = S.collect_jobs(adj, ntaxa, 10)     # beyond the diameter: every SPR of the tree
        assert jobs
        for job in jobs:
            scores = S.job_scores(job, dv)
            assert scores[0] == now and [k for k, v in enumerate(scores) if v is None] == [
                k for k, s in enumerate(job["steps"]) if s["depth"] == 0][1:]
            for sc, step in zip(scores, job["steps"]):
                if step["depth"] == 0:
                    continue
                new = S.apply_move(adj, job["p"], job["s"], *step["move"])
                assert len(F.branches(new)) == 2 * ntaxa - 3 and all(len(v) in (1, 3) for v in new.values())
                assert sc == F.tree_score(new, tips), (job["p"], job["s"], step)
                assert sc == F.sankoff_min(new, st, sp, 4), (job["p"], job["s"], step)
                seen.add(frozenset(frozenset(x) for x in splits(new, ntaxa)))
    assert len(seen) > 10     # many different topologies were reached


def splits(adj, ntaxa):
    """the non-trivial bipartitions of a tree, each as the side that holds leaf 0"""
    out = []

    def leaves(u, dad):
        return {u} if u < ntaxa else set().union(*(leaves(k, u) for k in adj[u] if k != dad))

    for a, b in F.branches(adj):
        if a >= ntaxa and b >= ntaxa:
            side = leaves(a, b)
            out.append(side if 0 in side else set(range(ntaxa)) - side)
    return out


def test_search_restatement_ends_in_a_local_optimum():
    rng = np.random.default_rng(9)
    ntaxa = 9
    st = F.random_states(ntaxa, 60, 4, rng, amb_frac=0.10)
    sp = F.site_patterns(np.ones(60))
    tips = F.tip_vectors(st, sp, 4)
    start = F.caterpillar(ntaxa)
    score, adj, rounds = S.search(start, tips, ntaxa, 3)
    assert rounds and not rounds[-1]["applied"] and all(r["applied"] for r in rounds[:-1])
    befores = [r["score_before"] for r in rounds]
    assert befores[0] == F.tree_score(start, tips) and all(a > b for a, b in zip(befores, befores[1:]))
    assert score == befores[-1] == F.tree_score(adj, tips)
    dv = F.directed_vectors(adj, tips)
    assert all(sc is None or sc >= score for job in S.collect_jobs(adj, ntaxa, 3) for sc in S.job_scores(job, dv))
    one, adj1, r1 = S.search(start, tips, ntaxa, 3, max_rounds=1)
    assert len(r1) == 1 and r1[0] == rounds[0] and (one == rounds[0]["score"] == F.tree_score(adj1, tips) if rounds[0]["applied"] else True)
