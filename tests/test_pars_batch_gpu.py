"""GPU: the segmented insertion scan iqhip_pars_insert_scores_batch (include/iqhip.h "Fitch parsimony") -- one
stepwise-addition step of many trees in one call -- against the numpy restatement of tests/fitch_ref.py and against
iqhip_pars_insert_scores.  Integer arithmetic throughout: every comparison is exact equality.

Site counts: 1; 33 (padding bits in the last word); 2049 = 65 word columns (a wave's strided loop makes a second, partial
pass); 8225 = 258 columns (the workgroup route makes a second, partial pass, and the unforced call leaves the wave route).
The vectors are those of a 9-taxon random tree; five segments of 1, 3, 7, 2 and 9 branches with five different taxa: unequal
lengths, a one-branch segment, and 22 branches in all, so the last workgroup of the wave route is half empty."""
import functools

import numpy as np
import pytest

import fitch_ref as F
from test_parsimony_gpu import alignment, all_directed_ops, make_tree, slot_of

pytestmark = pytest.mark.gpu

NTREE, NNEW = 9, 5
T = NTREE + NNEW
SEG_LEN = (1, 3, 7, 2, 9)
ROUTES = (None, "wave", "wg")


@functools.lru_cache(maxsize=None)
def problem(n, nsites):
    """-> states, freq, mask, ops, ends of every branch, and per (branch, taxon) the restated score; computed once per shape
    and left unchanged"""
    rng = np.random.default_rng(n * 1009 + nsites)
    states, freq, mask = alignment(n, T, nsites, rng)
    states[NTREE + 1] = states[2]          # a copy of a leaf of the tree: ties between the two branches beside it
    sp = F.site_patterns(freq, mask)
    tips = F.tip_vectors(states, sp, n)
    adj = F.random_tree(NTREE, rng, first_internal=T)
    ops, slot = all_directed_ops(adj, T)
    br = F.branches(adj)
    assert len(br) == 2 * NTREE - 3
    ends = [(slot_of(slot, a, b, T), slot_of(slot, b, a, T)) for a, b in br]
    dv = F.directed_vectors(adj, tips)
    want = np.array([[F.insert_score(dv[(a, b)], dv[(b, a)], (tips[x], 0)) for x in range(NTREE, T)] for a, b in br])
    return states, freq, mask, ops, ends, want


def set_route(monkeypatch, route):
    if route is None:
        monkeypatch.delenv("IQHIP_PARS_BATCH_ROUTE", raising=False)
    else:
        monkeypatch.setenv("IQHIP_PARS_BATCH_ROUTE", route)


def ready_tree(pkg, synth, n, nsites):
    states, freq, mask, ops, ends, want = problem(n, nsites)
    t = make_tree(pkg, synth, n, states, freq)
    assert t.pars_init(mask) == nsites
    t.pars_update(ops)
    return t, ends, want


def segments(rng, nbranch):
    """five segments over the tree's branches, any branch in any segment -> branch indices per segment, taxa"""
    idx = [[int(x) for x in rng.choice(nbranch, size=k, replace=False)] for k in SEG_LEN]
    taxa = [int(x) for x in NTREE + rng.permutation(NNEW)]
    return idx, taxa


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("nsites", [1, 33, 2049, 8225])
@pytest.mark.parametrize("n", [4, 20, 64])
def test_segments_equal_the_restatement(pkg, synth, monkeypatch, n, nsites, route):
    set_route(monkeypatch, route)
    t, ends, want = ready_tree(pkg, synth, n, nsites)
    assert t.pars_shape()[1] == (nsites + 31) // 32
    rng = np.random.default_rng(nsites + n)
    idx, taxa = segments(rng, len(ends))
    assert sum(len(s) for s in idx) == 22 and len(set(taxa)) == 5
    flat = [ends[b] for s in idx for b in s]
    seg_start = np.concatenate([[0], np.cumsum([len(s) for s in idx])])
    t.pars_timing()
    t.pars_batch_timing()
    score, best, best_score = t.pars_insert_scores_batch(flat, seg_start, taxa)
    want_seg = [[int(want[b, x - NTREE]) for b in s] for s, x in zip(idx, taxa)]
    assert score.tolist() == [w for s in want_seg for w in s]
    assert best.tolist() == [int(np.argmin(w)) for w in want_seg]            # np.argmin: the first minimum
    assert best_score.tolist() == [min(w) for w in want_seg]
    # without the scores only the minima come back, and they are the same; so is a second run
    none, best2, bs2 = t.pars_insert_scores_batch(flat, seg_start, taxa, want_scores=False)
    assert none is None and best2.tolist() == best.tolist() and bs2.tolist() == best_score.tolist()
    again = t.pars_insert_scores_batch(flat, seg_start, taxa)
    assert all(np.array_equal(a, b) for a, b in zip(again, (score, best, best_score)))
    # the batch has its own counters; those of the one-taxon scan do not move
    bt = t.pars_batch_timing()
    assert (bt["launches"], bt["branches"], bt["segments"]) == (6, 66, 15)
    pt = t.pars_timing()
    assert (pt["update_launches"], pt["scan_launches"], pt["ops"], pt["branches"]) == (0, 0, 0, 0)
    assert t.pars_batch_timing()["launches"] == 0                              # (the read reset them)
    # one segment per call is iqhip_pars_insert_scores
    for s, x in zip(idx, taxa):
        e = [ends[b] for b in s]
        one = t.pars_insert_scores(e, x)
        got = t.pars_insert_scores_batch(e, [0, len(e)], [x])
        assert got[0].tolist() == one[0].tolist() and (int(got[1][0]), int(got[2][0])) == (one[1], one[2])
    t.close()


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("n", [4, 20, 64])
def test_ties_go_to_the_lower_index(pkg, synth, monkeypatch, n, route):
    set_route(monkeypatch, route)
    t, ends, want = ready_tree(pkg, synth, n, 33)
    x = NTREE + int(np.argmax((want > want.min(axis=0)).sum(axis=0)))   # the taxon with the most branches above its minimum
    col = want[:, x - NTREE]
    lo = int(np.argmin(col))
    others = [b for b in range(len(ends)) if col[b] > col[lo]]
    assert len(others) >= 1
    # the minimum twice, at indices 1 and 3; and a second segment whose minimum is its last branch, listed once
    seg0 = [others[0], lo, others[-1], lo]
    seg1 = [others[-1], others[0], lo]
    flat = [ends[b] for b in seg0 + seg1]
    score, best, best_score = t.pars_insert_scores_batch(flat, [0, 4, 7], [x, x])
    assert score.tolist() == [int(col[b]) for b in seg0 + seg1]
    assert best.tolist() == [1, 2] and best_score.tolist() == [int(col[lo])] * 2
    # the twin of a leaf costs the same on either side of ... the branch of that leaf listed twice
    twin = NTREE + 1
    tcol = want[:, twin - NTREE]
    m = int(np.argmin(tcol))
    _, b2, s2 = t.pars_insert_scores_batch([ends[m], ends[m]], [0, 2], [twin], want_scores=False)
    assert b2.tolist() == [0] and s2.tolist() == [int(tcol[m])]
    t.close()


def test_every_branch_of_a_large_forest_step(pkg, synth, monkeypatch):
    """more segments than one workgroup has threads for a minimum search to be trivial: 300 segments of all 15 branches"""
    n, nsites = 4, 2049
    t, ends, want = ready_tree(pkg, synth, n, nsites)
    nseg = 300
    taxa = [NTREE + (g % NNEW) for g in range(nseg)]
    rng = np.random.default_rng(5)
    perms = [rng.permutation(len(ends)) for _ in range(nseg)]
    flat = [ends[b] for p in perms for b in p]
    seg_start = np.arange(nseg + 1) * len(ends)
    res = {}
    for route in ROUTES:
        set_route(monkeypatch, route)
        res[route] = t.pars_insert_scores_batch(flat, seg_start, taxa)
    want_seg = [[int(want[b, x - NTREE]) for b in p] for p, x in zip(perms, taxa)]
    for route in ROUTES:
        score, best, best_score = res[route]
        assert score.tolist() == [w for s in want_seg for w in s], route
        assert best.tolist() == [int(np.argmin(w)) for w in want_seg], route
        assert best_score.tolist() == [min(w) for w in want_seg], route
    t.close()
