"""GPU: K stepwise-addition parsimony trees built in lockstep (iq-tree_amd/host/pars_forest_host.h,
PhyloTree.compute_parsimony_forest) against the one-tree path compute_parsimony_tree -- trace, score and Newick string with
lengths, string for string -- and against the restatement fitch_ref.stepwise_addition; the engine calls a forest costs; the
chunked form; SPR rounds in lockstep against optimize_parsimony_spr on every tree alone; and the owner tree afterwards."""
import functools

import numpy as np
import pytest

import fitch_ref as F
from init_trees_case import adj_splits
from test_parsimony_gpu import alignment, make_tree

pytestmark = pytest.mark.gpu

K = 6
SHAPES = [(4, 9, 33), (4, 12, 70), (20, 9, 40), (64, 7, 40)]   # states, taxa, sites


@functools.lru_cache(maxsize=None)
def case(n, ntaxa, nsites):
    rng = np.random.default_rng(n * 100 + ntaxa)
    states, freq, _ = alignment(n, ntaxa, nsites, rng)
    if n != 4:   # few states per column, or hardly any protein / codon column is informative
        states = np.where(states < n, states % 4, states).astype(np.uint8)
    return states, freq


@functools.lru_cache(maxsize=None)
def single_trees(pkg, synth, n, ntaxa, nsites, spr=0):
    """every order through compute_parsimony_tree on a fresh tree: (score, steps, newick[, after SPR: score, newick])"""
    states, freq = case(n, ntaxa, nsites)
    out = []
    for order in pkg.parsimony_orders(17, K, ntaxa):
        t = make_tree(pkg, synth, n, states, freq)
        score, steps = t.compute_parsimony_tree(order, trace=True)
        row = [score, steps, t.tree_string()]
        if spr:
            row += [t.optimize_parsimony_spr(spr), t.tree_string()]
        out.append(tuple(row))
        t.close()
    return out


@pytest.mark.parametrize("n,ntaxa,nsites", SHAPES)
def test_forest_equals_every_tree_alone(pkg, synth, monkeypatch, n, ntaxa, nsites):
    monkeypatch.delenv("IQHIP_PARS_FOREST_CHUNK", raising=False)
    states, freq = case(n, ntaxa, nsites)
    orders = pkg.parsimony_orders(17, K, ntaxa)
    alone = single_trees(pkg, synth, n, ntaxa, nsites)
    t = make_tree(pkg, synth, n, states, freq)
    before = t.tree_string()
    t.pars_timing()
    t.pars_batch_timing()
    forest = t.compute_parsimony_forest(orders, trace=True)
    assert len(forest) == K and t.tree_string() == before
    # the engine calls of a whole forest: T - 3 batch scans, as many updates plus the final one, one branch-scores call
    bt, pt, fc = t.pars_batch_timing(), t.pars_timing(), t.forest_calls
    assert (bt["launches"], bt["segments"]) == (2 * (ntaxa - 3), K * (ntaxa - 3))
    assert bt["branches"] == K * sum(2 * cur - 3 for cur in range(3, ntaxa))
    assert (pt["update_launches"], pt["scan_launches"]) == (ntaxa - 2, 0)
    assert fc == dict(updates=ntaxa - 2, scans=ntaxa - 3, branch_scores=1, spr_scans=0, inits=1)
    inf = F.is_informative(states, n)
    tips = F.tip_vectors(states, F.site_patterns(freq, inf), n)
    for order, got, (score, steps, newick) in zip(orders, forest, alone):
        assert got["score"] == score and got["newick"] == newick
        assert got["topology"] == pkg.PhyloTree(newick).sorted_taxon_id_string()     # the key of a tree that read the string
        assert len(got["steps"]) == len(steps) == ntaxa - 3
        for g, w in zip(got["steps"], steps):
            assert g["branches"] == w["branches"] and g["scores"] == w["scores"] and g["chosen"] == w["chosen"]
            assert g["best_score"] == min(w["scores"])
        ref_score, adj, _, _ = F.stepwise_addition(tips, order)
        assert got["score"] == ref_score
        assert set(pkg.newick_splits(got["newick"], ntaxa)) == adj_splits(adj, ntaxa)
    # without a trace: the same trees
    plain = t.compute_parsimony_forest(orders)
    assert [(m["newick"], m["score"], m["steps"]) for m in plain] == [(m["newick"], m["score"], None) for m in forest]
    # the chunked form: three arenas of two trees, the same results
    monkeypatch.setenv("IQHIP_PARS_FOREST_CHUNK", "2")
    chunked = t.compute_parsimony_forest(orders, trace=True)
    assert t.forest_calls == dict(updates=3 * (ntaxa - 2), scans=3 * (ntaxa - 3), branch_scores=3, spr_scans=0, inits=3)
    assert chunked == forest
    monkeypatch.setenv("IQHIP_PARS_FOREST_CHUNK", "4")    # a last chunk that is not full
    assert t.compute_parsimony_forest(orders, trace=True) == forest
    monkeypatch.setenv("IQHIP_PARS_FOREST_CHUNK", "two")
    with pytest.raises(pkg.HostError):
        t.compute_parsimony_forest(orders)
    monkeypatch.delenv("IQHIP_PARS_FOREST_CHUNK")
    # the owner afterwards: its own tree, its own parsimony arena again, its likelihood
    fresh = make_tree(pkg, synth, n, states, freq, nwk=before)
    assert t.compute_parsimony() == fresh.compute_parsimony()
    assert t.compute_likelihood() == fresh.compute_likelihood()
    assert t.compute_parsimony_tree(orders[0]) == alone[0][0] and t.tree_string() == alone[0][2]
    fresh.close()
    t.close()


def test_spr_rounds_in_lockstep(pkg, synth, monkeypatch):
    monkeypatch.delenv("IQHIP_PARS_FOREST_CHUNK", raising=False)
    n, ntaxa, nsites = 4, 12, 70
    states, freq = case(n, ntaxa, nsites)
    orders = pkg.parsimony_orders(17, K, ntaxa)
    alone = single_trees(pkg, synth, n, ntaxa, nsites, 3)
    t = make_tree(pkg, synth, n, states, freq)
    t.pars_spr_timing()
    forest = t.compute_parsimony_forest(orders, spr_radius=3)
    for got, (_, _, _, score, newick) in zip(forest, alone):
        assert got["score"] == score and got["newick"] == newick
    # one scan per round, and a member scans once more than it moves: the longest member sets the number of rounds
    rounds = 1 + max(m["spr_moves"] for m in forest)
    assert t.forest_calls["spr_scans"] == rounds and t.pars_spr_timing()["launches"] >= rounds
    assert any(m["spr_moves"] > 0 for m in forest)     # (the case moves something, or it shows nothing)
    monkeypatch.setenv("IQHIP_PARS_FOREST_CHUNK", "4")
    assert t.compute_parsimony_forest(orders, spr_radius=3) == forest
    with pytest.raises(pkg.HostError):
        t.compute_parsimony_forest(orders, spr_radius=11)
    t.close()
