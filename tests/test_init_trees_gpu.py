"""GPU: the starting population of the tree search -- TreeSearch(num_init_trees > 0), the reference's createInitTrees +
initCandidateTreeSet on a forest of parsimony trees built in lockstep -- against its restatement tests/init_trees_ref.py,
which builds every parsimony tree alone and runs nni_search_ref's optimize_nni.  Inputs: tests/init_trees_case.py (their
conditions are checked in test_init_trees_host.py).  Scores are compared to 1e-10 relative, the tolerance of the existing
search traces (the restatement reads every tree into a fresh engine)."""
import functools

import numpy as np
import pytest

import init_trees_case as case
import init_trees_ref as iref
import nni_search_ref as ref
import ufboot_ref
from test_tree_search_gpu import BootReplay, assert_same_steps, attach, boot_tree, strip_steps

pytestmark = pytest.mark.gpu

RTOL = 1e-10
NUM_NNI = 3
LOOP = 2


@functools.lru_cache(maxsize=None)
def start_of(name):
    """-> (data for attach, the given tree: a random topology with optimised lengths)"""
    import importlib
    from conftest import load_package
    pkg = load_package()
    synth = importlib.import_module("iqtree_amd.synth")
    true, n, model, pat, freq = case.data(name)
    data = (n, model, pat, freq)
    t = attach(pkg, synth.random_tree_newick(pat.shape[0], 4000 + case.CASES[name][4]), data)
    t.compute_likelihood()
    t.optimize_all_branches()
    return data, t.tree_string()


def close(a, b):
    return abs(a - b) <= RTOL * abs(b)


@pytest.mark.parametrize("name", ["dna10", "prot8"])
def test_initial_candidate_set_equals_the_restatement(pkg, synth, monkeypatch, name):
    monkeypatch.delenv("IQHIP_PARS_FOREST_CHUNK", raising=False)
    data, start = start_of(name)
    ntaxa, seed = case.CASES[name][2], case.SEARCH_SEED[name]
    make = lambda nwk: attach(pkg, nwk, data)
    t = make(start)
    t.pars_batch_timing()
    ts = pkg.TreeSearch(t, seed=seed, iterations=LOOP, num_init_trees=case.NUM_INIT, num_nni_trees=NUM_NNI)
    best, its = ts.search(trace=True)
    # the forest was one: T - 3 batch scans for the seven trees
    bt = t.pars_batch_timing()
    assert (bt["launches"], bt["segments"]) == (2 * (ntaxa - 3), (case.NUM_INIT - 1) * (ntaxa - 3))
    init, dup, kept, scores, traces, cand = iref.init_candidate_set(pkg, make, start, seed, case.NUM_INIT, NUM_NNI)
    # the distinct starting trees in generation order, and the duplicates (both occur: test_init_trees_host.py)
    assert ts.init_duplicates == dup >= 1 and len(ts.init_trees) == len(init) == case.NUM_INIT - dup >= 3
    assert [c[2] for c in ts.init_trees] == [c[2] for c in init]
    assert ts.init_trees[0][2] == make(start).sorted_taxon_id_string()
    for g, w in zip(ts.init_trees, init):
        assert close(g[0], w[0]), (g[0], w[0])
        assert set(pkg.newick_splits(g[1], ntaxa)) == set(pkg.newick_splits(w[1], ntaxa))
    # which three are kept, and their order: the iterations 1 .. 3 read them
    order = sorted(range(len(ts.init_trees)), key=lambda k: -ts.init_trees[k][0])[:NUM_NNI]
    assert [ts.init_trees[k][2] for k in order] == [c[2] for c in kept]
    assert [it["iteration"] for it in its] == list(range(1, NUM_NNI + LOOP + 1))
    assert all(it["parent"] == -1 and it["random_nnis"] == [] for it in its[:NUM_NNI])
    assert all(it["parent"] >= 0 and len(it["random_nnis"]) == int(0.5 * (ntaxa - 3)) for it in its[NUM_NNI:])
    for it, s, tr in zip(its[:NUM_NNI], scores, traces):
        assert close(it["score"], s), (it["iteration"], it["score"], s)
        assert_same_steps(it["steps"], tr, RTOL)
    assert its[0]["new_best"]
    # the loop continues at M + 1 on the set the starting trees left
    nstart = len(cand.trees)
    loop_scores, loop_traces = iref.replay_loop(make, cand, its[NUM_NNI:])
    for it, s, tr in zip(its[NUM_NNI:], loop_scores, loop_traces):
        assert close(it["score"], s), (it["iteration"], it["score"], s)
        assert_same_steps(it["steps"], tr, RTOL)
    assert its[NUM_NNI]["parent"] == pkg.search_rand_int(pkg.search_rand(seed, NUM_NNI + 1, 0), min(5, nstart))
    got = ts.candidates()
    assert [c[2] for c in got] == [c[2] for c in cand.ranked()] and len({c[2] for c in got}) == len(got)
    np.testing.assert_allclose([c[0] for c in got], [c[0] for c in cand.ranked()], rtol=RTOL)
    assert best == ts.best_score == got[0][0] == max(it["score"] for it in its)
    assert close(t.compute_likelihood(), best)
    # the same seed again: the same trace; the chunked forest: the same trace
    monkeypatch.setenv("IQHIP_PARS_FOREST_CHUNK", "3")
    ts2 = pkg.TreeSearch(make(start), seed=seed, iterations=LOOP, num_init_trees=case.NUM_INIT, num_nni_trees=NUM_NNI)
    _, its2 = ts2.search(trace=True)
    assert strip_steps(its2) == strip_steps(its) and ts2.init_trees == ts.init_trees


def test_default_is_the_one_tree_search(pkg, synth):
    """num_init_trees = 0: the trace of the search from the given tree alone, whatever the other two parameters say"""
    data, start = start_of("dna10")
    runs = []
    for kw in ({}, dict(num_init_trees=0, num_nni_trees=3, init_spr_radius=2)):
        t = attach(pkg, start, data)
        t.pars_batch_timing()
        ts = pkg.TreeSearch(t, seed=2, iterations=3, **kw)
        best, its = ts.search(trace=True)
        assert t.pars_batch_timing()["launches"] == 0 and ts.init_trees == [] and ts.init_duplicates == 0
        runs.append((best, strip_steps(its), ts.candidates()))
    assert runs[0] == runs[1]
    assert [x[0] for x in runs[0][1]] == [1, 2, 3, 4] and runs[0][1][0][1] == -1
    # and it is what the restatement of the one-tree search replays
    t = attach(pkg, start, data)
    _, its = pkg.TreeSearch(t, seed=2, iterations=3).search(trace=True)
    scores, _ = ref.replay_search(lambda nwk: attach(pkg, nwk, data), start, its)
    assert all(close(it["score"], s) for it, s in zip(its, scores))


def test_one_kept_tree_and_more_kept_than_there_are(pkg, synth):
    data, start = start_of("dna10")
    seed = case.SEARCH_SEED["dna10"]
    t = attach(pkg, start, data)
    ts = pkg.TreeSearch(t, seed=seed, iterations=1, num_init_trees=case.NUM_INIT, num_nni_trees=1)
    _, its = ts.search(trace=True)
    assert [it["iteration"] for it in its] == [1, 2] and its[1]["parent"] == 0
    ndistinct = len(ts.init_trees)
    ts = pkg.TreeSearch(attach(pkg, start, data), seed=seed, iterations=0, num_init_trees=case.NUM_INIT, num_nni_trees=50)
    _, its = ts.search(trace=True)
    assert len(its) == ndistinct == case.NUM_INIT - ts.init_duplicates        # every distinct tree, no loop iteration
    # SPR rounds on the parsimony trees: the restatement runs optimize_parsimony_spr on every tree alone
    ts = pkg.TreeSearch(attach(pkg, start, data), seed=seed, iterations=0, num_init_trees=5, num_nni_trees=2, init_spr_radius=2)
    ts.search()
    init, dup, *_ = iref.init_candidate_set(pkg, lambda nwk: attach(pkg, nwk, data), start, seed, 5, 2, spr_radius=2)
    assert ts.init_duplicates == dup and [c[2] for c in ts.init_trees] == [c[2] for c in init]
    assert all(close(g[0], w[0]) for g, w in zip(ts.init_trees, init))


def test_starting_trees_feed_the_bootstrap(pkg, synth):
    data, start = start_of("dna10")
    freq, seed = data[3], case.SEARCH_SEED["dna10"]
    ns = 100
    W = np.random.default_rng(7).multinomial(int(freq.sum()), freq / freq.sum(), size=ns).astype(np.float32)
    t = boot_tree(pkg, start, data, W)
    t.ufboot_init(ns, seed=11)
    # (with UFBoot `iterations` caps max_iterations, which counts the starting trees' iterations too: 3 + 1 in all)
    ts = pkg.TreeSearch(t, seed=seed, iterations=NUM_NNI, step_iterations=2, num_init_trees=case.NUM_INIT, num_nni_trees=NUM_NNI)
    best, its = ts.search(trace=True)
    assert [it["iteration"] for it in its] == [1, 2, 3, 4]
    fed = sum(1 + len(s["evaluated"]) for it in its for s in it["steps"] if s["branches"])
    assert t.ufboot_info()["trees_fed"] == fed
    fed_start = sum(1 + len(s["evaluated"]) for it in its[:NUM_NNI] for s in it["steps"] if s["branches"])
    assert 0 < fed_start < fed
    replay = BootReplay(pkg, ns, 11)
    make = lambda nwk: boot_tree(pkg, nwk, data, W)
    init, dup, kept, scores, traces, cand = iref.init_candidate_set(pkg, make, start, seed, case.NUM_INIT, NUM_NNI, boot=replay)
    assert replay.next_id == fed_start                      # every evaluated tree of the iterations 1 .. M, and nothing else
    iref.replay_loop(make, cand, its[NUM_NNI:], boot=replay)
    assert replay.next_id == fed
    got = t.ufboot_state()
    np.testing.assert_array_equal(got["boot_tree"], replay.state["boot_tree"])
    np.testing.assert_array_equal(got["boot_counts"], replay.state["boot_counts"])
    np.testing.assert_allclose(got["boot_logl"], replay.state["boot_logl"], rtol=1e-12)
    np.testing.assert_allclose(got["boot_orig_logl"], replay.state["boot_orig_logl"], rtol=1e-10)


def test_refusals(pkg, synth):
    data, start = start_of("dna10")
    t = attach(pkg, start, data)
    before = t.tree_string()
    for kw in (dict(num_init_trees=-1), dict(num_init_trees=4, init_spr_radius=11), dict(num_init_trees=4, init_spr_radius=-1)):
        with pytest.raises(pkg.HostError, match="numInitTrees"):
            pkg.TreeSearch(t, iterations=1, **kw).search()
    # an engine the parsimony calls refuse: 5 states are embedded
    model5 = synth.random_reversible_model(5, 4, alpha=0.7, ncat=4)
    nwk, pat, freq = synth.make_workload(8, 100, model5, seed=3)
    t5 = pkg.PhyloTree(nwk)
    t5.set_mem_mode(pkg.LM_ALL_BRANCH)
    t5.set_alignment(5, 3, pat, freq)
    t5.set_model(model5)
    t5.set_likelihood_kernel(pkg.LK_EIGEN_HIP)
    t5.attach_engine(0)
    with pytest.raises(pkg.HostError, match="parsimony"):
        pkg.TreeSearch(t5, iterations=1, num_init_trees=4).search()
    assert np.isfinite(pkg.TreeSearch(t5, iterations=1).search())            # without starting trees it searches
    assert t.tree_string() == before
