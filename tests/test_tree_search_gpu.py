"""GPU: the NNI tree search (iq-tree_amd/host/tree_search_host.h) against its Python restatement (tests/nni_search_ref.py):
the batched evaluators on a branch list, optimize_nni step by step, the stochastic loop of TreeSearch.search with and without
UFBoot, and the refusals.  Data: synth.simulate_alignment on synth.random_tree_newick (branch lengths 0.02 .. 0.2)."""
import functools

import numpy as np
import pytest

import nni_search_ref as ref
import ufboot_ref
from test_parity_gpu import LNL_RTOL

pytestmark = pytest.mark.gpu

SEQ_TYPE = {4: 0, 20: 1, 64: 2}

# name -> (nstates, ncat, ntaxa, nsites, patterns kept (0: all), seed).  The seeds are ones for which the RESTATEMENT, started
# three random NNIs away from the tree the data were simulated on, ends on that tree's topology (chosen by running
# nni_search_ref.optimize_nni over seeds 0, 1, 2, ... and keeping the first that does; the code under test had no say).
SHAPES = {
    "dna12": (4, 4, 12, 1500, 0, 0),
    "prot8": (20, 4, 8, 600, 0, 0),
    "codon7": (64, 1, 7, 300, 0, 0),
    "dna30": (4, 4, 30, 64000, 40000, 0),
    "dna4": (4, 4, 4, 400, 0, 0),
}
# random topologies of 14 taxa x 800 sites, seeds 0 .. 199 through the restatement: the first seed whose trace rolls a step
# back (128), or None when no seed does (see test_rollback)
ROLLBACK_SEED = 128
VARIANTS = {"default": {}, "nni1": dict(nni5=False), "allnni": dict(speed=False), "unbatched": dict(batched=False)}


def model_for(synth, n, ncat, seed):
    return synth.gtr_model(alpha=0.9, ncat=ncat) if n == 4 else synth.random_reversible_model(n, seed, alpha=0.9, ncat=ncat)


def attach(pkg, newick, data, mem_mode=None):
    n, model, pat, freq = data
    t = pkg.PhyloTree(newick)
    t.set_mem_mode(pkg.LM_ALL_BRANCH if mem_mode is None else mem_mode)
    t.set_alignment(n, SEQ_TYPE[n], pat, freq)
    t.set_model(model)
    t.set_likelihood_kernel(pkg.LK_EIGEN_HIP)
    t.attach_engine(0)
    return t


def make_data(pkg, synth, n, ncat, ntaxa, nsites, keep, seed, start_from_true=True):
    """-> (true newick, data, start newick): the start is the true tree after three random NNIs (drawn with numpy from the
    seed) with its lengths re-optimised -- or, for the rollback hunt, a random topology with re-optimised lengths"""
    model = model_for(synth, n, ncat, seed)
    true = synth.random_tree_newick(ntaxa, 1000 + seed)
    pat, freq = synth.compress_patterns(synth.simulate_alignment(true, model, nsites, 2000 + seed))
    while keep and pat.shape[1] < keep:                     # (short branches: many sites repeat a pattern)
        nsites = int(nsites * 1.5)
        pat, freq = synth.compress_patterns(synth.simulate_alignment(true, model, nsites, 2000 + seed))
    if keep:
        pat, freq = np.ascontiguousarray(pat[:, :keep]), freq[:keep].copy()
    data = (n, model, pat, freq)
    rng = np.random.default_rng(3000 + seed)
    t = attach(pkg, true if start_from_true else synth.random_tree_newick(ntaxa, 4000 + seed), data)
    if start_from_true:
        for _ in range(3):
            inner = ref.internal_branches(ref.adjacency(t))
            a, b = inner[int(rng.integers(0, len(inner)))]
            t.do_random_nni(a, b, int(rng.integers(0, 2)), int(rng.integers(0, 2)))
        t.clear_all_partial_lh()
    t.compute_likelihood()
    t.optimize_all_branches()
    return true, data, t.tree_string()


@functools.lru_cache(maxsize=None)
def _shape(name):
    from conftest import load_package
    import importlib
    pkg = load_package()
    return make_data(pkg, importlib.import_module("iqtree_amd.synth"), *SHAPES[name])


@functools.lru_cache(maxsize=None)
def _reference_run(name, variant):
    """the restatement's run of (shape, variant), computed once; the unbatched variant is compared with the batched C++ run"""
    from conftest import load_package
    pkg = load_package()
    true, data, start = _shape(name)
    t = attach(pkg, start, data)
    start_lnl = t.compute_likelihood()
    return (start_lnl,) + ref.optimize_nni(t, **{k: v for k, v in VARIANTS[variant].items() if k != "batched"}) + (t.tree_string(),)


def moves_key(moves):
    return [(m["node1"], m["node2"], m["node1_nei"], m["node2_nei"]) for m in moves]


def assert_same_steps(got, want, rtol):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert [tuple(b) for b in g["branches"]] == [tuple(b) for b in w["branches"]]
        assert g["all_branches"] == w["all_branches"] and g["rolled_back"] == w["rolled_back"]
        assert moves_key(g["positive"]) == moves_key(w["positive"])
        assert moves_key(g["applied"]) == moves_key(w["applied"])
        for a, b in zip(g["positive"], w["positive"]):
            assert abs(a["newloglh"] - b["newloglh"]) <= rtol * abs(b["newloglh"])
        assert abs(g["score"] - w["score"]) <= rtol * abs(w["score"])


# ---- 1. restricted evaluation --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,ncat,ntaxa,nptn", [(4, 4, 13, 500), (20, 4, 8, 250)])
def test_restricted_evaluation_equals_the_full_call(pkg, synth, n, ncat, ntaxa, nptn):
    model = model_for(synth, n, ncat, 5)
    nwk, pat, freq = synth.make_workload(ntaxa, nptn, model, seed=60 + n)
    t = attach(pkg, nwk, (n, model, pat, freq))
    lnl = t.compute_likelihood()
    tree0 = t.tree_string()
    inner = ref.internal_branches(ref.adjacency(t))
    subset = [inner[-1], inner[0], inner[len(inner) // 2]]
    listed = [subset[0], (subset[1][1], subset[1][0]), subset[2]]             # one branch given the other way round
    for nni5 in (True, False):
        fresh = attach(pkg, nwk, (n, model, pat, freq))                       # no vector valid yet: only those needed are made
        fresh.compute_likelihood()
        n0 = fresh.num_partial_lh_computations
        part = fresh.evaluate_nnis5_batch(branches=listed) if nni5 else fresh.evaluate_nnis_batch(branches=listed)
        made = fresh.num_partial_lh_computations - n0
        full = t.evaluate_nnis5_batch() if nni5 else t.evaluate_nnis_batch()
        by = {}
        for m in full:
            by.setdefault((m["node1"], m["node2"]), []).append(m)
        want = [m for br in subset for m in by[br]]
        assert len(part) == 6 and moves_key(part) == moves_key(want)
        for g, w in zip(part, want):
            print("nni5 %d: lnL %.17g vs %.17g" % (nni5, g["newloglh"], w["newloglh"]))
            assert g["newloglh"] == w["newloglh"]
            assert (g["new_lens"] == w["new_lens"]) if nni5 else (g["new_len"] == w["new_len"])
        assert fresh.tree_string() == tree0
        assert abs(fresh.compute_likelihood() - lnl) <= 1e-12 * abs(lnl)
        fresh2 = attach(pkg, nwk, (n, model, pat, freq))
        fresh2.compute_likelihood()
        n1 = fresh2.num_partial_lh_computations
        fresh2.compute_all_partial_lh()
        assert made < fresh2.num_partial_lh_computations - n1                 # fewer vectors than "all of them"
    assert t.evaluate_nnis5_batch(branches=[]) == []
    with pytest.raises(pkg.HostError, match="not an internal branch"):
        t.evaluate_nnis5_batch(branches=[(0, t.neighbors(0)[0][0])])
    rows = t.evaluate_nnis5_batch(first_row=1, branches=subset)               # rows follow the LIST: candidate k -> row 1 + k
    assert abs(float(t.ptnlh_fetch(1 + 3) @ freq) - rows[3]["newloglh"]) <= 1e-9 * abs(lnl)


# ---- 2. + 3. optimize_nni against the restatement, and what every run must satisfy ----------------------------------------
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name", list(SHAPES))
def test_optimize_nni_equals_the_restatement(pkg, synth, name, variant):
    true, data, start = _shape(name)
    ntaxa = SHAPES[name][2]
    start_lnl, want_lnl, want_count, want_steps, want_trace, want_tree = _reference_run(name, variant)
    t = attach(pkg, start, data)
    lnl, count, steps, trace = t.optimize_nni(trace=True, **VARIANTS[variant])
    # batched against the restatement: one path run twice; unbatched against the batched restatement: batch vs sequential
    rtol = 1e-9 if variant == "unbatched" else 1e-10
    assert_same_steps(trace, want_trace, rtol)
    assert (count, steps) == (want_count, want_steps)
    assert abs(lnl - want_lnl) <= rtol * abs(want_lnl)
    got_splits = set(pkg.newick_splits(t.tree_string(), ntaxa))
    assert got_splits == set(pkg.newick_splits(want_tree, ntaxa))
    # properties
    accepted = [start_lnl] + [s["score"] for s in trace if s["applied"] and not s["rolled_back"]]
    assert all(b >= a for a, b in zip(accepted, accepted[1:]))
    assert lnl >= start_lnl
    assert abs(t.compute_likelihood() - lnl) <= 1e-10 * abs(lnl)
    again = attach(pkg, t.tree_string(), data)
    assert abs(again.compute_likelihood() - lnl) <= LNL_RTOL * abs(lnl)
    assert got_splits == set(pkg.newick_splits(true, ntaxa))                  # the seeds are chosen so (see SHAPES)
    if variant == "default" and ntaxa > 4:
        assert any(s["applied"] for s in trace)
        later = [s for s in trace[1:] if s["branches"]]
        assert all(not s["all_branches"] and len(s["branches"]) <= ntaxa - 3 for s in later)


def test_optimize_nni_works_per_node_when_unbatched(pkg, synth):
    true, data, start = _shape("dna12")
    _, want_lnl, want_count, want_steps, want_trace, _ = _reference_run("dna12", "default")
    t = attach(pkg, start, data, mem_mode=pkg.LM_PER_NODE)
    lnl, count, steps, trace = t.optimize_nni(batched=False, trace=True)
    assert_same_steps(trace, want_trace, 1e-9)
    assert count == want_count and abs(lnl - want_lnl) <= 1e-9 * abs(want_lnl)
    assert abs(t.compute_likelihood() - lnl) <= 1e-10 * abs(lnl)


# ---- 4. rollback ---------------------------------------------------------------------------------------------------------
def test_rollback(pkg, synth):
    """Seed 128 is the first of 0 .. 199 (random 14-taxon topologies, 800 sites) for which the restatement rolls a step back:
    the sweep after the applied set ends below the best single move, so the moves are reverted, the lengths restored, every
    vector cleared -- and, as in the reference, the loop ends there (the gain of a rolled-back step is 0).  The C++ loop must
    take the same steps and end on the same score.  Then the undo path on its own: k moves applied with their lengths,
    reverted, lengths restored and every vector cleared reproduce the starting lnL."""
    if ROLLBACK_SEED is not None:
        true, data, start = make_data(pkg, synth, 4, 4, 14, 800, 0, ROLLBACK_SEED, start_from_true=False)
        t = attach(pkg, start, data)
        want = ref.optimize_nni(t)
        assert any(s["rolled_back"] for s in want[3])
        t2 = attach(pkg, start, data)
        lnl, count, steps, trace = t2.optimize_nni(trace=True)
        assert_same_steps(trace, want[3], 1e-10)
        assert abs(lnl - want[0]) <= 1e-10 * abs(lnl) and abs(t2.compute_likelihood() - lnl) <= 1e-10 * abs(lnl)
        assert trace[-1]["rolled_back"] and set(pkg.newick_splits(t2.tree_string(), 14)) == set(pkg.newick_splits(t.tree_string(), 14))
    true, data, start = make_data(pkg, synth, 4, 4, 14, 800, 0, 0, start_from_true=False)
    t = attach(pkg, start, data)
    lnl = t.compute_likelihood()
    tree0 = t.tree_string()
    moves = t.evaluate_nnis5_batch()
    best = [max(moves[q:q + 2], key=lambda m: m["newloglh"]) for q in range(0, len(moves), 2)]
    chosen = ref.non_touching(ref.select_non_conflicting(sorted(best, key=lambda m: -m["newloglh"])))
    assert len(chosen) >= 2
    lens = t.save_branch_lengths()
    for m in chosen:
        t.do_nni(m)
        t.change_nni_brans(m, True)
    assert abs(t.optimize_all_branches(1, 0.001, 10) - lnl) > 1e-6 * abs(lnl)
    for m in chosen:
        t.do_nni(m)
    t.restore_branch_lengths(lens)
    t.clear_all_partial_lh()
    assert t.tree_string() == tree0
    assert abs(t.compute_likelihood() - lnl) <= 1e-12 * abs(lnl)


# ---- 5. the stochastic search -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _search_data():
    from conftest import load_package
    import importlib
    return make_data(load_package(), importlib.import_module("iqtree_amd.synth"), 4, 4, 10, 1000, 0, 1)


def strip_steps(iterations):
    return [(it["iteration"], it["parent"], it["random_nnis"], it["perturb_score"], it["score"], it["new_best"],
             [(s["branches"], moves_key(s["positive"]), moves_key(s["applied"]), s["score"], s["rolled_back"]) for s in it["steps"]])
            for it in iterations]


def test_tree_search_replays_through_the_restatement(pkg, synth):
    true, data, start = _search_data()
    traces = {}
    for seed in (1, 2):
        t = attach(pkg, start, data)
        ts = pkg.TreeSearch(t, seed=seed, iterations=6)
        best, its = ts.search(trace=True)
        traces[seed] = its
        assert [it["iteration"] for it in its] == list(range(1, 8)) and its[0]["parent"] == -1
        assert all(len(it["random_nnis"]) == int(0.5 * (10 - 3)) for it in its[1:])
        scores, cand = ref.replay_search(lambda nwk: attach(pkg, nwk, data), start, its)
        for it, s in zip(its, scores):
            assert abs(it["score"] - s) <= 1e-10 * abs(s)
        got = ts.candidates()
        assert [c[2] for c in got] == [c[2] for c in cand.ranked()]           # topologies and order
        assert len({c[2] for c in got}) == len(got)                            # no topology twice
        np.testing.assert_allclose([c[0] for c in got], [c[0] for c in cand.ranked()], rtol=1e-10)
        assert best == ts.best_score == got[0][0] == max(it["score"] for it in its)
        lnl = t.compute_likelihood()
        assert abs(lnl - best) <= 1e-10 * abs(best)                            # the best tree is loaded
        assert set(pkg.newick_splits(t.tree_string(), 10)) == set(pkg.newick_splits(got[0][1], 10))
        assert best >= its[0]["score"]
        # the same seed again: an identical trace
        t2 = attach(pkg, start, data)
        _, its2 = pkg.TreeSearch(t2, seed=seed, iterations=6).search(trace=True)
        assert strip_steps(its2) == strip_steps(its)
    assert [it["random_nnis"] for it in traces[1][1:]] != [it["random_nnis"] for it in traces[2][1:]]
    # the draws are those of the documented stream
    it = traces[1][1]
    assert it["parent"] == pkg.search_rand_int(pkg.search_rand(1, 2, 0), 1)
    assert it["random_nnis"][0][2:] == (pkg.search_rand(1, 2, 2) >> 63, pkg.search_rand(1, 2, 3) >> 63)


def test_tree_search_stops_without_improvement(pkg, synth):
    true, data, start = _search_data()
    t = attach(pkg, start, data)
    ts = pkg.TreeSearch(t, seed=3, num_stop=2)
    best, its = ts.search(trace=True)
    last = max(it["iteration"] for it in its if it["new_best"])
    assert its[-1]["iteration"] == last + 2                                   # two iterations without a better tree
    only_start = pkg.TreeSearch(attach(pkg, start, data), iterations=0)
    assert only_start.search() == its[0]["score"] <= best and len(only_start.candidates()) == 1


# ---- 6. search with UFBoot -----------------------------------------------------------------------------------------------
class BootReplay:
    """the bootstrap side of a replayed search: every tree the search feeds, in its order, through ufboot_ref.ufboot_rule on
    the device's RELL sums of the rows"""

    def __init__(self, pkg, nsamples, seed):
        self.pkg, self.ns, self.seed = pkg, nsamples, seed
        self.state = ufboot_ref.ufboot_start(nsamples)
        self.next_id = 0
        self.cutoff = 0.0
        self.min_orig = ufboot_ref.DBL_MAX

    def feed(self, tree, rows, logl):
        ids = np.arange(self.next_id, self.next_id + len(rows), dtype=np.int64)
        self.next_id += len(rows)
        rand = np.array([self.pkg.ufboot_rand(self.seed, int(k)) for k in ids])
        R = tree.ptnlh_rell(np.asarray(rows), self.ns)
        _, self.min_orig = ufboot_ref.ufboot_rule(self.state, R, ids, np.asarray(logl), rand, logl_cutoff=self.cutoff)

    def next_iteration(self):
        if self.min_orig != ufboot_ref.DBL_MAX:
            self.cutoff = self.min_orig

    def current(self, tree, score):
        def end(frm, to):
            return self.pkg.leaf_end(to) if to < tree.num_leaves else self.pkg.key_end(tree.neighbor_info(frm, to)["key"])

        a, b = tree.current_branch()
        tree.ptnlh_reserve(1)
        tree.ptnlh_put_current(0, end(a, b), end(b, a))
        self.feed(tree, [0], [score])

    def evaluate(self, tree, listed):
        moves = tree.evaluate_nnis5_batch(first_row=1, branches=listed)
        self.feed(tree, [1 + k for k in range(len(moves))], [m["newloglh"] for m in moves])
        return moves


def boot_tree(pkg, newick, data, W):
    t = attach(pkg, newick, data)
    t.set_boot_samples(W)
    return t


def test_search_with_ufboot(pkg, synth):
    true, data, start = make_data(pkg, synth, 4, 4, 9, 600, 0, 2)
    freq = data[3]
    ns = 200
    W = np.random.default_rng(7).multinomial(int(freq.sum()), freq / freq.sum(), size=ns).astype(np.float32)
    t = boot_tree(pkg, start, data, W)
    t.ufboot_init(ns, seed=11)
    ts = pkg.TreeSearch(t, seed=4, iterations=8, step_iterations=4)
    best, its = ts.search(trace=True)
    assert [it["iteration"] for it in its] == list(range(1, 10))              # the start + 8: iterations caps the rule
    assert [k for k, _ in ts.correlation_log] == [4, 8] and len(ts.boot_splits) == 4
    assert ts.correlation_log[0][1] == pkg.bootstrap_correlation(ts.boot_splits[:2], 9)
    assert ts.correlation_log[1][1] == pkg.bootstrap_correlation(ts.boot_splits, 9)
    fed = sum(1 + len(s["evaluated"]) for it in its for s in it["steps"] if s["branches"])
    assert t.ufboot_info()["trees_fed"] == fed
    # the same trees in the same order through the numpy rule
    replay = BootReplay(pkg, ns, 11)

    def make(nwk):
        return boot_tree(pkg, nwk, data, W)

    ref.replay_search(make, start, its, boot=replay)
    assert replay.next_id == fed
    got = t.ufboot_state()
    np.testing.assert_array_equal(got["boot_tree"], replay.state["boot_tree"])
    np.testing.assert_array_equal(got["boot_counts"], replay.state["boot_counts"])
    np.testing.assert_allclose(got["boot_logl"], replay.state["boot_logl"], rtol=1e-12)
    np.testing.assert_allclose(got["boot_orig_logl"], replay.state["boot_orig_logl"], rtol=1e-10)
    s = t.summarize_bootstrap()
    assert len(s["boot_trees"]) == ns
    # a minimal min_correlation and nothing to wait for (num_stop = 0): the rule ends the search at the first full step.
    # (Before that step the correlation counts as 0.0, so a literal min_correlation = 0 would end the search before its
    # first iteration -- the reference's rule reads the same.)
    t2 = boot_tree(pkg, start, data, W)
    t2.ufboot_init(ns, seed=11)
    ts2 = pkg.TreeSearch(t2, seed=4, step_iterations=4, min_correlation=1e-9, num_stop=0)
    _, its2 = ts2.search(trace=True)
    assert [k for k, _ in ts2.correlation_log] == [4] and its2[-1]["iteration"] == 4
    assert ts2.correlation_log[0][1] > 1e-9
    t3 = boot_tree(pkg, start, data, W)
    t3.ufboot_init(ns, seed=11)
    assert len(pkg.TreeSearch(t3, seed=4, step_iterations=4, min_correlation=0.0, num_stop=0).search(trace=True)[1]) == 1


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_tree_untouched(pkg, synth):
    model = synth.gtr_model(alpha=0.9, ncat=4)
    nwk, pat, freq = synth.make_workload(8, 200, model, seed=77)
    data = (4, model, pat, freq)

    def refused(t, match, **kw):
        before = t.tree_string()
        with pytest.raises(pkg.HostError, match=match):
            t.optimize_nni(**kw)
        with pytest.raises(pkg.HostError, match=match):
            pkg.TreeSearch(t, iterations=1, **kw).search()
        assert t.tree_string() == before

    multi = pkg.PhyloTree(synth.random_multifurcating_newick(8, 3, p_multi=1.0))
    multi.set_mem_mode(pkg.LM_ALL_BRANCH)
    multi.set_alignment(4, 0, pat, freq)
    multi.set_model(model)
    multi.set_likelihood_kernel(pkg.LK_EIGEN_HIP)
    multi.attach_engine(0)
    refused(multi, "multifurcating")
    refused(attach(pkg, nwk, data, mem_mode=pkg.LM_PER_NODE), "LM_ALL_BRANCH")
    three = attach(pkg, "(0:0.1,1:0.1,2:0.1);", (4, model, pat[:3], freq))
    refused(three, "at least 4 taxa")
    sh = pkg.PhyloTree(nwk)
    sh.set_mem_mode(pkg.LM_ALL_BRANCH)
    sh.set_alignment(4, 0, pat, freq)
    sh.set_model(model)
    sh.set_likelihood_kernel(pkg.LK_EIGEN_HIP)
    sh.attach_engine_sharded([0, 0], pkg.REDUCE_HOST)
    refused(sh, "sharded")
    mix = synth.mixture_model(4, 2, 5, ncat=2)
    mt = pkg.PhyloTree(nwk)
    mt.set_mem_mode(pkg.LM_ALL_BRANCH)
    mt.set_alignment(4, 0, pat, freq)
    mt.set_model(mix)
    mt.set_likelihood_kernel(pkg.LK_EIGEN_HIP)
    mt.attach_engine(0)
    lnl, *_ = mt.optimize_nni()                                               # a mixture engine may search ...
    assert abs(mt.compute_likelihood() - lnl) <= 1e-10 * abs(lnl)
    mt.set_boot_samples(np.ones((4, pat.shape[1]), dtype=np.float32))          # ... but not feed a bootstrap
    mt.ufboot_init(4)
    refused(mt, "UFBoot is not available with mixture")
    assert mt.ufboot_info()["trees_fed"] == 0
