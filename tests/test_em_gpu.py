"""GPU: the EM estimation of +R free-rate models on the device (kernels_em.hip, iqhip_em_*, PhyloTree::optimizeFreeRatesEM)
and the empirical-Bayes site rates.
  1. E-step: W, its column sums, site rates and best categories against numpy on compute_pattern_lh_cat() (rtol 1e-10, the
     tolerance test_pattern_lh_cat uses for that quantity); two calls give identical bits.
  2. objective: F_c against sum_p W[p][c] log L_p(s_c), log L_p from the probability-space textbook pruning of a one-category
     model of rate s_c (tolerance of tests/test_oracle.py for per-pattern log-likelihoods, on F_c / sum_p W[p][c]); floored
     counts 0; a deep caterpillar with scale counters at both branch ends checks the scale-counter term.
  3. EM loop against em_ref.optimize_with_em (one category at a time on the textbook pruning).
  4. refusals."""
import copy
import ctypes as C

import numpy as np
import pytest

import em_ref
from test_parity_gpu import make_case

pytestmark = pytest.mark.gpu

# (states, categories, taxa, patterns asked for, seq_type, deep).  deep = 1: the deep caterpillar of test_rell_gpu.py at its
# root branch (a leaf and 199 taxa: scaling events at the inner end).  No branch of a 200-taxon tree of 4-state data has
# scaling events at BOTH ends: a conditional likelihood of k taxa is at least about 0.25^k, the threshold is 2^-256 =
# 0.25^128, so each side needs more than 128 taxa.  deep = 2 is therefore a case of 400 taxa (the tree of
# test_rell_internal_branch_and_errors), evaluated on an inner branch where both ends carry them.
CASES = [(4, 4, 12, 300, 0, 0), (4, 4, 200, 300, 0, 1), (4, 4, 400, 200, 0, 2), (4, 10, 12, 130, 0, 0), (4, 5, 8, 64, 0, 0),
         (4, 1, 8, 70, 0, 0), (20, 4, 10, 100, 1, 0), (64, 2, 8, 50, 2, 0)]
# per-pattern log-likelihoods against the textbook: tests/test_oracle.py test_oracle_matches_textbook
TEXTBOOK_RTOL, TEXTBOOK_ATOL = 1e-9, 1e-9


def free_rates(ncat):
    """unequal +R weights and rates whose mean rate is not 1"""
    w = np.arange(ncat, 0, -1) + 0.5
    props = w / w.sum()
    rates = np.geomspace(0.1, 4.0, ncat) if ncat > 1 else np.array([0.8])
    assert abs(float(np.dot(props, rates)) - 1.0) > 0.05
    return props, rates


def with_rates(model, props, rates):
    m = copy.copy(model)
    m.props = np.ascontiguousarray(props, dtype=np.float64)
    m.rates = np.ascontiguousarray(rates, dtype=np.float64)
    m.ncat = len(m.rates)
    return m


def em_case(pkg, synth, oracle, n, ncat, ntaxa, nptn, seq_type, deep):
    """-> tree (free-rate model set, likelihood computed, current branch (a, b) chosen), oracle tree (for adj), model, pat,
    freq, (a, b).  deep = 2: an internal branch of the caterpillar whose two ends both carry scaling events."""
    kw = dict(lo=0.4 if deep == 1 else 0.5, hi=0.9, caterpillar=True) if deep else {}
    t, ot, model, pat, freq = make_case(synth, oracle, pkg, ntaxa, nptn, n, ncat, 7300 + n + ncat + ntaxa, seq_type=seq_type, **kw)
    props, rates = free_rates(ncat)
    model = with_rates(model, props, rates)
    t.set_model(model)
    t.clear_all_partial_lh()
    t.compute_likelihood()
    a, b = t.current_branch()
    if deep == 1:
        inner_end = (a, b) if not ot.is_leaf(b) else (b, a)
        assert t.fetch_scale_num(*inner_end).max() >= 1
    if deep == 2:
        inner = [(x, y) for x in range(t.num_nodes) for y, _ in t.neighbors(x) if x < y and not ot.is_leaf(x) and not ot.is_leaf(y)]
        found = None
        for x, y in inner[len(inner) // 2:] + inner[:len(inner) // 2]:
            t.compute_likelihood_derv(x, y)              # makes (x, y) the current branch, both vectors computed
            if t.fetch_scale_num(x, y).max() >= 1 and t.fetch_scale_num(y, x).max() >= 1:
                found = (x, y)
                break
        assert found, "no internal branch with scaling events at both ends"
        a, b = found
    return t, ot, model, pat, freq, (a, b)


@pytest.fixture(scope="module", params=CASES, ids=lambda c: "n%d_c%d_t%d_p%d" % c[:4])
def case(request, pkg, synth, oracle):
    n, ncat, ntaxa, nptn, seq_type, deep = request.param
    t, ot, model, pat, freq, (a, b) = em_case(pkg, synth, oracle, n, ncat, ntaxa, nptn, seq_type, deep)
    t.compute_likelihood_derv(a, b)                       # current branch = (a, b)
    cat = t.compute_pattern_lh_cat()
    W, cat_sum = t.em_posteriors()
    return dict(t=t, ot=ot, model=model, pat=pat, freq=np.asarray(freq, dtype=np.float64), a=a, b=b, cat=cat, W=W,
                cat_sum=cat_sum, n=n, ncat=ncat, seq_type=seq_type, deep=deep, su=oracle.state_unknown_for(n, seq_type))


def test_e_step(case):
    t, cat, W, cat_sum, freq, ncat = case["t"], case["cat"], case["W"], case["cat_sum"], case["freq"], case["ncat"]
    assert W.shape == (t.nptn, ncat) and t.nptn > 0
    expect = freq[:, None] * cat / cat.sum(axis=1, keepdims=True)
    np.testing.assert_allclose(W, expect, rtol=1e-10, atol=0)
    np.testing.assert_allclose(cat_sum, expect.sum(axis=0), rtol=1e-10, atol=0)
    np.testing.assert_allclose(cat_sum, W.sum(axis=0), rtol=1e-10, atol=0)
    if ncat == 1:
        np.testing.assert_allclose(W[:, 0], freq, rtol=1e-15, atol=0)   # the degenerate case: W is ptn_freq
    else:
        assert np.all((cat == cat.max(axis=1, keepdims=True)).sum(axis=1) == 1)   # no exact ties in this case
    ref_rate, ref_cat = em_ref.pattern_rates(cat, case["model"].rates)
    rate, best = t.site_rates()
    np.testing.assert_allclose(rate, ref_rate, rtol=1e-10, atol=0)
    assert np.array_equal(best, ref_cat)
    # identical bits on a second call (site_rates() above ran one more E-step as well)
    W2, cat_sum2 = t.em_posteriors()
    assert np.array_equal(W2, W) and np.array_equal(cat_sum2, cat_sum)
    rate2, best2 = t.site_rates()
    assert np.array_equal(rate2, rate) and np.array_equal(best2, best)


def test_objective(case):
    import textbook
    t, ot, model, W, a, b = case["t"], case["ot"], case["model"], case["W"], case["a"], case["b"]
    if case["deep"] == 2:
        assert t.fetch_scale_num(a, b).max() >= 1 and t.fetch_scale_num(b, a).max() >= 1
    col = W.sum(axis=0)
    for factor in (1.0, 0.5, 2.0):
        rates = model.rates * factor
        if factor != 1.0:
            t.set_model(with_rates(model, model.props, rates))
            t.clear_all_partial_lh()
            t.compute_likelihood()
        F, floored = t.em_objective(a, b)
        F_again, _ = t.em_objective(a, b)
        assert np.array_equal(F, F_again)
        assert np.all(floored == 0), floored
        for c in range(case["ncat"]):
            one = with_rates(model, [1.0], [rates[c]])
            logl = textbook.site_log_likelihoods(ot.adj, case["pat"], one, case["seq_type"], case["su"])
            ref = float(np.dot(W[:, c], logl))
            print("objective x%.1f cat %d: F/S %.12f ref/S %.12f diff %.3e" % (factor, c, F[c] / col[c], ref / col[c],
                                                                                 abs(F[c] - ref) / col[c]))
            assert abs(F[c] / col[c] - ref / col[c]) <= TEXTBOOK_ATOL + TEXTBOOK_RTOL * abs(ref / col[c]), (factor, c)
    t.set_model(model)                                    # leave the case as the other tests expect it
    t.clear_all_partial_lh()
    t.compute_likelihood()
    t.compute_likelihood_derv(a, b)


# The device EM against the numpy EM of em_ref, both run on an MI355X box: largest relative
# difference of the rates 1.347e-12, of the weights 2.252e-13, lnL difference 7.276e-12, the same number of Brent evaluations
# in every search.  The bounds are ten times those (the ceiling for rates and weights is 5e-3, five Brent tolerances: two
# correct runs may part ways on near-equal function values, and these two did not).
EM_RATE_RTOL, EM_PROP_RTOL, EM_LNL_ATOL = 1.4e-11, 2.3e-12, 7.3e-11


@pytest.fixture(scope="module")
def em_run(pkg, synth, oracle):
    import textbook
    true = with_rates(synth.gtr_model(alpha=0.9, ncat=3), [0.5, 0.35, 0.15], [0.15, 1.0, 3.8333333333333335])
    nwk = synth.random_tree_newick(12, 4711, 0.05, 0.3)
    st = synth.simulate_alignment(nwk, true, 1500, 4712)
    pat, freq = synth.compress_patterns(st)
    p0, r0 = pkg.free_rate_start(3)
    start = with_rates(true, p0, r0)
    ot = oracle.OracleTree(nwk, 4, 0, pat, freq, None, start)
    t = pkg.PhyloTree(nwk)
    t.set_alignment(4, 0, pat, freq)
    t.set_model(start)
    t.set_likelihood_kernel(pkg.LK_EIGEN_HIP)
    t.attach_engine(0)
    runs = []
    for _ in range(2):
        t.set_model(start)
        t.clear_all_partial_lh()
        lnl0 = t.compute_likelihood()
        runs.append(t.optimize_free_rates_em(trace=True))
    cache = {}

    def log_lh(s):
        if s not in cache:
            cache[s] = textbook.site_log_likelihoods(ot.adj, pat, with_rates(true, [1.0], [s]), 0, 18)
        return cache[s]

    ref = em_ref.optimize_with_em(log_lh, freq, p0, r0)
    return dict(runs=runs, ref=ref, lnl0=lnl0, true=true)


def test_em_loop_invariants(em_run):
    res = em_run["runs"][0]
    tr = res["trace"]
    assert res["steps"] == len(tr) and 1 <= len(tr) <= 3
    lnls = [s["lnl_before"] for s in tr] + [res["lnl"]]
    assert abs(lnls[0] - em_run["lnl0"]) <= 1e-9 * abs(lnls[0])
    for k in range(1, len(lnls)):
        assert lnls[k] >= lnls[k - 1] - 1e-6, lnls           # the likelihood never decreases
    assert lnls[-1] > lnls[0] + 1.0                          # ... and the start was far from the estimate
    assert np.all(res["props"] >= 1e-4) and abs(res["props"].sum() - 1.0) <= 1e-4
    for s in tr:
        assert s["rounds"] == int(max(s["evals"]))          # the lockstep claim: traversals = the longest search
        assert np.all(s["floored"] == 0)
    assert sum(int(s["evals"].sum()) for s in tr) > sum(s["rounds"] for s in tr)


def test_em_loop_matches_the_sequential_reference(em_run):
    res, ref = em_run["runs"][0], em_run["ref"]
    d_rate = np.max(np.abs(res["rates"] - ref["rates"]) / ref["rates"])
    d_prop = np.max(np.abs(res["props"] - ref["props"]) / ref["props"])
    d_lnl = abs(res["lnl"] - ref["lnl"])
    print("EM device vs numpy: rates", res["rates"], ref["rates"], "props", res["props"], ref["props"])
    print("EM device vs numpy: max rel rates %.3e, max rel props %.3e, lnL %.12f vs %.12f (diff %.3e), steps %d vs %d"
          % (d_rate, d_prop, res["lnl"], ref["lnl"], d_lnl, res["steps"], ref["steps"]))
    print("EM evals per step: device", [list(s["evals"]) for s in res["trace"]], "numpy", [s["evals"] for s in ref["trace"]])
    assert EM_RATE_RTOL <= 5e-3 and EM_PROP_RTOL <= 5e-3
    assert d_rate <= EM_RATE_RTOL and d_prop <= EM_PROP_RTOL and d_lnl <= EM_LNL_ATOL


def test_em_loop_is_reproducible(em_run):
    r1, r2 = em_run["runs"]
    assert np.array_equal(r1["props"], r2["props"]) and np.array_equal(r1["rates"], r2["rates"]) and r1["lnl"] == r2["lnl"]
    assert [s["lnl_before"] for s in r1["trace"]] == [s["lnl_before"] for s in r2["trace"]]


def test_em_single_category(pkg, synth, oracle):
    """one category: W is ptn_freq, the EM returns weight 1 and the tree-length scaling as the rate"""
    t, ot, model, pat, freq, (a, b) = em_case(pkg, synth, oracle, 4, 1, 8, 70, 0, 0)
    lnl0 = t.compute_likelihood()
    res = t.optimize_free_rates_em(trace=True)
    assert abs(res["props"][0] - 1.0) <= 1e-12 and res["lnl"] >= lnl0 - 1e-6
    assert all(s["rounds"] == int(s["evals"][0]) for s in res["trace"])


def test_refusals(pkg, synth, oracle):
    lib = pkg.libiqhip()
    dp = C.POINTER(C.c_double)
    buf = np.zeros(4096)
    d = buf.ctypes.data_as(dp)
    end = pkg.leaf_end(0)
    cats = np.zeros(4096, dtype=np.int32).ctypes.data_as(C.POINTER(C.c_int32))
    # a plain engine: theta not resident, then no E-step yet
    t, ot, model, pat, freq = make_case(synth, oracle, pkg, 8, 100, 4, 4, 99)
    t.compute_likelihood()
    assert lib.iqhip_em_posteriors(t.engine, 0.1, d) == pkg.ERR_INVALID and b"compute_theta" in lib.iqhip_last_error()
    a, b = t.current_branch()
    t.compute_likelihood_derv(a, b)                       # theta resident
    assert lib.iqhip_em_objective(t.engine, end, end, 0.1, d, None) == pkg.ERR_INVALID
    assert b"iqhip_em_posteriors first" in lib.iqhip_last_error()
    assert lib.iqhip_em_fetch_posteriors(t.engine, d) == pkg.ERR_INVALID
    assert lib.iqhip_em_site_rates(t.engine, d, cats) == pkg.ERR_INVALID
    assert lib.iqhip_em_posteriors(t.engine, -1.0, d) == pkg.ERR_INVALID
    assert lib.iqhip_em_posteriors(t.engine, float("nan"), d) == pkg.ERR_INVALID
    assert lib.iqhip_em_posteriors(t.engine, 0.1, d) == 0, lib.iqhip_last_error()
    assert lib.iqhip_em_fetch_posteriors(t.engine, d) == 0
    # a weight of zero: the objective divides by it
    zero = with_rates(model, [0.5, 0.5, 0.0, 0.0], model.rates)
    t.set_model(zero)
    t.clear_all_partial_lh()
    t.compute_likelihood()
    t.compute_likelihood_derv(a, b)
    with pytest.raises(pkg.HostError, match="weight"):
        t.em_objective(a, b)
    # a new model drops theta
    t.set_model(model)
    t.clear_all_partial_lh()
    t.compute_likelihood()
    assert lib.iqhip_em_objective(t.engine, end, end, 0.1, d, None) == pkg.ERR_INVALID and b"compute_theta" in lib.iqhip_last_error()
    # mixture
    mix = synth.mixture_model(4, 2, 5, ncat=2)
    tm, _, _, _, _ = make_case(synth, oracle, pkg, 8, 100, 4, 4, 98)
    tm.set_model(mix)
    tm.clear_all_partial_lh()
    tm.compute_likelihood()
    am, bm = tm.current_branch()
    tm.compute_likelihood_derv(am, bm)
    assert lib.iqhip_em_posteriors(tm.engine, 0.1, d) == pkg.ERR_UNSUPPORTED and b"mixture" in lib.iqhip_last_error()
    assert lib.iqhip_em_objective(tm.engine, end, end, 0.1, d, None) == pkg.ERR_UNSUPPORTED
    with pytest.raises(pkg.HostError, match="mixture"):
        tm.optimize_free_rates_em()
    # +ASC
    nwk = synth.random_tree_newick(9, 5)
    st = synth.simulate_alignment(nwk, model, 300, 6)
    st = st[:, [s for s in range(st.shape[1]) if len(set(st[:, s].tolist())) > 1]]
    p2, f2 = synth.compress_patterns(st)
    nsite = int(f2.sum())
    p2 = np.concatenate([p2, np.tile(np.arange(4, dtype=np.uint8), (9, 1))], axis=1)
    f2 = np.concatenate([f2, np.zeros(4)])
    ta = pkg.PhyloTree(nwk)
    ta.set_alignment(4, 0, p2, f2)
    ta.set_ascertainment(4, nsite)
    ta.set_model(model)
    ta.attach_engine(0)
    ta.compute_likelihood()
    aa, ba = ta.current_branch()
    ta.compute_likelihood_derv(aa, ba)
    assert lib.iqhip_em_posteriors(ta.engine, 0.1, d) == pkg.ERR_UNSUPPORTED and b"ascertainment" in lib.iqhip_last_error()
    assert lib.iqhip_em_site_rates(ta.engine, d, cats) == pkg.ERR_UNSUPPORTED
    with pytest.raises(pkg.HostError, match="ASC"):
        ta.optimize_free_rates_em()
    # sharded: two shards on one device
    ts = pkg.PhyloTree(nwk)
    ts.set_alignment(4, 0, p2[:, :-4], f2[:-4])
    ts.set_model(model)
    ts.set_likelihood_kernel(pkg.LK_EIGEN_HIP)
    ts.attach_engine_sharded([0, 0], pkg.REDUCE_HOST)
    ts.compute_likelihood()
    assert lib.iqhip_em_posteriors(ts.engine, 0.1, d) == pkg.ERR_UNSUPPORTED and b"sharded" in lib.iqhip_last_error()
    assert lib.iqhip_em_objective(ts.engine, end, end, 0.1, d, None) == pkg.ERR_UNSUPPORTED
    assert lib.iqhip_em_fetch_posteriors(ts.engine, d) == pkg.ERR_UNSUPPORTED
    # embedded state count: 3 states on the 4-state kernels
    m3 = synth.random_reversible_model(3, 17, alpha=0.9, ncat=2)
    st3 = synth.simulate_alignment(nwk, m3, 120, 8)
    p3, f3 = synth.compress_patterns(st3)
    t3 = pkg.PhyloTree(nwk)
    t3.set_alignment(3, 3, p3, f3)
    t3.set_model(m3)
    t3.set_likelihood_kernel(pkg.LK_EIGEN_HIP)
    t3.attach_engine(0)
    t3.compute_likelihood()
    a3, b3 = t3.current_branch()
    t3.compute_likelihood_derv(a3, b3)
    assert lib.iqhip_em_posteriors(t3.engine, 0.1, d) == pkg.ERR_UNSUPPORTED and b"embedded" in lib.iqhip_last_error()
    assert lib.iqhip_em_objective(t3.engine, end, end, 0.1, d, None) == pkg.ERR_UNSUPPORTED
