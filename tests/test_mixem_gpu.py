"""GPU: the EM estimation of mixture class weights on the device (kernels_mixem.hip, iqhip_mix_*,
PhyloTree::optimizeMixtureWeights), the class posteriors and the pattern state frequencies.
  1. mix_class_lh() against compute_pattern_lh_cat() summed per class (rtol 1e-10, the tolerance test_em_gpu.py uses for
     that quantity).
  2. mix_weights_em(max_steps = nclass) against mixem_ref.optimize_weights on the fetched device matrix: weights, p_invar,
     step count and trace at rtol 1e-10 (every sum has positive terms only: the error is about steps * (nptn + nclass) * 2^-53,
     1e-11 at these sizes); one step against the restatement on the textbook per-class likelihoods at rtol 1e-8, ten times the
     project's textbook tolerance; both again with p_invar = 0.2 on alignments with constant patterns.
  3. the weights moved by more than 1e-3.
  4. the convergence path: max_steps = 200, converged, the restatement's step count, and the same bits with max_steps = 400.
  5. posteriors and pattern state frequencies against mixem_ref (rtol 1e-10); rows of the posteriors sum to 1.
  6. two calls of every function give identical bits.
  7. optimize_mixture_weights(): its lnL is that of a fresh evaluation with the new weights, not below the one before, and
     the oracle's for the same weights.
  8. the EM chain reports 2 * max_steps launches plus a constant.  The figure is the host's own count of what it enqueued, so it
     shows that the loop's length does not depend on what the device finds, not that no read happens inside; that is read off
     the code (iqhip_mix_weights_em: one upload, the loop of launches, one read).
  9. the refusals.
Two cases carry patterns of frequency 0 (every fifth): they contribute nothing, to the sums or to the site count.
The alignments hold an equal share of sites from every class, so the simulated weights (Dirichlet) are not the estimate.  The
96-class case has one site per class (96 sites, not 60: a share cannot be less than one site)."""
import copy
import ctypes as C

import numpy as np
import pytest

import mixem_ref
from test_mixem_host import class_weights, mix_alignment, mix_ptn_invar, textbook_class_lh

pytestmark = pytest.mark.gpu

# name: (states, seq_type, classes, rates, taxa, sites, p_invar, constant columns, tree keywords, permuted cat_class)
CASES = {
    "n4_2x1": (4, 0, 2, 1, 8, 64, 0.0, 0, {}, False),                    # the fewest components
    "n4_3x4": (4, 0, 3, 4, 12, 300, 0.0, 0, {}, False),                  # wide DNA: 12 components on 16-pattern tiles
    "n20_3x2": (20, 1, 3, 2, 9, 150, 0.0, 0, {}, False),                 # matrix-core theta layout
    "n20_10x4": (20, 1, 10, 4, 8, 300, 0.0, 0, {}, False),               # more classes than stay in registers
    "n20_96x1": (20, 1, 96, 1, 8, 96, 0.0, 0, {}, False),                # the class limit
    "n64_2x2": (64, 2, 2, 2, 8, 50, 0.0, 0, {}, False),                  # 64-state layout
    # the caterpillar of test_hip_mixture_matches_oracle: scaling events at the branch
    "n20_2x3_deep": (20, 1, 2, 3, 150, 300, 0.0, 0, dict(lo=0.4, hi=0.9, caterpillar=True), False),
    # more than two step-workgroups' share of patterns (256 each; 1024 would hold as well) and not a multiple of it
    "n4_3x1_long": (4, 0, 3, 1, 20, 4000, 0.0, 0, dict(lo=0.1, hi=0.4), False),
    "n4_3x4_perm": (4, 0, 3, 4, 12, 300, 0.0, 0, {}, True),              # a permuted, non-contiguous cat_class
    "n4_3x4_inv": (4, 0, 3, 4, 12, 300, 0.2, 16, {}, False),             # +I
    "n20_3x2_inv": (20, 1, 3, 2, 9, 150, 0.2, 40, {}, False),
    "n4_3x4_zero": (4, 0, 3, 4, 12, 300, 0.0, 0, {}, False),             # patterns of frequency 0, classes in registers
    "n20_10x4_zero": (20, 1, 10, 4, 8, 300, 0.0, 0, {}, False),          # ... classes read twice
}
CONVERGENCE_CASES = ("n4_2x1", "n20_3x2")
SEED = 4100


def scaled_props(model, factor, perm=None):
    """a copy of the mixture with every component weight times factor and, with perm, its components reordered"""
    m = copy.copy(model)
    m.props = model.props * factor
    m.classes = []
    for c in model.classes:
        cc = copy.copy(c)
        cc.props = c.props * factor
        m.classes.append(cc)
    if perm is not None:
        m.rates, m.props, m.cat_class = m.rates[perm].copy(), m.props[perm].copy(), m.cat_class[perm].copy()
    return m


def build_case(synth, oracle, name):
    n, seq_type, nclass, ncat, ntaxa, nsites, p_invar, nconst, kw, permuted = CASES[name]
    model, nwk, pat, freq, su = mix_alignment(synth, oracle, n, nclass, ncat, ntaxa, nsites, SEED + n + nclass + ntaxa, seq_type,
                                              const_sites=nconst, **kw)
    freq = np.asarray(freq, dtype=np.float64).copy()
    if name.endswith("_zero"):
        freq[1::5] = 0.0
        assert np.count_nonzero(freq == 0.0) >= 10
    perm = None
    if permuted:
        perm = np.random.default_rng(5).permutation(model.ncat)
        assert np.any(np.diff(model.cat_class[perm]) < 0)
    invar = mix_ptn_invar(pat, model, p_invar) if p_invar else None
    model = scaled_props(model, 1.0 - p_invar, perm)
    return dict(name=name, n=n, seq_type=seq_type, nclass=nclass, ncat=ncat, model=model, nwk=nwk, pat=pat,
                freq=np.asarray(freq, dtype=np.float64), su=su, invar=invar, p_invar=p_invar or None, w0=class_weights(model))


_built = {}


@pytest.fixture(scope="module")
def cases(pkg, synth, oracle):
    """name -> the case with its tree on the device, the class likelihoods, the EM run of nclass steps and the restatement's
    run on the fetched matrix; built once, shared by the tests and left unchanged"""
    def get(name):
        if name not in _built:
            c = build_case(synth, oracle, name)
            t = pkg.PhyloTree(c["nwk"])
            t.set_alignment(c["n"], c["seq_type"], c["pat"], c["freq"], c["invar"])
            t.set_model(c["model"])
            t.set_likelihood_kernel(pkg.LK_EIGEN_HIP)
            t.attach_engine(0)
            c["lnl0"] = t.compute_likelihood()
            c["cat"] = t.compute_pattern_lh_cat()
            c["Lc"] = t.mix_class_lh()
            c["t"] = t
            c["em"] = t.mix_weights_em(c["w0"], p_invar=c["p_invar"], trace=True)
            c["ref"] = mixem_ref.optimize_weights(c["Lc"], c["freq"], c["invar"], c["w0"], p_invar=c["p_invar"],
                                                  max_steps=c["nclass"])
            _built[name] = c
        return _built[name]
    yield get
    _built.clear()


ALL = sorted(CASES)
NO_INVAR = [k for k in ALL if not CASES[k][6]]
INVAR = [k for k in ALL if CASES[k][6]]


@pytest.fixture
def case(request, cases):
    return cases(request.param)


def per_case(names):
    return pytest.mark.parametrize("case", names, indirect=True)


@per_case(ALL)
def test_class_lh(case):
    t, Lc, cat, model = case["t"], case["Lc"], case["cat"], case["model"]
    assert Lc.shape == (t.nptn, case["nclass"]) and cat.shape == (t.nptn, model.ncat)
    if case["name"] == "n4_3x1_long":
        assert t.nptn > 2 * 1024 and t.nptn % 1024 != 0 and t.nptn % 256 != 0
    expect = np.zeros_like(Lc)
    for m in range(case["nclass"]):
        comps = np.nonzero(model.cat_class == m)[0]
        assert len(comps) == case["ncat"]
        for q in comps:                                      # ascending q
            expect[:, m] = cat[:, q] if q == comps[0] else expect[:, m] + cat[:, q]
    assert np.all(expect > 0.0)
    np.testing.assert_allclose(Lc, expect, rtol=1e-10, atol=0)
    assert np.array_equal(t.mix_class_lh(), Lc)              # identical bits on a second call


@per_case(ALL)
def test_em_matches_the_restatement_on_the_device_matrix(case):
    em, ref, nclass = case["em"], case["ref"], case["nclass"]
    print("%s: steps %d / %d, converged %d / %d, per-step change %s" % (case["name"], em["steps"], ref["steps"], em["converged"],
                                                                      ref["converged"], ref["last_change"]))
    print("weights device", em["weights"], "restatement", ref["prop"], "p_invar", em["p_invar"], ref["p_invar"])
    assert em["steps"] == ref["steps"] and em["converged"] == ref["converged"]
    np.testing.assert_allclose(em["weights"], ref["prop"], rtol=1e-10, atol=0)
    np.testing.assert_allclose(em["trace"], ref["trace"], rtol=1e-10, atol=0)
    if case["p_invar"]:
        assert abs(em["p_invar"] - ref["p_invar"]) <= 1e-10 * ref["p_invar"] and em["p_invar"] != case["p_invar"]
        assert np.count_nonzero(case["invar"]) >= 4
    else:
        assert em["p_invar"] is None and np.all(em["trace"][:, nclass] == 0.0)
    assert np.array_equal(em["trace"][-1, :nclass], em["weights"])
    total = em["weights"].sum() + (em["p_invar"] or 0.0)
    assert abs(total - 1.0) <= 1e-10
    # 3. the weights moved
    moved = np.max(np.abs(ref["prop"] - case["w0"]))
    print("moved by", moved)
    assert moved > 1e-3
    # 6. identical bits on a second run
    again = case["t"].mix_weights_em(case["w0"], p_invar=case["p_invar"], trace=True)
    assert np.array_equal(again["weights"], em["weights"]) and np.array_equal(again["trace"], em["trace"])
    assert again["steps"] == em["steps"] and again["p_invar"] == em["p_invar"]


@per_case(ALL)
def test_one_step_matches_the_textbook(case, oracle):
    c = case
    ot = oracle.OracleTree(c["nwk"], c["n"], c["seq_type"], c["pat"], c["freq"], c["invar"], c["model"])
    L, mx = textbook_class_lh(ot.adj, c["pat"], c["model"], c["seq_type"], c["su"])
    invar = c["invar"] * np.exp(-mx) if c["p_invar"] else None
    ref = mixem_ref.optimize_weights(L, c["freq"], invar, c["w0"], p_invar=c["p_invar"], max_steps=1)
    one = c["t"].mix_weights_em(c["w0"], max_steps=1, p_invar=c["p_invar"], trace=True)
    print("%s one step: device %s textbook %s, max rel %.3e" % (c["name"], one["weights"], ref["prop"],
                                                               np.max(np.abs(one["weights"] - ref["prop"]) / ref["prop"])))
    assert one["steps"] == 1 and one["trace"].shape == (1, c["nclass"] + 1)
    np.testing.assert_allclose(one["weights"], ref["prop"], rtol=1e-8, atol=0)
    if c["p_invar"]:
        assert abs(one["p_invar"] - ref["p_invar"]) <= 1e-8 * ref["p_invar"]
    np.testing.assert_allclose(one["weights"], c["em"]["trace"][0, :c["nclass"]], rtol=0, atol=0)   # the first step of the long run


@per_case(list(CONVERGENCE_CASES))
def test_convergence_path(case):
    c, t = case, case["t"]
    ref = mixem_ref.optimize_weights(c["Lc"], c["freq"], c["invar"], c["w0"], max_steps=200)
    last = ref["last_change"]
    print("%s: restatement converged in %d steps, last changes %s" % (c["name"], ref["steps"], last[-2:]))
    assert ref["converged"] == 1 and 3 <= ref["steps"] < 200
    for d in last[-2:]:                                      # precondition: no step sits on the threshold
        assert not (1e-4 * (1 - 1e-6) <= d <= 1e-4 * (1 + 1e-6))
    em = t.mix_weights_em(c["w0"], max_steps=200, trace=True)
    assert em["converged"] == 1 and em["steps"] == ref["steps"]
    np.testing.assert_allclose(em["weights"], ref["prop"], rtol=1e-10, atol=0)
    np.testing.assert_allclose(em["trace"], ref["trace"], rtol=1e-10, atol=0)
    more = t.mix_weights_em(c["w0"], max_steps=400, trace=True)   # the steps behind the converged one are no-ops
    assert more["steps"] == em["steps"] and more["converged"] == 1
    assert np.array_equal(more["weights"], em["weights"]) and np.array_equal(more["trace"], em["trace"])


@per_case(ALL)
def test_posteriors_and_state_freq(case):
    t, Lc, model = case["t"], case["Lc"], case["model"]
    cf = np.stack([c.freqs for c in model.classes])
    post = t.mix_posteriors()
    post2, sf = t.mix_posteriors(cf)
    assert np.array_equal(post, post2)
    np.testing.assert_allclose(post, mixem_ref.posteriors(Lc), rtol=1e-10, atol=0)
    np.testing.assert_allclose(post.sum(axis=1), 1.0, rtol=0, atol=1e-13)
    np.testing.assert_allclose(sf, mixem_ref.pattern_state_freq(Lc, cf), rtol=1e-10, atol=0)
    np.testing.assert_allclose(sf.sum(axis=1), 1.0, rtol=0, atol=1e-12)
    post3, sf3 = t.mix_posteriors(cf)
    assert np.array_equal(post3, post) and np.array_equal(sf3, sf)
    # PhyloTree::computePatternStateFreq of the host mirror: class likelihoods rebuilt, then the same kernel
    assert np.array_equal(t.pattern_state_freq(cf), sf)


@per_case(["n4_3x4_inv", "n20_10x4"])
def test_chain_launches(case):
    """the chain's length is 2 launches per step whatever the device finds, plus a constant (the host's own count: see the
    module docstring for what this does and does not show)"""
    t = case["t"]
    extra = set()
    for steps in (1, 5, 200):
        t.mix_weights_em(case["w0"], max_steps=steps, p_invar=case["p_invar"])
        extra.add(t.mix_timing()["launches"] - 2 * steps)
    assert len(extra) == 1 and 0 <= extra.pop() <= 4


@per_case(NO_INVAR)
def test_optimize_mixture_weights(case, oracle):
    c, t, model = case, case["t"], case["model"]
    from test_parity_gpu import LNL_RTOL
    res = t.optimize_mixture_weights()
    print("%s: lnL %.9f -> %.9f in %d steps, weights %s" % (c["name"], c["lnl0"], res["lnl"], res["steps"], res["weights"]))
    np.testing.assert_allclose(res["weights"], c["em"]["weights"], rtol=1e-12, atol=0)
    assert res["steps"] == c["em"]["steps"]
    np.testing.assert_allclose(res["props"], model.props * (res["weights"] / c["w0"])[model.cat_class], rtol=1e-14, atol=0)
    assert res["lnl"] > c["lnl0"]                            # the weights moved by more than 1e-3: the gain is far above rounding
    new_model = copy.copy(model)
    new_model.props = res["props"].copy()
    t.set_model(new_model)
    t.clear_all_partial_lh()
    assert t.compute_likelihood() == res["lnl"]
    ot = oracle.OracleTree(c["nwk"], c["n"], c["seq_type"], c["pat"], c["freq"], None, new_model)
    ref, _ = ot.likelihood()
    assert abs(res["lnl"] - ref) <= LNL_RTOL * abs(ref)
    # the matrix of the old model is gone
    with pytest.raises(RuntimeError, match="iqhip_mix_class_lh first"):
        t.mix_posteriors()
    t.set_model(model)                                       # leave the case as the other tests expect it
    t.clear_all_partial_lh()
    assert t.compute_likelihood() == c["lnl0"]
    assert np.array_equal(t.mix_class_lh(), c["Lc"])


@per_case(INVAR)
def test_optimize_mixture_weights_with_invar(case, oracle):
    """the +I branch of optimizeMixtureWeights: ptn_invar follows the new p_invar and is sent again"""
    c, t, model = case, case["t"], case["model"]
    from test_parity_gpu import LNL_RTOL
    p_old = c["p_invar"]
    res = t.optimize_mixture_weights(p_invar=p_old)
    print("%s: lnL %.9f -> %.9f, p_invar %.6f -> %.6f, weights %s" % (c["name"], c["lnl0"], res["lnl"], p_old, res["p_invar"],
                                                                    res["weights"]))
    np.testing.assert_allclose(res["weights"], c["em"]["weights"], rtol=1e-12, atol=0)
    assert res["steps"] == c["em"]["steps"] and abs(res["p_invar"] - c["em"]["p_invar"]) <= 1e-12 and res["p_invar"] != p_old
    np.testing.assert_allclose(res["props"], model.props * (res["weights"] / c["w0"])[model.cat_class], rtol=1e-14, atol=0)
    assert abs(res["props"].sum() + res["p_invar"] - 1.0) <= 1e-10
    assert res["lnl"] > c["lnl0"]
    new_model = copy.copy(model)
    new_model.props = res["props"].copy()
    new_invar = c["invar"] * (res["p_invar"] / p_old)
    t.set_model(new_model)
    t.set_ptn_invar(new_invar)
    t.clear_all_partial_lh()
    assert t.compute_likelihood() == res["lnl"]
    ot = oracle.OracleTree(c["nwk"], c["n"], c["seq_type"], c["pat"], c["freq"], new_invar, new_model)
    ref, _ = ot.likelihood()
    assert abs(res["lnl"] - ref) <= LNL_RTOL * abs(ref)
    t.set_model(model)                                       # leave the case as the other tests expect it
    t.set_ptn_invar(c["invar"])
    t.clear_all_partial_lh()
    assert t.compute_likelihood() == c["lnl0"]
    assert np.array_equal(t.mix_class_lh(), c["Lc"])


def test_refusals(pkg, synth, oracle):
    from test_parity_gpu import make_case
    lib = pkg.libiqhip()
    dp = C.POINTER(C.c_double)
    d = np.zeros(1 << 16).ctypes.data_as(dp)
    n, conv = C.c_int(), C.c_int()

    def em(engine, max_steps=2, nsites=100.0, w=(0.5, 0.5), pinv=None):
        wa = np.array(w, dtype=np.float64)
        p = C.c_double(pinv if pinv is not None else 0.0)
        return lib.iqhip_mix_weights_em(engine, max_steps, nsites, wa.ctypes.data_as(dp), C.byref(p) if pinv is not None else None,
                                        C.byref(n), C.byref(conv), None)

    # a mixture engine: theta not resident, bad lengths, no class likelihoods yet
    c = build_case(synth, oracle, "n4_2x1")
    t = pkg.PhyloTree(c["nwk"])
    t.set_alignment(4, 0, c["pat"], c["freq"])
    t.set_model(c["model"])
    t.set_likelihood_kernel(pkg.LK_EIGEN_HIP)
    t.attach_engine(0)
    t.compute_likelihood()
    assert lib.iqhip_mix_class_lh(t.engine, 0.1, d) == pkg.ERR_INVALID and b"compute_theta" in lib.iqhip_last_error()
    assert em(t.engine) == pkg.ERR_INVALID and b"iqhip_mix_class_lh first" in lib.iqhip_last_error()
    assert lib.iqhip_mix_posteriors(t.engine, None, d, None) == pkg.ERR_INVALID and b"iqhip_mix_class_lh first" in lib.iqhip_last_error()
    a, b = t.current_branch()
    t.compute_likelihood_derv(a, b)                          # theta resident
    assert lib.iqhip_mix_class_lh(t.engine, -1.0, d) == pkg.ERR_INVALID
    assert lib.iqhip_mix_class_lh(t.engine, float("nan"), d) == pkg.ERR_INVALID
    assert em(t.engine) == pkg.ERR_INVALID                   # still no class likelihoods
    assert lib.iqhip_mix_class_lh(t.engine, 0.1, None) == 0, lib.iqhip_last_error()   # device only
    assert em(t.engine) == 0, lib.iqhip_last_error()
    assert lib.iqhip_mix_posteriors(t.engine, None, d, None) == 0
    assert lib.iqhip_mix_posteriors(t.engine, None, None, d) == pkg.ERR_INVALID      # state frequencies without class_freq
    assert em(t.engine, max_steps=0) == pkg.ERR_INVALID and b"max_steps" in lib.iqhip_last_error()
    assert em(t.engine, max_steps=4097) == pkg.ERR_INVALID and b"4096" in lib.iqhip_last_error()   # IQHIP_MIX_MAX_STEPS
    assert em(t.engine, nsites=0.0) == pkg.ERR_INVALID and b"nsites" in lib.iqhip_last_error()
    assert em(t.engine, nsites=float("nan")) == pkg.ERR_INVALID
    assert em(t.engine, w=(1.0, 0.0)) == pkg.ERR_INVALID and b"weight" in lib.iqhip_last_error()
    assert em(t.engine, w=(0.5, -0.5)) == pkg.ERR_INVALID
    assert em(t.engine, w=(0.5, float("inf"))) == pkg.ERR_INVALID
    assert em(t.engine, w=(0.5, float("nan"))) == pkg.ERR_INVALID
    assert em(t.engine, pinv=1.0) == pkg.ERR_INVALID and b"p_invar" in lib.iqhip_last_error()
    assert em(t.engine, pinv=-0.1) == pkg.ERR_INVALID
    assert em(t.engine, pinv=float("nan")) == pkg.ERR_INVALID
    assert em(t.engine, pinv=0.0) == 0                       # 0: no +I handling
    # a model change drops the matrix (and theta)
    t.set_model(c["model"])
    t.clear_all_partial_lh()
    t.compute_likelihood()
    t.compute_likelihood_derv(a, b)
    assert em(t.engine) == pkg.ERR_INVALID and b"iqhip_mix_class_lh first" in lib.iqhip_last_error()
    assert lib.iqhip_mix_posteriors(t.engine, None, d, None) == pkg.ERR_INVALID
    with pytest.raises(pkg.HostError, match="iqhip_mix_class_lh first"):
        t.mix_weights_em([0.5, 0.5])
    # one class
    tp, _, model, _, _ = make_case(synth, oracle, pkg, 8, 100, 4, 4, 97)
    tp.compute_likelihood()
    ap, bp = tp.current_branch()
    tp.compute_likelihood_derv(ap, bp)
    assert lib.iqhip_mix_class_lh(tp.engine, 0.1, d) == pkg.ERR_UNSUPPORTED and b"one class" in lib.iqhip_last_error()
    assert em(tp.engine) == pkg.ERR_UNSUPPORTED
    assert lib.iqhip_mix_posteriors(tp.engine, None, d, None) == pkg.ERR_UNSUPPORTED
    with pytest.raises(pkg.HostError, match="no mixture"):
        tp.optimize_mixture_weights()
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
    assert lib.iqhip_mix_class_lh(ta.engine, 0.1, d) == pkg.ERR_UNSUPPORTED and b"ascertainment" in lib.iqhip_last_error()
    assert em(ta.engine) == pkg.ERR_UNSUPPORTED
    assert lib.iqhip_mix_posteriors(ta.engine, None, d, None) == pkg.ERR_UNSUPPORTED
    # sharded: two shards on one device
    ts = pkg.PhyloTree(nwk)
    ts.set_alignment(4, 0, p2[:, :-4], f2[:-4])
    ts.set_model(model)
    ts.set_likelihood_kernel(pkg.LK_EIGEN_HIP)
    ts.attach_engine_sharded([0, 0], pkg.REDUCE_HOST)
    ts.compute_likelihood()
    assert lib.iqhip_mix_class_lh(ts.engine, 0.1, d) == pkg.ERR_UNSUPPORTED and b"sharded" in lib.iqhip_last_error()
    assert em(ts.engine) == pkg.ERR_UNSUPPORTED
    assert lib.iqhip_mix_posteriors(ts.engine, None, d, None) == pkg.ERR_UNSUPPORTED
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
    assert lib.iqhip_mix_class_lh(t3.engine, 0.1, d) == pkg.ERR_UNSUPPORTED and b"embedded" in lib.iqhip_last_error()
    assert em(t3.engine) == pkg.ERR_UNSUPPORTED
    assert lib.iqhip_mix_posteriors(t3.engine, None, d, None) == pkg.ERR_UNSUPPORTED


def test_refusal_on_a_communicator_rank(pkg, synth, oracle):
    """one rank on this device (creating the communicator is what takes this test's seconds)"""
    lib = pkg.libiqhip()
    dp = C.POINTER(C.c_double)
    d = np.zeros(1 << 12).ctypes.data_as(dp)
    n, conv = C.c_int(), C.c_int()
    w = np.array([0.5, 0.5])

    def em(engine):
        return lib.iqhip_mix_weights_em(engine, 2, 100.0, w.ctypes.data_as(dp), None, C.byref(n), C.byref(conv), None)

    c = build_case(synth, oracle, "n4_2x1")
    tc = pkg.PhyloTree(c["nwk"])
    tc.set_alignment(4, 0, c["pat"], c["freq"])
    tc.set_model(c["model"])
    tc.set_likelihood_kernel(pkg.LK_EIGEN_HIP)
    tc.attach_engine(0)
    tc.attach_comm(1, 0, pkg.comm_unique_id())
    assert lib.iqhip_comm_size(tc.engine) == 1
    tc.compute_likelihood()
    ac, bc = tc.current_branch()
    tc.compute_likelihood_derv(ac, bc)
    assert lib.iqhip_mix_class_lh(tc.engine, 0.1, d) == pkg.ERR_UNSUPPORTED and b"sharded" in lib.iqhip_last_error()
    assert em(tc.engine) == pkg.ERR_UNSUPPORTED
    assert lib.iqhip_mix_posteriors(tc.engine, None, d, None) == pkg.ERR_UNSUPPORTED
