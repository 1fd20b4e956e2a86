"""CPU: the host half of the mixture class-weight EM -- the numpy restatement of ModelMixture::optimizeWeights
(tests/mixem_ref.py) never lowers the likelihood on per-class textbook likelihoods, the MIX{...} model strings through
libiqhost (weights normalised, sum w * rate = 1, component order, error cases), the new symbols, and the refusals of the
iqhip_mix_* entry points that need no device.  Also home of the case builders tests/test_mixem_gpu.py shares."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mixem_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "iq-tree_amd", "lib", "iqhip_lnl")
EXAMPLE = os.path.join(ROOT, "tests", "golden", "example.phy")


def mix_alignment(synth, oracle, n, nclass, ncat, ntaxa, nsites, seed, seq_type, missing=0.0, const_sites=0, **tree_kw):
    """A mixture model of synth.mixture_model and an alignment with an equal share of sites from EVERY class (and const_sites
    constant columns) -> model, newick, patterns, frequencies, state_unknown"""
    model = synth.mixture_model(n, nclass, seed, ncat=ncat)
    su = oracle.state_unknown_for(n, seq_type)
    nwk = synth.random_tree_newick(ntaxa, seed, **tree_kw)
    share = -(-nsites // nclass)
    parts = [synth.simulate_alignment(nwk, model.classes[m], share, seed + 1 + m, missing, su) for m in range(nclass)]
    if const_sites:
        parts.append(np.tile((np.arange(const_sites) % n).astype(np.uint8), (ntaxa, 1)))
    pat, freq = synth.compress_patterns(np.concatenate(parts, axis=1))
    return model, nwk, pat, freq, su


def class_weights(model):
    return np.array([model.props[model.cat_class == m].sum() for m in range(model.nclass)])


def mix_ptn_invar(pat, model, p_invar):
    """computePtnInvar: p_invar * frequency of the state of a constant pattern, with the weighted mean class frequencies"""
    f = sum(w * c.freqs for w, c in zip(class_weights(model), model.classes))
    const = np.all(pat == pat[0:1], axis=0) & (pat[0] < model.nstates)
    return np.where(const, p_invar * f[np.minimum(pat[0], model.nstates - 1)], 0.0)


def textbook_class_lh(adj, pat, model, seq_type, su):
    """per-class pattern likelihoods from the probability-space pruning, each pattern divided by its largest class
    -> L[nptn, nclass], log of the divisor [nptn]"""
    import textbook
    logs = np.stack([textbook.site_log_likelihoods(adj, pat, c, seq_type, su) for c in model.classes], axis=1)
    mx = logs.max(axis=1)
    return np.exp(logs - mx[:, None]), mx


@pytest.mark.parametrize("n,seq_type,nclass,ncat,p_invar", [(4, 0, 3, 4, 0.0), (20, 1, 3, 2, 0.0), (4, 0, 2, 1, 0.2)])
def test_restatement_never_lowers_the_likelihood(synth, oracle, n, seq_type, nclass, ncat, p_invar):
    model, nwk, pat, freq, su = mix_alignment(synth, oracle, n, nclass, ncat, 9, 150, 40 + n + nclass, seq_type,
                                              const_sites=12 if p_invar else 0)
    ot = oracle.OracleTree(nwk, n, seq_type, pat, freq, None, model)
    L, mx = textbook_class_lh(ot.adj, pat, model, seq_type, su)
    w0 = class_weights(model)
    invar = mix_ptn_invar(pat, model, p_invar) * np.exp(-mx) if p_invar else None
    if p_invar:
        assert np.count_nonzero(invar) >= 4
        w0 = w0 * (1.0 - p_invar)
        L = L * (1.0 - p_invar)
    res = mixem_ref.optimize_weights(L, freq, invar, w0, p_invar=p_invar or None, max_steps=40)
    assert res["steps"] >= 3 and res["last_change"][0] > 1e-3
    obj = [mixem_ref.em_objective(L, freq, invar, np.ones(nclass))]
    for row in res["trace"]:
        iv = invar * (row[nclass] / p_invar) if p_invar else None
        obj.append(mixem_ref.em_objective(L, freq, iv, row[:nclass] / w0))
    print("objective per step:", obj)
    for k in range(1, len(obj)):
        assert obj[k] >= obj[k - 1] - 1e-9 * abs(obj[k - 1]), (k, obj)
    assert obj[-1] > obj[0]
    total = res["prop"].sum() + (res["p_invar"] or 0.0)
    assert abs(total - 1.0) < 1e-12                      # every E-step's posteriors sum to the site count
    # a second run from the same start: the same bits (the input matrix is not modified)
    again = mixem_ref.optimize_weights(L, freq, invar, w0, p_invar=p_invar or None, max_steps=40)
    assert np.array_equal(again["trace"], res["trace"])


def test_mix_model_strings(pkg):
    aln = pkg.Alignment(EXAMPLE)
    gtr = "GTR{1.5,2.4,1.8,1.9,2.8}+F{0.2,0.3,0.24,0.26}"
    m = aln.build_model("MIX{JC,HKY{2.0},%s}+G4{0.8}" % gtr)
    assert m.nclass == 3 and m.ncat == 12 and m.eval.shape == (3, 4) and m.evec.shape == (3, 4, 4)
    np.testing.assert_allclose(m.class_weights, 1.0 / 3, rtol=1e-15)
    np.testing.assert_allclose(m.class_rates, 1.0, rtol=1e-15)
    assert np.array_equal(m.cat_class, np.repeat(np.arange(3), 4))            # [class][rate] order
    g = pkg.gamma_rates(0.8, 4)
    np.testing.assert_allclose(m.rates, np.tile(g, 3), rtol=1e-15)
    np.testing.assert_allclose(m.props, np.repeat(m.class_weights, 4) / 4, rtol=1e-15)
    # every class is the plain model of its name
    for k, name in enumerate(["JC", "HKY{2.0}", gtr]):
        one = aln.build_model(name + "+G4{0.8}")
        np.testing.assert_allclose(m.eval[k], one.eval, rtol=1e-13, atol=1e-15)
        assert np.array_equal(m.evec[k], one.evec) and np.array_equal(m.inv_evec[k], one.inv_evec)
        assert np.array_equal(m.class_freq[k], one.state_freq)
    np.testing.assert_allclose(m.state_freq, (m.class_weights[:, None] * m.class_freq).sum(axis=0), rtol=1e-14)
    # rates and weights: weights normalised to sum 1, rates rescaled so that sum w * rate = 1, eigenvalues carry the rate
    m2 = aln.build_model("MIX{JC:0.5:2,HKY{2.0}:2:1,%s:1:1}+G4{0.8}" % gtr)
    np.testing.assert_allclose(m2.class_weights, [0.5, 0.25, 0.25], rtol=1e-15)
    assert abs(float(np.dot(m2.class_weights, m2.class_rates)) - 1.0) < 1e-15
    np.testing.assert_allclose(m2.class_rates, np.array([0.5, 2.0, 1.0]) / 1.0, rtol=1e-15)
    np.testing.assert_allclose(m2.eval, m.eval * m2.class_rates[:, None], rtol=1e-13, atol=1e-15)
    np.testing.assert_allclose(m2.props, np.repeat(m2.class_weights, 4) / 4, rtol=1e-15)
    # a rate alone leaves the weights at 1 / k; the rates are rescaled
    m3 = aln.build_model("MIX{JC:3,HKY{2.0}}")
    assert m3.ncat == 2 and np.array_equal(m3.cat_class, [0, 1])
    np.testing.assert_allclose(m3.class_weights, [0.5, 0.5], rtol=1e-15)
    np.testing.assert_allclose(m3.class_rates, [1.5, 0.5], rtol=1e-15)
    np.testing.assert_allclose(m3.rates, [1.0, 1.0], rtol=1e-15)
    # +I: component weights w_m (1 - p) / k
    m4 = aln.build_model("MIX{JC,HKY{2.0}}+I{0.2}+G2{0.5}")
    assert m4.p_invar == 0.2
    np.testing.assert_allclose(m4.props, 0.5 * 0.8 / 2, rtol=1e-15)
    # the limit: 4 states take 32 components
    assert aln.build_model("MIX{%s}+G4{1.0}" % ",".join(["JC"] * 8)).ncat == 32
    for bad, text in [("MIX{%s}+G4{1.0}" % ",".join(["JC"] * 9), "at most 32"),
                      ("MIX{JC,MIX{JC,HKY{2}}}", "inside a MIX"),
                      ("MIX{JC,,HKY{2}}", "empty"),
                      ("MIX{JC}", "at least two"),
                      ("MIX{JC,HKY{2}:1:-0.5}", "negative"),
                      ("MIX{JC,HKY{2}:abc}", "bad number"),
                      ("MIX{JC,HKY{2}:0}", "rate must be > 0"),
                      ("MIX{JC+G4{1.0},HKY{2}}", "behind the closing brace"),
                      ("MIX{JC,HKY{2}}+F{0.25,0.25,0.25,0.25}", "inside MIX"),
                      ("MIX{JC,HKY{2}}+FO", "inside MIX"),
                      ("MIX{JC,HKY{2}}+FQ+G4{0.5}", "inside MIX"),
                      ("MIX{JC,HKY{2}}+F", "inside MIX"),
                      ("MIX{JC,HKY{2}}+F1X4", "inside MIX"),
                      ("MIX{JC,HKY{2}", "Missing }"),
                      ("MIX{JC,WAG}", "Unknown DNA model")]:
        with pytest.raises(pkg.HostError, match=text):
            aln.build_model(bad)


def test_new_symbols_exist(pkg):
    hip, host = pkg.libiqhip(), pkg.libiqhost()
    for name in ("iqhip_mix_class_lh", "iqhip_mix_weights_em", "iqhip_mix_posteriors", "iqhip_debug_mix_timing"):
        assert name in pkg.IQHIP_SYMBOLS and hasattr(hip, name)
    for name in ("iqhost_mix_class_lh", "iqhost_mix_weights_em", "iqhost_mix_posteriors", "iqhost_pattern_state_freq",
                 "iqhost_optimize_mixture_weights", "iqhost_mix_timing", "iqmodel_mixture_dims", "iqmodel_build_mixture"):
        assert hasattr(host, name)
    for name in ("mix_class_lh", "mix_weights_em", "mix_posteriors", "optimize_mixture_weights", "mix_timing"):
        assert callable(getattr(pkg.PhyloTree, name))


def test_mix_entry_points_refuse_without_a_device(pkg):
    lib = pkg.libiqhip()
    dp = C.POINTER(C.c_double)
    d = np.zeros(4096).ctypes.data_as(dp)
    w = np.full(4, 0.25)
    n, conv = C.c_int(), C.c_int()
    # null arguments
    assert lib.iqhip_mix_class_lh(None, 0.1, d) == pkg.ERR_INVALID
    assert lib.iqhip_mix_weights_em(None, 2, 100.0, w.ctypes.data_as(dp), None, C.byref(n), C.byref(conv), None) == pkg.ERR_INVALID
    assert lib.iqhip_mix_posteriors(None, None, d, None) == pkg.ERR_INVALID
    assert lib.iqhip_debug_mix_timing(None, d, None) == pkg.ERR_INVALID
    # a planning-only engine (4 states, 4 components, 2 classes)
    e = C.c_void_p()
    assert lib.iqhip_debug_create_planner(C.byref(e), 4, 4, 300, 8, 256, 18, 2) == 0, lib.iqhip_last_error()
    try:
        assert lib.iqhip_mix_class_lh(e, 0.1, d) == pkg.ERR_INVALID and b"planning-only" in lib.iqhip_last_error()
        assert lib.iqhip_mix_class_lh(e, 0.1, None) == pkg.ERR_INVALID and b"planning-only" in lib.iqhip_last_error()
        assert lib.iqhip_mix_weights_em(e, 2, 100.0, w.ctypes.data_as(dp), None, C.byref(n), C.byref(conv), None) == pkg.ERR_INVALID
        assert b"planning-only" in lib.iqhip_last_error()
        assert lib.iqhip_mix_weights_em(e, 2, 100.0, None, None, C.byref(n), C.byref(conv), None) == pkg.ERR_INVALID
        assert lib.iqhip_mix_posteriors(e, None, d, None) == pkg.ERR_INVALID and b"planning-only" in lib.iqhip_last_error()
        assert lib.iqhip_mix_posteriors(e, None, None, None) == pkg.ERR_INVALID
        assert lib.iqhip_mix_posteriors(e, None, None, d) == pkg.ERR_INVALID      # state frequencies need class_freq
    finally:
        lib.iqhip_destroy(e)


def test_cli_refuses_mixweights_without_a_mixture(tmp_path):
    """the model is parsed before the engine is created: no device is touched"""
    tree = tmp_path / "t.nwk"
    tree.write_text("(a,b,c);\n")
    r = subprocess.run([BIN, "-s", EXAMPLE, "-te", str(tree), "-m", "HKY{2.0}+G4{0.5}", "-mixweights", "-pre", str(tmp_path / "x")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "-mixweights needs a MIX{...} model" in r.stderr
    r = subprocess.run([BIN, "-s", EXAMPLE, "-te", str(tree), "-m", "MIX{JC,HKY{2.0}}+R2{0.5,0.5,0.5,1.5}", "-emrates", "-pre",
                        str(tmp_path / "x")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "not available for mixture models" in r.stderr
    r = subprocess.run([BIN, "-s", EXAMPLE, "-te", str(tree), "-m", "MIX{JC,HKY{2.0}}+I{0.1}", "-mixweights", "-pre", str(tmp_path / "x")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "-mixweights: +I is not supported" in r.stderr
    r = subprocess.run([BIN, "-s", EXAMPLE, "-te", str(tree), "-m", "MIX{JC,MIX{JC,HKY{2.0}}}", "-pre", str(tmp_path / "x")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "inside a MIX" in r.stderr
