"""GPU: per-class log-likelihoods of a mixture engine (kernels_classlnl.hip, iqhip_class_lnl, PhyloTree.class_lnl): K candidate
models ride as the K classes of one mixture engine and one traversal returns K log-likelihoods.
  1. every lnl[m] against np.dot(freq, textbook.site_log_likelihoods(.., model_m)) of that class's plain model, relative
     bound 1e-9 (the bound tests/test_mixture.py uses for lnL); floored == 0; two calls return identical bits.
  2. the same against compute_likelihood() of a plain engine holding model m, same bound.
  3. class weights other than 1 (1 / K folded into props): the same values within the bound.
  4. +I in both forms: the resident ptn_invar for every class, and a class_invar matrix with a different p-inv per class.
  5. the deep caterpillar of tests/test_em_gpu.py (400 taxa), on an inner branch whose two ends both carry scale counters:
     the scale term.
  6. the refusals.
Shapes: 4 states / 300 patterns cross one 256-pattern workgroup with a remainder; 8 x 4 = 32 components is the wide 4-state
route, 24 x 4 = 96 components the 20-state limit, 5 x 1 a class of one component."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RTOL = 1e-9
# name: (states, seq_type, classes, rates per class, taxa, patterns asked for)
CASES = {
    "n4_3x4": (4, 0, 3, 4, 8, 300),
    "n4_5x1": (4, 0, 5, 1, 8, 300),
    "n4_8x4": (4, 0, 8, 4, 8, 300),
    "n20_3x4": (20, 1, 3, 4, 8, 70),
    "n20_24x4": (20, 1, 24, 4, 8, 70),
    "n64_4x1": (64, 2, 4, 1, 6, 40),
}
SEED = 5200


def candidate_classes(synth, n, nclass, ncat, seed, weight=1.0, pinv=None):
    """nclass unrelated reversible models (own exchangeabilities, frequencies and Gamma shape): the candidates.  The props of
    class m are weight * (1 - pinv[m]) / ncat -> the mixture model and the plain per-class models (props without weight)"""
    plain, folded = [], []
    for m in range(nclass):
        pm = 0.0 if pinv is None else float(pinv[m])
        base = synth.random_reversible_model(n, seed + 17 * m, alpha=0.5 + 0.3 * m, ncat=ncat)
        props = np.full(ncat, (1.0 - pm) / ncat)
        plain.append(synth.Model(base.Q, base.freqs, base.eval, base.evec, base.inv_evec, base.rates, props, 0.0, "cand%d" % m))
        folded.append(synth.Model(base.Q, base.freqs, base.eval, base.evec, base.inv_evec, base.rates, props * weight, 0.0,
                                  "cand%d" % m))
    mix = synth.MixtureModel(folded, np.repeat(np.arange(nclass), ncat), np.concatenate([c.rates for c in folded]),
                             np.concatenate([c.props for c in folded]))
    return mix, plain


def device_tree(pkg, nwk, n, seq_type, pat, freq, invar, model):
    t = pkg.PhyloTree(nwk)
    t.set_alignment(n, seq_type, pat, freq, invar)
    t.set_model(model)
    t.set_likelihood_kernel(pkg.LK_EIGEN_HIP)
    t.attach_engine(0)
    return t


def textbook_lnl(ot, pat, freq, plain, seq_type, su, invar=None):
    """per class: sum_p freq[p] log(L_p + invar[m][p]), L_p from the probability-space pruning"""
    import textbook
    out = []
    for m, model in enumerate(plain):
        logs = textbook.site_log_likelihoods(ot.adj, pat, model, seq_type, su)
        if invar is not None:
            iv = invar[m]
            logs = np.where(iv > 0.0, np.logaddexp(logs, np.log(np.where(iv > 0.0, iv, 1.0))), logs)
        out.append(float(np.dot(freq, logs)))
    return np.array(out)


_built = {}


@pytest.fixture(scope="module")
def cases(pkg, synth, oracle):
    """name -> the case: mixture tree on the device, its class_lnl on the current branch, the textbook values; built once"""
    def get(name):
        if name not in _built:
            n, seq_type, nclass, ncat, ntaxa, nptn = CASES[name]
            mix, plain = candidate_classes(synth, n, nclass, ncat, SEED + n + nclass)
            su = oracle.state_unknown_for(n, seq_type)
            nwk, pat, freq = synth.make_workload(ntaxa, nptn, plain[0], SEED + n + nclass + 1, 0.02, su)
            freq = np.asarray(freq, dtype=np.float64)
            ot = oracle.OracleTree(nwk, n, seq_type, pat, freq, None, plain[0])
            t = device_tree(pkg, nwk, n, seq_type, pat, freq, None, mix)
            t.compute_likelihood()
            a, b = t.current_branch()
            lnl, floored = t.class_lnl(a, b, np.ones(nclass))
            _built[name] = dict(name=name, n=n, seq_type=seq_type, nclass=nclass, ncat=ncat, nwk=nwk, pat=pat, freq=freq, su=su,
                                ot=ot, t=t, a=a, b=b, mix=mix, plain=plain, lnl=lnl, floored=floored,
                                ref=textbook_lnl(ot, pat, freq, plain, seq_type, su))
        return _built[name]
    yield get
    _built.clear()


@pytest.fixture
def case(request, cases):
    return cases(request.param)


per_case = pytest.mark.parametrize("case", sorted(CASES), indirect=True)


def report(what, got, ref):
    print("%s: max rel %.3e" % (what, float(np.max(np.abs(got - ref) / np.abs(ref)))))


@per_case
def test_against_the_textbook(case):
    c = case
    assert c["pat"].shape[1] == CASES[c["name"]][5] and c["t"].nclass == c["nclass"]
    if c["n"] == 4:
        assert c["pat"].shape[1] > 256 and c["pat"].shape[1] % 256 != 0
    report(c["name"] + " textbook", c["lnl"], c["ref"])
    assert c["lnl"].shape == (c["nclass"],) and np.all(c["floored"] == 0)
    assert len(set(np.round(c["ref"], 3))) == c["nclass"]          # the candidates differ
    np.testing.assert_allclose(c["lnl"], c["ref"], rtol=RTOL, atol=0)
    again, fl = c["t"].class_lnl(c["a"], c["b"], np.ones(c["nclass"]))
    assert np.array_equal(again, c["lnl"]) and np.all(fl == 0)     # identical bits


@per_case
def test_against_a_plain_engine(case, pkg):
    c = case
    t = device_tree(pkg, c["nwk"], c["n"], c["seq_type"], c["pat"], c["freq"], None, c["plain"][0])
    own = []
    for model in c["plain"]:
        t.set_model(model)
        t.clear_all_partial_lh()
        own.append(t.compute_likelihood())
    own = np.array(own)
    report(c["name"] + " plain engine", c["lnl"], own)
    np.testing.assert_allclose(c["lnl"], own, rtol=RTOL, atol=0)


@per_case
def test_folded_class_weights(case, pkg, synth):
    c = case
    K = c["nclass"]
    mix, _ = candidate_classes(synth, c["n"], K, c["ncat"], SEED + c["n"] + K, weight=1.0 / K)
    t = device_tree(pkg, c["nwk"], c["n"], c["seq_type"], c["pat"], c["freq"], None, mix)
    t.compute_likelihood()
    lnl, fl = t.class_lnl(*t.current_branch(), np.full(K, 1.0 / K))
    report(c["name"] + " weights 1/K", lnl, c["ref"])
    assert np.all(fl == 0)
    np.testing.assert_allclose(lnl, c["ref"], rtol=RTOL, atol=0)
    np.testing.assert_allclose(lnl, c["lnl"], rtol=RTOL, atol=0)
    # on another branch of the same tree: the same numbers within the bound
    x = next(v for v in range(t.num_nodes) if len(t.neighbors(v)) > 1)
    y = t.neighbors(x)[-1][0]
    other, _ = t.class_lnl(x, y, np.full(K, 1.0 / K))
    np.testing.assert_allclose(other, c["ref"], rtol=RTOL, atol=0)


@pytest.mark.parametrize("name", ["n4_3x4", "n20_3x4"])
def test_invariable_sites(name, pkg, synth, oracle):
    n, seq_type, K, ncat, ntaxa, nptn = CASES[name]
    pinv = np.linspace(0.1, 0.3, K)
    mix, plain = candidate_classes(synth, n, K, ncat, SEED + n + K, pinv=pinv)
    su = oracle.state_unknown_for(n, seq_type)
    nwk, pat, freq = synth.make_workload(ntaxa, nptn - 8, plain[0], SEED + n + K + 1, 0.0, su)
    pat = np.concatenate([pat, np.tile((np.arange(8) % n).astype(np.uint8), (ntaxa, 1))], axis=1)   # constant patterns
    freq = np.concatenate([np.asarray(freq, dtype=np.float64), np.full(8, 5.0)])
    const = np.all(pat == pat[0:1], axis=0) & (pat[0] < n)
    assert np.count_nonzero(const) >= 8
    # per class: p-inv of the class times the class's frequency of the constant state (computePtnInvar)
    per_class = np.stack([np.where(const, pinv[m] * plain[m].freqs[np.minimum(pat[0], n - 1)], 0.0) for m in range(K)])
    ot = oracle.OracleTree(nwk, n, seq_type, pat, freq, None, plain[0])
    # (a) the resident ptn_invar (class 0's) for every class
    t = device_tree(pkg, nwk, n, seq_type, pat, freq, per_class[0], mix)
    t.compute_likelihood()
    a, b = t.current_branch()
    lnl, fl = t.class_lnl(a, b, np.ones(K))
    ref = textbook_lnl(ot, pat, freq, plain, seq_type, su, invar=np.tile(per_class[0], (K, 1)))
    none = textbook_lnl(ot, pat, freq, plain, seq_type, su)
    report(name + " resident ptn_invar", lnl, ref)
    assert np.all(fl == 0) and np.all(np.abs(ref - none) > 1e-6 * np.abs(ref))   # the term matters
    np.testing.assert_allclose(lnl, ref, rtol=RTOL, atol=0)
    # (b) a matrix with a different p-inv per class
    lnl2, fl2 = t.class_lnl(a, b, np.ones(K), class_invar=per_class)
    ref2 = textbook_lnl(ot, pat, freq, plain, seq_type, su, invar=per_class)
    report(name + " class_invar", lnl2, ref2)
    assert np.all(fl2 == 0) and np.all(np.abs(ref2[1:] - ref[1:]) > 1e-6 * np.abs(ref[1:]))
    np.testing.assert_allclose(lnl2, ref2, rtol=RTOL, atol=0)
    # ... and against a plain engine that holds model m with its own ptn_invar
    p = device_tree(pkg, nwk, n, seq_type, pat, freq, per_class[K - 1], plain[K - 1])
    own = p.compute_likelihood()
    assert abs(lnl2[K - 1] - own) <= RTOL * abs(own)


def test_scale_counters_at_both_ends(pkg, synth, oracle):
    """the deep caterpillar of tests/test_em_gpu.py: 400 taxa, an inner branch with scaling events at both ends"""
    n, seq_type, K, ncat, ntaxa = 4, 0, 2, 2, 400
    mix, plain = candidate_classes(synth, n, K, ncat, SEED + 77)
    su = oracle.state_unknown_for(n, seq_type)
    nwk = synth.random_tree_newick(ntaxa, 7300 + 4 + 4 + ntaxa, 0.5, 0.9, True)
    st = synth.simulate_alignment(nwk, plain[0], 200, SEED + 78, 0.0, su)
    pat, freq = synth.compress_patterns(st)
    ot = oracle.OracleTree(nwk, n, seq_type, pat, freq, None, plain[0])
    t = device_tree(pkg, nwk, n, seq_type, pat, freq, None, mix)
    t.compute_likelihood()
    inner = [(x, y) for x in range(t.num_nodes) for y, _ in t.neighbors(x) if x < y and not ot.is_leaf(x) and not ot.is_leaf(y)]
    found = None
    for x, y in inner[len(inner) // 2:] + inner[:len(inner) // 2]:
        t.compute_likelihood_derv(x, y)              # makes (x, y) the current branch, both vectors computed
        if t.fetch_scale_num(x, y).max() >= 1 and t.fetch_scale_num(y, x).max() >= 1:
            found = (x, y)
            break
    assert found, "no internal branch with scaling events at both ends"
    lnl, fl = t.class_lnl(*found, np.ones(K))
    assert t.fetch_scale_num(found[0], found[1]).max() >= 1 and t.fetch_scale_num(found[1], found[0]).max() >= 1
    ref = textbook_lnl(ot, pat, freq, plain, seq_type, su)
    report("deep caterpillar", lnl, ref)
    assert np.all(fl == 0)
    np.testing.assert_allclose(lnl, ref, rtol=RTOL, atol=0)


def test_refusals(cases, pkg):
    c = cases("n4_3x4")
    t, K, a, b = c["t"], c["nclass"], c["a"], c["b"]
    lib = pkg.libiqhip()
    dp = C.POINTER(C.c_double)
    out, ones = np.zeros(K), np.ones(K)
    o, w = out.ctypes.data_as(dp), ones.ctypes.data_as(dp)
    for bad in (0.0, -1.0, np.nan, np.inf):
        wb = np.ones(K)
        wb[1] = bad
        with pytest.raises(RuntimeError, match="class weight"):
            t.class_lnl(a, b, wb)

    def end(frm, to):
        """the end of the branch at `to` as seen from `frm`: a leaf, or the key of the vector frm -> to"""
        if len(t.neighbors(to)) == 1:
            return pkg.BranchEnd(0, to, 0)
        return pkg.BranchEnd(t.neighbor_info(frm, to)["key"], -1, 0)

    t.class_lnl(a, b, ones)                                  # theta of (a, b) resident, every vector computed
    ea, eb = end(b, a), end(a, b)
    ln = t.neighbor_info(a, b)["length"]
    assert lib.iqhip_class_lnl(t.engine, ea, eb, ln, w, None, o, None) == 0, lib.iqhip_last_error()
    assert np.array_equal(out, c["lnl"])                      # the raw call: the same bits
    assert lib.iqhip_class_lnl(t.engine, ea, eb, -1.0, w, None, o, None) == pkg.ERR_INVALID
    assert lib.iqhip_class_lnl(t.engine, ea, eb, float("nan"), w, None, o, None) == pkg.ERR_INVALID
    assert lib.iqhip_class_lnl(None, ea, eb, ln, w, None, o, None) == pkg.ERR_INVALID
    assert lib.iqhip_class_lnl(t.engine, ea, eb, ln, None, None, o, None) == pkg.ERR_INVALID
    assert lib.iqhip_class_lnl(t.engine, ea, eb, ln, w, None, None, None) == pkg.ERR_INVALID
    # another branch than the one theta was built from.  With one vector per directed branch (LM_ALL_BRANCH) every key
    # stays valid while theta moves
    t2 = pkg.PhyloTree(c["nwk"])
    t2.set_mem_mode(pkg.LM_ALL_BRANCH)
    t2.set_alignment(c["n"], c["seq_type"], c["pat"], c["freq"], None)
    t2.set_model(c["mix"])
    t2.set_likelihood_kernel(pkg.LK_EIGEN_HIP)
    t2.attach_engine(0)
    t2.compute_likelihood()
    inner = [(x, y) for x in range(t2.num_nodes) for y, _ in t2.neighbors(x)
             if x < y and len(t2.neighbors(x)) > 1 and len(t2.neighbors(y)) > 1]
    (x, y), (u, v) = inner[0], inner[1]
    t2.compute_likelihood_derv(x, y)                         # both vectors of (x, y); theta is that of (x, y)
    t2.compute_likelihood_derv(u, v)                         # both vectors of (u, v); theta_computed is still set, as in the
                                                             # reference (its callers reset it): theta stays that of (x, y)

    def end2(frm, to):
        return pkg.BranchEnd(t2.neighbor_info(frm, to)["key"], -1, 0)

    assert lib.iqhip_class_lnl(t2.engine, end2(v, u), end2(u, v), ln, w, None, o, None) == pkg.ERR_INVALID
    assert b"not resident for this branch" in lib.iqhip_last_error()
    assert lib.iqhip_class_lnl(t2.engine, end2(y, x), end2(x, y), ln, w, None, o, None) == 0, lib.iqhip_last_error()
    # theta never computed: a fresh engine
    t3 = device_tree(pkg, c["nwk"], c["n"], c["seq_type"], c["pat"], c["freq"], None, c["mix"])
    assert lib.iqhip_class_lnl(t3.engine, ea, eb, ln, w, None, o, None) == pkg.ERR_INVALID
    assert b"compute_theta" in lib.iqhip_last_error()
    # a plain engine (the model came through iqhip_set_model): unsupported
    p = device_tree(pkg, c["nwk"], c["n"], c["seq_type"], c["pat"], c["freq"], None, c["plain"][0])
    p.compute_likelihood()
    p.compute_likelihood_derv(*p.current_branch())
    assert lib.iqhip_class_lnl(p.engine, ea, eb, ln, w, None, o, None) == pkg.ERR_UNSUPPORTED
    with pytest.raises(RuntimeError, match="no mixture"):
        p.class_lnl(*p.current_branch(), np.ones(1))
    ms = C.c_double()
    assert lib.iqhip_debug_class_lnl_timing(None, C.byref(ms)) == pkg.ERR_INVALID
    assert t.class_lnl_timing() >= 0.0


def test_one_class_through_the_mixture_call(pkg, synth, oracle):
    """nclass == 1 is allowed when the model came through iqhip_set_mixture_model: a 4-state engine on 64-pattern tiles"""
    n, seq_type, ntaxa, nptn = 4, 0, 8, 300
    _, plain = candidate_classes(synth, n, 1, 4, SEED + 3)
    m = plain[0]
    su = oracle.state_unknown_for(n, seq_type)
    nwk, pat, freq = synth.make_workload(ntaxa, nptn, m, SEED + 4, 0.02, su)
    t = device_tree(pkg, nwk, n, seq_type, pat, freq, None, m)
    ref = t.compute_likelihood()
    a, b = t.current_branch()
    t.compute_likelihood_derv(a, b)
    lib = pkg.libiqhip()
    dp = C.POINTER(C.c_double)
    arr = [np.ascontiguousarray(x, dtype=np.float64) for x in (m.eval, m.evec, m.inv_evec, m.rates, m.props)]
    tip = np.ascontiguousarray(t.tip_partial_lh())
    assert lib.iqhip_set_mixture_model(t.engine, 1, None, *[x.ctypes.data_as(dp) for x in arr], t.state_unknown,
                                       tip.ctypes.data_as(dp)) == 0, lib.iqhip_last_error()
    # (the same model: the vectors on the device stay valid; theta is rebuilt)
    def end(frm, to):
        if len(t.neighbors(to)) == 1:
            return pkg.BranchEnd(0, to, 0)
        return pkg.BranchEnd(t.neighbor_info(frm, to)["key"], -1, 0)
    ea, eb = end(b, a), end(a, b)
    assert lib.iqhip_compute_theta(t.engine, ea, eb) == 0, lib.iqhip_last_error()
    out, w, fl = np.zeros(1), np.ones(1), np.zeros(1, dtype=np.int64)
    rc = lib.iqhip_class_lnl(t.engine, ea, eb, t.neighbor_info(a, b)["length"], w.ctypes.data_as(dp), None, out.ctypes.data_as(dp),
                             fl.ctypes.data_as(C.POINTER(C.c_int64)))
    assert rc == 0, lib.iqhip_last_error()
    print("one class: %.12f plain engine %.12f" % (out[0], ref))
    assert fl[0] == 0 and abs(out[0] - ref) <= RTOL * abs(ref)
