"""GPU: DNA engines with 9 .. 32 rate categories or mixture components (iqhip_engine::wide4) against the CPU oracle.
Such an engine lives on the 16-pattern tile layout and updates its nodes with k_traverse4w (kernels_valu4w.hip,
IQHIP_WIDE4=valu: what every test here runs unless it says otherwise) or with the padded matrix-core kernel on the same
plans (IQHIP_WIDE4=generic).  Tolerances are the project's own: LNL_RTOL and
check_all_vectors (values + bit-exact scale_num) of test_parity_gpu.py, the 1e-8 derivative bounds of
test_hip_mixtures_of_4_and_64_states."""
import ctypes as C
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wide4_plan_shapes.json")
TRAV_GENERIC, TRAV_WIDE4 = 1, 10   # iqhip_debug_plan_shape slot 14
DEFAULT_VARIANT = TRAV_GENERIC     # what an engine created without IQHIP_WIDE4 runs


@pytest.fixture(autouse=True)
def new_kernel_route(monkeypatch):
    monkeypatch.setenv("IQHIP_WIDE4", "valu")   # (read when an engine is created)


def attach(pkg, nwk, pat, freq, model, invar=None):
    t = pkg.PhyloTree(nwk)
    t.set_alignment(4, 0, pat, freq, invar)
    t.set_model(model)
    t.set_likelihood_kernel(pkg.LK_EIGEN_HIP)
    t.attach_engine(0)
    return t


def plan_loaded_bytes(pkg, t):
    st, ld = C.c_double(), C.c_double()
    assert pkg.libiqhip().iqhip_timing_plan_bytes(t.engine, C.byref(st), C.byref(ld)) == 0
    return ld.value


def traversal_launches(pkg, t):
    """traversal kernel launches of one full evaluation (iqhip_timing_read counts them): 1 + the stages below the top"""
    lib = pkg.libiqhip()
    lib.iqhip_timing_enable(t.engine, 1)
    t.clear_all_partial_lh()
    t.compute_likelihood()
    ms, n = C.c_double(), C.c_int64()
    assert lib.iqhip_timing_read(t.engine, C.byref(ms), C.byref(n), 1) == 0
    lib.iqhip_timing_enable(t.engine, 0)
    return n.value


def planned_shape(pkg, synth, ncat, nptn, ntaxa, seed, nclass=1):
    """iqhip_debug_plan_shape of the full traversal of random_tree_newick(ntaxa, seed), in the caller's environment"""
    from test_plan_check import plan_of, planner
    plib, e = planner(pkg, 4, ncat, nptn, ntaxa, nclass=nclass)
    try:
        ops = plan_of(pkg, synth, ntaxa, seed, 4)
        assert plib.iqhip_debug_plan(e, ops, len(ops)) == 0, plib.iqhip_last_error()
        rec = (C.c_int64 * len(pkg.PLAN_SHAPE_SLOTS))()
        assert plib.iqhip_debug_plan_shape(e, rec, len(rec)) == 0
        return dict(zip(pkg.PLAN_SHAPE_SLOTS, rec))
    finally:
        plib.iqhip_destroy(e)


def plain_case(synth, oracle, ncat, seed, ntaxa=11, nsites=420, missing=0.02, **tree_kw):
    """alignment + oracle tree of a GTR+G<ncat> model; nsites random sites of 11 taxa give > 256 patterns"""
    model = synth.gtr_model(alpha=0.9, ncat=ncat)
    nwk = synth.random_tree_newick(ntaxa, seed, **tree_kw)
    st = synth.simulate_alignment(nwk, model, nsites, seed + 1, missing, 18)
    pat, freq = synth.compress_patterns(st)
    return model, nwk, pat, freq, oracle.OracleTree(nwk, 4, 0, pat, freq, None, model)


def case_301(synth, oracle, ncat, seed):
    """11 taxa, exactly 301 patterns (a partly filled last tile), 2 % missing data"""
    model = synth.gtr_model(alpha=0.9, ncat=ncat)
    nwk = synth.random_tree_newick(11, seed)
    st = synth.simulate_alignment(nwk, model, 2000, seed + 1, 0.02, 18)
    pat, freq = synth.compress_patterns(st)
    assert pat.shape[1] >= 301
    pat, freq = np.ascontiguousarray(pat[:, :301]), np.ascontiguousarray(freq[:301])
    return model, nwk, pat, freq, oracle.OracleTree(nwk, 4, 0, pat, freq, None, model)


def check_engine(t, ot, ntaxa):
    """lnL, every vector with its counters, derivatives, lnL from the theta buffer, one branch optimisation"""
    from test_parity_gpu import check_all_vectors, LNL_RTOL
    t.clear_all_partial_lh()
    lnl = t.compute_likelihood()
    ref, (a, b) = ot.likelihood()
    assert abs(lnl - ref) <= LNL_RTOL * abs(ref), (lnl, ref)
    assert check_all_vectors(t, ot) == ntaxa - 2
    df, ddf = t.compute_likelihood_derv(a, b)
    rdf, rddf = ot.derv(a, b)
    assert abs(ddf - rddf) <= 1e-8 * abs(rddf) and abs(df - rdf) <= 1e-8 * max(abs(rdf), 1e-3 * abs(rddf)), (df, rdf, ddf, rddf)
    assert abs(t.compute_likelihood_from_buffer() - ref) <= LNL_RTOL * abs(ref)
    before = t.compute_likelihood()
    x, y = [(x, y) for x in range(t.num_nodes) for y, _ in t.neighbors(x) if x < y][3]
    t.optimize_one_branch(x, y)
    assert t.compute_likelihood() >= before - 1e-9 * abs(before)
    return ref


@pytest.mark.parametrize("ncat", [9, 10, 13, 16, 31, 32])
def test_plain_models_match_the_oracle(pkg, synth, oracle, ncat):
    model, nwk, pat, freq, ot = case_301(synth, oracle, ncat, 300 + ncat)
    t = attach(pkg, nwk, pat, freq, model)
    check_engine(t, ot, 11)


@pytest.mark.parametrize("nclass,ncat,fused", [(3, 4, False), (5, 4, False), (9, 1, True)])
def test_mixtures_match_the_oracle_and_models_switch(pkg, synth, oracle, nclass, ncat, fused):
    from test_parity_gpu import LNL_RTOL
    from test_mixture import make_mix
    model, nwk, pat, freq, ot = make_mix(synth, oracle, 4, nclass, ncat, fused, 11, 420, 500 + nclass, 0)
    assert model.ncat == (nclass if fused else nclass * ncat) and model.ncat > 8
    t = attach(pkg, nwk, pat, freq, model)
    check_engine(t, ot, 11)
    # plain -> mixture -> plain on the same engine: the layout stays, the kernel instantiation follows the class count
    plain = synth.gtr_model(alpha=0.7, ncat=model.ncat)
    for m2 in (plain, model, plain):
        t.set_model(m2)
        t.clear_all_partial_lh()
        o2 = oracle.OracleTree(t.tree_string(), 4, 0, pat, freq, None, m2)   # (one branch was optimised above)
        r2, _ = o2.likelihood()
        assert abs(t.compute_likelihood() - r2) <= LNL_RTOL * abs(r2)


def test_scaling_and_register_hand_over_on_a_caterpillar(pkg, synth, oracle, monkeypatch):
    """320-taxon caterpillar with long branches, 12 categories: every op but the first takes one child from the registers
    of the op before it, counters included, and patterns are rescaled along the chain"""
    from test_parity_gpu import check_all_vectors, LNL_RTOL
    model, nwk, pat, freq, ot = plain_case(synth, oracle, 12, 77, ntaxa=320, nsites=200, lo=0.4, hi=0.9, caterpillar=True)
    t = attach(pkg, nwk, pat, freq, model)
    lnl = t.compute_likelihood()
    ref, (a, b) = ot.likelihood()
    frm, to = (a, b) if not ot.is_leaf(b) else (b, a)
    assert ot.partial(frm, to)[1].max() >= 1
    assert abs(lnl - ref) <= LNL_RTOL * abs(ref)
    assert check_all_vectors(t, ot) == 320 - 2
    # the hand-over in the plan's own account (iqhip_timing_plan_bytes): on the generic route each of the 317 ops after the
    # first loads its inner child, k_traverse4w only where a segment begins -- a chain has few segments, so most of them go
    monkeypatch.setenv("IQHIP_WIDE4", "generic")
    tg = attach(pkg, nwk, pat, freq, model)
    tg.compute_likelihood()
    t.clear_all_partial_lh()
    t.compute_likelihood()   # (the account is of the last submission: the full traversal again)
    per_vector = (-(-pat.shape[1] // 64) * 64) * (4 * 12 * 8 + 2)
    saved = (plan_loaded_bytes(pkg, tg) - plan_loaded_bytes(pkg, t)) / per_vector
    print("inner-child loads saved:", saved, "of 317")
    assert 317 / 2 < saved <= 317 and saved == int(saved)


def test_iupac_codes_take_the_slow_leaf_path(pkg, synth, oracle):
    from test_parity_gpu import check_all_vectors, LNL_RTOL
    model = synth.gtr_model(alpha=0.9, ncat=10)
    nwk = synth.random_tree_newick(10, 3)
    st = synth.simulate_alignment(nwk, model, 500, 4)
    rng = np.random.default_rng(1)
    m = rng.random(st.shape) < 0.35
    st[m] = rng.integers(4, 19, m.sum())
    st[3, :] = 18  # an all-gap sequence
    pat, freq = synth.compress_patterns(st)
    ot = oracle.OracleTree(nwk, 4, 0, pat, freq, None, model)
    t = attach(pkg, nwk, pat, freq, model)
    ref, _ = ot.likelihood()
    assert abs(t.compute_likelihood() - ref) <= LNL_RTOL * abs(ref)
    assert check_all_vectors(t, ot) > 0


def test_other_consumers_rell_pattern_lh_and_staged_plans(pkg, synth, oracle, monkeypatch):
    """C = 12: scaled pattern lnL, per-category pattern likelihoods, RELL, and a staged plan (IQHIP_SPLIT)"""
    from test_parity_gpu import check_all_vectors, LNL_RTOL
    model, nwk, pat, freq, ot = plain_case(synth, oracle, 12, 41, ntaxa=24)
    monkeypatch.setenv("IQHIP_SPLIT", "4")
    t = attach(pkg, nwk, pat, freq, model)
    shape = planned_shape(pkg, synth, 12, pat.shape[1], 24, 41)   # the same tree (plain_case's seed) under the same switch
    monkeypatch.delenv("IQHIP_SPLIT")
    assert shape["stages"] >= 1 and shape["stage_units_0"] >= 2 and shape["unit_variant"] == shape["top_variant"] == TRAV_WIDE4
    assert traversal_launches(pkg, t) == 1 + shape["stages"]   # the engine ran the staged plan, one launch per stage + the top
    lnl = t.compute_likelihood()
    ref, (a, b) = ot.likelihood()
    assert abs(lnl - ref) <= LNL_RTOL * abs(ref)
    assert check_all_vectors(t, ot) == 24 - 2
    _, oplh = ot.branch_lnl(a, b)
    _, sc_b, _ = ot.partial(a, b)   # a is the leaf end of the root branch
    scaled = oracle.pattern_lh_scaled(oplh, None, sc_b)
    np.testing.assert_allclose(t.compute_pattern_likelihood(), scaled, rtol=1e-10)
    n, ncat = 4, 12
    th, _ = ot.theta(a, b)
    val = (np.exp(np.outer(model.rates * ot.length(a, b), model.eval)) * model.props[:, None]).reshape(-1)
    expect = (th * val[None, :]).reshape(th.shape[0], ncat, n).sum(axis=2)
    np.testing.assert_allclose(t.compute_pattern_lh_cat(), expect, rtol=1e-10, atol=1e-300)
    rng = np.random.default_rng(5)
    nsite = int(freq.sum())
    boot = rng.multinomial(nsite, freq / freq.sum(), size=8).astype(np.float32)
    t.set_boot_samples(boot)
    np.testing.assert_allclose(t.compute_rell(), boot.astype(np.float64) @ scaled, rtol=1e-9)


@pytest.mark.parametrize("kind", ["plain9", "plain32", "mix12"])
def test_new_kernel_agrees_with_the_generic_route(pkg, synth, oracle, kind, monkeypatch):
    """the same plans on k_traverse4w and, under IQHIP_WIDE4=generic, on k_traverse_mfma<4, 256, true>: values at
    check_all_vectors' tolerance, identical scale_num"""
    from test_mixture import make_mix
    if kind == "mix12":
        model, nwk, pat, freq, ot = make_mix(synth, oracle, 4, 3, 4, False, 11, 420, 611, 0)
    else:
        model, nwk, pat, freq, ot = plain_case(synth, oracle, int(kind[5:]), 600 + len(kind))
    got = []
    for route in ("generic", "valu"):
        monkeypatch.setenv("IQHIP_WIDE4", route)
        t = attach(pkg, nwk, pat, freq, model)
        t.compute_likelihood()
        vecs = []
        for a in range(t.num_nodes):
            for b, _ in t.neighbors(a):
                info = t.neighbor_info(a, b)
                if not ot.is_leaf(b) and (info["computed"] & 1) and info["key"] != 0:
                    vecs.append((a, b, t.fetch_partial(a, b), t.fetch_scale_num(a, b)))
        got.append(vecs)
    assert len(got[0]) == len(got[1]) == 11 - 2
    for (a, b, v0, s0), (a1, b1, v1, s1) in zip(*got):
        assert (a, b) == (a1, b1) and np.array_equal(s0, s1)
        scale = np.abs(v0).max(axis=1, keepdims=True)
        np.testing.assert_allclose(v1 / scale, v0 / scale, rtol=0, atol=1e-10)


def test_default_route(pkg, synth, oracle, monkeypatch):
    """IQHIP_WIDE4 unset: the engine's own choice (DEFAULT_VARIANT) against the oracle; a word that names
    neither route is refused at creation, not taken for one of them"""
    monkeypatch.delenv("IQHIP_WIDE4")
    model, nwk, pat, freq, ot = plain_case(synth, oracle, 12, 43)
    assert planned_shape(pkg, synth, 12, pat.shape[1], 11, 43)["top_variant"] == DEFAULT_VARIANT
    check_engine(attach(pkg, nwk, pat, freq, model), ot, 11)
    assert planned_shape(pkg, synth, 12, pat.shape[1], 11, 43, nclass=3)["top_variant"] == DEFAULT_VARIANT
    monkeypatch.setenv("IQHIP_WIDE4", "wide4")
    e = C.c_void_p()
    assert pkg.libiqhip().iqhip_create(C.byref(e), 0, 4, 12, 500, 8) == 2   # IQHIP_ERR_INVALID
    assert pkg.libiqhip().iqhip_create(C.byref(e), 0, 4, 8, 500, 8) == 0   # (an engine of at most 8 categories never reads it)
    pkg.libiqhip().iqhip_destroy(e)


def test_limits_and_unchanged_narrow_plans(pkg, synth, monkeypatch):
    """4 states stop at 32 categories, embedded 3-state data at 8; engines of at most 8 categories plan as before"""
    from test_plan_check import plan_of, planner
    lib = pkg.libiqhip()
    for nstates, ncat in ((4, 33), (3, 9)):
        e = C.c_void_p()
        assert lib.iqhip_create(C.byref(e), 0, nstates, ncat, 500, 8) == 3   # IQHIP_ERR_UNSUPPORTED
    golden = json.load(open(GOLDEN))
    for key, want in golden["records"].items():
        ncat, nclass = map(int, key.split("-"))
        plib, e = planner(pkg, 4, ncat, 3000, 30, nclass=nclass)
        try:
            ops = plan_of(pkg, synth, 30, 41, 4)
            assert plib.iqhip_debug_plan(e, ops, len(ops)) == 0, plib.iqhip_last_error()
            rec = (C.c_int64 * len(pkg.PLAN_SHAPE_SLOTS))()
            assert plib.iqhip_debug_plan_shape(e, rec, len(rec)) == 0
            assert list(rec) == want, key
        finally:
            plib.iqhip_destroy(e)
    for route, variant in (("generic", TRAV_GENERIC), ("valu", TRAV_WIDE4)):
        monkeypatch.setenv("IQHIP_WIDE4", route)
        plib, e = planner(pkg, 4, 12, 3000, 30)
        try:
            ops = plan_of(pkg, synth, 30, 41, 4)
            assert plib.iqhip_debug_plan(e, ops, len(ops)) == 0, plib.iqhip_last_error()
            rec = (C.c_int64 * len(pkg.PLAN_SHAPE_SLOTS))()
            assert plib.iqhip_debug_plan_shape(e, rec, len(rec)) == 0
            assert rec[14] == variant
        finally:
            plib.iqhip_destroy(e)


def test_polytomies_no_scale_chains_and_the_scalar_zero_rule(pkg, synth, oracle):
    """C = 9: a tree with polytomies (IQHIP_OP_NO_SCALE intermediates, IQHIP_OP_SCALAR_RULE at the node), then the scalar
    kernel's lh_max == 0 rule forced through the C ABI with all-zero patterns -- the checks of test_multifurcation_gpu.py"""
    import test_multifurcation_gpu as mf
    mf.test_polytomies_against_oracle(pkg, synth, oracle, 4, 9, 0, 12, 400, 0)
    mf.test_scalar_kernel_zero_rule_at_a_multifurcating_node(pkg, synth, oracle, 4, 9, 0, 300)


def test_ascertainment_correction_batch_and_per_step_sweep(pkg, synth, oracle):
    """+ASC at C = 16: lnL against the oracle, batched NNI candidates against the oracle and against the branch-by-branch
    evaluator, and a one-submission sweep whose lengths equal the per-branch form's bit for bit, on the per-step path
    (never the persistent 4-state sweep kernel) -- the checks of test_asc_batch_gpu.py"""
    import test_asc_batch_gpu as ab
    from test_parity_gpu import LNL_RTOL
    inputs = ab.asc_inputs(synth, 4, 16, 0, 12, 800)
    t = ab.asc_tree(pkg, inputs, 4, 0)
    ot = ab.asc_oracle(oracle, inputs, 4, 0)
    ref, (a, b) = ot.likelihood()
    assert abs(t.compute_likelihood() - ref) <= LNL_RTOL * abs(ref)
    df, ddf = t.compute_likelihood_derv(a, b)
    rdf, rddf = ot.derv(a, b)
    assert abs(ddf - rddf) <= 1e-8 * abs(rddf) and abs(df - rdf) <= 1e-8 * max(abs(rdf), 1e-3 * abs(rddf))
    ab.test_asc_batch_against_the_oracle(pkg, synth, oracle, 4, 16, 0, 12, 800)
    ab.test_asc_sweep_equals_the_per_branch_form(pkg, synth, oracle, 4, 16, 0, 14, 400)


def test_newton_forms_against_the_oracle(pkg, synth, oracle, monkeypatch):
    """C = 10: the one-launch solver and the enqueued chain (IQHIP_NEWTON=chain) against the oracle's minimize_newton, at
    test_solver_paths_gpu.py's tolerances"""
    import test_solver_paths_gpu as sp
    make = sp.plain(4, 10, 0, 9, 300, 5110)
    sp.check_solvers(pkg, lambda: make(pkg, synth, oracle), monkeypatch)


def test_two_shards_with_the_host_reduction(pkg, synth, oracle):
    """C = 12 on two shards of device 0 (IQHIP_REDUCE_HOST): the checks of test_sharded_gpu.py"""
    import test_sharded_gpu as sh
    sh.test_sharded_engine_matches_plain_engine_and_oracle(pkg, synth, oracle, 4, 12, 0, 14, 2600, dict(missing=0.04), "host2")


@pytest.mark.parametrize("rates", ["+R10{%s}" % ",".join("0.1,%g" % (0.2 * (k + 1)) for k in range(10)), "+G16{0.934}"])
def test_command_line_driver_evaluates_wide_models(pkg, synth, oracle, tmp_path, rates):
    """iqhip_lnl -m 'GTR{..}+F{..}+R10{..}' / '+G16{..}' end to end against the oracle fed by the same model producers"""
    import test_cli_gpu as cli
    model_string = "GTR{1.513,2.393,1.769,1.912,2.838}+F{0.249,0.262,0.251,0.238}" + rates
    aln = pkg.Alignment(cli.EXAMPLE)
    st, fr, _, _ = aln.arrays()
    model = aln.build_model(model_string)
    assert model.ncat == (10 if rates.startswith("+R") else 16)
    nwk = synth.random_tree_newick(44, 12)
    tf = tmp_path / "t.nwk"
    tf.write_text(cli.named_tree(nwk, aln.seq_names) + "\n")
    pre = str(tmp_path / "run")
    cli.run_cli(["-s", cli.EXAMPLE, "-te", str(tf), "-m", model_string, "-blfix", "-n", "0", "-pre", pre])
    ref, _ = oracle.OracleTree(nwk, 4, 0, st, fr, None, model).likelihood()
    lnl = float(cli.read_report(pre)["lnL"])
    assert abs(lnl - ref) <= 1e-9 * abs(ref)
