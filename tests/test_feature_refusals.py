"""The feature drivers' shared plumbing: iqhip::require (one eligibility check) and iqhip::PhaseTimer (one phase timer).
  CPU: a null engine and a planning-only engine are refused with IQHIP_ERR_INVALID by one entry point per driver.
  GPU: the status of one entry point per driver on every kind of engine a refusal distinguishes, against a literal table
       that records what the drivers returned while each still carried its own check (the table was produced by running
       observed_statuses() below on the commit before the checks were folded; it characterises that commit, not this code).
  GPU: with iqhip_timing_enable every driver's phase readings are finite, positive where the phase launched a kernel, the
       launch counts are the ones the feature tests assert, and the readings are exactly 0 once timing is off again."""
import ctypes as C
import math

import numpy as np
import pytest

from test_parity_gpu import make_case

DP, I32P = C.POINTER(C.c_double), C.POINTER(C.c_int32)
OK, INVALID, UNSUPPORTED = 0, 2, 3
NTAXA, NSITES = 8, 100


def entry_points(pkg):
    """one entry point per eligibility check the drivers had (+ iqhip_bionj) -> {name: call(engine) -> status}; every
    argument but the engine is acceptable"""
    lib = pkg.libiqhip()
    d = np.zeros(1 << 16)
    dp = d.ctypes.data_as(DP)
    i32 = np.zeros(64, dtype=np.int32)
    end = pkg.leaf_end(0)
    ones = np.ones(8)
    pair = np.array([0, 1], dtype=np.int32)
    quartet = np.array([0, 1, 2, 3], dtype=np.int32)
    D = np.abs(np.subtract.outer(np.arange(5.0), np.arange(5.0))) + 1.0 - np.eye(5)
    steps = np.zeros(5 * 4)
    last, last_len = np.zeros(3, dtype=np.int32), np.zeros(3)
    keep = (d, i32, ones, pair, quartet, D, steps, last, last_len)   # (the calls below hold pointers into these)
    return {
        "iqhip_em_posteriors": lambda e: lib.iqhip_em_posteriors(e, 0.1, dp),
        "iqhip_mix_class_lh": lambda e: lib.iqhip_mix_class_lh(e, 0.1, dp),
        "iqhip_class_lnl": lambda e: lib.iqhip_class_lnl(e, end, end, 0.1, ones.ctypes.data_as(DP), None, dp, None),
        "iqhip_ptnlh_reserve": lambda e: lib.iqhip_ptnlh_reserve(e, 2),
        "iqhip_pair_counts": lambda e: lib.iqhip_pair_counts(e, pair.ctypes.data_as(I32P), 1, dp),
        "iqhip_quartet_cells": lambda e: lib.iqhip_quartet_cells(e, quartet.ctypes.data_as(I32P), 1, dp, i32.ctypes.data_as(I32P)),
        "iqhip_pars_init": lambda e: lib.iqhip_pars_init(e, None, 0, None),
        "iqhip_bionj": lambda e: lib.iqhip_bionj(e, 5, D.ctypes.data_as(DP), None, steps.ctypes.data_as(C.c_void_p),
                                                 last.ctypes.data_as(I32P), last_len.ctypes.data_as(DP)),
        "_keep": keep,
    }


def test_null_and_planning_only_engines_are_refused(pkg):
    lib = pkg.libiqhip()
    calls = entry_points(pkg)
    names = [k for k in calls if k != "_keep"]
    for name in names:
        assert calls[name](None) == INVALID, name
    e = C.c_void_p()
    assert lib.iqhip_debug_create_planner(C.byref(e), 4, 4, 300, NTAXA, 256, 18, 2) == 0, lib.iqhip_last_error()
    try:
        for name in names:
            assert calls[name](e) == INVALID, name
            msg = lib.iqhip_last_error()
            assert b"planning-only" in msg and msg.startswith(name.encode() + b": "), msg
    finally:
        lib.iqhip_destroy(e)


# ------------------------------------------------------------------------------------------
# the engines
# ------------------------------------------------------------------------------------------
def attached(pkg, nwk, nstates, seq_type, pat, freq, model, n_unobs=0, nsites=0, sharded=0):
    t = pkg.PhyloTree(nwk)
    t.set_alignment(nstates, seq_type, pat, freq)
    if n_unobs:
        t.set_ascertainment(n_unobs, nsites)
    t.set_model(model)
    t.set_likelihood_kernel(pkg.LK_EIGEN_HIP)
    if sharded:
        t.attach_engine_sharded([0] * sharded, pkg.REDUCE_HOST)
    else:
        t.attach_engine(0)
    return t


def with_theta(t):
    t.compute_likelihood()
    a, b = t.current_branch()
    t.compute_likelihood_derv(a, b)
    return t


def plain_tree(pkg, synth, oracle):
    return make_case(synth, oracle, pkg, NTAXA, NSITES, 4, 4, 99)[0]


def mixture_tree(pkg, synth, oracle):
    t = make_case(synth, oracle, pkg, NTAXA, NSITES, 4, 4, 98)[0]
    t.set_model(synth.mixture_model(4, 2, 5, ncat=2))
    t.clear_all_partial_lh()
    return t


def asc_tree(pkg, synth):
    """as tests/test_em_gpu.py: the variable sites, the four constant patterns appended as unobserved"""
    model = synth.gtr_model(alpha=0.9, ncat=4)
    nwk = synth.random_tree_newick(NTAXA, 5)
    st = synth.simulate_alignment(nwk, model, NSITES, 6)
    st = st[:, [s for s in range(st.shape[1]) if len(set(st[:, s].tolist())) > 1]]
    pat, freq = synth.compress_patterns(st)
    pat = np.concatenate([pat, np.tile(np.arange(4, dtype=np.uint8), (NTAXA, 1))], axis=1)
    return attached(pkg, nwk, 4, 0, pat, np.concatenate([freq, np.zeros(4)]), model, n_unobs=4, nsites=int(freq.sum()))


def embedded_tree(pkg, synth):
    """5 states on the 20-state kernels"""
    m5 = synth.random_reversible_model(5, 17, alpha=0.9, ncat=2)
    nwk = synth.random_tree_newick(NTAXA, 5)
    pat, freq = synth.compress_patterns(synth.simulate_alignment(nwk, m5, NSITES, 8))
    return attached(pkg, nwk, 5, 3, pat, freq, m5)


def sharded_tree(pkg, synth):
    """two shards on device 0.  A shard holds at least 64 patterns, which 100 sites cannot give two of: 200 patterns"""
    states = np.random.default_rng(2).integers(0, 4, size=(NTAXA, 200)).astype(np.uint8)
    return attached(pkg, synth.random_tree_newick(NTAXA, 5), 4, 0, states, np.ones(200), synth.gtr_model(alpha=0.9, ncat=4),
                    sharded=2)


def raw_engine(pkg, model=None, mixture_api=False):
    """iqhip_create alone (model None), or with the model set and no alignment.  iqhip_set_alignment refuses an engine
    without a model, so `alignment set, no model` cannot be built: the engine without either stands for it"""
    lib = pkg.libiqhip()
    e = C.c_void_p()
    ncat = 4 if model is None else len(model.rates)
    assert lib.iqhip_create(C.byref(e), 0, 4, ncat, NSITES, NTAXA) == 0, lib.iqhip_last_error()
    if model is not None:
        a = [np.ascontiguousarray(x, dtype=np.float64) for x in (model.eval, model.evec, model.inv_evec, model.rates, model.props)]
        nclass = int(getattr(model, "nclass", 1))
        tip = np.zeros(19 * nclass * 4)   # (nothing is evaluated on these engines)
        if mixture_api:
            cls = np.ascontiguousarray(getattr(model, "cat_class", np.zeros(ncat)), dtype=np.int32)
            rc = lib.iqhip_set_mixture_model(e, nclass, cls.ctypes.data_as(I32P), *[x.ctypes.data_as(DP) for x in a], 18,
                                             tip.ctypes.data_as(DP))
        else:
            rc = lib.iqhip_set_model(e, *[x.ctypes.data_as(DP) for x in a], 18, tip.ctypes.data_as(DP))
        assert rc == 0, lib.iqhip_last_error()
    return e


def observed_statuses(pkg, synth, oracle):
    """{(entry point, engine kind): status} of every entry point on every engine kind, with the refusal's text"""
    lib = pkg.libiqhip()
    calls = entry_points(pkg)
    names = [k for k in calls if k != "_keep"]
    got = {}

    def record(kind, engine):
        for name in names:
            rc = calls[name](engine)
            got[(name, kind)] = (rc, lib.iqhip_last_error().decode() if rc else "")

    t = plain_tree(pkg, synth, oracle)
    t.compute_likelihood()
    record("plain, theta not computed", t.engine)
    t.close()
    for kind, tree in (("plain", with_theta(plain_tree(pkg, synth, oracle))),
                       ("mixture", with_theta(mixture_tree(pkg, synth, oracle))),
                       ("+ASC", with_theta(asc_tree(pkg, synth))),
                       ("embedded", with_theta(embedded_tree(pkg, synth))),
                       ("sharded", sharded_tree(pkg, synth))):
        if kind == "sharded":
            tree.compute_likelihood()
        record(kind, tree.engine)
        tree.close()
    gtr, mix = synth.gtr_model(alpha=0.9, ncat=4), synth.mixture_model(4, 2, 5, ncat=2)
    for kind, args in (("no model", ()), ("model, no alignment", (gtr,)), ("mixture, no alignment", (mix, True)),
                       ("one-class mixture, no alignment", (gtr, True))):
        e = raw_engine(pkg, *args)
        record(kind, e)
        lib.iqhip_destroy(e)
    return got


# What each entry point returned on each engine kind BEFORE the drivers' own checks were folded into iqhip::require
# (recorded by running observed_statuses() on that commit).  Every (entry point, kind) pair is listed: no cell had to be
# left out.  iqhip_class_lnl is called with leaf ends, which name no branch theta was built from: where the engine is
# eligible it answers INVALID ("theta is not resident for this branch") from its own argument check.
ENTRY_POINTS = ("iqhip_em_posteriors", "iqhip_mix_class_lh", "iqhip_class_lnl", "iqhip_ptnlh_reserve", "iqhip_pair_counts",
                "iqhip_quartet_cells", "iqhip_pars_init", "iqhip_bionj")
_I, _U = INVALID, UNSUPPORTED
STATUS_ROWS = {                              # em   mix  class  reserve  pair  quartet  pars  bionj
    "plain, theta not computed":              (_I,  _U,  _U,    OK,      OK,   OK,      OK,   OK),
    "plain":                                  (OK,  _U,  _U,    OK,      OK,   OK,      OK,   OK),
    "mixture":                                (_U,  OK,  _I,    OK,      _U,   _U,      OK,   OK),
    "+ASC":                                   (_U,  _U,  _U,    OK,      OK,   _U,      OK,   OK),
    "embedded":                               (_U,  _U,  _U,    OK,      _U,   _U,      _U,   OK),
    "sharded":                                (_U,  _U,  _U,    _U,      _U,   _U,      _U,   _U),
    "no model":                               (_I,  _U,  _U,    OK,      _I,   _I,      _I,   OK),
    "model, no alignment":                    (_I,  _U,  _U,    OK,      _I,   _I,      _I,   OK),
    # a mixture without an alignment: the pair distances ask for the alignment first, likelihood mapping for the model shape
    "mixture, no alignment":                  (_U,  _I,  _I,    OK,      _I,   _U,      _I,   OK),
    "one-class mixture, no alignment":        (_I,  _U,  _I,    OK,      _I,   _U,      _I,   OK),
}
STATUS = {(name, kind): row[k] for kind, row in STATUS_ROWS.items() for k, name in enumerate(ENTRY_POINTS)}


@pytest.mark.gpu
def test_statuses_are_those_of_the_drivers_own_checks(pkg, synth, oracle):
    got = observed_statuses(pkg, synth, oracle)
    for key in sorted(got):
        print("%-22s %-34s %d  %s" % (key[0], key[1], got[key][0], got[key][1]))
    assert sorted(got) == sorted(STATUS)
    wrong = {k: (got[k][0], STATUS[k]) for k in got if got[k][0] != STATUS[k]}
    assert not wrong, wrong
    for (name, kind), (rc, msg) in got.items():
        assert rc == OK or msg.startswith(name + ": "), (name, kind, msg)


# ------------------------------------------------------------------------------------------
# the phase timer
# ------------------------------------------------------------------------------------------
def positive(*ms):
    return all(math.isfinite(x) and x > 0.0 for x in ms)


@pytest.mark.gpu
def test_phase_readings_of_every_driver(pkg, synth, oracle, monkeypatch):
    lib = pkg.libiqhip()
    ms = np.zeros(2)
    msp = ms.ctypes.data_as(DP)
    t = with_theta(plain_tree(pkg, synth, oracle))
    a, b = t.current_branch()
    assert lib.iqhip_timing_enable(t.engine, 1) == 0
    # +R EM: the E-step, the objective
    t.em_posteriors()
    t.em_objective(a, b)
    assert lib.iqhip_debug_em_timing(t.engine, msp) == 0 and positive(*ms), ms
    # pairwise distances: counts, solves
    t.compute_dist()
    assert lib.iqhip_debug_pair_timing(t.engine, msp, ms[1:].ctypes.data_as(DP)) == 0 and positive(*ms), ms
    # likelihood mapping: two chunks of one quartet, cells and solves summed over both
    monkeypatch.setenv("IQHIP_QUARTET_CHUNK", "1")
    t.quartet_likelihoods([(0, 1, 2, 3), (4, 5, 6, 7)])
    monkeypatch.delenv("IQHIP_QUARTET_CHUNK")
    assert positive(*t.quartet_timing()), t.quartet_timing()
    # BIONJ
    D = np.abs(np.subtract.outer(np.arange(5.0), np.arange(5.0))) + 1.0 - np.eye(5)
    t.bionj(D)
    bj_ms, bj_launches = t.bionj_timing()
    assert positive(bj_ms) and bj_launches == 4 * (5 - 3) + 3
    # parsimony: one update; iqhip_pars_branch_scores is not the timed scan (its launches were never counted), an
    # insertion scan is
    t.pars_init(None, 2)
    t.pars_timing(reset=True)
    t.pars_update([(NTAXA, 0, 1)])
    t.pars_branch_scores([(NTAXA, 2)])
    pt = t.pars_timing(reset=False)
    assert positive(pt["update_ms"]) and pt["scan_ms"] == 0.0 and (pt["update_launches"], pt["ops"], pt["scan_launches"]) == (1, 1, 0)
    t.pars_insert_scores([(NTAXA, 2)], 3)
    pt = t.pars_timing()
    assert positive(pt["update_ms"], pt["scan_ms"]) and pt["scan_launches"] >= 1 and pt["branches"] == 1
    assert t.pars_timing()["update_ms"] == 0.0                     # (the read before this one reset the sums)
    # UFBoot: two trees, one per chunk
    rng = np.random.default_rng(3)
    t.ptnlh_reserve(2)
    for r in range(2):
        t.ptnlh_upload(r, rng.uniform(-9.0, -1.0, size=t.nptn))
    t.set_boot_samples(rng.integers(0, 4, size=(5, t.nptn)).astype(np.float32))
    t.ufboot_init(5)
    monkeypatch.setenv("IQHIP_UFBOOT_CHUNK", "1")
    t.ufboot_update([0, 1], [1, 2], [-10.0, -11.0], [0.5, 0.5])
    monkeypatch.delenv("IQHIP_UFBOOT_CHUNK")
    product_ms, update_ms, launches = t.ufboot_timing()
    assert positive(product_ms, update_ms) and launches == 3 * 2
    # timing off again: the readings of the next calls are exactly 0
    assert lib.iqhip_timing_enable(t.engine, 0) == 0
    t.compute_dist()
    ms[:] = -1.0
    assert lib.iqhip_debug_pair_timing(t.engine, msp, ms[1:].ctypes.data_as(DP)) == 0 and ms.tolist() == [0.0, 0.0]
    t.quartet_likelihoods([(0, 1, 2, 3), (4, 5, 6, 7)])
    assert t.quartet_timing() == (0.0, 0.0)
    t.close()
    # the mixture engine: class likelihoods, two EM steps, per-class log-likelihoods
    tm = with_theta(mixture_tree(pkg, synth, oracle))
    am, bm = tm.current_branch()
    assert lib.iqhip_timing_enable(tm.engine, 1) == 0
    tm.mix_class_lh()
    tm.mix_weights_em([0.5, 0.5], max_steps=2)
    mt = tm.mix_timing()
    assert positive(mt["class_lh_ms"], mt["em_ms"]) and mt["launches"] == 2 * 2
    tm.class_lnl(am, bm, np.ones(2))
    assert positive(tm.class_lnl_timing())
    tm.close()
