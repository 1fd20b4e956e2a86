"""CPU: the public boundary and the planner for DNA engines with 9 .. 32 categories or components, and the +R<k>{...}
free-rate component of the -m string.  A planning-only engine builds and checks the descriptors k_traverse4w would walk
(iqhip_debug_plan, plan check always on) and reports the launch chosen for them (iqhip_debug_plan_shape)."""
import ctypes as C

import numpy as np
import pytest

from test_plan_check import plan_of, planner

TRAV_GENERIC, TRAV_WIDE4 = 1, 10   # iqhip_debug_plan_shape slot 14
IQHIP_OK, IQHIP_ERR_NO_DEVICE, IQHIP_ERR_INVALID, IQHIP_ERR_UNSUPPORTED = 0, 1, 2, 3


def shape_of(pkg, lib, e):
    rec = (C.c_int64 * len(pkg.PLAN_SHAPE_SLOTS))()
    assert lib.iqhip_debug_plan_shape(e, rec, len(rec)) == 0, lib.iqhip_last_error()
    return dict(zip(pkg.PLAN_SHAPE_SLOTS, rec)), list(rec)


@pytest.mark.parametrize("ncat", [9, 16, 32])
@pytest.mark.parametrize("nptn", [301, 100000])
@pytest.mark.parametrize("nclass", [1, 3])
def test_wide_plans_satisfy_the_kernel_contract(pkg, synth, monkeypatch, ncat, nptn, nclass):
    monkeypatch.setenv("IQHIP_WIDE4", "valu")
    lib, e = planner(pkg, 4, ncat, nptn, 30, nclass=nclass)
    try:
        for seed, mf in ((1, False), (3, True)):
            ops = plan_of(pkg, synth, 30, 40 + seed, 4, multifurcating=mf)
            assert lib.iqhip_debug_plan(e, ops, len(ops)) == 0, lib.iqhip_last_error()
            _, rec = shape_of(pkg, lib, e)
            assert rec[14] == TRAV_WIDE4
            assert 0 < rec[19] <= 64 * 1024          # dynamic LDS bytes of the top-stage launch
            assert rec[18] >= (nptn + 63) // 64      # grid: four 16-pattern tiles per workgroup, per segment
            if rec[5] > 0:                           # a staged plan: the units' launch is the same kernel
                assert rec[21] == TRAV_WIDE4 and 0 < rec[26] <= 64 * 1024
            assert lib.iqhip_debug_plan(e, ops, min(2, len(ops))) == 0, lib.iqhip_last_error()
    finally:
        lib.iqhip_destroy(e)


def test_generic_route_plans_the_same_chunks(pkg, synth, monkeypatch):
    """IQHIP_WIDE4=generic | valu: the same descriptors and chunks, the padded matrix-core kernel | k_traverse4w in slot 14"""
    recs = []
    for route in ("generic", "valu"):
        monkeypatch.setenv("IQHIP_WIDE4", route)
        lib, e = planner(pkg, 4, 12, 5000, 30, nclass=3)
        try:
            ops = plan_of(pkg, synth, 30, 41, 4)
            assert lib.iqhip_debug_plan(e, ops, len(ops)) == 0, lib.iqhip_last_error()
            recs.append(shape_of(pkg, lib, e)[1])
        finally:
            lib.iqhip_destroy(e)
    assert recs[0][14] == TRAV_GENERIC and recs[1][14] == TRAV_WIDE4
    assert recs[0][:14] == recs[1][:14]      # budget, chunk sizes, chunk and stage counts
    assert recs[0][17:19] == recs[1][17:19]  # workgroups per segment, grid


def test_category_limits_at_the_public_boundary(pkg):
    lib = pkg.libiqhip()
    e = C.c_void_p()
    rc = lib.iqhip_create(C.byref(e), 0, 4, 12, 500, 8)
    assert rc in (IQHIP_OK, IQHIP_ERR_NO_DEVICE), lib.iqhip_last_error()
    if rc == IQHIP_OK:
        lib.iqhip_destroy(e)
    for nstates, ncat in ((4, 33), (3, 9), (2, 9)):
        e = C.c_void_p()
        assert lib.iqhip_create(C.byref(e), 0, nstates, ncat, 500, 8) == IQHIP_ERR_UNSUPPORTED, (nstates, ncat)
    e = C.c_void_p()
    assert lib.iqhip_debug_create_planner(C.byref(e), 4, 33, 500, 8, 256, 18, 1) == IQHIP_ERR_UNSUPPORTED
    # (the 4 GiB-per-vector check keeps its place: 2^23 patterns x 32 categories x 4 states x 8 bytes)
    assert lib.iqhip_create(C.byref(e), 0, 4, 32, 1 << 23, 8) == IQHIP_ERR_UNSUPPORTED


def test_the_route_switch_takes_two_words_only(pkg, monkeypatch):
    """IQHIP_WIDE4 other than generic / valu is an error of a wide engine's creation, named after the function called,
    before any device is opened; an engine of at most 8 categories never reads it"""
    lib = pkg.libiqhip()
    monkeypatch.setenv("IQHIP_WIDE4", "wide4")
    e = C.c_void_p()
    assert lib.iqhip_create(C.byref(e), 0, 4, 12, 500, 8) == IQHIP_ERR_INVALID
    assert lib.iqhip_last_error().decode().startswith("iqhip_create: IQHIP_WIDE4")
    assert lib.iqhip_debug_create_planner(C.byref(e), 4, 12, 500, 8, 256, 18, 1) == IQHIP_ERR_INVALID
    assert lib.iqhip_last_error().decode().startswith("iqhip_debug_create_planner: IQHIP_WIDE4")
    assert lib.iqhip_debug_create_planner(C.byref(e), 4, 33, 500, 8, 256, 18, 1) == IQHIP_ERR_UNSUPPORTED
    assert lib.iqhip_last_error().decode().startswith("iqhip_debug_create_planner:")
    assert lib.iqhip_debug_create_planner(C.byref(e), 4, 8, 500, 8, 256, 18, 1) == IQHIP_OK
    lib.iqhip_destroy(e)


def dna_alignment(pkg, tmp_path):
    p = tmp_path / "a.phy"
    p.write_text("4 8\nA ACGTACGT\nB ACGTACGA\nC ACGAACGT\nD TCGTACGT\n")
    return pkg.Alignment(str(p))


def test_free_rate_component_of_the_model_string(pkg, tmp_path):
    aln = dna_alignment(pkg, tmp_path)
    # +R3: weights 0.5, 0.3, 0.2, rates 0.2, 1, 4 -> mean 0.1 + 0.3 + 0.8 = 1.2
    m = aln.build_model("JC+R3{0.5,0.2,0.3,1.0,0.2,4.0}")
    assert m.ncat == 3 and m.p_invar == 0.0
    np.testing.assert_allclose(m.props, [0.5, 0.3, 0.2], rtol=1e-15)
    np.testing.assert_allclose(m.rates, [0.2 / 1.2, 1.0 / 1.2, 4.0 / 1.2], rtol=1e-15)
    # +R10: equal weights, rates 1 .. 10 -> mean 5.5
    body = ",".join("0.1,%d" % (k + 1) for k in range(10))
    m = aln.build_model("HKY{2.0}+F{0.1,0.2,0.3,0.4}+R10{%s}" % body)
    assert m.ncat == 10
    np.testing.assert_allclose(m.props, np.full(10, 0.1), rtol=1e-15)
    np.testing.assert_allclose(m.rates, np.arange(1, 11) / 5.5, rtol=1e-14)
    assert abs(np.dot(m.props, m.rates) - 1.0) < 1e-14
    # +I{0.2}+R4: weights 0.4, 0.3, 0.2, 0.1 scaled by 0.8, rates 0.5, 1, 2, 3 -> mean 0.2 + 0.3 + 0.4 + 0.3 = 1.2
    m = aln.build_model("JC+I{0.2}+R4{0.4,0.5,0.3,1,0.2,2,0.1,3}")
    assert m.ncat == 4 and m.p_invar == 0.2
    np.testing.assert_allclose(m.props, [0.32, 0.24, 0.16, 0.08], rtol=1e-15)
    np.testing.assert_allclose(m.rates, [0.5 / 1.2, 1 / 1.2, 2 / 1.2, 3 / 1.2], rtol=1e-15)
    # a Gamma model of 16 categories parses as before
    m = aln.build_model("JC+G16{0.7}")
    assert m.ncat == 16 and abs(m.rates.mean() - 1.0) < 1e-12


@pytest.mark.parametrize("bad", ["JC+R3{0.5,0.2,0.3,1.0,0.3,4.0}",      # weights sum to 1.1
                                 "JC+R3{0.5,0.2,0.3,1.0,0.2}",          # odd number of values
                                 "JC+R2{0.5,0.2,0.3,1.0,0.2,4.0}",      # three pairs for two categories
                                 "JC+R3"])
def test_bad_free_rate_strings_are_refused(pkg, tmp_path, bad):
    aln = dna_alignment(pkg, tmp_path)
    with pytest.raises(Exception):
        aln.build_model(bad)
