"""CPU: the host half of the +R EM -- BrentStateMachine (iq-tree_amd/host/brent_host.h) against the direct restatement of
Optimization::minimizeOneDimen / brent_opt in tests/em_ref.py (same evaluation points in the same order, same result, bit
for bit), free_rate_start, the refusals of the iqhip_em_* entry points that need no device, and the command line's refusal of a
bare +R<k> without -emrates."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import em_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "iq-tree_amd", "lib", "iqhip_lnl")
EXAMPLE = os.path.join(ROOT, "tests", "golden", "example.phy")


def run_machine(pkg, func, xmin, xguess, xmax, tol):
    m = pkg.BrentStateMachine(xmin, xguess, xmax, tol)
    xs = []
    while not m.done:
        xs.append(m.x)
        m.update(func(m.x))
        assert len(xs) < 1000
    return m.result(), xs


CASES = {
    # the minimum inside the first bracket [0.95, 1.05]
    "quadratic_inside": (lambda x: (x - 1.01) ** 2 + 3.0, 1e-4, 1.0, 10.0, 0.001),
    # decreasing up to the upper bound: the first bracket fails, the bounds are evaluated, the minimum sits at xmax
    "minimum_at_upper_bound": (lambda x: (x - 8.0) ** 2, 1e-4, 1.0, 3.0, 0.001),
    # ... and the same at the lower bound
    "minimum_at_lower_bound": (lambda x: (x + 2.0) ** 2, 0.5, 2.0, 6.0, 0.001),
    # skewed, the shape of a rate objective
    "skewed": (lambda x: 250.0 * (x - math.log(x)), 1e-4, 0.3, 12.0, 0.001),
    # the start is a narrow dip below everything Brent's steps see afterwards: the nearest one can get to "the final value
    # is worse than the start".  brent_opt replaces its best point only by a value <= the best so far, and that starts as
    # f(bx), so `*fx > fb` (optimization.cpp:332) cannot hold for any sequence of function values, NaN included: the
    # "if worse, return the initial value" rule is restated in the machine but is unreachable, here as in the reference
    "start_is_best": (lambda x: -5.0 if x == 1.0 else (x - 3.0) ** 2, 1e-4, 1.0, 6.0, 0.001),
    # the guess outside the bounds is clamped
    "clamped_guess": (lambda x: math.cosh(x - 2.5), 1.0, 0.2, 4.0, 0.01),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_brent_state_machine_follows_the_reference(pkg, name):
    func, xmin, xguess, xmax, tol = CASES[name]
    optx, fx, xs = em_ref.minimize_one_dimen(func, xmin, xguess, xmax, tol)
    (m_optx, m_fx, nevals), m_xs = run_machine(pkg, func, xmin, xguess, xmax, tol)
    assert m_xs == xs                       # the same points in the same order, bit for bit
    assert (m_optx, m_fx) == (optx, fx) and nevals == len(xs)
    bx = min(max(xguess, xmin), xmax)
    assert xs[0] == bx and len(xs) >= 3
    if name.startswith("minimum_at"):
        assert xmin in xs[3:5] or xmax in xs[3:5]            # the fall-back evaluated a bound
        bound = xmax if "upper" in name else xmin
        assert abs(optx - bound) <= 4 * tol * max(abs(bound), 1.0)
    if name == "start_is_best":
        assert optx == bx and fx == -5.0 and xs.count(bx) == 1 and len(xs) > 5
    if name == "quadratic_inside":
        assert abs(optx - 1.01) < 2e-3 and xmin not in xs and xmax not in xs


def test_brent_state_machine_refuses_bad_input(pkg):
    with pytest.raises(pkg.HostError):
        pkg.BrentStateMachine(2.0, 1.0, 1.0, 0.001)
    m = pkg.BrentStateMachine(0.1, 1.0, 2.0, 0.001)
    with pytest.raises(pkg.HostError):
        m.result()                                           # not finished


@pytest.mark.parametrize("k", [2, 4, 10])
def test_free_rate_start(pkg, k):
    props, rates = pkg.free_rate_start(k)
    assert props.shape == (k,) and np.all(props == 1.0 / k)
    assert np.array_equal(rates, pkg.gamma_rates(1.0, k))
    assert abs(float(np.dot(props, rates)) - 1.0) < 1e-12


def test_em_entry_points_refuse_without_a_device(pkg):
    lib = pkg.libiqhip()
    dp = C.POINTER(C.c_double)
    buf = np.zeros(64)
    cat = np.zeros(64, dtype=np.int32)
    d = buf.ctypes.data_as(dp)
    end = pkg.leaf_end(0)
    # null arguments
    assert lib.iqhip_em_posteriors(None, 0.1, d) == pkg.ERR_INVALID
    assert lib.iqhip_em_fetch_posteriors(None, d) == pkg.ERR_INVALID
    assert lib.iqhip_em_site_rates(None, d, cat.ctypes.data_as(C.POINTER(C.c_int32))) == pkg.ERR_INVALID
    assert lib.iqhip_em_objective(None, end, end, 0.1, d, None) == pkg.ERR_INVALID
    # a planning-only engine
    e = C.c_void_p()
    assert lib.iqhip_debug_create_planner(C.byref(e), 4, 4, 300, 8, 256, 18, 1) == 0, lib.iqhip_last_error()
    try:
        assert lib.iqhip_em_posteriors(e, 0.1, None) == pkg.ERR_INVALID
        assert lib.iqhip_em_posteriors(e, 0.1, d) == pkg.ERR_INVALID and b"planning-only" in lib.iqhip_last_error()
        assert lib.iqhip_em_fetch_posteriors(e, d) == pkg.ERR_INVALID and b"planning-only" in lib.iqhip_last_error()
        assert lib.iqhip_em_site_rates(e, d, cat.ctypes.data_as(C.POINTER(C.c_int32))) == pkg.ERR_INVALID
        assert lib.iqhip_em_site_rates(e, d, None) == pkg.ERR_INVALID
        assert lib.iqhip_em_objective(e, end, end, 0.1, d, None) == pkg.ERR_INVALID and b"planning-only" in lib.iqhip_last_error()
        assert lib.iqhip_em_objective(e, end, end, 0.1, None, None) == pkg.ERR_INVALID
    finally:
        lib.iqhip_destroy(e)


def test_cli_refuses_bare_free_rate_without_emrates(tmp_path):
    """a bare +R3 is accepted with -emrates only; without it the model producer's refusal stands (no device is touched:
    the model is parsed before the engine is created)"""
    tree = tmp_path / "t.nwk"
    tree.write_text("(a,b,c);\n")
    r = subprocess.run([BIN, "-s", EXAMPLE, "-te", str(tree), "-m", "HKY{2.0}+R3", "-pre", str(tmp_path / "x")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "+R needs its weights and rates" in r.stderr
    # -emrates without a +R component is refused as well
    r = subprocess.run([BIN, "-s", EXAMPLE, "-te", str(tree), "-m", "HKY{2.0}+G4{0.5}", "-emrates", "-pre", str(tmp_path / "x")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "-emrates needs a +R<k> model" in r.stderr
