"""CPU: the host half of the model-parameter estimation.
  1. BfgsStateMachine (bfgs_host.h) against tests/bfgs_ref.py, the direct restatement of derivativeFunk / lnsrch / dfpmin /
     minimizeMultiDimen: on five analytic functions the machine requests the SAME POINTS IN THE SAME ORDER, bit for bit, and
     returns the same minimum, value and iteration count.
  2. the shape of the requests: a stencil is the base point plus its ndim forward points with h = (x + h) - x.
  3. bound_check = true is refused.
  4. parameter counts, bounds and candidates per traversal per model name (model_opt_describe).
  5. refusals that need no device: iqhip_class_lnl with null arguments; the optimiser / -optmodel with MIX{}, +R, +ASC, +FO;
     a brace-less string without -optmodel.
  6. tests/modelopt_ref.py on a small problem: the restated run ends in the interior and does not lower the likelihood."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import bfgs_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "iq-tree_amd", "lib", "iqhip_lnl")
EXAMPLE = os.path.join(ROOT, "tests", "golden", "example.phy")


def bowl5(x):
    return sum((i + 1) * (x[i] - 0.3 * (i + 1)) ** 2 for i in range(5))


def rosenbrock(x):
    return 100.0 * (x[1] - x[0] ** 2) ** 2 + (1.0 - x[0]) ** 2


def beyond_bound(x):
    return (x[0] - 3.0) ** 2 + (x[1] + 1.0) ** 2


def with_zero(x):
    return (x[0] - 1.0) ** 2 + (x[1] - 2.0) ** 2 + 0.1 * x[0] * x[1]


# name: (function, start, lower, upper)
FUNCTIONS = {
    "bowl5": (bowl5, [1.0] * 5, [-10.0] * 5, [10.0] * 5),
    "rosenbrock": (rosenbrock, [-1.2, 1.0], [-5.0, -5.0], [5.0, 5.0]),
    "beyond_upper_bound": (beyond_bound, [0.5, 0.5], [0.0, -2.0], [2.0, 2.0]),       # the minimum (3, -1) lies beyond x0 <= 2
    "started_at_minimum": (bowl5, [0.3 * (i + 1) for i in range(5)], [-10.0] * 5, [10.0] * 5),
    "zero_coordinate": (with_zero, [0.0, 1.0], [-5.0, -5.0], [5.0, 5.0]),            # h falls back to ERROR_X
}


def run_machine(pkg, f, x0, lo, up, gtol):
    m = pkg.BfgsStateMachine(x0, lo, up, gtol)
    points, kinds = [], []
    while not m.done:
        kinds.append((m.kind, None if m.steps is None else m.steps.copy(), m.points.copy()))
        points += [list(p) for p in m.points]
        m.update([f(list(p)) for p in m.points])
    return m.result(), points, kinds


@pytest.mark.parametrize("name", sorted(FUNCTIONS))
def test_machine_requests_the_reference_points(pkg, name):
    f, x0, lo, up = FUNCTIONS[name]
    gtol = 1e-4
    asked = []

    def target(x):
        asked.append(list(x))
        return f(x)

    grads = []
    ref = bfgs_ref.minimize_multi_dimen(target, x0, lo, up, [False] * len(x0), gtol, grads)
    res, points, kinds = run_machine(pkg, f, x0, lo, up, gtol)
    print("%s: %d evaluations, %d iterations, minimum %s value %.6e" % (name, len(asked), ref["iter"], ref["x"], ref["fret"]))
    assert len(points) == len(asked)
    assert points == asked                                   # the same points in the same order, bit for bit
    assert list(res["x"]) == ref["x"] and res["fret"] == ref["fret"] and res["iter"] == ref["iter"]
    assert list(res["gradient"]) == grads[-1]
    assert res["stencils"] == len(grads) and res["stencils"] + res["singles"] == len(kinds)
    n = len(x0)
    for kind, steps, pts in kinds:
        if kind == "stencil":                                 # the base point and its ndim forward points
            assert pts.shape == (n + 1, n)
            for d in range(n):
                expect = pts[0].copy()
                h = bfgs_ref.ERROR_X * abs(expect[d]) or bfgs_ref.ERROR_X
                expect[d] = expect[d] + h
                assert np.array_equal(pts[1 + d], expect) and steps[d] == expect[d] - pts[0][d]
        else:                                                 # a line-search point, inside the bounds
            assert kind == "single" and pts.shape == (1, n)
            assert np.all(pts[0] >= lo) and np.all(pts[0] <= up)
    if name == "beyond_upper_bound":
        assert res["x"][0] == 2.0 and abs(res["x"][1] + 1.0) < 1e-3      # fixBound clamps
    if name == "started_at_minimum":
        assert res["iter"] == 1 and np.allclose(res["x"], x0, rtol=0, atol=1e-6)
    if name == "zero_coordinate":
        assert kinds[0][1][0] == bfgs_ref.ERROR_X
    if name in ("bowl5", "zero_coordinate"):
        assert res["fret"] < f(x0) - 0.1


def test_machine_refuses_bound_check(pkg):
    with pytest.raises(pkg.HostError, match="bound_check"):
        pkg.BfgsStateMachine([1.0, 1.0], [0.0, 0.0], [2.0, 2.0], 1e-4, bound_check=[False, True])
    with pytest.raises(ValueError):
        bfgs_ref.minimize_multi_dimen(bowl5, [1.0] * 5, [-1.0] * 5, [1.0] * 5, [True] * 5, 1e-4)
    m = pkg.BfgsStateMachine([1.0], [0.0], [2.0], 1e-4, bound_check=[False])
    assert m.kind == "stencil" and m.points.shape == (2, 1)
    with pytest.raises(pkg.HostError, match="one value per requested point"):
        m.update([1.0])
    with pytest.raises(pkg.HostError):
        pkg.BfgsStateMachine([1.0], [2.0], [0.0], 1e-4)      # lower > upper


@pytest.mark.parametrize("model,ndim,K", [("JC", 0, 1), ("F81+G4", 0, 1), ("K80", 1, 2), ("HKY+G4", 1, 2), ("TN+I+G4", 2, 3),
                                          ("GTR", 5, 6), ("GTR+G4", 5, 6), ("GTR+I+G4{0.5}", 5, 6), ("GTR+G8", 5, 4),
                                          ("GTR{1,2,3,4,5}+F{0.1,0.2,0.3,0.4}+I{0.1}+G4", 5, 6)])
def test_parameter_counts_and_bounds(pkg, model, ndim, K):
    d = pkg.model_opt_describe(model, 4)
    assert d["ndim"] == ndim and d["K"] == K                 # K = min(ndim + 1, 32 / C)
    assert (d["lower"], d["upper"]) == (1e-4, 100.0)         # MIN_RATE, MAX_RATE
    assert d["alpha_bounds"] == (0.02, 1000.0) and d["pinv_lower"] == 1e-6
    assert d["has_gamma"] == ("+G" in model) and d["has_invar"] == ("+I" in model)


def test_protein_models_have_no_rate_parameters(pkg):
    d = pkg.model_opt_describe("POISSON+I+G4", 20)
    assert d["ndim"] == 0 and d["has_gamma"] and d["has_invar"]
    assert pkg.model_opt_describe("some_matrix.paml+G4", 20)["ndim"] == 0     # a PAML file (not opened here)


@pytest.mark.parametrize("model,word", [("MIX{JC,HKY}+G4", "MIX"), ("GTR+R3{0.2,0.5,0.3,1.0,0.5,1.2}", "+R"), ("GTR+R3", "+R"),
                                        ("GTR+G4+ASC", "ASC"), ("GTR+FO+G4", "+FO")])
def test_optimiser_refusals(pkg, model, word):
    with pytest.raises(pkg.HostError, match=word.replace("+", r"\+").replace("{", r"\{")):
        pkg.model_opt_describe(model, 4)


def cli(*args):
    return subprocess.run([BIN] + list(args), capture_output=True, text=True)


@pytest.mark.parametrize("model", ["MIX{JC,HKY{2.0}}+G4{0.5}", "GTR+R3{0.2,0.5,0.3,1.0,0.5,1.2}", "GTR+G4+ASC", "GTR+FO+G4"])
def test_cli_optmodel_refusals(tmp_path, model):
    tree = tmp_path / "t.nwk"
    tree.write_text("(a,b,c);")                              # (never read: the model is refused first)
    r = cli("-s", EXAMPLE, "-te", str(tree), "-m", model, "-optmodel", "-pre", str(tmp_path / "x"))
    assert r.returncode == 2 and "not supported" in r.stderr, (r.stdout, r.stderr)


@pytest.mark.parametrize("model,word", [("GTR+G4{0.5}", "expects 5 rate parameter"), ("HKY{2.0}+G4", "+G needs a shape"),
                                        ("JC+I", "+I needs a value")])
def test_cli_refuses_missing_values_without_optmodel(tmp_path, model, word):
    tree = tmp_path / "t.nwk"
    tree.write_text("(a,b,c);")
    r = cli("-s", EXAMPLE, "-te", str(tree), "-m", model, "-pre", str(tmp_path / "x"))
    assert r.returncode == 2 and word in r.stderr, (r.stdout, r.stderr)


def test_class_lnl_refusals_without_a_device(pkg):
    lib = pkg.libiqhip()
    assert "iqhip_class_lnl" in pkg.IQHIP_SYMBOLS and "iqhip_debug_class_lnl_timing" in pkg.IQHIP_SYMBOLS
    dp = C.POINTER(C.c_double)
    one = np.ones(1)
    be = pkg.BranchEnd(0, 0, 0)
    assert lib.iqhip_class_lnl(None, be, be, 0.1, one.ctypes.data_as(dp), None, one.ctypes.data_as(dp), None) == pkg.ERR_INVALID
    assert b"null argument" in lib.iqhip_last_error()
    assert lib.iqhip_debug_class_lnl_timing(None, one.ctypes.data_as(dp)) == pkg.ERR_INVALID
    # a planning-only engine
    eng = C.c_void_p()
    assert lib.iqhip_debug_create_planner(C.byref(eng), 4, 4, 100, 6, 256, 18, 1) == 0, lib.iqhip_last_error()
    assert lib.iqhip_class_lnl(eng, be, be, 0.1, one.ctypes.data_as(dp), None, one.ctypes.data_as(dp), None) == pkg.ERR_INVALID
    assert b"planning-only" in lib.iqhip_last_error()
    lib.iqhip_destroy(eng)
    assert lib.iqhip_abi_version() == 2


def test_restated_optimiser_on_a_small_problem(synth, oracle):
    """modelopt_ref on 6 taxa x 300 sites of GTR+G4 data from rates 1, alpha 1: interior end, likelihood gained"""
    import modelopt_ref
    truth = synth.gtr_model(alpha=0.6, ncat=4)
    nwk = synth.random_tree_newick(6, 31, 0.05, 0.3)
    st = synth.simulate_alignment(nwk, truth, 300, 32, 0.0, 18)
    pat, freq = synth.compress_patterns(st)
    ot = oracle.OracleTree(nwk, 4, 0, pat, freq, None, truth)
    pb = modelopt_ref.Problem(synth, ot.adj, pat, freq, 0, 18, modelopt_ref.gtr_exch, truth.freqs, 4, True, False, 0.0)
    start = pb.lnl([1.0] * 5, 1.0, 0.0)
    res = modelopt_ref.optimize_parameters(pb, [1.0] * 5, 1.0, 0.0)
    print("start %.4f end %.4f rounds %d params %s alpha %.4f, %d likelihood evaluations" % (start, res["lnl"], res["rounds"],
                                                                                         res["params"], res["alpha"], pb.evaluations))
    assert res["lnl"] > start + 1.0
    for k in range(1, len(res["trace"])):
        assert res["trace"][k] >= res["trace"][k - 1] - 1e-6
    for p in res["params"]:
        assert 1e-4 + 1e-4 < p < 100.0 - 1e-4
    assert 0.02 + 1e-4 < res["alpha"] < 1000.0 - 1e-4
