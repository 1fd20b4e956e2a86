"""BIONJ on the device (include/iqhip.h "BIONJ"): iqhip_bionj against the fp64 restatement of tests/bionj_ref.py (equal
pairs, numbers to 1e-12) and against the reference's recorded trees (tests/golden/bionj_cases.json), a separate variance
matrix, an asymmetric input, bit-identical repeats, the refusals, and PhyloTree.compute_bionj / `iqhip_lnl -bionjtree`
end to end.

The sizes 3, 4, 5, 8, 24, 65, 130, 257 cover no merge, one merge, pairs inside one workgroup, pairs over many workgroups
and rows across the 256 threads of a workgroup.  The device differs from the restatement only in the order of its sums
(the kernels are built without contraction), so the tolerance is 1000 x the spread tests/test_bionj_host.py asserts
between two summation orders of the restatement.  A guard rejects an input where some Q lies within 1e-9 of the pair
threshold m + 1e-6, where a rounding difference could legitimately move a pair across it; the listed seeds trip it
nowhere, and a test asserts that."""
import ctypes as C
import functools
import math
import os
import re
import subprocess

import numpy as np
import pytest

import bionj_ref as br
from test_bionj_host import GOLDEN, GOLDEN_LENGTH_TOL, ORDER_SPREAD_BOUND, golden_case

pytestmark = pytest.mark.gpu

IQHIP_ERR_INVALID, IQHIP_ERR_UNSUPPORTED = 2, 3
HERE = os.path.dirname(os.path.abspath(__file__))
BIN = os.path.join(os.path.dirname(HERE), "iq-tree_amd", "lib", "iqhip_lnl")
EXAMPLE = os.path.join(HERE, "golden", "example.phy")
MODEL = "GTR{1.513,2.393,1.769,1.912,2.838}+F{0.249,0.262,0.251,0.238}+G4{0.934}"   # as tests/test_pair_dist_gpu.py
DEVICE_TOL = 1000 * ORDER_SPREAD_BOUND   # 1e-12, absolute
GUARD = 1e-9
CASES = [("uniform", n) for n in (3, 4, 5, 8, 24, 65, 130, 257)] + [("duplicates", n) for n in (9, 24, 130)]
DP, I32P = C.POINTER(C.c_double), C.POINTER(C.c_int32)


def case_matrix(kind, n):
    return br.uniform_matrix(n, 1) if kind == "uniform" else br.duplicates_matrix(n)


@functools.lru_cache(maxsize=None)
def restated(kind, n):
    return br.bionj(case_matrix(kind, n))


def small_tree(pkg, synth, sharded=0):
    rng = np.random.default_rng(2)
    states = rng.integers(0, 4, size=(5, 200)).astype(np.uint8)   # (a shard holds at least 64 patterns)
    t = pkg.PhyloTree(synth.random_tree_newick(5, 1))
    t.set_alignment(4, 0, states, np.ones(200))
    t.set_model(synth.gtr_model())
    t.set_likelihood_kernel(pkg.LK_EIGEN_HIP)
    if sharded:
        t.attach_engine_sharded([0] * sharded, pkg.REDUCE_HOST)
    else:
        t.attach_engine(0)
    return t


@pytest.fixture(scope="module")
def eng(pkg, synth):
    """the engine supplies the device and the stream only: its own 5 taxa have nothing to do with n"""
    t = small_tree(pkg, synth)
    yield t
    t.close()


def assert_log_matches(got, want, tol):
    steps, last, last_len = got
    assert [(int(s["a"]), int(s["b"])) for s in steps] == [s[:2] for s in want["steps"]]
    assert list(last) == want["last"]
    worst = 0.0
    for s, w in zip(steps, want["steps"]):
        worst = max(worst, abs(s["la"] - w[2]), abs(s["lb"] - w[3]), abs(s["lambda"] - w[4]))
    worst = max([worst] + [abs(a - b) for a, b in zip(last_len, want["last_len"])])
    print("largest difference of la, lb, lambda, final lengths: %.3e" % worst)
    assert worst <= tol
    return worst


def test_the_guard_rejects_no_input():
    for kind, n in CASES:
        r = restated(kind, n)
        assert not r["guard"] or min(r["guard"]) >= GUARD, (kind, n)
        assert len(r["steps"]) == n - 3


@pytest.mark.parametrize("kind,n", CASES)
def test_device_matches_the_restatement(eng, kind, n):
    want = restated(kind, n)
    assert not want["guard"] or min(want["guard"]) >= GUARD
    got = eng.bionj(case_matrix(kind, n))
    assert got[0].dtype.itemsize == 32 and len(got[0]) == n - 3
    assert_log_matches(got, want, DEVICE_TOL)
    for s in got[0]:
        assert s["a"] > s["b"] and 0.0 <= s["lambda"] <= 1.0
    if kind == "duplicates":   # V_ab == 0 between duplicates: the lambda = 0.5 branch ran
        assert any(s["lambda"] == 0.5 for s in got[0])
    ms, launches = eng.bionj_timing()
    assert ms == 0.0 and launches == (3 if n == 3 else 4 * (n - 3) + 3)


def test_separate_variance_matrix(eng):
    n = 24
    D, V = br.uniform_matrix(n, 1), br.uniform_matrix(n, 2)
    want = br.bionj(D, var=V)
    assert min(want["guard"]) >= GUARD
    got = eng.bionj(D, V)
    assert_log_matches(got, want, DEVICE_TOL)
    plain = eng.bionj(D)
    assert not np.array_equal(got[0]["lambda"], plain[0]["lambda"])


def test_asymmetric_input_equals_its_symmetrised_form(eng):
    n = 24
    rng = np.random.default_rng(7)
    A = rng.uniform(0.05, 1, (n, n))
    A[np.arange(n), np.arange(n)] = rng.uniform(1, 2, n)   # (the diagonal is ignored)
    got, sym = eng.bionj(A), eng.bionj(br.symmetrise(A))
    for x, y in zip(got, sym):
        assert x.tobytes() == y.tobytes()
    want = br.bionj(A)
    assert min(want["guard"]) >= GUARD
    assert_log_matches(got, want, DEVICE_TOL)


def test_two_calls_are_bit_identical(eng):
    D = br.uniform_matrix(257, 1)
    first, second = eng.bionj(D), eng.bionj(D)
    for x, y in zip(first, second):
        assert x.tobytes() == y.tobytes()


def test_device_gives_the_recorded_trees(eng):
    worst = 0.0
    for case in GOLDEN:
        names, D, want = golden_case(case)
        steps, last, last_len = eng.bionj(D)
        log = [(int(s["a"]), int(s["b"]), float(s["la"]), float(s["lb"]), float(s["lambda"])) for s in steps]
        d = br.max_split_diff(br.log_splits(log, last, last_len, len(names)), want)
        print("%-22s max |length - reference| %.3e" % (case["name"], d))
        worst = max(worst, d)
    assert worst <= GOLDEN_LENGTH_TOL


def raw_bionj(lib, engine, n, dist):
    steps = np.zeros(max(1, n), dtype=np.dtype([("x", np.float64, (4,))]))
    last, last_len = np.zeros(3, dtype=np.int32), np.zeros(3)
    return lib.iqhip_bionj(engine, n, None if dist is None else dist.ctypes.data_as(DP), None, steps.ctypes.data_as(C.c_void_p),
                           last.ctypes.data_as(I32P), last_len.ctypes.data_as(DP))


def test_refusals(pkg, synth, eng):
    lib = pkg.libiqhip()
    D = br.uniform_matrix(5, 1)
    assert raw_bionj(lib, eng.engine, 2, D) == IQHIP_ERR_INVALID and b"3 taxa" in lib.iqhip_last_error()
    assert raw_bionj(lib, eng.engine, 5, None) == IQHIP_ERR_INVALID and b"null" in lib.iqhip_last_error()
    bad = D.copy()
    bad[3, 1] = math.nan
    assert raw_bionj(lib, eng.engine, 5, bad) == IQHIP_ERR_INVALID and b"finite" in lib.iqhip_last_error()
    with pytest.raises(pkg.EngineError) as err:
        eng.bionj(bad)
    assert err.value.code == IQHIP_ERR_INVALID
    # sharded engine
    t = small_tree(pkg, synth, sharded=2)
    assert raw_bionj(lib, t.engine, 5, D) == IQHIP_ERR_UNSUPPORTED and b"sharded" in lib.iqhip_last_error()
    t.close()
    # planning-only engine
    e = C.c_void_p()
    assert lib.iqhip_debug_create_planner(C.byref(e), 4, 4, 1000, 8, 256, 18, 1) == 0
    assert raw_bionj(lib, e, 5, D) == IQHIP_ERR_INVALID and b"planning-only" in lib.iqhip_last_error()
    lib.iqhip_destroy(e)
    # and the engine still works
    assert_log_matches(eng.bionj(D), br.bionj(D), DEVICE_TOL)


# ------------------------------------------------------------------------------------------
# end to end
# ------------------------------------------------------------------------------------------
def test_compute_bionj_python_and_command_line(pkg, synth, tmp_path):
    aln = pkg.Alignment(EXAMPLE)
    st, fr, _, _ = aln.arrays()
    model = aln.build_model(MODEL)
    T = st.shape[0]
    t = pkg.PhyloTree(synth.random_tree_newick(T, 12))
    t.set_alignment(4, 0, st, fr)
    t.set_model(model)
    t.set_likelihood_kernel(pkg.LK_EIGEN_HIP)
    t.attach_engine(0)
    ids = [str(i) for i in range(T)]
    nwk0, steps0, _, _ = t.compute_bionj()            # distances first, then the tree
    dist = t.compute_dist()
    nwk, steps, last, last_len = t.compute_bionj(dist)
    assert nwk == nwk0 and steps.tobytes() == steps0.tobytes()
    assert t.num_leaves == T and t.num_nodes == 2 * T - 2
    want = br.bionj(dist)
    assert min(want["guard"]) >= GUARD
    assert_log_matches((steps, last, last_len), want, DEVICE_TOL)
    want_splits = br.log_splits(want["steps"], want["last"], want["last_len"], T)
    assert br.max_split_diff(br.newick_splits(nwk, ids), want_splits) <= 0.5e-8 + DEVICE_TOL   # (%10.8f)
    assert set(br.newick_splits(t.tree_string(), ids)) == set(want_splits)   # the tree in place is that tree
    t.fix_negative_branch(False)
    assert math.isfinite(t.compute_likelihood())
    t.close()

    names = aln.seq_names
    pre = tmp_path / "x"
    r = subprocess.run([BIN, "-s", EXAMPLE, "-bionjtree", "-m", MODEL, "-pre", str(pre)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr + r.stdout
    mldist, bionj = tmp_path / "x.mldist", tmp_path / "x.bionj"
    assert mldist.exists() and bionj.exists()
    fnames, fdist = br.parse_matrix_text(mldist.read_text())
    assert fnames == list(names)
    fwant = br.bionj(fdist)
    assert min(fwant["guard"]) >= GUARD
    fsplits = br.log_splits(fwant["steps"], fwant["last"], fwant["last_len"], T)
    assert br.max_split_diff(br.newick_splits(bionj.read_text(), names), fsplits) <= 0.5e-8 + DEVICE_TOL
    assert re.search(r"BIONJ tree: [0-9.]+ s, printed to %s\.bionj" % re.escape(str(pre)), r.stdout), r.stdout
    assert re.search(r"^\d+ negative branch lengths fixed$", r.stdout, re.M), r.stdout
    m = re.search(r"Log-likelihood after branch-length optimisation: (\S+)", r.stdout)
    assert m and math.isfinite(float(m.group(1))) and float(m.group(1)) < 0.0, r.stdout
    # -bionjtree excludes -te and -parstree
    for extra in (["-te", str(bionj)], ["-parstree"]):
        r = subprocess.run([BIN, "-s", EXAMPLE, "-bionjtree", "-m", MODEL, "-pre", str(pre)] + extra, capture_output=True,
                           text=True, timeout=60)
        assert r.returncode == 2 and "usage" in r.stderr
