"""Tree topology tests on the device (include/iqhip.h "tree topology tests"): iqhip_ptnlh_upload, the resampling
generator iqhip_gen_boot_samples, iqhip_ptnlh_diff_variance, iqhip_tree_tests and iqhip_multiscale_bp against the numpy
restatements of tests/test_tree_tests_host.py, and evaluateTrees end to end through the Python view and the command line.

The statistics are integer counts over S replicates; the restatement is fed the device's own RELL sums (iqhip_ptnlh_rell
on the same rows and samples) and the device's own variances, so every count must be EXACTLY equal."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from test_tree_tests_host import (MS_SAMPLES, MS_SCALES, MS_SEED, STREAM_RELL, asc_freq, multiscale_case, multiscale_truth,
                                  restate_diff_variance, restate_gen, restate_tree_tests, tie_uniforms, tree_rows)

pytestmark = pytest.mark.gpu

IQHIP_ERR_INVALID, IQHIP_ERR_UNSUPPORTED = 2, 3
HERE = os.path.dirname(os.path.abspath(__file__))
BIN = os.path.join(os.path.dirname(HERE), "iq-tree_amd", "lib", "iqhip_lnl")
EXAMPLE = os.path.join(HERE, "golden", "example.phy")
MODEL = "GTR{1.513,2.393,1.769,1.912,2.838}+F{0.249,0.262,0.251,0.238}+G4{0.934}"


def make_engine(pkg, synth, nptn, freq, seed=1, sharded=0):
    """a three-taxon DNA tree whose engine has nptn patterns of the given frequencies; the store is filled by upload"""
    rng = np.random.default_rng(seed)
    pat = rng.integers(0, 4, size=(3, nptn)).astype(np.uint8)
    t = pkg.PhyloTree("(0:0.1,1:0.2,2:0.3);")
    t.set_alignment(4, pkg.SEQ_DNA, pat, freq)
    t.set_model(synth.gtr_model(alpha=0.9, ncat=4))
    t.set_likelihood_kernel(pkg.LK_EIGEN_HIP)
    if sharded:
        t.attach_engine_sharded([0] * sharded, pkg.REDUCE_HOST)
    else:
        t.attach_engine(0)
    return t


def fetch_samples(t, nsamples):
    """the first nsamples rows of the sample matrix, read through the product with unit rows of the store (exact: every
    sum is one count times 1.0)"""
    if not getattr(t, "_unit_rows", False):
        eye = np.eye(t.nptn)
        t.ptnlh_reserve(t.nptn)
        for p in range(t.nptn):
            t.ptnlh_upload(p, eye[p])
        t._unit_rows = True
    return t.ptnlh_rell(np.arange(t.nptn), nsamples).T


# ---- upload ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nptn", [1, 63, 64, 65, 1000])
def test_upload_fetch_round_trip(pkg, synth, nptn):
    rng = np.random.default_rng(nptn)
    t = make_engine(pkg, synth, nptn, asc_freq(rng, nptn))
    t.ptnlh_reserve(3)
    rows = rng.uniform(-12.0, -1.0, size=(3, nptn))
    for r in (2, 0, 1):
        t.ptnlh_upload(r, rows[r])
    for r in range(3):
        np.testing.assert_array_equal(t.ptnlh_fetch(r), rows[r])
    t.ptnlh_upload(1, rows[2])                                   # a second upload replaces the row, its neighbours stay
    np.testing.assert_array_equal(t.ptnlh_fetch(1), rows[2])
    np.testing.assert_array_equal(t.ptnlh_fetch(0), rows[0])
    np.testing.assert_array_equal(t.ptnlh_fetch(2), rows[2])


# ---- generator ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nptn", [1, 63, 64, 65, 1000])
def test_generator_equals_restatement(pkg, synth, nptn):
    rng = np.random.default_rng(100 + nptn)
    freq = asc_freq(rng, nptn)
    nsite = int(freq.sum())
    t = make_engine(pkg, synth, nptn, freq)
    for ndraws in (1, round(0.5 * nsite), round(1.4 * nsite)):
        for first in (0, 5):
            t.gen_boot_samples(16, ndraws, 77, STREAM_RELL, first)
            got = fetch_samples(t, 16)
            want = restate_gen(freq, 16, first, ndraws, 77, STREAM_RELL)
            np.testing.assert_array_equal(got, want.astype(np.float64))
            assert got.sum(axis=1).tolist() == [ndraws] * 16    # every draw landed on a pattern, none on the padding
            assert not got[:, freq == 0].any()
    # [0, 16) at once equals [0, 5) then [5, 16); the same call twice gives the same matrix
    t.gen_boot_samples(16, nsite, 5, STREAM_RELL)
    whole = fetch_samples(t, 16)
    t.gen_boot_samples(16, nsite, 5, STREAM_RELL)
    np.testing.assert_array_equal(fetch_samples(t, 16), whole)
    t.gen_boot_samples(5, nsite, 5, STREAM_RELL)
    np.testing.assert_array_equal(fetch_samples(t, 5), whole[:5])
    t.gen_boot_samples(11, nsite, 5, STREAM_RELL, first_replicate=5)
    np.testing.assert_array_equal(fetch_samples(t, 11), whole[5:])


def test_generator_refusals(pkg, synth):
    lib = pkg.libiqhip()
    rng = np.random.default_rng(5)
    freq = asc_freq(rng, 65)
    t = make_engine(pkg, synth, 65, freq)
    assert lib.iqhip_gen_boot_samples(t.engine, 0, 0, 10, 1, 0) == IQHIP_ERR_INVALID
    assert lib.iqhip_gen_boot_samples(t.engine, 4, -1, 10, 1, 0) == IQHIP_ERR_INVALID
    assert lib.iqhip_gen_boot_samples(t.engine, 4, 0, (1 << 24) + 1, 1, 0) == IQHIP_ERR_INVALID
    assert lib.iqhip_gen_boot_samples(t.engine, 4, 0, 10, 1, 0) == 0
    bad = freq.copy()
    bad[3] = 1.5
    assert lib.iqhip_set_ptn_freq(t.engine, bad.ctypes.data_as(C.POINTER(C.c_double))) == 0
    assert lib.iqhip_gen_boot_samples(t.engine, 4, 0, 10, 1, 0) == IQHIP_ERR_INVALID
    assert b"integers" in lib.iqhip_last_error()
    bad[3] = -1.0
    assert lib.iqhip_set_ptn_freq(t.engine, bad.ctypes.data_as(C.POINTER(C.c_double))) == 0
    assert lib.iqhip_gen_boot_samples(t.engine, 4, 0, 10, 1, 0) == IQHIP_ERR_INVALID
    # new frequencies rebuild the prefix sums: all sites on pattern 7
    one = np.zeros(65)
    one[7] = 9.0
    assert lib.iqhip_set_ptn_freq(t.engine, one.ctypes.data_as(C.POINTER(C.c_double))) == 0
    t.gen_boot_samples(3, 20, 1)
    got = fetch_samples(t, 3)
    assert got[:, 7].tolist() == [20.0] * 3 and got.sum() == 60.0


# ---- variance ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nptn", [63, 1000])
@pytest.mark.parametrize("nrows", [2, 5, 17])
def test_diff_variance(pkg, synth, nrows, nptn):
    rng = np.random.default_rng(nrows * nptn)
    freq = asc_freq(rng, nptn)
    t = make_engine(pkg, synth, nptn, freq)
    L = tree_rows(rng, nrows, nptn, freq)
    if nrows > 2:
        L[-1] = L[0]                                            # two identical rows
    t.ptnlh_reserve(nrows)
    for r in range(nrows):
        t.ptnlh_upload(r, L[r])
    got = t.ptnlh_diff_variance(np.arange(nrows))
    want = restate_diff_variance(L, freq)
    # a sum of nptn non-negative terms has relative error at most nptn eps in any order; 64 x is headroom for the mean pass
    np.testing.assert_allclose(got, want, rtol=64 * nptn * 2.0 ** -53, atol=0)
    np.testing.assert_array_equal(got, got.T)
    assert not np.diag(got).any() and (got[0, nrows - 1] == 0.0) == (nrows > 2)
    # a list with a repeated row, in another order
    perm = np.array([nrows - 1, 0, 1, 1][:max(2, min(4, nrows + 1))])
    np.testing.assert_array_equal(t.ptnlh_diff_variance(perm), got[np.ix_(perm, perm)])


# ---- iqhip_tree_tests --------------------------------------------------------------------------------------------------
TT_SAMPLES = (1, 63, 64, 65, 257, 1000)
TT_SEED = 4711


@pytest.fixture(scope="module", params=[65, 700])
def tt_engine(request, pkg, synth):
    """70 store rows and 1000 generated samples; rows 0 and 1 are bit-identical"""
    nptn = request.param
    rng = np.random.default_rng(9000 + nptn)
    freq = asc_freq(rng, nptn)
    t = make_engine(pkg, synth, nptn, freq)
    L = tree_rows(rng, 70, nptn, freq)
    L[1] = L[0]
    t.ptnlh_reserve(70)
    for r in range(70):
        t.ptnlh_upload(r, L[r])
    t.gen_boot_samples(1000, int(freq.sum()), TT_SEED, STREAM_RELL)
    return t, L, freq


def tt_rows(ntrees, nptn):
    """the row list of a case: the identical pair (ties in BP, KH and in the choice of the second-best tree) except for
    the two-tree case of 700 patterns; from 17 trees on the last tree repeats store row 2"""
    if ntrees == 2:
        return np.array([0, 1] if nptn == 65 else [3, 4])
    rows = np.arange(ntrees)
    if ntrees >= 17:
        rows[-1] = 2
    return rows


@pytest.mark.parametrize("ntrees", [2, 3, 17, 70])
def test_tree_tests_equal_restatement(pkg, tt_engine, ntrees):
    t, L, freq = tt_engine
    rows = tt_rows(ntrees, t.nptn)
    lh = L[rows] @ freq                                          # rows 0 and 1: equal lnL
    if ntrees >= 3:
        lh[2] = lh.max()                                         # a third tree whose lnL equals the maximum
    var = t.ptnlh_diff_variance(rows)
    with np.errstate(divide="ignore"):
        weights = 1.0 / np.sqrt(var)
    np.fill_diagonal(weights, 0.0)
    for S in TT_SAMPLES:
        R = t.ptnlh_rell(rows, S)
        tie_u = tie_uniforms(TT_SEED + 1, ntrees, S)
        for eps in (0.0, 0.5):
            for weighted in (False, True):
                got = t.tree_tests(rows, lh, S, epsilon=eps, weighted=weighted, tie_seed=TT_SEED + 1)
                want = restate_tree_tests(R, lh, eps, weights if weighted else None, tie_u)
                tag = (ntrees, S, eps, weighted)
                for name, key in (("rell_bp", "bp"), ("kh_pvalue", "kh"), ("sh_pvalue", "sh"), ("wkh_pvalue", "wkh"),
                                  ("wsh_pvalue", "wsh")):
                    assert got[name].tolist() == want[key].tolist(), (tag, name)
                assert got["rell_confident"].tolist() == want["rell_confident"].tolist(), tag
                assert got["elw_confident"].tolist() == want["elw_confident"].tolist(), tag
                counts = got["rell_bp"] * S
                assert np.all(np.abs(counts - np.rint(counts)) < 1e-9) and int(np.rint(counts).sum()) == S, tag
                # device exp differs from libm by a few ulp per term, and the terms are at most 1
                assert np.all(np.abs(got["elw_value"] - want["elw"]) <= 1e-12), tag
                assert abs(got["elw_value"].sum() - 1.0) <= 1e-9, tag
                if not weighted:
                    assert np.all(got["wkh_pvalue"] == -1.0) and np.all(got["wsh_pvalue"] == -1.0)
    if t.nptn == 65 or ntrees >= 3:
        # the identical pair: with epsilon = 0 the later twin never wins a replicate
        twin = 1
        assert t.tree_tests(rows, lh, 1000, epsilon=0.0)["rell_bp"][twin] == 0.0
    # the same call twice: the same bits
    a = t.tree_tests(rows, lh, 257, epsilon=0.5, weighted=True, tie_seed=3)
    b = t.tree_tests(rows, lh, 257, epsilon=0.5, weighted=True, tie_seed=3)
    assert a.tobytes() == b.tobytes()


# ---- iqhip_multiscale_bp -----------------------------------------------------------------------------------------------
def test_multiscale_bp(pkg, synth, monkeypatch):
    L, freq = multiscale_case()
    t = make_engine(pkg, synth, 700, freq)
    t.ptnlh_reserve(17)
    for r in range(17):
        t.ptnlh_upload(r, L[r])
    counts, excluded = multiscale_truth(L, freq)
    print("excluded per scale:", excluded.tolist())
    assert np.all(excluded <= 0.01 * MS_SAMPLES)
    monkeypatch.delenv("IQHIP_BOOT_CHUNK", raising=False)
    bp = t.multiscale_bp(np.arange(17), MS_SCALES, MS_SAMPLES, MS_SEED)
    assert bp.shape == (3, 17)
    got = bp * MS_SAMPLES
    assert np.all(np.abs(got - np.rint(got)) < 1e-9)
    got = np.rint(got).astype(np.int64)
    assert got.sum(axis=1).tolist() == [MS_SAMPLES] * 3          # sum_tid bp[k] = 1, as a count
    for k in range(3):
        # the truth's counts leave the near-ties out: each count may differ by at most their number
        assert np.all(got[k] >= counts[k]) and np.all(got[k] - counts[k] <= excluded[k]), (k, got[k], counts[k])
    for chunk in ("7", "64", "300"):
        monkeypatch.setenv("IQHIP_BOOT_CHUNK", chunk)
        again = t.multiscale_bp(np.arange(17), MS_SCALES, MS_SAMPLES, MS_SEED)
        assert again.tobytes() == bp.tobytes(), chunk
    monkeypatch.delenv("IQHIP_BOOT_CHUNK")
    # a repeated row shares its twin's sums: the first of the two takes every replicate either wins
    rows = np.arange(17)
    rows[16] = 0
    dup = np.rint(t.multiscale_bp(rows, MS_SCALES, MS_SAMPLES, MS_SEED) * MS_SAMPLES)
    assert not dup[:, 16].any() and dup.sum(axis=1).tolist() == [MS_SAMPLES] * 3


# ---- consistency with the uploaded-sample route -------------------------------------------------------------------------
def test_generated_samples_serve_the_older_calls(pkg, synth, oracle):
    from test_branch_tests_gpu import make_case
    t, okw, freq = make_case(synth, oracle, pkg, 4, 4, 0, 8, 400, 9100)
    nsite = int(freq.sum())
    t.compute_likelihood()
    row0 = t.compute_pattern_likelihood()
    nb = len(t.evaluate_nnis5_batch(first_row=1)) // 2           # rows 1 .. 2 nb: the NNI neighbours
    t.ptnlh_upload(0, row0)
    rows3 = np.array([[0, 1 + 2 * q, 2 + 2 * q] for q in range(nb)])
    lh3 = np.array([[t.ptnlh_fetch(r) @ freq for r in row] for row in rows3])
    t.gen_boot_samples(100, nsite, 31, STREAM_RELL)
    gen_bt = t.branch_tests(rows3, lh3, 100, 80)
    t.compute_likelihood()
    gen_rell = t.compute_rell()
    gen_R = t.ptnlh_rell(np.arange(1 + 2 * nb), 100)
    t.set_boot_samples(restate_gen(freq, 100, 0, nsite, 31, STREAM_RELL).astype(np.float32))
    np.testing.assert_array_equal(t.branch_tests(rows3, lh3, 100, 80), gen_bt)
    np.testing.assert_array_equal(t.compute_rell(), gen_rell)
    np.testing.assert_array_equal(t.ptnlh_rell(np.arange(1 + 2 * nb), 100), gen_R)
    assert gen_rell.shape == (100,) and np.all(gen_rell < 0.0)


# ---- refusals ----------------------------------------------------------------------------------------------------------
def call_all_five(pkg, t, rows, ntrees, nsamples, scale=1.0):
    lib = pkg.libiqhip()
    buf = np.zeros(max(t.nptn, 64 * 64))
    dp = buf.ctypes.data_as(C.POINTER(C.c_double))
    r = np.asarray(rows, dtype=np.int32)
    ip = r.ctypes.data_as(C.POINTER(C.c_int32))
    lh = np.linspace(-100.0, -101.0, max(ntrees, 1))
    sc = np.array([scale])
    res = (pkg.TreeTest * max(ntrees, 1))()
    return dict(upload=lib.iqhip_ptnlh_upload(t.engine, int(r[0]), dp),
                gen=lib.iqhip_gen_boot_samples(t.engine, 8, 0, 50, 1, STREAM_RELL),
                variance=lib.iqhip_ptnlh_diff_variance(t.engine, ip, ntrees, dp),
                tests=lib.iqhip_tree_tests(t.engine, ip, lh.ctypes.data_as(C.POINTER(C.c_double)), ntrees, nsamples, 0.5, 1, 1,
                                           res),
                multiscale=lib.iqhip_multiscale_bp(t.engine, ip, ntrees, sc.ctypes.data_as(C.POINTER(C.c_double)), 1, 8, 1, dp))


def test_sharded_engine_is_unsupported(pkg, synth):
    rng = np.random.default_rng(2)
    t = make_engine(pkg, synth, 700, asc_freq(rng, 700), sharded=2)
    assert pkg.libiqhip().iqhip_num_shards(t.engine) == 2
    rc = call_all_five(pkg, t, [0, 1, 2], 3, 8)
    assert set(rc.values()) == {IQHIP_ERR_UNSUPPORTED}, rc


def test_invalid_arguments(pkg, synth):
    rng = np.random.default_rng(3)
    freq = asc_freq(rng, 65)
    t = make_engine(pkg, synth, 65, freq)
    t.ptnlh_reserve(4)
    L = tree_rows(rng, 4, 65, freq)
    for r in range(4):
        t.ptnlh_upload(r, L[r])
    ok = call_all_five(pkg, t, [0, 1, 2], 3, 8)
    assert set(ok.values()) == {0}, ok
    for bad in ([4, 1, 2], [-1, 1, 2]):                          # a row outside the store
        rc = call_all_five(pkg, t, bad, 3, 8)
        assert rc["upload"] == rc["variance"] == rc["tests"] == rc["multiscale"] == IQHIP_ERR_INVALID, rc
    rc = call_all_five(pkg, t, [2, 1, 0], 3, 8)
    assert set(rc.values()) == {0}
    rc = call_all_five(pkg, t, [0, 1, 2], 1, 8)                   # one tree is no test
    assert rc["tests"] == rc["multiscale"] == IQHIP_ERR_INVALID and rc["variance"] == 0
    rc = call_all_five(pkg, t, [0, 1, 2], 3, 9)                   # more replicates than the matrix holds
    assert rc["tests"] == IQHIP_ERR_INVALID and rc["multiscale"] == 0
    assert call_all_five(pkg, t, [0, 1, 2], 3, 0)["tests"] == IQHIP_ERR_INVALID
    for scale in (0.0, -1.0, float("nan")):
        assert call_all_five(pkg, t, [0, 1, 2], 3, 8, scale=scale)["multiscale"] == IQHIP_ERR_INVALID
    assert set(call_all_five(pkg, t, [0, 1, 2], 3, 8).values()) == {0}       # the engine still works


# ---- end to end --------------------------------------------------------------------------------------------------------
def named_tree(nwk, names):
    return re.sub(r"([(,])(\d+):", lambda m: "%s%s:" % (m.group(1), names[int(m.group(2))]), nwk)


def run_cli(args):
    r = subprocess.run([BIN] + args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr + r.stdout
    return r.stdout


def test_evaluate_trees_python_and_command_line(pkg, synth, tmp_path):
    aln = pkg.Alignment(EXAMPLE)
    st, fr, _, _ = aln.arrays()
    model = aln.build_model(MODEL)
    newicks = [synth.random_tree_newick(44, s) for s in (12, 13, 14)]
    t = pkg.PhyloTree(newicks[0])
    t.set_alignment(4, 0, st, fr)
    t.set_model(model)
    t.attach_engine(0)
    res, au = t.evaluate_trees(newicks, 200, weighted=True, au_scales=pkg.AU_SCALES, seed=3)
    assert len(res) == 3 and au.shape == (10, 3)
    assert abs(res["rell_bp"].sum() - 1.0) < 1e-12 and abs(res["elw_value"].sum() - 1.0) < 1e-9
    assert np.all(np.abs(au.sum(axis=1) - 1.0) < 1e-12)
    for f in ("kh_pvalue", "sh_pvalue", "wkh_pvalue", "wsh_pvalue"):
        assert np.all((res[f] >= 0.0) & (res[f] <= 1.0))
    assert res["rell_confident"].any() and res["elw_confident"].any()
    # store row tid holds tree tid's per-pattern lnL
    for tid in range(3):
        assert abs(t.ptnlh_fetch(tid) @ fr - res["logl"][tid]) <= 1e-9 * abs(res["logl"][tid])
    # the command line on the same trees
    zf = tmp_path / "set.nwk"
    zf.write_text("".join(named_tree(n, aln.seq_names) + "\n" for n in newicks))
    tfs = []
    for k, n in enumerate(newicks):
        tf = tmp_path / ("t%d.nwk" % k)
        tf.write_text(named_tree(n, aln.seq_names) + "\n")
        tfs.append(tf)
    out = run_cli(["-s", EXAMPLE, "-te", str(tfs[0]), "-m", MODEL, "-pre", str(tmp_path / "z"), "-z", str(zf), "-zb", "200",
                   "-zw", "-au", "-seed", "3"])
    rows = [ln.split() for ln in out.splitlines() if ln.startswith("TOPOTEST")]
    assert [int(r[1]) for r in rows] == [1, 2, 3] and all(len(r) == 15 for r in rows)
    fields = ("rell_bp", "kh_pvalue", "sh_pvalue", "wkh_pvalue", "wsh_pvalue", "elw_value")
    for tid, r in enumerate(rows):
        assert r[2] == "%.6f" % res["logl"][tid]
        for k, f in enumerate(fields):
            assert r[3 + 2 * k] == "%.4f" % res[f][tid], (tid, f)
            assert r[4 + 2 * k] in "+-"
        assert r[4] == "-+"[int(res["rell_confident"][tid])] and r[14] == "-+"[int(res["elw_confident"][tid])]
        assert r[6] == "+-"[int(res["kh_pvalue"][tid] < 0.05)]
    scale_line = [ln.split() for ln in out.splitlines() if ln.startswith("AUSCALE")]
    assert [float(x) for x in scale_line[0][2:]] == list(pkg.AU_SCALES)
    aubp = [ln.split() for ln in out.splitlines() if ln.startswith("AUBP")]
    assert len(aubp) == 3
    for tid, r in enumerate(aubp):
        assert r[2:] == ["%.4f" % x for x in au[:, tid]]
    # logL per tree equals a separate -te run of that tree (the -z run itself evaluated the first one as its -te tree)
    def report_lnl(prefix):
        return [float(ln.split()[1]) for ln in open(prefix + ".iqhip") if ln.startswith("lnL ")][0]

    assert "%.6f" % report_lnl(str(tmp_path / "z")) == rows[0][2]
    for tid in (1, 2):
        pre = str(tmp_path / ("s%d" % tid))
        run_cli(["-s", EXAMPLE, "-te", str(tfs[tid]), "-m", MODEL, "-pre", pre])
        assert "%.6f" % report_lnl(pre) == rows[tid][2]
