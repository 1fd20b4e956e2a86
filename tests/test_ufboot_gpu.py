"""UFBoot bookkeeping on the device (include/iqhip.h "ultrafast bootstrap"): iqhip_ufboot_init / update / fetch against
the numpy restatement of IQTree::saveCurrentTree's rule (tests/ufboot_ref.py).

Exact cases: rows of small negative integers times samples of small integer counts -- every RELL sum is an exact integer
in any summation order, so the device state must equal the restatement BIT FOR BIT, whatever the chunking.
Real rows: the state must be bit-identical to the restatement fed with the device's own sums (iqhip_ptnlh_rell at the same
nsamples), and equal to the restatement fed with the numpy float64 product wherever no comparison sits within the
product's error bound of its threshold."""
import ctypes as C

import numpy as np
import pytest

import ufboot_ref as ref

pytestmark = pytest.mark.gpu

IQHIP_ERR_INVALID, IQHIP_ERR_UNSUPPORTED = 2, 3
NROWS, NSAMPLES = 12, 257


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def assert_state_equal(got, want, what=""):
    for f in ("boot_tree", "boot_counts"):
        np.testing.assert_array_equal(got[f], want[f], err_msg="%s %s" % (f, what))
    for f in ("boot_logl", "boot_orig_logl"):
        np.testing.assert_array_equal(bits(got[f]), bits(want[f]), err_msg="%s %s" % (f, what))


def make_engine(pkg, synth, nptn, sharded=0):
    rng = np.random.default_rng(nptn)
    pat = rng.integers(0, 4, size=(3, nptn)).astype(np.uint8)
    t = pkg.PhyloTree("(0:0.1,1:0.2,2:0.3);")
    t.set_alignment(4, pkg.SEQ_DNA, pat, np.ones(nptn))
    t.set_model(synth.gtr_model(alpha=0.9, ncat=4))
    t.set_likelihood_kernel(pkg.LK_EIGEN_HIP)
    if sharded:
        t.attach_engine_sharded([0] * sharded, pkg.REDUCE_HOST)
    else:
        t.attach_engine(0)
    return t


_EXACT = {}


def exact_engine(pkg, synth, nptn):
    """one engine per pattern count for the whole module: NROWS integer rows in the store, NSAMPLES integer samples.
    Row 0 is random in -9 .. -1; every other row is row 0 with -1 / 0 / +1 added at three patterns, so the sums of two
    rows differ by a small integer, often by 0 or +-1: ties at epsilon 0.5, the strict edges at epsilon 1 and 0."""
    if nptn not in _EXACT:
        rng = np.random.default_rng(1000 + nptn)
        t = make_engine(pkg, synth, nptn)
        L = np.tile(rng.integers(-9, 0, size=nptn).astype(np.float64), (NROWS, 1))
        for r in range(1, NROWS):
            at = rng.choice(nptn, 3, replace=False)
            L[r, at] = np.clip(L[r, at] + rng.integers(-1, 2, size=3), -9, -1)
        L[NROWS - 1] = L[1]                                  # two store rows with the same content
        W = rng.integers(0, 4, size=(NSAMPLES, nptn)).astype(np.float32)
        t.ptnlh_reserve(NROWS)
        for r in range(NROWS):
            t.ptnlh_upload(r, L[r])
        t.set_boot_samples(W)
        _EXACT[nptn] = (t, L, W.astype(np.float64))
    return _EXACT[nptn]


def entry_list(rng, ntrees):
    rows = rng.integers(0, NROWS, size=ntrees)
    if ntrees >= 2:
        rows[1] = rows[0]                                    # a repeated row: difference 0 in every replicate
    if ntrees >= 5:
        rows[4] = rows[2]
    ids = 5 + np.arange(ntrees, dtype=np.int64) * 3
    ids[-1] = (1 << 40) + 7                                  # ids are 64-bit tags
    logl = rng.uniform(-5000.0, -4000.0, size=ntrees)
    rand = rng.uniform(0.0, 1.0, size=ntrees)
    rand[::7] = 0.5
    if ntrees >= 2:
        rand[1] = 0.25                                       # ... which is taken as a tie: 0.25 <= 1 / (1 + 1)
    if ntrees >= 3:
        rand[2] = 0.0
    if ntrees >= 4:
        rand[3] = 1.0
    return rows, ids, logl, rand


@pytest.mark.parametrize("ntrees", [1, 2, 37])
@pytest.mark.parametrize("nsamples", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("nptn", [70, 1000])
def test_exact_cases(pkg, synth, monkeypatch, nptn, nsamples, ntrees):
    t, L, W = exact_engine(pkg, synth, nptn)
    rng = np.random.default_rng(nptn + 7 * nsamples + 1000 * ntrees)
    rows, ids, logl, rand = entry_list(rng, ntrees)
    R = L[rows] @ W[:nsamples].T                             # exact integers
    assert np.array_equal(R, np.round(R)) and np.abs(R).max() < 2 ** 40
    saw_tie = False
    for eps in (0.5, 1.0, 0.0):
        want = ref.ufboot_start(nsamples)
        wcounts, wmin = ref.ufboot_rule(want, R, ids, logl, rand, epsilon=eps)
        saw_tie = saw_tie or bool((want["boot_counts"] > 1).any())
        for chunk in (None, "1", "5"):
            if chunk is None:
                monkeypatch.delenv("IQHIP_UFBOOT_CHUNK", raising=False)
            else:
                monkeypatch.setenv("IQHIP_UFBOOT_CHUNK", chunk)
            t.ufboot_init(nsamples)
            counts, mn = t.ufboot_update(rows, ids, logl, rand, epsilon=eps)
            assert_state_equal(t.ufboot_state(), want, "eps %g chunk %s" % (eps, chunk))
            assert counts.tolist() == wcounts.tolist() and mn == wmin
            launches = t.ufboot_timing()[2]
            assert launches == 3 * (ntrees if chunk == "1" else -(-ntrees // 5) if chunk == "5" else 1)
        monkeypatch.delenv("IQHIP_UFBOOT_CHUNK", raising=False)
        # one call over the list == one call per entry
        t.ufboot_init(nsamples)
        total = np.zeros(3, dtype=np.int64)
        for k in range(ntrees):
            c, mn = t.ufboot_update(rows[k:k + 1], ids[k:k + 1], logl[k:k + 1], rand[k:k + 1], epsilon=eps)
            total += c
        assert_state_equal(t.ufboot_state(), want, "eps %g entry by entry" % eps)
        assert total.tolist() == wcounts.tolist() and mn == wmin
    if ntrees >= 2 and nsamples > 1:
        assert saw_tie                                       # the inputs do force the tie branch


def test_cutoff_drops_entries(pkg, synth):
    t, L, W = exact_engine(pkg, synth, 70)
    rng = np.random.default_rng(11)
    rows, ids, logl, rand = entry_list(rng, 37)
    ns = 65
    R = L[rows] @ W[:ns].T
    cutoff = float(np.sort(logl)[12]) + 1.0                  # the 12 lowest fall below cutoff - 1
    want = ref.ufboot_start(ns)
    wcounts, wmin = ref.ufboot_rule(want, R, ids, logl, rand, logl_cutoff=cutoff)
    assert wcounts[:2].tolist() == [25, 12]
    t.ufboot_init(ns)
    counts, mn = t.ufboot_update(rows, ids, logl, rand, logl_cutoff=cutoff)
    assert_state_equal(t.ufboot_state(), want)
    assert counts.tolist() == wcounts.tolist() and mn == wmin
    # everything dropped: nothing is multiplied, the state stays, the minimum is still reported
    counts, mn2 = t.ufboot_update(rows[:3], ids[:3], [-9e5, -9e5, -9e5], rand[:3], logl_cutoff=cutoff)
    assert counts.tolist() == [0, 3, 0] and mn2 == wmin
    assert_state_equal(t.ufboot_state(), want)
    assert t.ufboot_timing()[2] == 1
    # a fresh state with everything dropped holds no tree: DBL_MAX
    t.ufboot_init(ns)
    counts, mn3 = t.ufboot_update(rows[:3], ids[:3], [-9e5, -9e5, -9e5], rand[:3], logl_cutoff=cutoff)
    assert counts.tolist() == [0, 3, 0] and mn3 == ref.DBL_MAX
    assert_state_equal(t.ufboot_state(), ref.ufboot_start(ns))


# ---- real rows ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def real_case(pkg, synth):
    """8 taxa, 300 DNA patterns: the current tree's row 0 and the 10 NNI rows 1 .. 10 of evaluate_nnis5_batch"""
    model = synth.gtr_model(alpha=0.9, ncat=4)
    nwk, pat, freq = synth.make_workload(8, 300, model, seed=41)
    t = pkg.PhyloTree(nwk)
    t.set_mem_mode(pkg.LM_ALL_BRANCH)
    t.set_alignment(4, pkg.SEQ_DNA, pat, freq)
    t.set_model(model)
    t.set_likelihood_kernel(pkg.LK_EIGEN_HIP)
    t.attach_engine(0)
    rng = np.random.default_rng(41)
    p = np.asarray(freq, dtype=np.float64)
    W = rng.multinomial(int(p.sum()), p / p.sum(), size=NSAMPLES).astype(np.float32)
    t.set_boot_samples(W)
    lnl = t.compute_likelihood()
    t.ptnlh_reserve(11)
    t.ufboot_init(1)
    t.save_current_tree(lnl)                                 # the mirror puts the current tree's row into row 0
    moves = t.evaluate_nnis5_batch(first_row=1)
    assert len(moves) == 10
    rows = np.arange(11)
    logl = np.array([lnl] + [m["newloglh"] for m in moves])
    ids = np.arange(11, dtype=np.int64)
    rand = np.array([pkg.ufboot_rand(9, k) for k in range(11)])
    L = np.array([t.ptnlh_fetch(r) for r in rows])
    assert abs(L[0] @ freq - lnl) <= 1e-9 * abs(lnl)
    return t, rows, ids, logl, rand, L, W.astype(np.float64)


@pytest.mark.parametrize("nsamples", [64, 257])
def test_real_rows_bit_identical_to_the_rule_on_the_device_sums(pkg, real_case, monkeypatch, nsamples):
    t, rows, ids, logl, rand, L, W = real_case
    R = t.ptnlh_rell(rows, nsamples)
    want = ref.ufboot_start(nsamples)
    wcounts, wmin = ref.ufboot_rule(want, R, ids, logl, rand)
    for chunk in (None, "1", "5"):
        if chunk is None:
            monkeypatch.delenv("IQHIP_UFBOOT_CHUNK", raising=False)
        else:
            monkeypatch.setenv("IQHIP_UFBOOT_CHUNK", chunk)
        t.ufboot_init(nsamples)
        counts, mn = t.ufboot_update(rows, ids, logl, rand)
        assert_state_equal(t.ufboot_state(), want, "chunk %s" % chunk)
        assert counts.tolist() == wcounts.tolist() and mn == wmin
    assert len(set(want["boot_tree"].tolist())) > 1          # the replicates do disagree about the best tree


def test_real_rows_against_the_numpy_product(pkg, real_case):
    """The restatement on numpy's float64 product L W^T.  The device product differs from it by at most
    1e-13 * sum |L| |W| per element (the bound tests/test_branch_tests_gpu.py uses for this product), so a replicate counts
    only where every comparison of the numpy run keeps a margin |rell - (boot_logl +- epsilon)| above that bound; there
    boot_tree, boot_counts and boot_orig_logl must be equal and boot_logl must agree within the bound (it IS a sum).  At
    most 1 % of the replicates may be left out.  The bound is below 5e-10 here (|lnL| ~ 3000) against margins spread over
    several log-likelihood units: a comparison falls inside it with probability ~1e-10, so 22 comparisons x 257
    replicates leave out none for any seed one could reasonably draw (seed 41 on an MI355X: none left out, smallest
    margin 7.7e-4, largest bound 4.6e-10)."""
    t, rows, ids, logl, rand, L, W = real_case
    ns = NSAMPLES
    R = L @ W[:ns].T
    bound = (1e-13 * (np.abs(L) @ np.abs(W[:ns]).T)).max(axis=0)
    margins = np.full(ns, np.inf)
    want = ref.ufboot_start(ns)
    ref.ufboot_rule(want, R, ids, logl, rand, margins=margins)
    counted = margins > bound
    print("replicates left out: %d of %d; smallest margin %.3e, largest bound %.3e" % ((~counted).sum(), ns, margins.min(), bound.max()))
    assert (~counted).sum() <= ns // 100
    t.ufboot_init(ns)
    t.ufboot_update(rows, ids, logl, rand)
    got = t.ufboot_state()
    for f in ("boot_tree", "boot_counts"):
        np.testing.assert_array_equal(got[f][counted], want[f][counted], err_msg=f)
    np.testing.assert_array_equal(bits(got["boot_orig_logl"][counted]), bits(want["boot_orig_logl"][counted]))
    assert (np.abs(got["boot_logl"] - want["boot_logl"])[counted] <= bound[counted]).all()


def test_mirror_feeds_the_same_entries(pkg, real_case):
    """save_current_tree + save_nni_trees == one update over {current row, the 10 NNI rows} with sequential ids and the
    documented tie draws; the kept strings are those of the ids some replicate refers to"""
    t, rows, ids, logl, rand, L, W = real_case
    ns = 65
    t.ufboot_init(ns)
    t.ufboot_update(rows[:1], ids[:1], logl[:1], rand[:1])
    t.ufboot_update(rows[1:], ids[1:], logl[1:], rand[1:])
    want = t.ufboot_state()
    t.ufboot_init(ns, seed=9)
    lnl = t.compute_likelihood()
    assert abs(lnl - logl[0]) <= 1e-9 * abs(lnl)
    c0, _ = t.save_current_tree(logl[0])
    assert c0.tolist() == [1, 0, ns]
    c1, mn = t.save_nni_trees()
    assert c1[0] == 10 and abs(mn - want["boot_orig_logl"].min()) <= 1e-9 * abs(mn)
    got = t.ufboot_state()
    np.testing.assert_array_equal(got["boot_tree"], want["boot_tree"])
    np.testing.assert_array_equal(got["boot_counts"], want["boot_counts"])
    np.testing.assert_allclose(got["boot_logl"], want["boot_logl"], rtol=1e-12)   # the NNI rows were optimised again
    info = t.ufboot_info()
    assert info["trees_fed"] == 11 and info["trees_kept"] == len(set(got["boot_tree"].tolist()))
    s = t.summarize_bootstrap()
    assert len(s["boot_trees"]) == ns and s["distinct_trees"] == info["trees_kept"]
    base = t.sorted_taxon_id_string()
    for k in range(ns):
        if got["boot_tree"][k] == 0:
            assert s["boot_trees"][k] == base
        else:
            assert s["boot_trees"][k] != base and len(pkg.newick_splits(s["boot_trees"][k], 8)) == 5
    want_sup = pkg.split_supports(s["boot_trees"], base, 8)
    assert sorted(p for _, _, p in s["supports"]) == sorted(want_sup)
    assert s["consensus_tree"] == ref.consensus(s["boot_trees"], 8)


# ---- state rules and refusals ----------------------------------------------------------------------------------------
def test_state_rules(pkg, synth):
    lib = pkg.libiqhip()
    t = make_engine(pkg, synth, 70)
    t.ptnlh_reserve(2)
    t.ptnlh_upload(0, -np.ones(70))
    t.ptnlh_upload(1, -2.0 * np.ones(70))
    ent = (pkg.UFBootTree * 2)(pkg.UFBootTree(0, 0, 3, -70.0, 0.5), pkg.UFBootTree(1, 0, 4, -140.0, 0.5))
    upd = lambda: lib.iqhip_ufboot_update(t.engine, ent, 2, 0.5, 0.0, None, None)
    fetch = lambda: lib.iqhip_ufboot_fetch(t.engine, None, None, None, None)
    assert lib.iqhip_ufboot_init(t.engine, 1) == IQHIP_ERR_INVALID           # no samples yet
    assert upd() == IQHIP_ERR_INVALID and fetch() == IQHIP_ERR_INVALID          # before init
    assert b"iqhip_ufboot_init" in lib.iqhip_last_error()
    t.set_boot_samples(np.ones((8, 70), dtype=np.float32))
    assert lib.iqhip_ufboot_init(t.engine, 0) == IQHIP_ERR_INVALID
    assert lib.iqhip_ufboot_init(t.engine, 9) == IQHIP_ERR_INVALID           # above the uploaded samples
    assert upd() == IQHIP_ERR_INVALID
    t.ufboot_init(8)
    assert upd() == 0
    st = t.ufboot_state()
    assert st["boot_tree"].tolist() == [3] * 8 and st["boot_logl"].tolist() == [-70.0] * 8
    t.ufboot_init(5)                                                            # a second init resets the state
    assert_state_equal(t.ufboot_state(), ref.ufboot_start(5))
    assert upd() == 0
    # replacing the sample matrix invalidates the state, whichever call replaces it
    t.gen_boot_samples(8, 70, 3)
    assert upd() == IQHIP_ERR_INVALID and fetch() == IQHIP_ERR_INVALID
    t.ufboot_init(8)
    assert upd() == 0
    t.set_boot_samples(np.ones((8, 70), dtype=np.float32))
    assert upd() == IQHIP_ERR_INVALID
    t.ufboot_init(8)
    assert upd() == 0
    t.multiscale_bp([0, 1], [1.0], 8, 1)
    assert upd() == IQHIP_ERR_INVALID and fetch() == IQHIP_ERR_INVALID
    t.ufboot_init(8)
    assert upd() == 0


def test_refusals(pkg, synth):
    lib = pkg.libiqhip()
    t = make_engine(pkg, synth, 70)
    t.ptnlh_reserve(2)
    t.set_boot_samples(np.ones((4, 70), dtype=np.float32))
    t.ufboot_init(4)
    good = dict(row=0, tree_id=1, logl=-10.0, rand=0.5)

    def rc(eps=0.5, n=1, null=False, **kw):
        f = dict(good, **kw)
        ent = (pkg.UFBootTree * 1)(pkg.UFBootTree(f["row"], 0, f["tree_id"], f["logl"], f["rand"]))
        return lib.iqhip_ufboot_update(t.engine, None if null else ent, n, eps, 0.0, None, None)

    assert rc() == 0
    before = t.ufboot_state()
    assert rc(null=True) == IQHIP_ERR_INVALID
    assert rc(n=0) == IQHIP_ERR_INVALID
    assert rc(row=2) == IQHIP_ERR_INVALID and rc(row=-1) == IQHIP_ERR_INVALID
    assert rc(tree_id=-1) == IQHIP_ERR_INVALID
    for bad in (-1e-9, 1.0000001, float("nan")):
        assert rc(rand=bad) == IQHIP_ERR_INVALID
    for bad in (float("inf"), float("-inf"), float("nan")):
        assert rc(logl=bad) == IQHIP_ERR_INVALID
    assert rc(eps=-0.1) == IQHIP_ERR_INVALID and rc(eps=float("nan")) == IQHIP_ERR_INVALID
    assert rc(rand=0.0) == 0 and rc(rand=1.0) == 0 and rc(eps=0.0) == 0
    # a bad entry anywhere in the list refuses the whole call before anything runs
    ent = (pkg.UFBootTree * 3)(pkg.UFBootTree(0, 0, 7, -1.0, 0.0), pkg.UFBootTree(1, 0, 8, -1.0, 0.0), pkg.UFBootTree(5, 0, 9, -1.0, 0.0))
    t.ufboot_init(4)
    assert lib.iqhip_ufboot_update(t.engine, ent, 3, 0.5, 0.0, None, None) == IQHIP_ERR_INVALID
    assert_state_equal(t.ufboot_state(), ref.ufboot_start(4))
    assert before["boot_tree"].tolist() == [1] * 4
    d = np.zeros(2)
    assert lib.iqhip_debug_ufboot_timing(t.engine, None, None) == IQHIP_ERR_INVALID
    assert lib.iqhip_debug_ufboot_timing(t.engine, d.ctypes.data_as(C.POINTER(C.c_double)), None) == 0


def test_sharded_engine_is_unsupported(pkg, synth):
    lib = pkg.libiqhip()
    t = make_engine(pkg, synth, 200, sharded=2)              # (a shard holds at least 64 patterns)
    ent = (pkg.UFBootTree * 1)(pkg.UFBootTree(0, 0, 1, -1.0, 0.5))
    d = np.zeros(2)
    for rc in (lib.iqhip_ufboot_init(t.engine, 1), lib.iqhip_ufboot_update(t.engine, ent, 1, 0.5, 0.0, None, None),
               lib.iqhip_ufboot_fetch(t.engine, None, None, None, None),
               lib.iqhip_debug_ufboot_timing(t.engine, d.ctypes.data_as(C.POINTER(C.c_double)), None)):
        assert rc == IQHIP_ERR_UNSUPPORTED
