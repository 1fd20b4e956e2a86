"""Tree topology tests (include/iqhip.h "tree topology tests"), the parts that need no device: numpy restatements of the
reference's evaluateTrees statistics (phylotesting.cpp:2218-2411), of the engine's counter-based resampling generator
(exact 64-bit arithmetic) and of computeLogLDiffVariance (phylotree.cpp:1390-1416) that the GPU tests compare the engine
with, their self-checks, the inputs of the multi-scale test, the new symbols and the refusal of a planning-only engine."""
import ctypes as C

import numpy as np

DBL_MAX = np.finfo(np.float64).max
MASK32 = np.uint64(0xFFFFFFFF)
GOLDEN = np.uint64(0x9E3779B97F4A7C15)
STREAM_RELL, STREAM_TIE = 0xA0, 0xB9


# ---- the generator -----------------------------------------------------------------------------------------------------
def u64(x):
    return np.atleast_1d(np.asarray(x, dtype=np.uint64))


def mix(z):
    """splitmix64 finaliser on uint64 arrays (products wrap modulo 2^64)"""
    z = u64(z)
    z = z ^ (z >> np.uint64(30))
    z = z * np.uint64(0xBF58476D1CE4E5B9)
    z = z ^ (z >> np.uint64(27))
    z = z * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def mulhi64(a, b):
    """high 64 bits of the 128-bit product of uint64 arrays a and the integer b < 2^64, from 32-bit limbs"""
    a = u64(a)
    b = np.uint64(b)
    al, ah, bl, bh = a & MASK32, a >> np.uint64(32), b & MASK32, b >> np.uint64(32)
    t = al * bl
    k = t >> np.uint64(32)
    t = ah * bl + k
    w2, w1 = t & MASK32, t >> np.uint64(32)
    t = al * bh + w2
    return ah * bh + w1 + (t >> np.uint64(32))


def draws(seed, stream, rho, j):
    """z of (seed, stream, replicate rho, draw j); rho and j broadcast"""
    key = mix(u64(seed % (1 << 64)) + GOLDEN * u64(stream + 1))
    h = mix(key + GOLDEN * (u64(rho) + np.uint64(1)))
    return mix(h + GOLDEN * (u64(j) + np.uint64(1)))


def restate_gen(freq, nsamples, first, ndraws, seed, stream):
    """iqhip_gen_boot_samples: int64 [nsamples, nptn] pattern counts of replicates first .. first + nsamples - 1"""
    f = np.asarray(freq, dtype=np.float64)
    assert np.all(f >= 0) and np.all(f == np.floor(f))
    prefix = np.cumsum(f.astype(np.int64))
    nsite = int(prefix[-1])
    out = np.zeros((nsamples, f.size), dtype=np.int64)
    j = np.arange(ndraws, dtype=np.uint64)
    for i in range(nsamples):
        site = mulhi64(draws(seed, stream, first + i, j), nsite).astype(np.int64)
        pattern = np.searchsorted(prefix, site, side="right")   # the first p with prefix[p] > site
        out[i] = np.bincount(pattern, minlength=f.size)
    return out


def tie_uniforms(tie_seed, ntrees, nsamples):
    """random_double() of the RELL-BP tie rule: u[tid, boot] = (z >> 11) 2^-53, z of (tie_seed, 0xB9, boot, tid)"""
    u = np.zeros((ntrees, nsamples))
    boot = np.arange(nsamples, dtype=np.uint64)
    for tid in range(ntrees):
        u[tid] = (draws(tie_seed, STREAM_TIE, boot, tid) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    return u


# ---- the statistics ----------------------------------------------------------------------------------------------------
def cmax(a, b):
    """std::max(a, b): b where a < b, else a (a NaN b leaves a)"""
    return np.where(a < b, b, a)


def confidence_set(share):
    """trees by decreasing share until the shares pass 0.95 (phylotesting.cpp:2248-2255); equal shares: highest index first"""
    rank = np.argsort(np.asarray(share), kind="stable")
    inside = np.zeros(len(share), dtype=bool)
    total = 0.0
    for k in range(len(share) - 1, -1, -1):
        inside[rank[k]] = True
        total += share[rank[k]]
        if total > 0.95:
            break
    return inside


def restate_tree_tests(R, lh, eps, weights, tie_u):
    """phylotesting.cpp:2218-2411 on the RELL sums R[ntrees, S] and the trees' total lnL; weights: [ntrees, ntrees] matrix
    1 / sqrt(variance of the difference) or None; tie_u[ntrees, S]: the uniforms of the BP tie rule.  Every expression
    keeps the reference's order, in IEEE double without contraction."""
    R = np.asarray(R, dtype=np.float64)
    lh = np.asarray(lh, dtype=np.float64)
    T, S = R.shape
    with np.errstate(invalid="ignore", over="ignore"):
        # RELL-BP (:2220-2247)
        maxL = R[0].copy()
        maxtid = np.zeros(S, dtype=np.int64)
        maxcount = np.ones(S, dtype=np.int64)
        for tid in range(1, T):
            r = R[tid]
            c1 = r > maxL + eps
            c2 = ~c1 & (r > maxL - eps) & (tie_u[tid] <= 1.0 / (maxcount + 1))
            maxL = np.where(c1, r, np.where(c2, cmax(maxL, r), maxL))
            maxtid = np.where(c1 | c2, tid, maxtid)
            maxcount = np.where(c1, 1, np.where(c2, maxcount + 1, maxcount))
        bp = np.bincount(maxtid, minlength=T) / S
        # SH centring (:2270-2282): avg_lh summed in replicate order
        avg = np.array([np.add.accumulate(R[tid])[-1] / S for tid in range(T)])
        max_sh = np.full(S, -DBL_MAX)
        for tid in range(T):
            max_sh = cmax(max_sh, R[tid] - avg[tid])
        orig_max_id, orig_max_lh = 0, lh[0]
        for tid in range(1, T):
            if orig_max_lh < lh[tid]:
                orig_max_lh, orig_max_id = lh[tid], tid
        orig_2nd_id, orig_2nd_lh = -1, -DBL_MAX
        for tid in range(T):
            if tid != orig_max_id and orig_2nd_lh < lh[tid]:
                orig_2nd_lh, orig_2nd_id = lh[tid], tid
        kh, sh = np.zeros(T), np.zeros(T)
        for tid in range(T):
            max_id = orig_max_id if tid != orig_max_id else orig_2nd_id
            orig_diff = lh[max_id] - lh[tid] - avg[tid]
            sh[tid] = np.count_nonzero(max_sh - R[tid] > orig_diff) / S
            kh[tid] = np.count_nonzero((R[max_id] - avg[max_id]) - R[tid] > orig_diff) / S
        wkh, wsh = np.full(T, -1.0), np.full(T, -1.0)
        if weights is not None:
            for tid in range(T):
                worig_diff, max_id = -DBL_MAX, -1
                for tid2 in range(T):
                    if tid2 != tid:
                        wdiff = (lh[tid2] - lh[tid]) * weights[tid, tid2]
                        if wdiff > worig_diff:
                            worig_diff, max_id = wdiff, tid2
                wmax = np.full(S, -DBL_MAX)
                for tid2 in range(T):
                    if tid2 != tid:
                        wmax = cmax(wmax, (R[tid2] - avg[tid2] - R[tid] + avg[tid]) * weights[tid, tid2])
                wsh[tid] = np.count_nonzero(wmax > worig_diff) / S
                if max_id >= 0:
                    wkh[tid] = np.count_nonzero(R[max_id] - avg[max_id] - R[tid] + avg[tid] > lh[max_id] - lh[tid]) / S
                else:
                    wkh[tid] = 0.0
        # ELW (:2377-2402)
        max_lh = np.full(S, -DBL_MAX)
        for tid in range(T):
            max_lh = cmax(max_lh, R[tid])
        E = np.exp(R - max_lh)
        sumL = np.zeros(S)
        for tid in range(T):
            sumL = sumL + E[tid]
        elw = np.array([np.sum(E[tid] / sumL) / S for tid in range(T)])
    return dict(bp=bp, kh=kh, sh=sh, wkh=wkh, wsh=wsh, elw=elw, rell_confident=confidence_set(bp),
                elw_confident=confidence_set(elw))


def restate_diff_variance(L, freq):
    """computeLogLDiffVariance for all pairs of the rows L[n, nptn]: symmetric, diagonal 0"""
    L = np.asarray(L, dtype=np.float64)
    f = np.asarray(freq, dtype=np.float64)
    nsite = f.sum()
    n = L.shape[0]
    var = np.zeros((n, n))
    for i in range(n):
        for j in range(i + 1, n):
            d = L[j] - L[i]
            mean = np.sum(d * f) / nsite
            v = np.sum((d - mean) * (d - mean) * f)
            var[i, j] = var[j, i] = 0.0 if nsite <= 1 else v * (nsite / (nsite - 1.0))
    return var


# ---- shared inputs -----------------------------------------------------------------------------------------------------
def asc_freq(rng, nptn, nzero=None):
    """integer pattern frequencies 1 .. 5 with zeros at the end (the +ASC layout)"""
    f = rng.integers(1, 6, size=nptn).astype(np.float64)
    nzero = min(4, nptn - 1) if nzero is None else nzero
    if nzero:
        f[nptn - nzero:] = 0.0
    return f


def tree_rows(rng, ntrees, nptn, freq):
    """per-pattern lnL rows: random in [-12, -1] plus per-tree offsets of order 0.01 .. 1, the offsets of a tree centred
    on its weighted mean so that the trees' total lnL are close and the replicates have more than one winner"""
    base = rng.uniform(-12.0, -1.0, size=nptn)
    off = 10.0 ** rng.uniform(-2.0, 0.0, size=(ntrees, 1)) * rng.uniform(-1.0, 1.0, size=(ntrees, nptn))
    off -= (off @ freq / freq.sum())[:, None]
    return base + off


MS_SEED, MS_SCALES, MS_SAMPLES = 20240611, (0.5, 1.0, 1.4), 300


def multiscale_case():
    """the inputs of the multi-scale test: 17 trees x 700 patterns"""
    rng = np.random.default_rng(1707)
    freq = asc_freq(rng, 700)
    return tree_rows(rng, 17, 700, freq), freq


def multiscale_truth(L, freq, scales=MS_SCALES, nsamples=MS_SAMPLES, seed=MS_SEED):
    """per scale k: first-wins arg-max counts of the float64 sums over restate_gen's samples (stream k), and the number of
    replicates whose two largest sums differ by less than 1e-9 |max| (left out of the counts)"""
    nsite = freq.sum()
    counts = np.zeros((len(scales), L.shape[0]), dtype=np.int64)
    excluded = np.zeros(len(scales), dtype=np.int64)
    for k, sc in enumerate(scales):
        W = restate_gen(freq, nsamples, 0, int(round(sc * nsite)), seed, k).astype(np.float64)
        R = L @ W.T
        top2 = np.sort(R, axis=0)[-2:]
        close = top2[1] - top2[0] < 1e-9 * np.abs(top2[1])
        excluded[k] = close.sum()
        counts[k] = np.bincount(np.argmax(R, axis=0)[~close], minlength=L.shape[0])   # argmax: the first maximum
    return counts, excluded


# ---- self-checks -------------------------------------------------------------------------------------------------------
def test_mix_and_mulhi_are_exact():
    # splitmix64 of state 0 gives 0xE220A8397B1DCDAF first: mix(0 + G)
    assert int(mix(GOLDEN)[0]) == 0xE220A8397B1DCDAF
    rng = np.random.default_rng(3)
    a = rng.integers(0, 1 << 63, size=200, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=200, dtype=np.uint64)
    for b in (1, 3, 12345, (1 << 32) - 1, (1 << 32) + 7, (1 << 62) + 12345, (1 << 64) - 1):
        assert [int(x) for x in mulhi64(a, b)] == [(int(x) * b) >> 64 for x in a]


def test_two_trees_by_hand():
    R = np.array([[-100.0, -99.0, -104.0, -100.0],
                  [-101.0, -98.0, -103.0, -103.0]])
    lh = [-100.0, -101.0]
    # avg = (-100.75, -101.25); centred sums: tree 0 (.75, 1.75, -3.25, .75), tree 1 (.25, 3.25, -1.75, -1.75)
    # SH maximum per replicate (.75, 3.25, -1.75, .75)
    # tree 0 against tree 1: orig_diff = -101 + 100 + 100.75 = 99.75
    #   SH  max - R0 = (100.75, 102.25, 102.25, 100.75) > 99.75: 4;  KH  c1 - R0 = (100.25, 102.25, 102.25, 98.25): 3
    # tree 1 against tree 0: orig_diff = 1 + 101.25 = 102.25
    #   SH  max - R1 = (101.75, 101.25, 101.25, 103.75): 1;          KH  c0 - R1 = (101.75, 99.75, 99.75, 103.75): 1
    never = np.ones((2, 4))
    r = restate_tree_tests(R, lh, 0.0, None, never)
    assert r["bp"].tolist() == [0.5, 0.5]                 # strict winners: tree 0 in replicates 0 and 3
    assert r["sh"].tolist() == [1.0, 0.25] and r["kh"].tolist() == [0.75, 0.25]
    assert r["wkh"].tolist() == [-1.0, -1.0] and r["wsh"].tolist() == [-1.0, -1.0]
    assert r["rell_confident"].tolist() == [True, True]
    assert abs(r["elw"].sum() - 1.0) < 1e-15
    e = np.exp(-1.0)                                      # R0 - R1 = 1, -1, -1, 3
    want0 = (1.0 / (1.0 + e) + 2.0 * e / (1.0 + e) + 1.0 / (1.0 + np.exp(-3.0))) / 4.0
    assert abs(r["elw"][0] - want0) < 1e-15
    # the tie rule with epsilon = 1.5: replicates 0 .. 2 are within epsilon (a draw decides), replicate 3 is not
    r = restate_tree_tests(R, lh, 1.5, None, np.full((2, 4), 0.3))       # 0.3 <= 1/2: tree 1 takes them
    assert r["bp"].tolist() == [0.25, 0.75]
    r = restate_tree_tests(R, lh, 1.5, None, np.full((2, 4), 0.7))
    assert r["bp"].tolist() == [1.0, 0.0]
    assert r["rell_confident"].tolist() == [True, False]
    # weights of 1: wSH = SH with two trees, wKH compares the centred difference with lh[other] - lh[tid]
    w = np.array([[0.0, 1.0], [1.0, 0.0]])
    r = restate_tree_tests(R, lh, 0.0, w, never)
    # tree 0: c1 - c0 = (-.5, 1.5, 1.5, -2.5) > -1: 3;  tree 1: c0 - c1 = (.5, -1.5, -1.5, 2.5) > 1: 1
    assert r["wkh"].tolist() == [0.75, 0.25] and r["wsh"].tolist() == [0.75, 0.25]
    # identical trees: infinite weights make every weighted difference NaN, nothing is counted
    with np.errstate(divide="ignore"):
        winf = 1.0 / np.sqrt(np.zeros((2, 2)))
    r = restate_tree_tests(np.array([R[0], R[0]]), [-100.0, -100.0], 0.0, winf, never)
    assert r["wkh"].tolist() == [0.0, 0.0] and r["wsh"].tolist() == [0.0, 0.0] and r["bp"].tolist() == [1.0, 0.0]
    assert r["kh"].tolist() == [0.0, 0.0] and r["sh"].tolist() == [0.0, 0.0]


def test_generator_restatement():
    rng = np.random.default_rng(8)
    freq = asc_freq(rng, 65)
    nsite = int(freq.sum())
    for ndraws in (1, round(0.5 * nsite), round(1.4 * nsite)):
        W = restate_gen(freq, 6, 5, ndraws, 99, STREAM_RELL)
        assert W.sum(axis=1).tolist() == [ndraws] * 6
        assert not W[:, freq == 0].any()
    # a split gives the same rows; another stream, seed or replicate gives other rows
    whole = restate_gen(freq, 16, 0, nsite, 99, STREAM_RELL)
    np.testing.assert_array_equal(whole[5:], restate_gen(freq, 11, 5, nsite, 99, STREAM_RELL))
    assert not np.array_equal(whole[:11], whole[5:])
    assert not np.array_equal(whole, restate_gen(freq, 16, 0, nsite, 99, STREAM_RELL + 1))
    assert not np.array_equal(whole, restate_gen(freq, 16, 0, nsite, 100, STREAM_RELL))
    # mean counts over 2000 replicates within 5 sigma of ndraws f / nsite (sigma of a mean of binomial counts)
    W = restate_gen(freq, 2000, 0, nsite, 7, 3)
    p = freq / nsite
    sigma = np.sqrt(nsite * p * (1.0 - p) / 2000.0)
    assert np.all(np.abs(W.mean(axis=0) - nsite * p) <= 5.0 * sigma)
    u = tie_uniforms(5, 3, 1000)
    assert u.min() >= 0.0 and u.max() < 1.0 and abs(u.mean() - 0.5) < 5.0 / np.sqrt(12 * 3000)


def test_diff_variance_restatement():
    f = np.array([2.0, 1.0, 1.0])
    L = np.array([[-1.0, -2.0, -3.0], [-1.5, -2.0, -1.0]])
    # d = (-.5, 0, 2), mean = (-1 + 0 + 2) / 4 = .25; sum f (d - mean)^2 = 2 (.5625) + .0625 + 3.0625 = 4.25; x 4/3
    v = restate_diff_variance(L, f)
    assert v[0, 0] == v[1, 1] == 0.0 and v[0, 1] == v[1, 0]
    assert abs(v[0, 1] - 4.25 * 4.0 / 3.0) < 1e-15
    assert restate_diff_variance(L, np.array([1.0, 0.0, 0.0]))[0, 1] == 0.0     # nsite <= 1
    assert restate_diff_variance(np.array([L[0], L[0]]), f)[0, 1] == 0.0


def test_multiscale_inputs_have_no_near_tie():
    """the multi-scale GPU test compares counts exactly when no replicate's two best sums are within 1e-9 |max|"""
    L, freq = multiscale_case()
    counts, excluded = multiscale_truth(L, freq)
    print("excluded per scale:", excluded.tolist())
    assert np.all(excluded <= 0.01 * MS_SAMPLES)
    assert excluded.sum() == 0
    assert counts.sum(axis=1).tolist() == [MS_SAMPLES] * len(MS_SCALES)
    assert (counts > 0).sum(axis=1).min() >= 2            # more than one tree wins replicates at every scale


# ---- the library -------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("iqhip_ptnlh_upload", "iqhip_gen_boot_samples", "iqhip_ptnlh_diff_variance", "iqhip_tree_tests",
               "iqhip_multiscale_bp")


def test_new_symbols_exist(pkg):
    lib = pkg.libiqhip()
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s), s
        assert s in pkg.IQHIP_SYMBOLS
    assert lib.iqhip_abi_version() == 2
    assert C.sizeof(pkg.TreeTest) == 56
    for s in ("iqhost_evaluate_trees", "iqhost_gen_boot_samples"):
        assert hasattr(pkg.libiqhost(), s), s


def test_planning_only_engine_refuses_the_new_calls(pkg):
    lib = pkg.libiqhip()
    e = C.c_void_p()
    assert lib.iqhip_debug_create_planner(C.byref(e), 4, 4, 1000, 8, 256, 18, 1) == 0
    try:
        buf = np.zeros(1000)
        dp = buf.ctypes.data_as(C.POINTER(C.c_double))
        rows = np.zeros(3, dtype=np.int32)
        ip = rows.ctypes.data_as(C.POINTER(C.c_int32))
        res = (pkg.TreeTest * 3)()
        calls = [lambda: lib.iqhip_ptnlh_upload(e, 0, dp),
                 lambda: lib.iqhip_gen_boot_samples(e, 4, 0, 100, 1, 0xA0),
                 lambda: lib.iqhip_ptnlh_diff_variance(e, ip, 3, dp),
                 lambda: lib.iqhip_tree_tests(e, ip, dp, 3, 4, 0.5, 0, 1, res),
                 lambda: lib.iqhip_multiscale_bp(e, ip, 3, dp, 1, 4, 1, dp)]
        for call in calls:
            assert call() == 2                                  # IQHIP_ERR_INVALID
            assert b"planning-only" in lib.iqhip_last_error()
    finally:
        lib.iqhip_destroy(e)
