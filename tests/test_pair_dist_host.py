"""Pairwise maximum-likelihood distances (include/iqhip.h "pairwise maximum-likelihood distances"), the parts that need no
device: numpy restatements of AlignmentPairwise's constructor (restate_counts), of computeFuncDerv's default branch over
computeTransDerv (restate_func_derv, restate_function), of Alignment::computeJCDist (restate_jc) and of the solve
(restate_solve: the oracle's own minimize_newton over the restated derivatives, so that the update rule is not restated
a third time), the cases tests/test_pair_dist_gpu.py runs on the device, and the properties of the restatement itself."""
import collections
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "oracle"))
import oracle_driver  # noqa: E402

IQHIP_ERR_INVALID = 2
MAX_GENETIC_DIST = 9.0
X1, X2, XACC, MAX_STEPS = 1e-6, MAX_GENETIC_DIST, 1e-6, 100   # AlignmentPairwise::optimizeDist's call of minimizeNewton
NEW_SYMBOLS = ("iqhip_pair_counts", "iqhip_pair_distances", "iqhip_debug_pair_timing")


# ------------------------------------------------------------------------------------------
# restatements
# ------------------------------------------------------------------------------------------
def restate_counts(states, freq, nstates, pairs):
    """counts[k, a, b] = sum of freq over the patterns where taxon pairs[k][0] shows a and pairs[k][1] shows b, both
    unambiguous (alignmentpairwise.cpp:29-79: addPattern returns before its ambiguity branch)"""
    pairs = np.asarray(pairs).reshape(-1, 2)
    out = np.zeros((len(pairs), nstates, nstates))
    for k, (i, j) in enumerate(pairs):
        a, b = states[i].astype(np.int64), states[j].astype(np.int64)
        ok = (a < nstates) & (b < nstates)
        np.add.at(out[k], (a[ok], b[ok]), np.asarray(freq, dtype=np.float64)[ok])
    return out


def category_sums(model, t, weighted=True):
    """S, S', S'' of the header: per category P = U diag(exp(t r_c eval)) U^-1 with one and two more factors eval for P',
    P''; negative P -> 0 (computeTransDerv leaves the derivatives); summed with props (weighted) or 1 (the reference)"""
    n = len(model.eval)
    U, Ui = np.asarray(model.evec).reshape(n, n), np.asarray(model.inv_evec).reshape(n, n)
    lam = np.asarray(model.eval, dtype=np.float64)
    S, S1, S2 = np.zeros((n, n)), np.zeros((n, n)), np.zeros((n, n))
    for r, p in zip(model.rates, model.props):
        w = p if weighted else 1.0
        e = np.exp(t * r * lam)
        P = (U * e) @ Ui
        S += w * np.where(P < 0.0, 0.0, P)
        S1 += w * r * ((U * (e * lam)) @ Ui)
        S2 += w * r * r * ((U * (e * lam * lam)) @ Ui)
    return S, S1, S2


def restate_func_derv(counts, model, t, weighted=True):
    """(df, ddf) of computeFuncDerv's default branch (alignmentpairwise.cpp:253-279)"""
    S, S1, S2 = category_sums(model, t, weighted)
    m = (counts > 0) & (S > 0)
    d1 = S1[m] / S[m]
    return -float(np.sum(counts[m] * d1)), -float(np.sum(counts[m] * (S2[m] / S[m] - d1 * d1)))


def restate_function(counts, model, t):
    """the negative log-likelihood whose derivatives restate_func_derv returns (computeFunction,
    alignmentpairwise.cpp:153-171, with the weighted category sum)"""
    S = category_sums(model, t)[0]
    m = (counts > 0) & (S > 0)
    return -float(np.sum(counts[m] * np.log(S[m])))


def restate_jc(counts):
    """Alignment::computeJCDist (alignment.cpp:2552-2584) from the pair's counts"""
    n = counts.shape[0]
    total = counts.sum()
    if total == 0:
        return MAX_GENETIC_DIST
    z = n / (n - 1.0)
    x = 1.0 - z * ((total - np.trace(counts)) / total)
    return MAX_GENETIC_DIST if x <= 0 else -np.log(x) / z


class PairFunction:
    """stands where OracleTree.minimize_newton expects a tree: derv() returns the likelihood's derivatives (-df, -ddf)"""

    def __init__(self, counts, model):
        self.counts, self.model = counts, model

    def derv(self, a, b, length=None, theta=None):
        df, ddf = restate_func_derv(self.counts, self.model, length)
        return -df, -ddf


def restate_solve(counts, model, init=0.0, x1=X1, x2=X2, xacc=XACC, max_steps=MAX_STEPS, stats=None, who=None):
    """PhyloTree::computeDist for one pair -> (optx, d2l, evaluated points).  With `stats` the walk is followed point by
    point as tests/test_solver_paths_gpu.py oracle_solve does: what happened is counted, and an input whose stopping tests
    are decided within 1e-6 xacc of their threshold is rejected ("change the seed")."""
    guess = restate_jc(counts) if init == 0.0 else init
    fn = PairFunction(counts, model)
    optx, d2l, pts, status = oracle_driver.OracleTree.minimize_newton(fn, 0, 1, x1, guess, x2, xacc, max_steps, theta=0)
    assert status == "ok", (who, status)
    if stats is not None:
        xl, xh = x1, x2
        for k, x in enumerate(pts):
            f, df = restate_func_derv(counts, model, x)
            if f < 0.0:
                xl = x
            else:
                xh = x
            bisect = df <= 0.0 or ((x - xh) * df - f) * ((x - xl) * df - f) >= 0.0
            dx = 0.5 * (xh - xl) if bisect else f / df
            if k + 1 < len(pts):
                assert pts[k + 1] == (xl + dx if bisect else x - dx), (who, k, pts)
                stats["bisection"] += int(bisect)
            assert abs(abs(dx) - xacc) > 1e-6 * xacc and abs(abs(f) - xacc) > 1e-6 * xacc, ("change the seed", who, x, dx, f)
        stats["at_x1"] += int(optx == x1)
        stats["near_x2"] += int(counts.sum() > 0 and guess == x2 and optx >= 0.5 * x2)
        stats["no_overlap"] += int(counts.sum() == 0 and optx == MAX_GENETIC_DIST and len(pts) == 1)
        stats["solves"] += 1
    return optx, d2l, pts


def all_pairs(ntaxa):
    return [(i, j) for i in range(ntaxa) for j in range(i + 1, ntaxa)]


def restate_matrix(states, freq, model, init=None, stats=None):
    """-> dist, d2l, nsteps [ntaxa, ntaxa] of the restatement"""
    T, n = states.shape[0], len(model.eval)
    dist, d2l, nst = np.zeros((T, T)), np.zeros((T, T)), np.zeros((T, T), dtype=np.int32)
    pairs = all_pairs(T)
    cnt = restate_counts(states, freq, n, pairs)
    for k, (i, j) in enumerate(pairs):
        g = 0.0 if init is None else init[i, j]
        if stats is not None:
            stats["init"] += int(g != 0.0)
        x, d, pts = restate_solve(cnt[k], model, g, stats=stats, who=(i, j))
        dist[i, j] = dist[j, i] = x
        d2l[i, j] = d2l[j, i] = d
        nst[i, j] = nst[j, i] = len(pts)
    return dist, d2l, nst


# ------------------------------------------------------------------------------------------
# the cases of tests/test_pair_dist_gpu.py (built and solved here, without a device)
# ------------------------------------------------------------------------------------------
def rate_model(synth, kind):
    """-> (model, nstates, seq_type)"""
    if kind == "gtr_g4":
        return synth.gtr_model(alpha=0.9, ncat=4), 4, 0
    if kind == "dna_1":
        return synth.gtr_model(alpha=None, ncat=1), 4, 0
    if kind == "dna_12":
        return synth.gtr_model(alpha=0.6, ncat=12), 4, 0
    if kind == "prot_g4":
        return synth.random_reversible_model(20, 5, alpha=0.9, ncat=4), 20, 1
    if kind == "i_g4":
        return synth.gtr_model(alpha=0.9, ncat=4, pinvar=0.2), 4, 0
    if kind == "r4":   # +R4: free rates with unequal weights (mean rate 1)
        m = synth.gtr_model(alpha=0.9, ncat=4)
        props = np.array([0.4, 0.3, 0.2, 0.1])
        rates = np.array([0.15, 0.6, 1.5, 4.0])
        m.props, m.rates = props, rates / float(props @ rates)
        return m, 4, 0
    raise ValueError(kind)


KINDS = ("gtr_g4", "dna_1", "dna_12", "prot_g4", "codon_1", "i_g4", "r4")
SHAPES = ((5, 65), (17, 1000))
# chosen on the CPU so that no pair of a case trips restate_solve's guard
SEEDS = {k: {s: 11 for s in SHAPES} for k in KINDS}
SEEDS["dna_1"][(5, 65)] = 15   # (seed 11: no pair with the random sequence starts from JC = 9 at this size)


def dist_case(pkg, synth, kind, ntaxa, nptn):
    """-> (nstates, seq_type, states[ntaxa, nptn], freq, model, init[ntaxa, ntaxa]).  The columns of a simulated alignment
    serve as patterns (repeats allowed) with frequencies 1 .. 3.  The last taxon shows only unknown states, the one before
    it independent random states, the one before that is a copy of taxon 0; init asks for a far-off start of pair (0, 1)."""
    seed = SEEDS[kind][(ntaxa, nptn)]
    rng = np.random.default_rng(1000 + seed)
    if kind == "codon_1":
        _, states, _, model = synth.codon_gy94_workload(ntaxa, nptn, seed)
        n, seq_type, unknown = 64, 2, 64
        states = states.copy()
        sense = np.unique(states)
        states[rng.random(states.shape) < 0.03] = unknown
    else:
        model, n, seq_type = rate_model(synth, kind)
        unknown = 18 if n == 4 else 23
        nwk = synth.random_tree_newick(ntaxa, seed, 0.02, 0.4)
        states = synth.simulate_alignment(nwk, model, nptn, seed + 1)
        sense = np.arange(n)
        amb = rng.random(states.shape) < 0.03   # ambiguity codes and unknown characters
        states[amb] = rng.integers(n, unknown + 1, size=int(amb.sum()))
    states[ntaxa - 1] = unknown
    states[ntaxa - 2] = rng.choice(sense, size=nptn)
    states[ntaxa - 3] = states[0]
    freq = rng.integers(1, 4, size=nptn).astype(np.float64)
    init = np.zeros((ntaxa, ntaxa))
    init[0, 1] = init[1, 0] = 3.0
    return n, seq_type, np.ascontiguousarray(states, dtype=np.uint8), freq, model, init


def assert_case_stats(stats, ntaxa):
    """what every case must contain (the module docstring of tests/test_pair_dist_gpu.py)"""
    assert stats["solves"] == ntaxa * (ntaxa - 1) // 2
    for what in ("at_x1", "no_overlap", "near_x2", "bisection", "init"):
        assert stats[what] >= 1, (what, dict(stats))


# ------------------------------------------------------------------------------------------
# tests
# ------------------------------------------------------------------------------------------
def jc_counts(p, nsites=1000.0):
    c = np.full((4, 4), nsites * p / 12.0)
    np.fill_diagonal(c, nsites * (1.0 - p) / 4.0)
    return c


@pytest.mark.parametrize("p", [0.01, 0.1, 0.3, 0.5, 0.7])
def test_jc_closed_form(synth, p):
    jc = synth.reversible_model(np.ones((4, 4)), np.full(4, 0.25))
    want = -0.75 * np.log(1.0 - 4.0 * p / 3.0)
    counts = jc_counts(p)
    assert abs(restate_jc(counts) - want) <= 1e-12
    # from a start that is not the optimum.  minimizeNewton returns the iterate BEFORE the first step shorter than xacc, so
    # the optimum is located to xacc, not to its square: the reference's xacc = 1e-6 cannot give 1e-9, xacc = 1e-11 does
    optx, d2l, pts = restate_solve(counts, jc, init=1.7 * want + 0.05, xacc=1e-11)
    assert abs(optx - want) <= 1e-9, (optx, want, pts)
    assert d2l > 0.0 and len(pts) >= 2


@pytest.mark.parametrize("kind", ["gtr_g4", "prot_g4", "r4"])
def test_derivatives_agree_with_central_differences(pkg, synth, kind):
    n, _, states, freq, model, _ = dist_case(pkg, synth, kind, 5, 65)
    counts = restate_counts(states, freq, n, [(0, 1)])[0]
    for t in (0.05, 0.3, 1.5):
        df, ddf = restate_func_derv(counts, model, t)
        # a central difference D(h) of g has truncation error g''' h^2 / 6 + O(h^4), so D(h) - D(h/2) is three quarters
        # of D(h)'s truncation error and three times that of D(h/2): |D(h/2) - g'| <= |D(h) - D(h/2)| / 3 up to O(h^4);
        # the full difference is allowed (3x headroom for the O(h^4) term).  Rounding adds at most 2 eps |g| / h per
        # quotient (two evaluations of g, each off by a few eps |g|: 8 eps |g| / h allowed).  h = 1e-3 t keeps both small.
        h = 1e-3 * t
        eps = 2.0 ** -52
        for g, want in ((lambda x: restate_function(counts, model, x), df), (lambda x: restate_func_derv(counts, model, x)[0], ddf)):
            D = lambda s: (g(t + s) - g(t - s)) / (2.0 * s)   # noqa: E731
            d1, d2 = D(h), D(h / 2)
            tol = abs(d1 - d2) + 8 * eps * abs(g(t)) / (h / 2)
            assert abs(d2 - want) <= tol, (kind, t, d2, want, tol)
            assert tol <= 1e-4 * abs(want)   # (the check is not vacuous)


@pytest.mark.parametrize("kind", ["gtr_g4", "dna_12", "prot_g4", "i_g4"])
def test_unweighted_sum_is_the_weighted_one_for_equal_proportions(pkg, synth, kind):
    n, _, states, freq, model, _ = dist_case(pkg, synth, kind, 5, 65)
    assert np.ptp(model.props) == 0.0
    for counts in restate_counts(states, freq, n, [(0, 1), (1, 3)]):
        for t in (1e-6, 0.2, 9.0):
            a, b = restate_func_derv(counts, model, t), restate_func_derv(counts, model, t, weighted=False)
            assert abs(a[0] - b[0]) <= 1e-13 * abs(a[0]) and abs(a[1] - b[1]) <= 1e-13 * abs(a[1]), (kind, t, a, b)


def test_counts_skip_ambiguous_states():
    states = np.array([[0, 1, 4, 18, 3, 3], [0, 2, 1, 0, 18, 3]], dtype=np.uint8)
    c = restate_counts(states, [1, 2, 3, 4, 5, 6], 4, [(0, 1), (1, 0)])
    want = np.zeros((4, 4))
    want[0, 0], want[1, 2], want[3, 3] = 1, 2, 6
    np.testing.assert_array_equal(c[0], want)
    np.testing.assert_array_equal(c[1], want.T)


def test_symbols(pkg):
    src = open(os.path.join(ROOT, "include", "iqhip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = pkg.libiqhip()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in pkg.IQHIP_SYMBOLS and hasattr(lib, name), name
    assert lib.iqhip_abi_version() == 2


def test_planning_only_engine_refuses(pkg):
    lib = pkg.libiqhip()
    e = C.c_void_p()
    assert lib.iqhip_debug_create_planner(C.byref(e), 4, 4, 1000, 5, 256, 18, 1) == 0
    pairs = np.array([0, 1], dtype=np.int32)
    counts, dist = np.zeros(16), np.zeros(25)
    dp = C.POINTER(C.c_double)
    assert lib.iqhip_pair_counts(e, pairs.ctypes.data_as(C.POINTER(C.c_int32)), 1, counts.ctypes.data_as(dp)) == IQHIP_ERR_INVALID
    assert b"planning-only" in lib.iqhip_last_error()
    assert lib.iqhip_pair_distances(e, None, X1, X2, XACC, MAX_STEPS, dist.ctypes.data_as(dp), None, None) == IQHIP_ERR_INVALID
    assert b"planning-only" in lib.iqhip_last_error()
    lib.iqhip_destroy(e)


@pytest.mark.parametrize("kind", KINDS)
def test_cases_hold_what_the_device_tests_need(pkg, synth, kind):
    """the smaller shape of every model on the CPU: no pair trips the guard, and every required situation occurs (the
    larger shape is solved in tests/test_pair_dist_gpu.py, where the same asserts run)"""
    ntaxa, nptn = SHAPES[0]
    _, _, states, freq, model, init = dist_case(pkg, synth, kind, ntaxa, nptn)
    stats = collections.Counter()
    dist, d2l, nst = restate_matrix(states, freq, model, init, stats)
    assert_case_stats(stats, ntaxa)
    assert dist[0, ntaxa - 3] == X1 and dist[1, ntaxa - 1] == MAX_GENETIC_DIST and nst[1, ntaxa - 1] == 1
