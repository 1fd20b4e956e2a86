"""A numpy restatement of likelihood mapping (quartet.cpp of the reference; include/iqhip.h "Likelihood mapping"): the
expected values of tests/test_lmap_host.py and tests/test_lmap_gpu.py.

  sub_alignment     the columns of a quartet and their compression (np.unique over the columns of frequency > 0)
  cells_ref         the 256 cells and the other-list of a quartet
  start_lengths     fixNegativeBranch(true): Fitch through tests/fitch_ref.py over the informative columns, JC correction
  quartet_tree_ref  optimizeAllBranches(iterations, tolerance) on oracle_driver.OracleTree (4 leaves): minimize_newton per
                    branch in the order of computeBestTraversal (derived here from the adjacency, not from a table), the
                    diverged-solve rule, lnl_from_theta after every sweep, the restore rule; the scale counters of every
                    vector are asserted to be 0
  weights_ref / region_ref   the Bayesian weights, the corner and the region of three log-likelihoods

The guard: a quartet tree is flagged (`guard` non-empty) when a discrete decision could legitimately differ between two
correct implementations -- a Newton stop test within 1e-6 relative of xacc (the rule of tests/test_solver_paths_gpu.py), or a
sweep-stop / lnL-decrease comparison within 1e-7 of its threshold."""
import math
import sys

import numpy as np

import fitch_ref

QC = (0, 1, 2, 3, 0, 2, 1, 3, 0, 3, 1, 2)   # quartet.cpp:925
NEWICK = "(0,1,(2,3));"
X1, X2, MAX_STEPS, DIVERGE = 1e-6, 100.0, 100, 0.95
SU = 18
MASKS = fitch_ref.state_masks(4)


# ---- columns, cells ---------------------------------------------------------------------------------------------------
def sub_alignment(states, freq, quartet):
    """(columns [4, m], weights [m]) of the quartet's compressed sub-alignment; frequency-0 patterns are dropped"""
    st = np.asarray(states)[list(quartet)]
    f = np.asarray(freq, dtype=np.float64)
    keep = f > 0
    cols, inv = np.unique(st[:, keep], axis=1, return_inverse=True)
    w = np.zeros(cols.shape[1])
    np.add.at(w, np.asarray(inv).reshape(-1), f[keep])
    return np.ascontiguousarray(cols, dtype=np.uint8), w


def cells_ref(states, freq, quartet):
    """(cells [4, 4, 4, 4], other: the pattern indices with a state >= 4 among the four, in pattern order)"""
    st = np.asarray(states)[list(quartet)].astype(np.int64)
    f = np.asarray(freq, dtype=np.float64)
    cells = np.zeros((4, 4, 4, 4))
    plain = np.all(st < 4, axis=0) & (f > 0)
    np.add.at(cells, tuple(st[:, plain]), f[plain])
    other = np.nonzero(~np.all(st < 4, axis=0) & (f > 0))[0]
    return cells, other


def const_char_of(cols):
    """computeConst on every column [4, m]: the one state every sequence allows, 4 for a column of unknowns only, -1 else"""
    m = np.array(MASKS)[np.asarray(cols).astype(np.int64)]
    common = m[0] & m[1] & m[2] & m[3]
    out = np.full(common.shape, -1, dtype=np.int64)
    for p, c in enumerate(common):
        if c == 15:
            out[p] = 4
        elif bin(int(c)).count("1") == 1:
            out[p] = int(c).bit_length() - 1
    return out


def const_invar_of(cols, const_invar):
    """the invariant term of every column: const_invar[const_char], 0 where the column is not constant"""
    out = np.zeros(np.asarray(cols).shape[1])
    if const_invar is None:
        return out
    cc = const_char_of(cols)
    out[cc >= 0] = np.asarray(const_invar, dtype=np.float64)[cc[cc >= 0]]
    return out


# ---- starting lengths --------------------------------------------------------------------------------------------------
def quartet_adj():
    return {0: [4], 1: [4], 2: [5], 3: [5], 4: [0, 1, 5], 5: [2, 3, 4]}


def start_lengths(cols, w, nsite, x1=X1):
    """{(a, b): length} of the tree (0,1,(2,3)) over the columns cols [4, m]: fixNegativeBranch(true)"""
    inf = fitch_ref.is_informative(cols, 4)
    site_ptn = fitch_ref.site_patterns(w, inf)
    tips = fitch_ref.tip_vectors(cols, site_ptn, 4)
    adj = quartet_adj()
    dv = fitch_ref.directed_vectors(adj, {t: tips[t] for t in range(4)})
    out = {}
    for a, b in fitch_ref.branches(adj):
        subst = fitch_ref.branch_score(dv[(a, b)], dv[(b, a)])[1]
        bl = subst / nsite if subst > 0 else 1.0 / nsite
        z = 4.0 / 3.0
        x = 1.0 - z * bl
        if x > 0:
            bl = -np.log(x) / z
        out[(a, b)] = max(bl, x1)
    return out


# ---- the traversal order -------------------------------------------------------------------------------------------------
def preorder_branches(ot):
    """optimizeAllBranches' branch order: the farthest leaf from leaf 0, edge-count heights from there, pre-order with the
    neighbours taken by ascending height (the exchange sort of mtree.cpp:2102-2113)"""
    far = ot.farthest_leaf(0)
    height = {}

    def heights(node, dad):
        height[node] = 0
        if dad is not None and ot.is_leaf(node):
            return
        for nb, _ in ot.adj[node]:
            if nb != dad:
                heights(nb, node)
                height[node] = max(height[node], height[nb] + 1)

    heights(far, None)
    out = []

    def walk(node, dad):
        if dad is not None:
            out.append((node, dad))
        nei = [nb for nb, _ in ot.adj[node]]
        for i in range(len(nei)):
            for j in range(i + 1, len(nei)):
                if height[nei[i]] > height[nei[j]]:
                    nei[i], nei[j] = nei[j], nei[i]
        for nb in nei:
            if nb != dad:
                walk(nb, node)

    walk(far, None)
    return out


# ---- optimizeAllBranches ---------------------------------------------------------------------------------------------
GUARD_LNL = 1e-7   # a sweep-stop or lnL-decrease comparison this close to its threshold is not decided by the method


def _solve(ot, a, b, cur, x1, x2, xacc, max_steps, theta, guard):
    optx, _, pts, status = ot.minimize_newton(a, b, x1, cur, x2, xacc, max_steps, theta=theta)
    assert status == "ok", status
    xl, xh = x1, x2
    for x in pts:   # the walk of tests/test_solver_paths_gpu.py oracle_solve
        df, ddf = ot.derv(a, b, length=x, theta=theta)
        f, df = -df, -ddf
        if f < 0.0:
            xl = x
        else:
            xh = x
        bisect = df <= 0.0 or ((x - xh) * df - f) * ((x - xl) * df - f) >= 0.0
        dx = 0.5 * (xh - xl) if bisect else f / df
        if not (abs(abs(dx) - xacc) > 1e-6 * xacc and abs(abs(f) - xacc) > 1e-6 * xacc):
            guard.append(("newton", a, b, x, dx, f))
    return optx, len(pts)


def _assert_unscaled(ot):
    for (frm, to), (_, sc, sf) in ot.cache.items():
        assert sf == 0.0 and not np.any(sc), ("a scale counter moved", frm, to)


def optimize_all_branches(ot, iterations, tolerance, x1=X1, x2=X2, max_steps=MAX_STEPS, diverge=DIVERGE):
    """-> dict(logl, nsweeps, neval, guard, stats); ot keeps the optimised lengths"""
    order = preorder_branches(ot)
    guard, stats = [], dict(lower=0, upper=0, diverged=0, restored=0, limit=0)
    n1, n2 = order[0]
    tree_lh = ot.branch_lnl(n1, n2)[0]
    nsweeps = neval = 0
    for _ in range(iterations):
        saved = {(a, b): ot.length(a, b) for a, b in order}
        theta = sf = None
        changed = False
        for a, b in order:
            cur = ot.length(a, b)
            theta, sf = ot.theta(a, b)
            _assert_unscaled(ot)
            optx, n = _solve(ot, a, b, cur, x1, x2, x1, max_steps, theta, guard)
            neval += n
            if optx > diverge * x2:
                stats["diverged"] += 1
                opt_lh = ot.lnl_from_theta(a, b, length=optx, theta=theta, sf=sf)[0]
                orig_lh = ot.lnl_from_theta(a, b, length=cur, theta=theta, sf=sf)[0]
                if orig_lh > opt_lh:
                    optx = cur
            stats["lower"] += int(optx - x1 <= 2 * x1)
            stats["upper"] += int(optx > 0.5 * x2)
            if optx != cur:
                changed = True
                ot.set_length(a, b, optx)   # (drops the cached vectors; theta of this branch does not depend on its length)
        nsweeps += 1
        a, b = order[-1]
        new_lh = ot.lnl_from_theta(a, b, length=ot.length(a, b), theta=theta, sf=sf)[0]
        # (a sweep that changed no length recomputes the same value: equal on every implementation, no decision to guard)
        if abs(new_lh - tree_lh) <= GUARD_LNL and (changed or nsweeps == 1):
            guard.append(("decrease", new_lh, tree_lh))
        if abs(new_lh - (tree_lh + tolerance)) <= GUARD_LNL:
            guard.append(("stop", new_lh, tree_lh + tolerance))
        if new_lh < tree_lh:
            stats["restored"] += 1
            for (a, b), ln in saved.items():
                ot.set_length(a, b, ln)
            tree_lh = ot.likelihood(0)[0]
            _assert_unscaled(ot)
            return dict(logl=tree_lh, nsweeps=nsweeps, neval=neval, guard=guard, stats=stats)
        stop = tree_lh <= new_lh <= tree_lh + tolerance
        tree_lh = new_lh
        if stop:
            break
    else:
        stats["limit"] += 1
    _assert_unscaled(ot)
    return dict(logl=tree_lh, nsweeps=nsweeps, neval=neval, guard=guard, stats=stats)


def quartet_tree_ref(od, states, freq, quartet, k, model, nsite, iterations=10, tolerance=0.1, const_invar=None):
    """topology k of the quartet -> dict(logl, len [5]: pendant branches of the tree's four taxa then the internal one, start
    [5] likewise, nsweeps, neval, guard, stats, nitems)"""
    taxa = [quartet[QC[4 * k + j]] for j in range(4)]
    cols, w = sub_alignment(states, freq, taxa)
    start = start_lengths(cols, w, nsite)
    nwk = "(0:%.17g,1:%.17g,(2:%.17g,3:%.17g):%.17g);" % (start[(0, 4)], start[(1, 4)], start[(2, 5)], start[(3, 5)], start[(4, 5)])
    ot = od.OracleTree(nwk, 4, od.SEQ_DNA, cols, w, const_invar_of(cols, const_invar), model)
    for key, ln in start.items():
        assert ot.length(*key) == ln
    out = optimize_all_branches(ot, iterations, tolerance)
    keys = [(0, 4), (1, 4), (2, 5), (3, 5), (4, 5)]
    out["len"] = np.array([ot.length(*kk) for kk in keys])
    out["start"] = np.array([start[kk] for kk in keys])
    out["nitems"] = cols.shape[1]
    return out


# ---- weights, regions ----------------------------------------------------------------------------------------------------
def order3(v):
    """descending order of three values, ties as the comparison tree of quartet.cpp:974-1005 leaves them"""
    if v[0] > v[1]:
        if v[2] > v[0]:
            return (2, 0, 1)
        return (0, 1, 2) if v[2] < v[1] else (0, 2, 1)
    if v[2] > v[1]:
        return (2, 1, 0)
    return (1, 0, 2) if v[2] < v[0] else (1, 2, 0)


def weights_ref(logl):
    o = order3(logl)
    w = np.zeros(3)
    w[o[0]] = 1.0
    for k in (1, 2):
        d = logl[o[k]] - logl[o[0]]
        w[o[k]] = 0.0 if d < -40.0 else math.exp(d)   # (the C library's exp, as the mirror)
    return w / (w[0] + w[1] + w[2]), o


def region_ref(logl):
    """-> (weights, corner, region)"""
    w, o = weights_ref(logl)
    targets = (np.array([1.0, 0.0, 0.0]), np.array([0.5, 0.5, 0.0]), np.array([1.0 / 3.0] * 3))
    ws = np.array([w[o[0]], w[o[1]], w[o[2]]])
    sq = [float(np.sum((t - ws) ** 2)) for t in targets]
    bits = (1 << o[0], (1 << o[0]) + (1 << o[1]), 7)
    nearest = order3(sq)[2]
    area = {1: 0, 2: 1, 4: 2, 3: 3, 6: 4, 5: 5, 7: 6}[bits[nearest]]
    return w, o[0], area


# ---- the test inputs -----------------------------------------------------------------------------------------------------
# name -> (seed, sites); the seeds were chosen on the CPU with this file alone so that the guard rejects no quartet tree
CASES = {"jc": (7574, 260), "gtr_g4": (106, 300), "gtr_i_g4": (100, 300), "hky_r3": (108, 280), "wide10": (101, 240)}


def case_model(synth, name):
    """-> (model, const_invar or None)"""
    freqs = np.array([0.3, 0.2, 0.22, 0.28])
    if name == "jc":
        return synth.reversible_model(np.ones((4, 4)), np.full(4, 0.25), None, 1, name="JC"), None
    if name == "gtr_g4":
        return synth.gtr_model(), None
    if name == "gtr_i_g4":
        m = synth.gtr_model(pinvar=0.2)
        return m, np.concatenate([m.pinvar * m.freqs, [m.pinvar]])
    if name == "hky_r3":
        k = 2.0
        m = synth.reversible_model(np.array([[0, 1, k, 1], [1, 0, 1, k], [k, 1, 0, 1], [1, k, 1, 0]], dtype=float), freqs, 0.8, 3,
                                   name="HKY+R3")
        props = np.array([0.5, 0.3, 0.2])
        rates = np.array([0.2, 1.0, 3.0])
        m.props = props
        m.rates = rates / float(props @ rates)
        return m, None
    if name == "wide10":
        return synth.gtr_model(alpha=0.6, ncat=10), None
    raise KeyError(name)


def lmap_case(synth, name, ntaxa=6, seed=None):
    """dict(states [ntaxa, nptn], freq, model, const_invar, nsite): taxon 1 repeats taxon 0, taxon ntaxa - 2 holds independent
    random states, taxon ntaxa - 1 is gap-only; ambiguity codes and unknowns in the others; three all-gap columns"""
    nsites = CASES[name][1]
    seed = CASES[name][0] if seed is None else seed
    model, const_invar = case_model(synth, name)
    rng = np.random.default_rng(seed)
    nwk = synth.random_tree_newick(ntaxa, seed, lo=0.05, hi=0.6)
    sim_model = synth.gtr_model() if name in ("gtr_i_g4", "wide10") else model
    st = synth.simulate_alignment(nwk, sim_model, nsites, seed + 1).astype(np.uint8)
    if name == "gtr_i_g4":
        st[:, : nsites // 5] = st[0, : nsites // 5]          # invariable sites
    st[1] = st[0]
    st[ntaxa - 2] = rng.integers(0, 4, nsites)
    amb = rng.random(st.shape) < 0.06
    amb[[0, 1, ntaxa - 2]] = False
    st[amb] = rng.integers(4, SU + 1, int(amb.sum()))
    st[ntaxa - 1] = SU
    st[:, -3:] = SU
    pat, freq = synth.compress_patterns(st)
    return dict(name=name, states=np.ascontiguousarray(pat), freq=freq, model=model, const_invar=const_invar,
                nsite=float(freq.sum()))


sys.setrecursionlimit(max(sys.getrecursionlimit(), 10000))
