"""Plain restatements, used by tests/test_em_host.py and tests/test_em_gpu.py, of
  Optimization::minimizeOneDimen over brent_opt   (one-dimensional minimiser: the first bracket bx, ax, cx, the fall-back to
                                                   the bounds, Brent's iteration, "if worse, return the initial value")
  RateFree::optimizeWithEM                        (EM for +R weights and rates; the rate of each category by the minimiser
                                                   above on a one-category tree, ONE CATEGORY AT A TIME)
  RateGamma::computePatternRates                  (posterior mean rate and best category per pattern)
as direct Python: the function is called where the algorithm needs it.  Every evaluation point is recorded,
so that a resumable state machine can be required to visit the same points in the same order."""
import numpy as np

ITMAX = 100
CGOLD = 0.3819660
ZEPS = 1.0e-10


def _sign(a, b):
    return abs(a) if b >= 0.0 else -abs(a)


def brent_opt(f, ax, bx, cx, tol, fax, fbx, fcx):
    """-> (x, fx)"""
    d = 0.0
    e = 0.0
    a = ax if ax < cx else cx
    b = ax if ax > cx else cx
    x = bx
    fx = fbx
    if fax < fcx:
        w, fw, v, fv = ax, fax, cx, fcx
    else:
        w, fw, v, fv = cx, fcx, ax, fax
    for _ in range(ITMAX):
        xm = 0.5 * (a + b)
        tol1 = tol * abs(x) + ZEPS
        tol2 = 2.0 * tol1
        if abs(x - xm) <= (tol2 - 0.5 * (b - a)):
            return x, fx
        if abs(e) > tol1:
            r = (x - w) * (fx - fv)
            q = (x - v) * (fx - fw)
            p = (x - v) * q - (x - w) * r
            q = 2.0 * (q - r)
            if q > 0.0:
                p = -p
            q = abs(q)
            etemp = e
            e = d
            if abs(p) >= abs(0.5 * q * etemp) or p <= q * (a - x) or p >= q * (b - x):
                e = a - x if x >= xm else b - x
                d = CGOLD * e
            else:
                d = p / q
                u = x + d
                if u - a < tol2 or b - u < tol2:
                    d = _sign(tol1, xm - x)
        else:
            e = a - x if x >= xm else b - x
            d = CGOLD * e
        u = x + d if abs(d) >= tol1 else x + _sign(tol1, d)
        fu = f(u)
        if fu <= fx:
            if u >= x:
                a = x
            else:
                b = x
            v, w, x = w, x, u
            fv, fw, fx = fw, fx, fu
        else:
            if u < x:
                a = u
            else:
                b = u
            if fu <= fw or w == x:
                v, w, fv, fw = w, u, fw, fu
            elif fu <= fv or v == x or v == w:
                v, fv = u, fu
    return x, fx


def minimize_one_dimen(func, xmin, xguess, xmax, tolerance):
    """-> (optx, fx, [every evaluation point in order])"""
    xs = []

    def f(x):
        xs.append(x)
        return func(x)

    if xguess < xmin:
        xguess = xmin
    if xguess > xmax:
        xguess = xmax
    eps = xguess * tolerance * 50.0
    ax = xguess - eps
    if ax < xmin:
        ax = xmin
    bx = xguess
    cx = xguess + eps
    if cx > xmax:
        cx = xmax
    fb = f(bx)
    fa = f(ax)
    fc = f(cx)
    if fa < fb or fc < fb:
        if ax != xmin:
            fa = f(xmin)
        if cx != xmax:
            fc = f(xmax)
        ax = xmin
        cx = xmax
    optx, fx = brent_opt(f, ax, bx, cx, tolerance, fa, fb, fc)
    if fx > fb:
        fx = f(bx)
        return bx, fx, xs
    return optx, fx, xs


def pattern_rates(lh_cat, rates):
    """computePatternRates with the first maximum as the best category -> (rates[nptn], cat[nptn])"""
    lh_cat = np.asarray(lh_cat)
    return (lh_cat * np.asarray(rates)[None, :]).sum(axis=1) / lh_cat.sum(axis=1), lh_cat.argmax(axis=1)


def optimize_with_em(log_lh_at_rate, ptn_freq, props, rates):
    """log_lh_at_rate(s) -> log-likelihood per pattern of the one-category tree of rate s (weight 1).
    -> dict(props, rates, lnl, steps, trace=[dict(lnl_before, evals)])"""
    MIN_PROP = 1e-4
    prop = np.array(props, dtype=np.float64)
    rates = np.array(rates, dtype=np.float64)
    freq = np.asarray(ptn_freq, dtype=np.float64)
    nmix = prop.size
    nsite = freq.sum()

    def log_cat():
        return np.stack([np.log(prop[c]) + log_lh_at_rate(rates[c]) for c in range(nmix)], axis=1)   # [nptn, ncat]

    def total(lc):
        m = lc.max(axis=1)
        return float(np.dot(freq, m + np.log(np.exp(lc - m[:, None]).sum(axis=1))))

    trace = []
    for _ in range(nmix):
        lc = log_cat()
        m = lc.max(axis=1)
        post = np.exp(lc - m[:, None])
        W = post / post.sum(axis=1, keepdims=True) * freq[:, None]
        step = dict(lnl_before=total(lc), evals=[0] * nmix)
        trace.append(step)
        new_prop = W.sum(axis=0) / nsite
        maxpropid = int(np.argmax(new_prop))
        zero_prop = False
        for c in range(nmix):
            if new_prop[c] < MIN_PROP:
                new_prop[maxpropid] -= MIN_PROP - new_prop[c]
                new_prop[c] = MIN_PROP
                zero_prop = True
        if zero_prop:
            break
        converged = bool(np.all(np.abs(prop - new_prop) < 1e-4))
        prop = new_prop.copy()
        for c in range(nmix):
            scaling = rates[c]
            optx, _, xs = minimize_one_dimen(lambda s: -float(np.dot(W[:, c], log_lh_at_rate(s))), min(scaling, MIN_PROP),
                                             scaling, max(1.0 / prop[c], scaling), max(0.001, 0.001))
            step["evals"][c] = len(xs)
            converged = converged and abs(rates[c] - optx) < 1e-4
            rates[c] = optx
        if converged:
            break
    return dict(props=prop, rates=rates, lnl=total(log_cat()), steps=len(trace), trace=trace)
