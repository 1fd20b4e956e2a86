"""A direct Python restatement of the reference's multi-dimensional minimiser, as em_ref.py is for Brent: derivativeFunk
(optimization.cpp:725-748), lnsrch with fixBound (:484-552, :148-155), dfpmin (:623-709) and the first pass of
minimizeMultiDimen (:560-607).  Plain floats, the reference's order of operations, the target function called one point at a
time in the reference's order.  The random restart at the boundary is not restated: bound_check must be all False (as
ModelGTR::setBounds passes it)."""
import math

ERROR_X = 1.0e-4
ALF = 1.0e-4
LNSRCH_TOLX = 1.0e-7
EPS = 3.0e-8
TOLX = 4 * EPS
STPMX = 100.0
ITMAX = 200


def fmax(a, b):
    return a if a > b else b


def sqr(a):
    return 0.0 if a == 0.0 else a * a


def fix_bound(x, lower, upper):
    for i in range(len(x)):
        if x[i] < lower[i]:
            x[i] = lower[i]
        elif x[i] > upper[i]:
            x[i] = upper[i]


def derivative_funk(target, x, dfx):
    """-> f(x); dfx[i] = (f(x + h_i e_i) - f(x)) / h_i"""
    n = len(x)
    h = [0.0] * n
    fx = target(list(x))
    for d in range(n):
        temp = x[d]
        h[d] = ERROR_X * abs(temp)
        if h[d] == 0.0:
            h[d] = ERROR_X
        x[d] = temp + h[d]
        h[d] = x[d] - temp
        dfx[d] = target(list(x))
        x[d] = temp
    for d in range(n):
        dfx[d] = (dfx[d] - fx) / h[d]
    return fx


def lnsrch(target, xold, fold, g, p, x, stpmax, lower, upper):
    """-> (f, check); x receives the new point, p may be rescaled"""
    n = len(xold)
    alam2 = f2 = fold2 = 0.0
    s = 0.0
    for i in range(n):
        s += p[i] * p[i]
    s = math.sqrt(s)
    if s > stpmax:
        for i in range(n):
            p[i] *= stpmax / s
    slope = 0.0
    for i in range(n):
        slope += g[i] * p[i]
    test = 0.0
    for i in range(n):
        temp = abs(p[i]) / fmax(abs(xold[i]), 1.0)
        if temp > test:
            test = temp
    alamin = LNSRCH_TOLX / test if test != 0.0 else math.inf
    alam = 1.0
    first_time = True
    while True:
        for i in range(n):
            x[i] = xold[i] + alam * p[i]
        fix_bound(x, lower, upper)
        f = target(list(x))
        if alam < alamin:
            for i in range(n):
                x[i] = xold[i]
            return f, 1
        elif f <= fold + ALF * alam * slope:
            return f, 0
        else:
            if first_time:
                tmplam = -slope / (2.0 * (f - fold - slope))
            else:
                rhs1 = f - fold - alam * slope
                rhs2 = f2 - fold2 - alam2 * slope
                a = (rhs1 / (alam * alam) - rhs2 / (alam2 * alam2)) / (alam - alam2)
                b = (-alam2 * rhs1 / (alam * alam) + alam * rhs2 / (alam2 * alam2)) / (alam - alam2)
                if a == 0.0:
                    tmplam = -slope / (2.0 * b)
                else:
                    disc = b * b - 3.0 * a * slope
                    if disc < 0.0:
                        tmplam = 0.5 * alam
                    elif b <= 0.0:
                        tmplam = (-b + math.sqrt(disc)) / (3.0 * a)
                    else:
                        tmplam = -slope / (b + math.sqrt(disc))
                if tmplam > 0.5 * alam:
                    tmplam = 0.5 * alam
        alam2 = alam
        f2 = f
        fold2 = fold
        alam = fmax(tmplam, 0.1 * alam)
        first_time = False


def dfpmin(target, p, lower, upper, gtol, gradients=None):
    """p is updated in place -> (iter, fret).  gradients (a list): receives a copy of every gradient derivativeFunk formed"""
    n = len(p)
    g = [0.0] * n
    dg = [0.0] * n
    hdg = [0.0] * n
    pnew = [0.0] * n
    xi = [0.0] * n
    hessin = [[0.0] * n for _ in range(n)]
    fret = 0.0
    fp = derivative_funk(target, p, g)
    if gradients is not None:
        gradients.append(list(g))
    s = 0.0
    for i in range(n):
        for j in range(n):
            hessin[i][j] = 0.0
        hessin[i][i] = 1.0
        xi[i] = -g[i]
        s += p[i] * p[i]
    stpmax = STPMX * fmax(math.sqrt(s), float(n))
    it = 0
    for its in range(1, ITMAX + 1):
        it = its
        fret, _ = lnsrch(target, p, fp, g, xi, pnew, stpmax, lower, upper)
        fp = fret
        for i in range(n):
            xi[i] = pnew[i] - p[i]
            p[i] = pnew[i]
        test = 0.0
        for i in range(n):
            temp = abs(xi[i]) / fmax(abs(p[i]), 1.0)
            if temp > test:
                test = temp
        if test < TOLX:
            return it, fret
        for i in range(n):
            dg[i] = g[i]
        derivative_funk(target, p, g)          # (its return value is not used)
        if gradients is not None:
            gradients.append(list(g))
        test = 0.0
        den = fmax(abs(fret), 1.0)
        for i in range(n):
            temp = abs(g[i]) * fmax(abs(p[i]), 1.0) / den
            if temp > test:
                test = temp
        if test < gtol:
            return it, fret
        for i in range(n):
            dg[i] = g[i] - dg[i]
        for i in range(n):
            hdg[i] = 0.0
            for j in range(n):
                hdg[i] += hessin[i][j] * dg[j]
        fac = fae = sumdg = sumxi = 0.0
        for i in range(n):
            fac += dg[i] * xi[i]
            fae += dg[i] * hdg[i]
            sumdg += sqr(dg[i])
            sumxi += sqr(xi[i])
        if fac * fac > EPS * sumdg * sumxi:
            fac = 1.0 / fac
            fad = 1.0 / fae
            for i in range(n):
                dg[i] = fac * xi[i] - fad * hdg[i]
            for i in range(n):
                for j in range(n):
                    hessin[i][j] += fac * xi[i] * xi[j] - fad * hdg[i] * hdg[j] + fae * dg[i] * dg[j]
        for i in range(n):
            xi[i] = 0.0
            for j in range(n):
                xi[i] -= hessin[i][j] * g[j]
    return it, fret


def minimize_multi_dimen(target, guess, lower, upper, bound_check, gtol, gradients=None):
    """the first pass of minimizeMultiDimen -> dict(x, fret, iter)"""
    if any(bound_check):
        raise ValueError("bound_check = True (the random restart at the boundary) is not restated")
    p = [float(v) for v in guess]
    it, fret = dfpmin(target, p, [float(v) for v in lower], [float(v) for v in upper], gtol, gradients)
    return dict(x=p, fret=fret, iter=it)
