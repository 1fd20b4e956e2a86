// brent_host.h -- Optimization::minimizeOneDimen over brent_opt (optimization.cpp:183-276, 288-335) as a resumable state
// machine, in the style of the engine's iqhip_newton_host_* trio: init() gives the first x, update(f(x)) gives the next x
// or reports done, then optx / fx / nevals are the result.  The caller owns the function; the order of evaluations is the
// reference's: bx, ax, cx; the bounds when the first bracket fails; Brent's iteration; and the start point once more when
// the iteration ended on a worse value ("if worse, return initial value", :332-336; restated, although brent_opt replaces
// its best point only by a value <= the best so far, which starts as f(bx), so the rule cannot fire).  Pure host
// arithmetic, no device.
#pragma once
#include <cmath>

namespace iqhost {

struct BrentMachine {
    // result
    double optx = 0.0, fx_opt = 0.0;
    int nevals = 0;
    bool done = true;

    double init(double xmin_, double xguess, double xmax_, double tolerance) {
        xmin = xmin_;
        xmax = xmax_;
        tol = tolerance;
        if (xguess < xmin) xguess = xmin;
        if (xguess > xmax) xguess = xmax;
        const double eps = xguess * tolerance * 50.0;
        ax = xguess - eps;
        if (ax < xmin) ax = xmin;
        bx = xguess;
        cx = xguess + eps;
        if (cx > xmax) cx = xmax;
        nevals = 0;
        done = false;
        phase = EVAL_B;
        return cur = bx;
    }

    // f = the function at the x last handed out; returns the next x (meaningless once done)
    double update(double f) {
        if (done) return cur;
        nevals++;
        switch (phase) {
        case EVAL_B:
            fb = f;
            phase = EVAL_A;
            return cur = ax;
        case EVAL_A:
            fa = f;
            phase = EVAL_C;
            return cur = cx;
        case EVAL_C:
            fc = f;
            if ((fa < fb) || (fc < fb)) {   // the bracket failed: be conservative, take the bounds
                if (ax != xmin) {
                    phase = EVAL_MIN;
                    return cur = xmin;
                }
                if (cx != xmax) {
                    phase = EVAL_MAX;
                    return cur = xmax;
                }
                ax = xmin;
                cx = xmax;
            }
            return brentStart();
        case EVAL_MIN:
            fa = f;
            if (cx != xmax) {
                phase = EVAL_MAX;
                return cur = xmax;
            }
            ax = xmin;
            cx = xmax;
            return brentStart();
        case EVAL_MAX:
            fc = f;
            ax = xmin;
            cx = xmax;
            return brentStart();
        case BRENT: {
            const double fu = f;
            if (fu <= fx) {
                if (u >= x) a = x; else b = x;
                v = w; w = x; x = u;
                fv = fw; fw = fx; fx = fu;
            } else {
                if (u < x) a = u; else b = u;
                if (fu <= fw || w == x) {
                    v = w; w = u;
                    fv = fw; fw = fu;
                } else if (fu <= fv || v == x || v == w) {
                    v = u;
                    fv = fu;
                }
            }
            iter++;
            return brentPropose();
        }
        case EVAL_START:
            fx_opt = f;
            optx = bx;
            done = true;
            return cur = bx;
        }
        return cur;
    }

private:
    enum Phase { EVAL_B, EVAL_A, EVAL_C, EVAL_MIN, EVAL_MAX, BRENT, EVAL_START };
    static constexpr int ITMAX = 100;
    static constexpr double CGOLD = 0.3819660, ZEPS = 1.0e-10;
    Phase phase = EVAL_B;
    double xmin = 0, xmax = 0, tol = 0, cur = 0;
    double ax = 0, bx = 0, cx = 0, fa = 0, fb = 0, fc = 0;
    double a = 0, b = 0, d = 0, e = 0, u = 0, v = 0, w = 0, x = 0, fv = 0, fw = 0, fx = 0;
    int iter = 0;

    static double sign(double p, double q) { return q >= 0.0 ? std::fabs(p) : -std::fabs(p); }

    double brentStart() {
        d = 0.0;
        e = 0.0;
        a = (ax < cx ? ax : cx);
        b = (ax > cx ? ax : cx);
        x = bx;
        fx = fb;
        if (fa < fc) {
            w = ax; fw = fa;
            v = cx; fv = fc;
        } else {
            w = cx; fw = fc;
            v = ax; fv = fa;
        }
        iter = 1;
        phase = BRENT;
        return brentPropose();
    }

    // the head of brent_opt's loop: converged (or out of iterations) -> finish, else the next trial point
    double brentPropose() {
        if (iter > ITMAX) return finish();
        const double xm = 0.5 * (a + b);
        const double tol1 = tol * std::fabs(x) + ZEPS;
        const double tol2 = 2.0 * tol1;
        if (std::fabs(x - xm) <= (tol2 - 0.5 * (b - a))) return finish();
        if (std::fabs(e) > tol1) {
            const double r = (x - w) * (fx - fv);
            double q = (x - v) * (fx - fw);
            double p = (x - v) * q - (x - w) * r;
            q = 2.0 * (q - r);
            if (q > 0.0) p = -p;
            q = std::fabs(q);
            const double etemp = e;
            e = d;
            if (std::fabs(p) >= std::fabs(0.5 * q * etemp) || p <= q * (a - x) || p >= q * (b - x))
                d = CGOLD * (e = (x >= xm ? a - x : b - x));
            else {
                d = p / q;
                u = x + d;
                if (u - a < tol2 || b - u < tol2) d = sign(tol1, xm - x);
            }
        } else
            d = CGOLD * (e = (x >= xm ? a - x : b - x));
        u = (std::fabs(d) >= tol1 ? x + d : x + sign(tol1, d));
        return cur = u;
    }

    double finish() {
        if (fx > fb) {   // worse than the start: the reference evaluates and returns the start point
            phase = EVAL_START;
            return cur = bx;
        }
        optx = x;
        fx_opt = fx;
        done = true;
        return cur = x;
    }
};

}  // namespace iqhost
