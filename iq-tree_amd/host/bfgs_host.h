// bfgs_host.h -- the first pass of Optimization::minimizeMultiDimen (optimization.cpp:560-607): dfpmin (:623-709) over lnsrch
// (:484-552, with fixBound :148-155) and the forward-difference gradient derivativeFunk (:725-748), as a resumable state
// machine in the style of BrentMachine (brent_host.h).  The caller owns the function.  The machine hands out REQUESTS and
// takes back the function values:
//   STENCIL : ndim + 1 points, row 0 the base point x, row i = x with x[i-1] + h[i-1]; h = ERROR_X |x| (ERROR_X when that is
//             0) and then h = (x + h) - x, exactly as derivativeFunk.  The points are independent of each other: this is the
//             request a caller may evaluate in one batch.  As in the reference they are NOT clamped to the bounds.
//   SINGLE  : one point, a trial of the line search (clamped by fixBound).
// The order of the requests and every point in them are the reference's, bit for bit.  dfpmin uses the value derivativeFunk
// RETURNS (the base point's) at its very first call only (fp, :634); every later call (:663) discards it and keeps the
// line search's value as fp.  The gradient itself is always formed from the stencil's own base value, (f_i - f_0) / h_i.
// The machine restates that: values[0] of a later stencil enters the differences and nothing else.
// NOT restated: the random restart at the boundary (:574-598, random_double).  It runs only for parameters with
// bound_check[i] == true; init() refuses those, and ModelGTR::setBounds (model/modelgtr.cpp:511-519) passes false for all.
// With bound_check false the loop of minimizeMultiDimen runs once and returns dfpmin's fret and point.
// Pure host arithmetic, no device.
#pragma once
#include <cmath>
#include <stdexcept>
#include <vector>

namespace iqhost {

struct BfgsMachine {
    enum Request { STENCIL = 0, SINGLE = 1, DONE = 2 };
    static constexpr double ERROR_X = 1.0e-4;                 // optimization.cpp:23
    static constexpr double ALF = 1.0e-4, LNSRCH_TOLX = 1.0e-7;   // :478-479
    static constexpr double EPS = 3.0e-8, TOLX = 4 * EPS, STPMX = 100.0;   // :613-615
    static constexpr int ITMAX = 200;                         // :610

    // the pending request: STENCIL -> points [(n + 1)][n] and steps h [n]; SINGLE -> points [n]
    Request request = DONE;
    std::vector<double> points, h;
    // result (once request == DONE): the point, minimizeMultiDimen's return value, dfpmin's *iter; counts of what was asked
    std::vector<double> x;
    double fret = 0.0;
    int iter = 0, nstencils = 0, nsingles = 0;
    // the gradient of the last stencil (what derivativeFunk wrote to dfx)
    std::vector<double> g;

    int ndim() const { return n; }
    int npoints() const { return request == STENCIL ? n + 1 : request == SINGLE ? 1 : 0; }

    void init(int ndim, const double *guess, const double *lower_, const double *upper_, const bool *bound_check, double gtol_) {
        if (ndim < 1) throw std::runtime_error("BfgsMachine: at least one dimension");
        for (int i = 0; i < ndim; i++) {
            if (bound_check && bound_check[i])
                throw std::runtime_error("BfgsMachine: bound_check = true (the random restart at the boundary) is not restated");
            if (!(lower_[i] <= upper_[i]) || guess[i] != guess[i]) throw std::runtime_error("BfgsMachine: bad bounds");
        }
        n = ndim;
        gtol = gtol_;
        x.assign(guess, guess + n);
        lower.assign(lower_, lower_ + n);
        upper.assign(upper_, upper_ + n);
        g.assign(n, 0.0);
        dg.assign(n, 0.0);
        hdg.assign(n, 0.0);
        xi.assign(n, 0.0);
        pnew.assign(n, 0.0);
        hessin.assign((size_t)n * n, 0.0);
        h.assign(n, 0.0);
        fret = 0.0;
        iter = nstencils = nsingles = 0;
        first_stencil = true;
        askStencil();
    }

    // values: the function at the points of the pending request, in their order
    void update(const double *values) {
        if (request == STENCIL) {
            const double fx = values[0];
            for (int d = 0; d < n; d++) g[d] = (values[1 + d] - fx) / h[d];   // :744-745
            if (first_stencil) {   // :634-644
                first_stencil = false;
                fp = fx;
                double sum = 0.0;
                for (int i = 0; i < n; i++) {
                    for (int j = 0; j < n; j++) hessin[(size_t)i * n + j] = 0.0;
                    hessin[(size_t)i * n + i] = 1.0;
                    xi[i] = -g[i];
                    sum += x[i] * x[i];
                }
                stpmax = STPMX * fmax_(std::sqrt(sum), (double)n);
                its = 1;
                iter = its;
                lnsrchStart();
                return;
            }
            afterGradient();
        } else if (request == SINGLE)
            lnsrchValue(values[0]);
    }

private:
    int n = 0, its = 0;
    double gtol = 0.0, fp = 0.0, stpmax = 0.0;
    bool first_stencil = true;
    std::vector<double> lower, upper, dg, hdg, xi, pnew, hessin;
    // lnsrch
    double alam = 0, alam2 = 0, alamin = 0, f2 = 0, fold2 = 0, slope = 0, f_ls = 0;
    bool first_time = true;

    static double fmax_(double a, double b) { return a > b ? a : b; }   // FMAX (:481-482)
    static double sqr(double a) { return a == 0.0 ? 0.0 : a * a; }      // SQR (:612)

    void askStencil() {   // derivativeFunk :734-743
        points.assign((size_t)(n + 1) * n, 0.0);
        for (int r = 0; r <= n; r++)
            for (int i = 0; i < n; i++) points[(size_t)r * n + i] = x[i];
        for (int d = 0; d < n; d++) {
            const double temp = x[d];
            h[d] = ERROR_X * std::fabs(temp);
            if (h[d] == 0.0) h[d] = ERROR_X;
            volatile double moved = temp + h[d];   // (a stored double, as x[dim] is in the reference)
            h[d] = moved - temp;
            points[(size_t)(1 + d) * n + d] = moved;
        }
        request = STENCIL;
        nstencils++;
    }

    void lnsrchStart() {   // :490-503, xold = x, fold = fp, the direction xi
        double sum = 0.0;
        for (int i = 0; i < n; i++) sum += xi[i] * xi[i];
        sum = std::sqrt(sum);
        if (sum > stpmax)
            for (int i = 0; i < n; i++) xi[i] *= stpmax / sum;
        slope = 0.0;
        for (int i = 0; i < n; i++) slope += g[i] * xi[i];
        double test = 0.0;
        for (int i = 0; i < n; i++) {
            const double temp = std::fabs(xi[i]) / fmax_(std::fabs(x[i]), 1.0);
            if (temp > test) test = temp;
        }
        alamin = LNSRCH_TOLX / test;
        alam = 1.0;
        alam2 = f2 = fold2 = 0.0;
        first_time = true;
        lnsrchPropose();
    }

    void lnsrchPropose() {   // :517-520
        for (int i = 0; i < n; i++) pnew[i] = x[i] + alam * xi[i];
        for (int i = 0; i < n; i++) {   // fixBound :148-155
            if (pnew[i] < lower[i]) pnew[i] = lower[i];
            else if (pnew[i] > upper[i]) pnew[i] = upper[i];
        }
        points = pnew;
        request = SINGLE;
        nsingles++;
    }

    void lnsrchValue(double f) {   // :521-550
        const double fold = fp;
        f_ls = f;
        if (alam < alamin) {
            for (int i = 0; i < n; i++) pnew[i] = x[i];
            afterLnsrch();
            return;
        } else if (f <= fold + ALF * alam * slope) {
            afterLnsrch();
            return;
        }
        double tmplam;
        if (first_time)
            tmplam = -slope / (2.0 * (f - fold - slope));
        else {
            const double rhs1 = f - fold - alam * slope;
            const double rhs2 = f2 - fold2 - alam2 * slope;
            const double a = (rhs1 / (alam * alam) - rhs2 / (alam2 * alam2)) / (alam - alam2);
            const double b = (-alam2 * rhs1 / (alam * alam) + alam * rhs2 / (alam2 * alam2)) / (alam - alam2);
            if (a == 0.0) tmplam = -slope / (2.0 * b);
            else {
                const double disc = b * b - 3.0 * a * slope;
                if (disc < 0.0) tmplam = 0.5 * alam;
                else if (b <= 0.0) tmplam = (-b + std::sqrt(disc)) / (3.0 * a);
                else tmplam = -slope / (b + std::sqrt(disc));
            }
            if (tmplam > 0.5 * alam) tmplam = 0.5 * alam;
        }
        alam2 = alam;
        f2 = f;
        fold2 = fold;
        alam = fmax_(tmplam, 0.1 * alam);
        first_time = false;
        lnsrchPropose();
    }

    void afterLnsrch() {   // dfpmin :648-663
        fret = f_ls;
        fp = fret;
        for (int i = 0; i < n; i++) {
            xi[i] = pnew[i] - x[i];
            x[i] = pnew[i];
        }
        double test = 0.0;
        for (int i = 0; i < n; i++) {
            const double temp = std::fabs(xi[i]) / fmax_(std::fabs(x[i]), 1.0);
            if (temp > test) test = temp;
        }
        if (test < TOLX) {
            finish();
            return;
        }
        for (int i = 0; i < n; i++) dg[i] = g[i];
        askStencil();
    }

    void afterGradient() {   // dfpmin :664-705
        double test = 0.0;
        const double den = fmax_(std::fabs(fret), 1.0);
        for (int i = 0; i < n; i++) {
            const double temp = std::fabs(g[i]) * fmax_(std::fabs(x[i]), 1.0) / den;
            if (temp > test) test = temp;
        }
        if (test < gtol) {
            finish();
            return;
        }
        for (int i = 0; i < n; i++) dg[i] = g[i] - dg[i];
        for (int i = 0; i < n; i++) {
            hdg[i] = 0.0;
            for (int j = 0; j < n; j++) hdg[i] += hessin[(size_t)i * n + j] * dg[j];
        }
        double fac = 0.0, fae = 0.0, sumdg = 0.0, sumxi = 0.0;
        for (int i = 0; i < n; i++) {
            fac += dg[i] * xi[i];
            fae += dg[i] * hdg[i];
            sumdg += sqr(dg[i]);
            sumxi += sqr(xi[i]);
        }
        if (fac * fac > EPS * sumdg * sumxi) {
            fac = 1.0 / fac;
            const double fad = 1.0 / fae;
            for (int i = 0; i < n; i++) dg[i] = fac * xi[i] - fad * hdg[i];
            for (int i = 0; i < n; i++)
                for (int j = 0; j < n; j++)
                    hessin[(size_t)i * n + j] += fac * xi[i] * xi[j] - fad * hdg[i] * hdg[j] + fae * dg[i] * dg[j];
        }
        for (int i = 0; i < n; i++) {
            xi[i] = 0.0;
            for (int j = 0; j < n; j++) xi[i] -= hessin[(size_t)i * n + j] * g[j];
        }
        its++;
        if (its > ITMAX) {   // (the loop ran out: *iter stays ITMAX)
            finish();
            return;
        }
        iter = its;
        lnsrchStart();
    }

    void finish() {
        points.clear();
        request = DONE;
    }
};

}  // namespace iqhost
