// kernels_bionj.hip -- the BIONJ starting tree (PhyloTree::computeBioNJ, phylotree.cpp:2619-2635; BioNj::create, bionj.h)
// on a distance matrix, all in fp64: the arithmetic is written out in include/iqhip.h ("BIONJ").
//
// Device state of a call: D and V (n x n, both triangles kept equal), S[row], the ordered list of active rows (two
// buffers, a step reads one and writes the other), rowmin[position], one Pick record and the step log.  The host enqueues
// the whole merge loop -- it knows r = n - step, nothing else -- and reads the log once at the end.  Per step:
//   k_bj_rowmin   workgroup x = position of row act[x]: min over y < x of Q_xy.  The scan order of the reference is
//                 "x ascending, then y < x ascending", so the first pair within 1e-6 of the minimum is in the first ROW
//                 whose own minimum is within 1e-6 of it;
//   k_bj_pick     one workgroup: m = min rowmin, that row, the first y in it (Q recomputed by the same expression, hence
//                 the same bits), then la, lb, the lambda sum and the log entry;
//   k_bj_update   row and column a of D and V (formulae 4 and 10), and the active list without b;
//   k_bj_rowsum   S of every active row, recomputed from D as the reference does (Compute_sums_Sx).
// Work per step is about 1.5 r^2 loads (r^2 / 2 for the minima, r^2 for the sums).  No floating-point atomics; every sum
// is a thread-strided partial, the xor butterfly of wave_sum64 and the waves' totals added in wave order: the same bits on
// every run.  Built with -ffp-contract=off (Makefile), like kernels_dist.hip.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <vector>

#include "iqhip_internal.h"

#pragma clang fp contract(off)

namespace iqhip {

constexpr int kBjThreads = 256;
constexpr double kBjPairEps = 1e-6;   // Best_pair's 0.000001, bionj.h:442

struct BjPick {
    int32_t a, b, posa, posb;   // rows and their positions in the active list (a > b, posa > posb)
    double la, lb, lambda, vab;
};

__device__ __forceinline__ double bj_q(double rm2, double dxy, double sx, double sy) { return rm2 * dxy - sx - sy; }

// minimum over the workgroup, every thread gets it (s: kBjThreads values; T is double or int)
template <typename T>
__device__ __forceinline__ T block_min(T v, T *s) {
    __syncthreads();
    s[threadIdx.x] = v;
    __syncthreads();
    for (int w = kBjThreads / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            const T o = s[threadIdx.x + w];
            if (o < s[threadIdx.x]) s[threadIdx.x] = o;
        }
        __syncthreads();
    }
    return s[0];
}

// sum over the workgroup in a fixed order, every thread gets it (s: one double per wave)
__device__ __forceinline__ double block_sum(double v, double *s) {
    const double w = wave_sum64(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = w;
    __syncthreads();
    double tot = s[0];
    for (int k = 1; k < kBjThreads / 64; k++) tot += s[k];
    return tot;
}

// D_ij = (T_ij + T_ji) / 2, diagonal 0
__global__ __launch_bounds__(kBjThreads) void k_bj_sym(const double *__restrict__ T, double *__restrict__ D, int n) {
    const size_t idx = (size_t)blockIdx.x * kBjThreads + threadIdx.x;
    if (idx >= (size_t)n * n) return;
    const size_t i = idx / n, j = idx % n;
    D[idx] = i == j ? 0.0 : (T[idx] + T[j * n + i]) / 2.0;
}

__global__ __launch_bounds__(kBjThreads) void k_bj_iota(int32_t *__restrict__ act, int n) {
    const int k = blockIdx.x * kBjThreads + threadIdx.x;
    if (k < n) act[k] = k;
}

// grid r: S[act[x]] = sum over the other active rows
__global__ __launch_bounds__(kBjThreads) void k_bj_rowsum(const double *__restrict__ D, int n, const int32_t *__restrict__ act,
                                                          int r, double *__restrict__ S) {
    __shared__ double s_w[kBjThreads / 64];
    const int x = blockIdx.x;
    const int i = act[x];
    const double *row = D + (size_t)i * n;
    double part = 0.0;
    for (int k = threadIdx.x; k < r; k += kBjThreads)
        if (k != x) part += row[act[k]];
    const double tot = block_sum(part, s_w);
    if (threadIdx.x == 0) S[i] = tot;
}

// grid r: rowmin[x] = min over y < x of Q(act[x], act[y]); +inf for x = 0
__global__ __launch_bounds__(kBjThreads) void k_bj_rowmin(const double *__restrict__ D, int n, const int32_t *__restrict__ act,
                                                          int r, const double *__restrict__ S, double *__restrict__ rowmin) {
    __shared__ double s_m[kBjThreads];
    const int x = blockIdx.x;
    const int i = act[x];
    const double *row = D + (size_t)i * n;
    const double si = S[i], rm2 = (double)(r - 2);
    double m = INFINITY;
    for (int y = threadIdx.x; y < x; y += kBjThreads) {
        const int j = act[y];
        const double q = bj_q(rm2, row[j], si, S[j]);
        if (q < m) m = q;
    }
    m = block_min(m, s_m);
    if (threadIdx.x == 0) rowmin[x] = m;
}

// one workgroup: the pair, its branch lengths, lambda, the log entry
__global__ __launch_bounds__(kBjThreads) void k_bj_pick(const double *__restrict__ D, const double *__restrict__ V, int n,
                                                        const int32_t *__restrict__ act, int r, const double *__restrict__ S,
                                                        const double *__restrict__ rowmin, BjPick *__restrict__ pick,
                                                        iqhip_bionj_step *__restrict__ log_entry) {
    __shared__ double s_d[kBjThreads];
    __shared__ int s_i[kBjThreads];
    __shared__ double s_w[kBjThreads / 64];
    const int t = threadIdx.x;
    double m = INFINITY;
    for (int x = t; x < r; x += kBjThreads)
        if (rowmin[x] < m) m = rowmin[x];
    m = block_min(m, s_d);
    const double thr = m + kBjPairEps;
    // the first row whose minimum is within the threshold (rows whose minimum is above it hold no candidate) ...
    int px = INT_MAX;
    for (int x = t; x < r; x += kBjThreads)
        if (rowmin[x] <= thr) {
            px = x;
            break;
        }
    px = block_min(px, s_i);
    if (px < 1 || px >= r) px = 1;   // (only when every Q is NaN or infinite: stay inside the arrays)
    const int a = act[px];
    const double *rowa = D + (size_t)a * n;
    const double sa = S[a], rm2 = (double)(r - 2);
    // ... and the first pair of that row
    int py = INT_MAX;
    for (int y = t; y < px; y += kBjThreads) {
        const int j = act[y];
        if (bj_q(rm2, rowa[j], sa, S[j]) <= thr) {
            py = y;
            break;
        }
    }
    py = block_min(py, s_i);
    if (py < 0 || py >= px) py = 0;
    const int b = act[py];
    const double sb = S[b], dab = rowa[b], vab = V[(size_t)a * n + b];
    double lambda = 0.5;
    if (vab != 0.0) {   // (uniform: every thread read the same vab)
        const double *va = V + (size_t)a * n, *vb = V + (size_t)b * n;
        double part = 0.0;
        for (int k = t; k < r; k += kBjThreads)
            if (k != px && k != py) {
                const int i = act[k];
                part += vb[i] - va[i];
            }
        const double sum = block_sum(part, s_w);
        lambda = 0.5 + sum / (2.0 * rm2 * vab);
    }
    if (lambda > 1.0) lambda = 1.0;
    if (lambda < 0.0) lambda = 0.0;
    if (t == 0) {
        const double la = 0.5 * (dab + (sa - sb) / rm2), lb = 0.5 * (dab + (sb - sa) / rm2);
        pick->a = a;
        pick->b = b;
        pick->posa = px;
        pick->posb = py;
        pick->la = la;
        pick->lb = lb;
        pick->lambda = lambda;
        pick->vab = vab;
        log_entry->a = a;
        log_entry->b = b;
        log_entry->la = la;
        log_entry->lb = lb;
        log_entry->lambda = lambda;
    }
}

// grid ceil(r / 256), one thread per position: row / column a of D and V; act_next = act without b
__global__ __launch_bounds__(kBjThreads) void k_bj_update(double *__restrict__ D, double *__restrict__ V, int n,
                                                          const int32_t *__restrict__ act, int r,
                                                          const BjPick *__restrict__ pick, int32_t *__restrict__ act_next) {
    const int k = blockIdx.x * kBjThreads + threadIdx.x;
    if (k >= r) return;
    const BjPick P = *pick;
    if (k == P.posb) return;
    const int i = act[k];
    act_next[k - (k > P.posb ? 1 : 0)] = i;
    if (k == P.posa) return;
    const size_t ai = (size_t)P.a * n + i, bi = (size_t)P.b * n + i, ia = (size_t)i * n + P.a;
    const double lam = P.lambda;
    const double nd = lam * (D[ai] - P.la) + (1.0 - lam) * (D[bi] - P.lb);
    const double nv = lam * V[ai] + (1.0 - lam) * V[bi] - lam * (1.0 - lam) * P.vab;
    D[ai] = nd;
    D[ia] = nd;
    V[ai] = nv;
    V[ia] = nv;
}

// the three rows left, l0 < l1 < l2
__global__ void k_bj_finish(const double *__restrict__ D, int n, const int32_t *__restrict__ act, int32_t *__restrict__ last,
                            double *__restrict__ last_len) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const int l0 = act[0], l1 = act[1], l2 = act[2];
    auto d = [&](int i, int j) { return D[(size_t)i * n + j]; };
    last[0] = l0;
    last[1] = l1;
    last[2] = l2;
    last_len[0] = 0.5 * (d(l0, l1) + d(l0, l2) - d(l1, l2));
    last_len[1] = 0.5 * (d(l1, l0) + d(l1, l2) - d(l0, l2));
    last_len[2] = 0.5 * (d(l2, l1) + d(l2, l0) - d(l1, l0));
}

}  // namespace iqhip

using namespace iqhip;

extern "C" int iqhip_bionj(iqhip_engine *e, int n, const double *dist, const double *var, iqhip_bionj_step *steps,
                           int32_t *last, double *last_len) {
    const int rc = require(e, "iqhip_bionj", REQ_SINGLE_DEVICE);
    if (rc) return rc;
    if (n < 3) return fail(IQHIP_ERR_INVALID, "iqhip_bionj: at least 3 taxa");
    if (!dist || !last || !last_len || (n > 3 && !steps)) return fail(IQHIP_ERR_INVALID, "iqhip_bionj: null argument");
    if (n > 65536)
        return fail(IQHIP_ERR_UNSUPPORTED, "iqhip_bionj: more than 65536 taxa (the pairs no longer fit a 32-bit index)");
    const size_t nn = (size_t)n * n;
    for (const double *m : {dist, var})
        if (m)
            for (size_t i = 0; i < (size_t)n; i++)
                for (size_t j = 0; j < (size_t)n; j++)
                    if (i != j && !std::isfinite(m[i * n + j]))
                        return fail(IQHIP_ERR_INVALID, "iqhip_bionj: a distance or variance is not finite");
    HIPCHK(use_device(e));
    // the device memory of one call, freed on every way out
    DevBuf<double> b_T, b_D, b_V, b_S, b_rowmin, b_last_len;
    DevBuf<int32_t> b_act[2], b_last;
    DevBuf<BjPick> b_pick;
    DevBuf<iqhip_bionj_step> b_steps;
    const int nsteps = n - 3;
    if (b_T.ensure(e, nn) != hipSuccess || b_D.ensure(e, nn) != hipSuccess || b_V.ensure(e, nn) != hipSuccess ||
        b_S.ensure(e, (size_t)n) != hipSuccess || b_rowmin.ensure(e, (size_t)n) != hipSuccess ||
        b_act[0].ensure(e, (size_t)n) != hipSuccess || b_act[1].ensure(e, (size_t)n) != hipSuccess ||
        b_pick.ensure(e, 1) != hipSuccess || b_steps.ensure(e, (size_t)std::max(nsteps, 1)) != hipSuccess ||
        b_last.ensure(e, 3) != hipSuccess || b_last_len.ensure(e, 3) != hipSuccess) {
        (void)hipGetLastError();
        return fail(IQHIP_ERR_NOMEM, "iqhip_bionj: out of device memory (three n x n matrices of doubles)");
    }
    double *d_T = b_T.p, *d_D = b_D.p, *d_V = b_V.p, *d_S = b_S.p, *d_rowmin = b_rowmin.p, *d_last_len = b_last_len.p;
    int32_t *d_act[2] = {b_act[0].p, b_act[1].p}, *d_last = b_last.p;
    BjPick *d_pick = b_pick.p;
    iqhip_bionj_step *d_steps = b_steps.p;
    PhaseTimer timer(e, 1);
    hipStream_t st = e->stream;
    const unsigned nn_blocks = (unsigned)((nn + kBjThreads - 1) / kBjThreads);
    int64_t launches = 0;
    HIPCHK(hipMemcpyAsync(d_T, dist, sizeof(double) * nn, hipMemcpyHostToDevice, st));
    timer.mark();
    hipLaunchKernelGGL(k_bj_sym, dim3(nn_blocks), dim3(kBjThreads), 0, st, d_T, d_D, n);
    launches++;
    if (var) {
        HIPCHK(hipMemcpyAsync(d_T, var, sizeof(double) * nn, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_bj_sym, dim3(nn_blocks), dim3(kBjThreads), 0, st, d_T, d_V, n);
        launches++;
    } else
        HIPCHK(hipMemcpyAsync(d_V, d_D, sizeof(double) * nn, hipMemcpyDeviceToDevice, st));
    hipLaunchKernelGGL(k_bj_iota, dim3((unsigned)((n + kBjThreads - 1) / kBjThreads)), dim3(kBjThreads), 0, st, d_act[0], n);
    launches++;
    int cur = 0;
    if (nsteps > 0) {
        hipLaunchKernelGGL(k_bj_rowsum, dim3((unsigned)n), dim3(kBjThreads), 0, st, d_D, n, d_act[0], n, d_S);
        launches++;
    }
    for (int step = 0; step < nsteps; step++) {
        const int r = n - step;
        hipLaunchKernelGGL(k_bj_rowmin, dim3((unsigned)r), dim3(kBjThreads), 0, st, d_D, n, d_act[cur], r, d_S, d_rowmin);
        hipLaunchKernelGGL(k_bj_pick, dim3(1), dim3(kBjThreads), 0, st, d_D, d_V, n, d_act[cur], r, d_S, d_rowmin, d_pick,
                           d_steps + step);
        hipLaunchKernelGGL(k_bj_update, dim3((unsigned)((r + kBjThreads - 1) / kBjThreads)), dim3(kBjThreads), 0, st, d_D, d_V, n,
                           d_act[cur], r, d_pick, d_act[cur ^ 1]);
        cur ^= 1;
        launches += 3;
        if (r - 1 > 3) {   // (the finish reads D only)
            hipLaunchKernelGGL(k_bj_rowsum, dim3((unsigned)(r - 1)), dim3(kBjThreads), 0, st, d_D, n, d_act[cur], r - 1, d_S);
            launches++;
        }
        if ((step & 255) == 255) HIPCHK(hipGetLastError());
    }
    hipLaunchKernelGGL(k_bj_finish, dim3(1), dim3(64), 0, st, d_D, n, d_act[cur], d_last, d_last_len);
    launches++;
    HIPCHK(hipGetLastError());
    timer.mark();
    if (nsteps > 0) HIPCHK(hipMemcpyAsync(steps, d_steps, sizeof(iqhip_bionj_step) * (size_t)nsteps, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(last, d_last, sizeof(int32_t) * 3, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(last_len, d_last_len, sizeof(double) * 3, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    e->bj.ms = 0.0;
    timer.read(&e->bj.ms);
    e->bj.launches = launches;
    return IQHIP_OK;
}

extern "C" int iqhip_debug_bionj_timing(iqhip_engine *e, double *ms, int64_t *launches) {
    if (!e || e->planner || !e->shards.empty()) return fail(IQHIP_ERR_INVALID, "iqhip_debug_bionj_timing: needs a single-device engine");
    if (ms) *ms = e->bj.ms;
    if (launches) *launches = e->bj.launches;
    return IQHIP_OK;
}
