// kernels_classlnl.hip -- per-class log-likelihoods of a mixture engine (iqhip_class_lnl): K candidate models ride as the K
// classes of one mixture engine, one traversal builds theta for all of them, and this file turns theta into K numbers.
//   k_class_lnl  : grid (pattern blocks of 256, classes).  Lc[p][m] as k_mix_class_lh (kernels_mixem.hip) forms it -- the
//                  components of class m in ascending q, the same LDS table exp(eval_i r_q len) prop_q, the same arithmetic
//                  per component, either theta layout -- and then, for the patterns with ptn_freq > 0,
//                    term = ptn_freq[p] (log(Lc / class_weight[m] + inv_m[p]) + (max(sc_a, 0) + max(sc_b, 0)) LOG_SCALING_THRESHOLD)
//                  the expression the branch lnL kernels form for a plain model (phylokernel.h:1000-1016) with the scale
//                  counters put back as k_em_objective (kernels_em.hip) does.  A term whose argument is not a positive
//                  normal number takes log(DBL_MIN) and is counted.  The nptn x nclass matrix is never written: a workgroup
//                  reduces its 256 patterns (lanes by shuffles, then wave 0 .. 3) into row blockIdx.x of part
//                  [rows][2 nclass] = {sum, floored count} per class.
//   k_class_fold : out[v] = the rows of column v added in a fixed order (thread t rows t, t + 256, ...; then a tree).
// No atomics; the decomposition follows from nptn_pad and nclass alone: the same bits on every run and every CU count.
#include <float.h>
#include <hip/hip_runtime.h>

#include "iqhip_internal.h"

namespace iqhip {

// theta[ptn][e], as mix_theta_at of kernels_mixem.hip
__device__ __forceinline__ double cl_theta_at(const double *base, int tile, int pl, int e) {
    return tile == 64 ? base[(size_t)(e >> 1) * 128 + pl * 2 + (e & 1)] : base[(size_t)e * 16 + pl];
}

__device__ __forceinline__ double cl_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

// cls_list: first[nclass + 1] ++ the components of class 0, of class 1, ... (each ascending), as k_mix_class_lh reads it.
// class_invar: nullptr (every class takes invar, the engine's resident ptn_invar) or [nclass][nptn_pad]
__global__ __launch_bounds__(256) void k_class_lnl(const double *__restrict__ theta, const double *__restrict__ evalc,
                                                   const double *__restrict__ rates, const double *__restrict__ props,
                                                   const int32_t *__restrict__ cls_list, const double *__restrict__ class_weight,
                                                   const double *__restrict__ freq, const double *__restrict__ invar,
                                                   const double *__restrict__ class_invar, const int16_t *__restrict__ sc_a,
                                                   const int16_t *__restrict__ sc_b, double len, int n, int ncat, int nclass,
                                                   int tile, int64_t nptn, int64_t nptn_pad, double *__restrict__ part) {
    extern __shared__ double s_val[];  // [components of the class][n] ++ wave sums [4][2]
    const int m = blockIdx.y;
    const int q0 = cls_list[m], q1 = cls_list[m + 1];
    const int32_t *comp = cls_list + nclass + 1;
    double *s_wave = s_val + (size_t)(q1 - q0) * n;
    for (int t = threadIdx.x; t < (q1 - q0) * n; t += 256) {
        const int k = t / n, c = comp[q0 + k];
        s_val[t] = exp(evalc[c * n + (t - k * n)] * rates[c] * len) * props[c];
    }
    __syncthreads();
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;   // (the last workgroup may hang over the padded pattern count)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double term = 0.0, floored = 0.0;
    const double f = p < nptn ? freq[p] : 0.0;
    if (f > 0.0) {
        const int64_t tl = p / tile;
        const int pl = (int)(p - tl * tile);
        const double *base = theta + (size_t)tl * tile * n * ncat;
        double lh = 0.0;
        for (int k = q0; k < q1; k++) {
            const int c = comp[k];
            double acc = 0.0;
            for (int i = 0; i < n; i++) acc += s_val[(k - q0) * n + i] * cl_theta_at(base, tile, pl, c * n + i);
            lh = k == q0 ? acc : lh + acc;
        }
        int s = 0;
        if (sc_a) s += max((int)sc_a[p], 0);
        if (sc_b) s += max((int)sc_b[p], 0);
        const double inv = class_invar ? class_invar[(size_t)m * nptn_pad + p] : invar[p];
        const double arg = lh / class_weight[m] + inv;
        double l;
        if (arg >= DBL_MIN && arg <= DBL_MAX)   // a positive normal number (false for NaN)
            l = log(arg);
        else {
            l = log(DBL_MIN);
            floored = 1.0;
        }
        term = f * (l + (double)s * kLogScalingThreshold);
    }
    const double ws = cl_wave_sum(term), wk = cl_wave_sum(floored);
    if (lane == 0) {
        s_wave[wave * 2] = ws;
        s_wave[wave * 2 + 1] = wk;
    }
    __syncthreads();
    if (threadIdx.x < 2)
        part[(size_t)blockIdx.x * 2 * nclass + threadIdx.x * nclass + m] =
            ((s_wave[threadIdx.x] + s_wave[2 + threadIdx.x]) + s_wave[4 + threadIdx.x]) + s_wave[6 + threadIdx.x];
}

__global__ __launch_bounds__(256) void k_class_fold(const double *__restrict__ part, int64_t nrows, int nvals,
                                                    double *__restrict__ out) {
    __shared__ double red[256];
    const int v = blockIdx.x;
    double acc = 0.0;
    for (int64_t r = threadIdx.x; r < nrows; r += 256) acc += part[(size_t)r * nvals + v];
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[v] = red[0];
}

int64_t class_lnl_part_rows(const iqhip_engine *e) { return (e->nptn_pad + 255) / 256; }

// d_cw: class weights [nclass]; d_class_invar: nullptr or [nclass][nptn_pad]; part: [class_lnl_part_rows][2 nclass];
// out: lnl [nclass] ++ floored counts [nclass] (as doubles: exact below 2^53).  max_comp: the largest class's component count
hipError_t launch_class_lnl(iqhip_engine *e, const int16_t *sc_a, const int16_t *sc_b, double len, const int32_t *d_cls_list,
                            int max_comp, const double *d_cw, const double *d_class_invar, double *part, double *out) {
    const int M = e->nclass;
    const int64_t rows = class_lnl_part_rows(e);
    const size_t lds = sizeof(double) * ((size_t)max_comp * e->n + 8);
    hipLaunchKernelGGL(k_class_lnl, dim3((unsigned)rows, (unsigned)M), dim3(256), lds, e->stream, e->d_theta.p, e->d_evalc,
                       e->d_rates, e->d_props, d_cls_list, d_cw, e->d_freq.p, e->d_invar.p, d_class_invar, sc_a, sc_b, len, e->n,
                       e->ncat, M, e->tile, e->nptn, e->nptn_pad, part);
    hipLaunchKernelGGL(k_class_fold, dim3((unsigned)(2 * M)), dim3(256), 0, e->stream, part, rows, 2 * M, out);
    return hipGetLastError();
}

}  // namespace iqhip
