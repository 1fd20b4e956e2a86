// kernels_em.hip -- the device half of the EM estimation of +R free-rate models (RateFree::optimizeWithEM,
// model/ratefree.cpp:450-579) and of the empirical-Bayes site rates (RateGamma::computePatternRates,
// model/rategamma.cpp:235-258).  Both kernels are one streaming pass over the theta buffer of the current branch in either
// vector layout (64-pattern tiles: 4 states; 16-pattern tiles: 20 / 64 states and wide DNA), one thread per pattern, with
// the per-category table exp(eval_i r_c len) prop_c in LDS as k_pattern_lh_cat (kernels_rell.hip) keeps it:
//   k_em_posteriors : L_pc = sum_i table[c][i] theta[p][c][i] (the quantity iqhip_pattern_lh_cat returns, same arithmetic),
//                     W[c][p] = ptn_freq[p] L_pc / sum_c L_pc (category-major, padding patterns 0), the posterior mean
//                     rate and the first best category of the pattern, and the column sums S_c = sum_p W[c][p]
//   k_em_objective  : F_c = sum_p W[c][p] (log(L_pc / prop_c) + (max(sc_a, 0) + max(sc_b, 0)) LOG_SCALING_THRESHOLD) with the
//                     rates, weights and theta the engine holds now, and per category the number of floored terms
// Sums: every workgroup reduces its 256 patterns in a fixed order (wave shuffles, then the four waves in order) into its own
// row of a partial matrix; k_em_fold adds the rows in a fixed order.  No atomics: the same bits on every run.
#include <float.h>
#include <hip/hip_runtime.h>

#include "iqhip_internal.h"

namespace iqhip {

// theta[ptn][e], as theta_at of kernels_rell.hip
__device__ __forceinline__ double em_theta_at(const double *base, int tile, int pl, int e) {
    return tile == 64 ? base[(size_t)(e >> 1) * 128 + pl * 2 + (e & 1)] : base[(size_t)e * 16 + pl];
}

// sum over the workgroup's 256 threads of v, for value slot k of the workgroup's row: lanes by shuffles, then wave 0 .. 3
__device__ __forceinline__ double em_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

__global__ __launch_bounds__(256) void k_em_posteriors(const double *__restrict__ theta, const double *__restrict__ evalc,
                                                       const double *__restrict__ rates, const double *__restrict__ props,
                                                       const double *__restrict__ freq, double len, int n, int ncat, int tile,
                                                       int64_t nptn, int64_t nptn_pad, double *__restrict__ W,
                                                       double *__restrict__ ptn_rate, int32_t *__restrict__ ptn_cat,
                                                       double *__restrict__ part) {
    extern __shared__ double s_val[];  // [ncat][n] ++ wave sums [4][ncat]
    const int B = n * ncat;
    double *s_wave = s_val + B;
    for (int t = threadIdx.x; t < B; t += 256) {
        const int c = t / n;
        s_val[t] = exp(evalc[t] * rates[c] * len) * props[c];
    }
    __syncthreads();
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool live = p < nptn, inside = p < nptn_pad;   // (the last workgroup may hang over the padded pattern count)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double scale = 0.0;
    if (live) {
        const int64_t tl = p / tile;
        const int pl = (int)(p - tl * tile);
        const double *base = theta + (size_t)tl * tile * B;
        double sum = 0.0, sum_rate = 0.0, best_lh = 0.0;
        int best = 0;
        for (int c = 0; c < ncat; c++) {
            double acc = 0.0;
            for (int i = 0; i < n; i++) {
                const int e = c * n + i;
                acc += s_val[e] * em_theta_at(base, tile, pl, e);
            }
            W[(size_t)c * nptn_pad + p] = acc;
            sum += acc;
            sum_rate += rates[c] * acc;
            if (c == 0 || acc > best_lh) {   // the first maximum (the reference draws among equal ones)
                best_lh = acc;
                best = c;
            }
        }
        scale = freq[p] / sum;
        ptn_rate[p] = sum_rate / sum;
        ptn_cat[p] = best;
    } else if (inside) {
        ptn_rate[p] = 0.0;
        ptn_cat[p] = 0;
    }
    for (int c = 0; c < ncat; c++) {
        double w = 0.0;
        if (live) w = W[(size_t)c * nptn_pad + p] * scale;   // (this thread's own store above)
        if (inside) W[(size_t)c * nptn_pad + p] = w;
        const double s = em_wave_sum(w);
        if (lane == 0) s_wave[wave * ncat + c] = s;
    }
    __syncthreads();
    for (int c = threadIdx.x; c < ncat; c += 256)
        part[(size_t)blockIdx.x * ncat + c] = ((s_wave[c] + s_wave[ncat + c]) + s_wave[2 * ncat + c]) + s_wave[3 * ncat + c];
}

__global__ __launch_bounds__(256) void k_em_objective(const double *__restrict__ theta, const double *__restrict__ evalc,
                                                      const double *__restrict__ rates, const double *__restrict__ props,
                                                      const double *__restrict__ W, const int16_t *__restrict__ sc_a,
                                                      const int16_t *__restrict__ sc_b, double len, int n, int ncat, int tile,
                                                      int64_t nptn, int64_t nptn_pad, double *__restrict__ part) {
    extern __shared__ double s_val[];  // [ncat][n] ++ wave sums [4][2 ncat]
    const int B = n * ncat;
    double *s_wave = s_val + B;
    for (int t = threadIdx.x; t < B; t += 256) {
        const int c = t / n;
        s_val[t] = exp(evalc[t] * rates[c] * len) * props[c];
    }
    __syncthreads();
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool live = p < nptn;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double shift = 0.0;
    const double *base = theta;
    int pl = 0;
    if (live) {
        int s = 0;
        if (sc_a) s += max((int)sc_a[p], 0);
        if (sc_b) s += max((int)sc_b[p], 0);
        shift = (double)s * kLogScalingThreshold;
        const int64_t tl = p / tile;
        pl = (int)(p - tl * tile);
        base = theta + (size_t)tl * tile * B;
    }
    const double log_floor = log(DBL_MIN);
    for (int c = 0; c < ncat; c++) {
        double term = 0.0, floored = 0.0;
        if (live) {
            const double w = W[(size_t)c * nptn_pad + p];
            if (w > 0.0) {
                double acc = 0.0;
                for (int i = 0; i < n; i++) {
                    const int e = c * n + i;
                    acc += s_val[e] * em_theta_at(base, tile, pl, e);
                }
                double l;
                if (acc >= DBL_MIN && acc <= DBL_MAX)   // a positive normal number (false for NaN)
                    l = log(acc / props[c]);
                else {
                    l = log_floor;
                    floored = 1.0;
                }
                term = w * (l + shift);
            }
        }
        const double s = em_wave_sum(term), k = em_wave_sum(floored);
        if (lane == 0) {
            s_wave[wave * 2 * ncat + c] = s;
            s_wave[wave * 2 * ncat + ncat + c] = k;
        }
    }
    __syncthreads();
    const int V = 2 * ncat;
    for (int v = threadIdx.x; v < V; v += 256)
        part[(size_t)blockIdx.x * V + v] = ((s_wave[v] + s_wave[V + v]) + s_wave[2 * V + v]) + s_wave[3 * V + v];
}

// out[v] = sum over the rows of part [nrows][nvals] in a fixed order: workgroup v, thread t takes rows t, t + 256, ...
__global__ __launch_bounds__(256) void k_em_fold(const double *__restrict__ part, int64_t nrows, int nvals,
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

// part: [nptn_pad / 256 rounded up][ncat]; out: [ncat]
hipError_t launch_em_posteriors(iqhip_engine *e, double len, double *W, double *ptn_rate, int32_t *ptn_cat, double *part,
                                double *out) {
    const int64_t P = e->nptn_pad;   // a multiple of the tile size; the last workgroup may hang over it
    const unsigned nblocks = (unsigned)((P + 255) / 256);
    const size_t lds = sizeof(double) * ((size_t)e->block + 4 * (size_t)e->ncat);
    hipLaunchKernelGGL(k_em_posteriors, dim3(nblocks), dim3(256), lds, e->stream, e->d_theta.p, e->d_evalc, e->d_rates, e->d_props,
                       e->d_freq.p, len, e->n, e->ncat, e->tile, e->nptn, P, W, ptn_rate, ptn_cat, part);
    hipLaunchKernelGGL(k_em_fold, dim3((unsigned)e->ncat), dim3(256), 0, e->stream, part, (int64_t)nblocks, e->ncat, out);
    return hipGetLastError();
}

// part: [workgroups][2 ncat]; out: F [ncat] ++ floored counts [ncat] (as doubles: exact below 2^53)
hipError_t launch_em_objective(iqhip_engine *e, const int16_t *sc_a, const int16_t *sc_b, double len, const double *W,
                               double *part, double *out) {
    const int64_t P = e->nptn_pad;
    const unsigned nblocks = (unsigned)((P + 255) / 256);
    const size_t lds = sizeof(double) * ((size_t)e->block + 8 * (size_t)e->ncat);
    hipLaunchKernelGGL(k_em_objective, dim3(nblocks), dim3(256), lds, e->stream, e->d_theta.p, e->d_evalc, e->d_rates, e->d_props,
                       W, sc_a, sc_b, len, e->n, e->ncat, e->tile, e->nptn, P, part);
    hipLaunchKernelGGL(k_em_fold, dim3((unsigned)(2 * e->ncat)), dim3(256), 0, e->stream, part, (int64_t)nblocks, 2 * e->ncat, out);
    return hipGetLastError();
}

}  // namespace iqhip
