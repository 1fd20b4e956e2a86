// kernels_rell.hip -- consumers of the device-resident per-pattern log-likelihoods:
//   k_pattern_lh_scaled : PhyloTree::computePatternLikelihood (phylotree.cpp:1200-1230) -- the scaling
//                         events of both ends of the evaluated branch put back into _pattern_lh
//   k_rell              : UFBoot's RELL scores (IQTree::saveCurrentTree, iqtree.cpp:2726-2736):
//                         one dot product <pattern_lh, boot_sample[s]> per bootstrap sample
//   k_ptnlh_rows        : the per-pattern log-likelihoods of the tasks of one k_newton_batch launch, each at its
//                         accepted length, into rows of the engine's store (the reference's nniMoves[cnt].ptnlh,
//                         phylotree.cpp:3019-3020) -- what k_pattern_lh_scaled gives for one branch, for a whole chunk
// The first two are one pass over HBM-resident data (the sample matrix is the only traffic that matters:
// nsamples * nptn * 4 bytes); nothing but the nsamples scores leaves the device.
// The reference accumulates in float over eight AVX lanes (dotProductSIMD<float,Vec8f,8>); here
// the products are formed from the double pattern lnL and the float weight and accumulated in
// double in a fixed order (deterministic, more accurate; tests bound the difference).
#include <hip/hip_runtime.h>

#include "iqhip_internal.h"

namespace iqhip {

__global__ __launch_bounds__(256) void k_pattern_lh_scaled(const double *__restrict__ pattern_lh,
                                                           const int16_t *__restrict__ sc_a,
                                                           const int16_t *__restrict__ sc_b, int64_t nobs,
                                                           int64_t nptn_pad, double shift,
                                                           double *__restrict__ out) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= nptn_pad) return;
    double v = 0.0;  // unobserved (+ASC) and padding patterns carry no site
    if (p < nobs) {
        int s = 0;
        if (sc_a) s += max((int)sc_a[p], 0);
        if (sc_b) s += max((int)sc_b[p], 0);
        v = (pattern_lh[p] - shift) + (double)s * kLogScalingThreshold;
    }
    out[p] = v;
}

// one workgroup per bootstrap sample; thread t owns patterns 4*(t + 256*j) .. +3
__global__ __launch_bounds__(256) void k_rell(const double *__restrict__ ptn_lh, const float *__restrict__ samples,
                                              int64_t nptn_pad, double *__restrict__ out) {
    __shared__ double red[256];
    const float *w = samples + (size_t)blockIdx.x * nptn_pad;
    double acc = 0.0;
    for (int64_t p = (int64_t)threadIdx.x * 4; p < nptn_pad; p += 1024) {  // nptn_pad is a multiple of 64
        const float4 wv = *reinterpret_cast<const float4 *>(w + p);
        const double2 l0 = *reinterpret_cast<const double2 *>(ptn_lh + p);
        const double2 l1 = *reinterpret_cast<const double2 *>(ptn_lh + p + 2);
        acc += l0.x * (double)wv.x;
        acc += l0.y * (double)wv.y;
        acc += l1.x * (double)wv.z;
        acc += l1.y * (double)wv.w;
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[blockIdx.x] = red[0];
}

// _pattern_lh_cat of the scalar kernels (phylotreesse.cpp:1190-1237): per pattern and category
// sum_i exp(eval_i r_c t) prop_c theta[ptn][c][i], from the theta buffer of the current branch, unscaled.
// Generic in the vector layout: 64-pattern tiles (4 states) or 16-pattern tiles (20 / 64 states).
__global__ __launch_bounds__(256) void k_pattern_lh_cat(const double *__restrict__ theta, const double *__restrict__ evalc,
                                                        const double *__restrict__ rates, const double *__restrict__ props,
                                                        double len, int n, int ncat, int tile, int64_t nptn,
                                                        double *__restrict__ out) {
    extern __shared__ double s_val[];  // [ncat][n]
    const int B = n * ncat;
    for (int t = threadIdx.x; t < B; t += 256) {
        const int c = t / n;
        s_val[t] = exp(evalc[t] * rates[c] * len) * props[c];
    }
    __syncthreads();
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= nptn * ncat) return;
    const int64_t p = idx / ncat;
    const int c = (int)(idx - p * ncat);
    const int64_t tl = p / tile;
    const int pl = (int)(p - tl * tile);
    const double *base = theta + (size_t)tl * tile * B;
    double acc = 0.0;
    for (int i = 0; i < n; i++) {
        const int e = c * n + i;
        const double th = (tile == 64) ? base[(size_t)(e >> 1) * 128 + pl * 2 + (e & 1)] : base[(size_t)e * 16 + pl];
        acc += s_val[e] * th;
    }
    out[idx] = acc;
}

// theta[ptn][e] of one pattern in either vector layout (see k_pattern_lh_cat): 64-pattern tiles hold double2 pairs of
// block entries per pattern, 16-pattern tiles one row of 16 patterns per block entry
__device__ __forceinline__ double theta_at(const double *base, int tile, int pl, int e) {
    return tile == 64 ? base[(size_t)(e >> 1) * 128 + pl * 2 + (e & 1)] : base[(size_t)e * 16 + pl];
}
// sum_e val[e] * theta[ptn][e] in the order of k_newton_batch's lnL pass (wg_partial): one chain of fused multiply-adds
// over the block (64-pattern tiles), or four interleaved chains combined as (c0 + c1) + (c2 + c3) (16-pattern tiles)
__device__ __forceinline__ double theta_dot(const double *theta, const double *s_val, int B, int tile, int64_t p) {
    const int64_t tl = p / tile;
    const int pl = (int)(p - tl * tile);
    const double *base = theta + (size_t)tl * tile * B;
    if (tile == 64) {
        double lh = 0.0;
        for (int e = 0; e < B; e++) lh = fma(s_val[e], theta_at(base, 64, pl, e), lh);
        return lh;
    }
    double c[4] = {0.0, 0.0, 0.0, 0.0};
    for (int e0 = 0; e0 < B; e0 += 4)
#pragma unroll
        for (int g = 0; g < 4; g++)
            if (e0 + g < B) c[g] = fma(s_val[e0 + g], theta_at(base, 16, pl, e0 + g), c[g]);
    return (c[0] + c[1]) + (c[2] + c[3]);
}

// grid (pattern blocks, tasks of the chunk); task t reads its descriptor (the two branch ends' scale counters), its
// accepted length out6[6t] and its theta buffer, which k_newton_batch left complete in memory.  +ASC: every workgroup
// sums prob_const of its task over the unobserved patterns itself (phylokernel.h:1138-1163, fixed order), so that the
// row carries log|lh| - log(1 - prob_const) as iqhip_fetch_pattern_lh_scaled gives it.
__global__ __launch_bounds__(256) void k_ptnlh_rows(const char *__restrict__ tasks, size_t task_stride, size_t br_off,
                                                    const double *__restrict__ out6, const double *__restrict__ theta_base,
                                                    size_t theta_stride, const double *__restrict__ evalc,
                                                    const double *__restrict__ rates, const double *__restrict__ props,
                                                    const double *__restrict__ invar, int n, int ncat, int tile, int64_t nobs,
                                                    int64_t nptn, int64_t nptn_pad, const int32_t *__restrict__ rows,
                                                    double *__restrict__ store) {
    extern __shared__ double s_val[];  // [ncat][n]
    __shared__ double s_red[256];
    const int t = blockIdx.y;
    const int32_t row = rows[t];
    if (row < 0) return;   // (uniform over the workgroup)
    const DevBranch *br = reinterpret_cast<const DevBranch *>(tasks + (size_t)t * task_stride + br_off);
    const int16_t *a_sc = br->a_sc, *b_sc = br->b_sc;
    const double len = out6[(size_t)t * 6];
    const double *theta = theta_base + (size_t)t * theta_stride;
    const int B = n * ncat;
    for (int k = threadIdx.x; k < B; k += 256) {
        const int c = k / n;
        s_val[k] = exp(evalc[k] * rates[c] * len) * props[c];
    }
    __syncthreads();
    double shift = 0.0;
    if (nobs < nptn) {
        double pc = 0.0;
        for (int64_t p = nobs + threadIdx.x; p < nptn; p += 256) {
            const double lh = theta_dot(theta, s_val, B, tile, p);
            int ssc = 0;
            if (a_sc) ssc += a_sc[p];
            if (b_sc) ssc += b_sc[p];
            pc += (ssc >= 1 ? lh * kScalingThreshold : lh) + invar[p];
        }
        s_red[threadIdx.x] = pc;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if ((int)threadIdx.x < o) s_red[threadIdx.x] += s_red[threadIdx.x + o];
            __syncthreads();
        }
        shift = log(1.0 - s_red[0]);
    }
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= nptn_pad) return;
    double v = 0.0;  // unobserved (+ASC) and padding patterns carry no site
    if (p < nobs) {
        const double lh = theta_dot(theta, s_val, B, tile, p) + invar[p];
        double l = log(fabs(lh));
        if (isnan(l) || isinf(l)) l = kLogScalingThreshold * 4;  // the reference's repair, phylokernel.h:1100-1122
        int s = 0;
        if (a_sc) s += max((int)a_sc[p], 0);
        if (b_sc) s += max((int)b_sc[p], 0);
        v = (l - shift) + (double)s * kLogScalingThreshold;
    }
    store[(size_t)row * nptn_pad + p] = v;
}

hipError_t launch_ptnlh_rows(iqhip_engine *e, const void *d_tasks, int m, const double *theta_base, size_t theta_stride,
                             const double *batch_out, const int32_t *d_rows) {
    const int64_t P = e->nptn_pad;
    hipLaunchKernelGGL(k_ptnlh_rows, dim3((unsigned)((P + 255) / 256), (unsigned)m), dim3(256), sizeof(double) * e->block,
                       e->stream, static_cast<const char *>(d_tasks), newton_task_bytes(), newton_task_branch_offset(),
                       batch_out, theta_base, theta_stride, e->d_evalc, e->d_rates, e->d_props, e->d_invar.p, e->n, e->ncat,
                       e->tile, e->nptn - e->n_unobs, e->nptn, P, d_rows, e->d_ptnlh.p);
    return hipGetLastError();
}

hipError_t launch_pattern_lh_cat(iqhip_engine *e, double len, double *out) {
    const int64_t total = e->nptn * e->ncat;
    hipLaunchKernelGGL(k_pattern_lh_cat, dim3((unsigned)((total + 255) / 256)), dim3(256), sizeof(double) * e->block, e->stream,
                       e->d_theta.p, e->d_evalc, e->d_rates, e->d_props, len, e->n, e->ncat, e->tile, e->nptn, out);
    return hipGetLastError();
}

hipError_t launch_pattern_lh_scaled(iqhip_engine *e, const int16_t *sc_a, const int16_t *sc_b, double *out) {
    const int64_t P = e->nptn_pad;
    hipLaunchKernelGGL(k_pattern_lh_scaled, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, e->stream, e->d_pattern_lh.p,
                       sc_a, sc_b, e->nptn - e->n_unobs, P, e->asc_active ? e->pattern_lh_shift : 0.0, out);
    return hipGetLastError();
}

hipError_t launch_rell(iqhip_engine *e, double *out) {
    hipLaunchKernelGGL(k_rell, dim3((unsigned)e->nboot), dim3(256), 0, e->stream, e->d_ptn_scaled.p, e->d_boot.p,
                       e->nptn_pad, out);
    return hipGetLastError();
}

}  // namespace iqhip
