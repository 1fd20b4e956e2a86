// kernels_alrt.hip -- SH-aLRT and local-bootstrap branch supports (PhyloTree::testOneBranch, phylotree.cpp:3984-4056)
// from the engine's store of per-pattern log-likelihood rows.
//
// Pass 1, the product.  The reference forms, per branch and replicate, the three weighted sums
// sum_p w[p] * pat_lh[k][p] (resampleLh, phylotree.cpp:3779-3809).  For all branches of a tree and all replicates that
// is ONE tall-skinny fp64 product  R[M x S] = L[M x P] * W^T[P x S]  (M = 1 + 2 (T - 3) distinct rows, P = nptn_pad,
// S replicates, W the float sample matrix of iqhip_set_boot_samples), here on v_mfma_f64_16x16x4_f64:
//   * A operand = L (lane l: row l & 15, k = l >> 4), B operand = W^T (lane l: k = l >> 4, sample l & 15), converted
//     float -> double on the way in; D register r of lane l = row (l >> 4) + 4 r, sample l & 15.
//   * a workgroup (4 waves) owns 64 samples x ALL rows of a row group (MT tiles of 16 rows, at most 13 = 208 rows, so
//     the 195 rows of a 100-taxon tree are one group and the sample matrix is read from HBM once) x one K-chunk; wave w
//     owns samples 16 w .. 16 w + 15 and keeps MT accumulators (4 MT doubles per lane).
//   * both operands are K-contiguous in memory, so K-steps of 32 patterns are staged through LDS with coalesced
//     16-byte loads (256 B per row of L, 128 B per row of W) and prefetched into registers one step ahead.  LDS rows are
//     padded (34 doubles / 36 floats) so that the operand reads of a k-step touch every bank once.
//   * the pattern axis is split over workgroups to fill the machine (alrt_ksplit); chunk ks of all sample blocks sits on
//     XCD ks % 8 (workgroups go round the XCDs), so a chunk of L is fetched into one L2 only.
//   * the partial tiles go to [ks][row][sample]; k_alrt_combine adds them in chunk order -- no floating-point atomics,
//     the same bits run to run.
// Pass 2, the statistics: one workgroup per branch applies phylotree.cpp:4018-4044 per replicate and counts.
#include <hip/hip_runtime.h>

#include "iqhip_internal.h"

namespace iqhip {

typedef double v4f64 __attribute__((ext_vector_type(4)));

constexpr int kAlrtKT = 32;        // patterns per staged K-step
constexpr int kAlrtNS = 64;        // samples per workgroup
constexpr int kAlrtLStride = 34;   // doubles per LDS row of L: bank = 4 row + 2 k, a 64-bit read per lane, no conflicts
constexpr int kAlrtWStride = 36;   // floats per LDS row of W: bank = 36 sample + k, all 64 lanes distinct
constexpr int kAlrtMaxMT = 13;

template <int MT>
__global__ __launch_bounds__(256) void k_alrt_product(const double *__restrict__ store, const int32_t *__restrict__ rows,
                                                      int M, const float *__restrict__ W, int S, int64_t nptn_pad,
                                                      int nsb, int ksplit, int steps_per_chunk,
                                                      double *__restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    double *sL = smem;                                                          // [MT * 16][kAlrtLStride]
    float *sW = reinterpret_cast<float *>(smem + MT * 16 * kAlrtLStride);       // [kAlrtNS][kAlrtWStride]
    // block -> (chunk, sample block): chunk % 8 is the XCD the block lands on
    const int bid = (int)blockIdx.x;
    const int ks = (bid / (8 * nsb)) * 8 + (bid & 7);
    const int sb = (bid >> 3) % nsb;
    if (ks >= ksplit) return;   // (uniform over the workgroup)
    const int total_steps = (int)(nptn_pad / kAlrtKT);
    const int step0 = ks * steps_per_chunk;
    const int step1 = min(step0 + steps_per_chunk, total_steps);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // staging roles: L -- 16 threads per row (a double2 each), 16 rows per pass; W -- 8 threads per sample (a float4 each)
    const int l_row = threadIdx.x >> 4, l_k = 2 * (threadIdx.x & 15);
    const int w_smp = threadIdx.x >> 3, w_k = 4 * (threadIdx.x & 7);
    const int ngroups = (M + MT * 16 - 1) / (MT * 16);
    for (int grp = 0; grp < ngroups; grp++) {
        const int row0 = grp * MT * 16;
        const double *lp[MT];
#pragma unroll
        for (int m = 0; m < MT; m++) {
            const int r = row0 + m * 16 + l_row;
            lp[m] = r < M ? store + (size_t)rows[r] * nptn_pad + l_k : nullptr;
        }
        const float *wp[2];
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const int s = sb * kAlrtNS + h * 32 + w_smp;
            wp[h] = s < S ? W + (size_t)s * nptn_pad + w_k : nullptr;
        }
        v4f64 acc[MT];
#pragma unroll
        for (int m = 0; m < MT; m++) acc[m] = (v4f64){0.0, 0.0, 0.0, 0.0};
        double2 lreg[MT];
        float4 wreg[2];
        auto fetch = [&](int step) {
            const size_t off = (size_t)step * kAlrtKT;
#pragma unroll
            for (int m = 0; m < MT; m++)
                lreg[m] = lp[m] ? *reinterpret_cast<const double2 *>(lp[m] + off) : make_double2(0.0, 0.0);
#pragma unroll
            for (int h = 0; h < 2; h++)
                wreg[h] = wp[h] ? *reinterpret_cast<const float4 *>(wp[h] + off) : make_float4(0.f, 0.f, 0.f, 0.f);
        };
        if (step0 < step1) fetch(step0);
        for (int step = step0; step < step1; step++) {
            __syncthreads();   // the previous step's operand reads are done
#pragma unroll
            for (int m = 0; m < MT; m++)
                *reinterpret_cast<double2 *>(sL + (m * 16 + l_row) * kAlrtLStride + l_k) = lreg[m];
#pragma unroll
            for (int h = 0; h < 2; h++)
                *reinterpret_cast<float4 *>(sW + (h * 32 + w_smp) * kAlrtWStride + w_k) = wreg[h];
            __syncthreads();
            if (step + 1 < step1) fetch(step + 1);
            const double *la = sL + (lane & 15) * kAlrtLStride + (lane >> 4);
            const float *wb = sW + (wave * 16 + (lane & 15)) * kAlrtWStride + (lane >> 4);
#pragma unroll
            for (int s = 0; s < kAlrtKT / 4; s++) {
                const double b = (double)wb[4 * s];
#pragma unroll
                for (int m = 0; m < MT; m++)
                    acc[m] = __builtin_amdgcn_mfma_f64_16x16x4f64(la[m * 16 * kAlrtLStride + 4 * s], b, acc[m], 0, 0, 0);
            }
        }
        const int smp = sb * kAlrtNS + wave * 16 + (lane & 15);
        if (smp < S) {
            double *dst = part + (size_t)ks * M * S + smp;
#pragma unroll
            for (int m = 0; m < MT; m++)
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int row = row0 + m * 16 + (lane >> 4) + 4 * r;
                    if (row < M) dst[(size_t)row * S] = acc[m][r];
                }
        }
    }
}

// sums[i] = part[0][i] + part[1][i] + ... in chunk order
__global__ __launch_bounds__(256) void k_alrt_combine(const double *__restrict__ part, int ksplit, size_t count,
                                                      double *__restrict__ sums) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    double a = 0.0;
    for (int k = 0; k < ksplit; k++) a += part[(size_t)k * count + i];
    sums[i] = a;
}

// one workgroup per branch: testOneBranch's replicate loop (phylotree.cpp:4014-4045) on the three rows' sums, counted
// over the workgroup (integers: any order gives the same count; an LDS tree all the same)
__global__ __launch_bounds__(256) void k_alrt_stats(const int32_t *__restrict__ idx3, const double *__restrict__ lh3,
                                                    int S, const double *__restrict__ sums, double *__restrict__ out) {
    __shared__ int s_sh[256], s_lbp[256];
    const int b = blockIdx.x;
    const double lh[3] = {lh3[3 * b], lh3[3 * b + 1], lh3[3 * b + 2]};
    const double *r0 = sums + (size_t)idx3[3 * b] * S, *r1 = sums + (size_t)idx3[3 * b + 1] * S,
                 *r2 = sums + (size_t)idx3[3 * b + 2] * S;
    const double aLRT = lh[1] > lh[2] ? lh[0] - lh[1] : lh[0] - lh[2];
    int n_sh = 0, n_lbp = 0;
    for (int i = threadIdx.x; i < S; i += 256) {
        const double lh_new[3] = {r0[i], r1[i], r2[i]};
        if (lh_new[0] > lh_new[1] && lh_new[0] > lh_new[2]) n_lbp++;
        double cs[3], cs_best, cs_2nd_best;
        cs[0] = lh_new[0] - lh[0];
        cs[1] = lh_new[1] - lh[1];
        cs[2] = lh_new[2] - lh[2];
        if (cs[0] >= cs[1] && cs[0] >= cs[2]) {
            cs_best = cs[0];
            cs_2nd_best = cs[1] > cs[2] ? cs[1] : cs[2];
        } else if (cs[1] >= cs[2]) {
            cs_best = cs[1];
            cs_2nd_best = cs[0] > cs[2] ? cs[0] : cs[2];
        } else {
            cs_best = cs[2];
            cs_2nd_best = cs[0] > cs[1] ? cs[0] : cs[1];
        }
        if (aLRT > (cs_best - cs_2nd_best) + 0.05) n_sh++;
    }
    s_sh[threadIdx.x] = n_sh;
    s_lbp[threadIdx.x] = n_lbp;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            s_sh[threadIdx.x] += s_sh[threadIdx.x + o];
            s_lbp[threadIdx.x] += s_lbp[threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        double *o = out + 4 * (size_t)b;
        o[0] = S > 0 ? (double)s_sh[0] / S : 0.0;
        o[1] = S > 0 ? (double)s_lbp[0] / S : 0.0;
        o[2] = 1.0 / (1.0 + exp(lh[1] - lh[0]) + exp(lh[2] - lh[0]));
        o[3] = 2.0 * aLRT;
    }
}

// K-chunks: enough workgroups for two per CU, at least 8 K-steps each, a multiple of 8 when there is more than one
int alrt_ksplit(const iqhip_engine *e, int nrows, int nsamples) {
    (void)nrows;
    const int nsb = (nsamples + kAlrtNS - 1) / kAlrtNS;
    const int total_steps = (int)(e->nptn_pad / kAlrtKT);
    int want = std::max(1, (2 * e->num_cus + nsb - 1) / nsb);
    want = std::min(want, std::max(1, total_steps / 8));
    if (want > 1) want = (want + 7) / 8 * 8;
    want = std::min(want, total_steps);
    const int per = (total_steps + want - 1) / want;
    return (total_steps + per - 1) / per;   // (no empty chunk)
}

template <int MT>
static hipError_t launch_product_mt(iqhip_engine *e, const int32_t *d_rows, int M, int S, int ksplit, double *part) {
    const int nsb = (S + kAlrtNS - 1) / kAlrtNS;
    const int total_steps = (int)(e->nptn_pad / kAlrtKT);
    const int per = (total_steps + ksplit - 1) / ksplit;
    const int grid = (ksplit + 7) / 8 * 8 * nsb;
    const size_t lds = sizeof(double) * MT * 16 * kAlrtLStride + sizeof(float) * kAlrtNS * kAlrtWStride;
    // more than 64 KB of dynamic LDS (13 row tiles: 64.25 KB) needs the opt-in on the device the launch goes to
    if (lds > 64 * 1024) {
        const hipError_t a = raise_lds_ceiling<&k_alrt_product<MT>>(e, (int)lds);
        if (a != hipSuccess) return a;
    }
    hipLaunchKernelGGL(k_alrt_product<MT>, dim3((unsigned)grid), dim3(256), lds, e->stream, e->d_ptnlh.p, d_rows, M, e->d_boot.p, S,
                       e->nptn_pad, nsb, ksplit, per, part);
    return hipGetLastError();
}

hipError_t launch_alrt_product(iqhip_engine *e, const int32_t *d_rows, int nrows, int nsamples, int ksplit, double *part,
                               double *sums) {
    const int tiles = (nrows + 15) / 16;
    hipError_t s;
    if (tiles <= 1) s = launch_product_mt<1>(e, d_rows, nrows, nsamples, ksplit, part);
    else if (tiles <= 2) s = launch_product_mt<2>(e, d_rows, nrows, nsamples, ksplit, part);
    else if (tiles <= 4) s = launch_product_mt<4>(e, d_rows, nrows, nsamples, ksplit, part);
    else if (tiles <= 8) s = launch_product_mt<8>(e, d_rows, nrows, nsamples, ksplit, part);
    else s = launch_product_mt<kAlrtMaxMT>(e, d_rows, nrows, nsamples, ksplit, part);
    if (s != hipSuccess) return s;
    const size_t count = (size_t)nrows * nsamples;
    hipLaunchKernelGGL(k_alrt_combine, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, e->stream, part, ksplit, count, sums);
    return hipGetLastError();
}

hipError_t launch_alrt_stats(iqhip_engine *e, const int32_t *d_idx3, const double *d_lh3, int nbranch, int nsamples,
                             const double *sums, double *out) {
    hipLaunchKernelGGL(k_alrt_stats, dim3((unsigned)nbranch), dim3(256), 0, e->stream, d_idx3, d_lh3, nsamples, sums, out);
    return hipGetLastError();
}

}  // namespace iqhip
