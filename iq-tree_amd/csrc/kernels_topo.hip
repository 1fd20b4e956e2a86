// kernels_topo.hip -- tree topology tests (evaluateTrees / performAUTest, phylotesting.cpp:1916-2050, 2053-2442) on the
// RELL sums R[tree][replicate] that kernels_alrt.hip forms from the engine's store of per-pattern log-likelihood rows.
//
//   k_topo_gen / k_topo_counts_to_float   bootstrap resamples drawn on the device: one thread per draw, a counter-based
//       generator (splitmix64 finaliser keyed by seed, stream, replicate and draw), site -> pattern by binary search in the
//       int64 prefix sums of ptn_freq, integer atomics on a uint32 view of the sample row, converted to float afterwards.
//       No floating-point atomic: the same key gives the same matrix on every run, whatever the launch shape.
//   k_topo_diff_variance   computeLogLDiffVariance (phylotree.cpp:1390-1416) for every pair of rows, the reference's two
//       passes (the Gram-matrix form G_ii + G_jj - 2 G_ij cancels ten digits on rows that differ in the third decimal).
//   k_topo_avg, k_topo_replicate, k_topo_tree   RELL-BP, KH, SH, weighted KH / SH and c-ELW (phylotesting.cpp:2218-2411):
//       avg_lh summed in replicate order by one lane per tree (bit-identical to the reference's loop), the per-replicate
//       maxima and the BP winner by one lane per replicate, the counts by one workgroup per tree.
//   k_topo_argmax   STEP 2 of performAUTest: per replicate the first tree with the strictly largest sum, counted.
// The file is built with -ffp-contract=off (Makefile): every comparison sees the bits a plain IEEE restatement of the
// reference's expressions sees.
#include <float.h>
#include <hip/hip_runtime.h>

#include "iqhip_internal.h"

#pragma clang fp contract(off)

namespace iqhip {

constexpr uint64_t kTopoGolden = 0x9E3779B97F4A7C15ull;

__host__ __device__ inline uint64_t topo_mix(uint64_t z) {
    z ^= z >> 30;
    z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27;
    z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}

// the generator's value for (key of seed and stream, replicate rho, draw j)
__device__ inline uint64_t topo_draw(uint64_t stream_key, int64_t rho, int64_t j) {
    const uint64_t h = topo_mix(stream_key + kTopoGolden * (uint64_t)(rho + 1));
    return topo_mix(h + kTopoGolden * (uint64_t)(j + 1));
}

uint64_t topo_stream_key(uint64_t seed, uint32_t stream) { return topo_mix(seed + kTopoGolden * ((uint64_t)stream + 1)); }

// blockIdx.y = row of the sample matrix (replicate first_replicate + row); the draws of a row go round its blocks
__global__ __launch_bounds__(256) void k_topo_gen(uint32_t *__restrict__ counts, int64_t nptn_pad, int64_t nptn,
                                                  const int64_t *__restrict__ prefix, uint64_t nsite, uint64_t stream_key,
                                                  int64_t first_replicate, int64_t ndraws) {
    const int64_t row = blockIdx.y;
    const uint64_t h = topo_mix(stream_key + kTopoGolden * (uint64_t)(first_replicate + row + 1));
    uint32_t *dst = counts + (size_t)row * nptn_pad;
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < ndraws; j += (int64_t)gridDim.x * 256) {
        const uint64_t z = topo_mix(h + kTopoGolden * (uint64_t)(j + 1));
        const int64_t site = (int64_t)__umul64hi(z, nsite);   // < nsite = prefix[nptn - 1]
        int64_t lo = 0, hi = nptn - 1;                        // the first pattern whose inclusive prefix sum exceeds site
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (prefix[mid] > site) hi = mid;
            else lo = mid + 1;
        }
        atomicAdd(dst + lo, 1u);
    }
}

__global__ __launch_bounds__(256) void k_topo_counts_to_float(float *__restrict__ w, size_t count) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    w[i] = (float)reinterpret_cast<const uint32_t *>(w)[i];
}

// a workgroup's sum of one double per thread, in a fixed order (LDS tree)
__device__ inline double topo_block_sum(double v, double *s) {
    s[threadIdx.x] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) s[threadIdx.x] += s[threadIdx.x + o];
        __syncthreads();
    }
    const double r = s[0];
    __syncthreads();
    return r;
}

// one workgroup per pair i < j of the row list (blockIdx.x = i, blockIdx.y = j); the diagonal is zeroed by the caller
__global__ __launch_bounds__(256) void k_topo_diff_variance(const double *__restrict__ store, const int32_t *__restrict__ rows,
                                                            int n, int64_t nptn_pad, int64_t nptn,
                                                            const double *__restrict__ freq, double nsite,
                                                            double *__restrict__ var) {
    __shared__ double s[256];
    const int i = blockIdx.x, j = blockIdx.y;
    if (i >= j) return;   // (uniform over the workgroup)
    const double *a = store + (size_t)rows[j] * nptn_pad, *b = store + (size_t)rows[i] * nptn_pad;
    double acc = 0.0;
    for (int64_t p = threadIdx.x; p < nptn; p += 256) acc += (a[p] - b[p]) * freq[p];
    const double mean = topo_block_sum(acc, s) / nsite;
    acc = 0.0;
    for (int64_t p = threadIdx.x; p < nptn; p += 256) {
        const double diff = a[p] - b[p] - mean;
        acc += diff * diff * freq[p];
    }
    const double variance = topo_block_sum(acc, s);
    if (threadIdx.x == 0) {
        const double v = nsite <= 1.0 ? 0.0 : variance * (nsite / (nsite - 1.0));
        var[(size_t)i * n + j] = v;
        var[(size_t)j * n + i] = v;
    }
}

// avg_lh[tid] (phylotesting.cpp:2273-2278): one lane per tree, the replicates in order
__global__ __launch_bounds__(64) void k_topo_avg(const double *__restrict__ sums, const int32_t *__restrict__ idx, int T, int S,
                                                 double *__restrict__ avg) {
    const int tid = blockIdx.x * 64 + threadIdx.x;
    if (tid >= T) return;
    const double *r = sums + (size_t)idx[tid] * S;
    double a = 0.0;
    for (int boot = 0; boot < S; boot++) a += r[boot];
    avg[tid] = a / S;
}

// std::max(a, b) of the reference: b when a < b, else a
__device__ inline double topo_max(double a, double b) { return a < b ? b : a; }

// one lane per replicate: the SH-centred maximum (:2279-2281), the ELW maximum and sumL (:2377-2392) and the RELL-BP
// winner with the tie rule of :2227-2240; random_double() is ((z >> 11) * 2^-53) of the draw (tie_key, boot, tid)
__global__ __launch_bounds__(256) void k_topo_replicate(const double *__restrict__ sums, const int32_t *__restrict__ idx, int T,
                                                        int S, const double *__restrict__ avg, double epsilon,
                                                        uint64_t tie_key, double *__restrict__ max_sh,
                                                        double *__restrict__ max_elw, double *__restrict__ sum_l,
                                                        int32_t *__restrict__ winner) {
    const int boot = blockIdx.x * 256 + threadIdx.x;
    if (boot >= S) return;
    double msh = -DBL_MAX, melw = -DBL_MAX;
    for (int tid = 0; tid < T; tid++) {
        const double r = sums[(size_t)idx[tid] * S + boot];
        msh = topo_max(msh, r - avg[tid]);
        melw = topo_max(melw, r);
    }
    double sl = 0.0;
    for (int tid = 0; tid < T; tid++) sl += exp(sums[(size_t)idx[tid] * S + boot] - melw);
    double maxL = sums[(size_t)idx[0] * S + boot];
    int maxtid = 0, maxcount = 1;
    for (int tid = 1; tid < T; tid++) {
        const double r = sums[(size_t)idx[tid] * S + boot];
        if (r > maxL + epsilon) {
            maxL = r;
            maxtid = tid;
            maxcount = 1;
        } else if (r > maxL - epsilon &&
                   (double)(topo_draw(tie_key, boot, tid) >> 11) * 0x1.0p-53 <= 1.0 / (maxcount + 1)) {
            maxL = topo_max(maxL, r);
            maxtid = tid;
            maxcount++;
        }
    }
    max_sh[boot] = msh;
    max_elw[boot] = melw;
    sum_l[boot] = sl;
    winner[boot] = maxtid;
}

// one workgroup per tree: the KH / SH counts (:2303-2321), the BP share (:2241-2247), the ELW mean (:2393-2401) and, with
// weights, the wKH / wSH counts (:2339-2369).  kh_id[tid]: orig_max_id, or orig_2ndmax_id for the best tree; w_id / w_orig:
// max_id / worig_diff of :2343-2352 (w_id < 0: no tree qualified).  out[tid] = bp, kh, sh, wkh, wsh, elw.
__global__ __launch_bounds__(256) void k_topo_tree(const double *__restrict__ sums, const int32_t *__restrict__ idx, int T, int S,
                                                   const double *__restrict__ lh, const double *__restrict__ avg,
                                                   const int32_t *__restrict__ kh_id, const double *__restrict__ max_sh,
                                                   const double *__restrict__ max_elw, const double *__restrict__ sum_l,
                                                   const int32_t *__restrict__ winner, const double *__restrict__ weights,
                                                   const int32_t *__restrict__ w_id, const double *__restrict__ w_orig,
                                                   double *__restrict__ out) {
    __shared__ int s_cnt[5][256];
    __shared__ double s_sum[256];
    const int tid = blockIdx.x;
    const double *mine = sums + (size_t)idx[tid] * S;
    const int max_id = kh_id[tid];
    const double *max_kh = sums + (size_t)idx[max_id] * S;
    const double orig_diff = lh[max_id] - lh[tid] - avg[tid];
    const double avg_max = avg[max_id], avg_tid = avg[tid];
    const int wmax_id = weights ? w_id[tid] : -1;
    const double worig_diff = weights ? w_orig[tid] : 0.0;
    const double wkh_diff = wmax_id >= 0 ? lh[wmax_id] - lh[tid] : 0.0;
    int n_bp = 0, n_kh = 0, n_sh = 0, n_wkh = 0, n_wsh = 0;
    double elw = 0.0;
    for (int boot = threadIdx.x; boot < S; boot += 256) {
        const double r = mine[boot];
        if (winner[boot] == tid) n_bp++;
        if (max_sh[boot] - r > orig_diff) n_sh++;
        const double max_kh_here = max_kh[boot] - avg_max;
        if (max_kh_here - r > orig_diff) n_kh++;
        elw += exp(r - max_elw[boot]) / sum_l[boot];
        if (weights) {
            double wmax_diff = -DBL_MAX;
            for (int tid2 = 0; tid2 < T; tid2++)
                if (tid2 != tid)
                    wmax_diff = topo_max(wmax_diff, (sums[(size_t)idx[tid2] * S + boot] - avg[tid2] - r + avg_tid) *
                                                        weights[(size_t)tid * T + tid2]);
            if (wmax_diff > worig_diff) n_wsh++;
            if (wmax_id >= 0) {
                wmax_diff = sums[(size_t)idx[wmax_id] * S + boot] - avg[wmax_id] - r + avg_tid;
                if (wmax_diff > wkh_diff) n_wkh++;
            }
        }
    }
    s_cnt[0][threadIdx.x] = n_bp;
    s_cnt[1][threadIdx.x] = n_kh;
    s_cnt[2][threadIdx.x] = n_sh;
    s_cnt[3][threadIdx.x] = n_wkh;
    s_cnt[4][threadIdx.x] = n_wsh;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o)
            for (int k = 0; k < 5; k++) s_cnt[k][threadIdx.x] += s_cnt[k][threadIdx.x + o];
        __syncthreads();
    }
    const double elw_sum = topo_block_sum(elw, s_sum);
    if (threadIdx.x == 0) {
        double *o = out + 6 * (size_t)tid;
        o[0] = (double)s_cnt[0][0] / S;
        o[1] = (double)s_cnt[1][0] / S;
        o[2] = (double)s_cnt[2][0] / S;
        o[3] = weights ? (double)s_cnt[3][0] / S : -1.0;
        o[4] = weights ? (double)s_cnt[4][0] / S : -1.0;
        o[5] = elw_sum / S;
    }
}

// one lane per replicate of a chunk: the first tree with the strictly largest sum (phylotesting.cpp:1961-1979)
__global__ __launch_bounds__(256) void k_topo_argmax(const double *__restrict__ sums, const int32_t *__restrict__ idx, int T,
                                                     int S, uint32_t *__restrict__ counts) {
    const int boot = blockIdx.x * 256 + threadIdx.x;
    if (boot >= S) return;
    double max_lh = -1e20;
    int max_tid = -1;
    for (int tid = 0; tid < T; tid++) {
        const double r = sums[(size_t)idx[tid] * S + boot];
        if (r > max_lh) {
            max_lh = r;
            max_tid = tid;
        }
    }
    if (max_tid >= 0) atomicAdd(counts + max_tid, 1u);
}

// ---- launches ---------------------------------------------------------------------------------------------------------
hipError_t launch_topo_gen(iqhip_engine *e, int nsamples, int64_t first_replicate, int64_t ndraws, uint64_t stream_key) {
    const size_t count = (size_t)nsamples * e->nptn_pad;
    hipError_t s = hipMemsetAsync(e->d_boot.p, 0, sizeof(float) * count, e->stream);
    if (s != hipSuccess) return s;
    const unsigned gx = (unsigned)std::max<int64_t>(1, std::min<int64_t>((ndraws + 255) / 256, 256));
    hipLaunchKernelGGL(k_topo_gen, dim3(gx, (unsigned)nsamples), dim3(256), 0, e->stream, reinterpret_cast<uint32_t *>(e->d_boot.p),
                       e->nptn_pad, e->nptn, e->d_freq_prefix.p, (uint64_t)e->freq_nsite, stream_key, first_replicate, ndraws);
    if ((s = hipGetLastError()) != hipSuccess) return s;
    hipLaunchKernelGGL(k_topo_counts_to_float, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, e->stream, e->d_boot.p, count);
    return hipGetLastError();
}

hipError_t launch_topo_diff_variance(iqhip_engine *e, const int32_t *d_rows, int n, double *d_var) {
    hipError_t s = hipMemsetAsync(d_var, 0, sizeof(double) * (size_t)n * n, e->stream);
    if (s != hipSuccess) return s;
    hipLaunchKernelGGL(k_topo_diff_variance, dim3((unsigned)n, (unsigned)n), dim3(256), 0, e->stream, e->d_ptnlh.p, d_rows, n,
                       e->nptn_pad, e->nptn, e->d_freq.p, (double)e->freq_nsite, d_var);
    return hipGetLastError();
}

hipError_t launch_topo_tests(iqhip_engine *e, const TopoTestArgs &a) {
    hipLaunchKernelGGL(k_topo_avg, dim3((unsigned)((a.T + 63) / 64)), dim3(64), 0, e->stream, a.sums, a.idx, a.T, a.S, a.avg);
    hipError_t s = hipGetLastError();
    if (s != hipSuccess) return s;
    hipLaunchKernelGGL(k_topo_replicate, dim3((unsigned)((a.S + 255) / 256)), dim3(256), 0, e->stream, a.sums, a.idx, a.T, a.S,
                       a.avg, a.epsilon, a.tie_key, a.max_sh, a.max_elw, a.sum_l, a.winner);
    return hipGetLastError();
}

hipError_t launch_topo_tree(iqhip_engine *e, const TopoTestArgs &a) {
    hipLaunchKernelGGL(k_topo_tree, dim3((unsigned)a.T), dim3(256), 0, e->stream, a.sums, a.idx, a.T, a.S, a.lh, a.avg, a.kh_id,
                       a.max_sh, a.max_elw, a.sum_l, a.winner, a.weights, a.w_id, a.w_orig, a.out);
    return hipGetLastError();
}

hipError_t launch_topo_argmax(iqhip_engine *e, const double *sums, const int32_t *d_idx, int T, int S, uint32_t *counts) {
    hipLaunchKernelGGL(k_topo_argmax, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, e->stream, sums, d_idx, T, S, counts);
    return hipGetLastError();
}

}  // namespace iqhip
