// kernels_spr.hip -- the parsimony SPR scan (include/iqhip.h "Parsimony SPR scan"; the scan of pll/fastDNAparsimony.c:1169-1427
// rearrangeParsimony / addTraverseParsimony / testInsertParsimony for every prune point of a tree at once).
//
// A word column of any Fitch vector depends on the same column of its inputs only (kernels_pars.hip), so a lane that owns a
// column can walk the whole regraft neighbourhood of a prune point on its own: the vectors U of the path from the prune
// point to the branch under test (the pruned tree's directed vectors, which exist nowhere in memory) live in a stack indexed
// by depth, the stored vectors V(side) / V(target) of the unpruned tree are read once per step, and only scores leave.
//
//   k_pars_spr      grid (column chunks, jobs), one wave per workgroup, no barrier of any kind.  Q lanes share a column,
//                   each holding N / Q planes (the planes of a Fitch step meet in one OR: log2 Q xor-shuffles), so a wave
//                   owns 64 / Q columns.  Where the stack lives and what it costs (512 registers per lane and SIMD, 160 KiB
//                   of LDS per CU: MI355X_MICROARCH.md "Register files"):
//        4 states   Q = 1, 64 columns a wave; the stack is 10 levels x (4 planes + score) = 50 registers, selected by the
//                   wave-uniform depth through unrolled compares (constant indices only: 81 VGPRs, no scratch, 5 waves a
//                   SIMD)
//       20 states   Q = 2, 32 columns a wave (128-byte runs of a plane); the stack is in LDS, [level][plane or score][lane]:
//                   a lane touches its own words only (no barrier) and the 64 lanes of an access hit 64 consecutive words
//                   (no bank conflict).  levels x 11 x 256 bytes: 16.5 KiB at radius 6 (9 waves a CU), 27.5 KiB at radius
//                   10.  Measured: Q = 1 (31.5 KiB, 126 VGPRs) took 1.7 times as long, Q = 4 the same
//       64 states   Q = 4, 16 columns a wave = the 64-byte runs of k_pars_update; LDS levels x 17 x 256 bytes: 25.5 KiB at
//                   radius 6 (6 waves a CU), 42.5 KiB at radius 10.  With Q = 1 the stack of one wave would be 97.5 KiB at
//                   radius 6; Q = 2 (208 VGPRs) measured 1.2 times slower, Q = 8 the same within the spread
//                   The LDS size follows the deepest step of the LAUNCH (host-validated), not the job count.
//        A step at the deepest level is nobody's parent and is not stored.  The step list is never written on the device
//        and its index is wave-uniform; the vectors are read with per-lane vector loads.
//        Scores: integer shuffle reduction over the wave, then one integer atomicAdd per (step, column chunk) -- exact and
//        the same on every run.  The score array starts at -1 everywhere (what NO_SCORE steps keep) and chunk 0 adds the 1.
//   k_pars_spr_min  per job the first minimum over its scored steps (one wave per job)
//   k_pars_spr_best the first job that holds the global minimum (one workgroup)
#include <hip/hip_runtime.h>

#include "iqhip_internal.h"

namespace iqhip {

constexpr int kSprLevels = IQHIP_PARS_SPR_MAX_RADIUS;   // stack levels 0 .. 9

// planes q * P .. q * P + P - 1 and the score of column w of a slot
template <int N, int Q>
__device__ __forceinline__ void spr_load(const uint32_t *__restrict__ vec, const uint32_t *__restrict__ score, int slot,
                                         int64_t nwords, int64_t w, int q, uint32_t (&x)[N / Q], uint32_t &sc) {
    constexpr int P = N / Q;
    const uint32_t *v = vec + (size_t)slot * (size_t)nwords * N;
    if constexpr (N == 4) {
        const uint4 r = *reinterpret_cast<const uint4 *>(v + 4 * w);
        x[0] = r.x;
        x[1] = r.y;
        x[2] = r.z;
        x[3] = r.w;
    } else {
#pragma unroll
        for (int i = 0; i < P; i++) x[i] = v[(size_t)(q * P + i) * nwords + w];
    }
    sc = score[(size_t)slot * nwords + w];
}

// OR over the Q lanes that share a column
template <int Q>
__device__ __forceinline__ uint32_t spr_or(uint32_t v) {
#pragma unroll
    for (int m = 32; m >= 64 / Q && Q > 1; m >>= 1) v |= (uint32_t)__shfl_xor((int)v, m);
    return v;
}

// x = fitch(x, y) over this lane's planes; returns the sites of the column that cost a substitution
template <int P, int Q>
__device__ __forceinline__ uint32_t spr_fitch(uint32_t (&x)[P], const uint32_t (&y)[P]) {
    uint32_t any = 0;
#pragma unroll
    for (int i = 0; i < P; i++) any |= x[i] & y[i];
    const uint32_t w = ~spr_or<Q>(any);
#pragma unroll
    for (int i = 0; i < P; i++) x[i] = (x[i] & y[i]) | (w & (x[i] | y[i]));
    return w;
}

template <int N, int Q>
__global__ __launch_bounds__(64) void k_pars_spr(const uint32_t *__restrict__ vec, const uint32_t *__restrict__ score,
                                                 const iqhip_pars_spr_job *__restrict__ jobs, int njobs,
                                                 const iqhip_pars_spr_step *__restrict__ steps /* parent = the depth */,
                                                 int64_t nwords, int levels, int32_t *__restrict__ out) {
    constexpr int P = N / Q, C = 64 / Q;
    extern __shared__ uint32_t s_stk[];   // N > 4: [levels][P + 1][64]
    const int lane = threadIdx.x, q = lane / C;
    const int64_t w0 = (int64_t)blockIdx.x * C + lane % C;
    const bool counts = w0 < nwords && q == 0;             // one lane per real column adds to the sums
    const int64_t w = w0 < nwords ? w0 : nwords - 1;       // (the other lanes recompute the last column and drop it)
    uint32_t reg[N == 4 ? kSprLevels : 1][P + 1];          // 4 states: the stack
    for (int j = blockIdx.y; j < njobs; j += gridDim.y) {
        const iqhip_pars_spr_job job = jobs[j];
        uint32_t S[P], ssc;
        spr_load<N, Q>(vec, score, job.subtree, nwords, w, q, S, ssc);
        for (int k = 0; k < job.nsteps; k++) {
            const iqhip_pars_spr_step st = steps[job.first_step + k];
            const int d = st.parent;
            uint32_t u[P], usc;
            spr_load<N, Q>(vec, score, st.side, nwords, w, q, u, usc);
            if (d > 0) {   // (uniform)
                uint32_t par[P], psc = 0;
                if constexpr (N == 4) {
#pragma unroll
                    for (int l = 0; l < kSprLevels; l++)
                        if (l == d - 1) {
#pragma unroll
                            for (int i = 0; i < P; i++) par[i] = reg[l][i];
                            psc = reg[l][P];
                        }
                } else {
                    const uint32_t *s = s_stk + (size_t)(d - 1) * (P + 1) * 64 + lane;
#pragma unroll
                    for (int i = 0; i < P; i++) par[i] = s[i * 64];
                    psc = s[P * 64];
                }
                usc += psc + (uint32_t)__popc(spr_fitch<P, Q>(u, par));
            }
            if constexpr (N == 4) {
#pragma unroll
                for (int l = 0; l < kSprLevels; l++)
                    if (l == d) {
#pragma unroll
                        for (int i = 0; i < P; i++) reg[l][i] = u[i];
                        reg[l][P] = usc;
                    }
            } else if (d < levels) {
                uint32_t *s = s_stk + (size_t)d * (P + 1) * 64 + lane;
#pragma unroll
                for (int i = 0; i < P; i++) s[i * 64] = u[i];
                s[P * 64] = usc;
            }
            if (st.flags & IQHIP_PARS_SPR_NO_SCORE) continue;
            uint32_t t[P], tsc;
            spr_load<N, Q>(vec, score, st.target, nwords, w, q, t, tsc);
            const uint32_t cost = spr_fitch<P, Q>(u, t);
            uint32_t any = 0;
#pragma unroll
            for (int i = 0; i < P; i++) any |= u[i] & S[i];
            any = spr_or<Q>(any);
            uint32_t s = usc + tsc + ssc + (uint32_t)__popc(cost) + (uint32_t)__popc(~any);
            if (!counts) s = 0;
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) s += (uint32_t)__shfl_down((int)s, off);
            if (lane == 0) atomicAdd(out + job.first_step + k, (int32_t)s + (blockIdx.x == 0 ? 1 : 0));
        }
    }
}

// best_step[j] / best_score[j]: the first minimum over job j's scored steps (score >= 0), -1 / INT32_MAX without one
__global__ __launch_bounds__(64) void k_pars_spr_min(const int32_t *__restrict__ score, const iqhip_pars_spr_job *__restrict__ jobs,
                                                     int32_t *__restrict__ best_step, int32_t *__restrict__ best_score) {
    const iqhip_pars_spr_job job = jobs[blockIdx.x];
    int32_t best = 0x7fffffff, at = 0x7fffffff;
    for (int k = threadIdx.x; k < job.nsteps; k += 64) {   // (ascending k: a strict < keeps the first)
        const int32_t s = score[job.first_step + k];
        if (s >= 0 && s < best) {
            best = s;
            at = k;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const int32_t s2 = __shfl_down(best, off), i2 = __shfl_down(at, off);
        if (s2 < best || (s2 == best && i2 < at)) {
            best = s2;
            at = i2;
        }
    }
    if (threadIdx.x == 0) {
        best_step[blockIdx.x] = at == 0x7fffffff ? -1 : at;
        best_score[blockIdx.x] = best;
    }
}

__global__ __launch_bounds__(256) void k_pars_spr_best(const int32_t *__restrict__ best_score, int njobs, int32_t *__restrict__ best_job) {
    __shared__ int32_t s_score[256], s_idx[256];
    int32_t best = 0x7fffffff, at = 0x7fffffff;
    for (int j = threadIdx.x; j < njobs; j += 256) {
        const int32_t s = best_score[j];
        if (s < best) {
            best = s;
            at = j;
        }
    }
    s_score[threadIdx.x] = best;
    s_idx[threadIdx.x] = at;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            const int32_t s2 = s_score[threadIdx.x + o], i2 = s_idx[threadIdx.x + o];
            if (s2 < s_score[threadIdx.x] || (s2 == s_score[threadIdx.x] && i2 < s_idx[threadIdx.x])) {
                s_score[threadIdx.x] = s2;
                s_idx[threadIdx.x] = i2;
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) *best_job = s_idx[0] == 0x7fffffff ? -1 : s_idx[0];
}

// d_out: score [nsteps] ++ best_step [njobs] ++ best_score [njobs] ++ best_job
hipError_t launch_pars_spr(iqhip_engine *e, const iqhip_pars_spr_job *d_jobs, int njobs, const iqhip_pars_spr_step *d_steps,
                           int nsteps, int max_depth, int32_t *d_out, int *nlaunches) {
    *nlaunches = 0;
    if (njobs < 1 || nsteps < 1) return hipErrorInvalidValue;
    if (max_depth < 0 || max_depth > IQHIP_PARS_SPR_MAX_RADIUS) return hipErrorInvalidValue;
    hipError_t s = hipMemsetAsync(d_out, 0xff, sizeof(int32_t) * (size_t)nsteps, e->stream);
    if (s != hipSuccess) return s;
    const int levels = max_depth < 1 ? 1 : max_depth;
    const unsigned gy = (unsigned)(njobs < 65535 ? njobs : 65535);
#define IQHIP_PARS_SPR(N, Q)                                                                                              \
    hipLaunchKernelGGL((k_pars_spr<N, Q>), dim3((unsigned)((e->pars_nwords + 64 / Q - 1) / (64 / Q)), gy), dim3(64),      \
                       (N == 4 ? 0 : sizeof(uint32_t) * (size_t)levels * (N / Q + 1) * 64), e->stream, e->pars.vec.p,      \
                       e->pars.score.p, d_jobs, njobs, d_steps, e->pars_nwords, levels, d_out)
    if (e->n == 4) IQHIP_PARS_SPR(4, 1);
    else if (e->n == 20) IQHIP_PARS_SPR(20, 2);
    else if (e->n == 64) IQHIP_PARS_SPR(64, 4);
    else return hipErrorInvalidValue;
#undef IQHIP_PARS_SPR
    if ((s = hipGetLastError()) != hipSuccess) return s;
    hipLaunchKernelGGL(k_pars_spr_min, dim3((unsigned)njobs), dim3(64), 0, e->stream, d_out, d_jobs, d_out + nsteps,
                       d_out + nsteps + njobs);
    if ((s = hipGetLastError()) != hipSuccess) return s;
    hipLaunchKernelGGL(k_pars_spr_best, dim3(1), dim3(256), 0, e->stream, d_out + nsteps + njobs, njobs,
                       d_out + nsteps + 2 * (size_t)njobs);
    *nlaunches = 3;
    return hipGetLastError();
}

}  // namespace iqhip
