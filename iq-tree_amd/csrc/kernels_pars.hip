// kernels_pars.hip -- bit-parallel Fitch parsimony (phylotreepars.cpp:18-282; SIMD twins phylokernel.h:1280-1560).
//
// A vector holds, per word column w (32 sites), one word per state ("bit-plane": bit b of plane i = site 32 w + b allows
// state i) and one score word: the substitutions of the subtree inside that column.  Device layout:
//    4 states        word-major, vec[w * 4 + i] -- the reference's layout; a lane's column is one 16-byte load
//   20 / 64 states   plane-major, vec[i * nwords + w] -- threads on consecutive columns read consecutive words of a plane
//                    (64-byte runs per op in k_pars_update, whole 256-byte requests in k_pars_branch); word-major would
//                    stride them 80 / 256 bytes apart
//   scores           score[slot * nwords + w]
// Per-column scores mean that an update needs no reduction and no atomics; only the kernels that return a score reduce.
//
//   k_pars_tips     the tip vectors (:39-146): one thread per (taxon, column, plane) looks up its 32 sites' state codes
//   k_pars_update   the node update (:169-211) for a whole op list in ONE launch at any tree depth.  An op on column w reads
//       only column w of its children, so a workgroup that owns kParsWordsPerWg columns never needs another workgroup: it
//       walks the host-assigned levels, its threads share out the ops of a level (kParsThreads / kParsWordsPerWg ops side
//       by side: short alignments have few columns, so the parallelism comes from the ops of a level), and
//       __syncthreads() separates the levels.  What this relies on: a vector store of one wave is visible to a vector load of another wave
//       of the SAME workgroup behind __syncthreads() -- the workgroup's waves share their CU's L1, and __syncthreads() is a
//       workgroup-scope release/acquire that drains the storing waves' stores (vmcnt(0)) before the barrier
//       (MI355X_MICROARCH.md "visibility", fence table: workgroup scope is exactly what cannot be relied on ACROSS CUs and
//       what holds within one; cdna_hip_programming.md Guideline 16 lists the cross-workgroup case this design avoids).
//       The vectors are not __restrict__ and are read with per-lane vector loads only, never through the scalar path.
//       No cooperative launch, no grid barrier, no spinning: nothing here waits on another workgroup.
//   k_pars_branch   computeParsimonyBranchFast (:218-282) / the insertion scan of addTaxonMPFast (:428-465): one workgroup
//       per branch, columns strided over its threads, shuffle reduction per wave and a cross-wave sum in LDS
//   k_pars_argmin   the first minimum of the scan's scores in list order (one workgroup)
//   k_pars_insert_wave / k_pars_insert_wg / k_pars_argmin_seg   the insertion scan of MANY trees in one launch: segments of
//       branches with a taxon each (one stepwise-addition step of a whole forest), a wave or a workgroup per branch, and a
//       workgroup per segment for its first minimum
#include <hip/hip_runtime.h>

#include "iqhip_internal.h"

namespace iqhip {

template <int N>
__device__ __forceinline__ void pars_load(const uint32_t *v, int64_t nwords, int64_t w, uint32_t (&x)[N]) {
    if constexpr (N == 4) {
        const uint4 q = *reinterpret_cast<const uint4 *>(v + 4 * w);
        x[0] = q.x;
        x[1] = q.y;
        x[2] = q.z;
        x[3] = q.w;
    } else {
#pragma unroll
        for (int i = 0; i < N; i++) x[i] = v[(size_t)i * nwords + w];
    }
}

template <int N>
__device__ __forceinline__ void pars_store(uint32_t *v, int64_t nwords, int64_t w, const uint32_t (&x)[N]) {
    if constexpr (N == 4) {
        *reinterpret_cast<uint4 *>(v + 4 * w) = make_uint4(x[0], x[1], x[2], x[3]);
    } else {
#pragma unroll
        for (int i = 0; i < N; i++) v[(size_t)i * nwords + w] = x[i];
    }
}

// z = fitch(x, y) in place of x; returns w = the sites that cost a substitution
template <int N>
__device__ __forceinline__ uint32_t pars_fitch(uint32_t (&x)[N], const uint32_t (&y)[N]) {
    uint32_t any = 0;
#pragma unroll
    for (int i = 0; i < N; i++) any |= x[i] & y[i];
    const uint32_t w = ~any;
#pragma unroll
    for (int i = 0; i < N; i++) x[i] = (x[i] & y[i]) | (w & (x[i] | y[i]));
    return w;
}

// ---- tips ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_pars_tips(const uint8_t *__restrict__ states, int64_t nptn_pad,
                                                   const int32_t *__restrict__ site_ptn, int64_t nsites, int64_t nwords,
                                                   const uint64_t *__restrict__ masks, int n, int ntaxa,
                                                   uint32_t *__restrict__ vec, uint32_t *__restrict__ score) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)ntaxa * nwords * n) return;
    const int i = (int)(idx % n);
    const int64_t w = idx / n % nwords;
    const int t = (int)(idx / n / nwords);
    const uint8_t *row = states + (size_t)t * nptn_pad;
    uint32_t bits = 0;
    for (int b = 0; b < 32; b++) {
        const int64_t site = w * 32 + b;
        // (the padding bits of the last word: plane 0 at every tip, phylotreepars.cpp:74-75)
        const uint32_t bit = site < nsites ? (uint32_t)((masks[row[site_ptn[site]]] >> i) & 1u) : (i == 0 ? 1u : 0u);
        bits |= bit << b;
    }
    const size_t at = n == 4 ? (size_t)w * 4 + i : (size_t)i * nwords + w;
    vec[(size_t)t * nwords * n + at] = bits;
    if (i == 0) score[(size_t)t * nwords + w] = 0;
}

// ---- node updates -------------------------------------------------------------------------------------------------------
// thread = (column, op slot): kParsWordsPerWg columns x (kParsThreads / kParsWordsPerWg) ops of a level side by side
template <int N>
__global__ __launch_bounds__(kParsThreads) void k_pars_update(uint32_t *vec, uint32_t *score, const iqhip_pars_op *__restrict__ ops,
                                                              const int32_t *__restrict__ lev_start, int nlev, int64_t nwords) {
    constexpr int kSlots = kParsThreads / kParsWordsPerWg;
    const int col = threadIdx.x % kParsWordsPerWg, slot = threadIdx.x / kParsWordsPerWg;
    const int64_t w = (int64_t)blockIdx.x * kParsWordsPerWg + col;
    const size_t vstride = (size_t)nwords * N;
    for (int lev = 0; lev < nlev; lev++) {
        const int o1 = lev_start[lev + 1];
        if (w < nwords)
            for (int o = lev_start[lev] + slot; o < o1; o += kSlots) {
                const iqhip_pars_op op = ops[o];
                const uint32_t *vx = vec + (size_t)op.left * vstride, *vy = vec + (size_t)op.right * vstride;
                uint32_t *vz = vec + (size_t)op.dst * vstride;
                const uint32_t sx = score[(size_t)op.left * nwords + w], sy = score[(size_t)op.right * nwords + w];
                uint32_t cost;
                if constexpr (N <= 20) {   // both columns in registers: all 2 N loads in flight together
                    uint32_t x[N], y[N];
                    pars_load<N>(vx, nwords, w, x);
                    pars_load<N>(vy, nwords, w, y);
                    cost = pars_fitch<N>(x, y);
                    pars_store<N>(vz, nwords, w, x);
                } else {
                    // 64 states: two passes over the planes (the second one hits the L1) instead of 128 registers of
                    // columns, so that the 16 waves of a workgroup fit a CU
                    uint32_t any = 0;
#pragma unroll 8
                    for (int i = 0; i < N; i++) any |= vx[(size_t)i * nwords + w] & vy[(size_t)i * nwords + w];
                    cost = ~any;
#pragma unroll 8
                    for (int i = 0; i < N; i++) {
                        const uint32_t xi = vx[(size_t)i * nwords + w], yi = vy[(size_t)i * nwords + w];
                        vz[(size_t)i * nwords + w] = (xi & yi) | (cost & (xi | yi));
                    }
                }
                score[(size_t)op.dst * nwords + w] = sx + sy + (uint32_t)__popc(cost);
            }
        if (lev + 1 < nlev) __syncthreads();   // (uniform: every thread of the workgroup walks all levels)
    }
}

// ---- branch scores and the insertion scan --------------------------------------------------------------------------------
// the sum of v over the workgroup's 256 threads, valid in thread 0
__device__ __forceinline__ uint32_t pars_block_sum(uint32_t v, uint32_t *s_red) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    __syncthreads();   // (s_red may still be read from the previous sum)
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
    __syncthreads();
    return s_red[0] + s_red[1] + s_red[2] + s_red[3];
}

template <int N, bool INSERT>
__global__ __launch_bounds__(256) void k_pars_branch(const uint32_t *__restrict__ vec, const uint32_t *__restrict__ score,
                                                     const int32_t *__restrict__ ends, int nbranch, int64_t nwords, int taxon,
                                                     int32_t *__restrict__ out) {
    __shared__ uint32_t s_red[4];
    const int b = blockIdx.x;
    const int a = ends[2 * b], c = ends[2 * b + 1];
    const size_t vstride = (size_t)nwords * N;
    const uint32_t *va = vec + (size_t)a * vstride, *vc = vec + (size_t)c * vstride;
    uint32_t total = 0, subst = 0;
    const uint32_t *vt = vec + (size_t)(INSERT ? taxon : 0) * vstride;
    for (int64_t w = threadIdx.x; w < nwords; w += 256) {
        uint32_t s = score[(size_t)a * nwords + w] + score[(size_t)c * nwords + w];
        // the sites where the two ends share no state; with N > 4 the planes are streamed, not held (two passes for the scan)
        uint32_t any = 0, anyt = 0;
        if constexpr (N == 4) {
            uint32_t x[N], y[N];
            pars_load<N>(va, nwords, w, x);
            pars_load<N>(vc, nwords, w, y);
            if constexpr (INSERT) {
                uint32_t t[N];
                pars_load<N>(vt, nwords, w, t);
                any = ~pars_fitch<N>(x, y);
#pragma unroll
                for (int i = 0; i < N; i++) anyt |= x[i] & t[i];
            } else {
#pragma unroll
                for (int i = 0; i < N; i++) any |= x[i] & y[i];
            }
        } else {
#pragma unroll 4
            for (int i = 0; i < N; i++) any |= va[(size_t)i * nwords + w] & vc[(size_t)i * nwords + w];
            if constexpr (INSERT) {
#pragma unroll 4
                for (int i = 0; i < N; i++) {
                    const uint32_t xi = va[(size_t)i * nwords + w], yi = vc[(size_t)i * nwords + w];
                    anyt |= ((xi & yi) | (~any & (xi | yi))) & vt[(size_t)i * nwords + w];
                }
            }
        }
        const uint32_t k = (uint32_t)__popc(~any);
        s += k;
        if constexpr (INSERT) s += (uint32_t)__popc(~anyt);
        else subst += k;
        total += s;
    }
    total = pars_block_sum(total, s_red);
    if constexpr (!INSERT) subst = pars_block_sum(subst, s_red);
    if (threadIdx.x == 0) {
        out[b] = (int32_t)total;
        out[nbranch + b] = (int32_t)subst;
    }
}

// the first minimum of score[lo .. hi) by a workgroup of 256 threads: afterwards s_idx[0] = its index, s_score[0] = it
__device__ __forceinline__ void pars_block_argmin(const int32_t *score, int lo, int hi, int32_t *s_score, int32_t *s_idx) {
    int32_t best = 0x7fffffff, at = 0x7fffffff;
    for (int b = lo + (int)threadIdx.x; b < hi; b += 256) {   // (ascending b: a strict < keeps the first)
        const int32_t s = score[b];
        if (s < best) {
            best = s;
            at = b;
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
}

// out[2 nbranch] = the first index of the smallest score, out[2 nbranch + 1] = that score
__global__ __launch_bounds__(256) void k_pars_argmin(int32_t *out, int nbranch) {
    __shared__ int32_t s_score[256], s_idx[256];
    pars_block_argmin(out, 0, nbranch, s_score, s_idx);
    if (threadIdx.x == 0) {
        out[2 * nbranch] = s_idx[0];
        out[2 * nbranch + 1] = s_score[0];
    }
}

// ---- the segmented insertion scan (iqhip_pars_insert_scores_batch) ------------------------------------------------------
// Branch b of segment g against the tip taxon[b] (the host expands the segment's taxon to its branches): one scoring
// function, two ways to share the columns out.  The vectors were written by an earlier launch on the same stream and are
// only read here.  Nothing is accumulated across workgroups and there are no atomics: a branch's sum is one wave's (or one
// workgroup's) fixed reduction tree, so every run gives the same bits.
//
// the insertion score of word column w -- k_pars_branch<N, true>'s term: m = fitch(a, c) in registers, then
// a_score + c_score + popc(w_ac) + popc(~OR_i(m_i & t_i))
template <int N>
__device__ __forceinline__ uint32_t pars_insert_word(const uint32_t *__restrict__ va, const uint32_t *__restrict__ vc,
                                                     const uint32_t *__restrict__ vt, const uint32_t *__restrict__ sa,
                                                     const uint32_t *__restrict__ sc, int64_t nwords, int64_t w) {
    uint32_t cost, anyt = 0;
    if constexpr (N <= 20) {
        uint32_t x[N], y[N], t[N];
        pars_load<N>(va, nwords, w, x);
        pars_load<N>(vc, nwords, w, y);
        pars_load<N>(vt, nwords, w, t);
        cost = pars_fitch<N>(x, y);
#pragma unroll
        for (int i = 0; i < N; i++) anyt |= x[i] & t[i];
    } else {   // 64 states: the planes are streamed in two passes, as in k_pars_update, instead of 192 registers of columns
        uint32_t any = 0;
#pragma unroll 4
        for (int i = 0; i < N; i++) any |= va[(size_t)i * nwords + w] & vc[(size_t)i * nwords + w];
        cost = ~any;
#pragma unroll 4
        for (int i = 0; i < N; i++) {
            const uint32_t xi = va[(size_t)i * nwords + w], yi = vc[(size_t)i * nwords + w];
            anyt |= ((xi & yi) | (cost & (xi | yi))) & vt[(size_t)i * nwords + w];
        }
    }
    return sa[w] + sc[w] + (uint32_t)__popc(cost) + (uint32_t)__popc(~anyt);
}

// the partial sum of a branch over the columns first, first + stride, ...
template <int N>
__device__ __forceinline__ uint32_t pars_insert_partial(const uint32_t *__restrict__ vec, const uint32_t *__restrict__ score,
                                                        const int32_t *__restrict__ ends, const int32_t *__restrict__ taxon, int b,
                                                        int64_t nwords, int first, int stride) {
    const int a = ends[2 * b], c = ends[2 * b + 1], t = taxon[b];
    const size_t vstride = (size_t)nwords * N;
    const uint32_t *va = vec + (size_t)a * vstride, *vc = vec + (size_t)c * vstride, *vt = vec + (size_t)t * vstride;
    const uint32_t *sa = score + (size_t)a * nwords, *sc = score + (size_t)c * nwords;
    uint32_t total = 0;
    for (int64_t w = first; w < nwords; w += stride) total += pars_insert_word<N>(va, vc, vt, sa, sc, nwords, w);
    return total;
}

// wave per branch: four branches per workgroup, columns strided over the 64 lanes, shuffle reduction, no LDS and no
// __syncthreads() -- so a wave whose branch lies past the list simply returns
template <int N>
__global__ __launch_bounds__(256) void k_pars_insert_wave(const uint32_t *__restrict__ vec, const uint32_t *__restrict__ score,
                                                          const int32_t *__restrict__ ends, const int32_t *__restrict__ taxon,
                                                          int nbranch, int64_t nwords, int32_t *__restrict__ out) {
    const int b = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    if (b >= nbranch) return;   // (wave-uniform)
    uint32_t total = pars_insert_partial<N>(vec, score, ends, taxon, b, nwords, (int)(threadIdx.x & 63), 64);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) total += __shfl_down(total, off);
    if ((threadIdx.x & 63) == 0) out[b] = (int32_t)total;
}

// workgroup per branch: the shape of k_pars_branch
template <int N>
__global__ __launch_bounds__(256) void k_pars_insert_wg(const uint32_t *__restrict__ vec, const uint32_t *__restrict__ score,
                                                        const int32_t *__restrict__ ends, const int32_t *__restrict__ taxon,
                                                        int nbranch, int64_t nwords, int32_t *__restrict__ out) {
    __shared__ uint32_t s_red[4];
    const int b = blockIdx.x;   // (the grid is nbranch workgroups)
    uint32_t total = pars_insert_partial<N>(vec, score, ends, taxon, b, nwords, (int)threadIdx.x, 256);
    total = pars_block_sum(total, s_red);
    if (threadIdx.x == 0) out[b] = (int32_t)total;
}

// one workgroup per segment: out[nbranch + g] = the first minimum of the segment's scores as an index within the segment,
// out[nbranch + nseg + g] = that score (k_pars_argmin's tie rule: the same reduction)
__global__ __launch_bounds__(256) void k_pars_argmin_seg(int32_t *out, const int32_t *__restrict__ seg_start, int nbranch, int nseg) {
    __shared__ int32_t s_score[256], s_idx[256];
    const int g = blockIdx.x;
    const int lo = seg_start[g];
    pars_block_argmin(out, lo, seg_start[g + 1], s_score, s_idx);
    if (threadIdx.x == 0) {
        out[nbranch + g] = s_idx[0] - lo;
        out[nbranch + nseg + g] = s_score[0];
    }
}

// ---- launches -----------------------------------------------------------------------------------------------------------
hipError_t launch_pars_tips(iqhip_engine *e, const int32_t *d_site_ptn) {
    const int64_t total = (int64_t)e->ntaxa * e->pars_nwords * e->n;
    hipLaunchKernelGGL(k_pars_tips, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, e->stream, e->d_states.p, e->nptn_pad,
                       d_site_ptn, e->pars_nsites, e->pars_nwords, e->pars.masks.p, e->n, e->ntaxa, e->pars.vec.p,
                       e->pars.score.p);
    return hipGetLastError();
}

hipError_t launch_pars_update(iqhip_engine *e, const iqhip_pars_op *d_ops, const int32_t *d_lev_start, int nlev) {
    if (nlev < 1) return hipSuccess;
    const dim3 grid((unsigned)((e->pars_nwords + kParsWordsPerWg - 1) / kParsWordsPerWg));
#define IQHIP_PARS_UPDATE(N)                                                                                       \
    hipLaunchKernelGGL(k_pars_update<N>, grid, dim3(kParsThreads), 0, e->stream, e->pars.vec.p, e->pars.score.p, d_ops, d_lev_start, \
                       nlev, e->pars_nwords)
    if (e->n == 4) IQHIP_PARS_UPDATE(4);
    else if (e->n == 20) IQHIP_PARS_UPDATE(20);
    else if (e->n == 64) IQHIP_PARS_UPDATE(64);
    else return hipErrorInvalidValue;
#undef IQHIP_PARS_UPDATE
    return hipGetLastError();
}

hipError_t launch_pars_branch(iqhip_engine *e, const int32_t *d_ends, int nbranch, int taxon, int32_t *d_out, int *nlaunches) {
    *nlaunches = 0;
    if (nbranch < 1) return hipSuccess;
#define IQHIP_PARS_BRANCH(N, INS)                                                                                     \
    hipLaunchKernelGGL((k_pars_branch<N, INS>), dim3((unsigned)nbranch), dim3(256), 0, e->stream, e->pars.vec.p,      \
                       e->pars.score.p, d_ends, nbranch, e->pars_nwords, taxon, d_out)
    const bool ins = taxon >= 0;
    if (e->n == 4) { if (ins) IQHIP_PARS_BRANCH(4, true); else IQHIP_PARS_BRANCH(4, false); }
    else if (e->n == 20) { if (ins) IQHIP_PARS_BRANCH(20, true); else IQHIP_PARS_BRANCH(20, false); }
    else if (e->n == 64) { if (ins) IQHIP_PARS_BRANCH(64, true); else IQHIP_PARS_BRANCH(64, false); }
    else return hipErrorInvalidValue;
#undef IQHIP_PARS_BRANCH
    hipError_t s = hipGetLastError();
    if (s != hipSuccess) return s;
    *nlaunches = 1;
    if (ins) {
        hipLaunchKernelGGL(k_pars_argmin, dim3(1), dim3(256), 0, e->stream, d_out, nbranch);
        s = hipGetLastError();
        *nlaunches = 2;
    }
    return s;
}

hipError_t launch_pars_insert_batch(iqhip_engine *e, const int32_t *d_ends, const int32_t *d_taxon, int nbranch,
                                    const int32_t *d_seg_start, int nseg, ParsBatchRoute route, int32_t *d_out, int *nlaunches) {
    *nlaunches = 0;
    if (nbranch < 1 || nseg < 1) return hipSuccess;
    const bool wave = route == PARS_BATCH_WAVE || (route == PARS_BATCH_AUTO && e->pars_nwords <= kParsBatchWaveWords);
#define IQHIP_PARS_INSERT(N)                                                                                                 \
    do {                                                                                                                     \
        if (wave)                                                                                                            \
            hipLaunchKernelGGL(k_pars_insert_wave<N>, dim3((unsigned)((nbranch + 3) / 4)), dim3(256), 0, e->stream,          \
                               e->pars.vec.p, e->pars.score.p, d_ends, d_taxon, nbranch, e->pars_nwords, d_out);             \
        else                                                                                                                 \
            hipLaunchKernelGGL(k_pars_insert_wg<N>, dim3((unsigned)nbranch), dim3(256), 0, e->stream, e->pars.vec.p,         \
                               e->pars.score.p, d_ends, d_taxon, nbranch, e->pars_nwords, d_out);                            \
    } while (0)
    if (e->n == 4) IQHIP_PARS_INSERT(4);
    else if (e->n == 20) IQHIP_PARS_INSERT(20);
    else if (e->n == 64) IQHIP_PARS_INSERT(64);
    else return hipErrorInvalidValue;
#undef IQHIP_PARS_INSERT
    hipError_t s = hipGetLastError();
    if (s != hipSuccess) return s;
    *nlaunches = 1;
    hipLaunchKernelGGL(k_pars_argmin_seg, dim3((unsigned)nseg), dim3(256), 0, e->stream, d_out, d_seg_start, nbranch, nseg);
    s = hipGetLastError();
    if (s == hipSuccess) *nlaunches = 2;
    return s;
}

}  // namespace iqhip
