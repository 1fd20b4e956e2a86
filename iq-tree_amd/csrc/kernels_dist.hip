// kernels_dist.hip -- pairwise maximum-likelihood distances (PhyloTree::computeDist, phylotree.cpp:2432-2541; per pair
// AlignmentPairwise, alignmentpairwise.cpp:29-312, and Optimization::minimizeNewton).
//
//   k_pair_counts4 / k_pair_counts_lds   AlignmentPairwise's constructor for a tile of 4 x 4 taxa: counts[pair][a * n + b] =
//       sum of ptn_freq over the patterns where the pair shows the unambiguous states (a, b).  A workgroup owns one tile and
//       its waves own sub-tiles of 2 x 2 pairs (1 x 1 at 64 states), so a lane reads the state bytes of two row pairs and the
//       frequency of a pattern once for four pairs.
//         4 states: 16 tallies per pair in the lane's registers (a select chain, no memory traffic, no serialisation on the
//           four diagonal cells that close sequences hit almost exclusively), one wave sum per cell at the end;
//         20 / 64 states: an n x n table per pair in the wave's own LDS, updated with LDS atomics.
//       Integer-valued frequencies below 2^53 sum exactly in any order: the same bits on every run.
//   k_pair_coef    coef[i][j][k] = evec[i][k] * inv_evec[k][j], once per call.
//   k_pair_solve   one wave per pair: the JC start (Alignment::computeJCDist), then minimizeNewton over
//       AlignmentPairwise::computeFuncDerv's default branch -- newton_init / newton_update of iqhip_internal.h, the one
//       restatement of the reference's update rule -- until the pair is done; only the cells with a non-zero count are
//       evaluated (compacted once per pair; the evaluation itself is pair_eval.h).  No host round trip per step.
// Built with -ffp-contract=off (Makefile), like kernels_topo.hip: the arithmetic is the one a plain IEEE restatement does.
#include <hip/hip_runtime.h>

#include "iqhip_internal.h"
#include "pair_eval.h"

#pragma clang fp contract(off)

namespace iqhip {

// ---- counts -------------------------------------------------------------------------------------------------------------
// 4 states: wave w of the workgroup owns the pairs (x, y), x in {2 (w >> 1), +1}, y in {2 (w & 1), +1} of the tile
__global__ __launch_bounds__(256) void k_pair_counts4(const PairTile *__restrict__ tiles, const uint8_t *__restrict__ states,
                                                      int64_t nptn_pad, int64_t nptn, const double *__restrict__ freq,
                                                      double *__restrict__ counts) {
    const PairTile &T = tiles[blockIdx.x];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int x0 = 2 * (w >> 1), y0 = 2 * (w & 1);
    int out[4];
#pragma unroll
    for (int q = 0; q < 4; q++) out[q] = T.out[(x0 + (q >> 1)) * 4 + y0 + (q & 1)];
    if ((out[0] & out[1] & out[2] & out[3]) < 0) return;   // (wave-uniform: no pair of this sub-tile is asked for)
    const uint8_t *A0 = states + (size_t)T.ra[x0] * nptn_pad, *A1 = states + (size_t)T.ra[x0 + 1] * nptn_pad;
    const uint8_t *B0 = states + (size_t)T.rb[y0] * nptn_pad, *B1 = states + (size_t)T.rb[y0 + 1] * nptn_pad;
    double acc[4][16];
#pragma unroll
    for (int q = 0; q < 4; q++)
#pragma unroll
        for (int k = 0; k < 16; k++) acc[q][k] = 0.0;
    for (int64_t p = lane; p < nptn; p += 64) {
        const double f = freq[p];
        const int sa[2] = {A0[p], A1[p]}, sb[2] = {B0[p], B1[p]};
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int a = sa[q >> 1], b = sb[q & 1];
            const double v = (a < 4 && b < 4) ? f : 0.0;   // ambiguity codes, gaps, STATE_UNKNOWN: skipped (addPattern)
            const int cell = a * 4 + b;
#pragma unroll
            for (int k = 0; k < 16; k++) acc[q][k] += cell == k ? v : 0.0;
        }
    }
#pragma unroll
    for (int q = 0; q < 4; q++) {
        double mine = 0.0;
#pragma unroll
        for (int k = 0; k < 16; k++) {
            const double tot = wave_sum64(acc[q][k]);
            if (lane == k) mine = tot;
        }
        if (out[q] >= 0 && lane < 16) counts[(size_t)out[q] * 16 + lane] = mine;
    }
}

// 20 / 64 states: W waves per workgroup, sub-tiles of TW x TW pairs go round the waves; every wave keeps TW * TW tables of
// N * N doubles in LDS.  The barriers are reached by all waves the same number of times (rounds), whatever a wave has to do.
template <int N, int TW, int W>
__global__ __launch_bounds__(64 * W) void k_pair_counts_lds(const PairTile *__restrict__ tiles,
                                                            const uint8_t *__restrict__ states, int64_t nptn_pad,
                                                            int64_t nptn, const double *__restrict__ freq,
                                                            double *__restrict__ counts) {
    extern __shared__ double s_tab[];   // [W][TW * TW][N * N]
    constexpr int NN = N * N, Q = TW * TW, SIDE = 4 / TW, NSUB = SIDE * SIDE;
    const PairTile &T = tiles[blockIdx.x];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double *tab = s_tab + (size_t)w * Q * NN;
    for (int round = 0; round * W < NSUB; round++) {
        const int s = round * W + w;
        const int x0 = (s / SIDE) * TW, y0 = (s % SIDE) * TW;
        int out[Q];
        bool any = false;
#pragma unroll
        for (int q = 0; q < Q; q++) {
            out[q] = s < NSUB ? T.out[(x0 + q / TW) * 4 + y0 + q % TW] : -1;
            any = any || out[q] >= 0;
        }
        if (any)
            for (int i = lane; i < Q * NN; i += 64) tab[i] = 0.0;
        __syncthreads();
        if (any) {
            const uint8_t *A[TW], *B[TW];
#pragma unroll
            for (int t = 0; t < TW; t++) {
                A[t] = states + (size_t)T.ra[x0 + t] * nptn_pad;
                B[t] = states + (size_t)T.rb[y0 + t] * nptn_pad;
            }
            for (int64_t p = lane; p < nptn; p += 64) {
                const double f = freq[p];
                if (f == 0.0) continue;   // (the unobserved +ASC patterns contribute nothing)
                int sa[TW], sb[TW];
#pragma unroll
                for (int t = 0; t < TW; t++) {
                    sa[t] = A[t][p];
                    sb[t] = B[t][p];
                }
#pragma unroll
                for (int q = 0; q < Q; q++) {
                    const int a = sa[q / TW], b = sb[q % TW];
                    if (out[q] >= 0 && a < N && b < N) atomicAdd(&tab[q * NN + a * N + b], f);
                }
            }
        }
        __syncthreads();
        if (any) {
#pragma unroll
            for (int q = 0; q < Q; q++)
                if (out[q] >= 0)
                    for (int i = lane; i < NN; i += 64) counts[(size_t)out[q] * NN + i] = tab[q * NN + i];
        }
        __syncthreads();
    }
}

// ---- solver -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_pair_coef(const double *__restrict__ evec, const double *__restrict__ inv_evec, int n,
                                                   double *__restrict__ coef) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)n * n * n) return;
    const int k = (int)(idx % n), j = (int)(idx / n % n), i = (int)(idx / n / n);
    coef[idx] = evec[(size_t)i * n + k] * inv_evec[(size_t)k * n + j];
}

// one workgroup of one wave per pair slot.  LDS: e[ncat * n] ++ lam[n] ++ lam2[n] doubles ++ the non-zero cells (uint16)
__global__ __launch_bounds__(64) void k_pair_solve(const PairSolveArgs A) {
    extern __shared__ double s_dyn[];
    const int n = A.n, ncat = A.ncat, nn = n * n, lane = threadIdx.x;
    const int slot = blockIdx.x;
    double *s_e = s_dyn, *s_lam = s_e + (size_t)ncat * n, *s_lam2 = s_lam + n;
    uint16_t *s_cell = reinterpret_cast<uint16_t *>(s_lam2 + n);
    const double *cnt = A.counts + (size_t)slot * nn;
    // the non-zero cells in cell order, and the two sums of the JC start
    double total = 0.0, same = 0.0;
    const int nnz = pair_compact_cells(cnt, n, lane, s_cell, &total, &same);
    for (int k = lane; k < n; k += 64) {
        const double l = A.eval[k];
        s_lam[k] = l;
        s_lam2[k] = l * l;
    }
    total = __shfl(wave_sum64(total), 0);
    same = __shfl(wave_sum64(same), 0);
    const int64_t pair = A.first_pair + slot;
    double guess = A.init ? A.init[pair] : 0.0;
    if (guess == 0.0) {   // Alignment::computeJCDist, alignment.cpp:2552-2584
        guess = kMaxGeneticDist;
        if (total > 0.0) {
            const double z = (double)n / (double)(n - 1);
            const double x = 1.0 - z * ((total - same) / total);
            if (x > 0.0) guess = -log(x) / z;
        }
    }
    NewtonState st;
    newton_init(st, guess, A.x1, A.x2, A.xacc, A.max_steps);
    const PairEval E = {cnt, A.coef, A.rates, A.props, s_cell, s_lam, s_lam2, s_e, n, ncat, nnz};
    while (!st.done) {   // (wave-uniform: every lane advances the same state with the same sums)
        // computeFuncDerv's df = -pdf, ddf = -pddf; newton_update takes the likelihood's derivatives and negates
        double pdf, pddf;
        pair_func_derv(E, st.rts, lane, &pdf, &pddf);
        newton_update(st, pdf, pddf);
    }
    if (lane == 0) {
        double *o = A.out + 4 * (size_t)pair;
        o[0] = st.result;
        o[1] = st.d2l;
        o[2] = (double)st.neval;
        o[3] = (double)st.status;
    }
}

// ---- launches -------------------------------------------------------------------------------------------------------------
hipError_t launch_pair_counts(iqhip_engine *e, const PairTile *d_tiles, int ntiles, double *d_counts) {
    if (ntiles < 1) return hipSuccess;
    if (e->n == 4) {
        hipLaunchKernelGGL(k_pair_counts4, dim3((unsigned)ntiles), dim3(256), 0, e->stream, d_tiles, e->d_states.p, e->nptn_pad,
                           e->nptn, e->d_freq.p, d_counts);
    } else if (e->n == 20) {
        constexpr size_t lds = sizeof(double) * 4 * 4 * 400;
        hipLaunchKernelGGL((k_pair_counts_lds<20, 2, 4>), dim3((unsigned)ntiles), dim3(256), lds, e->stream, d_tiles, e->d_states.p,
                           e->nptn_pad, e->nptn, e->d_freq.p, d_counts);
    } else if (e->n == 64) {
        constexpr size_t lds = sizeof(double) * 2 * 4096;
        const hipError_t a = raise_lds_ceiling<&k_pair_counts_lds<64, 1, 2>>(e, (int)lds);
        if (a != hipSuccess) return a;
        hipLaunchKernelGGL((k_pair_counts_lds<64, 1, 2>), dim3((unsigned)ntiles), dim3(128), lds, e->stream, d_tiles, e->d_states.p,
                           e->nptn_pad, e->nptn, e->d_freq.p, d_counts);
    } else
        return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t launch_pair_coef(iqhip_engine *e, double *d_coef) {
    const size_t n3 = (size_t)e->n * e->n * e->n;
    hipLaunchKernelGGL(k_pair_coef, dim3((unsigned)((n3 + 255) / 256)), dim3(256), 0, e->stream, e->d_evec, e->d_inv_evec, e->n,
                       d_coef);
    return hipGetLastError();
}

size_t pair_solve_lds_bytes(int n, int ncat) {
    return sizeof(double) * ((size_t)ncat * n + 2 * (size_t)n) + sizeof(uint16_t) * (((size_t)n * n + 3) / 4 * 4);
}

hipError_t launch_pair_solve(iqhip_engine *e, const PairSolveArgs &a, int npairs) {
    if (npairs < 1) return hipSuccess;
    hipLaunchKernelGGL(k_pair_solve, dim3((unsigned)npairs), dim3(64), pair_solve_lds_bytes(a.n, a.ncat), e->stream, a);
    return hipGetLastError();
}

}  // namespace iqhip
