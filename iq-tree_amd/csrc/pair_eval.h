// pair_eval.h -- one evaluation of AlignmentPairwise::computeFuncDerv's default branch (alignmentpairwise.cpp:253-279) over
// computeTransDerv (modelgtr.cpp:301-338) by one wave: the one statement of it, shared by k_pair_solve (kernels_dist.hip, one
// engine per pair) and k_partpair_solve (kernels_partdist.hip, the members of a partition group summed per pair).  Both files
// are built with -ffp-contract=off: the arithmetic is the one a plain IEEE restatement does.
#pragma once
#include <hip/hip_runtime.h>

#include "iqhip_internal.h"

#pragma clang fp contract(off)

namespace iqhip {

constexpr double kMaxGeneticDist = 9.0;   // MAX_GENETIC_DIST, tools.h

// What the wave of a pair knows of one alignment + model.  cnt: the pair's n * n counts; cells: its nnz non-zero cells in
// cell order (LDS or device memory); coef[cell][k] = evec[i][k] * inv_evec[k][j]; s_lam / s_lam2: eval[k] and its square
// in LDS; s_e: ncat * n doubles of LDS the evaluation fills
struct PairEval {
    const double *cnt, *coef, *rates, *props;
    const uint16_t *cells;
    const double *s_lam, *s_lam2;
    double *s_e;
    int n, ncat, nnz;
};

// the likelihood's derivatives at distance t over the cells with a non-zero count (computeFuncDerv's df = -*pdf, ddf =
// -*pddf), the same value in every lane.  Wave-uniform; two workgroup barriers around the fill of s_e
__device__ __forceinline__ void pair_func_derv(const PairEval &E, double t, int lane, double *pdf, double *pddf) {
    const int n = E.n, ncat = E.ncat;
    __syncthreads();
    for (int idx = lane; idx < ncat * n; idx += 64) E.s_e[idx] = exp(t * E.rates[idx / n] * E.s_lam[idx % n]);
    __syncthreads();
    double d1_sum = 0.0, d2_sum = 0.0;
    for (int q = lane; q < E.nnz; q += 64) {
        const int cell = E.cells[q];
        const double *cf = E.coef + (size_t)cell * n;
        double S = 0.0, S1 = 0.0, S2 = 0.0;
        for (int c = 0; c < ncat; c++) {
            const double *ec = E.s_e + (size_t)c * n;
            double P = 0.0, P1 = 0.0, P2 = 0.0;
            for (int k = 0; k < n; k++) {
                const double ce = cf[k] * ec[k];
                P += ce;
                P1 += ce * E.s_lam[k];
                P2 += ce * E.s_lam2[k];
            }
            if (P < 0.0) P = 0.0;   // (computeTransDerv clamps the probability only)
            const double r = E.rates[c], pr = E.props[c];
            S += pr * P;
            S1 += pr * r * P1;
            S2 += pr * (r * r) * P2;
        }
        if (S > 0.0) {
            const double d1 = S1 / S;
            d1_sum += E.cnt[cell] * d1;
            d2_sum += E.cnt[cell] * (S2 / S - d1 * d1);
        }
    }
    *pdf = __shfl(wave_sum64(d1_sum), 0);
    *pddf = __shfl(wave_sum64(d2_sum), 0);
}

// the non-zero cells of cnt[0 .. nn) in cell order -> cells (LDS or device memory; visible to the wave after the next
// barrier); returns their number and adds this lane's share of the counts and of the diagonal to *total / *same
__device__ __forceinline__ int pair_compact_cells(const double *cnt, int n, int lane, uint16_t *cells, double *total, double *same) {
    const int nn = n * n;
    int nnz = 0;
    for (int base = 0; base < nn; base += 64) {
        const int cell = base + lane;
        const double c = cell < nn ? cnt[cell] : 0.0;
        const bool nz = c > 0.0;
        const unsigned long long mask = __ballot(nz);
        if (nz) cells[nnz + __popcll(mask & ((1ull << lane) - 1ull))] = (uint16_t)cell;
        nnz += __popcll(mask);
        *total += c;
        if (nz && cell / n == cell % n) *same += c;
    }
    return nnz;
}

}  // namespace iqhip
