// kernels_partdist.hip -- joint pairwise maximum-likelihood distances of an edge-linked partition group
// (PhyloSuperTreePlen::computeDist, phylosupertreeplen.cpp:361-371, per pair SuperAlignmentPairwisePlen, :18-45).
//
//   k_partpair_solve   one wave per pair.  Every member's counts of the pair (launch_pair_counts, kernels_dist.hip) are
//       compacted ONCE into the member's cell list in device memory (n^2 x 2 bytes per pair and member: the LDS of the wave
//       does not grow with the number of members); the start is SuperAlignment::computeDist (superalignment.cpp:384-421:
//       the members' counts pooled, z from member 0's state count), a start of MAX_GENETIC_DIST is returned without a solve
//       (phylosupertree.cpp:697); then minimizeNewton (newton_init / newton_update) on
//           df = sum_p r_p df_p(r_p x),   ddf = sum_p r_p^2 ddf_p(r_p x)      in member order,
//       (df_p, ddf_p) being pair_func_derv of pair_eval.h -- the evaluation k_pair_solve runs for one engine.  A member in
//       which the pair shares no column contributes 0.  No host round trip per step.
//       LDS: e[max ncat * n] ++ lam[max n] ++ lam2[max n] doubles, refilled per member and evaluation.
// Built with -ffp-contract=off (Makefile), like kernels_dist.hip.
#include <hip/hip_runtime.h>

#include "iqhip_internal.h"
#include "pair_eval.h"

#pragma clang fp contract(off)

namespace iqhip {

__global__ __launch_bounds__(64) void k_partpair_solve(const PartPairArgs A) {
    extern __shared__ double s_dyn[];
    const int lane = threadIdx.x, P = A.nparts;
    const size_t slot = blockIdx.x;
    double *s_e = s_dyn, *s_lam = s_e + A.e_doubles, *s_lam2 = s_lam + A.max_n;
    int32_t *nnz = A.nnz + slot * (size_t)P;
    double total = 0.0, same = 0.0;
    for (int p = 0; p < P; p++) {
        const PartPairDesc &D = A.desc[p];
        const size_t nn = (size_t)D.n * D.n;
        const int k = pair_compact_cells(D.counts + slot * nn, D.n, lane, D.cells + slot * nn, &total, &same);
        if (lane == 0) nnz[p] = k;
    }
    total = __shfl(wave_sum64(total), 0);
    same = __shfl(wave_sum64(same), 0);
    const int64_t pair = A.first_pair + (int64_t)slot;
    double guess = A.init ? A.init[pair] : 0.0;
    if (guess == 0.0) {   // SuperAlignment::computeDist: the pooled counts, z of partitions[0]->num_states
        guess = kMaxGeneticDist;
        if (total > 0.0) {
            const int n0 = A.desc[0].n;
            const double z = (double)n0 / (double)(n0 - 1);
            const double x = 1.0 - z * ((total - same) / total);
            if (x > 0.0) guess = -log(x) / z;
        }
    }
    double *o = A.out + 4 * (size_t)pair;
    if (guess == kMaxGeneticDist) {   // (wave-uniform) no solve: phylosupertreeplen.cpp:365
        if (lane == 0) {
            o[0] = kMaxGeneticDist;
            o[1] = 0.0;
            o[2] = 0.0;
            o[3] = 0.0;
        }
        return;
    }
    __syncthreads();   // the cell lists and their lengths are visible to the whole wave
    NewtonState st;
    newton_init(st, guess, A.x1, A.x2, A.xacc, A.max_steps);
    while (!st.done) {   // (wave-uniform: every lane advances the same state with the same sums)
        const double t = st.rts;
        double df = 0.0, ddf = 0.0;
        for (int p = 0; p < P; p++) {
            const PartPairDesc &D = A.desc[p];
            const int k = nnz[p];
            double pdf = 0.0, pddf = 0.0;
            if (k > 0) {   // (wave-uniform)
                const size_t nn = (size_t)D.n * D.n;
                __syncthreads();   // the member before has read its eigenvalues
                for (int i = lane; i < D.n; i += 64) {
                    const double l = D.eval[i];
                    s_lam[i] = l;
                    s_lam2[i] = l * l;
                }
                const PairEval E = {D.counts + slot * nn, D.coef, D.rates, D.props, D.cells + slot * nn, s_lam, s_lam2, s_e, D.n, D.ncat, k};
                pair_func_derv(E, t * D.rate, lane, &pdf, &pddf);
            }
            const double r = D.rate, rdf = r * pdf, rddf = (r * r) * pddf;
            df = p == 0 ? rdf : df + rdf;
            ddf = p == 0 ? rddf : ddf + rddf;
        }
        newton_update(st, df, ddf);
    }
    if (lane == 0) {
        o[0] = st.result;
        o[1] = st.d2l;
        o[2] = (double)st.neval;
        o[3] = (double)st.status;
    }
}

size_t partpair_solve_lds_bytes(int e_doubles, int max_n) { return sizeof(double) * ((size_t)e_doubles + 2 * (size_t)max_n); }

hipError_t launch_partpair_solve(hipStream_t s, const PartPairArgs &a, int npairs) {
    if (npairs < 1) return hipSuccess;
    hipLaunchKernelGGL(k_partpair_solve, dim3((unsigned)npairs), dim3(64), partpair_solve_lds_bytes(a.e_doubles, a.max_n), s, a);
    return hipGetLastError();
}

}  // namespace iqhip
