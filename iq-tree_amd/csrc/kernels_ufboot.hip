// kernels_ufboot.hip -- the ultrafast bootstrap's bookkeeping (IQTree::saveCurrentTree, iqtree.cpp:2676-2786) on the RELL
// sums R[tree][replicate] that kernels_alrt.hip forms from the engine's store of per-pattern log-likelihood rows.
//
//   k_ufboot_update   one thread per replicate s: the replicate's four state words (boot_logl, boot_orig_logl, boot_counts,
//       boot_tree) are loaded once, the entries of the chunk are applied IN LIST ORDER with the comparisons of
//       iqtree.cpp:2738-2750 word for word, and the state is stored once.  The sums of one list position are contiguous in
//       s, so a wave's loads are coalesced; the entry descriptors are wave-uniform reads.  The replaced slots are counted
//       per workgroup (integer LDS tree) and added with ONE integer atomic per workgroup; the minimum of boot_orig_logl
//       over the replicates that hold a tree goes to wgmin[workgroup], folded by the host in workgroup order.  No
//       floating-point atomic: the same bits on every run.  The state, the rule and the fold are ufboot_rule.h's, shared
//       with the partition group's update (kernels_partboot.hip).
// The file is built with -ffp-contract=off (Makefile): every comparison sees the bits a plain IEEE restatement sees.
#include <float.h>
#include <hip/hip_runtime.h>

#include "iqhip_internal.h"
#include "ufboot_rule.h"

#pragma clang fp contract(off)

namespace iqhip {

// ent[i].row: the entry's row of `sums` (an index into the chunk's distinct rows, not a store row)
__global__ __launch_bounds__(256) void k_ufboot_update(const double *__restrict__ sums, int S,
                                                       const iqhip_ufboot_tree *__restrict__ ent, int n, double epsilon,
                                                       double *__restrict__ boot_logl, double *__restrict__ boot_orig_logl,
                                                       int32_t *__restrict__ boot_counts, int64_t *__restrict__ boot_tree,
                                                       unsigned long long *__restrict__ replaced, double *__restrict__ wgmin) {
    const int s = blockIdx.x * 256 + threadIdx.x;
    int nrep = 0;
    double mn = DBL_MAX;
    if (s < S) {
        UfbootSlot z;
        z.load(boot_logl, boot_orig_logl, boot_counts, boot_tree, s);
        for (int i = 0; i < n; i++) z.apply(sums[(size_t)ent[i].row * S + s], ent[i], epsilon);
        mn = z.store(boot_logl, boot_orig_logl, boot_counts, boot_tree, s);
        nrep = z.nrep;
    }
    ufboot_fold(nrep, mn, replaced, wgmin);
}

int ufboot_workgroups(int nsamples) { return (nsamples + 255) / 256; }

hipError_t launch_ufboot_update(iqhip_engine *e, const double *sums, int nsamples, const iqhip_ufboot_tree *d_entries, int n,
                                double epsilon, double *boot_logl, double *boot_orig_logl, int32_t *boot_counts,
                                int64_t *boot_tree, unsigned long long *replaced, double *wgmin) {
    hipLaunchKernelGGL(k_ufboot_update, dim3((unsigned)ufboot_workgroups(nsamples)), dim3(256), 0, e->stream, sums, nsamples,
                       d_entries, n, epsilon, boot_logl, boot_orig_logl, boot_counts, boot_tree, replaced, wgmin);
    return hipGetLastError();
}

}  // namespace iqhip
