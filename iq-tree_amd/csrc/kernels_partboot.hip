// kernels_partboot.hip -- RELL sums and the ultrafast bootstrap's bookkeeping of an edge-linked partition model.
//
// The RELL score of a super tree in replicate s is  sum_p sum_ptn W_p[s][ptn] * L_p[row][ptn]:  every member p of the group
// forms its own product R_p = L_p W_p^T with launch_alrt_product (kernels_alrt.hip) on its own stream, from its own store
// of per-pattern rows and its own sample matrix (resampling WITHIN partitions, superalignment.cpp:360-370).  The kernels
// here read the members' [M][S] sums through a device table of nparts pointers and add them IN MEMBER ORDER,
//     rell = ((R_0 + R_1) + R_2) + ...
//   k_part_rell_sum       the summed matrix itself (iqhip_partition_ptnlh_rell)
//   k_part_ufboot_update  k_ufboot_update (kernels_ufboot.hip) with `rell` formed as that sum inside the update: no M x S
//       summed matrix is materialised.  One thread per replicate; the sums of eight entries are loaded together (all
//       members' loads in flight at once), then the entries are applied IN LIST ORDER with the comparisons of
//       iqtree.cpp:2738-2750 (ufboot_rule.h, shared with k_ufboot_update), one integer atomic per workgroup for the replaced count, the minimum per
//       workgroup folded by the host in workgroup order.  No floating-point atomic: the same bits on every run.
// The file is built with -ffp-contract=off (Makefile): every sum and comparison sees the bits a plain IEEE restatement sees.
#include <float.h>
#include <hip/hip_runtime.h>

#include "iqhip_internal.h"
#include "ufboot_rule.h"

#pragma clang fp contract(off)

namespace iqhip {

constexpr int kPartBootAhead = 8;   // entries whose sums k_part_ufboot_update forms before it applies them

// the member-order sum of element i of the members' matrices
__device__ __forceinline__ double part_rell(const double *const *__restrict__ sums, int nparts, size_t i) {
    double r = sums[0][i];
    for (int p = 1; p < nparts; p++) r = r + sums[p][i];
    return r;
}

__global__ __launch_bounds__(256) void k_part_rell_sum(const double *const *__restrict__ sums, int nparts, size_t count,
                                                       double *__restrict__ out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    out[i] = part_rell(sums, nparts, i);
}

// ent[i].row: the entry's row of every member's sums (an index into the chunk's distinct rows, not a store row)
__global__ __launch_bounds__(256) void k_part_ufboot_update(const double *const *__restrict__ sums, int nparts, int S,
                                                            const iqhip_ufboot_tree *__restrict__ ent, int n, double epsilon,
                                                            double *__restrict__ boot_logl, double *__restrict__ boot_orig_logl,
                                                            int32_t *__restrict__ boot_counts, int64_t *__restrict__ boot_tree,
                                                            unsigned long long *__restrict__ replaced,
                                                            double *__restrict__ wgmin) {
    const int s = blockIdx.x * 256 + threadIdx.x;
    int nrep = 0;
    double mn = DBL_MAX;
    if (s < S) {
        UfbootSlot z;
        z.load(boot_logl, boot_orig_logl, boot_counts, boot_tree, s);
        // kPartBootAhead entries at a time: their sums are formed first -- the loads of all of them and of all members are in
        // flight together, each sum still in member order -- and the entries are then applied in list order
        for (int i0 = 0; i0 < n; i0 += kPartBootAhead) {
            double ahead[kPartBootAhead];
            size_t at[kPartBootAhead];
#pragma unroll
            for (int u = 0; u < kPartBootAhead; u++) at[u] = (size_t)ent[i0 + u < n ? i0 + u : i0].row * S + s;
            for (int p = 0; p < nparts; p++) {   // (member by member: ahead[u] = ((R_0 + R_1) + R_2) + ..)
                const double *__restrict__ R = sums[p];
#pragma unroll
                for (int u = 0; u < kPartBootAhead; u++) {
                    const double v = R[at[u]];
                    ahead[u] = p == 0 ? v : ahead[u] + v;
                }
            }
#pragma unroll
            for (int u = 0; u < kPartBootAhead; u++)
                if (i0 + u < n) z.apply(ahead[u], ent[i0 + u], epsilon);
        }
        mn = z.store(boot_logl, boot_orig_logl, boot_counts, boot_tree, s);
        nrep = z.nrep;
    }
    ufboot_fold(nrep, mn, replaced, wgmin);
}

hipError_t launch_part_rell_sum(hipStream_t s, const double *const *d_sums, int nparts, size_t count, double *out) {
    hipLaunchKernelGGL(k_part_rell_sum, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, d_sums, nparts, count, out);
    return hipGetLastError();
}

hipError_t launch_part_ufboot_update(hipStream_t s, const double *const *d_sums, int nparts, int nsamples,
                                     const iqhip_ufboot_tree *d_entries, int n, double epsilon, double *boot_logl,
                                     double *boot_orig_logl, int32_t *boot_counts, int64_t *boot_tree,
                                     unsigned long long *replaced, double *wgmin) {
    hipLaunchKernelGGL(k_part_ufboot_update, dim3((unsigned)ufboot_workgroups(nsamples)), dim3(256), 0, s, d_sums, nparts,
                       nsamples, d_entries, n, epsilon, boot_logl, boot_orig_logl, boot_counts, boot_tree, replaced, wgmin);
    return hipGetLastError();
}

}  // namespace iqhip
