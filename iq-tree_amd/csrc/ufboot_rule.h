// ufboot_rule.h -- what k_ufboot_update (kernels_ufboot.hip) and k_part_ufboot_update (kernels_partboot.hip) share, so that
// the two stay word for word by construction: one replicate's state, the comparisons of IQTree::saveCurrentTree
// (iqtree.cpp:2738-2750) for one entry, and the fold of a workgroup's replaced count and minimum.  The kernels differ only
// in how an entry's `rell` is formed.  Both files are built with -ffp-contract=off (Makefile).
#pragma once
#include <float.h>
#include <hip/hip_runtime.h>

#include "iqhip_internal.h"

#pragma clang fp contract(off)

namespace iqhip {

// the four state words of replicate s, loaded once and stored once, and the slots this thread replaced
struct UfbootSlot {
    double bl, bo;
    int32_t bc;
    int64_t bt;
    int nrep;
    __device__ __forceinline__ void load(const double *boot_logl, const double *boot_orig_logl, const int32_t *boot_counts,
                                         const int64_t *boot_tree, int s) {
        bl = boot_logl[s];
        bo = boot_orig_logl[s];
        bc = boot_counts[s];
        bt = boot_tree[s];
        nrep = 0;
    }
    // one entry, iqtree.cpp:2738-2750
    __device__ __forceinline__ void apply(double rell, const iqhip_ufboot_tree &e, double epsilon) {
        bool better = rell > bl + epsilon;
        if (!better && rell > bl - epsilon) better = (e.rand <= 1.0 / (bc + 1));
        if (better) {
            if (rell <= bl + epsilon) bc++;
            else bc = 1;
            bl = bl < rell ? rell : bl;   // max(boot_logl, rell)
            bo = e.logl;
            bt = e.tree_id;
            nrep++;
        }
    }
    // -> the replicate's term of the minimum of boot_orig_logl: DBL_MAX while it holds no tree
    __device__ __forceinline__ double store(double *boot_logl, double *boot_orig_logl, int32_t *boot_counts, int64_t *boot_tree,
                                            int s) const {
        boot_logl[s] = bl;
        boot_orig_logl[s] = bo;
        boot_counts[s] = bc;
        boot_tree[s] = bt;
        return bt >= 0 ? bo : DBL_MAX;
    }
};

// a workgroup of 256: the replaced slots counted (integer LDS tree) and added with ONE integer atomic, the minimum to
// wgmin[workgroup].  Every thread of the workgroup calls it (nrep = 0, mn = DBL_MAX past the last replicate)
__device__ __forceinline__ void ufboot_fold(int nrep, double mn, unsigned long long *__restrict__ replaced,
                                            double *__restrict__ wgmin) {
    __shared__ int s_cnt[256];
    __shared__ double s_min[256];
    s_cnt[threadIdx.x] = nrep;
    s_min[threadIdx.x] = mn;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            s_cnt[threadIdx.x] += s_cnt[threadIdx.x + o];
            const double other = s_min[threadIdx.x + o];
            if (other < s_min[threadIdx.x]) s_min[threadIdx.x] = other;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if (s_cnt[0] > 0) atomicAdd(replaced, (unsigned long long)s_cnt[0]);
        wgmin[blockIdx.x] = s_min[0];
    }
}

}  // namespace iqhip
