// supertree_brlen.h -- the weighted mean of PhyloSuperTree::computeBranchLengths behind PhyloSuperTree::fixNegativeBranch
// (supertree_host.cpp).  Plain C++ without a tree, so that tools/asan_partition_dist.sh runs it under ASan + UBSan as a
// stand-alone program.
#pragma once
#include <stddef.h>

namespace iqhost {

// rescale_codon_brlen (phylosupertree.cpp:536-546): codon AND other members are present
inline bool rescaleCodonBrlen(const char *codon, size_t nparts) {
    bool has_codon = false, has_other = false;
    for (size_t p = 0; p < nparts; p++) (codon[p] ? has_codon : has_other) = true;
    return has_codon && has_other;
}

// PhyloSuperTree::computeBranchLengths (phylosupertree.cpp:1353-1398) for a branch that occurs once in every member: sum_p
// len_p nsite_p / sum_p nsite_p in member order; with rescale_codon_brlen a codon member counts 3 nsite_p in the denominator
inline double weightedBranchLength(const double *len, const double *nsite, const char *codon, size_t nparts, bool rescale_codon_brlen) {
    double length = 0.0, occurence = 0.0;
    for (size_t p = 0; p < nparts; p++) {
        length += len[p] * nsite[p];
        occurence += (codon[p] && rescale_codon_brlen) ? nsite[p] * 3 : nsite[p];
    }
    if (occurence != 0.0) length /= occurence;
    return length;
}

}  // namespace iqhost
