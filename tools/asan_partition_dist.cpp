// Stand-alone driver of the plain C++ side of the starting tree of a partitioned alignment for tools/asan_partition_dist.sh
// (AddressSanitizer + UBSan on the CPU): the chunk and cell-list layout of iq-tree_amd/csrc/partpair_layout.h and the weighted
// mean of iq-tree_amd/host/supertree_brlen.h.
#include <stdio.h>
#include <stdlib.h>

#include "../iq-tree_amd/csrc/partpair_layout.h"
#include "../iq-tree_amd/host/supertree_brlen.h"

static int failures = 0;
#define EXPECT(cond)                                                     \
    do {                                                                 \
        if (!(cond)) {                                                   \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            failures++;                                                  \
        }                                                                \
    } while (0)

int main() {
    // ---- layout: every (slot, member, cell) of a chunk owns one element of a buffer of chunk * sum_nn, no two the same
    const std::vector<std::vector<int>> groups = {{4}, {4, 4, 20}, {64, 4}, {64, 64, 64, 64, 64, 64, 64, 64, 64, 64}, {20, 4, 64, 4}};
    for (const std::vector<int> &n : groups)
        for (int64_t npairs : {1, 3, 10, 136, 4950, 1000000})
            for (int64_t over : {0, 1, 7, 37, 100000000}) {
                const iqhip::PartPairLayout L = iqhip::partpair_layout(n.data(), (int)n.size(), npairs, over);
                size_t sum = 0;
                for (int v : n) sum += (size_t)v * v;
                EXPECT(L.sum_nn == sum && L.cell_first.size() == n.size());
                EXPECT(L.chunk >= 1 && L.chunk <= npairs);
                if (over > 0) EXPECT(L.chunk == std::min(over, npairs));
                else EXPECT(L.chunk == npairs || (size_t)L.chunk * sum * 8 <= ((size_t)64 << 20));
                if (over == 0 && L.chunk < npairs) EXPECT((size_t)(L.chunk + 1) * sum * 8 > ((size_t)64 << 20));
                if ((size_t)L.chunk * sum > ((size_t)1 << 24)) continue;   // (the walk below stays small)
                std::vector<unsigned char> owner((size_t)L.chunk * sum, 0);
                for (size_t p = 0; p < n.size(); p++) {
                    const size_t nn = (size_t)n[p] * n[p];
                    for (int64_t slot : {(int64_t)0, L.chunk / 2, L.chunk - 1})
                        for (size_t cell : {(size_t)0, nn - 1}) {
                            const size_t at = L.cell_first[p] + (size_t)slot * nn + cell;   // D.cells + slot * nn + cell
                            EXPECT(at < owner.size());
                            if (at < owner.size()) {
                                EXPECT(owner[at] == 0 || owner[at] == p + 1);
                                owner[at] = (unsigned char)(p + 1);
                            }
                        }
                    EXPECT(L.cell_first[p] + (size_t)L.chunk * nn <= (p + 1 < n.size() ? L.cell_first[p + 1] : owner.size()));
                }
            }
    {
        const iqhip::PartPairLayout L = iqhip::partpair_layout(nullptr, 0, 5, 0);   // no member: nothing to divide by
        EXPECT(L.sum_nn == 0 && L.chunk == 5 && L.cell_first.empty());
    }

    // ---- weighted mean: member order, the codon rule, an empty denominator
    {
        const double len[3] = {0.1, 0.4, 0.25}, nsite[3] = {100.0, 300.0, 50.0};
        const char none[3] = {0, 0, 0}, all[3] = {1, 1, 1}, mixed[3] = {1, 0, 0};
        EXPECT(!iqhost::rescaleCodonBrlen(none, 3) && !iqhost::rescaleCodonBrlen(all, 3) && iqhost::rescaleCodonBrlen(mixed, 3));
        EXPECT(!iqhost::rescaleCodonBrlen(none, 0));
        const double sum = 0.0 + 0.1 * 100.0 + 0.4 * 300.0 + 0.25 * 50.0;
        EXPECT(iqhost::weightedBranchLength(len, nsite, none, 3, false) == sum / 450.0);
        EXPECT(iqhost::weightedBranchLength(len, nsite, all, 3, false) == sum / 450.0);
        EXPECT(iqhost::weightedBranchLength(len, nsite, mixed, 3, true) == sum / 650.0);
        EXPECT(iqhost::weightedBranchLength(len, nsite, none, 1, false) == 0.1 * 100.0 / 100.0);
        EXPECT(iqhost::weightedBranchLength(len, nsite, none, 0, false) == 0.0);
        const double zero[2] = {0.0, 0.0};
        EXPECT(iqhost::weightedBranchLength(len, zero, none, 2, false) == 0.0);
    }
    if (failures) {
        fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    printf("asan_partition_dist: ok\n");
    return 0;
}
