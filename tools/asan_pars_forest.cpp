// Stand-alone driver of the plain C++ side of the parsimony forest for tools/asan_pars_forest.sh (AddressSanitizer + UBSan on
// the CPU): the addition orders and the duplicate filter of iq-tree_amd/host/search_host.h, and the slot bases, chunk sizes
// and merged segment lists of iq-tree_amd/host/pars_forest_plan.h.
#include <stdio.h>
#include <stdlib.h>

#include <set>

#include "../iq-tree_amd/host/pars_forest_plan.h"
#include "../iq-tree_amd/host/search_host.h"

static int failures = 0;
#define EXPECT(cond)                                                     \
    do {                                                                 \
        if (!(cond)) {                                                   \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            failures++;                                                  \
        }                                                                \
    } while (0)

template <class F>
static bool throws(F f) {
    try {
        f();
    } catch (const std::exception &) {
        return true;
    }
    return false;
}

int main() {
    // ---- addition orders: permutations, a function of (seed, k) alone, the draws of iteration 0
    for (uint64_t seed : {0ull, 1ull, 0xFFFFFFFFFFFFFFFFull})
        for (int ntaxa : {0, 1, 2, 3, 10, 257}) {
            const auto orders = iqsearch::parsimonyOrders(seed, 9, ntaxa);
            EXPECT(orders.size() == 9);
            for (size_t k = 0; k < orders.size(); k++) {
                std::set<int> seen(orders[k].begin(), orders[k].end());
                EXPECT((int)orders[k].size() == ntaxa && (int)seen.size() == ntaxa);
                EXPECT(seen.empty() || (*seen.begin() == 0 && *seen.rbegin() == ntaxa - 1));
                std::vector<int> o((size_t)ntaxa);
                for (int i = 0; i < ntaxa; i++) o[(size_t)i] = i;
                for (int i = ntaxa - 1; i >= 1; i--)
                    std::swap(o[(size_t)i], o[(size_t)iqsearch::searchRandInt(iqsearch::searchRand(seed, 0, (uint64_t)k * ntaxa + i), i + 1)]);
                EXPECT(o == orders[k]);
            }
            EXPECT(iqsearch::parsimonyOrders(seed, 4, ntaxa) == std::vector<std::vector<int>>(orders.begin(), orders.begin() + 4));
        }
    EXPECT(iqsearch::parsimonyOrders(1, 0, 10).empty() && iqsearch::parsimonyOrders(1, -3, 10).empty());
    EXPECT(iqsearch::parsimonyOrders(1, 8, 10) != iqsearch::parsimonyOrders(2, 8, 10));

    // ---- duplicate filter
    {
        const std::vector<std::string> keys = {"a", "b", "a", "g", "c", "b", "c"};
        EXPECT((iqsearch::duplicateKeys(keys, {"g"}) == std::vector<int>{2, 3, 5, 6}));
        EXPECT((iqsearch::duplicateKeys(keys, {}) == std::vector<int>{2, 5, 6}));
        EXPECT(iqsearch::duplicateKeys({}, {"g"}).empty());
    }

    // ---- slots: the members' ranges tile the arena behind the tips, without gaps or overlap
    for (int T : {3, 4, 9, 50, 1000}) {
        const int per = iqforest::memberVectors(T);
        EXPECT(per == 3 * T - 6 && iqforest::slotBase(T, 0) == T);
        for (int k = 0; k < 7; k++) EXPECT(iqforest::slotBase(T, k + 1) == iqforest::slotBase(T, k) + per);
        EXPECT(iqforest::arenaVectors(T, 7) == (int64_t)iqforest::slotBase(T, 7) - T);
    }
    EXPECT(iqforest::memberVectors(2) == 0);

    // ---- chunks: within the budget, never 0, never more than K, slots stay int32
    EXPECT(iqforest::memberBytes(50, 4, 100000) == (int64_t)144 * 3125 * 5 * 4);
    EXPECT(iqforest::chunkMembers(100, 50, 4, 100000, 0) == 100);                    // 0.9 GB: one chunk
    EXPECT(iqforest::chunkMembers(100, 50, 4, 1000000, 0) == 11);                    // 90 MB a tree
    EXPECT(iqforest::chunkMembers(100, 50, 64, 100000000, 0) == 1);                  // one tree over the budget: still 1
    EXPECT(iqforest::chunkMembers(100, 50, 4, 0, 0) == 100 && iqforest::chunkMembers(0, 50, 4, 10, 0) == 0);
    EXPECT(iqforest::chunkMembers(6, 9, 4, 33, 2) == 2 && iqforest::chunkMembers(6, 9, 4, 33, 50) == 6);
    {
        const int m = iqforest::chunkMembers(2000000000, 1000, 4, 1, 2000000000);
        EXPECT(m >= 1 && (int64_t)1000 + (int64_t)m * iqforest::memberVectors(1000) <= 2147483647);
    }
    EXPECT(iqforest::parseChunk(nullptr) == 0 && iqforest::parseChunk("") == 0 && iqforest::parseChunk("17") == 17);
    for (const char *bad : {"0", "-1", "two", "3x", " 4", "99999999999999999999"}) EXPECT(throws([&] { iqforest::parseChunk(bad); }));

    // ---- merged segment lists
    {
        iqforest::Segments seg;
        seg.clear();
        int32_t next = 0;
        std::vector<int> lens = {1, 3, 7, 2, 9};
        for (size_t g = 0; g < lens.size(); g++) {
            std::vector<int32_t> ends;
            for (int b = 0; b < 2 * lens[g]; b++) ends.push_back(next++);
            seg.add(ends, (int32_t)(100 + g));
        }
        EXPECT(seg.nseg() == 5 && seg.seg_start == (std::vector<int32_t>{0, 1, 4, 11, 13, 22}) && seg.ends.size() == 44);
        for (size_t k = 0; k < seg.ends.size(); k++) EXPECT(seg.ends[k] == (int32_t)k);
        EXPECT(seg.taxon == (std::vector<int32_t>{100, 101, 102, 103, 104}));
        EXPECT(throws([&] { seg.add({}, 1); }) && throws([&] { seg.add({1, 2, 3}, 1); }) && seg.nseg() == 5);
        seg.clear();
        EXPECT(seg.nseg() == 0 && seg.seg_start == std::vector<int32_t>{0} && seg.ends.empty());
        iqforest::Segments fresh;   // add without clear
        fresh.add({5, 6}, 2);
        EXPECT(fresh.seg_start == (std::vector<int32_t>{0, 1}));
    }
    if (failures) {
        fprintf(stderr, "asan_pars_forest: %d failure(s)\n", failures);
        return 1;
    }
    printf("asan_pars_forest: ok\n");
    return 0;
}
