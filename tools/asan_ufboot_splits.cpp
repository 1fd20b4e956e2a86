// Stand-alone driver of iq-tree_amd/host/ufboot_splits.h for tools/asan_ufboot_splits.sh (AddressSanitizer + UBSan on the
// CPU): the splits of well-formed and of broken Newick strings, split counts, supports and the greedy consensus on
// hand-made and on random tree sets up to 130 taxa (bitsets of one, two and three words).
#include <stdio.h>
#include <stdlib.h>

#include <random>

#include "../iq-tree_amd/host/ufboot_splits.h"

static int failures = 0;
#define EXPECT(cond)                                                     \
    do {                                                                 \
        if (!(cond)) {                                                   \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            failures++;                                                  \
        }                                                                \
    } while (0)

static std::string randomTree(std::mt19937_64 &gen, int ntaxa) {
    std::vector<std::string> parts;
    for (int t = 0; t < ntaxa; t++) parts.push_back(std::to_string(t));
    std::shuffle(parts.begin(), parts.end(), gen);
    while (parts.size() > 3) {
        size_t i = gen() % parts.size(), j = gen() % (parts.size() - 1);
        if (j >= i) j++;
        const std::string joined = "(" + parts[i] + ":0.1," + parts[j] + ")";
        if (i < j) std::swap(i, j);
        parts.erase(parts.begin() + (long)i);
        parts.erase(parts.begin() + (long)j);
        parts.push_back(joined);
    }
    std::string s = "(";
    for (size_t k = 0; k < parts.size(); k++) s += (k ? "," : "") + parts[k];
    return s + ");";
}

int main() {
    using namespace ufboot;
    std::vector<Split> sp;
    newickSplits("((0,1),2,(3,(4,5)));", 6, sp);
    EXPECT(sp.size() == 3 && splitCount(sp[0]) == 4 && splitCount(sp[1]) == 2 && splitCount(sp[2]) == 3);
    newickSplits("((Hs:1,Pt:1):1,Gg:1,(Mm:2,Rn:2)99:1[x]);", 5, sp, {"Hs", "Pt", "Gg", "Mm", "Rn"});
    EXPECT(sp.size() == 2);
    newickSplits("(0,1,2);", 3, sp);
    EXPECT(sp.empty());
    const char *broken[] = {"", ";", "(", ")", "((0,1),2", "((0,1),2,(3,(4,5));", "((0,1),2,(3,(4,4)));", "((0,1),2,(3,4));",
                            "((0,1),2,(3,(4,7)));", "((0,1),2,(3,(4,x)));", "((0,1),2,(3,(4,5)))(", "0,1,2;", "((0,1),2,(3,(4,5[)));",
                            "((0,1),2,(3,(4,99999999999)));", "(((((((((("};
    for (const char *b : broken) {
        bool threw = false;
        try {
            newickSplits(b, 6, sp);
        } catch (const std::runtime_error &) {
            threw = true;
        }
        EXPECT(threw);
    }
    SplitCounts sc(6);
    const char *trees[] = {"((0,1),2,(3,(4,5)));", "((0,2),1,(3,(4,5)));", "(0,(1,2),((3,5),4));"};
    const int64_t w[] = {3, 2, 1};
    for (int k = 0; k < 3; k++) {
        newickSplits(trees[k], 6, sp);
        sc.addTree(sp, w[k]);
    }
    EXPECT(sc.total == 6 && consensusTree(sc) == "(0,1,(2,(3,(4,5)83)100)50);");
    newickSplits("((0,1),(2,3),(4,5));", 6, sp);
    EXPECT(splitSupport(sc, sp[0], 6) == 50 && splitSupport(sc, sp[1], 6) == 0 && splitSupport(sc, sp[2], 6) == 83);
    EXPECT(splitSupport(sc, sp[0], 0) == 0);
    EXPECT(consensusTree(SplitCounts(4)) == "(0,1,2,3);");
    std::mt19937_64 gen(5);
    for (int ntaxa : {4, 5, 63, 64, 65, 130}) {
        SplitCounts rc(ntaxa);
        std::vector<std::string> all;
        for (int k = 0; k < 9; k++) {
            all.push_back(randomTree(gen, ntaxa));
            newickSplits(all.back(), ntaxa, sp);
            EXPECT((int)sp.size() == ntaxa - 3);
            rc.addTree(sp, 1 + (int64_t)(gen() % 4));
        }
        const std::string con = consensusTree(rc);
        std::vector<Split> csp;
        newickSplits(con, ntaxa, csp);
        EXPECT(csp.size() == maxCompatibleSplits(rc).size());
        for (const Split &s : csp) EXPECT(rc.count(s) > 0);
        // a tree's own splits rebuild a tree with the same splits
        newickSplits(all[0], ntaxa, sp);
        std::vector<Split> back;
        newickSplits(splitsNewick(ntaxa, sp, std::vector<std::string>(sp.size(), "")), ntaxa, back);
        std::sort(sp.begin(), sp.end());
        std::sort(back.begin(), back.end());
        EXPECT(sp == back);
    }
    if (failures) {
        fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    printf("ufboot_splits.h: all checks passed\n");
    return 0;
}
