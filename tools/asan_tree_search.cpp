// Stand-alone driver of iq-tree_amd/host/search_host.h for tools/asan_tree_search.sh (AddressSanitizer + UBSan on the CPU):
// the sort and the non-conflicting selection on drawn move lists, branchesForNNI on random binary trees, the candidate set
// through replacement and eviction, the stop rule, the correlation of split-count tables and the random stream.
#include <stdio.h>
#include <stdlib.h>

#include <random>

#include "../iq-tree_amd/host/search_host.h"

static int failures = 0;
#define EXPECT(cond)                                                     \
    do {                                                                 \
        if (!(cond)) {                                                   \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            failures++;                                                  \
        }                                                                \
    } while (0)

struct Move {
    int node1, node2;
    double newloglh;
    int tag;
};

// random unrooted binary tree: leaves 0 .. n-1, internal nodes n .. 2n-3, by inserting each new leaf into a random branch
static iqsearch::Adjacency randomTree(std::mt19937_64 &gen, int n) {
    iqsearch::Adjacency adj((size_t)(2 * n - 2));
    auto link = [&](int a, int b) { adj[(size_t)a].push_back(b); adj[(size_t)b].push_back(a); };
    auto unlink = [&](int a, int b) {
        adj[(size_t)a].erase(std::find(adj[(size_t)a].begin(), adj[(size_t)a].end(), b));
        adj[(size_t)b].erase(std::find(adj[(size_t)b].begin(), adj[(size_t)b].end(), a));
    };
    int next = n;
    link(0, next); link(1, next); link(2, next);
    next++;
    for (int leaf = 3; leaf < n; leaf++) {
        std::vector<std::pair<int, int>> edges;
        for (int a = 0; a < next; a++)
            for (int b : adj[(size_t)a])
                if (a < b) edges.push_back({a, b});
        const auto e = edges[gen() % edges.size()];
        unlink(e.first, e.second);
        link(e.first, next); link(e.second, next); link(leaf, next);
        next++;
    }
    return adj;
}

int main() {
    using namespace iqsearch;
    std::mt19937_64 gen(12345);

    // sort + selection
    for (int trial = 0; trial < 200; trial++) {
        std::vector<Move> mv((size_t)(gen() % 40));
        for (size_t k = 0; k < mv.size(); k++) mv[k] = Move{(int)(gen() % 15), (int)(gen() % 15), (double)(gen() % 5), (int)k};
        sortMoves(mv);
        for (size_t k = 1; k < mv.size(); k++) {
            EXPECT(mv[k - 1].newloglh >= mv[k].newloglh);
            if (mv[k - 1].newloglh == mv[k].newloglh) EXPECT(mv[k - 1].tag < mv[k].tag);   // stable
        }
        const std::vector<Move> sel = selectNonConflicting(mv);
        for (size_t a = 0; a < sel.size(); a++)
            for (size_t b = a + 1; b < sel.size(); b++)
                EXPECT(sel[a].node1 != sel[b].node1 && sel[a].node1 != sel[b].node2 && sel[a].node2 != sel[b].node1 &&
                       sel[a].node2 != sel[b].node2);
        if (!mv.empty()) EXPECT(!sel.empty() && sel[0].tag == mv[0].tag);
    }
    EXPECT(selectNonConflicting(std::vector<Move>()).empty());

    // branchesForNNI
    for (int n : {4, 5, 9, 40, 200}) {
        const Adjacency adj = randomTree(gen, n);
        BranchList inner;
        for (int a = n; a < 2 * n - 2; a++)
            for (int b : adj[(size_t)a])
                if (b > a) inner.push_back({a, b});
        EXPECT((int)inner.size() == n - 3);
        for (int trial = 0; trial < 20; trial++) {
            std::vector<Move> applied;
            for (int k = 0; k < 1 + (int)(gen() % 3); k++) {
                const auto br = inner[gen() % inner.size()];
                applied.push_back(gen() & 1 ? Move{br.first, br.second, 0, k} : Move{br.second, br.first, 0, k});
            }
            const BranchList got = branchesForNNI(applied, adj);
            EXPECT(!got.empty() && got.size() <= inner.size());
            for (size_t q = 0; q < got.size(); q++) {
                EXPECT(branchExist(got[q].first, got[q].second, inner));
                for (size_t r = q + 1; r < got.size(); r++)
                    EXPECT(!((got[q].first == got[r].first && got[q].second == got[r].second) ||
                             (got[q].first == got[r].second && got[q].second == got[r].first)));
            }
        }
        EXPECT(branchesForNNI(std::vector<Move>(), adj).empty());
    }

    // candidate set
    {
        CandidateSet cs;
        cs.maxCandidates = 8;
        EXPECT(cs.getBestScore() < -1e300 && cs.getTopTrees().empty());
        for (int k = 0; k < 500; k++) {
            const std::string topo = "T" + std::to_string(gen() % 30);
            const double score = -(double)(gen() % 1000);
            const bool known = cs.treeTopologyExist(topo);
            const double before = known ? cs.getTopologyScore(topo) : 0.0;
            const bool is_new = cs.update("tree" + std::to_string(k), topo, score);
            EXPECT(is_new == !known);
            if (known) EXPECT(cs.getTopologyScore(topo) == std::max(before, score));
            for (size_t r = 1; r < cs.size(); r++) EXPECT(cs.byRank(r - 1).score >= cs.byRank(r).score);
            for (size_t a = 0; a < cs.size(); a++)
                for (size_t b = a + 1; b < cs.size(); b++) EXPECT(cs.byRank(a).topology != cs.byRank(b).topology);
            const size_t rank = cs.randCandRank(5, searchRand(1, (uint64_t)k, 0));
            EXPECT(rank < std::min<size_t>(5, cs.size()));
            EXPECT(cs.getRandCandTree(5, searchRand(1, (uint64_t)k, 0)) == cs.byRank(rank).tree);
        }
        EXPECT(cs.getTopTrees(3).size() == 3 && cs.getTopTrees(3)[0] == cs.byRank(0).tree);
    }

    // stop rule
    {
        StopRule r;
        r.stop_condition = SC_FIXED_ITERATION;
        r.min_iteration = 3;
        EXPECT(!r.meetStopCondition(3, 0.0) && r.meetStopCondition(4, 0.0));
        r.stop_condition = SC_UNSUCCESS_ITERATION;
        r.addImprovedIteration(7);
        EXPECT(!r.meetStopCondition(106, 0.0) && r.meetStopCondition(107, 0.0));
        r.stop_condition = SC_BOOTSTRAP_CORRELATION;
        EXPECT(r.meetStopCondition(107, 0.99) && !r.meetStopCondition(107, 0.98) && r.meetStopCondition(1001, 0.0));
    }

    // correlation of split-count tables (one, two and three words per split)
    for (int ntaxa : {8, 70, 130}) {
        std::vector<ufboot::SplitCounts> snaps;
        EXPECT(bootstrapCorrelation(snaps) == 0.0);
        for (int s = 0; s < 5; s++) {
            ufboot::SplitCounts sc(ntaxa);
            for (int k = 0; k < 12; k++) {
                ufboot::Split sp(ufboot::splitWords(ntaxa), 0);
                ufboot::splitSet(sp, 1 + (int)(gen() % (ntaxa - 1)));
                ufboot::splitSet(sp, 1 + (int)(gen() % (ntaxa - 1)));
                if (ufboot::splitTrivial(sp, ntaxa)) continue;
                sc.addTree(std::vector<ufboot::Split>(1, sp), 1 + (int64_t)(gen() % 100));
            }
            snaps.push_back(sc);
            const double c = bootstrapCorrelation(snaps);
            EXPECT(snaps.size() < 2 ? c == 0.0 : (c >= -1.0000001 && c <= 1.0000001));
        }
        EXPECT(fabs(bootstrapCorrelation(snaps[0], snaps[0]) - 1.0) < 1e-12);
        EXPECT(bootstrapCorrelation(ufboot::SplitCounts(ntaxa), ufboot::SplitCounts(ntaxa)) == 1.0);
    }

    // random stream
    {
        int hist[7] = {0, 0, 0, 0, 0, 0, 0};
        for (uint64_t d = 0; d < 7000; d++) hist[searchRandInt(searchRand(3, 1, d), 7)]++;
        for (int h : hist) EXPECT(h > 800);
        EXPECT(searchRandInt(~0ull, 7) == 6 && searchRandInt(0, 7) == 0 && searchRandInt(99, 1) == 0 && searchRandInt(99, 0) == 0);
        EXPECT(searchRand(1, 2, 3) != searchRand(1, 3, 2));
    }

    if (failures) {
        fprintf(stderr, "asan_tree_search: %d check(s) failed\n", failures);
        return 1;
    }
    printf("asan_tree_search: ok\n");
    return 0;
}
