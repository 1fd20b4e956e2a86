// search_host.h -- the decisions of the NNI tree search that need no likelihood: which evaluated moves are applied together
// (IQTree::genNonconfNNIs, iqtree.cpp:2468-2483), which branches are looked at after a step (getBranchesForNNI over
// MTree::getInnerBranches, iqtree.cpp:2290-2300, mtree.cpp:842-872), the set of candidate trees (candidateset.cpp), the stop
// rule (stoprule.cpp:104-122), the correlation of bootstrap split frequencies (iqtree.cpp:2970-3057) and the search's random
// stream.  Plain C++: no HIP, no engine, no PhyloTree -- as ufboot_splits.h, on whose split counts the correlation is built.
//
// DEVIATIONS from the reference:
//   * the moves are sorted with std::stable_sort, so moves of equal newloglh keep their evaluation order; the reference's
//     std::sort leaves that order open
//   * the random numbers are this project's own counter-based stream (searchRand), not the reference's generator
//   * no stable splits (-fss): every internal branch is a candidate
#pragma once
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "ufboot_splits.h"

namespace iqsearch {

typedef std::vector<std::pair<int, int>> BranchList;   // internal branches by the ids of their two nodes
typedef std::vector<std::vector<int>> Adjacency;       // node id -> ids of its neighbours, in neighbour order

// ---- moves: any struct with node1, node2, newloglh (PhyloTree::NNIMove) ------------------------------------------------
// NNIMove::operator< (phylotree.h:227-230): descending newloglh
template <class Move>
inline void sortMoves(std::vector<Move> &moves) {
    std::stable_sort(moves.begin(), moves.end(), [](const Move &a, const Move &b) { return a.newloglh > b.newloglh; });
}

// genNonconfNNIs: in the given (sorted) order a move is taken unless one of its two nodes is an end of a move already taken
template <class Move>
inline std::vector<Move> selectNonConflicting(const std::vector<Move> &sorted) {
    std::vector<Move> taken;
    for (const Move &m : sorted) {
        bool chosen = true;
        for (const Move &t : taken)
            if (m.node1 == t.node1 || m.node2 == t.node1 || m.node1 == t.node2 || m.node2 == t.node2) {
                chosen = false;
                break;
            }
        if (chosen) taken.push_back(m);
    }
    return taken;
}

inline bool branchExist(int a, int b, const BranchList &list) {
    for (const auto &br : list)
        if ((br.first == a && br.second == b) || (br.first == b && br.second == a)) return true;
    return false;
}

// MTree::getInnerBranches: the internal branches within `depth` of `node`, walking away from `dad`, each once
inline void innerBranches(BranchList &out, int depth, int node, int dad, const Adjacency &adj) {
    if (depth == 0) return;
    for (int nb : adj[(size_t)node]) {
        if (nb == dad) continue;
        if (adj[(size_t)nb].size() > 1 && !branchExist(node, nb, out)) {
            out.push_back({node, nb});
            innerBranches(out, depth - 1, nb, node, adj);
        }
    }
}

// getBranchesForNNI on the tree AFTER the moves were applied: per applied move its own branch, then the internal branches
// up to two steps away on either side
template <class Move>
inline BranchList branchesForNNI(const std::vector<Move> &applied, const Adjacency &adj) {
    BranchList out;
    for (const Move &m : applied) {
        if (!branchExist(m.node1, m.node2, out)) out.push_back({m.node1, m.node2});
        innerBranches(out, 2, m.node1, m.node2, adj);
        innerBranches(out, 2, m.node2, m.node1, adj);
    }
    return out;
}

// ---- the random stream: splitmix64 keyed by (seed, iteration, draw index), the construction of PhyloTree::ufbootRand with
//      stream 0x5E ---------------------------------------------------------------------------------------------------------
inline uint64_t searchRand(uint64_t seed, uint64_t iteration, uint64_t draw) {
    const uint64_t G = 0x9E3779B97F4A7C15ull;
    auto mix = [](uint64_t z) {
        z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
        z ^= z >> 27; z *= 0x94D049BB133111EBull;
        z ^= z >> 31;
        return z;
    };
    return mix(mix(mix(seed + G * (0x5Eull + 1)) + G * (iteration + 1)) + G * (draw + 1));
}
// random_int(n): the top 53 bits scaled to [0, n)
inline int searchRandInt(uint64_t z, int n) {
    if (n <= 1) return 0;
    const int k = (int)((double)(z >> 11) * 0x1.0p-53 * (double)n);
    return k < n ? k : n - 1;
}

// ---- the addition orders of the K parsimony starting trees (createInitTrees -> computeParsimonyTree's shuffle,
//      phylotreepars.cpp:320-331).  Order k is a Fisher-Yates shuffle of 0 .. ntaxa-1: for i = ntaxa-1 ... 1, swap i with
//      searchRandInt(searchRand(seed, 0, k * ntaxa + i), i + 1).  Iteration 0 of the stream is otherwise unused, so the
//      search's own draws do not move.  DEVIATION: the reference shuffles with my_random_shuffle on its own generator.
inline std::vector<std::vector<int>> parsimonyOrders(uint64_t seed, int K, int ntaxa) {
    std::vector<std::vector<int>> orders;
    for (int k = 0; k < K; k++) {
        std::vector<int> o((size_t)(ntaxa > 0 ? ntaxa : 0));
        for (int i = 0; i < ntaxa; i++) o[(size_t)i] = i;
        for (int i = ntaxa - 1; i >= 1; i--) {
            const int j = searchRandInt(searchRand(seed, 0, (uint64_t)k * (uint64_t)ntaxa + (uint64_t)i), i + 1);
            std::swap(o[(size_t)i], o[(size_t)j]);
        }
        orders.push_back(o);
    }
    return orders;
}

// the indices of `keys` (topology strings) that repeat an earlier key or one of `known`, in order: what the initial
// candidate set skips and counts
inline std::vector<int> duplicateKeys(const std::vector<std::string> &keys, const std::vector<std::string> &known) {
    std::map<std::string, int> seen;
    for (const std::string &k : known) seen[k] = 1;
    std::vector<int> dup;
    for (size_t i = 0; i < keys.size(); i++)
        if (!seen.insert({keys[i], 1}).second) dup.push_back((int)i);
    return dup;
}

// ---- candidate trees (candidateset.cpp:76-99, 158-222, 275-302): a multimap score -> tree, the best last; a topology is
//      held once.  The topology string is the caller's (PhyloTree::sortedTaxonIdString). --------------------------------
struct CandidateTree {
    std::string tree, topology;
    double score = 0.0;
};

class CandidateSet {
public:
    int maxCandidates = 1000;
    // true: a new topology.  A known topology is replaced only by a better score; a new one is ALWAYS inserted, and the
    // worst tree leaves only when the set is full and the new tree beats it (so, as in the reference, a full set grows by
    // a tree that is worse than all it holds)
    bool update(const std::string &tree, const std::string &topology, double score) {
        CandidateTree c;
        c.tree = tree;
        c.topology = topology;
        c.score = score;
        auto known = topologies.find(topology);
        if (known != topologies.end()) {
            if (known->second < score) {
                removeTopology(topology);
                topologies[topology] = score;
                insert(c);
            }
            return false;
        }
        if (!trees.empty() && trees.front().score < score && (int)trees.size() >= maxCandidates) {
            topologies.erase(trees.front().topology);
            trees.erase(trees.begin());
        }
        insert(c);
        topologies[topology] = score;
        return true;
    }
    size_t size() const { return trees.size(); }
    bool empty() const { return trees.empty(); }
    double getBestScore() const { return trees.empty() ? -1.7976931348623157e308 : trees.back().score; }
    double getWorstScore() const { return trees.front().score; }
    bool treeTopologyExist(const std::string &topology) const { return topologies.count(topology) != 0; }
    double getTopologyScore(const std::string &topology) const { return topologies.at(topology); }
    // rank 0 = the best tree (reverse iteration of the multimap: among equal scores the one inserted last comes first)
    const CandidateTree &byRank(size_t rank) const { return trees[trees.size() - 1 - rank]; }
    // getRandCandTree: a uniform draw among the best min(popSize, size) trees; r = a searchRand value
    size_t randCandRank(int popSize, uint64_t r) const {
        return (size_t)searchRandInt(r, std::min(popSize, (int)trees.size()));
    }
    const std::string &getRandCandTree(int popSize, uint64_t r) const { return byRank(randCandRank(popSize, r)).tree; }
    std::vector<std::string> getTopTrees(int numTree = 0) const {
        if (numTree == 0) numTree = maxCandidates;
        std::vector<std::string> res;
        for (size_t k = 0; k < trees.size() && (int)k < numTree; k++) res.push_back(byRank(k).tree);
        return res;
    }

private:
    std::vector<CandidateTree> trees;            // ascending score; equal scores in insertion order
    std::map<std::string, double> topologies;
    void insert(const CandidateTree &c) {
        auto at = std::upper_bound(trees.begin(), trees.end(), c.score,
                                   [](double s, const CandidateTree &t) { return s < t.score; });
        trees.insert(at, c);
    }
    void removeTopology(const std::string &topology) {
        for (size_t k = trees.size(); k-- > 0;)
            if (trees[k].topology == topology) {
                trees.erase(trees.begin() + (long)k);
                topologies.erase(topology);
                return;
            }
    }
};

// ---- stop rule (stoprule.cpp:104-122) --------------------------------------------------------------------------------------
enum StopCondition { SC_FIXED_ITERATION = 0, SC_UNSUCCESS_ITERATION = 1, SC_BOOTSTRAP_CORRELATION = 2 };

struct StopRule {
    StopCondition stop_condition = SC_UNSUCCESS_ITERATION;
    int min_iteration = 0;           // -n
    int unsuccess_iteration = 100;   // -numstop
    double min_correlation = 0.99;   // -bcor
    int max_iteration = 1000;        // -nm
    int cur_iteration = 0;
    int last_improved_iteration = 0;
    void addImprovedIteration(int it) { last_improved_iteration = it; }
    bool meetStopCondition(int cur_it, double cur_correlation) const {
        switch (stop_condition) {
            case SC_FIXED_ITERATION:
                return cur_it > min_iteration;
            case SC_UNSUCCESS_ITERATION:
                return cur_it >= last_improved_iteration + unsuccess_iteration;
            case SC_BOOTSTRAP_CORRELATION:
                return (cur_correlation >= min_correlation && cur_it >= last_improved_iteration + unsuccess_iteration) ||
                       cur_it > max_iteration;
        }
        return false;
    }
};

// ---- computeBootstrapCorrelation (iqtree.cpp:3018-3057) over computeCorrelation (:2970-3016): the split weights of the
//      snapshot at index (n - 1) / 2 against those of the last one; a split that one side lacks counts as 0 there.  Only
//      non-trivial splits are counted (SplitCounts holds no others).  0 with fewer than two snapshots. --------------------
inline double correlation(const std::vector<double> &ix, const std::vector<double> &iy) {
    const size_t n = ix.size();
    if (n == 0) return 1.0;
    double mx = 0.0, my = 0.0;
    for (size_t i = 0; i < n; i++) { mx += ix[i]; my += iy[i]; }
    mx /= (double)n;
    my /= (double)n;
    if (mx == 0.0 || my == 0.0) return 1.0;
    double f1 = 0.0, f2 = 0.0, f3 = 0.0;
    for (size_t i = 0; i < n; i++) {
        const double x = ix[i] / mx - 1.0, y = iy[i] / my - 1.0;
        f1 += x * y;
        f2 += x * x;
        f3 += y * y;
    }
    if (f2 == 0.0 || f3 == 0.0) return 1.0;
    return f1 / (sqrt(f2) * sqrt(f3));
}

inline double bootstrapCorrelation(const ufboot::SplitCounts &half, const ufboot::SplitCounts &now) {
    std::vector<double> a, b;
    for (size_t k = 0; k < half.splits.size(); k++) {
        a.push_back((double)half.weight[k]);
        b.push_back((double)now.count(half.splits[k]));
    }
    for (size_t k = 0; k < now.splits.size(); k++)
        if (half.index.find(now.splits[k]) == half.index.end()) {
            a.push_back(0.0);
            b.push_back((double)now.weight[k]);
        }
    return correlation(a, b);
}

inline double bootstrapCorrelation(const std::vector<ufboot::SplitCounts> &snapshots) {
    if (snapshots.size() < 2) return 0.0;
    return bootstrapCorrelation(snapshots[(snapshots.size() - 1) / 2], snapshots.back());
}

}  // namespace iqsearch
