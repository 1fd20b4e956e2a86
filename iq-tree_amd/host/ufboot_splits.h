// ufboot_splits.h -- what turns UFBoot's per-replicate winners into what the user reads: the splits of a Newick string, the
// weighted split counts of a set of trees (MTreeSet::convertSplits(..., SW_COUNT)), the supports of a tree's branches
// (MExtTree::createBootstrapSupport, mexttree.cpp:416-461) and the greedy consensus tree (computeConsensusTree over
// SplitGraph::findMaxCompatibleSplits, splitgraph.cpp:673-706).  Plain C++: no HIP, no engine, no PhyloTree -- as
// PhyloTree::bionjNewick is pure host code.
//
// A split is a bitset over the taxa with taxon 0 on the CLEAR side (the reference's Split::shouldInvert normal form), so a
// split is also the clade of the tree rooted at taxon 0.  Only non-trivial splits (at least two taxa on either side) are
// kept: the trivial ones occur in every tree.
// DEVIATION from the reference: its std::sort leaves the order of splits of equal weight open; here ties go to the split
// that appeared first (trees in the order they were added -- replicate order --, splits of a tree in the post-order of its
// string).
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <map>
#include <stdexcept>
#include <string>
#include <vector>

namespace ufboot {

typedef std::vector<uint64_t> Split;   // (ntaxa + 63) / 64 words, bit t = taxon t

inline size_t splitWords(int ntaxa) { return ((size_t)ntaxa + 63) / 64; }
inline bool splitHas(const Split &s, int t) { return (s[(size_t)t >> 6] >> (t & 63)) & 1; }
inline void splitSet(Split &s, int t) { s[(size_t)t >> 6] |= (uint64_t)1 << (t & 63); }
inline int splitCount(const Split &s) {
    int n = 0;
    for (uint64_t w : s) n += __builtin_popcountll(w);
    return n;
}
// taxon 0 to the clear side
inline void splitNormalise(Split &s, int ntaxa) {
    if (!splitHas(s, 0)) return;
    for (uint64_t &w : s) w = ~w;
    if (ntaxa & 63) s.back() &= ((uint64_t)1 << (ntaxa & 63)) - 1;
}
inline bool splitTrivial(const Split &s, int ntaxa) {
    const int c = splitCount(s);
    return c < 2 || c > ntaxa - 2;
}
// two normalised splits (both clades of the tree rooted at taxon 0) fit one tree: disjoint or nested (Split::compatible)
inline bool splitCompatible(const Split &a, const Split &b) {
    bool meet = false, a_only = false, b_only = false;
    for (size_t w = 0; w < a.size(); w++) {
        meet = meet || (a[w] & b[w]);
        a_only = a_only || (a[w] & ~b[w]);
        b_only = b_only || (b[w] & ~a[w]);
    }
    return !meet || !a_only || !b_only;
}

// The non-trivial splits of a Newick string in the post-order of the string.  Leaf labels are looked up in `names`
// (taxon = index) or, when names is empty, read as integer taxon ids; branch lengths, internal labels and [comments] are
// skipped.  Every taxon 0 .. ntaxa-1 must occur exactly once.  Throws std::runtime_error on anything else.
inline void newickSplits(const std::string &nwk, int ntaxa, std::vector<Split> &out,
                         const std::vector<std::string> &names = std::vector<std::string>()) {
    if (ntaxa < 1) throw std::runtime_error("newickSplits: no taxa");
    out.clear();
    const size_t W = splitWords(ntaxa);
    std::map<std::string, int> by_name;
    for (size_t i = 0; i < names.size(); i++) by_name[names[i]] = (int)i;
    std::vector<Split> stack;        // the open groups' taxon sets
    Split seen(W, 0);
    size_t i = 0;
    const size_t n = nwk.size();
    bool closed = false;
    auto skip_tail = [&]() {   // label / length / comment behind a ')' or a leaf
        while (i < n && nwk[i] != ',' && nwk[i] != ')' && nwk[i] != '(' && nwk[i] != ';') {
            if (nwk[i] == '[') {
                while (i < n && nwk[i] != ']') i++;
                if (i == n) throw std::runtime_error("newickSplits: unterminated comment");
            }
            i++;
        }
    };
    while (i < n) {
        const char c = nwk[i];
        if (c == ' ' || c == '\t' || c == '\n' || c == '\r' || c == ',') {
            i++;
        } else if (c == '(') {
            if (closed) throw std::runtime_error("newickSplits: text behind the tree");
            stack.push_back(Split(W, 0));
            i++;
        } else if (c == ')') {
            if (stack.empty()) throw std::runtime_error("newickSplits: unbalanced ')'");
            Split grp = stack.back();
            stack.pop_back();
            i++;
            skip_tail();
            if (stack.empty()) {
                closed = true;
            } else {
                for (size_t w = 0; w < W; w++) stack.back()[w] |= grp[w];
                splitNormalise(grp, ntaxa);
                if (!splitTrivial(grp, ntaxa) && std::find(out.begin(), out.end(), grp) == out.end()) out.push_back(grp);
            }
        } else if (c == ';') {
            break;
        } else {
            if (stack.empty()) throw std::runtime_error("newickSplits: a label outside the tree");
            size_t j = i;
            while (j < n && nwk[j] != ':' && nwk[j] != ',' && nwk[j] != ')' && nwk[j] != '(' && nwk[j] != ';' && nwk[j] != '[' &&
                   nwk[j] != ' ')
                j++;
            const std::string label = nwk.substr(i, j - i);
            int t = -1;
            if (!names.empty()) {
                const auto at = by_name.find(label);
                if (at != by_name.end()) t = at->second;
            } else if (!label.empty() && label.size() < 10 && label.find_first_not_of("0123456789") == std::string::npos) {
                t = atoi(label.c_str());
            }
            if (t < 0 || t >= ntaxa) throw std::runtime_error("newickSplits: unknown taxon '" + label + "'");
            if (splitHas(seen, t)) throw std::runtime_error("newickSplits: taxon '" + label + "' occurs twice");
            splitSet(seen, t);
            splitSet(stack.back(), t);
            i = j;
            skip_tail();
        }
    }
    if (!closed || !stack.empty()) throw std::runtime_error("newickSplits: unbalanced '('");
    if (splitCount(seen) != ntaxa) throw std::runtime_error("newickSplits: a taxon is missing");
}

// MTreeSet::convertSplits(..., SW_COUNT): every distinct split with the summed weight of the trees that contain it, in
// first-appearance order
struct SplitCounts {
    int ntaxa = 0;
    std::vector<Split> splits;
    std::vector<int64_t> weight;
    std::map<Split, size_t> index;
    int64_t total = 0;   // sum of the tree weights
    explicit SplitCounts(int ntaxa_) : ntaxa(ntaxa_) {}
    void addTree(const std::vector<Split> &tree_splits, int64_t tree_weight = 1) {
        total += tree_weight;
        for (const Split &s : tree_splits) {
            const auto at = index.emplace(s, splits.size());
            if (at.second) {
                splits.push_back(s);
                weight.push_back(0);
            }
            weight[at.first->second] += tree_weight;
        }
    }
    int64_t count(const Split &s) const {
        const auto at = index.find(s);
        return at == index.end() ? 0 : weight[at->second];
    }
};

// createBootstrapSupport's number: round(100 count / nsamples), 0 for a split that does not occur
inline int splitSupport(const SplitCounts &sc, const Split &s, int64_t nsamples) {
    if (nsamples < 1) return 0;
    return (int)std::lround(100.0 * (double)sc.count(s) / (double)nsamples);
}

// findMaxCompatibleSplits: the splits in descending weight (ties: first appearance), each taken when it is compatible with
// all taken so far; at most ntaxa - 3 non-trivial splits fit a tree (the reference's 2n-3 counts the trivial ones too)
inline std::vector<size_t> maxCompatibleSplits(const SplitCounts &sc) {
    std::vector<size_t> order(sc.splits.size());
    for (size_t k = 0; k < order.size(); k++) order[k] = k;
    std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return sc.weight[a] > sc.weight[b]; });
    std::vector<size_t> taken;
    for (size_t k : order) {
        if ((int)taken.size() >= sc.ntaxa - 3) break;
        bool ok = true;
        for (size_t t : taken) ok = ok && splitCompatible(sc.splits[t], sc.splits[k]);
        if (ok) taken.push_back(k);
    }
    return taken;
}

// The tree of a compatible split set as a Newick string rooted at taxon 0's node: every split is a clade, labelled
// label[k]; children in ascending order of their smallest taxon; names empty: taxon ids
inline std::string splitsNewick(int ntaxa, const std::vector<Split> &splits, const std::vector<std::string> &label,
                                const std::vector<std::string> &names = std::vector<std::string>()) {
    const size_t m = splits.size();
    for (size_t a = 0; a < m; a++)
        for (size_t b = a + 1; b < m; b++)
            if (!splitCompatible(splits[a], splits[b]) || splits[a] == splits[b])
                throw std::runtime_error("splitsNewick: the splits do not fit one tree");
    // parent of a clade / a taxon: the smallest clade that contains it (m: the root)
    std::vector<int> size(m);
    for (size_t k = 0; k < m; k++) size[k] = splitCount(splits[k]);
    auto smallest_containing = [&](const Split &s, size_t self) {
        size_t best = m;
        for (size_t k = 0; k < m; k++) {
            if (k == self) continue;
            bool inside = true;
            for (size_t w = 0; w < s.size(); w++) inside = inside && !(s[w] & ~splits[k][w]);
            if (inside && (best == m || size[k] < size[best])) best = k;
        }
        return best;
    };
    struct Child { int min_taxon; int clade; };   // clade < 0: the taxon itself
    std::vector<std::vector<Child>> kids(m + 1);
    const size_t W = splitWords(ntaxa);
    for (int t = 0; t < ntaxa; t++) {
        Split one(W, 0);
        splitSet(one, t);
        kids[smallest_containing(one, m)].push_back(Child{t, -1});
    }
    for (size_t k = 0; k < m; k++) {
        int mt = 0;
        while (!splitHas(splits[k], mt)) mt++;
        kids[smallest_containing(splits[k], k)].push_back(Child{mt, (int)k});
    }
    std::string out;
    // (recursion depth <= ntaxa; an explicit stack of (node, next child) keeps it off the call stack)
    struct Frame { size_t node; size_t next; };
    std::vector<Frame> st;
    for (auto &v : kids) std::sort(v.begin(), v.end(), [](const Child &a, const Child &b) { return a.min_taxon < b.min_taxon; });
    st.push_back(Frame{m, 0});
    out += "(";
    while (!st.empty()) {
        Frame &f = st.back();
        if (f.next == kids[f.node].size()) {
            out += ")";
            if (f.node < m && f.node < label.size()) out += label[f.node];
            st.pop_back();
            continue;
        }
        if (f.next > 0) out += ",";
        const Child c = kids[f.node][f.next++];
        if (c.clade < 0) {
            out += names.empty() ? std::to_string(c.min_taxon) : names[(size_t)c.min_taxon];
        } else {
            out += "(";
            st.push_back(Frame{(size_t)c.clade, 0});
        }
    }
    out += ";";
    return out;
}

// computeConsensusTree: the greedy consensus of the counted trees with round(100 weight / total) as labels
inline std::string consensusTree(const SplitCounts &sc, const std::vector<std::string> &names = std::vector<std::string>()) {
    const std::vector<size_t> taken = maxCompatibleSplits(sc);
    std::vector<Split> splits;
    std::vector<std::string> label;
    for (size_t k : taken) {
        splits.push_back(sc.splits[k]);
        label.push_back(std::to_string(splitSupport(sc, sc.splits[k], sc.total)));
    }
    return splitsNewick(sc.ntaxa, splits, label, names);
}

}  // namespace ufboot
