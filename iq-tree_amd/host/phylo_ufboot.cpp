// phylo_ufboot.cpp -- bootstrap samples, RELL and the ultrafast bootstrap bookkeeping (see phylo_host.h)
#include "phylo_host.h"
#include "ufboot_splits.h"

#include <float.h>
#include <string.h>

#include <algorithm>

namespace iqhost {

void PhyloTree::setBootSamples(const float *samples, int nsamples) {
    needEngine("setBootSamples");
    pushInputs();
    check(iqhip_set_boot_samples(engine, samples, nsamples), "iqhip_set_boot_samples");
    num_boot_samples = nsamples;
}

void PhyloTree::genBootSamples(int nsamples, int64_t ndraws, uint64_t seed, uint32_t stream, int64_t first_replicate) {
    needEngine("genBootSamples");
    pushInputs();
    check(iqhip_gen_boot_samples(engine, nsamples, first_replicate, ndraws, seed, stream), "iqhip_gen_boot_samples");
    num_boot_samples = nsamples;
}

void PhyloTree::computeRELL(std::vector<double> &rell) {
    needEngine("computeRELL");
    if (!current_it) throw std::runtime_error("computeRELL before computeLikelihood");
    rell.assign((size_t)num_boot_samples, 0.0);
    if (allreduce_hook) {  // pattern shards: partial dot products are summed over the ranks
        check(iqhip_rell_async(engine, branchEnd(current_it), branchEnd(current_it_back)), "iqhip_rell_async");
        allreduce_hook(iqhip_result_device_ptr(engine), num_boot_samples, allreduce_ctx);
        check(iqhip_result_read(engine, rell.data(), num_boot_samples), "iqhip_result_read");
    } else
        check(iqhip_rell(engine, branchEnd(current_it), branchEnd(current_it_back), rell.data()), "iqhip_rell");
}

// ---- ultrafast bootstrap bookkeeping, iqtree.cpp:2676-2801 (saveCurrentTree / saveNNITrees), 2803-2880 (summarizeBootstrap)
double PhyloTree::ufbootRand(uint64_t seed, int64_t tree_id) {
    // include/iqhip.h, iqhip_gen_boot_samples: z = mix(mix(mix(seed + G (stream + 1)) + G (rho + 1)) + G (j + 1))
    const uint64_t G = 0x9E3779B97F4A7C15ull;
    auto mix = [](uint64_t z) {
        z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
        z ^= z >> 27; z *= 0x94D049BB133111EBull;
        z ^= z >> 31;
        return z;
    };
    const uint64_t z = mix(mix(mix(seed + G * (0xBBull + 1)) + G * ((uint64_t)tree_id + 1)) + G * 1);
    return (double)(z >> 11) * 0x1.0p-53;
}

void PhyloTree::needUFBootDevice(const char *who) const {
    if (!nni_backend) needDevice(who);
}

void PhyloTree::initUFBoot(int nsamples, uint64_t seed) {
    needUFBootDevice("initUFBoot");
    noCallerCollective("initUFBoot");
    if (nni_backend) nni_backend->ufbootInit(nsamples);
    else {
        pushInputs();
        check(iqhip_ufboot_init(engine, nsamples), "iqhip_ufboot_init");
    }
    ufboot_nsamples = nsamples;
    ufboot_seed = seed;
    ufboot_next_id = 0;
    ufboot_logl_cutoff = 0.0;
    ufboot_min_orig_logl = DBL_MAX;
    ufboot_counts[0] = ufboot_counts[1] = ufboot_counts[2] = 0;
    ufboot_trees.clear();
}

void PhyloTree::ufbootNextIteration() {
    if (ufboot_min_orig_logl != DBL_MAX) ufboot_logl_cutoff = ufboot_min_orig_logl;
}

namespace {
// (smallest taxon id, string) of the subtree at `node` seen from `dad` in an adjacency list; children by smallest taxon id
std::pair<int, std::string> sortedSubtree(const std::vector<std::vector<int>> &adj, int node, int dad) {
    if (adj[node].size() <= 1 && dad >= 0) return {node, std::to_string(node)};
    std::vector<std::pair<int, std::string>> kids;
    for (int c : adj[node])
        if (c != dad) kids.push_back(sortedSubtree(adj, c, node));
    std::sort(kids.begin(), kids.end(), [](const std::pair<int, std::string> &a, const std::pair<int, std::string> &b) { return a.first < b.first; });
    std::string s = "(";
    for (size_t k = 0; k < kids.size(); k++) s += (k ? "," : "") + kids[k].second;
    return {kids.empty() ? node : kids[0].first, s + ")"};
}
}  // namespace

std::string PhyloTree::sortedTaxonIdString(const NNIMove *mv) const {
    if (!root || root->neighbors.empty()) return ";";
    std::vector<std::vector<int>> adj = adjacency();
    if (mv) {   // the subtree at node1_nei goes to node2, the one at node2_nei to node1
        auto swap_in = [&](int at, int from, int to) {
            for (int &x : adj[(size_t)at])
                if (x == from) { x = to; return; }
            throw std::runtime_error("sortedTaxonIdString: the move does not belong to this tree");
        };
        swap_in(mv->node1, mv->node1_nei, mv->node2_nei);
        swap_in(mv->node2, mv->node2_nei, mv->node1_nei);
        swap_in(mv->node1_nei, mv->node1, mv->node2);
        swap_in(mv->node2_nei, mv->node2, mv->node1);
    }
    // MTree::printTree: from the root leaf's neighbour, the root leaf among its children
    return sortedSubtree(adj, root->neighbors[0]->node->id, -1).second + ";";
}

// keeps id -> Newick for the ids of boot_tree only
static void ufbootKeepReferred(std::vector<std::pair<int64_t, std::string>> &trees, const std::vector<int64_t> &boot_tree) {
    std::vector<int64_t> ids(boot_tree);
    std::sort(ids.begin(), ids.end());
    ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
    std::vector<std::pair<int64_t, std::string>> kept;
    for (auto &t : trees)
        if (std::binary_search(ids.begin(), ids.end(), t.first)) kept.push_back(std::move(t));
    trees.swap(kept);
}

// one update over ent (row and logl set): assigns ids and tie draws; false: no replicate took one, else boot_tree = the winners
bool PhyloTree::ufbootFeed(std::vector<iqhip_ufboot_tree> &ent, std::vector<int64_t> &boot_tree) {
    for (iqhip_ufboot_tree &t : ent) {
        t.tree_id = ufboot_next_id++;
        t.rand = ufbootRand(ufboot_seed, t.tree_id);
    }
    if (nni_backend)
        nni_backend->ufbootUpdate(ent.data(), (int)ent.size(), ufboot_epsilon, ufboot_logl_cutoff, ufboot_counts, &ufboot_min_orig_logl);
    else
        check(iqhip_ufboot_update(engine, ent.data(), (int)ent.size(), ufboot_epsilon, ufboot_logl_cutoff, ufboot_counts, &ufboot_min_orig_logl),
              "iqhip_ufboot_update");
    if (ufboot_counts[2] == 0) return false;
    boot_tree.resize((size_t)ufboot_nsamples);
    if (nni_backend) nni_backend->ufbootFetchTrees(boot_tree.data());
    else check(iqhip_ufboot_fetch(engine, nullptr, nullptr, nullptr, boot_tree.data()), "iqhip_ufboot_fetch");
    return true;
}

void PhyloTree::saveCurrentTree(double logl) {
    needUFBootDevice("saveCurrentTree");
    if (ufboot_nsamples < 1) throw std::runtime_error("saveCurrentTree before initUFBoot");
    if (nni_backend) {
        nni_backend->ufbootReserveRows(1);
        nni_backend->ufbootPutCurrentRow(0);
    } else {
        if (!current_it) throw std::runtime_error("saveCurrentTree before computeLikelihood");
        check(iqhip_ptnlh_reserve(engine, 1), "iqhip_ptnlh_reserve");
        check(iqhip_ptnlh_put_current(engine, 0, branchEnd(current_it), branchEnd(current_it_back)), "iqhip_ptnlh_put_current");
    }
    std::vector<iqhip_ufboot_tree> ent(1);   // (row 0)
    ent[0].logl = logl;
    std::vector<int64_t> boot_tree;
    if (!ufbootFeed(ent, boot_tree)) return;
    ufboot_trees.push_back({ent[0].tree_id, sortedTaxonIdString()});
    ufbootKeepReferred(ufboot_trees, boot_tree);
}

void PhyloTree::saveNNITrees() {
    needUFBootDevice("saveNNITrees");
    if (ufboot_nsamples < 1) throw std::runtime_error("saveNNITrees before initUFBoot");
    if (lh_mem_save != LM_ALL_BRANCH) throw std::runtime_error("saveNNITrees needs LM_ALL_BRANCH");
    std::vector<PhyloNode *> n1, n2;
    internalBranches(n1, n2);
    const size_t nc = 2 * n1.size();
    if (nc == 0) return;
    if (nni_backend) nni_backend->ufbootReserveRows((int)(1 + nc));
    else check(iqhip_ptnlh_reserve(engine, (int)(1 + nc)), "iqhip_ptnlh_reserve");
    std::vector<int> rows(nc);
    for (size_t k = 0; k < nc; k++) rows[k] = (int)(1 + k);
    std::vector<NNIMove> moves;
    evaluateNNIs5Batch(moves, rows.data());
    for (size_t k = 0; k < nc; k++)
        if (moves[k].ptnlh_row != rows[k]) throw std::runtime_error("saveNNITrees: NNI moves out of order");
    saveNNITrees(moves);
}

void PhyloTree::saveNNITrees(const std::vector<NNIMove> &moves) {
    needUFBootDevice("saveNNITrees");
    if (ufboot_nsamples < 1) throw std::runtime_error("saveNNITrees before initUFBoot");
    const size_t nc = moves.size();
    if (nc == 0) return;
    std::vector<iqhip_ufboot_tree> ent(nc);
    const int64_t first_id = ufboot_next_id;
    for (size_t k = 0; k < nc; k++) {
        if (moves[k].ptnlh_row < 0) throw std::runtime_error("saveNNITrees: a move was evaluated without a store row");
        ent[k].row = moves[k].ptnlh_row;
        ent[k].logl = moves[k].newloglh;
    }
    std::vector<int64_t> boot_tree;
    if (!ufbootFeed(ent, boot_tree)) return;
    std::vector<char> taken(nc, 0);
    for (int64_t id : boot_tree)
        if (id >= first_id) taken[(size_t)(id - first_id)] = 1;
    for (size_t k = 0; k < nc; k++)
        if (taken[k]) ufboot_trees.push_back({first_id + (int64_t)k, sortedTaxonIdString(&moves[k])});
    ufbootKeepReferred(ufboot_trees, boot_tree);
}

// the winner of every replicate (out.boot_trees, out.distinct_trees) and the split counts of the winners
void PhyloTree::ufbootWinners(UFBootSummary &out, ufboot::SplitCounts &sc) {
    needUFBootDevice("summarizeBootstrap");
    if (ufboot_nsamples < 1) throw std::runtime_error("summarizeBootstrap before initUFBoot");
    const size_t S = (size_t)ufboot_nsamples;
    std::vector<int64_t> boot_tree(S);
    if (nni_backend) nni_backend->ufbootFetchTrees(boot_tree.data());
    else check(iqhip_ufboot_fetch(engine, nullptr, nullptr, nullptr, boot_tree.data()), "iqhip_ufboot_fetch");
    out = UFBootSummary();
    sc = ufboot::SplitCounts(leafNum);
    out.boot_trees.resize(S);
    // trees.convertSplits(taxname, sg, hash_ss, SW_COUNT, ...): every winner once, weighted by its replicates, in the order
    // the replicates first name it
    std::vector<int64_t> order;
    std::vector<int64_t> weight;
    std::vector<const std::string *> text;
    for (size_t s = 0; s < S; s++) {
        const int64_t id = boot_tree[s];
        const auto at = std::lower_bound(ufboot_trees.begin(), ufboot_trees.end(), id,
                                         [](const std::pair<int64_t, std::string> &t, int64_t v) { return t.first < v; });
        if (at == ufboot_trees.end() || at->first != id) throw std::runtime_error("summarizeBootstrap: a replicate holds no tree");
        out.boot_trees[s] = at->second;
        size_t k = 0;
        while (k < order.size() && order[k] != id) k++;
        if (k == order.size()) {
            order.push_back(id);
            weight.push_back(0);
            text.push_back(&at->second);
        }
        weight[k]++;
    }
    out.distinct_trees = (int)order.size();
    std::vector<ufboot::Split> splits;
    for (size_t k = 0; k < order.size(); k++) {
        ufboot::newickSplits(*text[k], leafNum, splits);
        sc.addTree(splits, weight[k]);
    }
}

void PhyloTree::ufbootSplitCounts(ufboot::SplitCounts &sc) {
    UFBootSummary winners;
    ufbootWinners(winners, sc);
}

void PhyloTree::summarizeBootstrap(UFBootSummary &out) {
    ufboot::SplitCounts sc(leafNum);
    ufbootWinners(out, sc);
    const size_t S = (size_t)ufboot_nsamples;
    // createBootstrapSupport: the split of every internal branch of the current tree
    std::vector<PhyloNode *> n1, n2;
    internalBranches(n1, n2);
    std::vector<std::string> label(nodes.size());
    std::vector<std::vector<int>> below(nodes.size());   // taxa below `node` seen from its dad, from the root leaf
    std::vector<std::pair<PhyloNode *, PhyloNode *>> pre;
    pre.push_back({root, nullptr});
    for (size_t k = 0; k < pre.size(); k++)
        for (PhyloNeighbor *nb : pre[k].first->neighbors)
            if (nb->node != pre[k].second) pre.push_back({nb->node, pre[k].first});
    std::vector<int> support_of(nodes.size(), -1);
    std::vector<PhyloNode *> dad_of(nodes.size(), nullptr);
    for (const auto &pr : pre) dad_of[(size_t)pr.first->id] = pr.second;
    for (size_t k = pre.size(); k-- > 0;) {
        PhyloNode *node = pre[k].first, *dad = pre[k].second;
        std::vector<int> &mine = below[(size_t)node->id];
        if (node->isLeaf()) mine.push_back(node->id);
        if (dad) {
            if (!node->isLeaf() && !dad->isLeaf()) {
                ufboot::Split sp(ufboot::splitWords(leafNum), 0);
                for (int t : mine) ufboot::splitSet(sp, t);
                ufboot::splitNormalise(sp, leafNum);
                support_of[(size_t)node->id] = ufboot::splitSupport(sc, sp, (int64_t)S);
                label[(size_t)node->id] = std::to_string(support_of[(size_t)node->id]);
            }
            std::vector<int> &up = below[(size_t)dad->id];
            up.insert(up.end(), mine.begin(), mine.end());
            std::vector<int>().swap(mine);
        }
    }
    for (size_t q = 0; q < n1.size(); q++) {
        out.node1.push_back(n1[q]->id);
        out.node2.push_back(n2[q]->id);
        // the label of an internal branch sits on its node farther from the root
        out.support.push_back(support_of[(size_t)(dad_of[(size_t)n2[q]->id] == n1[q] ? n2[q] : n1[q])->id]);
    }
    out.support_tree = labelledTreeString(label);
    out.consensus_tree = ufboot::consensusTree(sc, leafNames());
}

}  // namespace iqhost
