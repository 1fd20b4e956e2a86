// phylo_support.cpp -- SH-aLRT / local bootstrap supports and the tree topology tests (see phylo_host.h)
#include "phylo_host.h"

#include <algorithm>
#include <sstream>

namespace iqhost {

// ---- SH-aLRT / local bootstrap, phylotree.cpp:3984-4103
double PhyloTree::testAllBranches(int reps, int lbp_reps, std::vector<BranchSupport> &out, bool batched) {
    needDevice("testAllBranches");
    noCallerCollective("testAllBranches");
    if (reps < 0 || lbp_reps < 0 || std::max(reps, lbp_reps) < 1) throw std::runtime_error("testAllBranches: no replicates");
    if (std::max(reps, lbp_reps) > num_boot_samples) throw std::runtime_error("testAllBranches: more replicates than setBootSamples uploaded");
    if (batched && lh_mem_save != LM_ALL_BRANCH) throw std::runtime_error("testAllBranches(batched) needs LM_ALL_BRANCH");
    std::vector<PhyloNode *> n1, n2;
    internalBranches(n1, n2);
    const size_t nb = n1.size();
    if (nb == 0) throw std::runtime_error("testAllBranches: the tree has no internal branch");
    const double lh0 = computeLikelihood();
    check(iqhip_ptnlh_reserve(engine, (int)(1 + 2 * nb)), "iqhip_ptnlh_reserve");
    check(iqhip_ptnlh_put_current(engine, 0, branchEnd(current_it), branchEnd(current_it_back)), "iqhip_ptnlh_put_current");
    std::vector<int> rows(2 * nb);
    for (size_t k = 0; k < 2 * nb; k++) rows[k] = (int)(1 + k);
    std::vector<NNIMove> moves;
    if (batched) {
        evaluateNNIs5Batch(moves, rows.data());
    } else {
        moves.resize(2 * nb);
        for (size_t q = 0; q < nb; q++) {
            NNIMove two[2];
            getBestNNIForBran(n1[q], n2[q], true, two, &rows[2 * q]);
            moves[2 * q] = two[0];
            moves[2 * q + 1] = two[1];
        }
    }
    std::vector<int32_t> rows3(3 * nb);
    std::vector<double> lh3(3 * nb);
    for (size_t q = 0; q < nb; q++) {
        rows3[3 * q] = 0;
        lh3[3 * q] = lh0;
        for (int cnt = 0; cnt < 2; cnt++) {
            const NNIMove &m = moves[2 * q + cnt];
            if (m.node1 != n1[q]->id || m.node2 != n2[q]->id || m.ptnlh_row != rows[2 * q + cnt])
                throw std::runtime_error("testAllBranches: NNI moves out of order");
            rows3[3 * q + 1 + cnt] = m.ptnlh_row;
            lh3[3 * q + 1 + cnt] = m.newloglh;
        }
    }
    std::vector<iqhip_branch_support> res(nb);
    check(iqhip_branch_tests(engine, rows3.data(), lh3.data(), (int)nb, reps, lbp_reps, res.data()), "iqhip_branch_tests");
    out.assign(nb, BranchSupport());
    for (size_t q = 0; q < nb; q++) {
        BranchSupport &b = out[q];
        b.node1 = n1[q]->id;
        b.node2 = n2[q]->id;
        for (int k = 0; k < 3; k++) b.lh[k] = lh3[3 * q + k];
        b.sh_alrt = res[q].sh_alrt;
        b.lbp = res[q].lbp;
        b.abayes = res[q].abayes;
        b.alrt_stat = res[q].alrt_stat;
    }
    return lh0;
}

std::string PhyloTree::supportLabel(double sh_alrt, double lbp, bool with_sh, bool with_lbp) {
    std::ostringstream ss;  // phylotree.cpp:4078-4091 (node names are empty here)
    ss.precision(3);
    if (with_sh) ss << sh_alrt * 100;
    if (with_lbp) ss << "/" << lbp * 100;
    return ss.str();
}

static void writeSupportNewick(std::ostringstream &os, const PhyloNode *node, const PhyloNode *dad,
                               const std::vector<std::string> &label) {
    if (node->isLeaf() && dad) {
        if (node->name.empty()) os << node->id;  // leaf labels as read (MTree::printTree writes names)
        else os << node->name;
        return;
    }
    os << "(";
    bool first = true;
    for (PhyloNeighbor *nb : node->neighbors)
        if (nb->node != dad) {
            if (!first) os << ",";
            first = false;
            writeSupportNewick(os, nb->node, node, label);
            os.precision(17);
            os << ":" << nb->length;
        }
    os << ")" << label[node->id];
}

std::string PhyloTree::supportTreeString(const std::vector<BranchSupport> &sup, bool with_sh, bool with_lbp) const {
    // testAllBranches walks from the root leaf and names `node` of every internal (node, dad): the far end of the branch,
    // which is also where a Newick string printed from the root's neighbour puts the label of that branch
    if (!root) return ";";
    std::vector<std::string> label(nodes.size());
    std::vector<std::pair<PhyloNode *, PhyloNode *>> stack;
    stack.push_back({root, nullptr});
    while (!stack.empty()) {
        PhyloNode *node = stack.back().first, *dad = stack.back().second;
        stack.pop_back();
        if (dad && !node->isLeaf() && !dad->isLeaf())
            for (const BranchSupport &b : sup)
                if ((b.node1 == node->id && b.node2 == dad->id) || (b.node2 == node->id && b.node1 == dad->id))
                    label[node->id] = supportLabel(b.sh_alrt, b.lbp, with_sh, with_lbp);
        for (PhyloNeighbor *nb : node->neighbors)
            if (nb->node != dad) stack.push_back({nb->node, node});
    }
    return labelledTreeString(label);
}

std::string PhyloTree::labelledTreeString(const std::vector<std::string> &label) const {
    std::ostringstream os;  // from the internal node next to the root leaf, so that the output is a trifurcation
    writeSupportNewick(os, root->neighbors[0]->node, nullptr, label);
    os << ";";
    return os.str();
}

// ---- tree topology tests, phylotesting.cpp:2053-2442
void PhyloTree::evaluateTrees(const std::vector<std::string> &newicks, bool fixed_lengths, int nsamples, bool weighted,
                              const std::vector<double> &au_scales, uint64_t seed, std::vector<TreeTest> &out,
                              std::vector<double> &au_bp, double epsilon) {
    needDevice("evaluateTrees");
    noCallerCollective("evaluateTrees");
    if (newicks.size() < 2) throw std::runtime_error("evaluateTrees: at least two trees");
    if (nsamples < 1) throw std::runtime_error("evaluateTrees: no replicates");
    const int ntrees = (int)newicks.size();
    const std::vector<std::string> names = leafNames();
    const int leaves = leafNum;
    check(iqhip_ptnlh_reserve(engine, ntrees), "iqhip_ptnlh_reserve");
    out.assign((size_t)ntrees, TreeTest());
    std::vector<int32_t> rows((size_t)ntrees);
    std::vector<double> lh((size_t)ntrees);
    for (int tid = 0; tid < ntrees; tid++) {
        readTreeString(newicks[tid], names);
        if (leafNum != leaves) throw std::runtime_error("evaluateTrees: a tree with another number of taxa");
        initializeAllPartialLh();
        clearAllPartialLH();
        double lnl = computeLikelihood();
        if (!fixed_lengths) {
            optimizeAllBranches();
            clearAllPartialLH();
            lnl = computeLikelihood();
        }
        check(iqhip_ptnlh_put_current(engine, tid, branchEnd(current_it), branchEnd(current_it_back)), "iqhip_ptnlh_put_current");
        rows[tid] = tid;
        lh[tid] = out[tid].logl = lnl;
    }
    genBootSamples(nsamples, (int64_t)getAlnNSite(), seed, 0xA0u);
    std::vector<iqhip_tree_test> res((size_t)ntrees);
    check(iqhip_tree_tests(engine, rows.data(), lh.data(), ntrees, nsamples, epsilon, weighted ? 1 : 0, seed, res.data()),
          "iqhip_tree_tests");
    for (int tid = 0; tid < ntrees; tid++) out[tid].t = res[tid];
    au_bp.clear();
    if (!au_scales.empty()) {
        au_bp.assign(au_scales.size() * (size_t)ntrees, 0.0);
        check(iqhip_multiscale_bp(engine, rows.data(), ntrees, au_scales.data(), (int)au_scales.size(), nsamples, seed,
                                  au_bp.data()),
              "iqhip_multiscale_bp");
    }
}

}  // namespace iqhost
