// supertree_host.cpp -- see supertree_host.h.  Host-side C++; the arithmetic is in libiqhip.so.
#include "supertree_host.h"

#include <math.h>
#include <string.h>

#include <algorithm>
#include <fstream>
#include <sstream>

#include "brent_host.h"
#include "supertree_brlen.h"

namespace iqhost {

std::string partitionSequenceType(const std::string &model) {
    std::string name = parseModelString(model).name;
    for (char &c : name) c = (char)toupper((unsigned char)c);
    static const char *dna[] = {"JC", "JC69", "F81", "K80", "K2P", "HKY", "HKY85", "TN", "TRN", "TN93", "GTR"};
    for (const char *d : dna)
        if (name == d) return "DNA";
    if (name == "GY" || name == "GY94") return "CODON";
    if (name == "JC2" || name == "GTR2") return "BIN";
    return "AA";
}

void readPartitionStrings(const std::string &aln_content, const std::string &part_content, std::vector<std::string> &seq_names,
                          std::vector<PartitionInput> &parts) {
    std::vector<std::string> sequences;
    Alignment::readSequences(aln_content, seq_names, sequences);
    if (sequences.empty()) throw std::runtime_error("empty alignment");
    const std::vector<PartitionSpec> specs = parsePartitionFile(part_content, (int)sequences[0].size());
    parts.clear();
    parts.resize(specs.size());
    for (size_t k = 0; k < specs.size(); k++) {
        PartitionInput &in = parts[k];
        in.name = specs[k].name;
        in.model = specs[k].model;
        const ModelSpec spec = parseModelString(in.model);
        if (!spec.mix_classes.empty()) throw std::runtime_error("partition " + in.name + ": mixture models cannot join a partition model");
        if (spec.ascertainment) throw std::runtime_error("partition " + in.name + ": +ASC cannot join a partition model");
        in.aln.seq_names = seq_names;
        in.aln.buildPattern(extractSites(sequences, specs[k].sites), partitionSequenceType(in.model));
        buildModel(spec, in.aln, in.inputs);
    }
}

void readPartitionRaxml(const std::string &aln_file, const std::string &part_file, std::vector<std::string> &seq_names,
                        std::vector<PartitionInput> &parts) {
    auto slurp = [](const std::string &file, const char *what) {
        std::ifstream in(file.c_str(), std::ios::binary);
        if (!in) throw std::runtime_error(std::string("cannot open ") + what + " " + file);
        std::ostringstream ss;
        ss << in.rdbuf();
        return ss.str();
    };
    readPartitionStrings(slurp(aln_file, "alignment file"), slurp(part_file, "partition file"), seq_names, parts);
}

PhyloSuperTree::PhyloSuperTree() {}

PhyloSuperTree::~PhyloSuperTree() {
    super.nni_backend = nullptr;
    if (group) iqhip_partition_destroy(group);   // before its members
    for (PhyloTree *t : parts) delete t;
}

void PhyloSuperTree::hip(int rc, const char *what) const {
    if (rc != IQHIP_OK) throw std::runtime_error(std::string(what) + ": " + iqhip_last_error());
}

void PhyloSuperTree::needGroup() const {
    if (!group) throw std::runtime_error("PhyloSuperTree: attachEngines first");
}

void PhyloSuperTree::readTreeString(const std::string &newick, const std::vector<std::string> &names) {
    if (parts.empty()) {
        super.readTreeString(newick, names);
        return;
    }
    // a candidate tree of the search: the same taxa on every tree, engines, models and rates kept.  Every tree parses the
    // same string, so node ids and neighbour order agree; all member vectors are dropped and their keys handed out anew,
    // alike on every member
    const int nleaf = super.leafNum;
    super.readTreeString(newick, names);
    if (super.leafNum != nleaf) throw std::runtime_error("PhyloSuperTree: the tree has another number of taxa than the partitions");
    for (PhyloTree *t : parts) {
        t->readTreeString(newick, names);
        t->theta_computed = false;
    }
    pushLengths();
}

PhyloTree *PhyloSuperTree::addPartition(const std::string &name) {
    if (!super.root) throw std::runtime_error("PhyloSuperTree: no tree");
    if (group) throw std::runtime_error("PhyloSuperTree: partitions are added before attachEngines");
    PhyloTree *t = new PhyloTree();
    t->copyTopology(super);
    parts.push_back(t);
    part_name.push_back(name);
    part_rate.push_back(1.0);
    cur_score.push_back(0.0);
    return t;
}

PhyloTree *PhyloSuperTree::addPartition(const PartitionInput &in) {
    if (super.leafNum != in.aln.getNSeq()) throw std::runtime_error("Tree and alignment have different numbers of taxa");
    PhyloTree *t = addPartition(in.name);
    std::vector<uint8_t> states;
    std::vector<double> freq, invar;
    in.aln.statesByLeaf(states);
    in.aln.ptnFreq(freq);
    in.aln.ptnInvar(in.inputs.p_invar, in.inputs.state_freq.data(), invar);
    t->setAlignment(in.aln.num_states, in.aln.seq_type, in.aln.getNPattern(), states.data(), freq.data(), invar.data());
    t->setModel(in.inputs.ncat, in.inputs.eig.eval.data(), in.inputs.eig.evec.data(), in.inputs.eig.inv_evec.data(),
                in.inputs.rates.data(), in.inputs.props.data());
    return t;
}

void PhyloSuperTree::attachEngines(int device) {
    if (parts.empty()) throw std::runtime_error("PhyloSuperTree: no partition");
    if (group) throw std::runtime_error("PhyloSuperTree: engines already attached");
    std::vector<iqhip_engine *> members;
    for (PhyloTree *t : parts) {
        t->min_branch_length = min_branch_length;
        t->max_branch_length = max_branch_length;
        t->setLikelihoodKernel(LK_EIGEN_HIP);
        if (!t->engine) t->attachEngine(device);
        members.push_back(t->engine);
    }
    hip(iqhip_partition_create(&group, members.data(), (int)members.size()), "iqhip_partition_create");
    hip(iqhip_partition_set_rates(group, part_rate.data()), "iqhip_partition_set_rates");
    pushLengths();
    super.nni_backend = this;   // from here on the NNI scaffold run on `super` goes to the group
    super.min_branch_length = min_branch_length;
    super.max_branch_length = max_branch_length;
}

double PhyloSuperTree::totalNSite() const {
    double n = 0.0;
    for (const PhyloTree *t : parts) n += t->getAlnNSite();
    return n;
}

void PhyloSuperTree::pushLengths() {
    for (size_t p = 0; p < parts.size(); p++) {
        PhyloTree *t = parts[p];
        const double r = part_rate[p];
        for (size_t i = 0; i < super.nodes.size(); i++) {
            const std::vector<PhyloNeighbor *> &src = super.nodes[i]->neighbors, &dst = t->nodes[i]->neighbors;
            for (size_t k = 0; k < src.size(); k++) dst[k]->length = r * src[k]->length;
        }
        t->theta_computed = false;
        t->clearAllPartialLH();
    }
}

void PhyloSuperTree::setRates(const double *rates) {
    for (size_t p = 0; p < parts.size(); p++)
        if (!(rates[p] > 0.0) || !std::isfinite(rates[p])) throw std::runtime_error("PhyloSuperTree: a rate must be finite and > 0");
    part_rate.assign(rates, rates + parts.size());
    if (group) {
        hip(iqhip_partition_set_rates(group, part_rate.data()), "iqhip_partition_set_rates");
        pushLengths();
    }
}

double PhyloSuperTree::sumScores() const {
    double s = 0.0;
    for (double v : cur_score) s += v;
    return s;
}

double PhyloSuperTree::computeLikelihood() {
    needGroup();
    for (size_t p = 0; p < parts.size(); p++) cur_score[p] = parts[p]->computeLikelihood();
    return sumScores();
}

void PhyloSuperTree::prepareBranch(int a, int b) {
    if (a < 0 || b < 0 || a >= super.nodeNum || b >= super.nodeNum || !super.nodes[a]->findNeighbor(super.nodes[b]))
        throw std::runtime_error("PhyloSuperTree: nodes are not adjacent");
    super.current_it = super.nodes[a]->findNeighbor(super.nodes[b]);
    super.current_it_back = super.nodes[b]->findNeighbor(super.nodes[a]);
    for (PhyloTree *t : parts) {
        t->current_it = t->nodes[a]->findNeighbor(t->nodes[b]);
        t->current_it_back = t->nodes[b]->findNeighbor(t->nodes[a]);
        t->theta_computed = false;
        double df, ddf;
        t->computeLikelihoodDerv(t->current_it, t->nodes[a], df, ddf);   // pending partials of both ends + theta
    }
}

void PhyloSuperTree::partitionNewtonBranch(int a, int b, double xguess, double x1, double x2, double xacc, int max_steps,
                                           double *optx, double *d2l, int *nsteps, double *part_lnl) {
    needGroup();
    prepareBranch(a, b);
    num_group_solves++;
    hip(iqhip_partition_newton_branch(group, xguess, x1, x2, xacc, max_steps, optx, d2l, nsteps, part_lnl),
        "iqhip_partition_newton_branch");
}

double PhyloSuperTree::optimizeOneBranch(int a, int b, bool clearLH, int maxNRStep) {
    needGroup();
    prepareBranch(a, b);
    const double current_len = super.current_it->length;
    double optx = current_len, d2l = 0.0;
    int nsteps = 0;
    std::vector<double> lnl(parts.size(), 0.0);
    num_group_solves++;
    hip(iqhip_partition_newton_branch(group, current_len, min_branch_length, max_branch_length, min_branch_length, maxNRStep,
                                      &optx, &d2l, &nsteps, lnl.data()),
        "iqhip_partition_newton_branch");
    for (PhyloTree *t : parts) t->num_derv_calls += nsteps;
    if (optx > max_branch_length * 0.95) {  // newton raphson diverged, reset (phylotree.cpp:2167-2176), on the summed lnL
        num_diverged++;
        std::vector<double> orig(parts.size(), 0.0);
        hip(iqhip_partition_lnl_from_theta(group, current_len, orig.data()), "iqhip_partition_lnl_from_theta");
        double opt_lh = 0.0, orig_lh = 0.0;
        for (size_t p = 0; p < parts.size(); p++) { opt_lh += lnl[p]; orig_lh += orig[p]; }
        if (orig_lh > opt_lh) {
            optx = current_len;
            lnl = orig;
        }
    }
    cur_score = lnl;   // part_info[part].cur_score = computeLikelihoodFromBuffer() (phylosupertreeplen.cpp:453-458)
    super.current_it->length = super.current_it_back->length = optx;
    for (size_t p = 0; p < parts.size(); p++) {
        PhyloTree *t = parts[p];
        t->current_it->length = t->current_it_back->length = part_rate[p] * optx;
        if (clearLH && current_len != optx) {
            t->nodes[a]->clearReversePartialLh(t->nodes[b]);
            t->nodes[b]->clearReversePartialLh(t->nodes[a]);
        }
    }
    return optx;
}

void PhyloSuperTree::setBranchBounds(double lo, double hi) {
    min_branch_length = lo;
    max_branch_length = hi;
    super.min_branch_length = lo;
    super.max_branch_length = hi;
    for (PhyloTree *t : parts) {
        t->min_branch_length = lo;
        t->max_branch_length = hi;
    }
}

void PhyloSuperTree::branchOrder(std::vector<int> &n1, std::vector<int> &n2) {
    std::vector<PhyloNode *> nodes1, nodes2;
    PhyloNode *farleaf = super.findFarthestLeaf();
    super.findFarthestLeaf(farleaf);
    super.getPreOrderBranches(nodes1, nodes2, farleaf, nullptr);
    n1.clear();
    n2.clear();
    for (size_t j = 0; j < nodes1.size(); j++) {
        n1.push_back(nodes1[j]->id);
        n2.push_back(nodes2[j]->id);
    }
}

double PhyloSuperTree::optimizeAllBranches(int my_iterations, double tolerance, int maxNRStep) {
    needGroup();
    for (double &v : cur_score) v = 0.0;
    std::vector<PhyloNode *> nodes1, nodes2;
    PhyloNode *farleaf = super.findFarthestLeaf();
    super.findFarthestLeaf(farleaf);  // phylotree.cpp:2241-2250
    super.getPreOrderBranches(nodes1, nodes2, farleaf, nullptr);
    {   // computeLikelihoodBranch on the first branch (PhyloSuperTreePlen::computeLikelihoodBranch -> computeFunction)
        const int a = nodes1[0]->id, b = nodes2[0]->id;
        for (size_t p = 0; p < parts.size(); p++) {
            PhyloTree *t = parts[p];
            cur_score[p] = t->computeLikelihoodBranch(t->nodes[a]->findNeighbor(t->nodes[b]), t->nodes[a]);
        }
    }
    double tree_lh = sumScores();
    for (int i = 0; i < my_iterations; i++) {
        std::vector<double> lenvec;
        for (PhyloNeighbor *nb : super.all_neighbors) lenvec.push_back(nb->length);
        for (size_t j = 0; j < nodes1.size(); j++) optimizeOneBranch(nodes1[j]->id, nodes2[j]->id, true, maxNRStep);
        double new_tree_lh = sumScores();   // PhyloSuperTreePlen::computeLikelihoodFromBuffer (:519-528)
        if (new_tree_lh < tree_lh) {  // rare: restore and stop (phylotree.cpp:2303-2319)
            for (size_t k = 0; k < super.all_neighbors.size(); k++) super.all_neighbors[k]->length = lenvec[k];
            pushLengths();
            return computeLikelihood();
        }
        if (tree_lh <= new_tree_lh && new_tree_lh <= tree_lh + tolerance) return new_tree_lh;
        tree_lh = new_tree_lh;
    }
    return tree_lh;
}

double PhyloSuperTree::optimizeGeneRate(double gradient_epsilon) {
    needGroup();
    const size_t P = parts.size();
    // the branch of computeLikelihood() (phylotree.cpp:1031-1072): the farthest leaf's pendant branch
    PhyloNode *leaf = super.findFarthestLeaf();
    const int la = leaf->id, lb = leaf->neighbors[0]->node->id;
    // every member plans the whole tree for that branch; the plans must agree (one op list serves all members)
    std::vector<iqhip_node_op> ops;
    std::vector<int> len_branch;
    iqhip_branch_end ea = {0, -1, 0}, eb = {0, -1, 0};
    int root_branch = -1;
    for (size_t p = 0; p < P; p++) {
        PhyloTree *t = parts[p];
        t->clearAllPartialLH();
        t->theta_computed = false;
        t->current_it = t->nodes[la]->findNeighbor(t->nodes[lb]);
        t->current_it_back = t->nodes[lb]->findNeighbor(t->nodes[la]);
        std::vector<iqhip_node_op> o;
        std::vector<int> lbr;
        iqhip_branch_end a, b;
        int rb;
        t->collectBranchPlan(t->current_it, t->nodes[la], o, lbr, a, b, rb);
        if (p == 0) {
            ops = o; len_branch = lbr; ea = a; eb = b; root_branch = rb;
            continue;
        }
        bool same = o.size() == ops.size() && lbr == len_branch && rb == root_branch && a.key == ea.key && a.leaf == ea.leaf &&
                    b.key == eb.key && b.leaf == eb.leaf;
        for (size_t k = 0; same && k < o.size(); k++)
            same = o[k].dst_key == ops[k].dst_key && o[k].left_key == ops[k].left_key && o[k].right_key == ops[k].right_key &&
                   o[k].left_leaf == ops[k].left_leaf && o[k].right_leaf == ops[k].right_leaf && o[k].flags == ops[k].flags;
        if (!same) throw std::runtime_error("optimizeGeneRate: the members' traversal plans differ (same memory mode and history needed)");
    }
    // ... with the super tree's lengths; member p runs them times its trial scale
    std::vector<double> blen((size_t)super.branchNum + 1, 0.0);
    for (PhyloNeighbor *nb : super.all_neighbors)
        if (nb->id >= 0 && (size_t)nb->id < blen.size()) blen[(size_t)nb->id] = nb->length;
    auto len_of = [&](int id) { return id < 0 ? 0.0 : blen.at((size_t)id); };
    for (size_t k = 0; k < ops.size(); k++) {
        ops[k].left_len = len_of(len_branch[2 * k]);
        ops[k].right_len = len_of(len_branch[2 * k + 1]);
    }
    const double root_len = len_of(root_branch);

    // optimizeTreeLengthScaling(1 / nsite_p, part_rate, nsite / nsite_p, gradient_epsilon) for all p in lockstep
    const double nsites = totalNSite();
    const double tol = std::max(0.001, gradient_epsilon);   // TOL_TREE_LENGTH_SCALE
    std::vector<BrentMachine> bm(P);
    std::vector<double> scale(P), lnl(P);
    for (size_t p = 0; p < P; p++) {
        const double np = parts[p]->getAlnNSite(), r = part_rate[p];
        scale[p] = bm[p].init(std::min(r, 1.0 / np), r, std::max(nsites / np, r), tol);
    }
    gene_rate_rounds = 0;
    for (;;) {
        bool any = false;
        for (size_t p = 0; p < P; p++) any = any || !bm[p].done;
        if (!any) break;
        gene_rate_rounds++;
        num_group_traversals++;
        hip(iqhip_partition_traverse_lnl(group, ops.empty() ? nullptr : ops.data(), (int)ops.size(), ea, eb, root_len,
                                         scale.data(), lnl.data()),
            "iqhip_partition_traverse_lnl");
        for (size_t p = 0; p < P; p++)
            if (!bm[p].done) {
                const double next = bm[p].update(-lnl[p]);
                scale[p] = bm[p].done ? bm[p].optx : next;
            }
    }
    gene_rate_evals.assign(P, 0);
    for (size_t p = 0; p < P; p++) {
        part_rate[p] = bm[p].optx;
        cur_score[p] = -bm[p].fx_opt;   // the lnL at the accepted scale (optimizeTreeLengthScaling returns computeLikelihood())
        gene_rate_evals[p] = bm[p].nevals;
    }
    // now normalize the rates (:238-252)
    double sum = 0.0;
    for (size_t p = 0; p < P; p++) sum += part_rate[p] * parts[p]->getAlnNSite();
    sum /= nsites;
    super.scaleLength(sum);
    sum = 1.0 / sum;
    for (size_t p = 0; p < P; p++) part_rate[p] *= sum;
    hip(iqhip_partition_set_rates(group, part_rate.data()), "iqhip_partition_set_rates");
    pushLengths();   // (the members' vectors belong to the last trial scales: all dropped)
    return sumScores();
}

// ---- NNI on the super tree ------------------------------------------------------------------------------------------------
void PhyloSuperTree::setAllBranchMode() {
    if (group) throw std::runtime_error("PhyloSuperTree: setAllBranchMode comes before attachEngines");
    super.lh_mem_save = LM_ALL_BRANCH;
    for (PhyloTree *t : parts) t->lh_mem_save = LM_ALL_BRANCH;
}

void PhyloSuperTree::doNNI(const NNIMove &move) {
    super.doNNI(move, true);
    for (PhyloTree *t : parts) t->doNNI(move, true);
}

void PhyloSuperTree::changeNNIBrans(const NNIMove &move, bool nni5) {
    super.changeNNIBrans(move, nni5);
    for (size_t p = 0; p < parts.size(); p++) {
        PhyloTree *t = parts[p];
        NNIMove mine = move;
        for (double &l : mine.newLen) l *= part_rate[p];
        t->changeNNIBrans(mine, nni5);
        PhyloNode *node1 = t->nodes[(size_t)move.node1], *node2 = t->nodes[(size_t)move.node2];
        node1->findNeighbor(node2)->clearPartialLh();
        node2->findNeighbor(node1)->clearPartialLh();
        node2->clearReversePartialLh(node1);
        node1->clearReversePartialLh(node2);
        t->theta_computed = false;
    }
}

PhyloSuperTree::NNIMove PhyloSuperTree::doOneRandomNNI(int a, int b, int bit1, int bit2) {
    if (a < 0 || b < 0 || a >= super.nodeNum || b >= super.nodeNum) throw std::runtime_error("doOneRandomNNI: bad node id");
    const NNIMove mv = super.doOneRandomNNI(super.nodes[(size_t)a], super.nodes[(size_t)b], bit1, bit2);
    for (PhyloTree *t : parts) t->doNNI(mv, false);   // (no vector is cleared: the caller recomputes everything)
    return mv;
}

void PhyloSuperTree::restoreBranchLengths(const std::vector<double> &lenvec) {
    super.restoreBranchLengths(lenvec);
    pushLengths();
}

void PhyloSuperTree::clearAllPartialLH() {
    for (PhyloTree *t : parts) {
        t->theta_computed = false;
        t->clearAllPartialLH();
    }
}

PhyloSuperTree::NNIMove PhyloSuperTree::getBestNNIForBran(int a, int b, bool nni5, NNIMove moves[2], const int *ptnlh_rows) {
    needGroup();
    if (a < 0 || b < 0 || a >= super.nodeNum || b >= super.nodeNum) throw std::runtime_error("getBestNNIForBran: bad node id");
    PhyloNode *node1 = super.nodes[(size_t)a], *node2 = super.nodes[(size_t)b];
    if (!node1->findNeighbor(node2) || node1->isLeaf() || node2->isLeaf() || node1->degree() != 3 || node2->degree() != 3)
        throw std::runtime_error("getBestNNIForBran needs an internal branch of a binary tree");
    std::vector<double> saved;
    super.saveBranchLengths(saved);
    const std::vector<double> backup = cur_score;
    auto others = [](PhyloNode *at, PhyloNode *other) {
        std::vector<int> ids;
        for (PhyloNeighbor *nb : at->neighbors)
            if (nb->node != other) ids.push_back(nb->node->id);
        return ids;
    };
    // the two moves: first other neighbour of node1 against each other neighbour of node2 (:2951-2960), named before any swap
    const int first1 = others(node1, node2)[0];
    const std::vector<int> at2 = others(node2, node1);
    for (int cnt = 0; cnt < 2; cnt++) {
        NNIMove &m = moves[cnt] = NNIMove();
        m.node1 = a; m.node2 = b; m.node1_nei = first1; m.node2_nei = at2[(size_t)cnt];
        doNNI(m);
        int i = 1;
        if (nni5)
            for (int x : others(node1, node2)) m.newLen[i++] = optimizeOneBranch(a, x, true, PhyloTree::NNI_MAX_NR_STEP);
        m.newLen[0] = optimizeOneBranch(a, b, true, PhyloTree::NNI_MAX_NR_STEP);
        if (nni5)
            for (int y : others(node2, node1)) m.newLen[i++] = optimizeOneBranch(b, y, true, PhyloTree::NNI_MAX_NR_STEP);
        m.newloglh = sumScores();
        if (ptnlh_rows && ptnlh_rows[cnt] >= 0) {   // computePatternLikelihood(nni.ptnlh), phylosupertreeplen.cpp:1367-1372
            ufbootPutCurrentRow(ptnlh_rows[cnt]);
            m.ptnlh_row = ptnlh_rows[cnt];
        }
        doNNI(m);   // (the same move again restores the tree, neighbour order included; the lengths stay for the second swap)
    }
    restoreBranchLengths(saved);
    cur_score = backup;
    return moves[0].newloglh > moves[1].newloglh ? moves[0] : moves[1];
}

void PhyloSuperTree::pendingVectors(const std::vector<PhyloNode *> &n1, const std::vector<PhyloNode *> &n2, bool all) {
    needGroup();
    uint64_t top = super.next_key;
    for (PhyloTree *t : parts) {
        if (t->lh_mem_save != LM_ALL_BRANCH) throw std::runtime_error("PhyloSuperTree: the batched NNI evaluation needs setAllBranchMode");
        if (all) t->computeAllPartialLh();
        else {
            std::vector<PhyloNode *> m1, m2;
            for (size_t q = 0; q < n1.size(); q++) {
                m1.push_back(t->nodes[(size_t)n1[q]->id]);
                m2.push_back(t->nodes[(size_t)n2[q]->id]);
            }
            t->computePartialLhAround(m1, m2);
        }
        t->pushInputs();
        t->theta_computed = false;
        top = std::max(top, t->next_key);
    }
    // one key space: the super tree's Neighbors name the members' vectors, and no tree hands out a key another one uses
    for (size_t i = 0; i < super.nodes.size(); i++)
        for (size_t k = 0; k < super.nodes[i]->neighbors.size(); k++) {
            const uint64_t key = parts[0]->nodes[i]->neighbors[k]->partial_lh;
            for (PhyloTree *t : parts)
                if (t->nodes[i]->neighbors[k]->partial_lh != key || t->nodes[i]->neighbors[k]->node->id != super.nodes[i]->neighbors[k]->node->id)
                    throw std::runtime_error("PhyloSuperTree: the members' vector keys differ (same memory mode and history needed)");
            super.nodes[i]->neighbors[k]->partial_lh = key;
            super.nodes[i]->neighbors[k]->lh_scale_factor = 0.0;
        }
    super.central_partial_lh = true;
    for (uint64_t k : super.nni_batch_keys) top = std::max(top, k + 1);
    super.next_key = top;
    const uint64_t after = top + 4 * (uint64_t)n1.size();   // (beyond the scratch keys the scaffold may take now)
    for (PhyloTree *t : parts) t->next_key = std::max(t->next_key, after);
}

void PhyloSuperTree::submitTasks(const std::vector<iqhip_branch_task> &tasks, std::vector<iqhip_branch_result> &res,
                                 const int32_t *rows) {
    num_group_batches++;
    hip(iqhip_partition_optimize_branch_batch_rows(group, tasks.data(), (int)tasks.size(), res.data(), nullptr, rows),
        "iqhip_partition_optimize_branch_batch_rows");
    for (const iqhip_branch_result &r : res)
        for (PhyloTree *t : parts) t->num_derv_calls += r.nsteps;
}

void PhyloSuperTree::evaluateNNIsBatch(std::vector<NNIMove> &moves, const BranchList *branches) {
    needGroup();
    super.evaluateNNIsBatch(moves, branches);
}

void PhyloSuperTree::evaluateNNIs5Batch(std::vector<NNIMove> &moves, const int *ptnlh_rows, const BranchList *branches) {
    needGroup();
    super.evaluateNNIs5Batch(moves, ptnlh_rows, branches);
}

// ---- UFBoot on the super tree -------------------------------------------------------------------------------------------------
void PhyloSuperTree::genBootSamples(int nsamples, uint64_t seed) {
    needGroup();
    for (size_t p = 0; p < parts.size(); p++)
        parts[p]->genBootSamples(nsamples, (int64_t)llround(parts[p]->getAlnNSite()), seed, (uint32_t)p, 0);
}

void PhyloSuperTree::setBootSamples(int part, const float *samples, int nsamples) {
    needGroup();
    if (part < 0 || part >= size()) throw std::runtime_error("PhyloSuperTree::setBootSamples: no such partition");
    parts[(size_t)part]->setBootSamples(samples, nsamples);
}

void PhyloSuperTree::reservePtnlhRows(int nrows) {
    needGroup();
    hip(iqhip_partition_ptnlh_reserve(group, nrows), "iqhip_partition_ptnlh_reserve");
}

void PhyloSuperTree::ufbootInit(int nsamples) {
    needGroup();
    for (PhyloTree *t : parts) t->pushInputs();
    hip(iqhip_partition_ufboot_init(group, nsamples), "iqhip_partition_ufboot_init");
}

void PhyloSuperTree::ufbootPutCurrentRow(int row) {
    needGroup();
    // every member's likelihood on its current branch (the branch of the last joint solve or computeLikelihood; any branch
    // of the tree where there was none), then the pattern values of that evaluation with the scaling events put back
    for (PhyloTree *t : parts) {
        if (!t->current_it || !t->current_it_back) {
            PhyloNode *leaf = t->findFarthestLeaf();
            t->current_it = leaf->neighbors[0];
            t->current_it_back = t->current_it->node->findNeighbor(leaf);
        }
        t->computeLikelihoodBranch(t->current_it, t->current_it_back->node);
        hip(iqhip_ptnlh_put_current(t->engine, row, t->branchEnd(t->current_it), t->branchEnd(t->current_it_back)),
            "iqhip_ptnlh_put_current");
    }
}

void PhyloSuperTree::ufbootUpdate(const iqhip_ufboot_tree *ent, int n, double epsilon, double logl_cutoff, int64_t counts[3],
                                  double *min_orig_logl) {
    needGroup();
    hip(iqhip_partition_ufboot_update(group, ent, n, epsilon, logl_cutoff, counts, min_orig_logl), "iqhip_partition_ufboot_update");
}

void PhyloSuperTree::ufbootFetchTrees(int64_t *boot_tree) {
    needGroup();
    hip(iqhip_partition_ufboot_fetch(group, nullptr, nullptr, nullptr, boot_tree), "iqhip_partition_ufboot_fetch");
}

// ---- the starting tree of a partitioned alignment -----------------------------------------------------------------------------
void PhyloSuperTree::computeDist(double *dist, double *d2l, const double *init) {
    needGroup();
    for (PhyloTree *t : parts) t->pushInputs();
    hip(iqhip_partition_pair_distances(group, init, min_branch_length, PhyloTree::MAX_GENETIC_DIST, min_branch_length, 100, dist, d2l, nullptr),
        "iqhip_partition_pair_distances");
}

void PhyloSuperTree::pairTiming(double *counts_ms, double *solve_ms) const {
    needGroup();
    hip(iqhip_debug_partition_pair_timing(group, counts_ms, solve_ms), "iqhip_debug_partition_pair_timing");
}

void PhyloSuperTree::computeBioNJ(const double *dist, const double *var, std::string *newick) {
    needGroup();
    const int n = super.leafNum;
    if (n < 3) throw std::runtime_error("computeBioNJ needs at least 3 taxa");
    const std::vector<std::string> names = super.leafNames();
    std::vector<iqhip_bionj_step> steps((size_t)std::max(1, n - 3));
    int32_t last[3];
    double last_len[3];
    hip(iqhip_bionj(parts[0]->engine, n, dist, var, steps.data(), last, last_len), "iqhip_bionj");
    const std::string nwk = PhyloTree::bionjNewick(steps.data(), n, last, last_len, names);
    readTreeString(nwk, names);   // the super tree and every member; member lengths = rate x super lengths
    if (newick) *newick = nwk;
}

int PhyloSuperTree::fixNegativeBranch(bool force) {
    needGroup();
    pushLengths();   // mapTrees
    int fixed = 0;
    for (PhyloTree *t : parts) {
        t->initializeAllPartialPars();
        fixed += t->fixNegativeBranch(force);
    }
    if (!fixed) return 0;
    // PhyloSuperTree::computeBranchLengths: every branch occurs once in every member
    const size_t P = parts.size();
    std::vector<double> len(P), nsite(P);
    std::vector<char> codon(P);
    for (size_t p = 0; p < P; p++) {
        nsite[p] = parts[p]->getAlnNSite();
        codon[p] = parts[p]->seq_type == SEQ_CODON;
    }
    const bool rescale_codon_brlen = rescaleCodonBrlen(codon.data(), P);
    for (size_t i = 0; i < super.nodes.size(); i++) {
        const std::vector<PhyloNeighbor *> &dst = super.nodes[i]->neighbors;
        for (size_t k = 0; k < dst.size(); k++) {
            for (size_t p = 0; p < P; p++) len[p] = parts[p]->nodes[i]->neighbors[k]->length;
            dst[k]->length = weightedBranchLength(len.data(), nsite.data(), codon.data(), P, rescale_codon_brlen);
        }
    }
    pushLengths();   // it is necessary to map the branch lengths from supertree into gene trees
    return fixed;
}

double PhyloSuperTree::optimizeParameters(bool fixed_len, double logl_epsilon, double gradient_epsilon) {
    needGroup();
    for (double &v : cur_score) v = 0.0;
    double tree_lh = fixed_len ? computeLikelihood() : optimizeAllBranches(1);
    for (int i = 1; i < num_param_iterations; i++) {
        // (the members' substitution parameters are taken as given: cur_score = computeLikelihood(), :136-139)
        double cur_lh = computeLikelihood();
        for (PhyloTree *t : parts) t->clearAllPartialLH();
        if (!fixed_rates) cur_lh = optimizeGeneRate(gradient_epsilon);
        const int my_iter = std::min(5, i + 1);
        if (!fixed_len) cur_lh = optimizeAllBranches(my_iter, logl_epsilon);
        if (fabs(cur_lh - tree_lh) < logl_epsilon) {
            tree_lh = cur_lh;
            break;
        }
        tree_lh = cur_lh;
    }
    return tree_lh;
}

}  // namespace iqhost
