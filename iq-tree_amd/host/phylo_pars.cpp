// phylo_pars.cpp -- see phylo_host.h.  Fitch parsimony (phylotreepars.cpp; include/iqhip.h "Fitch parsimony"): scores,
// stepwise addition and the parsimony SPR search
#include "phylo_host.h"
#include "alignment_host.h"

#include <math.h>

namespace iqhost {

void PhyloTree::needParsimony(const char *what) {
    needDevice(what);
    if (!pars_initialized) initializeAllPartialPars();
}

int64_t PhyloTree::parsInformativeSites() {
    // parsimony-informative patterns: Alignment::isInformative, the rule of computeConst, asked of this tree's data type
    Alignment rule;
    rule.seq_type = seq_type;
    rule.num_states = num_states;
    rule.STATE_UNKNOWN = STATE_UNKNOWN;
    pars_informative.assign((size_t)nptn, 0);
    int64_t total = 0;
    for (int64_t p = 0; p < nptn; p++) {
        pars_informative[(size_t)p] = rule.isInformative(aln_states.data() + p, leafNum, (size_t)nptn);
        if (pars_informative[(size_t)p]) total += (int64_t)ptn_freq[(size_t)p];
    }
    return total;
}

void PhyloTree::initializeAllPartialPars() {
    needDevice("initializeAllPartialPars");
    if (!root) throw std::runtime_error("no tree");
    pushInputs();
    parsInformativeSites();
    check(iqhip_pars_init(engine, pars_informative.data(), 4 * (leafNum - 1), &pars_nsites), "iqhip_pars_init");
    assignParsSlots();
    pars_initialized = true;
}

void PhyloTree::assignParsSlots() {   // one slot per directed vector that is not a tip's; every parsimony flag goes down
    pars_next_slot = pars_slot_base < 0 ? leafNum : pars_slot_base;
    for (PhyloNeighbor *nb : all_neighbors) {
        nb->pars_slot = nb->node->isLeaf() ? nb->node->id : pars_next_slot++;
        nb->partial_lh_computed &= ~2;
    }
}

void PhyloTree::collectParsOps(PhyloNeighbor *dad_branch, PhyloNode *dad, std::vector<iqhip_pars_op> &ops) {
    PhyloNode *node = dad_branch->node;
    if (node->isLeaf() || (dad_branch->partial_lh_computed & 2)) return;
    PhyloNeighbor *kid[2] = {nullptr, nullptr};
    int nkid = 0;
    for (PhyloNeighbor *nb : node->neighbors)
        if (nb->node != dad) {
            if (nkid == 2) throw std::runtime_error("parsimony needs a strictly bifurcating tree");
            kid[nkid++] = nb;
        }
    if (nkid != 2) throw std::runtime_error("parsimony needs a strictly bifurcating tree");
    collectParsOps(kid[0], node, ops);
    collectParsOps(kid[1], node, ops);
    ops.push_back(iqhip_pars_op{dad_branch->pars_slot, kid[0]->pars_slot, kid[1]->pars_slot, 0});
    dad_branch->partial_lh_computed |= 2;
}

void PhyloTree::submitParsOps(std::vector<iqhip_pars_op> &ops) {
    if (ops.empty()) return;
    check(iqhip_pars_update(engine, ops.data(), (int)ops.size()), "iqhip_pars_update");
    ops.clear();
}

void PhyloTree::computePartialParsimony(PhyloNeighbor *dad_branch, PhyloNode *dad) {
    (this->*computePartialParsimonyPointer)(dad_branch, dad);
}
int PhyloTree::computeParsimonyBranch(PhyloNeighbor *dad_branch, PhyloNode *dad, int *branch_subst) {
    return (this->*computeParsimonyBranchPointer)(dad_branch, dad, branch_subst);
}

void PhyloTree::computePartialParsimonyHIP(PhyloNeighbor *dad_branch, PhyloNode *dad) {
    needParsimony("computePartialParsimony");
    std::vector<iqhip_pars_op> ops;
    collectParsOps(dad_branch, dad, ops);
    submitParsOps(ops);
}

int PhyloTree::computeParsimonyBranchHIP(PhyloNeighbor *dad_branch, PhyloNode *dad, int *branch_subst) {
    needParsimony("computeParsimonyBranch");
    PhyloNeighbor *node_branch = dad_branch->node->findNeighbor(dad);
    std::vector<iqhip_pars_op> ops;
    collectParsOps(dad_branch, dad, ops);
    collectParsOps(node_branch, dad_branch->node, ops);
    submitParsOps(ops);
    const int32_t ends[2] = {dad_branch->pars_slot, node_branch->pars_slot};
    int32_t score = 0, subst = 0;
    check(iqhip_pars_branch_scores(engine, ends, 1, &score, &subst), "iqhip_pars_branch_scores");
    if (branch_subst) *branch_subst = subst;
    return score;
}

int PhyloTree::computeParsimony() {
    if (!root) throw std::runtime_error("no tree");
    return computeParsimonyBranch(root->neighbors[0], root);
}

void PhyloTree::computeAllPartialPars() {
    needParsimony("computeAllPartialPars");
    std::vector<iqhip_pars_op> ops;
    collectAllParsOps(ops);
    submitParsOps(ops);
}

void PhyloTree::collectAllParsOps(std::vector<iqhip_pars_op> &ops) {
    std::vector<PhyloNode *> n1, n2;
    getBranches(n1, n2);
    for (size_t k = 0; k < n1.size(); k++) {
        collectParsOps(n1[k]->findNeighbor(n2[k]), n1[k], ops);
        collectParsOps(n2[k]->findNeighbor(n1[k]), n2[k], ops);
    }
}

void PhyloTree::getBranches(std::vector<PhyloNode *> &n1, std::vector<PhyloNode *> &n2, PhyloNode *node, PhyloNode *dad) const {
    if (!node) node = root;
    for (PhyloNeighbor *nb : node->neighbors)
        if (nb->node != dad) {
            const bool lower = node->id < nb->node->id;
            n1.push_back(lower ? node : nb->node);
            n2.push_back(lower ? nb->node : node);
            getBranches(n1, n2, nb->node, node);
        }
}

void PhyloTree::fixBranchList(std::vector<PhyloNeighbor *> &all, std::vector<PhyloNode *> &from) const {
    // the branches in the reference's recursion order: (node, neighbour) from the root downwards
    struct Rec {
        std::vector<PhyloNeighbor *> &all;
        std::vector<PhyloNode *> &from;
        void go(PhyloNode *node, PhyloNode *dad) {
            for (PhyloNeighbor *nb : node->neighbors)
                if (nb->node != dad) {
                    all.push_back(nb);
                    from.push_back(node);
                    go(nb->node, node);
                }
        }
    } rec{all, from};
    rec.go(root, nullptr);
}

int PhyloTree::fixNegativeBranch(bool force) {
    if (!root) throw std::runtime_error("no tree");
    std::vector<PhyloNeighbor *> all;
    std::vector<PhyloNode *> from;
    fixBranchList(all, from);
    std::vector<int32_t> ends;
    size_t ntodo = 0;
    for (size_t k = 0; k < all.size(); k++)
        if (all[k]->length < 0.0 || force) ntodo++;
    std::vector<int32_t> subst(ntodo);
    if (ntodo) {
        computeAllPartialPars();
        for (size_t k = 0; k < all.size(); k++)
            if (all[k]->length < 0.0 || force) {
                ends.push_back(all[k]->pars_slot);
                ends.push_back(all[k]->node->findNeighbor(from[k])->pars_slot);
            }
        check(iqhip_pars_branch_scores(engine, ends.data(), (int)ntodo, nullptr, subst.data()), "iqhip_pars_branch_scores");
    }
    return applyParsLengths(all, from, subst.data(), force, getAlnNSite());
}

int PhyloTree::applyParsLengths(const std::vector<PhyloNeighbor *> &all, const std::vector<PhyloNode *> &from, const int32_t *subst,
                                bool force, double nsite) {
    int fixed = 0;
    size_t q = 0;
    for (size_t k = 0; k < all.size(); k++) {
        PhyloNeighbor *nb = all[k], *back = nb->node->findNeighbor(from[k]);
        if (nb->length < 0.0 || force) {
            const int branch_subst = subst[q++];
            double branch_length = (branch_subst > 0) ? ((double)branch_subst / nsite) : (1.0 / nsite);
            const double z = (double)num_states / (num_states - 1);
            const double x = 1.0 - (z * branch_length);
            if (x > 0) branch_length = -log(x) / z;
            if (branch_length < min_branch_length) branch_length = min_branch_length;
            nb->length = back->length = branch_length;
            fixed++;
        }
        if (nb->length <= 0.0) nb->length = back->length = min_branch_length;
    }
    if (fixed) {   // new lengths: every likelihood vector is stale (the parsimony flags stay)
        for (PhyloNeighbor *nb : all_neighbors) nb->partial_lh_computed &= ~1;
        current_it = current_it_back = nullptr;
        theta_computed = false;
    }
    return fixed;
}

void PhyloTree::startParsimonyTree(const int *taxon_order, const std::vector<std::string> &names) {
    const int size = leafNum;
    {
        std::vector<char> seen((size_t)size, 0);
        for (int k = 0; k < size; k++) {
            if (taxon_order[k] < 0 || taxon_order[k] >= size || seen[(size_t)taxon_order[k]])
                throw std::runtime_error("computeParsimonyTree: the addition order is not a permutation of the taxa");
            seen[(size_t)taxon_order[k]] = 1;
        }
    }
    deleteAllPartialLh();
    freeTree();
    nodes.assign((size_t)(2 * size - 2), nullptr);
    pars_names = names;
    // the initial tree of 3 taxa around node `size`
    PhyloNode *centre = newParsNode(size);
    for (int k = 0; k < 3; k++) {
        PhyloNode *leaf = newParsNode(taxon_order[k]);
        newParsNeighbor(centre, leaf);
        newParsNeighbor(leaf, centre);
    }
    root = nodes[(size_t)taxon_order[0]];
}

PhyloNode *PhyloTree::newParsNode(int id) {
    PhyloNode *nd = new PhyloNode();
    nd->id = id;
    if (id < leafNum && id < (int)pars_names.size()) nd->name = pars_names[(size_t)id];
    nodes[(size_t)id] = nd;
    return nd;
}

PhyloNeighbor *PhyloTree::newParsNeighbor(PhyloNode *from, PhyloNode *to) {
    PhyloNeighbor *nb = new PhyloNeighbor();
    nb->node = to;
    nb->length = -1.0;
    from->neighbors.push_back(nb);
    all_neighbors.push_back(nb);
    return nb;
}

void PhyloTree::collectInsertScan(std::vector<PhyloNode *> &nodes1, std::vector<PhyloNode *> &nodes2, std::vector<iqhip_pars_op> &ops,
                                  std::vector<int32_t> &ends) {
    nodes1.clear();
    nodes2.clear();
    getBranches(nodes1, nodes2);
    for (size_t k = 0; k < nodes1.size(); k++) {
        PhyloNeighbor *a = nodes2[k]->findNeighbor(nodes1[k]), *c = nodes1[k]->findNeighbor(nodes2[k]);
        collectParsOps(a, nodes2[k], ops);
        collectParsOps(c, nodes1[k], ops);
        ends.push_back(a->pars_slot);
        ends.push_back(c->pars_slot);
    }
}

void PhyloTree::insertParsimonyTaxon(PhyloNode *target_node, PhyloNode *target_dad, int taxon, int cur) {
    // insert added_node in the middle of target_node -- target_dad (:382-405); its neighbours: the new taxon, then
    // target_node, then target_dad
    PhyloNode *new_taxon = newParsNode(taxon), *added_node = newParsNode(leafNum + cur - 2);
    PhyloNeighbor *to_taxon = newParsNeighbor(added_node, new_taxon);
    PhyloNeighbor *from_taxon = newParsNeighbor(new_taxon, added_node);
    PhyloNeighbor *dad_side = target_dad->findNeighbor(target_node), *node_side = target_node->findNeighbor(target_dad);
    PhyloNeighbor *to_node = newParsNeighbor(added_node, target_node), *to_dad = newParsNeighbor(added_node, target_dad);
    // added_node -> target_node inherits what target_dad saw of target_node, and the other way round
    to_node->pars_slot = dad_side->pars_slot;
    to_node->partial_lh_computed = dad_side->partial_lh_computed;
    to_dad->pars_slot = node_side->pars_slot;
    to_dad->partial_lh_computed = node_side->partial_lh_computed;
    dad_side->node = added_node;    // updateNeighbor: in place, the position in the neighbour list is kept
    node_side->node = added_node;
    to_taxon->pars_slot = new_taxon->id;
    // (the reference copies the scan's fitch(a, c) into this vector; here its flag stays down and the next
    // submission computes it with everything else)
    from_taxon->pars_slot = pars_next_slot++;
    dad_side->clearPartialLh();
    dad_side->pars_slot = pars_next_slot++;
    node_side->clearPartialLh();
    node_side->pars_slot = pars_next_slot++;
    target_dad->clearReversePartialLh(added_node);
    target_node->clearReversePartialLh(added_node);
}

void PhyloTree::renumberBranches() {   // branch ids in traversal order from the root
    int next_id = 0;
    std::vector<PhyloNode *> n1, n2;
    getBranches(n1, n2);
    for (size_t k = 0; k < n1.size(); k++) n1[k]->findNeighbor(n2[k])->id = n2[k]->findNeighbor(n1[k])->id = next_id++;
}

void PhyloTree::finishParsimonyTree() {
    nodeNum = 2 * leafNum - 2;
    branchNum = 2 * leafNum - 3;
    renumberBranches();
    current_it = current_it_back = nullptr;
    theta_computed = false;
}

int PhyloTree::computeParsimonyTree(const int *taxon_order, std::vector<ParsStep> *trace) {
    needDevice("computeParsimonyTree");
    const int size = leafNum;
    if (size < 3) throw std::runtime_error("computeParsimonyTree needs at least 3 taxa");
    std::vector<std::string> names((size_t)size);
    for (int k = 0; k < size && k < (int)nodes.size(); k++)
        if (nodes[(size_t)k]) names[(size_t)k] = nodes[(size_t)k]->name;
    startParsimonyTree(taxon_order, names);
    pars_initialized = false;
    initializeAllPartialPars();   // (the three vectors that point at the centre take slots; leaves are their own)
    if (trace) trace->clear();
    int best_pars_score = 0;
    std::vector<iqhip_pars_op> ops;
    for (int cur = 3; cur < size; cur++) {
        std::vector<PhyloNode *> nodes1, nodes2;
        // every vector the scan reads, in one submission
        std::vector<int32_t> ends;
        collectInsertScan(nodes1, nodes2, ops, ends);
        submitParsOps(ops);
        ParsStep step;
        int32_t best = 0, best_score = 0;
        if (trace) step.score.resize(nodes1.size());
        check(iqhip_pars_insert_scores(engine, ends.data(), (int)nodes1.size(), taxon_order[cur], trace ? step.score.data() : nullptr,
                                       &best, &best_score),
              "iqhip_pars_insert_scores");
        best_pars_score = best_score;
        if (trace) {
            for (size_t k = 0; k < nodes1.size(); k++) {
                step.node1.push_back(nodes1[k]->id);
                step.node2.push_back(nodes2[k]->id);
            }
            step.chosen = best;
            step.best_score = best_score;
            trace->push_back(step);
        }
        insertParsimonyTaxon(nodes1[(size_t)best], nodes2[(size_t)best], taxon_order[cur], cur);
    }
    finishParsimonyTree();
    fixNegativeBranch(true);
    if (size == 3) best_pars_score = computeParsimony();
    return best_pars_score;
}

// ---- parsimony SPR search ------------------------------------------------------------------------------------------------
void PhyloTree::collectSprJobs(int radius, std::vector<iqhip_pars_spr_job> &jobs, std::vector<iqhip_pars_spr_step> &steps,
                               std::vector<SprMove> &moves) {
    if (!root) throw std::runtime_error("no tree");
    if (radius < 1 || radius > IQHIP_PARS_SPR_MAX_RADIUS) throw std::runtime_error("collectSprJobs: radius outside 1 .. 10");
    if (!pars_initialized) {
        if (engine && !dry_run) initializeAllPartialPars();
        else assignParsSlots();
    }
    jobs.clear();
    steps.clear();
    moves.clear();
    struct Walk {
        int radius, first;
        PhyloNode *p, *s;
        std::vector<iqhip_pars_spr_step> &steps;
        std::vector<SprMove> &moves;
        // the branches beyond node a (reached from dad); step `parent` holds everything on dad's side of dad -- a
        void go(PhyloNode *a, PhyloNode *dad, int parent, int depth) {
            if (a->isLeaf() || depth > radius) return;
            PhyloNeighbor *kid[2] = {nullptr, nullptr};
            int nkid = 0;
            for (PhyloNeighbor *nb : a->neighbors)
                if (nb->node != dad) {
                    if (nkid == 2) throw std::runtime_error("parsimony needs a strictly bifurcating tree");
                    kid[nkid++] = nb;
                }
            if (nkid != 2) throw std::runtime_error("parsimony needs a strictly bifurcating tree");
            for (int c = 0; c < 2; c++) {
                const int k = (int)steps.size() - first;
                steps.push_back(iqhip_pars_spr_step{parent, kid[1 - c]->pars_slot, kid[c]->pars_slot, 0});
                moves.push_back(SprMove{p->id, s->id, a->id, kid[c]->node->id, depth});
                go(kid[c]->node, a, k, depth + 1);
            }
        }
    };
    for (PhyloNode *p : nodes) {
        if (!p || p->isLeaf()) continue;
        if (p->degree() != 3) throw std::runtime_error("parsimony needs a strictly bifurcating tree");
        for (int i = 0; i < 3; i++) {
            PhyloNeighbor *to_s = p->neighbors[(size_t)i], *to_q1 = p->neighbors[(size_t)(i == 0 ? 1 : 0)],
                          *to_q2 = p->neighbors[(size_t)(i == 2 ? 1 : 2)];
            PhyloNode *q1 = to_q1->node, *q2 = to_q2->node;
            const int first = (int)steps.size();
            Walk w{radius, first, p, to_s->node, steps, moves};
            steps.push_back(iqhip_pars_spr_step{-1, to_q2->pars_slot, to_q1->pars_slot, 0});
            moves.push_back(SprMove{p->id, to_s->node->id, q1->id, q2->id, 0});
            // (q1 is reached over the merged branch: its far side is q2, and p itself is not q1's neighbour any more)
            w.go(q1, p, 0, 1);
            const int second = (int)steps.size() - first;
            steps.push_back(iqhip_pars_spr_step{-1, to_q1->pars_slot, to_q2->pars_slot, IQHIP_PARS_SPR_NO_SCORE});
            moves.push_back(SprMove{p->id, to_s->node->id, q2->id, q1->id, 0});
            w.go(q2, p, second, 1);
            const int n = (int)steps.size() - first;
            if (n == 2) {   // two leaves beyond p: nowhere to go
                steps.resize((size_t)first);
                moves.resize((size_t)first);
                continue;
            }
            jobs.push_back(iqhip_pars_spr_job{to_s->pars_slot, first, n, 0});
        }
    }
}

void PhyloTree::applySprMove(const SprMove &mv) {
    const int nn = (int)nodes.size();
    auto node_of = [&](int id) -> PhyloNode * {
        if (id < 0 || id >= nn || !nodes[(size_t)id]) throw std::runtime_error("applySprMove: no such node");
        return nodes[(size_t)id];
    };
    PhyloNode *p = node_of(mv.prune), *s = node_of(mv.subtree), *a = node_of(mv.node1), *b = node_of(mv.node2);
    if (p->degree() != 3 || !p->findNeighbor(s)) throw std::runtime_error("applySprMove: the subtree does not hang at the prune node");
    PhyloNeighbor *to_q[2] = {nullptr, nullptr};
    int nq = 0;
    for (PhyloNeighbor *nb : p->neighbors)
        if (nb->node != s) to_q[nq++] = nb;
    PhyloNode *q1 = to_q[0]->node, *q2 = to_q[1]->node;
    // the target: a branch of the tree as it stands that neither touches the prune node nor lies inside the pruned subtree
    // (every branch of the pruned tree but the merged one); everything is checked before anything changes
    PhyloNeighbor *a_b = a->findNeighbor(b), *b_a = b->findNeighbor(a);
    if (a == p || b == p || !a_b || !b_a) throw std::runtime_error("applySprMove: the target is not a branch of the pruned tree");
    {
        std::vector<std::pair<PhyloNode *, PhyloNode *>> todo{{s, p}};
        while (!todo.empty()) {
            PhyloNode *x = todo.back().first, *dad = todo.back().second;
            todo.pop_back();
            if (x == a || x == b) throw std::runtime_error("applySprMove: the target lies inside the pruned subtree");
            for (PhyloNeighbor *nb : x->neighbors)
                if (nb->node != dad) todo.push_back({nb->node, x});
        }
    }
    deleteAllPartialLh();   // (topology change: every likelihood vector and every parsimony flag)
    // merge q1 -- p -- q2 into q1 -- q2 (in place: the positions in the neighbour lists are kept)
    PhyloNeighbor *q1_p = q1->findNeighbor(p), *q2_p = q2->findNeighbor(p);
    const double merged = to_q[0]->length + to_q[1]->length;
    q1_p->node = q2;
    q2_p->node = q1;
    q1_p->length = q2_p->length = merged;
    // split a -- b with p
    const double half = a_b->length * 0.5;
    a_b->node = p;
    b_a->node = p;
    to_q[0]->node = a;
    to_q[1]->node = b;
    a_b->length = b_a->length = to_q[0]->length = to_q[1]->length = half;
    renumberBranches();
    assignParsSlots();   // (a neighbour that pointed at a leaf may point at an internal node now, and the other way round)
    current_it = current_it_back = nullptr;
    theta_computed = false;
}

int PhyloTree::optimizeParsimonySPR(int radius, int max_rounds, std::vector<SprRound> *trace) {
    needDevice("optimizeParsimonySPR");
    if (radius < 1 || radius > IQHIP_PARS_SPR_MAX_RADIUS) throw std::runtime_error("optimizeParsimonySPR: radius outside 1 .. 10");
    if (trace) trace->clear();
    std::vector<iqhip_pars_spr_job> jobs;
    std::vector<iqhip_pars_spr_step> steps;
    std::vector<SprMove> moves;
    std::vector<int32_t> score, best_step, best_score;
    int current = -1;
    for (int round = 0; max_rounds < 0 || round < max_rounds; round++) {
        computeAllPartialPars();
        collectSprJobs(radius, jobs, steps, moves);
        if (jobs.empty()) break;   // (4 taxa or fewer branches than a move needs)
        score.resize(steps.size());
        best_step.resize(jobs.size());
        best_score.resize(jobs.size());
        int32_t best_job = -1;
        check(iqhip_pars_spr_scan(engine, jobs.data(), (int)jobs.size(), steps.data(), (int)steps.size(), score.data(),
                                  best_step.data(), best_score.data(), &best_job),
              "iqhip_pars_spr_scan");
        SprRound r;
        r.score_before = score[(size_t)jobs[0].first_step];
        for (const iqhip_pars_spr_job &job : jobs)   // every scored root step is the tree as it stands
            if (score[(size_t)job.first_step] != r.score_before)
                throw std::runtime_error("optimizeParsimonySPR: the prune points disagree about the score of the current tree");
        for (int32_t v : score) r.steps_scored += v >= 0;
        if (best_job < 0) throw std::runtime_error("optimizeParsimonySPR: nothing was scored");
        r.job = best_job;
        r.step = best_step[(size_t)best_job];
        r.score = best_score[(size_t)best_job];
        r.move = moves[(size_t)jobs[(size_t)best_job].first_step + (size_t)r.step];
        r.applied = r.score < r.score_before;
        if (r.applied && r.move.depth < 1) throw std::runtime_error("optimizeParsimonySPR: a root step beats the current tree");
        current = r.applied ? r.score : r.score_before;
        if (r.applied) applySprMove(r.move);
        if (trace) trace->push_back(r);
        if (!r.applied) break;
    }
    return current >= 0 ? current : computeParsimony();
}

}  // namespace iqhost
