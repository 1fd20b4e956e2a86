// phylo_nni.cpp -- see phylo_host.h.  NNI evaluation, phylotree.cpp:2873-3066 (upper-bound shortcut left out; the ptnlh
// output goes to the engine's store), and below it the tree edits of the NNI search
#include "phylo_host.h"
#include "mirror_policy.h"

#include <string.h>

#include <algorithm>

namespace iqhost {

static void updateNeighborNode(PhyloNode *at, PhyloNode *oldn, PhyloNode *newn) {
    for (PhyloNeighbor *nb : at->neighbors)
        if (nb->node == oldn) { nb->node = newn; return; }
    throw std::runtime_error("updateNeighbor: not adjacent");
}

PhyloTree::NNIMove PhyloTree::getBestNNIForBran(PhyloNode *node1, PhyloNode *node2, bool nni5, NNIMove moves[2],
                                                const int *ptnlh_rows) {
    if (node1->isLeaf() || node2->isLeaf() || node1->degree() != 3 || node2->degree() != 3)
        throw std::runtime_error("getBestNNIForBran needs an internal branch of a binary tree");
    if (!central_partial_lh) initializeAllPartialLh();
    const int IT_NUM = nni5 ? 6 : 2;
    if (!nni_keys[0])
        for (int i = 0; i < 6; i++) nni_keys[i] = next_key++;
    // the neighbour slots that get a scratch copy (:2901-2924)
    std::vector<PhyloNeighbor **> slot;
    auto slot_of = [](PhyloNode *at, PhyloNode *to) -> PhyloNeighbor ** {
        for (auto &nb : at->neighbors)
            if (nb->node == to) return &nb;
        throw std::runtime_error("not adjacent");
    };
    slot.push_back(slot_of(node1, node2));
    slot.push_back(slot_of(node2, node1));
    if (nni5) {
        for (PhyloNeighbor *nb : node1->neighbors) if (nb->node != node2) slot.push_back(slot_of(nb->node, node1));
        for (PhyloNeighbor *nb : node2->neighbors) if (nb->node != node1) slot.push_back(slot_of(nb->node, node2));
    }
    std::vector<PhyloNeighbor *> saved(IT_NUM);
    for (int id = 0; id < IT_NUM; id++) {
        saved[id] = *slot[id];
        PhyloNeighbor *tmp = new PhyloNeighbor();
        tmp->node = saved[id]->node;
        tmp->length = saved[id]->length;
        tmp->id = saved[id]->id;
        tmp->partial_lh = nni_keys[id];
        *slot[id] = tmp;
    }
    PhyloNeighbor *node12_it = node1->findNeighbor(node2), *node21_it = node2->findNeighbor(node1);

    // the two moves: first non-node2 neighbour of node1 against each non-node1 neighbour of node2 (:2951-2960)
    size_t i1 = 0;
    while (node1->neighbors[i1]->node == node2) i1++;
    std::vector<size_t> i2s;
    for (size_t j = 0; j < node2->neighbors.size(); j++)
        if (node2->neighbors[j]->node != node1) i2s.push_back(j);
    const double backupScore = curScore;
    for (int cnt = 0; cnt < 2; cnt++) {
        const size_t i2 = i2s[cnt];
        PhyloNeighbor *node1_nei = node1->neighbors[i1], *node2_nei = node2->neighbors[i2];
        moves[cnt] = NNIMove();
        moves[cnt].node1 = node1->id;
        moves[cnt].node2 = node2->id;
        moves[cnt].node1_nei = node1_nei->node->id;
        moves[cnt].node2_nei = node2_nei->node->id;
        // do the NNI swap (:2976-2980)
        node1->neighbors[i1] = node2_nei;
        updateNeighborNode(node2_nei->node, node2, node1);
        node2->neighbors[i2] = node1_nei;
        updateNeighborNode(node1_nei->node, node1, node2);
        node12_it->clearPartialLh();
        node21_it->clearPartialLh();
        int i = 1;
        if (nni5) {
            for (PhyloNeighbor *nb : std::vector<PhyloNeighbor *>(node1->neighbors))
                if (nb->node != node2) {
                    nb->node->findNeighbor(node1)->clearPartialLh();
                    optimizeOneBranch(node1, nb->node, false, NNI_MAX_NR_STEP);
                    moves[cnt].newLen[i++] = node1->findNeighbor(nb->node)->length;
                }
            node21_it->clearPartialLh();
        }
        optimizeOneBranch(node1, node2, false, NNI_MAX_NR_STEP);
        moves[cnt].newLen[0] = node1->findNeighbor(node2)->length;
        if (nni5) {
            for (PhyloNeighbor *nb : std::vector<PhyloNeighbor *>(node2->neighbors))
                if (nb->node != node1) {
                    nb->node->findNeighbor(node2)->clearPartialLh();
                    optimizeOneBranch(node2, nb->node, false, NNI_MAX_NR_STEP);
                    moves[cnt].newLen[i++] = node2->findNeighbor(nb->node)->length;
                }
            node12_it->clearPartialLh();
        }
        moves[cnt].newloglh = computeLikelihoodFromBuffer();
        if (ptnlh_rows && ptnlh_rows[cnt] >= 0) {  // computePatternLikelihood(nniMoves[cnt].ptnlh), phylotree.cpp:3019-3020
            needDevice("getBestNNIForBran with store rows");
            check(iqhip_ptnlh_put_current(engine, ptnlh_rows[cnt], branchEnd(current_it), branchEnd(current_it_back)),
                  "iqhip_ptnlh_put_current");
            moves[cnt].ptnlh_row = ptnlh_rows[cnt];
        }
        // swap back (:3027-3030)
        node1->neighbors[i1] = node1_nei;
        updateNeighborNode(node1_nei->node, node2, node1);
        node2->neighbors[i2] = node2_nei;
        updateNeighborNode(node2_nei->node, node1, node2);
    }
    // restore the Neighbor objects (:3036-3044)
    for (int id = IT_NUM - 1; id >= 0; id--) {
        if (*slot[id] == current_it) current_it = saved[id];
        if (*slot[id] == current_it_back) current_it_back = saved[id];
        delete *slot[id];
        *slot[id] = saved[id];
    }
    // restore the length of the 4 branches around node1, node2 (:3048-3051)
    for (PhyloNeighbor *nb : node1->neighbors) if (nb->node != node2) nb->length = nb->node->findNeighbor(node1)->length;
    for (PhyloNeighbor *nb : node2->neighbors) if (nb->node != node1) nb->length = nb->node->findNeighbor(node2)->length;
    theta_computed = false;
    curScore = backupScore;
    return moves[0].newloglh > moves[1].newloglh ? moves[0] : moves[1];
}

void PhyloTree::computeAllPartialLh() {
    if (lh_mem_save != LM_ALL_BRANCH) throw std::runtime_error("computeAllPartialLh needs LM_ALL_BRANCH");
    if (!central_partial_lh) initializeAllPartialLh();
    // one plan for every pending directed vector (each has its own buffer in this mode), one submission
    MirrorPolicy::Plan plan;
    for (PhyloNode *node : nodes)
        for (PhyloNeighbor *nb : node->neighbors)
            if (!nb->node->isLeaf() && (nb->partial_lh_computed & 1) == 0)
                iqhip_adapter::collectPlan<MirrorPolicy>(this, nb, node, plan);
    submitPendingVectors(plan, "computeAllPartialLh");
}

void PhyloTree::submitPendingVectors(MirrorPolicy::Plan &plan, const char *who) {
    MirrorPolicy::record(this, plan);
    if (plan.empty()) return;
    if (!dry_run) noCallerCollective(who);
    std::vector<double> sum_scale(plan.size(), 0.0);
    pushInputs();
    MirrorPolicy::updatePartials(this, plan, sum_scale.data());
    iqhip_adapter::applyScaleFactors<MirrorPolicy>(plan, sum_scale.data());
}

void PhyloTree::computePartialLhAround(const std::vector<PhyloNode *> &n1, const std::vector<PhyloNode *> &n2) {
    if (lh_mem_save != LM_ALL_BRANCH) throw std::runtime_error("computePartialLhAround needs LM_ALL_BRANCH");
    if (!central_partial_lh) initializeAllPartialLh();
    MirrorPolicy::Plan plan;   // as computeAllPartialLh, for the vectors of the listed branches only
    for (size_t q = 0; q < n1.size(); q++)
        for (int side = 0; side < 2; side++) {
            PhyloNode *node = side ? n2[q] : n1[q], *other = side ? n1[q] : n2[q];
            for (PhyloNeighbor *nb : node->neighbors)
                if (nb->node != other && !nb->node->isLeaf() && (nb->partial_lh_computed & 1) == 0)
                    iqhip_adapter::collectPlan<MirrorPolicy>(this, nb, node, plan);
        }
    submitPendingVectors(plan, "computePartialLhAround");
}

// the branches of a batched NNI evaluation: all internal ones, or the caller's list with each branch normalised to
// node1->id < node2->id (the orientation internalBranches gives, so that a listed branch has the full call's entries)
static void nniBranches(const PhyloTree *t, const PhyloTree::BranchList *branches, const char *who, std::vector<PhyloNode *> &n1,
                        std::vector<PhyloNode *> &n2) {
    if (!branches) t->internalBranches(n1, n2);
    else {
        n1.clear();
        n2.clear();
        for (const auto &br : *branches) {
            const int a = std::min(br.first, br.second), b = std::max(br.first, br.second);
            if (a < 0 || b >= (int)t->nodes.size() || a == b || !t->nodes[(size_t)a]->findNeighbor(t->nodes[(size_t)b]) ||
                t->nodes[(size_t)a]->isLeaf() || t->nodes[(size_t)b]->isLeaf())
                throw std::runtime_error(std::string(who) + ": a listed branch is not an internal branch of the tree");
            n1.push_back(t->nodes[(size_t)a]);
            n2.push_back(t->nodes[(size_t)b]);
        }
    }
    for (size_t q = 0; q < n1.size(); q++)
        if (n1[q]->degree() != 3 || n2[q]->degree() != 3) throw std::runtime_error(std::string(who) + " needs a binary tree");
}

// ---- what the two batched evaluators share ---------------------------------------------------------------------------------
bool PhyloTree::beginNNIBatch(const char *who, const BranchList *branches, std::vector<PhyloNode *> &bn1,
                              std::vector<PhyloNode *> &bn2) {
    if (!nni_backend) needDevice(who);
    if (allreduce_hook) throw std::runtime_error(std::string(who) + ": runs with a caller-owned collective use getBestNNIForBran");
    nniBranches(this, branches, who, bn1, bn2);
    if (branches && bn1.empty()) return false;
    if (nni_backend) {
        nni_backend->pendingVectors(bn1, bn2, !branches);
    } else {
        if (branches) computePartialLhAround(bn1, bn2);
        else computeAllPartialLh();
        pushInputs();
    }
    while (nni_batch_keys.size() < 4 * bn1.size()) nni_batch_keys.push_back(next_key++);   // four scratch vectors per branch
    return true;
}

namespace {
// an outward subtree vector around the branch: fixed while the candidate is evaluated (a leaf carries no scaling events)
struct Ext { uint64_t key; int32_t leaf; double sf; };
Ext extOf(const PhyloNeighbor *nb) {
    Ext x;
    if (nb->node->isLeaf()) { x.key = 0; x.leaf = nb->node->id; x.sf = 0.0; }
    else { x.key = nb->partial_lh; x.leaf = -1; x.sf = nb->lh_scale_factor; }
    return x;
}
iqhip_branch_end endOf(const Ext &x) { return iqhip_branch_end{x.key, x.leaf, 0}; }
iqhip_branch_end endOf(uint64_t scratch_key) { return iqhip_branch_end{scratch_key, -1, 0}; }
// one node update; each side is a subtree vector (a, b) or, where that is nullptr, the scratch vector akey / bkey
iqhip_node_op mkop(uint64_t dst, const Ext *a, uint64_t akey, double alen, const Ext *b, uint64_t bkey, double blen) {
    iqhip_node_op o;
    memset(&o, 0, sizeof o);
    o.dst_key = dst;
    o.left_key = a ? a->key : akey;  o.left_leaf = a ? a->leaf : -1;  o.left_len = alen;
    o.right_key = b ? b->key : bkey; o.right_leaf = b ? b->leaf : -1; o.right_len = blen;
    return o;
}
// the solve of the branch between a and b once `ops` have run, within the tree's bounds and the NNI step limit
iqhip_branch_task nniTask(const PhyloTree *t, const iqhip_node_op *ops, int nops, iqhip_branch_end a, iqhip_branch_end b,
                          double xguess) {
    return iqhip_branch_task{ops, nops, PhyloTree::NNI_MAX_NR_STEP, a, b, xguess, t->min_branch_length, t->max_branch_length,
                             t->min_branch_length};
}
}  // namespace

void PhyloTree::submitBranchTasks(const std::vector<iqhip_branch_task> &tasks, const int32_t *rows, std::vector<double> &sum_scale,
                                  std::vector<iqhip_branch_result> &res, std::vector<char> &diverged) {
    const size_t n = tasks.size();
    size_t nops = 0;
    for (const iqhip_branch_task &k : tasks) nops += (size_t)k.nops;
    sum_scale.assign(nops, 0.0);
    res.resize(n);
    if (nni_backend) {   // (the backend's lnL carries the scale-factor terms: the per-op sums stay 0)
        nni_backend->submitTasks(tasks, res, rows);
    } else if (rows)
        check(iqhip_optimize_branch_batch_rows(engine, tasks.data(), (int)n, sum_scale.data(), res.data(), rows),
              "iqhip_optimize_branch_batch_rows");
    else
        check(iqhip_optimize_branch_batch(engine, tasks.data(), (int)n, sum_scale.data(), res.data()), "iqhip_optimize_branch_batch");
    num_submissions++;
    diverged.assign(n, 0);
    for (size_t q = 0; q < n; q++) {
        if (res[q].status == 2) throw std::runtime_error("Wrong computeFuncDerv (non-finite derivative)");
        num_derv_calls += res[q].nsteps;
        diverged[q] = res[q].optx > max_branch_length * 0.95;
    }
}

// the fallback of a diverged solve: this tree's own getBestNNIForBran, or the backend's
void PhyloTree::branchByBranch(PhyloNode *node1, PhyloNode *node2, bool nni5, NNIMove moves[2], const int *ptnlh_rows) {
    if (nni_backend) nni_backend->bestNNIForBran(node1->id, node2->id, nni5, moves, ptnlh_rows);
    else getBestNNIForBran(node1, node2, nni5, moves, ptnlh_rows);
}

void PhyloTree::evaluateNNIsBatch(std::vector<NNIMove> &moves, const BranchList *branches) {
    std::vector<PhyloNode *> bn1, bn2;
    if (!beginNNIBatch("evaluateNNIsBatch", branches, bn1, bn2)) { moves.clear(); return; }
    struct Cand {
        PhyloNode *node1, *node2;
        NNIMove move;
        Ext a, o, x, b;   // node1's first subtree a and node2's x change places; o, b: the other subtree of node2, of node1
        iqhip_node_op ops[2];
    };
    std::vector<Cand> cands;
    for (size_t bq = 0; bq < bn1.size(); bq++) {
        PhyloNode *node1 = bn1[bq], *node2 = bn2[bq];
        std::vector<PhyloNeighbor *> s1, s2;
        for (PhyloNeighbor *nb : node1->neighbors) if (nb->node != node2) s1.push_back(nb);
        for (PhyloNeighbor *nb : node2->neighbors) if (nb->node != node1) s2.push_back(nb);
        for (int cnt = 0; cnt < 2; cnt++) {  // phylotree.cpp:2951-2960: first neighbour of node1 against each of node2's
            const size_t t = cands.size();
            Cand c;
            c.node1 = node1; c.node2 = node2;
            c.move.node1 = node1->id; c.move.node2 = node2->id;
            c.move.node1_nei = s1[0]->node->id; c.move.node2_nei = s2[cnt]->node->id;
            c.a = extOf(s1[0]); c.o = extOf(s2[1 - cnt]); c.x = extOf(s2[cnt]); c.b = extOf(s1[1]);
            // after the swap node2's subtree (seen from node1) joins a and o, node1's joins x and b
            c.ops[0] = mkop(nni_batch_keys[2 * t], &c.a, 0, s1[0]->length, &c.o, 0, s2[1 - cnt]->length);
            c.ops[1] = mkop(nni_batch_keys[2 * t + 1], &c.x, 0, s2[cnt]->length, &c.b, 0, s1[1]->length);
            cands.push_back(c);
        }
    }
    // Two rounds: the reference evaluates the second swap of a branch starting from the length the first swap's
    // optimisation left on that branch (the Neighbor copies are restored only after both, phylotree.cpp:3036-3051),
    // so the first swaps of all branches run side by side, then the second swaps with those lengths as guesses.
    const size_t nc = cands.size();
    std::vector<double> ss[2];
    std::vector<iqhip_branch_result> rr[2];
    std::vector<char> dv[2];
    std::vector<iqhip_branch_task> sub;
    for (int round = 0; round < 2; round++) {
        sub.clear();
        for (size_t t = round; t < nc; t += 2)   // (the tasks hold pointers into cands)
            sub.push_back(nniTask(this, cands[t].ops, 2, endOf(nni_batch_keys[2 * t]), endOf(nni_batch_keys[2 * t + 1]),
                                  round ? rr[0][t / 2].optx : cands[t].node1->findNeighbor(cands[t].node2)->length));
        submitBranchTasks(sub, nullptr, ss[round], rr[round], dv[round]);
    }
    moves.resize(nc);
    for (size_t t = 0; t < nc; t++) {
        const Cand &c = cands[t];
        const size_t round = t & 1, q = t / 2;
        NNIMove &m = moves[t] = c.move;
        m.newLen[0] = rr[round][q].optx;
        const double sf = c.a.sf + c.o.sf + ss[round][2 * q] + c.x.sf + c.b.sf + ss[round][2 * q + 1];
        m.newloglh = rr[round][q].lnl + sf;
        if (dv[round][q] || dv[0][q]) {
            // diverged Newton (phylotree.cpp:2167-2176: optimizeOneBranch compares lnL at the optimum with lnL at the old
            // length and may restore the latter): rare; the one-branch path for this candidate -- and for the second swap
            // of a branch whose first swap diverged, because its starting length is whatever that comparison left
            NNIMove two[2];
            branchByBranch(c.node1, c.node2, false, two, nullptr);
            m = two[round];
        }
    }
}

void PhyloTree::internalBranches(std::vector<PhyloNode *> &n1, std::vector<PhyloNode *> &n2) const {
    n1.clear();
    n2.clear();
    for (PhyloNode *node1 : nodes)
        for (PhyloNeighbor *nb12 : node1->neighbors) {
            PhyloNode *node2 = nb12->node;
            if (node1->isLeaf() || node2->isLeaf() || node1->id > node2->id) continue;
            n1.push_back(node1);
            n2.push_back(node2);
        }
}

void PhyloTree::evaluateNNIs5Batch(std::vector<NNIMove> &moves, const int *ptnlh_rows, const BranchList *branches_in) {
    std::vector<PhyloNode *> bn1, bn2;
    if (!beginNNIBatch("evaluateNNIs5Batch", branches_in, bn1, bn2)) { moves.clear(); return; }
    struct Branch {  // one internal branch: the five Neighbor lengths carry over from the first swap to the second
        PhyloNode *node1, *node2;
        PhyloNeighbor *n1[2], *n2[2];
        double len1[2], len2[2], l0;
    };
    std::vector<Branch> branches;
    for (size_t bq = 0; bq < bn1.size(); bq++) {
        PhyloNode *node1 = bn1[bq], *node2 = bn2[bq];
        Branch b;
        b.node1 = node1; b.node2 = node2;
        int i = 0, j = 0;
        for (PhyloNeighbor *nb : node1->neighbors) if (nb->node != node2) { b.n1[i] = nb; b.len1[i++] = nb->length; }
        for (PhyloNeighbor *nb : node2->neighbors) if (nb->node != node1) { b.n2[j] = nb; b.len2[j++] = nb->length; }
        b.l0 = node1->findNeighbor(node2)->length;
        branches.push_back(b);
    }
    const size_t nb = branches.size();
    moves.assign(2 * nb, NNIMove());
    struct Work {
        Ext X[2], Y[2];               // subtrees at node1 (X1 = moved in, X2) and at node2 in optimisation order
        double *lX[2], *lY[2], *l0;   // their lengths and the central one: the Branch's slots, where the second swap finds them
        const uint64_t *s;            // the branch's four scratch vectors
        double sf0, sf1, sf2, sf3;
        iqhip_node_op ops[2];
        bool diverged;
    };
    static const int len_slot[5] = {1, 2, 0, 3, 4};   // newLen index of the branch each round solves (phylotree.cpp:2984-3024)
    std::vector<Work> work(nb);
    std::vector<iqhip_branch_task> tasks(nb);
    std::vector<double> ss;
    std::vector<iqhip_branch_result> rr;
    std::vector<char> dv;
    std::vector<int32_t> rows(nb);
    for (int cnt = 0; cnt < 2; cnt++) {
        for (size_t q = 0; q < nb; q++) {
            Branch &b = branches[q];
            Work &w = work[q];
            // swap n1[0] <-> n2[cnt]: node1 now holds {n2[cnt], n1[1]}, node2 holds n1[0] at n2[cnt]'s index, which
            // is its place in the neighbour-index order at node2 (phylotree.cpp:3008-3016)
            const int other = 1 - cnt;
            w.X[0] = extOf(b.n2[cnt]);       w.lX[0] = &b.len2[cnt];
            w.X[1] = extOf(b.n1[1]);         w.lX[1] = &b.len1[1];
            w.Y[cnt] = extOf(b.n1[0]);       w.lY[cnt] = &b.len1[0];
            w.Y[other] = extOf(b.n2[other]); w.lY[other] = &b.len2[other];
            w.l0 = &b.l0;
            w.s = &nni_batch_keys[4 * q];
            w.diverged = false;
            NNIMove &m = moves[2 * q + cnt];
            m.node1 = b.node1->id; m.node2 = b.node2->id;
            m.node1_nei = b.n1[0]->node->id; m.node2_nei = b.n2[cnt]->node->id;
        }
        for (int round = 0; round < 5; round++) {
            for (size_t q = 0; q < nb; q++) {
                Work &w = work[q];
                const Ext &Ya = w.Y[0], &Yb = w.Y[1];
                const uint64_t *s = w.s;
                const double l0 = *w.l0;
                const double *const len[5] = {w.lX[0], w.lX[1], w.l0, w.lY[0], w.lY[1]};   // the branch each round solves
                iqhip_branch_end a, b;
                switch (round) {
                    case 0:  // branch node1 - X1: u12 = f(Y...), w = f(u12, X2)
                        w.ops[0] = mkop(s[0], &Ya, 0, *w.lY[0], &Yb, 0, *w.lY[1]);
                        w.ops[1] = mkop(s[1], nullptr, s[0], l0, &w.X[1], 0, *w.lX[1]);
                        a = endOf(w.X[0]); b = endOf(s[1]);
                        break;
                    case 1:  // branch node1 - X2
                        w.ops[0] = mkop(s[1], nullptr, s[0], l0, &w.X[0], 0, *w.lX[0]);
                        a = endOf(w.X[1]); b = endOf(s[1]);
                        break;
                    case 2:  // central branch
                        w.ops[0] = mkop(s[2], &w.X[0], 0, *w.lX[0], &w.X[1], 0, *w.lX[1]);
                        a = endOf(s[0]); b = endOf(s[2]);
                        break;
                    case 3:  // branch node2 - Y1
                        w.ops[0] = mkop(s[3], nullptr, s[2], l0, &Yb, 0, *w.lY[1]);
                        a = endOf(Ya); b = endOf(s[3]);
                        break;
                    default:  // branch node2 - Y2
                        w.ops[0] = mkop(s[3], nullptr, s[2], l0, &Ya, 0, *w.lY[0]);
                        a = endOf(Yb); b = endOf(s[3]);
                        break;
                }
                tasks[q] = nniTask(this, w.ops, round == 0 ? 2 : 1, a, b, *len[round]);
            }
            const bool keep_rows = round == 4 && ptnlh_rows;  // the lnL of the last round is the candidate's: keep its per-pattern values
            for (size_t q = 0; keep_rows && q < nb; q++) moves[2 * q + cnt].ptnlh_row = rows[q] = ptnlh_rows[2 * q + cnt];
            submitBranchTasks(tasks, keep_rows ? rows.data() : nullptr, ss, rr, dv);
            size_t sp = 0;
            for (size_t q = 0; q < nb; q++) {
                Work &w = work[q];
                double *const len[5] = {w.lX[0], w.lX[1], w.l0, w.lY[0], w.lY[1]};
                *len[round] = moves[2 * q + cnt].newLen[len_slot[round]] = rr[q].optx;
                if (dv[q]) w.diverged = true;
                switch (round) {
                    case 0:
                        w.sf0 = w.Y[0].sf + w.Y[1].sf + ss[sp];
                        w.sf1 = w.sf0 + w.X[1].sf + ss[sp + 1];
                        sp += 2;
                        break;
                    case 1: w.sf1 = w.sf0 + w.X[0].sf + ss[sp++]; break;
                    case 2: w.sf2 = w.X[0].sf + w.X[1].sf + ss[sp++]; break;
                    case 3: w.sf3 = w.sf2 + w.Y[1].sf + ss[sp++]; break;
                    default:
                        w.sf3 = w.sf2 + w.Y[0].sf + ss[sp++];
                        moves[2 * q + cnt].newloglh = rr[q].lnl + w.Y[1].sf + w.sf3;
                        break;
                }
            }
        }
        for (size_t q = 0; q < nb; q++)
            if (work[q].diverged) {  // diverged Newton (phylotree.cpp:2167-2176): rare; take the branch-by-branch path
                NNIMove two[2];
                branchByBranch(branches[q].node1, branches[q].node2, true, two, ptnlh_rows ? ptnlh_rows + 2 * q : nullptr);
                moves[2 * q] = two[0];
                moves[2 * q + 1] = two[1];
            }
    }
}

// ---- tree edits of the NNI search, phylotree.cpp:2726-2871
namespace {
// the slot of `at`'s neighbour list that holds one of the two subtrees of the move
PhyloNeighbor **swapSlot(PhyloNode *at, PhyloNode *other_end, int id_a, int id_b) {
    for (PhyloNeighbor *&nb : at->neighbors)
        if (nb->node != other_end && (nb->node->id == id_a || nb->node->id == id_b)) return &nb;
    throw std::runtime_error("doNNI: the move does not belong to this tree");
}
// PhyloNeighbor::reorientPartialLh (phylonode.cpp:22-39): `nb` points to a node whose one buffer may sit on another Neighbor
void reorientPartialLh(PhyloNeighbor *nb, PhyloNode *dad) {
    if (nb->partial_lh) return;
    for (PhyloNeighbor *kid : nb->node->neighbors) {
        if (kid->node == dad) continue;
        PhyloNeighbor *backnei = kid->node->findNeighbor(nb->node);
        if (backnei->partial_lh) {
            nb->partial_lh = backnei->partial_lh;
            backnei->partial_lh = 0;
            backnei->partial_lh_computed &= ~1;
            return;
        }
    }
    throw std::runtime_error("doNNI: partial_lh is not re-oriented");
}
}  // namespace

void PhyloTree::doNNI(const NNIMove &move, bool clearLH) {
    if (move.node1 < 0 || move.node2 < 0 || move.node1 >= (int)nodes.size() || move.node2 >= (int)nodes.size())
        throw std::runtime_error("doNNI: bad node id");
    PhyloNode *node1 = nodes[(size_t)move.node1], *node2 = nodes[(size_t)move.node2];
    PhyloNeighbor *node12_it = node1->findNeighbor(node2), *node21_it = node2->findNeighbor(node1);
    if (!node12_it || !node21_it || node1->degree() != 3 || node2->degree() != 3)
        throw std::runtime_error("doNNI needs an internal branch of a binary tree");
    PhyloNeighbor **slot1 = swapSlot(node1, node2, move.node1_nei, move.node2_nei);
    PhyloNeighbor **slot2 = swapSlot(node2, node1, move.node1_nei, move.node2_nei);
    if ((*slot1)->node == (*slot2)->node) throw std::runtime_error("doNNI: the move does not belong to this tree");
    if (lh_mem_save == LM_PER_NODE && central_partial_lh) {  // reorient partial_lh before swap (:2799-2803)
        reorientPartialLh(node12_it, node1);
        reorientPartialLh(node21_it, node2);
    }
    PhyloNeighbor *node1_nei = *slot1, *node2_nei = *slot2;
    *slot1 = node2_nei;
    updateNeighborNode(node2_nei->node, node2, node1);
    *slot2 = node1_nei;
    updateNeighborNode(node1_nei->node, node1, node2);
    if (clearLH) {
        node12_it->clearPartialLh();
        node21_it->clearPartialLh();
        node2->clearReversePartialLh(node1);
        node1->clearReversePartialLh(node2);
    }
    theta_computed = false;
}

void PhyloTree::changeNNIBrans(const NNIMove &move, bool nni5) {
    if (move.node1 < 0 || move.node2 < 0 || move.node1 >= (int)nodes.size() || move.node2 >= (int)nodes.size())
        throw std::runtime_error("changeNNIBrans: bad node id");
    PhyloNode *node1 = nodes[(size_t)move.node1], *node2 = nodes[(size_t)move.node2];
    PhyloNeighbor *n12 = node1->findNeighbor(node2), *n21 = node2->findNeighbor(node1);
    if (!n12 || !n21) throw std::runtime_error("changeNNIBrans: the move does not belong to this tree");
    n12->length = n21->length = move.newLen[0];
    if (!nni5) return;
    int i = 1;
    for (PhyloNeighbor *nb : node1->neighbors)
        if (nb->node != node2) nb->length = nb->node->findNeighbor(node1)->length = move.newLen[i++];
    for (PhyloNeighbor *nb : node2->neighbors)
        if (nb->node != node1) nb->length = nb->node->findNeighbor(node2)->length = move.newLen[i++];
}

void PhyloTree::saveBranchLengths(std::vector<double> &lenvec) const {
    lenvec.clear();
    for (const PhyloNeighbor *nb : all_neighbors) lenvec.push_back(nb->length);
}

void PhyloTree::restoreBranchLengths(const std::vector<double> &lenvec) {
    if (lenvec.size() != all_neighbors.size()) throw std::runtime_error("restoreBranchLengths: the lengths are not this tree's");
    for (size_t k = 0; k < all_neighbors.size(); k++) all_neighbors[k]->length = lenvec[k];
}

PhyloTree::NNIMove PhyloTree::doOneRandomNNI(PhyloNode *node1, PhyloNode *node2, int bit1, int bit2) {
    if (node1->isLeaf() || node2->isLeaf() || node1->degree() != 3 || node2->degree() != 3 || !node1->findNeighbor(node2))
        throw std::runtime_error("doOneRandomNNI needs an internal branch of a binary tree");
    auto pick = [](PhyloNode *at, PhyloNode *other, int bit) {   // :2732-2758: a draw of 0 takes the first, else the next
        std::vector<PhyloNeighbor *> s;
        for (PhyloNeighbor *nb : at->neighbors)
            if (nb->node != other) s.push_back(nb);
        return s[bit ? 1 : 0];
    };
    NNIMove mv;
    mv.node1 = node1->id;
    mv.node2 = node2->id;
    mv.node1_nei = pick(node1, node2, bit1)->node->id;
    mv.node2_nei = pick(node2, node1, bit2)->node->id;
    doNNI(mv, false);
    return mv;
}

std::vector<std::vector<int>> PhyloTree::adjacency() const {
    std::vector<std::vector<int>> adj(nodes.size());
    for (const PhyloNode *nd : nodes)
        for (const PhyloNeighbor *nb : nd->neighbors) adj[(size_t)nd->id].push_back(nb->node->id);
    return adj;
}

}  // namespace iqhost
