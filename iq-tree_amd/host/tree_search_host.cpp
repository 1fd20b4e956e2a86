// tree_search_host.cpp -- see tree_search_host.h
#include "tree_search_host.h"

#include <math.h>

#include <stdexcept>

#include "pars_forest_host.h"

namespace iqhost {

TreeSearch::TreeSearch(PhyloTree *t) : tree(t) {
    if (!t) throw std::runtime_error("TreeSearch: no tree");
}

TreeSearch::TreeSearch(PhyloSuperTree *st) : tree(st ? &st->super : nullptr), stree(st) {
    if (!st) throw std::runtime_error("TreeSearch: no tree");
}

double TreeSearch::computeLikelihood() {
    if (stree) tree->curScore = stree->computeLikelihood();
    else tree->computeLikelihood();
    return tree->curScore;
}
void TreeSearch::readTree(const std::string &newick, const std::vector<std::string> &names) {
    if (stree) stree->readTreeString(newick, names);
    else tree->readTreeString(newick, names);
}
void TreeSearch::doNNI(const NNIMove &mv) {
    if (stree) stree->doNNI(mv);
    else tree->doNNI(mv);
}
void TreeSearch::changeNNIBrans(const NNIMove &mv) {
    if (stree) stree->changeNNIBrans(mv, nni5);
    else tree->changeNNIBrans(mv, nni5);
}
double TreeSearch::sweep() {
    return stree ? stree->optimizeAllBranches(1, loglh_epsilon, PhyloTree::NNI_MAX_NR_STEP)
                 : tree->optimizeAllBranches(1, loglh_epsilon, PhyloTree::NNI_MAX_NR_STEP);
}
void TreeSearch::restore(const std::vector<double> &lenvec) {
    if (stree) {
        stree->restoreBranchLengths(lenvec);
        stree->clearAllPartialLH();
    } else {
        tree->restoreBranchLengths(lenvec);
        tree->clearAllPartialLH();
    }
}

void TreeSearch::checkEligible(const char *who) const {
    const PhyloTree &t = *tree;
    const std::string w = std::string(who) + ": ";
    if (!t.root) throw std::runtime_error(w + "no tree");
    if (t.leafNum < 4) throw std::runtime_error(w + "a tree search needs at least 4 taxa");
    for (const PhyloNode *n : t.nodes)
        if (!n->isLeaf() && n->degree() != 3) throw std::runtime_error(w + "the tree is multifurcating; a tree search needs a binary tree");
    if (stree) {
        if (!stree->group) throw std::runtime_error(w + "the super tree has no engines");
        if (numInitTrees > 0) throw std::runtime_error(w + "the parsimony starting trees (numInitTrees > 0) are not available on a super tree");
        for (const PhyloTree *m : stree->parts) {
            if (m->ufboot_nsamples > 0) throw std::runtime_error(w + "UFBoot is not available on a super tree");
            if (batched && m->lh_mem_save != LM_ALL_BRANCH)
                throw std::runtime_error(w + "the batched NNI evaluation needs setAllBranchMode on the super tree");
        }
        // (the super tree's own UFBoot state lives on the group: initUFBoot on the PhyloSuperTree, the members' stay 0)
        if (t.ufboot_nsamples > 0 && batched && !nni5)
            throw std::runtime_error(w + "UFBoot with the batched evaluation needs nni5 (the nni1 batch keeps no per-pattern rows)");
        return;
    }
    if (!t.engine) throw std::runtime_error(w + "the tree has no engine");
    if (iqhip_comm_size(t.engine) > 1) throw std::runtime_error(w + "not available on sharded engines and communicator ranks");
    if (batched && t.lh_mem_save != LM_ALL_BRANCH) throw std::runtime_error(w + "the batched NNI evaluation needs LM_ALL_BRANCH");
    if (numInitTrees > 0 && t.num_states != 4 && t.num_states != 20 && t.num_states != 64)
        throw std::runtime_error(w + "the parsimony starting trees (numInitTrees > 0) need an engine of 4, 20 or 64 states: the parsimony calls refuse embedded state counts");
    if (numInitTrees < 0 || initSprRadius < 0 || initSprRadius > IQHIP_PARS_SPR_MAX_RADIUS)
        throw std::runtime_error(w + "numInitTrees must be >= 0 and initSprRadius within 0 .. 10");
    if (t.ufboot_nsamples > 0) {
        if (t.nmixture > 1 || t.n_unobserved > 0) throw std::runtime_error(w + "UFBoot is not available with mixture models and +ASC");
        if (batched && !nni5) throw std::runtime_error(w + "UFBoot with the batched evaluation needs nni5 (the nni1 batch keeps no per-pattern rows)");
    }
}

std::vector<std::string> TreeSearch::leafNames() const {
    std::vector<std::string> names((size_t)tree->leafNum);
    for (int i = 0; i < tree->leafNum; i++) {
        const PhyloNode *n = tree->nodes[(size_t)i];
        names[(size_t)i] = n->name.empty() ? std::to_string(n->id) : n->name;
    }
    return names;
}

// IQTree::evalNNIs over the listed branches: both candidates of every branch, in list order
void TreeSearch::evaluate(const BranchList &branches, bool all, std::vector<NNIMove> &moves) {
    PhyloTree &t = *tree;
    std::vector<PhyloNode *> n1, n2;
    if (all) t.internalBranches(n1, n2);
    else
        for (const auto &br : branches) {
            n1.push_back(t.nodes[(size_t)std::min(br.first, br.second)]);
            n2.push_back(t.nodes[(size_t)std::max(br.first, br.second)]);
        }
    moves.clear();
    const bool boot = t.ufboot_nsamples > 0;
    std::vector<int> rows;
    if (boot) {   // store row 0 is saveCurrentTree's, row 1 + k candidate k's
        rows.resize(2 * n1.size());
        for (size_t k = 0; k < rows.size(); k++) rows[k] = (int)(1 + k);
        if (stree) stree->reservePtnlhRows((int)(1 + rows.size()));
        else if (iqhip_ptnlh_reserve(t.engine, (int)(1 + rows.size())) != 0) throw std::runtime_error(iqhip_last_error());
    }
    if (stree) {
        if (batched) {
            if (nni5) stree->evaluateNNIs5Batch(moves, boot ? rows.data() : nullptr, all ? nullptr : &branches);
            else stree->evaluateNNIsBatch(moves, all ? nullptr : &branches);
        } else {
            for (size_t q = 0; q < n1.size(); q++) {
                NNIMove two[2];
                stree->getBestNNIForBran(n1[q]->id, n2[q]->id, nni5, two, boot ? rows.data() + 2 * q : nullptr);
                moves.push_back(two[0]);
                moves.push_back(two[1]);
            }
        }
        if (boot) stree->saveNNITrees(moves);
        return;
    }
    if (batched) {
        if (nni5) t.evaluateNNIs5Batch(moves, boot ? rows.data() : nullptr, all ? nullptr : &branches);
        else t.evaluateNNIsBatch(moves, all ? nullptr : &branches);
    } else {
        for (size_t q = 0; q < n1.size(); q++) {
            NNIMove two[2];
            t.getBestNNIForBran(n1[q], n2[q], nni5, two, boot ? rows.data() + 2 * q : nullptr);
            moves.push_back(two[0]);
            moves.push_back(two[1]);
        }
    }
    if (boot) t.saveNNITrees(moves);
}

double TreeSearch::optimizeNNI(int &nni_count, int &nni_steps, std::vector<NNIStep> *steps) {
    checkEligible("optimizeNNI");
    PhyloTree &t = *tree;
    bool rollBack = false;
    nni_count = 0;
    int numNNIs = 0;                  // number of NNIs applied in each step
    const int MAXSTEPS = t.leafNum;   // aln->getNSeq()
    BranchList branches;              // empty: all internal branches
    std::vector<double> lenvec;
    std::vector<NNIMove> nonConfNNIs, appliedNNIs;
    for (nni_steps = 1; nni_steps <= MAXSTEPS; nni_steps++) {
        const double oldScore = t.curScore;
        const long submissions0 = t.num_submissions;
        NNIStep st;
        if (!rollBack) {
            if (t.ufboot_nsamples > 0) t.saveCurrentTree(t.curScore);
            t.saveBranchLengths(lenvec);
            std::vector<NNIMove> moves, plusNNIs;
            const bool all = branches.empty();
            evaluate(branches, all, moves);
            for (size_t q = 0; q + 1 < moves.size(); q += 2) {   // getBestNNIForBran's return value, then evalNNIs' test
                const NNIMove &best = moves[q].newloglh > moves[q + 1].newloglh ? moves[q] : moves[q + 1];
                if (best.newloglh > t.curScore + loglh_epsilon) plusNNIs.push_back(best);
            }
            iqsearch::sortMoves(plusNNIs);
            if (steps) {
                st.all_branches = all;
                for (size_t q = 0; q < moves.size(); q += 2) st.branches.push_back({moves[q].node1, moves[q].node2});
                st.evaluated = moves;
                st.positive = plusNNIs;
            }
            if (plusNNIs.empty()) {
                if (steps) {
                    st.score = t.curScore;
                    st.submissions = t.num_submissions - submissions0;
                    steps->push_back(st);
                }
                break;
            }
            nonConfNNIs = iqsearch::selectNonConflicting(plusNNIs);
            numNNIs = (int)nonConfNNIs.size();
        }
        // doNNIs: apply the moves with their lengths.  The reference's moves name neighbour SLOTS (iterators), so when an
        // earlier move of the step has re-hung an end of a later one (non-conflicting moves may be adjacent), the later move
        // swaps what its slots hold by then: the slots are looked up on the tree as it was evaluated
        auto slot_of = [&](int at, int to) {
            const std::vector<PhyloNeighbor *> &nb = t.nodes[(size_t)at]->neighbors;
            for (size_t k = 0; k < nb.size(); k++)
                if (nb[k]->node->id == to) return k;
            throw std::runtime_error("optimizeNNI: a move does not belong to the tree");
        };
        std::vector<std::pair<size_t, size_t>> slots;
        for (int i = 0; i < numNNIs; i++)
            slots.push_back({slot_of(nonConfNNIs[(size_t)i].node1, nonConfNNIs[(size_t)i].node1_nei),
                             slot_of(nonConfNNIs[(size_t)i].node2, nonConfNNIs[(size_t)i].node2_nei)});
        appliedNNIs.clear();
        for (int i = 0; i < numNNIs; i++) {
            NNIMove mv = nonConfNNIs[(size_t)i];
            mv.node1_nei = t.nodes[(size_t)mv.node1]->neighbors[slots[(size_t)i].first]->node->id;
            mv.node2_nei = t.nodes[(size_t)mv.node2]->neighbors[slots[(size_t)i].second]->node->id;
            doNNI(mv);
            appliedNNIs.push_back(mv);
            changeNNIBrans(mv);
        }
        t.current_it = t.current_it_back = nullptr;
        branches.clear();
        if (speednni) branches = iqsearch::branchesForNNI(appliedNNIs, t.adjacency());
        t.curScore = sweep();
        st.applied = appliedNNIs;
        st.score = t.curScore;
        if (t.curScore >= nonConfNNIs[0].newloglh - loglh_epsilon) {
            nni_count += numNNIs;
            rollBack = false;
        } else {
            // restore the tree by reverting all NNIs -- last first, the order that also undoes adjacent moves; the reference
            // reverts first to last, which is the same for moves that do not touch -- then the lengths; every vector is
            // stale afterwards
            for (size_t i = appliedNNIs.size(); i-- > 0;) doNNI(appliedNNIs[i]);
            restore(lenvec);
            rollBack = true;
            numNNIs = 1;   // only apply the best NNI
            t.curScore = oldScore;
            st.rolled_back = true;
        }
        if (steps) {
            st.submissions = t.num_submissions - submissions0;
            steps->push_back(st);
        }
        if (t.curScore - oldScore < 0.1) break;
    }
    return t.curScore;
}

void TreeSearch::doRandomNNIs(int numNNI, uint64_t iteration, std::vector<std::array<int, 4>> *done) {
    checkEligible("doRandomNNIs");
    PhyloTree &t = *tree;
    std::vector<PhyloNode *> n1, n2;
    for (int cnt = 0; cnt < numNNI; cnt++) {
        t.internalBranches(n1, n2);
        if (n1.empty()) break;
        const uint64_t d = 1 + 3 * (uint64_t)cnt;
        const int index = iqsearch::searchRandInt(iqsearch::searchRand(seed, iteration, d), (int)n1.size());
        const int bit1 = (int)(iqsearch::searchRand(seed, iteration, d + 1) >> 63);
        const int bit2 = (int)(iqsearch::searchRand(seed, iteration, d + 2) >> 63);
        if (done) done->push_back({n1[(size_t)index]->id, n2[(size_t)index]->id, bit1, bit2});
        if (stree) stree->doOneRandomNNI(n1[(size_t)index]->id, n2[(size_t)index]->id, bit1, bit2);
        else t.doOneRandomNNI(n1[(size_t)index], n2[(size_t)index], bit1, bit2);
    }
    if (stree) stree->clearAllPartialLH();
    else t.clearAllPartialLH();   // resetCurScore / setAlignment of the reference: nothing computed survives
}

double TreeSearch::doTreeSearch() {
    checkEligible("doTreeSearch");
    PhyloTree &t = *tree;
    const bool boot = t.ufboot_nsamples > 0;
    if (stop_rule.stop_condition == iqsearch::SC_BOOTSTRAP_CORRELATION) {
        if (!boot) throw std::runtime_error("doTreeSearch: the correlation stop rule needs initUFBoot");
        if (step_iterations < 2 || step_iterations % 2) throw std::runtime_error("doTreeSearch: step_iterations must be even and >= 2");
    }
    if (popSize < 1) throw std::runtime_error("doTreeSearch: popSize < 1");
    if (!(initPS >= 0.0 && initPS <= 1.0)) throw std::runtime_error("doTreeSearch: the perturbation strength must lie in [0, 1]");
    const std::vector<std::string> names = leafNames();
    trace.clear();
    boot_splits.clear();
    correlation_log.clear();
    candidates = iqsearch::CandidateSet();

    init_trees.clear();
    init_duplicates = 0;
    int nni_count = 0, nni_steps = 0;
    int num_start = 1;   // the iterations the starting trees take
    if (numInitTrees > 0) {
        // createInitTrees: the given tree (computeInitialTree's) and numInitTrees - 1 parsimony trees; duplicate topologies
        // are skipped and counted, every other tree is scored with optimizeAllBranches(2) and enters the set
        auto add_start = [&](const std::string &topology) {
            t.curScore = t.optimizeAllBranches(2);
            iqsearch::CandidateTree c;
            c.tree = t.getTreeString();
            c.topology = topology;
            c.score = t.curScore;
            candidates.update(c.tree, c.topology, c.score);
            init_trees.push_back(c);
        };
        // (the forest works in the engine's parsimony arena: the given tree stays in place while it is built)
        ParsimonyForest forest(&t);
        forest.spr_radius = initSprRadius;
        forest.build(iqsearch::parsimonyOrders(seed, numInitTrees - 1, t.leafNum));
        const std::string given = t.sortedTaxonIdString();
        std::vector<std::string> keys;
        for (const ParsimonyForest::Member &m : forest.members) keys.push_back(m.topology);
        const std::vector<int> dup = iqsearch::duplicateKeys(keys, std::vector<std::string>(1, given));
        init_duplicates = (int)dup.size();
        if (on_init_phase) on_init_phase(*this, 0, numInitTrees - init_duplicates);
        if (on_init_phase) on_init_phase(*this, 1, numInitTrees - init_duplicates);
        add_start(given);
        size_t next_dup = 0;
        for (size_t k = 0; k < forest.members.size(); k++) {
            if (next_dup < dup.size() && dup[next_dup] == (int)k) {
                next_dup++;
                continue;
            }
            t.readTreeString(forest.members[k].newick, names);
            add_start(forest.members[k].topology);
        }
        // initCandidateTreeSet: the best numNNITrees, best first, each one optimizeNNI; the set starts again from them
        const std::vector<std::string> kept = candidates.getTopTrees(std::max(1, std::min(numNNITrees, (int)candidates.size())));
        candidates = iqsearch::CandidateSet();
        num_start = (int)kept.size();
        if (on_init_phase) on_init_phase(*this, 2, num_start);
        stop_rule.addImprovedIteration(1);
        for (int i = 1; i <= num_start; i++) {
            Iteration it;
            it.iteration = i;
            t.readTreeString(kept[(size_t)(i - 1)], names);
            t.computeLikelihood();
            it.perturb_score = t.curScore;
            optimizeNNI(nni_count, nni_steps, keep_trace ? &it.steps : nullptr);
            it.nni_count = nni_count;
            if (t.curScore > candidates.getBestScore() + modeps) {
                t.curScore = t.optimizeAllBranches(100, loglh_epsilon);
                if (!candidates.treeTopologyExist(t.sortedTaxonIdString())) {
                    stop_rule.addImprovedIteration(i);
                    it.new_best = true;
                }
            }
            it.score = t.curScore;
            candidates.update(t.getTreeString(), t.sortedTaxonIdString(), t.curScore);
            if (on_iteration) on_iteration(*this, it);
            if (keep_trace) trace.push_back(it);
        }
        stop_rule.cur_iteration = num_start;
    } else {
        // the starting tree is iteration 1: one optimizeNNI, then into the candidate set
        Iteration it;
        it.iteration = 1;
        computeLikelihood();
        it.perturb_score = t.curScore;
        optimizeNNI(nni_count, nni_steps, keep_trace ? &it.steps : nullptr);
        it.score = t.curScore;
        it.nni_count = nni_count;
        it.new_best = true;
        candidates.update(t.getTreeString(), t.sortedTaxonIdString(), t.curScore);
        if (on_iteration) on_iteration(*this, it);
        if (keep_trace) trace.push_back(it);
        stop_rule.cur_iteration = 1;
        stop_rule.addImprovedIteration(1);
    }
    const double curPerStrength = initPS;
    double cur_correlation = 0.0;
    // a fixed iteration count counts the iterations of the loop below, whatever the starting trees took
    const int fixed_shift = stop_rule.stop_condition == iqsearch::SC_FIXED_ITERATION ? num_start - 1 : 0;

    while (!stop_rule.meetStopCondition(stop_rule.cur_iteration - fixed_shift, cur_correlation)) {
        const int cur = ++stop_rule.cur_iteration;
        Iteration it;
        it.iteration = cur;
        if (boot) t.ufbootNextIteration();   // logl_cutoff = min boot_orig_logl
        // perturb a random one of the best popSize trees
        const int numNNI = (int)floor(curPerStrength * (t.leafNum - 3));
        it.parent = (int)candidates.randCandRank(popSize, iqsearch::searchRand(seed, (uint64_t)cur, 0));
        readTree(candidates.byRank((size_t)it.parent).tree, names);
        doRandomNNIs(numNNI, (uint64_t)cur, &it.random_nnis);
        computeLikelihood();
        it.perturb_score = t.curScore;
        optimizeNNI(nni_count, nni_steps, keep_trace ? &it.steps : nullptr);
        it.nni_count = nni_count;
        // a better tree: the reference re-estimates the model here; the model is given, the lengths are optimised fully
        if (t.curScore > candidates.getBestScore() + modeps) {
            t.curScore = stree ? stree->optimizeAllBranches(100, loglh_epsilon) : t.optimizeAllBranches(100, loglh_epsilon);
            if (!candidates.treeTopologyExist(t.sortedTaxonIdString())) {
                stop_rule.addImprovedIteration(cur);
                it.new_best = true;
            }
        }
        it.score = t.curScore;
        candidates.update(t.getTreeString(), t.sortedTaxonIdString(), t.curScore);
        // convergence criterion of the ultrafast bootstrap
        if (stop_rule.stop_condition == iqsearch::SC_BOOTSTRAP_CORRELATION && cur % (step_iterations / 2) == 0) {
            ufboot::SplitCounts sc(t.leafNum);
            t.ufbootSplitCounts(sc);
            boot_splits.push_back(sc);
            if (cur % step_iterations == 0) {
                cur_correlation = iqsearch::bootstrapCorrelation(boot_splits);
                correlation_log.push_back({cur, cur_correlation});
            }
        }
        if (on_iteration) on_iteration(*this, it);
        if (keep_trace) trace.push_back(it);
    }
    readTree(candidates.getTopTrees(1)[0], names);
    computeLikelihood();
    return candidates.getBestScore();
}

}  // namespace iqhost
