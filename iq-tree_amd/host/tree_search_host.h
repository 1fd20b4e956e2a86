// tree_search_host.h -- the NNI tree search of the reference on top of the device calls of phylo_host.h:
//   IQTree::optimizeNNI    iqtree.cpp:2125-2288   hill climbing by sets of non-conflicting NNIs
//   IQTree::doRandomNNIs   iqtree.cpp:1302-1339   the perturbation of the stochastic search
//   IQTree::doTreeSearch   iqtree.cpp:1834-2098   the stochastic loop (the snni branch) with the UFBoot stopping rule
// The decisions that need no likelihood are search_host.h; this file drives the tree and the engine.  The hot path of a
// search -- NNI evaluation and one-pass branch sweeps -- is evaluateNNIs[5]Batch and optimizeAllBranches: no kernel is
// added.  Per NNI step the engine sees: one submission for the vectors the listed branches read, ten (nni5) or two (nni1)
// batched solves over the listed branches only, one for the pending vectors of the sweep and one sweep; with UFBoot one
// update that reuses the per-pattern rows the evaluation left in the store (no row crosses to the host).
//
// DEVIATIONS from the reference (see also search_host.h): all internal branches are listed in internalBranches order
// (ascending node id), not in the reference's depth-first order; every branch is evaluated as (node1->id < node2->id),
// the orientation of the batched evaluators, where the reference passes getBranchesForNNI's orientation on; the model is
// taken as given (optimizeAllBranches(100) stands where the reference re-estimates the model for a better tree);
// doOneRandomNNI's coin flips are real coin flips (the reference draws random_int(1), which is always 0).
// The starting population: with numInitTrees == 0 (the default) the search starts from the one tree it was given; with
// numInitTrees > 0 doTreeSearch first restates createInitTrees + initCandidateTreeSet (iqtree.cpp:577-773): the given tree
// plus numInitTrees - 1 stepwise-addition parsimony trees built in lockstep (pars_forest_host.h) on the addition orders of
// iqsearch::parsimonyOrders (the reference shuffles with its own generator), duplicates dropped, each scored with
// optimizeAllBranches(2), the best numNNITrees optimised with optimizeNNI.  PLL's randomised visiting order inside its
// parsimony SPR is not restated (initSprRadius > 0 runs the project's own SPR rounds).
// The reference's moves hold neighbour iterators: when an earlier move of a step has re-hung an end of a later one
// (non-conflicting moves share no end, but may be adjacent), the later move swaps what its slots hold by then.  The moves here
// hold node ids, so a step looks the slots up on the evaluated tree and applies what they hold; the applied moves are
// reverted last first, the order that restores the tree also then (the reference reverts first to last -- the same thing
// for moves that do not touch).
// As in the reference, a step that is rolled back ends optimizeNNI: curScore goes back to the score before the step, so
// the gain of the step is 0 < 0.1.  The "apply only the best move" branch is kept as the reference has it.
#pragma once
#include <array>
#include <functional>
#include <string>
#include <vector>

#include "phylo_host.h"
#include "search_host.h"
#include "supertree_host.h"

namespace iqhost {

class TreeSearch {
public:
    typedef PhyloTree::NNIMove NNIMove;
    typedef iqsearch::BranchList BranchList;

    explicit TreeSearch(PhyloTree *tree);
    // over the super tree of an edge-linked partition model: `tree` is its topology (super), every edit and evaluation goes
    // to the super tree and all members (a candidate tree is re-read by every tree, PhyloSuperTree::readTreeString).
    // optimizeNNI, doRandomNNIs and doTreeSearch; partition rates and models are taken as given inside the loop, as the
    // model is on a plain tree.  With PhyloSuperTree::initUFBoot done the search feeds the group's UFBoot state (rows out of
    // the group's batched solves, saveNNITrees(moves), the current tree per step) and the correlation rule applies
    explicit TreeSearch(PhyloSuperTree *super_tree);

    // ---- parameters (the reference's defaults) ------------------------------------------------------------------------
    bool nni5 = true;             // params.nni5
    bool speednni = true;         // searchinfo.speednni: after the first step only branchesForNNI(applied) are evaluated
    bool batched = true;          // evaluateNNIs[5]Batch (LM_ALL_BRANCH); false: getBestNNIForBran branch by branch
    double loglh_epsilon = 0.001; // params.loglh_epsilon
    double modeps = 0.01;         // params.modeps
    int popSize = 5;              // params.popSize
    double initPS = 0.5;          // params.initPS
    uint64_t seed = 0;
    iqsearch::StopRule stop_rule; // SC_UNSUCCESS_ITERATION with 100; a bootstrap search uses SC_BOOTSTRAP_CORRELATION
    int step_iterations = 100;    // params.step_iterations
    int numInitTrees = 0;         // params.numInitTrees (the reference: 100); 0: start from the given tree alone
    int numNNITrees = 20;         // params.numNNITrees: the best initial trees that get an optimizeNNI
    int initSprRadius = 0;        // SPR rounds on the parsimony trees (ParsimonyForest::spr_radius); 0: none

    // ---- trace ----------------------------------------------------------------------------------------------------------
    struct NNIStep {
        BranchList branches;             // evaluated, each as (node1 < node2); empty for the step after a rollback
        bool all_branches = false;       // the list is every internal branch
        std::vector<NNIMove> evaluated;  // both candidates of every listed branch, in evaluation order
        std::vector<NNIMove> positive;   // the better candidate of a branch when above curScore + epsilon, sorted
        std::vector<NNIMove> applied;
        double score = 0.0;              // after the sweep (before a rollback puts the old score back)
        bool rolled_back = false;
        long submissions = 0;            // engine submissions of this step
    };
    struct Iteration {
        int iteration = 0;
        int parent = -1;                               // rank of the candidate tree that was read (-1: the starting tree)
        std::vector<std::array<int, 4>> random_nnis;   // node1, node2, bit1, bit2
        double perturb_score = 0.0;
        std::vector<NNIStep> steps;
        double score = 0.0;
        bool new_best = false;
        int nni_count = 0;
    };
    bool keep_trace = false;
    std::vector<Iteration> trace;
    // called at the end of every search iteration (the steps are filled only with keep_trace); a correlation computed in
    // this iteration is the last entry of correlation_log
    std::function<void(const TreeSearch &, const Iteration &)> on_iteration;
    std::vector<ufboot::SplitCounts> boot_splits;   // the snapshots of the correlation rule, every step_iterations / 2
    std::vector<std::pair<int, double>> correlation_log;   // (iteration, correlation) every step_iterations
    iqsearch::CandidateSet candidates;
    // numInitTrees > 0: the distinct starting trees in generation order (the given tree first), each with its string and
    // score after optimizeAllBranches(2), and how many parsimony trees repeated an earlier topology
    std::vector<iqsearch::CandidateTree> init_trees;
    int init_duplicates = 0;
    // the phases of the starting population, for a driver's log: 0 = the parsimony trees are built (count = distinct
    // starting trees, the given one included), 1 = their likelihoods come next (the same count), 2 = the NNI optimisation
    // of the best `count` of them comes next
    std::function<void(const TreeSearch &, int phase, int count)> on_init_phase;

    // ---- the search -------------------------------------------------------------------------------------------------------
    // on the current tree with curScore valid (computeLikelihood / optimizeAllBranches came last); returns curScore
    double optimizeNNI(int &nni_count, int &nni_steps, std::vector<NNIStep> *steps = nullptr);
    // numNNI random NNIs with the draws 1 + 3k (branch), 2 + 3k, 3 + 3k (coins) of `iteration`; all vectors go stale
    void doRandomNNIs(int numNNI, uint64_t iteration, std::vector<std::array<int, 4>> *done = nullptr);
    // returns the best score; the best candidate tree is loaded, its lengths as stored, its lnL recomputed.
    // With numInitTrees > 0 the M = min(numNNITrees, distinct trees) kept starting trees are the iterations 1 .. M (parent
    // = -1, each through on_iteration and the UFBoot feeding of optimizeNNI, as iteration 1 without them) and the
    // stochastic loop continues at M + 1; a fixed iteration count (SC_FIXED_ITERATION) counts the loop's iterations.
    double doTreeSearch();
    // refuses multifurcating trees, fewer than 4 taxa, trees without an engine, sharded engines and communicator ranks,
    // `batched` without LM_ALL_BRANCH, UFBoot together with mixtures, +ASC or the batched nni1 evaluation (it keeps no
    // per-pattern rows), numInitTrees > 0 on engines the parsimony calls refuse (anything but 4, 20 or 64 states):
    // throws std::runtime_error, the tree is not touched.  Every entry point calls it first.  On a super tree: multifurcations,
    // fewer than 4 taxa, no engines, UFBoot on a MEMBER (the super tree's own state lives on the group), numInitTrees > 0,
    // `batched` without setAllBranchMode, UFBoot with the batched nni1 evaluation
    void checkEligible(const char *who) const;

    PhyloTree *tree;
    PhyloSuperTree *stree = nullptr;
    double computeLikelihood();   // of the tree or of the super tree; curScore follows

private:
    // the tree edits and the sweep of a step, on the tree or on the super tree and its members
    void readTree(const std::string &newick, const std::vector<std::string> &names);
    void doNNI(const NNIMove &mv);
    void changeNNIBrans(const NNIMove &mv);
    double sweep();
    void restore(const std::vector<double> &lenvec);
    void evaluate(const BranchList &branches, bool all, std::vector<NNIMove> &moves);
    std::vector<std::string> leafNames() const;
};

}  // namespace iqhost
