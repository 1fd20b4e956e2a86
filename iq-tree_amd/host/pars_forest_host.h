// pars_forest_host.h -- K stepwise-addition parsimony trees built in lockstep on ONE engine (the reference builds its
// starting trees under "#pragma omp parallel for", iqtree.cpp:591-601; the device form is one launch per step for all).
//
// The members are PhyloTree topology objects without an engine.  They share the owner's parsimony arena: iqhip_pars_init
// runs once per chunk with nvectors = members * (3 T - 6), the tips are slots 0 .. T-1 for everybody, member k owns the
// slots from T + k (3 T - 6) (pars_forest_plan.h) and never initialises the arena.  Per step cur = 3 .. T-1 the engine sees
//     ONE iqhip_pars_update              the ops of all members
//     ONE iqhip_pars_insert_scores_batch one segment per member, its branches in getBranches order
// and every member applies the surgery of phylotreepars.cpp:382-405 at its own first minimum.  After the last step: one
// merged update, ONE iqhip_pars_branch_scores over the branches of all members and fixNegativeBranch(true)'s Jukes-Cantor
// lengths per member.  For the same order a member's trace, score and Newick string equal what
// PhyloTree::computeParsimonyTree(order, trace) gives on that tree alone.
//
// spr_radius 1 .. 10 (0 = off): SPR rounds in lockstep.  Per round one merged update and ONE iqhip_pars_spr_scan over the
// jobs of every member that improved in the previous round; a member applies the first job of its job range that holds
// its minimum when that beats its current score (PhyloTree::optimizeParsimonySPR's rule) and drops out otherwise.
//
// Chunks: IQHIP_PARS_FOREST_CHUNK (trees per chunk, read per call) or, by default, as many trees as
// iqforest::kForestArenaBudget (1 GiB) holds.  Chunks are built one after the other; no result depends on the chunk size.
// The owner's tree is not touched; its parsimony state is dropped (the next parsimony call of the owner initialises its
// own arena again), its likelihood vectors stay.
// Out of scope: PLL's randomised visiting order inside its SPR, and sharded engines (refused by the engine calls).
#pragma once
#include <string>
#include <vector>

#include "pars_forest_plan.h"
#include "phylo_host.h"

namespace iqhost {

class ParsimonyForest {
public:
    explicit ParsimonyForest(PhyloTree *owner);

    int spr_radius = 0;
    bool keep_trace = false;

    struct Member {
        std::string newick, topology;   // with lengths; sortedTaxonIdString as a tree that READ the string gives it (root: taxon 0)
        int score = 0;
        int spr_rounds = 0;             // moves applied
        std::vector<PhyloTree::ParsStep> steps;   // with keep_trace
    };
    std::vector<Member> members;
    // engine calls of the last build(): updates, batch scans, branch-scores calls, SPR scans, arena initialisations
    struct Calls {
        long updates = 0, scans = 0, branch_scores = 0, spr_scans = 0, inits = 0;
    } calls;

    // orders: K permutations of 0 .. leafNum-1
    void build(const std::vector<std::vector<int>> &orders);

private:
    PhyloTree *owner;
    void buildChunk(const std::vector<std::vector<int>> &orders, size_t first, size_t count, double nsite,
                    const std::vector<std::string> &names);
    void sprRounds(std::vector<PhyloTree *> &trees, std::vector<int> &score, size_t first);
};

}  // namespace iqhost
