// pars_forest_host.cpp -- see pars_forest_host.h
#include "pars_forest_host.h"

#include <stdlib.h>

#include <memory>
#include <stdexcept>

namespace iqhost {

ParsimonyForest::ParsimonyForest(PhyloTree *t) : owner(t) {
    if (!t) throw std::runtime_error("ParsimonyForest: no tree");
}

void ParsimonyForest::build(const std::vector<std::vector<int>> &orders) {
    PhyloTree &o = *owner;
    if (!o.engine || o.dry_run) throw std::runtime_error("ParsimonyForest needs an attached engine");
    const int T = o.leafNum;
    if (T < 3) throw std::runtime_error("ParsimonyForest needs at least 3 taxa");
    if (spr_radius < 0 || spr_radius > IQHIP_PARS_SPR_MAX_RADIUS) throw std::runtime_error("ParsimonyForest: spr_radius outside 0 .. 10");
    for (const std::vector<int> &ord : orders)
        if ((int)ord.size() != T) throw std::runtime_error("ParsimonyForest: an addition order is not a permutation of the taxa");
    members.assign(orders.size(), Member());
    calls = Calls();
    if (orders.empty()) return;
    const int forced = iqforest::parseChunk(getenv("IQHIP_PARS_FOREST_CHUNK"));
    std::vector<std::string> names((size_t)T);
    for (int k = 0; k < T && k < (int)o.nodes.size(); k++)
        if (o.nodes[(size_t)k]) names[(size_t)k] = o.nodes[(size_t)k]->name;
    o.pushInputs();
    const int64_t nsites = o.parsInformativeSites();
    double nsite = 0.0;   // getAlnNSite()
    for (double f : o.ptn_freq) nsite += f;
    const int chunk = iqforest::chunkMembers((int)orders.size(), T, o.num_states, nsites, forced);
    // the owner's own arena is gone after the first chunk, whatever happens below
    o.pars_initialized = false;
    for (size_t first = 0; first < orders.size(); first += (size_t)chunk)
        buildChunk(orders, first, std::min((size_t)chunk, orders.size() - first), nsite, names);
}

void ParsimonyForest::buildChunk(const std::vector<std::vector<int>> &orders, size_t first, size_t count, double nsite,
                                 const std::vector<std::string> &names) {
    PhyloTree &o = *owner;
    const int T = o.leafNum;
    o.check(iqhip_pars_init(o.engine, o.pars_informative.data(), (int)iqforest::arenaVectors(T, (int)count), &o.pars_nsites), "iqhip_pars_init");
    calls.inits++;
    std::vector<std::unique_ptr<PhyloTree>> own(count);
    std::vector<PhyloTree *> trees(count);
    for (size_t k = 0; k < count; k++) {
        own[k].reset(new PhyloTree());
        PhyloTree *m = trees[k] = own[k].get();
        m->leafNum = T;
        m->num_states = o.num_states;
        m->min_branch_length = o.min_branch_length;
        m->pars_slot_base = iqforest::slotBase(T, (int)k);
        m->startParsimonyTree(orders[first + k].data(), names);
        m->assignParsSlots();
        m->pars_initialized = true;   // (the arena is the forest's: a member never initialises it)
        if (keep_trace) members[first + k].steps.clear();
    }
    std::vector<iqhip_pars_op> ops;
    std::vector<int> score(count, 0);
    std::vector<std::vector<PhyloNode *>> n1(count), n2(count);
    iqforest::Segments seg;
    std::vector<int32_t> ends, all_scores, best(count), best_score(count);
    for (int cur = 3; cur < T; cur++) {
        seg.clear();
        ops.clear();
        for (size_t k = 0; k < count; k++) {
            ends.clear();
            trees[k]->collectInsertScan(n1[k], n2[k], ops, ends);
            seg.add(ends, orders[first + k][(size_t)cur]);
        }
        if (!ops.empty()) {
            o.check(iqhip_pars_update(o.engine, ops.data(), (int)ops.size()), "iqhip_pars_update");
            calls.updates++;
        }
        if (keep_trace) all_scores.resize(seg.ends.size() / 2);
        o.check(iqhip_pars_insert_scores_batch(o.engine, seg.ends.data(), seg.seg_start.data(), seg.nseg(), seg.taxon.data(),
                                               keep_trace ? all_scores.data() : nullptr, best.data(), best_score.data()),
                "iqhip_pars_insert_scores_batch");
        calls.scans++;
        for (size_t k = 0; k < count; k++) {
            score[k] = best_score[k];
            if (keep_trace) {
                PhyloTree::ParsStep step;
                for (size_t q = 0; q < n1[k].size(); q++) {
                    step.node1.push_back(n1[k][q]->id);
                    step.node2.push_back(n2[k][q]->id);
                    step.score.push_back(all_scores[(size_t)seg.seg_start[k] + q]);
                }
                step.chosen = best[k];
                step.best_score = best_score[k];
                members[first + k].steps.push_back(step);
            }
            trees[k]->insertParsimonyTaxon(n1[k][(size_t)best[k]], n2[k][(size_t)best[k]], orders[first + k][(size_t)cur], cur);
        }
    }
    // fixNegativeBranch(true) of every member: one update, one branch-scores call, the lengths on the host
    ops.clear();
    std::vector<std::vector<PhyloNeighbor *>> all(count);
    std::vector<std::vector<PhyloNode *>> from(count);
    std::vector<size_t> at(count + 1, 0);
    ends.clear();
    for (size_t k = 0; k < count; k++) {
        PhyloTree *m = trees[k];
        m->finishParsimonyTree();
        m->collectAllParsOps(ops);
        m->fixBranchList(all[k], from[k]);
        for (size_t q = 0; q < all[k].size(); q++) {
            ends.push_back(all[k][q]->pars_slot);
            ends.push_back(all[k][q]->node->findNeighbor(from[k][q])->pars_slot);
        }
        at[k + 1] = ends.size() / 2;
    }
    if (!ops.empty()) {
        o.check(iqhip_pars_update(o.engine, ops.data(), (int)ops.size()), "iqhip_pars_update");
        calls.updates++;
    }
    std::vector<int32_t> tree_score(ends.size() / 2), subst(ends.size() / 2);
    o.check(iqhip_pars_branch_scores(o.engine, ends.data(), (int)(ends.size() / 2), tree_score.data(), subst.data()), "iqhip_pars_branch_scores");
    calls.branch_scores++;
    for (size_t k = 0; k < count; k++) {
        trees[k]->applyParsLengths(all[k], from[k], subst.data() + at[k], true, nsite);
        if (T == 3) score[k] = tree_score[at[k]];   // (no step ran: the score at the first branch is the tree's)
    }
    if (spr_radius > 0) sprRounds(trees, score, first);
    for (size_t k = 0; k < count; k++) {
        Member &mb = members[first + k];
        mb.newick = trees[k]->getTreeString();
        // the key as the tree gives it once its string is read back: the reader roots at taxon 0, a member at its first taxon
        PhyloNode *own_root = trees[k]->root;
        trees[k]->root = trees[k]->nodes[0];
        mb.topology = trees[k]->sortedTaxonIdString();
        trees[k]->root = own_root;
        mb.score = score[k];
    }
}

void ParsimonyForest::sprRounds(std::vector<PhyloTree *> &trees, std::vector<int> &score, size_t first) {
    PhyloTree &o = *owner;
    std::vector<size_t> active;
    for (size_t k = 0; k < trees.size(); k++) active.push_back(k);
    std::vector<iqhip_pars_op> ops;
    std::vector<iqhip_pars_spr_job> jobs, mj;
    std::vector<iqhip_pars_spr_step> steps, ms;
    std::vector<PhyloTree::SprMove> moves, mm;
    while (!active.empty()) {
        ops.clear();
        jobs.clear();
        steps.clear();
        moves.clear();
        std::vector<size_t> scanned, job_at(1, 0);
        for (size_t k : active) {
            trees[k]->collectAllParsOps(ops);
            trees[k]->collectSprJobs(spr_radius, mj, ms, mm);
            if (mj.empty()) continue;   // (4 taxa or fewer branches than a move needs: the member drops out)
            const int off = (int)steps.size();
            for (iqhip_pars_spr_job j : mj) {
                j.first_step += off;
                jobs.push_back(j);
            }
            steps.insert(steps.end(), ms.begin(), ms.end());
            moves.insert(moves.end(), mm.begin(), mm.end());
            scanned.push_back(k);
            job_at.push_back(jobs.size());
        }
        if (scanned.empty()) break;
        if (!ops.empty()) {
            o.check(iqhip_pars_update(o.engine, ops.data(), (int)ops.size()), "iqhip_pars_update");
            calls.updates++;
        }
        std::vector<int32_t> sc(steps.size()), best_step(jobs.size()), best_score(jobs.size());
        int32_t best_job = -1;
        o.check(iqhip_pars_spr_scan(o.engine, jobs.data(), (int)jobs.size(), steps.data(), (int)steps.size(), sc.data(),
                                    best_step.data(), best_score.data(), &best_job),
                "iqhip_pars_spr_scan");
        calls.spr_scans++;
        active.clear();
        for (size_t a = 0; a < scanned.size(); a++) {
            const size_t k = scanned[a], j0 = job_at[a], j1 = job_at[a + 1];
            const int before = sc[(size_t)jobs[j0].first_step];
            size_t bj = j0;
            for (size_t j = j0; j < j1; j++) {   // every scored root step is the tree as it stands
                if (sc[(size_t)jobs[j].first_step] != before)
                    throw std::runtime_error("ParsimonyForest: the prune points disagree about the score of the current tree");
                if (best_score[j] < best_score[bj]) bj = j;   // (strict: the first job that holds the minimum)
            }
            if (best_step[bj] < 0) throw std::runtime_error("ParsimonyForest: nothing was scored");
            score[k] = before;
            if (best_score[bj] < before) {
                const PhyloTree::SprMove &mv = moves[(size_t)jobs[bj].first_step + (size_t)best_step[bj]];
                if (mv.depth < 1) throw std::runtime_error("ParsimonyForest: a root step beats the current tree");
                trees[k]->applySprMove(mv);
                score[k] = best_score[bj];
                members[first + k].spr_rounds++;
                active.push_back(k);
            }
        }
    }
}

}  // namespace iqhost
