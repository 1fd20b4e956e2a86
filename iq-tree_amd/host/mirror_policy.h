// mirror_policy.h -- private to the host mirror's translation units (phylo_host.cpp, phylo_nni.cpp).
// The adapter (include/iqhip_adapter.h) instantiated for this mirror.  The policy answers the adapter's questions
// about the tree types and wraps the engine calls with what only the mirror has: dry-run mode (CPU tests record
// plans without a device), the legacy caller-owned collective (allreduce_hook) and the call counters.
#pragma once
#include <math.h>

#include "../../include/iqhip_adapter.h"
#include "phylo_host.h"

namespace iqhost {

struct MirrorPolicy : iqhip_adapter::EngineCalls<MirrorPolicy, PhyloTree> {
    typedef iqhip_adapter::EngineCalls<MirrorPolicy, PhyloTree> Base;
    typedef iqhip_adapter::Plan<MirrorPolicy> Plan;
    typedef PhyloTree Tree;
    typedef PhyloNode Node;
    typedef PhyloNeighbor Neighbor;
    static Node *node(Neighbor *nb) { return nb->node; }
    static double length(Neighbor *nb) { return nb->length; }
    static void setLength(Neighbor *nb, double len) { nb->length = len; }
    static bool isLeaf(Node *n) { return n->isLeaf(); }
    static int degree(Node *n) { return n->degree(); }
    static int leafId(Node *n) { return n->id; }
    static int numNeighbors(Node *n) { return (int)n->neighbors.size(); }
    static Neighbor *neighborAt(Node *n, int k) { return n->neighbors[k]; }
    static Neighbor *findNeighbor(Node *at, Node *to) { return at->findNeighbor(to); }
    static int &computed(Neighbor *nb) { return nb->partial_lh_computed; }
    static double &scaleFactor(Neighbor *nb) { return nb->lh_scale_factor; }
    static uint64_t key(Neighbor *nb) { return nb->partial_lh; }
    static void stealBuffer(Neighbor *to, Neighbor *from) { to->partial_lh = from->partial_lh; from->partial_lh = 0; }
    static bool perNodeMode(Tree *t) { return t->lh_mem_save == LM_PER_NODE; }
    static bool heavyFirst(Tree *t) { return t->heavy_first; }
    static void ensureBuffers(Tree *t) { if (!t->central_partial_lh) t->initializeAllPartialLh(); }
    static void sync(Tree *t) { t->pushInputs(); }
    static iqhip_engine *engine(Tree *t) { return t->engine; }
    static void fail(Tree *, const char *what, const char *detail) {
        throw std::runtime_error(std::string(what) + ": " + detail);
    }
    static void countComputation(Tree *t) { t->num_partial_lh_computations++; }
    static bool &thetaComputed(Tree *t) { return t->theta_computed; }
    static Neighbor *currentIt(Tree *t) { return t->current_it; }
    static Neighbor *currentItBack(Tree *t) { return t->current_it_back; }
    static void clearReversePartialLh(Node *n, Node *dad) { n->clearReversePartialLh(dad); }
    static void setCurrent(Tree *t, Neighbor *it, Neighbor *back) { t->current_it = it; t->current_it_back = back; }
    static void optimizeSweep(Tree *t, const iqhip_sweep_step *steps, int nsteps, int max_steps, double diverge_frac,
                              double *sum_scale, iqhip_branch_result *results) {
        needEngine(t);
        Base::optimizeSweep(t, steps, nsteps, max_steps, diverge_frac, sum_scale, results);
    }
    static double minBranchLength(Tree *t) { return t->min_branch_length; }
    static double maxBranchLength(Tree *t) { return t->max_branch_length; }

    static void record(Tree *t, const Plan &plan) {
        t->last_plan.clear();
        for (size_t k = 0; k < plan.ops.size(); k++) {
            PlanOp p;
            p.dst = plan.dst[k];
            const bool binary = plan.dst[k] && plan.nkids(k) == 2;
            p.left = binary ? plan.kid(k, 0) : nullptr;
            p.right = binary ? plan.kid(k, 1) : nullptr;
            p.op = plan.ops[k];
            t->last_plan.push_back(p);
        }
    }
    static void needEngine(Tree *t) {
        if (!t->engine) throw std::runtime_error("HIP likelihood kernel selected but no engine attached");
    }
    static void updatePartials(Tree *t, Plan &plan, double *sum_scale) {
        record(t, plan);
        if (t->dry_run) return;
        needEngine(t);
        Base::updatePartials(t, plan, sum_scale);
        t->num_submissions++;
    }
    static double traverseLnl(Tree *t, Plan &plan, iqhip_branch_end a, iqhip_branch_end b, double len, double *sum_scale) {
        record(t, plan);
        const int nops = (int)plan.ops.size();
        if (t->dry_run) {
            if (!t->allreduce_hook) return 0.0;
            // CPU rehearsal of the caller-owned collective (tests, gloo): the hook receives a HOST vector laid out
            // like the device result {lnl, -, sum_scale[k]...}, fills in this rank's share and all-reduces it; no
            // likelihood arithmetic happens in this library.
            std::vector<double> res(2 + plan.ops.size(), 0.0);
            t->allreduce_hook(res.data(), (int)res.size(), t->allreduce_ctx);
            for (int k = 0; k < nops; k++) sum_scale[k] = res[2 + k];
            return res[0];
        }
        needEngine(t);
        double lnl;
        if (t->allreduce_hook) {  // caller-owned collective (the engine's own: iqhip_comm_init_rank / iqhip_create_sharded)
            chk(t, iqhip_traverse_lnl_async(t->engine, plan.empty() ? nullptr : plan.ops.data(), nops, a, b, len),
                "iqhip_traverse_lnl_async");
            const int nres = 2 + nops;
            t->allreduce_hook(iqhip_result_device_ptr(t->engine), nres, t->allreduce_ctx);
            std::vector<double> res(nres);
            chk(t, iqhip_result_read(t->engine, res.data(), nres), "iqhip_result_read");
            lnl = res[0];
            for (int k = 0; k < nops; k++) sum_scale[k] = res[2 + k];
        } else {
            lnl = Base::traverseLnl(t, plan, a, b, len, sum_scale);
        }
        t->num_submissions++;
        return lnl;
    }
    static void computeTheta(Tree *t, iqhip_branch_end a, iqhip_branch_end b) {
        if (t->dry_run) return;
        needEngine(t);
        Base::computeTheta(t, a, b);
    }
    static void derv(Tree *t, double len, double &df, double &ddf) {
        t->num_derv_calls++;
        if (t->dry_run) return;
        needEngine(t);
        if (t->allreduce_hook) {
            chk(t, iqhip_derv_async(t->engine, len), "iqhip_derv_async");
            t->allreduce_hook(iqhip_result_device_ptr(t->engine), 2, t->allreduce_ctx);
            double res[2];
            chk(t, iqhip_result_read(t->engine, res, 2), "iqhip_result_read");
            df = res[0];
            ddf = res[1];
            if (isnan(df) || isinf(df)) df = ddf = 0.0;  // phylokernel.h:647-651
        } else {
            Base::derv(t, len, df, ddf);
        }
    }
    static double lnlFromTheta(Tree *t, double len) {
        if (t->dry_run) return 0.0;
        needEngine(t);
        return Base::lnlFromTheta(t, len);
    }
    static double optimizeBranch(Tree *t, Plan &plan, iqhip_branch_end a, iqhip_branch_end b, double xguess, int max_steps,
                                 double *sum_scale, int *nsteps) {
        record(t, plan);
        needEngine(t);
        const double optx = Base::optimizeBranch(t, plan, a, b, xguess, max_steps, sum_scale, nsteps);
        t->num_submissions++;
        t->num_derv_calls += *nsteps;
        return optx;
    }
};

}  // namespace iqhost
