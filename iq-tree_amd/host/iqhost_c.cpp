// iqhost_c.cpp -- flat C view of iqhost::PhyloTree for ctypes (tests, bench.py, smoke()).
// Not part of the drop-in boundary (that is include/iqhip.h); this is how the Python side of
// the repository drives the same call sequence the reference's C++ callers use.
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <array>
#include <memory>
#include <new>

#include <string>
#include <vector>

#include "bfgs_host.h"
#include "brent_host.h"
#include "model_opt_host.h"
#include "pars_forest_host.h"
#include "phylo_host.h"
#include "search_host.h"
#include "supertree_host.h"
#include "tree_search_host.h"
#include "ufboot_splits.h"

using namespace iqhost;

static thread_local std::string g_host_err;

#define IQHOST_TRY(...)                    \
    try {                                  \
        __VA_ARGS__;                       \
        return 0;                          \
    } catch (const std::exception &ex) {   \
        g_host_err = ex.what();            \
        return 1;                          \
    }

static PhyloNeighbor *nei(PhyloTree *t, int from, int to) {
    if (from < 0 || to < 0 || from >= t->nodeNum || to >= t->nodeNum) throw std::runtime_error("bad node id");
    PhyloNeighbor *n = t->nodes[from]->findNeighbor(t->nodes[to]);
    if (!n) throw std::runtime_error("nodes are not adjacent");
    return n;
}

extern "C" {

const char *iqhost_last_error(void) { return g_host_err.c_str(); }

int iqhost_create(void **out, const char *newick, const char **names, int nnames) {
    *out = nullptr;
    PhyloTree *t = nullptr;
    try {
        t = new PhyloTree();
        std::vector<std::string> nm;
        for (int i = 0; i < nnames; i++) nm.push_back(names[i]);
        t->readTreeString(newick, nm);
        *out = t;
        return 0;
    } catch (const std::exception &ex) {
        g_host_err = ex.what();
        delete t;
        return 1;
    }
}
void iqhost_destroy(void *h) { delete (PhyloTree *)h; }

int iqhost_set_alignment(void *h, int nstates, int seq_type, int64_t nptn, const uint8_t *states,
                         const double *freq, const double *invar) {
    IQHOST_TRY(((PhyloTree *)h)->setAlignment(nstates, (SeqType)seq_type, nptn, states, freq, invar));
}
int iqhost_set_ptn_freq(void *h, const double *f) { IQHOST_TRY(((PhyloTree *)h)->setPtnFreq(f)); }
int iqhost_set_ptn_invar(void *h, const double *v) { IQHOST_TRY(((PhyloTree *)h)->setPtnInvar(v)); }
int iqhost_set_ascertainment(void *h, int64_t n_unobserved, double nsites) {
    IQHOST_TRY(((PhyloTree *)h)->setAscertainment(n_unobserved, nsites));
}
int iqhost_set_model(void *h, int ncat, const double *eval, const double *evec, const double *inv_evec,
                     const double *rates, const double *props) {
    IQHOST_TRY(((PhyloTree *)h)->setModel(ncat, eval, evec, inv_evec, rates, props));
}
int iqhost_set_mixture_model(void *h, int nclass, int ncat, const int *cat_class, const double *eval, const double *evec,
                             const double *inv_evec, const double *rates, const double *props) {
    IQHOST_TRY(((PhyloTree *)h)->setMixtureModel(nclass, ncat, cat_class, eval, evec, inv_evec, rates, props));
}
int iqhost_set_mem_mode(void *h, int lm) {
    IQHOST_TRY(((PhyloTree *)h)->lh_mem_save = (LhMemSave)lm);
}
int iqhost_set_kernel(void *h, int lk) { IQHOST_TRY(((PhyloTree *)h)->setLikelihoodKernel((LikelihoodKernel)lk)); }
int iqhost_attach_engine(void *h, int device) { IQHOST_TRY(((PhyloTree *)h)->attachEngine(device)); }
int iqhost_attach_engine_sharded(void *h, const int *device_ids, int ndev, int reduce_mode) {
    IQHOST_TRY(((PhyloTree *)h)->attachEngineSharded(device_ids, ndev, reduce_mode));
}
int iqhost_attach_comm(void *h, int nranks, int rank, const void *unique_id) {
    IQHOST_TRY(((PhyloTree *)h)->attachComm(nranks, rank, unique_id));
}
int iqhost_set_device_newton(void *h, int on) { IQHOST_TRY(((PhyloTree *)h)->device_newton = on != 0); }
int iqhost_set_device_sweep(void *h, int on) { IQHOST_TRY(((PhyloTree *)h)->device_sweep = on != 0); }
long iqhost_num_derv_calls(void *h) { return ((PhyloTree *)h)->num_derv_calls; }
int iqhost_set_heavy_first(void *h, int on) { IQHOST_TRY(((PhyloTree *)h)->heavy_first = on != 0); }
int iqhost_set_dry_run(void *h, int on) { IQHOST_TRY(((PhyloTree *)h)->setDryRun(on != 0)); }
void *iqhost_engine(void *h) { return ((PhyloTree *)h)->engine; }
int iqhost_set_allreduce_hook(void *h, void (*fn)(void *, int, void *), void *ctx) {
    IQHOST_TRY(((PhyloTree *)h)->setAllReduceHook(fn, ctx));
}

int iqhost_num_nodes(void *h) { return ((PhyloTree *)h)->nodeNum; }
int iqhost_num_leaves(void *h) { return ((PhyloTree *)h)->leafNum; }
int iqhost_root(void *h) { return ((PhyloTree *)h)->root->id; }
int iqhost_state_unknown(void *h) { return ((PhyloTree *)h)->STATE_UNKNOWN; }
int iqhost_tip_partial_lh(void *h, double *out) {
    PhyloTree *t = (PhyloTree *)h;
    memcpy(out, t->tip_partial_lh.data(), sizeof(double) * t->tip_partial_lh.size());
    return 0;
}
// neighbours of `node` in stored order; returns the degree
int iqhost_neighbors(void *h, int node, int *out_ids, double *out_len, int cap) {
    PhyloTree *t = (PhyloTree *)h;
    if (node < 0 || node >= t->nodeNum) return -1;
    int d = t->nodes[node]->degree();
    for (int i = 0; i < d && i < cap; i++) {
        out_ids[i] = t->nodes[node]->neighbors[i]->node->id;
        if (out_len) out_len[i] = t->nodes[node]->neighbors[i]->length;
    }
    return d;
}
int iqhost_set_branch_length(void *h, int a, int b, double len, int clear_reverse) {
    IQHOST_TRY({
        PhyloTree *t = (PhyloTree *)h;
        nei(t, a, b)->length = len;
        nei(t, b, a)->length = len;
        if (clear_reverse) {
            t->nodes[a]->clearReversePartialLh(t->nodes[b]);
            t->nodes[b]->clearReversePartialLh(t->nodes[a]);
        }
        t->theta_computed = false;
    });
}
// state of the neighbour `from -> to`
int iqhost_neighbor_info(void *h, int from, int to, int *computed, uint64_t *key, double *lh_scale_factor,
                         double *length) {
    IQHOST_TRY({
        PhyloNeighbor *n = nei((PhyloTree *)h, from, to);
        if (computed) *computed = n->partial_lh_computed;
        if (key) *key = n->partial_lh;
        if (lh_scale_factor) *lh_scale_factor = n->lh_scale_factor;
        if (length) *length = n->length;
    });
}

int iqhost_initialize_all_partial_lh(void *h) { IQHOST_TRY(((PhyloTree *)h)->initializeAllPartialLh()); }
int iqhost_clear_all_partial_lh(void *h) { IQHOST_TRY(((PhyloTree *)h)->clearAllPartialLH()); }
// hot loop 1 in one call: clearAllPartialLH(); computeLikelihood()  (model/modelgtr.cpp:510-518)
int iqhost_clear_and_compute_likelihood(void *h, double *lnl) {
    IQHOST_TRY({
        PhyloTree *t = (PhyloTree *)h;
        t->clearAllPartialLH();
        *lnl = t->computeLikelihood(nullptr);
    });
}
int iqhost_compute_likelihood(void *h, double *lnl, double *pattern_lh) {
    IQHOST_TRY(*lnl = ((PhyloTree *)h)->computeLikelihood(pattern_lh));
}
// current_it = from->to as chosen by the last computeLikelihood / optimizeOneBranch
int iqhost_current_branch(void *h, int *from, int *to) {
    PhyloTree *t = (PhyloTree *)h;
    if (!t->current_it) return 1;
    *to = t->current_it->node->id;
    *from = t->current_it_back->node->id;
    return 0;
}
int iqhost_compute_partial(void *h, int dad, int node) {
    IQHOST_TRY({
        PhyloTree *t = (PhyloTree *)h;
        t->computePartialLikelihood(nei(t, dad, node), t->nodes[dad]);
    });
}
int iqhost_compute_branch(void *h, int dad, int node, double *lnl) {
    IQHOST_TRY({
        PhyloTree *t = (PhyloTree *)h;
        *lnl = t->computeLikelihoodBranch(nei(t, dad, node), t->nodes[dad]);
    });
}
int iqhost_compute_derv(void *h, int dad, int node, double *df, double *ddf) {
    IQHOST_TRY({
        PhyloTree *t = (PhyloTree *)h;
        t->current_it = nei(t, dad, node);
        t->current_it_back = nei(t, node, dad);
        t->computeLikelihoodDerv(t->current_it, t->nodes[dad], *df, *ddf);
    });
}
int iqhost_reset_theta(void *h) { IQHOST_TRY(((PhyloTree *)h)->theta_computed = false); }
int iqhost_compute_from_buffer(void *h, double *lnl) {
    IQHOST_TRY(*lnl = ((PhyloTree *)h)->computeLikelihoodFromBuffer());
}
int iqhost_optimize_one_branch(void *h, int a, int b, int clear_lh, int max_nr_step, double *new_len) {
    IQHOST_TRY({
        PhyloTree *t = (PhyloTree *)h;
        t->optimizeOneBranch(t->nodes[a], t->nodes[b], clear_lh != 0, max_nr_step);
        *new_len = nei(t, a, b)->length;
    });
}
int iqhost_optimize_all_branches(void *h, int iterations, double tolerance, int max_nr_step, double *lnl) {
    IQHOST_TRY(*lnl = ((PhyloTree *)h)->optimizeAllBranches(iterations, tolerance, max_nr_step));
}
// both NNI moves around the internal branch (a, b): out[cnt*8 + {0:newloglh, 1:node1_nei, 2:node2_nei, 3..7:newLen}]
int iqhost_nni_for_branch(void *h, int a, int b, int nni5, double *out) {
    IQHOST_TRY({
        PhyloTree *t = (PhyloTree *)h;
        PhyloTree::NNIMove mv[2];
        t->getBestNNIForBran(t->nodes[a], t->nodes[b], nni5 != 0, mv);
        for (int c = 0; c < 2; c++) {
            out[c * 8 + 0] = mv[c].newloglh;
            out[c * 8 + 1] = mv[c].node1_nei;
            out[c * 8 + 2] = mv[c].node2_nei;
            for (int k = 0; k < 5; k++) out[c * 8 + 3 + k] = mv[c].newLen[k];
        }
    });
}
int iqhost_set_branch_bounds(void *h, double minlen, double maxlen) {
    IQHOST_TRY({
        ((PhyloTree *)h)->min_branch_length = minlen;
        ((PhyloTree *)h)->max_branch_length = maxlen;
    });
}
int iqhost_tree_string(void *h, char *out, int cap) {
    std::string s = ((PhyloTree *)h)->getTreeString();
    if ((int)s.size() + 1 > cap) return (int)s.size() + 1;
    memcpy(out, s.c_str(), s.size() + 1);
    return 0;
}

int iqhost_fetch_scale_num(void *h, int from, int to, int16_t *out) {
    IQHOST_TRY({
        PhyloTree *t = (PhyloTree *)h;
        t->fetchScaleNum(nei(t, from, to), out);
    });
}
int iqhost_fetch_partial(void *h, int from, int to, double *out) {
    IQHOST_TRY({
        PhyloTree *t = (PhyloTree *)h;
        t->fetchPartialLh(nei(t, from, to), out);
    });
}
int iqhost_fetch_pattern_lh(void *h, double *out) { IQHOST_TRY(((PhyloTree *)h)->fetchPatternLh(out)); }
int iqhost_compute_pattern_likelihood(void *h, double *out) { IQHOST_TRY(((PhyloTree *)h)->computePatternLikelihood(out)); }
int iqhost_compute_pattern_lh_cat(void *h, double *out) { IQHOST_TRY(((PhyloTree *)h)->computePatternLhCat(out)); }
// ---- Brent's minimiser as a state machine (brent_host.h); state: IQHOST_BRENT_STATE_BYTES opaque bytes, 8-byte aligned
#define IQHOST_BRENT_STATE_BYTES 512
static_assert(sizeof(BrentMachine) <= IQHOST_BRENT_STATE_BYTES, "BrentMachine must fit its opaque state");
int iqhost_brent_state_bytes(void) { return IQHOST_BRENT_STATE_BYTES; }
int iqhost_brent_init(void *state, double xmin, double xguess, double xmax, double tolerance, double *first_x) {
    IQHOST_TRY({
        if (!state || !first_x) throw std::runtime_error("iqhost_brent_init: null argument");
        if (!(xmin <= xmax) || xguess != xguess || !(tolerance > 0.0)) throw std::runtime_error("iqhost_brent_init: bad bounds");
        *first_x = (new (state) BrentMachine())->init(xmin, xguess, xmax, tolerance);
    });
}
int iqhost_brent_update(void *state, double f, double *next_x, int *done) {
    IQHOST_TRY({
        if (!state || !next_x || !done) throw std::runtime_error("iqhost_brent_update: null argument");
        BrentMachine *m = (BrentMachine *)state;
        *next_x = m->update(f);
        *done = m->done ? 1 : 0;
    });
}
int iqhost_brent_result(const void *state, double *optx, double *fx, int *nevals) {
    IQHOST_TRY({
        if (!state || !optx || !fx || !nevals) throw std::runtime_error("iqhost_brent_result: null argument");
        const BrentMachine *m = (const BrentMachine *)state;
        if (!m->done) throw std::runtime_error("iqhost_brent_result: the search has not finished");
        *optx = m->optx;
        *fx = m->fx_opt;
        *nevals = m->nevals;
    });
}
// ---- the reference's BFGS as a state machine (bfgs_host.h).  bound_check: NULL or ndim ints
int iqhost_bfgs_create(void **out, int ndim, const double *guess, const double *lower, const double *upper, const int *bound_check,
                       double gtol) {
    IQHOST_TRY({
        if (!out || !guess || !lower || !upper) throw std::runtime_error("iqhost_bfgs_create: null argument");
        *out = nullptr;
        if (ndim < 1) throw std::runtime_error("iqhost_bfgs_create: at least one dimension");
        std::unique_ptr<bool[]> bc(new bool[(size_t)ndim]);
        for (int i = 0; i < ndim; i++) bc[i] = bound_check && bound_check[i] != 0;
        BfgsMachine *m = new BfgsMachine();
        try {
            m->init(ndim, guess, lower, upper, bc.get(), gtol);
        } catch (...) {
            delete m;
            throw;
        }
        *out = m;
    });
}
void iqhost_bfgs_destroy(void *m) { delete (BfgsMachine *)m; }
// *kind: BfgsMachine::Request (0 stencil, 1 single, 2 done); *npoints: the points of the pending request
int iqhost_bfgs_request(const void *h, int *kind, int *npoints) {
    IQHOST_TRY({
        const BfgsMachine *m = (const BfgsMachine *)h;
        if (!m || !kind || !npoints) throw std::runtime_error("iqhost_bfgs_request: null argument");
        *kind = (int)m->request;
        *npoints = m->npoints();
    });
}
// points: npoints * ndim doubles; steps: NULL or ndim (the stencil's h)
int iqhost_bfgs_points(const void *h, double *points, double *steps) {
    IQHOST_TRY({
        const BfgsMachine *m = (const BfgsMachine *)h;
        if (!m || !points) throw std::runtime_error("iqhost_bfgs_points: null argument");
        memcpy(points, m->points.data(), sizeof(double) * m->points.size());
        if (steps) memcpy(steps, m->h.data(), sizeof(double) * m->h.size());
    });
}
int iqhost_bfgs_update(void *h, const double *values, int nvalues) {
    IQHOST_TRY({
        BfgsMachine *m = (BfgsMachine *)h;
        if (!m || !values) throw std::runtime_error("iqhost_bfgs_update: null argument");
        if (m->request == BfgsMachine::DONE) throw std::runtime_error("iqhost_bfgs_update: the search has finished");
        if (nvalues != m->npoints()) throw std::runtime_error("iqhost_bfgs_update: one value per requested point");
        m->update(values);
    });
}
// x, gradient: ndim each (gradient: of the last stencil); counts: {iter, stencils, singles}
int iqhost_bfgs_result(const void *h, double *x, double *fret, double *gradient, int *counts) {
    IQHOST_TRY({
        const BfgsMachine *m = (const BfgsMachine *)h;
        if (!m || !x || !fret || !counts) throw std::runtime_error("iqhost_bfgs_result: null argument");
        memcpy(x, m->x.data(), sizeof(double) * m->x.size());
        if (gradient) memcpy(gradient, m->g.data(), sizeof(double) * m->g.size());
        *fret = m->fret;
        counts[0] = m->iter;
        counts[1] = m->nstencils;
        counts[2] = m->nsingles;
    });
}
// ---- model parameter estimation (model_opt_host.h).  tree: an iqhost tree with its engine attached; aln: an iqaln handle;
// batch: 0 every point on the main tree, 1 stencils batched up to BATCH_MAX_PATTERNS patterns, 2 batched at every size
int iqhost_modelopt_create(void **out, void *tree, void *aln, const char *model, int batch) {
    IQHOST_TRY({
        if (!out || !tree || !aln || !model) throw std::runtime_error("iqhost_modelopt_create: null argument");
        *out = nullptr;
        ModelOptimizer *o = new ModelOptimizer(*(PhyloTree *)tree, *(const Alignment *)aln, parseModelString(model, true), batch != 0);
        if (batch == 2) o->batch_max_patterns = INT64_MAX;   // batched at every size
        *out = o;
    });
}
void iqhost_modelopt_destroy(void *h) { delete (ModelOptimizer *)h; }
// what: 0 optimizeModel, 1 optimizeRates, 2 optimizeParametersOnly, 3 optimizeParameters (fixed_len, logl_epsilon used)
int iqhost_modelopt_run(void *h, int what, int fixed_len, double logl_epsilon, double gradient_epsilon, double *lnl, int *rounds) {
    IQHOST_TRY({
        ModelOptimizer *o = (ModelOptimizer *)h;
        if (!o || !lnl) throw std::runtime_error("iqhost_modelopt_run: null argument");
        if (what == 0) *lnl = o->optimizeModel(gradient_epsilon);
        else if (what == 1) *lnl = o->optimizeRates(gradient_epsilon);
        else if (what == 2) *lnl = o->optimizeParametersOnly(gradient_epsilon);
        else if (what == 3) *lnl = o->optimizeParameters(fixed_len != 0, logl_epsilon, gradient_epsilon, false);
        else throw std::runtime_error("iqhost_modelopt_run: unknown step");
        if (rounds) *rounds = o->rounds;
    });
}
// which: 0 the model string with the estimates, 1 the writeInfo lines
int iqhost_modelopt_string(void *h, int which, char *buf, int cap) {
    IQHOST_TRY({
        const ModelOptimizer *o = (const ModelOptimizer *)h;
        if (!o || !buf || cap < 1) throw std::runtime_error("iqhost_modelopt_string: null argument");
        const std::string s = which == 0 ? o->modelString() : o->writeInfo();
        if ((int)s.size() + 1 > cap) throw std::runtime_error("iqhost_modelopt_string: buffer too small");
        memcpy(buf, s.c_str(), s.size() + 1);
    });
}
// vals: {nparams, alpha, p_invar, has_gamma, has_invar}; params: up to cap rate parameters
int iqhost_modelopt_values(void *h, double *vals, double *params, int cap) {
    IQHOST_TRY({
        const ModelOptimizer *o = (const ModelOptimizer *)h;
        if (!o || !vals) throw std::runtime_error("iqhost_modelopt_values: null argument");
        const ModelSpec &s = o->getSpec();
        const int k = ModelOptimizer::numParams(s);
        vals[0] = k;
        vals[1] = s.gamma_shape;
        vals[2] = s.p_invar;
        vals[3] = s.has_gamma;
        vals[4] = s.has_invar;
        for (int i = 0; i < k && i < cap && params; i++) params[i] = s.params[(size_t)i];
    });
}
int iqhost_modelopt_trace_len(void *h) { return h ? (int)((ModelOptimizer *)h)->trace.size() : 0; }
// what: 16 bytes; ints: {requests, stencils, stencil_traversals, single_traversals, stencils_redone, K, ndim of the first
// stencil}; lnl: {before, after}; x0 / grad0 / h0: ndim each, values0: ndim + 1 (NULL: not wanted; cap doubles each)
int iqhost_modelopt_trace_row(void *h, int k, char *what, int *ints, double *lnl, double *x0, double *grad0, double *h0,
                              double *values0, int cap) {
    IQHOST_TRY({
        const ModelOptimizer *o = (const ModelOptimizer *)h;
        if (!o || k < 0 || k >= (int)o->trace.size() || !what || !ints || !lnl) throw std::runtime_error("iqhost_modelopt_trace_row: bad argument");
        const ModelOptimizer::Call &c = o->trace[(size_t)k];
        snprintf(what, 16, "%s", c.what.c_str());
        ints[0] = c.requests;
        ints[1] = c.stencils;
        ints[2] = c.stencil_traversals;
        ints[3] = c.single_traversals;
        ints[4] = c.stencils_redone;
        ints[5] = c.K;
        ints[6] = (int)c.x0.size();
        lnl[0] = c.lnl_before;
        lnl[1] = c.lnl_after;
        auto put = [&](double *dst, const std::vector<double> &src) {
            if (dst) memcpy(dst, src.data(), sizeof(double) * std::min((size_t)cap, src.size()));
        };
        put(x0, c.x0);
        put(grad0, c.grad0);
        put(h0, c.h0);
        put(values0, c.values0);
    });
}
// no device: the refusals of the optimiser, the number of free rate parameters, their bounds, the candidates per traversal
// and whether alpha / p-inv are estimated.  out: {ndim, K, lower, upper, has_gamma, has_invar, alpha bounds 2, p-inv lower}
int iqhost_modelopt_describe(const char *model, int nstates, double *out) {
    IQHOST_TRY({
        if (!model || !out) throw std::runtime_error("iqhost_modelopt_describe: null argument");
        const ModelSpec s = parseModelString(model, true);
        ModelOptimizer::checkScope(s);
        const int k = ModelOptimizer::numParams(s);
        out[0] = k;
        out[1] = ModelOptimizer::candidatesPerTraversal(k, s.ncat, nstates);
        out[2] = MIN_RATE;
        out[3] = MAX_RATE;
        out[4] = s.has_gamma;
        out[5] = s.has_invar;
        out[6] = MIN_GAMMA_SHAPE;
        out[7] = MAX_GAMMA_SHAPE;
        out[8] = MIN_PINVAR;
    });
}
int iqhost_free_rate_start(int k, double *props, double *rates) {
    IQHOST_TRY({
        std::vector<double> p;
        std::vector<double> r;
        PhyloTree::freeRateStart(k, p, r);
        memcpy(props, p.data(), sizeof(double) * p.size());
        memcpy(rates, r.data(), sizeof(double) * r.size());
    });
}
// one E-step on the current branch; W: NULL or nptn * ncat doubles [ptn][cat]
int iqhost_em_posteriors(void *h, double *W, double *cat_sum) {
    IQHOST_TRY({
        PhyloTree *t = (PhyloTree *)h;
        t->emPosteriors(cat_sum);
        if (W && iqhip_em_fetch_posteriors(t->engine, W) != 0) throw std::runtime_error(iqhip_last_error());
    });
}
int iqhost_em_objective(void *h, int a, int b, double *f, int64_t *floored) {
    IQHOST_TRY({
        PhyloTree *t = (PhyloTree *)h;
        t->emObjective(nei(t, a, b), t->nodes[a], f, floored);
    });
}
int iqhost_site_rates(void *h, double *rates, int *cats) {
    IQHOST_TRY({
        PhyloTree *t = (PhyloTree *)h;
        std::vector<double> r;
        std::vector<int> c;
        t->computePatternRates(r, c);
        memcpy(rates, r.data(), sizeof(double) * r.size());
        memcpy(cats, c.data(), sizeof(int) * c.size());
    });
}
// props / rates: ncat each; trace: NULL or rows of 2 + 4 ncat doubles {lnl_before, rounds, props, rates, evals, floored},
// at most trace_cap rows (ncat suffice); *nsteps = the EM steps taken
int iqhost_optimize_free_rates_em(void *h, double *props, double *rates, double *lnl, int *nsteps, double *trace, int trace_cap) {
    IQHOST_TRY({
        PhyloTree *t = (PhyloTree *)h;
        std::vector<PhyloTree::EmStep> steps;
        *lnl = t->optimizeFreeRatesEM(&steps);
        const size_t C = (size_t)t->ncat;
        memcpy(props, t->getProps().data(), sizeof(double) * C);
        memcpy(rates, t->getRates().data(), sizeof(double) * C);
        *nsteps = (int)steps.size();
        for (size_t k = 0; k < steps.size() && trace && (int)k < trace_cap; k++) {
            double *row = trace + k * (2 + 4 * C);
            row[0] = steps[k].lnl_before;
            row[1] = steps[k].rounds;
            for (size_t c = 0; c < C; c++) {
                row[2 + c] = steps[k].props[c];
                row[2 + C + c] = steps[k].rates[c];
                row[2 + 2 * C + c] = steps[k].evals[c];
                row[2 + 3 * C + c] = (double)steps[k].floored[c];
            }
        }
    });
}
// ---- EM for mixture class weights.  out / post / state_freq: NULL or [ptn][class] / [ptn][class] / [ptn][state]
int iqhost_mix_class_lh(void *h, double *out) {
    IQHOST_TRY(((PhyloTree *)h)->computePatternLhCat(PhyloTree::WSL_MIXTURE, out));
}
int iqhost_mix_weights_em(void *h, int max_steps, double *weights, double *p_invar, int *nsteps, int *converged, double *trace) {
    IQHOST_TRY(((PhyloTree *)h)->mixWeightsEM(max_steps, weights, p_invar, nsteps, converged, trace));
}
// on the matrix of the last iqhost_mix_class_lh
int iqhost_mix_posteriors(void *h, const double *class_freq, double *post, double *state_freq) {
    IQHOST_TRY({
        PhyloTree *t = (PhyloTree *)h;
        if (!t->engine) throw std::runtime_error("no engine");
        t->syncInputs();   // (as mixWeightsEM: a pending model change must reach the engine before it judges the matrix)
        if (iqhip_mix_posteriors(t->engine, class_freq, post, state_freq) != 0) throw std::runtime_error(iqhip_last_error());
    });
}
int iqhost_pattern_state_freq(void *h, const double *class_freq, double *state_freq) {
    IQHOST_TRY(((PhyloTree *)h)->computePatternStateFreq(class_freq, state_freq));
}
// weights: nmixture, props: ncat (the component weights re-sent to the engine); p_invar: NULL or in/out
int iqhost_optimize_mixture_weights(void *h, double *p_invar, double *weights, double *props, double *lnl, int *nsteps,
                                    int *converged) {
    IQHOST_TRY({
        PhyloTree *t = (PhyloTree *)h;
        *lnl = t->optimizeMixtureWeights(p_invar, nsteps, converged);
        const std::vector<double> w = t->getMixtureWeights();
        memcpy(weights, w.data(), sizeof(double) * w.size());
        memcpy(props, t->getProps().data(), sizeof(double) * (size_t)t->ncat);
    });
}
int iqhost_mix_timing(void *h, double *ms, int64_t *launches) {
    IQHOST_TRY({
        PhyloTree *t = (PhyloTree *)h;
        if (!t->engine) throw std::runtime_error("no engine");
        if (iqhip_debug_mix_timing(t->engine, ms, launches) != 0) throw std::runtime_error(iqhip_last_error());
    });
}
// ---- per-class log-likelihoods of the branch a -> b.  class_invar: NULL or [class][ptn]; floored: NULL or nmixture
int iqhost_class_lnl(void *h, int a, int b, const double *class_weight, const double *class_invar, double *lnl, int64_t *floored) {
    IQHOST_TRY({
        PhyloTree *t = (PhyloTree *)h;
        t->classLnl(nei(t, a, b), t->nodes[a], class_weight, class_invar, lnl, floored);
    });
}
int iqhost_class_lnl_timing(void *h, double *ms) {
    IQHOST_TRY({
        PhyloTree *t = (PhyloTree *)h;
        if (!t->engine) throw std::runtime_error("no engine");
        if (iqhip_debug_class_lnl_timing(t->engine, ms) != 0) throw std::runtime_error(iqhip_last_error());
    });
}
int iqhost_set_boot_samples(void *h, const float *samples, int nsamples) {
    IQHOST_TRY(((PhyloTree *)h)->setBootSamples(samples, nsamples));
}
int iqhost_compute_rell(void *h, double *out, int cap) {
    IQHOST_TRY({
        std::vector<double> r;
        ((PhyloTree *)h)->computeRELL(r);
        if ((int)r.size() > cap) throw std::runtime_error("output too small");
        memcpy(out, r.data(), r.size() * sizeof(double));
    });
}

// last submitted plan: 7 ints per op {dst_from, dst_to, left_node, right_node, left_leaf, right_leaf, 0}
// plus 2 doubles per op {left_len, right_len}; dst_from->dst_to is the neighbour that was filled
// all nni1 candidates of the tree in one submission: ids[4*k + {0..3}] = node1, node2, node1_nei, node2_nei ids,
// vals[2*k + {0,1}] = newLen[0], newloglh.  Returns the number of candidates in *n.
// nni5 batch: vals[6*k + {0..5}] = newLen[0..4], newloglh
// both on a branch list (2 node ids per branch; NULL: all internal branches); first_row >= 0 (nni5 only) keeps candidate
// k's per-pattern lnL in row first_row + k of the engine's store
int iqhost_evaluate_nnis_list(void *h, int nni5, const int *branches, int nbranches, int first_row, int *ids, double *vals,
                              int cap, int *n) {
    IQHOST_TRY({
        PhyloTree *t = (PhyloTree *)h;
        PhyloTree::BranchList list;
        for (int q = 0; branches && q < nbranches; q++) list.push_back({branches[2 * q], branches[2 * q + 1]});
        std::vector<PhyloTree::NNIMove> mv;
        if (!nni5) {
            if (first_row >= 0) throw std::runtime_error("evaluateNNIsBatch keeps no per-pattern rows");
            t->evaluateNNIsBatch(mv, branches ? &list : nullptr);
        } else if (first_row >= 0) {
            std::vector<PhyloNode *> n1, n2;
            if (!branches) t->internalBranches(n1, n2);
            std::vector<int> rows(2 * (branches ? list.size() : n1.size()));
            for (size_t k = 0; k < rows.size(); k++) rows[k] = first_row + (int)k;
            if (!t->engine) throw std::runtime_error("no engine");
            if (iqhip_ptnlh_reserve(t->engine, first_row + (int)rows.size()) != 0) throw std::runtime_error(iqhip_last_error());
            t->evaluateNNIs5Batch(mv, rows.data(), branches ? &list : nullptr);
        } else
            t->evaluateNNIs5Batch(mv, nullptr, branches ? &list : nullptr);
        if ((int)mv.size() > cap) throw std::runtime_error("output too small");
        *n = (int)mv.size();
        const int w = nni5 ? 6 : 2;
        for (size_t k = 0; k < mv.size(); k++) {
            ids[4 * k] = mv[k].node1; ids[4 * k + 1] = mv[k].node2;
            ids[4 * k + 2] = mv[k].node1_nei; ids[4 * k + 3] = mv[k].node2_nei;
            if (nni5)
                for (int i = 0; i < 5; i++) vals[w * k + i] = mv[k].newLen[i];
            else
                vals[w * k] = mv[k].newLen[0];
            vals[w * k + w - 1] = mv[k].newloglh;
        }
    });
}
int iqhost_evaluate_nnis_batch(void *h, int *ids, double *vals, int cap, int *n) {
    return iqhost_evaluate_nnis_list(h, 0, nullptr, 0, -1, ids, vals, cap, n);
}
int iqhost_evaluate_nnis5_batch(void *h, int *ids, double *vals, int cap, int *n) {
    return iqhost_evaluate_nnis_list(h, 1, nullptr, 0, -1, ids, vals, cap, n);
}
int iqhost_evaluate_nnis5_batch_rows(void *h, int *ids, double *vals, int cap, int *n, int first_row) {
    return iqhost_evaluate_nnis_list(h, 1, nullptr, 0, first_row, ids, vals, cap, n);
}
// testAllBranches: ids[2q + {0,1}] = node1, node2; vals[7q + {0..6}] = lh0, lh1, lh2, sh_alrt, lbp, abayes, alrt_stat
int iqhost_test_all_branches(void *h, int reps, int lbp_reps, int batched, int *ids, double *vals, int cap, int *n, double *lnl) {
    IQHOST_TRY({
        std::vector<PhyloTree::BranchSupport> sup;
        *lnl = ((PhyloTree *)h)->testAllBranches(reps, lbp_reps, sup, batched != 0);
        if ((int)sup.size() > cap) throw std::runtime_error("output too small");
        *n = (int)sup.size();
        for (size_t q = 0; q < sup.size(); q++) {
            ids[2 * q] = sup[q].node1; ids[2 * q + 1] = sup[q].node2;
            for (int k = 0; k < 3; k++) vals[7 * q + k] = sup[q].lh[k];
            vals[7 * q + 3] = sup[q].sh_alrt; vals[7 * q + 4] = sup[q].lbp;
            vals[7 * q + 5] = sup[q].abayes; vals[7 * q + 6] = sup[q].alrt_stat;
        }
    });
}
// the tree with "SH-aLRT[/LBP]" labels from n supports laid out as iqhost_test_all_branches returns them
int iqhost_support_tree_string(void *h, const int *ids, const double *vals, int n, int with_sh, int with_lbp, char *out, int cap) {
    IQHOST_TRY({
        std::vector<PhyloTree::BranchSupport> sup((size_t)n);
        for (int q = 0; q < n; q++) {
            sup[q].node1 = ids[2 * q]; sup[q].node2 = ids[2 * q + 1];
            sup[q].sh_alrt = vals[7 * q + 3]; sup[q].lbp = vals[7 * q + 4];
        }
        std::string s = ((PhyloTree *)h)->supportTreeString(sup, with_sh != 0, with_lbp != 0);
        if ((int)s.size() + 1 > cap) throw std::runtime_error("output too small");
        memcpy(out, s.c_str(), s.size() + 1);
    });
}
int iqhost_gen_boot_samples(void *h, int nsamples, int64_t first_replicate, int64_t ndraws, uint64_t seed, uint32_t stream) {
    IQHOST_TRY(((PhyloTree *)h)->genBootSamples(nsamples, ndraws, seed, stream, first_replicate));
}
// evaluateTrees: vals[9t + {0..8}] = logL, bp-RELL, p-KH, p-SH, p-WKH, p-WSH, c-ELW, in the RELL-BP confidence set, in the
// ELW one; au_bp[k * ntrees + t] for the nscales scales (nscales == 0: no AU replicates)
int iqhost_evaluate_trees(void *h, const char **newicks, int ntrees, int fixed_lengths, int nsamples, int weighted,
                          const double *au_scales, int nscales, uint64_t seed, double epsilon, double *vals, double *au_bp) {
    IQHOST_TRY({
        std::vector<std::string> nwk;
        for (int t = 0; t < ntrees; t++) nwk.push_back(newicks[t]);
        std::vector<double> scales(au_scales, au_scales + (nscales > 0 ? nscales : 0));
        std::vector<PhyloTree::TreeTest> res;
        std::vector<double> bp;
        ((PhyloTree *)h)->evaluateTrees(nwk, fixed_lengths != 0, nsamples, weighted != 0, scales, seed, res, bp, epsilon);
        for (size_t t = 0; t < res.size(); t++) {
            const iqhip_tree_test &r = res[t].t;
            double *v = vals + 9 * t;
            v[0] = res[t].logl; v[1] = r.rell_bp; v[2] = r.kh_pvalue; v[3] = r.sh_pvalue;
            v[4] = r.wkh_pvalue; v[5] = r.wsh_pvalue; v[6] = r.elw_value;
            v[7] = (double)r.rell_confident; v[8] = (double)r.elw_confident;
        }
        if (!bp.empty()) memcpy(au_bp, bp.data(), sizeof(double) * bp.size());
    });
}
int iqhost_compute_dist(void *h, const double *init, double *dist, double *d2l) {
    IQHOST_TRY(((PhyloTree *)h)->computeDist(init, dist, d2l));
}
int iqhost_pair_counts(void *h, const int32_t *pairs, int npairs, double *counts) {
    IQHOST_TRY(((PhyloTree *)h)->pairCounts(pairs, npairs, counts));
}
// likelihood mapping: results = nq records of iqhip_quartet_result
int iqhost_quartet_cells(void *h, const int32_t *quartets, int nq, double *cells, int32_t *nother) {
    IQHOST_TRY(((PhyloTree *)h)->quartetCells(quartets, nq, cells, nother));
}
int iqhost_quartet_likelihoods(void *h, const int32_t *quartets, int nq, int iterations, double tolerance,
                               const double *const_invar, iqhip_quartet_result *results) {
    IQHOST_TRY(((PhyloTree *)h)->computeQuartetLikelihoods(quartets, nq, results, iterations, tolerance, const_invar));
}
// *nq = the number of quartets evaluated (call with cap = 0 first: nothing is computed then); with cap >= *nq: seq_id
// [4 nq], logl and weight [3 nq each], corner and area [nq each], counts = 7 areas ++ 3 corners, seq_count [(leafNum + 1) * 10]
int iqhost_likelihood_mapping(void *h, int64_t nquartets, uint64_t seed, const double *const_invar, int64_t cap, int64_t *nq,
                              int32_t *seq_id, double *logl, double *weight, int32_t *corner, int32_t *area, int64_t *counts,
                              int64_t *seq_count) {
    IQHOST_TRY({
        PhyloTree *t = (PhyloTree *)h;
        if (t->leafNum < 4) throw std::runtime_error("likelihood mapping needs at least 4 taxa");
        const int64_t all = lmap::numQuartets(t->leafNum);
        const int64_t n = (nquartets == 0 || nquartets >= all) ? all : nquartets;
        *nq = n;
        if (cap >= n && n > 0) {
            PhyloTree::LmapResult r;
            t->doLikelihoodMapping(nquartets, seed, r, const_invar);
            for (size_t q = 0; q < r.info.size(); q++) {
                for (int k = 0; k < 4; k++) seq_id[4 * q + k] = r.info[q].seqID[k];
                for (int k = 0; k < 3; k++) {
                    logl[3 * q + k] = r.info[q].logl[k];
                    weight[3 * q + k] = r.info[q].qweight[k];
                }
                corner[q] = r.info[q].corner;
                area[q] = r.info[q].area;
            }
            for (int k = 0; k < 7; k++) counts[k] = r.areacount[k];
            for (int k = 0; k < 3; k++) counts[7 + k] = r.cornercount[k];
            memcpy(seq_count, r.seq_count.data(), sizeof(int64_t) * r.seq_count.size());
        }
    });
}
// the pure host pieces of lmap_host.h
int iqhost_lmap_region(const double *logl3, double *weight3, int *corner, int *area) {
    IQHOST_TRY(lmap::region(logl3, weight3, corner, area));
}
int64_t iqhost_lmap_num_quartets(int n) { return lmap::numQuartets(n); }
int iqhost_lmap_all_quartets(int n, int32_t *out) {
    IQHOST_TRY({
        std::vector<int32_t> q;
        lmap::allQuartets(n, q);
        if (!q.empty()) memcpy(out, q.data(), sizeof(int32_t) * q.size());
    });
}
int iqhost_lmap_draw_quartets(int n, int64_t count, uint64_t seed, int32_t *out) {
    IQHOST_TRY({
        std::vector<int32_t> q;
        lmap::drawQuartets(n, count, seed, q);
        if (!q.empty()) memcpy(out, q.data(), sizeof(int32_t) * q.size());
    });
}
// out: NULL or cap bytes for the Newick string; *need = its length + 1 (the string is copied only when it fits)
int iqhost_bionj_newick(const iqhip_bionj_step *steps, int n, const int32_t *last, const double *last_len, const char **names,
                        char *out, int cap, int *need) {
    IQHOST_TRY({
        if (n < 3 || !names) throw std::runtime_error("bionjNewick: one name per taxon, at least 3 taxa");
        std::vector<std::string> nm;
        for (int i = 0; i < n; i++) nm.push_back(names[i]);
        const std::string s = PhyloTree::bionjNewick(steps, n, last, last_len, nm);
        if (need) *need = (int)s.size() + 1;
        if (out && (int)s.size() + 1 <= cap) memcpy(out, s.c_str(), s.size() + 1);
    });
}
// steps: leafNum - 3 entries (at least room for one), last / last_len: 3; the Newick string as above
int iqhost_compute_bionj(void *h, const double *dist, const double *var, iqhip_bionj_step *steps, int32_t *last, double *last_len,
                         char *out, int cap, int *need) {
    IQHOST_TRY({
        PhyloTree *t = (PhyloTree *)h;
        std::string s;
        t->computeBioNJ(dist, var, &s, steps, last, last_len);
        if (need) *need = (int)s.size() + 1;
        if (out && (int)s.size() + 1 <= cap) memcpy(out, s.c_str(), s.size() + 1);
    });
}
int iqhost_compute_parsimony(void *h, int *score) { IQHOST_TRY(*score = ((PhyloTree *)h)->computeParsimony()); }
int iqhost_parsimony_branch(void *h, int a, int b, int *score, int *subst) {
    IQHOST_TRY({
        PhyloTree *t = (PhyloTree *)h;
        *score = t->computeParsimonyBranch(nei(t, a, b), t->nodes[a], subst);
    });
}
int iqhost_initialize_all_partial_pars(void *h) { IQHOST_TRY(((PhyloTree *)h)->initializeAllPartialPars()); }
int iqhost_compute_all_partial_pars(void *h) { IQHOST_TRY(((PhyloTree *)h)->computeAllPartialPars()); }
int iqhost_fix_negative_branch(void *h, int force, int *fixed) {
    IQHOST_TRY(*fixed = ((PhyloTree *)h)->fixNegativeBranch(force != 0));
}
int64_t iqhost_pars_nsites(void *h) { return ((PhyloTree *)h)->pars_nsites; }
int iqhost_get_branches(void *h, int *out /* 2 per branch */, int cap) {
    PhyloTree *t = (PhyloTree *)h;
    std::vector<PhyloNode *> n1, n2;
    if (t->root) t->getBranches(n1, n2);
    for (size_t k = 0; k < n1.size() && (int)k < cap; k++) {
        out[2 * k] = n1[k]->id;
        out[2 * k + 1] = n2[k]->id;
    }
    return (int)n1.size();
}
// trace (optional): rows of (step, node1, node2, score), at most trace_cap of them, *ntrace = how many there are;
// chosen: per step the index of the branch taken (ntaxa - 3 entries)
int iqhost_compute_parsimony_tree(void *h, const int *order, int *score, int *trace, int trace_cap, int *ntrace, int *chosen) {
    IQHOST_TRY({
        PhyloTree *t = (PhyloTree *)h;
        std::vector<PhyloTree::ParsStep> steps;
        *score = t->computeParsimonyTree(order, trace ? &steps : nullptr);
        int rows = 0;
        for (size_t s = 0; s < steps.size(); s++) {
            if (chosen) chosen[s] = steps[s].chosen;
            for (size_t k = 0; k < steps[s].node1.size(); k++, rows++)
                if (rows < trace_cap) {
                    trace[4 * rows] = (int)s;
                    trace[4 * rows + 1] = steps[s].node1[k];
                    trace[4 * rows + 2] = steps[s].node2[k];
                    trace[4 * rows + 3] = steps[s].score[k];
                }
        }
        if (ntrace) *ntrace = rows;
    });
}
// jobs / steps: rows of 4 ints as the structs of include/iqhip.h; moves: rows of (prune, subtree, node1, node2, depth).
// *njobs / *nsteps = how many there are; a buffer is filled only when its cap suffices
int iqhost_collect_spr_jobs(void *h, int radius, int *jobs, int jobs_cap, int *steps, int *moves, int steps_cap, int *njobs,
                            int *nsteps) {
    IQHOST_TRY({
        PhyloTree *t = (PhyloTree *)h;
        std::vector<iqhip_pars_spr_job> jv;
        std::vector<iqhip_pars_spr_step> sv;
        std::vector<PhyloTree::SprMove> mv;
        t->collectSprJobs(radius, jv, sv, mv);
        *njobs = (int)jv.size();
        *nsteps = (int)sv.size();
        if (jobs && (int)jv.size() <= jobs_cap && !jv.empty()) memcpy(jobs, jv.data(), sizeof(jv[0]) * jv.size());
        if ((int)sv.size() <= steps_cap)
            for (size_t k = 0; k < sv.size(); k++) {
                if (steps) memcpy(steps + 4 * k, &sv[k], sizeof(sv[k]));
                if (moves) {
                    int *row = moves + 5 * k;
                    row[0] = mv[k].prune;
                    row[1] = mv[k].subtree;
                    row[2] = mv[k].node1;
                    row[3] = mv[k].node2;
                    row[4] = mv[k].depth;
                }
            }
    });
}
int iqhost_apply_spr_move(void *h, int prune, int subtree, int node1, int node2) {
    IQHOST_TRY({
        PhyloTree::SprMove mv;
        mv.prune = prune;
        mv.subtree = subtree;
        mv.node1 = node1;
        mv.node2 = node2;
        mv.depth = 1;
        ((PhyloTree *)h)->applySprMove(mv);
    });
}
// trace (optional): rows of (score_before, job, step, score, steps_scored, prune, subtree, node1, node2, applied)
int iqhost_optimize_parsimony_spr(void *h, int radius, int max_rounds, int *score, int *trace, int trace_cap, int *nrounds) {
    IQHOST_TRY({
        PhyloTree *t = (PhyloTree *)h;
        std::vector<PhyloTree::SprRound> rounds;
        *score = t->optimizeParsimonySPR(radius, max_rounds, &rounds);
        for (size_t k = 0; k < rounds.size() && trace && (int)k < trace_cap; k++) {
            const PhyloTree::SprRound &r = rounds[k];
            int *row = trace + 10 * k;
            row[0] = r.score_before;
            row[1] = r.job;
            row[2] = r.step;
            row[3] = r.score;
            row[4] = r.steps_scored;
            row[5] = r.move.prune;
            row[6] = r.move.subtree;
            row[7] = r.move.node1;
            row[8] = r.move.node2;
            row[9] = r.applied ? 1 : 0;
        }
        if (nrounds) *nrounds = (int)rounds.size();
    });
}
// ---- the parsimony forest (pars_forest_host.h).  orders: K rows of ntaxa taxon ids.  *out = a result handle for the
// accessors below, freed with iqhost_pars_forest_free.  calls: updates, batch scans, branch-scores calls, SPR scans, inits
int iqhost_parsimony_orders(uint64_t seed, int K, int ntaxa, int *out) {
    IQHOST_TRY({
        if (K < 0 || ntaxa < 0) throw std::runtime_error("parsimony_orders: negative count");
        const std::vector<std::vector<int>> o = iqsearch::parsimonyOrders(seed, K, ntaxa);
        for (int k = 0; k < K; k++)
            for (int i = 0; i < ntaxa; i++) out[(size_t)k * ntaxa + i] = o[(size_t)k][(size_t)i];
    });
}
int iqhost_pars_forest_build(void *h, const int *orders, int K, int spr_radius, int trace, void **out, int64_t *calls) {
    IQHOST_TRY({
        PhyloTree *t = (PhyloTree *)h;
        *out = nullptr;
        if (K < 0) throw std::runtime_error("compute_parsimony_forest: negative count");
        std::vector<std::vector<int>> ord((size_t)K);
        for (int k = 0; k < K; k++) ord[(size_t)k].assign(orders + (size_t)k * t->leafNum, orders + (size_t)(k + 1) * t->leafNum);
        std::unique_ptr<ParsimonyForest> f(new ParsimonyForest(t));
        f->spr_radius = spr_radius;
        f->keep_trace = trace != 0;
        f->build(ord);
        if (calls) {
            calls[0] = f->calls.updates; calls[1] = f->calls.scans; calls[2] = f->calls.branch_scores;
            calls[3] = f->calls.spr_scans; calls[4] = f->calls.inits;
        }
        *out = f.release();
    });
}
void iqhost_pars_forest_free(void *f) { delete (ParsimonyForest *)f; }
// text: Newick, newline, topology; nrows = the trace rows of the member
int iqhost_pars_forest_member(void *f, int k, int *score, int *spr_rounds, int *nrows, char *text, int cap, int *need) {
    IQHOST_TRY({
        ParsimonyForest *pf = (ParsimonyForest *)f;
        if (k < 0 || k >= (int)pf->members.size()) throw std::runtime_error("forest member out of range");
        const ParsimonyForest::Member &m = pf->members[(size_t)k];
        *score = m.score;
        *spr_rounds = m.spr_rounds;
        int rows = 0;
        for (const PhyloTree::ParsStep &s : m.steps) rows += (int)s.node1.size();
        *nrows = rows;
        const std::string s = m.newick + "\n" + m.topology;
        if (need) *need = (int)s.size() + 1;
        if (text && (int)s.size() + 1 <= cap) memcpy(text, s.c_str(), s.size() + 1);
    });
}
// trace: rows of (step, node1, node2, score) as iqhost_compute_parsimony_tree; chosen / best: one entry per step
int iqhost_pars_forest_trace(void *f, int k, int *trace, int trace_cap, int *chosen, int *best, int steps_cap) {
    IQHOST_TRY({
        ParsimonyForest *pf = (ParsimonyForest *)f;
        if (k < 0 || k >= (int)pf->members.size()) throw std::runtime_error("forest member out of range");
        const std::vector<PhyloTree::ParsStep> &steps = pf->members[(size_t)k].steps;
        int rows = 0;
        for (size_t s = 0; s < steps.size(); s++) {
            if ((int)s < steps_cap) {
                chosen[s] = steps[s].chosen;
                best[s] = steps[s].best_score;
            }
            for (size_t q = 0; q < steps[s].node1.size(); q++, rows++)
                if (rows < trace_cap) {
                    trace[4 * rows] = (int)s;
                    trace[4 * rows + 1] = steps[s].node1[q];
                    trace[4 * rows + 2] = steps[s].node2[q];
                    trace[4 * rows + 3] = steps[s].score[q];
                }
        }
    });
}
int iqhost_sync_inputs(void *h) { IQHOST_TRY(((PhyloTree *)h)->syncInputs()); }
int iqhost_compute_all_partial_lh(void *h) { IQHOST_TRY(((PhyloTree *)h)->computeAllPartialLh()); }
int iqhost_last_plan(void *h, int *ints, double *lens, uint64_t *keys, int cap) {
    PhyloTree *t = (PhyloTree *)h;
    int n = (int)t->last_plan.size();
    for (int k = 0; k < n && k < cap; k++) {
        const PlanOp &p = t->last_plan[k];
        // find the owner node of dst: the node whose neighbour list contains it
        int from = -1;
        for (PhyloNode *nd : t->nodes)
            for (PhyloNeighbor *nb : nd->neighbors)
                if (nb == p.dst) from = nd->id;
        ints[k * 7 + 0] = from;
        ints[k * 7 + 1] = p.dst ? p.dst->node->id : -1;
        ints[k * 7 + 2] = p.left ? p.left->node->id : -1;
        ints[k * 7 + 3] = p.right ? p.right->node->id : -1;
        ints[k * 7 + 4] = p.op.left_leaf;
        ints[k * 7 + 5] = p.op.right_leaf;
        ints[k * 7 + 6] = (int)p.op.flags;
        if (lens) { lens[k * 2] = p.op.left_len; lens[k * 2 + 1] = p.op.right_len; }
        if (keys) { keys[k * 3] = p.op.dst_key; keys[k * 3 + 1] = p.op.left_key; keys[k * 3 + 2] = p.op.right_key; }
    }
    return n;
}
long iqhost_num_partial_lh_computations(void *h) { return ((PhyloTree *)h)->num_partial_lh_computations; }
long iqhost_num_submissions(void *h) { return ((PhyloTree *)h)->num_submissions; }


// ---- ultrafast bootstrap bookkeeping (PhyloTree::initUFBoot ...) and the pure split functions of ufboot_splits.h
static void ufboot_report(PhyloTree *t, int64_t *counts, double *min_orig_logl) {
    if (counts) memcpy(counts, t->ufboot_counts, sizeof t->ufboot_counts);
    if (min_orig_logl) *min_orig_logl = t->ufboot_min_orig_logl;
}
int iqhost_ufboot_init(void *h, int nsamples, uint64_t seed) { IQHOST_TRY(((PhyloTree *)h)->initUFBoot(nsamples, seed)); }
int iqhost_ufboot_params(void *h, double epsilon, double logl_cutoff) {
    IQHOST_TRY({
        if (!(epsilon >= 0.0)) throw std::runtime_error("ufboot epsilon must be >= 0");
        ((PhyloTree *)h)->ufboot_epsilon = epsilon;
        ((PhyloTree *)h)->ufboot_logl_cutoff = logl_cutoff;
    });
}
int iqhost_ufboot_next_iteration(void *h) { IQHOST_TRY(((PhyloTree *)h)->ufbootNextIteration()); }
// info: {trees fed so far, Newick strings kept}; vals: {logl_cutoff, min_orig_logl}
int iqhost_ufboot_info(void *h, int64_t *info, double *vals) {
    IQHOST_TRY({
        PhyloTree *t = (PhyloTree *)h;
        info[0] = t->ufboot_next_id;
        info[1] = (int64_t)t->ufboot_trees.size();
        vals[0] = t->ufboot_logl_cutoff;
        vals[1] = t->ufboot_min_orig_logl;
    });
}
int iqhost_save_current_tree(void *h, double logl, int64_t *counts, double *min_orig_logl) {
    IQHOST_TRY({
        ((PhyloTree *)h)->saveCurrentTree(logl);
        ufboot_report((PhyloTree *)h, counts, min_orig_logl);
    });
}
int iqhost_save_nni_trees(void *h, int64_t *counts, double *min_orig_logl) {
    IQHOST_TRY({
        ((PhyloTree *)h)->saveNNITrees();
        ufboot_report((PhyloTree *)h, counts, min_orig_logl);
    });
}
int iqhost_sorted_taxon_id_string(void *h, char *out, int cap, int *need) {
    IQHOST_TRY({
        const std::string s = ((PhyloTree *)h)->sortedTaxonIdString();
        if (need) *need = (int)s.size() + 1;
        if (out && (int)s.size() + 1 <= cap) memcpy(out, s.c_str(), s.size() + 1);
    });
}
// ids: node1, node2 per internal branch; text: support tree, consensus tree and the nsamples winners, one per line
int iqhost_summarize_bootstrap(void *h, int *ids, int *support, int cap, int *nbranch, int *distinct, char *text, int text_cap,
                               int *need) {
    IQHOST_TRY({
        PhyloTree::UFBootSummary sum;
        ((PhyloTree *)h)->summarizeBootstrap(sum);
        const int n = (int)sum.support.size();
        if (nbranch) *nbranch = n;
        if (distinct) *distinct = sum.distinct_trees;
        if (n > cap) throw std::runtime_error("summarizeBootstrap: output too small");
        for (int q = 0; q < n; q++) {
            ids[2 * q] = sum.node1[q];
            ids[2 * q + 1] = sum.node2[q];
            support[q] = sum.support[q];
        }
        std::string s = sum.support_tree + "\n" + sum.consensus_tree + "\n";
        for (const std::string &t : sum.boot_trees) s += t + "\n";
        if (need) *need = (int)s.size() + 1;
        if (text && (int)s.size() + 1 <= text_cap) memcpy(text, s.c_str(), s.size() + 1);
    });
}
static std::vector<std::string> ufboot_names(const char **names, int ntaxa) {
    std::vector<std::string> nm;
    if (names)
        for (int i = 0; i < ntaxa; i++) nm.push_back(names[i]);
    return nm;
}
static void ufboot_count_trees(ufboot::SplitCounts &sc, const char **trees, int ntrees, const int64_t *weights,
                               const std::vector<std::string> &nm) {
    if (ntrees < 0 || (ntrees > 0 && !trees)) throw std::runtime_error("bad tree list");
    std::vector<ufboot::Split> splits;
    for (int k = 0; k < ntrees; k++) {
        if (weights && weights[k] < 0) throw std::runtime_error("a tree weight must be >= 0");
        ufboot::newickSplits(trees[k], sc.ntaxa, splits, nm);
        sc.addTree(splits, weights ? weights[k] : 1);
    }
}
// words: cap * ((ntaxa + 63) / 64) uint64; names: NULL (integer taxon ids) or ntaxa labels
int iqhost_ufboot_newick_splits(const char *newick, int ntaxa, const char **names, uint64_t *words, int cap, int *nsplits) {
    IQHOST_TRY({
        if (!newick || !nsplits) throw std::runtime_error("newickSplits: null argument");
        std::vector<ufboot::Split> splits;
        ufboot::newickSplits(newick, ntaxa, splits, ufboot_names(names, ntaxa));
        *nsplits = (int)splits.size();
        const size_t W = ufboot::splitWords(ntaxa);
        if (words && (int)splits.size() <= cap)
            for (size_t k = 0; k < splits.size(); k++) memcpy(words + k * W, splits[k].data(), sizeof(uint64_t) * W);
    });
}
// the supports round(100 count / sum of weights) of the splits of `query` (iqhost_ufboot_newick_splits order) among `trees`
int iqhost_ufboot_split_supports(const char **trees, int ntrees, const int64_t *weights, int ntaxa, const char **names,
                                 const char *query, int *support, int cap, int *nsplits) {
    IQHOST_TRY({
        if (!query || !nsplits) throw std::runtime_error("splitSupports: null argument");
        const std::vector<std::string> nm = ufboot_names(names, ntaxa);
        ufboot::SplitCounts sc(ntaxa);
        ufboot_count_trees(sc, trees, ntrees, weights, nm);
        std::vector<ufboot::Split> splits;
        ufboot::newickSplits(query, ntaxa, splits, nm);
        *nsplits = (int)splits.size();
        if (support && (int)splits.size() <= cap)
            for (size_t k = 0; k < splits.size(); k++) support[k] = ufboot::splitSupport(sc, splits[k], sc.total);
    });
}
int iqhost_ufboot_consensus(const char **trees, int ntrees, const int64_t *weights, int ntaxa, const char **names, char *out,
                            int cap, int *need) {
    IQHOST_TRY({
        const std::vector<std::string> nm = ufboot_names(names, ntaxa);
        ufboot::SplitCounts sc(ntaxa);
        ufboot_count_trees(sc, trees, ntrees, weights, nm);
        const std::string s = ufboot::consensusTree(sc, nm);
        if (need) *need = (int)s.size() + 1;
        if (out && (int)s.size() + 1 <= cap) memcpy(out, s.c_str(), s.size() + 1);
    });
}

// ---- NNI tree search (search_host.h, tree_search_host.h) ---------------------------------------------------------------
static PhyloTree::NNIMove nni_move(PhyloTree *t, int node1, int node2, int node1_nei, int node2_nei) {
    if (node1 < 0 || node2 < 0 || node1 >= t->nodeNum || node2 >= t->nodeNum) throw std::runtime_error("bad node id");
    PhyloTree::NNIMove mv;
    mv.node1 = node1; mv.node2 = node2; mv.node1_nei = node1_nei; mv.node2_nei = node2_nei;
    return mv;
}
int iqhost_do_nni(void *h, int node1, int node2, int node1_nei, int node2_nei, int clear_lh) {
    IQHOST_TRY({
        PhyloTree *t = (PhyloTree *)h;
        t->doNNI(nni_move(t, node1, node2, node1_nei, node2_nei), clear_lh != 0);
    });
}
int iqhost_change_nni_brans(void *h, int node1, int node2, const double *new_len, int nni5) {
    IQHOST_TRY({
        PhyloTree *t = (PhyloTree *)h;
        PhyloTree::NNIMove mv = nni_move(t, node1, node2, -1, -1);
        for (int i = 0; i < 5; i++) mv.newLen[i] = new_len[i];
        t->changeNNIBrans(mv, nni5 != 0);
    });
}
// out: node1, node2, node1_nei, node2_nei of the move that was made
int iqhost_do_random_nni(void *h, int a, int b, int bit1, int bit2, int *out) {
    IQHOST_TRY({
        PhyloTree *t = (PhyloTree *)h;
        nei(t, a, b);
        const PhyloTree::NNIMove mv = t->doOneRandomNNI(t->nodes[a], t->nodes[b], bit1, bit2);
        out[0] = mv.node1; out[1] = mv.node2; out[2] = mv.node1_nei; out[3] = mv.node2_nei;
    });
}
int iqhost_save_branch_lengths(void *h, double *out, int cap, int *n) {
    IQHOST_TRY({
        std::vector<double> v;
        ((PhyloTree *)h)->saveBranchLengths(v);
        *n = (int)v.size();
        if (out && (int)v.size() <= cap) memcpy(out, v.data(), sizeof(double) * v.size());
    });
}
int iqhost_restore_branch_lengths(void *h, const double *v, int n) {
    IQHOST_TRY(((PhyloTree *)h)->restoreBranchLengths(std::vector<double>(v, v + (n > 0 ? n : 0))));
}
namespace {
struct ScoredMove {
    int node1, node2;
    double newloglh;
    int index;
};
std::string jnum(double v) {
    char buf[40];
    snprintf(buf, sizeof buf, "%.17g", v);
    return buf;
}
std::string jmove(const PhyloTree::NNIMove &m) {
    std::string s = "[" + std::to_string(m.node1) + "," + std::to_string(m.node2) + "," + std::to_string(m.node1_nei) + "," +
                    std::to_string(m.node2_nei) + "," + jnum(m.newloglh);
    for (int i = 0; i < 5; i++) s += "," + jnum(m.newLen[i]);
    return s + "]";
}
std::string jmoves(const std::vector<PhyloTree::NNIMove> &v) {
    std::string s = "[";
    for (size_t k = 0; k < v.size(); k++) s += (k ? "," : "") + jmove(v[k]);
    return s + "]";
}
std::string jsteps(const std::vector<TreeSearch::NNIStep> &steps) {
    std::string s = "[";
    for (size_t k = 0; k < steps.size(); k++) {
        const TreeSearch::NNIStep &st = steps[k];
        s += k ? ",{" : "{";
        s += "\"branches\":[";
        for (size_t q = 0; q < st.branches.size(); q++)
            s += (q ? ",[" : "[") + std::to_string(st.branches[q].first) + "," + std::to_string(st.branches[q].second) + "]";
        s += "],\"all_branches\":" + std::string(st.all_branches ? "true" : "false");
        s += ",\"evaluated\":" + jmoves(st.evaluated) + ",\"positive\":" + jmoves(st.positive) + ",\"applied\":" + jmoves(st.applied);
        s += ",\"score\":" + jnum(st.score) + ",\"rolled_back\":" + (st.rolled_back ? "true" : "false");
        s += ",\"submissions\":" + std::to_string(st.submissions) + "}";
    }
    return s + "]";
}
std::string jstring(const std::string &t) {   // Newick strings and topologies hold no character that needs escaping but these
    std::string s = "\"";
    for (char c : t) {
        if (c == '"' || c == '\\') s += '\\';
        s += c;
    }
    return s + "\"";
}
struct SearchHandle {
    TreeSearch search;
    std::vector<TreeSearch::NNIStep> nni_steps;   // of the last iqhost_search_optimize_nni
    explicit SearchHandle(PhyloTree *t) : search(t) {}
    explicit SearchHandle(PhyloSuperTree *t) : search(t) {}
};
void put_text(const std::string &s, char *out, int cap, int *need) {
    if (need) *need = (int)s.size() + 1;
    if (out && (int)s.size() + 1 <= cap) memcpy(out, s.c_str(), s.size() + 1);
}
}  // namespace

// order[k] = index of the k-th move of the descending stable sort
int iqhost_search_sort_moves(const double *score, int n, int *order) {
    IQHOST_TRY({
        std::vector<ScoredMove> mv((size_t)(n > 0 ? n : 0));
        for (int k = 0; k < n; k++) mv[(size_t)k] = ScoredMove{0, 0, score[k], k};
        iqsearch::sortMoves(mv);
        for (int k = 0; k < n; k++) order[k] = mv[(size_t)k].index;
    });
}
// nodes: node1, node2 per move, in sorted order; taken: indices of the moves kept
int iqhost_search_select_non_conflicting(const int *nodes, int n, int *taken, int *ntaken) {
    IQHOST_TRY({
        std::vector<ScoredMove> mv((size_t)(n > 0 ? n : 0));
        for (int k = 0; k < n; k++) mv[(size_t)k] = ScoredMove{nodes[2 * k], nodes[2 * k + 1], 0.0, k};
        const std::vector<ScoredMove> sel = iqsearch::selectNonConflicting(mv);
        *ntaken = (int)sel.size();
        for (size_t k = 0; k < sel.size(); k++) taken[k] = sel[k].index;
    });
}
// adjacency in CSR form: the neighbours of node v are adj[adj_off[v] .. adj_off[v + 1]); applied: node1, node2 per move
int iqhost_search_branches_for_nni(const int *applied, int napplied, const int *adj_off, const int *adj, int nnodes, int *out,
                                   int cap, int *n) {
    IQHOST_TRY({
        iqsearch::Adjacency a((size_t)(nnodes > 0 ? nnodes : 0));
        for (int v = 0; v < nnodes; v++) a[(size_t)v].assign(adj + adj_off[v], adj + adj_off[v + 1]);
        std::vector<ScoredMove> mv;
        for (int k = 0; k < napplied; k++) {
            if (applied[2 * k] < 0 || applied[2 * k] >= nnodes || applied[2 * k + 1] < 0 || applied[2 * k + 1] >= nnodes)
                throw std::runtime_error("branchesForNNI: bad node id");
            mv.push_back(ScoredMove{applied[2 * k], applied[2 * k + 1], 0.0, k});
        }
        const iqsearch::BranchList list = iqsearch::branchesForNNI(mv, a);
        *n = (int)list.size();
        if ((int)list.size() > cap) throw std::runtime_error("output too small");
        for (size_t q = 0; q < list.size(); q++) { out[2 * q] = list[q].first; out[2 * q + 1] = list[q].second; }
    });
}
uint64_t iqhost_search_rand(uint64_t seed, uint64_t iteration, uint64_t draw) { return iqsearch::searchRand(seed, iteration, draw); }
int iqhost_search_rand_int(uint64_t z, int n) { return iqsearch::searchRandInt(z, n); }
int iqhost_search_stop(int condition, int cur_iteration, double cur_correlation, int min_iteration, int unsuccess_iteration,
                       double min_correlation, int max_iteration, int last_improved) {
    iqsearch::StopRule r;
    r.stop_condition = (iqsearch::StopCondition)condition;
    r.min_iteration = min_iteration;
    r.unsuccess_iteration = unsuccess_iteration;
    r.min_correlation = min_correlation;
    r.max_iteration = max_iteration;
    r.last_improved_iteration = last_improved;
    return r.meetStopCondition(cur_iteration, cur_correlation) ? 1 : 0;
}
// nsnap snapshots one after the other: snapshot s has nsplits[s] splits of (ntaxa + 63) / 64 words with one weight each
int iqhost_search_bootstrap_correlation(int ntaxa, int nsnap, const int *nsplits, const uint64_t *words, const int64_t *weights,
                                        double *out) {
    IQHOST_TRY({
        const size_t W = ufboot::splitWords(ntaxa);
        std::vector<ufboot::SplitCounts> snaps;
        size_t at = 0;
        for (int s = 0; s < nsnap; s++) {
            ufboot::SplitCounts sc(ntaxa);
            for (int k = 0; k < nsplits[s]; k++, at++) {
                ufboot::Split sp(words + at * W, words + (at + 1) * W);
                ufboot::splitNormalise(sp, ntaxa);
                if (ufboot::splitTrivial(sp, ntaxa)) continue;
                sc.addTree(std::vector<ufboot::Split>(1, sp), weights[at]);
            }
            snaps.push_back(sc);
        }
        *out = iqsearch::bootstrapCorrelation(snaps);
    });
}
int iqhost_candset_create(void **out, int max_candidates) {
    IQHOST_TRY({
        iqsearch::CandidateSet *c = new iqsearch::CandidateSet();
        if (max_candidates > 0) c->maxCandidates = max_candidates;
        *out = c;
    });
}
void iqhost_candset_destroy(void *c) { delete (iqsearch::CandidateSet *)c; }
int iqhost_candset_update(void *c, const char *tree, const char *topology, double score, int *is_new) {
    IQHOST_TRY(*is_new = ((iqsearch::CandidateSet *)c)->update(tree, topology, score) ? 1 : 0);
}
int iqhost_candset_size(void *c) { return (int)((iqsearch::CandidateSet *)c)->size(); }
int iqhost_candset_exists(void *c, const char *topology) { return ((iqsearch::CandidateSet *)c)->treeTopologyExist(topology) ? 1 : 0; }
double iqhost_candset_best_score(void *c) { return ((iqsearch::CandidateSet *)c)->getBestScore(); }
int iqhost_candset_rand_rank(void *c, int pop_size, uint64_t r, int *rank) {
    IQHOST_TRY({
        iqsearch::CandidateSet *s = (iqsearch::CandidateSet *)c;
        if (s->empty()) throw std::runtime_error("getRandCandTree on an empty candidate set");
        *rank = (int)s->randCandRank(pop_size, r);
    });
}
// text: tree, newline, topology
int iqhost_candset_entry(void *c, int rank, double *score, char *text, int cap, int *need) {
    IQHOST_TRY({
        iqsearch::CandidateSet *s = (iqsearch::CandidateSet *)c;
        if (rank < 0 || rank >= (int)s->size()) throw std::runtime_error("candidate rank out of range");
        const iqsearch::CandidateTree &t = s->byRank((size_t)rank);
        *score = t.score;
        put_text(t.tree + "\n" + t.topology, text, cap, need);
    });
}

int iqhost_search_create(void **out, void *tree) {
    IQHOST_TRY(*out = new SearchHandle((PhyloTree *)tree));
}
int iqhost_search_create_super(void **out, void *super_tree) {
    IQHOST_TRY(*out = new SearchHandle((PhyloSuperTree *)super_tree));
}
void iqhost_search_destroy(void *s) { delete (SearchHandle *)s; }
// iv: nni5, speednni, batched, popSize, stop condition, min_iteration, unsuccess_iteration, max_iteration, step_iterations,
// keep_trace, numInitTrees, numNNITrees, initSprRadius; dv: initPS, min_correlation
int iqhost_search_set_params(void *s, const int *iv, const double *dv, uint64_t seed) {
    IQHOST_TRY({
        TreeSearch &ts = ((SearchHandle *)s)->search;
        ts.numInitTrees = iv[10]; ts.numNNITrees = iv[11]; ts.initSprRadius = iv[12];
        ts.nni5 = iv[0] != 0; ts.speednni = iv[1] != 0; ts.batched = iv[2] != 0; ts.popSize = iv[3];
        if (iv[4] < 0 || iv[4] > 2) throw std::runtime_error("TreeSearch: unknown stop condition");
        ts.stop_rule.stop_condition = (iqsearch::StopCondition)iv[4];
        ts.stop_rule.min_iteration = iv[5]; ts.stop_rule.unsuccess_iteration = iv[6]; ts.stop_rule.max_iteration = iv[7];
        ts.step_iterations = iv[8]; ts.keep_trace = iv[9] != 0;
        ts.initPS = dv[0]; ts.stop_rule.min_correlation = dv[1];
        ts.seed = seed;
    });
}
// computeLikelihood(), then optimizeNNI; the steps are kept for iqhost_search_trace_json when keep_trace is set
int iqhost_search_optimize_nni(void *s, double *lnl, int *nni_count, int *nni_steps) {
    IQHOST_TRY({
        SearchHandle *sh = (SearchHandle *)s;
        sh->search.checkEligible("optimizeNNI");
        sh->nni_steps.clear();
        sh->search.computeLikelihood();
        *lnl = sh->search.optimizeNNI(*nni_count, *nni_steps, sh->search.keep_trace ? &sh->nni_steps : nullptr);
    });
}
// out: node1, node2, bit1, bit2 per NNI
int iqhost_search_do_random_nnis(void *s, int num_nni, uint64_t iteration, int *out, int cap, int *n) {
    IQHOST_TRY({
        std::vector<std::array<int, 4>> done;
        ((SearchHandle *)s)->search.doRandomNNIs(num_nni, iteration, &done);
        *n = (int)done.size();
        for (size_t k = 0; k < done.size() && (int)k < cap; k++)
            for (int i = 0; i < 4; i++) out[4 * k + i] = done[k][(size_t)i];
    });
}
int iqhost_search_do_tree_search(void *s, double *best) {
    IQHOST_TRY(*best = ((SearchHandle *)s)->search.doTreeSearch());
}
// {"nni_steps": [...], "iterations": [...], "candidates": [[score, tree, topology] best first], "correlation_log":
//  [[iteration, correlation]], "boot_splits": [[[taxa of the split], weight] per snapshot]}
int iqhost_search_trace_json(void *s, char *out, int cap, int *need) {
    IQHOST_TRY({
        SearchHandle *sh = (SearchHandle *)s;
        const TreeSearch &ts = sh->search;
        std::string j = "{\"nni_steps\":" + jsteps(sh->nni_steps) + ",\"iterations\":[";
        for (size_t k = 0; k < ts.trace.size(); k++) {
            const TreeSearch::Iteration &it = ts.trace[k];
            j += k ? ",{" : "{";
            j += "\"iteration\":" + std::to_string(it.iteration) + ",\"parent\":" + std::to_string(it.parent) + ",\"random_nnis\":[";
            for (size_t q = 0; q < it.random_nnis.size(); q++) {
                j += q ? ",[" : "[";
                for (size_t i = 0; i < 4; i++) j += (i ? "," : "") + std::to_string(it.random_nnis[q][i]);
                j += "]";
            }
            j += "],\"perturb_score\":" + jnum(it.perturb_score) + ",\"steps\":" + jsteps(it.steps) + ",\"score\":" + jnum(it.score);
            j += ",\"new_best\":" + std::string(it.new_best ? "true" : "false") + ",\"nni_count\":" + std::to_string(it.nni_count) + "}";
        }
        j += "],\"candidates\":[";
        for (size_t k = 0; k < ts.candidates.size(); k++) {
            const iqsearch::CandidateTree &c = ts.candidates.byRank(k);
            j += (k ? ",[" : "[") + jnum(c.score) + "," + jstring(c.tree) + "," + jstring(c.topology) + "]";
        }
        j += "],\"init_duplicates\":" + std::to_string(ts.init_duplicates) + ",\"init_trees\":[";
        for (size_t k = 0; k < ts.init_trees.size(); k++) {
            const iqsearch::CandidateTree &c = ts.init_trees[k];
            j += (k ? ",[" : "[") + jnum(c.score) + "," + jstring(c.tree) + "," + jstring(c.topology) + "]";
        }
        j += "],\"correlation_log\":[";
        for (size_t k = 0; k < ts.correlation_log.size(); k++)
            j += (k ? ",[" : "[") + std::to_string(ts.correlation_log[k].first) + "," + jnum(ts.correlation_log[k].second) + "]";
        j += "],\"boot_splits\":[";
        for (size_t k = 0; k < ts.boot_splits.size(); k++) {
            const ufboot::SplitCounts &sc = ts.boot_splits[k];
            j += k ? ",[" : "[";
            for (size_t q = 0; q < sc.splits.size(); q++) {
                j += q ? ",[[" : "[[";
                bool first = true;
                for (int t = 0; t < sc.ntaxa; t++)
                    if (ufboot::splitHas(sc.splits[q], t)) { j += (first ? "" : ",") + std::to_string(t); first = false; }
                j += "]," + std::to_string(sc.weight[q]) + "]";
            }
            j += "]";
        }
        j += "]}";
        put_text(j, out, cap, need);
    });
}

// ---- edge-linked partition models (supertree_host.h).  A member handle is a PhyloTree owned by the super tree: every
// iqhost_* call above takes it, iqhost_destroy must not.
int iqhost_super_create(void **out, const char *newick, const char **names, int nnames) {
    *out = nullptr;
    PhyloSuperTree *t = nullptr;
    try {
        t = new PhyloSuperTree();
        std::vector<std::string> nm;
        for (int i = 0; i < nnames; i++) nm.push_back(names[i]);
        t->readTreeString(newick, nm);
        *out = t;
        return 0;
    } catch (const std::exception &ex) {
        g_host_err = ex.what();
        delete t;
        return 1;
    }
}
void iqhost_super_destroy(void *h) { delete (PhyloSuperTree *)h; }
int iqhost_super_add_partition(void *h, const char *name, void **member) {
    IQHOST_TRY(*member = ((PhyloSuperTree *)h)->addPartition(name ? name : ""));
}
int iqhost_super_attach_engines(void *h, int device) { IQHOST_TRY(((PhyloSuperTree *)h)->attachEngines(device)); }
int iqhost_super_num_parts(void *h) { return ((PhyloSuperTree *)h)->size(); }
void *iqhost_super_group(void *h) { return ((PhyloSuperTree *)h)->group; }
int iqhost_super_set_fixed_rates(void *h, int on) { IQHOST_TRY(((PhyloSuperTree *)h)->fixed_rates = on != 0); }
int iqhost_super_set_rates(void *h, const double *rates) { IQHOST_TRY(((PhyloSuperTree *)h)->setRates(rates)); }
int iqhost_super_get_rates(void *h, double *rates) {
    IQHOST_TRY({
        PhyloSuperTree *t = (PhyloSuperTree *)h;
        for (int p = 0; p < t->size(); p++) rates[p] = t->part_rate[(size_t)p];
    });
}
int iqhost_super_part_lnl(void *h, double *out) {
    IQHOST_TRY({
        PhyloSuperTree *t = (PhyloSuperTree *)h;
        for (int p = 0; p < t->size(); p++) out[p] = t->cur_score[(size_t)p];
    });
}
int iqhost_super_set_branch_bounds(void *h, double lo, double hi) { IQHOST_TRY(((PhyloSuperTree *)h)->setBranchBounds(lo, hi)); }
int iqhost_super_compute_likelihood(void *h, double *lnl) { IQHOST_TRY(*lnl = ((PhyloSuperTree *)h)->computeLikelihood()); }
int iqhost_super_optimize_one_branch(void *h, int a, int b, int clear_lh, int max_nr_step, double *new_len) {
    IQHOST_TRY(*new_len = ((PhyloSuperTree *)h)->optimizeOneBranch(a, b, clear_lh != 0, max_nr_step));
}
int iqhost_super_optimize_all_branches(void *h, int iterations, double tolerance, int max_nr_step, double *lnl) {
    IQHOST_TRY(*lnl = ((PhyloSuperTree *)h)->optimizeAllBranches(iterations, tolerance, max_nr_step));
}
// evals: Brent evaluations per member (nparts); *rounds: lockstep rounds = group traversals of this call
int iqhost_super_optimize_gene_rates(void *h, double gradient_epsilon, double *lnl, int *evals, int *rounds) {
    IQHOST_TRY({
        PhyloSuperTree *t = (PhyloSuperTree *)h;
        *lnl = t->optimizeGeneRate(gradient_epsilon);
        if (evals)
            for (int p = 0; p < t->size(); p++) evals[p] = t->gene_rate_evals[(size_t)p];
        if (rounds) *rounds = t->gene_rate_rounds;
    });
}
int iqhost_super_optimize_parameters(void *h, int fixed_len, double logl_epsilon, double gradient_epsilon, double *lnl) {
    IQHOST_TRY(*lnl = ((PhyloSuperTree *)h)->optimizeParameters(fixed_len != 0, logl_epsilon, gradient_epsilon));
}
int iqhost_super_newton_branch(void *h, int a, int b, double xguess, double x1, double x2, double xacc, int max_steps,
                               double *optx, double *d2l, int *nsteps, double *part_lnl) {
    IQHOST_TRY(((PhyloSuperTree *)h)->partitionNewtonBranch(a, b, xguess, x1, x2, xacc, max_steps, optx, d2l, nsteps, part_lnl));
}
int iqhost_super_branch_length(void *h, int a, int b, double *len) {
    IQHOST_TRY(*len = nei(&((PhyloSuperTree *)h)->super, a, b)->length);
}
// the branches in optimizeAllBranches' order; returns their number
int iqhost_super_branch_order(void *h, int *n1, int *n2, int cap) {
    try {
        std::vector<int> a, b;
        ((PhyloSuperTree *)h)->branchOrder(a, b);
        for (size_t k = 0; k < a.size() && (int)k < cap; k++) { n1[k] = a[k]; n2[k] = b[k]; }
        return (int)a.size();
    } catch (const std::exception &ex) {
        g_host_err = ex.what();
        return -1;
    }
}
int iqhost_super_tree_string(void *h, char *out, int cap) {
    std::string s = ((PhyloSuperTree *)h)->getTreeString();
    if ((int)s.size() + 1 > cap) return (int)s.size() + 1;
    memcpy(out, s.c_str(), s.size() + 1);
    return 0;
}
// out[3] = joint solves, group traversals, diverged-Newton resets so far
int iqhost_super_counters(void *h, long *out) {
    PhyloSuperTree *t = (PhyloSuperTree *)h;
    out[0] = t->num_group_solves;
    out[1] = t->num_group_traversals;
    out[2] = t->num_diverged;
    return 0;
}
long iqhost_super_group_batches(void *h) { return ((PhyloSuperTree *)h)->num_group_batches; }

// ---- the starting tree of a partitioned alignment (supertree_host.h)
int iqhost_super_compute_dist(void *h, const double *init, double *dist, double *d2l) {
    IQHOST_TRY(((PhyloSuperTree *)h)->computeDist(dist, d2l, init));
}
int iqhost_super_compute_bionj(void *h, const double *dist, const double *var, char *out, int cap, int *need) {
    IQHOST_TRY({
        std::string s;
        ((PhyloSuperTree *)h)->computeBioNJ(dist, var, &s);
        if (need) *need = (int)s.size() + 1;
        if (out && (int)s.size() + 1 <= cap) memcpy(out, s.c_str(), s.size() + 1);
    });
}
int iqhost_super_fix_negative_branch(void *h, int force, int *fixed) {
    IQHOST_TRY(*fixed = ((PhyloSuperTree *)h)->fixNegativeBranch(force != 0));
}

// ---- NNI on the super tree (supertree_host.h): the layouts of the plain tree's calls above
int iqhost_super_set_all_branch_mode(void *h) { IQHOST_TRY(((PhyloSuperTree *)h)->setAllBranchMode()); }
// the super tree's topology as a PhyloTree handle for the read-only calls above (tree string, sorted taxon ids, neighbours);
// it has no engine and is owned by the super tree
void *iqhost_super_tree(void *h) { return &((PhyloSuperTree *)h)->super; }
// a candidate tree on the same taxa: re-read by the super tree and every member, engines kept
int iqhost_super_read_tree(void *h, const char *newick) {
    IQHOST_TRY({
        PhyloSuperTree *t = (PhyloSuperTree *)h;
        std::vector<std::string> names;
        bool named = false;
        for (int i = 0; i < t->super.leafNum; i++) {
            const PhyloNode *n = t->super.nodes[(size_t)i];
            named = named || !n->name.empty();
            names.push_back(n->name.empty() ? std::to_string(n->id) : n->name);
        }
        t->readTreeString(newick, named ? names : std::vector<std::string>());
    });
}
int iqhost_super_num_nodes(void *h) { return ((PhyloSuperTree *)h)->super.nodeNum; }
int iqhost_super_num_leaves(void *h) { return ((PhyloSuperTree *)h)->super.leafNum; }
int iqhost_super_neighbors(void *h, int node, int *ids, double *lens, int cap) {
    return iqhost_neighbors(&((PhyloSuperTree *)h)->super, node, ids, lens, cap);
}
int iqhost_super_do_nni(void *h, int node1, int node2, int node1_nei, int node2_nei) {
    IQHOST_TRY({
        PhyloSuperTree *t = (PhyloSuperTree *)h;
        t->doNNI(nni_move(&t->super, node1, node2, node1_nei, node2_nei));
    });
}
int iqhost_super_change_nni_brans(void *h, int node1, int node2, const double *new_len, int nni5) {
    IQHOST_TRY({
        PhyloSuperTree *t = (PhyloSuperTree *)h;
        PhyloTree::NNIMove mv = nni_move(&t->super, node1, node2, -1, -1);
        for (int i = 0; i < 5; i++) mv.newLen[i] = new_len[i];
        t->changeNNIBrans(mv, nni5 != 0);
    });
}
int iqhost_super_do_random_nni(void *h, int a, int b, int bit1, int bit2, int *out) {
    IQHOST_TRY({
        PhyloSuperTree *t = (PhyloSuperTree *)h;
        nei(&t->super, a, b);
        const PhyloTree::NNIMove mv = t->doOneRandomNNI(a, b, bit1, bit2);
        out[0] = mv.node1; out[1] = mv.node2; out[2] = mv.node1_nei; out[3] = mv.node2_nei;
    });
}
int iqhost_super_save_branch_lengths(void *h, double *out, int cap, int *n) {
    IQHOST_TRY({
        std::vector<double> v;
        ((PhyloSuperTree *)h)->saveBranchLengths(v);
        *n = (int)v.size();
        if (out && (int)v.size() <= cap) memcpy(out, v.data(), sizeof(double) * v.size());
    });
}
int iqhost_super_restore_branch_lengths(void *h, const double *in, int n) {
    IQHOST_TRY(((PhyloSuperTree *)h)->restoreBranchLengths(std::vector<double>(in, in + n)));
}
int iqhost_super_clear_all_partial_lh(void *h) { IQHOST_TRY(((PhyloSuperTree *)h)->clearAllPartialLH()); }
int iqhost_super_gen_boot_samples(void *h, int nsamples, uint64_t seed) {
    IQHOST_TRY(((PhyloSuperTree *)h)->genBootSamples(nsamples, seed));
}
// first_row >= 0: the two neighbours' per-pattern values go to rows first_row, first_row + 1 of every member's store
int iqhost_super_nni_for_branch_rows(void *h, int a, int b, int nni5, int first_row, double *out) {
    IQHOST_TRY({
        PhyloTree::NNIMove mv[2];
        const int rows[2] = {first_row, first_row + 1};
        if (first_row >= 0) ((PhyloSuperTree *)h)->reservePtnlhRows(first_row + 2);
        ((PhyloSuperTree *)h)->getBestNNIForBran(a, b, nni5 != 0, mv, first_row >= 0 ? rows : nullptr);
        for (int c = 0; c < 2; c++) {
            out[c * 8 + 0] = mv[c].newloglh;
            out[c * 8 + 1] = mv[c].node1_nei;
            out[c * 8 + 2] = mv[c].node2_nei;
            for (int k = 0; k < 5; k++) out[c * 8 + 3 + k] = mv[c].newLen[k];
        }
    });
}
// ... without rows
int iqhost_super_nni_for_branch(void *h, int a, int b, int nni5, double *out) {
    return iqhost_super_nni_for_branch_rows(h, a, b, nni5, -1, out);
}
// first_row >= 0 (nni5 only): candidate k's per-pattern values go to row first_row + k of every member's store
int iqhost_super_evaluate_nnis_list_rows(void *h, int nni5, const int *branches, int nbranches, int first_row, int *ids,
                                         double *vals, int cap, int *n) {
    IQHOST_TRY({
        PhyloSuperTree *t = (PhyloSuperTree *)h;
        PhyloTree::BranchList list;
        for (int q = 0; branches && q < nbranches; q++) list.push_back({branches[2 * q], branches[2 * q + 1]});
        std::vector<PhyloTree::NNIMove> mv;
        if (first_row >= 0 && !nni5) throw std::runtime_error("per-pattern rows need the nni5 evaluation");
        if (first_row >= 0) {
            std::vector<PhyloNode *> n1, n2;
            t->super.internalBranches(n1, n2);
            const size_t nc = 2 * (branches ? list.size() : n1.size());
            std::vector<int> rows(nc);
            for (size_t k = 0; k < nc; k++) rows[k] = first_row + (int)k;
            t->reservePtnlhRows(first_row + (int)nc);
            t->evaluateNNIs5Batch(mv, rows.data(), branches ? &list : nullptr);
        } else if (nni5) t->evaluateNNIs5Batch(mv, branches ? &list : nullptr);
        else t->evaluateNNIsBatch(mv, branches ? &list : nullptr);
        if ((int)mv.size() > cap) throw std::runtime_error("output too small");
        *n = (int)mv.size();
        const int w = nni5 ? 6 : 2;
        for (size_t k = 0; k < mv.size(); k++) {
            ids[4 * k] = mv[k].node1; ids[4 * k + 1] = mv[k].node2;
            ids[4 * k + 2] = mv[k].node1_nei; ids[4 * k + 3] = mv[k].node2_nei;
            for (int i = 0; i < w - 1; i++) vals[w * k + i] = mv[k].newLen[i];
            vals[w * k + w - 1] = mv[k].newloglh;
        }
    });
}

// ... without rows
int iqhost_super_evaluate_nnis_list(void *h, int nni5, const int *branches, int nbranches, int *ids, double *vals, int cap, int *n) {
    return iqhost_super_evaluate_nnis_list_rows(h, nni5, branches, nbranches, -1, ids, vals, cap, n);
}

}  // extern "C"
