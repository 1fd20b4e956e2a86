// solve.hip -- host side of libiqhip.so: the branch-length solvers.  Newton-Raphson on one branch (one launch of
// k_newton, or a chain of enqueued steps), a whole sweep over the branches of a tree, and the batched evaluator of NNI
// candidates, each through the extern "C" entry points declared in include/iqhip.h.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include "iqhip_internal.h"

using namespace iqhip;

// ---------------------------------------------------------------------------------------
// What every form shares (iqhip_internal.h)
// ---------------------------------------------------------------------------------------
int iqhip::newton_check_bounds(const char *entry, double xguess, double x1, double x2, double xacc, int max_steps) {
    if (!(x1 >= 0.0) || !(x2 > x1) || !(xacc > 0.0) || max_steps < 1 || !(xguess >= 0.0))
        return fail(IQHIP_ERR_INVALID, std::string(entry) + ": bad bounds / tolerance / step count");
    return IQHIP_OK;
}

int iqhip::newton_status(int status, bool *gave_up) {
    if (gave_up) *gave_up = status == 4;
    if (status == 2) return fail(IQHIP_ERR_INVALID, "Wrong computeFuncDerv (non-finite derivative)");
    if (status == 3) return fail(IQHIP_ERR_INVALID, "Maximum number of iterations exceeded in minimizeNewton");
    return IQHIP_OK;
}

// ---------------------------------------------------------------------------------------
// Newton as a chain of enqueued steps (kernels_newton.hip, "state machine" kernels): the form a sharded engine
// uses -- every derivative evaluation is followed by an in-stream all-reduce of {df, ddf}, so the loop cannot live
// in one kernel -- and the fallback when k_newton's grid barrier cannot be trusted.  Steps are enqueued in chunks
// (drive_chain); the host reads the 128-byte state once per chunk; steps enqueued after convergence do nothing.
// ---------------------------------------------------------------------------------------
int iqhip::newton_state_alloc(iqhip_engine *e) {
    if (e->d_nstate.ensure(e, 1) != hipSuccess || e->h_nstate.ensure(e, 1) != hipSuccess)
        return fail(IQHIP_ERR_NOMEM, "Newton state");
    return IQHIP_OK;
}

// one evaluation at state->rts on the engine's stream: derivative kernel + k_reduce -> result[0..1]
static int newton_eval_enqueue(iqhip_engine *e) {
    const int nwaves = (int)e->ntiles;
    // (+ASC: prob_const, df_const, ddf_const ride along; a shard without unobserved patterns contributes zeros)
    if (e->asc_active && e->n_unobs == 0 && hipMemsetAsync(e->d_result + 2, 0, 3 * sizeof(double), e->stream) != hipSuccess)
        return fail(IQHIP_ERR_HIP, "Newton chain: memset failed");
    if (launch_derv_at_state(e, nwaves) != hipSuccess || launch_reduce(e, 0, e->n_unobs > 0 ? 5 : 2, nwaves) != hipSuccess)
        return fail(IQHIP_ERR_HIP, "Newton chain: launch failed");
    return IQHIP_OK;
}

// the pieces one at a time, for the single-process front, which interleaves its shards' steps with one grouped
// all-reduce per step
int iqhip::eng_newton_begin(iqhip_engine *e, double xguess, double x1, double x2, double xacc, int max_steps) {
    int rc = check_ready(e);
    if (rc) return rc;
    if (!e->theta_valid) return fail(IQHIP_ERR_INVALID, "Newton: theta not computed");
    rc = newton_state_alloc(e);
    if (rc) return rc;
    rc = ensure_slab_rows(e, 5);
    if (rc) return rc;
    if (launch_newton_state_init(e, xguess, x1, x2, xacc, max_steps) != hipSuccess)
        return fail(IQHIP_ERR_HIP, "Newton chain: launch failed");
    return IQHIP_OK;
}
int iqhip::eng_newton_eval_enqueue(iqhip_engine *e) {
    if (use_device(e) != hipSuccess) return fail(IQHIP_ERR_HIP, "hipSetDevice");
    return newton_eval_enqueue(e);
}
int iqhip::eng_newton_update_enqueue(iqhip_engine *e) {
    if (use_device(e) != hipSuccess) return fail(IQHIP_ERR_HIP, "hipSetDevice");
    if (launch_newton_state_update(e) != hipSuccess) return fail(IQHIP_ERR_HIP, "Newton chain: launch failed");
    return IQHIP_OK;
}

int iqhip::newton_state_read(iqhip_engine *e) {
    if (use_device(e) != hipSuccess) return fail(IQHIP_ERR_HIP, "hipSetDevice");
    if (hipMemcpyAsync(e->h_nstate.p, e->d_nstate.p, sizeof(NewtonState), hipMemcpyDeviceToHost, e->stream) != hipSuccess ||
        hipStreamSynchronize(e->stream) != hipSuccess)
        return fail(IQHIP_ERR_HIP, "Newton chain: state read failed");
    e->staging_busy = false;
    return IQHIP_OK;
}

// The state machine on the host, for callers that own the collective themselves (they evaluate {df, ddf} with
// iqhip_derv_async, all-reduce them their own way and need the reference's update rule between evaluations) and for
// the CPU tests, which check it step by step against the loop form of optimization.cpp:388-465.
extern "C" int iqhip_newton_host_init(void *state, double xguess, double x1, double x2, double xacc, int max_steps,
                                      double *first_x) {
    if (!state) return fail(IQHIP_ERR_INVALID, "null argument");
    int rc = newton_check_bounds("iqhip_newton_host_init", xguess, x1, x2, xacc, max_steps);
    if (rc) return rc;
    static_assert(sizeof(NewtonState) == IQHIP_NEWTON_STATE_BYTES, "NewtonState size");
    NewtonState st;
    newton_init(st, xguess, x1, x2, xacc, max_steps);
    memcpy(state, &st, sizeof st);
    if (first_x) *first_x = st.rts;
    return IQHIP_OK;
}

extern "C" int iqhip_newton_host_update(void *state, double df_sum, double ddf_sum, double *next_x, int *done) {
    if (!state) return fail(IQHIP_ERR_INVALID, "null argument");
    NewtonState st;
    memcpy(&st, state, sizeof st);
    newton_update(st, df_sum, ddf_sum);
    memcpy(state, &st, sizeof st);
    if (next_x) *next_x = st.rts;
    if (done) *done = st.done;
    return IQHIP_OK;
}

extern "C" int iqhip_newton_host_result(const void *state, double *optx, double *d2l, int *nsteps, int *status) {
    if (!state) return fail(IQHIP_ERR_INVALID, "null argument");
    NewtonState st;
    memcpy(&st, state, sizeof st);
    if (!st.done) return fail(IQHIP_ERR_INVALID, "Newton state machine has not finished");
    NewtonResult(st).store(optx, d2l, nsteps);
    if (status) *status = st.status;
    return IQHIP_OK;
}

// theta must be resident; result[2..] untouched
static int newton_chain(iqhip_engine *e, double xguess, double x1, double x2, double xacc, int max_steps,
                        double *optx, double *d2l, int *nsteps) {
    int rc = newton_state_alloc(e);
    if (rc) return rc;
    rc = ensure_slab_rows(e, 5);
    if (rc) return rc;
    HIPCHK(launch_newton_state_init(e, xguess, x1, x2, xacc, max_steps));
    rc = drive_chain(
        max_steps,
        [&] {   // evaluation, the engine's own all-reduce, update
            int rc = newton_eval_enqueue(e);
            if (!rc) rc = comm_allreduce(e, e->asc_active ? 5 : 2);
            if (!rc && launch_newton_state_update(e) != hipSuccess) rc = fail(IQHIP_ERR_HIP, "Newton chain: launch failed");
            return rc;
        },
        [&](bool *done) {
            const int rc = newton_state_read(e);
            *done = !rc && e->h_nstate.p->done;
            return rc;
        });
    if (rc) return rc;
    const NewtonState &st = *e->h_nstate.p;
    rc = newton_status(st.status);
    if (rc) return rc;
    NewtonResult(st).store(optx, d2l, nsteps);
    return IQHIP_OK;
}

// k_newton's grid barrier needs every workgroup resident; a single workgroup needs no barrier.  IQHIP_NEWTON=chain
// forces the chain form (tests).
static bool newton_use_chain(const iqhip_engine *e) { return e->comm || e->newton_chain_forced; }

// The end of a one-launch solve (k_newton) whose result row has been read back.  When the grid barrier gave up (another
// kernel held the CUs) the solve is finished with the chain, which needs no barrier; theta is resident either way.
static int newton_one_launch_result(iqhip_engine *e, const double *row, double xguess, double x1, double x2, double xacc,
                                    int max_steps, double *optx, double *d2l, int *nsteps) {
    const NewtonResult r(row);
    bool gave_up;
    const int rc = newton_status(r.status, &gave_up);
    if (rc) return rc;
    if (gave_up) {
        (void)hipStreamSynchronize(e->stream);
        e->path_counts[IQHIP_PATH_NEWTON_FALLBACK]++;
        return newton_chain(e, xguess, x1, x2, xacc, max_steps, optx, d2l, nsteps);
    }
    r.store(optx, d2l, nsteps);
    return IQHIP_OK;
}

extern "C" int iqhip_newton_branch(iqhip_engine *e, double xguess, double x1, double x2, double xacc,
                                   int max_steps, double *optx, double *d2l, int *nsteps) {
    int rc = newton_check_bounds("iqhip_newton_branch", xguess, x1, x2, xacc, max_steps);
    if (rc) return rc;
    if (e && !e->shards.empty()) {
        iqhip_branch_end none = {0, -1, 0};
        return sharded::optimize_branch(e, nullptr, 0, false, none, none, xguess, x1, x2, xacc, max_steps, nullptr, optx,
                                        d2l, nsteps);
    }
    rc = check_ready(e);
    if (rc) return rc;
    if (!e->theta_valid) return fail(IQHIP_ERR_INVALID, "iqhip_newton_branch: theta not computed");
    if (newton_use_chain(e)) {
        e->path_counts[IQHIP_PATH_NEWTON_CHAIN]++;
        return newton_chain(e, xguess, x1, x2, xacc, max_steps, optx, d2l, nsteps);
    }
    HIPCHK(launch_newton(e, xguess, x1, x2, xacc, max_steps, e->d_result));
    e->path_counts[IQHIP_PATH_NEWTON_ONE_LAUNCH]++;
    rc = read_result(e, 4);
    if (rc) return rc;
    return newton_one_launch_result(e, e->h_result.p, xguess, x1, x2, xacc, max_steps, optx, d2l, nsteps);
}

extern "C" int iqhip_optimize_branch(iqhip_engine *e, const iqhip_node_op *ops, int nops, iqhip_branch_end a,
                                     iqhip_branch_end b, double xguess, double x1, double x2, double xacc,
                                     int max_steps, double *sum_scale, double *optx, double *d2l, int *nsteps) {
    int rc = newton_check_bounds("iqhip_optimize_branch", xguess, x1, x2, xacc, max_steps);
    if (rc) return rc;
    if (e && !e->shards.empty())
        return sharded::optimize_branch(e, ops, nops, true, a, b, xguess, x1, x2, xacc, max_steps, sum_scale, optx, d2l,
                                        nsteps);
    iqhip_branch_end none = {0, -1, 0};
    if (e && newton_use_chain(e)) {
        // sharded rank: node updates (their sum_scale rows all-reduced), theta, then the enqueued Newton chain
        if (nops > 0) {
            rc = iqhip_update_partials(e, ops, nops, sum_scale);
            if (rc) return rc;
        }
        rc = iqhip_compute_theta(e, a, b);
        if (rc) return rc;
        e->path_counts[IQHIP_PATH_NEWTON_CHAIN]++;
        return newton_chain(e, xguess, x1, x2, xacc, max_steps, optx, d2l, nsteps);
    }
    // two launches per branch: the pending node updates, then one kernel that sums their sum_scale rows,
    // builds theta during its first derivative evaluation and runs the whole Newton-Raphson loop
    if (nops > 0) rc = submit_traverse(e, ops, nops, false, none, none, 0.0, /*skip_reduce=*/true);
    else rc = check_ready(e);
    if (rc) return rc;
    if (nops + 6 > e->result_cap) return fail(IQHIP_ERR_INVALID, "too many node updates in one submission");
    DevBranch br;
    rc = build_branch(e, a, b, 0.0, -1, &br);
    if (rc) return rc;
    set_theta_branch(e, br, a, b);
    double *out = e->d_result + 2 + nops;
    HIPCHK(launch_newton(e, xguess, x1, x2, xacc, max_steps, out, &br, nops, (int)e->ntiles * e->lane_split));
    e->path_counts[IQHIP_PATH_NEWTON_ONE_LAUNCH]++;
    rc = read_result(e, 2 + nops + 4);
    if (rc) return rc;
    if (sum_scale)
        for (int k = 0; k < nops; k++) sum_scale[k] = e->h_result.p[2 + k];
    // (a barrier that gave up: theta was built by the first evaluation)
    return newton_one_launch_result(e, e->h_result.p + 2 + nops, xguess, x1, x2, xacc, max_steps, optx, d2l, nsteps);
}

// ---------------------------------------------------------------------------------------
// A whole branch-length sweep -- PhyloTree::optimizeAllBranches' loop over optimizeOneBranch (phylotree.cpp:2252-2332,
// 2148-2192) -- in ONE submission.  Step j = {the node updates that are pending at both ends of branch j, theta, the
// Newton solve, the diverged-solve rule}; a child branch that an earlier step of the sweep optimised has its length read
// from device memory (sweep_len[step]), where that step's Newton kernel left it, so nothing comes back to the host
// between steps: 2 launches per step are enqueued back to back and the host reads one result block per sweep.
// The caller builds the steps as if every step changed its branch (optimizeOneBranch's clearReversePartialLh on both
// sides); a step that ends where it started only makes the later steps recompute vectors that were still valid.
// ---------------------------------------------------------------------------------------
static int sweep_resolve_ops(const iqhip_sweep_step &st, const iqhip_branch_result *results, std::vector<iqhip_node_op> &ops) {
    ops.assign(st.ops, st.ops + st.nops);
    if (st.len_from)
        for (int k = 0; k < st.nops; k++) {
            if (st.len_from[2 * k] >= 0) ops[k].left_len = results[st.len_from[2 * k]].optx;
            if (st.len_from[2 * k + 1] >= 0) ops[k].right_len = results[st.len_from[2 * k + 1]].optx;
        }
    return IQHIP_OK;
}

// the same sweep one step at a time (a host round trip per step): sharded engines and engines with a communicator, where
// every Newton step contains an all-reduce; and the remainder of a sweep whose grid-wide exchange timed out
static int sweep_sequential(iqhip_engine *e, const iqhip_sweep_step *steps, int first, int nsteps, double x1, double x2,
                            double xacc, int max_steps, double diverge_frac, double *sum_scale, size_t ss_off,
                            iqhip_branch_result *results) {
    e->path_counts[IQHIP_PATH_SWEEP_SEQUENTIAL]++;
    std::vector<iqhip_node_op> ops;
    for (int j = first; j < nsteps; j++) {
        const iqhip_sweep_step &st = steps[j];
        sweep_resolve_ops(st, results, ops);
        iqhip_branch_result &r = results[j];
        r.status = 0;
        r.lnl = 0.0;
        int rc = iqhip_optimize_branch(e, ops.empty() ? nullptr : ops.data(), st.nops, st.a, st.b, st.xguess, x1, x2, xacc, max_steps,
                                       sum_scale ? sum_scale + ss_off : nullptr, &r.optx, &r.d2l, &r.nsteps);
        if (rc) return rc;
        if (diverge_frac > 0.0 && r.optx > diverge_frac * x2) {   // phylotree.cpp:2167-2176
            double opt_lh = 0.0, orig_lh = 0.0;
            rc = iqhip_lnl_from_theta(e, r.optx, &opt_lh);
            if (!rc) rc = iqhip_lnl_from_theta(e, st.xguess, &orig_lh);
            if (rc) return rc;
            if (orig_lh > opt_lh) r.optx = st.xguess;
            r.status = 5;   // (informational: the rule was applied)
        }
        ss_off += (size_t)st.nops;
    }
    return IQHIP_OK;
}

// The end of both one-submission forms: the steps' result rows {optx, d2l, nsteps, status, diverged, -}, step j's at
// row_of(j) of the host result vector, into `results`.  A step whose grid-wide exchange gave up (another kernel held the
// CUs) voids its length and everything after it: the sweep is finished from there one step at a time (the chain form
// needs no co-residency), with that step's offset into sum_scale.
template <typename RowOf>
static int sweep_results(iqhip_engine *e, const iqhip_sweep_step *steps, int nsteps, double x1, double x2, double xacc,
                         int max_steps, double diverge_frac, double *sum_scale, iqhip_branch_result *results, RowOf &&row_of) {
    size_t ss = 0;
    for (int j = 0; j < nsteps; j++) {
        const double *o = e->h_result.p + row_of(j);
        const NewtonResult r(o);
        bool gave_up;
        const int rc = newton_status(r.status, &gave_up);
        if (rc) return rc;
        if (gave_up) {
            (void)hipStreamSynchronize(e->stream);
            return sweep_sequential(e, steps, j, nsteps, x1, x2, xacc, max_steps, diverge_frac, sum_scale, ss, results);
        }
        r.store(results[j]);
        results[j].status = o[4] != 0.0 ? 5 : 0;
        results[j].lnl = 0.0;
        ss += (size_t)steps[j].nops;
    }
    return IQHIP_OK;
}

// 4-state engines: the whole sweep as ONE launch of the persistent kernel k_sweep4 (kernels_sweep.hip) + one k_reduce for
// the sum_scale rows; the host only resolves keys into descriptors, copies them down once and reads one result block
static int sweep_persistent4(iqhip_engine *e, const iqhip_sweep_step *steps, int nsteps, size_t total_ops, double x1, double x2,
                             double xacc, int max_steps, double diverge_frac, double *sum_scale, iqhip_branch_result *results) {
    const bool dbg = e->debug_sweep;
    Stopwatch watch;
    if (dbg) watch.start();
    const size_t bytes_ops = sizeof(SweepOp) * total_ops, bytes_steps = sizeof(SweepStep) * (size_t)nsteps;
    const size_t need = bytes_ops + bytes_steps;
    if (need > std::min(e->d_sweep_desc.cap, e->h_sweep_desc.cap)) {
        HIPCHK(e->d_sweep_desc.ensure(e, need * 2 + 4096));
        HIPCHK(e->h_sweep_desc.ensure(e, need * 2 + 4096));
    }
    SweepOp *hops = reinterpret_cast<SweepOp *>(e->h_sweep_desc.p);
    SweepStep *hsteps = reinterpret_cast<SweepStep *>(e->h_sweep_desc.p + bytes_ops);
    size_t row = 0;
    for (int j = 0; j < nsteps; j++) {
        const iqhip_sweep_step &st = steps[j];
        SweepStep &hs = hsteps[j];
        hs.op_begin = (int32_t)row;
        hs.nops = st.nops;
        hs.xguess = st.xguess;
        for (int k = 0; k < st.nops; k++, row++) {
            const iqhip_node_op &o = st.ops[k];
            SweepOp &d = hops[row];
            memset(&d, 0, sizeof d);
            if (!(o.left_len >= 0.0) || !(o.right_len >= 0.0)) return fail(IQHIP_ERR_INVALID, "negative or NaN branch length");
            const uint8_t *lst, *rst;
            int32_t lk, rk;
            int rc = resolve_child(e, o.left_key, o.left_leaf, -1, &d.lv, &d.lsc, &lst, &lk);
            if (rc) return rc;
            rc = resolve_child(e, o.right_key, o.right_leaf, -1, &d.rv, &d.rsc, &rst, &rk);
            if (rc) return rc;
            d.ls = lst ? lst : e->d_states.p;
            d.rs = rst ? rst : e->d_states.p;
            int didx;
            rc = slab_for_key(e, o.dst_key, true, &didx);
            if (rc) return rc;
            d.dst = e->slabs[didx].plh.p;
            d.dst_sc = e->slabs[didx].sc.p;
            if (d.lv == d.dst || d.rv == d.dst) return fail(IQHIP_ERR_INVALID, "node update writes onto one of its own children");
            d.llen = o.left_len;
            d.rlen = o.right_len;
            d.llen_step = st.len_from ? st.len_from[2 * k] : -1;
            d.rlen_step = st.len_from ? st.len_from[2 * k + 1] : -1;
            d.no_scale = (o.flags & IQHIP_OP_NO_SCALE) ? 1 : (((o.flags & IQHIP_OP_SCALAR_RULE) || e->scalar_rule_all) ? 2 : 0);
            d.row = (int32_t)row;
        }
        int rc = build_branch(e, st.a, st.b, 0.0, -1, &hs.br);
        if (rc) return rc;
    }
    const int grid = sweep4_grid(e), nwaves = grid * sweep4_waves(e);
    const size_t slab_need = total_ops * (size_t)nwaves + 1024;
    if (total_ops * (size_t)nwaves > e->d_slab.cap) HIPCHK(e->d_slab.ensure(e, slab_need));
    const size_t posts_need = (size_t)2 * kNewtonPostEpochs * grid * 2;
    HIPCHK(e->d_sweep_posts.ensure(e, posts_need));
    HIPCHK(hipMemcpyAsync(e->d_sweep_desc.p, e->h_sweep_desc.p, need, hipMemcpyHostToDevice, e->stream));
    if (grid > 1) HIPCHK(hipMemsetAsync(e->d_sweep_posts.p, 0xFF, posts_need * sizeof(double), e->stream));
    double *out = e->d_result + total_ops;      // (rows [0, total_ops) receive the sum_scale sums from k_reduce)
    memset(e->h_result.p + total_ops, 0, sizeof(double) * 6 * (size_t)nsteps);
    e->path_counts[IQHIP_PATH_SWEEP_PERSISTENT]++;
    HIPCHK(launch_sweep4(e, reinterpret_cast<const SweepOp *>(e->d_sweep_desc.p),
                         reinterpret_cast<const SweepStep *>(e->d_sweep_desc.p + bytes_ops), nsteps, x1, x2, xacc, max_steps,
                         diverge_frac * x2, e->d_sweep_posts.p, out));
    HIPCHK(launch_reduce(e, 0, (int)total_ops, nwaves));
    set_theta_branch(e, hsteps[nsteps - 1].br, steps[nsteps - 1].a, steps[nsteps - 1].b);
    e->plan_cache.version = 0;
    const double enqueue_us = dbg ? watch.us() : 0.0;
    int rc = read_result(e, (int)(total_ops + 6 * (size_t)nsteps));
    if (rc) return rc;
    if (dbg)
        fprintf(stderr, "[iqhip] persistent sweep of %d steps (%zu node updates): descriptors + enqueue %.1f us, wait %.1f us\n", nsteps,
                total_ops, enqueue_us, watch.us() - enqueue_us);
    if (sum_scale)
        for (size_t k = 0; k < total_ops; k++) sum_scale[k] = e->h_result.p[k];
    return sweep_results(e, steps, nsteps, x1, x2, xacc, max_steps, diverge_frac, sum_scale, results,
                         [&](int j) { return total_ops + 6 * (size_t)j; });
}

extern "C" int iqhip_optimize_sweep(iqhip_engine *e, const iqhip_sweep_step *steps, int nsteps, double x1, double x2,
                                    double xacc, int max_steps, double diverge_frac, double *sum_scale,
                                    iqhip_branch_result *results) {
    if (!e) return fail(IQHIP_ERR_INVALID, "null engine");
    if (!steps || !results || nsteps < 1) return fail(IQHIP_ERR_INVALID, "iqhip_optimize_sweep: bad step array");
    if (!(x1 >= 0.0) || !(x2 > x1) || !(xacc > 0.0) || max_steps < 1 || !(diverge_frac >= 0.0) || diverge_frac >= 1.0)
        return fail(IQHIP_ERR_INVALID, "iqhip_optimize_sweep: bad bounds / tolerance / step count");
    size_t total_ops = 0;
    for (int j = 0; j < nsteps; j++) {
        const iqhip_sweep_step &st = steps[j];
        if (st.nops < 0 || (st.nops > 0 && !st.ops)) return fail(IQHIP_ERR_INVALID, "bad ops array in a sweep step");
        if (!(st.xguess >= 0.0)) return fail(IQHIP_ERR_INVALID, "iqhip_optimize_sweep: bad starting length");
        if (st.len_from)
            for (int q = 0; q < 2 * st.nops; q++)
                if (st.len_from[q] >= j) return fail(IQHIP_ERR_INVALID, "a sweep step may only use the lengths of earlier steps");
        total_ops += (size_t)st.nops;
    }
    if (!e->shards.empty() || e->comm || !e->sweep_one_submission || newton_use_chain(e) ||
        2 + total_ops + 6 * (size_t)nsteps > (size_t)e->result_cap || e->d_result != e->d_result_own)
        return sweep_sequential(e, steps, 0, nsteps, x1, x2, xacc, max_steps, diverge_frac, sum_scale, 0, results);
    int rc = check_ready(e);
    if (rc) return rc;
    // (+ASC: k_sweep4 has no correction; k_newton applies it to the derivatives and to both lnL of the diverged-solve rule)
    if (e->sweep_persistent && !e->asc_active && !e->mfma && e->nclass == 1 && nsteps <= 4096 && max_steps + 5 <= kNewtonPostEpochs && total_ops > 0)
        return sweep_persistent4(e, steps, nsteps, total_ops, x1, x2, xacc, max_steps, diverge_frac, sum_scale, results);
    (void)e->h_plan_arena.ensure(e, (size_t)1 << 20);   // (without it the plans of this sweep upload the ordinary way)
    struct ArenaScope {   // plan uploads of this sweep go through the arena; whatever happens, switched off on return
        iqhip_engine *e;
        explicit ArenaScope(iqhip_engine *e_) : e(e_) { e->plan_arena_on = e->h_plan_arena.p != nullptr; e->plan_arena_used = 0; }
        ~ArenaScope() { e->plan_arena_on = false; }
    } arena_scope(e);
    e->path_counts[IQHIP_PATH_SWEEP_PER_STEP]++;
    if ((size_t)nsteps > e->d_sweep_len.cap) HIPCHK(e->d_sweep_len.ensure(e, (size_t)nsteps + 64));
    const bool dbg = e->debug_sweep;
    double t_trav = 0.0, t_newt = 0.0;
    int n_uploaded = 0;
    Stopwatch whole, part;
    if (dbg) whole.start();
    // result block in the (host-mapped) result vector: per step its sum_scale rows, then {optx, d2l, nsteps, status, diverged, -}
    std::vector<size_t> row_of(nsteps);
    size_t row = 2;
    std::vector<const double *> len_ptrs;
    iqhip_branch_end none = {0, -1, 0};
    for (int j = 0; j < nsteps; j++) {
        const iqhip_sweep_step &st = steps[j];
        row_of[j] = row;
        if (st.nops > 0) {
            const double *const *lp = nullptr;
            if (st.len_from) {
                len_ptrs.assign((size_t)2 * st.nops, nullptr);
                bool any = false;
                for (int q = 0; q < 2 * st.nops; q++)
                    if (st.len_from[q] >= 0) { len_ptrs[q] = e->d_sweep_len.p + st.len_from[q]; any = true; }
                if (any) lp = len_ptrs.data();
            }
            if (dbg) part.start();
            rc = submit_traverse(e, st.ops, st.nops, false, none, none, 0.0, /*skip_reduce=*/true, nullptr, lp);
            if (rc) return rc;
            if (dbg) { t_trav += part.us(); n_uploaded += e->plan.small ? 0 : 1; }
        }
        DevBranch br;
        rc = build_branch(e, st.a, st.b, 0.0, -1, &br);
        if (rc) return rc;
        set_theta_branch(e, br, st.a, st.b);
        NewtonSweepStep sw;
        sw.len_out = e->d_sweep_len.p + j;
        sw.rows_base = e->d_result + row;
        sw.diverge_x = diverge_frac * x2;
        sw.publish = (j == nsteps - 1);
        if (dbg) part.start();
        HIPCHK(launch_newton(e, st.xguess, x1, x2, xacc, max_steps, e->d_result + row + st.nops, &br, st.nops,
                             (int)e->ntiles * e->lane_split, &sw));
        e->path_counts[IQHIP_PATH_NEWTON_ONE_LAUNCH]++;
        if (dbg) t_newt += part.us();
        row += (size_t)st.nops + 6;
    }
    const double enqueue_us = dbg ? whole.us() : 0.0;
    rc = read_result(e, (int)row);
    if (rc) return rc;
    if (dbg) {
        fprintf(stderr, "[iqhip] sweep of %d steps (%d plans uploaded, the others in the kernel arguments): submit_traverse %.1f us (build_plan %.1f us since the last report), launch_newton %.1f us; enqueue %.1f us, wait %.1f us\n", nsteps, n_uploaded, t_trav, debug_build_us, t_newt,
                enqueue_us, whole.us() - enqueue_us);
        debug_build_us = 0.0;
    }
    if (sum_scale) {
        size_t ss = 0;
        for (int j = 0; j < nsteps; j++)
            for (int k = 0; k < steps[j].nops; k++) sum_scale[ss++] = e->h_result.p[row_of[j] + k];
    }
    return sweep_results(e, steps, nsteps, x1, x2, xacc, max_steps, diverge_frac, sum_scale, results,
                         [&](int j) { return row_of[j] + (size_t)steps[j].nops; });
}

// ---------------------------------------------------------------------------------------
// Batched chain: iqhip_optimize_branch_batch on pattern shards.  The m tasks of a chunk advance side by side: per Newton
// step ONE derivative launch (grid.y = task, branch length read from the task's device-resident state machine), ONE
// k_reduce over 2m slab rows, ONE all-reduce of 2m doubles, ONE update kernel (thread = task); tasks that have converged
// do nothing.  Identical sums on every rank => identical iterates, so all ranks leave the loop together.
// +ASC: 5 rows per task and step, {df, ddf, prob_const, df_const, ddf_const} (an engine without unobserved patterns of its
// own writes zeros into the last three); the lnL pass has its 2 rows {lnl, prob_const} as ever.
// ---------------------------------------------------------------------------------------
int iqhip::batch_derv_rows(const iqhip_engine *e) { return e->asc_active ? 5 : 2; }

static BatchChain batch_chain_of(const iqhip_engine *e, int m) {
    return BatchChain{e->d_theta_batch.p, (size_t)e->nptn_pad * e->block, e->d_bstates.p, m, batch_derv_rows(e),
                      e->asc_active ? e->d_bsc.p : nullptr};
}

// phylokernel.h:1183-1186 on a task's all-reduced {lnl, prob_const}
int iqhip::batch_asc_lnl(const iqhip_engine *e, double prob_const, double *lnl) {
    if (!e->asc_active) return IQHIP_OK;
    double lp;
    const int rc = asc_log_term(prob_const, &lp);
    if (rc) return rc;
    *lnl -= e->asc_nsites * lp;
    return IQHIP_OK;
}

// init == nullptr: the theta slots only -- the caller keeps the state machines and sums the slots itself (partition.hip)
int iqhip::eng_batch_prepare(iqhip_engine *e, const iqhip_branch_task *tasks, int m, const NewtonState *init) {
    int rc = check_ready(e);
    if (rc) return rc;
    const int rows = batch_derv_rows(e);
    if (rows * m > e->result_cap) return fail(IQHIP_ERR_INVALID, "too many tasks in one chunk");
    rc = ensure_slab_rows(e, std::max(5, rows * m));
    if (rc) return rc;
    const size_t theta_stride = (size_t)e->nptn_pad * e->block;
    HIPCHK(e->d_theta_batch.ensure(e, (size_t)m * theta_stride));
    if (init) HIPCHK(e->d_bstates.ensure(e, (size_t)m));
    if (e->asc_active) HIPCHK(e->d_bsc.ensure(e, (size_t)2 * m));
    std::vector<const int16_t *> sc;
    for (int t = 0; t < m; t++) {
        DevBranch br;
        rc = build_branch(e, tasks[t].a, tasks[t].b, 0.0, -1, &br);
        if (rc) return rc;
        sc.push_back(br.a_sc);
        sc.push_back(br.b_sc);
        double *slot = e->d_theta_batch.p + (size_t)t * theta_stride;
        if (e->mfma) HIPCHK(launch_stream_mfma(e, 1, &br, 0.0, (int)e->ntiles, nullptr, -1, slot));
        else HIPCHK(launch_theta4(e, br, slot));
    }
    // (pageable source, as the states below)
    if (e->asc_active)
        HIPCHK(hipMemcpyAsync(e->d_bsc.p, sc.data(), sizeof(const int16_t *) * sc.size(), hipMemcpyHostToDevice, e->stream));
    return init ? eng_batch_states_write(e, m, init) : IQHIP_OK;
}

int iqhip::eng_batch_states_write(iqhip_engine *e, int m, const NewtonState *in) {
    if (use_device(e) != hipSuccess) return fail(IQHIP_ERR_HIP, "hipSetDevice");
    // (pageable source: the copy has left the host buffer when the call returns)
    if (hipMemcpyAsync(e->d_bstates.p, in, sizeof(NewtonState) * (size_t)m, hipMemcpyHostToDevice, e->stream) != hipSuccess)
        return fail(IQHIP_ERR_HIP, "batched chain: state upload failed");
    return IQHIP_OK;
}

int iqhip::eng_batch_states_read(iqhip_engine *e, int m, NewtonState *out) {
    if (use_device(e) != hipSuccess) return fail(IQHIP_ERR_HIP, "hipSetDevice");
    if (hipMemcpyAsync(out, e->d_bstates.p, sizeof(NewtonState) * (size_t)m, hipMemcpyDeviceToHost, e->stream) != hipSuccess ||
        hipStreamSynchronize(e->stream) != hipSuccess)
        return fail(IQHIP_ERR_HIP, "batched chain: state read failed");
    e->staging_busy = false;
    return IQHIP_OK;
}

// one pass over the tasks' theta slots at the lengths in their state machines + k_reduce -> result[0..2m) (+ASC
// derivatives: [0..5m)): {df, ddf} at states[t].rts, or {lnL, prob_const} at states[t].result
static int batch_pass_enqueue(iqhip_engine *e, int m, bool lnl) {
    if (use_device(e) != hipSuccess) return fail(IQHIP_ERR_HIP, "hipSetDevice");
    const BatchChain bc = batch_chain_of(e, m);
    const int nwaves = (int)e->ntiles;
    const hipError_t s = e->mfma ? launch_stream_mfma(e, lnl ? 3 : 2, nullptr, 0.0, nwaves, nullptr, -1, nullptr, &bc)
                         : lnl   ? launch_lnl_theta4(e, 0.0, nwaves, &bc)
                                 : launch_derv4(e, 0.0, nwaves, nullptr, &bc);
    if (s != hipSuccess || launch_reduce(e, 0, (lnl ? 2 : bc.derv_rows) * m, nwaves) != hipSuccess)
        return fail(IQHIP_ERR_HIP, "batched chain: launch failed");
    return IQHIP_OK;
}
int iqhip::eng_batch_eval_enqueue(iqhip_engine *e, int m) { return batch_pass_enqueue(e, m, false); }
int iqhip::eng_batch_lnl_enqueue(iqhip_engine *e, int m) { return batch_pass_enqueue(e, m, true); }

int iqhip::eng_batch_update_enqueue(iqhip_engine *e, int m) {
    if (use_device(e) != hipSuccess) return fail(IQHIP_ERR_HIP, "hipSetDevice");
    if (launch_newton_state_update_batch(e, e->d_bstates.p, m) != hipSuccess)
        return fail(IQHIP_ERR_HIP, "batched chain: launch failed");
    return IQHIP_OK;
}

int iqhip::batch_chunk(int chunk) {
    if (const char *bc = getenv("IQHIP_BATCH_CHUNK")) chunk = std::max(1, std::min(chunk, atoi(bc)));
    return chunk;
}

static int batch_task_check(const iqhip_branch_task &k) {
    if (k.nops < 0 || (k.nops > 0 && !k.ops)) return fail(IQHIP_ERR_INVALID, "bad ops array in a task");
    return newton_check_bounds("iqhip_optimize_branch_batch", k.xguess, k.x1, k.x2, k.xacc, k.max_steps);
}

int iqhip::batch_gather_ops(const iqhip_branch_task *tasks, int ntasks, std::vector<iqhip_node_op> &all, std::vector<int> &segs) {
    all.clear();
    segs.resize((size_t)ntasks);
    for (int t = 0; t < ntasks; t++) {
        const int rc = batch_task_check(tasks[t]);
        if (rc) return rc;
        segs[t] = tasks[t].nops;
        all.insert(all.end(), tasks[t].ops, tasks[t].ops + tasks[t].nops);
    }
    return IQHIP_OK;
}

int iqhip::batch_task_results(const std::vector<NewtonState> &st, int m, iqhip_branch_result *results) {
    for (int t = 0; t < m; t++) {
        const int rc = newton_status(st[t].status);
        if (rc) return rc;
        NewtonResult(st[t]).store(results[t]);
    }
    return IQHIP_OK;
}

// a rank with a communicator: node updates of all tasks in one submission, then the batched chain
static int optimize_branch_batch_comm(iqhip_engine *e, const iqhip_branch_task *tasks, int ntasks, double *sum_scale,
                                      iqhip_branch_result *results) {
    int rc = check_ready(e);
    if (rc) return rc;
    std::vector<iqhip_node_op> all;
    std::vector<int> segs;
    rc = batch_gather_ops(tasks, ntasks, all, segs);
    if (rc) return rc;
    const int total_ops = (int)all.size();
    if (total_ops + 2 > e->result_cap) return fail(IQHIP_ERR_INVALID, "too many node updates in one submission");
    iqhip_branch_end none = {0, -1, 0};
    if (total_ops > 0) {
        rc = submit_traverse(e, all.data(), total_ops, false, none, none, 0.0, /*skip_reduce=*/false, &segs);
        if (rc) return rc;
        rc = comm_allreduce(e, 2 + total_ops);
        if (rc) return rc;
        rc = read_result(e, 2 + total_ops);
        if (rc) return rc;
        if (sum_scale)
            for (int k = 0; k < total_ops; k++) sum_scale[k] = e->h_result.p[2 + k];
    }
    const int chunk = batch_chunk(std::min(ntasks, kBatchChainChunk));
    std::vector<NewtonState> st((size_t)chunk);
    for (int first = 0; first < ntasks; first += chunk) {
        const int m = std::min(chunk, ntasks - first);
        int max_steps = 1;
        for (int t = 0; t < m; t++) {
            const iqhip_branch_task &k = tasks[first + t];
            newton_init(st[t], k.xguess, k.x1, k.x2, k.xacc, k.max_steps);
            max_steps = std::max(max_steps, k.max_steps);
        }
        rc = eng_batch_prepare(e, tasks + first, m, st.data());
        if (rc) return rc;
        rc = drive_chain(
            max_steps,
            [&] {
                int rc = eng_batch_eval_enqueue(e, m);
                if (!rc) rc = comm_allreduce(e, batch_derv_rows(e) * m);
                if (!rc) rc = eng_batch_update_enqueue(e, m);
                return rc;
            },
            [&](bool *done) {
                const int rc = eng_batch_states_read(e, m, st.data());
                *done = !rc && std::all_of(st.begin(), st.begin() + m, [](const NewtonState &s) { return s.done != 0; });
                return rc;
            });
        if (rc) return rc;
        rc = batch_task_results(st, m, results + first);
        if (rc) return rc;
        // lnL of every task at its accepted length: one launch, one reduction, one all-reduce
        rc = eng_batch_lnl_enqueue(e, m);
        if (!rc) rc = comm_allreduce(e, 2 * m);
        if (!rc) rc = read_result(e, 2 * m);
        if (rc) return rc;
        const std::vector<double> lnl(e->h_result.p, e->h_result.p + 2 * (size_t)m);   // {lnl, prob_const} per task
        for (int t = 0; t < m; t++) {
            results[first + t].lnl = lnl[2 * t];
            if (isnan(lnl[2 * t]) || isinf(lnl[2 * t])) {   // phylokernel.h:1091-1109: redo this task alone (same decision on every rank)
                const iqhip_branch_task &k = tasks[first + t];
                rc = iqhip_compute_theta(e, k.a, k.b);
                if (!rc) rc = iqhip_lnl_from_theta(e, results[first + t].optx, &results[first + t].lnl);
            } else {
                rc = batch_asc_lnl(e, lnl[2 * t + 1], &results[first + t].lnl);
            }
            if (rc) return rc;
        }
    }
    return IQHIP_OK;
}

// iqhip_optimize_branch_batch, one task after the other through the chain form (IQHIP_BATCH_SEQUENTIAL=1: the form the
// batched chain is tested against)
static int optimize_branch_batch_sequential(iqhip_engine *e, const iqhip_branch_task *tasks, int ntasks,
                                            double *sum_scale, iqhip_branch_result *results) {
    size_t off = 0;
    for (int t = 0; t < ntasks; t++) {
        const iqhip_branch_task &k = tasks[t];
        if (k.nops < 0 || (k.nops > 0 && !k.ops)) return fail(IQHIP_ERR_INVALID, "bad ops array in a task");
        iqhip_branch_result &r = results[t];
        r.status = 0;
        int rc = iqhip_optimize_branch(e, k.ops, k.nops, k.a, k.b, k.xguess, k.x1, k.x2, k.xacc, k.max_steps,
                                       sum_scale ? sum_scale + off : nullptr, &r.optx, &r.d2l, &r.nsteps);
        if (rc) return rc;
        rc = iqhip_lnl_from_theta(e, r.optx, &r.lnl);
        if (rc) return rc;
        off += (size_t)k.nops;
    }
    return IQHIP_OK;
}

extern "C" int iqhip_optimize_branch_batch(iqhip_engine *e, const iqhip_branch_task *tasks, int ntasks,
                                           double *sum_scale, iqhip_branch_result *results) {
    return iqhip_optimize_branch_batch_rows(e, tasks, ntasks, sum_scale, results, nullptr);
}

// rows != NULL: after each chunk of k_newton_batch, k_ptnlh_rows (kernels_rell.hip) writes the per-pattern log-likelihood
// of every task with a row from the task's theta buffer (complete in memory once the launch has finished: the first
// evaluation of a task stores every tile of it, in both vector layouts) at the accepted length in the result block
extern "C" int iqhip_optimize_branch_batch_rows(iqhip_engine *e, const iqhip_branch_task *tasks, int ntasks,
                                                double *sum_scale, iqhip_branch_result *results, const int32_t *rows) {
    if (!e) return fail(IQHIP_ERR_INVALID, "null engine");
    if (!tasks || !results || ntasks < 1) return fail(IQHIP_ERR_INVALID, "bad task array");
    if (rows) {
        const int rc = require(e, "iqhip_optimize_branch_batch_rows", REQ_SINGLE_DEVICE);   // (the per-pattern store)
        if (rc) return rc;
        for (int t = 0; t < ntasks; t++)
            if (rows[t] >= e->ptnlh_rows)
                return fail(IQHIP_ERR_INVALID, "iqhip_optimize_branch_batch_rows: row outside the store (iqhip_ptnlh_reserve)");
    }
    const char *seq_env = getenv("IQHIP_BATCH_SEQUENTIAL");   // (read per call: the tests compare the two forms)
    const bool sequential = seq_env && atoi(seq_env) != 0;
    if (!e->shards.empty())
        return sequential ? optimize_branch_batch_sequential(e, tasks, ntasks, sum_scale, results)
                          : sharded::optimize_branch_batch(e, tasks, ntasks, sum_scale, results);
    if (e->comm)
        return sequential ? optimize_branch_batch_sequential(e, tasks, ntasks, sum_scale, results)
                          : optimize_branch_batch_comm(e, tasks, ntasks, sum_scale, results);
    int rc = check_ready(e);
    if (rc) return rc;
    std::vector<iqhip_node_op> all;
    std::vector<int> segs;
    rc = batch_gather_ops(tasks, ntasks, all, segs);
    if (rc) return rc;
    const int total_ops = (int)all.size();
    if (total_ops + 2 > e->result_cap) return fail(IQHIP_ERR_INVALID, "too many node updates in one submission");
    iqhip_branch_end none = {0, -1, 0};
    if (total_ops > 0) {
        rc = submit_traverse(e, all.data(), total_ops, false, none, none, 0.0, /*skip_reduce=*/false, &segs);
        if (rc) return rc;
    }
    // workgroups per task: every workgroup of a launch must be resident (grid barrier inside each task)
    // ... which bounds the batch by what fits the chip at once: 3 workgroups per CU (k_newton_batch: 145 VGPRs, i.e.
    // three waves per SIMD), fewer when its LDS (3 val arrays of a block + the exchange and +ASC cells) says so
    const size_t newton_lds = (size_t)(3 * e->block + 8) * sizeof(double) + 64;
    const int wg_per_cu = (int)std::max<size_t>(1, std::min<size_t>(3, (size_t)(150 * 1024) / newton_lds));
    const int capacity = e->num_cus * wg_per_cu;
    const int wgs_needed = (int)std::max<int64_t>(1, (e->ntiles + 3) / 4);
    int chunk = std::min(ntasks, capacity);             // tasks per launch
    {   // every task of a launch owns a theta buffer: keep them within a quarter of the free device memory and
        // run larger batches in several launches (protein+G4 at 50k patterns: 32 MB per task)
        size_t free_b = 0, total_b = 0;
        const size_t per_task = (size_t)e->nptn_pad * e->block * sizeof(double);
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
            const size_t have = e->d_theta_batch.cap * sizeof(double);
            const size_t room = (free_b + have) / 4;
            const size_t fit = std::max<size_t>(1, room / std::max<size_t>(1, per_task));
            if ((size_t)chunk > fit) chunk = (int)fit;
        }
    }
    chunk = batch_chunk(chunk);
    const int G = std::max(1, std::min(wgs_needed, capacity / chunk));
    const size_t theta_stride = (size_t)e->nptn_pad * e->block;
    HIPCHK(e->d_theta_batch.ensure(e, (size_t)chunk * theta_stride));
    if (chunk > e->batch_cap) {
        e->batch_cap = 0;
        HIPCHK(e->d_batch_partials.ensure(e, (size_t)chunk * 4 * (e->num_cus * 4)));
        HIPCHK(e->d_batch_out.ensure(e, (size_t)chunk * 6));
        HIPCHK(e->d_batch_barriers.ensure(e, (size_t)2 * chunk));
        HIPCHK(e->d_batch_tasks.ensure(e, newton_task_bytes() * (size_t)chunk));
        HIPCHK(hipMemsetAsync(e->d_batch_barriers.p, 0, sizeof(unsigned int) * 2 * chunk, e->stream));
        e->batch_cap = chunk;
    }
    std::vector<char> host_tasks(newton_task_bytes() * (size_t)chunk);
    std::vector<double> out((size_t)chunk * 6);
    if (rows) HIPCHK(e->d_batch_rows.ensure(e, (size_t)chunk));
    for (int first = 0; first < ntasks; first += chunk) {
        const int m = std::min(chunk, ntasks - first);
        for (int t = 0; t < m; t++) {
            const iqhip_branch_task &k = tasks[first + t];
            DevBranch br;
            rc = build_branch(e, k.a, k.b, 0.0, -1, &br);
            if (rc) return rc;
            newton_task_fill(host_tasks.data() + newton_task_bytes() * (size_t)t, br, k.xguess, k.x1, k.x2, k.xacc,
                             k.max_steps);
        }
        HIPCHK(hipMemcpyAsync(e->d_batch_tasks.p, host_tasks.data(), newton_task_bytes() * (size_t)m,
                              hipMemcpyHostToDevice, e->stream));
        // posted exchange of the tasks' partial sums (k_newton_batch): slots of this launch, [task][evaluation][workgroup][2]
        double *posts = nullptr, *posts_other = nullptr;
        size_t posts_other_used = 0;
        int post_epochs = 0;
        if (G > 1 && e->newton_posts) {
            int max_steps = 1;
            for (int t = 0; t < m; t++) max_steps = std::max(max_steps, tasks[first + t].max_steps);
            post_epochs = max_steps + 4;   // derivative evaluations + the lnL pass(es)
            const size_t need = (size_t)m * post_epochs * G * 2;
            if (2 * need > e->d_batch_posts.cap) {   // (two launch parities, half of the buffer each)
                HIPCHK(e->d_batch_posts.ensure(e, 2 * need));
                HIPCHK(hipMemsetAsync(e->d_batch_posts.p, 0xFF, 2 * need * sizeof(double), e->stream));
                e->batch_posts_used[0] = e->batch_posts_used[1] = 0;
            }
            const unsigned int pp = e->batch_post_launches & 1u;
            e->batch_post_launches++;
            posts = e->d_batch_posts.p + (size_t)pp * (e->d_batch_posts.cap / 2);
            posts_other = e->d_batch_posts.p + (size_t)(1u - pp) * (e->d_batch_posts.cap / 2);
            posts_other_used = e->batch_posts_used[1u - pp];
            e->batch_posts_used[pp] = need;
            e->batch_posts_used[1u - pp] = 0;   // (reset by this launch)
        }
        const unsigned int parity = e->batch_launches & 1u;
        e->batch_launches++;
        // this launch's arrival counters start at zero whatever the task counts of earlier launches were (a launch
        // only clears the first m counters of the other parity, so a smaller batch in between leaves the rest dirty)
        HIPCHK(hipMemsetAsync(e->d_batch_barriers.p + (size_t)parity * e->batch_cap, 0, sizeof(unsigned int) * (size_t)m,
                              e->stream));
        HIPCHK(launch_newton_batch(e, e->d_batch_tasks.p, m, G, e->d_theta_batch.p, theta_stride, e->d_batch_partials.p,
                                   e->d_batch_barriers.p + (size_t)parity * e->batch_cap,
                                   e->d_batch_barriers.p + (size_t)(1u - parity) * e->batch_cap, e->d_batch_out.p, posts, posts_other,
                                   posts_other_used, post_epochs));
        if (rows) {   // (the theta buffers are reused by the next chunk: per chunk)
            HIPCHK(hipMemcpyAsync(e->d_batch_rows.p, rows + first, sizeof(int32_t) * (size_t)m, hipMemcpyHostToDevice, e->stream));
            HIPCHK(launch_ptnlh_rows(e, e->d_batch_tasks.p, m, e->d_theta_batch.p, theta_stride, e->d_batch_out.p, e->d_batch_rows.p));
        }
        HIPCHK(hipMemcpyAsync(out.data(), e->d_batch_out.p, sizeof(double) * 6 * (size_t)m, hipMemcpyDeviceToHost,
                              e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));  // also: host_tasks / out are reused by the next chunk
        for (int t = 0; t < m; t++) {
            const double *o = &out[(size_t)t * 6];
            iqhip_branch_result &r = results[first + t];
            NewtonResult(o).store(r);   // (a status 2 or 3 goes to the caller in r.status)
            r.lnl = o[4];
            if (r.status == 4) {
                // the task's grid barrier gave up (its workgroups were not co-resident): redo this one task with the
                // barrier-free chain form -- its node updates have run, so only theta + the solve + lnL remain
                const iqhip_branch_task &k = tasks[first + t];
                (void)hipStreamSynchronize(e->stream);
                rc = iqhip_compute_theta(e, k.a, k.b);
                if (!rc) rc = newton_chain(e, k.xguess, k.x1, k.x2, k.xacc, k.max_steps, &r.optx, &r.d2l, &r.nsteps);
                if (!rc) rc = iqhip_lnl_from_theta(e, r.optx, &r.lnl);
                if (!rc && rows && rows[first + t] >= 0) rc = iqhip_ptnlh_put_current(e, rows[first + t], k.a, k.b);
                if (rc) return rc;
                r.status = 0;
            }
        }
    }
    if (total_ops > 0) {
        rc = read_result(e, 2 + total_ops);
        if (rc) return rc;
        if (sum_scale)
            for (int k = 0; k < total_ops; k++) sum_scale[k] = e->h_result.p[2 + k];
    }
    return IQHIP_OK;
}
