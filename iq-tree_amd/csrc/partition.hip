// partition.hip -- host side of the edge-linked partition model (-q / -spp): a group of existing single-device engines,
// one per partition (partition.h), its life cycle and the joint branch solves that span the members (include/iqhip.h,
// "Edge-linked partition models").  The kernels are in kernels_partnewton.hip.  The group owns a stream, a device-resident
// NewtonState, the descriptor table of its members and the work-item slots; it owns nothing of the members.  (The group's
// per-pattern rows, RELL sums and UFBoot are in ufboot.hip, its joint pairwise distances in pairdist.hip.)
//
// Descriptors: re-filled from the members' engine fields on EVERY call (a few hundred bytes per member) and uploaded only
// when the bytes differ from what the device holds -- so a new model, alignment, theta buffer or rate is picked up without
// a generation counter on the engine.
// Streams: every call first makes the group's stream wait for an event recorded on each member's stream (the thetas and
// vectors the group reads are complete), and after its last launch makes every member's stream wait for an event of the
// group's stream (no member overwrites theta while the group still reads it).  The host waits once, for the group's stream.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "partition.h"

using namespace iqhip;

namespace {

constexpr int kPartItemTiles4 = 16;     // 64-pattern tiles per work item (4-state engines): 1024 patterns
constexpr int kPartItemTilesM = 32;     // 16-pattern tiles per work item (matrix-core engines): 512 patterns

// what a member must be, at create and again at every call (a model or a correction may have been set since)
int member_ok(const iqhip_engine *e, int p) {
    const std::string who = "partition member " + std::to_string(p);
    if (!e) return fail(IQHIP_ERR_INVALID, who + ": null engine");
    if (!e->shards.empty() || e->comm)
        return fail(IQHIP_ERR_UNSUPPORTED, who + ": sharded engines and communicator ranks cannot join a partition group");
    if (e->planner) return fail(IQHIP_ERR_INVALID, who + ": planning-only engine");
    if (!e->model_set || !e->aln_set) return fail(IQHIP_ERR_INVALID, who + ": needs iqhip_set_model and iqhip_set_alignment first");
    if (e->asc_active || e->n_unobs > 0)
        return fail(IQHIP_ERR_UNSUPPORTED, who + ": ascertainment bias correction is not available in a partition group");
    if (e->nclass > 1) return fail(IQHIP_ERR_UNSUPPORTED, who + ": mixture models are not available in a partition group");
    return IQHIP_OK;
}

int members_ok(const iqhip_partition *g) {
    for (int p = 0; p < g->nparts; p++) {
        const int rc = member_ok(g->m[p], p);
        if (rc) return rc;
    }
    return IQHIP_OK;
}

bool same_end(const iqhip_branch_end &x, const iqhip_branch_end &y) {
    if (x.leaf >= 0 || y.leaf >= 0) return x.leaf == y.leaf;
    return x.key == y.key;
}

int thetas_ok(const iqhip_partition *g, const char *what) {
    for (int p = 0; p < g->nparts; p++) {
        const iqhip_engine *e = g->m[p], *e0 = g->m[0];
        if (!e->theta_valid)
            return fail(IQHIP_ERR_INVALID, std::string(what) + ": theta not computed on member " + std::to_string(p));
        // (two internal ends come in the caller's order)
        const bool same = (same_end(e->theta_end[0], e0->theta_end[0]) && same_end(e->theta_end[1], e0->theta_end[1])) ||
                          (same_end(e->theta_end[0], e0->theta_end[1]) && same_end(e->theta_end[1], e0->theta_end[0]));
        if (!same)
            return fail(IQHIP_ERR_INVALID, std::string(what) + ": theta of member " + std::to_string(p) +
                                               " was built for another branch than that of member 0");
    }
    return IQHIP_OK;
}

// the descriptor table from the members as they are now; uploaded when its bytes changed
int refresh_table(iqhip_partition *g) {
    const int P = g->nparts;
    std::vector<PartDesc> desc((size_t)P);
    std::vector<PartItem> items;
    int maxB = 0;
    for (int p = 0; p < P; p++) {
        const iqhip_engine *e = g->m[p];
        PartDesc &D = desc[p];
        memset(&D, 0, sizeof D);
        D.theta = e->d_theta.p;
        D.evalc = e->d_evalc;
        D.rates = e->d_rates;
        D.props = e->d_props;
        D.freq = e->d_freq.p;
        D.invar = e->d_invar.p;
        D.a_sc = e->theta_a_sc;
        D.b_sc = e->theta_b_sc;
        D.nptn = e->nptn;
        D.ntiles = e->ntiles;
        D.n = e->n;
        D.ncat = e->ncat;
        D.mfma = e->mfma ? 1 : 0;
        D.rate = g->rate[p];
        D.item_first = (int32_t)items.size();
        const int64_t per = e->mfma ? kPartItemTilesM : kPartItemTiles4;
        for (int64_t t = 0; t < e->ntiles; t += per) {
            PartItem it;
            it.first_tile = t;
            it.member = p;
            it.ntiles = (int32_t)std::min<int64_t>(per, e->ntiles - t);
            items.push_back(it);
        }
        D.nitems = (int32_t)items.size() - D.item_first;
        maxB = std::max(maxB, e->block);
        if (items.size() > (size_t)1 << 30) return fail(IQHIP_ERR_UNSUPPORTED, "partition group: too many work items");
    }
    if ((size_t)(3 * maxB + 8) * sizeof(double) > kPartMaxLdsBytes)
        return fail(IQHIP_ERR_UNSUPPORTED, "partition group: nstates * ncat of a member exceeds the solve's LDS");
    g->lds_doubles = 3 * maxB;
    g->nitems = (int)items.size();
    const size_t bytes_desc = sizeof(PartDesc) * (size_t)P, bytes = bytes_desc + sizeof(PartItem) * items.size();
    std::vector<char> now(bytes);
    memcpy(now.data(), desc.data(), bytes_desc);
    memcpy(now.data() + bytes_desc, items.data(), bytes - bytes_desc);
    HIPCHK(g->d_partials.ensure(g->stream, 2 * (size_t)g->nitems));
    if (now == g->uploaded) return IQHIP_OK;
    if (bytes > g->table.d.cap) g->uploaded.clear();   // (a new buffer holds nothing)
    HIPCHK(g->table.ensure(g->stream, bytes));
    // (the staging is free: every call of the group ends with a wait for its stream)
    memcpy(g->table.h.p, now.data(), bytes);
    HIPCHK(hipMemcpyAsync(g->table.d.p, g->table.h.p, bytes, hipMemcpyHostToDevice, g->stream));
    g->uploaded.swap(now);
    return IQHIP_OK;
}

const PartDesc *d_desc(const iqhip_partition *g) { return reinterpret_cast<const PartDesc *>(g->table.d.p); }
const PartItem *d_items(const iqhip_partition *g) {
    return reinterpret_cast<const PartItem *>(g->table.d.p + sizeof(PartDesc) * (size_t)g->nparts);
}

}  // namespace

int iqhip::wait_for_members(iqhip_partition *g) {
    for (int p = 0; p < g->nparts; p++) {
        HIPCHK(hipEventRecord(g->ev[p], g->m[p]->stream));
        HIPCHK(hipStreamWaitEvent(g->stream, g->ev[p], 0));
    }
    return IQHIP_OK;
}
int iqhip::members_wait(iqhip_partition *g) {
    HIPCHK(hipEventRecord(g->ev_done, g->stream));
    for (int p = 0; p < g->nparts; p++) HIPCHK(hipStreamWaitEvent(g->m[p]->stream, g->ev_done, 0));
    return IQHIP_OK;
}

int iqhip::use_group(iqhip_partition *g, const char *what) {
    if (!g) return fail(IQHIP_ERR_INVALID, std::string(what) + ": null group");
    const int rc = members_ok(g);
    if (rc) return rc;
    HIPCHK(hipSetDevice(g->device));
    return IQHIP_OK;
}

int iqhip::group_rows_ok(const iqhip_partition *g, const char *what, const int32_t *rows, int nrows) {
    for (int p = 0; p < g->nparts; p++)
        for (int i = 0; i < nrows; i++)
            if (rows[i] < 0 || rows[i] >= g->m[p]->ptnlh_rows)
                return fail(IQHIP_ERR_INVALID, std::string(what) + ": row outside the store of member " + std::to_string(p) +
                                                   " (iqhip_partition_ptnlh_reserve)");
    return IQHIP_OK;
}

namespace {

// the MODE 1 pass over the thetas -> out.h[0 .. nparts) after the caller's wait for the stream; st: at its result, only once
// it is done (the pass is enqueued behind a chunk of steps that may not have finished the solve)
int enqueue_part_lnl(iqhip_partition *g, const NewtonState *st, double x) {
    HIPCHK(launch_part_derv(g->stream, 1, d_desc(g), d_items(g), g->nitems, g->lds_doubles, st, x, g->d_partials.p));
    HIPCHK(launch_part_lnl_finish(g->stream, d_desc(g), g->nparts, g->d_partials.p, g->out.d.p));
    HIPCHK(hipMemcpyAsync(g->out.h.p, g->out.d.p, sizeof(double) * (size_t)g->nparts, hipMemcpyDeviceToHost, g->stream));
    g->launches += 2;
    return IQHIP_OK;
}

// one evaluation of an enqueued chain: the derivative launch, then the update launch, a round of the timer's two phases
template <typename Derv, typename Update>
int enqueue_step(iqhip_partition *g, PhaseTimer &timer, Derv &&derv, Update &&update) {
    timer.mark();
    HIPCHK(derv());
    timer.mark();
    HIPCHK(update());
    timer.mark();
    g->launches += 2;
    return IQHIP_OK;
}

int steps_per_chunk(int enqueued, int max_steps) {
    int chunk_env = 0;
    if (const char *s = getenv("IQHIP_PART_STEPS")) chunk_env = atoi(s);
    return chunk_env > 0 ? chunk_env : (enqueued == 0 ? std::min(4, max_steps + 1) : 2);
}

int solve(iqhip_partition *g, double xguess, double x1, double x2, double xacc, int max_steps, bool want_lnl,
          NewtonState *result) {
    PhaseTimer timer(g->m[0]->timing, g->stream, 2);   // iqhip_debug_partition_timing: derivative, update, summed over the steps
    if (g->m[0]->timing) g->ms[0] = g->ms[1] = 0.0;
    HIPCHK(launch_newton_state_init_on(g->stream, g->state.d.p, xguess, x1, x2, xacc, max_steps));
    g->launches++;
    for (int enq = 0;;) {
        const int chunk = steps_per_chunk(enq, max_steps);
        for (int k = 0; k < chunk; k++) {
            const int rc = enqueue_step(
                g, timer,
                [&] {
                    return launch_part_derv(g->stream, 0, d_desc(g), d_items(g), g->nitems, g->lds_doubles, g->state.d.p, 0.0,
                                            g->d_partials.p);
                },
                [&] { return launch_part_newton_update(g->stream, d_desc(g), g->nparts, g->d_partials.p, g->state.d.p); });
            if (rc) return rc;
        }
        enq += chunk;
        if (want_lnl) {
            const int rc = enqueue_part_lnl(g, g->state.d.p, 0.0);
            if (rc) return rc;
        }
        HIPCHK(hipMemcpyAsync(g->state.h.p, g->state.d.p, sizeof(NewtonState), hipMemcpyDeviceToHost, g->stream));
        HIPCHK(hipStreamSynchronize(g->stream));
        if (g->state.h.p->done) break;
        if (enq > max_steps + 2) return fail(IQHIP_ERR_INVALID, "Newton chain did not terminate");
    }
    timer.read(g->ms);
    *result = *g->state.h.p;
    return IQHIP_OK;
}

}  // namespace

extern "C" int iqhip_partition_create(iqhip_partition **out, iqhip_engine *const *members, int nparts) {
    if (!out || !members) return fail(IQHIP_ERR_INVALID, "iqhip_partition_create: null argument");
    *out = nullptr;
    if (nparts < 1) return fail(IQHIP_ERR_INVALID, "iqhip_partition_create: nparts < 1");
    for (int p = 0; p < nparts; p++) {
        const int rc = member_ok(members[p], p);
        if (rc) return rc;
        if (members[p]->device != members[0]->device)
            return fail(IQHIP_ERR_INVALID, "iqhip_partition_create: all members must sit on one device");
    }
    {
        std::vector<iqhip_engine *> sorted(members, members + nparts);
        std::sort(sorted.begin(), sorted.end());
        if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end())
            return fail(IQHIP_ERR_INVALID, "iqhip_partition_create: a member is listed twice");
    }
    iqhip_partition *g = new iqhip_partition;
    g->device = members[0]->device;
    g->nparts = nparts;
    g->m.assign(members, members + nparts);
    g->rate.assign((size_t)nparts, 1.0);
    hipError_t s = hipSetDevice(g->device);
    if (s == hipSuccess) s = hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking);
    if (s == hipSuccess) s = hipEventCreateWithFlags(&g->ev_done, hipEventDisableTiming);
    for (int p = 0; p < nparts && s == hipSuccess; p++) {
        hipEvent_t e = nullptr;
        s = hipEventCreateWithFlags(&e, hipEventDisableTiming);
        if (s == hipSuccess) g->ev.push_back(e);
    }
    if (s == hipSuccess) s = g->state.ensure(g->stream, 1);
    if (s == hipSuccess) s = g->out.ensure(g->stream, (size_t)nparts);
    if (s == hipSuccess) s = g->scale.ensure(g->stream, (size_t)nparts);
    if (s != hipSuccess) {
        iqhip_partition_destroy(g);
        return fail(IQHIP_ERR_HIP, std::string("iqhip_partition_create: ") + hipGetErrorString(s));
    }
    *out = g;
    return IQHIP_OK;
}

extern "C" void iqhip_partition_destroy(iqhip_partition *g) {
    if (!g) return;
    (void)hipSetDevice(g->device);
    if (g->stream) (void)hipStreamSynchronize(g->stream);
    for (hipEvent_t e : g->ev) hipEventDestroy(e);
    if (g->ev_done) hipEventDestroy(g->ev_done);
    if (g->stream) hipStreamDestroy(g->stream);
    delete g;   // (its buffers free themselves: the stream has drained)
}

extern "C" int iqhip_partition_set_rates(iqhip_partition *g, const double *rate) {
    if (!g || !rate) return fail(IQHIP_ERR_INVALID, "iqhip_partition_set_rates: null argument");
    for (int p = 0; p < g->nparts; p++)
        if (!(rate[p] > 0.0) || !std::isfinite(rate[p]))
            return fail(IQHIP_ERR_INVALID, "iqhip_partition_set_rates: every rate must be finite and > 0");
    g->rate.assign(rate, rate + g->nparts);
    return IQHIP_OK;
}

extern "C" int iqhip_partition_newton_branch(iqhip_partition *g, double xguess, double x1, double x2, double xacc,
                                             int max_steps, double *optx, double *d2l, int *nsteps, double *part_lnl) {
    const char *what = "iqhip_partition_newton_branch";
    int rc = newton_check_bounds(what, xguess, x1, x2, xacc, max_steps);
    if (rc) return rc;
    rc = use_group(g, what);
    if (rc) return rc;
    rc = thetas_ok(g, what);
    if (rc) return rc;
    g->launches = 0;
    rc = refresh_table(g);
    if (rc) return rc;
    rc = wait_for_members(g);
    if (rc) return rc;
    NewtonState st;
    rc = solve(g, xguess, x1, x2, xacc, max_steps, part_lnl != nullptr, &st);
    // (whatever happened: the members wait for what the group did enqueue)
    const int rc2 = members_wait(g);
    if (rc) return rc;
    if (rc2) return rc2;
    rc = newton_status(st.status);
    if (rc) return rc;
    NewtonResult(st).store(optx, d2l, nsteps);
    if (part_lnl) memcpy(part_lnl, g->out.h.p, sizeof(double) * (size_t)g->nparts);
    return IQHIP_OK;
}

extern "C" int iqhip_partition_lnl_from_theta(iqhip_partition *g, double x, double *part_lnl) {
    const char *what = "iqhip_partition_lnl_from_theta";
    if (!part_lnl) return fail(IQHIP_ERR_INVALID, std::string(what) + ": null argument");
    if (!(x >= 0.0) || !std::isfinite(x)) return fail(IQHIP_ERR_INVALID, std::string(what) + ": negative or non-finite branch length");
    int rc = use_group(g, what);
    if (rc) return rc;
    rc = thetas_ok(g, what);
    if (rc) return rc;
    g->launches = 0;
    rc = refresh_table(g);
    if (rc) return rc;
    rc = wait_for_members(g);
    if (rc) return rc;
    rc = enqueue_part_lnl(g, nullptr, x);
    const int rc2 = members_wait(g);
    if (rc) return rc;
    if (rc2) return rc2;
    HIPCHK(hipStreamSynchronize(g->stream));
    memcpy(part_lnl, g->out.h.p, sizeof(double) * (size_t)g->nparts);
    return IQHIP_OK;
}

extern "C" int iqhip_partition_traverse_lnl(iqhip_partition *g, const iqhip_node_op *ops, int nops, iqhip_branch_end a,
                                            iqhip_branch_end b, double len, const double *scale, double *part_lnl) {
    const char *what = "iqhip_partition_traverse_lnl";
    if (!part_lnl) return fail(IQHIP_ERR_INVALID, std::string(what) + ": null argument");
    if (nops < 0 || (nops > 0 && !ops)) return fail(IQHIP_ERR_INVALID, std::string(what) + ": bad ops array");
    int rc = use_group(g, what);
    if (rc) return rc;
    const int P = g->nparts;
    for (int p = 0; scale && p < P; p++)
        if (!(scale[p] > 0.0) || !std::isfinite(scale[p]))
            return fail(IQHIP_ERR_INVALID, std::string(what) + ": every scale must be finite and > 0");
    g->launches = 0;
    std::vector<iqhip_node_op> mine(ops, ops + nops);
    for (int p = 0; p < P; p++) {
        iqhip_engine *e = g->m[p];
        const double s = scale ? scale[p] : g->rate[p];
        for (int k = 0; k < nops; k++) {
            mine[k].left_len = ops[k].left_len * s;
            mine[k].right_len = ops[k].right_len * s;
        }
        rc = submit_traverse(e, nops ? mine.data() : nullptr, nops, true, a, b, len * s);
        if (rc) return rc;
        if (e->d_result != e->d_result_own)   // caller-bound device result vector
            HIPCHK(hipMemcpyAsync(e->h_result.p, e->d_result, sizeof(double) * (size_t)(2 + nops), hipMemcpyDeviceToHost, e->stream));
        DevBranch br;
        rc = build_branch(e, a, b, len * s, -1, &br);   // (a lookup: the scale counters of the two ends)
        if (rc) return rc;
        g->scale.h.p[p] = PartScale{br.a_sc, br.b_sc, e->d_freq.p, e->nptn};
    }
    HIPCHK(hipSetDevice(g->device));
    rc = wait_for_members(g);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(g->scale.d.p, g->scale.h.p, sizeof(PartScale) * (size_t)P, hipMemcpyHostToDevice, g->stream));
    HIPCHK(launch_part_scale_terms(g->stream, g->scale.d.p, P, g->out.d.p));
    g->launches++;
    HIPCHK(hipMemcpyAsync(g->out.h.p, g->out.d.p, sizeof(double) * (size_t)P, hipMemcpyDeviceToHost, g->stream));
    rc = members_wait(g);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(g->stream));   // the one wait: every member's stream has drained behind its event
    for (int p = 0; p < P; p++) {
        iqhip_engine *e = g->m[p];
        result_arrived(e);
        double v = e->h_result.p[0];
        if (isnan(v) || isinf(v)) {   // phylokernel.h:848-866, the rare slow path
            rc = eng_repair_lnl(e, &v);
            if (rc) return rc;
        }
        part_lnl[p] = v + g->out.h.p[p];
    }
    return IQHIP_OK;
}

namespace {

// Tasks per chunk of a batch: every task owns a theta slot on every member.  All members' slots together stay within a
// quarter of the free device memory (what the slots hold already counts as free); IQHIP_PART_BATCH_CHUNK, read per call,
// lowers the bound.
int batch_tasks_per_chunk(const iqhip_partition *g, int ntasks) {
    int chunk = std::min(ntasks, kBatchChainChunk);
    size_t per_task = 0, have = 0;
    for (const iqhip_engine *e : g->m) {
        per_task += (size_t)e->nptn_pad * e->block * sizeof(double);
        have += e->d_theta_batch.cap * sizeof(double);
        chunk = std::min(chunk, std::max(1, e->result_cap / 2));   // (eng_batch_prepare's own bound)
    }
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
        const size_t fit = std::max<size_t>(1, ((free_b + have) / 4) / std::max<size_t>(1, per_task));
        if ((size_t)chunk > fit) chunk = (int)fit;
    }
    // (it cannot raise the bound, which is memory and eng_batch_prepare's limit: the rule of IQHIP_BATCH_CHUNK, batch_chunk())
    if (const char *s = getenv("IQHIP_PART_BATCH_CHUNK")) chunk = std::max(1, std::min(chunk, atoi(s)));
    return chunk;
}

// one chunk of m tasks: node updates and theta slots on the members' streams, the chain of joint solves on the group's
// ops[0 .. total_ops): the tasks' node updates in task order, seg_of[t] of them task t's
// rows (nullptr: none): per task the row of every member's store that takes its per-pattern values (< 0: none), all checked
int batch_run_chunk(iqhip_partition *g, const iqhip_branch_task *tasks, int m, const iqhip_node_op *ops, int total_ops,
                    const int *seg_of, iqhip_branch_result *results, double *part_lnl, const int32_t *rows) {
    const int P = g->nparts;
    const std::vector<int> segs(seg_of, seg_of + m);
    int rc = IQHIP_OK;
    std::vector<NewtonState> init((size_t)m);
    int max_steps = 1;
    for (int t = 0; t < m; t++) {
        const iqhip_branch_task &k = tasks[t];
        newton_init(init[t], k.xguess, k.x1, k.x2, k.xacc, k.max_steps);
        max_steps = std::max(max_steps, k.max_steps);
    }
    const size_t bytes_slots = sizeof(PartSlots) * (size_t)P;
    const size_t bytes_sc = sizeof(const int16_t *) * 2 * (size_t)m * P;
    const size_t bytes_table = bytes_slots + bytes_sc + (rows ? sizeof(double *) * (size_t)m * P : 0);
    HIPCHK(hipSetDevice(g->device));
    HIPCHK(g->bstate.ensure(g->stream, (size_t)m));
    HIPCHK(g->btable.ensure(g->stream, bytes_table));
    HIPCHK(g->bout.ensure(g->stream, (size_t)m * P));
    HIPCHK(g->d_bpartials.ensure(g->stream, 2 * (size_t)m * g->nitems));
    HIPCHK(g->d_blnl.ensure(g->stream, (size_t)m));
    PartSlots *slots = reinterpret_cast<PartSlots *>(g->btable.h.p);
    const int16_t **sc = reinterpret_cast<const int16_t **>(g->btable.h.p + bytes_slots);
    double **rowp = reinterpret_cast<double **>(g->btable.h.p + bytes_slots + bytes_sc);
    std::vector<iqhip_node_op> mine(ops, ops + total_ops);
    const iqhip_branch_end none = {0, -1, 0};
    for (int p = 0; p < P; p++) {
        iqhip_engine *e = g->m[p];
        if (total_ops > 0) {
            const double r = g->rate[p];
            for (int k = 0; k < total_ops; k++) {
                mine[k].left_len = ops[k].left_len * r;
                mine[k].right_len = ops[k].right_len * r;
            }
            // (no reduction: the sum_scale rows are not read; the lnL takes its scale term from the counters)
            rc = submit_traverse(e, mine.data(), total_ops, false, none, none, 0.0, /*skip_reduce=*/true, &segs);
            if (rc) return rc;
        }
        rc = eng_batch_prepare(e, tasks, m, nullptr);   // (the states are the group's)
        if (rc) return rc;
        slots[p] = PartSlots{e->d_theta_batch.p, (size_t)e->nptn_pad * e->block};
        for (int t = 0; t < m; t++) {
            rc = branch_scale_counters(e, tasks[t].a, tasks[t].b, sc + 2 * ((size_t)t * P + p));
            if (rc) return rc;
            if (rows) rowp[(size_t)t * P + p] = rows[t] >= 0 ? e->d_ptnlh.p + (size_t)rows[t] * e->nptn_pad : nullptr;
        }
    }
    HIPCHK(hipSetDevice(g->device));
    rc = wait_for_members(g);
    if (rc) return rc;
    memcpy(g->bstate.h.p, init.data(), sizeof(NewtonState) * (size_t)m);
    HIPCHK(hipMemcpyAsync(g->bstate.d.p, g->bstate.h.p, sizeof(NewtonState) * (size_t)m, hipMemcpyHostToDevice, g->stream));
    HIPCHK(hipMemcpyAsync(g->btable.d.p, g->btable.h.p, bytes_table, hipMemcpyHostToDevice, g->stream));
    HIPCHK(hipMemsetAsync(g->d_blnl.p, 0, sizeof(int32_t) * (size_t)m, g->stream));
    const PartSlots *d_slots = reinterpret_cast<const PartSlots *>(g->btable.d.p);
    const int16_t *const *d_sc = reinterpret_cast<const int16_t *const *>(g->btable.d.p + bytes_slots);
    double *const *d_rowp = rows ? reinterpret_cast<double *const *>(g->btable.d.p + bytes_slots + bytes_sc) : nullptr;
    PhaseTimer timer(g->m[0]->timing, g->stream, 2);
    const auto derv = [&](int mode) {
        return launch_part_derv_batch(g->stream, mode, d_desc(g), d_items(g), g->nitems, g->lds_doubles, d_slots, d_sc, P,
                                      g->bstate.d.p, g->d_blnl.p, m, g->d_bpartials.p, mode == 1 ? d_rowp : nullptr);
    };
    for (int enq = 0;;) {
        const int chunk = steps_per_chunk(enq, max_steps);
        for (int k = 0; k < chunk; k++) {
            rc = enqueue_step(g, timer, [&] { return derv(0); }, [&] {
                return launch_part_newton_update_batch(g->stream, d_desc(g), P, g->nitems, g->d_bpartials.p, g->bstate.d.p, m);
            });
            if (rc) return rc;
        }
        enq += chunk;
        // the lnL pass rides behind every chunk of steps (the host cannot know which is the last): a task still solving
        // does nothing, a task done in an earlier chunk has its sums already, and what the last finish wrote is what is read
        HIPCHK(derv(1));
        HIPCHK(launch_part_lnl_finish_batch(g->stream, d_desc(g), P, g->nitems, g->d_bpartials.p, g->bstate.d.p, g->d_blnl.p, g->bout.d.p,
                                            m));
        g->launches += 2;
        HIPCHK(hipMemcpyAsync(g->bout.h.p, g->bout.d.p, sizeof(double) * (size_t)m * P, hipMemcpyDeviceToHost, g->stream));
        HIPCHK(hipMemcpyAsync(g->bstate.h.p, g->bstate.d.p, sizeof(NewtonState) * (size_t)m, hipMemcpyDeviceToHost, g->stream));
        HIPCHK(hipStreamSynchronize(g->stream));
        if (std::all_of(g->bstate.h.p, g->bstate.h.p + m, [](const NewtonState &s) { return s.done != 0; })) break;
        if (enq > max_steps + 2) return fail(IQHIP_ERR_INVALID, "Newton chain did not terminate");
    }
    // (the group's stream waited for the members' and has drained: so have their submissions)
    for (iqhip_engine *e : g->m) result_arrived(e);
    double ms[2];   // (the entry point zeroed the sums: they run over the chunks of the call)
    if (timer.read(ms)) {
        g->ms[0] += ms[0];
        g->ms[1] += ms[1];
    }
    for (int t = 0; t < m; t++) {
        NewtonResult(g->bstate.h.p[t]).store(results[t]);   // (a status 2 or 3 goes to the caller in results[t].status)
        const double *o = g->bout.h.p + (size_t)t * P;
        double lnl = 0.0;
        for (int p = 0; p < P; p++) lnl += o[p];
        results[t].lnl = lnl;
        if (part_lnl) memcpy(part_lnl + (size_t)t * P, o, sizeof(double) * (size_t)P);
    }
    return IQHIP_OK;
}

}  // namespace

extern "C" int iqhip_partition_optimize_branch_batch(iqhip_partition *g, const iqhip_branch_task *tasks, int ntasks,
                                                     iqhip_branch_result *results, double *part_lnl) {
    return iqhip_partition_optimize_branch_batch_rows(g, tasks, ntasks, results, part_lnl, nullptr);
}

extern "C" int iqhip_partition_optimize_branch_batch_rows(iqhip_partition *g, const iqhip_branch_task *tasks, int ntasks,
                                                          iqhip_branch_result *results, double *part_lnl, const int32_t *rows) {
    const char *what = rows ? "iqhip_partition_optimize_branch_batch_rows" : "iqhip_partition_optimize_branch_batch";
    if (!g) return fail(IQHIP_ERR_INVALID, std::string(what) + ": null group");
    if (!tasks || !results || ntasks < 1) return fail(IQHIP_ERR_INVALID, std::string(what) + ": bad task array");
    // every task is checked before any member is touched; a chunk takes its slice of the gathered ops
    std::vector<iqhip_node_op> ops;
    std::vector<int> segs;
    int rc = batch_gather_ops(tasks, ntasks, ops, segs);
    if (rc) return rc;
    rc = use_group(g, what);
    if (rc) return rc;
    if (rows) {   // inside every member's store, and no row named twice: two tasks' passes would store to it in one launch
        std::vector<int32_t> named;
        for (int t = 0; t < ntasks; t++)
            if (rows[t] >= 0) {
                if ((rc = group_rows_ok(g, what, rows + t, 1))) return rc;
                named.push_back(rows[t]);
            }
        std::sort(named.begin(), named.end());
        if (std::adjacent_find(named.begin(), named.end()) != named.end())
            return fail(IQHIP_ERR_INVALID, std::string(what) + ": two tasks name the same row");
    }
    g->launches = 0;
    if (g->m[0]->timing) g->ms[0] = g->ms[1] = 0.0;
    rc = refresh_table(g);
    if (rc) return rc;
    const int chunk = batch_tasks_per_chunk(g, ntasks);
    size_t op_first = 0;
    for (int first = 0; first < ntasks && !rc; first += chunk) {
        const int m = std::min(chunk, ntasks - first);
        size_t nops = 0;
        for (int t = 0; t < m; t++) nops += (size_t)segs[first + t];
        rc = batch_run_chunk(g, tasks + first, m, ops.data() + op_first, (int)nops, segs.data() + first, results + first,
                             part_lnl ? part_lnl + (size_t)first * g->nparts : nullptr, rows ? rows + first : nullptr);
        op_first += nops;
        // (whatever happened: the members wait for what the group did enqueue, and no slot is rewritten under it)
        const int rc2 = members_wait(g);
        if (!rc) rc = rc2;
    }
    if (rc) (void)hipStreamSynchronize(g->stream);   // (the staging buffers are free for the next call)
    return rc;
}

extern "C" int iqhip_debug_partition_timing(iqhip_partition *g, double *ms, int64_t *launches) {
    if (!g) return fail(IQHIP_ERR_INVALID, "iqhip_debug_partition_timing: null group");
    if (ms) { ms[0] = g->ms[0]; ms[1] = g->ms[1]; }
    if (launches) *launches = g->launches;
    return IQHIP_OK;
}
