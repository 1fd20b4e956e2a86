// partition.hip -- host side of the edge-linked partition model (-q / -spp): a group of existing single-device engines,
// one per partition, and the calls that span them (include/iqhip.h, "Edge-linked partition models").  The kernels are in
// kernels_partnewton.hip.  The group owns a stream, a device-resident NewtonState, the descriptor table of its members and
// the work-item slots; it owns nothing of the members.  At the end of the file: the group's per-pattern rows, RELL sums and
// UFBoot state ("UFBoot on edge-linked partition models"; kernels in kernels_partboot.hip).
//
// Descriptors: re-filled from the members' engine fields on EVERY call (a few hundred bytes per member) and uploaded only
// when the bytes differ from what the device holds -- so a new model, alignment, theta buffer or rate is picked up without
// a generation counter on the engine.
// Streams: every call first makes the group's stream wait for an event recorded on each member's stream (the thetas and
// vectors the group reads are complete), and after its last launch makes every member's stream wait for an event of the
// group's stream (no member overwrites theta while the group still reads it).  The host waits once, for the group's stream.
// The joint pairwise distances (end of the file; kernel in kernels_partdist.hip) follow the same rule chunk by chunk: the
// members count a chunk of pairs on their own streams, the group solves it, and no member counts the next chunk before.
#include <float.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "iqhip_internal.h"
#include "partpair_layout.h"

using namespace iqhip;

namespace {
constexpr int kPartItemTiles4 = 16;     // 64-pattern tiles per work item (4-state engines): 1024 patterns
constexpr int kPartItemTilesM = 32;     // 16-pattern tiles per work item (matrix-core engines): 512 patterns
constexpr size_t kPartMaxLdsBytes = 64 * 1024;
}  // namespace

struct iqhip_partition {
    int device = 0, nparts = 0;
    std::vector<iqhip_engine *> m;
    std::vector<double> rate;
    hipStream_t stream = nullptr;
    std::vector<hipEvent_t> ev;      // one per member, recorded on its stream
    hipEvent_t ev_done = nullptr;    // recorded on the group's stream behind its last launch
    PairBuf<char> table;             // [nparts] PartDesc ++ [nitems] PartItem
    std::vector<char> uploaded;      // the bytes of `table` the device holds
    PairBuf<PartScale> scale;
    PairBuf<double> out;             // per member: lnL sums / scale-factor terms
    PairBuf<NewtonState> state;
    DevBuf<double> d_partials;       // [nitems][2]
    // iqhip_partition_optimize_branch_batch, per chunk of tasks
    PairBuf<NewtonState> bstate;     // [tasks]
    PairBuf<char> btable;            // [nparts] PartSlots ++ [tasks][nparts][2] scale-counter pointers ++ [tasks][nparts] row pointers
    PairBuf<double> bout;            // [tasks][nparts]
    DevBuf<double> d_bpartials;      // [tasks][nitems][2]
    DevBuf<int32_t> d_blnl;          // [tasks]: the task's lnL sums are in d_bpartials
    int nitems = 0, lds_doubles = 0;
    // iqhip_debug_partition_timing
    std::vector<hipEvent_t> tev;
    double ms[2] = {0.0, 0.0};
    int64_t launches = 0;
    // RELL sums and UFBoot bookkeeping of the group (iqhip_partition_ptnlh_rell, iqhip_partition_ufboot_*): the engine's ufb
    // state, owned by the group; sums: the device table of the members' bt.sums pointers; rell: the summed matrix of
    // iqhip_partition_ptnlh_rell; gen: every member's sample-matrix generation at init.  nsamples == 0: no state
    struct {
        DevBuf<double> dbl, res, rell;
        DevBuf<int64_t> tree;
        DevBuf<int32_t> counts;
        DevBuf<iqhip_ufboot_tree> entries;
        PairBuf<const double *> sums;
        std::vector<uint64_t> gen;
        int nsamples = 0;
        double ms[2] = {0.0, 0.0};   // iqhip_debug_partition_ufboot_timing: the members' products, the update kernels
        int64_t launches = 0;
    } ufb;
    // iqhip_partition_pair_distances: the members' descriptors, the compacted cell lists [chunk][sum_p n_p^2] (member p's at
    // chunk * sum_{q < p} n_q^2) and their lengths [chunk][nparts] of one chunk of pairs, per pair the initial distance and
    // the result {optx, d2l, evaluations, status}
    struct {
        PairBuf<PartPairDesc> desc;
        DevBuf<uint16_t> cells;
        DevBuf<int32_t> nnz;
        DevBuf<double> init, out;
        double ms[2] = {0.0, 0.0};   // iqhip_debug_partition_pair_timing: the members' count launches, the solve launches
    } pdist;
};

namespace {

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

// the group's stream waits for everything enqueued on the members' streams so far
int wait_for_members(iqhip_partition *g) {
    for (int p = 0; p < g->nparts; p++) {
        HIPCHK(hipEventRecord(g->ev[p], g->m[p]->stream));
        HIPCHK(hipStreamWaitEvent(g->stream, g->ev[p], 0));
    }
    return IQHIP_OK;
}
// ... and the members' streams for everything enqueued on the group's
int members_wait(iqhip_partition *g) {
    HIPCHK(hipEventRecord(g->ev_done, g->stream));
    for (int p = 0; p < g->nparts; p++) HIPCHK(hipStreamWaitEvent(g->m[p]->stream, g->ev_done, 0));
    return IQHIP_OK;
}

int use_group(iqhip_partition *g, const char *what) {
    if (!g) return fail(IQHIP_ERR_INVALID, std::string(what) + ": null group");
    const int rc = members_ok(g);
    if (rc) return rc;
    HIPCHK(hipSetDevice(g->device));
    return IQHIP_OK;
}

// every row of a list lies inside every member's store: row r of the group is row r of each member
int group_rows_ok(const iqhip_partition *g, const char *what, const int32_t *rows, int nrows) {
    for (int p = 0; p < g->nparts; p++)
        for (int i = 0; i < nrows; i++)
            if (rows[i] < 0 || rows[i] >= g->m[p]->ptnlh_rows)
                return fail(IQHIP_ERR_INVALID, std::string(what) + ": row outside the store of member " + std::to_string(p) +
                                                   " (iqhip_partition_ptnlh_reserve)");
    return IQHIP_OK;
}

// the MODE 1 pass over the thetas -> out.h[0 .. nparts) after the caller's wait for the stream; st: at its result, only once
// it is done (the pass is enqueued behind a chunk of steps that may not have finished the solve)
int enqueue_part_lnl(iqhip_partition *g, const NewtonState *st, double x) {
    HIPCHK(launch_part_derv(g->stream, 1, d_desc(g), d_items(g), g->nitems, g->lds_doubles, st, x, g->d_partials.p));
    HIPCHK(launch_part_lnl_finish(g->stream, d_desc(g), g->nparts, g->d_partials.p, g->out.d.p));
    HIPCHK(hipMemcpyAsync(g->out.h.p, g->out.d.p, sizeof(double) * (size_t)g->nparts, hipMemcpyDeviceToHost, g->stream));
    g->launches += 2;
    return IQHIP_OK;
}

hipEvent_t timing_event(iqhip_partition *g, size_t k) {
    while (g->tev.size() <= k) {
        hipEvent_t e = nullptr;
        if (hipEventCreate(&e) != hipSuccess) return nullptr;
        g->tev.push_back(e);
    }
    return g->tev[k];
}

// one evaluation of an enqueued chain: the derivative launch, then the update launch; with timing, an event around each
template <typename Derv, typename Update>
int enqueue_step(iqhip_partition *g, bool timing, size_t *nev, Derv &&derv, Update &&update) {
    hipEvent_t e0 = nullptr, e1 = nullptr, e2 = nullptr;
    if (timing) {
        e0 = timing_event(g, *nev);
        e1 = timing_event(g, *nev + 1);
        e2 = timing_event(g, *nev + 2);
        if (!e0 || !e1 || !e2) return fail(IQHIP_ERR_HIP, "partition group: hipEventCreate failed");
        *nev += 3;
        HIPCHK(hipEventRecord(e0, g->stream));
    }
    HIPCHK(derv());
    if (timing) HIPCHK(hipEventRecord(e1, g->stream));
    HIPCHK(update());
    if (timing) HIPCHK(hipEventRecord(e2, g->stream));
    g->launches += 2;
    return IQHIP_OK;
}

// ms[0] / ms[1] += the device time of the derivative / update launches between the first nev events (the stream has drained)
int collect_timing(iqhip_partition *g, size_t nev) {
    for (size_t k = 0; k + 3 <= nev; k += 3) {
        float a = 0.0f, b = 0.0f;
        HIPCHK(hipEventElapsedTime(&a, g->tev[k], g->tev[k + 1]));
        HIPCHK(hipEventElapsedTime(&b, g->tev[k + 1], g->tev[k + 2]));
        g->ms[0] += a;
        g->ms[1] += b;
    }
    return IQHIP_OK;
}

int steps_per_chunk(int enqueued, int max_steps) {
    int chunk_env = 0;
    if (const char *s = getenv("IQHIP_PART_STEPS")) chunk_env = atoi(s);
    return chunk_env > 0 ? chunk_env : (enqueued == 0 ? std::min(4, max_steps + 1) : 2);
}

int solve(iqhip_partition *g, double xguess, double x1, double x2, double xacc, int max_steps, bool want_lnl,
          NewtonState *result) {
    const bool timing = g->m[0]->timing;
    size_t nev = 0;
    if (timing) g->ms[0] = g->ms[1] = 0.0;
    HIPCHK(launch_newton_state_init_on(g->stream, g->state.d.p, xguess, x1, x2, xacc, max_steps));
    g->launches++;
    for (int enq = 0;;) {
        const int chunk = steps_per_chunk(enq, max_steps);
        for (int k = 0; k < chunk; k++) {
            const int rc = enqueue_step(
                g, timing, &nev,
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
    if (timing) {
        const int rc = collect_timing(g, nev);
        if (rc) return rc;
    }
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
    for (hipEvent_t e : g->tev) hipEventDestroy(e);
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
    const bool timing = g->m[0]->timing;
    size_t nev = 0;
    const auto derv = [&](int mode) {
        return launch_part_derv_batch(g->stream, mode, d_desc(g), d_items(g), g->nitems, g->lds_doubles, d_slots, d_sc, P,
                                      g->bstate.d.p, g->d_blnl.p, m, g->d_bpartials.p, mode == 1 ? d_rowp : nullptr);
    };
    for (int enq = 0;;) {
        const int chunk = steps_per_chunk(enq, max_steps);
        for (int k = 0; k < chunk; k++) {
            rc = enqueue_step(g, timing, &nev, [&] { return derv(0); }, [&] {
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
    if (timing) {
        rc = collect_timing(g, nev);
        if (rc) return rc;
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

// ---- per-pattern rows, RELL sums and UFBoot on the group (include/iqhip.h, "UFBoot on edge-linked partition models") --------
// Every member forms its own product R_p = L_p W_p^T on its own stream (launch_alrt_product, its own K-split); the group's
// stream waits for them by events, adds them in member order (kernels_partboot.hip), and the members wait for the group
// before their bt.sums are overwritten again.
namespace {

// nsamples replicates exist in every member's sample matrix
int group_samples_ok(const iqhip_partition *g, const char *what, int nsamples) {
    if (nsamples < 1) return fail(IQHIP_ERR_INVALID, std::string(what) + ": nsamples < 1");
    for (int p = 0; p < g->nparts; p++)
        if (nsamples > g->m[p]->nboot)
            return fail(IQHIP_ERR_INVALID, std::string(what) + ": member " + std::to_string(p) +
                                               (g->m[p]->nboot == 0 ? " has no bootstrap samples (iqhip_gen_boot_samples / iqhip_set_boot_samples)"
                                                                    : " holds fewer samples than nsamples"));
    return IQHIP_OK;
}

// the state exists and every member's sample matrix is still the one it was initialised on
int group_ufboot_ready(const iqhip_partition *g, const char *what) {
    bool ok = g->ufb.nsamples >= 1 && g->ufb.gen.size() == (size_t)g->nparts;
    for (int p = 0; ok && p < g->nparts; p++) ok = g->ufb.gen[p] == g->m[p]->boot_generation && g->ufb.nsamples <= g->m[p]->nboot;
    if (!ok)
        return fail(IQHIP_ERR_INVALID, std::string(what) + " needs iqhip_partition_ufboot_init first (again after a member's sample matrix was replaced)");
    return IQHIP_OK;
}

// every member's product buffers sized for M distinct rows (so that the pointers stay put over the chunks of a call), and the
// table of their bt.sums uploaded on the group's stream
int group_sums_table(iqhip_partition *g, const std::vector<int> &ksplit, size_t M, size_t S) {
    const int P = g->nparts;
    HIPCHK(g->ufb.sums.ensure(g->stream, (size_t)P));
    for (int p = 0; p < P; p++) {
        iqhip_engine *e = g->m[p];
        HIPCHK(e->bt.part.ensure(e, M * S * ksplit[p]));
        HIPCHK(e->bt.sums.ensure(e, M * S));
        g->ufb.sums.h.p[p] = e->bt.sums.p;
    }
    HIPCHK(hipMemcpyAsync(g->ufb.sums.d.p, g->ufb.sums.h.p, sizeof(const double *) * (size_t)P, hipMemcpyHostToDevice, g->stream));
    return IQHIP_OK;
}

// a pair of events around something enqueued on a stream, while timing is enabled; read once everything has drained
struct SpanTimer {
    explicit SpanTimer(bool on_) : on(on_) {}
    SpanTimer(const SpanTimer &) = delete; SpanTimer &operator=(const SpanTimer &) = delete;
    ~SpanTimer() { for (hipEvent_t x : ev) hipEventDestroy(x); }
    void mark(hipStream_t s) {
        hipEvent_t x = nullptr;
        if (!on || !(on = hipEventCreate(&x) == hipSuccess)) return;
        ev.push_back(x);
        on = hipEventRecord(x, s) == hipSuccess;
    }
    double read() {   // the summed time between marks 2k and 2k + 1
        double sum = 0.0;
        if (!on || ev.size() % 2) return 0.0;
        for (size_t k = 0; k < ev.size(); k += 2) {
            float t = 0.0f;
            if (hipEventElapsedTime(&t, ev[k], ev[k + 1]) != hipSuccess) return 0.0;
            sum += t;
        }
        return sum;
    }
    bool on;
    std::vector<hipEvent_t> ev;
};

// one chunk's products: the list staged and multiplied on every member's stream
int group_products(iqhip_partition *g, const RowList &rl, const std::vector<int> &ksplit, int S, SpanTimer &timer) {
    for (int p = 0; p < g->nparts; p++) {
        iqhip_engine *e = g->m[p];
        const int rc = bt_stage(e, rl, ksplit[p], (size_t)S);
        if (rc) return rc;
        timer.mark(e->stream);
        HIPCHK(launch_alrt_product(e, e->bt.rows.p, rl.M, S, ksplit[p], e->bt.part.p, e->bt.sums.p));
        timer.mark(e->stream);
    }
    return IQHIP_OK;
}

}  // namespace

extern "C" int iqhip_partition_ptnlh_reserve(iqhip_partition *g, int nrows) {
    int rc = use_group(g, "iqhip_partition_ptnlh_reserve");
    if (rc) return rc;
    if (nrows < 0 || nrows > (1 << 20)) return fail(IQHIP_ERR_INVALID, "iqhip_partition_ptnlh_reserve: bad row count");
    for (int p = 0; p < g->nparts; p++)
        if ((rc = iqhip_ptnlh_reserve(g->m[p], nrows))) return rc;
    return IQHIP_OK;
}

extern "C" int iqhip_partition_ptnlh_rell(iqhip_partition *g, const int32_t *rows, int nrows, int nsamples, double *out) {
    const char *what = "iqhip_partition_ptnlh_rell";
    int rc = use_group(g, what);
    if (rc) return rc;
    if (!rows || !out || nrows < 1) return fail(IQHIP_ERR_INVALID, std::string(what) + ": bad row list");
    if ((rc = group_samples_ok(g, what, nsamples))) return rc;
    if ((rc = group_rows_ok(g, what, rows, nrows))) return rc;
    const int P = g->nparts;
    const RowList rl = row_list(rows, nrows);
    const size_t count = (size_t)rl.M * nsamples;
    std::vector<int> ksplit((size_t)P);
    for (int p = 0; p < P; p++) ksplit[p] = alrt_ksplit(g->m[p], rl.M, nsamples);
    HIPCHK(g->ufb.rell.ensure(g->stream, count));
    rc = group_sums_table(g, ksplit, (size_t)rl.M, (size_t)nsamples);
    if (rc) return rc;
    SpanTimer timer(false);
    rc = group_products(g, rl, ksplit, nsamples, timer);
    std::vector<double> sums(count);
    if (!rc) rc = wait_for_members(g);
    hipError_t s = hipSuccess;
    if (!rc) s = launch_part_rell_sum(g->stream, g->ufb.sums.d.p, P, count, g->ufb.rell.p);
    if (!rc && s == hipSuccess)
        s = hipMemcpyAsync(sums.data(), g->ufb.rell.p, sizeof(double) * count, hipMemcpyDeviceToHost, g->stream);
    const int rc2 = members_wait(g);
    const hipError_t drained = hipStreamSynchronize(g->stream);
    if (rc) return rc;
    HIPCHK(s);
    if (rc2) return rc2;
    HIPCHK(drained);
    const int32_t *idx = rl.list.data() + rl.M;
    for (int i = 0; i < nrows; i++)
        memcpy(out + (size_t)i * nsamples, sums.data() + (size_t)idx[i] * nsamples, sizeof(double) * (size_t)nsamples);
    return IQHIP_OK;
}

extern "C" int iqhip_partition_ufboot_init(iqhip_partition *g, int nsamples) {
    const char *what = "iqhip_partition_ufboot_init";
    int rc = use_group(g, what);
    if (rc) return rc;
    if ((rc = group_samples_ok(g, what, nsamples))) return rc;
    const size_t S = (size_t)nsamples;
    g->ufb.nsamples = 0;
    HIPCHK(g->ufb.dbl.ensure(g->stream, 2 * S));
    HIPCHK(g->ufb.tree.ensure(g->stream, S));
    HIPCHK(g->ufb.counts.ensure(g->stream, S));
    HIPCHK(g->ufb.res.ensure(g->stream, 1 + (size_t)ufboot_workgroups(nsamples)));
    // iqtree.cpp:308-312, the starting values of iqhip_ufboot_init
    std::vector<double> lo(2 * S, -DBL_MAX);
    std::vector<int64_t> none(S, -1);
    HIPCHK(hipStreamSynchronize(g->stream));   // (pageable sources)
    HIPCHK(hipMemcpyAsync(g->ufb.dbl.p, lo.data(), sizeof(double) * lo.size(), hipMemcpyHostToDevice, g->stream));
    HIPCHK(hipMemcpyAsync(g->ufb.tree.p, none.data(), sizeof(int64_t) * S, hipMemcpyHostToDevice, g->stream));
    HIPCHK(hipMemsetAsync(g->ufb.counts.p, 0, sizeof(int32_t) * S, g->stream));
    HIPCHK(hipStreamSynchronize(g->stream));
    g->ufb.gen.resize((size_t)g->nparts);
    for (int p = 0; p < g->nparts; p++) g->ufb.gen[p] = g->m[p]->boot_generation;
    g->ufb.nsamples = nsamples;
    g->ufb.ms[0] = g->ufb.ms[1] = 0.0;
    g->ufb.launches = 0;
    return IQHIP_OK;
}

extern "C" int iqhip_partition_ufboot_update(iqhip_partition *g, const iqhip_ufboot_tree *trees, int ntrees, double epsilon,
                                             double logl_cutoff, int64_t *counts, double *min_orig_logl) {
    const char *what = "iqhip_partition_ufboot_update";
    int rc = use_group(g, what);
    if (rc) return rc;
    if (!trees || ntrees < 1) return fail(IQHIP_ERR_INVALID, std::string(what) + ": bad tree list");
    if (!(epsilon >= 0.0)) return fail(IQHIP_ERR_INVALID, std::string(what) + ": epsilon must be >= 0");
    if ((rc = group_ufboot_ready(g, what))) return rc;
    for (int i = 0; i < ntrees; i++) {
        const iqhip_ufboot_tree &t = trees[i];
        if ((rc = group_rows_ok(g, what, &t.row, 1))) return rc;
        if (t.tree_id < 0) return fail(IQHIP_ERR_INVALID, std::string(what) + ": tree_id must be >= 0");
        if (!(t.rand >= 0.0 && t.rand <= 1.0)) return fail(IQHIP_ERR_INVALID, std::string(what) + ": rand outside [0, 1]");
        if (!std::isfinite(t.logl)) return fail(IQHIP_ERR_INVALID, std::string(what) + ": log-likelihoods must be finite");
    }
    // iqtree.cpp:2678
    std::vector<iqhip_ufboot_tree> ent;
    ent.reserve((size_t)ntrees);
    for (int i = 0; i < ntrees; i++)
        if (!(logl_cutoff != 0.0 && trees[i].logl < logl_cutoff - 1.0)) ent.push_back(trees[i]);
    const int n = (int)ent.size(), S = g->ufb.nsamples, P = g->nparts;
    // entries per chunk: all members' part [ksplit][M][S] and sums [M][S] of M <= chunk distinct rows together within 256 MB.
    // A member's K-split follows from nsamples, its pattern count and the CU count alone, so a (row, replicate) sum has the
    // same bits whatever the chunk
    std::vector<int> ksplit((size_t)P);
    int64_t per_entry = 0;
    for (int p = 0; p < P; p++) {
        ksplit[p] = alrt_ksplit(g->m[p], 1, S);
        per_entry += (int64_t)sizeof(double) * S * (ksplit[p] + 1);
    }
    int64_t chunk = std::max<int64_t>(1, ((int64_t)256 << 20) / per_entry);
    if (const char *uc = getenv("IQHIP_UFBOOT_CHUNK")) chunk = std::max(1, atoi(uc));
    chunk = std::min<int64_t>(chunk, std::max(n, 1));
    // every chunk's row list, and the entries with `row` rewritten to the row of their chunk's sums
    std::vector<RowList> lists;
    std::vector<int32_t> rows((size_t)chunk);
    size_t maxM = 1;
    for (int first = 0; first < n; first += (int)chunk) {
        const int m = (int)std::min<int64_t>(chunk, n - first);
        for (int i = 0; i < m; i++) rows[i] = ent[first + i].row;
        lists.push_back(row_list(rows.data(), m));
        const int32_t *idx = lists.back().list.data() + lists.back().M;
        for (int i = 0; i < m; i++) ent[first + i].row = idx[i];
        maxM = std::max(maxM, (size_t)lists.back().M);
    }
    const size_t nwg = (size_t)ufboot_workgroups(S);
    HIPCHK(g->ufb.entries.ensure(g->stream, (size_t)std::max(n, 1)));
    HIPCHK(g->ufb.res.ensure(g->stream, 1 + nwg));
    HIPCHK(hipStreamSynchronize(g->stream));   // (pageable source, and an earlier launch may still read the entries)
    if (n > 0)
        HIPCHK(hipMemcpyAsync(g->ufb.entries.p, ent.data(), sizeof(iqhip_ufboot_tree) * (size_t)n, hipMemcpyHostToDevice, g->stream));
    HIPCHK(hipMemsetAsync(g->ufb.res.p, 0, sizeof(double), g->stream));
    rc = group_sums_table(g, ksplit, maxM, (size_t)S);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(g->stream));
    unsigned long long *d_replaced = reinterpret_cast<unsigned long long *>(g->ufb.res.p);
    double *boot_logl = g->ufb.dbl.p, *boot_orig = g->ufb.dbl.p + S;
    const bool timing = g->m[0]->timing;
    SpanTimer t_prod(timing), t_upd(timing);
    int64_t launches = 0;
    hipError_t s = hipSuccess;
    if (n == 0) {   // everything fell to the cutoff: the state is only read for its minimum
        s = launch_part_ufboot_update(g->stream, g->ufb.sums.d.p, P, S, g->ufb.entries.p, 0, epsilon, boot_logl, boot_orig,
                                      g->ufb.counts.p, g->ufb.tree.p, d_replaced, g->ufb.res.p + 1);
        launches = 1;
    }
    for (size_t c = 0, first = 0; c < lists.size() && s == hipSuccess && rc == IQHIP_OK; c++) {
        const RowList &rl = lists[c];
        const int m = (int)(rl.list.size() - (size_t)rl.M);
        // (a member's stream waits for the update of the chunk before: its sums are not overwritten under it)
        if ((rc = group_products(g, rl, ksplit, S, t_prod))) break;
        if ((rc = wait_for_members(g))) break;
        t_upd.mark(g->stream);
        s = launch_part_ufboot_update(g->stream, g->ufb.sums.d.p, P, S, g->ufb.entries.p + first, m, epsilon, boot_logl, boot_orig,
                                      g->ufb.counts.p, g->ufb.tree.p, d_replaced, g->ufb.res.p + 1);
        t_upd.mark(g->stream);
        const int rc2 = members_wait(g);
        if (!rc) rc = rc2;
        launches += 2 * P + 1;
        first += (size_t)m;
    }
    std::vector<double> res(1 + nwg);
    if (s == hipSuccess && rc == IQHIP_OK)
        s = hipMemcpyAsync(res.data(), g->ufb.res.p, sizeof(double) * res.size(), hipMemcpyDeviceToHost, g->stream);
    const hipError_t drained = hipStreamSynchronize(g->stream);
    if (s == hipSuccess) s = drained;
    if (rc) return rc;
    HIPCHK(s);
    g->ufb.ms[0] = t_prod.read();
    g->ufb.ms[1] = t_upd.read();
    g->ufb.launches = launches;
    if (counts) {
        unsigned long long replaced;
        memcpy(&replaced, &res[0], sizeof(replaced));
        counts[0] = n;
        counts[1] = ntrees - n;
        counts[2] = (int64_t)replaced;
    }
    if (min_orig_logl) {   // the workgroups' minima in workgroup order
        double mn = DBL_MAX;
        for (size_t w = 0; w < nwg; w++)
            if (res[1 + w] < mn) mn = res[1 + w];
        *min_orig_logl = mn;
    }
    return IQHIP_OK;
}

extern "C" int iqhip_partition_ufboot_fetch(iqhip_partition *g, double *boot_logl, double *boot_orig_logl, int32_t *boot_counts,
                                            int64_t *boot_tree) {
    const char *what = "iqhip_partition_ufboot_fetch";
    int rc = use_group(g, what);
    if (rc) return rc;
    if ((rc = group_ufboot_ready(g, what))) return rc;
    const size_t S = (size_t)g->ufb.nsamples;
    if (boot_logl) HIPCHK(hipMemcpyAsync(boot_logl, g->ufb.dbl.p, sizeof(double) * S, hipMemcpyDeviceToHost, g->stream));
    if (boot_orig_logl) HIPCHK(hipMemcpyAsync(boot_orig_logl, g->ufb.dbl.p + S, sizeof(double) * S, hipMemcpyDeviceToHost, g->stream));
    if (boot_counts) HIPCHK(hipMemcpyAsync(boot_counts, g->ufb.counts.p, sizeof(int32_t) * S, hipMemcpyDeviceToHost, g->stream));
    if (boot_tree) HIPCHK(hipMemcpyAsync(boot_tree, g->ufb.tree.p, sizeof(int64_t) * S, hipMemcpyDeviceToHost, g->stream));
    HIPCHK(hipStreamSynchronize(g->stream));
    return IQHIP_OK;
}

extern "C" int iqhip_debug_partition_ufboot_timing(iqhip_partition *g, double *ms, int64_t *launches) {
    if (!g) return fail(IQHIP_ERR_INVALID, "iqhip_debug_partition_ufboot_timing: null group");
    if (!ms) return fail(IQHIP_ERR_INVALID, "iqhip_debug_partition_ufboot_timing: null argument");
    ms[0] = g->ufb.ms[0];
    ms[1] = g->ufb.ms[1];
    if (launches) *launches = g->ufb.launches;
    return IQHIP_OK;
}

// ---- joint pairwise distances (include/iqhip.h, "Joint pairwise distances of a partition group") ------------------------------
// Per chunk of pairs: every member's launch_pair_counts on its own stream into its own pd.counts, then ONE k_partpair_solve
// on the group's stream behind the members' events, then the members wait for the group (the next chunk's counts overwrite
// what the solve read).  P + 1 launches per chunk, P more per call for the members' coefficient tables; no host round trip.
extern "C" int iqhip_partition_pair_distances(iqhip_partition *g, const double *init, double x1, double x2, double xacc,
                                              int max_steps, double *dist, double *d2l, int32_t *nsteps) {
    const char *what = "iqhip_partition_pair_distances";
    if (!g) return fail(IQHIP_ERR_INVALID, std::string(what) + ": null group");
    if (!dist) return fail(IQHIP_ERR_INVALID, std::string(what) + ": null argument");
    if (!(x1 >= 0.0) || x1 > x2 || !std::isfinite(x2) || !(xacc > 0.0) || max_steps < 1)
        return fail(IQHIP_ERR_INVALID, std::string(what) + ": bad bounds / tolerance / step count (x1 <= x2, max_steps >= 1)");
    int rc = use_group(g, what);
    if (rc) return rc;
    const int P = g->nparts, T = g->m[0]->ntaxa;
    std::vector<int> nstates;
    int e_doubles = 0, max_n = 0;
    for (int p = 0; p < P; p++) {
        iqhip_engine *e = g->m[p];
        if ((rc = pair_require(e, what))) return rc;
        if (e->ntaxa != T)
            return fail(IQHIP_ERR_INVALID, std::string(what) + ": member " + std::to_string(p) + " has another number of taxa than member 0");
        nstates.push_back(e->n);
        e_doubles = std::max(e_doubles, e->n * e->ncat);
        max_n = std::max(max_n, e->n);
    }
    if (partpair_solve_lds_bytes(e_doubles, max_n) > kPartMaxLdsBytes)
        return fail(IQHIP_ERR_UNSUPPORTED, std::string(what) + ": nstates * ncat of a member exceeds the solve's LDS");
    const int64_t npairs = (int64_t)T * (T - 1) / 2;
    std::vector<int32_t> pairs;
    pair_list(T, pairs);
    std::vector<double> h_init;
    if (init) {
        h_init.resize((size_t)npairs);
        for (int64_t k = 0; k < npairs; k++) {
            const double v = init[(size_t)pairs[2 * k] * T + pairs[2 * k + 1]];
            if (!(v >= 0.0) || !std::isfinite(v)) return fail(IQHIP_ERR_INVALID, std::string(what) + ": an initial distance is negative or not finite");
            h_init[(size_t)k] = v;
        }
    }
    for (size_t k = 0; k < (size_t)T * T; k++) {
        dist[k] = 0.0;
        if (d2l) d2l[k] = 0.0;
        if (nsteps) nsteps[k] = 0;
    }
    g->pdist.ms[0] = g->pdist.ms[1] = 0.0;
    g->launches = 0;
    if (npairs == 0) return IQHIP_OK;
    // pairs per chunk: all members' counts of a chunk together within 64 MB; IQHIP_PAIR_CHUNK (read per call) overrides
    const char *pc = getenv("IQHIP_PAIR_CHUNK");
    const PartPairLayout lay = partpair_layout(nstates.data(), P, npairs, pc ? std::max(1, atoi(pc)) : 0);
    const int64_t chunk = lay.chunk;
    const size_t sum_nn = lay.sum_nn;
    // all tiles up front, chunk by chunk (a chunk's slots start at 0): the same list serves every member
    std::vector<PairTile> tiles;
    std::vector<size_t> tile_first;
    for (int64_t first = 0; first < npairs; first += chunk) {
        tile_first.push_back(tiles.size());
        pair_tiles(pairs.data() + 2 * first, std::min<int64_t>(chunk, npairs - first), T, tiles);
    }
    tile_first.push_back(tiles.size());
    HIPCHK(g->pdist.desc.ensure(g->stream, (size_t)P));
    HIPCHK(g->pdist.cells.ensure(g->stream, (size_t)chunk * sum_nn));
    HIPCHK(g->pdist.nnz.ensure(g->stream, (size_t)chunk * P));
    HIPCHK(g->pdist.init.ensure(g->stream, (size_t)npairs));
    HIPCHK(g->pdist.out.ensure(g->stream, (size_t)4 * npairs));
    // every buffer first: up to here nothing is enqueued, and a failure returns at once
    for (int p = 0; p < P; p++) {
        iqhip_engine *e = g->m[p];
        const size_t nn = (size_t)e->n * e->n;
        HIPCHK(e->pd.tiles.ensure(e, tiles.size()));
        HIPCHK(e->pd.counts.ensure(e, (size_t)chunk * nn));
        HIPCHK(e->pd.coef.ensure(e, nn * e->n));
        HIPCHK(hipStreamSynchronize(e->stream));
    }
    // From the first copy on `tiles` and `h_init` (pageable) are sources of enqueued copies: whatever fails below, the call
    // leaves through the drain at its end, never straight out
    const auto enqueue_setup = [&]() -> int {
        for (int p = 0; p < P; p++) {
            iqhip_engine *e = g->m[p];
            HIPCHK(hipMemcpyAsync(e->pd.tiles.p, tiles.data(), sizeof(PairTile) * tiles.size(), hipMemcpyHostToDevice, e->stream));
            HIPCHK(launch_pair_coef(e, e->pd.coef.p));
            PartPairDesc &D = g->pdist.desc.h.p[p];
            D.counts = e->pd.counts.p;
            D.coef = e->pd.coef.p;
            D.eval = e->d_eval;
            D.rates = e->d_rates;
            D.props = e->d_props;
            D.cells = g->pdist.cells.p + lay.cell_first[(size_t)p];
            D.n = e->n;
            D.ncat = e->ncat;
            D.rate = g->rate[p];
        }
        g->launches += P;
        HIPCHK(hipSetDevice(g->device));
        HIPCHK(hipMemcpyAsync(g->pdist.desc.d.p, g->pdist.desc.h.p, sizeof(PartPairDesc) * (size_t)P, hipMemcpyHostToDevice, g->stream));
        if (init) HIPCHK(hipMemcpyAsync(g->pdist.init.p, h_init.data(), sizeof(double) * h_init.size(), hipMemcpyHostToDevice, g->stream));
        return IQHIP_OK;
    };
    rc = enqueue_setup();
    PartPairArgs a;
    a.desc = g->pdist.desc.d.p;
    a.nnz = g->pdist.nnz.p;
    a.init = init ? g->pdist.init.p : nullptr;
    a.out = g->pdist.out.p;
    a.nparts = P;
    a.max_steps = max_steps;
    a.e_doubles = e_doubles;
    a.max_n = max_n;
    a.x1 = x1;
    a.x2 = x2;
    a.xacc = xacc;
    const bool timing = g->m[0]->timing;
    SpanTimer t_counts(timing), t_solve(timing);
    hipError_t s = hipSuccess;
    int64_t first = 0;
    for (size_t c = 0; first < npairs && s == hipSuccess && rc == IQHIP_OK; c++, first += chunk) {
        const int m = (int)std::min<int64_t>(chunk, npairs - first);
        a.first_pair = first;
        // (a member's stream waits for the solve of the chunk before: its counts are not overwritten under it)
        for (int p = 0; p < P && s == hipSuccess; p++) {
            iqhip_engine *e = g->m[p];
            t_counts.mark(e->stream);
            s = launch_pair_counts(e, e->pd.tiles.p + tile_first[c], (int)(tile_first[c + 1] - tile_first[c]), e->pd.counts.p);
            t_counts.mark(e->stream);
        }
        if (s != hipSuccess || (rc = wait_for_members(g))) break;
        t_solve.mark(g->stream);
        s = launch_partpair_solve(g->stream, a, m);
        t_solve.mark(g->stream);
        const int rc2 = members_wait(g);
        if (!rc) rc = rc2;
        g->launches += P + 1;
    }
    std::vector<double> out((size_t)4 * npairs);
    if (s == hipSuccess && rc == IQHIP_OK)
        s = hipMemcpyAsync(out.data(), g->pdist.out.p, sizeof(double) * out.size(), hipMemcpyDeviceToHost, g->stream);
    // (whatever happened: the host waits for everything enqueued, the members' streams included; the staging is free again)
    hipError_t drained = hipStreamSynchronize(g->stream);
    for (int p = 0; p < P; p++) {
        const hipError_t d = hipStreamSynchronize(g->m[p]->stream);
        if (drained == hipSuccess) drained = d;
    }
    if (rc) return rc;
    HIPCHK(s);
    HIPCHK(drained);
    g->pdist.ms[0] = t_counts.read();
    g->pdist.ms[1] = t_solve.read();
    int worst = 0;
    for (int64_t k = 0; k < npairs; k++) {
        const size_t ij = (size_t)pairs[2 * k] * T + pairs[2 * k + 1], ji = (size_t)pairs[2 * k + 1] * T + pairs[2 * k];
        const NewtonResult r(out.data() + 4 * k);
        dist[ij] = dist[ji] = r.optx;
        if (d2l) d2l[ij] = d2l[ji] = r.d2l;
        if (nsteps) nsteps[ij] = nsteps[ji] = r.nsteps;
        if (r.status && !worst) worst = r.status;
    }
    return newton_status(worst);   // (minimizeNewton's two nrerror() exits; the matrices are filled all the same)
}

extern "C" int iqhip_debug_partition_pair_timing(iqhip_partition *g, double *counts_ms, double *solve_ms) {
    if (!g) return fail(IQHIP_ERR_INVALID, "iqhip_debug_partition_pair_timing: null group");
    if (counts_ms) *counts_ms = g->pdist.ms[0];
    if (solve_ms) *solve_ms = g->pdist.ms[1];
    return IQHIP_OK;
}
