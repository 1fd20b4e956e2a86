// ufboot.hip -- drivers of the ultrafast bootstrap: saveCurrentTree's per-replicate bookkeeping (iqtree.cpp:2676-2786) on one
// engine (iqhip_ufboot_*; include/iqhip.h "UFBoot") and on a partition group (iqhip_partition_ufboot_*, with the group's
// per-pattern rows and RELL sums; "UFBoot on edge-linked partition models").  Host code only; the kernels are in
// kernels_ufboot.hip and kernels_partboot.hip.
//
// One state (UfbootState) and one driver (ufb_update) serve both owners; what differs is a chunk's step --
//   engine: the list staged, the product R = L W^T, the update on its sums: 3 launches on the engine's stream;
//   group:  every member forms its own product R_p = L_p W_p^T on its own stream (launch_alrt_product, its own K-split); the
//           group's stream waits for them by events, the update adds them in member order (kernels_partboot.hip), and the
//           members wait for the group before their bt.sums are overwritten again: 2 P + 1 launches.
#include <float.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <functional>
#include <vector>

#include "partition.h"

using namespace iqhip;

namespace {

// ---- what both owners share ------------------------------------------------------------------------------------------------
// a state of nsamples replicates that hold no tree yet (iqtree.cpp:308-312); the stream drains
int ufb_init(UfbootState &u, hipStream_t stream, int nsamples) {
    const size_t S = (size_t)nsamples;
    u.nsamples = 0;
    HIPCHK(u.dbl.ensure(stream, 2 * S));
    HIPCHK(u.tree.ensure(stream, S));
    HIPCHK(u.counts.ensure(stream, S));
    HIPCHK(u.res.ensure(stream, 1 + (size_t)ufboot_workgroups(nsamples)));
    std::vector<double> lo(2 * S, -DBL_MAX);
    std::vector<int64_t> none(S, -1);
    HIPCHK(hipStreamSynchronize(stream));   // (pageable sources)
    HIPCHK(hipMemcpyAsync(u.dbl.p, lo.data(), sizeof(double) * lo.size(), hipMemcpyHostToDevice, stream));
    HIPCHK(hipMemcpyAsync(u.tree.p, none.data(), sizeof(int64_t) * S, hipMemcpyHostToDevice, stream));
    HIPCHK(hipMemsetAsync(u.counts.p, 0, sizeof(int32_t) * S, stream));
    HIPCHK(hipStreamSynchronize(stream));
    u.nsamples = nsamples;
    u.ms[0] = u.ms[1] = 0.0;
    u.launches = 0;
    return IQHIP_OK;
}

// What an update asks of its owner, an engine or a group: ready / row_ok -- the state is current, a row lies in the store;
// bytes_per_entry -- part [ksplit][M][S] and sums [M][S] per distinct row of a chunk, of all members together (asked once
// the state is ready); prepare -- before the first chunk, with the largest M of the call; update -- the kernel on entries
// [first, first + m); step -- one chunk of `launches` kernels: the products of its row list, then update
struct UfbOwner {
    UfbootState &u;
    hipStream_t stream;
    int launches;
    std::function<int()> ready;
    std::function<int(const int32_t *row)> row_ok;
    std::function<int64_t()> bytes_per_entry;
    std::function<int(size_t maxM)> prepare;
    std::function<hipError_t(size_t first, int m)> update;
    std::function<int(const RowList &rl, size_t first, int m)> step;
};

int ufb_update(const char *what, const UfbOwner &o, const iqhip_ufboot_tree *trees, int ntrees, double epsilon, double logl_cutoff,
               int64_t *counts, double *min_orig_logl) {
    static_assert(sizeof(iqhip_ufboot_tree) == 32, "iqhip_ufboot_tree is 32 bytes");
    UfbootState &u = o.u;
    if (!trees || ntrees < 1) return fail(IQHIP_ERR_INVALID, std::string(what) + ": bad tree list");
    if (!(epsilon >= 0.0)) return fail(IQHIP_ERR_INVALID, std::string(what) + ": epsilon must be >= 0");
    int rc = o.ready();
    if (rc) return rc;
    for (int i = 0; i < ntrees; i++) {
        const iqhip_ufboot_tree &t = trees[i];
        if ((rc = o.row_ok(&t.row))) return rc;
        if (t.tree_id < 0) return fail(IQHIP_ERR_INVALID, std::string(what) + ": tree_id must be >= 0");
        if (!(t.rand >= 0.0 && t.rand <= 1.0)) return fail(IQHIP_ERR_INVALID, std::string(what) + ": rand outside [0, 1]");
        if (!std::isfinite(t.logl)) return fail(IQHIP_ERR_INVALID, std::string(what) + ": log-likelihoods must be finite");
    }
    // iqtree.cpp:2678
    std::vector<iqhip_ufboot_tree> ent;
    ent.reserve((size_t)ntrees);
    for (int i = 0; i < ntrees; i++)
        if (!(logl_cutoff != 0.0 && trees[i].logl < logl_cutoff - 1.0)) ent.push_back(trees[i]);
    const int n = (int)ent.size();
    // entries per chunk: the owner's bytes of M <= chunk distinct rows stay within 256 MB; the environment switch, read per
    // call, overrides.  A K-split follows from nsamples, the pattern count and the CU count alone, so a (row, replicate) sum
    // has the same bits whatever the chunk
    int64_t chunk = std::max<int64_t>(1, ((int64_t)256 << 20) / o.bytes_per_entry());
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
    const size_t nwg = (size_t)ufboot_workgroups(u.nsamples);
    HIPCHK(u.entries.ensure(o.stream, (size_t)std::max(n, 1)));
    HIPCHK(u.res.ensure(o.stream, 1 + nwg));
    HIPCHK(hipStreamSynchronize(o.stream));   // (pageable source, and an earlier launch may still read the entries)
    if (n > 0) HIPCHK(hipMemcpyAsync(u.entries.p, ent.data(), sizeof(iqhip_ufboot_tree) * (size_t)n, hipMemcpyHostToDevice, o.stream));
    HIPCHK(hipMemsetAsync(u.res.p, 0, sizeof(double), o.stream));   // (the replaced slots)
    if (o.prepare && (rc = o.prepare(maxM))) return rc;
    HIPCHK(hipStreamSynchronize(o.stream));
    // from here on the call leaves through the wait for the stream, whatever fails
    hipError_t s = hipSuccess;
    if (n == 0) s = o.update(0, 0);   // everything fell to the cutoff: the state is only read for its minimum
    size_t first = 0;
    for (size_t c = 0; c < lists.size() && rc == IQHIP_OK; c++) {
        const int m = (int)(lists[c].list.size() - (size_t)lists[c].M);
        rc = o.step(lists[c], first, m);
        first += (size_t)m;
    }
    std::vector<double> res(1 + nwg);
    if (s == hipSuccess && rc == IQHIP_OK) s = hipMemcpyAsync(res.data(), u.res.p, sizeof(double) * res.size(), hipMemcpyDeviceToHost, o.stream);
    const hipError_t drained = hipStreamSynchronize(o.stream);
    if (rc) return rc;
    HIPCHK(s);
    HIPCHK(drained);
    u.launches = n == 0 ? 1 : (int64_t)o.launches * (int64_t)lists.size();
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

int ufb_fetch(const UfbootState &u, hipStream_t stream, double *boot_logl, double *boot_orig_logl, int32_t *boot_counts,
              int64_t *boot_tree) {
    const size_t S = (size_t)u.nsamples;
    if (boot_logl) HIPCHK(hipMemcpyAsync(boot_logl, u.dbl.p, sizeof(double) * S, hipMemcpyDeviceToHost, stream));
    if (boot_orig_logl) HIPCHK(hipMemcpyAsync(boot_orig_logl, u.dbl.p + S, sizeof(double) * S, hipMemcpyDeviceToHost, stream));
    if (boot_counts) HIPCHK(hipMemcpyAsync(boot_counts, u.counts.p, sizeof(int32_t) * S, hipMemcpyDeviceToHost, stream));
    if (boot_tree) HIPCHK(hipMemcpyAsync(boot_tree, u.tree.p, sizeof(int64_t) * S, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    return IQHIP_OK;
}

int ufb_timing(const char *what, const UfbootState &u, double *ms, int64_t *launches) {
    if (!ms) return fail(IQHIP_ERR_INVALID, std::string(what) + ": null argument");
    ms[0] = u.ms[0];
    ms[1] = u.ms[1];
    if (launches) *launches = u.launches;
    return IQHIP_OK;
}

unsigned long long *ufb_replaced(const UfbootState &u) { return reinterpret_cast<unsigned long long *>(u.res.p); }

// ---- the engine ------------------------------------------------------------------------------------------------------------
// the state exists and still belongs to the sample matrix
int ufboot_ready(iqhip_engine *e, const char *what) {
    if (e->ufb.nsamples < 1 || e->ufb.nsamples > e->nboot)
        return fail(IQHIP_ERR_INVALID, std::string(what) + " needs iqhip_ufboot_init first (again after the sample matrix was replaced)");
    return IQHIP_OK;
}

}  // namespace

extern "C" int iqhip_ufboot_init(iqhip_engine *e, int nsamples) {
    int rc = require(e, "iqhip_ufboot_init", REQ_SINGLE_DEVICE);
    if (rc) return rc;
    if (nsamples < 1 || nsamples > e->nboot)
        return fail(IQHIP_ERR_INVALID, e->nboot == 0 ? "iqhip_ufboot_init: no bootstrap samples (iqhip_gen_boot_samples / iqhip_set_boot_samples)"
                                                     : "iqhip_ufboot_init: nsamples must be 1 .. the number of uploaded samples");
    HIPCHK(use_device(e));
    return ufb_init(e->ufb, e->stream, nsamples);
}

extern "C" int iqhip_ufboot_update(iqhip_engine *e, const iqhip_ufboot_tree *trees, int ntrees, double epsilon, double logl_cutoff,
                                   int64_t *counts, double *min_orig_logl) {
    const char *what = "iqhip_ufboot_update";
    int rc = require(e, what, REQ_SINGLE_DEVICE);
    if (rc) return rc;
    HIPCHK(use_device(e));
    UfbootState &u = e->ufb;
    const int &S = u.nsamples;
    int ksplit = 0;
    PhaseTimer timer(e, 2);   // per chunk: before the product, between, behind the update
    UfbOwner o{u, e->stream, 3};
    o.ready = [&] { return ufboot_ready(e, what); };
    o.row_ok = [&](const int32_t *row) {
        return *row < 0 || *row >= e->ptnlh_rows ? fail(IQHIP_ERR_INVALID, std::string(what) + ": row outside the store") : IQHIP_OK;
    };
    o.bytes_per_entry = [&] {
        ksplit = alrt_ksplit(e, 1, S);
        return (int64_t)sizeof(double) * S * (ksplit + 1);
    };
    o.update = [&](size_t first, int m) {
        return launch_ufboot_update(e, m ? e->bt.sums.p : nullptr, S, u.entries.p + first, m, epsilon, u.dbl.p, u.dbl.p + S,
                                    u.counts.p, u.tree.p, ufb_replaced(u), u.res.p + 1);
    };
    o.step = [&](const RowList &rl, size_t first, int m) -> int {
        const int staged = bt_stage(e, rl, ksplit, (size_t)S);
        if (staged) return staged;
        timer.mark();
        HIPCHK(launch_alrt_product(e, e->bt.rows.p, rl.M, S, ksplit, e->bt.part.p, e->bt.sums.p));
        timer.mark();
        HIPCHK(o.update(first, m));
        timer.mark();
        return IQHIP_OK;
    };
    if ((rc = ufb_update(what, o, trees, ntrees, epsilon, logl_cutoff, counts, min_orig_logl))) return rc;
    u.ms[0] = u.ms[1] = 0.0;
    timer.read(u.ms);
    return IQHIP_OK;
}

extern "C" int iqhip_ufboot_fetch(iqhip_engine *e, double *boot_logl, double *boot_orig_logl, int32_t *boot_counts,
                                  int64_t *boot_tree) {
    int rc = require(e, "iqhip_ufboot_fetch", REQ_SINGLE_DEVICE);
    if (rc) return rc;
    if ((rc = ufboot_ready(e, "iqhip_ufboot_fetch"))) return rc;
    HIPCHK(use_device(e));
    return ufb_fetch(e->ufb, e->stream, boot_logl, boot_orig_logl, boot_counts, boot_tree);
}

extern "C" int iqhip_debug_ufboot_timing(iqhip_engine *e, double *ms, int64_t *launches) {
    const int rc = require(e, "iqhip_debug_ufboot_timing", REQ_SINGLE_DEVICE);
    return rc ? rc : ufb_timing("iqhip_debug_ufboot_timing", e->ufb, ms, launches);
}

// ---- the group: per-pattern rows, RELL sums, UFBoot ------------------------------------------------------------------------
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
    bool ok = g->ufb.nsamples >= 1 && g->ufb_gen.size() == (size_t)g->nparts;
    for (int p = 0; ok && p < g->nparts; p++) ok = g->ufb_gen[p] == g->m[p]->boot_generation && g->ufb.nsamples <= g->m[p]->nboot;
    if (!ok)
        return fail(IQHIP_ERR_INVALID, std::string(what) + " needs iqhip_partition_ufboot_init first (again after a member's sample matrix was replaced)");
    return IQHIP_OK;
}

// every member's product buffers sized for M distinct rows (so that the pointers stay put over the chunks of a call), and the
// table of their bt.sums uploaded on the group's stream
int group_sums_table(iqhip_partition *g, const std::vector<int> &ksplit, size_t M, size_t S) {
    const int P = g->nparts;
    HIPCHK(g->ufb_sums.ensure(g->stream, (size_t)P));
    for (int p = 0; p < P; p++) {
        iqhip_engine *e = g->m[p];
        HIPCHK(e->bt.part.ensure(e, M * S * ksplit[p]));
        HIPCHK(e->bt.sums.ensure(e, M * S));
        g->ufb_sums.h.p[p] = e->bt.sums.p;
    }
    HIPCHK(hipMemcpyAsync(g->ufb_sums.d.p, g->ufb_sums.h.p, sizeof(const double *) * (size_t)P, hipMemcpyHostToDevice, g->stream));
    return IQHIP_OK;
}

// one chunk's products: the list staged and multiplied on every member's stream, a round of the timer around each product
int group_products(iqhip_partition *g, const RowList &rl, const std::vector<int> &ksplit, int S, PhaseTimer &timer) {
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
    HIPCHK(g->ufb_rell.ensure(g->stream, count));
    rc = group_sums_table(g, ksplit, (size_t)rl.M, (size_t)nsamples);
    if (rc) return rc;
    PhaseTimer untimed(false, g->stream, 1);
    rc = group_products(g, rl, ksplit, nsamples, untimed);
    std::vector<double> sums(count);
    if (!rc) rc = wait_for_members(g);
    hipError_t s = hipSuccess;
    if (!rc) s = launch_part_rell_sum(g->stream, g->ufb_sums.d.p, P, count, g->ufb_rell.p);
    if (!rc && s == hipSuccess)
        s = hipMemcpyAsync(sums.data(), g->ufb_rell.p, sizeof(double) * count, hipMemcpyDeviceToHost, g->stream);
    const int rc2 = members_wait(g);
    const hipError_t drained = hipStreamSynchronize(g->stream);
    if (rc) return rc;
    HIPCHK(s);
    if (rc2) return rc2;
    HIPCHK(drained);
    row_list_scatter(rl, sums.data(), nsamples, out);
    return IQHIP_OK;
}

extern "C" int iqhip_partition_ufboot_init(iqhip_partition *g, int nsamples) {
    const char *what = "iqhip_partition_ufboot_init";
    int rc = use_group(g, what);
    if (rc) return rc;
    if ((rc = group_samples_ok(g, what, nsamples))) return rc;
    if ((rc = ufb_init(g->ufb, g->stream, nsamples))) return rc;
    g->ufb_gen.resize((size_t)g->nparts);
    for (int p = 0; p < g->nparts; p++) g->ufb_gen[p] = g->m[p]->boot_generation;
    return IQHIP_OK;
}

extern "C" int iqhip_partition_ufboot_update(iqhip_partition *g, const iqhip_ufboot_tree *trees, int ntrees, double epsilon,
                                             double logl_cutoff, int64_t *counts, double *min_orig_logl) {
    const char *what = "iqhip_partition_ufboot_update";
    int rc = use_group(g, what);
    if (rc) return rc;
    UfbootState &u = g->ufb;
    const int P = g->nparts, &S = u.nsamples;
    std::vector<int> ksplit((size_t)P);
    const bool timing = g->m[0]->timing;
    PhaseTimer t_prod(timing, g->stream, 1), t_upd(timing, g->stream, 1);
    UfbOwner o{u, g->stream, 2 * P + 1};
    o.ready = [&] { return group_ufboot_ready(g, what); };
    o.row_ok = [&](const int32_t *row) { return group_rows_ok(g, what, row, 1); };
    o.bytes_per_entry = [&] {
        int64_t bytes = 0;
        for (int p = 0; p < P; p++) {
            ksplit[p] = alrt_ksplit(g->m[p], 1, S);
            bytes += (int64_t)sizeof(double) * S * (ksplit[p] + 1);
        }
        return bytes;
    };
    o.prepare = [&](size_t maxM) { return group_sums_table(g, ksplit, maxM, (size_t)S); };
    o.update = [&](size_t first, int m) {
        return launch_part_ufboot_update(g->stream, g->ufb_sums.d.p, P, S, u.entries.p + first, m, epsilon, u.dbl.p, u.dbl.p + S,
                                         u.counts.p, u.tree.p, ufb_replaced(u), u.res.p + 1);
    };
    o.step = [&](const RowList &rl, size_t first, int m) -> int {
        // (a member's stream waits for the update of the chunk before: its sums are not overwritten under it)
        int rc = group_products(g, rl, ksplit, S, t_prod);
        if (rc || (rc = wait_for_members(g))) return rc;
        t_upd.mark();
        const hipError_t s = o.update(first, m);
        t_upd.mark();
        if ((rc = members_wait(g))) return rc;
        HIPCHK(s);
        return IQHIP_OK;
    };
    if ((rc = ufb_update(what, o, trees, ntrees, epsilon, logl_cutoff, counts, min_orig_logl))) return rc;
    u.ms[0] = u.ms[1] = 0.0;
    t_prod.read(&u.ms[0]);
    t_upd.read(&u.ms[1]);
    return IQHIP_OK;
}

extern "C" int iqhip_partition_ufboot_fetch(iqhip_partition *g, double *boot_logl, double *boot_orig_logl, int32_t *boot_counts,
                                            int64_t *boot_tree) {
    const char *what = "iqhip_partition_ufboot_fetch";
    int rc = use_group(g, what);
    if (rc) return rc;
    if ((rc = group_ufboot_ready(g, what))) return rc;
    return ufb_fetch(g->ufb, g->stream, boot_logl, boot_orig_logl, boot_counts, boot_tree);
}

extern "C" int iqhip_debug_partition_ufboot_timing(iqhip_partition *g, double *ms, int64_t *launches) {
    if (!g) return fail(IQHIP_ERR_INVALID, "iqhip_debug_partition_ufboot_timing: null group");
    return ufb_timing("iqhip_debug_partition_ufboot_timing", g->ufb, ms, launches);
}
