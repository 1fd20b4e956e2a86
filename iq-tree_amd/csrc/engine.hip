// engine.hip -- host side of libiqhip.so: device memory, key->slab map, submissions and the
// extern "C" entry points declared in include/iqhip.h.  There is NO CPU fallback in this
// library: every compute entry point launches HIP kernels or fails with a status.
#include <float.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <atomic>

#include "iqhip_internal.h"

using namespace iqhip;

static thread_local std::string g_err;
namespace iqhip {
int set_error(int code, const std::string &msg) {
    g_err = msg;
    return code;
}
double debug_build_us = 0.0;
}  // namespace iqhip

extern "C" const char *iqhip_last_error(void) { return g_err.c_str(); }
extern "C" int iqhip_abi_version(void) { return IQHIP_ABI_VERSION; }
extern "C" int iqhip_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

static int64_t round_up(int64_t v, int64_t m) { return (v + m - 1) / m * m; }

hipError_t iqhip::use_device(const iqhip_engine *e) { return e->planner ? hipErrorInvalidDevice : hipSetDevice(e->device); }
// everything about an engine that follows from its shape, the CU count (e->num_cus, set by the caller) and the
// environment switches -- no HIP call, so that the planning-only engine of iqhip_debug_create_planner shares it
static void configure_engine(iqhip_engine *e, int device, int nstates, int nstates_user, int ncat, int64_t nptn, int ntaxa) {
    e->device = device;
    e->n = nstates;
    e->n_user = nstates_user;
    e->embed2 = nstates_user != nstates;   // the caller's state count is embedded into the next kernel size
    e->scalar_rule_all = nstates_user != 2 && nstates_user != 4 && nstates_user != 20 && nstates_user != 64;
    e->ncat = ncat;
    e->ntaxa = ntaxa;
    e->nptn = nptn;
    e->wide4 = nstates_user == 4 && ncat > 8;
    // IQHIP_WIDE4=valu | generic: the node update of a wide engine (k_traverse4w | the padded matrix-core kernel).  The
    // default is the generic kernel until k_traverse4w has been measured faster on an MI355X
    e->wide4_generic = e->wide4;
    if (const char *w = getenv("IQHIP_WIDE4")) e->wide4_generic = e->wide4 && strcmp(w, "valu") != 0;   // (check_shape4 has refused every other word)
    e->mfma = nstates != 4 || e->wide4;
    e->mfma_pipelined_ok = ((nstates == 20 && (ncat == 4 || ncat == 1)) || (nstates == 64 && ncat == 1)) &&
                           !getenv("IQHIP_MFMA_V1");
    e->mfma_pipelined = e->mfma_pipelined_ok;
    e->tile = e->mfma ? 16 : 64;
    e->block = nstates * ncat;
    e->nptn_pad = round_up(nptn, 64);
    e->ntiles = e->nptn_pad / e->tile;

    if (const char *ab = getenv("IQHIP_ABLATE")) e->ablate = atoi(ab);
    if (const char *cp = getenv("IQHIP_CHECK_PLAN")) e->check_plans = atoi(cp) != 0;
    if (const char *h = getenv("IQHIP_HOLD")) e->use_hold = atoi(h) != 0;
    if (const char *h = getenv("IQHIP_HOLD_LDS")) e->hold_lds = atoi(h) != 0;
    if (const char *h = getenv("IQHIP_NEWTON_POSTS")) e->newton_posts = atoi(h) != 0;
    if (const char *h = getenv("IQHIP_SMALL_PLANS")) e->small_plans = atoi(h) != 0;
    if (const char *h = getenv("IQHIP_MIXED_TOP")) e->mixed_top = atoi(h) != 0;
    if (const char *f = getenv("IQHIP_FOLD")) e->fold_reduce = atoi(f) != 0;
    if (const char *f = getenv("IQHIP_POLL")) e->poll_result = atoi(f) != 0;
    if (const char *f = getenv("IQHIP_CHERRY_TABLES")) e->cherry_on = atoi(f) != 0;
    if (const char *sp = getenv("IQHIP_SPLIT")) e->split_target = atoi(sp);
    if (const char *ml = getenv("IQHIP_LEVELS")) e->max_levels = std::max(1, atoi(ml));
    if (const char *kb = getenv("IQHIP_MFMA_LDS_KB")) e->mfma_lds_kb = std::max(0, atoi(kb));
    e->debug_plan = getenv("IQHIP_DEBUG_PLAN") != nullptr;
    e->debug_sweep = getenv("IQHIP_DEBUG_SWEEP") != nullptr;
    if (const char *br = getenv("IQHIP_DEBUG_BREAK_PLAN")) e->debug_break_plan = br;
    if (const char *v = getenv("IQHIP_NEWTON")) e->newton_chain_forced = !strcmp(v, "chain");
    if (const char *v = getenv("IQHIP_SWEEP")) e->sweep_one_submission = atoi(v) != 0;
    if (const char *v = getenv("IQHIP_SWEEP_KERNEL")) e->sweep_persistent = atoi(v) != 0;
    if (const char *kb = getenv("IQHIP_LDS_KB")) {
        int v = atoi(kb);
        if (v >= 8 && v <= 150) e->lds_budget_bytes = v * 1024;
    }
    // K2 tables for leaf children: on for 64 states (matrix-pipe bound: 0.50 -> 0.40 ms per traversal at 50 x 20k);
    // off for 20 states, where the traversal is not bound by the MFMA count (1.08 vs 1.11 ms at 100 x 50k) and a model
    // change would cost a table rebuild per evaluation.  IQHIP_LEAF_TABLES=0|1 overrides (tests run both).
    e->leaf_tables = e->mfma_pipelined_ok && nstates == 64;
    if (const char *lt = getenv("IQHIP_LEAF_TABLES")) e->leaf_tables = e->mfma_pipelined_ok && atoi(lt) != 0;
    if (const char *wg = getenv("IQHIP_WG")) {
        int v = atoi(wg);
        if (v == 64 || v == 128 || v == 256) e->wg_size = v;
    }

    // 4-state kernel, two lanes per pattern: twice the waves with half the register state each, as long as
    // they all fit the chip at once (2 waves per SIMD).  Measured, GTR+G4 50 taxa: 10k..65k patterns 0.116..
    // 0.130 ms -> 0.086..0.114 ms; 80k patterns 0.145 -> 0.191 ms (second round).  IQHIP_LANE_SPLIT=1|2 overrides
    if (!e->mfma && ncat % 2 == 0) {
        e->lane_split = (2 * (e->nptn_pad / 64) <= 2 * (int64_t)e->num_cus * 4) ? 2 : 1;
        if (const char *ls = getenv("IQHIP_LANE_SPLIT")) e->lane_split = (atoi(ls) == 2) ? 2 : 1;
    }
    // 20 states x 4 categories on a small alignment: one wave per (tile, category) while that is at most one wave
    // per SIMD (100 taxa: 500 patterns 0.221 -> 0.111 ms, 2000 patterns 0.219 -> 0.145 ms, 8000 patterns 0.247 -> 0.267 ms)
    if (e->mfma_pipelined_ok && e->n == 20 && e->ncat == 4) {
        e->cat_split = 4 * e->ntiles <= (int64_t)e->num_cus * 4;
        if (const char *cs = getenv("IQHIP_CAT_SPLIT")) e->cat_split = atoi(cs) != 0;
        // the dependent top stage of a staged plan with two waves per tile (two categories each, three waves per SIMD) while the
        // alignment has only a few tiles per SIMD: 3125 tiles on 2048 two-wave slots took two rounds of full chains (-1.8 %)
        e->top_cs2 = !e->cat_split && e->ntiles < 6 * (int64_t)e->num_cus * 4;
        if (const char *cs = getenv("IQHIP_TOP_CS2")) e->top_cs2 = atoi(cs) != 0;
    }
    if (e->n == 20) {
        e->mix_generic = getenv("IQHIP_MIX_GENERIC") != nullptr;
        // the mixture kernel's component split while the alignment is small (at most 3/4 tile per SIMD: 10k patterns x 40
        // components 1.96 -> 1.77 ms, but 30k patterns x 8 components 1.78 -> 2.62 ms) and the components divide by 4
        e->mix_split = 4 * e->ntiles <= 3 * (int64_t)e->num_cus * 4;
        if (const char *cs = getenv("IQHIP_CAT_SPLIT")) e->mix_split = atoi(cs) != 0;
        e->mix_split = e->mix_split && e->ncat % 4 == 0;
    }
    if (e->mfma_pipelined_ok && e->n == 64 && e->ncat == 1) {
        e->row_split = 4 * e->ntiles <= (int64_t)e->num_cus * 4;
        if (const char *rs = getenv("IQHIP_ROW_SPLIT")) e->row_split = atoi(rs) != 0;
    }
}

// 4-state kernels: 1 .. 8 categories, and 9 .. 32 for exactly 4 states (binary and 3-state data run on the 4-state
// kernels through the embedding and keep the limit of 8).  A wide engine reads IQHIP_WIDE4: a word other than the two
// routes is refused here, before the device is opened, not taken for one of them
static int check_shape4(const char *who, int nstates, int nstates_user, int ncat) {
    if (nstates != 4) return IQHIP_OK;
    if (!(ncat >= 1 && ncat <= (nstates_user == 4 ? 32 : 8)))
        return fail(IQHIP_ERR_UNSUPPORTED, std::string(who) + (nstates_user == 4 ? ": 4 states support ncat in {1..32}"
                                                                                 : ": 2- and 3-state data support ncat in {1..8}"));
    const char *w = ncat > 8 ? getenv("IQHIP_WIDE4") : nullptr;
    if (w && strcmp(w, "valu") != 0 && strcmp(w, "generic") != 0)
        return fail(IQHIP_ERR_INVALID, std::string(who) + ": IQHIP_WIDE4 must be generic or valu, not '" + w + "'");
    return IQHIP_OK;
}

extern "C" int iqhip_create(iqhip_engine **out, int device, int nstates, int ncat, int64_t nptn,
                            int ntaxa) {
    if (!out) return fail(IQHIP_ERR_INVALID, "iqhip_create: out == NULL");
    *out = nullptr;
    if (nptn <= 0 || ntaxa < 2 || ncat < 1)
        return fail(IQHIP_ERR_INVALID, "iqhip_create: bad nptn/ntaxa/ncat");
    const int nstates_user = nstates;
    // binary data, and every state count the reference hands to its scalar kernel (morphological / multi-state data,
    // phylotreesse.cpp:281-309), run on the next kernel size up through an exact embedding (iqhip_internal.h: embed2)
    if (nstates < 2 || nstates > 64) return fail(IQHIP_ERR_UNSUPPORTED, "iqhip_create: nstates must be 2 .. 64");
    nstates = nstates <= 4 ? 4 : nstates <= 20 ? 20 : 64;
    {
        const int rc = check_shape4("iqhip_create", nstates, nstates_user, ncat);
        if (rc) return rc;
    }
    if (nstates != 4 && ncat > (nstates == 20 ? 96 : 16))  // 20 states: (class, rate) components of mixtures
        return fail(IQHIP_ERR_UNSUPPORTED, "iqhip_create: ncat must be <= 16 (<= 96 components for 20 states)");
    // the 4-state kernels address a vector slab with a wave-uniform base + one 32-bit per-lane byte offset
    // (kernels_valu4.hip, voff): a slab of 4 GiB or more would wrap silently, so it is refused here
    if (nstates == 4 && (uint64_t)round_up(nptn, 64) * (uint64_t)(nstates * ncat) * 8u >= (1ull << 32))
        return fail(IQHIP_ERR_UNSUPPORTED,
                    "iqhip_create: nptn * nstates * ncat * 8 must stay below 4 GiB per vector on the 4-state path "
                    "(shard the patterns over more engines)");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(IQHIP_ERR_NO_DEVICE, "iqhip_create: no HIP device available");
    if (device < 0 || device >= ndev) return fail(IQHIP_ERR_INVALID, "iqhip_create: bad device id");
    HIPCHK(hipSetDevice(device));

    iqhip_engine *e = new iqhip_engine();
    {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0)
            e->num_cus = cus;
    }
    configure_engine(e, device, nstates, nstates_user, ncat, nptn, ntaxa);

    hipError_t s = hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking);
    if (s != hipSuccess) {
        delete e;
        return fail(IQHIP_ERR_HIP, std::string("hipStreamCreate: ") + hipGetErrorString(s));
    }
    e->own_stream = true;
    const size_t P = (size_t)e->nptn_pad;
    bool ok = dmalloc(&e->d_states, (size_t)ntaxa * P) == hipSuccess &&
              dmalloc(&e->d_freq, P) == hipSuccess && dmalloc(&e->d_invar, P) == hipSuccess &&
              dmalloc(&e->d_theta, P * e->block) == hipSuccess &&
              dmalloc(&e->d_pattern_lh, P) == hipSuccess;
    e->result_cap = 8 + 16384;  // up to 16384 node updates per submission
    // default result buffer: pinned host memory mapped into the device address space -- the
    // reduction kernel writes the handful of result doubles straight to the host (no D2H copy
    // on the critical path); a caller-bound device buffer (RCCL) replaces it
    ok = ok && hipHostMalloc((void **)&e->h_result, e->result_cap * sizeof(double), hipHostMallocMapped) == hipSuccess &&
         hipHostGetDevicePointer((void **)&e->d_result_own, e->h_result, 0) == hipSuccess &&
         hipHostMalloc((void **)&e->h_done, 64, hipHostMallocMapped) == hipSuccess &&
         hipHostGetDevicePointer((void **)&e->d_done, (void *)e->h_done, 0) == hipSuccess &&
         hipEventCreateWithFlags(&e->staging_free, hipEventDisableTiming) == hipSuccess;
    if (!ok) {
        iqhip_destroy(e);
        return fail(IQHIP_ERR_NOMEM, "iqhip_create: device allocation failed");
    }
    ok = dmalloc(&e->dummy.plh, P * e->block) == hipSuccess && dmalloc(&e->dummy.sc, P) == hipSuccess;
    if (!ok) {
        iqhip_destroy(e);
        return fail(IQHIP_ERR_NOMEM, "iqhip_create: device allocation failed");
    }
    hipMemsetAsync(e->dummy.plh, 0, P * e->block * sizeof(double), e->stream);
    hipMemsetAsync(e->dummy.sc, 0, P * sizeof(int16_t), e->stream);
    {
        ok = dmalloc(&e->d_newton_partials, (size_t)4 * e->num_cus) == hipSuccess &&
             dmalloc(&e->d_newton_barrier, 2) == hipSuccess && dmalloc(&e->d_fold_ticket, 4) == hipSuccess &&
             dmalloc(&e->d_newton_posts, (size_t)2 * kNewtonPostEpochs * (2 * e->num_cus) * 2) == hipSuccess &&
             dmalloc(&e->d_fold_flags, (size_t)e->result_cap) == hipSuccess;
        if (ok) hipMemsetAsync(e->d_newton_barrier, 0, 2 * sizeof(unsigned int), e->stream);
        if (ok) hipMemsetAsync(e->d_newton_posts, 0xFF, (size_t)2 * kNewtonPostEpochs * (2 * e->num_cus) * 2 * sizeof(double), e->stream);
        if (ok) hipMemsetAsync(e->d_fold_ticket, 0, 4 * sizeof(unsigned int), e->stream);
        if (ok) hipMemsetAsync(e->d_fold_flags, 0, (size_t)e->result_cap * sizeof(int), e->stream);
        if (!ok) {
            iqhip_destroy(e);
            return fail(IQHIP_ERR_NOMEM, "iqhip_create: device allocation failed");
        }
    }
    e->d_result = e->d_result_own;
    hipMemsetAsync(e->d_theta, 0, P * e->block * sizeof(double), e->stream);
    hipMemsetAsync(e->d_pattern_lh, 0, P * sizeof(double), e->stream);
    memset(e->h_result, 0, e->result_cap * sizeof(double));
    *e->h_done = 0;
    hipStreamSynchronize(e->stream);
    *out = e;
    return IQHIP_OK;
}

extern "C" void iqhip_destroy(iqhip_engine *e) {
    if (!e) return;
    if (!e->shards.empty()) {
        sharded::destroy(e);
        delete e;
        return;
    }
    if (e->planner) {
        free(e->h_ops);
        delete e;
        return;
    }
    use_device(e);
    if (e->stream) hipStreamSynchronize(e->stream);
    if (e->pair) iqhip_destroy(e->pair);   // (runs on this engine's stream, which it does not own)
    e->pair = nullptr;
    if (e->d_cherry_tab) hipFree(e->d_cherry_tab);
    comm_destroy(e);
    if (e->d_result_dev) hipFree(e->d_result_dev);
    if (e->d_nstate) hipFree(e->d_nstate);
    if (e->d_bstates) hipFree(e->d_bstates);
    if (e->d_bsc) hipFree(e->d_bsc);
    if (e->h_nstate) hipHostFree(e->h_nstate);
    if (e->stream) hipStreamSynchronize(e->stream);
    for (auto &s : e->slabs) {
        if (s.plh) hipFree(s.plh);
        if (s.sc) hipFree(s.sc);
    }
    void *ptrs[] = {e->d_states, e->d_freq, e->d_invar, e->d_model, e->d_ops, e->d_slab,
                    e->d_theta, e->d_pattern_lh, e->d_leaf_tab, e->dummy.plh, e->dummy.sc, e->d_newton_partials,
                    e->d_newton_barrier, e->d_newton_posts, e->d_fold_ticket, e->d_fold_flags, e->d_ptn_scaled, e->d_boot, e->d_img, e->d_theta_batch, e->d_batch_partials,
                    e->d_batch_out, e->d_batch_barriers, e->d_batch_tasks, e->d_batch_posts, e->d_sweep_len,
                    e->d_ptnlh, e->d_bt_rows, e->d_bt_part, e->d_bt_sums, e->d_bt_out, e->d_batch_rows,
                    e->d_freq_prefix, e->d_tt_var, e->d_tt_dbl, e->d_tt_int,
                    e->d_pd_tiles, e->d_pd_counts, e->d_pd_coef, e->d_pd_init, e->d_pd_out,
                    e->d_pars_vec, e->d_pars_score, e->d_pars_int, e->d_pars_out, e->d_pars_masks};
    for (void *p : ptrs)
        if (p) hipFree(p);
    if (e->h_ops) hipHostFree(e->h_ops);
    for (int32_t *h : {e->h_pars_ops, e->h_pars_ends, e->h_pars_out})
        if (h) hipHostFree(h);
    if (e->h_sweep_desc) hipHostFree(e->h_sweep_desc);
    if (e->h_plan_arena) hipHostFree(e->h_plan_arena);
    if (e->d_sweep_desc) hipFree(e->d_sweep_desc);
    if (e->d_sweep_posts) hipFree(e->d_sweep_posts);
    if (e->h_result) hipHostFree(e->h_result);
    if (e->h_done) hipHostFree((void *)e->h_done);
    if (e->staging_free) hipEventDestroy(e->staging_free);
    for (auto &p : e->tev) {
        hipEventDestroy(p.first);
        hipEventDestroy(p.second);
    }
    for (auto &p : e->cev) {
        hipEventDestroy(p.first);
        hipEventDestroy(p.second);
    }
    if (e->own_stream && e->stream) hipStreamDestroy(e->stream);
    delete e;
}

extern "C" int iqhip_set_stream(iqhip_engine *e, void *hip_stream) {
    if (!e) return fail(IQHIP_ERR_INVALID, "null engine");
    if (!e->shards.empty()) return fail(IQHIP_ERR_UNSUPPORTED, "a sharded engine runs on its shards' own streams");
    HIPCHK(use_device(e));
    HIPCHK(hipStreamSynchronize(e->stream));
    if (e->own_stream) hipStreamDestroy(e->stream);
    e->stream = (hipStream_t)hip_stream;
    e->own_stream = false;
    if (e->pair) return iqhip_set_stream(e->pair, hip_stream);
    return IQHIP_OK;
}

// ---------------------------------------------------------------------------------------
// slabs
// ---------------------------------------------------------------------------------------
static int new_slab(iqhip_engine *e, int *idx) {
    if (!e->free_slabs.empty()) {
        *idx = e->free_slabs.back();
        e->free_slabs.pop_back();
        return IQHIP_OK;
    }
    Slab s;
    const size_t P = (size_t)e->nptn_pad;
    if (e->planner) {
        s.plh = fake_alloc<double>(e, P * e->block);
        s.sc = fake_alloc<int16_t>(e, P);
        e->slabs.push_back(s);
        *idx = (int)e->slabs.size() - 1;
        return IQHIP_OK;
    }
    if (dmalloc(&s.plh, P * e->block) != hipSuccess) return fail(IQHIP_ERR_NOMEM, "slab alloc");
    if (dmalloc(&s.sc, P) != hipSuccess) {
        hipFree(s.plh);
        return fail(IQHIP_ERR_NOMEM, "slab alloc");
    }
    // padded lanes must hold finite values from the start
    hipMemsetAsync(s.plh, 0, P * e->block * sizeof(double), e->stream);
    hipMemsetAsync(s.sc, 0, P * sizeof(int16_t), e->stream);
    e->slabs.push_back(s);
    *idx = (int)e->slabs.size() - 1;
    return IQHIP_OK;
}

int iqhip::slab_for_key(iqhip_engine *e, uint64_t key, bool create, int *idx) {
    auto it = e->key2slab.find(key);
    if (it != e->key2slab.end()) {
        *idx = it->second;
        return IQHIP_OK;
    }
    if (!create) return fail(IQHIP_ERR_INVALID, "unknown partial_lh key (vector never computed)");
    int rc = new_slab(e, idx);
    if (rc) return rc;
    e->key2slab[key] = *idx;
    e->keymap_version++;
    return IQHIP_OK;
}

extern "C" int iqhip_reserve(iqhip_engine *e, int nvectors) {
    if (!e) return fail(IQHIP_ERR_INVALID, "null engine");
    if (!e->shards.empty()) return sharded::reserve(e, nvectors);
    HIPCHK(use_device(e));
    int have = (int)e->slabs.size();
    for (int i = have; i < nvectors; i++) {
        int idx;
        // temporarily empty the free list so that new_slab really allocates
        std::vector<int> keep;
        keep.swap(e->free_slabs);
        int rc = new_slab(e, &idx);
        keep.swap(e->free_slabs);
        if (rc) return rc;
        e->free_slabs.push_back(idx);
    }
    return IQHIP_OK;
}

extern "C" int iqhip_release(iqhip_engine *e, uint64_t key) {
    if (!e) return fail(IQHIP_ERR_INVALID, "null engine");
    if (!e->shards.empty()) return sharded::release(e, key);
    auto it = e->key2slab.find(key);
    if (it == e->key2slab.end()) return IQHIP_OK;
    e->free_slabs.push_back(it->second);
    e->key2slab.erase(it);
    e->keymap_version++;
    return IQHIP_OK;
}

extern "C" int iqhip_rekey(iqhip_engine *e, uint64_t old_key, uint64_t new_key) {
    if (!e) return fail(IQHIP_ERR_INVALID, "null engine");
    if (!e->shards.empty()) return sharded::rekey(e, old_key, new_key);
    auto it = e->key2slab.find(old_key);
    if (it == e->key2slab.end()) return fail(IQHIP_ERR_INVALID, "iqhip_rekey: unknown key");
    if (old_key == new_key) return IQHIP_OK;
    if (e->key2slab.count(new_key)) iqhip_release(e, new_key);
    int idx = it->second;
    e->key2slab.erase(it);
    e->key2slab[new_key] = idx;
    e->keymap_version++;
    return IQHIP_OK;
}

// ---------------------------------------------------------------------------------------
// inputs
// ---------------------------------------------------------------------------------------
extern "C" int iqhip_set_ptn_freq(iqhip_engine *e, const double *ptn_freq) {
    if (!e || !ptn_freq) return fail(IQHIP_ERR_INVALID, "null argument");
    if (!e->shards.empty()) return sharded::set_ptn_array(e, ptn_freq, false);
    HIPCHK(use_device(e));
    std::vector<double> tmp((size_t)e->nptn_pad, 0.0);
    memcpy(tmp.data(), ptn_freq, sizeof(double) * (size_t)e->nptn);
    HIPCHK(hipMemcpyAsync(e->d_freq, tmp.data(), tmp.size() * sizeof(double), hipMemcpyHostToDevice,
                          e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    e->freq_prefix_valid = false;   // (iqhip_gen_boot_samples rebuilds its prefix sums)
    e->h_freq.assign(ptn_freq, ptn_freq + e->nptn);
    e->pars_ready = false;          // (the parsimony sites follow the frequencies: iqhip_pars_init lays them out again)
    return IQHIP_OK;
}

extern "C" int iqhip_set_ptn_invar(iqhip_engine *e, const double *ptn_invar) {
    if (!e || !ptn_invar) return fail(IQHIP_ERR_INVALID, "null argument");
    if (!e->shards.empty()) return sharded::set_ptn_array(e, ptn_invar, true);
    HIPCHK(use_device(e));
    std::vector<double> tmp((size_t)e->nptn_pad, 0.0);
    memcpy(tmp.data(), ptn_invar, sizeof(double) * (size_t)e->nptn);
    HIPCHK(hipMemcpyAsync(e->d_invar, tmp.data(), tmp.size() * sizeof(double),
                          hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return IQHIP_OK;
}

extern "C" int iqhip_set_alignment(iqhip_engine *e, const uint8_t *states, const double *ptn_freq,
                                   const double *ptn_invar) {
    if (!e || !states || !ptn_freq || !ptn_invar) return fail(IQHIP_ERR_INVALID, "null argument");
    if (!e->shards.empty()) return sharded::set_alignment(e, states, ptn_freq, ptn_invar);
    if (!e->model_set)
        return fail(IQHIP_ERR_INVALID,
                    "iqhip_set_alignment: call iqhip_set_model first (needs state_unknown)");
    HIPCHK(use_device(e));
    const size_t P = (size_t)e->nptn_pad, N = (size_t)e->nptn;
    // (embedded data: padding patterns and missing characters are the ambiguity code whose tip row is the caller's
    // unknown row -- internal state n -- never the kernels' own unknown state, whose probability-space vector of exactly
    // 1.0 in every component would leak into the padding components)
    std::vector<uint8_t> tmp((size_t)e->ntaxa * P, (uint8_t)(e->embed2 ? e->n : e->state_unknown));
    for (int t = 0; t < e->ntaxa; t++) {
        const uint8_t *src = states + (size_t)t * N;
        if (e->embed2) {
            uint8_t *dst = tmp.data() + (size_t)t * P;
            for (size_t p = 0; p < N; p++) {
                if (src[p] > e->n_user) return fail(IQHIP_ERR_INVALID, "iqhip_set_alignment: state > STATE_UNKNOWN");
                dst[p] = src[p] == e->n_user ? (uint8_t)e->n : src[p];
            }
            continue;
        }
        for (size_t p = 0; p < N; p++)
            if (src[p] > e->state_unknown)
                return fail(IQHIP_ERR_INVALID, "iqhip_set_alignment: state > STATE_UNKNOWN");
        memcpy(tmp.data() + (size_t)t * P, src, N);
    }
    HIPCHK(hipMemcpyAsync(e->d_states, tmp.data(), tmp.size(), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    e->pars_ready = false;
    int rc = iqhip_set_ptn_freq(e, ptn_freq);
    if (rc) return rc;
    rc = iqhip_set_ptn_invar(e, ptn_invar);
    if (rc) return rc;
    e->aln_set = true;
    return IQHIP_OK;
}

extern "C" int iqhip_set_ascertainment(iqhip_engine *e, int64_t n_unobserved, double nsites) {
    if (!e) return fail(IQHIP_ERR_INVALID, "null engine");
    if (n_unobserved < 0 || n_unobserved >= e->nptn || (n_unobserved > 0 && !(nsites > 0.0)))
        return fail(IQHIP_ERR_INVALID, "iqhip_set_ascertainment: bad pattern count / site count");
    if (!e->shards.empty()) return sharded::set_ascertainment(e, n_unobserved, nsites);
    e->n_unobs = n_unobserved;
    e->asc_nsites = nsites;
    // one rank of a pattern-sharded run (iqhip_comm_init_rank): every rank passes the alignment's site count; the ranks
    // that hold none of the unobserved patterns pass n_unobserved = 0 with nsites > 0
    e->asc_active = n_unobserved > 0 || (e->comm && nsites > 0.0);
    e->pattern_lh_shift = 0.0;
    return IQHIP_OK;
}

static int set_model_common(iqhip_engine *e, int nclass, const int32_t *cat_class, const double *eval,
                            const double *evec, const double *inv_evec, const double *rates, const double *props,
                            int state_unknown, const double *tip /* [state][class][n] */) {
    if (!e || !eval || !evec || !inv_evec || !rates || !props || !tip)
        return fail(IQHIP_ERR_INVALID, "null argument");
    if (!e->shards.empty())
        return sharded::set_model(e, nclass, cat_class, eval, evec, inv_evec, rates, props, state_unknown, tip);
    if (state_unknown < e->n || state_unknown > (e->mfma ? 255 : 31))
        return fail(IQHIP_ERR_INVALID, "iqhip_set_model: state_unknown out of range");
    if (e->aln_set && state_unknown != e->state_unknown)
        return fail(IQHIP_ERR_INVALID, "iqhip_set_model: state_unknown changed after set_alignment");
    if (nclass < 1 || nclass > e->ncat) return fail(IQHIP_ERR_INVALID, "bad number of mixture classes");
    // Mixtures: 20 states have a kernel of their own (k_traverse_mfma_mix20); 64 and 4 states take the generic
    // matrix-core kernel with per-class A images.  A 4-state engine therefore changes its vector layout (64-pattern
    // tiles of the VALU kernels <-> 16-pattern tiles of the matrix-core kernels) when the model becomes / stops being
    // a mixture; as with every model change the caller invalidates all vectors (clearAllPartialLH).
    if (e->n == 4 && !e->wide4) {   // (a wide engine stays on the 16-pattern tiles)
        const bool want_mfma = nclass > 1;
        if (want_mfma != e->mfma) {
            HIPCHK(use_device(e));
            HIPCHK(hipStreamSynchronize(e->stream));
            e->mfma = want_mfma;
            if (want_mfma) { e->lane_split_valu = e->lane_split; e->lane_split = 1; }  // (a VALU-kernel notion)
            else e->lane_split = e->lane_split_valu;
            e->tile = want_mfma ? 16 : 64;
            e->ntiles = e->nptn_pad / e->tile;
            e->plan_cache.invalidate();
            e->theta_valid = false;
            // k_newton's posted exchange resets, per launch, the slots its OWN grid used in the other parity; the grid
            // follows ntiles, so after a layout change start both parities from the all-ones state again
            HIPCHK(hipMemsetAsync(e->d_newton_posts, 0xFF, (size_t)2 * kNewtonPostEpochs * (2 * e->num_cus) * 2 * sizeof(double), e->stream));
            e->newton_post_launches = 0;
        }
    }
    std::vector<int> cls(e->ncat, 0);
    if (nclass > 1) {
        if (!cat_class) return fail(IQHIP_ERR_INVALID, "null argument");
        for (int c = 0; c < e->ncat; c++) {
            if (cat_class[c] < 0 || cat_class[c] >= nclass) return fail(IQHIP_ERR_INVALID, "category class out of range");
            cls[c] = cat_class[c];
        }
    }
    HIPCHK(use_device(e));
    const int n = e->n, C = e->ncat;
    HIPCHK(hipStreamSynchronize(e->stream));  // previous work may still read the old model
    // One device block, one copy per model change (the model optimisers call this once per evaluation):
    // {eval, evec, inv_evec, tip} of class 0 for the 4-state and pipelined kernels, rates, props, the
    // per-category expansions evalc[c][i], tipc[state][c][i], and the category -> class map.
    const size_t nst = (size_t)state_unknown + 1;
    const size_t o_eval = 0, o_evec = o_eval + n, o_ievec = o_evec + (size_t)n * n, o_rates = o_ievec + (size_t)n * n,
                 o_props = o_rates + C, o_tip = o_props + C, o_evalc = o_tip + nst * n, o_tipc = o_evalc + (size_t)C * n,
                 o_cls = o_tipc + nst * C * n;
    const int a_mt = n / 16, a_ks = n / 4;
    const bool a_tail = (n % 16) == 4;
    const size_t aimg_doubles = (n == 20 || n == 64) ? (size_t)2 * a_mt * a_ks * 64 + (a_tail ? (size_t)2 * a_ks * 64 : 0) : 0;
    const size_t o_aimg = (o_cls + ((size_t)C + 1) / 2 + 1) / 2 * 2;   // 16-byte aligned
    const size_t total = o_aimg + aimg_doubles;
    std::vector<double> blk(total, 0.0);
    memcpy(&blk[o_eval], eval, sizeof(double) * n);
    memcpy(&blk[o_evec], evec, sizeof(double) * n * n);
    memcpy(&blk[o_ievec], inv_evec, sizeof(double) * n * n);
    memcpy(&blk[o_rates], rates, sizeof(double) * C);
    memcpy(&blk[o_props], props, sizeof(double) * C);
    for (size_t s = 0; s < nst; s++) memcpy(&blk[o_tip + s * n], &tip[(s * nclass) * n], sizeof(double) * n);
    for (int c = 0; c < C; c++) memcpy(&blk[o_evalc + (size_t)c * n], &eval[(size_t)cls[c] * n], sizeof(double) * n);
    for (size_t s = 0; s < nst; s++)
        for (int c = 0; c < C; c++)
            memcpy(&blk[o_tipc + (s * C + c) * n], &tip[(s * nclass + cls[c]) * n], sizeof(double) * n);
    memcpy(&blk[o_cls], cls.data(), sizeof(int) * C);
    // (iqhip_pars_init recovers the states a code allows from class 0's eigenvectors and tip rows)
    e->h_evec0.assign(evec, evec + (size_t)n * n);
    e->h_tip0.assign(&blk[o_tip], &blk[o_tip] + nst * n);
    if (aimg_doubles) {
        double *U = &blk[o_aimg], *Ui = U + (size_t)a_mt * a_ks * 64, *U4 = Ui + (size_t)a_mt * a_ks * 64, *Ui4 = U4 + (size_t)a_ks * 64;
        for (int m = 0; m < a_mt; m++)
            for (int ks = 0; ks < a_ks; ks++)
                for (int l = 0; l < 64; l++) {
                    const int row = 16 * m + (l & 15), k = 4 * ks + (l >> 4);
                    U[((size_t)m * a_ks + ks) * 64 + l] = evec[(size_t)row * n + k];
                    Ui[((size_t)m * a_ks + ks) * 64 + l] = inv_evec[(size_t)row * n + k];
                }
        if (a_tail)
            for (int ks = 0; ks < a_ks; ks++)
                for (int l = 0; l < 64; l++) {
                    const int row = 16 * a_mt + (l & 3), k = 4 * ks + (l >> 4);
                    U4[(size_t)ks * 64 + l] = evec[(size_t)row * n + k];
                    Ui4[(size_t)ks * 64 + l] = inv_evec[(size_t)row * n + k];
                }
    }
    if (e->model_cap < total) HIPCHK(regrow(e, &e->d_model, &e->model_cap, total, total));
    HIPCHK(hipMemcpy(e->d_model, blk.data(), sizeof(double) * total, hipMemcpyHostToDevice));
    e->d_eval = e->d_model + o_eval;
    e->d_evec = e->d_model + o_evec;
    e->d_inv_evec = e->d_model + o_ievec;
    e->d_rates = e->d_model + o_rates;
    e->d_props = e->d_model + o_props;
    e->d_tip = e->d_model + o_tip;
    e->d_evalc = e->d_model + o_evalc;
    e->d_tipc = e->d_model + o_tipc;
    e->d_cls = reinterpret_cast<int *>(e->d_model + o_cls);
    e->d_aimg = aimg_doubles ? e->d_model + o_aimg : nullptr;
    e->aimg_doubles = (int)aimg_doubles;
    if (nclass > 1 || (e->n == 20 && !e->mfma_pipelined_ok) || e->wide4) {  // (20 states with a category count that has no
        // pipelined instantiation also run on the mixture kernel: one class; wide DNA reads the generic images, one class too)
        // MFMA A-operand images of every class for k_traverse_mfma_mix20: [class][U16 | U4 | Ui16 | Ui4][s][lane]
        // (16-row tile: row = lane & 15; 4-row tail: row = 16 + (lane & 3); k = 4s + (lane >> 4)), followed by
        // the padded two-tile images [class][U | U^-1][m][s][lane] of the generic kernel (IQHIP_MIX_GENERIC)
        const int MT = (n + 15) / 16, KS = n / 4;
        const size_t mix_doubles = (size_t)nclass * 4 * KS * 64;  // (only read by the 20-state kernel)
        std::vector<double> img(mix_doubles + (size_t)nclass * 2 * MT * KS * 64, 0.0);
        for (int m = 0; m < nclass; m++) {
            const double *U = evec + (size_t)m * n * n, *Ui = inv_evec + (size_t)m * n * n;
            for (int s = 0; s < KS; s++)
                for (int l = 0; l < 64; l++) {
                    const int k = 4 * s + (l >> 4), r16 = l & 15, r4 = 16 + (l & 3);
                    double *b = &img[(size_t)m * 4 * KS * 64];
                    if (r16 < n) {
                        b[(0 * KS + s) * 64 + l] = U[r16 * n + k];
                        b[(2 * KS + s) * 64 + l] = Ui[r16 * n + k];
                    }
                    if (r4 < n) {
                        b[(1 * KS + s) * 64 + l] = U[r4 * n + k];
                        b[(3 * KS + s) * 64 + l] = Ui[r4 * n + k];
                    }
                }
            for (int t = 0; t < MT * KS * 64; t++) {
                const int l = t & 63, ms = t >> 6, s = ms % KS, mt = ms / KS;
                const int row = 16 * mt + (l & 15), k = 4 * s + (l >> 4);
                if (row < n) {
                    img[mix_doubles + ((size_t)m * 2 + 0) * MT * KS * 64 + t] = U[row * n + k];
                    img[mix_doubles + ((size_t)m * 2 + 1) * MT * KS * 64 + t] = Ui[row * n + k];
                }
            }
        }
        e->img_generic_off = mix_doubles;
        if (e->img_cap < img.size()) HIPCHK(regrow(e, &e->d_img, &e->img_cap, img.size(), img.size()));
        HIPCHK(hipMemcpy(e->d_img, img.data(), sizeof(double) * img.size(), hipMemcpyHostToDevice));
    }
    // the pipelined kernels hold one eigen-system in registers / LDS: mixtures take the generic kernel,
    // whose plans have a different canonical form -> drop the cached descriptors
    const bool pipelined = e->mfma_pipelined_ok && nclass == 1;
    if (pipelined != e->mfma_pipelined || nclass != e->nclass) {
        e->mfma_pipelined = pipelined;
        e->plan_cache.invalidate();
    }
    e->nclass = nclass;
    e->state_unknown = state_unknown;
    e->model_set = true;
    e->theta_valid = false;
    e->model_version++;
    e->cherry_model_synced = false;
    return IQHIP_OK;
}

// embedded data: pad the caller's m-state system (m = n_user) to the n-state one the kernels run (see iqhip_engine::embed2):
// eigenvalues (l_0 .. l_m-1, 0 ...), U = diag(U_m, I), U^-1 = diag(U_m^-1, I); tip rows of the m states padded with zeros;
// internal state n = "missing" with the caller's unknown row, internal STATE_UNKNOWN = n + 1 (never present in the data, its
// tip row = the caller's unknown row as well)
// ---------------------------------------------------------------------------------------
// cherry tables (DevOp::cherry): which engines use them, and their pair engine
// ---------------------------------------------------------------------------------------
bool iqhip::cherry_candidate(const iqhip_engine *e) {
    if (!e || !e->cherry_on || !e->shards.empty() || e->ablate) return false;   // (a planning-only engine plans them too)
    if (!e->mfma_pipelined_ok || e->n_user != e->n) return false;
    if (e->n == 20) return e->ncat == 4 && !e->leaf_tables && !e->cat_split && e->nptn_pad >= 8 * 1024;
    return false;
}

static int cherry_sync_model(iqhip_engine *e, const double *eval, const double *evec, const double *inv_evec,
                             const double *rates, const double *props, int state_unknown, const double *tip) {
    const int s2 = state_unknown + 1;
    // a table costs one node update over s2^2 patterns per new pair of pendant lengths, and 8 * block * s2^2 bytes
    if (s2 * s2 > 4356 || (int64_t)4 * s2 * s2 > e->nptn_pad) {
        if (e->pair) iqhip_destroy(e->pair);
        e->pair = nullptr;
        return IQHIP_OK;
    }
    if (e->pair && e->cherry_s2 != s2) {
        HIPCHK(hipStreamSynchronize(e->stream));
        iqhip_destroy(e->pair);
        e->pair = nullptr;
    }
    int rc = IQHIP_OK;
    if (!e->pair) {
        const int npairs = s2 * s2;
        rc = iqhip_create(&e->pair, e->device, e->n, e->ncat, npairs, 2);
        if (rc) return rc;
        e->pair->cherry_on = false;
        e->pair->check_plans = e->check_plans;
        rc = iqhip_set_stream(e->pair, e->stream);
        if (rc) return rc;
        e->cherry_s2 = s2;
        e->cherry_npairs = (int)e->pair->nptn_pad;
        e->cherry_slot_of.clear();
        e->cherry_slots.clear();
    }
    rc = set_model_common(e->pair, 1, nullptr, eval, evec, inv_evec, rates, props, state_unknown, tip);
    if (rc) return rc;
    if (!e->pair->aln_set) {
        const int npairs = s2 * s2;
        std::vector<uint8_t> st((size_t)2 * npairs);
        for (int q = 0; q < npairs; q++) {
            st[q] = (uint8_t)(q / s2);
            st[(size_t)npairs + q] = (uint8_t)(q % s2);
        }
        const std::vector<double> ones((size_t)npairs, 1.0), zeros((size_t)npairs, 0.0);
        rc = iqhip_set_alignment(e->pair, st.data(), ones.data(), zeros.data());
    }
    return rc;
}

static int set_model_binary(iqhip_engine *e, const double *eval, const double *evec, const double *inv_evec,
                            const double *rates, const double *props, int state_unknown, const double *tip) {
    if (!eval || !evec || !inv_evec || !rates || !props || !tip) return fail(IQHIP_ERR_INVALID, "null argument");
    const int m = e->n_user, n = e->n;
    if (state_unknown != m)
        return fail(IQHIP_ERR_INVALID, "iqhip_set_model: data of this state count has STATE_UNKNOWN = nstates (no ambiguity codes)");
    std::vector<double> ev((size_t)n, 0.0), U((size_t)n * n, 0.0), Ui((size_t)n * n, 0.0), tp((size_t)(n + 2) * n, 0.0);
    for (int i = 0; i < m; i++) ev[i] = eval[i];
    for (int x = 0; x < m; x++)
        for (int i = 0; i < m; i++) { U[(size_t)x * n + i] = evec[x * m + i]; Ui[(size_t)x * n + i] = inv_evec[x * m + i]; }
    for (int x = m; x < n; x++) U[(size_t)x * n + x] = Ui[(size_t)x * n + x] = 1.0;
    for (int st = 0; st < m; st++)
        for (int i = 0; i < m; i++) tp[(size_t)st * n + i] = tip[st * m + i];
    // row n: the caller's unknown row.  Row n + 1 (the kernels' STATE_UNKNOWN, never in the data) gets it too: the scalar
    // kernel's lh_max == 0 rule writes row STATE_UNKNOWN's vector, which must be the caller's tip_partial_lh[STATE_UNKNOWN]
    // (phylotreesse.cpp:777-788), not zeros
    for (int i = 0; i < m; i++) tp[(size_t)n * n + i] = tp[(size_t)(n + 1) * n + i] = tip[m * m + i];
    return set_model_common(e, 1, nullptr, ev.data(), U.data(), Ui.data(), rates, props, n + 1, tp.data());
}

extern "C" int iqhip_set_model(iqhip_engine *e, const double *eval, const double *evec,
                               const double *inv_evec, const double *rates, const double *props,
                               int state_unknown, const double *tip_partial_lh) {
    if (e && e->embed2 && e->shards.empty())
        return set_model_binary(e, eval, evec, inv_evec, rates, props, state_unknown, tip_partial_lh);
    int rc = set_model_common(e, 1, nullptr, eval, evec, inv_evec, rates, props, state_unknown, tip_partial_lh);
    if (!rc && cherry_candidate(e)) {
        rc = cherry_sync_model(e, eval, evec, inv_evec, rates, props, state_unknown, tip_partial_lh);
        e->cherry_model_synced = !rc && e->pair != nullptr;
    }
    return rc;
}

extern "C" int iqhip_set_mixture_model(iqhip_engine *e, int nclass, const int32_t *cat_class, const double *eval,
                                       const double *evec, const double *inv_evec, const double *rates,
                                       const double *props, int state_unknown, const double *tip_partial_lh) {
    if (e && (e->embed2 || (e->n_user != 4 && e->n_user != 20 && e->n_user != 64)) && nclass > 1)
        return fail(IQHIP_ERR_UNSUPPORTED, "mixture models of embedded data (state counts other than 4, 20, 64) are not implemented");
    if (e && e->embed2 && e->shards.empty())
        return set_model_binary(e, eval, evec, inv_evec, rates, props, state_unknown, tip_partial_lh);
    return set_model_common(e, nclass, cat_class, eval, evec, inv_evec, rates, props, state_unknown, tip_partial_lh);
}

// ---------------------------------------------------------------------------------------
// submissions (the descriptors come from the planner, plan.hip)
// ---------------------------------------------------------------------------------------
int iqhip::ensure_slab_rows(iqhip_engine *e, int nrows) {
    const int64_t need = (int64_t)nrows * e->ntiles * e->lane_split;
    if (need <= e->slab_cap) return IQHIP_OK;
    HIPCHK(regrow(e, &e->d_slab, &e->slab_cap, need, need));
    return IQHIP_OK;
}

int iqhip::check_ready(iqhip_engine *e) {
    if (!e) return fail(IQHIP_ERR_INVALID, "null engine");
    if (!e->model_set || !e->aln_set)
        return fail(IQHIP_ERR_INVALID, "engine needs iqhip_set_model and iqhip_set_alignment first");
    hipError_t s = use_device(e);
    if (s != hipSuccess) return fail(IQHIP_ERR_HIP, hipGetErrorString(s));
    return IQHIP_OK;
}

static void timing_begin(iqhip_engine *e) {
    if (!e->timing) return;
    if (e->tev_used == e->tev.size()) {
        hipEvent_t a, b;
        hipEventCreate(&a);
        hipEventCreate(&b);
        e->tev.emplace_back(a, b);
    }
    hipEventRecord(e->tev[e->tev_used].first, e->stream);
}
static void timing_end(iqhip_engine *e) {
    if (!e->timing) return;
    hipEventRecord(e->tev[e->tev_used].second, e->stream);
    e->tev_used++;
}

// the tables the current plan needs: one node update per table on the pair engine (independent segments of one
// submission, same stream), then the move into register order
static int build_cherry_tables(iqhip_engine *e) {
    iqhip_engine *p = e->pair;
    const int n = (int)e->plan.cherry_jobs.size();
    std::vector<iqhip_node_op> ops((size_t)n);
    const std::vector<int> segs((size_t)n, 1);
    for (int i = 0; i < n; i++) {
        const iqhip_engine::CherrySlot &cs = e->cherry_slots[e->plan.cherry_jobs[i]];
        iqhip_node_op &o = ops[i];
        memset(&o, 0, sizeof o);
        o.dst_key = (uint64_t)e->plan.cherry_jobs[i] + 1;
        o.left_leaf = 0;
        o.right_leaf = 1;
        o.left_len = cs.len_l;
        o.right_len = cs.len_r;
    }
    iqhip_branch_end none = {0, -1, 0};
    int rc = submit_traverse(p, ops.data(), n, false, none, none, 0.0, /*skip_reduce=*/true, &segs, nullptr);
    if (rc) return rc;
    std::vector<const double *> src((size_t)n);
    std::vector<double *> dst((size_t)n);
    const size_t per = (size_t)e->cherry_npairs * e->block;
    for (int i = 0; i < n; i++) {
        int idx;
        rc = slab_for_key(p, ops[i].dst_key, false, &idx);
        if (rc) return rc;
        src[i] = p->slabs[idx].plh;
        dst[i] = e->d_cherry_tab + (size_t)e->plan.cherry_jobs[i] * per;
    }
    HIPCHK(launch_cherry_transpose(e, src.data(), dst.data(), n, e->cherry_npairs));
    for (int i = 0; i < n; i++) e->cherry_slots[e->plan.cherry_jobs[i]].model_version = e->model_version;
    e->cherry_built_total += n;
    e->plan.cherry_jobs.clear();
    return IQHIP_OK;
}

// enqueue: plan upload, K1, fused traversal (+ optional root lnL), fixed-order reduction
int iqhip::submit_traverse(iqhip_engine *e, const iqhip_node_op *ops, int nops, bool has_root,
                           iqhip_branch_end a, iqhip_branch_end b, double len, bool skip_reduce,
                           const std::vector<int> *explicit_segs, const double *const *len_ptrs) {
    int rc = check_ready(e);
    if (rc) return rc;
    if (nops < 0 || (nops > 0 && !ops)) return fail(IQHIP_ERR_INVALID, "bad ops array");
    int last_dst = -1;
    Stopwatch watch;
    if (e->debug_sweep) watch.start();
    rc = build_plan(e, ops, nops, &last_dst, explicit_segs, len_ptrs);
    if (rc) return rc;
    if (e->debug_sweep) debug_build_us += watch.us();
    DevBranch br;
    if (has_root) {
        rc = build_branch(e, a, b, len, last_dst, &br);
        if (rc) return rc;
    }
    rc = ensure_slab_rows(e, 2 + nops);
    if (rc) return rc;
    const int nwaves = (int)e->ntiles * e->lane_split;  // columns of the wave-partial slab
    if (e->plan.nleaf_tabs > 0) {
        // tables whose branch length changed since they were built -- all of the plan's after a model change
        // (a cached plan skipped build_plan, which is where a model change is normally noticed)
        const int njobs = leaf_tables_follow_model(e) ? e->plan.nleaf_tabs : e->plan.tab_dirty;
        if (njobs > 0)
            HIPCHK(launch_leaf_tables(e, reinterpret_cast<const TabJob *>(e->d_ops + e->plan.jobs_off), njobs));
        e->plan.tab_dirty = 0;  // built; the same (cached) plan needs nothing until a length or the model changes
    }
    if (!e->plan.cherry_jobs.empty()) {
        rc = build_cherry_tables(e);
        if (rc) return rc;
    }
    if (e->plan.uses_cherry)
        for (int k = 0; k < nops; k++) e->cherry_ops_total += e->h_ops[k].cherry != nullptr;
    timing_begin(e);
    const int *table = reinterpret_cast<const int *>(e->d_ops + e->plan.table_off);
    {   // the stages of independent subtrees, level by level: one launch each, one set of workgroups per unit
        int off = 2;
        for (int n : e->plan.stage_units) {
            if (e->mfma) HIPCHK(launch_traverse_mfma(e, table + off, n, nwaves));
            else HIPCHK(launch_traverse4(e, table + off, n, e->plan.units_have_load, nullptr, nwaves));
            off += 2 * n;
        }
    }
    const bool empty_top = e->plan.nunits > 0 && !has_root && e->plan.top_nops == 0;  // explicit segments only
    // the submission's last kernel sums the wave partials itself (FoldArgs) where it can: the 4-state traversal
    // (its top-stage launch) and the matrix-core path's root-branch kernel; otherwise a k_reduce launch follows
    const bool fold4 = e->fold_reduce && !e->mfma && !empty_top && !skip_reduce && e->wg_size == 256;
    const bool foldm = e->fold_reduce && e->mfma && has_root && e->n_unobs == 0;
    if (empty_top) {
    } else if (e->mfma) HIPCHK(launch_traverse_mfma(e, table, nops > 0 ? 1 : 0, nwaves, /*top_stage=*/true));
    else HIPCHK(launch_traverse4(e, table, 1, e->plan.has_load, has_root ? &br : nullptr, nwaves, fold4 ? nops : -1));
    timing_end(e);
    if (e->timing) e->tev_launches += (int)e->plan.stage_units.size() + (empty_top ? 0 : 1);
    if (e->mfma && has_root) HIPCHK(launch_stream_mfma(e, 0, &br, br.len, nwaves, nullptr, foldm ? nops : -1));
    if (fold4 || foldm) {
    } else if (has_root) HIPCHK(launch_reduce(e, 0, 2 + nops, nwaves));
    else if (!skip_reduce) HIPCHK(launch_reduce(e, 2, nops, nwaves));
    e->last_nops = nops;
    e->last_has_root = has_root;
    e->last_root_loads_b = has_root && br.b_kind != CHILD_PREV;
    return IQHIP_OK;
}

int iqhip::read_result(iqhip_engine *e, int ndoubles) {
    if (e->d_result != e->d_result_own)  // caller-bound device buffer
        HIPCHK(hipMemcpyAsync(e->h_result, e->d_result, sizeof(double) * ndoubles, hipMemcpyDeviceToHost,
                              e->stream));
    else if (e->poll_pending) {
        // the last kernel of the submission is a k_reduce that publishes a sequence number in mapped host memory:
        // spinning on it sees the result a few microseconds before a stream synchronisation returns.  Bounded: long
        // kernels fall through to the ordinary wait.
        e->poll_pending = false;
        const unsigned long long want = e->result_seq;
        for (int spin = 0; spin < 200000; spin++) {
            if (*e->h_done == want) {
                std::atomic_thread_fence(std::memory_order_acquire);
                e->staging_busy = false;  // (in-order stream: the plan upload finished long before k_reduce)
                if (e->folded_rows >= 0) {   // folded reduction: unflagged sum_scale rows were not written (fold_tail)
                    if (e->h_result[2 + e->folded_rows] == 0.0)
                        for (int k = 0; k < e->folded_rows; k++) e->h_result[2 + k] = 0.0;
                    e->folded_rows = -1;
                }
                return IQHIP_OK;
            }
            __builtin_ia32_pause();
        }
    }
    e->poll_pending = false;
    HIPCHK(hipStreamSynchronize(e->stream));
    e->staging_busy = false;
    if (e->folded_rows >= 0) {
        if (e->h_result[2 + e->folded_rows] == 0.0)
            for (int k = 0; k < e->folded_rows; k++) e->h_result[2 + k] = 0.0;
        e->folded_rows = -1;
    }
    return IQHIP_OK;
}

// the NaN/Inf repair of phylokernel.h:848-866 / :1100-1122, done on the (rare) slow path
static int repair_lnl(iqhip_engine *e, double *lnl) {
    std::vector<double> plh((size_t)e->nptn_pad), freq((size_t)e->nptn_pad);
    HIPCHK(hipMemcpy(plh.data(), e->d_pattern_lh, sizeof(double) * plh.size(), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(freq.data(), e->d_freq, sizeof(double) * freq.size(), hipMemcpyDeviceToHost));
    double s = 0.0;
    for (int64_t p = 0; p < e->nptn; p++) {
        if (isnan(plh[p]) || isinf(plh[p])) plh[p] = kLogScalingThreshold * 4;
        s += plh[p] * freq[p];
    }
    HIPCHK(hipMemcpy(e->d_pattern_lh, plh.data(), sizeof(double) * plh.size(), hipMemcpyHostToDevice));
    *lnl = s;
    return IQHIP_OK;
}

// +ASC finalisation of a lnL evaluation (phylokernel.h:1009-1016, 1183-1186): result[1] holds
// prob_const; tree_lh -= nsites*log(1-prob_const), _pattern_lh[observed] -= log(1-prob_const)
int iqhip::asc_log_term(double prob_const, double *lp) {
    if (!(prob_const < 1.0 && prob_const >= 0.0))
        return fail(IQHIP_ERR_INVALID, "+ASC: prob_const outside [0,1) (the reference asserts here)");
    *lp = log(1.0 - prob_const);
    return IQHIP_OK;
}

static int asc_finish_lnl(iqhip_engine *e, double *lnl) {
    e->pattern_lh_shift = 0.0;
    if (!e->asc_active) return IQHIP_OK;
    double lp;
    const int rc = asc_log_term(e->h_result[1], &lp);
    if (rc) return rc;
    e->pattern_lh_shift = lp;
    *lnl -= e->asc_nsites * lp;
    return IQHIP_OK;
}

int iqhip::eng_repair_lnl(iqhip_engine *e, double *lnl) { return repair_lnl(e, lnl); }

// Sharded engines (comm.hip): a non-finite lnL is repaired rank by rank (each rank fixes its own _pattern_lh and
// re-sums its share), then the shares are all-reduced again.  Every rank sees the same all-reduced value, so every
// rank takes this branch together.
static int repair_lnl_comm(iqhip_engine *e, double *lnl) {
    int rc = repair_lnl(e, lnl);
    if (rc || !e->comm) return rc;
    HIPCHK(hipMemcpyAsync(e->d_result, lnl, sizeof(double), hipMemcpyHostToDevice, e->stream));
    rc = comm_allreduce(e, 1);
    if (rc) return rc;
    rc = read_result(e, 1);
    if (rc) return rc;
    *lnl = e->h_result[0];
    return IQHIP_OK;
}

extern "C" int iqhip_update_partials(iqhip_engine *e, const iqhip_node_op *ops, int nops,
                                     double *sum_scale) {
    iqhip_branch_end none = {0, -1, 0};
    if (e && !e->shards.empty()) return sharded::traverse(e, ops, nops, false, none, none, 0.0, sum_scale, nullptr);
    int rc = submit_traverse(e, ops, nops, false, none, none, 0.0);
    if (rc) return rc;
    rc = comm_allreduce(e, 2 + nops);
    if (rc) return rc;
    rc = read_result(e, 2 + nops);
    if (rc) return rc;
    if (sum_scale)
        for (int k = 0; k < nops; k++) sum_scale[k] = e->h_result[2 + k];
    return IQHIP_OK;
}

extern "C" int iqhip_traverse_lnl(iqhip_engine *e, const iqhip_node_op *ops, int nops,
                                  iqhip_branch_end a, iqhip_branch_end b, double len,
                                  double *sum_scale, double *lnl) {
    if (e && !e->shards.empty()) return sharded::traverse(e, ops, nops, true, a, b, len, sum_scale, lnl);
    int rc = submit_traverse(e, ops, nops, true, a, b, len);
    if (rc) return rc;
    rc = comm_allreduce(e, 2 + nops);
    if (rc) return rc;
    rc = read_result(e, 2 + nops);
    if (rc) return rc;
    if (sum_scale)
        for (int k = 0; k < nops; k++) sum_scale[k] = e->h_result[2 + k];
    double v = e->h_result[0];
    if (isnan(v) || isinf(v)) {
        rc = repair_lnl_comm(e, &v);
        if (rc) return rc;
    }
    rc = asc_finish_lnl(e, &v);
    if (rc) return rc;
    if (lnl) *lnl = v;
    return IQHIP_OK;
}

extern "C" int iqhip_branch_lnl(iqhip_engine *e, iqhip_branch_end a, iqhip_branch_end b, double len,
                                double *lnl) {
    return iqhip_traverse_lnl(e, nullptr, 0, a, b, len, nullptr, lnl);
}

extern "C" int iqhip_traverse_lnl_async(iqhip_engine *e, const iqhip_node_op *ops, int nops,
                                        iqhip_branch_end a, iqhip_branch_end b, double len) {
    if (e && !e->shards.empty())
        return fail(IQHIP_ERR_UNSUPPORTED, "a sharded engine reduces its results itself: use the synchronous calls");
    // (+ASC: result[1] then holds this engine's share of prob_const; the caller owns the correction, phylokernel.h:1009-1016)
    return submit_traverse(e, ops, nops, true, a, b, len);
}

extern "C" int iqhip_update_partials_async(iqhip_engine *e, const iqhip_node_op *ops, int nops) {
    if (e && !e->shards.empty())
        return fail(IQHIP_ERR_UNSUPPORTED, "a sharded engine reduces its results itself: use the synchronous calls");
    iqhip_branch_end none = {0, -1, 0};
    return submit_traverse(e, ops, nops, false, none, none, 0.0);
}

void iqhip::set_theta_branch(iqhip_engine *e, const DevBranch &br) {
    e->theta_valid = true;
    e->theta_a_sc = br.a_sc;
    e->theta_b_sc = br.b_sc;
}

extern "C" int iqhip_compute_theta(iqhip_engine *e, iqhip_branch_end a, iqhip_branch_end b) {
    if (e && !e->shards.empty()) return sharded::compute_theta(e, a, b);
    int rc = check_ready(e);
    if (rc) return rc;
    DevBranch br;
    rc = build_branch(e, a, b, 0.0, -1, &br);
    if (rc) return rc;
    if (e->mfma) HIPCHK(launch_stream_mfma(e, 1, &br, 0.0, (int)e->ntiles));
    else HIPCHK(launch_theta4(e, br));
    set_theta_branch(e, br);
    return IQHIP_OK;
}

extern "C" int iqhip_derv_async(iqhip_engine *e, double len) {
    if (e && !e->shards.empty())
        return fail(IQHIP_ERR_UNSUPPORTED, "a sharded engine reduces its results itself: use the synchronous calls");
    int rc = check_ready(e);
    if (rc) return rc;
    if (!e->theta_valid) return fail(IQHIP_ERR_INVALID, "iqhip_derv: theta not computed");
    if (!(len >= 0.0)) return fail(IQHIP_ERR_INVALID, "negative or NaN branch length");
    const int nrows = e->n_unobs > 0 ? 5 : 2;  // +ASC: prob_const, df_const, ddf_const as well
    if (e->asc_active && e->n_unobs == 0) {   // a shard without unobserved patterns contributes zeros to those three sums
        if (e->d_result == e->d_result_own) e->h_result[2] = e->h_result[3] = e->h_result[4] = 0.0;
        else HIPCHK(hipMemsetAsync(e->d_result + 2, 0, 3 * sizeof(double), e->stream));
    }
    rc = ensure_slab_rows(e, nrows);
    if (rc) return rc;
    const int nwaves = (int)e->ntiles;
    if (e->mfma) HIPCHK(launch_stream_mfma(e, 2, nullptr, len, nwaves));
    else HIPCHK(launch_derv4(e, len, nwaves));
    HIPCHK(launch_reduce(e, 0, nrows, nwaves));
    return IQHIP_OK;
}

extern "C" int iqhip_derv(iqhip_engine *e, double len, double *df, double *ddf) {
    if (e && !e->shards.empty()) return sharded::derv(e, len, df, ddf);
    int rc = iqhip_derv_async(e, len);
    if (rc) return rc;
    rc = comm_allreduce(e, e->asc_active ? 5 : 2);
    if (rc) return rc;
    rc = read_result(e, e->asc_active ? 5 : 2);
    if (rc) return rc;
    double a = e->h_result[0], b = e->h_result[1];
    if (isnan(a) || isinf(a)) { a = 0.0; b = 0.0; }  // phylokernel.h:647-651
    if (e->asc_active) {  // phylokernel.h:719-724
        const double prob_const = 1.0 - e->h_result[2];
        const double df_frac = e->h_result[3] / prob_const, ddf_frac = e->h_result[4] / prob_const;
        a += e->asc_nsites * df_frac;
        b += e->asc_nsites * (ddf_frac + df_frac * df_frac);
    }
    if (df) *df = a;
    if (ddf) *ddf = b;
    return IQHIP_OK;
}

extern "C" int iqhip_debug_cherry_tables(iqhip_engine *e, int64_t *tables_built, int64_t *ops_from_tables) {
    if (!e) return fail(IQHIP_ERR_INVALID, "null engine");
    if (tables_built) *tables_built = e->cherry_built_total;
    if (ops_from_tables) *ops_from_tables = e->cherry_ops_total;
    return IQHIP_OK;
}

extern "C" int iqhip_debug_path_counts(iqhip_engine *e, int64_t *out, int n) {
    if (!e) return fail(IQHIP_ERR_INVALID, "null engine");
    if (!out && n > 0) return fail(IQHIP_ERR_INVALID, "null argument");
    for (int k = 0; k < n && k < IQHIP_PATH_NSLOTS; k++) out[k] = e->path_counts[k];
    return IQHIP_OK;
}

extern "C" int iqhip_lnl_from_theta_async(iqhip_engine *e, double len) {
    if (e && !e->shards.empty())
        return fail(IQHIP_ERR_UNSUPPORTED, "a sharded engine reduces its results itself: use the synchronous calls");
    int rc = check_ready(e);
    if (rc) return rc;
    if (!e->theta_valid) return fail(IQHIP_ERR_INVALID, "iqhip_lnl_from_theta: theta not computed");
    if (!(len >= 0.0)) return fail(IQHIP_ERR_INVALID, "negative or NaN branch length");
    rc = ensure_slab_rows(e, 2);
    if (rc) return rc;
    const int nwaves = (int)e->ntiles;
    if (e->mfma) HIPCHK(launch_stream_mfma(e, 3, nullptr, len, nwaves));
    else HIPCHK(launch_lnl_theta4(e, len, nwaves));
    HIPCHK(launch_reduce(e, 0, 2, nwaves));
    return IQHIP_OK;
}

extern "C" int iqhip_lnl_from_theta(iqhip_engine *e, double len, double *lnl) {
    if (e && !e->shards.empty()) return sharded::lnl_from_theta(e, len, lnl);
    int rc = iqhip_lnl_from_theta_async(e, len);
    if (rc) return rc;
    rc = comm_allreduce(e, e->asc_active ? 2 : 1);
    if (rc) return rc;
    rc = read_result(e, 2);
    if (rc) return rc;
    double v = e->h_result[0];
    if (isnan(v) || isinf(v)) {
        rc = repair_lnl_comm(e, &v);
        if (rc) return rc;
    }
    rc = asc_finish_lnl(e, &v);
    if (rc) return rc;
    if (lnl) *lnl = v;
    return IQHIP_OK;
}

// ---------------------------------------------------------------------------------------
// result buffer / sync
// ---------------------------------------------------------------------------------------
extern "C" int iqhip_bind_result_buffer(iqhip_engine *e, void *device_ptr, int capacity_doubles) {
    if (!e) return fail(IQHIP_ERR_INVALID, "null engine");
    if (!e->shards.empty() || e->comm)
        return fail(IQHIP_ERR_UNSUPPORTED, "an engine with a communicator reduces in its own device result vector");
    HIPCHK(use_device(e));
    HIPCHK(hipStreamSynchronize(e->stream));
    if (!device_ptr) {
        e->d_result = e->d_result_own;
        e->result_cap = 8 + 16384;
        return IQHIP_OK;
    }
    if (capacity_doubles < 2) return fail(IQHIP_ERR_INVALID, "result buffer too small");
    e->d_result = (double *)device_ptr;
    e->result_cap = std::min(capacity_doubles, 8 + 16384);
    return IQHIP_OK;
}
extern "C" void *iqhip_result_device_ptr(iqhip_engine *e) { return (e && e->shards.empty()) ? (void *)e->d_result : nullptr; }
extern "C" int iqhip_result_capacity(iqhip_engine *e) { return e ? e->result_cap : 0; }

extern "C" int iqhip_result_read(iqhip_engine *e, double *out, int ndoubles) {
    if (e && !e->shards.empty())
        return fail(IQHIP_ERR_UNSUPPORTED, "a sharded engine reduces its results itself: use the synchronous calls");
    if (!e || !out || ndoubles < 0 || ndoubles > e->result_cap)
        return fail(IQHIP_ERR_INVALID, "iqhip_result_read: bad arguments");
    HIPCHK(use_device(e));
    int rc = read_result(e, ndoubles);
    if (rc) return rc;
    memcpy(out, e->h_result, sizeof(double) * ndoubles);
    return IQHIP_OK;
}

extern "C" int iqhip_synchronize(iqhip_engine *e) {
    if (!e) return fail(IQHIP_ERR_INVALID, "null engine");
    if (!e->shards.empty()) return sharded::synchronize(e);
    HIPCHK(use_device(e));
    HIPCHK(hipStreamSynchronize(e->stream));
    e->staging_busy = false;
    return IQHIP_OK;
}

// ---------------------------------------------------------------------------------------
// host views (layout conversion on the host; these are off the hot path)
// ---------------------------------------------------------------------------------------
static inline size_t dev_index(const iqhip_engine *e, int64_t p, int k) {
    const int B = e->block;
    if (e->mfma) return (size_t)(p >> 4) * 16 * B + (size_t)k * 16 + (size_t)(p & 15);
    return (size_t)(p >> 6) * 64 * B + (size_t)(k >> 1) * 128 + (size_t)(p & 63) * 2 + (k & 1);
}

static int fetch_vec(iqhip_engine *e, const double *dptr, double *out) {
    std::vector<double> tmp((size_t)e->nptn_pad * e->block);
    HIPCHK(hipStreamSynchronize(e->stream));
    HIPCHK(hipMemcpy(tmp.data(), dptr, tmp.size() * sizeof(double), hipMemcpyDeviceToHost));
    const int B = e->block;
    if (e->embed2) {  // the caller's block is n_user doubles per category: the first components of the embedded vector
        const int m = e->n_user, n = e->n;
        for (int64_t p = 0; p < e->nptn; p++)
            for (int c = 0; c < e->ncat; c++)
                for (int i = 0; i < m; i++) out[((size_t)p * e->ncat + c) * m + i] = tmp[dev_index(e, p, c * n + i)];
        return IQHIP_OK;
    }
    for (int64_t p = 0; p < e->nptn; p++)
        for (int k = 0; k < B; k++) out[(size_t)p * B + k] = tmp[dev_index(e, p, k)];
    return IQHIP_OK;
}

extern "C" int iqhip_fetch_partial(iqhip_engine *e, uint64_t key, double *out) {
    if (!e || !out) return fail(IQHIP_ERR_INVALID, "null argument");
    if (!e->shards.empty()) return sharded::fetch_vec(e, key, false, out);
    HIPCHK(use_device(e));
    int idx;
    int rc = slab_for_key(e, key, false, &idx);
    if (rc) return rc;
    return fetch_vec(e, e->slabs[idx].plh, out);
}

extern "C" int iqhip_fetch_theta(iqhip_engine *e, double *out) {
    if (!e || !out) return fail(IQHIP_ERR_INVALID, "null argument");
    if (!e->shards.empty()) return sharded::fetch_vec(e, 0, true, out);
    HIPCHK(use_device(e));
    return fetch_vec(e, e->d_theta, out);
}

extern "C" int iqhip_fetch_scale_num(iqhip_engine *e, uint64_t key, int16_t *out) {
    if (!e || !out) return fail(IQHIP_ERR_INVALID, "null argument");
    if (!e->shards.empty()) return sharded::fetch_scale_num(e, key, out);
    HIPCHK(use_device(e));
    int idx;
    int rc = slab_for_key(e, key, false, &idx);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(e->stream));
    HIPCHK(hipMemcpy(out, e->slabs[idx].sc, sizeof(int16_t) * (size_t)e->nptn, hipMemcpyDeviceToHost));
    return IQHIP_OK;
}

extern "C" int iqhip_fetch_pattern_lh(iqhip_engine *e, double *out) {
    if (!e || !out) return fail(IQHIP_ERR_INVALID, "null argument");
    if (!e->shards.empty()) return sharded::fetch_pattern_lh(e, out, 0, iqhip_branch_end{0, -1, 0}, iqhip_branch_end{0, -1, 0});
    HIPCHK(use_device(e));
    HIPCHK(hipStreamSynchronize(e->stream));
    HIPCHK(hipMemcpy(out, e->d_pattern_lh, sizeof(double) * (size_t)e->nptn, hipMemcpyDeviceToHost));
    if (e->asc_active) {  // phylokernel.h:1013-1014: observed patterns only
        const int64_t nobs = e->nptn - e->n_unobs;
        for (int64_t p = 0; p < nobs; p++) out[p] -= e->pattern_lh_shift;
        for (int64_t p = nobs; p < e->nptn; p++) out[p] = 0.0;
    }
    return IQHIP_OK;
}

// ---- consumers of the device-resident pattern lnL (kernels_rell.hip) ---------------------------
static int scaled_pattern_lh(iqhip_engine *e, iqhip_branch_end a, iqhip_branch_end b) {
    const int16_t *sc[2] = {nullptr, nullptr};
    const iqhip_branch_end ends[2] = {a, b};
    for (int k = 0; k < 2; k++) {
        if (ends[k].leaf >= 0) continue;  // leaves carry no scaling events
        int idx;
        int rc = slab_for_key(e, ends[k].key, false, &idx);
        if (rc) return rc;
        sc[k] = e->slabs[idx].sc;
    }
    if (!e->d_ptn_scaled) HIPCHK(hipMalloc((void **)&e->d_ptn_scaled, sizeof(double) * (size_t)e->nptn_pad));
    HIPCHK(launch_pattern_lh_scaled(e, sc[0], sc[1], e->d_ptn_scaled));
    return IQHIP_OK;
}

extern "C" int iqhip_fetch_pattern_lh_scaled(iqhip_engine *e, iqhip_branch_end a, iqhip_branch_end b, double *out) {
    if (!e || !out) return fail(IQHIP_ERR_INVALID, "null argument");
    if (!e->shards.empty()) return sharded::fetch_pattern_lh(e, out, 1, a, b);
    HIPCHK(use_device(e));
    int rc = scaled_pattern_lh(e, a, b);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(out, e->d_ptn_scaled, sizeof(double) * (size_t)e->nptn, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return IQHIP_OK;
}

extern "C" int iqhip_pattern_lh_cat(iqhip_engine *e, double len, double *out) {
    if (!e || !out) return fail(IQHIP_ERR_INVALID, "null argument");
    if (!e->shards.empty()) return sharded::pattern_lh_cat(e, len, out);
    if (!e->theta_valid) return fail(IQHIP_ERR_INVALID, "iqhip_pattern_lh_cat needs iqhip_compute_theta first");
    if (!(len >= 0.0)) return fail(IQHIP_ERR_INVALID, "negative or NaN branch length");
    HIPCHK(use_device(e));
    const size_t count = (size_t)e->nptn * e->ncat;
    double *d_out = nullptr;
    HIPCHK(hipMalloc((void **)&d_out, sizeof(double) * count));
    hipError_t s = launch_pattern_lh_cat(e, len, d_out);
    if (s == hipSuccess) s = hipMemcpyAsync(out, d_out, sizeof(double) * count, hipMemcpyDeviceToHost, e->stream);
    if (s == hipSuccess) s = hipStreamSynchronize(e->stream);
    hipFree(d_out);
    if (s != hipSuccess) return fail(IQHIP_ERR_HIP, hipGetErrorString(s));
    return IQHIP_OK;
}

extern "C" int iqhip_set_boot_samples(iqhip_engine *e, const float *samples, int nsamples) {
    if (!e || (nsamples > 0 && !samples) || nsamples < 0) return fail(IQHIP_ERR_INVALID, "bad bootstrap samples");
    if (nsamples > 16384) return fail(IQHIP_ERR_INVALID, "at most 16384 bootstrap samples");
    if (!e->shards.empty()) return sharded::set_boot_samples(e, samples, nsamples);
    HIPCHK(use_device(e));
    HIPCHK(hipStreamSynchronize(e->stream));
    if (e->d_boot) HIPCHK(hipFree(e->d_boot));
    e->d_boot = nullptr;
    e->nboot = 0;
    if (nsamples == 0) return IQHIP_OK;
    const size_t pitch = (size_t)e->nptn_pad;
    HIPCHK(hipMalloc((void **)&e->d_boot, sizeof(float) * pitch * nsamples));
    HIPCHK(hipMemset(e->d_boot, 0, sizeof(float) * pitch * nsamples));
    HIPCHK(hipMemcpy2D(e->d_boot, pitch * sizeof(float), samples, (size_t)e->nptn * sizeof(float),
                       (size_t)e->nptn * sizeof(float), nsamples, hipMemcpyHostToDevice));
    e->nboot = nsamples;
    return IQHIP_OK;
}

extern "C" int iqhip_rell_async(iqhip_engine *e, iqhip_branch_end a, iqhip_branch_end b) {
    if (!e) return fail(IQHIP_ERR_INVALID, "null engine");
    if (!e->shards.empty())
        return fail(IQHIP_ERR_UNSUPPORTED, "a sharded engine reduces its results itself: use the synchronous calls");
    if (e->nboot == 0) return fail(IQHIP_ERR_INVALID, "no bootstrap samples (iqhip_set_boot_samples)");
    if (e->nboot > e->result_cap) return fail(IQHIP_ERR_INVALID, "result buffer too small for the sample count");
    HIPCHK(use_device(e));
    int rc = scaled_pattern_lh(e, a, b);
    if (rc) return rc;
    HIPCHK(launch_rell(e, e->d_result));
    return IQHIP_OK;
}

extern "C" int iqhip_rell(iqhip_engine *e, iqhip_branch_end a, iqhip_branch_end b, double *rell) {
    if (!rell) return fail(IQHIP_ERR_INVALID, "null argument");
    if (e && !e->shards.empty()) return sharded::rell(e, a, b, rell);
    int rc = iqhip_rell_async(e, a, b);
    if (rc) return rc;
    rc = comm_allreduce(e, e->nboot);
    if (rc) return rc;
    rc = read_result(e, e->nboot);
    if (rc) return rc;
    memcpy(rell, e->h_result, sizeof(double) * (size_t)e->nboot);
    return IQHIP_OK;
}

// ---- branch tests (SH-aLRT, local bootstrap): the store of per-pattern log-likelihood rows and its consumers --------
// (kernels_rell.hip k_ptnlh_rows fills rows from batched tasks, kernels_alrt.hip multiplies them with the sample matrix)
int iqhip::ptnlh_plain_engine(iqhip_engine *e, const char *what) {
    if (!e) return fail(IQHIP_ERR_INVALID, std::string(what) + ": null engine");
    if (e->planner) return fail(IQHIP_ERR_INVALID, std::string(what) + ": not available on a planning-only engine");
    if (!e->shards.empty() || e->comm)
        return fail(IQHIP_ERR_UNSUPPORTED, std::string(what) + ": pattern-sharded engines keep no per-pattern store");
    return IQHIP_OK;
}

extern "C" int iqhip_ptnlh_reserve(iqhip_engine *e, int nrows) {
    int rc = ptnlh_plain_engine(e, "iqhip_ptnlh_reserve");
    if (rc) return rc;
    if (nrows < 0 || nrows > (1 << 20)) return fail(IQHIP_ERR_INVALID, "iqhip_ptnlh_reserve: bad row count");
    HIPCHK(use_device(e));
    if (nrows <= e->ptnlh_rows) return IQHIP_OK;   // (rows keep their contents while the store does not grow)
    double *grown = nullptr;
    HIPCHK(hipStreamSynchronize(e->stream));
    if (hipMalloc((void **)&grown, sizeof(double) * (size_t)nrows * e->nptn_pad) != hipSuccess)
        return fail(IQHIP_ERR_NOMEM, "iqhip_ptnlh_reserve: out of device memory");
    // (on the engine's stream: a memset on the null stream is not ordered against the kernels that fill rows next)
    HIPCHK(hipMemsetAsync(grown, 0, sizeof(double) * (size_t)nrows * e->nptn_pad, e->stream));
    if (e->d_ptnlh)
        HIPCHK(hipMemcpyAsync(grown, e->d_ptnlh, sizeof(double) * (size_t)e->ptnlh_rows * e->nptn_pad, hipMemcpyDeviceToDevice,
                              e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    if (e->d_ptnlh) HIPCHK(hipFree(e->d_ptnlh));
    e->d_ptnlh = grown;
    e->ptnlh_rows = nrows;
    return IQHIP_OK;
}

extern "C" int iqhip_ptnlh_put_current(iqhip_engine *e, int row, iqhip_branch_end a, iqhip_branch_end b) {
    int rc = ptnlh_plain_engine(e, "iqhip_ptnlh_put_current");
    if (rc) return rc;
    if (row < 0 || row >= e->ptnlh_rows) return fail(IQHIP_ERR_INVALID, "iqhip_ptnlh_put_current: row outside the store (iqhip_ptnlh_reserve)");
    HIPCHK(use_device(e));
    const int16_t *sc[2] = {nullptr, nullptr};
    const iqhip_branch_end ends[2] = {a, b};
    for (int k = 0; k < 2; k++) {
        if (ends[k].leaf >= 0) continue;
        int idx;
        rc = slab_for_key(e, ends[k].key, false, &idx);
        if (rc) return rc;
        sc[k] = e->slabs[idx].sc;
    }
    HIPCHK(launch_pattern_lh_scaled(e, sc[0], sc[1], e->d_ptnlh + (size_t)row * e->nptn_pad));
    return IQHIP_OK;
}

extern "C" int iqhip_ptnlh_fetch(iqhip_engine *e, int row, double *out) {
    int rc = ptnlh_plain_engine(e, "iqhip_ptnlh_fetch");
    if (rc) return rc;
    if (!out) return fail(IQHIP_ERR_INVALID, "iqhip_ptnlh_fetch: null argument");
    if (row < 0 || row >= e->ptnlh_rows) return fail(IQHIP_ERR_INVALID, "iqhip_ptnlh_fetch: row outside the store");
    HIPCHK(use_device(e));
    HIPCHK(hipMemcpyAsync(out, e->d_ptnlh + (size_t)row * e->nptn_pad, sizeof(double) * (size_t)e->nptn, hipMemcpyDeviceToHost,
                          e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return IQHIP_OK;
}

// the distinct rows of a row list in first-appearance order (d_bt_rows[0, M)) and, behind them, every entry's index into
// that list; the product R = L W^T of the distinct rows ends in d_bt_sums [M][nsamples]
static int ptnlh_product(iqhip_engine *e, const char *what, const int32_t *rows, int nrows, int nsamples, int *M_out) {
    if (nsamples < 1 || nsamples > e->nboot)
        return fail(IQHIP_ERR_INVALID, std::string(what) + (e->nboot == 0 ? ": no bootstrap samples (iqhip_set_boot_samples)"
                                                                          : ": more replicates than uploaded samples"));
    std::vector<int32_t> host((size_t)nrows, 0), distinct;
    std::unordered_map<int32_t, int32_t> seen;
    for (int i = 0; i < nrows; i++) {
        if (rows[i] < 0 || rows[i] >= e->ptnlh_rows) return fail(IQHIP_ERR_INVALID, std::string(what) + ": row outside the store");
        auto it = seen.find(rows[i]);
        if (it == seen.end()) {
            it = seen.emplace(rows[i], (int32_t)distinct.size()).first;
            distinct.push_back(rows[i]);
        }
        host[i] = it->second;
    }
    const int M = (int)distinct.size();
    distinct.insert(distinct.end(), host.begin(), host.end());
    HIPCHK(use_device(e));
    if (distinct.size() > e->bt_rows_cap) HIPCHK(regrow(e, &e->d_bt_rows, &e->bt_rows_cap, distinct.size(), distinct.size()));
    HIPCHK(hipStreamSynchronize(e->stream));   // (pageable source: the copy below must not outlive `distinct`)
    HIPCHK(hipMemcpyAsync(e->d_bt_rows, distinct.data(), sizeof(int32_t) * distinct.size(), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    const int ksplit = alrt_ksplit(e, M, nsamples);
    const size_t sums = (size_t)M * nsamples, part = sums * ksplit;
    if (part > e->bt_part_cap) HIPCHK(regrow(e, &e->d_bt_part, &e->bt_part_cap, part, part));
    if (sums > e->bt_sums_cap) HIPCHK(regrow(e, &e->d_bt_sums, &e->bt_sums_cap, sums, sums));
    HIPCHK(launch_alrt_product(e, e->d_bt_rows, M, nsamples, ksplit, e->d_bt_part, e->d_bt_sums));
    *M_out = M;
    return IQHIP_OK;
}

extern "C" int iqhip_ptnlh_rell(iqhip_engine *e, const int32_t *rows, int nrows, int nsamples, double *out) {
    int rc = ptnlh_plain_engine(e, "iqhip_ptnlh_rell");
    if (rc) return rc;
    if (!rows || !out || nrows < 1) return fail(IQHIP_ERR_INVALID, "iqhip_ptnlh_rell: bad row list");
    int M = 0;
    rc = ptnlh_product(e, "iqhip_ptnlh_rell", rows, nrows, nsamples, &M);
    if (rc) return rc;
    std::vector<double> sums((size_t)M * nsamples);
    HIPCHK(hipMemcpyAsync(sums.data(), e->d_bt_sums, sizeof(double) * sums.size(), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    std::unordered_map<int32_t, int> idx;
    for (int i = 0; i < nrows; i++) {
        const int k = idx.emplace(rows[i], (int)idx.size()).first->second;
        memcpy(out + (size_t)i * nsamples, sums.data() + (size_t)k * nsamples, sizeof(double) * (size_t)nsamples);
    }
    return IQHIP_OK;
}

extern "C" int iqhip_branch_tests(iqhip_engine *e, const int32_t *rows3, const double *lh3, int nbranch, int reps_sh,
                                  int reps_lbp, iqhip_branch_support *out) {
    int rc = ptnlh_plain_engine(e, "iqhip_branch_tests");
    if (rc) return rc;
    if (!rows3 || !lh3 || !out || nbranch < 1 || nbranch > (1 << 24) || reps_sh < 0 || reps_lbp < 0)
        return fail(IQHIP_ERR_INVALID, "iqhip_branch_tests: bad arguments");
    const int times = std::max(reps_sh, reps_lbp);
    int M = 0;
    rc = ptnlh_product(e, "iqhip_branch_tests", rows3, 3 * nbranch, times, &M);
    if (rc) return rc;
    const size_t need = (size_t)7 * nbranch;
    if (need > e->bt_out_cap) HIPCHK(regrow(e, &e->d_bt_out, &e->bt_out_cap, need, need));
    HIPCHK(hipStreamSynchronize(e->stream));
    HIPCHK(hipMemcpyAsync(e->d_bt_out, lh3, sizeof(double) * 3 * (size_t)nbranch, hipMemcpyHostToDevice, e->stream));
    double *d_res = e->d_bt_out + 3 * (size_t)nbranch;
    HIPCHK(launch_alrt_stats(e, e->d_bt_rows + M, e->d_bt_out, nbranch, times, e->d_bt_sums, d_res));
    static_assert(sizeof(iqhip_branch_support) == 4 * sizeof(double), "iqhip_branch_support is four doubles");
    HIPCHK(hipMemcpyAsync(out, d_res, sizeof(iqhip_branch_support) * (size_t)nbranch, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return IQHIP_OK;
}

// ---- tree topology tests (evaluateTrees / performAUTest, phylotesting.cpp:1916-2442; kernels_topo.hip) ---------------
extern "C" int iqhip_ptnlh_upload(iqhip_engine *e, int row, const double *in) {
    int rc = ptnlh_plain_engine(e, "iqhip_ptnlh_upload");
    if (rc) return rc;
    if (!in) return fail(IQHIP_ERR_INVALID, "iqhip_ptnlh_upload: null argument");
    if (row < 0 || row >= e->ptnlh_rows) return fail(IQHIP_ERR_INVALID, "iqhip_ptnlh_upload: row outside the store (iqhip_ptnlh_reserve)");
    HIPCHK(use_device(e));
    std::vector<double> tmp((size_t)e->nptn_pad, 0.0);
    memcpy(tmp.data(), in, sizeof(double) * (size_t)e->nptn);
    HIPCHK(hipStreamSynchronize(e->stream));
    HIPCHK(hipMemcpyAsync(e->d_ptnlh + (size_t)row * e->nptn_pad, tmp.data(), sizeof(double) * tmp.size(), hipMemcpyHostToDevice,
                          e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return IQHIP_OK;
}

// the int64 inclusive prefix sums of ptn_freq and nsite = their last entry, from the engine's own copy of the frequencies
static int topo_freq_prefix(iqhip_engine *e, const char *what) {
    if (e->freq_prefix_valid) return IQHIP_OK;
    if (!e->aln_set) return fail(IQHIP_ERR_INVALID, std::string(what) + ": needs iqhip_set_alignment first");
    std::vector<double> freq((size_t)e->nptn);
    HIPCHK(hipStreamSynchronize(e->stream));
    HIPCHK(hipMemcpy(freq.data(), e->d_freq, sizeof(double) * freq.size(), hipMemcpyDeviceToHost));
    std::vector<int64_t> prefix(freq.size());
    int64_t total = 0;
    for (size_t p = 0; p < freq.size(); p++) {
        const double f = freq[p];
        if (!(f >= 0.0) || f != floor(f) || f > 9007199254740992.0 || total > (INT64_MAX >> 2) - (int64_t)f)
            return fail(IQHIP_ERR_INVALID, std::string(what) + ": pattern frequencies must be non-negative integers");
        total += (int64_t)f;
        prefix[p] = total;
    }
    if (total < 1) return fail(IQHIP_ERR_INVALID, std::string(what) + ": the alignment has no site");
    if (!e->d_freq_prefix) HIPCHK(dmalloc(&e->d_freq_prefix, prefix.size()));
    HIPCHK(hipMemcpy(e->d_freq_prefix, prefix.data(), sizeof(int64_t) * prefix.size(), hipMemcpyHostToDevice));
    e->freq_nsite = total;
    e->freq_prefix_valid = true;
    return IQHIP_OK;
}

// a sample matrix of exactly (exact) or at least nsamples rows, contents undefined
static int topo_boot_rows(iqhip_engine *e, int nsamples, bool exact) {
    if (e->d_boot && (exact ? e->nboot == nsamples : e->nboot >= nsamples)) return IQHIP_OK;
    HIPCHK(hipStreamSynchronize(e->stream));
    if (e->d_boot) HIPCHK(hipFree(e->d_boot));
    e->d_boot = nullptr;
    e->nboot = 0;
    if (hipMalloc((void **)&e->d_boot, sizeof(float) * (size_t)e->nptn_pad * nsamples) != hipSuccess)
        return fail(IQHIP_ERR_NOMEM, "bootstrap sample matrix: out of device memory");
    e->nboot = nsamples;
    return IQHIP_OK;
}

static const int64_t kTopoMaxDraws = (int64_t)1 << 24;   // counts above 2^24 are not representable in float

extern "C" int iqhip_gen_boot_samples(iqhip_engine *e, int nsamples, int64_t first_replicate, int64_t ndraws, uint64_t seed,
                                      uint32_t stream) {
    int rc = ptnlh_plain_engine(e, "iqhip_gen_boot_samples");
    if (rc) return rc;
    if (nsamples < 1 || nsamples > 16384) return fail(IQHIP_ERR_INVALID, "iqhip_gen_boot_samples: 1 .. 16384 bootstrap samples");
    if (first_replicate < 0 || first_replicate > INT64_MAX - nsamples - 1)
        return fail(IQHIP_ERR_INVALID, "iqhip_gen_boot_samples: bad first replicate");
    if (ndraws < 0 || ndraws > kTopoMaxDraws)
        return fail(IQHIP_ERR_INVALID, "iqhip_gen_boot_samples: ndraws must be 0 .. 2^24 (a float holds no larger count exactly)");
    HIPCHK(use_device(e));
    rc = topo_freq_prefix(e, "iqhip_gen_boot_samples");
    if (rc) return rc;
    rc = topo_boot_rows(e, nsamples, true);
    if (rc) return rc;
    HIPCHK(launch_topo_gen(e, nsamples, first_replicate, ndraws, topo_stream_key(seed, stream)));
    HIPCHK(hipStreamSynchronize(e->stream));
    return IQHIP_OK;
}

static int topo_check_rows(iqhip_engine *e, const char *what, const int32_t *rows, int nrows) {
    for (int i = 0; i < nrows; i++)
        if (rows[i] < 0 || rows[i] >= e->ptnlh_rows) return fail(IQHIP_ERR_INVALID, std::string(what) + ": row outside the store");
    return IQHIP_OK;
}

// variances of all pairs of the row list -> host [nrows][nrows] (uses d_bt_rows for the list)
static int topo_diff_variance(iqhip_engine *e, const char *what, const int32_t *rows, int nrows, double *var) {
    int rc = topo_freq_prefix(e, what);
    if (rc) return rc;
    const size_t nn = (size_t)nrows * nrows;
    if ((size_t)nrows > e->bt_rows_cap) HIPCHK(regrow(e, &e->d_bt_rows, &e->bt_rows_cap, (size_t)nrows, (size_t)nrows));
    if (nn > e->tt_var_cap) HIPCHK(regrow(e, &e->d_tt_var, &e->tt_var_cap, nn, nn));
    HIPCHK(hipStreamSynchronize(e->stream));
    HIPCHK(hipMemcpyAsync(e->d_bt_rows, rows, sizeof(int32_t) * (size_t)nrows, hipMemcpyHostToDevice, e->stream));
    HIPCHK(launch_topo_diff_variance(e, e->d_bt_rows, nrows, e->d_tt_var));
    HIPCHK(hipMemcpyAsync(var, e->d_tt_var, sizeof(double) * nn, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return IQHIP_OK;
}

extern "C" int iqhip_ptnlh_diff_variance(iqhip_engine *e, const int32_t *rows, int nrows, double *var) {
    int rc = ptnlh_plain_engine(e, "iqhip_ptnlh_diff_variance");
    if (rc) return rc;
    if (!rows || !var || nrows < 1 || nrows > 4096) return fail(IQHIP_ERR_INVALID, "iqhip_ptnlh_diff_variance: bad row list");
    rc = topo_check_rows(e, "iqhip_ptnlh_diff_variance", rows, nrows);
    if (rc) return rc;
    HIPCHK(use_device(e));
    return topo_diff_variance(e, "iqhip_ptnlh_diff_variance", rows, nrows, var);
}

// the 95 % confidence set of phylotesting.cpp:2248-2255 / 2404-2411: trees by decreasing share until the shares pass 0.95;
// equal shares are taken highest index first (the reference's order among equal shares is its quicksort's)
static void topo_confidence_set(const std::vector<double> &share, std::vector<int32_t> &in_set) {
    const int n = (int)share.size();
    std::vector<int> rank((size_t)n);
    for (int i = 0; i < n; i++) rank[i] = i;
    std::stable_sort(rank.begin(), rank.end(), [&](int a, int b) { return share[a] < share[b]; });
    in_set.assign((size_t)n, 0);
    double prob_sum = 0.0;
    for (int k = n - 1; k >= 0; k--) {
        in_set[rank[k]] = 1;
        prob_sum += share[rank[k]];
        if (prob_sum > 0.95) break;
    }
}

extern "C" int iqhip_tree_tests(iqhip_engine *e, const int32_t *rows, const double *lh, int ntrees, int nsamples, double epsilon,
                                int weighted, uint64_t tie_seed, iqhip_tree_test *out) {
    int rc = ptnlh_plain_engine(e, "iqhip_tree_tests");
    if (rc) return rc;
    if (!rows || !lh || !out || ntrees < 2 || ntrees > 4096 || !(epsilon >= 0.0) || !std::isfinite(epsilon))
        return fail(IQHIP_ERR_INVALID, "iqhip_tree_tests: bad arguments (at least two trees)");
    if (nsamples < 1 || nsamples > e->nboot)
        return fail(IQHIP_ERR_INVALID, e->nboot == 0 ? "iqhip_tree_tests: no bootstrap samples (iqhip_gen_boot_samples / iqhip_set_boot_samples)"
                                                     : "iqhip_tree_tests: more replicates than samples in the matrix");
    for (int t = 0; t < ntrees; t++)
        if (!std::isfinite(lh[t])) return fail(IQHIP_ERR_INVALID, "iqhip_tree_tests: log-likelihoods must be finite");
    rc = topo_check_rows(e, "iqhip_tree_tests", rows, ntrees);
    if (rc) return rc;
    HIPCHK(use_device(e));
    const size_t T = (size_t)ntrees, S = (size_t)nsamples;
    // phylotesting.cpp:2284-2299, 2308: the tree every tree is compared with in the KH test
    int orig_max_id = 0, orig_2ndmax_id = -1;
    double orig_max_lh = lh[0], orig_2ndmax_lh = -DBL_MAX;
    for (int t = 1; t < ntrees; t++)
        if (orig_max_lh < lh[t]) {
            orig_max_lh = lh[t];
            orig_max_id = t;
        }
    for (int t = 0; t < ntrees; t++)
        if (t != orig_max_id && orig_2ndmax_lh < lh[t]) {
            orig_2ndmax_lh = lh[t];
            orig_2ndmax_id = t;
        }
    if (orig_2ndmax_id < 0) return fail(IQHIP_ERR_INVALID, "iqhip_tree_tests: log-likelihoods out of range");
    // host staging: doubles lh, avg, w_orig [T each] ++ weights [T][T]; ints kh_id, w_id [T each]
    std::vector<double> hd(3 * T + (weighted ? T * T : 0), 0.0);
    std::vector<int32_t> hi(2 * T, -1);
    for (int t = 0; t < ntrees; t++) {
        hd[t] = lh[t];
        hi[t] = t != orig_max_id ? orig_max_id : orig_2ndmax_id;
    }
    if (weighted) {
        // :2327-2352: weights 1 / sqrt(variance of the difference), and per tree the largest weighted difference
        std::vector<double> var(T * T);
        rc = topo_diff_variance(e, "iqhip_tree_tests", rows, ntrees, var.data());
        if (rc) return rc;
        double *w = hd.data() + 3 * T;
        for (size_t a = 0; a < T; a++)
            for (size_t b = a + 1; b < T; b++) w[a * T + b] = w[b * T + a] = 1.0 / sqrt(var[a * T + b]);
        for (int t = 0; t < ntrees; t++) {
            double worig_diff = -DBL_MAX;
            int max_id = -1;
            for (int t2 = 0; t2 < ntrees; t2++)
                if (t2 != t) {
                    const double wdiff = (lh[t2] - lh[t]) * w[(size_t)t * T + t2];
                    if (wdiff > worig_diff) {
                        worig_diff = wdiff;
                        max_id = t2;
                    }
                }
            hd[2 * T + t] = worig_diff;
            hi[T + t] = max_id;
        }
    }
    int M = 0;
    rc = ptnlh_product(e, "iqhip_tree_tests", rows, ntrees, nsamples, &M);
    if (rc) return rc;
    const size_t ndbl = hd.size() + 3 * S + 6 * T, nint = 2 * T + S;
    if (ndbl > e->tt_dbl_cap) HIPCHK(regrow(e, &e->d_tt_dbl, &e->tt_dbl_cap, ndbl, ndbl));
    if (nint > e->tt_int_cap) HIPCHK(regrow(e, &e->d_tt_int, &e->tt_int_cap, nint, nint));
    HIPCHK(hipStreamSynchronize(e->stream));
    HIPCHK(hipMemcpyAsync(e->d_tt_dbl, hd.data(), sizeof(double) * hd.size(), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(e->d_tt_int, hi.data(), sizeof(int32_t) * hi.size(), hipMemcpyHostToDevice, e->stream));
    TopoTestArgs a;
    a.sums = e->d_bt_sums;
    a.idx = e->d_bt_rows + M;
    a.T = ntrees;
    a.S = nsamples;
    a.epsilon = epsilon;
    a.tie_key = topo_stream_key(tie_seed, 0xB9u);
    a.lh = e->d_tt_dbl;
    a.avg = e->d_tt_dbl + T;
    a.w_orig = e->d_tt_dbl + 2 * T;
    a.weights = weighted ? e->d_tt_dbl + 3 * T : nullptr;
    a.max_sh = e->d_tt_dbl + hd.size();
    a.max_elw = a.max_sh + S;
    a.sum_l = a.max_elw + S;
    a.out = a.sum_l + S;
    a.kh_id = e->d_tt_int;
    a.w_id = e->d_tt_int + T;
    a.winner = e->d_tt_int + 2 * T;
    HIPCHK(launch_topo_tests(e, a));
    HIPCHK(launch_topo_tree(e, a));
    std::vector<double> res(6 * T);
    HIPCHK(hipMemcpyAsync(res.data(), a.out, sizeof(double) * res.size(), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    std::vector<double> share(T);
    std::vector<int32_t> rell_set, elw_set;
    for (size_t t = 0; t < T; t++) share[t] = res[6 * t];
    topo_confidence_set(share, rell_set);
    for (size_t t = 0; t < T; t++) share[t] = res[6 * t + 5];
    topo_confidence_set(share, elw_set);
    for (size_t t = 0; t < T; t++) {
        iqhip_tree_test &o = out[t];
        o.rell_bp = res[6 * t];
        o.kh_pvalue = res[6 * t + 1];
        o.sh_pvalue = res[6 * t + 2];
        o.wkh_pvalue = res[6 * t + 3];
        o.wsh_pvalue = res[6 * t + 4];
        o.elw_value = res[6 * t + 5];
        o.rell_confident = rell_set[t];
        o.elw_confident = elw_set[t];
    }
    return IQHIP_OK;
}

extern "C" int iqhip_multiscale_bp(iqhip_engine *e, const int32_t *rows, int ntrees, const double *scales, int nscales,
                                   int nsamples, uint64_t seed, double *bp) {
    int rc = ptnlh_plain_engine(e, "iqhip_multiscale_bp");
    if (rc) return rc;
    if (!rows || !scales || !bp || ntrees < 2 || ntrees > 4096 || nscales < 1 || nscales > 4096 || nsamples < 1)
        return fail(IQHIP_ERR_INVALID, "iqhip_multiscale_bp: bad arguments (at least two trees, one scale, one replicate)");
    rc = topo_check_rows(e, "iqhip_multiscale_bp", rows, ntrees);
    if (rc) return rc;
    HIPCHK(use_device(e));
    rc = topo_freq_prefix(e, "iqhip_multiscale_bp");
    if (rc) return rc;
    std::vector<int64_t> ndraws((size_t)nscales);
    for (int k = 0; k < nscales; k++) {
        if (!(scales[k] > 0.0) || !std::isfinite(scales[k])) return fail(IQHIP_ERR_INVALID, "iqhip_multiscale_bp: a scale must be > 0");
        const double d = round(scales[k] * (double)e->freq_nsite);
        if (d < 1.0 || d > (double)kTopoMaxDraws)
            return fail(IQHIP_ERR_INVALID, "iqhip_multiscale_bp: round(scale * nsite) must be 1 .. 2^24 draws");
        ndraws[k] = (int64_t)d;
    }
    // distinct rows in first-appearance order, then every tree's index into them (as ptnlh_product lays d_bt_rows out)
    std::vector<int32_t> list;
    std::vector<int32_t> idx((size_t)ntrees);
    {
        std::unordered_map<int32_t, int32_t> seen;
        for (int t = 0; t < ntrees; t++) {
            auto it = seen.find(rows[t]);
            if (it == seen.end()) {
                it = seen.emplace(rows[t], (int32_t)list.size()).first;
                list.push_back(rows[t]);
            }
            idx[t] = it->second;
        }
    }
    const int M = (int)list.size();
    list.insert(list.end(), idx.begin(), idx.end());
    // replicates per chunk: the sample matrix stays within 256 MB; IQHIP_BOOT_CHUNK (read per call) overrides.  The K-split
    // follows from the pattern count and the CU count alone (the budget's chunk, not this call's), so that a (row,
    // replicate) sum has the same bits whatever the chunk size
    const int64_t budget = std::max<int64_t>(1, std::min<int64_t>(16384, ((int64_t)256 << 20) / (4 * e->nptn_pad)));
    const int ksplit = alrt_ksplit(e, M, (int)budget);
    int64_t chunk = budget;
    if (const char *bc = getenv("IQHIP_BOOT_CHUNK")) chunk = std::max(1, std::min(16384, atoi(bc)));
    chunk = std::min<int64_t>(chunk, nsamples);
    rc = topo_boot_rows(e, (int)chunk, false);
    if (rc) return rc;
    const size_t sums = (size_t)M * chunk, part = sums * ksplit, ncount = (size_t)nscales * ntrees;
    if (list.size() > e->bt_rows_cap) HIPCHK(regrow(e, &e->d_bt_rows, &e->bt_rows_cap, list.size(), list.size()));
    if (part > e->bt_part_cap) HIPCHK(regrow(e, &e->d_bt_part, &e->bt_part_cap, part, part));
    if (sums > e->bt_sums_cap) HIPCHK(regrow(e, &e->d_bt_sums, &e->bt_sums_cap, sums, sums));
    if (ncount > e->tt_int_cap) HIPCHK(regrow(e, &e->d_tt_int, &e->tt_int_cap, ncount, ncount));
    HIPCHK(hipStreamSynchronize(e->stream));
    HIPCHK(hipMemcpyAsync(e->d_bt_rows, list.data(), sizeof(int32_t) * list.size(), hipMemcpyHostToDevice, e->stream));
    uint32_t *d_counts = reinterpret_cast<uint32_t *>(e->d_tt_int);
    HIPCHK(hipMemsetAsync(d_counts, 0, sizeof(uint32_t) * ncount, e->stream));
    for (int k = 0; k < nscales; k++) {
        const uint64_t key = topo_stream_key(seed, (uint32_t)k);
        for (int64_t first = 0; first < nsamples; first += chunk) {
            const int n = (int)std::min<int64_t>(chunk, nsamples - first);
            HIPCHK(launch_topo_gen(e, n, first, ndraws[k], key));
            HIPCHK(launch_alrt_product(e, e->d_bt_rows, M, n, ksplit, e->d_bt_part, e->d_bt_sums));
            HIPCHK(launch_topo_argmax(e, e->d_bt_sums, e->d_bt_rows + M, ntrees, n, d_counts + (size_t)k * ntrees));
        }
    }
    std::vector<uint32_t> counts(ncount);
    HIPCHK(hipMemcpyAsync(counts.data(), d_counts, sizeof(uint32_t) * ncount, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    for (size_t i = 0; i < ncount; i++) bp[i] = (double)counts[i] / nsamples;
    return IQHIP_OK;
}

// ---- pairwise ML distances (PhyloTree::computeDist, phylotree.cpp:2432-2541; kernels_dist.hip) -----------------------
static int pair_engine(iqhip_engine *e, const char *what) {
    if (!e) return fail(IQHIP_ERR_INVALID, std::string(what) + ": null engine");
    if (e->planner) return fail(IQHIP_ERR_INVALID, std::string(what) + ": not available on a planning-only engine");
    if (!e->shards.empty() || e->comm)
        return fail(IQHIP_ERR_UNSUPPORTED, std::string(what) + ": pattern-sharded engines are out of scope (the counts would need an all-reduce)");
    if (e->n_user != e->n || (e->n != 4 && e->n != 20 && e->n != 64))
        return fail(IQHIP_ERR_UNSUPPORTED, std::string(what) + ": 4, 20 or 64 states only (no embedded state counts)");
    if (!e->model_set || !e->aln_set)
        return fail(IQHIP_ERR_INVALID, std::string(what) + ": needs iqhip_set_model and iqhip_set_alignment first");
    if (e->nclass > 1) return fail(IQHIP_ERR_UNSUPPORTED, std::string(what) + ": mixture models are out of scope");
    return IQHIP_OK;
}

// pairs per chunk: the counts of a chunk stay within 64 MB; IQHIP_PAIR_CHUNK (read per call) overrides
static int64_t pair_chunk(const iqhip_engine *e, int64_t npairs) {
    int64_t chunk = std::max<int64_t>(1, ((int64_t)64 << 20) / (8 * (int64_t)e->n * e->n));
    if (const char *pc = getenv("IQHIP_PAIR_CHUNK")) chunk = std::max(1, atoi(pc));
    return std::max<int64_t>(1, std::min(chunk, npairs));
}

// tiles of 4 x 4 taxa for the m pairs of a chunk: pair k goes to slot k.  Pairs of one block of taxa share a tile, whatever
// their order in the list; a pair listed twice opens a new tile
static void pair_tiles(const int32_t *pairs, int64_t m, int ntaxa, std::vector<PairTile> &tiles) {
    std::unordered_map<uint64_t, size_t> open;
    for (int64_t k = 0; k < m; k++) {
        const int i = pairs[2 * k], j = pairs[2 * k + 1];
        const uint64_t key = ((uint64_t)(i >> 2) << 32) | (uint64_t)(j >> 2);
        const int cell = (i & 3) * 4 + (j & 3);
        auto it = open.find(key);
        if (it == open.end() || tiles[it->second].out[cell] >= 0) {
            PairTile t;
            for (int x = 0; x < 4; x++) {
                t.ra[x] = std::min((i & ~3) + x, ntaxa - 1);
                t.rb[x] = std::min((j & ~3) + x, ntaxa - 1);
            }
            for (int c = 0; c < 16; c++) t.out[c] = -1;
            open[key] = tiles.size();
            tiles.push_back(t);
            it = open.find(key);
        }
        tiles[it->second].out[cell] = (int32_t)k;
    }
}

extern "C" int iqhip_pair_counts(iqhip_engine *e, const int32_t *pairs, int npairs, double *counts) {
    int rc = pair_engine(e, "iqhip_pair_counts");
    if (rc) return rc;
    if (!pairs || !counts || npairs < 0) return fail(IQHIP_ERR_INVALID, "iqhip_pair_counts: bad pair list");
    for (int64_t k = 0; k < 2 * (int64_t)npairs; k++)
        if (pairs[k] < 0 || pairs[k] >= e->ntaxa) return fail(IQHIP_ERR_INVALID, "iqhip_pair_counts: pair index outside [0, ntaxa)");
    HIPCHK(use_device(e));
    const size_t nn = (size_t)e->n * e->n;
    const int64_t chunk = pair_chunk(e, npairs);
    for (int64_t first = 0; first < npairs; first += chunk) {
        const int64_t m = std::min<int64_t>(chunk, npairs - first);
        std::vector<PairTile> tiles;
        pair_tiles(pairs + 2 * first, m, e->ntaxa, tiles);
        if (tiles.size() > e->pd_tiles_cap) HIPCHK(regrow(e, &e->d_pd_tiles, &e->pd_tiles_cap, tiles.size(), tiles.size()));
        if ((size_t)m * nn > e->pd_counts_cap) HIPCHK(regrow(e, &e->d_pd_counts, &e->pd_counts_cap, (size_t)m * nn, (size_t)m * nn));
        HIPCHK(hipStreamSynchronize(e->stream));   // (pageable source: the copy must not outlive `tiles`)
        HIPCHK(hipMemcpyAsync(e->d_pd_tiles, tiles.data(), sizeof(PairTile) * tiles.size(), hipMemcpyHostToDevice, e->stream));
        HIPCHK(launch_pair_counts(e, e->d_pd_tiles, (int)tiles.size(), e->d_pd_counts));
        HIPCHK(hipMemcpyAsync(counts + (size_t)first * nn, e->d_pd_counts, sizeof(double) * (size_t)m * nn, hipMemcpyDeviceToHost,
                              e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
    }
    return IQHIP_OK;
}

extern "C" int iqhip_pair_distances(iqhip_engine *e, const double *init, double x1, double x2, double xacc, int max_steps,
                                    double *dist, double *d2l, int32_t *nsteps) {
    int rc = pair_engine(e, "iqhip_pair_distances");
    if (rc) return rc;
    if (!dist) return fail(IQHIP_ERR_INVALID, "iqhip_pair_distances: null argument");
    if (!(x1 >= 0.0) || x1 > x2 || !std::isfinite(x2) || !(xacc > 0.0) || max_steps < 1)
        return fail(IQHIP_ERR_INVALID, "iqhip_pair_distances: bad bounds / tolerance / step count (x1 <= x2, max_steps >= 1)");
    const int T = e->ntaxa, n = e->n;
    const int64_t npairs = (int64_t)T * (T - 1) / 2;
    // the pairs i < j block by block of 4 x 4 taxa, so that the pairs of a tile are neighbours in the list (and in a chunk)
    std::vector<int32_t> pairs;
    pairs.reserve((size_t)2 * npairs);
    for (int I = 0; I < T; I += 4)
        for (int J = I; J < T; J += 4)
            for (int i = I; i < std::min(I + 4, T); i++)
                for (int j = std::max(J, i + 1); j < std::min(J + 4, T); j++) {
                    pairs.push_back(i);
                    pairs.push_back(j);
                }
    std::vector<double> h_init;
    if (init) {
        h_init.resize((size_t)npairs);
        for (int64_t k = 0; k < npairs; k++) {
            const double v = init[(size_t)pairs[2 * k] * T + pairs[2 * k + 1]];
            if (!(v >= 0.0) || !std::isfinite(v)) return fail(IQHIP_ERR_INVALID, "iqhip_pair_distances: an initial distance is negative or not finite");
            h_init[(size_t)k] = v;
        }
    }
    for (size_t k = 0; k < (size_t)T * T; k++) {
        dist[k] = 0.0;
        if (d2l) d2l[k] = 0.0;
        if (nsteps) nsteps[k] = 0;
    }
    if (npairs == 0) return IQHIP_OK;
    HIPCHK(use_device(e));
    const size_t nn = (size_t)n * n, n3 = nn * n;
    const int64_t chunk = pair_chunk(e, npairs);
    // all tiles up front, chunk by chunk (a chunk's slots start at 0): the chunk loop below makes no host round trip
    std::vector<PairTile> tiles;
    std::vector<size_t> tile_first;
    for (int64_t first = 0; first < npairs; first += chunk) {
        tile_first.push_back(tiles.size());
        pair_tiles(pairs.data() + 2 * first, std::min<int64_t>(chunk, npairs - first), T, tiles);
    }
    tile_first.push_back(tiles.size());
    if (tiles.size() > e->pd_tiles_cap) HIPCHK(regrow(e, &e->d_pd_tiles, &e->pd_tiles_cap, tiles.size(), tiles.size()));
    if ((size_t)chunk * nn > e->pd_counts_cap) HIPCHK(regrow(e, &e->d_pd_counts, &e->pd_counts_cap, (size_t)chunk * nn, (size_t)chunk * nn));
    if (n3 > e->pd_coef_cap) HIPCHK(regrow(e, &e->d_pd_coef, &e->pd_coef_cap, n3, n3));
    if ((size_t)npairs > e->pd_init_cap) HIPCHK(regrow(e, &e->d_pd_init, &e->pd_init_cap, (size_t)npairs, (size_t)npairs));
    if ((size_t)4 * npairs > e->pd_out_cap) HIPCHK(regrow(e, &e->d_pd_out, &e->pd_out_cap, (size_t)4 * npairs, (size_t)4 * npairs));
    HIPCHK(hipStreamSynchronize(e->stream));
    HIPCHK(hipMemcpyAsync(e->d_pd_tiles, tiles.data(), sizeof(PairTile) * tiles.size(), hipMemcpyHostToDevice, e->stream));
    if (init) HIPCHK(hipMemcpyAsync(e->d_pd_init, h_init.data(), sizeof(double) * h_init.size(), hipMemcpyHostToDevice, e->stream));
    HIPCHK(launch_pair_coef(e, e->d_pd_coef));
    PairSolveArgs a;
    a.counts = e->d_pd_counts;
    a.coef = e->d_pd_coef;
    a.eval = e->d_eval;
    a.rates = e->d_rates;
    a.props = e->d_props;
    a.init = init ? e->d_pd_init : nullptr;
    a.out = e->d_pd_out;
    a.n = n;
    a.ncat = e->ncat;
    a.max_steps = max_steps;
    a.x1 = x1;
    a.x2 = x2;
    a.xacc = xacc;
    // iqhip_timing_enable: device time of the count and the solve launches (HIP events), summed over the chunks
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    if (e->timing)
        for (int k = 0; k < 3; k++) HIPCHK(hipEventCreate(&ev[k]));
    e->pd_counts_ms = e->pd_solve_ms = 0.0;
    int64_t first = 0;
    for (size_t c = 0; first < npairs; c++, first += chunk) {
        const int m = (int)std::min<int64_t>(chunk, npairs - first);
        a.first_pair = first;
        if (e->timing) HIPCHK(hipEventRecord(ev[0], e->stream));
        HIPCHK(launch_pair_counts(e, e->d_pd_tiles + tile_first[c], (int)(tile_first[c + 1] - tile_first[c]), e->d_pd_counts));
        if (e->timing) HIPCHK(hipEventRecord(ev[1], e->stream));
        HIPCHK(launch_pair_solve(e, a, m));
        if (e->timing) {
            HIPCHK(hipEventRecord(ev[2], e->stream));
            HIPCHK(hipEventSynchronize(ev[2]));
            float ms = 0.f;
            HIPCHK(hipEventElapsedTime(&ms, ev[0], ev[1]));
            e->pd_counts_ms += ms;
            HIPCHK(hipEventElapsedTime(&ms, ev[1], ev[2]));
            e->pd_solve_ms += ms;
        }
    }
    for (int k = 0; k < 3; k++)
        if (ev[k]) hipEventDestroy(ev[k]);
    std::vector<double> out((size_t)4 * npairs);
    HIPCHK(hipMemcpyAsync(out.data(), e->d_pd_out, sizeof(double) * out.size(), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
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

extern "C" int iqhip_debug_pair_timing(iqhip_engine *e, double *counts_ms, double *solve_ms) {
    if (!e || !e->shards.empty()) return fail(IQHIP_ERR_INVALID, "iqhip_debug_pair_timing: needs a single-device engine");
    if (counts_ms) *counts_ms = e->pd_counts_ms;
    if (solve_ms) *solve_ms = e->pd_solve_ms;
    return IQHIP_OK;
}

extern "C" int iqhip_upload_partial(iqhip_engine *e, uint64_t key, const double *partial_lh,
                                    const int16_t *scale_num) {
    if (!e || !partial_lh || !scale_num) return fail(IQHIP_ERR_INVALID, "null argument");
    if (!e->shards.empty()) return sharded::upload_partial(e, key, partial_lh, scale_num);
    HIPCHK(use_device(e));
    int idx;
    int rc = slab_for_key(e, key, true, &idx);
    if (rc) return rc;
    const int B = e->block;
    std::vector<double> tmp((size_t)e->nptn_pad * B, 0.0);
    if (e->embed2) {
        const int m = e->n_user, n = e->n;
        for (int64_t p = 0; p < e->nptn; p++)
            for (int c = 0; c < e->ncat; c++)
                for (int i = 0; i < m; i++) tmp[dev_index(e, p, c * n + i)] = partial_lh[((size_t)p * e->ncat + c) * m + i];
    } else
    for (int64_t p = 0; p < e->nptn; p++)
        for (int k = 0; k < B; k++) tmp[dev_index(e, p, k)] = partial_lh[(size_t)p * B + k];
    std::vector<int16_t> sc((size_t)e->nptn_pad, 0);
    memcpy(sc.data(), scale_num, sizeof(int16_t) * (size_t)e->nptn);
    HIPCHK(hipStreamSynchronize(e->stream));
    HIPCHK(hipMemcpy(e->slabs[idx].plh, tmp.data(), tmp.size() * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(e->slabs[idx].sc, sc.data(), sc.size() * sizeof(int16_t), hipMemcpyHostToDevice));
    return IQHIP_OK;
}

// ---------------------------------------------------------------------------------------
// timing of the dominant kernel (HIP events on the launch stream)
// ---------------------------------------------------------------------------------------
extern "C" int iqhip_timing_enable(iqhip_engine *e, int on) {
    if (!e) return fail(IQHIP_ERR_INVALID, "null engine");
    if (!e->shards.empty()) {
        for (iqhip_engine *c : e->shards) c->timing = on != 0;
        return IQHIP_OK;
    }
    e->timing = on != 0;
    return IQHIP_OK;
}

// average duration (us) of the engine's own all-reduces since the last reset, HIP events on its stream (comm.hip)
extern "C" int iqhip_timing_collective_read(iqhip_engine *e, double *avg_us, int64_t *count, int reset) {
    if (!e) return fail(IQHIP_ERR_INVALID, "null engine");
    if (!e->shards.empty()) e = e->shards[0];   // (grouped all-reduce of a single-process front: not bracketed; reads 0)
    HIPCHK(use_device(e));
    HIPCHK(hipStreamSynchronize(e->stream));
    double total = 0.0;
    for (size_t i = 0; i < e->cev_used; i++) {
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, e->cev[i].first, e->cev[i].second));
        total += ms;
    }
    if (avg_us) *avg_us = e->cev_used ? total * 1e3 / (double)e->cev_used : 0.0;
    if (count) *count = (int64_t)e->cev_used;
    if (reset) e->cev_used = 0;
    return IQHIP_OK;
}

// bytes the last submission's traversal launches ask the memory system for, from its descriptors: every result vector
// and its counters stored once; the children that are neither the previous result nor parked (streamed / second memory
// child) loaded once each; leaf state rows; the root-branch pass (its vector unless it is the previous result, ptn_freq,
// ptn_invar, _pattern_lh).  Loads of vectors written earlier in the same launch may be served by the L2 / Infinity Cache,
// so `loaded` bounds the fabric reads from above; `stored` is exact.
extern "C" int iqhip_timing_plan_bytes(iqhip_engine *e, double *stored, double *loaded) {
    if (!e) return fail(IQHIP_ERR_INVALID, "null engine");
    double st = 0.0, ld = 0.0;
    if (!e->shards.empty()) {
        for (iqhip_engine *c : e->shards) {
            double a = 0.0, b = 0.0;
            int rc = iqhip_timing_plan_bytes(c, &a, &b);
            if (rc) return rc;
            st += a; ld += b;
        }
    } else {
        const double P = (double)e->nptn_pad, V = (double)e->block * 8.0;
        // k_traverse4w takes a child that is the previous op's result from registers, within one segment: a wave starts
        // every segment (and so every launch) with nothing held, whatever op k - 1 of the array was
        const bool hands_over = e->wide4 && !e->wide4_generic && e->h_ops && e->last_nops > 0;
        std::vector<char> seg_first(hands_over ? (size_t)e->last_nops : 0, 0);
        if (hands_over) {
            const int *tab = reinterpret_cast<const int *>(e->h_ops + e->plan.table_off);
            for (int u = 0; u <= e->plan.nunits; u++)
                if (tab[2 * u + 1] > 0 && tab[2 * u] >= 0 && tab[2 * u] < e->last_nops) seg_first[tab[2 * u]] = 1;
        }
        for (int k = 0; k < e->last_nops && e->h_ops; k++) {
            const DevOp &d = e->h_ops[k];
            st += P * (V + 2.0);
            const double *held = (hands_over && k > 0 && !seg_first[k]) ? e->h_ops[k - 1].dst : nullptr;
            if (d.left_kind == CHILD_LEAF) ld += P;
            else if ((d.left_kind == CHILD_PF || d.left_kind == CHILD_LOAD) && d.pf != held) ld += P * (V + 2.0);
            if (d.right_kind == CHILD_LEAF) ld += P; else if (d.right_kind == CHILD_LOAD && d.ld != held) ld += P * (V + 2.0);
        }
        if (e->last_has_root) {
            st += P * 8.0;
            ld += P * 16.0 + (e->last_root_loads_b ? P * V : 0.0) + P;
        }
    }
    if (stored) *stored = st;
    if (loaded) *loaded = ld;
    return IQHIP_OK;
}

extern "C" int iqhip_timing_read(iqhip_engine *e, double *avg_ms, int64_t *launches, int reset) {
    if (!e) return fail(IQHIP_ERR_INVALID, "null engine");
    if (!e->shards.empty()) {  // the slowest shard's average; launches of shard 0
        double worst = 0.0;
        int64_t n0 = 0;
        for (size_t g = 0; g < e->shards.size(); g++) {
            double a = 0.0;
            int64_t n = 0;
            int rc = iqhip_timing_read(e->shards[g], &a, &n, reset);
            if (rc) return rc;
            if (a > worst) worst = a;
            if (g == 0) n0 = n;
        }
        if (avg_ms) *avg_ms = worst;
        if (launches) *launches = n0;
        return IQHIP_OK;
    }
    HIPCHK(use_device(e));
    HIPCHK(hipStreamSynchronize(e->stream));
    double total = 0.0;
    for (size_t i = 0; i < e->tev_used; i++) {
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, e->tev[i].first, e->tev[i].second));
        total += ms;
    }
    // a staged plan is two launches of the traversal kernel inside one bracket: report per launch, as a
    // profiler's per-kernel average does
    if (avg_ms) *avg_ms = e->tev_launches ? total / (double)e->tev_launches : 0.0;
    if (launches) *launches = e->tev_launches;
    if (reset) { e->tev_used = 0; e->tev_launches = 0; }
    return IQHIP_OK;
}

// ---------------------------------------------------------------------------------------
// planning-only engine (CPU tests of build_plan + check_plan; no HIP call)
// ---------------------------------------------------------------------------------------
extern "C" int iqhip_debug_create_planner(iqhip_engine **out, int nstates, int ncat, int64_t nptn, int ntaxa, int num_cus,
                                          int state_unknown, int nclass) {
    if (!out) return fail(IQHIP_ERR_INVALID, "iqhip_debug_create_planner: out == NULL");
    *out = nullptr;
    if (nptn <= 0 || ntaxa < 2 || ncat < 1 || num_cus < 1 || nclass < 1 || nclass > ncat)
        return fail(IQHIP_ERR_INVALID, "iqhip_debug_create_planner: bad shape");
    if (nstates != 4 && nstates != 20 && nstates != 64)
        return fail(IQHIP_ERR_UNSUPPORTED, "iqhip_debug_create_planner: nstates must be 4, 20 or 64");
    if (state_unknown < nstates || state_unknown > 255) return fail(IQHIP_ERR_INVALID, "state_unknown out of range");
    {
        const int rc = check_shape4("iqhip_debug_create_planner", nstates, nstates, ncat);
        if (rc) return rc;
    }
    iqhip_engine *e = new iqhip_engine();
    e->planner = true;
    e->check_plans = true;
    e->num_cus = num_cus;
    configure_engine(e, -1, nstates, nstates, ncat, nptn, ntaxa);
    const size_t P = (size_t)e->nptn_pad;
    e->d_states = fake_alloc<uint8_t>(e, (size_t)ntaxa * P);
    e->dummy.plh = fake_alloc<double>(e, P * e->block);
    e->dummy.sc = fake_alloc<int16_t>(e, P);
    e->result_cap = 8 + 16384;
    e->state_unknown = state_unknown;
    e->nclass = nclass;
    if (nclass > 1 && nstates == 4 && !e->wide4) {   // as set_model_common: a 4-state mixture runs on the matrix-core kernels
        e->mfma = true;
        e->lane_split = 1;
        e->tile = 16;
        e->ntiles = e->nptn_pad / 16;
    }
    e->mfma_pipelined = e->mfma_pipelined_ok && nclass == 1;
    e->model_set = e->aln_set = true;
    {   // cherry tables as cherry_sync_model would set them up
        const int s2 = state_unknown + 1;
        if (cherry_candidate(e) && nclass == 1 && s2 * s2 <= 4356 && (int64_t)4 * s2 * s2 <= e->nptn_pad) {
            e->cherry_s2 = s2;
            e->cherry_npairs = (int)round_up(s2 * s2, 64);
        }
    }
    *out = e;
    return IQHIP_OK;
}

// build the descriptors of one submission exactly as iqhip_update_partials would and validate them (check_plan)
extern "C" int iqhip_debug_plan(iqhip_engine *e, const iqhip_node_op *ops, int nops) {
    if (!e || !e->planner) return fail(IQHIP_ERR_INVALID, "iqhip_debug_plan needs a planning-only engine");
    if (nops < 0 || (nops > 0 && !ops)) return fail(IQHIP_ERR_INVALID, "bad ops array");
    int last_dst = -1;
    const int rc = build_plan(e, ops, nops, &last_dst, nullptr);
    if (!rc) {   // (what submit_traverse would count: iqhip_debug_cherry_tables)
        e->cherry_built_total += (int64_t)e->plan.cherry_jobs.size();
        for (int slot : e->plan.cherry_jobs) e->cherry_slots[slot].model_version = e->model_version;   // ("built")
        e->plan.cherry_jobs.clear();
        for (int k = 0; k < nops; k++) e->cherry_ops_total += e->h_ops[k].cherry != nullptr;
    }
    return rc;
}

// the shape of the last plan and of the launches it would get (tests/test_plan_check.py pins them)
extern "C" int iqhip_debug_plan_shape(iqhip_engine *e, int64_t *out, int n) {
    if (!e || !e->planner || !out || n < IQHIP_PLAN_SHAPE_NSLOTS)
        return fail(IQHIP_ERR_INVALID, "iqhip_debug_plan_shape needs a planning-only engine and IQHIP_PLAN_SHAPE_NSLOTS slots");
    std::fill(out, out + n, (int64_t)0);
    const Plan &p = e->plan;
    const int nops = p.small_nops;   // (the plan's op count, small or not)
    int chunks = 0;
    for (int k = 0; k < nops; k += e->h_ops[k].chunk_nops) chunks++;
    out[0] = lds_budget(e); out[1] = p.lds_doubles; out[2] = p.state_slots; out[3] = p.nhold; out[4] = chunks;
    out[5] = (int64_t)p.stage_units.size();
    for (size_t s = 0; s < p.stage_units.size() && s < 8; s++) out[6 + s] = p.stage_units[s];
    auto launch = [&](int64_t *o, bool top_stage, int nsegs) {
        TravLaunch L = {TRAV_NONE, false, 0, 0, 0, 0, -1};
        if (e->mfma) L = choose_traverse_mfma(e, top_stage, nsegs);
        else {   // k_traverse4 (kernels_valu4.hip launch_traverse4)
            L.variant = (TravVariant)-1;
            L.ngroups = trav4_ngroups(e);
            L.grid = L.ngroups * nsegs;
            L.lds_bytes = trav4_lds_bytes(e->block, e->wg_size, p.lds_doubles, p.state_slots);
        }
        const int64_t v[7] = {L.variant, L.tab, L.nfull, L.ngroups, L.grid, (int64_t)L.lds_bytes, L.hold_off};
        std::copy(v, v + 7, o);
    };
    launch(out + 14, true, nops > 0 ? 1 : 0);
    if (!p.stage_units.empty()) launch(out + 21, false, p.stage_units[0]);
    return IQHIP_OK;
}
