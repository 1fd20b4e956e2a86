// engine.hip -- host side of libiqhip.so: device memory, key->slab map, submissions and the
// extern "C" entry points declared in include/iqhip.h.  There is NO CPU fallback in this
// library: every compute entry point launches HIP kernels or fails with a status.
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

extern "C" void iqhip_debug_memory(int64_t *device_bytes, int64_t *host_bytes) {
    if (device_bytes) *device_bytes = g_mem_bytes[0].load();
    if (host_bytes) *host_bytes = g_mem_bytes[1].load();
}
extern "C" void iqhip_debug_fail_alloc(int nth) { g_fail_alloc_in.store(nth > 0 ? nth : 0); }

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
    e->mfma_pipelined_ok = (nstates == 20 && (ncat == 4 || ncat == 1)) || (nstates == 64 && ncat == 1);
    e->mfma_pipelined = e->mfma_pipelined_ok;
    e->tile = e->mfma ? 16 : 64;
    e->block = nstates * ncat;
    e->nptn_pad = round_up(nptn, 64);
    e->ntiles = e->nptn_pad / e->tile;

    if (const char *cp = getenv("IQHIP_CHECK_PLAN")) e->check_plans = atoi(cp) != 0;
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
    e->result_cap = 8 + 16384;  // up to 16384 node updates per submission
    const size_t nposts = (size_t)2 * kNewtonPostEpochs * (2 * e->num_cus) * 2;
    // default result buffer: pinned host memory mapped into the device address space -- the
    // reduction kernel writes the handful of result doubles straight to the host (no D2H copy
    // on the critical path); a caller-bound device buffer (RCCL) replaces it
    const bool ok = e->d_states.ensure(e, (size_t)ntaxa * P) == hipSuccess && e->d_freq.ensure(e, P) == hipSuccess &&
                    e->d_invar.ensure(e, P) == hipSuccess && e->d_theta.ensure(e, P * e->block) == hipSuccess &&
                    e->d_pattern_lh.ensure(e, P) == hipSuccess &&
                    e->h_result.ensure(e, (size_t)e->result_cap, true) == hipSuccess &&
                    hipHostGetDevicePointer((void **)&e->d_result_own, e->h_result.p, 0) == hipSuccess &&
                    e->h_done.ensure(e, 8, true) == hipSuccess &&
                    hipHostGetDevicePointer((void **)&e->d_done, (void *)e->h_done.p, 0) == hipSuccess &&
                    hipEventCreateWithFlags(&e->staging_free, hipEventDisableTiming) == hipSuccess &&
                    e->dummy.plh.ensure(e, P * e->block) == hipSuccess && e->dummy.sc.ensure(e, P) == hipSuccess &&
                    e->d_newton_partials.ensure(e, (size_t)4 * e->num_cus) == hipSuccess &&
                    e->d_newton_barrier.ensure(e, 2) == hipSuccess && e->d_fold_ticket.ensure(e, 4) == hipSuccess &&
                    e->d_newton_posts.ensure(e, nposts) == hipSuccess &&
                    e->d_fold_flags.ensure(e, (size_t)e->result_cap) == hipSuccess;
    if (!ok) {   // (nothing has been enqueued on the half-built engine)
        iqhip_destroy(e);
        return fail(IQHIP_ERR_NOMEM, "iqhip_create: device allocation failed");
    }
    hipMemsetAsync(e->dummy.plh.p, 0, P * e->block * sizeof(double), e->stream);
    hipMemsetAsync(e->dummy.sc.p, 0, P * sizeof(int16_t), e->stream);
    hipMemsetAsync(e->d_newton_barrier.p, 0, 2 * sizeof(unsigned int), e->stream);
    hipMemsetAsync(e->d_newton_posts.p, 0xFF, nposts * sizeof(double), e->stream);
    hipMemsetAsync(e->d_fold_ticket.p, 0, 4 * sizeof(unsigned int), e->stream);
    hipMemsetAsync(e->d_fold_flags.p, 0, (size_t)e->result_cap * sizeof(int), e->stream);
    e->d_result = e->d_result_own;
    hipMemsetAsync(e->d_theta.p, 0, P * e->block * sizeof(double), e->stream);
    hipMemsetAsync(e->d_pattern_lh.p, 0, P * sizeof(double), e->stream);
    memset(e->h_result.p, 0, e->result_cap * sizeof(double));
    *e->h_done.p = 0;
    hipStreamSynchronize(e->stream);
    *out = e;
    return IQHIP_OK;
}

// (every DevBuf and PinBuf of the engine, its slabs included, frees itself when the engine is deleted: the device is
// current and the stream drained by then; a sharded front and a planning-only engine have no device and no stream)
extern "C" void iqhip_destroy(iqhip_engine *e) {
    if (!e) return;
    if (!e->shards.empty()) sharded::destroy(e);
    use_device(e);
    if (e->stream) hipStreamSynchronize(e->stream);
    if (e->pair) iqhip_destroy(e->pair);   // (runs on this engine's stream, which it does not own)
    e->pair = nullptr;
    comm_destroy(e);
    if (e->stream) hipStreamSynchronize(e->stream);
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
    if (s.plh.ensure(e, P * e->block) != hipSuccess || s.sc.ensure(e, P) != hipSuccess) return fail(IQHIP_ERR_NOMEM, "slab alloc");
    if (!e->planner) {   // padded lanes must hold finite values from the start
        hipMemsetAsync(s.plh.p, 0, P * e->block * sizeof(double), e->stream);
        hipMemsetAsync(s.sc.p, 0, P * sizeof(int16_t), e->stream);
    }
    e->slabs.push_back(std::move(s));
    *idx = (int)e->slabs.size() - 1;
    return IQHIP_OK;
}

int iqhip::slab_for_key(iqhip_engine *e, uint64_t key, bool create, int *idx) {
    auto it = e->key2slab.find(key);
    if (it != e->key2slab.end()) {
        *idx = it->second;
        Slab &s = e->slabs[*idx];
        if (s.virt && !create && !e->planner) {   // a reader: the pair table becomes the vector it stands for
            HIPCHK(launch_pair_expand(e, s));
            e->pair_slabs_expanded++;
        }
        s.virt = false;   // (create: about to be overwritten)
        return IQHIP_OK;
    }
    if (!create) return fail(IQHIP_ERR_INVALID, "unknown partial_lh key (vector never computed)");
    int rc = new_slab(e, idx);
    if (rc) return rc;
    e->key2slab[key] = *idx;
    e->keymap_version++;
    return IQHIP_OK;
}

int iqhip::expand_virtual_slabs(iqhip_engine *e) {
    if (e->planner) return IQHIP_OK;
    for (Slab &s : e->slabs) {
        if (!s.virt) continue;
        HIPCHK(use_device(e));
        HIPCHK(launch_pair_expand(e, s));
        e->pair_slabs_expanded++;
        s.virt = false;
    }
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
    e->slabs[it->second].virt = false;
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
    HIPCHK(hipMemcpyAsync(e->d_freq.p, tmp.data(), tmp.size() * sizeof(double), hipMemcpyHostToDevice,
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
    HIPCHK(hipMemcpyAsync(e->d_invar.p, tmp.data(), tmp.size() * sizeof(double),
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
    {   // vectors that exist as pair tables only are those of the old alignment
        const int rc = expand_virtual_slabs(e);
        if (rc) return rc;
    }
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
    HIPCHK(hipMemcpyAsync(e->d_states.p, tmp.data(), tmp.size(), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    // pair children (plan.hip select_pair_children): which rows hold nothing but states 0 .. 3 and STATE_UNKNOWN; the code rows
    // and the descriptors that point at them belong to the old alignment
    e->taxon_plain.assign((size_t)e->ntaxa, 1);
    for (int t = 0; t < e->ntaxa; t++)
        for (size_t p = 0; p < P; p++) {
            const uint8_t st = tmp[(size_t)t * P + p];
            if (st >= 4 && st != (uint8_t)e->state_unknown) { e->taxon_plain[t] = 0; break; }
        }
    e->pair_row_of.clear();
    e->plan_cache.invalidate();
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
    if (e->model_set) {   // vectors that exist as pair tables only are those of the model that is about to go
        HIPCHK(use_device(e));
        const int rc = expand_virtual_slabs(e);
        if (rc) return rc;
    }
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
            HIPCHK(hipMemsetAsync(e->d_newton_posts.p, 0xFF, (size_t)2 * kNewtonPostEpochs * (2 * e->num_cus) * 2 * sizeof(double), e->stream));
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
    HIPCHK(e->d_model.ensure(e, total));
    double *const d_model = e->d_model.p;
    HIPCHK(hipMemcpy(d_model, blk.data(), sizeof(double) * total, hipMemcpyHostToDevice));
    e->d_eval = d_model + o_eval;
    e->d_evec = d_model + o_evec;
    e->d_inv_evec = d_model + o_ievec;
    e->d_rates = d_model + o_rates;
    e->d_props = d_model + o_props;
    e->d_tip = d_model + o_tip;
    e->d_evalc = d_model + o_evalc;
    e->d_tipc = d_model + o_tipc;
    e->d_cls = reinterpret_cast<int *>(d_model + o_cls);
    e->d_aimg = aimg_doubles ? d_model + o_aimg : nullptr;
    e->aimg_doubles = (int)aimg_doubles;
    if (nclass > 1 || (e->n == 20 && !e->mfma_pipelined_ok) || e->wide4) {  // (20 states with a category count that has no
        // pipelined instantiation also run on the mixture kernel: one class; wide DNA reads the generic images, one class too)
        // MFMA A-operand images of every class for k_traverse_mfma_mix20: [class][U16 | U4 | Ui16 | Ui4][s][lane]
        // (16-row tile: row = lane & 15; 4-row tail: row = 16 + (lane & 3); k = 4s + (lane >> 4)), followed by
        // the padded two-tile images [class][U | U^-1][m][s][lane] of the generic kernel (64-state mixtures, wide DNA)
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
        HIPCHK(e->d_img.ensure(e, img.size()));
        HIPCHK(hipMemcpy(e->d_img.p, img.data(), sizeof(double) * img.size(), hipMemcpyHostToDevice));
    }
    // the pipelined kernels hold one eigen-system in registers / LDS: mixtures take the generic kernel,
    // whose plans have a different canonical form -> drop the cached descriptors
    const bool pipelined = e->mfma_pipelined_ok && nclass == 1;
    if (pipelined != e->mfma_pipelined || nclass != e->nclass) {
        e->mfma_pipelined = pipelined;
        e->plan_cache.invalidate();
    }
    e->h_props.assign(props, props + e->ncat);   // (iqhip_em_objective checks the weights it divides by)
    e->h_cls = cls;                              // (iqhip_mix_class_lh builds the per-class component lists from it)
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
    if (!e || !e->cherry_on || !e->shards.empty()) return false;   // (a planning-only engine plans them too)
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
        e->pair->fill_image.on = false;
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
    if (!rc) e->mixture_api = false;
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
    const int rc = set_model_common(e, nclass, cat_class, eval, evec, inv_evec, rates, props, state_unknown, tip_partial_lh);
    if (!rc) e->mixture_api = true;   // (iqhip_class_lnl: a mixture engine, even with one class)
    return rc;
}

// ---------------------------------------------------------------------------------------
// submissions (the descriptors come from the planner, plan.hip)
// ---------------------------------------------------------------------------------------
int iqhip::ensure_slab_rows(iqhip_engine *e, int nrows) {
    HIPCHK(e->d_slab.ensure(e, (size_t)nrows * e->ntiles * e->lane_split));
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

int iqhip::require(iqhip_engine *e, const char *what, unsigned needs) {
    const auto no = [what](int code, const char *why) { return fail(code, std::string(what) + ": " + why); };
    if (!e) return no(IQHIP_ERR_INVALID, "null engine");
    if (e->planner) return no(IQHIP_ERR_INVALID, "not available on a planning-only engine");
    if ((needs & REQ_SINGLE_DEVICE) && (!e->shards.empty() || e->comm))
        return no(IQHIP_ERR_UNSUPPORTED, "not available on pattern-sharded engines");
    if ((needs & REQ_NO_ASC) && (e->asc_active || e->n_unobs > 0))
        return no(IQHIP_ERR_UNSUPPORTED, "not available with ascertainment bias correction (+ASC)");
    const bool only4 = needs & REQ_STATES_4;
    if ((needs & REQ_PLAIN_STATES) && (e->embed2 || e->n_user != e->n))
        return no(IQHIP_ERR_UNSUPPORTED, only4 ? "not available for embedded state counts (4 states only)"
                                               : "not available for embedded state counts (4, 20 or 64 states only)");
    if ((needs & REQ_STATES_4_20_64) && e->n != 4 && e->n != 20 && e->n != 64) return no(IQHIP_ERR_UNSUPPORTED, "4, 20 or 64 states only");
    if (only4 && e->n != 4) return no(IQHIP_ERR_UNSUPPORTED, "4 states only");
    if ((needs & REQ_NO_MIXTURE) && e->nclass > 1) return no(IQHIP_ERR_UNSUPPORTED, "not available for mixture models");
    if ((needs & REQ_MIXTURE) && e->nclass < 2) return no(IQHIP_ERR_UNSUPPORTED, "the model is no mixture (one class)");
    if ((needs & REQ_MODEL_ALN) && (!e->model_set || !e->aln_set))
        return no(IQHIP_ERR_INVALID, "needs iqhip_set_model and iqhip_set_alignment first");
    if ((needs & REQ_THETA) && !e->theta_valid) return no(IQHIP_ERR_INVALID, "needs iqhip_compute_theta first");
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
        src[i] = p->slabs[idx].plh.p;
        dst[i] = e->d_cherry_tab.p + (size_t)e->plan.cherry_jobs[i] * per;
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
    e->n_root_end_keys = 0;
    if (has_root) {
        if (a.leaf < 0) e->root_end_keys[e->n_root_end_keys++] = a.key;
        if (b.leaf < 0) e->root_end_keys[e->n_root_end_keys++] = b.key;
    }
    rc = build_plan(e, ops, nops, &last_dst, explicit_segs, len_ptrs);
    e->n_root_end_keys = 0;
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
            HIPCHK(launch_leaf_tables(e, reinterpret_cast<const TabJob *>(e->d_ops.p + e->plan.jobs_off), njobs));
        e->plan.tab_dirty = 0;  // built; the same (cached) plan needs nothing until a length or the model changes
    }
    if (!e->plan.cherry_jobs.empty()) {
        rc = build_cherry_tables(e);
        if (rc) return rc;
    }
    if (e->plan.uses_cherry)
        for (int k = 0; k < nops; k++) e->cherry_ops_total += e->h_ops.p[k].cherry != nullptr;
    timing_begin(e);
    rc = fill_image_submission(e);   // (k_traverse4: the producer's launch, when the cached plan's image is stale; inside the timed span)
    if (rc) return rc;
    const int *table = reinterpret_cast<const int *>(e->d_ops.p + e->plan.table_off);
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
    const bool fold4 = e->fold_reduce && !e->mfma && !empty_top && !skip_reduce;
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
        HIPCHK(hipMemcpyAsync(e->h_result.p, e->d_result, sizeof(double) * ndoubles, hipMemcpyDeviceToHost,
                              e->stream));
    else if (e->poll_pending) {
        // the last kernel of the submission is a k_reduce that publishes a sequence number in mapped host memory:
        // spinning on it sees the result a few microseconds before a stream synchronisation returns.  Bounded: long
        // kernels fall through to the ordinary wait.
        e->poll_pending = false;
        const unsigned long long want = e->result_seq;
        for (int spin = 0; spin < 200000; spin++) {
            if (*e->h_done.p == want) {
                std::atomic_thread_fence(std::memory_order_acquire);
                e->staging_busy = false;  // (in-order stream: the plan upload finished long before k_reduce)
                if (e->folded_rows >= 0) {   // folded reduction: unflagged sum_scale rows were not written (fold_tail)
                    if (e->h_result.p[2 + e->folded_rows] == 0.0)
                        for (int k = 0; k < e->folded_rows; k++) e->h_result.p[2 + k] = 0.0;
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
        if (e->h_result.p[2 + e->folded_rows] == 0.0)
            for (int k = 0; k < e->folded_rows; k++) e->h_result.p[2 + k] = 0.0;
        e->folded_rows = -1;
    }
    return IQHIP_OK;
}

void iqhip::result_arrived(iqhip_engine *e) {
    e->poll_pending = false;
    e->staging_busy = false;
    if (e->folded_rows >= 0) {
        if (e->h_result.p[2 + e->folded_rows] == 0.0)
            for (int k = 0; k < e->folded_rows; k++) e->h_result.p[2 + k] = 0.0;
        e->folded_rows = -1;
    }
}

// the NaN/Inf repair of phylokernel.h:848-866 / :1100-1122, done on the (rare) slow path
static int repair_lnl(iqhip_engine *e, double *lnl) {
    std::vector<double> plh((size_t)e->nptn_pad), freq((size_t)e->nptn_pad);
    HIPCHK(hipMemcpy(plh.data(), e->d_pattern_lh.p, sizeof(double) * plh.size(), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(freq.data(), e->d_freq.p, sizeof(double) * freq.size(), hipMemcpyDeviceToHost));
    double s = 0.0;
    for (int64_t p = 0; p < e->nptn; p++) {
        if (isnan(plh[p]) || isinf(plh[p])) plh[p] = kLogScalingThreshold * 4;
        s += plh[p] * freq[p];
    }
    HIPCHK(hipMemcpy(e->d_pattern_lh.p, plh.data(), sizeof(double) * plh.size(), hipMemcpyHostToDevice));
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
    const int rc = asc_log_term(e->h_result.p[1], &lp);
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
    *lnl = e->h_result.p[0];
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
        for (int k = 0; k < nops; k++) sum_scale[k] = e->h_result.p[2 + k];
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
        for (int k = 0; k < nops; k++) sum_scale[k] = e->h_result.p[2 + k];
    double v = e->h_result.p[0];
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

void iqhip::set_theta_branch(iqhip_engine *e, const DevBranch &br, iqhip_branch_end a, iqhip_branch_end b) {
    e->theta_valid = true;
    e->theta_a_sc = br.a_sc;
    e->theta_b_sc = br.b_sc;
    if (b.leaf >= 0) std::swap(a, b);   // (build_branch's order)
    e->theta_end[0] = a;
    e->theta_end[1] = b;
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
    set_theta_branch(e, br, a, b);
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
        if (e->d_result == e->d_result_own) e->h_result.p[2] = e->h_result.p[3] = e->h_result.p[4] = 0.0;
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
    double a = e->h_result.p[0], b = e->h_result.p[1];
    newton_repair(a, b);                                                            // phylokernel.h:647-651
    if (e->asc_active) asc_derv_correct(e->h_result.p + 2, e->asc_nsites, a, b);   // phylokernel.h:719-724
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

extern "C" int iqhip_debug_pair_children(iqhip_engine *e, int64_t *ops_removed, int64_t *slabs_expanded, int64_t *last_plan_removed) {
    if (!e) return fail(IQHIP_ERR_INVALID, "null engine");
    if (!e->shards.empty()) e = e->shards[0];
    if (ops_removed) *ops_removed = e->pair_ops_removed;
    if (slabs_expanded) *slabs_expanded = e->pair_slabs_expanded;
    if (last_plan_removed) *last_plan_removed = (int64_t)e->plan.virt.size();
    return IQHIP_OK;
}

// the pair-code row table (plan.hip select_pair_children, pair_code_row); a planning-only engine counts the same way
extern "C" int iqhip_debug_pair_rows(iqhip_engine *e, int64_t *slots_in_use, int64_t *restarts, int64_t *kept_real_for_lack_of_a_row) {
    if (!e) return fail(IQHIP_ERR_INVALID, "null engine");
    if (!e->shards.empty()) e = e->shards[0];
    if (slots_in_use) *slots_in_use = (int64_t)e->pair_row_of.size();
    if (restarts) *restarts = e->pair_row_restarts;
    if (kept_real_for_lack_of_a_row) *kept_real_for_lack_of_a_row = e->pair_ops_without_row;
    return IQHIP_OK;
}

// k_traverse4's fill image (plan.hip fill_image_submission): submissions that launched the producer (a planning-only engine:
// that would have), submissions that copied an image already there, bytes of the current plan's image (0: it can have none)
extern "C" int iqhip_debug_fill_image(iqhip_engine *e, int64_t *built, int64_t *reused, int64_t *bytes) {
    if (!e) return fail(IQHIP_ERR_INVALID, "null engine");
    if (!e->shards.empty()) e = e->shards[0];
    if (built) *built = e->fill_image.built;
    if (reused) *reused = e->fill_image.reused;
    if (bytes) *bytes = (e->plan.image_ok && !e->plan.small) ? e->plan.image_doubles * (int64_t)sizeof(double) : 0;
    return IQHIP_OK;
}

// planning-only engines have no alignment: say which taxa hold plain states only (nullptr: none known, nothing is virtualised)
extern "C" int iqhip_debug_planner_plain_taxa(iqhip_engine *e, const uint8_t *plain) {
    if (!e || !e->planner) return fail(IQHIP_ERR_INVALID, "iqhip_debug_planner_plain_taxa needs a planning-only engine");
    e->taxon_plain.clear();
    if (plain) e->taxon_plain.assign(plain, plain + e->ntaxa);
    e->plan_cache.invalidate();
    return IQHIP_OK;
}

// what the last plan removed: out[k] = 1 when row k of the caller's op list was answered by a pair child
extern "C" int iqhip_debug_plan_removed(iqhip_engine *e, int32_t *out, int nrows) {
    if (!e || !e->planner || !out || nrows != e->plan.nrows)
        return fail(IQHIP_ERR_INVALID, "iqhip_debug_plan_removed needs a planning-only engine and the last plan's row count");
    std::fill(out, out + nrows, 1);
    for (int k = 0; k < e->plan.small_nops; k++) out[e->h_ops.p[k].out_row] = 0;
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
    double v = e->h_result.p[0];
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
    memcpy(out, e->h_result.p, sizeof(double) * ndoubles);
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
    return fetch_vec(e, e->slabs[idx].plh.p, out);
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
    HIPCHK(hipMemcpy(e->slabs[idx].plh.p, tmp.data(), tmp.size() * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(e->slabs[idx].sc.p, sc.data(), sc.size() * sizeof(int16_t), hipMemcpyHostToDevice));
    return IQHIP_OK;
}

extern "C" int iqhip_fetch_theta(iqhip_engine *e, double *out) {
    if (!e || !out) return fail(IQHIP_ERR_INVALID, "null argument");
    if (!e->shards.empty()) return sharded::fetch_vec(e, 0, true, out);
    HIPCHK(use_device(e));
    return fetch_vec(e, e->d_theta.p, out);
}

extern "C" int iqhip_fetch_scale_num(iqhip_engine *e, uint64_t key, int16_t *out) {
    if (!e || !out) return fail(IQHIP_ERR_INVALID, "null argument");
    if (!e->shards.empty()) return sharded::fetch_scale_num(e, key, out);
    HIPCHK(use_device(e));
    int idx;
    int rc = slab_for_key(e, key, false, &idx);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(e->stream));
    HIPCHK(hipMemcpy(out, e->slabs[idx].sc.p, sizeof(int16_t) * (size_t)e->nptn, hipMemcpyDeviceToHost));
    return IQHIP_OK;
}

extern "C" int iqhip_fetch_pattern_lh(iqhip_engine *e, double *out) {
    if (!e || !out) return fail(IQHIP_ERR_INVALID, "null argument");
    if (!e->shards.empty()) return sharded::fetch_pattern_lh(e, out, 0, iqhip_branch_end{0, -1, 0}, iqhip_branch_end{0, -1, 0});
    HIPCHK(use_device(e));
    HIPCHK(hipStreamSynchronize(e->stream));
    HIPCHK(hipMemcpy(out, e->d_pattern_lh.p, sizeof(double) * (size_t)e->nptn, hipMemcpyDeviceToHost));
    if (e->asc_active) {  // phylokernel.h:1013-1014: observed patterns only
        const int64_t nobs = e->nptn - e->n_unobs;
        for (int64_t p = 0; p < nobs; p++) out[p] -= e->pattern_lh_shift;
        for (int64_t p = nobs; p < e->nptn; p++) out[p] = 0.0;
    }
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
        const bool hands_over = e->wide4 && !e->wide4_generic && e->h_ops.p && e->last_nops > 0;
        std::vector<char> seg_first(hands_over ? (size_t)e->last_nops : 0, 0);
        if (hands_over) {
            const int *tab = reinterpret_cast<const int *>(e->h_ops.p + e->plan.table_off);
            for (int u = 0; u <= e->plan.nunits; u++)
                if (tab[2 * u + 1] > 0 && tab[2 * u] >= 0 && tab[2 * u] < e->last_nops) seg_first[tab[2 * u]] = 1;
        }
        // (k_traverse4: the ops that pair children replaced are not in the descriptors -- nothing stored, and their consumers
        // read one code byte per pattern)
        const int ndev = (!e->mfma && e->last_nops > 0) ? e->plan.small_nops : e->last_nops;
        for (int k = 0; k < ndev && e->h_ops.p; k++) {
            const DevOp &d = e->h_ops.p[k];
            st += P * (V + 2.0);
            ld += P * ((d.left_kind == CHILD_PAIR) + (d.right_kind == CHILD_PAIR));
            const double *held = (hands_over && k > 0 && !seg_first[k]) ? e->h_ops.p[k - 1].dst : nullptr;
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
    e->d_states.ensure(e, (size_t)ntaxa * P);   // (fake addresses: these cannot fail)
    e->dummy.plh.ensure(e, P * e->block);
    e->dummy.sc.ensure(e, P);
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
    return iqhip_debug_plan_submit(e, ops, nops, nullptr, 0, 0);
}

// ... with explicit segments (nsegs > 0) or with every length on the device (device_lengths: the pointers are fake addresses)
extern "C" int iqhip_debug_plan_submit(iqhip_engine *e, const iqhip_node_op *ops, int nops, const int32_t *segs, int nsegs,
                                       int device_lengths) {
    if (!e || !e->planner) return fail(IQHIP_ERR_INVALID, "iqhip_debug_plan_submit needs a planning-only engine");
    if (nops < 0 || (nops > 0 && !ops) || nsegs < 0 || (nsegs > 0 && !segs)) return fail(IQHIP_ERR_INVALID, "bad ops array");
    int last_dst = -1;
    const std::vector<int> seg_list(segs, segs + nsegs);
    std::vector<const double *> lp;
    if (device_lengths) lp.assign((size_t)2 * nops, e->dummy.plh.p);
    int rc = build_plan(e, ops, nops, &last_dst, nsegs > 0 ? &seg_list : nullptr, device_lengths ? lp.data() : nullptr);
    if (!rc) rc = fill_image_submission(e);
    if (!rc) {   // (what submit_traverse would count: iqhip_debug_cherry_tables)
        e->cherry_built_total += (int64_t)e->plan.cherry_jobs.size();
        for (int slot : e->plan.cherry_jobs) e->cherry_slots[slot].model_version = e->model_version;   // ("built")
        e->plan.cherry_jobs.clear();
        for (int k = 0; k < nops; k++) e->cherry_ops_total += e->h_ops.p[k].cherry != nullptr;
    }
    return rc;
}

// what the engine's state goes through between submissions, on a planning-only engine: 0 iqhip_set_model, 1 iqhip_set_alignment
extern "C" int iqhip_debug_planner_event(iqhip_engine *e, int what) {
    if (!e || !e->planner || what < 0 || what > 1) return fail(IQHIP_ERR_INVALID, "iqhip_debug_planner_event needs a planning-only engine and event 0 or 1");
    if (what == 0) e->model_version++;
    else { e->pair_row_of.clear(); e->plan_cache.invalidate(); }
    return IQHIP_OK;
}

// the fill image of the last plan, chunk by chunk: out[2 i] = byte offset, out[2 i + 1] = byte extent of chunk i; returns through
// *nchunks how many there are (at most `cap` pairs are written)
extern "C" int iqhip_debug_fill_image_chunks(iqhip_engine *e, int64_t *out, int cap, int *nchunks) {
    if (!e || !e->planner || !nchunks || (cap > 0 && !out)) return fail(IQHIP_ERR_INVALID, "iqhip_debug_fill_image_chunks needs a planning-only engine");
    int n = 0;
    for (int k = 0; k < e->plan.small_nops && !e->mfma; k += e->h_ops.p[k].chunk_nops, n++) {
        int regs = 0;
        for (int q = k; q < k + e->h_ops.p[k].chunk_nops; q++) {
            const DevOp &d = e->h_ops.p[q];
            regs = std::max(regs, std::max(d.lds_left + child_region_blocks(d.left_kind) * e->block,
                                           d.lds_right + child_region_blocks(d.right_kind) * e->block));
        }
        if (n < cap) { out[2 * n] = (int64_t)e->h_ops.p[k].image_off * 8; out[2 * n + 1] = (int64_t)regs * 8; }
    }
    *nchunks = n;
    return IQHIP_OK;
}

// the shape of the last plan and of the launches it would get (tests/test_plan_check.py pins them)
extern "C" int iqhip_debug_plan_shape(iqhip_engine *e, int64_t *out, int n) {
    if (!e || !e->planner || !out || n < IQHIP_PLAN_SHAPE_NSLOTS)
        return fail(IQHIP_ERR_INVALID, "iqhip_debug_plan_shape needs a planning-only engine and IQHIP_PLAN_SHAPE_NSLOTS slots");
    std::fill(out, out + n, (int64_t)0);
    const Plan &p = e->plan;
    const int nops = p.small_nops;   // (the plan's op count, small or not)
    int chunks = 0;
    for (int k = 0; k < nops; k += e->h_ops.p[k].chunk_nops) chunks++;
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
            L.lds_bytes = trav4_lds_bytes(e->block, p.lds_doubles, p.state_slots);
        }
        const int64_t v[7] = {L.variant, L.tab, L.nfull, L.ngroups, L.grid, (int64_t)L.lds_bytes, L.hold_off};
        std::copy(v, v + 7, o);
    };
    launch(out + 14, true, nops > 0 ? 1 : 0);
    if (!p.stage_units.empty()) launch(out + 21, false, p.stage_units[0]);
    return IQHIP_OK;
}

// the LDS layout of the last plan, op by op (tests/test_fill_states_plan.py)
extern "C" int iqhip_debug_plan_layout(iqhip_engine *e, int32_t *out, int nops) {
    if (!e || !e->planner || !out || nops != e->plan.small_nops)
        return fail(IQHIP_ERR_INVALID, "iqhip_debug_plan_layout needs a planning-only engine and the last plan's op count");
    for (int k = 0; k < nops; k++) {
        const DevOp &d = e->h_ops.p[k];
        const int32_t v[IQHIP_PLAN_LAYOUT_NSLOTS] = {d.chunk_nops, d.chunk_slots, d.left_kind == CHILD_LEAF, d.right_kind == CHILD_LEAF,
                                                     d.lds_left, d.lds_right, d.sl_slot, d.sr_slot};
        std::copy(v, v + IQHIP_PLAN_LAYOUT_NSLOTS, out + (size_t)k * IQHIP_PLAN_LAYOUT_NSLOTS);
    }
    return IQHIP_OK;
}
