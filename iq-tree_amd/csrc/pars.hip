// pars.hip -- host side of the Fitch parsimony calls (include/iqhip.h "Fitch parsimony"; kernels in kernels_pars.hip):
// the site layout and the state masks of iqhip_pars_init, the validation and level assignment of an op list (in the spirit
// of check_plan: everything is checked before anything is launched), and the launches.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "iqhip_internal.h"
#include "pars_spr_check.h"

using namespace iqhip;

// Validation of an op list and its levels.  valid: one flag per caller slot (NULL: none written yet).  level: nops entries
// or NULL.  Returns an empty string or what is wrong.
static std::string pars_levels(int ntaxa, int nvectors, const uint8_t *valid, const iqhip_pars_op *ops, int nops,
                               int32_t *level) {
    if (ntaxa < 1 || nvectors < 0) return "bad slot counts";
    if (nops < 0 || (nops > 0 && !ops)) return "bad op list";
    const int64_t nslots = (int64_t)ntaxa + nvectors;
    // per slot: the op of this call that writes it (-1: none), and whether an op of this call has read it so far
    std::vector<int32_t> writer((size_t)nslots, -1);
    std::vector<uint8_t> was_read((size_t)nslots, 0);
    std::vector<int32_t> lev((size_t)nops, 0);
    auto op_name = [](int k) { return "op " + std::to_string(k); };
    for (int k = 0; k < nops; k++) {
        const iqhip_pars_op &o = ops[k];
        const int32_t ch[2] = {o.left, o.right};
        if (o.dst < 0 || o.dst >= nslots || o.left < 0 || o.left >= nslots || o.right < 0 || o.right >= nslots)
            return op_name(k) + ": slot outside [0, ntaxa + nvectors)";
        if (o.dst < ntaxa) return op_name(k) + ": dst is a tip slot";
        if (o.dst == o.left || o.dst == o.right) return op_name(k) + ": dst is one of its own children";
        if (writer[(size_t)o.dst] >= 0) return op_name(k) + ": slot " + std::to_string(o.dst) + " is written twice in one call";
        if (was_read[(size_t)o.dst])
            return op_name(k) + ": slot " + std::to_string(o.dst) + " is read by an earlier op of this call";
        int l = 0;
        for (int c : ch) {
            if (c >= ntaxa) {
                if (writer[(size_t)c] >= 0) l = std::max(l, lev[(size_t)writer[(size_t)c]] + 1);
                else if (!(valid && valid[c - ntaxa]))
                    return op_name(k) + ": slot " + std::to_string(c) + " is read before anything has written it";
            }
            was_read[(size_t)c] = 1;
        }
        writer[(size_t)o.dst] = k;
        lev[(size_t)k] = l;
    }
    if (level) std::copy(lev.begin(), lev.end(), level);
    return std::string();
}

extern "C" int iqhip_debug_pars_levels(int ntaxa, int nvectors, const uint8_t *valid, const iqhip_pars_op *ops, int nops,
                                       int32_t *level) {
    const std::string err = pars_levels(ntaxa, nvectors, valid, ops, nops, level);
    if (!err.empty()) return fail(IQHIP_ERR_INVALID, "iqhip_debug_pars_levels: " + err);
    return IQHIP_OK;
}

// single-device plain engines of 4 / 20 / 64 states with model and alignment; need_init: the call works on what
// iqhip_pars_init laid out
static int pars_require(iqhip_engine *e, const char *what, bool need_init) {
    const int rc = require(e, what, REQ_SINGLE_DEVICE | REQ_PLAIN_STATES | REQ_STATES_4_20_64 | REQ_MODEL_ALN);
    if (rc) return rc;
    if (need_init && !e->pars_ready)
        return fail(IQHIP_ERR_INVALID, std::string(what) + ": needs iqhip_pars_init first (the alignment or its frequencies changed since)");
    return IQHIP_OK;
}

// the device time of a call's launches (with iqhip_timing_enable) adds up across calls until the debug read resets it
static void pars_add_ms(PhaseTimer &timer, double *ms) {
    double t;
    if (timer.read(&t)) *ms += t;
}

// pinned staging of at least `need` words, grown by half
static size_t pars_grown(size_t need) { return need + need / 2 + 64; }

extern "C" int iqhip_pars_shape(iqhip_engine *e, int64_t *nsites, int64_t *nwords, int *nvectors) {
    int rc = pars_require(e, "iqhip_pars_shape", true);
    if (rc) return rc;
    if (nsites) *nsites = e->pars_nsites;
    if (nwords) *nwords = e->pars_nwords;
    if (nvectors) *nvectors = e->pars_nvec;
    return IQHIP_OK;
}

extern "C" int iqhip_pars_init(iqhip_engine *e, const uint8_t *informative, int nvectors, int64_t *nsites) {
    int rc = pars_require(e, "iqhip_pars_init", false);
    if (rc) return rc;
    e->pars_ready = false;
    if (nvectors < 0) return fail(IQHIP_ERR_INVALID, "iqhip_pars_init: nvectors < 0");
    const int n = e->n;
    const int nst = e->state_unknown + 1;
    if ((int64_t)e->h_freq.size() != e->nptn || e->h_evec0.size() != (size_t)n * n || e->h_tip0.size() != (size_t)nst * n)
        return fail(IQHIP_ERR_INVALID, "iqhip_pars_init: the alignment or the model is not set");
    // the sites: pattern p, ptn_freq[p] times, in pattern order
    int64_t total = 0;
    for (int64_t p = 0; p < e->nptn; p++) {
        const double f = e->h_freq[(size_t)p];
        if (!(f >= 0.0) || f != std::floor(f) || f > 2147483647.0)
            return fail(IQHIP_ERR_INVALID, "iqhip_pars_init: pattern frequencies must be non-negative integers");
        if (!informative || informative[p]) total += (int64_t)f;
    }
    if (total > 2147483647LL - 32) return fail(IQHIP_ERR_UNSUPPORTED, "iqhip_pars_init: more than 2^31 sites");
    std::vector<int32_t> site_ptn;
    site_ptn.reserve((size_t)total + 1);
    for (int64_t p = 0; p < e->nptn; p++)
        if (!informative || informative[p]) site_ptn.insert(site_ptn.end(), (size_t)e->h_freq[(size_t)p], (int32_t)p);
    const int64_t nwords = std::max<int64_t>(1, (total + 31) / 32);
    // the states a code allows: the tip table row is U^-1 times the indicator, so U times the row gives it back
    std::vector<uint64_t> masks((size_t)nst, 0);
    for (int s = 0; s < nst; s++)
        for (int i = 0; i < n; i++) {
            double v = 0.0;
            for (int k = 0; k < n; k++) v += e->h_evec0[(size_t)i * n + k] * e->h_tip0[(size_t)s * n + k];
            if (v > 0.5) masks[(size_t)s] |= 1ull << i;
        }
    HIPCHK(use_device(e));
    const size_t nslots = (size_t)e->ntaxa + (size_t)nvectors;
    const size_t vec_words = nslots * (size_t)nwords * n, score_words = nslots * (size_t)nwords;
    HIPCHK(e->pars.vec.ensure(e, vec_words));
    HIPCHK(e->pars.score.ensure(e, score_words));
    HIPCHK(e->pars.ints.ensure(e, site_ptn.size() + 1));
    HIPCHK(e->pars.masks.ensure(e, (size_t)nst));
    e->pars_nsites = total;
    e->pars_nwords = nwords;
    e->pars_nvec = nvectors;
    e->pars_valid.assign((size_t)nvectors, 0);
    HIPCHK(hipStreamSynchronize(e->stream));   // (pageable sources: the copies must not outlive them)
    if (!site_ptn.empty())
        HIPCHK(hipMemcpyAsync(e->pars.ints.p, site_ptn.data(), sizeof(int32_t) * site_ptn.size(), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(e->pars.masks.p, masks.data(), sizeof(uint64_t) * masks.size(), hipMemcpyHostToDevice, e->stream));
    HIPCHK(launch_pars_tips(e, e->pars.ints.p));
    HIPCHK(hipStreamSynchronize(e->stream));
    if (nsites) *nsites = total;
    e->pars_ready = true;
    return IQHIP_OK;
}

extern "C" int iqhip_pars_update(iqhip_engine *e, const iqhip_pars_op *ops, int nops) {
    int rc = pars_require(e, "iqhip_pars_update", true);
    if (rc) return rc;
    std::vector<int32_t> level((size_t)std::max(nops, 0));
    const std::string err = pars_levels(e->ntaxa, e->pars_nvec, e->pars_valid.data(), ops, nops, level.data());
    if (!err.empty()) return fail(IQHIP_ERR_INVALID, "iqhip_pars_update: " + err);
    if (nops == 0) return IQHIP_OK;
    // the ops sorted by level (stable), and where each level starts
    int nlev = 0;
    for (int k = 0; k < nops; k++) nlev = std::max(nlev, level[(size_t)k] + 1);
    std::vector<int32_t> start((size_t)nlev + 1, 0);
    for (int k = 0; k < nops; k++) start[(size_t)level[(size_t)k] + 1]++;
    for (int l = 0; l < nlev; l++) start[(size_t)l + 1] += start[(size_t)l];
    // one upload from pinned staging: ops (4 words each) ++ level starts.  The staging buffer may still feed the previous
    // update's copy, so the stream is drained first (after a scores call it is idle); nothing waits after the launch
    const size_t nblob = (size_t)4 * nops + (size_t)nlev + 1;
    HIPCHK(use_device(e));
    HIPCHK(e->pars.ints.ensure(e, nblob));
    if (nblob > e->h_pars_ops.cap) HIPCHK(e->h_pars_ops.ensure(e, pars_grown(nblob)));
    HIPCHK(hipStreamSynchronize(e->stream));
    {
        std::vector<int32_t> at(start.begin(), start.end() - 1);
        iqhip_pars_op *sorted = reinterpret_cast<iqhip_pars_op *>(e->h_pars_ops.p);
        for (int k = 0; k < nops; k++) sorted[at[(size_t)level[(size_t)k]]++] = ops[k];
        std::copy(start.begin(), start.end(), e->h_pars_ops.p + (size_t)4 * nops);
    }
    HIPCHK(hipMemcpyAsync(e->pars.ints.p, e->h_pars_ops.p, sizeof(int32_t) * nblob, hipMemcpyHostToDevice, e->stream));
    PhaseTimer timer(e, 1);
    timer.mark();
    HIPCHK(launch_pars_update(e, reinterpret_cast<const iqhip_pars_op *>(e->pars.ints.p), e->pars.ints.p + (size_t)4 * nops, nlev));
    timer.mark();
    e->pars_counts[0] += 1;
    e->pars_counts[2] += nops;
    pars_add_ms(timer, &e->pars_ms[0]);
    for (int k = 0; k < nops; k++) e->pars_valid[(size_t)(ops[k].dst - e->ntaxa)] = 1;
    return IQHIP_OK;
}

// the slots of a branch list must hold something
static int pars_check_ends(iqhip_engine *e, const char *what, const int32_t *ends, int nbranch) {
    if (!ends || nbranch < 1) return fail(IQHIP_ERR_INVALID, std::string(what) + ": bad branch list (nbranch >= 1)");
    const int64_t nslots = (int64_t)e->ntaxa + e->pars_nvec;
    for (int64_t k = 0; k < 2 * (int64_t)nbranch; k++) {
        const int32_t s = ends[k];
        if (s < 0 || s >= nslots) return fail(IQHIP_ERR_INVALID, std::string(what) + ": slot outside [0, ntaxa + nvectors)");
        if (s >= e->ntaxa && !e->pars_valid[(size_t)(s - e->ntaxa)])
            return fail(IQHIP_ERR_INVALID, std::string(what) + ": slot " + std::to_string(s) + " has never been written");
    }
    return IQHIP_OK;
}

static int pars_scores(iqhip_engine *e, const int32_t *ends, int nbranch, int taxon, std::vector<int32_t> &out, size_t from,
                       size_t count) {
    HIPCHK(use_device(e));
    const size_t need_out = (size_t)2 * nbranch + 2;
    HIPCHK(e->pars.ints.ensure(e, (size_t)2 * nbranch));
    HIPCHK(e->pars.out.ensure(e, need_out));
    if ((size_t)2 * nbranch > e->h_pars_ends.cap) HIPCHK(e->h_pars_ends.ensure(e, pars_grown((size_t)2 * nbranch)));
    if (count > e->h_pars_out.cap) HIPCHK(e->h_pars_out.ensure(e, pars_grown(count)));
    // (no copy of h_pars_ends or into h_pars_out is in flight: every call of this function ends with a synchronise)
    memcpy(e->h_pars_ends.p, ends, sizeof(int32_t) * 2 * (size_t)nbranch);
    HIPCHK(hipMemcpyAsync(e->pars.ints.p, e->h_pars_ends.p, sizeof(int32_t) * 2 * (size_t)nbranch, hipMemcpyHostToDevice, e->stream));
    PhaseTimer timer(e, 1);
    int nlaunches = 0;
    timer.mark();
    HIPCHK(launch_pars_branch(e, e->pars.ints.p, nbranch, taxon, e->pars.out.p, &nlaunches));
    timer.mark();
    if (taxon >= 0) {   // (the insertion scans: plain branch scores are not tallied)
        e->pars_counts[1] += nlaunches;
        e->pars_counts[3] += nbranch;
        pars_add_ms(timer, &e->pars_ms[1]);
    }
    HIPCHK(hipMemcpyAsync(e->h_pars_out.p, e->pars.out.p + from, sizeof(int32_t) * count, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    out.assign(e->h_pars_out.p, e->h_pars_out.p + count);
    return IQHIP_OK;
}

extern "C" int iqhip_pars_branch_scores(iqhip_engine *e, const int32_t *ends, int nbranch, int32_t *score, int32_t *subst) {
    int rc = pars_require(e, "iqhip_pars_branch_scores", true);
    if (rc) return rc;
    rc = pars_check_ends(e, "iqhip_pars_branch_scores", ends, nbranch);
    if (rc) return rc;
    std::vector<int32_t> out;
    rc = pars_scores(e, ends, nbranch, -1, out, 0, (size_t)2 * nbranch);
    if (rc) return rc;
    if (score) memcpy(score, out.data(), sizeof(int32_t) * (size_t)nbranch);
    if (subst) memcpy(subst, out.data() + nbranch, sizeof(int32_t) * (size_t)nbranch);
    return IQHIP_OK;
}

extern "C" int iqhip_pars_insert_scores(iqhip_engine *e, const int32_t *ends, int nbranch, int32_t taxon, int32_t *score,
                                        int32_t *best, int32_t *best_score) {
    int rc = pars_require(e, "iqhip_pars_insert_scores", true);
    if (rc) return rc;
    rc = pars_check_ends(e, "iqhip_pars_insert_scores", ends, nbranch);
    if (rc) return rc;
    if (taxon < 0 || taxon >= e->ntaxa) return fail(IQHIP_ERR_INVALID, "iqhip_pars_insert_scores: taxon is not a tip slot");
    // without `score` the host reads back two integers
    std::vector<int32_t> out;
    const size_t from = score ? 0 : (size_t)2 * nbranch, count = score ? (size_t)2 * nbranch + 2 : 2;
    rc = pars_scores(e, ends, nbranch, taxon, out, from, count);
    if (rc) return rc;
    if (score) memcpy(score, out.data(), sizeof(int32_t) * (size_t)nbranch);
    if (best) *best = out[count - 2];
    if (best_score) *best_score = out[count - 1];
    return IQHIP_OK;
}

// ---- the segmented insertion scan: one stepwise-addition step of many trees ------------------------------------------------
extern "C" int iqhip_pars_insert_scores_batch(iqhip_engine *e, const int32_t *ends, const int32_t *seg_start, int nseg,
                                              const int32_t *taxon, int32_t *score, int32_t *best, int32_t *best_score) {
    const char *what = "iqhip_pars_insert_scores_batch";
    int rc = pars_require(e, what, true);
    if (rc) return rc;
    // IQHIP_PARS_BATCH_ROUTE, read per call: wave | wg forces a route; any other word is refused
    ParsBatchRoute route = PARS_BATCH_AUTO;
    if (const char *w = getenv("IQHIP_PARS_BATCH_ROUTE")) {
        if (!strcmp(w, "wave")) route = PARS_BATCH_WAVE;
        else if (!strcmp(w, "wg")) route = PARS_BATCH_WG;
        else return fail(IQHIP_ERR_INVALID, std::string(what) + ": IQHIP_PARS_BATCH_ROUTE must be wave or wg, not '" + w + "'");
    }
    if (!ends || !seg_start || !taxon || !best || !best_score) return fail(IQHIP_ERR_INVALID, std::string(what) + ": null argument");
    if (nseg < 1) return fail(IQHIP_ERR_INVALID, std::string(what) + ": nseg < 1");
    if (seg_start[0] != 0) return fail(IQHIP_ERR_INVALID, std::string(what) + ": seg_start[0] != 0");
    for (int g = 0; g < nseg; g++) {
        if (seg_start[g + 1] <= seg_start[g])
            return fail(IQHIP_ERR_INVALID, std::string(what) + ": seg_start is not strictly increasing (segment " + std::to_string(g) + " is empty)");
        if (taxon[g] < 0 || taxon[g] >= e->ntaxa)
            return fail(IQHIP_ERR_INVALID, std::string(what) + ": taxon " + std::to_string(g) + " is not a tip slot");
    }
    const int nbranch = seg_start[nseg];
    rc = pars_check_ends(e, what, ends, nbranch);
    if (rc) return rc;
    // one upload from pinned staging: ends ++ the taxon of every branch ++ seg_start; the results are score [nbranch] ++
    // best [nseg] ++ best_score [nseg], of which only the last 2 nseg come back without `score`
    const size_t nblob = (size_t)3 * nbranch + (size_t)nseg + 1, nout = (size_t)nbranch + 2 * (size_t)nseg;
    const size_t from = score ? 0 : (size_t)nbranch, count = nout - from;
    HIPCHK(use_device(e));
    HIPCHK(e->pars.ints.ensure(e, nblob));
    HIPCHK(e->pars.out.ensure(e, nout));
    if (nblob > e->h_pars_ends.cap) HIPCHK(e->h_pars_ends.ensure(e, pars_grown(nblob)));
    if (count > e->h_pars_out.cap) HIPCHK(e->h_pars_out.ensure(e, pars_grown(count)));
    // (no copy of h_pars_ends or into h_pars_out is in flight: every call that uses them ends with a synchronise)
    int32_t *blob = e->h_pars_ends.p;
    memcpy(blob, ends, sizeof(int32_t) * 2 * (size_t)nbranch);
    for (int g = 0; g < nseg; g++) std::fill(blob + 2 * (size_t)nbranch + seg_start[g], blob + 2 * (size_t)nbranch + seg_start[g + 1], taxon[g]);
    memcpy(blob + 3 * (size_t)nbranch, seg_start, sizeof(int32_t) * ((size_t)nseg + 1));
    HIPCHK(hipMemcpyAsync(e->pars.ints.p, blob, sizeof(int32_t) * nblob, hipMemcpyHostToDevice, e->stream));
    PhaseTimer timer(e, 1);
    int nlaunches = 0;
    timer.mark();
    HIPCHK(launch_pars_insert_batch(e, e->pars.ints.p, e->pars.ints.p + 2 * (size_t)nbranch, nbranch, e->pars.ints.p + 3 * (size_t)nbranch,
                                    nseg, route, e->pars.out.p, &nlaunches));
    timer.mark();
    e->pars_batch_counts[0] += nlaunches;
    e->pars_batch_counts[1] += nbranch;
    e->pars_batch_counts[2] += nseg;
    pars_add_ms(timer, &e->pars_batch_ms);
    HIPCHK(hipMemcpyAsync(e->h_pars_out.p, e->pars.out.p + from, sizeof(int32_t) * count, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    const int32_t *res = e->h_pars_out.p;
    if (score) {
        memcpy(score, res, sizeof(int32_t) * (size_t)nbranch);
        res += nbranch;
    }
    memcpy(best, res, sizeof(int32_t) * (size_t)nseg);
    memcpy(best_score, res + nseg, sizeof(int32_t) * (size_t)nseg);
    return IQHIP_OK;
}

extern "C" int iqhip_debug_pars_batch_timing(iqhip_engine *e, double *ms, int64_t *counts, int reset) {
    if (!e || !e->shards.empty() || e->planner) return fail(IQHIP_ERR_INVALID, "iqhip_debug_pars_batch_timing: needs a single-device engine");
    if (ms) *ms = e->pars_batch_ms;
    for (int k = 0; k < 3; k++)
        if (counts) counts[k] = e->pars_batch_counts[k];
    if (reset) {
        e->pars_batch_ms = 0.0;
        for (int k = 0; k < 3; k++) e->pars_batch_counts[k] = 0;
    }
    return IQHIP_OK;
}

extern "C" int iqhip_pars_fetch(iqhip_engine *e, int32_t slot, uint32_t *out) {
    int rc = pars_require(e, "iqhip_pars_fetch", true);
    if (rc) return rc;
    if (!out) return fail(IQHIP_ERR_INVALID, "iqhip_pars_fetch: null argument");
    if (slot < 0 || slot >= (int64_t)e->ntaxa + e->pars_nvec) return fail(IQHIP_ERR_INVALID, "iqhip_pars_fetch: slot outside [0, ntaxa + nvectors)");
    if (slot >= e->ntaxa && !e->pars_valid[(size_t)(slot - e->ntaxa)])
        return fail(IQHIP_ERR_INVALID, "iqhip_pars_fetch: the slot has never been written");
    HIPCHK(use_device(e));
    const int n = e->n;
    const size_t nw = (size_t)e->pars_nwords;
    std::vector<uint32_t> v(nw * n), sc(nw);
    HIPCHK(hipStreamSynchronize(e->stream));
    HIPCHK(hipMemcpy(v.data(), e->pars.vec.p + (size_t)slot * nw * n, sizeof(uint32_t) * v.size(), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(sc.data(), e->pars.score.p + (size_t)slot * nw, sizeof(uint32_t) * nw, hipMemcpyDeviceToHost));
    if (n == 4) memcpy(out, v.data(), sizeof(uint32_t) * v.size());
    else
        for (size_t w = 0; w < nw; w++)
            for (int i = 0; i < n; i++) out[w * n + i] = v[(size_t)i * nw + w];
    uint32_t total = 0;
    for (size_t w = 0; w < nw; w++) total += sc[w];
    out[nw * n] = total;
    return IQHIP_OK;
}

// ---- the SPR scan ---------------------------------------------------------------------------------------------------------
extern "C" int iqhip_debug_pars_spr_check(int ntaxa, int nvectors, const uint8_t *valid, const iqhip_pars_spr_job *jobs, int njobs,
                                          const iqhip_pars_spr_step *steps, int nsteps, int32_t *depth) {
    const std::string err = iqhip::pars_spr_check(ntaxa, nvectors, valid, jobs, njobs, steps, nsteps, depth, nullptr);
    if (!err.empty()) return fail(IQHIP_ERR_INVALID, "iqhip_debug_pars_spr_check: " + err);
    return IQHIP_OK;
}

extern "C" int iqhip_pars_spr_scan(iqhip_engine *e, const iqhip_pars_spr_job *jobs, int njobs, const iqhip_pars_spr_step *steps,
                                   int nsteps, int32_t *score, int32_t *best_step, int32_t *best_score, int32_t *best_job) {
    int rc = pars_require(e, "iqhip_pars_spr_scan", true);
    if (rc) return rc;
    std::vector<int32_t> depth((size_t)std::max(nsteps, 0));
    int max_depth = 0;
    const std::string err = pars_spr_check(e->ntaxa, e->pars_nvec, e->pars_valid.data(), jobs, njobs, steps, nsteps, depth.data(), &max_depth);
    if (!err.empty()) return fail(IQHIP_ERR_INVALID, "iqhip_pars_spr_scan: " + err);
    if (best_job) *best_job = -1;
    if (score) std::fill(score, score + nsteps, -1);
    if (njobs == 0) return IQHIP_OK;
    if (nsteps == 0) {   // jobs without steps: nothing to launch
        for (int j = 0; j < njobs; j++) {
            if (best_step) best_step[j] = -1;
            if (best_score) best_score[j] = 0x7fffffff;
        }
        return IQHIP_OK;
    }
    // one upload from pinned staging: jobs ++ steps (4 words each), the steps with their depth in the place of `parent`
    const size_t nblob = (size_t)4 * njobs + (size_t)4 * nsteps;
    const size_t nout = (size_t)nsteps + 2 * (size_t)njobs + 1;
    const size_t from = score ? 0 : (size_t)nsteps, count = nout - from;
    HIPCHK(use_device(e));
    HIPCHK(e->pars.ints.ensure(e, nblob));
    HIPCHK(e->pars.out.ensure(e, nout));
    if (nblob > e->h_pars_ops.cap) HIPCHK(e->h_pars_ops.ensure(e, pars_grown(nblob)));
    if (count > e->h_pars_out.cap) HIPCHK(e->h_pars_out.ensure(e, pars_grown(count)));
    HIPCHK(hipStreamSynchronize(e->stream));   // (the staging buffer may still feed the previous update's copy)
    memcpy(e->h_pars_ops.p, jobs, sizeof(iqhip_pars_spr_job) * (size_t)njobs);
    iqhip_pars_spr_step *hs = reinterpret_cast<iqhip_pars_spr_step *>(e->h_pars_ops.p + (size_t)4 * njobs);
    int64_t scored = 0;
    for (int k = 0; k < nsteps; k++) {
        hs[k] = steps[k];
        hs[k].parent = depth[(size_t)k];
        if (depth[(size_t)k] >= 0 && !(steps[k].flags & IQHIP_PARS_SPR_NO_SCORE)) scored++;
    }
    HIPCHK(hipMemcpyAsync(e->pars.ints.p, e->h_pars_ops.p, sizeof(int32_t) * nblob, hipMemcpyHostToDevice, e->stream));
    PhaseTimer timer(e, 1);
    int nlaunches = 0;
    timer.mark();
    HIPCHK(launch_pars_spr(e, reinterpret_cast<const iqhip_pars_spr_job *>(e->pars.ints.p), njobs,
                           reinterpret_cast<const iqhip_pars_spr_step *>(e->pars.ints.p + (size_t)4 * njobs), nsteps, max_depth,
                           e->pars.out.p, &nlaunches));
    timer.mark();
    e->pars_spr_counts[0] += nlaunches;
    e->pars_spr_counts[1] += scored;
    pars_add_ms(timer, &e->pars_spr_ms);
    HIPCHK(hipMemcpyAsync(e->h_pars_out.p, e->pars.out.p + from, sizeof(int32_t) * count, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    const int32_t *res = e->h_pars_out.p;
    if (score) {
        memcpy(score, res, sizeof(int32_t) * (size_t)nsteps);
        res += nsteps;
    }
    if (best_step) memcpy(best_step, res, sizeof(int32_t) * (size_t)njobs);
    if (best_score) memcpy(best_score, res + njobs, sizeof(int32_t) * (size_t)njobs);
    if (best_job) *best_job = res[2 * (size_t)njobs];
    return IQHIP_OK;
}

extern "C" int iqhip_debug_pars_spr_timing(iqhip_engine *e, double *ms, int64_t *counts, int reset) {
    if (!e || !e->shards.empty() || e->planner) return fail(IQHIP_ERR_INVALID, "iqhip_debug_pars_spr_timing: needs a single-device engine");
    if (ms) *ms = e->pars_spr_ms;
    for (int k = 0; k < 2; k++)
        if (counts) counts[k] = e->pars_spr_counts[k];
    if (reset) {
        e->pars_spr_ms = 0.0;
        e->pars_spr_counts[0] = e->pars_spr_counts[1] = 0;
    }
    return IQHIP_OK;
}

extern "C" int iqhip_debug_pars_timing(iqhip_engine *e, double *ms, int64_t *counts, int reset) {
    if (!e || !e->shards.empty() || e->planner) return fail(IQHIP_ERR_INVALID, "iqhip_debug_pars_timing: needs a single-device engine");
    for (int k = 0; k < 2; k++)
        if (ms) ms[k] = e->pars_ms[k];
    for (int k = 0; k < 4; k++)
        if (counts) counts[k] = e->pars_counts[k];
    if (reset) {
        e->pars_ms[0] = e->pars_ms[1] = 0.0;
        for (int k = 0; k < 4; k++) e->pars_counts[k] = 0;
    }
    return IQHIP_OK;
}
