// quartet.hip -- driver of likelihood mapping (PhyloTree::computeQuartetLikelihoods).  Host code only; the kernels are in
// kernels_quartet.hip.
#include <stdlib.h>
#include <cmath>
#include <cstring>

#include "iqhip_internal.h"

using namespace iqhip;

// single-device plain 4-state engines (the cell tally has 4^4 cells) without mixture or +ASC, model and alignment set.  A
// one-class model set through iqhip_set_mixture_model counts as a mixture, and as such before the alignment is asked for
static int quartet_require(iqhip_engine *e, const char *what) {
    int rc = require(e, what, REQ_SINGLE_DEVICE | REQ_NO_ASC | REQ_PLAIN_STATES | REQ_STATES_4 | REQ_NO_MIXTURE);
    if (rc) return rc;
    if (e->mixture_api) return fail(IQHIP_ERR_UNSUPPORTED, std::string(what) + ": not available for mixture models");
    return require(e, what, REQ_MODEL_ALN);
}

// the quartet list and the pattern frequencies; *nsite = the sum of all frequencies
static int quartet_inputs(const iqhip_engine *e, const char *what, const int32_t *quartets, int nq, double *nsite) {
    if (!quartets || nq < 1) return fail(IQHIP_ERR_INVALID, std::string(what) + ": bad quartet list (nq >= 1)");
    for (int64_t q = 0; q < nq; q++) {
        const int32_t *t = quartets + 4 * q;
        for (int i = 0; i < 4; i++) {
            if (t[i] < 0 || t[i] >= e->ntaxa) return fail(IQHIP_ERR_INVALID, std::string(what) + ": taxon outside [0, ntaxa)");
            for (int j = 0; j < i; j++)
                if (t[i] == t[j]) return fail(IQHIP_ERR_INVALID, std::string(what) + ": a taxon twice in a quartet");
        }
    }
    if ((int64_t)e->h_freq.size() != e->nptn) return fail(IQHIP_ERR_INVALID, std::string(what) + ": the alignment is not set");
    double total = 0.0;
    for (double f : e->h_freq) {
        if (!(f >= 0.0) || f != std::floor(f) || f >= 9007199254740992.0)
            return fail(IQHIP_ERR_INVALID, std::string(what) + ": pattern frequencies must be non-negative integers below 2^53");
        total += f;
    }
    if (nsite) *nsite = total;
    return IQHIP_OK;
}

// quartets per chunk: the cell tables and the worst-case other-lists of a chunk stay within 64 MB; IQHIP_QUARTET_CHUNK (read
// per call) overrides
static int64_t quartet_chunk(const iqhip_engine *e, int64_t nq) {
    const int64_t per = 256 * (int64_t)sizeof(double) + (int64_t)sizeof(int32_t) * (e->nptn + 1);
    int64_t chunk = std::max<int64_t>(1, ((int64_t)64 << 20) / per);
    if (const char *qc = getenv("IQHIP_QUARTET_CHUNK")) chunk = std::max(1, atoi(qc));
    return std::max<int64_t>(1, std::min(chunk, nq));
}

static int quartet_buffers(iqhip_engine *e, const int32_t *quartets, int nq, int64_t chunk) {
    HIPCHK(e->qt.quartets.ensure(e, (size_t)4 * nq));
    HIPCHK(e->qt.cells.ensure(e, (size_t)chunk * 256));
    HIPCHK(e->qt.nother.ensure(e, (size_t)chunk));
    HIPCHK(e->qt.other.ensure(e, (size_t)chunk * (size_t)e->nptn));
    HIPCHK(hipStreamSynchronize(e->stream));   // (pageable source: the copy must not outlive the caller's array)
    HIPCHK(hipMemcpyAsync(e->qt.quartets.p, quartets, sizeof(int32_t) * 4 * (size_t)nq, hipMemcpyHostToDevice, e->stream));
    return IQHIP_OK;
}

extern "C" int iqhip_quartet_cells(iqhip_engine *e, const int32_t *quartets, int nq, double *cells, int32_t *nother) {
    int rc = quartet_require(e, "iqhip_quartet_cells");
    if (rc) return rc;
    if (!cells || !nother) return fail(IQHIP_ERR_INVALID, "iqhip_quartet_cells: null argument");
    rc = quartet_inputs(e, "iqhip_quartet_cells", quartets, nq, nullptr);
    if (rc) return rc;
    HIPCHK(use_device(e));
    const int64_t chunk = quartet_chunk(e, nq);
    rc = quartet_buffers(e, quartets, nq, chunk);
    if (rc) return rc;
    for (int64_t first = 0; first < nq; first += chunk) {
        const int m = (int)std::min<int64_t>(chunk, nq - first);
        HIPCHK(launch_quartet_cells(e, e->qt.quartets.p + 4 * first, m, e->qt.cells.p, e->qt.nother.p, e->qt.other.p));
        HIPCHK(hipMemcpyAsync(cells + (size_t)first * 256, e->qt.cells.p, sizeof(double) * 256 * (size_t)m, hipMemcpyDeviceToHost,
                              e->stream));
        HIPCHK(hipMemcpyAsync(nother + first, e->qt.nother.p, sizeof(int32_t) * (size_t)m, hipMemcpyDeviceToHost, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
    }
    return IQHIP_OK;
}

extern "C" int iqhip_quartet_likelihoods(iqhip_engine *e, const int32_t *quartets, int nq, const double *const_invar, double x1,
                                         double x2, double xacc, int max_steps, double diverge_frac, int iterations,
                                         double tolerance, iqhip_quartet_result *results) {
    int rc = quartet_require(e, "iqhip_quartet_likelihoods");
    if (rc) return rc;
    if (!results) return fail(IQHIP_ERR_INVALID, "iqhip_quartet_likelihoods: null argument");
    if (!(x1 >= 0.0) || x1 > x2 || !std::isfinite(x2) || !(xacc > 0.0) || max_steps < 1)
        return fail(IQHIP_ERR_INVALID, "iqhip_quartet_likelihoods: bad bounds / tolerance / step count (x1 <= x2, max_steps >= 1)");
    if (iterations < 1 || !(tolerance >= 0.0) || !std::isfinite(diverge_frac))
        return fail(IQHIP_ERR_INVALID, "iqhip_quartet_likelihoods: iterations >= 1, tolerance >= 0");
    if (const_invar)
        for (int i = 0; i < 5; i++)
            if (!std::isfinite(const_invar[i]) || const_invar[i] < 0.0)
                return fail(IQHIP_ERR_INVALID, "iqhip_quartet_likelihoods: const_invar must be finite and non-negative");
    double nsite = 0.0;
    rc = quartet_inputs(e, "iqhip_quartet_likelihoods", quartets, nq, &nsite);
    if (rc) return rc;
    if (!(nsite > 0.0)) return fail(IQHIP_ERR_INVALID, "iqhip_quartet_likelihoods: the alignment has no sites");
    const int nst = e->state_unknown + 1;
    if (e->h_evec0.size() != 16 || e->h_tip0.size() != (size_t)nst * 4 || nst > 32)
        return fail(IQHIP_ERR_INVALID, "iqhip_quartet_likelihoods: the model is not set");
    QuartetSolveArgs a;
    memset(&a, 0, sizeof(a));
    // the states a code allows: the tip table row is U^-1 times the indicator, so U times the row gives it back (as iqhip_pars_init)
    for (int s = 0; s < nst; s++)
        for (int i = 0; i < 4; i++) {
            double v = 0.0;
            for (int k = 0; k < 4; k++) v += e->h_evec0[(size_t)i * 4 + k] * e->h_tip0[(size_t)s * 4 + k];
            if (v > 0.5) a.mask[s] |= (uint8_t)(1u << i);
        }
    HIPCHK(use_device(e));
    const int64_t chunk = quartet_chunk(e, nq);
    rc = quartet_buffers(e, quartets, nq, chunk);
    if (rc) return rc;
    HIPCHK(e->qt.out.ensure(e, (size_t)nq));
    HIPCHK(hipMemsetAsync(e->qt.out.p, 0, sizeof(iqhip_quartet_result) * (size_t)nq, e->stream));
    a.cells = e->qt.cells.p;
    a.nother = e->qt.nother.p;
    a.other = e->qt.other.p;
    a.states = e->d_states.p;
    a.freq = e->d_freq.p;
    a.evec = e->d_evec;
    a.inv_evec = e->d_inv_evec;
    a.eval = e->d_eval;
    a.rates = e->d_rates;
    a.props = e->d_props;
    a.tip = e->d_tip;
    a.out = e->qt.out.p;
    a.nptn_pad = e->nptn_pad;
    a.nptn = e->nptn;
    if (const_invar)
        for (int i = 0; i < 5; i++) a.const_invar[i] = const_invar[i];
    a.nsite = nsite;
    a.x1 = x1;
    a.x2 = x2;
    a.xacc = xacc;
    a.diverge_frac = diverge_frac;
    a.tolerance = tolerance;
    a.ncat = e->ncat;
    a.state_unknown = e->state_unknown;
    a.max_steps = max_steps;
    a.iterations = iterations;
    // iqhip_timing_enable: device time of the cell and the solve launches, summed over the chunks
    PhaseTimer timer(e, 2);
    e->qt.ms[0] = e->qt.ms[1] = 0.0;
    for (int64_t first = 0; first < nq; first += chunk) {
        const int m = (int)std::min<int64_t>(chunk, nq - first);
        a.quartets = e->qt.quartets.p + 4 * first;
        a.first = first;
        timer.mark();
        HIPCHK(launch_quartet_cells(e, a.quartets, m, e->qt.cells.p, e->qt.nother.p, e->qt.other.p));
        timer.mark();
        HIPCHK(launch_quartet_solve(e, a, m));
        timer.mark();
    }
    HIPCHK(hipMemcpyAsync(results, e->qt.out.p, sizeof(iqhip_quartet_result) * (size_t)nq, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    timer.read(e->qt.ms);
    int worst = 0;
    for (int64_t q = 0; q < nq && !worst; q++)
        for (int k = 0; k < 3 && !worst; k++) worst = results[q].status[k];
    return newton_status(worst);   // (minimizeNewton's two nrerror() exits; the results are filled all the same)
}

extern "C" int iqhip_debug_quartet_timing(iqhip_engine *e, double *cells_ms, double *solve_ms) {
    if (!e || !e->shards.empty()) return fail(IQHIP_ERR_INVALID, "iqhip_debug_quartet_timing: needs a single-device engine");
    if (cells_ms) *cells_ms = e->qt.ms[0];
    if (solve_ms) *solve_ms = e->qt.ms[1];
    return IQHIP_OK;
}
