// classlh.hip -- drivers of what consumes theta per category or per class: the EM for +R free-rate models and the
// empirical-Bayes site rates, the EM for mixture class weights with the class posteriors and pattern state frequencies, and
// the per-class log-likelihoods.  Host code only; the kernels are in kernels_em.hip, kernels_mixem.hip and
// kernels_classlnl.hip.
#include <string.h>
#include <cmath>

#include "iqhip_internal.h"

using namespace iqhip;

// rows [nrows][nptn_pad] on the device -> out [nptn][nrows] on the host
static int fetch_transposed(iqhip_engine *e, const double *d_rows, size_t nrows, double *out) {
    const size_t P = (size_t)e->nptn_pad, N = (size_t)e->nptn;
    std::vector<double> rows(nrows * P);
    HIPCHK(hipMemcpyAsync(rows.data(), d_rows, sizeof(double) * rows.size(), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    for (size_t p = 0; p < N; p++)
        for (size_t r = 0; r < nrows; r++) out[p * nrows + r] = rows[r * P + p];
    return IQHIP_OK;
}

// the per-class component lists, first [nclass + 1] ++ the components of every class in ascending order (cat_class is an
// arbitrary map); returns the size of the largest class
static size_t class_components(const iqhip_engine *e, std::vector<int32_t> &list) {
    const size_t M = (size_t)e->nclass, C = (size_t)e->ncat;
    list.assign(M + 1 + C, 0);
    size_t at = 0, max_comp = 0;
    for (size_t m = 0; m < M; m++) {
        list[m] = (int32_t)at;
        for (size_t c = 0; c < C; c++)
            if ((size_t)e->h_cls[c] == m) list[M + 1 + at++] = (int32_t)c;
        max_comp = std::max(max_comp, at - (size_t)list[m]);
    }
    list[M] = (int32_t)at;
    return max_comp;
}

// ---- EM for +R free-rate models, empirical-Bayes site rates (kernels_em.hip) ----------------------------------------
// plain engines of 4 / 20 / 64 states only
static const unsigned kEmNeeds = REQ_SINGLE_DEVICE | REQ_NO_MIXTURE | REQ_NO_ASC | REQ_PLAIN_STATES;

// the call reads what the last E-step left
static int em_estep_done(iqhip_engine *e, const char *what) {
    if (!e->em.valid || e->em.w.cap < (size_t)e->ncat * (size_t)e->nptn_pad)
        return fail(IQHIP_ERR_INVALID, std::string(what) + ": needs iqhip_em_posteriors first");
    return IQHIP_OK;
}

static size_t em_part_rows(const iqhip_engine *e) { return (size_t)((e->nptn_pad + 255) / 256); }

extern "C" int iqhip_debug_em_timing(iqhip_engine *e, double *ms) {
    if (!e || !ms) return fail(IQHIP_ERR_INVALID, "iqhip_debug_em_timing: null argument");
    ms[0] = e->em.ms[0];
    ms[1] = e->em.ms[1];
    return IQHIP_OK;
}

extern "C" int iqhip_em_posteriors(iqhip_engine *e, double len, double *cat_sum) {
    if (!e || !cat_sum) return fail(IQHIP_ERR_INVALID, "iqhip_em_posteriors: null argument");
    int rc = require(e, "iqhip_em_posteriors", kEmNeeds | REQ_THETA);
    if (rc) return rc;
    if (!(len >= 0.0)) return fail(IQHIP_ERR_INVALID, "iqhip_em_posteriors: negative or NaN branch length");
    HIPCHK(use_device(e));
    const size_t P = (size_t)e->nptn_pad, C = (size_t)e->ncat;
    e->em.valid = false;
    HIPCHK(e->em.w.ensure(e, C * P));
    HIPCHK(e->em.rate.ensure(e, P));
    HIPCHK(e->em.cat.ensure(e, P));
    HIPCHK(e->em.part.ensure(e, em_part_rows(e) * 2 * C));
    HIPCHK(e->em.out.ensure(e, 2 * C));
    PhaseTimer timer(e, 1);
    timer.mark();
    HIPCHK(launch_em_posteriors(e, len, e->em.w.p, e->em.rate.p, e->em.cat.p, e->em.part.p, e->em.out.p));
    timer.mark();
    HIPCHK(hipMemcpyAsync(cat_sum, e->em.out.p, sizeof(double) * C, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    timer.read(&e->em.ms[0]);
    e->em.valid = true;
    return IQHIP_OK;
}

extern "C" int iqhip_em_fetch_posteriors(iqhip_engine *e, double *out) {
    if (!e || !out) return fail(IQHIP_ERR_INVALID, "iqhip_em_fetch_posteriors: null argument");
    int rc = require(e, "iqhip_em_fetch_posteriors", kEmNeeds);
    if (!rc) rc = em_estep_done(e, "iqhip_em_fetch_posteriors");
    if (rc) return rc;
    HIPCHK(use_device(e));
    return fetch_transposed(e, e->em.w.p, (size_t)e->ncat, out);
}

extern "C" int iqhip_em_site_rates(iqhip_engine *e, double *ptn_rate, int32_t *ptn_cat) {
    if (!e || !ptn_rate || !ptn_cat) return fail(IQHIP_ERR_INVALID, "iqhip_em_site_rates: null argument");
    int rc = require(e, "iqhip_em_site_rates", kEmNeeds);
    if (!rc) rc = em_estep_done(e, "iqhip_em_site_rates");
    if (rc) return rc;
    HIPCHK(use_device(e));
    HIPCHK(hipMemcpyAsync(ptn_rate, e->em.rate.p, sizeof(double) * (size_t)e->nptn, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipMemcpyAsync(ptn_cat, e->em.cat.p, sizeof(int32_t) * (size_t)e->nptn, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return IQHIP_OK;
}

extern "C" int iqhip_em_objective(iqhip_engine *e, iqhip_branch_end a, iqhip_branch_end b, double len, double *f,
                                  int64_t *floored) {
    if (!e || !f) return fail(IQHIP_ERR_INVALID, "iqhip_em_objective: null argument");
    int rc = require(e, "iqhip_em_objective", kEmNeeds | REQ_THETA);
    if (!rc) rc = em_estep_done(e, "iqhip_em_objective");
    if (rc) return rc;
    if (!(len >= 0.0)) return fail(IQHIP_ERR_INVALID, "iqhip_em_objective: negative or NaN branch length");
    for (int c = 0; c < e->ncat; c++)
        if (!(e->h_props[c] > 0.0)) return fail(IQHIP_ERR_INVALID, "iqhip_em_objective: every category weight must be > 0");
    HIPCHK(use_device(e));
    const int16_t *sc[2];
    rc = branch_scale_counters(e, a, b, sc);
    if (rc) return rc;
    const size_t C = (size_t)e->ncat;
    HIPCHK(e->em.part.ensure(e, em_part_rows(e) * 2 * C));
    HIPCHK(e->em.out.ensure(e, 2 * C));
    PhaseTimer timer(e, 1);
    timer.mark();
    HIPCHK(launch_em_objective(e, sc[0], sc[1], len, e->em.w.p, e->em.part.p, e->em.out.p));
    timer.mark();
    std::vector<double> res(2 * C);
    HIPCHK(hipMemcpyAsync(res.data(), e->em.out.p, sizeof(double) * res.size(), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    timer.read(&e->em.ms[1]);
    for (size_t c = 0; c < C; c++) {
        f[c] = res[c];
        if (floored) floored[c] = (int64_t)res[C + c];
    }
    return IQHIP_OK;
}

// ---- EM for mixture class weights, class posteriors, pattern state frequencies (kernels_mixem.hip) -------------------
// plain mixture engines of 4 / 20 / 64 states only
static const unsigned kMixNeeds = REQ_SINGLE_DEVICE | REQ_NO_ASC | REQ_PLAIN_STATES | REQ_MIXTURE;

// the call reads what the last iqhip_mix_class_lh left
static int mix_class_lh_done(iqhip_engine *e, const char *what) {
    if (e->mix.model_version != e->model_version || e->mix.nptn_pad != e->nptn_pad || e->mix.nclass != e->nclass ||
        e->mix.lc.cap < (size_t)e->nclass * (size_t)e->nptn_pad)
        return fail(IQHIP_ERR_INVALID, std::string(what) + ": needs iqhip_mix_class_lh first (again after every model change)");
    return IQHIP_OK;
}

extern "C" int iqhip_debug_mix_timing(iqhip_engine *e, double *ms, int64_t *launches) {
    if (!e || !ms) return fail(IQHIP_ERR_INVALID, "iqhip_debug_mix_timing: null argument");
    ms[0] = e->mix.ms[0];
    ms[1] = e->mix.ms[1];
    if (launches) *launches = e->mix.launches;
    return IQHIP_OK;
}

extern "C" int iqhip_mix_class_lh(iqhip_engine *e, double len, double *out) {
    int rc = require(e, "iqhip_mix_class_lh", kMixNeeds | REQ_THETA);
    if (rc) return rc;
    if (!(len >= 0.0)) return fail(IQHIP_ERR_INVALID, "iqhip_mix_class_lh: negative or NaN branch length");
    HIPCHK(use_device(e));
    const size_t P = (size_t)e->nptn_pad, M = (size_t)e->nclass;
    std::vector<int32_t> list;
    class_components(e, list);
    e->mix.model_version = 0;
    HIPCHK(e->mix.lc.ensure(e, M * P));
    HIPCHK(e->mix.list.ensure(e, list.size()));
    HIPCHK(hipStreamSynchronize(e->stream));   // (pageable source, and an earlier launch may still read the list)
    HIPCHK(hipMemcpyAsync(e->mix.list.p, list.data(), sizeof(int32_t) * list.size(), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    PhaseTimer timer(e, 1);
    timer.mark();
    HIPCHK(launch_mix_class_lh(e, len, e->mix.list.p, e->mix.lc.p));
    timer.mark();
    HIPCHK(hipStreamSynchronize(e->stream));
    timer.read(&e->mix.ms[0]);
    e->mix.model_version = e->model_version;
    e->mix.nptn_pad = e->nptn_pad;
    e->mix.nclass = e->nclass;
    return out ? fetch_transposed(e, e->mix.lc.p, M, out) : IQHIP_OK;
}

// ---- per-class log-likelihoods: K candidate models as the K classes of a mixture engine (kernels_classlnl.hip) ----------
extern "C" int iqhip_debug_class_lnl_timing(iqhip_engine *e, double *ms) {
    if (!e || !ms) return fail(IQHIP_ERR_INVALID, "iqhip_debug_class_lnl_timing: null argument");
    *ms = e->cl.ms;
    return IQHIP_OK;
}

extern "C" int iqhip_class_lnl(iqhip_engine *e, iqhip_branch_end a, iqhip_branch_end b, double len, const double *class_weight,
                               const double *class_invar, double *lnl, int64_t *floored) {
    const char *what = "iqhip_class_lnl";
    if (!e || !class_weight || !lnl) return fail(IQHIP_ERR_INVALID, "iqhip_class_lnl: null argument");
    int rc = require(e, what, REQ_SINGLE_DEVICE | REQ_NO_ASC | REQ_PLAIN_STATES);
    if (rc) return rc;
    if (!e->model_set || !e->mixture_api)
        return fail(IQHIP_ERR_UNSUPPORTED, std::string(what) + ": the model was not set through iqhip_set_mixture_model");
    if ((rc = require(e, what, REQ_THETA))) return rc;   // (behind the line above: an unsupported model is not an invalid call)
    if (!(len >= 0.0)) return fail(IQHIP_ERR_INVALID, std::string(what) + ": negative or NaN branch length");
    const size_t P = (size_t)e->nptn_pad, N = (size_t)e->nptn, M = (size_t)e->nclass;
    for (size_t m = 0; m < M; m++)
        if (!(class_weight[m] > 0.0) || !std::isfinite(class_weight[m]))
            return fail(IQHIP_ERR_INVALID, std::string(what) + ": every class weight must be > 0 and finite");
    HIPCHK(use_device(e));
    const int16_t *sc[2];
    rc = branch_scale_counters(e, a, b, sc);
    if (rc) return rc;
    // theta remembers the scale counters of the ends it was built from (either order: build_branch puts a leaf first)
    if (!((sc[0] == e->theta_a_sc && sc[1] == e->theta_b_sc) || (sc[0] == e->theta_b_sc && sc[1] == e->theta_a_sc)))
        return fail(IQHIP_ERR_INVALID, std::string(what) + ": theta is not resident for this branch");
    std::vector<int32_t> list;
    const size_t max_comp = class_components(e, list);
    const size_t rows = (size_t)class_lnl_part_rows(e);
    HIPCHK(e->cl.list.ensure(e, list.size()));
    HIPCHK(e->cl.cw.ensure(e, M));
    HIPCHK(e->cl.part.ensure(e, rows * 2 * M));
    HIPCHK(e->cl.out.ensure(e, 2 * M));
    std::vector<double> inv;
    if (class_invar) {   // [class][nptn] -> [class][nptn_pad], padding 0
        HIPCHK(e->cl.inv.ensure(e, M * P));
        inv.assign(M * P, 0.0);
        for (size_t m = 0; m < M; m++) memcpy(&inv[m * P], class_invar + m * N, sizeof(double) * N);
    }
    HIPCHK(hipStreamSynchronize(e->stream));   // (pageable sources, and an earlier launch may still read the buffers)
    HIPCHK(hipMemcpyAsync(e->cl.list.p, list.data(), sizeof(int32_t) * list.size(), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(e->cl.cw.p, class_weight, sizeof(double) * M, hipMemcpyHostToDevice, e->stream));
    if (class_invar) HIPCHK(hipMemcpyAsync(e->cl.inv.p, inv.data(), sizeof(double) * inv.size(), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    PhaseTimer timer(e, 1);
    timer.mark();
    HIPCHK(launch_class_lnl(e, sc[0], sc[1], len, e->cl.list.p, (int)max_comp, e->cl.cw.p, class_invar ? e->cl.inv.p : nullptr,
                            e->cl.part.p, e->cl.out.p));
    timer.mark();
    std::vector<double> res(2 * M);
    HIPCHK(hipMemcpyAsync(res.data(), e->cl.out.p, sizeof(double) * res.size(), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    timer.read(&e->cl.ms);
    for (size_t m = 0; m < M; m++) {
        lnl[m] = res[m];
        if (floored) floored[m] = (int64_t)res[M + m];
    }
    return IQHIP_OK;
}

extern "C" int iqhip_mix_weights_em(iqhip_engine *e, int max_steps, double nsites, double *weights, double *p_invar, int *nsteps,
                                    int *converged, double *trace) {
    if (!e || !weights || !nsteps || !converged) return fail(IQHIP_ERR_INVALID, "iqhip_mix_weights_em: null argument");
    int rc = require(e, "iqhip_mix_weights_em", kMixNeeds);
    if (!rc) rc = mix_class_lh_done(e, "iqhip_mix_weights_em");
    if (rc) return rc;
    if (max_steps < 1 || max_steps > IQHIP_MIX_MAX_STEPS)
        return fail(IQHIP_ERR_INVALID, "iqhip_mix_weights_em: max_steps must be 1 .. " + std::to_string(IQHIP_MIX_MAX_STEPS));
    if (!(nsites > 0.0) || !std::isfinite(nsites)) return fail(IQHIP_ERR_INVALID, "iqhip_mix_weights_em: nsites must be > 0");
    const size_t M = (size_t)e->nclass;
    static_assert(kMixEmUpdateThreads >= 96, "k_mixem_update runs one thread per class: nclass <= ncat <= 96 (iqhip_create)");
    for (size_t m = 0; m < M; m++)
        if (!(weights[m] > 0.0) || !std::isfinite(weights[m]))
            return fail(IQHIP_ERR_INVALID, "iqhip_mix_weights_em: every class weight must be > 0 and finite");
    if (p_invar && !(*p_invar >= 0.0 && *p_invar < 1.0)) return fail(IQHIP_ERR_INVALID, "iqhip_mix_weights_em: p_invar outside [0, 1)");
    HIPCHK(use_device(e));
    const bool use_inv = p_invar && *p_invar > 0.0;
    std::vector<double> st(MIXEM_HDR + 2 * M + (size_t)max_steps * (M + 1), 0.0);
    st[MIXEM_PINV] = st[MIXEM_PINV_IN] = use_inv ? *p_invar : 0.0;
    st[MIXEM_V] = 1.0;
    st[MIXEM_USE_INV] = use_inv ? 1.0 : 0.0;
    st[MIXEM_NSITES] = nsites;
    for (size_t m = 0; m < M; m++) {
        st[MIXEM_HDR + m] = 1.0;
        st[MIXEM_HDR + M + m] = weights[m];
    }
    HIPCHK(e->mix.state.ensure(e, st.size()));
    HIPCHK(e->mix.part.ensure(e, (size_t)mixem_part_rows(e) * M));
    HIPCHK(hipStreamSynchronize(e->stream));   // (pageable source)
    // (the log is not uploaded: step k writes row k before anything reads it, and only the rows below *nsteps are handed out)
    HIPCHK(hipMemcpyAsync(e->mix.state.p, st.data(), sizeof(double) * (MIXEM_HDR + 2 * M), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    // the whole loop is enqueued: the steps behind the converged one return at once
    PhaseTimer timer(e, 1);
    timer.mark();
    int64_t launches = 0;
    for (int k = 0; k < max_steps; k++) {
        HIPCHK(launch_mixem_step(e, e->mix.lc.p, e->mix.state.p, max_steps, e->mix.part.p));
        launches += 2;
    }
    timer.mark();
    HIPCHK(hipMemcpyAsync(st.data(), e->mix.state.p, sizeof(double) * st.size(), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    timer.read(&e->mix.ms[1]);
    e->mix.launches = launches;
    *nsteps = (int)st[MIXEM_STEPS];
    *converged = st[MIXEM_DONE] != 0.0 ? 1 : 0;
    memcpy(weights, &st[MIXEM_HDR + M], sizeof(double) * M);
    if (use_inv) *p_invar = st[MIXEM_PINV];
    if (trace) {
        const size_t taken = (size_t)*nsteps * (M + 1), all = (size_t)max_steps * (M + 1);
        memcpy(trace, &st[MIXEM_HDR + 2 * M], sizeof(double) * taken);
        std::fill(trace + taken, trace + all, 0.0);
    }
    return IQHIP_OK;
}

extern "C" int iqhip_mix_posteriors(iqhip_engine *e, const double *class_freq, double *post, double *state_freq) {
    if (!e || (!post && !state_freq) || (state_freq && !class_freq))
        return fail(IQHIP_ERR_INVALID, "iqhip_mix_posteriors: null argument");
    int rc = require(e, "iqhip_mix_posteriors", kMixNeeds);
    if (!rc) rc = mix_class_lh_done(e, "iqhip_mix_posteriors");
    if (rc) return rc;
    HIPCHK(use_device(e));
    const size_t P = (size_t)e->nptn_pad, M = (size_t)e->nclass, n = (size_t)e->n;
    const size_t post_doubles = post ? M * P : 0;
    HIPCHK(e->mix.post.ensure(e, post_doubles + (state_freq ? n * P : 0)));
    double *d_post = post ? e->mix.post.p : nullptr, *d_sf = state_freq ? e->mix.post.p + post_doubles : nullptr;
    if (state_freq) {
        HIPCHK(e->mix.cfreq.ensure(e, M * n));
        HIPCHK(hipStreamSynchronize(e->stream));   // (pageable source)
        HIPCHK(hipMemcpyAsync(e->mix.cfreq.p, class_freq, sizeof(double) * M * n, hipMemcpyHostToDevice, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
    }
    HIPCHK(launch_mix_posteriors(e, e->mix.lc.p, e->mix.cfreq.p, d_post, d_sf));
    if (post && (rc = fetch_transposed(e, d_post, M, post))) return rc;
    if (state_freq && (rc = fetch_transposed(e, d_sf, n, state_freq))) return rc;
    return IQHIP_OK;
}
