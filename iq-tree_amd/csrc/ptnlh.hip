// ptnlh.hip -- drivers of everything that consumes per-pattern log-likelihoods on the device: UFBoot / RELL, the store of
// per-pattern log-likelihood rows, SH-aLRT and local bootstrap, the tree topology tests, UFBoot's per-replicate bookkeeping, the EM for +R free-rate models, the
// empirical-Bayes site rates, the EM for mixture class weights and the per-class log-likelihoods.  Host code only; the kernels
// are in kernels_rell.hip, kernels_alrt.hip, kernels_topo.hip, kernels_ufboot.hip, kernels_em.hip, kernels_mixem.hip and
// kernels_classlnl.hip.
#include <float.h>
#include <stdlib.h>
#include <string.h>
#include <cmath>

#include "iqhip_internal.h"

using namespace iqhip;

// ---- consumers of the device-resident pattern lnL (kernels_rell.hip) ---------------------------
// the scale counters of a branch's two ends; a leaf carries no scaling events: nullptr
static int branch_scale_counters(iqhip_engine *e, iqhip_branch_end a, iqhip_branch_end b, const int16_t *sc[2]) {
    const iqhip_branch_end ends[2] = {a, b};
    for (int k = 0; k < 2; k++) {
        sc[k] = nullptr;
        if (ends[k].leaf >= 0) continue;
        int idx;
        const int rc = slab_for_key(e, ends[k].key, false, &idx);
        if (rc) return rc;
        sc[k] = e->slabs[idx].sc;
    }
    return IQHIP_OK;
}

static int scaled_pattern_lh(iqhip_engine *e, iqhip_branch_end a, iqhip_branch_end b) {
    const int16_t *sc[2];
    const int rc = branch_scale_counters(e, a, b, sc);
    if (rc) return rc;
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

// ---- EM for +R free-rate models, empirical-Bayes site rates (kernels_em.hip) ----------------------------------------
// plain engines of 4 / 20 / 64 states only; needs_estep: the call reads what the last E-step left
static int em_engine(iqhip_engine *e, const char *what, bool needs_theta, bool needs_estep) {
    if (e->planner) return fail(IQHIP_ERR_INVALID, std::string(what) + ": not available on a planning-only engine");
    if (!e->shards.empty() || e->comm)
        return fail(IQHIP_ERR_UNSUPPORTED, std::string(what) + ": not available on pattern-sharded engines");
    if (e->nclass > 1) return fail(IQHIP_ERR_UNSUPPORTED, std::string(what) + ": not available for mixture models");
    if (e->asc_active || e->n_unobs > 0)
        return fail(IQHIP_ERR_UNSUPPORTED, std::string(what) + ": not available with ascertainment bias correction");
    if (e->embed2 || e->n_user != e->n)
        return fail(IQHIP_ERR_UNSUPPORTED, std::string(what) + ": not available for embedded state counts");
    if (needs_theta && !e->theta_valid) return fail(IQHIP_ERR_INVALID, std::string(what) + " needs iqhip_compute_theta first");
    if (needs_estep && (!e->em.valid || e->em.w.cap < (size_t)e->ncat * (size_t)e->nptn_pad))
        return fail(IQHIP_ERR_INVALID, std::string(what) + " needs iqhip_em_posteriors first");
    return IQHIP_OK;
}

static size_t em_part_rows(const iqhip_engine *e) { return (size_t)((e->nptn_pad + 255) / 256); }

// with iqhip_timing_enable: HIP events around the launches of one call; stop() after the stream has drained
struct EmTimer {
    hipEvent_t ev[2] = {nullptr, nullptr};
    iqhip_engine *e;
    explicit EmTimer(iqhip_engine *e_) : e(e_) {
        if (e->timing && hipEventCreate(&ev[0]) == hipSuccess && hipEventCreate(&ev[1]) == hipSuccess) hipEventRecord(ev[0], e->stream);
    }
    void mark() { if (ev[1]) hipEventRecord(ev[1], e->stream); }
    void stop(double *ms) {
        float t = 0.0f;
        if (ev[1] && hipEventElapsedTime(&t, ev[0], ev[1]) == hipSuccess) *ms = t;
    }
    ~EmTimer() {
        for (hipEvent_t x : ev) if (x) hipEventDestroy(x);
    }
};

extern "C" int iqhip_debug_em_timing(iqhip_engine *e, double *ms) {
    if (!e || !ms) return fail(IQHIP_ERR_INVALID, "iqhip_debug_em_timing: null argument");
    ms[0] = e->em.ms[0];
    ms[1] = e->em.ms[1];
    return IQHIP_OK;
}

extern "C" int iqhip_em_posteriors(iqhip_engine *e, double len, double *cat_sum) {
    if (!e || !cat_sum) return fail(IQHIP_ERR_INVALID, "iqhip_em_posteriors: null argument");
    int rc = em_engine(e, "iqhip_em_posteriors", true, false);
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
    EmTimer timer(e);
    HIPCHK(launch_em_posteriors(e, len, e->em.w.p, e->em.rate.p, e->em.cat.p, e->em.part.p, e->em.out.p));
    timer.mark();
    HIPCHK(hipMemcpyAsync(cat_sum, e->em.out.p, sizeof(double) * C, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    timer.stop(&e->em.ms[0]);
    e->em.valid = true;
    return IQHIP_OK;
}

extern "C" int iqhip_em_fetch_posteriors(iqhip_engine *e, double *out) {
    if (!e || !out) return fail(IQHIP_ERR_INVALID, "iqhip_em_fetch_posteriors: null argument");
    int rc = em_engine(e, "iqhip_em_fetch_posteriors", false, true);
    if (rc) return rc;
    HIPCHK(use_device(e));
    const size_t P = (size_t)e->nptn_pad, C = (size_t)e->ncat, N = (size_t)e->nptn;
    std::vector<double> w(C * P);
    HIPCHK(hipMemcpyAsync(w.data(), e->em.w.p, sizeof(double) * w.size(), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    for (size_t p = 0; p < N; p++)
        for (size_t c = 0; c < C; c++) out[p * C + c] = w[c * P + p];
    return IQHIP_OK;
}

extern "C" int iqhip_em_site_rates(iqhip_engine *e, double *ptn_rate, int32_t *ptn_cat) {
    if (!e || !ptn_rate || !ptn_cat) return fail(IQHIP_ERR_INVALID, "iqhip_em_site_rates: null argument");
    int rc = em_engine(e, "iqhip_em_site_rates", false, true);
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
    int rc = em_engine(e, "iqhip_em_objective", true, true);
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
    EmTimer timer(e);
    HIPCHK(launch_em_objective(e, sc[0], sc[1], len, e->em.w.p, e->em.part.p, e->em.out.p));
    timer.mark();
    std::vector<double> res(2 * C);
    HIPCHK(hipMemcpyAsync(res.data(), e->em.out.p, sizeof(double) * res.size(), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    timer.stop(&e->em.ms[1]);
    for (size_t c = 0; c < C; c++) {
        f[c] = res[c];
        if (floored) floored[c] = (int64_t)res[C + c];
    }
    return IQHIP_OK;
}

// ---- EM for mixture class weights, class posteriors, pattern state frequencies (kernels_mixem.hip) -------------------
// plain mixture engines of 4 / 20 / 64 states only; needs_lc: the call reads what the last iqhip_mix_class_lh left
static int mix_engine(iqhip_engine *e, const char *what, bool needs_lc) {
    if (e->planner) return fail(IQHIP_ERR_INVALID, std::string(what) + ": not available on a planning-only engine");
    if (!e->shards.empty() || e->comm)
        return fail(IQHIP_ERR_UNSUPPORTED, std::string(what) + ": not available on pattern-sharded engines");
    if (e->asc_active || e->n_unobs > 0)
        return fail(IQHIP_ERR_UNSUPPORTED, std::string(what) + ": mixture models with ascertainment bias correction are not supported");
    if (e->embed2 || e->n_user != e->n)
        return fail(IQHIP_ERR_UNSUPPORTED, std::string(what) + ": not available for embedded state counts");
    if (e->nclass < 2) return fail(IQHIP_ERR_UNSUPPORTED, std::string(what) + ": the model is no mixture (one class)");
    if (needs_lc && (e->mix.model_version != e->model_version || e->mix.nptn_pad != e->nptn_pad || e->mix.nclass != e->nclass ||
                     e->mix.lc.cap < (size_t)e->nclass * (size_t)e->nptn_pad))
        return fail(IQHIP_ERR_INVALID, std::string(what) + " needs iqhip_mix_class_lh first (again after every model change)");
    return IQHIP_OK;
}

// rows [nrows][nptn_pad] on the device -> out [nptn][nrows] on the host
static int mix_fetch_transposed(iqhip_engine *e, const double *d_rows, size_t nrows, double *out) {
    const size_t P = (size_t)e->nptn_pad, N = (size_t)e->nptn;
    std::vector<double> rows(nrows * P);
    HIPCHK(hipMemcpyAsync(rows.data(), d_rows, sizeof(double) * rows.size(), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    for (size_t p = 0; p < N; p++)
        for (size_t r = 0; r < nrows; r++) out[p * nrows + r] = rows[r * P + p];
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
    if (!e) return fail(IQHIP_ERR_INVALID, "iqhip_mix_class_lh: null argument");
    int rc = mix_engine(e, "iqhip_mix_class_lh", false);
    if (rc) return rc;
    if (!e->theta_valid) return fail(IQHIP_ERR_INVALID, "iqhip_mix_class_lh needs iqhip_compute_theta first");
    if (!(len >= 0.0)) return fail(IQHIP_ERR_INVALID, "iqhip_mix_class_lh: negative or NaN branch length");
    HIPCHK(use_device(e));
    const size_t P = (size_t)e->nptn_pad, M = (size_t)e->nclass, C = (size_t)e->ncat;
    // the components of every class in ascending order: cat_class is an arbitrary map
    std::vector<int32_t> list(M + 1 + C);
    size_t at = 0;
    for (size_t m = 0; m < M; m++) {
        list[m] = (int32_t)at;
        for (size_t c = 0; c < C; c++)
            if ((size_t)e->h_cls[c] == m) list[M + 1 + at++] = (int32_t)c;
    }
    list[M] = (int32_t)at;
    e->mix.model_version = 0;
    HIPCHK(e->mix.lc.ensure(e, M * P));
    HIPCHK(e->mix.list.ensure(e, list.size()));
    HIPCHK(hipStreamSynchronize(e->stream));   // (pageable source, and an earlier launch may still read the list)
    HIPCHK(hipMemcpyAsync(e->mix.list.p, list.data(), sizeof(int32_t) * list.size(), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    EmTimer timer(e);
    HIPCHK(launch_mix_class_lh(e, len, e->mix.list.p, e->mix.lc.p));
    timer.mark();
    HIPCHK(hipStreamSynchronize(e->stream));
    timer.stop(&e->mix.ms[0]);
    e->mix.model_version = e->model_version;
    e->mix.nptn_pad = e->nptn_pad;
    e->mix.nclass = e->nclass;
    return out ? mix_fetch_transposed(e, e->mix.lc.p, M, out) : IQHIP_OK;
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
    if (e->planner) return fail(IQHIP_ERR_INVALID, std::string(what) + ": not available on a planning-only engine");
    if (!e->shards.empty() || e->comm)
        return fail(IQHIP_ERR_UNSUPPORTED, std::string(what) + ": not available on pattern-sharded engines");
    if (e->asc_active || e->n_unobs > 0)
        return fail(IQHIP_ERR_UNSUPPORTED, std::string(what) + ": not available with ascertainment bias correction");
    if (e->embed2 || e->n_user != e->n)
        return fail(IQHIP_ERR_UNSUPPORTED, std::string(what) + ": not available for embedded state counts");
    if (!e->model_set || !e->mixture_api)
        return fail(IQHIP_ERR_UNSUPPORTED, std::string(what) + ": the model was not set through iqhip_set_mixture_model");
    if (!e->theta_valid) return fail(IQHIP_ERR_INVALID, std::string(what) + " needs iqhip_compute_theta first");
    if (!(len >= 0.0)) return fail(IQHIP_ERR_INVALID, std::string(what) + ": negative or NaN branch length");
    const size_t P = (size_t)e->nptn_pad, N = (size_t)e->nptn, M = (size_t)e->nclass, C = (size_t)e->ncat;
    for (size_t m = 0; m < M; m++)
        if (!(class_weight[m] > 0.0) || !std::isfinite(class_weight[m]))
            return fail(IQHIP_ERR_INVALID, std::string(what) + ": every class weight must be > 0 and finite");
    HIPCHK(use_device(e));
    const int16_t *sc[2];
    int rc = branch_scale_counters(e, a, b, sc);
    if (rc) return rc;
    // theta remembers the scale counters of the ends it was built from (either order: build_branch puts a leaf first)
    if (!((sc[0] == e->theta_a_sc && sc[1] == e->theta_b_sc) || (sc[0] == e->theta_b_sc && sc[1] == e->theta_a_sc)))
        return fail(IQHIP_ERR_INVALID, std::string(what) + ": theta is not resident for this branch");
    // the components of every class in ascending order, as iqhip_mix_class_lh
    std::vector<int32_t> list(M + 1 + C);
    size_t at = 0, max_comp = 0;
    for (size_t m = 0; m < M; m++) {
        list[m] = (int32_t)at;
        for (size_t c = 0; c < C; c++)
            if ((size_t)e->h_cls[c] == m) list[M + 1 + at++] = (int32_t)c;
        max_comp = std::max(max_comp, at - (size_t)list[m]);
    }
    list[M] = (int32_t)at;
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
    EmTimer timer(e);
    HIPCHK(launch_class_lnl(e, sc[0], sc[1], len, e->cl.list.p, (int)max_comp, e->cl.cw.p, class_invar ? e->cl.inv.p : nullptr,
                            e->cl.part.p, e->cl.out.p));
    timer.mark();
    std::vector<double> res(2 * M);
    HIPCHK(hipMemcpyAsync(res.data(), e->cl.out.p, sizeof(double) * res.size(), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    timer.stop(&e->cl.ms);
    for (size_t m = 0; m < M; m++) {
        lnl[m] = res[m];
        if (floored) floored[m] = (int64_t)res[M + m];
    }
    return IQHIP_OK;
}

extern "C" int iqhip_mix_weights_em(iqhip_engine *e, int max_steps, double nsites, double *weights, double *p_invar, int *nsteps,
                                    int *converged, double *trace) {
    if (!e || !weights || !nsteps || !converged) return fail(IQHIP_ERR_INVALID, "iqhip_mix_weights_em: null argument");
    int rc = mix_engine(e, "iqhip_mix_weights_em", true);
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
    EmTimer timer(e);
    int64_t launches = 0;
    for (int k = 0; k < max_steps; k++) {
        HIPCHK(launch_mixem_step(e, e->mix.lc.p, e->mix.state.p, max_steps, e->mix.part.p));
        launches += 2;
    }
    timer.mark();
    HIPCHK(hipMemcpyAsync(st.data(), e->mix.state.p, sizeof(double) * st.size(), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    timer.stop(&e->mix.ms[1]);
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
    int rc = mix_engine(e, "iqhip_mix_posteriors", true);
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
    if (post && (rc = mix_fetch_transposed(e, d_post, M, post))) return rc;
    if (state_freq && (rc = mix_fetch_transposed(e, d_sf, n, state_freq))) return rc;
    return IQHIP_OK;
}

// replaces the sample matrix by one of nsamples rows (0: none) once the engine's stream has drained; contents undefined
static hipError_t boot_matrix(iqhip_engine *e, int nsamples) {
    hipError_t s = hipStreamSynchronize(e->stream);
    if (s == hipSuccess && e->d_boot) s = hipFree(e->d_boot);
    if (s != hipSuccess) return s;
    e->d_boot = nullptr;
    e->nboot = 0;
    e->ufb.nsamples = 0;   // (the UFBoot state belongs to the matrix it was initialised on)
    if (nsamples == 0) return hipSuccess;
    if ((s = dmalloc(&e->d_boot, (size_t)e->nptn_pad * nsamples)) == hipSuccess) e->nboot = nsamples;
    return s;
}

extern "C" int iqhip_set_boot_samples(iqhip_engine *e, const float *samples, int nsamples) {
    if (!e || (nsamples > 0 && !samples) || nsamples < 0) return fail(IQHIP_ERR_INVALID, "bad bootstrap samples");
    if (nsamples > 16384) return fail(IQHIP_ERR_INVALID, "at most 16384 bootstrap samples");
    if (!e->shards.empty()) return sharded::set_boot_samples(e, samples, nsamples);
    HIPCHK(use_device(e));
    HIPCHK(boot_matrix(e, nsamples));
    if (nsamples == 0) return IQHIP_OK;
    const size_t pitch = (size_t)e->nptn_pad;
    HIPCHK(hipMemset(e->d_boot, 0, sizeof(float) * pitch * nsamples));
    HIPCHK(hipMemcpy2D(e->d_boot, pitch * sizeof(float), samples, (size_t)e->nptn * sizeof(float),
                       (size_t)e->nptn * sizeof(float), nsamples, hipMemcpyHostToDevice));
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

// every row of a list lies inside the store
static int ptnlh_check_rows(iqhip_engine *e, const char *what, const int32_t *rows, int nrows, const char *hint = "") {
    for (int i = 0; i < nrows; i++)
        if (rows[i] < 0 || rows[i] >= e->ptnlh_rows)
            return fail(IQHIP_ERR_INVALID, std::string(what) + ": row outside the store" + hint);
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
    rc = ptnlh_check_rows(e, "iqhip_ptnlh_put_current", &row, 1, " (iqhip_ptnlh_reserve)");
    if (rc) return rc;
    HIPCHK(use_device(e));
    const int16_t *sc[2];
    rc = branch_scale_counters(e, a, b, sc);
    if (rc) return rc;
    HIPCHK(launch_pattern_lh_scaled(e, sc[0], sc[1], e->d_ptnlh + (size_t)row * e->nptn_pad));
    return IQHIP_OK;
}

extern "C" int iqhip_ptnlh_fetch(iqhip_engine *e, int row, double *out) {
    int rc = ptnlh_plain_engine(e, "iqhip_ptnlh_fetch");
    if (rc) return rc;
    if (!out) return fail(IQHIP_ERR_INVALID, "iqhip_ptnlh_fetch: null argument");
    rc = ptnlh_check_rows(e, "iqhip_ptnlh_fetch", &row, 1);
    if (rc) return rc;
    HIPCHK(use_device(e));
    HIPCHK(hipMemcpyAsync(out, e->d_ptnlh + (size_t)row * e->nptn_pad, sizeof(double) * (size_t)e->nptn, hipMemcpyDeviceToHost,
                          e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return IQHIP_OK;
}

// the distinct rows of a row list in first-appearance order (list[0, M)) and, behind them, every entry's index into them
struct RowList {
    std::vector<int32_t> list;
    int M;
};
static RowList row_list(const int32_t *rows, int nrows) {
    RowList rl;
    std::vector<int32_t> idx((size_t)nrows);
    std::unordered_map<int32_t, int32_t> seen;
    for (int i = 0; i < nrows; i++) {
        const auto at = seen.emplace(rows[i], (int32_t)rl.list.size());
        if (at.second) rl.list.push_back(rows[i]);
        idx[i] = at.first->second;
    }
    rl.M = (int)rl.list.size();
    rl.list.insert(rl.list.end(), idx.begin(), idx.end());
    return rl;
}

// the list into bt.rows; bt.part and bt.sums sized for products of its distinct rows with nsamples replicates
static int bt_stage(iqhip_engine *e, const RowList &rl, int ksplit, size_t nsamples) {
    const size_t sums = (size_t)rl.M * nsamples;
    HIPCHK(e->bt.rows.ensure(e, rl.list.size()));
    HIPCHK(e->bt.part.ensure(e, sums * ksplit));
    HIPCHK(e->bt.sums.ensure(e, sums));
    HIPCHK(hipStreamSynchronize(e->stream));   // (pageable source: the copy below must not outlive the list)
    HIPCHK(hipMemcpyAsync(e->bt.rows.p, rl.list.data(), sizeof(int32_t) * rl.list.size(), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return IQHIP_OK;
}

// the product R = L W^T of a row list's distinct rows ends in bt.sums [M][nsamples]; bt.rows holds the list
static int ptnlh_product(iqhip_engine *e, const char *what, const int32_t *rows, int nrows, int nsamples, RowList *rl) {
    if (nsamples < 1 || nsamples > e->nboot)
        return fail(IQHIP_ERR_INVALID, std::string(what) + (e->nboot == 0 ? ": no bootstrap samples (iqhip_set_boot_samples)"
                                                                          : ": more replicates than uploaded samples"));
    int rc = ptnlh_check_rows(e, what, rows, nrows);
    if (rc) return rc;
    *rl = row_list(rows, nrows);
    HIPCHK(use_device(e));
    const int ksplit = alrt_ksplit(e, rl->M, nsamples);
    rc = bt_stage(e, *rl, ksplit, (size_t)nsamples);
    if (rc) return rc;
    HIPCHK(launch_alrt_product(e, e->bt.rows.p, rl->M, nsamples, ksplit, e->bt.part.p, e->bt.sums.p));
    return IQHIP_OK;
}

extern "C" int iqhip_ptnlh_rell(iqhip_engine *e, const int32_t *rows, int nrows, int nsamples, double *out) {
    int rc = ptnlh_plain_engine(e, "iqhip_ptnlh_rell");
    if (rc) return rc;
    if (!rows || !out || nrows < 1) return fail(IQHIP_ERR_INVALID, "iqhip_ptnlh_rell: bad row list");
    RowList rl;
    rc = ptnlh_product(e, "iqhip_ptnlh_rell", rows, nrows, nsamples, &rl);
    if (rc) return rc;
    std::vector<double> sums((size_t)rl.M * nsamples);
    HIPCHK(hipMemcpyAsync(sums.data(), e->bt.sums.p, sizeof(double) * sums.size(), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    const int32_t *idx = rl.list.data() + rl.M;
    for (int i = 0; i < nrows; i++)
        memcpy(out + (size_t)i * nsamples, sums.data() + (size_t)idx[i] * nsamples, sizeof(double) * (size_t)nsamples);
    return IQHIP_OK;
}

extern "C" int iqhip_branch_tests(iqhip_engine *e, const int32_t *rows3, const double *lh3, int nbranch, int reps_sh,
                                  int reps_lbp, iqhip_branch_support *out) {
    int rc = ptnlh_plain_engine(e, "iqhip_branch_tests");
    if (rc) return rc;
    if (!rows3 || !lh3 || !out || nbranch < 1 || nbranch > (1 << 24) || reps_sh < 0 || reps_lbp < 0)
        return fail(IQHIP_ERR_INVALID, "iqhip_branch_tests: bad arguments");
    const int times = std::max(reps_sh, reps_lbp);
    RowList rl;
    rc = ptnlh_product(e, "iqhip_branch_tests", rows3, 3 * nbranch, times, &rl);
    if (rc) return rc;
    HIPCHK(e->bt.out.ensure(e, (size_t)7 * nbranch));
    HIPCHK(hipStreamSynchronize(e->stream));
    HIPCHK(hipMemcpyAsync(e->bt.out.p, lh3, sizeof(double) * 3 * (size_t)nbranch, hipMemcpyHostToDevice, e->stream));
    double *d_res = e->bt.out.p + 3 * (size_t)nbranch;
    HIPCHK(launch_alrt_stats(e, e->bt.rows.p + rl.M, e->bt.out.p, nbranch, times, e->bt.sums.p, d_res));
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
    rc = ptnlh_check_rows(e, "iqhip_ptnlh_upload", &row, 1, " (iqhip_ptnlh_reserve)");
    if (rc) return rc;
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
    const hipError_t s = boot_matrix(e, nsamples);
    if (s == hipErrorOutOfMemory) return fail(IQHIP_ERR_NOMEM, "bootstrap sample matrix: out of device memory");
    HIPCHK(s);
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
    e->ufb.nsamples = 0;   // (new content, even where the matrix keeps its size)
    rc = topo_boot_rows(e, nsamples, true);
    if (rc) return rc;
    HIPCHK(launch_topo_gen(e, nsamples, first_replicate, ndraws, topo_stream_key(seed, stream)));
    HIPCHK(hipStreamSynchronize(e->stream));
    return IQHIP_OK;
}

// variances of all pairs of the row list -> host [nrows][nrows] (uses bt.rows for the list)
static int topo_diff_variance(iqhip_engine *e, const char *what, const int32_t *rows, int nrows, double *var) {
    int rc = topo_freq_prefix(e, what);
    if (rc) return rc;
    const size_t nn = (size_t)nrows * nrows;
    HIPCHK(e->bt.rows.ensure(e, (size_t)nrows));
    HIPCHK(e->tt.var.ensure(e, nn));
    HIPCHK(hipStreamSynchronize(e->stream));
    HIPCHK(hipMemcpyAsync(e->bt.rows.p, rows, sizeof(int32_t) * (size_t)nrows, hipMemcpyHostToDevice, e->stream));
    HIPCHK(launch_topo_diff_variance(e, e->bt.rows.p, nrows, e->tt.var.p));
    HIPCHK(hipMemcpyAsync(var, e->tt.var.p, sizeof(double) * nn, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return IQHIP_OK;
}

extern "C" int iqhip_ptnlh_diff_variance(iqhip_engine *e, const int32_t *rows, int nrows, double *var) {
    int rc = ptnlh_plain_engine(e, "iqhip_ptnlh_diff_variance");
    if (rc) return rc;
    if (!rows || !var || nrows < 1 || nrows > 4096) return fail(IQHIP_ERR_INVALID, "iqhip_ptnlh_diff_variance: bad row list");
    rc = ptnlh_check_rows(e, "iqhip_ptnlh_diff_variance", rows, nrows);
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
    rc = ptnlh_check_rows(e, "iqhip_tree_tests", rows, ntrees);
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
    RowList rl;
    rc = ptnlh_product(e, "iqhip_tree_tests", rows, ntrees, nsamples, &rl);
    if (rc) return rc;
    HIPCHK(e->tt.dbl.ensure(e, hd.size() + 3 * S + 6 * T));
    HIPCHK(e->tt.ints.ensure(e, 2 * T + S));
    HIPCHK(hipStreamSynchronize(e->stream));
    double *const d_dbl = e->tt.dbl.p;
    int32_t *const d_int = e->tt.ints.p;
    HIPCHK(hipMemcpyAsync(d_dbl, hd.data(), sizeof(double) * hd.size(), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(d_int, hi.data(), sizeof(int32_t) * hi.size(), hipMemcpyHostToDevice, e->stream));
    TopoTestArgs a;
    a.sums = e->bt.sums.p;
    a.idx = e->bt.rows.p + rl.M;
    a.T = ntrees;
    a.S = nsamples;
    a.epsilon = epsilon;
    a.tie_key = topo_stream_key(tie_seed, 0xB9u);
    a.lh = d_dbl;
    a.avg = d_dbl + T;
    a.w_orig = d_dbl + 2 * T;
    a.weights = weighted ? d_dbl + 3 * T : nullptr;
    a.max_sh = d_dbl + hd.size();
    a.max_elw = a.max_sh + S;
    a.sum_l = a.max_elw + S;
    a.out = a.sum_l + S;
    a.kh_id = d_int;
    a.w_id = d_int + T;
    a.winner = d_int + 2 * T;
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
    rc = ptnlh_check_rows(e, "iqhip_multiscale_bp", rows, ntrees);
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
    const RowList rl = row_list(rows, ntrees);
    // replicates per chunk: the sample matrix stays within 256 MB; IQHIP_BOOT_CHUNK (read per call) overrides.  The K-split
    // follows from the pattern count and the CU count alone (the budget's chunk, not this call's), so that a (row,
    // replicate) sum has the same bits whatever the chunk size
    const int64_t budget = std::max<int64_t>(1, std::min<int64_t>(16384, ((int64_t)256 << 20) / (4 * e->nptn_pad)));
    const int ksplit = alrt_ksplit(e, rl.M, (int)budget);
    int64_t chunk = budget;
    if (const char *bc = getenv("IQHIP_BOOT_CHUNK")) chunk = std::max(1, std::min(16384, atoi(bc)));
    chunk = std::min<int64_t>(chunk, nsamples);
    e->ufb.nsamples = 0;   // (the matrix is overwritten chunk by chunk)
    rc = topo_boot_rows(e, (int)chunk, false);
    if (rc) return rc;
    const size_t ncount = (size_t)nscales * ntrees;
    HIPCHK(e->tt.ints.ensure(e, ncount));
    rc = bt_stage(e, rl, ksplit, (size_t)chunk);
    if (rc) return rc;
    uint32_t *d_counts = reinterpret_cast<uint32_t *>(e->tt.ints.p);
    HIPCHK(hipMemsetAsync(d_counts, 0, sizeof(uint32_t) * ncount, e->stream));
    for (int k = 0; k < nscales; k++) {
        const uint64_t key = topo_stream_key(seed, (uint32_t)k);
        for (int64_t first = 0; first < nsamples; first += chunk) {
            const int n = (int)std::min<int64_t>(chunk, nsamples - first);
            HIPCHK(launch_topo_gen(e, n, first, ndraws[k], key));
            HIPCHK(launch_alrt_product(e, e->bt.rows.p, rl.M, n, ksplit, e->bt.part.p, e->bt.sums.p));
            HIPCHK(launch_topo_argmax(e, e->bt.sums.p, e->bt.rows.p + rl.M, ntrees, n, d_counts + (size_t)k * ntrees));
        }
    }
    std::vector<uint32_t> counts(ncount);
    HIPCHK(hipMemcpyAsync(counts.data(), d_counts, sizeof(uint32_t) * ncount, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    for (size_t i = 0; i < ncount; i++) bp[i] = (double)counts[i] / nsamples;
    return IQHIP_OK;
}

// ---- ultrafast bootstrap: saveCurrentTree's per-replicate bookkeeping (iqtree.cpp:2676-2786; kernels_ufboot.hip) -----------
extern "C" int iqhip_ufboot_init(iqhip_engine *e, int nsamples) {
    int rc = ptnlh_plain_engine(e, "iqhip_ufboot_init");
    if (rc) return rc;
    if (nsamples < 1 || nsamples > e->nboot)
        return fail(IQHIP_ERR_INVALID, e->nboot == 0 ? "iqhip_ufboot_init: no bootstrap samples (iqhip_gen_boot_samples / iqhip_set_boot_samples)"
                                                     : "iqhip_ufboot_init: nsamples must be 1 .. the number of uploaded samples");
    HIPCHK(use_device(e));
    const size_t S = (size_t)nsamples;
    e->ufb.nsamples = 0;
    HIPCHK(e->ufb.dbl.ensure(e, 2 * S));
    HIPCHK(e->ufb.tree.ensure(e, S));
    HIPCHK(e->ufb.counts.ensure(e, S));
    HIPCHK(e->ufb.res.ensure(e, 1 + (size_t)ufboot_workgroups(nsamples)));
    // iqtree.cpp:308-312
    std::vector<double> lo(2 * S, -DBL_MAX);
    std::vector<int64_t> none(S, -1);
    HIPCHK(hipStreamSynchronize(e->stream));   // (pageable sources)
    HIPCHK(hipMemcpyAsync(e->ufb.dbl.p, lo.data(), sizeof(double) * lo.size(), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(e->ufb.tree.p, none.data(), sizeof(int64_t) * S, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemsetAsync(e->ufb.counts.p, 0, sizeof(int32_t) * S, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    e->ufb.nsamples = nsamples;
    e->ufb.ms[0] = e->ufb.ms[1] = 0.0;
    e->ufb.launches = 0;
    return IQHIP_OK;
}

// the state exists and still belongs to the sample matrix
static int ufboot_ready(iqhip_engine *e, const char *what) {
    if (e->ufb.nsamples < 1 || e->ufb.nsamples > e->nboot)
        return fail(IQHIP_ERR_INVALID, std::string(what) + " needs iqhip_ufboot_init first (again after the sample matrix was replaced)");
    return IQHIP_OK;
}

extern "C" int iqhip_ufboot_update(iqhip_engine *e, const iqhip_ufboot_tree *trees, int ntrees, double epsilon, double logl_cutoff,
                                   int64_t *counts, double *min_orig_logl) {
    const char *what = "iqhip_ufboot_update";
    int rc = ptnlh_plain_engine(e, what);
    if (rc) return rc;
    if (!trees || ntrees < 1) return fail(IQHIP_ERR_INVALID, std::string(what) + ": bad tree list");
    if (!(epsilon >= 0.0)) return fail(IQHIP_ERR_INVALID, std::string(what) + ": epsilon must be >= 0");
    if ((rc = ufboot_ready(e, what))) return rc;
    static_assert(sizeof(iqhip_ufboot_tree) == 32, "iqhip_ufboot_tree is 32 bytes");
    for (int i = 0; i < ntrees; i++) {
        const iqhip_ufboot_tree &t = trees[i];
        if (t.row < 0 || t.row >= e->ptnlh_rows) return fail(IQHIP_ERR_INVALID, std::string(what) + ": row outside the store");
        if (t.tree_id < 0) return fail(IQHIP_ERR_INVALID, std::string(what) + ": tree_id must be >= 0");
        if (!(t.rand >= 0.0 && t.rand <= 1.0)) return fail(IQHIP_ERR_INVALID, std::string(what) + ": rand outside [0, 1]");
        if (!std::isfinite(t.logl)) return fail(IQHIP_ERR_INVALID, std::string(what) + ": log-likelihoods must be finite");
    }
    // iqtree.cpp:2678
    std::vector<iqhip_ufboot_tree> ent;
    ent.reserve((size_t)ntrees);
    for (int i = 0; i < ntrees; i++)
        if (!(logl_cutoff != 0.0 && trees[i].logl < logl_cutoff - 1.0)) ent.push_back(trees[i]);
    const int n = (int)ent.size(), S = e->ufb.nsamples;
    HIPCHK(use_device(e));
    // entries per chunk: part [ksplit][M][S] and sums [M][S] of M <= chunk distinct rows within 256 MB.  The K-split follows
    // from nsamples, the pattern count and the CU count alone, so a (row, replicate) sum has the same bits whatever the chunk
    const int ksplit = alrt_ksplit(e, 1, S);
    int64_t chunk = std::max<int64_t>(1, ((int64_t)256 << 20) / ((int64_t)sizeof(double) * S * (ksplit + 1)));
    if (const char *uc = getenv("IQHIP_UFBOOT_CHUNK")) chunk = std::max(1, atoi(uc));
    chunk = std::min<int64_t>(chunk, std::max(n, 1));
    // every chunk's row list, and the entries with `row` rewritten to the row of their chunk's sums
    std::vector<RowList> lists;
    std::vector<int32_t> rows((size_t)chunk);
    for (int first = 0; first < n; first += (int)chunk) {
        const int m = (int)std::min<int64_t>(chunk, n - first);
        for (int i = 0; i < m; i++) rows[i] = ent[first + i].row;
        lists.push_back(row_list(rows.data(), m));
        const int32_t *idx = lists.back().list.data() + lists.back().M;
        for (int i = 0; i < m; i++) ent[first + i].row = idx[i];
    }
    const size_t nwg = (size_t)ufboot_workgroups(S);
    HIPCHK(e->ufb.entries.ensure(e, (size_t)std::max(n, 1)));
    HIPCHK(e->ufb.res.ensure(e, 1 + nwg));
    HIPCHK(hipStreamSynchronize(e->stream));   // (pageable source, and an earlier launch may still read the entries)
    if (n > 0)
        HIPCHK(hipMemcpyAsync(e->ufb.entries.p, ent.data(), sizeof(iqhip_ufboot_tree) * (size_t)n, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemsetAsync(e->ufb.res.p, 0, sizeof(double), e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    unsigned long long *d_replaced = reinterpret_cast<unsigned long long *>(e->ufb.res.p);
    double *boot_logl = e->ufb.dbl.p, *boot_orig = e->ufb.dbl.p + S;
    // with iqhip_timing_enable: three events per chunk (before the product, between, behind the update)
    std::vector<hipEvent_t> ev;
    auto mark = [&]() {
        if (!e->timing) return;
        hipEvent_t x = nullptr;
        if (hipEventCreate(&x) == hipSuccess) {
            hipEventRecord(x, e->stream);
            ev.push_back(x);
        }
    };
    int64_t launches = 0;
    hipError_t s = hipSuccess;
    if (n == 0) {   // everything fell to the cutoff: the state is only read for its minimum
        s = launch_ufboot_update(e, nullptr, S, e->ufb.entries.p, 0, epsilon, boot_logl, boot_orig, e->ufb.counts.p, e->ufb.tree.p,
                                 d_replaced, e->ufb.res.p + 1);
        launches = 1;
    }
    for (size_t c = 0, first = 0; c < lists.size() && s == hipSuccess && rc == IQHIP_OK; c++) {
        const RowList &rl = lists[c];
        const int m = (int)(rl.list.size() - (size_t)rl.M);
        if ((rc = bt_stage(e, rl, ksplit, (size_t)S))) break;
        mark();
        s = launch_alrt_product(e, e->bt.rows.p, rl.M, S, ksplit, e->bt.part.p, e->bt.sums.p);
        mark();
        if (s == hipSuccess)
            s = launch_ufboot_update(e, e->bt.sums.p, S, e->ufb.entries.p + first, m, epsilon, boot_logl, boot_orig,
                                     e->ufb.counts.p, e->ufb.tree.p, d_replaced, e->ufb.res.p + 1);
        mark();
        launches += 3;
        first += (size_t)m;
    }
    std::vector<double> res(1 + nwg);
    if (s == hipSuccess && rc == IQHIP_OK)
        s = hipMemcpyAsync(res.data(), e->ufb.res.p, sizeof(double) * res.size(), hipMemcpyDeviceToHost, e->stream);
    const hipError_t drained = hipStreamSynchronize(e->stream);
    if (s == hipSuccess) s = drained;
    double ms[2] = {0.0, 0.0};
    for (size_t k = 0; k + 2 < ev.size() && ev.size() % 3 == 0; k += 3)
        for (int h = 0; h < 2; h++) {
            float t = 0.0f;
            if (hipEventElapsedTime(&t, ev[k + h], ev[k + h + 1]) == hipSuccess) ms[h] += t;
        }
    for (hipEvent_t x : ev) hipEventDestroy(x);
    if (rc) return rc;
    HIPCHK(s);
    e->ufb.ms[0] = ms[0];
    e->ufb.ms[1] = ms[1];
    e->ufb.launches = launches;
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

extern "C" int iqhip_ufboot_fetch(iqhip_engine *e, double *boot_logl, double *boot_orig_logl, int32_t *boot_counts,
                                  int64_t *boot_tree) {
    int rc = ptnlh_plain_engine(e, "iqhip_ufboot_fetch");
    if (rc) return rc;
    if ((rc = ufboot_ready(e, "iqhip_ufboot_fetch"))) return rc;
    HIPCHK(use_device(e));
    const size_t S = (size_t)e->ufb.nsamples;
    if (boot_logl) HIPCHK(hipMemcpyAsync(boot_logl, e->ufb.dbl.p, sizeof(double) * S, hipMemcpyDeviceToHost, e->stream));
    if (boot_orig_logl) HIPCHK(hipMemcpyAsync(boot_orig_logl, e->ufb.dbl.p + S, sizeof(double) * S, hipMemcpyDeviceToHost, e->stream));
    if (boot_counts) HIPCHK(hipMemcpyAsync(boot_counts, e->ufb.counts.p, sizeof(int32_t) * S, hipMemcpyDeviceToHost, e->stream));
    if (boot_tree) HIPCHK(hipMemcpyAsync(boot_tree, e->ufb.tree.p, sizeof(int64_t) * S, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return IQHIP_OK;
}

extern "C" int iqhip_debug_ufboot_timing(iqhip_engine *e, double *ms, int64_t *launches) {
    int rc = ptnlh_plain_engine(e, "iqhip_debug_ufboot_timing");
    if (rc) return rc;
    if (!ms) return fail(IQHIP_ERR_INVALID, "iqhip_debug_ufboot_timing: null argument");
    ms[0] = e->ufb.ms[0];
    ms[1] = e->ufb.ms[1];
    if (launches) *launches = e->ufb.launches;
    return IQHIP_OK;
}
