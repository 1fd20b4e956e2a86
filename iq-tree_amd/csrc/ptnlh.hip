// ptnlh.hip -- drivers of everything that consumes per-pattern log-likelihoods on the device: the scaled pattern-lh fetches,
// the bootstrap sample matrix and RELL, the store of per-pattern log-likelihood rows, SH-aLRT and local bootstrap and the
// tree topology tests.  Host code only; the kernels are in kernels_rell.hip, kernels_alrt.hip and kernels_topo.hip.  (What
// consumes theta per class is in classlh.hip, UFBoot's per-replicate bookkeeping on the rows in ufboot.hip.)
#include <float.h>
#include <stdlib.h>
#include <string.h>
#include <cmath>

#include "iqhip_internal.h"

using namespace iqhip;

// ---- consumers of the device-resident pattern lnL (kernels_rell.hip) ---------------------------
int iqhip::branch_scale_counters(iqhip_engine *e, iqhip_branch_end a, iqhip_branch_end b, const int16_t *sc[2]) {
    const iqhip_branch_end ends[2] = {a, b};
    for (int k = 0; k < 2; k++) {
        sc[k] = nullptr;
        if (ends[k].leaf >= 0) continue;
        int idx;
        const int rc = slab_for_key(e, ends[k].key, false, &idx);
        if (rc) return rc;
        sc[k] = e->slabs[idx].sc.p;
    }
    return IQHIP_OK;
}

static int scaled_pattern_lh(iqhip_engine *e, iqhip_branch_end a, iqhip_branch_end b) {
    const int16_t *sc[2];
    const int rc = branch_scale_counters(e, a, b, sc);
    if (rc) return rc;
    HIPCHK(e->d_ptn_scaled.ensure(e, (size_t)e->nptn_pad));
    HIPCHK(launch_pattern_lh_scaled(e, sc[0], sc[1], e->d_ptn_scaled.p));
    return IQHIP_OK;
}

extern "C" int iqhip_fetch_pattern_lh_scaled(iqhip_engine *e, iqhip_branch_end a, iqhip_branch_end b, double *out) {
    if (!e || !out) return fail(IQHIP_ERR_INVALID, "null argument");
    if (!e->shards.empty()) return sharded::fetch_pattern_lh(e, out, 1, a, b);
    HIPCHK(use_device(e));
    int rc = scaled_pattern_lh(e, a, b);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(out, e->d_ptn_scaled.p, sizeof(double) * (size_t)e->nptn, hipMemcpyDeviceToHost, e->stream));
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
    DevBuf<double> d_out;   // (lives for this call, which ends with the stream drained)
    HIPCHK(d_out.ensure(e, count));
    HIPCHK(launch_pattern_lh_cat(e, len, d_out.p));
    HIPCHK(hipMemcpyAsync(out, d_out.p, sizeof(double) * count, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return IQHIP_OK;
}

// replaces the sample matrix by one of nsamples rows (0: none) once the engine's stream has drained; contents undefined
static hipError_t boot_matrix(iqhip_engine *e, int nsamples) {
    hipError_t s = hipStreamSynchronize(e->stream);
    if (s != hipSuccess) return s;
    e->d_boot.reset();
    e->nboot = 0;
    e->ufb.nsamples = 0;   // (the UFBoot state belongs to the matrix it was initialised on)
    e->boot_generation++;
    if (nsamples == 0) return hipSuccess;
    if ((s = e->d_boot.ensure(e, (size_t)e->nptn_pad * nsamples)) == hipSuccess) e->nboot = nsamples;
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
    HIPCHK(hipMemset(e->d_boot.p, 0, sizeof(float) * pitch * nsamples));
    HIPCHK(hipMemcpy2D(e->d_boot.p, pitch * sizeof(float), samples, (size_t)e->nptn * sizeof(float),
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
    memcpy(rell, e->h_result.p, sizeof(double) * (size_t)e->nboot);
    return IQHIP_OK;
}

// ---- branch tests (SH-aLRT, local bootstrap): the store of per-pattern log-likelihood rows and its consumers --------
// (kernels_rell.hip k_ptnlh_rows fills rows from batched tasks, kernels_alrt.hip multiplies them with the sample matrix;
// single-device engines only: a pattern-sharded engine keeps no per-pattern store)
// every row of a list lies inside the store
static int ptnlh_check_rows(iqhip_engine *e, const char *what, const int32_t *rows, int nrows, const char *hint = "") {
    for (int i = 0; i < nrows; i++)
        if (rows[i] < 0 || rows[i] >= e->ptnlh_rows)
            return fail(IQHIP_ERR_INVALID, std::string(what) + ": row outside the store" + hint);
    return IQHIP_OK;
}

extern "C" int iqhip_ptnlh_reserve(iqhip_engine *e, int nrows) {
    int rc = require(e, "iqhip_ptnlh_reserve", REQ_SINGLE_DEVICE);
    if (rc) return rc;
    if (nrows < 0 || nrows > (1 << 20)) return fail(IQHIP_ERR_INVALID, "iqhip_ptnlh_reserve: bad row count");
    HIPCHK(use_device(e));
    if (nrows <= e->ptnlh_rows) return IQHIP_OK;   // (rows keep their contents while the store does not grow)
    DevBuf<double> grown;   // (the old store stays as it is until the new one is complete; whichever is left over frees itself)
    if (grown.ensure(e, (size_t)nrows * e->nptn_pad) != hipSuccess)
        return fail(IQHIP_ERR_NOMEM, "iqhip_ptnlh_reserve: out of device memory");
    // (on the engine's stream: a memset on the null stream is not ordered against the kernels that fill rows next)
    HIPCHK(hipMemsetAsync(grown.p, 0, sizeof(double) * (size_t)nrows * e->nptn_pad, e->stream));
    if (e->d_ptnlh.p)
        HIPCHK(hipMemcpyAsync(grown.p, e->d_ptnlh.p, sizeof(double) * (size_t)e->ptnlh_rows * e->nptn_pad, hipMemcpyDeviceToDevice,
                              e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    e->d_ptnlh.swap(grown);
    e->ptnlh_rows = nrows;
    return IQHIP_OK;
}

extern "C" int iqhip_ptnlh_put_current(iqhip_engine *e, int row, iqhip_branch_end a, iqhip_branch_end b) {
    int rc = require(e, "iqhip_ptnlh_put_current", REQ_SINGLE_DEVICE);
    if (rc) return rc;
    rc = ptnlh_check_rows(e, "iqhip_ptnlh_put_current", &row, 1, " (iqhip_ptnlh_reserve)");
    if (rc) return rc;
    HIPCHK(use_device(e));
    const int16_t *sc[2];
    rc = branch_scale_counters(e, a, b, sc);
    if (rc) return rc;
    HIPCHK(launch_pattern_lh_scaled(e, sc[0], sc[1], e->d_ptnlh.p + (size_t)row * e->nptn_pad));
    return IQHIP_OK;
}

extern "C" int iqhip_ptnlh_fetch(iqhip_engine *e, int row, double *out) {
    int rc = require(e, "iqhip_ptnlh_fetch", REQ_SINGLE_DEVICE);
    if (rc) return rc;
    if (!out) return fail(IQHIP_ERR_INVALID, "iqhip_ptnlh_fetch: null argument");
    rc = ptnlh_check_rows(e, "iqhip_ptnlh_fetch", &row, 1);
    if (rc) return rc;
    HIPCHK(use_device(e));
    HIPCHK(hipMemcpyAsync(out, e->d_ptnlh.p + (size_t)row * e->nptn_pad, sizeof(double) * (size_t)e->nptn, hipMemcpyDeviceToHost,
                          e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return IQHIP_OK;
}

RowList iqhip::row_list(const int32_t *rows, int nrows) {
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

void iqhip::row_list_scatter(const RowList &rl, const double *sums, int nsamples, double *out) {
    const int32_t *idx = rl.list.data() + rl.M;
    const size_t nrows = rl.list.size() - (size_t)rl.M;
    for (size_t i = 0; i < nrows; i++)
        memcpy(out + i * nsamples, sums + (size_t)idx[i] * nsamples, sizeof(double) * (size_t)nsamples);
}

// the list into bt.rows; bt.part and bt.sums sized for products of its distinct rows with nsamples replicates
int iqhip::bt_stage(iqhip_engine *e, const RowList &rl, int ksplit, size_t nsamples) {
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
    int rc = require(e, "iqhip_ptnlh_rell", REQ_SINGLE_DEVICE);
    if (rc) return rc;
    if (!rows || !out || nrows < 1) return fail(IQHIP_ERR_INVALID, "iqhip_ptnlh_rell: bad row list");
    RowList rl;
    rc = ptnlh_product(e, "iqhip_ptnlh_rell", rows, nrows, nsamples, &rl);
    if (rc) return rc;
    std::vector<double> sums((size_t)rl.M * nsamples);
    HIPCHK(hipMemcpyAsync(sums.data(), e->bt.sums.p, sizeof(double) * sums.size(), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    row_list_scatter(rl, sums.data(), nsamples, out);
    return IQHIP_OK;
}

extern "C" int iqhip_branch_tests(iqhip_engine *e, const int32_t *rows3, const double *lh3, int nbranch, int reps_sh,
                                  int reps_lbp, iqhip_branch_support *out) {
    int rc = require(e, "iqhip_branch_tests", REQ_SINGLE_DEVICE);
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
    int rc = require(e, "iqhip_ptnlh_upload", REQ_SINGLE_DEVICE);
    if (rc) return rc;
    if (!in) return fail(IQHIP_ERR_INVALID, "iqhip_ptnlh_upload: null argument");
    rc = ptnlh_check_rows(e, "iqhip_ptnlh_upload", &row, 1, " (iqhip_ptnlh_reserve)");
    if (rc) return rc;
    HIPCHK(use_device(e));
    std::vector<double> tmp((size_t)e->nptn_pad, 0.0);
    memcpy(tmp.data(), in, sizeof(double) * (size_t)e->nptn);
    HIPCHK(hipStreamSynchronize(e->stream));
    HIPCHK(hipMemcpyAsync(e->d_ptnlh.p + (size_t)row * e->nptn_pad, tmp.data(), sizeof(double) * tmp.size(), hipMemcpyHostToDevice,
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
    HIPCHK(hipMemcpy(freq.data(), e->d_freq.p, sizeof(double) * freq.size(), hipMemcpyDeviceToHost));
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
    HIPCHK(e->d_freq_prefix.ensure(e, prefix.size()));
    HIPCHK(hipMemcpy(e->d_freq_prefix.p, prefix.data(), sizeof(int64_t) * prefix.size(), hipMemcpyHostToDevice));
    e->freq_nsite = total;
    e->freq_prefix_valid = true;
    return IQHIP_OK;
}

// a sample matrix of exactly (exact) or at least nsamples rows, contents undefined
static int topo_boot_rows(iqhip_engine *e, int nsamples, bool exact) {
    if (e->d_boot.p && (exact ? e->nboot == nsamples : e->nboot >= nsamples)) return IQHIP_OK;
    const hipError_t s = boot_matrix(e, nsamples);
    if (s == hipErrorOutOfMemory) return fail(IQHIP_ERR_NOMEM, "bootstrap sample matrix: out of device memory");
    HIPCHK(s);
    return IQHIP_OK;
}

static const int64_t kTopoMaxDraws = (int64_t)1 << 24;   // counts above 2^24 are not representable in float

extern "C" int iqhip_gen_boot_samples(iqhip_engine *e, int nsamples, int64_t first_replicate, int64_t ndraws, uint64_t seed,
                                      uint32_t stream) {
    int rc = require(e, "iqhip_gen_boot_samples", REQ_SINGLE_DEVICE);
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
    e->boot_generation++;
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
    int rc = require(e, "iqhip_ptnlh_diff_variance", REQ_SINGLE_DEVICE);
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
    int rc = require(e, "iqhip_tree_tests", REQ_SINGLE_DEVICE);
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
    int rc = require(e, "iqhip_multiscale_bp", REQ_SINGLE_DEVICE);
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
    e->boot_generation++;
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
