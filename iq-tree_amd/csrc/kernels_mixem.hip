// kernels_mixem.hip -- the device half of the EM estimation of mixture class weights (ModelMixture::optimizeWeights,
// model/modelmixture.cpp:1355-1416; Wang, Li, Susko and Roger 2008), of the per-pattern class posteriors and of
// PhyloTree::computePatternStateFreq (phylotree.cpp:1162-1196).
//   k_mix_class_lh   : Lc[m][p] = sum of L_pq over the components q of class m in ascending q (phylotree.cpp:1132-1143), L_pq
//                      the quantity iqhip_pattern_lh_cat returns (same LDS table exp(eval_i r_q len) prop_q, same arithmetic
//                      per component), from the theta buffer of the current branch in either vector layout.  Class-major
//                      [nclass][nptn_pad], padding patterns 0, unscaled.
//   k_mixem_step     : one E-step on Lc.  The reference rescales its matrix in place by new_prop / prop after every step; here
//                      Lc is never rewritten: the cumulative factors g[m] (and v for the invariant term) are a few doubles of
//                      device state and a step is ONE streaming read of Lc, ptn_freq and ptn_invar:
//                        s_p = v ptn_invar[p] + sum_m g[m] Lc[m][p],  t_p = freq_p / s_p,  S[m] = sum_p (g[m] Lc[m][p]) t_p
//                      A thread owns one pattern of its workgroup's kMixEmTile = 256 and keeps t_p in a register; the second
//                      pass loops over the classes again: one wave reduction per class and wave.  (Four patterns per
//                      thread, i.e. a quarter of the reductions, measured slower: too few workgroups)  Up to
//                      kMixEmRegClasses classes stay in registers between the passes; more are read a second time, from
//                      cache (the workgroup's tile is kMixEmTile * nclass * 8 bytes, 192 KB at 96 classes), kMixEmBatch
//                      classes at a time so that a thread has kMixEmBatch loads in flight.
//   k_mixem_update   : one workgroup folds the workgroup rows of S in a fixed order and applies modelmixture.cpp:1390-1408.
// Sums are formed in a fixed order without atomics, in a decomposition that follows from nptn_pad and nclass alone: the same
// bits on every run and every CU count.  Both kernels of a step return at once when the state's done flag is set, so the
// host enqueues all max_steps pairs with no read in between.
//   k_mix_posteriors : post[m][p] = Lc[m][p] * (1 / sum_m Lc[m][p]) (no invariant term: phylotree.cpp:1174-1182) and, with
//                      the classes' state frequencies, state_freq[i][p] = sum_m class_freq[m][i] post[m][p].
#include <hip/hip_runtime.h>

#include "iqhip_internal.h"

namespace iqhip {

__device__ __forceinline__ double mix_theta_at(const double *base, int tile, int pl, int e) {
    return tile == 64 ? base[(size_t)(e >> 1) * 128 + pl * 2 + (e & 1)] : base[(size_t)e * 16 + pl];
}

// cls_list: first[nclass + 1] ++ the components of class 0, of class 1, ... (each ascending).  Grid (pattern blocks, classes):
// a workgroup builds the table of its class's components only
__global__ __launch_bounds__(256) void k_mix_class_lh(const double *__restrict__ theta, const double *__restrict__ evalc,
                                                      const double *__restrict__ rates, const double *__restrict__ props,
                                                      const int32_t *__restrict__ cls_list, double len, int n, int ncat,
                                                      int nclass, int tile, int64_t nptn, int64_t nptn_pad,
                                                      double *__restrict__ Lc) {
    extern __shared__ double s_val[];  // [components of the class][n]
    const int m = blockIdx.y;
    const int q0 = cls_list[m], q1 = cls_list[m + 1];
    const int32_t *comp = cls_list + nclass + 1;
    for (int t = threadIdx.x; t < (q1 - q0) * n; t += 256) {
        const int k = t / n, c = comp[q0 + k];
        s_val[t] = exp(evalc[c * n + (t - k * n)] * rates[c] * len) * props[c];
    }
    __syncthreads();
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= nptn_pad) return;   // (the last workgroup may hang over the padded pattern count)
    double lh = 0.0;
    if (p < nptn) {
        const int64_t tl = p / tile;
        const int pl = (int)(p - tl * tile);
        const double *base = theta + (size_t)tl * tile * n * ncat;
        for (int k = q0; k < q1; k++) {
            const int c = comp[k];
            double acc = 0.0;
            for (int i = 0; i < n; i++) acc += s_val[(k - q0) * n + i] * mix_theta_at(base, tile, pl, c * n + i);
            lh = k == q0 ? acc : lh + acc;
        }
    }
    Lc[(size_t)m * nptn_pad + p] = lh;
}

template <bool REG>
__global__ __launch_bounds__(256) void k_mixem_step(const double *__restrict__ Lc, const double *__restrict__ freq,
                                                    const double *__restrict__ invar, const double *__restrict__ state,
                                                    int nclass, int64_t nptn, int64_t nptn_pad, double *__restrict__ part) {
    extern __shared__ double s_g[];  // g [nclass] ++ wave sums [4][nclass]
    if (state[MIXEM_DONE] != 0.0) return;   // (uniform over the grid)
    double *s_wave = s_g + nclass;
    for (int m = threadIdx.x; m < nclass; m += 256) s_g[m] = state[MIXEM_HDR + m];
    __syncthreads();
    const double v = state[MIXEM_V];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t p = (int64_t)blockIdx.x * kMixEmTile + threadIdx.x;
    // Loads of Lc are unconditional, so that the compiler keeps a whole batch of them in flight: a pattern beyond the padded
    // count reads the last column instead (in bounds).  What a pattern that is not live (beyond nptn, or of frequency 0) reads
    // is never used: its terms are selected to 0, not multiplied by 0, so a non-finite value there cannot reach a sum
    const size_t col = (size_t)(p < nptn_pad ? p : nptn_pad - 1);
    const double f = p < nptn ? freq[p] : 0.0;
    const bool live = f > 0.0;
    double s = live ? v * invar[p] : 0.0;
    if (REG) {
        double x[kMixEmRegClasses];
#pragma unroll
        for (int m = 0; m < kMixEmRegClasses; m++) x[m] = Lc[(size_t)(m < nclass ? m : nclass - 1) * nptn_pad + col];
#pragma unroll
        for (int m = 0; m < kMixEmRegClasses; m++)
            if (m < nclass) {
                x[m] *= s_g[m];
                s += x[m];
            }
        const double t = f / s;
#pragma unroll
        for (int m = 0; m < kMixEmRegClasses; m++)
            if (m < nclass) {
                const double acc = wave_sum64(live ? x[m] * t : 0.0);
                if (lane == 0) s_wave[wave * nclass + m] = acc;
            }
    } else {
        double l[kMixEmBatch];
        for (int m0 = 0; m0 < nclass; m0 += kMixEmBatch) {
#pragma unroll
            for (int u = 0; u < kMixEmBatch; u++) l[u] = Lc[(size_t)min(m0 + u, nclass - 1) * nptn_pad + col];
#pragma unroll
            for (int u = 0; u < kMixEmBatch; u++)
                if (m0 + u < nclass) s += s_g[m0 + u] * l[u];
        }
        const double t = f / s;
        for (int m0 = 0; m0 < nclass; m0 += kMixEmBatch) {   // the second read: from cache
#pragma unroll
            for (int u = 0; u < kMixEmBatch; u++) l[u] = Lc[(size_t)min(m0 + u, nclass - 1) * nptn_pad + col];
#pragma unroll
            for (int u = 0; u < kMixEmBatch; u++)
                if (m0 + u < nclass) {
                    const double acc = wave_sum64(live ? (s_g[m0 + u] * l[u]) * t : 0.0);
                    if (lane == 0) s_wave[wave * nclass + m0 + u] = acc;
                }
        }
    }
    __syncthreads();
    for (int m = threadIdx.x; m < nclass; m += 256)
        part[(size_t)blockIdx.x * nclass + m] = ((s_wave[m] + s_wave[nclass + m]) + s_wave[2 * nclass + m]) + s_wave[3 * nclass + m];
}

// one workgroup of kMixEmUpdateThreads threads, nclass <= that.  S[m]: the threads form G = threads / nclass groups; thread
// (group, m) adds the rows group, group + G, ... of class m in order, thread m then adds the G group sums in order.  The
// per-class part of the update runs on thread m; thread 0 adds the new weights in ascending order for p_invar
__global__ __launch_bounds__(kMixEmUpdateThreads) void k_mixem_update(const double *__restrict__ part, int64_t nrows, int nclass,
                                                                      int max_steps, double *__restrict__ state) {
    extern __shared__ double s_S[];  // [G][nclass]
    if (state[MIXEM_DONE] != 0.0) return;   // (uniform)
    const int step = (int)state[MIXEM_STEPS];
    if (step >= max_steps) return;          // (the log has max_steps rows)
    const int G = kMixEmUpdateThreads / nclass;
    const int grp = threadIdx.x / nclass, m = threadIdx.x - grp * nclass;
    if (grp < G) {
        double acc = 0.0;
        for (int64_t r = grp; r < nrows; r += G) acc += part[(size_t)r * nclass + m];
        s_S[grp * nclass + m] = acc;
    }
    __syncthreads();
    double *g = state + MIXEM_HDR, *w = g + nclass;
    double *log_row = w + nclass + (size_t)step * (nclass + 1);
    int conv_m = 1;
    if ((int)threadIdx.x < nclass) {
        double S = s_S[m];
        for (int k = 1; k < G; k++) S += s_S[k * nclass + m];
        const double new_m = S / state[MIXEM_NSITES], old = w[m];
        conv_m = fabs(old - new_m) < 1e-4 ? 1 : 0;
        g[m] = old == 0.0 ? 0.0 : g[m] * (new_m / old);
        w[m] = new_m;
        log_row[m] = new_m;
        s_S[m] = new_m;   // (this thread alone reads column m)
    }
    const int conv_all = __syncthreads_and(conv_m);
    if (threadIdx.x != 0) return;
    bool conv = conv_all != 0;
    double sum = 0.0;
    for (int k = 0; k < nclass; k++) sum += s_S[k];
    double pinv = state[MIXEM_PINV];
    if (state[MIXEM_USE_INV] != 0.0) {
        const double pinv_new = 1.0 - sum;
        conv = conv && (fabs(pinv - pinv_new) < 1e-4);
        state[MIXEM_V] = pinv_new / state[MIXEM_PINV_IN];
        state[MIXEM_PINV] = pinv = pinv_new;
    }
    log_row[nclass] = pinv;
    state[MIXEM_STEPS] = (double)(step + 1);
    state[MIXEM_DONE] = conv ? 1.0 : 0.0;
}

// one thread per pattern; post [nclass][nptn_pad], sfreq [n][nptn_pad] (either may be nullptr); class_freq [nclass][n]
__global__ __launch_bounds__(256) void k_mix_posteriors(const double *__restrict__ Lc, const double *__restrict__ class_freq,
                                                        int n, int nclass, int64_t nptn, int64_t nptn_pad,
                                                        double *__restrict__ post, double *__restrict__ sfreq) {
    extern __shared__ double s_cf[];  // [nclass][n]
    if (sfreq) {
        for (int t = threadIdx.x; t < nclass * n; t += 256) s_cf[t] = class_freq[t];
        __syncthreads();
    }
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= nptn) return;
    double sum = 0.0;
    for (int m = 0; m < nclass; m++) sum += Lc[(size_t)m * nptn_pad + p];
    const double inv = 1.0 / sum;
    if (post)
        for (int m = 0; m < nclass; m++) post[(size_t)m * nptn_pad + p] = Lc[(size_t)m * nptn_pad + p] * inv;
    if (sfreq)
        for (int i = 0; i < n; i++) {
            double f = 0.0;
            for (int m = 0; m < nclass; m++) f += s_cf[m * n + i] * (Lc[(size_t)m * nptn_pad + p] * inv);
            sfreq[(size_t)i * nptn_pad + p] = f;
        }
}

hipError_t launch_mix_class_lh(iqhip_engine *e, double len, const int32_t *d_cls_list, double *Lc) {
    const int64_t P = e->nptn_pad;
    hipLaunchKernelGGL(k_mix_class_lh, dim3((unsigned)((P + 255) / 256), (unsigned)e->nclass), dim3(256), sizeof(double) * e->block, e->stream,
                       e->d_theta.p, e->d_evalc, e->d_rates, e->d_props, d_cls_list, len, e->n, e->ncat, e->nclass, e->tile,
                       e->nptn, P, Lc);
    return hipGetLastError();
}

int64_t mixem_part_rows(const iqhip_engine *e) { return (e->nptn_pad + kMixEmTile - 1) / kMixEmTile; }

// one step and its update: two launches.  part: [mixem_part_rows][nclass]
hipError_t launch_mixem_step(iqhip_engine *e, const double *Lc, double *state, int max_steps, double *part) {
    const int M = e->nclass;
    const int64_t rows = mixem_part_rows(e);
    const size_t lds = sizeof(double) * 5 * (size_t)M;
    if (M <= kMixEmRegClasses)
        hipLaunchKernelGGL(k_mixem_step<true>, dim3((unsigned)rows), dim3(256), lds, e->stream, Lc, e->d_freq.p, e->d_invar.p, state, M,
                           e->nptn, e->nptn_pad, part);
    else
        hipLaunchKernelGGL(k_mixem_step<false>, dim3((unsigned)rows), dim3(256), lds, e->stream, Lc, e->d_freq.p, e->d_invar.p, state, M,
                           e->nptn, e->nptn_pad, part);
    hipLaunchKernelGGL(k_mixem_update, dim3(1), dim3(kMixEmUpdateThreads), sizeof(double) * (size_t)(kMixEmUpdateThreads / M) * M, e->stream, part, rows, M, max_steps, state);
    return hipGetLastError();
}

hipError_t launch_mix_posteriors(iqhip_engine *e, const double *Lc, const double *d_class_freq, double *post, double *sfreq) {
    const int64_t P = e->nptn_pad;
    const size_t lds = sfreq ? sizeof(double) * (size_t)e->nclass * e->n : 0;
    hipLaunchKernelGGL(k_mix_posteriors, dim3((unsigned)((P + 255) / 256)), dim3(256), lds, e->stream, Lc, d_class_freq, e->n,
                       e->nclass, e->nptn, P, post, sfreq);
    return hipGetLastError();
}

}  // namespace iqhip
