// kernels_quartet.hip -- likelihood mapping (PhyloTree::computeQuartetLikelihoods, quartet.cpp:676-1152): per quartet of taxa
// the maximised log-likelihoods of its three trees.  4-state data only.
//
//   k_quartet_cells4   one wave per quartet, four waves per workgroup.  The wave walks the four state rows and ptn_freq in
//       pattern order.  A pattern whose four states are all < 4 adds its frequency to one of 256 fp64 cells in the wave's own
//       LDS slice (LDS atomics; integer-valued frequencies below 2^53 sum exactly in any order, so the table has the same bits
//       on every run).  Every other pattern of frequency > 0 is appended to the quartet's other-list in pattern order (ballot
//       plus prefix popcount, as k_pair_solve compacts its cells).
//   k_quartet_solve4   one workgroup of one wave per (quartet, topology).  Its work items are the non-zero cells, compacted
//       once, followed by the other-patterns (their states are read from the engine's state rows); item q belongs to lane
//       q % 64.  The wave restates fixNegativeBranch(true) (Fitch starting lengths) and optimizeAllBranches(iterations,
//       tolerance) with newton_init / newton_update of iqhip_internal.h as the only Newton rule -- include/iqhip.h describes
//       the steps and the traversal table.
//       The function, per item and category c, in the engine's eigen form:
//         leaf vector   v_x[s] = sum_j P_x,c[s][j] over the states j the leaf's code allows, P_x,c = U exp(L r_c t_x) U^-1 kept
//                       as a state-space table per pendant branch in LDS (one lookup for an unambiguous state, exactly 1.0
//                       for STATE_UNKNOWN -- the K2 rule);
//         cherry        Y = U^-1 (v o v);
//         pendant branch of leaf l with sibling s:  x = U^-1 (v_s o (E_int Y)),  theta_i = tip[code_l][i] x_i,
//                       E_int[s][i] = U[s][i] exp(L_i r_c t_int) kept in LDS;   internal branch:  theta = X o Y;
//         lh = invar + sum_c sum_i val0[c][i] theta_i with val0 = prop_c exp(L_i r_c t), df and ddf from val1 = L_i r_c val0 and
//         val2 = L_i r_c val1 (phylokernel.h:599-646); lnL = sum w log|lh|.
//       Theta is rebuilt at every evaluation: nothing per item is kept between evaluations, so the number of other-patterns is
//       unbounded.  Sums over items: every lane adds its items in item order, then one wave_sum64 -- a fixed order, so the
//       results are bit-identical from run to run and do not depend on the chunking.
//       No scaling step: with four leaves and lengths in [1e-6, 100] no vector gets near 2^-256 (the smallest is about
//       1e-28), so the reference's scale counters stay 0; the numpy restatement of the tests asserts that.
//       All loops are bounded: <= iterations sweeps x 5 branches x <= max_steps + 1 evaluations.  The kernel waits on no other
//       wave, uses no global atomics and no grid-wide step.
// Built with -ffp-contract=off (Makefile), like kernels_dist.hip.
#include <hip/hip_runtime.h>

#include "iqhip_internal.h"

#pragma clang fp contract(off)

namespace iqhip {

constexpr int kQuartetWaves = 4;   // quartets per workgroup of k_quartet_cells4

// ---- cells --------------------------------------------------------------------------------------------------------------
// Every wave reaches every barrier, whatever it has to do (a workgroup past the end of the chunk has idle waves).
__global__ __launch_bounds__(64 * kQuartetWaves) void k_quartet_cells4(const int32_t *__restrict__ quartets, int m,
                                                                       const uint8_t *__restrict__ states, int64_t nptn_pad,
                                                                       int64_t nptn, const double *__restrict__ freq,
                                                                       double *__restrict__ cells, int32_t *__restrict__ nother,
                                                                       int32_t *__restrict__ other) {
    __shared__ double s_tab[kQuartetWaves][256];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int slot = blockIdx.x * kQuartetWaves + w;
    const bool active = slot < m;   // (wave-uniform)
    double *tab = s_tab[w];
    for (int i = lane; i < 256; i += 64) tab[i] = 0.0;
    __syncthreads();
    int count = 0;
    if (active) {
        const uint8_t *row[4];
#pragma unroll
        for (int t = 0; t < 4; t++) row[t] = states + (size_t)quartets[4 * (size_t)slot + t] * nptn_pad;
        int32_t *list = other + (size_t)slot * nptn;
        for (int64_t base = 0; base < nptn; base += 64) {
            const int64_t p = base + lane;
            bool rest = false;
            if (p < nptn) {
                const double f = freq[p];
                const int s0 = row[0][p], s1 = row[1][p], s2 = row[2][p], s3 = row[3][p];
                if (f != 0.0) {
                    if ((s0 | s1 | s2 | s3) < 4)
                        atomicAdd(&tab[((s0 * 4 + s1) * 4 + s2) * 4 + s3], f);
                    else
                        rest = true;
                }
            }
            const unsigned long long mask = __ballot(rest);
            if (rest) list[count + __popcll(mask & ((1ull << lane) - 1ull))] = (int32_t)p;   // (count + .. < nptn)
            count += __popcll(mask);
        }
    }
    __syncthreads();
    if (active) {
        for (int i = lane; i < 256; i += 64) cells[(size_t)slot * 256 + i] = tab[i];
        if (lane == 0) nother[slot] = count;
    }
}

// ---- solver -------------------------------------------------------------------------------------------------------------
// LDS of a workgroup, doubles: P [4][C][16] ++ EI [C][16] ++ val [3][C][4] ++ U [16] ++ Ui [16] ++ lam [4] ++ rate [C] ++
// prop [C] ++ tip [(su + 1)][4] ++ w [256] ++ const_invar [8], then the cell codes uint8 [256] and the code masks uint8 [32]
__host__ __device__ inline size_t quartet_lds_doubles(int C, int su) {
    return (size_t)80 * C + (size_t)12 * C + 36 + (size_t)2 * C + (size_t)4 * (su + 1) + 256 + 8;
}

struct QuartetCtx {
    double *P, *EI, *val, *U, *Ui, *lam, *rate, *prop, *tip, *w;
    uint8_t *code, *mask;       // the compacted cell codes; the states every state code allows
    const uint8_t *row[4];      // state rows of p0 .. p3 (topology order)
    const int32_t *other;
    const double *freq;
    int C, su, nnz, nother, lane;
    int perm[4];                // p_j = quartet[perm[j]]
    const double *cinv;         // const_invar [5]
};

__device__ __forceinline__ unsigned q_mask(const QuartetCtx &x, int code) { return code < 4 ? 1u << code : x.mask[code]; }

// the four state codes of item q in topology order and its weight
__device__ __forceinline__ double q_item(const QuartetCtx &x, int q, int st[4]) {
    if (q < x.nnz) {
        const int cell = x.code[q];
#pragma unroll
        for (int j = 0; j < 4; j++) st[j] = (cell >> (6 - 2 * x.perm[j])) & 3;   // (the cell holds the states in quartet order)
        return x.w[q];
    }
    const int64_t p = x.other[q - x.nnz];
#pragma unroll
    for (int j = 0; j < 4; j++) st[j] = x.row[j][p];
    return x.freq[p];
}

// Alignment::computeConst on the four states -> the invariant term
__device__ __forceinline__ double q_invar(const QuartetCtx &x, const unsigned m[4]) {
    const unsigned all = m[0] & m[1] & m[2] & m[3];
    if (all == 15u) return x.cinv[4];
    if (__popc(all) == 1) {
        const int s = __ffs(all) - 1;
        return x.cinv[s];
    }
    return 0.0;
}

// v[s] = sum over the allowed states j of P[s][j]; STATE_UNKNOWN: exactly 1.0
__device__ __forceinline__ void q_leaf_vec(const double *P, int code, unsigned mask, int su, double v[4]) {
    if (code < 4) {
#pragma unroll
        for (int s = 0; s < 4; s++) v[s] = P[s * 4 + code];
    } else if (code == su) {
#pragma unroll
        for (int s = 0; s < 4; s++) v[s] = 1.0;
    } else {
#pragma unroll
        for (int s = 0; s < 4; s++) {
            double a = 0.0;
#pragma unroll
            for (int j = 0; j < 4; j++) a += ((mask >> j) & 1u) ? P[s * 4 + j] : 0.0;
            v[s] = a;
        }
    }
}

// out = Ui (a o b): out[i] = sum_s Ui[i][s] a[s] b[s]
__device__ __forceinline__ void q_to_eigen(const double Ui[16], const double a[4], const double b[4], double out[4]) {
    double t[4];
#pragma unroll
    for (int s = 0; s < 4; s++) t[s] = a[s] * b[s];
#pragma unroll
    for (int i = 0; i < 4; i++) out[i] = (Ui[i * 4] * t[0] + Ui[i * 4 + 1] * t[1]) + (Ui[i * 4 + 2] * t[2] + Ui[i * 4 + 3] * t[3]);
}

// the transition table of pendant branch b (state space) or, b == 4, the K1 table of the internal branch, for length t.
// `val` serves as scratch for the exponentials.  Ends with a barrier: the tables are ready for every lane.
__device__ __forceinline__ void q_build_table(const QuartetCtx &x, int b, double t) {
    const int C = x.C;
    __syncthreads();
    for (int idx = x.lane; idx < 4 * C; idx += 64) x.val[idx] = exp(x.lam[idx & 3] * (x.rate[idx >> 2] * t));
    __syncthreads();
    if (b < 4) {
        double *P = x.P + (size_t)b * 16 * C;
        for (int idx = x.lane; idx < 16 * C; idx += 64) {
            const int c = idx >> 4, s = (idx >> 2) & 3, j = idx & 3;
            const double *e = x.val + 4 * c;
            P[idx] = (x.U[s * 4] * e[0] * x.Ui[j] + x.U[s * 4 + 1] * e[1] * x.Ui[4 + j]) +
                     (x.U[s * 4 + 2] * e[2] * x.Ui[8 + j] + x.U[s * 4 + 3] * e[3] * x.Ui[12 + j]);
        }
    } else {
        for (int idx = x.lane; idx < 16 * C; idx += 64) x.EI[idx] = x.U[idx & 15] * x.val[4 * (idx >> 4) + (idx & 3)];
    }
    __syncthreads();
}

// One evaluation on branch b at length t with the other four lengths as the tables hold them: the wave's sums of
// w log|lh| (LNL) or of w df, w ddf (!LNL), the same value in every lane
template <bool LNL>
__device__ __forceinline__ void q_eval(const QuartetCtx &x, int b, double t, double &o0, double &o1) {
    const int C = x.C;
    __syncthreads();   // (the previous evaluation has read val)
    for (int idx = x.lane; idx < 4 * C; idx += 64) {
        const double cof = x.lam[idx & 3] * x.rate[idx >> 2];
        const double v0 = exp(cof * t) * x.prop[idx >> 2];
        x.val[idx] = v0;
        if (!LNL) {
            const double v1 = cof * v0;
            x.val[4 * C + idx] = v1;
            x.val[8 * C + idx] = cof * v1;
        }
    }
    __syncthreads();
    double Ui[16];
#pragma unroll
    for (int i = 0; i < 16; i++) Ui[i] = x.Ui[i];
    // pendant branch b: leaf l = b, its sibling sb, the far cherry (f1, f2)
    const int sb = b ^ 1, f1 = (b & 2) ? 0 : 2, f2 = f1 + 1;
    auto pick = [](unsigned packed, int i) { return (int)((packed >> (8 * i)) & 255u); };   // (no indexed register arrays)
    double acc0 = 0.0, acc1 = 0.0;
    const int nitems = x.nnz + x.nother;
    for (int q = x.lane; q < nitems; q += 64) {
        int st[4];
        const double w = q_item(x, q, st);
        unsigned m[4];
#pragma unroll
        for (int j = 0; j < 4; j++) m[j] = q_mask(x, st[j]);
        const unsigned stw = (unsigned)st[0] | ((unsigned)st[1] << 8) | ((unsigned)st[2] << 16) | ((unsigned)st[3] << 24);
        const unsigned mw = m[0] | (m[1] << 8) | (m[2] << 16) | (m[3] << 24);
        double lh = q_invar(x, m), d1 = 0.0, d2 = 0.0;
#pragma unroll 1
        for (int c = 0; c < C; c++) {
            double th[4];
            if (b < 4) {
                double va[4], vb[4], Y[4], z[4], xx[4];
                q_leaf_vec(x.P + ((size_t)f1 * C + c) * 16, pick(stw, f1), (unsigned)pick(mw, f1), x.su, va);
                q_leaf_vec(x.P + ((size_t)f2 * C + c) * 16, pick(stw, f2), (unsigned)pick(mw, f2), x.su, vb);
                q_to_eigen(Ui, va, vb, Y);
                const double *E = x.EI + (size_t)c * 16;
#pragma unroll
                for (int s = 0; s < 4; s++) z[s] = (E[s * 4] * Y[0] + E[s * 4 + 1] * Y[1]) + (E[s * 4 + 2] * Y[2] + E[s * 4 + 3] * Y[3]);
                q_leaf_vec(x.P + ((size_t)sb * C + c) * 16, pick(stw, sb), (unsigned)pick(mw, sb), x.su, va);
                q_to_eigen(Ui, va, z, xx);
                const double *tp = x.tip + 4 * pick(stw, b);
#pragma unroll
                for (int i = 0; i < 4; i++) th[i] = tp[i] * xx[i];
            } else {
                double va[4], vb[4], X[4], Y[4];
                q_leaf_vec(x.P + ((size_t)0 * C + c) * 16, st[0], m[0], x.su, va);
                q_leaf_vec(x.P + ((size_t)1 * C + c) * 16, st[1], m[1], x.su, vb);
                q_to_eigen(Ui, va, vb, X);
                q_leaf_vec(x.P + ((size_t)2 * C + c) * 16, st[2], m[2], x.su, va);
                q_leaf_vec(x.P + ((size_t)3 * C + c) * 16, st[3], m[3], x.su, vb);
                q_to_eigen(Ui, va, vb, Y);
#pragma unroll
                for (int i = 0; i < 4; i++) th[i] = X[i] * Y[i];
            }
            const double *v0 = x.val + 4 * c;
            lh += (v0[0] * th[0] + v0[1] * th[1]) + (v0[2] * th[2] + v0[3] * th[3]);
            if (!LNL) {
                const double *v1 = v0 + 4 * C, *v2 = v0 + 8 * C;
                d1 += (v1[0] * th[0] + v1[1] * th[1]) + (v1[2] * th[2] + v1[3] * th[3]);
                d2 += (v2[0] * th[0] + v2[1] * th[1]) + (v2[2] * th[2] + v2[3] * th[3]);
            }
        }
        if (LNL) {
            acc0 += w * log(fabs(lh));
        } else {
            const double inv = 1.0 / fabs(lh);
            const double dfp = d1 * inv;
            acc0 += w * dfp;
            acc1 += w * (d2 * inv - dfp * dfp);
        }
    }
    o0 = __shfl(wave_sum64(acc0), 0);
    o1 = LNL ? 0.0 : __shfl(wave_sum64(acc1), 0);
}

__device__ __forceinline__ unsigned q_fitch(unsigned a, unsigned b) { return (a & b) ? (a & b) : (a | b); }

__global__ __launch_bounds__(64) void k_quartet_solve4(const QuartetSolveArgs A) {
    extern __shared__ double s_dyn[];
    const int lane = threadIdx.x, C = A.ncat, su = A.state_unknown;
    const int slot = blockIdx.x / 3, k = blockIdx.x - 3 * slot;
    QuartetCtx x;
    x.P = s_dyn;
    x.EI = x.P + (size_t)64 * C;
    x.val = x.EI + (size_t)16 * C;
    x.U = x.val + (size_t)12 * C;
    x.Ui = x.U + 16;
    x.lam = x.Ui + 16;
    x.rate = x.lam + 4;
    x.prop = x.rate + C;
    x.tip = x.prop + C;
    x.w = x.tip + (size_t)4 * (su + 1);
    double *cinv = x.w + 256;
    x.cinv = cinv;
    x.code = reinterpret_cast<uint8_t *>(cinv + 8);
    x.mask = x.code + 256;
    x.C = C;
    x.su = su;
    x.lane = lane;
    x.freq = A.freq;
    x.other = A.other + (size_t)slot * A.nptn;
    x.nother = A.nother[slot];
    // qc[] of quartet.cpp:925
    x.perm[0] = 0;
    x.perm[1] = k == 0 ? 1 : k == 1 ? 2 : 3;
    x.perm[2] = k == 0 ? 2 : 1;
    x.perm[3] = k == 2 ? 2 : 3;
#pragma unroll
    for (int j = 0; j < 4; j++) x.row[j] = A.states + (size_t)A.quartets[4 * (size_t)slot + x.perm[j]] * A.nptn_pad;
    if (lane < 5) cinv[lane] = A.const_invar[lane];
    // the model, and the non-zero cells in cell order
    if (lane < 16) {
        x.U[lane] = A.evec[lane];
        x.Ui[lane] = A.inv_evec[lane];
    }
    if (lane < 4) x.lam[lane] = A.eval[lane];
    if (lane < 32) x.mask[lane] = A.mask[lane];
    for (int c = lane; c < C; c += 64) {
        x.rate[c] = A.rates[c];
        x.prop[c] = A.props[c];
    }
    for (int i = lane; i < 4 * (su + 1); i += 64) x.tip[i] = A.tip[i];
    const double *cnt = A.cells + (size_t)slot * 256;
    int nnz = 0;
    for (int base = 0; base < 256; base += 64) {
        const double c = cnt[base + lane];
        const bool nz = c > 0.0;
        const unsigned long long mask = __ballot(nz);
        if (nz) {
            const int at = nnz + __popcll(mask & ((1ull << lane) - 1ull));
            x.code[at] = (uint8_t)(base + lane);
            x.w[at] = c;
        }
        nnz += __popcll(mask);
    }
    x.nnz = nnz;
    __syncthreads();

    // fixNegativeBranch(true): Fitch over the informative items
    double sub[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    const int nitems = nnz + x.nother;
    for (int q = lane; q < nitems; q += 64) {
        int st[4];
        const double w = q_item(x, q, st);
        unsigned F[4];
        int twice = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) F[j] = q_mask(x, st[j]);
#pragma unroll
        for (int s = 0; s < 4; s++) {
            int app = 0;
#pragma unroll
            for (int j = 0; j < 4; j++) app += (st[j] != su && ((F[j] >> s) & 1u)) ? 1 : 0;
            twice += app >= 2 ? 1 : 0;
        }
        if (twice < 2) continue;
        const unsigned c01 = q_fitch(F[0], F[1]), c23 = q_fitch(F[2], F[3]);
        sub[0] += (F[0] & q_fitch(F[1], c23)) ? 0.0 : w;
        sub[1] += (F[1] & q_fitch(F[0], c23)) ? 0.0 : w;
        sub[2] += (F[2] & q_fitch(F[3], c01)) ? 0.0 : w;
        sub[3] += (F[3] & q_fitch(F[2], c01)) ? 0.0 : w;
        sub[4] += (c01 & c23) ? 0.0 : w;
    }
    double len[5];
#pragma unroll
    for (int b = 0; b < 5; b++) {
        const double s = __shfl(wave_sum64(sub[b]), 0);
        double bl = s > 0.0 ? s / A.nsite : 1.0 / A.nsite;
        const double z = 4.0 / 3.0;
        const double a = 1.0 - z * bl;
        if (a > 0.0) bl = -log(a) / z;
        if (bl < A.x1) bl = A.x1;
        len[b] = bl;
    }
#pragma unroll 1
    for (int j = 0; j < 5; j++) q_build_table(x, j, j == 0 ? len[0] : j == 1 ? len[1] : j == 2 ? len[2] : j == 3 ? len[3] : len[4]);

    // optimizeAllBranches(iterations, tolerance); the branch order of a sweep is the traversal table of include/iqhip.h
    constexpr int kQuartetOrder = 0x10432, kQuartetFirst = 2, kQuartetLast = 1;   // {2, 3, 4, 0, 1}, a nibble per step
    double tree_lh, unused;
    q_eval<true>(x, kQuartetFirst, len[kQuartetFirst], tree_lh, unused);
    int nsweeps = 0, neval = 0, status = 0;
#pragma unroll 1
    for (int it = 0; it < A.iterations; it++) {
        double saved[5];
#pragma unroll
        for (int j = 0; j < 5; j++) saved[j] = len[j];
#pragma unroll 1
        for (int o = 0; o < 5; o++) {
            const int b = (kQuartetOrder >> (4 * o)) & 7;
            const double cur = b == 0 ? len[0] : b == 1 ? len[1] : b == 2 ? len[2] : b == 3 ? len[3] : len[4];
            NewtonState st;
            newton_init(st, cur, A.x1, A.x2, A.xacc, A.max_steps);
            while (!st.done) {   // (wave-uniform: every lane advances the same state with the same sums)
                double df, ddf;
                q_eval<false>(x, b, st.rts, df, ddf);
                newton_update(st, df, ddf);
            }
            neval += st.neval;
            if (st.status && !status) status = st.status;
            double optx = st.result;
            if (optx > A.diverge_frac * A.x2) {   // the diverged solve (phylotree.cpp:2167-2176)
                double opt_lh, orig_lh;
                q_eval<true>(x, b, optx, opt_lh, unused);
                q_eval<true>(x, b, cur, orig_lh, unused);
                if (orig_lh > opt_lh) optx = cur;
            }
            if (optx != cur) {
#pragma unroll
                for (int j = 0; j < 5; j++) len[j] = j == b ? optx : len[j];
                q_build_table(x, b, optx);
            }
        }
        nsweeps++;
        double new_lh;
        q_eval<true>(x, kQuartetLast, len[kQuartetLast], new_lh, unused);
        if (new_lh < tree_lh) {   // restore and stop (phylotree.cpp:2303-2319)
#pragma unroll
            for (int j = 0; j < 5; j++) len[j] = saved[j];
#pragma unroll 1
            for (int j = 0; j < 5; j++) q_build_table(x, j, j == 0 ? len[0] : j == 1 ? len[1] : j == 2 ? len[2] : j == 3 ? len[3] : len[4]);
            q_eval<true>(x, kQuartetFirst, len[kQuartetFirst], tree_lh, unused);
            break;
        }
        const bool stop = tree_lh <= new_lh && new_lh <= tree_lh + A.tolerance;
        tree_lh = new_lh;
        if (stop) break;
    }
    if (lane == 0) {
        iqhip_quartet_result &r = A.out[A.first + slot];
        r.logl[k] = tree_lh;
#pragma unroll
        for (int b = 0; b < 5; b++) r.len[k][b] = len[b];
        r.nsweeps[k] = nsweeps;
        r.neval[k] = neval;
        r.status[k] = status;
    }
}

// ---- launches -------------------------------------------------------------------------------------------------------------
size_t quartet_solve_lds_bytes(int ncat, int state_unknown) {
    return sizeof(double) * quartet_lds_doubles(ncat, state_unknown) + 256 + 32;
}

hipError_t launch_quartet_cells(iqhip_engine *e, const int32_t *d_quartets, int m, double *d_cells, int32_t *d_nother,
                                int32_t *d_other) {
    if (m < 1) return hipSuccess;
    hipLaunchKernelGGL(k_quartet_cells4, dim3((unsigned)((m + kQuartetWaves - 1) / kQuartetWaves)), dim3(64 * kQuartetWaves), 0,
                       e->stream, d_quartets, m, e->d_states.p, e->nptn_pad, e->nptn, e->d_freq.p, d_cells, d_nother, d_other);
    return hipGetLastError();
}

hipError_t launch_quartet_solve(iqhip_engine *e, const QuartetSolveArgs &a, int m) {
    if (m < 1) return hipSuccess;
    hipLaunchKernelGGL(k_quartet_solve4, dim3((unsigned)(3 * m)), dim3(64), quartet_solve_lds_bytes(a.ncat, a.state_unknown),
                       e->stream, a);
    return hipGetLastError();
}

}  // namespace iqhip
