// trav_phases.h -- the phases the traversal kernels share, stated once (k_traverse4, k_traverse4w, k_sweep4's node update,
// k_traverse_mfma, trav_mfma2_body, k_traverse_mfma_mix20, trav_rows64_body).  Device only, forced inline, no state.  The
// kernels keep what differs: how maximum and non-zero bits are gathered, the barriers around a fill, the vector's rewrite.
#pragma once
#include "iqhip_internal.h"
namespace iqhip {
// 1. The scaling decision of one pattern.  SIMD rule (phylokernel.h:379-392, 461-474): an update whose children are not both
// leaves (TIP-TIP never scales, phylotreesse.cpp:807-843) rescales by 2^256, one event, when the maximum of the whole block is
// below 2^-256 and the pattern has no invariant-site term.  DevOp::no_scale: 0 that rule; 1 never (IQHIP_OP_NO_SCALE); 2 the
// scalar kernel's (IQHIP_OP_SCALAR_RULE, phylotreesse.cpp:774-788): `lh_max == 0` is tested FIRST, whatever ptn_invar says --
// the vector becomes the caller's STATE_UNKNOWN tip row in every category, FOUR events -- otherwise as rule 0.
// Key: the maximum as a double (k_traverse4, k_sweep4) or its magnitude's high word (amax_hi; promote_nonzero for denormals).
struct ScaleChoice {
    bool zero, scale;   // take the `lh_max == 0` branch; rewrite the vector at all (zero, or x 2^256)
    // events of a pattern that rescales: `sc += events()`, `my_scale = events() * (kLogScalingThreshold * freq)` (4, 1: exact)
    __device__ __forceinline__ int events() const { return zero ? 4 : 1; }
};
template <typename KEY>
__device__ __forceinline__ ScaleChoice scale_choice_on(int rule, bool tip_tip, KEY max, double invar, KEY threshold) {
    const bool zero = rule == 2 && !tip_tip && max == KEY(0);
    const bool do_scale = zero || (!tip_tip && (max < threshold) && (invar == 0.0) && rule != 1);
    return {zero, do_scale};
}
__device__ __forceinline__ ScaleChoice scale_choice(int rule, bool tip_tip, unsigned lmax, double invar) {
    return scale_choice_on<unsigned>(rule, tip_tip, lmax, invar, kScalingThresholdHi);
}
__device__ __forceinline__ ScaleChoice scale_choice(int rule, bool tip_tip, double lh_max, double invar) {
    return scale_choice_on<double>(rule, tip_tip, lh_max, invar, kScalingThreshold);
}
// 2. Only an exact zero takes the zero branch: the high-word key of a denormal below 2^-1042 is 0, so a lane that saw any
// non-zero bit (nz: the OR of nonzero_bits over its values, gathered under rule 2 at least) raises its key to 1.
__device__ __forceinline__ unsigned promote_nonzero(int rule, unsigned nz, unsigned lmax) {
    return (rule == 2 && nz != 0 && lmax == 0) ? 1u : lmax;
}
// 3. The pattern maximum over the CS waves that share a tile, through a [2 parities][waves][16] LDS array.  Contains exactly
// ONE __syncthreads(), between the g == 0 lanes' posts and the reads: every wave still in the op loop reaches it once per op
// with the op's parity (the write of the op after the next lies behind the next op's barrier: two parities suffice).
template <int CS, int W>
__device__ __forceinline__ unsigned tile_max(unsigned (&s)[2][W][16], int par, int wave, int p, int g, unsigned lmax) {
    if (g == 0) s[par][wave][p] = lmax;
    __syncthreads();
    const int w0 = (wave / CS) * CS;
    if constexpr (CS == 4) return max(max(s[par][w0][p], s[par][w0 + 1][p]), max(s[par][w0 + 2][p], s[par][w0 + 3][p]));
#pragma unroll
    for (int q = 0; q < CS; q++) lmax = max(lmax, s[par][w0 + q][p]);   // (integers: any association, the same bits)
    return lmax;
}
// 4. Posting an op's sum_scale partial: the wave's sum in fixed order (no lane rescaled: nothing to add), a plain store of it
// into the op's slab row by the writer lane, the row's fold flag raised (relaxed, agent scope) when it is non-zero; k_traverse4
// folds in-kernel and keeps its fold_store / fold_flag form.
__device__ __forceinline__ void post_scale_sum(double *slab, int *fold_flags, int out_row, int nwaves, int64_t tl, bool writer,
                                               double my_scale) {
    const double ws = __any(my_scale != 0.0) ? wave_sum64(my_scale) : 0.0;
    if (!writer) return;
    slab[(size_t)(2 + out_row) * nwaves + (int)tl] = ws;
    if (ws != 0.0) __hip_atomic_fetch_or(&fold_flags[2 + out_row], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// 5. The plain chunk fill: exp(ev(e) * (rate(e) * len)) for every element e < B of both children's regions of the kn ops from
// k; skip(op, child): children that need none (table children).  The barriers around it are the caller's.  (The staged fills
// of k_traverse4 and of trav_mfma2_body's 20 states are tuned apart and stay in their kernels.)
struct FillAll { template <typename Op> __device__ __forceinline__ bool operator()(const Op &, int) const { return false; } };
template <int WG, typename Ops, class Ev, class Rate, class Skip>
__device__ __forceinline__ void fill_exponentials(Ops ops, int k, int kn, int B, double *sReg, Ev ev, Rate rate, Skip skip) {
    for (int t = threadIdx.x; t < kn * 2 * B; t += WG) {
        const int o = t / (2 * B), r = t - o * (2 * B), child = r / B, e = r - child * B;
        const auto &d = ops[k + o];
        if (skip(d, child)) continue;
        sReg[(child ? d.lds_right : d.lds_left) + e] = exp(ev(e) * (rate(e) * op_child_len(d, child)));
    }
}
// 6. One entry of a 4-state K2 leaf table (phylokernel.h:187-232): E = U[x][.] * ex rounded first (LeafE4: made once, serves
// the table's four state rows), then the reference's (t0 + t1) + (t2 + t3) against the state's tip vector, all unfused.
struct LeafE4 {
    double e0, e1, e2, e3;
    __device__ __forceinline__ double entry(const double *tip4) const {
        return __dadd_rn(__dadd_rn(__dmul_rn(e0, tip4[0]), __dmul_rn(e1, tip4[1])), __dadd_rn(__dmul_rn(e2, tip4[2]), __dmul_rn(e3, tip4[3])));
    }
};
__device__ __forceinline__ LeafE4 leaf_e4(const double *Urow, const double *ex4) {
    return {__dmul_rn(Urow[0], ex4[0]), __dmul_rn(Urow[1], ex4[1]), __dmul_rn(Urow[2], ex4[2]), __dmul_rn(Urow[3], ex4[3])};
}
__device__ __forceinline__ double leaf_entry4(const double *Urow, const double *ex4, const double *tip4) {
    return leaf_e4(Urow, ex4).entry(tip4);
}
// 7. The items of k_traverse4's staged chunk fill, which k_fill4_image makes once per plan into the fill image: the same
// expressions, so the same bits.  model: [U 16][eigenvalues 4][rates C]; B = 4 C.
//   phase 1   element e of a region's exponentials
__device__ __forceinline__ double fill4_exp(const double *model, int e, double len) {
    return exp(model[16 + (e & 3)] * (model[20 + (e >> 2)] * len));
}
//   phase 2   element e = (c, x) of the four state rows and the unknown row of the K2 table behind a region's exponentials
__device__ __forceinline__ void fill4_leaf_table(double *reg, int B, int e, const double *model, const double *tip) {
    const int c = e >> 2, x = e & 3;
    const LeafE4 E = leaf_e4(model + x * 4, reg + c * 4);
#pragma unroll
    for (int row = 0; row < 4; row++) reg[B + row * B + e] = E.entry(tip + row * 4);
    reg[B + 4 * B + e] = 1.0;
}
//   phase 2b  row `code` of category c of a PAIR child's table, from the two leaf tables behind it (kPairRows rows; U, U^-1:
//   the kernel's scalar-operand views)
template <typename UPtr>
__device__ __forceinline__ void fill4_pair_row(double *reg, int B, int c, int code, UPtr U, UPtr uinv) {
    const int sa = code / 5, sb = code - 5 * sa;
    const double *ta = reg + (2 + kPairRows + sa) * B + c * 4, *tb = reg + (8 + kPairRows + sb) * B + c * 4;
    double tmp[4], l[4];
#pragma unroll
    for (int x = 0; x < 4; x++) tmp[x] = __dmul_rn(ta[x], tb[x]);
#pragma unroll
    for (int i = 0; i < 4; i++) {
        double v = __dmul_rn(uinv[i * 4], tmp[0]);
        v = fma(uinv[i * 4 + 1], tmp[1], v);
        v = fma(uinv[i * 4 + 2], tmp[2], v);
        v = fma(uinv[i * 4 + 3], tmp[3], v);
        l[i] = __dmul_rn(reg[c * 4 + i], v);
    }
#pragma unroll
    for (int x = 0; x < 4; x++) {
        double v = __dmul_rn(U[x * 4], l[0]);
        v = fma(U[x * 4 + 1], l[1], v);
        v = fma(U[x * 4 + 2], l[2], v);
        reg[B + code * B + c * 4 + x] = fma(U[x * 4 + 3], l[3], v);
    }
}
}  // namespace iqhip
