// kernels_valu4w.hip -- the node update of wide DNA engines: exactly 4 states with 9 .. 32 rate categories or mixture
// components (iqhip_engine::wide4), fp64 on the vector ALU, on the 16-pattern tile layout [tile16][e = c*4 + i][16].
//
// k_traverse_mfma<4, 256, true> runs the same plans, but pads the 4 states to a 16-row matrix tile (12 of 16 rows of every
// matrix instruction are zeros) and reads both children of every op from memory.  Here:
//   * one wave per tile; lane = (pattern p = lane & 15, group g = lane >> 4); group g owns the whole categories
//     c = g, g + 4, ..., CL = ceil(C / 4) of them (compile time), so that every access of a 16-lane group is one 128-byte
//     line and a category's four values sit in one lane: the products are k_traverse4's, U*(ex .* child) twice, Hadamard,
//     U^-1*, with no lane movement.  Lanes whose category is >= C compute on a clamped copy of the group's first category
//     and take no part in the maximum or in stores;
//   * the result of an op stays in registers: when a child pointer of the next op of the segment is that op's dst -- a
//     wave-uniform comparison of two descriptor fields -- the child and its scale counter are taken from there instead of
//     memory, which halves the loads of a caterpillar chain.  The Hadamard product commutes, so such a child is always made
//     the right one: the body is specialised on left in {LEAF, MEM} x right in {LEAF, MEM, PREV};
//   * a plain model keeps U and U^-1 wave-uniform through the constant address space (scalar operands), a mixture reads
//     its category's class from an LDS copy of every class;
//   * a LEAF child is the reference's K2 lookup as in k_traverse4: a 5-row table per (op, child) in LDS, built per chunk
//     with the reference's unfused association, the STATE_UNKNOWN row exactly 1.0; IUPAC codes take the wave-uniform slow
//     path that evaluates E*tip on the fly;
//   * scaling is the rule of the matrix-core kernels: per-pattern maximum over the whole block on the high words, the four
//     groups combined with the permlane swaps; the vector is stored unscaled per category and stored again in the rare
//     rescale (IQHIP_OP_SCALAR_RULE's lh_max == 0 branch: the tip row of STATE_UNKNOWN).  The decision, the posting of the
//     sum_scale partial, the fill of the exponentials and the leaf-table entry are trav_phases.h's.
// The descriptors are TRAV_GENERIC's (pf = left, ld = right, chunks, segments); patterns are independent, so there is no
// exchange between workgroups.
#include "iqhip_internal.h"
#include "trav_phases.h"

namespace iqhip {

#define CONST_AS __attribute__((address_space(4)))
#define LDS_AS __attribute__((address_space(3)))
template <typename T>
__device__ __forceinline__ const CONST_AS T *as_const(const T *p) {
    return (const CONST_AS T *)(p);
}
template <typename T>
__device__ __forceinline__ const LDS_AS T *as_lds(const T *p) {
    return (const LDS_AS T *)p;
}

struct Trav4wArgs {
    const DevOp *ops;
    const double *evec;       // class 0, [x][i]
    const double *inv_evec;   // class 0, [i][x]
    const double *img;        // every class: the generic kernel's padded images [class][U | U^-1][64], element (k * 16 + row)
    const double *evalc;      // [ncat][4]
    const double *rates;
    const double *tipc;       // [state][ncat][4]
    const int *cls;           // [ncat]
    const double *freq;
    const double *invar;
    double *slab;             // [nvals][nwaves]
    int *fold_flags;
    int64_t ntiles;
    int64_t nptn;
    const int *segs;          // {begin, nops} per segment; workgroup b works on segment b / ngroups
    int ngroups;
    int nwaves;
    int ncat;
    int nclass;
    int state_unknown;
};

enum : int { SRC_LEAF = 0, SRC_MEM = 1, SRC_PREV = 2 };

// a = M * l for a 4 x 4 row-major M in any address space
template <typename P>
__device__ __forceinline__ void mul4(P M, const double (&l)[4], double (&a)[4]) {
#pragma unroll
    for (int x = 0; x < 4; x++) {
        double v = M[x * 4] * l[0];
        v = fma(M[x * 4 + 1], l[1], v);
        v = fma(M[x * 4 + 2], l[2], v);
        a[x] = fma(M[x * 4 + 3], l[3], v);
    }
}

// a[x] of one child for the lane's j-th category c: reg = the child's LDS region ([ex B], a leaf's + [table 5B]), v = the
// lane's address of the category's first value in memory, prevj = the registers that hold it
template <int K, typename P>
__device__ __forceinline__ void child4w(const Trav4wArgs &A, P U, const double *reg, const char *v, const double *prevj, int c,
                                        int C, int s, int row, bool slow, double (&a)[4]) {
    const LDS_AS double *ex = as_lds(reg) + c * 4;
    double l[4];
    if (K == SRC_LEAF) {
        if (__builtin_expect(slow, 0)) {
            const double *tp = A.tipc + ((size_t)s * C + c) * 4;
#pragma unroll
            for (int i = 0; i < 4; i++) l[i] = ex[i] * tp[i];
            mul4(U, l, a);
#pragma unroll
            for (int x = 0; x < 4; x++) a[x] = (s == A.state_unknown) ? 1.0 : a[x];
        } else {
            const LDS_AS double *tab = as_lds(reg) + (1 + row) * 4 * C + c * 4;
#pragma unroll
            for (int x = 0; x < 4; x++) a[x] = tab[x];
        }
    } else {
#pragma unroll
        for (int i = 0; i < 4; i++) l[i] = ex[i] * (K == SRC_PREV ? prevj[i] : *reinterpret_cast<const double *>(v + i * 128));
        mul4(U, l, a);
    }
}

// one node update: the new vector replaces `prev` (which is the right child when KR == SRC_PREV) and is stored unscaled
template <int CL, bool MIX, int KL, int KR>
__device__ __forceinline__ void update4w(const Trav4wArgs &A, const int C, const double *sW, const int (&cc)[CL], const int (&woff)[CL],
                                         const uint32_t (&voff)[CL], const int g, const double *regL, const double *regR, const char *vL,
                                         const char *vR, const int sL, const int sR, char *dst, double (&prev)[4 * CL], unsigned &lmax,
                                         unsigned &nz) {
    bool slowL = false, slowR = false;
    int rowL = 0, rowR = 0;
    if (KL == SRC_LEAF) {
        slowL = __any((sL >= 4) && (sL != A.state_unknown));
        rowL = sL < 4 ? sL : 4;
    }
    if (KR == SRC_LEAF) {
        slowR = __any((sR >= 4) && (sR != A.state_unknown));
        rowR = sR < 4 ? sR : 4;
    }
#pragma unroll
    for (int j = 0; j < CL; j++) {
        const int c = cc[j];
        const uint32_t mo = voff[j];   // byte-offset addressing: a wave-uniform base plus one 32-bit offset per lane and category
        const bool valid = g + 4 * j < C;
        double a[4], b[4], tmp[4], o[4];
        if (MIX) {
            const LDS_AS double *W = as_lds(sW) + woff[j];
            child4w<KL>(A, W, regL, vL + mo, &prev[4 * j], c, C, sL, rowL, slowL, a);
            child4w<KR>(A, W, regR, vR + mo, &prev[4 * j], c, C, sR, rowR, slowR, b);
#pragma unroll
            for (int x = 0; x < 4; x++) tmp[x] = a[x] * b[x];
            mul4(W + 16, tmp, o);
        } else {
            child4w<KL>(A, as_const(A.evec), regL, vL + mo, &prev[4 * j], c, C, sL, rowL, slowL, a);
            child4w<KR>(A, as_const(A.evec), regR, vR + mo, &prev[4 * j], c, C, sR, rowR, slowR, b);
#pragma unroll
            for (int x = 0; x < 4; x++) tmp[x] = a[x] * b[x];
            mul4(as_const(A.inv_evec), tmp, o);
        }
#pragma unroll
        for (int i = 0; i < 4; i++) {
            prev[4 * j + i] = o[i];
            if (valid) {
                *reinterpret_cast<double *>(dst + mo + i * 128) = o[i];
                lmax = amax_hi(lmax, o[i]);
                nz |= nonzero_bits(o[i]);
            }
        }
    }
}

// CL = ceil(ncat / 4) categories per lane; MIX: a mixture (U, U^-1 of the category's class from LDS)
template <int CL, bool MIX>
__global__ __launch_bounds__(kTravWg) void k_traverse4w(const Trav4wArgs A) {
    constexpr int WPB = kTravWg / 64;
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int C = A.ncat, B = 4 * C;
    const Wide4Lds L = wide4_lds(A.nclass, B);
    double *sW = smem + L.sW;        // [nclass][U 16 | U^-1 16]
    double *sTipc = smem + L.sTipc;  // [4][B]
    double *sReg = smem + L.sReg;    // the chunk's per-(op, child) regions
    for (int t = threadIdx.x; t < 32 * A.nclass; t += kTravWg) {
        const int q = t & 15, m = (t >> 4) & 1, cl = t >> 5;
        sW[t] = A.img[(size_t)cl * 128 + m * 64 + (q & 3) * 16 + (q >> 2)];
    }
    for (int t = threadIdx.x; t < 4 * B; t += kTravWg) sTipc[t] = A.tipc[t];

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int seg = (int)blockIdx.x / A.ngroups;  // scalar
    const int k_begin = as_const(A.segs)[2 * seg], k_end = k_begin + as_const(A.segs)[2 * seg + 1];
    const int64_t tile = (int64_t)((int)blockIdx.x - seg * A.ngroups) * WPB + wave;
    const bool active = tile < A.ntiles;
    const int64_t tl = active ? tile : 0;
    const int p = lane & 15, g = lane >> 4;
    const int64_t ptn = tl * 16 + p;
    // (iqhip_create keeps a 4-state vector below 4 GiB, so a byte offset into one fits 32 bits)
    const uint32_t lbase = (uint32_t)(((size_t)tl * 16 * B + g * 64 + p) * sizeof(double));  // the lane's first category
    const double freq = A.freq[ptn];
    const double invar = A.invar[ptn];
    int cc[CL];   // the lane's categories; one past the end: a copy of its first
#pragma unroll
    for (int j = 0; j < CL; j++) cc[j] = g + 4 * j < C ? g + 4 * j : g;
    int woff[CL];   // mixtures: where the class of each of them starts in sW
#pragma unroll
    for (int j = 0; j < CL; j++) woff[j] = MIX ? 32 * A.cls[cc[j]] : 0;
    uint32_t voff[CL];   // ... and where each of them starts in a vector, in bytes
#pragma unroll
    for (int j = 0; j < CL; j++) voff[j] = lbase + (uint32_t)(cc[j] - g) * 64u * (uint32_t)sizeof(double);

    double prev[4 * CL];
#pragma unroll
    for (int e = 0; e < 4 * CL; e++) prev[e] = 0.0;
    int prev_sc = 0;
    const double *prev_dst = nullptr;

    int k = k_begin;
    while (k < k_end) {
        const int kn = as_const(A.ops)[k].chunk_nops;
        __syncthreads();
        // phase 1: the exponentials of every (op, child) of the chunk
        fill_exponentials<kTravWg>(as_const(A.ops), k, kn, B, sReg, [ev = A.evalc](int e) { return ev[e]; },
                                   [rt = A.rates](int e) { return rt[e >> 2]; }, FillAll{});
        __syncthreads();
        // phase 2: the leaf tables (K2).  One item = one (op, child, category, x): leaf_e4's four rounded products serve the
        // four state rows; the fifth row, STATE_UNKNOWN, is exactly 1.0
        for (int t = threadIdx.x; t < kn * 2 * B; t += kTravWg) {
            const int o = t / (2 * B), r = t - o * (2 * B), child = r / B, e = r - child * B, c = e >> 2, x = e & 3;
            const CONST_AS DevOp &d = as_const(A.ops)[k + o];
            if ((child ? d.right_kind : d.left_kind) != CHILD_LEAF) continue;
            double *reg = sReg + (child ? d.lds_right : d.lds_left);
            const double *W = sW + 32 * (MIX ? A.cls[c] : 0);
            const LeafE4 E = leaf_e4(W + x * 4, reg + c * 4);
#pragma unroll
            for (int row = 0; row < 4; row++) reg[B + row * B + e] = E.entry(sTipc + row * B + c * 4);
            reg[B + 4 * B + e] = 1.0;
        }
        __syncthreads();
        if (!active) { k += kn; continue; }

        for (int kk = 0; kk < kn; kk++, k++) {
            const CONST_AS DevOp &op = as_const(A.ops)[k];
            bool leafL = op.left_kind == CHILD_LEAF, leafR = op.right_kind == CHILD_LEAF;
            const double *pL = op.pf, *pR = op.ld;
            const int16_t *scLp = op.pf_sc, *scRp = op.ld_sc;
            const uint8_t *stL = op.sl, *stR = op.sr;
            int offL = op.lds_left, offR = op.lds_right;
            // the previous result as a child goes right (the Hadamard product commutes)
            if (!leafL && pL == prev_dst) {
                const double *tp = pL; pL = pR; pR = tp;
                const int16_t *ts = scLp; scLp = scRp; scRp = ts;
                const uint8_t *tt = stL; stL = stR; stR = tt;
                const int to = offL; offL = offR; offR = to;
                const bool tb = leafL; leafL = leafR; leafR = tb;
            }
            const bool prevR = !leafR && pR == prev_dst;
            // the scale counter of a pattern is carried by its g == 0 lane only
            int sc = 0, sL = 0, sR = 0;
            if (leafL) sL = stL[ptn]; else if (g == 0) sc += scLp[ptn];
            if (leafR) sR = stR[ptn]; else if (prevR) sc += prev_sc; else if (g == 0) sc += scRp[ptn];
            const double *regL = sReg + offL, *regR = sReg + offR;
            const char *vL = reinterpret_cast<const char *>(pL), *vR = reinterpret_cast<const char *>(pR);
            char *dst = reinterpret_cast<char *>(op.dst);
            unsigned lmax = 0, nz = 0;
#define IQHIP_W4(KL, KR) update4w<CL, MIX, KL, KR>(A, C, sW, cc, woff, voff, g, regL, regR, vL, vR, sL, sR, dst, prev, lmax, nz)
            if (leafL) {
                if (leafR) IQHIP_W4(SRC_LEAF, SRC_LEAF);
                else if (prevR) IQHIP_W4(SRC_LEAF, SRC_PREV);
                else IQHIP_W4(SRC_LEAF, SRC_MEM);
            } else {
                if (leafR) IQHIP_W4(SRC_MEM, SRC_LEAF);
                else if (prevR) IQHIP_W4(SRC_MEM, SRC_PREV);
                else IQHIP_W4(SRC_MEM, SRC_MEM);
            }
#undef IQHIP_W4
            // pattern maximum over the 4 lane groups (lmax orders the high words; a denormal below 2^-1042 still counts as
            // non-zero for the scalar rule's exact test)
            const int rule = op.no_scale;
            lmax = group_max_u(promote_nonzero(rule, nz, lmax));
            const ScaleChoice ch = scale_choice(rule, leafL && leafR, lmax, invar);
            double my_scale = 0.0;
            if (__any(ch.scale)) {
                if (ch.scale) {
#pragma unroll
                    for (int j = 0; j < CL; j++)
#pragma unroll
                        for (int i = 0; i < 4; i++) {
                            const double v = ch.zero ? A.tipc[(size_t)A.state_unknown * B + cc[j] * 4 + i] : prev[4 * j + i] * kScalingThresholdInv;
                            prev[4 * j + i] = v;
                            if (g + 4 * j < C) *reinterpret_cast<double *>(dst + voff[j] + i * 128) = v;
                        }
                    sc += ch.events();
                    if (g == 0 && ptn < A.nptn) my_scale = ch.events() * (kLogScalingThreshold * freq);
                }
            }
            if (g == 0) op.dst_sc[ptn] = (int16_t)sc;
            prev_sc = sc;
            prev_dst = op.dst;
            post_scale_sum(A.slab, A.fold_flags, op.out_row, A.nwaves, tl, lane == 0, my_scale);
        }
    }
}

template <int CL>
static hipError_t launch4w(iqhip_engine *e, const TravLaunch &L, const Trav4wArgs &A) {
    if (e->nclass > 1) (void)raise_lds_ceiling<&k_traverse4w<CL, true>>(e, kTravMaxLdsBytes);
    else (void)raise_lds_ceiling<&k_traverse4w<CL, false>>(e, kTravMaxLdsBytes);
    (void)hipGetLastError();
    if (e->nclass > 1) hipLaunchKernelGGL((k_traverse4w<CL, true>), dim3((unsigned)L.grid), dim3(kTravWg), L.lds_bytes, e->stream, A);
    else hipLaunchKernelGGL((k_traverse4w<CL, false>), dim3((unsigned)L.grid), dim3(kTravWg), L.lds_bytes, e->stream, A);
    return hipGetLastError();
}

hipError_t launch_traverse4w(iqhip_engine *e, const TravLaunch &L, const int *seg_table, int nwaves) {
    if (L.variant != TRAV_WIDE4 || !e->wide4 || !e->d_img.p) return hipErrorInvalidValue;
    Trav4wArgs A;
    A.ops = e->d_ops.p;
    A.evec = e->d_evec;
    A.inv_evec = e->d_inv_evec;
    A.img = e->d_img.p + e->img_generic_off;
    A.evalc = e->d_evalc;
    A.rates = e->d_rates;
    A.tipc = e->d_tipc;
    A.cls = e->d_cls;
    A.freq = e->d_freq.p;
    A.invar = e->d_invar.p;
    A.slab = e->d_slab.p;
    A.fold_flags = e->d_fold_flags.p;
    A.ntiles = e->ntiles;
    A.nptn = e->nptn;
    A.segs = seg_table;
    A.ngroups = L.ngroups;
    A.nwaves = nwaves;
    A.ncat = e->ncat;
    A.nclass = e->nclass;
    A.state_unknown = e->state_unknown;
    switch ((e->ncat + 3) / 4) {
        case 3: return launch4w<3>(e, L, A);
        case 4: return launch4w<4>(e, L, A);
        case 5: return launch4w<5>(e, L, A);
        case 6: return launch4w<6>(e, L, A);
        case 7: return launch4w<7>(e, L, A);
        case 8: return launch4w<8>(e, L, A);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace iqhip
