// iqhip_internal.h -- engine-private declarations shared by the engine and the kernel files.
// Device data layout (DESIGN.md "HBM layout"):
//   VALU path (nstates == 4): patterns are grouped in tiles of 64 (one wavefront); inside a
//   tile element e (= c*4+i, the reference's block index) of pattern p is stored at
//       tile*64*B + (e>>1)*128 + (p&63)*2 + (e&1)            [doubles]
//   so one global_load_dwordx4 per lane reads two consecutive elements and the wave reads
//   1 KiB contiguous.
//   MFMA path (nstates == 20 / 64): tiles of 16 patterns, state-major inside the tile:
//       tile*16*B + (c*n + i)*16 + (p&15)
//   which is exactly the B-operand / D-result image of v_mfma_f64_16x16x4_f64.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <time.h>
#include <algorithm>
#include <atomic>
#include <string>
#include <type_traits>
#include <unordered_map>
#include <vector>
#include "../../include/iqhip.h"
#include "trav_lds.h"

namespace iqhip {

constexpr int kSmallPlanOps = 4;         // op descriptors (incl. the two look-ahead sentinels) that fit the kernel arguments
constexpr int kNewtonPostEpochs = 128;   // evaluations of one k_newton launch that have a post slot
constexpr int kMixEmTile = 256;           // kernels_mixem.hip k_mixem_step: patterns per workgroup, one per thread ...
constexpr int kMixEmRegClasses = 8;       // ... classes whose tile values stay in registers between the two passes
constexpr int kMixEmBatch = 16;           // ... classes whose loads are issued together when there are more
constexpr int kMixEmUpdateThreads = 1024; // k_mixem_update: one workgroup; at most that many classes
constexpr double kScalingThreshold = 0x1p-256;       // phylotree.h:52
constexpr double kScalingThresholdInv = 0x1p256;     // phylotree.h:51
// log(2^-256) as libm returns it (phylotree.h:53)
constexpr double kLogScalingThreshold = -177.44567822334599;

// LEAF: state bytes; LOAD: read now; PREV: previous op's result (registers);
// PF: read one op ahead into the prefetch registers
// HOLD: parked in the HOLD registers by the producing op (push_hold) of the same launch
// PAIR (k_traverse4 only): the result of a leaf-leaf node update that the planner removed from the op list ("virtual", plan.hip
// select_pair_children) -- a function of the pair of leaf states only, read like a LEAF child from a 25-row table that the
// chunk fill builds, with the pair-code row 5 * min(sA, 4) + min(sB, 4) as its state row
enum ChildKind : int32_t { CHILD_LEAF = 0, CHILD_LOAD = 1, CHILD_PREV = 2, CHILD_PF = 3, CHILD_HOLD = 4, CHILD_PAIR = 5 };
// children read out of a table in LDS with a staged state byte as row index
constexpr bool child_is_table(int32_t kind) { return kind == CHILD_LEAF || kind == CHILD_PAIR; }
constexpr int kPairRows = 25;                  // rows of a PAIR child's table
// LDS region of a child, in blocks of B doubles: [ex][table 5] for a LEAF; [ex][table 25] and the leaf regions [ex][table 5] of the
// removed op's two leaves, which the fill builds the 25 rows from, for a PAIR; [ex] otherwise
constexpr int child_region_blocks(int32_t kind) { return kind == CHILD_LEAF ? 6 : (kind == CHILD_PAIR ? 1 + kPairRows + 12 : 1); }

// One node update as the device sees it. 16-byte aligned so that the wave-uniform reads
// of the descriptor become scalar loads.
struct __attribute__((aligned(16))) DevOp {
    double *dst;
    int16_t *dst_sc;
    const double *pf;        // the streamed child (kind CHILD_PF) or the engine's dummy slab
    const int16_t *pf_sc;    // its scale counters (or dummy)
    const uint8_t *sl;       // state row of a LEAF left child (or a dummy row)
    const uint8_t *sr;       // ... right child
    const double *ld;        // second memory child (kind CHILD_LOAD, right only), else dummy
    const int16_t *ld_sc;
    int32_t left_kind;
    int32_t right_kind;
    double left_len;
    double right_len;
    int32_t lds_left;   // offset (doubles) of the child's LDS region inside the chunk:
    int32_t lds_right;  //   internal child: [ex B]; leaf child: [ex B][table 5B]
    int32_t chunk_nops; // > 0 on the first op of an LDS chunk: number of ops in the chunk
    int32_t real_mask;  // bit0: pf/pf_sc are real (else dummies)
    int32_t sl_slot;    // LDS slot of the staged leaf states of the left / right child within
    int32_t sr_slot;    //   the chunk (slot 0 is shared by all non-leaf children)
    int32_t push_hold;  // 1: copy this op's result into the HOLD registers (consumed by a CHILD_HOLD)
    int32_t out_row;    // row of the caller's op list this op answers (sum_scale[out_row]); plans may be reordered
    int32_t no_scale;   // scaling rule: 0 SIMD kernel's; 1 never (IQHIP_OP_NO_SCALE: intermediate product of a multifurcating node);
                        // 2 scalar kernel's (IQHIP_OP_SCALAR_RULE: + the lh_max == 0 branch, phylotreesse.cpp:774-788)
    // matrix-core kernels: transition tables of the LEAF children (K2, phylokernel.h:187-232,293-317), built per
    // submission by k_leaf_tables into an L2-resident buffer: tab[c][state][n] (n permuted to the accumulator
    // image, see kernels_mfma.hip leaf_tab_pos); dummy-valid for non-leaf children
    const double *tabL;
    const double *tabR;
    // branch-length sweeps (iqhip_optimize_sweep): a child branch whose length is the result of an earlier step of the
    // same submission is read from device memory when the op runs (written there by that step's Newton solve);
    // nullptr: the host value left_len / right_len
    const double *left_len_p;
    const double *right_len_p;
    // 20 states x 4 categories, both children leaves ("cherry"): the node's whole vector is a function of the pair of leaf
    // states only -- cherry[(sL * (STATE_UNKNOWN + 1) + sR) * block + ...] holds it for every pair, in the order the lanes
    // keep it in registers (kernels_mfma.hip k_cherry_transpose); nullptr: compute the three matrix products
    const double *cherry;
    int32_t chunk_slots;   // 4-state path, on the first op of an LDS chunk: leaf-state slots of the chunk, the dummy slot 0 included
    // k_traverse4: where the chunk this op belongs to lies in the engine's fill image (doubles from its base, even: 16 bytes;
    // every op of the chunk carries it, the kernel reads the first op's); 0 in plans of other kernels
    int32_t image_off;
    // CHILD_PAIR children: the pendant branch lengths of the removed leaf-leaf op, {left child: its left, its right; right child:
    // its left, its right}, and the row of the caller's op list the removed op answers (-1: none) -- this op writes that row's
    // wave partial, always 0.0 (a leaf-leaf update never rescales)
    double pair_len[4];
    int32_t pair_row_l, pair_row_r;
};

#if defined(__HIPCC__)
// Sum over the 64 lanes of a wave, every lane gets it: the xor butterfly v += v^32, ^16, ^8, ^4, ^2, ^1 of the shuffle
// form, on the vector ALU instead of six dependent ds_bpermute round trips through the LDS crossbar (a derivative
// evaluation of a branch-length sweep spent half its 2 us in two of these).  Same bits as the shuffle form: the permlane
// swaps and quad permutes deliver exactly lane^32, ^16, ^2, ^1; row_ror:8 is lane^8 within a 16-lane row; row_ror:4
// delivers lane (i + 4) mod 16 instead of i^4, which holds the same value, because after the ^8 step lanes that agree in
// their low three bits hold equal sums -- and fp addition commutes.
__device__ __forceinline__ double wave_sum64(double v) {
    unsigned lo = __double2loint(v), hi = __double2hiint(v);
    auto a = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
    auto b = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
    v = __hiloint2double(b[0], a[0]) + __hiloint2double(b[1], a[1]);
    lo = __double2loint(v);
    hi = __double2hiint(v);
    auto c = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
    auto d = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
    v = __hiloint2double(d[0], c[0]) + __hiloint2double(d[1], c[1]);
#define IQHIP_DPP_STEP(ctrl)                                                                                  \
    v += __hiloint2double(__builtin_amdgcn_mov_dpp(__double2hiint(v), ctrl, 0xF, 0xF, true),                  \
                          __builtin_amdgcn_mov_dpp(__double2loint(v), ctrl, 0xF, 0xF, true));
    IQHIP_DPP_STEP(0x128)   // row_ror:8
    IQHIP_DPP_STEP(0x124)   // row_ror:4
    IQHIP_DPP_STEP(0x4E)    // quad_perm [2,3,0,1]
    IQHIP_DPP_STEP(0xB1)    // quad_perm [1,0,3,2]
#undef IQHIP_DPP_STEP
    return v;
}

// sum over the four lane groups of a pattern (lanes p, p+16, p+32, p+48) with gfx950's permlane swaps instead of
// ds_bpermute: swap(x, x) hands every lane its partner's value; (x + x^16) + (that of the lanes ^32), the order of
// the shuffle form (fp addition commutes), so the bits are the same
__device__ __forceinline__ double group_sum(double v) {
    unsigned lo = __double2loint(v), hi = __double2hiint(v);
    auto a = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
    auto b = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
    v = __hiloint2double(b[0], a[0]) + __hiloint2double(b[1], a[1]);
    lo = __double2loint(v);
    hi = __double2hiint(v);
    auto c = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
    auto d = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
    return __hiloint2double(d[0], c[0]) + __hiloint2double(d[1], c[1]);
}

// The scaling test max|x| < 2^-256 on the 32-bit vector ALU: for finite doubles |x| < 2^-256 <=> the high word of |x|
// is below that of 2^-256 (whose low word is 0), and the high words order like the values.  fp64 vector instructions
// run on the unit that executes the fp64 matrix instructions and ADD to their time (3.1 ns each against 29.5 ns for a
// 16x16x4, tools/mfma_issue_probe.hip), 32-bit ones overlap with them: v_and + v_max_u32 replace two v_max_f64 per value.
constexpr unsigned kScalingThresholdHi = 0x2FF00000u;   // high word of 0x1p-256
__device__ __forceinline__ unsigned amax_hi(unsigned m, double v) {
    const unsigned h = (unsigned)__double2hiint(v) & 0x7fffffffu;
    return m > h ? m : h;
}
// exactly-zero test for the scalar kernel's `lh_max == 0.0` branch (IQHIP_OP_SCALAR_RULE ops only): any bit of |x|
__device__ __forceinline__ unsigned nonzero_bits(double v) {
    return ((unsigned)__double2hiint(v) & 0x7fffffffu) | (unsigned)__double2loint(v);
}
// maximum over the four lane groups of a pattern (lanes p, p+16, p+32, p+48): kernels_mfma.hip group_max on one register
__device__ __forceinline__ unsigned group_max_u(unsigned v) {
    auto a = __builtin_amdgcn_permlane32_swap(v, v, false, false);
    v = a[0] > a[1] ? a[0] : a[1];
    auto b = __builtin_amdgcn_permlane16_swap(v, v, false, false);
    return b[0] > b[1] ? b[0] : b[1];
}

// length of a child branch of a node update: the host value, or the result of an earlier step of a sweep
template <typename OpRef>
__device__ __forceinline__ double op_child_len(const OpRef &d, int child) {
    const double *p = child ? d.right_len_p : d.left_len_p;
    return p ? *p : (child ? d.right_len : d.left_len);
}
#endif

// Root branch descriptor for the lnL / theta kernels.
struct __attribute__((aligned(16))) DevBranch {
    const double *a;            // internal side A (nullptr when A is a leaf)
    const uint8_t *a_states;    // leaf side states (nullptr when A is internal)
    const double *b;            // always internal
    const int16_t *a_sc;        // scale counters of the internal ends (+ASC rescale rule), else nullptr
    const int16_t *b_sc;
    int32_t a_kind;             // CHILD_LEAF / CHILD_LOAD / CHILD_PREV
    int32_t b_kind;             // CHILD_LOAD / CHILD_PREV
    double len;
};

// one node update / one step of a persistent branch-length sweep (kernels_sweep.hip k_sweep4)
struct __attribute__((aligned(16))) SweepOp {
    double *dst;
    int16_t *dst_sc;
    const double *lv, *rv;      // child vectors; nullptr: the child is a leaf
    const int16_t *lsc, *rsc;
    const uint8_t *ls, *rs;     // state rows of leaf children
    double llen, rlen;
    int32_t llen_step, rlen_step;  // >= 0: the child branch's length is the one that step of this sweep accepted
    int32_t no_scale;           // scaling rule, as DevOp::no_scale
    int32_t row;                // row of the wave-partial slab / of the caller's concatenated sum_scale array
};
struct __attribute__((aligned(16))) SweepStep {
    DevBranch br;
    double xguess;
    int32_t op_begin, nops;
};

// pairwise distances (kernels_dist.hip): a tile of 4 x 4 taxa of the pair list -- the pair (ra[x], rb[y]) is counted into
// slot out[4 x + y] of the chunk's counts (< 0: not asked for); unused rows name any valid taxon
struct __attribute__((aligned(16))) PairTile {
    int32_t ra[4], rb[4];
    int32_t out[16];
};

struct __attribute__((aligned(16))) TabJob {  // one K2 table to build: tab[c][state][pos(x)] for branch length len
    double len;
    double *tab;
    const double *len_p;   // non-null: the length is read from device memory (sweeps), `len` is ignored
    double _pad;
};

// What build_plan (plan.hip) leaves for the launchers besides the descriptors: one submission's plan.  Every field is
// reset when a plan is built; submit_traverse clears tab_dirty once the tables are built and empties cherry_jobs.
struct Plan {
    int lds_doubles = 0;            // LDS region size (doubles) of the largest chunk
    int state_slots = 1;            // leaf-state LDS slots of the largest chunk (4-state path)
    bool has_load = false;          // some op of the top stage has two memory children (slow kernel instantiation)
    bool units_have_load = false;   // ... some op of a unit
    // a plan of at most kSmallPlanOps - 2 ops with no units travels in the kernel arguments instead of d_ops (the copy
    // and the dependent-launch gap behind it cost ~9 us per changed plan, i.e. per branch of a sweep; IQHIP_SMALL_PLANS)
    bool small = false;
    int small_nops = 0;
    // Staged plans: independent subtrees ("units") run as their own workgroups in first launches, the ops above them
    // ("top") in a last one.  Segment table after the sentinel descriptors: {top_begin, top_nops, unit1_begin, unit1_nops, ...}
    int nunits = 0, top_nops = 0;
    std::vector<int> stage_units;   // units per stage, in launch order
    int table_off = 0, jobs_off = 0;  // DevOp index where the segment table / the K2 table job list starts
    int nhold = 0;                  // ops whose left child is parked (CHILD_HOLD)
    int nleaf_tabs = 0;             // K2 tables the plan uses (0: kernel variant without tables)
    std::vector<TabJob> tab_jobs;   // the plan's tables: [0, tab_dirty) need (re)building
    int tab_dirty = 0;
    std::vector<int> cherry_jobs;   // cherry-table slots the plan needs (re)built before its traversal
    bool uses_cherry = false;
    uint64_t cherry_model = 0;      // model version the plan's cherry tables were scheduled for
    // k_traverse4: leaf-leaf ops the planner removed (select_pair_children).  Their slabs are marked virtual at every submission
    // of the plan, a cached one included; nrows is the caller's op count (DevOp::out_row < nrows), small_nops the ops left
    struct Virtual { int slab; int32_t taxon_l, taxon_r; double len_l, len_r; };
    std::vector<Virtual> virt;
    int nrows = 0;
    // k_traverse4: doubles of the plan's fill image, the sum of its chunks' region extents (0: a plan of another kernel), and
    // whether the plan may have one at all (lay_out_lds: not with device-side lengths; small plans are excluded at submission)
    int64_t image_doubles = 0;
    bool image_ok = false;
};

// What the descriptors in d_ops were built from: an identical op list (same keys, leaves, lengths) with an unchanged key
// map needs no rebuilding at all
struct PlanCache {
    std::vector<char> ops_in;     // the caller's op list
    std::vector<int> segs;        // explicit segment sizes
    uint64_t version = 0;         // keymap_version the plan was built at (0: never re-used)
    int dst = -1;                 // slab the plan's last op writes
    std::vector<char> uploaded;   // bytes of the descriptors currently in d_ops
    void invalidate() { version = 0; uploaded.clear(); }
};

// Optimization::minimizeNewton (optimization.cpp:388-465) as a state machine that is advanced once per derivative
// evaluation: `newton_init`, then after every evaluation at `rts` one `newton_update(sum f*df_ptn, sum f*ddf_ptn)`
// until `done`.  It is the one statement of the rule: the in-kernel solvers (k_newton, k_newton_batch, k_sweep4, the
// pair, quartet and partition solvers) run it in every workgroup, sharded engines in a 1-thread kernel (derivative
// kernel -> all-reduce of {df, ddf} -> update kernel, all enqueued, no host round trip per step), single-process
// sharding on the host (pinned-host reduction), and the CPU tests compare it with the reference's loop.
// newton_update = newton_repair + newton_advance.  A caller with a +ASC correction to add puts it between the two
// (k_newton, k_newton_batch: a non-finite corrected sum then ends the solve with status 2, as in the reference); the
// chain forms add the correction first and call newton_update, which repairs such a sum once more.
struct __attribute__((aligned(16))) NewtonState {
    double x1, x2, xacc;
    double rts, rts_old, xl, xh, dx, f, df, d2l, result;
    int32_t max_steps, j, neval, status;  // status: 0 ok, 2 non-finite derivative, 3 step limit
    int32_t done, _pad[3];
};

__host__ __device__ inline void newton_init(NewtonState &s, double xguess, double x1, double x2, double xacc,
                                            int max_steps) {
    s.x1 = x1; s.x2 = x2; s.xacc = xacc;
    s.rts = xguess;
    if (s.rts < x1) s.rts = x1;
    if (s.rts > x2) s.rts = x2;
    s.rts_old = s.rts; s.xl = x1; s.xh = x2; s.dx = 0.0; s.f = s.df = s.d2l = 0.0;
    s.result = s.rts;
    s.max_steps = max_steps; s.j = 0; s.neval = 0; s.status = 0; s.done = 0;
    s._pad[0] = s._pad[1] = s._pad[2] = 0;
}

__host__ __device__ inline bool newton_finite(double v) { return v == v && v - v == 0.0; }

// computeLikelihoodDerv's repair of a non-finite derivative sum, phylokernel.h:647-651
__host__ __device__ inline void newton_repair(double &pdf, double &pddf) {
    if (!newton_finite(pdf)) { pdf = 0.0; pddf = 0.0; }
}

// +ASC, phylokernel.h:719-724: c = {prob_const_sum, df_const, ddf_const} over the unobserved constant patterns
__host__ __device__ inline void asc_derv_correct(const double *c, double asc_nsites, double &df, double &ddf) {
    const double prob_const = 1.0 - c[0];
    const double df_frac = c[1] / prob_const, ddf_frac = c[2] / prob_const;
    df += asc_nsites * df_frac;
    ddf += asc_nsites * (ddf_frac + df_frac * df_frac);
}

// one step of the rule from f = -dlnL/dt, df = -d2lnL/dt2 at s.rts (computeFuncDerv, phylotree.cpp:2135-2146)
__host__ __device__ inline void newton_advance(NewtonState &s, double f, double df) {
    if (s.done) return;
    s.f = f; s.df = df;
    s.neval++;
    if (s.neval == 1) {
        s.d2l = df;
        if (!newton_finite(f) || !newton_finite(df)) { s.status = 2; s.result = s.rts; s.done = 1; return; }
        if (df >= 0.0 && fabs(f) < s.xacc) { s.result = s.rts; s.done = 1; return; }
        if (f < 0.0) { s.xl = s.rts; s.xh = s.x2; } else { s.xh = s.rts; s.xl = s.x1; }
        s.dx = fabs(s.xh - s.xl);
        s.j = 1;
    } else {
        if (!newton_finite(f) || !newton_finite(df)) { s.status = 2; s.result = s.rts_old; s.done = 1; return; }
        if (df > 0.0 && fabs(f) < s.xacc) { s.d2l = df; s.result = s.rts; s.done = 1; return; }
        if (f < 0.0) s.xl = s.rts; else s.xh = s.rts;
        s.j++;
        if (s.j > s.max_steps) { s.status = 3; s.result = s.rts; s.done = 1; return; }
    }
    s.rts_old = s.rts;
    if ((df <= 0.0) || (((s.rts - s.xh) * df - f) * ((s.rts - s.xl) * df - f) >= 0.0)) {
        s.dx = 0.5 * (s.xh - s.xl);
        s.rts = s.xl + s.dx;
        s.d2l = df;
        if (s.xl == s.rts) { s.result = s.rts; s.done = 1; return; }
    } else {
        s.dx = f / df;
        const double temp = s.rts;
        s.rts -= s.dx;
        s.d2l = df;
        if (temp == s.rts) { s.result = s.rts; s.done = 1; return; }
    }
    if (fabs(s.dx) < s.xacc || s.j == s.max_steps) { s.result = s.rts_old; s.done = 1; return; }
}

__host__ __device__ inline void newton_update(NewtonState &s, double pdf, double pddf) {
    if (s.done) return;
    newton_repair(pdf, pddf);
    newton_advance(s, -pdf, -pddf);
}

// The one place device and pinned-host memory is allocated and freed.  It keeps two process-wide byte counts, device memory
// and pinned / host staging memory (iqhip_debug_memory), and can be told to fail the nth allocation from now without a HIP
// call (iqhip_debug_fail_alloc).  MEM_HOST: plain zeroed host memory, the staging of a planning-only engine.
enum MemKind : int { MEM_DEVICE = 0, MEM_PINNED, MEM_PINNED_MAPPED, MEM_HOST };
inline std::atomic<int64_t> g_mem_bytes[2];   // live through mem_alloc: device, pinned / host staging
inline std::atomic<int> g_fail_alloc_in{0};   // allocations until the one that fails (0: none)
inline hipError_t mem_alloc(void **p, size_t bytes, MemKind kind) {
    *p = nullptr;
    if (g_fail_alloc_in.load() > 0 && g_fail_alloc_in.fetch_sub(1) == 1) return hipErrorOutOfMemory;
    hipError_t s;
    if (kind == MEM_DEVICE) s = hipMalloc(p, bytes);
    else if (kind == MEM_HOST) s = (*p = calloc(1, bytes)) ? hipSuccess : hipErrorOutOfMemory;
    else s = hipHostMalloc(p, bytes, kind == MEM_PINNED_MAPPED ? hipHostMallocMapped : hipHostMallocDefault);
    if (s == hipSuccess) g_mem_bytes[kind != MEM_DEVICE] += (int64_t)bytes;
    return s;
}
inline void mem_free(void *p, size_t bytes, MemKind kind) {
    if (kind == MEM_DEVICE) hipFree(p);
    else if (kind == MEM_HOST) free(p);
    else hipHostFree(p);
    g_mem_bytes[kind != MEM_DEVICE] -= (int64_t)bytes;
}

// What DevBuf and PinBuf share: the allocation and its release.  Movable, not copyable; frees itself.
template <typename T>
struct OwnedBuf {
    T *p = nullptr; size_t cap = 0;   // cap in elements
    OwnedBuf() = default;
    OwnedBuf(OwnedBuf &&o) noexcept { swap(o); }
    OwnedBuf &operator=(OwnedBuf &&o) noexcept { swap(o); return *this; }
    ~OwnedBuf() { reset(); }
    void swap(OwnedBuf &o) { std::swap(p, o.p); std::swap(cap, o.cap); std::swap(bytes, o.bytes); std::swap(kind, o.kind); }
    void reset() {
        if (bytes) mem_free(const_cast<std::remove_cv_t<T> *>(p), bytes, kind);
        p = nullptr; cap = 0; bytes = 0;
    }
protected:
    // a buffer of `count` elements in place of the old one, whose contents are dropped, once stream `s` has drained;
    // cap == 0 while the allocation has failed
    hipError_t replace(hipStream_t s, size_t count, MemKind k) {
        if (k != MEM_HOST) {
            const hipError_t rc = hipStreamSynchronize(s);
            if (rc != hipSuccess) return rc;
        }
        reset();
        void *q = nullptr;
        const hipError_t rc = mem_alloc(&q, count * sizeof(T), k);
        if (rc != hipSuccess) return rc;
        p = static_cast<T *>(q); cap = count; bytes = count * sizeof(T); kind = k;
        return hipSuccess;
    }
    size_t bytes = 0;   // what mem_alloc gave (0: nothing, or a planning-only engine's fake address)
    MemKind kind = MEM_DEVICE;
};

// A device buffer that grows on demand.  ensure(e, count): nothing while count <= cap; otherwise the buffer is replaced --
// the engine's stream drains, the old contents are dropped, cap stays 0 while an allocation has failed, and a planning-only
// engine gets a fake address.  ensure(stream, count): the same for an owner that belongs to no engine.  The destructor frees
// the memory (never a fake address): iqhip_destroy makes the device current and drains the stream before it deletes the engine.
template <typename T>
struct DevBuf : OwnedBuf<T> {
    hipError_t ensure(hipStream_t s, size_t count) { return count <= this->cap ? hipSuccess : this->replace(s, count, MEM_DEVICE); }
    hipError_t ensure(iqhip_engine *e, size_t count);
};
// Its pinned-host counterpart; mapped: the memory is mapped into the device address space (the result vector the reduction
// kernel writes, the sequence number the host polls).  A planning-only engine gets plain host memory and makes no HIP call.
template <typename T>
struct PinBuf : OwnedBuf<T> {
    hipError_t ensure(hipStream_t s, size_t count, bool mapped = false) {
        return count <= this->cap ? hipSuccess : this->replace(s, count, mapped ? MEM_PINNED_MAPPED : MEM_PINNED);
    }
    hipError_t ensure(iqhip_engine *e, size_t count, bool mapped = false);
};
// a device buffer with its pinned staging copy
template <typename T>
struct PairBuf {
    DevBuf<T> d; PinBuf<T> h;
    template <typename Where>   // an engine or a stream
    hipError_t ensure(Where w, size_t count) {
        const hipError_t rc = d.ensure(w, count);
        return rc != hipSuccess ? rc : h.ensure(w, count);
    }
};

struct Slab {
    DevBuf<double> plh;
    DevBuf<int16_t> sc;
    // virtual: the vector is that of the leaf-leaf node update (taxon_l, taxon_r, len_l, len_r), which the planner removed from
    // the submission that names it; the memory holds something older until slab_for_key(create = false) expands it
    bool virt = false;
    int32_t taxon_l = -1, taxon_r = -1;
    double len_l = 0.0, len_r = 0.0;
};

// UFBoot bookkeeping of an engine (iqhip_ufboot_*) or of a partition group (iqhip_partition_ufboot_*); ufboot.hip,
// kernels_ufboot.hip, kernels_partboot.hip.  Per replicate boot_logl, boot_orig_logl [nsamples each, in `dbl`], boot_tree
// [nsamples], boot_counts [nsamples]; the entries of a call with `row` rewritten to the row of the chunk's sums; res =
// {replaced slots (64-bit integer), wgmin [workgroups]}.  nsamples == 0: no state (before the owner's init, and after a
// sample matrix it was initialised on was replaced)
struct UfbootState {
    DevBuf<double> dbl, res;
    DevBuf<int64_t> tree;
    DevBuf<int32_t> counts;
    DevBuf<iqhip_ufboot_tree> entries;
    int nsamples = 0;
    double ms[2] = {0.0, 0.0};   // the owner's timing read-out: the products, the update kernels (while timing is enabled)
    int64_t launches = 0;        // kernels the last update enqueued
};

}  // namespace iqhip

struct iqhip_engine {
    int device = 0;
    // planning-only engine (iqhip_debug_create_planner): no HIP call is ever made for it; "device" allocations are
    // distinct fake addresses that are never dereferenced.  It exists so that the planner (plan.hip build_plan, check_plan)
    // runs in CPU tests (tests/test_plan_check.py): the descriptors a kernel would receive are validated without a GPU.
    bool planner = false;
    uint64_t fake_next = 0x100000000000ull;
    bool check_plans = false;  // IQHIP_CHECK_PLAN=1 (always on for a planner): validate every DevOp before upload
    int n = 0, ncat = 0, ntaxa = 0;
    // Binary data (2 states; phylotreesse.cpp:262-276 binds <Vec2d, 2, 2>): embedded EXACTLY into the 4-state kernels --
    // the eigen-system is padded block-diagonally (U = diag(U2, I2), eigenvalues (l0, l1, 0, 0)), so components 2, 3 of
    // every vector are identically zero, and a missing character becomes the ambiguity set {0, 1} (DNA code 6 = "A or
    // C", whose tip vector is the caller's unknown row) instead of the kernels' "unknown = exactly 1.0 in every
    // component" rule, which would leak into the padding.  n stays 4 internally; the ABI speaks n_user = 2.
    bool embed2 = false;
    // The same embedding carries every state count the reference hands to its scalar kernel (3, 5 .. 19, 21 .. 63: morphological
    // / multi-state data, phylotreesse.cpp:281-309) on the next kernel size up (4 / 20 / 64): U = diag(U_m, I), zero
    // eigenvalues and zero tip components in the padding; internal state n = "missing" (the caller's unknown row), the
    // kernels' own unknown state n + 1 never occurs.  scalar_rule_all: such engines apply the scalar kernel's scaling rule
    // (IQHIP_OP_SCALAR_RULE, incl. its lh_max == 0 branch) at every node, as the reference does for them.
    bool scalar_rule_all = false;
    int n_user = 0;
    int64_t nptn = 0;      // caller-visible patterns
    int64_t nptn_pad = 0;  // padded to the tile size
    int64_t ntiles = 0;    // tiles of `tile` patterns
    int tile = 64;         // 64 (VALU path) or 16 (MFMA path)
    bool mfma = false;     // nstates 20 / 64: matrix-core path (kernels_mfma.hip)
    bool mfma_pipelined = false;  // (n, ncat) has a k_traverse_mfma2 instantiation and the model has one class
    bool row_split = false; // 64 states, 1 category: one wave per 16 output rows of a tile (small alignments)
    bool cat_split = false; // 20 states, 4 categories: one wave per category of a tile (small alignments)
    bool top_cs2 = false;   // 20 states, 4 categories: the sequential top stage with two waves per tile (two categories each), IQHIP_TOP_CS2
    int lane_split = 1;    // 4-state traversal: lanes per pattern (2: each lane owns half of the categories)
    // wide DNA: exactly 4 states with 9 .. 32 categories or components.  Such an engine lives on the 16-pattern tile
    // layout from creation (mfma semantics: tile 16, no lane split, no small plans, no persistent sweep) whatever its
    // number of classes; its node update is the padded matrix-core kernel k_traverse_mfma<4, 256, true> (IQHIP_WIDE4=generic,
    // the default) or, with IQHIP_WIDE4=valu, k_traverse4w (kernels_valu4w.hip) on the same plans
    bool wide4 = false, wide4_generic = false;
    int lane_split_valu = 1;  // ... remembered while a 4-state engine runs a mixture on the matrix-core kernels
    bool mix_split = false;   // k_traverse_mfma_mix20: one wave per quarter of a tile's components (small alignments; IQHIP_CAT_SPLIT)
    bool mixed_top = true; // 64 states: mixed-role top stage (kernels_mfma.hip k_traverse_mfma_top64; IQHIP_MIXED_TOP)
    // The 4-state traversal parks join operands in a second register set (HOLD, plan.hip park_operands).
    // 20-state pipelined kernel: the same idea with the parking place in LDS (10 KB per wave) -- a result that is the
    // streamed child of a later op of the same unit is kept there instead of being read back from memory (IQHIP_HOLD_LDS)
    bool hold_lds = true;
    int lds_budget_bytes = 64 * 1024;  // per-workgroup LDS for the per-branch regions (IQHIP_LDS_KB)
    bool small_plans = true;     // IQHIP_SMALL_PLANS (iqhip::Plan::small)
    int split_target = -1;       // IQHIP_SPLIT: -1 auto, 0 never, n > 0: unit size (plan.hip cut_units)
    int max_levels = 3;          // IQHIP_LEVELS: stages of units at most
    int mfma_lds_kb = -1;        // IQHIP_MFMA_LDS_KB: LDS per matrix-core workgroup (-1: by state count, plan.hip lds_budget)
    bool debug_plan = false;     // IQHIP_DEBUG_PLAN: print each plan's staging and parking to stderr
    bool debug_sweep = false;    // IQHIP_DEBUG_SWEEP: print where a sweep's host and kernel time went to stderr
    std::string debug_break_plan;  // IQHIP_DEBUG_BREAK_PLAN (planning-only engines): break one descriptor on purpose
    iqhip::Plan plan;            // the current plan (plan.hip build_plan)
    iqhip::Slab dummy;           // valid target of unconditional prefetches
    int block = 0;         // n*ncat
    int state_unknown = -1;
    bool model_set = false, aln_set = false, theta_valid = false;
    // +ASC (phylokernel.h:868-909,655-725,1124-1187): the last n_unobs patterns are the unobserved
    // constant patterns; asc_nsites = aln->getNSite()
    int64_t n_unobs = 0;
    // pattern-sharded runs: the correction is active on EVERY shard / rank (asc_active), while the unobserved patterns --
    // appended at the end of the alignment -- sit on the last one(s) only (n_unobs = this engine's share, possibly 0);
    // the sums prob_const / df_const / ddf_const travel with the result vector through the all-reduce
    bool asc_active = false;
    double asc_nsites = 0.0;
    double pattern_lh_shift = 0.0;        // log(1 - prob_const) of the last lnL evaluation
    const int16_t *theta_a_sc = nullptr;  // scale counters of the ends theta was built from (they point into slabs)
    const int16_t *theta_b_sc = nullptr;
    iqhip_branch_end theta_end[2] = {{0, -1, 0}, {0, -1, 0}};   // ... and the ends as the caller named them (a leaf end first)

    hipStream_t stream = nullptr;
    bool own_stream = false;

    // alignment side
    iqhip::DevBuf<uint8_t> d_states;  // [ntaxa][nptn_pad]
    iqhip::DevBuf<double> d_freq, d_invar;
    // model side (these point into d_model)
    double *d_eval = nullptr, *d_evec = nullptr, *d_inv_evec = nullptr;
    double *d_rates = nullptr, *d_props = nullptr, *d_tip = nullptr;
    std::vector<double> h_eval, h_rates, h_props;
    std::vector<int> h_cls;      // category -> class of the last set_model call (all 0 for a plain model)
    // per-call buffers
    iqhip::DevBuf<iqhip::DevOp> d_ops;   // (with its pinned staging copy h_ops: plan.hip ensure_plan_capacity)
    iqhip::DevBuf<double> d_slab;   // wave partials [nvals][nwaves]
    iqhip::DevBuf<unsigned int> d_fold_ticket;  // folded reduction (FoldArgs): ticket + per-row flags, zero between launches
    iqhip::DevBuf<int> d_fold_flags;
    bool fold_reduce = false;               // IQHIP_FOLD=1: the last kernel of a submission sums the slab itself (measured
                                            // slower than the k_reduce launch on MI355X; off by default)
    // host polling of the result (IQHIP_POLL): k_reduce's last block stores a sequence number to mapped host memory
    bool poll_result = true, poll_pending = false;
    unsigned long long result_seq = 0;
    iqhip::PinBuf<volatile unsigned long long> h_done;   // (mapped)
    unsigned long long *d_done = nullptr;       // the device address of h_done
    iqhip::DevBuf<double> d_theta, d_pattern_lh;
    // K2 tables of the leaf children (matrix-core pipelined kernels, kernels_mfma.hip k_leaf_tables).  A table depends
    // on (model, pendant branch length) only, so slot t < ntaxa belongs to taxon t and is rebuilt only when that
    // length or the model changed; a second length of one taxon inside one submission (batched NNI candidates)
    // takes an overflow slot >= ntaxa.
    iqhip::DevBuf<double> d_leaf_tab;     // whole tables of leaf_table_doubles(e) each
    std::vector<double> tab_len;          // per slot: branch length the table was built for (NaN: none)
    uint64_t model_version = 1, tab_model_version = 0;
    // cherry tables (20 states x 4 categories, DevOp::cherry): slot = pair of taxa; `pair` is a small engine of our own on
    // the same stream whose pseudo-alignment lists every pair of states -- a cherry's table is that engine's ordinary
    // node update for the two pendant lengths, moved into register order by k_cherry_transpose
    struct CherrySlot {
        double len_l = -1.0, len_r = -1.0;
        uint64_t model_version = 0;   // model the table was built for (0: never built)
        uint64_t stamp = 0;           // last plan that used the slot
    };
    bool cherry_on = true;                 // IQHIP_CHERRY_TABLES=0 switches the tables off
    iqhip_engine *pair = nullptr;
    int cherry_s2 = 0, cherry_npairs = 0;  // STATE_UNKNOWN + 1; its square padded to whole 64-pattern groups
    iqhip::DevBuf<double> d_cherry_tab;    // whole slots of cherry_npairs * block doubles each
    std::unordered_map<uint64_t, int> cherry_slot_of;   // (taxon_l << 32 | taxon_r) -> slot
    std::vector<CherrySlot> cherry_slots;
    uint64_t cherry_stamp = 0;
    int64_t cherry_built_total = 0, cherry_ops_total = 0;   // tables built / node updates answered from a table so far
    // Newton / sweep forms, read when the engine is created: IQHIP_NEWTON=chain (enqueued chain instead of the one-launch
    // k_newton), IQHIP_SWEEP=0 (sweeps step by step with a host round trip each), IQHIP_SWEEP_KERNEL=0 (4-state sweeps as
    // two launches per step instead of k_sweep4)
    bool newton_chain_forced = false, sweep_one_submission = true, sweep_persistent = true;
    // since creation, the IQHIP_PATH_* slots of include/iqhip.h (iqhip_debug_path_counts)
    int64_t path_counts[IQHIP_PATH_NSLOTS] = {};
    bool cherry_model_synced = false;      // the pair engine has the model of this engine's last set_model call
    bool leaf_tables = false;       // IQHIP_LEAF_TABLES (default on for the pipelined matrix-core kernels)
    // Mixture models (phylokernelmixture.h, phylokernelmixrate.h): the ncat categories are (class, rate)
    // components; category c uses eigen-system cat_class[c].  Per-category expansions for the kernels
    // that are generic in (n, ncat): evalc[c][i], tipc[state][c][i]; per-class MFMA A images for the
    // mixture traversal kernel.  A plain model is the one-class case.
    int nclass = 1;
    double *d_evalc = nullptr;   // [ncat][n]
    // 20 / 64 states, class 0: the A-operand fragments of U and U^-1 in the exact order of the pipelined kernels' LDS
    // image ([U 16-row tiles][U^-1 tiles][U tail][U^-1 tail], element (m, s, lane) = row 16m + (lane & 15), column
    // 4s + (lane >> 4)), so that a workgroup stages it with 16-byte coalesced copies: gathered element by element
    // from evec / inv_evec the 64 KB of 64 states cost every workgroup 10-15 us before its first matrix instruction
    // (wave trace, r02)
    double *d_aimg = nullptr;
    int aimg_doubles = 0;
    double *d_tipc = nullptr;    // [state_unknown+1][ncat][n]
    int *d_cls = nullptr;        // [ncat]
    iqhip::DevBuf<double> d_img;     // mixture A images: mix20 layout, then the generic kernel's (engine.hip)
    size_t img_generic_off = 0;
    iqhip::DevBuf<double> d_model;   // the block all model arrays above point into (set_model_common)
    bool mfma_pipelined_ok = false;  // (n, ncat) has a pipelined instantiation (used when nclass == 1)
    // UFBoot / RELL (kernels_rell.hip): scaled per-pattern lnL and the bootstrap sample matrix
    iqhip::DevBuf<double> d_ptn_scaled;
    iqhip::DevBuf<float> d_boot;  // [nboot][nptn_pad], zero padded
    int nboot = 0;
    uint64_t boot_generation = 0;   // advances, by one or more, whenever the matrix or its contents are replaced: only inequality
                                    // means something (a partition group's UFBoot state records it at init and is void once it differs)
    // branch tests (SH-aLRT / local bootstrap, ptnlh.hip): the store of per-pattern log-likelihood rows [ptnlh_rows][nptn_pad]
    // and the scratch of iqhip_branch_tests / iqhip_ptnlh_rell (row lists, K-split partial products, combined sums, results)
    iqhip::DevBuf<double> d_ptnlh;
    int ptnlh_rows = 0;
    struct {
        iqhip::DevBuf<int32_t> rows;    // [distinct rows] ++ [3 * nbranch indices into them]
        iqhip::DevBuf<double> part;     // [ksplit][M][nsamples]
        iqhip::DevBuf<double> sums;     // [M][nsamples]
        iqhip::DevBuf<double> out;      // lh3 [3 * nbranch] ++ iqhip_branch_support [nbranch]
    } bt;
    // tree topology tests (kernels_topo.hip): int64 inclusive prefix sums of ptn_freq for iqhip_gen_boot_samples (built when
    // first needed, dropped by iqhip_set_ptn_freq) and the scratch of iqhip_ptnlh_diff_variance / iqhip_tree_tests /
    // iqhip_multiscale_bp
    iqhip::DevBuf<int64_t> d_freq_prefix;
    bool freq_prefix_valid = false;
    int64_t freq_nsite = 0;
    struct {
        iqhip::DevBuf<double> var;      // [n][n] variances of the pairwise differences
        iqhip::DevBuf<double> dbl;      // lh, avg, w_orig [T each] ++ weights [T][T] ++ max_sh, max_elw, sum_l [S each] ++ out [6 T]
        iqhip::DevBuf<int32_t> ints;    // kh_id, w_id [T each] ++ winner [S]; iqhip_multiscale_bp: counters [nscales][T]
    } tt;
    // UFBoot bookkeeping (iqhip_ufboot_*, read out by iqhip_debug_ufboot_timing)
    iqhip::UfbootState ufb;
    // EM for +R free-rate models and empirical-Bayes site rates (classlh.hip, kernels_em.hip): what the last E-step left -- the
    // posterior matrix W [ncat][nptn_pad] (category-major, padding patterns 0), per pattern its posterior mean rate and
    // best category -- and the scratch of the sums (workgroup rows, folded values).  valid: an E-step has run for an
    // engine of these dimensions
    struct {
        iqhip::DevBuf<double> w, rate, part, out;
        iqhip::DevBuf<int32_t> cat;
        bool valid = false;
        double ms[2] = {0.0, 0.0};   // iqhip_debug_em_timing: the last E-step / objective launches (while timing is enabled)
    } em;
    // EM for mixture class weights, class posteriors, pattern state frequencies (classlh.hip, kernels_mixem.hip): the class
    // likelihoods Lc [nclass][nptn_pad] of the last iqhip_mix_class_lh (class-major, padding patterns 0) with the model
    // version and dimensions they belong to (0: none), the per-class component lists (first [nclass + 1] ++ components), the
    // state of an EM run (kernels_mixem.hip MIXEM_*), the workgroup rows of its sums, posteriors / state frequencies scratch
    struct {
        iqhip::DevBuf<double> lc, state, part, post, cfreq;
        iqhip::DevBuf<int32_t> list;
        uint64_t model_version = 0;
        int64_t nptn_pad = 0;
        int nclass = 0;
        double ms[2] = {0.0, 0.0};   // iqhip_debug_mix_timing: the class-lh launch, the EM chain (while timing is enabled)
        int64_t launches = 0;        // kernels the last EM chain enqueued
    } mix;
    // per-class log-likelihoods (iqhip_class_lnl; classlh.hip, kernels_classlnl.hip): the per-class component lists as mix.list,
    // the class weights [nclass], the caller's per-class invariant terms [nclass][nptn_pad], the workgroup rows of the sums
    // and the folded values {lnl, floored} [2 nclass].  mixture_api: the model came through iqhip_set_mixture_model
    struct {
        iqhip::DevBuf<double> cw, inv, part, out;
        iqhip::DevBuf<int32_t> list;
        double ms = 0.0;             // iqhip_debug_class_lnl_timing: the last call's two launches (while timing is enabled)
    } cl;
    bool mixture_api = false;
    // pairwise ML distances (pairdist.hip, kernels_dist.hip): tiles of the pair list, the counts of one chunk of pairs [chunk][n * n], the
    // coefficients evec[i][k] * inv_evec[k][j] of the call's model [n][n][n], per pair the initial distance and the result
    // {optx, d2l, evaluations, status}; with iqhip_timing_enable the device time of the last iqhip_pair_distances call
    struct {
        iqhip::DevBuf<iqhip::PairTile> tiles;
        iqhip::DevBuf<double> counts, coef, init, out;
        double ms[2] = {0.0, 0.0};   // iqhip_debug_pair_timing: the count launches, the solve launches
    } pd;
    // likelihood mapping (quartet.hip, kernels_quartet.hip): the taxa of the call's quartets, one chunk's cell tables
    // [chunk][256], other-list lengths [chunk] and other-lists [chunk][nptn], the results of the call; with
    // iqhip_timing_enable the device time of the last iqhip_quartet_likelihoods call
    struct {
        iqhip::DevBuf<int32_t> quartets, nother, other;
        iqhip::DevBuf<double> cells;
        iqhip::DevBuf<iqhip_quartet_result> out;
        double ms[2] = {0.0, 0.0};   // iqhip_debug_quartet_timing: the cell launches, the solve launches
    } qt;
    // BIONJ (kernels_bionj.hip): the device memory lives for one call; iqhip_debug_bionj_timing reads these
    struct {
        double ms = 0.0;
        int64_t launches = 0;
    } bj;
    // Fitch parsimony (pars.hip, kernels_pars.hip).  Host copies of what iqhip_pars_init reads: ptn_freq
    // (iqhip_set_ptn_freq), class 0's eigenvectors and tip table (set_model_common).  Vectors [ntaxa + nvectors] of
    // pars_nwords * n words (4 states: word-major, a column is one 16-byte load; 20 / 64 states: plane-major, lanes on
    // consecutive columns coalesce) and their score columns [ntaxa + nvectors][pars_nwords]; one valid flag per caller slot
    std::vector<double> h_freq, h_evec0, h_tip0;
    bool pars_ready = false;
    int pars_nvec = 0;
    int64_t pars_nsites = 0, pars_nwords = 0;
    std::vector<uint8_t> pars_valid;
    struct {
        iqhip::DevBuf<uint32_t> vec, score;
        iqhip::DevBuf<int32_t> ints;    // per call: ops ++ level starts, or branch ends; init: the pattern of every site
        iqhip::DevBuf<int32_t> out;     // score [nbranch] ++ subst [nbranch] ++ {best, best_score}
        iqhip::DevBuf<uint64_t> masks;  // [state_unknown + 1] the states a code allows
    } pars;
    // pinned staging, one buffer per direction and kind so that none is rewritten while a copy of it may be in flight: the
    // levelled ops of an update (rewritten only after a synchronise), the branch ends and the results of a scores call
    // (every scores call ends with a synchronise)
    iqhip::PinBuf<int32_t> h_pars_ops, h_pars_ends, h_pars_out;
    double pars_ms[2] = {0.0, 0.0};     // iqhip_debug_pars_timing: update, scan (while timing is enabled)
    int64_t pars_counts[4] = {0, 0, 0, 0};   // launches of the updates and of the scans, ops updated, branches scanned
    double pars_spr_ms = 0.0;           // iqhip_debug_pars_spr_timing: the SPR scan launches (while timing is enabled) ...
    int64_t pars_spr_counts[2] = {0, 0};   // ... their number and the steps scored
    double pars_batch_ms = 0.0;         // iqhip_debug_pars_batch_timing: the segmented insertion scans (while timing is enabled) ...
    int64_t pars_batch_counts[3] = {0, 0, 0};   // ... their launches (scores + first minima), branches and segments
    iqhip::DevBuf<int32_t> d_batch_rows;   // iqhip_optimize_branch_batch_rows: store row per task of a chunk
    // the result vector the kernels write: d_result_own is the device address of h_result, d_result that or d_result_dev
    double *d_result_own = nullptr, *d_result = nullptr;
    iqhip::DevBuf<double> d_newton_partials;   // [2][num_cus][2]
    iqhip::DevBuf<unsigned int> d_newton_barrier;  // [2], used alternately by consecutive k_newton launches
    unsigned int newton_launches = 0;
    // k_newton's exchange of the workgroup partial sums without an arrival counter: every (evaluation, workgroup) has a
    // slot of its own, {df, ddf}, that holds a sentinel until its owner posts; readers spin on the slots themselves.
    // Two buffers alternate between launches; a launch resets the other buffer's slots of its workgroups.
    iqhip::DevBuf<double> d_newton_posts;  // [2][kNewtonPostEpochs][num_cus][2]
    unsigned int newton_post_launches = 0;
    bool newton_posts = true;              // IQHIP_NEWTON_POSTS=0: the arrival-counter barrier of round 1
    // the same for k_newton_batch: [2 launch parities][cap / 2]; a launch lays its slots out as
    // [task][evaluation][workgroup][2] and resets what the previous launch of the other parity used
    iqhip::DevBuf<double> d_batch_posts;
    size_t batch_posts_used[2] = {0, 0};
    unsigned int batch_post_launches = 0;
    // batched branch optimisation (iqhip_optimize_branch_batch): per-task theta buffers, partial sums, arrival
    // counters (two sets, alternating per launch), results and the task descriptors
    iqhip::DevBuf<double> d_theta_batch, d_batch_partials, d_batch_out;
    iqhip::DevBuf<unsigned int> d_batch_barriers;
    iqhip::DevBuf<char> d_batch_tasks;   // NewtonTask descriptors (kernels_newton.hip), as bytes
    int batch_cap = 0;                   // tasks all four were last grown for
    unsigned int batch_launches = 0;
    iqhip::DevBuf<double> d_sweep_len;   // iqhip_optimize_sweep: the accepted length of every step, read by later steps' node updates
    // ... persistent form (4 states): descriptors of all steps (pinned staging + device copy) and the exchange slots
    iqhip::PinBuf<char> h_sweep_desc;
    iqhip::DevBuf<char> d_sweep_desc;
    iqhip::DevBuf<unsigned long long> d_sweep_prof;   // IQHIP_DEBUG_SWEEP: k_sweep4's cycle counters (kernels_sweep.hip)
    iqhip::DevBuf<double> d_sweep_posts;
    int num_cus = 256;
    int result_cap = 0;
    // ---- collectives (comm.hip).  comm != nullptr: this engine is one rank of a pattern-sharded run; every
    // host-visible sum is all-reduced (ncclAllReduce, SUM, f64, in place in the device result vector, on the engine's
    // stream) before it is read back.  RCCL is loaded lazily (dlopen) the first time a communicator is made.
    void *comm = nullptr;            // ncclComm_t
    int comm_nranks = 1, comm_rank = 0;
    iqhip::DevBuf<double> d_result_dev;  // device-memory result vector of a comm engine (the default one is mapped host memory)
    iqhip::DevBuf<iqhip::NewtonState> d_nstate;   // Newton state machine: device copy ...
    iqhip::PinBuf<iqhip::NewtonState> h_nstate;   // ... / pinned host copy
    iqhip::DevBuf<iqhip::NewtonState> d_bstates;                  // batched chain: one state machine per task
    iqhip::DevBuf<const int16_t *> d_bsc;                         // ... and (+ASC) the scale counters of its two branch ends
    // ---- single-process sharding (sharded.hip): this object owns no device memory, it fronts `shards`
    // (pattern ranges [shard_first[g], shard_first[g+1]) on the devices of iqhip_create_sharded)
    std::vector<iqhip_engine *> shards;
    std::vector<int64_t> shard_first;
    int reduce_mode = 0;             // IQHIP_REDUCE_RCCL / IQHIP_REDUCE_HOST
    // pinned host staging
    iqhip::PinBuf<iqhip::DevOp> h_ops;   // (plain host memory on a planning-only engine)
    iqhip::PinBuf<double> h_result;      // (mapped)
    iqhip::PlanCache plan_cache;
    iqhip::PinBuf<char> h_plan_arena;     // pinned slices for the plan uploads of a per-step sweep (plan.hip upload_plan)
    size_t plan_arena_used = 0;
    bool plan_arena_on = false;
    uint64_t keymap_version = 1;      // bumped whenever a key is created, released or moved
    hipEvent_t staging_free = nullptr;
    bool staging_busy = false;

    // pair children (CHILD_PAIR).  taxon_plain[t]: the taxon's row holds only states 0 .. 3 and STATE_UNKNOWN (recorded by
    // iqhip_set_alignment; empty: unknown, nothing is virtualised).  Pair-code rows: slot = ordered pair of taxa, nptn_pad bytes
    // each, built once per pair by k_pair_codes; the slots start over when a new plan finds them all taken or the alignment changes
    std::vector<char> taxon_plain;
    // the keys of the root-branch ends of the submission being planned (submit_traverse): their ops stay real -- the root
    // pass reads those vectors from memory, a virtual one would be expanded at every submission
    uint64_t root_end_keys[2] = {0, 0};
    int n_root_end_keys = 0;
    iqhip::DevBuf<uint8_t> d_pair_rows;
    std::unordered_map<uint64_t, int> pair_row_of;   // (taxon_l << 32 | taxon_r) -> slot
    int64_t pair_ops_removed = 0, pair_slabs_expanded = 0;   // iqhip_debug_pair_children
    int64_t pair_row_restarts = 0, pair_ops_without_row = 0; // iqhip_debug_pair_rows

    // k_traverse4's fill image (DESIGN.md 3.1 "Fill image"): every chunk's plan regions as the in-kernel fill leaves them, built by
    // k_fill4_image for the current plan and model and copied into LDS by the traversal instead of being computed per workgroup.
    // model: the model_version the image was built at (0: stale -- every build_plan that planned anew resets it).  plan_hit: the
    // last build_plan found its plan cached.  use: the launches of the submission in progress take the copy path.
    struct FillImage {
        iqhip::DevBuf<double> buf;
        uint64_t model = 0;
        bool on = true, plan_hit = false, use = false;
        int64_t built = 0, reused = 0;   // iqhip_debug_fill_image
    } fill_image;

    // key -> slab
    std::unordered_map<uint64_t, int> key2slab;
    std::vector<iqhip::Slab> slabs;
    std::vector<int> free_slabs;

    // timing of the dominant kernel
    bool timing = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> tev;
    size_t tev_used = 0;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> cev;  // ... around the engine's own all-reduces (comm.hip)
    size_t cev_used = 0;
    int64_t tev_launches = 0;  // traversal-kernel launches inside the recorded brackets
    int last_nops = 0;
    bool last_has_root = false, last_root_loads_b = false;  // ... of the last submission (iqhip_timing_plan_bytes)
    // the last submission's reduction was folded into its kernel and the host polls: the kernel wrote only the rows it
    // summed plus, behind them, the number of flagged sum_scale rows; read_result zero-fills the rest when that is 0
    int folded_rows = -1;
};

namespace iqhip {

// ---------------------------------------------------------------------------------------------------------------
// Reduction folded into the producing kernel ("last workgroup sums"): every wave leaves its partial sums in the slab
// [row][wave]; rows: 0 = lnL (or df), 1 = prob_const (or ddf), 2+k = sum_scale of node update k.  sum_scale rows are
// zero unless some pattern was rescaled at that node, so a wave that did rescale also raises flags[row]; the last
// workgroup to finish sums row 0/1 and the flagged rows in k_reduce's order (same bits) and writes 0.0 for the rest.
// Hand-off between workgroups (MI355X_MICROARCH.md, valid forms): partials are agent-scope (sc1, write-through)
// stores, each wave drains them (s_waitcnt vmcnt(0)) before the workgroup barrier, one lane then takes a ticket with
// an agent-scope atomic; the workgroup that draws the last ticket reads with agent-scope (sc1) loads.
// ---------------------------------------------------------------------------------------------------------------
struct FoldArgs {
    double *slab;          // [rows][nwaves]
    double *result;        // result[row]
    unsigned int *ticket;  // zero between launches
    int *flags;            // [rows], zero between launches
    int nwaves;
    int nrows_scale;       // sum_scale rows (2 .. 2+nrows_scale)
    int root_rows;         // 0: none; 2: rows 0 and 1 hold the root-branch sums
    int enabled;
    // non-NULL: result is mapped host memory; the last workgroup publishes this sequence number for the polling host
    volatile unsigned long long *done;
    unsigned long long seq;
};

#if defined(__HIPCC__)
__device__ __forceinline__ void fold_store(double *p, double v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void fold_flag(const FoldArgs &F, int row) {
    __hip_atomic_fetch_or(&F.flags[row], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// all live threads of a 256-thread workgroup call this once, after their last partial has been stored
__device__ inline void fold_tail(const FoldArgs &F) {
    __shared__ double s_f[256];
    __shared__ int s_last;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned int t = __hip_atomic_fetch_add(F.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_last = (t == gridDim.x - 1) ? 1 : 0;
    }
    __syncthreads();
    if (!s_last) return;
    // Only wave 0 is certain to be alive (the workgroup's trailing waves have exited when the tile count is not a
    // multiple of four), so its 64 lanes do the work; the other live waves only keep the barriers company.
    __shared__ int s_rows[256];
    __shared__ int s_n;
    const int nrows = 2 + F.nrows_scale;
    // one row: k_reduce's order -- 256 strided running sums (lane = 4 of them), then the LDS tree
    auto sum_row = [&](int row) {
        const double *r = F.slab + (size_t)row * F.nwaves;
        if (threadIdx.x < 64) {
            // the four strided running sums of this lane, 8 terms of each at a time: all 32 loads are in flight
            // together (one round trip), the additions keep k_reduce's order
            double acc[4] = {0.0, 0.0, 0.0, 0.0};
            for (int base = 0; base < F.nwaves; base += 8 * 256) {
                double v[4][8];
#pragma unroll
                for (int j = 0; j < 4; j++)
#pragma unroll
                    for (int q = 0; q < 8; q++) {
                        const int i = base + q * 256 + (int)threadIdx.x + 64 * j;
                        v[j][q] = i < F.nwaves ? __hip_atomic_load(&r[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
                    }
#pragma unroll
                for (int j = 0; j < 4; j++)
#pragma unroll
                    for (int q = 0; q < 8; q++) {
                        const int i = base + q * 256 + (int)threadIdx.x + 64 * j;
                        if (i < F.nwaves) acc[j] += v[j][q];
                    }
            }
#pragma unroll
            for (int j = 0; j < 4; j++) s_f[(int)threadIdx.x + 64 * j] = acc[j];
        }
        __syncthreads();
#pragma unroll
        for (int o = 128; o > 0; o >>= 1) {
            if (threadIdx.x < 64)
                for (int v = (int)threadIdx.x; v < o; v += 64) s_f[v] += s_f[v + o];
            __syncthreads();
        }
        if (threadIdx.x == 0) F.result[row] = s_f[0];
        __syncthreads();
    };
    if (F.root_rows) {
        sum_row(0);
        if (F.root_rows > 1) sum_row(1);
        else if (threadIdx.x == 0) F.result[1] = 0.0;   // (no +ASC: the prob_const row is zero)
    }
    // sum_scale rows, 256 at a time: the lanes look at the flags side by side.  With a polling host (F.done) the
    // unflagged rows are not written at all -- 48 stores over PCIe for a 50-taxon plan -- only their count is (the host
    // fills in the zeros, read_result); a device-resident result vector (collectives) gets every row.
    int nflagged = 0;
    for (int base = 2; base < nrows; base += 256) {
        if (threadIdx.x == 0) s_n = 0;
        __syncthreads();
        if (threadIdx.x < 64) {
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int row = base + (int)threadIdx.x + 64 * j;
                if (row < nrows) {
                    if (__hip_atomic_load(&F.flags[row], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) {
                        s_rows[atomicAdd(&s_n, 1)] = row;
                        __hip_atomic_store(&F.flags[row], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    } else if (!F.done) {
                        F.result[row] = 0.0;
                    }
                }
            }
        }
        __syncthreads();
        const int n = s_n;
        nflagged += n;
        if (n > 0 && F.done) {   // some rows are non-zero: the host will read all of them
            if (threadIdx.x < 64)
                for (int j = 0; j < 4; j++) {
                    const int row = base + (int)threadIdx.x + 64 * j;
                    if (row < nrows) {
                        bool flagged = false;
                        for (int q = 0; q < n; q++) flagged = flagged || s_rows[q] == row;
                        if (!flagged) F.result[row] = 0.0;
                    }
                }
        }
        for (int q = 0; q < n; q++) sum_row(s_rows[q]);
    }
    if (F.done && threadIdx.x == 0) F.result[nrows] = (double)nflagged;
    if (threadIdx.x == 0) {
        __hip_atomic_store(F.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (F.done) {
            __threadfence_system();
            *F.done = F.seq;
        }
    }
}
#endif

// engine.hip: records the calling thread's error text (iqhip_last_error) and returns `code`
int set_error(int code, const std::string &msg);
inline int fail(int code, const std::string &msg) { return set_error(code, msg); }
// in a function that returns an IQHIP status: a failed HIP call returns IQHIP_ERR_HIP with the call's text
#define HIPCHK(call)                                                                                           \
    do {                                                                                                       \
        hipError_t _s = (call);                                                                                \
        if (_s != hipSuccess)                                                                                  \
            return iqhip::set_error(IQHIP_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(_s));        \
    } while (0)

// planning-only engines: a distinct, 256-byte aligned address range that is never dereferenced
template <typename T>
T *fake_alloc(iqhip_engine *e, size_t count) {
    const uint64_t a = e->fake_next;
    e->fake_next += (count * sizeof(T) + 255) / 256 * 256 + 256;
    return reinterpret_cast<T *>(a);
}
template <typename T>
hipError_t DevBuf<T>::ensure(iqhip_engine *e, size_t count) {
    if (!e->planner) return ensure(e->stream, count);
    if (count > this->cap) {
        this->p = fake_alloc<T>(e, count);
        this->cap = count;
    }
    return hipSuccess;
}
template <typename T>
hipError_t PinBuf<T>::ensure(iqhip_engine *e, size_t count, bool mapped) {
    if (!e->planner) return ensure(e->stream, count, mapped);
    return count <= this->cap ? hipSuccess : this->replace(nullptr, count, MEM_HOST);
}
// Raises Kernel's dynamic-LDS ceiling to `bytes` on e->device the first time that kernel is launched on that device.  The
// attribute belongs to the device a launch goes to, so there is one flag per (kernel instantiation, device), not one per
// process: every launch after the first costs one branch.  A failure is returned and tried again at the next launch.
constexpr unsigned kLdsCeilingDevices = 64;   // (a device beyond them is opted in at every launch)
template <auto Kernel>
hipError_t raise_lds_ceiling(const iqhip_engine *e, int bytes) {
    static std::atomic<bool> raised[kLdsCeilingDevices];
    const unsigned dev = (unsigned)e->device;
    if (dev < kLdsCeilingDevices && raised[dev].load(std::memory_order_relaxed)) return hipSuccess;
    const hipError_t s = hipFuncSetAttribute(reinterpret_cast<const void *>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (s == hipSuccess && dev < kLdsCeilingDevices) raised[dev].store(true, std::memory_order_relaxed);
    return s;
}
// HIP events around the phases of one feature call, the one event timer of the drivers; nothing at all while `on` is false
// (an engine's e->timing; a partition group takes that of its member 0).  mark() records the next boundary on the timer's
// stream, mark(s) on another one (a group's marks around what a member's stream runs): a round of nphases phases is
// nphases + 1 marks, a call may record any number of rounds (one per chunk, per step, per member) and nothing waits inside
// its loop.  read() waits for the last recorded event -- a caller whose marks went to several streams has drained them all
// by then -- then ms[k] = the time of phase k summed over all rounds; false, ms untouched, while timing is off, nothing was
// recorded or an event call failed.  A failed event call never fails the feature call: the reading is then missing, not the
// result.  The destructor destroys every event, on every return path.
struct PhaseTimer {
    PhaseTimer(bool on, hipStream_t stream_, int nphases_) : stream(stream_), nphases(nphases_), ok(on) {}
    PhaseTimer(iqhip_engine *e, int nphases_) : PhaseTimer(e->timing, e->stream, nphases_) {}
    PhaseTimer(const PhaseTimer &) = delete; PhaseTimer &operator=(const PhaseTimer &) = delete;
    void mark() { mark(stream); }
    void mark(hipStream_t s) {
        hipEvent_t x = nullptr;
        if (!ok || !(ok = hipEventCreate(&x) == hipSuccess)) return;
        ev.push_back(x);
        ok = hipEventRecord(x, s) == hipSuccess;
    }
    bool read(double *ms) {
        const size_t round = (size_t)nphases + 1;
        if (!ok || ev.empty() || ev.size() % round || hipEventSynchronize(ev.back()) != hipSuccess) return false;
        std::vector<double> sum((size_t)nphases, 0.0);
        for (size_t k = 0; k < ev.size(); k += round)
            for (int h = 0; h < nphases; h++) {
                float t = 0.0f;
                if (hipEventElapsedTime(&t, ev[k + h], ev[k + h + 1]) != hipSuccess) return false;
                sum[(size_t)h] += t;
            }
        std::copy(sum.begin(), sum.end(), ms);
        return true;
    }
    ~PhaseTimer() { for (hipEvent_t x : ev) hipEventDestroy(x); }
    hipStream_t stream;
    int nphases;
    bool ok;
    std::vector<hipEvent_t> ev;
};
// engine.hip.  create: a new key gets a slab, and a virtual slab becomes an ordinary one that is about to be written;
// !create: the caller is going to read the slab -- a virtual one is expanded first (launch_pair_expand, on the engine's stream)
int slab_for_key(iqhip_engine *e, uint64_t key, bool create, int *idx);
int expand_virtual_slabs(iqhip_engine *e);   // all of them: before the model, the tip table or the alignment changes
hipError_t launch_pair_expand(iqhip_engine *e, const Slab &s);                                        // kernels_valu4.hip
hipError_t launch_pair_codes(iqhip_engine *e, const uint8_t *row_l, const uint8_t *row_r, uint8_t *out);   // kernels_valu4.hip
// k_traverse4's fill image.  fill_image_submission (plan.hip), after every build_plan: decides whether the submission's launches
// copy the image (e->fill_image.use), counts, and launches the producer when the image is stale -- a planning-only engine counts
// the same way.  launch_fill4_image (kernels_valu4.hip): one workgroup per (op, child) region of the current plan.
int fill_image_submission(iqhip_engine *e);
hipError_t launch_fill4_image(iqhip_engine *e, int nops);
bool cherry_candidate(const iqhip_engine *e);   // engine.hip: the engine uses cherry tables (DevOp::cherry)

// plan.hip -- the planner.  build_plan: one submission's descriptors into h_ops and d_ops, e->plan; *last_dst = the slab
// the last op writes.  explicit_segs: op counts of independent groups (each on its own workgroups); len_ptrs (sweeps):
// 2 * nops device pointers, [2k] / [2k+1] = where op k's left / right child length is found when it runs (nullptr: host)
int build_plan(iqhip_engine *e, const iqhip_node_op *ops, int nops, int *last_dst,
               const std::vector<int> *explicit_segs = nullptr, const double *const *len_ptrs = nullptr);
// the descriptor of a root branch; prev_dst: slab written by the op just before it (-1: none)
int build_branch(iqhip_engine *e, iqhip_branch_end a, iqhip_branch_end b, double len, int prev_dst, DevBranch *br);
// one child of a node op: a leaf's state row or a slab (CHILD_PREV when it is prev_dst)
int resolve_child(iqhip_engine *e, uint64_t key, int32_t leaf, int prev_dst, const double **plh, const int16_t **sc,
                  const uint8_t **states, int32_t *kind);
// After a model change every K2 table is stale: forget what the slots were built for, except the current plan's tables,
// which are then all (re)built.  Returns whether the model changed.
bool leaf_tables_follow_model(iqhip_engine *e);
int lds_budget(const iqhip_engine *e);   // doubles of LDS one chunk's per-(op, child) regions may use

// The dispatch of the matrix-core traversal kernels (kernels_mfma.hip), decided in one place without a HIP call, so that
// the planner and a planning-only engine ask the same function the launcher does.
enum TravVariant : int {
    TRAV_NONE = 0,           // no kernel for this shape
    TRAV_GENERIC,            // k_traverse_mfma<64, 256, nclass > 1>; 4-state mixtures and wide DNA: <4, 256, true>
    TRAV_MIX20,              // k_traverse_mfma_mix20<256, 1>
    TRAV_MIX20_SPLIT,        // k_traverse_mfma_mix20<256, 4>
    TRAV_M2,                 // k_traverse_mfma2<n, ncat, 256, 1, tab>
    TRAV_M2_CAT_SPLIT,       // k_traverse_mfma2<20, 1, 256, 4, tab>
    TRAV_M2_TOP_CS2,         // k_traverse_mfma2<20, 2, 256, 2, false>
    TRAV_TOP20,              // k_traverse_mfma_top20
    TRAV_ROWS64,             // k_traverse_mfma_rows64<256, tab>
    TRAV_TOP64,              // k_traverse_mfma_top64<tab>
    TRAV_WIDE4,              // k_traverse4w<ceil(ncat / 4), nclass > 1> (kernels_valu4w.hip): 4 states, 9 .. 32 categories
};
struct TravLaunch {
    TravVariant variant;
    bool tab;        // leaf children from the K2 tables
    int nfull;       // mixed-role launches: workgroups of the full role (they come first), else 0
    int ngroups;     // workgroups per segment (mixed-role launches: of the other role)
    int grid;
    size_t lds_bytes;
    int hold_off;    // TravMArgs::hold_off
};
TravLaunch choose_traverse_mfma(const iqhip_engine *e, bool top_stage, int nsegs);
// what the planner has to know of that choice before the plan exists
// the top stage may run with several waves per tile (TRAV_M2_TOP_CS2, TRAV_TOP20): no parking places, no cherry block there
inline bool top_stage_may_share_tiles(const iqhip_engine *e) { return e->top_cs2; }
// 64 states: the top stage may give its last tiles to row-split workgroups (TRAV_TOP64)
inline bool top_stage_may_mix_roles64(const iqhip_engine *e) { return e->n == 64 && e->mixed_top; }
// workgroups per segment of k_traverse4: one wave per tile and lane split
inline int trav4_ngroups(const iqhip_engine *e) {
    const int wpb = kTravWg / 64;
    return (int)((e->ntiles * e->lane_split + wpb - 1) / wpb);
}
// the engine's kernel reads a small plan out of its arguments (Plan::small): k_traverse4 and the 20-state pipelined
// kernels without leaf tables (tables come with a job list in the plan buffer)
inline bool kernel_takes_small_plan(const iqhip_engine *e) {
    return !e->mfma || (e->mfma_pipelined && e->n == 20 && !e->leaf_tables && e->plan.nleaf_tabs == 0);
}

// comm.hip -- RCCL, loaded lazily.  comm_allreduce: in-place SUM/f64 all-reduce of the first n doubles of the
// engine's device result vector on its stream (no-op without a communicator).  comm_group_allreduce: the same for
// the shards of a single-process sharded engine, inside one ncclGroupStart/End.  comm_init_all: ncclCommInitAll
// over the shards' devices.  All return an IQHIP status.
int comm_allreduce(iqhip_engine *e, int n);
int comm_group_allreduce(const std::vector<iqhip_engine *> &shards, int n);
int comm_init_all(const std::vector<iqhip_engine *> &shards);
void comm_destroy(iqhip_engine *e);
int comm_use_device_result(iqhip_engine *e);  // switch the engine to a device-memory result vector

// engine.hip internals the solvers (solve.hip), the feature drivers (ptnlh.hip, classlh.hip, pairdist.hip, ...) and the
// sharded front drive an engine with
// a planning-only engine has no device: every entry point that would touch one fails here ("invalid device ordinal")
hipError_t use_device(const iqhip_engine *e);
// May this engine run the feature `what` (an entry point's name)?  A null engine and a planning-only engine are always
// refused (IQHIP_ERR_INVALID); then, as far as `needs` asks: a sharded engine or communicator rank, the shape refusals in
// the order of the bits below (IQHIP_ERR_UNSUPPORTED), the state preconditions (IQHIP_ERR_INVALID).  Every text starts
// with "<what>: ".  What only one feature knows of (an E-step that must have run, iqhip_pars_init, ...) stays with it.
enum : unsigned {
    REQ_SINGLE_DEVICE = 1u << 0,    // no shards, no communicator
    REQ_NO_ASC = 1u << 1,
    REQ_PLAIN_STATES = 1u << 2,     // the caller's state count is the kernels' (no embedded state counts)
    REQ_STATES_4_20_64 = 1u << 3,
    REQ_STATES_4 = 1u << 4,
    REQ_NO_MIXTURE = 1u << 5,
    REQ_MIXTURE = 1u << 6,          // at least two classes
    REQ_MODEL_ALN = 1u << 7,        // model and alignment set
    REQ_THETA = 1u << 8,            // theta valid
};
int require(iqhip_engine *e, const char *what, unsigned needs);
int check_ready(iqhip_engine *e);                     // model and alignment set, device selected
// the scale counters of a branch's two ends; a leaf carries no scaling events: nullptr
int branch_scale_counters(iqhip_engine *e, iqhip_branch_end a, iqhip_branch_end b, const int16_t *sc[2]);
int ensure_slab_rows(iqhip_engine *e, int nrows);     // the wave-partial slab holds nrows rows
// enqueue: plan upload, K1, fused traversal (+ optional root lnL), fixed-order reduction (skip_reduce: the caller's next
// kernel sums the slab); explicit_segs, len_ptrs: see build_plan
int submit_traverse(iqhip_engine *e, const iqhip_node_op *ops, int nops, bool has_root, iqhip_branch_end a,
                    iqhip_branch_end b, double len, bool skip_reduce = false, const std::vector<int> *explicit_segs = nullptr,
                    const double *const *len_ptrs = nullptr);
int read_result(iqhip_engine *e, int ndoubles);       // D2H of the result vector (if it is device memory) + stream sync
// theta is (being) built from this branch's two ends, which the caller named a and b
void set_theta_branch(iqhip_engine *e, const DevBranch &br, iqhip_branch_end a, iqhip_branch_end b);
// read_result's bookkeeping for a caller that has waited for the engine's stream itself (partition.hip: one wait for
// all members); a caller-bound device result vector must have been copied to h_result on that stream before
void result_arrived(iqhip_engine *e);
int eng_repair_lnl(iqhip_engine *e, double *lnl);     // phylokernel.h:848-866 on this engine's _pattern_lh -> its own sum
extern double debug_build_us;                         // IQHIP_DEBUG_SWEEP: host time in build_plan since the last sweep report

// IQHIP_DEBUG_SWEEP: host time in microseconds
struct Stopwatch {
    timespec t0;
    void start() { clock_gettime(CLOCK_MONOTONIC, &t0); }
    double us() const {
        timespec t1;
        clock_gettime(CLOCK_MONOTONIC, &t1);
        return (t1.tv_sec - t0.tv_sec) * 1e6 + (t1.tv_nsec - t0.tv_nsec) * 1e-3;
    }
};

// solve.hip -- the branch-length solvers: Newton on one branch, a whole sweep, the batched NNI evaluator
// the pieces every form shares ...
int newton_check_bounds(const char *entry, double xguess, double x1, double x2, double xacc, int max_steps);
// the solver status every form reports: IQHIP_OK for 0, the reference's two failures for 2 (non-finite derivative) and
// 3 (step limit); 4 (the kernel's exchange between workgroups gave up) is no error: *gave_up tells the caller, who runs
// the fallback of its own form
int newton_status(int status, bool *gave_up = nullptr);
// what a solve hands back, from a result row {optx, d2l, nsteps, status, ..} of the kernels or from a state machine
struct NewtonResult {
    double optx, d2l;
    int nsteps, status;
    explicit NewtonResult(const double *row) : optx(row[0]), d2l(row[1]), nsteps((int)row[2]), status((int)row[3]) {}
    explicit NewtonResult(const NewtonState &st) : optx(st.result), d2l(st.d2l), nsteps(st.neval), status(st.status) {}
    void store(double *x, double *d, int *n) const {
        if (x) *x = optx;
        if (d) *d = d2l;
        if (n) *n = nsteps;
    }
    void store(iqhip_branch_result &r) const { r.optx = optx; r.d2l = d2l; r.nsteps = nsteps; r.status = status; }
};
// The pacing of every enqueued Newton chain.  A typical solve converges in 3..5 evaluations, so that many steps are
// enqueued before the first look at the state machine(s), then two at a time; steps enqueued after convergence do nothing.
// step(): enqueue one evaluation + reduction + update; all_done(&done): read the state(s) back.  Both return a status.
template <typename Step, typename AllDone>
int drive_chain(int max_steps, Step &&step, AllDone &&all_done) {
    for (int enq = 0;;) {
        const int chunk = enq == 0 ? std::min(4, max_steps + 1) : 2;
        for (int k = 0; k < chunk; k++) {
            const int rc = step();
            if (rc) return rc;
        }
        enq += chunk;
        bool done = false;
        const int rc = all_done(&done);
        if (rc) return rc;
        if (done) return IQHIP_OK;
        if (enq > max_steps + 2) return fail(IQHIP_ERR_INVALID, "Newton chain did not terminate");
    }
}
// ... of the batch: every task checked, its ops appended to `all`, their count to `segs`
int batch_gather_ops(const iqhip_branch_task *tasks, int ntasks, std::vector<iqhip_node_op> &all, std::vector<int> &segs);
// tasks per chunk of the batched chain: the same on every rank (the ranks' collectives must pair up), so a fixed number
// and not what the free memory of a device suggests
constexpr int kBatchChainChunk = 64;
int batch_chunk(int chunk);   // ... clamped by IQHIP_BATCH_CHUNK (read per call)
int batch_task_results(const std::vector<NewtonState> &st, int m, iqhip_branch_result *results);
int batch_derv_rows(const iqhip_engine *e);   // result rows per task of a derivative pass: 2, +ASC 5
int batch_asc_lnl(const iqhip_engine *e, double prob_const, double *lnl);   // +ASC: lnl -= nsites * log(1 - prob_const)
int asc_log_term(double prob_const, double *lp);   // log(1 - prob_const) after the reference's range assertion (engine.hip)
// Newton as a chain of enqueued steps, one piece at a time
int newton_state_alloc(iqhip_engine *e);
int newton_state_read(iqhip_engine *e);               // -> e->h_nstate (syncs the stream)
int eng_newton_begin(iqhip_engine *e, double xguess, double x1, double x2, double xacc, int max_steps);
int eng_newton_eval_enqueue(iqhip_engine *e);         // derivative kernel at state->rts + k_reduce -> result[0..1]
int eng_newton_update_enqueue(iqhip_engine *e);       // state machine step from result[0..1]
// batched chain (iqhip_optimize_branch_batch on sharded engines): m tasks side by side, ONE reduction of 2m rows and
// hence one all-reduce of 2m doubles per Newton step.  prepare: theta of every task into its slot + the initial states
int eng_batch_prepare(iqhip_engine *e, const iqhip_branch_task *tasks, int m, const NewtonState *init);   // init == nullptr: the theta slots only
int eng_batch_eval_enqueue(iqhip_engine *e, int m);   // derivative kernels at states[t].rts + k_reduce -> result[0..2m)
int eng_batch_update_enqueue(iqhip_engine *e, int m); // state machines step from result[0..2m)
int eng_batch_lnl_enqueue(iqhip_engine *e, int m);    // lnL at states[t].result -> result[2t]
int eng_batch_states_read(iqhip_engine *e, int m, NewtonState *out);        // (syncs the stream)
int eng_batch_states_write(iqhip_engine *e, int m, const NewtonState *in);

// sharded.hip -- the single-process multi-device front (iqhip_create_sharded); every public entry point of
// engine.hip, solve.hip and ptnlh.hip forwards here when e->shards is non-empty
namespace sharded {
void destroy(iqhip_engine *p);
int reserve(iqhip_engine *p, int nvectors);
int release(iqhip_engine *p, uint64_t key);
int rekey(iqhip_engine *p, uint64_t old_key, uint64_t new_key);
int set_alignment(iqhip_engine *p, const uint8_t *states, const double *ptn_freq, const double *ptn_invar);
int set_ascertainment(iqhip_engine *p, int64_t n_unobserved, double nsites);
int set_ptn_array(iqhip_engine *p, const double *v, bool invar);
int set_model(iqhip_engine *p, int nclass, const int32_t *cat_class, const double *eval, const double *evec,
              const double *inv_evec, const double *rates, const double *props, int state_unknown, const double *tip);
int traverse(iqhip_engine *p, const iqhip_node_op *ops, int nops, bool has_root, iqhip_branch_end a, iqhip_branch_end b,
             double len, double *sum_scale, double *lnl);
int compute_theta(iqhip_engine *p, iqhip_branch_end a, iqhip_branch_end b);
int derv(iqhip_engine *p, double len, double *df, double *ddf);
int lnl_from_theta(iqhip_engine *p, double len, double *lnl);
int optimize_branch(iqhip_engine *p, const iqhip_node_op *ops, int nops, bool build_theta, iqhip_branch_end a,
                    iqhip_branch_end b, double xguess, double x1, double x2, double xacc, int max_steps,
                    double *sum_scale, double *optx, double *d2l, int *nsteps);
int optimize_branch_batch(iqhip_engine *p, const iqhip_branch_task *tasks, int ntasks, double *sum_scale,
                          iqhip_branch_result *results);
int fetch_scale_num(iqhip_engine *p, uint64_t key, int16_t *out);
int fetch_pattern_lh(iqhip_engine *p, double *out, int kind, iqhip_branch_end a, iqhip_branch_end b);  // kind 0 plain, 1 scaled
int fetch_vec(iqhip_engine *p, uint64_t key, bool theta, double *out);
int pattern_lh_cat(iqhip_engine *p, double len, double *out);
int upload_partial(iqhip_engine *p, uint64_t key, const double *partial_lh, const int16_t *scale_num);
int set_boot_samples(iqhip_engine *p, const float *samples, int nsamples);
int rell(iqhip_engine *p, iqhip_branch_end a, iqhip_branch_end b, double *out);
int synchronize(iqhip_engine *p);
}  // namespace sharded

// kernels_valu4.hip
// seg_table: device ints {begin, nops} x nsegs; every segment runs on its own set of workgroups
// fold_rows >= 0: this is the submission's last launch and it sums the slab itself (rows 2 .. 2+fold_rows, plus 0/1
// with a root branch) instead of a k_reduce launch
hipError_t launch_traverse4(iqhip_engine *e, const int *seg_table, int nsegs, bool has_load, const DevBranch *root, int nwaves,
                            int fold_rows = -1);
// BatchChain: the batched form of the enqueued Newton chain (iqhip_optimize_branch_batch on sharded engines) -- task t
// (blockIdx.y) has theta at theta + t * theta_stride, its state machine at states[t] and slab rows 2t, 2t + 1
struct BatchChain {
    const double *theta;
    size_t theta_stride;
    const NewtonState *states;
    int ntasks;
    // slab rows per task of a derivative pass: 2 = {df, ddf}; 5 (+ASC) = {df, ddf, prob_const, df_const, ddf_const}, the last
    // three zero on an engine that holds none of the unobserved patterns.  The lnL pass has 2 = {lnl, prob_const} always.
    int derv_rows;
    const int16_t *const *sc;   // +ASC: [2 * ntasks] scale counters of the tasks' branch ends (the lnL pass's rescale rule)
};
hipError_t launch_theta4(iqhip_engine *e, const DevBranch &br, double *theta_out = nullptr);
hipError_t launch_derv4(iqhip_engine *e, double len, int nwaves, const NewtonState *st = nullptr, const BatchChain *bc = nullptr);
hipError_t launch_lnl_theta4(iqhip_engine *e, double len, int nwaves, const BatchChain *bc = nullptr);
hipError_t launch_reduce(iqhip_engine *e, int first_row, int nrows, int nwaves);

// kernels_newton.hip
// build_from != nullptr: the first evaluation also builds theta from that branch; reduce_rows > 0: the
// sum_scale rows [2, 2 + reduce_rows) of the slab are summed into the result vector first
// sweep != nullptr (one step of iqhip_optimize_sweep): the accepted length also goes to *len_out (device memory read by
// later steps), the sum_scale rows go to rows_base[0 .. reduce_rows) instead of result[2 ..], the diverged-solve rule is
// applied on the device above diverge_x, and only the step with `publish` signals the polling host
struct NewtonSweepStep {
    double *len_out;
    double *rows_base;
    double diverge_x;
    bool publish;
};
hipError_t launch_newton(iqhip_engine *e, double xguess, double x1, double x2, double xacc, int max_steps,
                         double *out, const DevBranch *build_from = nullptr, int reduce_rows = 0,
                         int reduce_nwaves = 0, const NewtonSweepStep *sweep = nullptr);

// Newton as a chain of enqueued steps (kernels_newton.hip): state init, derivative evaluation at state->rts
// (skipped once state->done), state update from result[0..1]
hipError_t launch_newton_state_init(iqhip_engine *e, double xguess, double x1, double x2, double xacc, int max_steps);
// ... of a state machine that belongs to no engine (partition.hip)
hipError_t launch_newton_state_init_on(hipStream_t s, NewtonState *st, double xguess, double x1, double x2, double xacc,
                                       int max_steps);
hipError_t launch_derv_at_state(iqhip_engine *e, int nwaves);
hipError_t launch_newton_state_update(iqhip_engine *e);   // (+ASC: result[2..4] and asc_nsites enter the update)
// from result[2t], result[2t+1]; +ASC: from result[5t .. 5t+4], corrected like launch_newton_state_update
hipError_t launch_newton_state_update_batch(iqhip_engine *e, NewtonState *states, int ntasks);

// kernels_sweep.hip: a whole sweep of a 4-state engine in one launch; posts: [2][kNewtonPostEpochs][grid][2] all-ones
int sweep4_grid(const iqhip_engine *e);
int sweep4_waves(const iqhip_engine *e);   // waves per workgroup (8: one 512-thread workgroup for <= 8 tiles)
hipError_t launch_sweep4(iqhip_engine *e, const SweepOp *d_ops, const SweepStep *d_steps, int nsteps, double x1, double x2,
                         double xacc, int max_steps, double diverge_x, double *posts, double *out);

// kernels_rell.hip
hipError_t launch_pattern_lh_scaled(iqhip_engine *e, const int16_t *sc_a, const int16_t *sc_b, double *out);
hipError_t launch_rell(iqhip_engine *e, double *out);
hipError_t launch_pattern_lh_cat(iqhip_engine *e, double len, double *out);
// kernels_em.hip: part holds one row of ncat (E-step) or 2 ncat (objective) doubles per 256 patterns of nptn_pad
hipError_t launch_em_posteriors(iqhip_engine *e, double len, double *W, double *ptn_rate, int32_t *ptn_cat, double *part,
                                double *out);
hipError_t launch_em_objective(iqhip_engine *e, const int16_t *sc_a, const int16_t *sc_b, double len, const double *W,
                               double *part, double *out);
// kernels_mixem.hip: d_cls_list = first [nclass + 1] ++ the components of every class; one EM step = the E-step kernel over
// Lc plus the one-workgroup update of the state (two launches); part holds mixem_part_rows rows of nclass doubles
hipError_t launch_mix_class_lh(iqhip_engine *e, double len, const int32_t *d_cls_list, double *Lc);
int64_t mixem_part_rows(const iqhip_engine *e);
// kernels_classlnl.hip: part holds class_lnl_part_rows rows of 2 nclass doubles; out = lnl [nclass] ++ floored [nclass]
int64_t class_lnl_part_rows(const iqhip_engine *e);
hipError_t launch_class_lnl(iqhip_engine *e, const int16_t *sc_a, const int16_t *sc_b, double len, const int32_t *d_cls_list,
                            int max_comp, const double *d_cw, const double *d_class_invar, double *part, double *out);
// the device-resident state of one EM run, all doubles: these scalars, then g [nclass], w [nclass], the log [max_steps][nclass + 1]
enum { MIXEM_DONE = 0, MIXEM_STEPS, MIXEM_PINV, MIXEM_V, MIXEM_PINV_IN, MIXEM_USE_INV, MIXEM_NSITES, MIXEM_HDR = 8 };
hipError_t launch_mixem_step(iqhip_engine *e, const double *Lc, double *state, int max_steps, double *part);
hipError_t launch_mix_posteriors(iqhip_engine *e, const double *Lc, const double *d_class_freq, double *post, double *sfreq);
// rows of the per-pattern store from a chunk of k_newton_batch: task t of the m tasks -> store row d_rows[t] (< 0: none)
hipError_t launch_ptnlh_rows(iqhip_engine *e, const void *d_tasks, int m, const double *theta_base, size_t theta_stride,
                             const double *batch_out, const int32_t *d_rows);

// kernels_alrt.hip: R = L W^T on the fp64 matrix cores (K-split partial products, then a fixed-order combine) and the
// SH-aLRT / local-bootstrap counts
int alrt_ksplit(const iqhip_engine *e, int nrows, int nsamples);
// ptnlh.hip: the distinct rows of a row list in first-appearance order (list[0, M)) and, behind them, every entry's index
// into them; bt_stage: the list into e->bt.rows, e->bt.part and e->bt.sums sized for products of its distinct rows with
// nsamples replicates (the engine's stream drains); row_list_scatter: the sums [M][nsamples] of the distinct rows back to
// the order of the list the RowList was made from, out [nrows][nsamples]
struct RowList {
    std::vector<int32_t> list;
    int M;
};
RowList row_list(const int32_t *rows, int nrows);
int bt_stage(iqhip_engine *e, const RowList &rl, int ksplit, size_t nsamples);
void row_list_scatter(const RowList &rl, const double *sums, int nsamples, double *out);
hipError_t launch_alrt_product(iqhip_engine *e, const int32_t *d_rows, int nrows, int nsamples, int ksplit, double *part,
                               double *sums);
hipError_t launch_alrt_stats(iqhip_engine *e, const int32_t *d_idx3, const double *d_lh3, int nbranch, int nsamples,
                             const double *sums, double *out /* 4 per branch */);

// kernels_topo.hip: tree topology tests on the sums of launch_alrt_product.  launch_topo_gen fills rows [0, nsamples) of
// e->d_boot from e->d_freq_prefix; launch_topo_tests enqueues avg_lh and the per-replicate pass, launch_topo_tree the counts
struct TopoTestArgs {
    const double *sums;       // [M][S]
    const int32_t *idx;       // [T] tree -> row of sums
    int T, S;
    double epsilon;
    uint64_t tie_key;         // topo_stream_key(tie_seed, 0xB9)
    const double *lh;         // [T]
    double *avg;              // [T]
    double *max_sh, *max_elw, *sum_l;   // [S]
    int32_t *winner;          // [S]
    const int32_t *kh_id;     // [T]
    const double *weights;    // [T][T] or nullptr (unweighted)
    const int32_t *w_id;      // [T]
    const double *w_orig;     // [T]
    double *out;              // [T][6] = bp, kh, sh, wkh, wsh, elw
};
uint64_t topo_stream_key(uint64_t seed, uint32_t stream);
hipError_t launch_topo_gen(iqhip_engine *e, int nsamples, int64_t first_replicate, int64_t ndraws, uint64_t stream_key);
hipError_t launch_topo_diff_variance(iqhip_engine *e, const int32_t *d_rows, int n, double *d_var);
hipError_t launch_topo_tests(iqhip_engine *e, const TopoTestArgs &a);
hipError_t launch_topo_tree(iqhip_engine *e, const TopoTestArgs &a);
hipError_t launch_topo_argmax(iqhip_engine *e, const double *sums, const int32_t *d_idx, int T, int S, uint32_t *counts);

// kernels_ufboot.hip: saveCurrentTree's per-replicate rule on the sums of launch_alrt_product [M][nsamples].  d_entries: n
// entries in list order whose `row` is the row of `sums`; *replaced += the slots replaced (one integer atomic per
// workgroup), wgmin[ufboot_workgroups(nsamples)] = per workgroup the minimum of boot_orig_logl over the slots holding a tree
int ufboot_workgroups(int nsamples);
hipError_t launch_ufboot_update(iqhip_engine *e, const double *sums, int nsamples, const iqhip_ufboot_tree *d_entries, int n,
                                double epsilon, double *boot_logl, double *boot_orig_logl, int32_t *boot_counts,
                                int64_t *boot_tree, unsigned long long *replaced, double *wgmin);

// kernels_dist.hip: pairwise ML distances.  launch_pair_counts: the tiles' pairs -> d_counts[slot][n * n]; launch_pair_solve:
// slot s of the chunk is pair first_pair + s of the call: start init[pair] (0 or no array: the pair's JC distance), result
// out[4 pair .. 4 pair + 3] = {optx, d2l, derivative evaluations, status of NewtonState}
struct PairSolveArgs {
    const double *counts;   // [chunk][n * n]
    const double *coef;     // [n][n][n] = evec[i][k] * inv_evec[k][j]
    const double *eval, *rates, *props;
    const double *init;     // [npairs] or nullptr
    double *out;            // [npairs][4]
    int64_t first_pair;
    int n, ncat, max_steps;
    double x1, x2, xacc;
};
hipError_t launch_pair_counts(iqhip_engine *e, const PairTile *d_tiles, int ntiles, double *d_counts);
hipError_t launch_pair_coef(iqhip_engine *e, double *d_coef);
hipError_t launch_pair_solve(iqhip_engine *e, const PairSolveArgs &a, int npairs);

// kernels_partdist.hip: the joint pairwise distances of a partition group (SuperAlignmentPairwisePlen).  One descriptor per
// member; slot s of a chunk is pair first_pair + s of the call.  The kernel compacts the non-zero cells of every member's
// counts of the slot into `cells` (nnz[slot][member] of them) once per pair and evaluates them per Newton step
struct __attribute__((aligned(16))) PartPairDesc {
    const double *counts;   // [chunk][n * n], what launch_pair_counts wrote for the member
    const double *coef;     // [n][n][n] (launch_pair_coef)
    const double *eval, *rates, *props;
    uint16_t *cells;        // [chunk][n * n]
    int32_t n, ncat;
    double rate;
};
struct PartPairArgs {
    const PartPairDesc *desc;   // [nparts]
    int32_t *nnz;               // [chunk][nparts]
    const double *init;         // [npairs] or nullptr
    double *out;                // [npairs][4] = {optx, d2l, derivative evaluations, status of NewtonState}
    int64_t first_pair;
    int32_t nparts, max_steps;
    int32_t e_doubles, max_n;   // LDS: e[e_doubles] ++ lam[max_n] ++ lam2[max_n]; the largest ncat * n and n of the members
    double x1, x2, xacc;
};
size_t partpair_solve_lds_bytes(int e_doubles, int max_n);
hipError_t launch_partpair_solve(hipStream_t s, const PartPairArgs &a, int npairs);

// kernels_quartet.hip: likelihood mapping.  launch_quartet_cells: quartet s of the chunk (taxa d_quartets[4 s ..]) ->
// d_cells[s][256], d_nother[s], d_other[s * nptn ..].  launch_quartet_solve: one workgroup per (slot, topology); slot s is
// quartet `first + s` of the call and writes out[first + s]
struct QuartetSolveArgs {
    const double *cells;        // [chunk][256]
    const int32_t *nother;      // [chunk]
    const int32_t *other;       // [chunk][nptn]
    const int32_t *quartets;    // [chunk][4]
    const uint8_t *states;      // [ntaxa][nptn_pad]
    const double *freq;
    const double *evec, *inv_evec, *eval, *rates, *props, *tip;
    iqhip_quartet_result *out;  // [nq]
    int64_t nptn_pad, nptn, first;
    double const_invar[5];      // all 0 without +I
    double nsite, x1, x2, xacc, diverge_frac, tolerance;
    int32_t ncat, state_unknown, max_steps, iterations;
    uint8_t mask[32];           // the states every state code allows (bit j: state j)
};
size_t quartet_solve_lds_bytes(int ncat, int state_unknown);
hipError_t launch_quartet_cells(iqhip_engine *e, const int32_t *d_quartets, int m, double *d_cells, int32_t *d_nother,
                                int32_t *d_other);
hipError_t launch_quartet_solve(iqhip_engine *e, const QuartetSolveArgs &a, int m);

// Fitch parsimony (kernels_pars.hip); all on e->stream, shapes from e->pars_nwords / e->n
constexpr int kParsWordsPerWg = 16;   // word columns a workgroup of k_pars_update owns ...
constexpr int kParsThreads = 1024;    // ... and its threads: 64 ops of a level side by side (measured: DESIGN.md 3.8)
hipError_t launch_pars_tips(iqhip_engine *e, const int32_t *d_site_ptn);
// d_ops: nops ops sorted by level; d_lev_start: nlev + 1 offsets into them
hipError_t launch_pars_update(iqhip_engine *e, const iqhip_pars_op *d_ops, const int32_t *d_lev_start, int nlev);
// d_out: score [nbranch] ++ subst [nbranch]; taxon >= 0: the insertion scan, which also writes {best, best_score} behind them
hipError_t launch_pars_branch(iqhip_engine *e, const int32_t *d_ends, int nbranch, int taxon, int32_t *d_out, int *nlaunches);
// the segmented insertion scan (iqhip_pars_insert_scores_batch): a wave per branch while nwords <= kParsBatchWaveWords (a
// wave then makes at most 4 passes over its 64 columns), a workgroup per branch above.  NOT MEASURED: the threshold is a
// guess from the shapes; tools/bench_pars_forest.py reports both routes (IQHIP_PARS_BATCH_ROUTE forces one) so that a
// later change can move it.
constexpr int64_t kParsBatchWaveWords = 256;
enum ParsBatchRoute { PARS_BATCH_AUTO = 0, PARS_BATCH_WAVE = 1, PARS_BATCH_WG = 2 };
// d_ends: 2 * nbranch slots; d_taxon: the tip slot of every branch; d_seg_start: nseg + 1 offsets into the branches;
// d_out = score [nbranch] ++ best [nseg] (index within the segment) ++ best_score [nseg]
hipError_t launch_pars_insert_batch(iqhip_engine *e, const int32_t *d_ends, const int32_t *d_taxon, int nbranch,
                                    const int32_t *d_seg_start, int nseg, ParsBatchRoute route, int32_t *d_out, int *nlaunches);
// the SPR scan (kernels_spr.hip): d_steps carry the depth in `parent`; d_out = score [nsteps] ++ best_step [njobs] ++
// best_score [njobs] ++ best_job; max_depth = the deepest step of the launch (sizes the LDS stack)
hipError_t launch_pars_spr(iqhip_engine *e, const iqhip_pars_spr_job *d_jobs, int njobs, const iqhip_pars_spr_step *d_steps,
                           int nsteps, int max_depth, int32_t *d_out, int *nlaunches);

// batched branch optimisation (k_newton_batch); d_tasks: device array of NewtonTask (kernels_newton.hip)
hipError_t launch_newton_batch(iqhip_engine *e, const void *d_tasks, int ntasks, int G, double *theta_base,
                               size_t theta_stride, double *partials, unsigned int *barriers, unsigned int *barriers_next,
                               double *out,
                               double *posts = nullptr, double *posts_other = nullptr, size_t posts_other_used = 0,
                               int post_epochs = 0);
size_t newton_task_bytes();
size_t newton_task_branch_offset();   // of the DevBranch inside a NewtonTask
void newton_task_fill(void *dst, const DevBranch &br, double xguess, double x1, double x2, double xacc, int max_steps);

// kernels_valu4w.hip (4 states, 9 .. 32 categories): the launch choose_traverse_mfma described as TRAV_WIDE4
hipError_t launch_traverse4w(iqhip_engine *e, const TravLaunch &L, const int *seg_table, int nwaves);

// kernels_mfma.hip (nstates 20 / 64)
hipError_t launch_traverse_mfma(iqhip_engine *e, const int *seg_table, int nsegs, int nwaves, bool top_stage = false);
hipError_t launch_leaf_tables(iqhip_engine *e, const TabJob *d_jobs, int njobs);
// cherry tables: src[i] (tile layout, npairs patterns) -> dst[i] (register order of the traversal kernel), host pointer arrays
hipError_t launch_cherry_transpose(iqhip_engine *e, const double *const *src, double *const *dst, int n, int npairs);
size_t leaf_table_doubles(const iqhip_engine *e);          // doubles per (leaf child) table: ncat * state_unknown * n
// mode 0: branch lnL, 1: theta, 2: df/ddf from theta, 3: lnL from theta
// theta_out (mode 1): write theta there instead of the engine's buffer; bc (modes 2, 3): batched chain, see BatchChain
hipError_t launch_stream_mfma(iqhip_engine *e, int mode, const DevBranch *br, double len, int nwaves,
                              const NewtonState *st = nullptr, int fold_rows = -1, double *theta_out = nullptr,
                              const BatchChain *bc = nullptr);

// kernels_partnewton.hip: the joint branch solve of a partition group (partition.hip).  One descriptor per member, filled
// from the engine fields that fill NewtonArgs; a work item is a contiguous run of tiles of ONE member, one workgroup each
struct __attribute__((aligned(16))) PartDesc {
    const double *theta, *evalc, *rates, *props, *freq, *invar;
    const int16_t *a_sc, *b_sc;   // scale counters of the ends theta was built from (nullptr: a leaf end)
    int64_t nptn, ntiles;
    int32_t n, ncat, mfma;
    int32_t item_first, nitems;   // the member's work items, in tile order
    int32_t _pad;
    double rate;
};
struct __attribute__((aligned(16))) PartItem {
    int64_t first_tile;
    int32_t member, ntiles;
};
// the root branch of one member for the scale-factor term of a traversal's lnL
struct __attribute__((aligned(16))) PartScale {
    const int16_t *a_sc, *b_sc;
    const double *freq;
    int64_t nptn;
};
// a member's theta slots of a batch of joint solves: slot t at theta + t * stride (the engine's d_theta_batch)
struct __attribute__((aligned(16))) PartSlots {
    const double *theta;
    size_t stride;
};
constexpr int kPartUpdateThreads = 64;   // k_part_newton_update: thread t owns members t, t + 64, ..
// mode 0: {df, ddf} of every item at rate * st->rts (nothing once st->done); mode 1: f * log|lh| sums (scale-factor term
// included) at rate * (st ? st->result : x) -> partials[2 item], [2 item + 1]; lds_doubles = 3 * the largest block
hipError_t launch_part_derv(hipStream_t s, int mode, const PartDesc *d_desc, const PartItem *d_items, int nitems,
                            int lds_doubles, const NewtonState *st, double x, double *partials);
// per member: its items summed in item order, the NaN rule; then r df, r^2 ddf summed in member order -> newton_update
hipError_t launch_part_newton_update(hipStream_t s, const PartDesc *d_desc, int nparts, const double *partials,
                                     NewtonState *st);
hipError_t launch_part_lnl_finish(hipStream_t s, const PartDesc *d_desc, int nparts, const double *partials, double *out);
// the batch of joint solves: task t (grid.y) on slot t of every member at the length in states[t]; d_sc: [ntasks][nparts][2]
// scale counters of the tasks' branch ends; partials: [ntasks][nitems][2]; out: [ntasks][nparts]; lnl_written: [ntasks], zero
// when the chain starts -- the finish launch marks a task that is done, and later mode 1 launches leave it alone.  d_rowp
// (mode 1; nullptr: none): [ntasks][nparts] rows of the members' per-pattern stores (nullptr: the task keeps no row), written
// in the one mode 1 pass that gets past the lnl_written guard
hipError_t launch_part_derv_batch(hipStream_t s, int mode, const PartDesc *d_desc, const PartItem *d_items, int nitems,
                                  int lds_doubles, const PartSlots *d_slots, const int16_t *const *d_sc, int nparts,
                                  const NewtonState *states, const int32_t *lnl_written, int ntasks, double *partials,
                                  double *const *d_rowp = nullptr);
hipError_t launch_part_newton_update_batch(hipStream_t s, const PartDesc *d_desc, int nparts, int nitems,
                                           const double *partials, NewtonState *states, int ntasks);
hipError_t launch_part_lnl_finish_batch(hipStream_t s, const PartDesc *d_desc, int nparts, int nitems, const double *partials,
                                        const NewtonState *states, int32_t *lnl_written, double *out, int ntasks);
// out[p] = kLogScalingThreshold * sum over patterns of freq * (a_sc + b_sc), fixed order
hipError_t launch_part_scale_terms(hipStream_t s, const PartScale *d_sc, int nparts, double *out);

// kernels_partboot.hip: the members' RELL sums [M][nsamples] added in member order, ((R_0 + R_1) + R_2) + ..; d_sums: a device
// table of nparts pointers.  launch_part_rell_sum: the summed matrix (count = M * nsamples elements);
// launch_part_ufboot_update: launch_ufboot_update with rell formed as that sum inside the kernel
hipError_t launch_part_rell_sum(hipStream_t s, const double *const *d_sums, int nparts, size_t count, double *out);
hipError_t launch_part_ufboot_update(hipStream_t s, const double *const *d_sums, int nparts, int nsamples,
                                     const iqhip_ufboot_tree *d_entries, int n, double epsilon, double *boot_logl,
                                     double *boot_orig_logl, int32_t *boot_counts, int64_t *boot_tree,
                                     unsigned long long *replaced, double *wgmin);

}  // namespace iqhip
