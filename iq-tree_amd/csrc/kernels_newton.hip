// kernels_newton.hip -- SURVEY.md 8(f)-1: a whole Newton-Raphson branch-length solve in ONE launch.
//
// The reference optimises a branch with Optimization::minimizeNewton (optimization.cpp:388-465)
// calling PhyloTree::computeFuncDerv -> computeLikelihoodDerv (phylotree.cpp:2135-2146,
// phylokernel.h:583-651) once per step: on a GPU that is one launch + one host round trip per
// step (hot loop 2, latency-bound).  Here the loop itself runs on the device: every step evaluates
// df/ddf from the resident theta_all (L2-resident after the first step), reduces them across the
// grid in a fixed order, and every workgroup applies the reference's update rule redundantly.
// A single workgroup needs no grid barrier at all (the common case: real alignments have a few
// thousand patterns); larger grids use a monotonic-counter barrier (agent-scope release/acquire,
// bounded spin) with one workgroup per CU.
#include <string.h>

#include <mutex>

#include "iqhip_internal.h"
#include "wg_exchange.h"

namespace iqhip {

// Kernels with a hand-rolled grid barrier (k_newton, k_newton_batch) need all their workgroups resident at once.
// Their grids are sized for that on an otherwise free chip, and ordinary kernels of other engines only delay them
// (those finish without waiting for anybody).  What must never happen is TWO barrier kernels of different engines
// (partition analyses drive one engine per host thread, phylosupertree.cpp:970) each holding part of the CUs while
// waiting for workgroups that cannot be scheduled.  So barrier kernels of one device are chained: each launch waits
// (hipStreamWaitEvent, device side, no host stall) for the previous barrier kernel of ANY engine on that device.
// The barriers use relaxed agent-scope atomics + s_waitcnt vmcnt(0) for the hand-off of the partial sums, which is
// outside the HIP memory model proper; it is the R2 "sc1 loads and stores both sides" form measured for gfx950 in
// MI355X_MICROARCH.md (Workgroup dispatch, valid forms).  A barrier that still times out reports status 4 and the
// engine finishes the solve with the barrier-free chain form.
namespace {
struct BarrierChain {
    std::mutex mu;
    hipEvent_t ev[64] = {};
    bool valid[64] = {};
};
BarrierChain &barrier_chain() {
    static BarrierChain c;
    return c;
}
struct BarrierLaunchGuard {
    int dev;
    hipStream_t stream;
    bool active;
    BarrierLaunchGuard(iqhip_engine *e, bool multi_wg) : dev(e->device), stream(e->stream), active(multi_wg && e->device < 64) {
        if (!active) return;
        BarrierChain &c = barrier_chain();
        c.mu.lock();
        if (c.valid[dev]) (void)hipStreamWaitEvent(stream, c.ev[dev], 0);
    }
    ~BarrierLaunchGuard() {
        if (!active) return;
        BarrierChain &c = barrier_chain();
        if (!c.ev[dev] && hipEventCreateWithFlags(&c.ev[dev], hipEventDisableTiming) != hipSuccess) c.ev[dev] = nullptr;
        if (c.ev[dev]) c.valid[dev] = hipEventRecord(c.ev[dev], stream) == hipSuccess;
        c.mu.unlock();
    }
};
}  // namespace

struct NewtonArgs {
    const double *theta;
    const double *eval;
    const double *rates;
    const double *props;
    const double *freq;
    const double *invar;
    double *partials;        // [2 parities][grid][2]
    double *posts;           // non-NULL: posted exchange, this launch's slots [kNewtonPostEpochs][grid][2] (sentinel = not yet)
    double *posts_other;     // the other launch parity's slots: reset here for the launch after this one
    // non-NULL: the result vector is mapped host memory; workgroup 0 publishes this sequence number when everything the
    // host will read has been written, and the host polls it instead of paying a stream synchronisation (read_result)
    volatile unsigned long long *done;
    unsigned long long seq;
    unsigned int *barrier;   // arrival counter of this launch (zero at its start), counts up over the epochs
    unsigned int *barrier_next;  // the next launch's counter
    double *out;             // {optx, d2l, evaluations, status}
    // fused front end (iqhip_optimize_branch): the first evaluation builds theta = a .* b (phylokernel.h:535-573)
    // while it accumulates, and the sum_scale rows of the preceding node updates are reduced here
    int build;               // 1: theta is written by the first evaluation from `br`
    DevBranch br;
    const double *tipc;      // [state][ncat][n]
    const double *slab;      // wave partials of the node updates
    double *result;          // result vector (rows 2.. receive the sums)
    int nrows, nwaves;
    int64_t ntiles;          // tiles of `tile` patterns
    int64_t nptn;
    int n, ncat, mfma;
    double xguess, x1, x2, xacc;
    int max_steps;
    // branch-length sweeps (iqhip_optimize_sweep): the accepted length also goes to device memory, where the node
    // updates of the later steps of the same submission read it (DevOp::left_len_p / right_len_p)
    double *len_out;
    // +ASC (phylokernel.h:655-725): patterns [nobs, nptn) are the unobserved constant patterns (nobs == nptn: no correction)
    int64_t nobs;
    double asc_nsites;
    // > 0: PhyloTree::optimizeOneBranch's "newton raphson diverged, reset" rule (phylotree.cpp:2167-2176) applied here:
    // a result above this length is kept only if the branch lnL there is not below the lnL at the starting length
    double diverge_x;
};

// sum over this workgroup's patterns of f*df_ptn and f*ddf_ptn at the val arrays in LDS
// MODE 0: derivative sums (f*df_ptn, f*ddf_ptn); MODE 1: lnL sum (f*log|lh_ptn|) in odf.  The workgroup is
// number `wg` of `nwg` that share the patterns of one branch (the whole grid for k_newton).
// Register-resident theta (ThetaRegs): when every wave of the solve owns at most ONE tile and a lane's share of it is at
// most 20 doubles (4 states: block <= 20; 16-pattern tiles: block <= 80), the values the first evaluation loads (or
// builds) stay in registers and the later evaluations of the solve touch no memory at all: a derivative pass then
// costs its arithmetic plus the exchange between the workgroups instead of an L2 round trip on top (protein 50 x 20k:
// 10 -> 5.5 us per evaluation).  Same values, same order of operations: same bits.
struct ThetaRegs {
    double v[20];
    bool use;    // launch-constant, wave-uniform
    bool have;   // v holds this wave's tile
};

template <bool BUILD, int MODE = 0>
__device__ __forceinline__ void wg_partial(const NewtonArgs &A, const double *theta_c, const DevBranch &br, int wg, int nwg,
                                           const double *s_v0, const double *s_v1,
                                           const double *s_v2, double *s_red, double &odf, double &oddf, ThetaRegs *R = nullptr) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int B = A.n * A.ncat;
    double adf = 0.0, addf = 0.0;
    for (int64_t tile = (int64_t)wg * 4 + wave; tile < A.ntiles; tile += (int64_t)nwg * 4) {
        double lh = 0.0, d1 = 0.0, d2 = 0.0;
        int64_t ptn;
        bool mine;
        if (R && R->use && !A.mfma) {
            // (at most one tile per wave: this loop body runs once)
            ptn = tile * 64 + lane;
            mine = ptn < A.nobs;
            const double2 *p = reinterpret_cast<const double2 *>(theta_c + tile * (64 * B)) + lane;
            if (!R->have) {
                const double2 *pb = nullptr, *pa = nullptr;
                const double *tp = nullptr;
                if (BUILD) {
                    pb = reinterpret_cast<const double2 *>(br.b + tile * (64 * B)) + lane;
                    if (br.a_kind == CHILD_LEAF) tp = A.tipc + (size_t)br.a_states[ptn] * B;
                    else pa = reinterpret_cast<const double2 *>(br.a + tile * (64 * B)) + lane;
                }
#pragma unroll
                for (int j = 0; j < 10; j++) {
                    double2 t = make_double2(0.0, 0.0);
                    if (2 * j < B) {
                        if (BUILD) {
                            const double2 bv = pb[j * 64];
                            const double2 av = tp ? make_double2(tp[2 * j], tp[2 * j + 1]) : pa[j * 64];
                            t = make_double2(av.x * bv.x, av.y * bv.y);
                            const_cast<double2 *>(p)[j * 64] = t;
                        } else {
                            t = p[j * 64];
                        }
                    }
                    R->v[2 * j] = t.x;
                    R->v[2 * j + 1] = t.y;
                }
                R->have = true;
            }
#pragma unroll
            for (int j = 0; j < 10; j++)
                if (2 * j < B) {
                    lh = fma(s_v0[2 * j], R->v[2 * j], lh); lh = fma(s_v0[2 * j + 1], R->v[2 * j + 1], lh);
                    d1 = fma(s_v1[2 * j], R->v[2 * j], d1); d1 = fma(s_v1[2 * j + 1], R->v[2 * j + 1], d1);
                    d2 = fma(s_v2[2 * j], R->v[2 * j], d2); d2 = fma(s_v2[2 * j + 1], R->v[2 * j + 1], d2);
                }
        } else if (R && R->use) {
            const int p = lane & 15, g = lane >> 4;
            ptn = tile * 16 + p;
            mine = (g == 0) && ptn < A.nobs;
            if (!R->have) {
                const double *th = theta_c + (size_t)tile * 16 * B;
                const double *bv = nullptr, *av = nullptr, *tp = nullptr;
                if (BUILD) {
                    bv = br.b + (size_t)tile * 16 * B;
                    if (br.a_kind == CHILD_LEAF) tp = A.tipc + (size_t)br.a_states[ptn] * B;
                    else av = br.a + (size_t)tile * 16 * B;
                }
#pragma unroll
                for (int q = 0; q < 20; q++) {
                    const int e = g + 4 * q;
                    double t = 0.0;
                    if (e < B) {
                        if (BUILD) {
                            t = (tp ? tp[e] : av[(size_t)e * 16 + p]) * bv[(size_t)e * 16 + p];
                            const_cast<double *>(th)[(size_t)e * 16 + p] = t;
                        } else {
                            t = th[(size_t)e * 16 + p];
                        }
                    }
                    R->v[q] = t;
                }
                R->have = true;
            }
#pragma unroll
            for (int q = 0; q < 20; q++) {
                const int e = g + 4 * q;
                if (e < B) {
                    lh = fma(s_v0[e], R->v[q], lh);
                    d1 = fma(s_v1[e], R->v[q], d1);
                    d2 = fma(s_v2[e], R->v[q], d2);
                }
            }
            lh = group_sum(lh);
            d1 = group_sum(d1);
            d2 = group_sum(d2);
        } else if (!A.mfma) {
            ptn = tile * 64 + lane;
            mine = ptn < A.nobs;   // (the unobserved patterns of +ASC enter through asc_unobserved_sums only)
            const double2 *p = reinterpret_cast<const double2 *>(theta_c + tile * (64 * B)) + lane;
            const double2 *pb = nullptr, *pa = nullptr;
            const double *tp = nullptr;
            if (BUILD) {
                pb = reinterpret_cast<const double2 *>(br.b + tile * (64 * B)) + lane;
                if (br.a_kind == CHILD_LEAF) tp = A.tipc + (size_t)br.a_states[ptn] * B;
                else pa = reinterpret_cast<const double2 *>(br.a + tile * (64 * B)) + lane;
            }
            for (int j = 0; j < B / 2; j++) {
                double2 t;
                if (BUILD) {
                    const double2 bv = pb[j * 64];
                    const double2 av = tp ? make_double2(tp[2 * j], tp[2 * j + 1]) : pa[j * 64];
                    t = make_double2(av.x * bv.x, av.y * bv.y);
                    const_cast<double2 *>(p)[j * 64] = t;
                } else {
                    t = p[j * 64];
                }
                lh = fma(s_v0[2 * j], t.x, lh); lh = fma(s_v0[2 * j + 1], t.y, lh);
                d1 = fma(s_v1[2 * j], t.x, d1); d1 = fma(s_v1[2 * j + 1], t.y, d1);
                d2 = fma(s_v2[2 * j], t.x, d2); d2 = fma(s_v2[2 * j + 1], t.y, d2);
            }
        } else {
            const int p = lane & 15, g = lane >> 4;
            ptn = tile * 16 + p;
            mine = (g == 0) && ptn < A.nobs;
            const double *th = theta_c + (size_t)tile * 16 * B;
            const double *bv = nullptr, *av = nullptr, *tp = nullptr;
            if (BUILD) {
                bv = br.b + (size_t)tile * 16 * B;
                if (br.a_kind == CHILD_LEAF) tp = A.tipc + (size_t)br.a_states[ptn] * B;
                else av = br.a + (size_t)tile * 16 * B;
            }
            // (unrolled: the loads of several rows are in flight together; the accumulation order is unchanged)
            // a pattern's rows 20 at a time: all 20 loads of a lane are in flight together (one L2 round trip per
            // 80 block entries instead of one per unrolled handful); the accumulation order is unchanged
            for (int e0 = g; e0 < B; e0 += 80) {
                double tv[20];
#pragma unroll
                for (int q = 0; q < 20; q++) {
                    const int e = e0 + 4 * q;
                    if (e < B) {
                        if (BUILD) tv[q] = (tp ? tp[e] : av[(size_t)e * 16 + p]) * bv[(size_t)e * 16 + p];
                        else tv[q] = th[(size_t)e * 16 + p];
                    } else {
                        tv[q] = 0.0;
                    }
                }
#pragma unroll
                for (int q = 0; q < 20; q++) {
                    const int e = e0 + 4 * q;
                    if (e < B) {
                        if (BUILD) const_cast<double *>(th)[(size_t)e * 16 + p] = tv[q];
                        lh = fma(s_v0[e], tv[q], lh);
                        d1 = fma(s_v1[e], tv[q], d1);
                        d2 = fma(s_v2[e], tv[q], d2);
                    }
                }
            }
            lh = group_sum(lh);
            d1 = group_sum(d1);
            d2 = group_sum(d2);
        }
        if (mine) {
            lh += A.invar[ptn];
            const double f = A.freq[ptn];
            if (MODE == 1) {
                double l = log(fabs(lh));
                if (isnan(l) || isinf(l)) l = kLogScalingThreshold * 4;  // the reference's repair, phylokernel.h:1100-1122
                adf = fma(l, f, adf);
            } else {
                const double inv = 1.0 / fabs(lh);
                const double dfp = d1 * inv;
                const double ddfp = fma(-dfp, dfp, d2 * inv);
                adf = fma(dfp, f, adf);
                addf = fma(ddfp, f, addf);
            }
        }
    }
    adf = wave_sum64(adf);
    addf = wave_sum64(addf);
    if (lane == 0) { s_red[2 * wave] = adf; s_red[2 * wave + 1] = addf; }
    __syncthreads();
    odf = (s_red[0] + s_red[2]) + (s_red[4] + s_red[6]);
    oddf = (s_red[1] + s_red[3]) + (s_red[5] + s_red[7]);
    __syncthreads();
}

// +ASC, computeLikelihoodDervEigenSIMD's tail (phylokernel.h:655-725): sums over the unobserved constant patterns of
// {lh_ptn + ptn_invar, sum val1*theta, sum val2*theta} at the val arrays in LDS -- no rescaling, no weights.  There are
// nstates such patterns, in the last tile(s); wave 0 of EVERY workgroup computes them for itself (theta of those
// patterns from the resident theta_all, or on the fly from the branch ends while theta is being built by its owner), so
// the exchange between the workgroups stays two doubles and every workgroup applies the same correction.
// MODE 1: prob_const of computeLikelihoodFromBuffer (phylokernel.h:1138-1163) in s_asc[0]: a pattern whose two ends were
// rescaled at least once enters as lh * 2^-256 (the counters of the branch ends, DevBranch::a_sc / b_sc).
template <bool BUILD, int MODE = 0>
__device__ __forceinline__ void asc_unobserved_sums(const NewtonArgs &A, const double *theta_c, const DevBranch &br,
                                                    const double *s_v0, const double *s_v1, const double *s_v2, double *s_asc) {
    if (threadIdx.x < 64) {
        const int lane = threadIdx.x;
        const int B = A.n * A.ncat;
        double u0 = 0.0, u1 = 0.0, u2 = 0.0;
        const int T = A.mfma ? 16 : 64;
        for (int64_t tile = A.nobs / T; tile * T < A.nptn; tile++) {
            double lh = 0.0, d1 = 0.0, d2 = 0.0;
            int64_t ptn;
            bool mine;
            if (!A.mfma) {
                ptn = tile * 64 + lane;
                mine = true;
                const double2 *p = reinterpret_cast<const double2 *>(theta_c + tile * (64 * B)) + lane;
                const double2 *pb = reinterpret_cast<const double2 *>(br.b + tile * (64 * B)) + lane;
                const double2 *pa = nullptr;
                const double *tp = nullptr;
                if (BUILD) {
                    if (br.a_kind == CHILD_LEAF) tp = A.tipc + (size_t)br.a_states[ptn] * B;
                    else pa = reinterpret_cast<const double2 *>(br.a + tile * (64 * B)) + lane;
                }
                for (int j = 0; j < B / 2; j++) {
                    double2 t;
                    if (BUILD) {
                        const double2 bv = pb[j * 64];
                        const double2 av = tp ? make_double2(tp[2 * j], tp[2 * j + 1]) : pa[j * 64];
                        t = make_double2(av.x * bv.x, av.y * bv.y);
                    } else {
                        t = p[j * 64];
                    }
                    lh = fma(s_v0[2 * j], t.x, lh); lh = fma(s_v0[2 * j + 1], t.y, lh);
                    if (MODE == 0) {
                        d1 = fma(s_v1[2 * j], t.x, d1); d1 = fma(s_v1[2 * j + 1], t.y, d1);
                        d2 = fma(s_v2[2 * j], t.x, d2); d2 = fma(s_v2[2 * j + 1], t.y, d2);
                    }
                }
            } else {
                const int p = lane & 15, g = lane >> 4;
                ptn = tile * 16 + p;
                mine = g == 0;
                const double *th = theta_c + (size_t)tile * 16 * B;
                const double *bv = br.b + (size_t)tile * 16 * B, *av = nullptr, *tp = nullptr;
                if (BUILD) {
                    if (br.a_kind == CHILD_LEAF) tp = A.tipc + (size_t)br.a_states[ptn] * B;
                    else av = br.a + (size_t)tile * 16 * B;
                }
                for (int e = g; e < B; e += 4) {
                    const double t = BUILD ? (tp ? tp[e] : av[(size_t)e * 16 + p]) * bv[(size_t)e * 16 + p] : th[(size_t)e * 16 + p];
                    lh = fma(s_v0[e], t, lh);
                    if (MODE == 0) {
                        d1 = fma(s_v1[e], t, d1);
                        d2 = fma(s_v2[e], t, d2);
                    }
                }
                lh = group_sum(lh);
                if (MODE == 0) {
                    d1 = group_sum(d1);
                    d2 = group_sum(d2);
                }
            }
            const bool unobs = mine && ptn >= A.nobs && ptn < A.nptn;
            if (MODE == 1) {
                double pc = 0.0;
                if (unobs) {
                    int ssc = 0;
                    if (br.a_sc) ssc += br.a_sc[ptn];
                    if (br.b_sc) ssc += br.b_sc[ptn];
                    pc = (ssc >= 1 ? lh * kScalingThreshold : lh) + A.invar[ptn];
                }
                u0 += wave_sum64(pc);
            } else {
                const double w0 = wave_sum64(unobs ? lh + A.invar[ptn] : 0.0), w1 = wave_sum64(unobs ? d1 : 0.0), w2 = wave_sum64(unobs ? d2 : 0.0);
                u0 += w0; u1 += w1; u2 += w2;
            }
        }
        if (lane == 0) { s_asc[0] = u0; s_asc[1] = u1; s_asc[2] = u2; }
    }
    __syncthreads();
}

// the three per-evaluation factor arrays at branch length x: exp(cof x) * prop, cof v, cof^2 v (phylokernel.h:600-617)
__device__ __forceinline__ void fill_factors(const NewtonArgs &A, double x, double *s_v0, double *s_v1, double *s_v2) {
    const int B = A.n * A.ncat;
    for (int t = threadIdx.x; t < B; t += 256) {
        const int c = t / A.n;
        const double cof = A.eval[t] * A.rates[c];  // eval: per-category expansion [ncat][n]
        const double v = exp(cof * x) * A.props[c];
        s_v0[t] = v;
        s_v1[t] = cof * v;
        s_v2[t] = cof * (cof * v);
    }
    __syncthreads();
}

// One solve as a workgroup of k_newton / k_newton_batch sees it: the group of workgroups that share the solve's patterns,
// where that group exchanges its partial sums, and the workgroup's LDS.
struct SolveGroup {
    const double *theta;
    int wg, G;                   // this workgroup's number in the group, workgroups in the group
    unsigned long long *posts;   // posted exchange: the group's slots [evaluation][G][2]; nullptr: the counter form
    double *partials;            // counter form: the group's slots [2 parities][G][2] ...
    unsigned int *counter;       // ... and its arrival counter (zero at the launch's start)
    ThetaRegs regs;              // theta in registers; regs.use = false: read from memory in every evaluation (the batch).
                                 // (by value, not an optional pointer: wg_partial's null test on a pointer into this
                                 // frame does not fold, and v[] then lives in scratch)
    bool build_first;            // the first evaluation builds theta = a .* b from the branch ends (phylokernel.h:535-573)
    bool asc_from_ends;          // +ASC: the unobserved patterns' theta comes from the branch ends in EVERY evaluation
                                 // (it does so in any case while theta is being built)
    double *s_v0, *s_v1, *s_v2, *s_red /* [8] */, *s_bcast /* [2] */, *s_asc /* [3] */;
    int *s_fail;
    unsigned int epoch;          // evaluations exchanged so far
};

// The group's sums at branch length x, left in every thread of every workgroup of the group.  `first`: this is the solve's
// first evaluation (a literal at every call: the first evaluation loads or builds theta, the later ones find it in
// ThetaRegs, and each call site is compiled for its own case).
// MODE 0: r0 = sum f*df_ptn, r1 = sum f*ddf_ptn as computeLikelihoodDerv returns them (phylokernel.h:583-651, the repair
// of a non-finite sum, then +ASC's correction :719-724); MODE 1: r0 = sum f*log|lh_ptn| (computeLikelihoodFromBuffer's
// sum, phylokernel.h:1040-1099) with +ASC's -nsites * log(1 - prob_const) (:1183-1186), r1 = 0.
template <int MODE>
__device__ __forceinline__ void solve_sums_at(const NewtonArgs &A, const DevBranch &br, SolveGroup &g, bool first, double x,
                                              double &r0, double &r1) {
    fill_factors(A, x, g.s_v0, g.s_v1, g.s_v2);
    const bool asc = A.nobs < A.nptn;
    const bool build = first && g.build_first;
    if (asc) {
        if (build || g.asc_from_ends) asc_unobserved_sums<true, MODE>(A, g.theta, br, g.s_v0, g.s_v1, g.s_v2, g.s_asc);
        else asc_unobserved_sums<false, MODE>(A, g.theta, br, g.s_v0, g.s_v1, g.s_v2, g.s_asc);
    }
    double p0, p1;
    if (MODE == 0 && build) wg_partial<true, 0>(A, g.theta, br, g.wg, g.G, g.s_v0, g.s_v1, g.s_v2, g.s_red, p0, p1, &g.regs);
    else wg_partial<false, MODE>(A, g.theta, br, g.wg, g.G, g.s_v0, g.s_v1, g.s_v2, g.s_red, p0, p1, &g.regs);
    if (g.G > 1) {
        if (g.posts)
            wg_exchange_posted(g.wg, g.G, g.posts + (size_t)g.epoch * g.G * 2, p0, p1, g.s_bcast, g.s_fail);
        else
            wg_exchange_counted(g.wg, g.G, g.partials + (size_t)(g.epoch & 1) * g.G * 2, g.counter,
                                (g.epoch + 1) * (unsigned int)g.G, p0, p1, g.s_bcast, g.s_fail);
        __syncthreads();   // (one broadcast pair: the next evaluation's wave 0 writes it again)
        g.epoch++;
    }
    if (MODE == 0) {
        newton_repair(p0, p1);
        if (asc) asc_derv_correct(g.s_asc, A.asc_nsites, p0, p1);
    } else if (asc) {
        p0 -= A.asc_nsites * log(1.0 - g.s_asc[0]);
    }
    r0 = p0;
    r1 = p1;
}

// Optimization::minimizeNewton (optimization.cpp:388-465) over solve_sums_at, every workgroup of the group for itself
__device__ __forceinline__ void solve_newton(const NewtonArgs &A, const DevBranch &br, SolveGroup &g, NewtonState &ns,
                                             double xguess, double x1, double x2, double xacc, int max_steps) {
    newton_init(ns, xguess, x1, x2, xacc, max_steps);
    double pdf, pddf;
    solve_sums_at<0>(A, br, g, true, ns.rts, pdf, pddf);
    newton_advance(ns, -pdf, -pddf);   // f = -dlnL/dt, df = -d2lnL/dt2 (phylotree.cpp:2135-2146)
    while (!ns.done) {
        solve_sums_at<0>(A, br, g, false, ns.rts, pdf, pddf);
        newton_advance(ns, -pdf, -pddf);
    }
}

__global__ __launch_bounds__(256) void k_newton(const NewtonArgs A) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int B = A.n * A.ncat;
    __shared__ double s_bcast[2];
    __shared__ double s_asc[3];
    __shared__ int s_fail;
    if (threadIdx.x == 0) s_fail = 0;
    // the arrival counters of consecutive launches alternate; this launch clears the next one's
    if (blockIdx.x == 0 && threadIdx.x == 0)
        __hip_atomic_store(A.barrier_next, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);

    // sum_scale rows of the node updates that ran just before (k_reduce's order: 256 threads, LDS tree)
    if (A.nrows > 0) {
        __shared__ double s_rr[256];
        for (int r = blockIdx.x; r < A.nrows; r += gridDim.x) {
            const double *row = A.slab + (size_t)(2 + r) * A.nwaves;
            double acc = 0.0;
            for (int i = threadIdx.x; i < A.nwaves; i += 256) acc += row[i];
            s_rr[threadIdx.x] = acc;
            __syncthreads();
#pragma unroll
            for (int o = 128; o > 0; o >>= 1) {
                if ((int)threadIdx.x < o) s_rr[threadIdx.x] += s_rr[threadIdx.x + o];
                __syncthreads();
            }
            if (threadIdx.x == 0) A.result[2 + r] = s_rr[0];
            __syncthreads();
        }
        // (the rows are host-visible before this workgroup's first post, hence before workgroup 0 publishes `done`)
        if (A.done && threadIdx.x == 0) __threadfence_system();
    }
    // posted exchange: the slots the NEXT launch will use (the other parity) go back to the sentinel; nobody reads
    // them during this launch
    if (A.posts) {
        for (int t = threadIdx.x; t < kNewtonPostEpochs * 2; t += 256) {
            const int ep = t >> 1;
            reinterpret_cast<unsigned long long *>(A.posts_other)[((size_t)ep * gridDim.x + blockIdx.x) * 2 + (t & 1)] = ~0ull;
        }
    }
    SolveGroup g;
    g.regs.have = false;
    g.regs.use = A.ntiles <= (int64_t)gridDim.x * 4 && (A.mfma ? B <= 80 : B <= 20);
    g.theta = A.theta;
    g.wg = (int)blockIdx.x;
    g.G = (int)gridDim.x;
    g.posts = reinterpret_cast<unsigned long long *>(A.posts);
    g.partials = A.partials;
    g.counter = A.barrier;
    g.build_first = A.build != 0;
    // a launch that builds theta never reads another workgroup's theta tiles (they are plain stores of this very
    // launch: not visible across workgroups without a release / acquire): from the branch ends in every evaluation
    g.asc_from_ends = A.build != 0;
    g.s_v0 = smem; g.s_v1 = smem + B; g.s_v2 = smem + 2 * B; g.s_red = smem + 3 * B;
    g.s_bcast = s_bcast; g.s_asc = s_asc; g.s_fail = &s_fail;
    g.epoch = 0;

    NewtonState ns;
    solve_newton(A, A.br, g, ns, A.xguess, A.x1, A.x2, A.xacc, A.max_steps);
    // "newton raphson diverged, reset" (phylotree.cpp:2167-2176): opt_lh at the result against orig_lh at the starting
    // length, both computeLikelihoodFromBuffer sums of this branch (their lh_scale_factor terms are the same; +ASC: both
    // carry their own -nsites * log(1 - prob_const)), exchanged like the derivative sums
    double result = ns.result, diverged = 0.0;
    if (A.diverge_x > 0.0 && ns.status == 0 && result > A.diverge_x) {
        double opt_lh, orig_lh, unused;
        solve_sums_at<1>(A, A.br, g, false, result, opt_lh, unused);
        solve_sums_at<1>(A, A.br, g, false, A.xguess, orig_lh, unused);
        diverged = 1.0;
        if (orig_lh > opt_lh) result = A.xguess;
    }
    __syncthreads();
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        A.out[0] = result;
        A.out[1] = ns.d2l;
        A.out[2] = (double)ns.neval;
        A.out[3] = (double)(s_fail ? 4 : ns.status);  // 4: the exchange gave up
        if (A.diverge_x > 0.0) A.out[4] = diverged;
        if (A.len_out) *A.len_out = result;
        if (A.done) {
            __threadfence_system();
            *A.done = A.seq;
        }
    }
}

// ---------------------------------------------------------------------------------------
// Batched form: M independent branches (the NNI candidates of a tree, IQTree::evaluateNNIs ->
// getBestNNIForBran, phylotree.cpp:2873-3066) in ONE launch.  Task t owns workgroups [t*G, (t+1)*G), its own
// theta buffer, partial-sum slots and arrival counter; inside a task everything is k_newton: theta is built
// by the first evaluation, every workgroup of the task runs minimizeNewton's control flow redundantly, and a
// last pass gives the lnL at the optimum (computeLikelihoodFromBuffer).  All M*G workgroups must be resident
// (the host sizes G for that and splits larger batches).
// ---------------------------------------------------------------------------------------
struct __attribute__((aligned(16))) NewtonTask {
    DevBranch br;
    double xguess, x1, x2, xacc;
    int32_t max_steps;
    int32_t _pad[3];
};

struct NewtonBatchArgs {
    NewtonArgs c;               // the model / alignment fields are used; theta, br, x*, out are per task
    const NewtonTask *tasks;
    double *theta_base;         // [ntasks][theta_stride]
    size_t theta_stride;
    double *partials;           // [ntasks][2 parities][G][2]
    unsigned int *barriers;     // [ntasks] arrival counters of this launch (zero at its start)
    unsigned int *barriers_next;  // the next launch's counters, cleared here
    double *out;                // [ntasks][6] = {optx, d2l, evaluations, status, lnl, 0}
    int G;
    // posted exchange (see k_newton): slots [task][evaluation][workgroup][2] of this launch, sentinel = not yet posted;
    // the first posts_other_used doubles of the other parity's buffer are reset for the launch after this one
    double *posts;
    double *posts_other;
    size_t posts_other_used;
    int post_epochs;
};

__global__ __launch_bounds__(256) void k_newton_batch(const NewtonBatchArgs P) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const NewtonArgs &A = P.c;
    const int B = A.n * A.ncat;
    __shared__ double s_bcast[2];
    __shared__ double s_asc[3];
    __shared__ int s_fail;
    const int task = (int)blockIdx.x / P.G, wg = (int)blockIdx.x - task * P.G, G = P.G;
    // (read through the constant address space: the branch-end pointers inside are then known to be global and the first
    // evaluation's vector reads are global_load, not flat_load with its catch-all waits)
    typedef const __attribute__((address_space(4))) NewtonTask CTask;
    CTask &Tc = ((CTask *)P.tasks)[task];
    NewtonTask T;
    T.br.a = Tc.br.a; T.br.a_states = Tc.br.a_states; T.br.b = Tc.br.b; T.br.a_sc = Tc.br.a_sc; T.br.b_sc = Tc.br.b_sc;
    T.br.a_kind = Tc.br.a_kind; T.br.b_kind = Tc.br.b_kind; T.br.len = Tc.br.len;
    T.xguess = Tc.xguess; T.x1 = Tc.x1; T.x2 = Tc.x2; T.xacc = Tc.xacc; T.max_steps = Tc.max_steps;
    if (threadIdx.x == 0) {
        s_fail = 0;
        if (wg == 0) __hip_atomic_store(P.barriers_next + task, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (P.posts)
        for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t < P.posts_other_used; t += (size_t)gridDim.x * 256)
            reinterpret_cast<unsigned long long *>(P.posts_other)[t] = ~0ull;
    SolveGroup g;
    g.theta = P.theta_base + (size_t)task * P.theta_stride;
    g.wg = wg;
    g.G = G;
    g.posts = P.posts ? reinterpret_cast<unsigned long long *>(P.posts) + (size_t)task * P.post_epochs * G * 2 : nullptr;
    g.partials = P.partials + (size_t)task * 4 * G;
    g.counter = P.barriers + task;
    g.regs.have = g.regs.use = false;
    g.build_first = true;
    // +ASC: theta of the last tile(s) is in flight from its owner during the task's first evaluation, and with several
    // workgroups per task the owner's plain stores never become visible to the others in this launch (k_newton's
    // rule): from the branch ends then; a task of one workgroup reads back what it wrote itself
    g.asc_from_ends = G > 1;
    g.s_v0 = smem; g.s_v1 = smem + B; g.s_v2 = smem + 2 * B; g.s_red = smem + 3 * B;
    g.s_bcast = s_bcast; g.s_asc = s_asc; g.s_fail = &s_fail;
    g.epoch = 0;

    NewtonState ns;
    solve_newton(A, T.br, g, ns, T.xguess, T.x1, T.x2, T.xacc, T.max_steps);
    // lnL of the branch at the returned length (computeLikelihoodFromBuffer, phylokernel.h:1022-1192)
    double lnl, unused;
    solve_sums_at<1>(A, T.br, g, false, ns.result, lnl, unused);
    __syncthreads();
    if (wg == 0 && threadIdx.x == 0) {
        double *o = P.out + (size_t)task * 6;
        o[0] = ns.result;
        o[1] = ns.d2l;
        o[2] = (double)ns.neval;
        o[3] = (double)(s_fail ? 4 : ns.status);
        o[4] = lnl;
        o[5] = 0.0;
    }
}

size_t newton_task_bytes() { return sizeof(NewtonTask); }
size_t newton_task_branch_offset() { return offsetof(NewtonTask, br); }
void newton_task_fill(void *dst, const DevBranch &br, double xguess, double x1, double x2, double xacc, int max_steps) {
    NewtonTask t;
    memset(&t, 0, sizeof t);
    t.br = br;
    t.xguess = xguess;
    t.x1 = x1;
    t.x2 = x2;
    t.xacc = xacc;
    t.max_steps = max_steps;
    memcpy(dst, &t, sizeof t);
}

// the model and alignment half of NewtonArgs, the same for every solve of an engine
static void fill_model_args(NewtonArgs &A, const iqhip_engine *e) {
    A.eval = e->d_evalc;
    A.rates = e->d_rates;
    A.props = e->d_props;
    A.freq = e->d_freq.p;
    A.invar = e->d_invar.p;
    A.tipc = e->d_tipc;
    A.ntiles = e->ntiles;
    A.nptn = e->nptn;
    A.n = e->n;
    A.ncat = e->ncat;
    A.mfma = e->mfma ? 1 : 0;
    A.nobs = e->nptn - e->n_unobs;
    A.asc_nsites = e->asc_nsites;
}

hipError_t launch_newton_batch(iqhip_engine *e, const void *d_tasks, int ntasks, int G, double *theta_base,
                               size_t theta_stride, double *partials, unsigned int *barriers, unsigned int *barriers_next,
                               double *out, double *posts, double *posts_other, size_t posts_other_used, int post_epochs) {
    NewtonBatchArgs P;
    P.c = NewtonArgs{};   // (theta, the branch, the bounds and the result are per task)
    fill_model_args(P.c, e);
    P.c.build = 1;
    P.tasks = static_cast<const NewtonTask *>(d_tasks);
    P.theta_base = theta_base;
    P.theta_stride = theta_stride;
    P.partials = partials;
    P.barriers = barriers;
    P.barriers_next = barriers_next;
    P.out = out;
    P.G = G;
    P.posts = posts;
    P.posts_other = posts_other;
    P.posts_other_used = posts_other_used;
    P.post_epochs = post_epochs;
    const size_t lds = (size_t)(3 * e->block + 8) * sizeof(double);
    BarrierLaunchGuard guard(e, G > 1);
    hipLaunchKernelGGL(k_newton_batch, dim3((unsigned)(ntasks * G)), dim3(256), lds, e->stream, P);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------
// Newton as a chain of enqueued steps (sharded engines: every step needs an all-reduce of {df, ddf} across the
// ranks, so the loop cannot live inside one kernel).  Per step the engine enqueues
//     derivative kernel at state->rts -> k_reduce -> ncclAllReduce(result[0..1]) -> k_newton_state_update
// and reads the state back once per chunk of steps; steps enqueued after `done` are no-ops.
// ---------------------------------------------------------------------------------------
__global__ void k_newton_state_init(NewtonState *st, double xguess, double x1, double x2, double xacc, int max_steps) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        NewtonState s;
        newton_init(s, xguess, x1, x2, xacc, max_steps);
        *st = s;
    }
}

// asc_nsites > 0: +ASC -- result[2..4] are prob_const, df_const, ddf_const summed over all shards (phylokernel.h:719-724)
__global__ void k_newton_state_update(NewtonState *st, const double *result, double asc_nsites) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        NewtonState s = *st;
        if (!s.done) {
            double df = result[0], ddf = result[1];
            if (asc_nsites > 0.0) {
                newton_repair(df, ddf);   // (phylokernel.h:647-651 comes first)
                asc_derv_correct(result + 2, asc_nsites, df, ddf);
            }
            newton_update(s, df, ddf);
            *st = s;
        }
    }
}

// batched chain: thread t advances task t's state machine from result[2t], result[2t + 1]; asc_nsites > 0 (+ASC): from
// result[5t .. 5t + 4] = {df, ddf, prob_const, df_const, ddf_const} summed over all shards, as k_newton_state_update
__global__ void k_newton_state_update_batch(NewtonState *st, const double *result, int ntasks, double asc_nsites) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= ntasks) return;
    NewtonState s = st[t];
    if (s.done) return;
    if (asc_nsites > 0.0) {
        const double *r = result + 5 * t;
        double df = r[0], ddf = r[1];
        newton_repair(df, ddf);
        asc_derv_correct(r + 2, asc_nsites, df, ddf);
        newton_update(s, df, ddf);
    } else {
        newton_update(s, result[2 * t], result[2 * t + 1]);
    }
    st[t] = s;
}

hipError_t launch_newton_state_update_batch(iqhip_engine *e, NewtonState *states, int ntasks) {
    hipLaunchKernelGGL(k_newton_state_update_batch, dim3((unsigned)((ntasks + 63) / 64)), dim3(64), 0, e->stream, states,
                       e->d_result, ntasks, e->asc_active ? e->asc_nsites : 0.0);
    return hipGetLastError();
}

hipError_t launch_newton_state_init(iqhip_engine *e, double xguess, double x1, double x2, double xacc, int max_steps) {
    hipLaunchKernelGGL(k_newton_state_init, dim3(1), dim3(64), 0, e->stream, e->d_nstate.p, xguess, x1, x2, xacc, max_steps);
    return hipGetLastError();
}

hipError_t launch_newton_state_init_on(hipStream_t s, NewtonState *st, double xguess, double x1, double x2, double xacc,
                                       int max_steps) {
    hipLaunchKernelGGL(k_newton_state_init, dim3(1), dim3(64), 0, s, st, xguess, x1, x2, xacc, max_steps);
    return hipGetLastError();
}

hipError_t launch_derv_at_state(iqhip_engine *e, int nwaves) {
    if (e->mfma) return launch_stream_mfma(e, 2, nullptr, 0.0, nwaves, e->d_nstate.p);
    return launch_derv4(e, 0.0, nwaves, e->d_nstate.p);
}

hipError_t launch_newton_state_update(iqhip_engine *e) {
    hipLaunchKernelGGL(k_newton_state_update, dim3(1), dim3(64), 0, e->stream, e->d_nstate.p, e->d_result, e->asc_active ? e->asc_nsites : 0.0);
    return hipGetLastError();
}

hipError_t launch_newton(iqhip_engine *e, double xguess, double x1, double x2, double xacc, int max_steps,
                         double *out, const DevBranch *build_from, int reduce_rows, int reduce_nwaves,
                         const NewtonSweepStep *sweep) {
    NewtonArgs A;
    fill_model_args(A, e);
    A.len_out = sweep ? sweep->len_out : nullptr;
    A.diverge_x = sweep ? sweep->diverge_x : 0.0;
    A.build = build_from ? 1 : 0;
    A.br = build_from ? *build_from : DevBranch{nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, 0.0};
    A.slab = e->d_slab.p;
    A.result = sweep ? sweep->rows_base - 2 : e->d_result;   // (row r of the node updates goes to result[2 + r])
    A.nrows = reduce_rows;
    A.nwaves = reduce_nwaves;
    A.theta = e->d_theta.p;
    A.partials = e->d_newton_partials.p;
    A.out = out;
    A.xguess = xguess;
    A.x1 = x1;
    A.x2 = x2;
    A.xacc = xacc;
    A.max_steps = max_steps;
    // every workgroup must be resident for the exchange: one per CU with the arrival counter (its slots are sized for that),
    // two per CU with the posted exchange (226 registers since theta stays in them: two fit), so that a 100 k-pattern alignment
    // has one tile per wave and a derivative pass is one round trip
    const bool posts = e->newton_posts && max_steps + 5 <= kNewtonPostEpochs;   // (+2: the lnL passes of the diverged-solve rule)
    const int64_t wgs = (e->ntiles + 3) / 4;
    const int64_t max_grid = posts ? 2 * (int64_t)e->num_cus : e->num_cus;
    int grid = (int)(wgs < 1 ? 1 : (wgs > max_grid ? max_grid : wgs));
    A.barrier = e->d_newton_barrier.p + (e->newton_launches & 1);
    A.barrier_next = e->d_newton_barrier.p + ((e->newton_launches + 1) & 1);
    e->newton_launches++;
    A.done = nullptr;
    A.seq = 0;
    // (a single workgroup reduces all rows itself; several need the posted exchange in between -- the counter form
    // gives the same ordering, the rows are written before the workgroup's first arrival)
    if ((!sweep || sweep->publish) && e->poll_result && e->d_result == e->d_result_own && out >= e->d_result &&
        out < e->d_result + e->result_cap) {
        A.seq = ++e->result_seq;
        A.done = e->d_done;
        e->poll_pending = true;
    }
    A.posts = A.posts_other = nullptr;
    if (grid > 1 && posts) {
        const size_t per = (size_t)kNewtonPostEpochs * (2 * e->num_cus) * 2;   // (slots are indexed with the launch's grid <= 2 num_cus)
        A.posts = e->d_newton_posts.p + (e->newton_post_launches & 1) * per;
        A.posts_other = e->d_newton_posts.p + ((e->newton_post_launches + 1) & 1) * per;
        e->newton_post_launches++;
    }
    const size_t lds = (size_t)(3 * e->block + 8) * sizeof(double);
    BarrierLaunchGuard guard(e, grid > 1);
    hipLaunchKernelGGL(k_newton, dim3(grid), dim3(256), lds, e->stream, A);
    return hipGetLastError();
}

}  // namespace iqhip
