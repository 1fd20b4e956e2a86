// kernels_partnewton.hip -- the joint branch solve of an edge-linked partition model (-q / -spp).
//
// PhyloSuperTreePlen::computeFuncDerv (phylosupertreeplen.cpp:530-578) optimises ONE super-tree branch length x against
// the sum over the partitions, sum_p r_p df_p(r_p x) and sum_p r_p^2 ddf_p(r_p x); every partition is an engine of its
// own with its own model, alignment and theta.  k_newton and its relatives see one engine, so the loop here is the
// enqueued chain of the sharded engines (kernels_newton.hip, "Newton as a chain of enqueued steps") with a derivative
// kernel that spans engines:
//     k_newton_state_init, then per evaluation  k_part_derv<0> -> k_part_newton_update
// and the host reads the 128-byte state once per chunk of steps (partition.hip).  Workgroups never talk to each other
// inside a launch -- no grid barrier, no spinning, no atomics: a work item's {df, ddf} goes to a slot of its own and the
// next launch of the same stream sums the slots in a fixed order, so the bits are the same on every run.
//
// The batch of joint solves (iqhip_partition_optimize_branch_batch: the NNI candidates of a super tree side by side) is
// the same chain with a task dimension: ntasks device-resident states, per evaluation
//     k_part_derv_batch<0> (grid: work item x task) -> k_part_newton_update_batch (one workgroup per task)
// and behind the last chunk of steps k_part_derv_batch<1> -> k_part_lnl_finish_batch -> out[task][member].  Task t reads
// slot t of every member's theta batch (eng_batch_prepare) and writes partials[t][item][2]; a task that is done does
// nothing.  The per-item body (part_item_sums), the member and item sums (part_newton_update, part_lnl_of_member) are the
// single solve's own functions, so a task's bits are those of iqhip_partition_newton_branch on the same theta.
// With rows (iqhip_partition_optimize_branch_batch_rows) that lnL pass also stores every pattern's value, before the
// multiplication by its frequency, into the task's row of the member's per-pattern store: no launch and no read is added.
#include "iqhip_internal.h"

namespace iqhip {

// The per-item body of k_part_derv and k_part_derv_batch.  A work item is a contiguous run of tiles of one member, one
// workgroup each, wave w taking tiles first + w, first + w + 4, ..
// The per-pattern arithmetic is wg_partial's (kernels_newton.hip) for a theta in memory: 64-pattern double2 tiles for the
// 4-state engines, 16-pattern tiles with the block entries spread over the four lane groups for the matrix-core ones.
// MODE 0: sums of f * df_ptn, f * ddf_ptn at the member's length rate * x.
// MODE 1: sum of f * (log|lh_ptn| + scale counters * LOG_SCALING_THRESHOLD) at rate * x.
// theta, a_sc, b_sc: the member's resident theta and its ends' counters (D's own), or those of a task's slot.
// row (MODE 1; nullptr: none): a row of the member's per-pattern store, nptn_pad doubles.  row[ptn] = the pattern's l before
// the multiplication by f -- log|lh + invar| with the repair, the counters of both ends put back -- and 0 in the padding of
// a ragged last tile.  A plain vector store by the lane that holds the value (matrix-core tiles: lane group 0); the tiles of
// a member cover [0, nptn_pad) exactly, every pattern once.
template <int MODE>
__device__ __forceinline__ void part_item_sums(const PartDesc &D, const PartItem &it, const double *__restrict__ theta,
                                               const int16_t *__restrict__ a_sc, const int16_t *__restrict__ b_sc, double x,
                                               double *smem, double *__restrict__ out2, double *__restrict__ row = nullptr) {
    const int B = D.n * D.ncat;
    double *s_v0 = smem, *s_v1 = smem + B, *s_v2 = smem + 2 * B, *s_red = smem + 3 * B;   // s_red[8]
    const double len = D.rate * x;
    for (int t = threadIdx.x; t < B; t += 256) {
        const int c = t / D.n;
        const double cof = D.evalc[t] * D.rates[c];   // evalc: per-category expansion [ncat][n]
        const double v = exp(cof * len) * D.props[c];
        s_v0[t] = v;
        s_v1[t] = cof * v;
        s_v2[t] = cof * (cof * v);
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double adf = 0.0, addf = 0.0;
    const int64_t tile_end = it.first_tile + it.ntiles;
    for (int64_t tile = it.first_tile + wave; tile < tile_end; tile += 4) {
        double lh = 0.0, d1 = 0.0, d2 = 0.0;
        int64_t ptn;
        bool mine, holder = true;   // holder: this lane has the pattern's value (and writes its row entry)
        if (!D.mfma) {
            ptn = tile * 64 + lane;
            mine = ptn < D.nptn;
            const double2 *p = reinterpret_cast<const double2 *>(theta + tile * (64 * B)) + lane;
            for (int j = 0; j < B / 2; j++) {
                const double2 t = p[j * 64];
                lh = fma(s_v0[2 * j], t.x, lh); lh = fma(s_v0[2 * j + 1], t.y, lh);
                if (MODE == 0) {
                    d1 = fma(s_v1[2 * j], t.x, d1); d1 = fma(s_v1[2 * j + 1], t.y, d1);
                    d2 = fma(s_v2[2 * j], t.x, d2); d2 = fma(s_v2[2 * j + 1], t.y, d2);
                }
            }
        } else {
            const int p = lane & 15, g = lane >> 4;
            ptn = tile * 16 + p;
            holder = g == 0;
            mine = holder && ptn < D.nptn;
            const double *th = theta + (size_t)tile * 16 * B;
            // a pattern's rows 20 at a time: all 20 loads of a lane are in flight together
            for (int e0 = g; e0 < B; e0 += 80) {
                double tv[20];
#pragma unroll
                for (int q = 0; q < 20; q++) {
                    const int e = e0 + 4 * q;
                    tv[q] = e < B ? th[(size_t)e * 16 + p] : 0.0;
                }
#pragma unroll
                for (int q = 0; q < 20; q++) {
                    const int e = e0 + 4 * q;
                    if (e < B) {
                        lh = fma(s_v0[e], tv[q], lh);
                        if (MODE == 0) {
                            d1 = fma(s_v1[e], tv[q], d1);
                            d2 = fma(s_v2[e], tv[q], d2);
                        }
                    }
                }
            }
            lh = group_sum(lh);
            if (MODE == 0) {
                d1 = group_sum(d1);
                d2 = group_sum(d2);
            }
        }
        if (mine) {
            lh += D.invar[ptn];
            const double f = D.freq[ptn];
            if (MODE == 1) {
                double l = log(fabs(lh));
                if (isnan(l) || isinf(l)) l = kLogScalingThreshold * 4;  // the reference's repair, phylokernel.h:1100-1122
                int ssc = 0;
                if (a_sc) ssc += a_sc[ptn];
                if (b_sc) ssc += b_sc[ptn];
                l += (double)ssc * kLogScalingThreshold;
                if (row) row[ptn] = l;
                adf = fma(l, f, adf);
            } else {
                const double inv = 1.0 / fabs(lh);
                const double dfp = d1 * inv;
                const double ddfp = fma(-dfp, dfp, d2 * inv);
                adf = fma(dfp, f, adf);
                addf = fma(ddfp, f, addf);
            }
        } else if (MODE == 1 && row && holder) {
            row[ptn] = 0.0;   // (ptn < nptn_pad: the member's tiles end there)
        }
    }
    adf = wave_sum64(adf);
    addf = wave_sum64(addf);
    if (lane == 0) { s_red[2 * wave] = adf; s_red[2 * wave + 1] = addf; }
    __syncthreads();
    if (threadIdx.x == 0) {
        out2[0] = (s_red[0] + s_red[2]) + (s_red[4] + s_red[6]);
        out2[1] = (s_red[1] + s_red[3]) + (s_red[5] + s_red[7]);
    }
}

// One workgroup per work item, the member's resident theta.
// MODE 0: at st->rts; nothing once the solve is done.
// MODE 1: at (st ? st->result : x_given); with a state machine, nothing until it is done.
template <int MODE>
__global__ __launch_bounds__(256) void k_part_derv(const PartDesc *__restrict__ descs, const PartItem *__restrict__ items,
                                                   const NewtonState *st, double x_given, double *__restrict__ partials) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    double x = x_given;
    if (MODE == 0) {
        if (st->done) return;
        x = st->rts;
    } else if (st) {   // (enqueued behind a chunk of steps: only once they have finished the solve)
        if (!st->done) return;
        x = st->result;
    }
    const PartItem it = items[blockIdx.x];
    const PartDesc D = descs[it.member];
    part_item_sums<MODE>(D, it, D.theta, D.a_sc, D.b_sc, x, smem, partials + 2 * (size_t)blockIdx.x);
}

// The batch of joint solves (iqhip_partition_optimize_branch_batch): workgroup (item, task) runs the same body on slot
// `task` of the item's member, at the length in the task's own state machine, into partials[task][item][2].
// MODE 0: a task that is done does nothing.  MODE 1: at the task's result; the pass rides behind every chunk of steps, as the
// single solve's does, so a task that is not done yet does nothing, and neither does one whose sums an earlier pass wrote
// (lnl_written[task], zero at the start of the chain and set by k_part_lnl_finish_batch; nothing overwrites the partials of a
// task that is done).
template <int MODE>
__global__ __launch_bounds__(256) void k_part_derv_batch(const PartDesc *__restrict__ descs, const PartItem *__restrict__ items,
                                                         const PartSlots *__restrict__ slots,
                                                         const int16_t *const *__restrict__ sc, int nparts,
                                                         const NewtonState *__restrict__ states,
                                                         const int32_t *__restrict__ lnl_written,
                                                         double *__restrict__ partials, double *const *__restrict__ rowp) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int task = blockIdx.y;
    const NewtonState *st = states + task;
    if ((MODE == 0) == (st->done != 0)) return;
    if (MODE == 1 && lnl_written[task]) return;   // (its sums are in partials already)
    const double x = MODE == 0 ? st->rts : st->result;
    const PartItem it = items[blockIdx.x];
    const PartDesc D = descs[it.member];
    const PartSlots S = slots[it.member];
    const int16_t *const *ends = sc + 2 * ((size_t)task * nparts + it.member);
    // rowp (MODE 1; nullptr: no rows): [ntasks][nparts], the task's row of the member's store or nullptr.  The guard above
    // lets a task through once, so its row is written exactly once -- from the slot, the counters and the result alone
    double *row = (MODE == 1 && rowp) ? rowp[(size_t)task * nparts + it.member] : nullptr;
    part_item_sums<MODE>(D, it, S.theta + (size_t)task * S.stride, ends[0], ends[1], x, smem,
                         partials + 2 * ((size_t)task * gridDim.x + blockIdx.x), row);
}

// The update of one solve, run by one workgroup of kPartUpdateThreads: 64 members at a time, thread t sums the items of
// member base + t in item order and applies the reference's per-partition NaN / inf rule (phylokernel.h:647-651); thread 0
// then adds r df and r^2 ddf of those members in member order.  After the last member: newton_update, the state machine
// of every enqueued chain.  partials: [nitems][2] of this solve; s_m: 2 * kPartUpdateThreads doubles of LDS.
__device__ __forceinline__ void part_newton_update(const PartDesc *__restrict__ descs, int nparts,
                                                   const double *__restrict__ partials, NewtonState *st, double *s_m) {
    if (st->done) return;
    double sdf = 0.0, sddf = 0.0;
    for (int base = 0; base < nparts; base += kPartUpdateThreads) {
        const int m = base + (int)threadIdx.x;
        if (m < nparts) {
            const int first = descs[m].item_first, cnt = descs[m].nitems;
            double df = 0.0, ddf = 0.0;
            for (int i = 0; i < cnt; i++) {
                df += partials[2 * (size_t)(first + i)];
                ddf += partials[2 * (size_t)(first + i) + 1];
            }
            if (isnan(df) || isinf(df)) { df = 0.0; ddf = 0.0; }
            const double r = descs[m].rate;
            s_m[2 * threadIdx.x] = r * df;
            s_m[2 * threadIdx.x + 1] = (r * r) * ddf;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            const int cnt = nparts - base < kPartUpdateThreads ? nparts - base : kPartUpdateThreads;
            for (int k = 0; k < cnt; k++) {
                sdf += s_m[2 * k];
                sddf += s_m[2 * k + 1];
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        NewtonState s = *st;
        newton_update(s, sdf, sddf);
        *st = s;
    }
}

__global__ __launch_bounds__(kPartUpdateThreads) void k_part_newton_update(const PartDesc *__restrict__ descs, int nparts,
                                                                           const double *__restrict__ partials,
                                                                           NewtonState *st) {
    __shared__ double s_m[2 * kPartUpdateThreads];
    part_newton_update(descs, nparts, partials, st, s_m);
}

// ... of a batch: workgroup t advances the state machine of task t from partials[t][nitems][2]
__global__ __launch_bounds__(kPartUpdateThreads) void k_part_newton_update_batch(const PartDesc *__restrict__ descs, int nparts,
                                                                                 int nitems, const double *__restrict__ partials,
                                                                                 NewtonState *states) {
    __shared__ double s_m[2 * kPartUpdateThreads];
    part_newton_update(descs, nparts, partials + 2 * (size_t)blockIdx.x * nitems, states + blockIdx.x, s_m);
}

// the MODE 1 sums of member m's items, in item order
__device__ __forceinline__ double part_lnl_of_member(const PartDesc *__restrict__ descs, int m, const double *__restrict__ partials) {
    const int first = descs[m].item_first, cnt = descs[m].nitems;
    double s = 0.0;
    for (int i = 0; i < cnt; i++) s += partials[2 * (size_t)(first + i)];
    return s;
}

// out[m] = the MODE 1 sums of member m's items
__global__ __launch_bounds__(64) void k_part_lnl_finish(const PartDesc *__restrict__ descs, int nparts,
                                                        const double *__restrict__ partials, double *__restrict__ out) {
    const int m = blockIdx.x * 64 + threadIdx.x;
    if (m >= nparts) return;
    out[m] = part_lnl_of_member(descs, m, partials);
}

// out[task][m] of a batch, task = blockIdx.y (of a task that is not done yet: whatever its partials hold; the pass behind
// a later chunk of steps writes it again); a task that is done is marked, so that later MODE 1 passes leave it alone
__global__ __launch_bounds__(64) void k_part_lnl_finish_batch(const PartDesc *__restrict__ descs, int nparts, int nitems,
                                                              const double *__restrict__ partials,
                                                              const NewtonState *__restrict__ states,
                                                              int32_t *__restrict__ lnl_written, double *__restrict__ out) {
    const int m = blockIdx.x * 64 + threadIdx.x;
    if (m >= nparts) return;
    out[(size_t)blockIdx.y * nparts + m] = part_lnl_of_member(descs, m, partials + 2 * (size_t)blockIdx.y * nitems);
    if (m == 0 && states[blockIdx.y].done) lnl_written[blockIdx.y] = 1;
}

// The scale-factor term of a traversal's root-branch lnL (the lh_scale_factor of the two ends, phylokernel.h:1028): block m
// sums freq * (a_sc + b_sc) over member m's patterns -- thread-strided, then an LDS tree, k_reduce's order
__global__ __launch_bounds__(256) void k_part_scale_terms(const PartScale *__restrict__ sc, double *__restrict__ out) {
    __shared__ double s[256];
    const PartScale S = sc[blockIdx.x];
    double acc = 0.0;
    for (int64_t p = threadIdx.x; p < S.nptn; p += 256) {
        int ssc = 0;
        if (S.a_sc) ssc += S.a_sc[p];
        if (S.b_sc) ssc += S.b_sc[p];
        acc += S.freq[p] * (double)ssc;
    }
    s[threadIdx.x] = acc;
    __syncthreads();
#pragma unroll
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) s[threadIdx.x] += s[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[blockIdx.x] = s[0] * kLogScalingThreshold;
}

hipError_t launch_part_derv(hipStream_t s, int mode, const PartDesc *d_desc, const PartItem *d_items, int nitems,
                            int lds_doubles, const NewtonState *st, double x, double *partials) {
    const size_t lds = (size_t)(lds_doubles + 8) * sizeof(double);
    if (mode == 0) hipLaunchKernelGGL(k_part_derv<0>, dim3((unsigned)nitems), dim3(256), lds, s, d_desc, d_items, st, x, partials);
    else hipLaunchKernelGGL(k_part_derv<1>, dim3((unsigned)nitems), dim3(256), lds, s, d_desc, d_items, st, x, partials);
    return hipGetLastError();
}

hipError_t launch_part_newton_update(hipStream_t s, const PartDesc *d_desc, int nparts, const double *partials,
                                     NewtonState *st) {
    hipLaunchKernelGGL(k_part_newton_update, dim3(1), dim3(kPartUpdateThreads), 0, s, d_desc, nparts, partials, st);
    return hipGetLastError();
}

hipError_t launch_part_lnl_finish(hipStream_t s, const PartDesc *d_desc, int nparts, const double *partials, double *out) {
    hipLaunchKernelGGL(k_part_lnl_finish, dim3((unsigned)((nparts + 63) / 64)), dim3(64), 0, s, d_desc, nparts, partials, out);
    return hipGetLastError();
}

hipError_t launch_part_derv_batch(hipStream_t s, int mode, const PartDesc *d_desc, const PartItem *d_items, int nitems,
                                  int lds_doubles, const PartSlots *d_slots, const int16_t *const *d_sc, int nparts,
                                  const NewtonState *states, const int32_t *lnl_written, int ntasks, double *partials,
                                  double *const *d_rowp) {
    const size_t lds = (size_t)(lds_doubles + 8) * sizeof(double);
    const dim3 grid((unsigned)nitems, (unsigned)ntasks);
    if (mode == 0) hipLaunchKernelGGL(k_part_derv_batch<0>, grid, dim3(256), lds, s, d_desc, d_items, d_slots, d_sc, nparts, states, lnl_written, partials, nullptr);
    else hipLaunchKernelGGL(k_part_derv_batch<1>, grid, dim3(256), lds, s, d_desc, d_items, d_slots, d_sc, nparts, states, lnl_written, partials, d_rowp);
    return hipGetLastError();
}

hipError_t launch_part_newton_update_batch(hipStream_t s, const PartDesc *d_desc, int nparts, int nitems,
                                           const double *partials, NewtonState *states, int ntasks) {
    hipLaunchKernelGGL(k_part_newton_update_batch, dim3((unsigned)ntasks), dim3(kPartUpdateThreads), 0, s, d_desc, nparts,
                       nitems, partials, states);
    return hipGetLastError();
}

hipError_t launch_part_lnl_finish_batch(hipStream_t s, const PartDesc *d_desc, int nparts, int nitems, const double *partials,
                                        const NewtonState *states, int32_t *lnl_written, double *out, int ntasks) {
    hipLaunchKernelGGL(k_part_lnl_finish_batch, dim3((unsigned)((nparts + 63) / 64), (unsigned)ntasks), dim3(64), 0, s, d_desc,
                       nparts, nitems, partials, states, lnl_written, out);
    return hipGetLastError();
}

hipError_t launch_part_scale_terms(hipStream_t s, const PartScale *d_sc, int nparts, double *out) {
    hipLaunchKernelGGL(k_part_scale_terms, dim3((unsigned)nparts), dim3(256), 0, s, d_sc, out);
    return hipGetLastError();
}

}  // namespace iqhip
