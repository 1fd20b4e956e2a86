// wg_exchange.h -- the hand-off of two partial sums between the resident workgroups of one group (k_newton's grid, one
// task of k_newton_batch, k_sweep4's grid), in its two forms.  Device only; nothing else lives here.
//
// Both forms take the group (wg of G), this evaluation's slots, the workgroup's two partial sums in p0 / p1, an LDS pair
// for the broadcast and the LDS fail flag, and leave the two group sums in p0 / p1 of EVERY thread: wave 0 adds the G
// slots in a fixed order (lane w takes w, w + 64, ...; then wave_sum64), identically in every workgroup and in both
// forms, so every workgroup continues from the same bits.
//
// The sums travel as relaxed agent-scope atomic stores (write-through) and are read back with relaxed agent-scope
// loads; there is no release / acquire fence -- a fence writes back and invalidates the XCD's L2, i.e. throws away the
// theta slice a workgroup re-reads in every Newton step.  This is outside the HIP memory model proper: it is the
// "8-byte agent atomics on both sides" form measured for gfx950 (MI355X_MICROARCH.md, Workgroup dispatch, valid forms).
// Every wait is a bounded s_sleep spin: an exchange that gives up sets *s_fail (status 4; the host then finishes the
// solve with the barrier-free chain form) and never hangs the GPU.
//
// Barriers: each form ends with exactly ONE __syncthreads(), the one between wave 0's write of `bcast` and everybody's
// read of it.  A caller that hands the same `bcast` pair to its next exchange puts a barrier of its own behind the call
// (k_newton, k_newton_batch); a caller that alternates between two pairs by the evaluation's parity needs none
// (k_sweep4: a write of the evaluation after the next lies behind the next evaluation's barrier).
// All G workgroups must be resident, and the slots (and the counter) belong to this evaluation alone; how they are
// reset for re-use is the calling kernel's schedule.
#pragma once
#include "iqhip_internal.h"

namespace iqhip {

// Posted form: every (evaluation, workgroup) owns a slot {p0, p1} that holds the all-ones pattern until its owner
// stores into it; each double is an 8-byte agent-scope store, valid on its own, so there is no arrival counter, no wait
// for a store acknowledgement before it and no ordering between the two stores to rely on.  Wave 0 of every workgroup
// spins on the slots of the evaluation.  9 -> 5.5 us per evaluation at 256 workgroups against the counter form.
// slots: [G][2] of this evaluation, all-ones = not posted yet.
__device__ __forceinline__ void wg_exchange_posted(int wg, int G, unsigned long long *slots, double &p0, double &p1,
                                                   double *bcast, int *s_fail) {
    if (threadIdx.x == 0) {
        unsigned long long ua = __double_as_longlong(p0), ub = __double_as_longlong(p1);
        if (ua == ~0ull) ua = 0x7ff8000000000000ull;   // (a NaN that happens to be the sentinel: any other NaN)
        if (ub == ~0ull) ub = 0x7ff8000000000000ull;
        __hip_atomic_store(&slots[2 * wg], ua, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&slots[2 * wg + 1], ub, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (threadIdx.x < 64) {
        double a = 0.0, b = 0.0;
        long spins = 0;
        for (;;) {
            bool ready = true;
            a = 0.0; b = 0.0;
            for (int w = threadIdx.x; w < G; w += 64) {
                const unsigned long long ua = __hip_atomic_load(&slots[2 * w], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const unsigned long long ub = __hip_atomic_load(&slots[2 * w + 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                ready = ready && ua != ~0ull && ub != ~0ull;
                a += __longlong_as_double(ua);
                b += __longlong_as_double(ub);
            }
            if (__all(ready)) break;
            __builtin_amdgcn_s_sleep(1);
            if (++spins > 2000000L) { if (threadIdx.x == 0) *s_fail = 1; break; }  // never hang the GPU
        }
        a = wave_sum64(a);
        b = wave_sum64(b);
        if (threadIdx.x == 0) { bcast[0] = a; bcast[1] = b; }
    }
    __syncthreads();
    p0 = bcast[0];
    p1 = bcast[1];
}

// Arrival-counter form: thread 0 stores the workgroup's slot, waits for the stores' acknowledgement (s_waitcnt
// vmcnt(0)), adds one to the group's counter and spins until all G workgroups of this evaluation have arrived
// (`target`: the counter only counts up over the evaluations of a launch); then wave 0 sums the slots.
// slot: [G][2] of this evaluation's parity (two parities alternate: a workgroup can be at most one evaluation ahead).
__device__ __forceinline__ void wg_exchange_counted(int wg, int G, double *slot, unsigned int *counter, unsigned int target,
                                                    double &p0, double &p1, double *bcast, int *s_fail) {
    if (threadIdx.x == 0) {
        __hip_atomic_store(&slot[2 * wg], p0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&slot[2 * wg + 1], p1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        long spins = 0;
        while (__hip_atomic_load(counter, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target) {
            __builtin_amdgcn_s_sleep(1);
            if (++spins > 4000000L) { *s_fail = 1; break; }  // never hang the GPU (~0.2 s)
        }
    }
    __syncthreads();
    if (threadIdx.x < 64) {
        double a = 0.0, b = 0.0;
        for (int w = threadIdx.x; w < G; w += 64) {
            a += __hip_atomic_load(&slot[2 * w], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            b += __hip_atomic_load(&slot[2 * w + 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        a = wave_sum64(a);
        b = wave_sum64(b);
        if (threadIdx.x == 0) { bcast[0] = a; bcast[1] = b; }
    }
    __syncthreads();
    p0 = bcast[0];
    p1 = bcast[1];
}

}  // namespace iqhip
