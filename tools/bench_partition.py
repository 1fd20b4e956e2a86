"""Edge-linked partition models: one joint branch solve (iqhip_partition_newton_branch) and one optimizeAllBranches pass of
the host mirror (PhyloSuperTree) at DNA GTR+G4, 50 taxa, P = 8 / 32 / 128 partitions of 500 patterns each, against the
route a caller of the public ABI had before the group existed: per Newton step and member one iqhip_derv, the weighted sum
and iqhip_newton_host_update on the host -- in the same process, on the same resident thetas, alternating with the joint
route.  Reported per P: launches and host reads per joint solve, device time of the two kernels per launch (HIP events),
wall time per solve of both routes (median of `reps` alternating repetitions over `nbranch` branches, after a warm-up of
every shape), the wall time per branch of one optimizeAllBranches pass, the wall time per branch of what both routes share
(pending partials + theta on every member), and whether both routes agree.
    python tools/bench_partition.py [reps [nbranch]]          default 20 repetitions on 6 branches
Prints one line of JSON per P.  No ratio is fixed here."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as g  # noqa: E402

pkg = g.load_package()
import importlib  # noqa: E402

import partition_ref as pr  # noqa: E402

synth = importlib.import_module("iqtree_amd.synth")
NTAXA, NPTN = 50, 500


def make_parts(nwk, P, rates):
    model = synth.gtr_model(alpha=0.9, ncat=4)
    parts = []
    for p in range(P):
        nsites = 620
        while True:
            st = synth.simulate_alignment(pr.scale_newick(nwk, rates[p]), model, nsites, 1000 + p)
            pat, freq = synth.compress_patterns(st)
            if pat.shape[1] >= NPTN:
                break
            nsites = int(nsites * 1.3)
        pat, freq = np.ascontiguousarray(pat[:, :NPTN]), freq[:NPTN].copy()
        parts.append(dict(name="p%d" % p, nstates=4, seq_type=0, pat=pat, freq=freq, model=model))
    return parts


def host_route(lib, engines, rates, xguess, x1, x2, xacc, max_steps):
    """per step and member: iqhip_derv, the weighted sum, iqhip_newton_host_update -> (optx, evaluations, host reads)"""
    sm = pkg.NewtonStateMachine(xguess, x1, x2, xacc, max_steps)
    df, ddf = C.c_double(), C.c_double()
    reads = 0
    while not sm.done:
        x = sm.x
        sdf = sddf = 0.0
        for e, r in zip(engines, rates):
            if lib.iqhip_derv(e, r * x, C.byref(df), C.byref(ddf)) != 0:
                raise RuntimeError(lib.iqhip_last_error())
            reads += 1
            sdf += r * df.value       # (iqhip_derv has applied the NaN / inf rule to this member already)
            sddf += r * r * ddf.value
        sm.update(sdf, sddf)
    optx, _, n, status = sm.result()
    assert status == 0
    return optx, n, reads


def chunks_for(evals, max_steps):
    """host reads of the joint solve: the state is read once per chunk of steps (4, then 2 at a time)"""
    enq, n = 0, 0
    while enq < evals:
        enq += min(4, max_steps + 1) if enq == 0 else 2
        n += 1
    return n


def run(P, reps, nbranch):
    lib = pkg.libiqhip()
    nwk = synth.random_tree_newick(NTAXA, 1, 0.02, 0.2)
    rng = np.random.default_rng(5 + P)
    rates = rng.uniform(0.5, 2.0, P)
    rates *= P / rates.sum()
    parts = make_parts(nwk, P, rates)
    st = pkg.PhyloSuperTree(nwk, parts)
    st.part_rates = rates
    st.compute_likelihood()
    engines = [t.engine for t in st.members]
    grp = pkg.PartitionGroup(engines)
    grp.set_rates(rates)
    order = st.branch_order()
    pick = [order[(k * len(order)) // nbranch] for k in range(nbranch)]
    args = (1e-6, 100.0, 1e-6, 100)
    joint_ms, host_ms, prep_ms, derv_us, upd_us = [], [], [], [], []
    launches = evals = reads_joint = reads_host = 0
    worst, mismatched = 0.0, 0
    for (a, b) in pick:
        x0 = st.branch_length(a, b)
        st.partition_newton_branch(a, b, x0, *args)                       # theta of (a, b) on every member (+ a warm-up solve)
        grp.newton_branch(x0, *args)
        host_route(lib, engines, rates, x0, *args)
        for t in st.members:                                              # what both routes share, timed on its own
            t.reset_theta()
        t0 = time.perf_counter()
        for t in st.members:
            t.compute_likelihood_derv(a, b)
        prep_ms.append((time.perf_counter() - t0) * 1e3)
        for _ in range(reps):                                             # alternating, same thetas
            t0 = time.perf_counter()
            got = grp.newton_branch(x0, *args)
            joint_ms.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            ref = host_route(lib, engines, rates, x0, *args)
            host_ms.append((time.perf_counter() - t0) * 1e3)
            worst = max(worst, abs(got[0] - ref[0]) / max(1.0, abs(ref[0])))
            mismatched += got[2] != ref[1]
        launches, evals = grp.timing()["launches"], got[2]
        reads_joint, reads_host = chunks_for(evals, 100), ref[2]
        lib.iqhip_timing_enable(engines[0], 1)
        grp.newton_branch(x0, *args)
        tm = grp.timing()
        lib.iqhip_timing_enable(engines[0], 0)
        steps = (tm["launches"] - 1 - 2 * chunks_for(evals, 100)) // 2      # (derivative, update) pairs enqueued
        derv_us.append(tm["derv_ms"] * 1e3 / steps)
        upd_us.append(tm["update_ms"] * 1e3 / steps)
    grp.close()
    st.optimize_all_branches(iterations=1)                                # warm-up pass (plans, scratch)
    t0 = time.perf_counter()
    st.optimize_all_branches(iterations=1)
    pass_ms = (time.perf_counter() - t0) * 1e3
    med = lambda v: float(np.median(v))   # noqa: E731
    print(json.dumps(dict(
        workload="DNA GTR+G4", taxa=NTAXA, partitions=P, patterns_per_partition=NPTN, branches_timed=nbranch, reps=reps,
        evaluations_last_solve=int(evals), joint_launches_per_solve=int(launches), joint_host_reads_per_solve=int(reads_joint),
        host_route_launches_per_solve=int(2 * reads_host), host_route_reads_per_solve=int(reads_host),
        k_part_derv_device_us=med(derv_us), k_part_newton_update_device_us=med(upd_us),
        joint_solve_wall_us=med(joint_ms) * 1e3, host_route_solve_wall_us=med(host_ms) * 1e3,
        joint_solve_wall_us_min=min(joint_ms) * 1e3, host_route_solve_wall_us_min=min(host_ms) * 1e3,
        shared_partials_theta_wall_us_per_branch=med(prep_ms) * 1e3,
        all_branches_pass_wall_us_per_branch=pass_ms * 1e3 / len(order), branches=len(order),
        max_rel_diff_optx=worst, solves_with_other_evaluation_count=int(mismatched))), flush=True)
    st.close()


if __name__ == "__main__":
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    nbranch = int(sys.argv[2]) if len(sys.argv) > 2 else 6
    if pkg.libiqhip().iqhip_device_count() < 1:
        raise SystemExit("bench_partition.py: no HIP device visible")
    for P in (8, 32, 128):
        run(P, reps, nbranch)
