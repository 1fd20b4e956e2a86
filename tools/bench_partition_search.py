"""A batch of joint branch solves on a partition group (iqhip_partition_optimize_branch_batch) against the same work done
branch by branch with the calls that existed before it: per candidate and member iqhip_update_partials + iqhip_compute_theta,
then one iqhip_partition_newton_branch.  The work is the first round of an nni1 evaluation of a 50-taxon super tree: for
each of the 47 internal branches the first NNI candidate (two node updates on scratch vectors, then the joint solve of the
central branch).  Four partitions: DNA GTR+G4 at 20 000 sites, DNA with one category, protein +G4 at 5 000 sites, binary
data with two categories.
    python tools/bench_partition_search.py [reps]              default 10 repetitions
Reports, per form: wall time per evaluation of all candidates (median), launches on the group's stream, host waits, and for
the batch the device time of the derivative and of the update launches (HIP events); and whether both forms return the same
bits.  Then, on the host mirror's PhyloSuperTree over the same data, one evaluation of all nni5 candidates batched
(evaluate_nnis5_batch) and branch by branch (nni_for_branch): wall time, batches, joint single solves, and the largest
relative difference of the candidates' log-likelihoods; and one optimize_nni from the tree after three random NNIs.  Prints
two lines of JSON.  No ratio is fixed here."""
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
oracle = g.load_oracle()
NTAXA = 50
RATES = [1.0, 0.4, 2.3, 0.7]
SHAPES = [(4, 4, pr.SEQ_DNA, 20000), (4, 1, pr.SEQ_DNA, 5000), (20, 4, pr.SEQ_PROTEIN, 5000), (2, 2, pr.SEQ_BINARY, 2000)]
SCRATCH = 1 << 40


def member(nwk, d):
    t = pkg.PhyloTree(pr.scale_newick(nwk, d["rate"]))
    t.set_mem_mode(pkg.LM_ALL_BRANCH)
    t.set_alignment(d["n"], d["seq_type"], d["pat"], d["freq"], d["invar"])
    t.set_model(d["model"])
    t.set_likelihood_kernel(pkg.LK_EIGEN_HIP)
    t.attach_engine(0)
    t.compute_likelihood()
    t.compute_all_partial_lh()
    return t


def candidate_ops(t0, a, b, key0, scale):
    """a's first subtree and b's first change places: the two node updates, lengths times `scale`"""
    def side(frm, to):
        if len(t0.neighbors(to)) == 1:   # a leaf
            return 0, to
        return t0.neighbor_info(frm, to)["key"], -1

    s1 = [v for v, _ in t0.neighbors(a) if v != b]
    s2 = [v for v, _ in t0.neighbors(b) if v != a]
    length = {(x, y): l for x in (a, b) for y, l in t0.neighbors(x)}   # member 0 has rate 1: the super tree's lengths
    ops = (pkg.NodeOp * 2)()
    for k, (dst, (fl, tl), (fr, tr)) in enumerate([(key0, (a, s1[0]), (b, s2[1])), (key0 + 1, (b, s2[0]), (a, s1[1]))]):
        (lk, ll), (rk, rl) = side(fl, tl), side(fr, tr)
        ops[k] = pkg.NodeOp(dst, lk, rk, ll, rl, length[(fl, tl)] * scale, length[(fr, tr)] * scale, 0, 0)
    return ops


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    lib = pkg.libiqhip()
    assert RATES[0] == 1.0
    nwk = synth.random_tree_newick(NTAXA, 9, 0.02, 0.2)
    data = [pr.member_data(synth, oracle, nwk, n, c, s, ns, 900 + 10 * k, RATES[k]) for k, (n, c, s, ns) in enumerate(SHAPES)]
    trees = [member(nwk, d) for d in data]
    t0 = trees[0]
    group = pkg.PartitionGroup(trees)
    group.set_rates(RATES)
    lib.iqhip_timing_enable(t0.engine, 1)
    inner = [(a, b) for a in range(t0.num_nodes) for b, _ in t0.neighbors(a)
             if a < b and len(t0.neighbors(a)) == 3 and len(t0.neighbors(b)) == 3]
    guess = {(a, b): dict(t0.neighbors(a))[b] for (a, b) in inner}
    keep = [candidate_ops(t0, a, b, SCRATCH + 2 * k, 1.0) for k, (a, b) in enumerate(inner)]
    tasks = (pkg.BranchTask * len(inner))(*[
        pkg.BranchTask(C.cast(keep[k], C.c_void_p), 2, 100, pkg.key_end(SCRATCH + 2 * k), pkg.key_end(SCRATCH + 2 * k + 1),
                       guess[e], 1e-6, 100.0, 1e-6) for k, e in enumerate(inner)])
    own = [[candidate_ops(t0, a, b, SCRATCH + 4096 + 2 * k, r) for k, (a, b) in enumerate(inner)] for r in RATES]

    def batched():
        res, part = group.optimize_branch_batch(tasks)
        tm = group.timing()
        return [(r["optx"], r["d2l"], r["nsteps"]) for r in res], part, tm

    def one_by_one():
        out, parts, launches = [], [], 0
        for k, e in enumerate(inner):
            for p, t in enumerate(trees):
                assert lib.iqhip_update_partials(t.engine, own[p][k], 2, None) == 0
                key0 = SCRATCH + 4096 + 2 * k
                assert lib.iqhip_compute_theta(t.engine, pkg.key_end(key0), pkg.key_end(key0 + 1)) == 0
            optx, d2l, ns, part = group.newton_branch(guess[e], 1e-6, 100.0, 1e-6, 100)
            launches += group.timing()["launches"]
            out.append((optx, d2l, ns))
            parts.append(part)
        return out, np.array(parts), launches

    b0, s0 = batched(), one_by_one()   # warm-up of both forms
    same = b0[0] == s0[0] and np.array_equal(b0[1], s0[1])
    wall = {"batch": [], "single": []}
    for _ in range(reps):
        t = time.perf_counter()
        b = batched()
        wall["batch"].append(time.perf_counter() - t)
        t = time.perf_counter()
        s = one_by_one()
        wall["single"].append(time.perf_counter() - t)
    evals = [n for _, _, n in b[0]]
    print(json.dumps({
        "taxa": NTAXA, "members": len(trees), "patterns": [int(d["pat"].shape[1]) for d in data], "candidates": len(inner),
        "evaluations_max": max(evals), "evaluations_sum": sum(evals),
        "batch_wall_ms": 1e3 * float(np.median(wall["batch"])), "single_wall_ms": 1e3 * float(np.median(wall["single"])),
        "batch_group_launches": b[2]["launches"], "single_group_launches": s[2],
        "batch_derv_ms": b[2]["derv_ms"], "batch_update_ms": b[2]["update_ms"],
        # host waits: the batch reads the states once per chunk of steps; branch by branch every member's node updates are
        # read back and every solve reads its state at least once
        "single_host_waits_min": len(inner) * (len(trees) + 1),
        "same_bits": bool(same)}))
    group.close()
    for t in trees:
        t.close()
    print(json.dumps(super_tree_evaluation(nwk, data, max(1, reps // 3))))


def super_tree_evaluation(nwk, data, reps):
    """one evaluation of ALL nni5 candidates of the host mirror's super tree: evaluate_nnis5_batch (ten batches of joint
    solves) against nni_for_branch on every internal branch (joint single solves on the swapped trees)"""
    st = pkg.PhyloSuperTree(nwk, data, all_branch=True)
    st.part_rates = RATES
    st.compute_likelihood()
    inner = [(a, b) for a in range(st.num_nodes) for b, _ in st.neighbors(a)
             if a < b and len(st.neighbors(a)) == 3 and len(st.neighbors(b)) == 3]
    batch = st.evaluate_nnis5_batch()   # warm-up
    wall = {"batch": [], "single": []}
    worst = 0.0
    for _ in range(reps):
        c0 = st.counters()
        t = time.perf_counter()
        batch = st.evaluate_nnis5_batch()
        wall["batch"].append(time.perf_counter() - t)
        c1 = st.counters()
        t = time.perf_counter()
        single = [st.nni_for_branch(a, b, nni5=True) for (a, b) in inner]
        wall["single"].append(time.perf_counter() - t)
        c2 = st.counters()
        for k, two in enumerate(single):
            for c in range(2):
                worst = max(worst, abs(batch[2 * k + c]["newloglh"] - two[c][0]) / abs(two[c][0]))
    out = {"what": "all nni5 candidates of the super tree", "candidates": len(batch),
           "batch_wall_ms": 1e3 * float(np.median(wall["batch"])), "single_wall_ms": 1e3 * float(np.median(wall["single"])),
           "batch_group_batches": c1["group_batches"] - c0["group_batches"], "batch_joint_single_solves": c1["group_solves"] - c0["group_solves"],
           "single_joint_single_solves": c2["group_solves"] - c1["group_solves"], "largest_relative_lnl_difference": worst}
    # one optimize_nni from the tree after three random NNIs
    rng = np.random.default_rng(5)
    for _ in range(3):
        a, b = inner[int(rng.integers(len(inner)))]
        if len(st.neighbors(a)) == 3 and len(st.neighbors(b)) == 3 and b in [v for v, _ in st.neighbors(a)]:
            st.do_random_nni(a, b, int(rng.integers(2)), int(rng.integers(2)))
    st.clear_all_partial_lh()
    start = st.compute_likelihood()
    c0 = st.counters()
    t = time.perf_counter()
    lnl, count, steps = st.optimize_nni()
    out.update({"optimize_nni_wall_ms": 1e3 * (time.perf_counter() - t), "optimize_nni_start_lnl": start, "optimize_nni_lnl": lnl,
                "optimize_nni_moves": count, "optimize_nni_steps": steps,
                "optimize_nni_group_batches": st.counters()["group_batches"] - c0["group_batches"],
                "optimize_nni_joint_single_solves": st.counters()["group_solves"] - c0["group_solves"]})
    st.close()
    return out


if __name__ == "__main__":
    main()
