#!/usr/bin/env python3
"""Times iqhip_partition_pair_distances (include/iqhip.h "Joint pairwise distances of a partition group") on a group of
DNA members (GTR+G4, columns of a simulated alignment as patterns, frequency 1), all rates 1:

  group    the whole call (wall clock, best of --repeat); with iqhip_timing_enable on member 0 the device time of the
           members' count launches (summed over the members, which run side by side) and of the solve launches
           (iqhip_debug_partition_pair_timing); derivative evaluations per solved pair; the kernels the call enqueued
  plain    one iqhip_pair_distances per member, one after the other: a COST yardstick -- P solves of one member each, not
           the same result
  host     the numpy restatement of tests/partition_dist_ref.py on --host-pairs pairs, scaled linearly to all pairs.  An
           orientation only: this is NOT the reference's OpenMP code.

`--members 4 --ntaxa 100 --nptn 2500`.  Prints one JSON line.  Not the flagship benchmark (bench.py)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as entry  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=4)
    ap.add_argument("--ntaxa", type=int, default=100)
    ap.add_argument("--nptn", type=int, default=2500)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--host-pairs", type=int, default=50)
    a = ap.parse_args()
    pkg = entry.load_package()
    synth = __import__("importlib").import_module("iqtree_amd.synth")
    import partition_dist_ref as R
    import test_pair_dist_host as H
    lib = pkg.libiqhip()
    nwk = synth.random_tree_newick(a.ntaxa, 1)
    members, trees = [], []
    for p in range(a.members):
        model = synth.gtr_model(alpha=0.5 + 0.2 * p, ncat=4)
        states = synth.simulate_alignment(nwk, model, a.nptn, 2 + p)
        members.append(dict(n=4, seq_type=0, pat=np.ascontiguousarray(states, dtype=np.uint8), freq=np.ones(a.nptn), model=model))
        t = pkg.PhyloTree(nwk)
        t.set_alignment(4, 0, states, members[-1]["freq"])
        t.set_model(model)
        t.attach_engine(0)
        trees.append(t)
    g = pkg.PartitionGroup(trees)
    dist, _, nst = g.pair_distances()                             # warm-up: allocations, first launches
    wall = []
    for _ in range(a.repeat):
        t0 = time.perf_counter()
        g.pair_distances()
        wall.append(time.perf_counter() - t0)
    lib.iqhip_timing_enable(trees[0].engine, 1)
    g.pair_distances()
    counts_ms, solve_ms = g.pair_timing()
    launches = g.timing()["launches"]
    lib.iqhip_timing_enable(trees[0].engine, 0)
    # the yardstick: every member's own matrix
    plain_wall, plain_counts, plain_solve = [], 0.0, 0.0
    for t in trees:
        t.compute_dist()
    for _ in range(a.repeat):
        t0 = time.perf_counter()
        for t in trees:
            t.compute_dist()
        plain_wall.append(time.perf_counter() - t0)
    for t in trees:
        lib.iqhip_timing_enable(t.engine, 1)
        t.compute_dist()
        cms, sms = C.c_double(), C.c_double()
        assert lib.iqhip_debug_pair_timing(t.engine, C.byref(cms), C.byref(sms)) == 0
        lib.iqhip_timing_enable(t.engine, 0)
        plain_counts += cms.value
        plain_solve += sms.value
    pairs = H.all_pairs(a.ntaxa)
    rng = np.random.default_rng(3)
    sample = [pairs[k] for k in rng.choice(len(pairs), size=min(a.host_pairs, len(pairs)), replace=False)]
    models, rates = [m["model"] for m in members], np.ones(a.members)
    t0 = time.perf_counter()
    worst = 0.0
    for (i, j) in sample:
        cnt = [c[0] for c in R.member_counts(members, [(i, j)])]
        worst = max(worst, abs(R.restate_joint_solve(cnt, models, rates)[0] - dist[i, j]))
    host = (time.perf_counter() - t0) / len(sample) * len(pairs)
    solved = nst[np.triu_indices(a.ntaxa, 1)]
    print(json.dumps(dict(members=a.members, ntaxa=a.ntaxa, nptn=a.nptn, npairs=len(pairs), wall_s=min(wall), counts_ms=counts_ms,
                          solve_ms=solve_ms, launches=launches, solved_pairs=int((solved > 0).sum()),
                          evals_per_solved_pair=float(solved[solved > 0].mean()) if (solved > 0).any() else 0.0,
                          plain_wall_s=min(plain_wall), plain_counts_ms=plain_counts, plain_solve_ms=plain_solve,
                          host_restatement_s_scaled=host, host_pairs=len(sample), max_abs_diff_on_host_pairs=worst)))
    g.close()
    for t in trees:
        t.close()


if __name__ == "__main__":
    main()
