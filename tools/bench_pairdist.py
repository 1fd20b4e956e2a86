#!/usr/bin/env python3
"""Times iqhip_pair_distances (include/iqhip.h "pairwise maximum-likelihood distances") for a few alignments:

  device   the whole call (wall clock, best of --repeat) and, with iqhip_timing_enable, the device time of its count
           launches and of its solve launches (HIP events, iqhip_debug_pair_timing)
  host     the same matrix as the numpy restatement of tests/test_pair_dist_host.py computes it, one pair at a time, on
           --host-pairs pairs and scaled linearly to all pairs.  An orientation only: this is NOT the reference's
           OpenMP code.

Shapes: `--shapes dna:200x10000,dna:1000x10000,protein:200x5000` (DNA: GTR+G4, protein: a random reversible 20-state
matrix +G4; columns of a simulated alignment as patterns, frequency 1).  Prints one JSON line per shape.  Not the flagship
benchmark (bench.py)."""
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
    ap.add_argument("--shapes", default="dna:200x10000,dna:1000x10000,protein:200x5000")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--host-pairs", type=int, default=100)
    a = ap.parse_args()
    pkg = entry.load_package()
    synth = __import__("importlib").import_module("iqtree_amd.synth")
    import test_pair_dist_host as H
    lib = pkg.libiqhip()
    for spec in a.shapes.split(","):
        kind, shape = spec.split(":")
        ntaxa, nptn = (int(x) for x in shape.split("x"))
        if kind == "dna":
            model, n, seq_type = synth.gtr_model(alpha=0.9, ncat=4), 4, 0
        else:
            model, n, seq_type = synth.random_reversible_model(20, 7, alpha=0.9, ncat=4), 20, 1
        nwk = synth.random_tree_newick(ntaxa, 1)
        states = synth.simulate_alignment(nwk, model, nptn, 2)
        freq = np.ones(nptn)
        t = pkg.PhyloTree(nwk)
        t.set_alignment(n, seq_type, states, freq)
        t.set_model(model)
        t.attach_engine(0)
        dist = t.compute_dist()                                   # warm-up: allocations, first launches
        wall = []
        for _ in range(a.repeat):
            t0 = time.perf_counter()
            t.compute_dist()
            wall.append(time.perf_counter() - t0)
        lib.iqhip_timing_enable(t.engine, 1)
        t.compute_dist()
        cms, sms = C.c_double(), C.c_double()
        assert lib.iqhip_debug_pair_timing(t.engine, C.byref(cms), C.byref(sms)) == 0
        lib.iqhip_timing_enable(t.engine, 0)
        pairs = H.all_pairs(ntaxa)
        rng = np.random.default_rng(3)
        sample = [pairs[k] for k in rng.choice(len(pairs), size=min(a.host_pairs, len(pairs)), replace=False)]
        t0 = time.perf_counter()
        worst = 0.0
        for (i, j) in sample:
            cnt = H.restate_counts(states, freq, n, [(i, j)])[0]
            worst = max(worst, abs(H.restate_solve(cnt, model)[0] - dist[i, j]))
        host = (time.perf_counter() - t0) / len(sample) * len(pairs)
        print(json.dumps(dict(kind=kind, ntaxa=ntaxa, nptn=nptn, npairs=len(pairs), wall_s=min(wall), counts_ms=cms.value,
                              solve_ms=sms.value, host_restatement_s_scaled=host, host_pairs=len(sample),
                              max_abs_diff_on_host_pairs=worst)))
        t.close()


if __name__ == "__main__":
    main()
