#!/usr/bin/env python3
"""Times one PhyloTree.compute_parsimony_tree -- stepwise addition by Fitch parsimony on the device (include/iqhip.h
"Fitch parsimony") -- for a few alignments:

  device   the whole call (wall clock, best of --repeat; tree surgery, validation, uploads, read-backs and the final
           fix_negative_branch included) and, from a further run with iqhip_timing_enable, the device time of its update
           launches and of its scan launches (HIP events, iqhip_debug_pars_timing), with the launches per step
  host     the numpy restatement of tests/fitch_ref.py doing the same steps (fitch_ref.stepwise_addition: per step it
           recomputes the vectors the last insertion invalidated, scores every branch and takes the first minimum, and at
           the end counts the substitutions of every branch as fix_negative_branch does), wall clock of one run; its score
           and branch count must equal the device's, its update count is printed next to the device's.  --no-host skips it.  An
           orientation only: this is NOT the reference's SIMD code.

Shapes: `--shapes dna:200x2000,dna:1000x10000,dna:2000x1000,protein:200x2000` (taxa x sites; DNA: GTR+G4, protein: a
random reversible 20-state matrix +G4; columns of a simulated alignment as patterns, frequency 1).  Prints one JSON line per
shape.  No pass threshold.  Not the flagship benchmark (bench.py)."""
import argparse
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
    ap.add_argument("--shapes", default="dna:200x2000,dna:1000x10000,dna:2000x1000,protein:200x2000")
    ap.add_argument("--repeat", type=int, default=2)
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    pkg = entry.load_package()
    synth = __import__("importlib").import_module("iqtree_amd.synth")
    import fitch_ref as F
    lib = pkg.libiqhip()
    for spec in a.shapes.split(","):
        kind, shape = spec.split(":")
        ntaxa, nsite = (int(x) for x in shape.split("x"))
        if kind == "dna":
            model, n, seq_type = synth.gtr_model(alpha=0.9, ncat=4), 4, 0
        else:
            model, n, seq_type = synth.random_reversible_model(20, 7, alpha=0.9, ncat=4), 20, 1
        nwk = synth.random_tree_newick(ntaxa, 1)
        states = synth.simulate_alignment(nwk, model, nsite, 2)
        t = pkg.PhyloTree(nwk)
        t.set_alignment(n, seq_type, states, np.ones(nsite))
        t.set_model(model)
        t.attach_engine(0)
        order = [int(x) for x in np.random.default_rng(3).permutation(ntaxa)]
        score = t.compute_parsimony_tree(order)                   # warm-up: allocations, first launches
        wall = []
        for _ in range(a.repeat):
            t0 = time.perf_counter()
            assert t.compute_parsimony_tree(order) == score
            wall.append(time.perf_counter() - t0)
        lib.iqhip_timing_enable(t.engine, 1)
        t.pars_timing(reset=True)
        t.compute_parsimony_tree(order)
        tm = t.pars_timing()
        lib.iqhip_timing_enable(t.engine, 0)
        nwords = t.pars_shape()[1]
        host = None
        if not a.no_host:
            inf = F.is_informative(states, n)
            tips = F.tip_vectors(states, F.site_patterns(np.ones(nsite), inf), n)
            t0 = time.perf_counter()
            hscore, _, hupd, hscan = F.stepwise_addition(tips, order)
            host = time.perf_counter() - t0
            assert (hscore, hscan) == (score, tm["branches"]), (hscore, hscan, score, tm)
        steps = max(1, ntaxa - 3)
        print(json.dumps({
            "shape": spec, "nstates": n, "informative_sites": t.pars_nsites, "nwords": nwords, "score": score,
            "device_wall_s": min(wall),
            "device_update_ms": tm["update_ms"], "device_scan_ms": tm["scan_ms"],
            "update_launches_per_step": tm["update_launches"] / steps, "scan_launches_per_step": tm["scan_launches"] / steps,
            "ops": tm["ops"], "branches_scanned": tm["branches"],
            "host_same_steps_s": host, "host_updates": None if host is None else hupd,
        }), flush=True)
        t.close()


if __name__ == "__main__":
    main()
