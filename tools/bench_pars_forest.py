#!/usr/bin/env python3
"""Times a forest of K stepwise-addition parsimony trees built in lockstep (PhyloTree.compute_parsimony_forest,
iq-tree_amd/host/pars_forest_host.h) next to the same K addition orders through compute_parsimony_tree one after the other,
on the same commit and the same engine:

  forest     per route of the batch scan (IQHIP_PARS_BATCH_ROUTE unset = the engine's choice from nwords, wave, wg): the
             whole call (wall clock, best of --repeat) and, from a further run with iqhip_timing_enable, the device time of the
             batch scans (iqhip_debug_pars_batch_timing) and of the updates (iqhip_debug_pars_timing), the kernel launches,
             the engine calls that end in a host read (batch scans + branch-scores calls) and the arena chunks
  one by one the K trees through compute_parsimony_tree: wall clock, device time of its updates and scans, launches, host
             reads (one scan per step and one branch-scores call per tree); every score and Newick string must equal the
             forest's

Shapes: `--shapes dna:50x100000,dna:44x355` (taxa x sites; GTR+G4, columns of a simulated alignment as patterns).  Prints
one JSON line per shape and route.  No ratio is promised and none is a pass condition; the threshold between the two routes
(kParsBatchWaveWords) can be moved from what this prints.  Not the flagship benchmark (bench.py)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="dna:50x100000,dna:44x355")
    ap.add_argument("--trees", type=int, default=100)
    ap.add_argument("--repeat", type=int, default=2)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    pkg = entry.load_package()
    synth = __import__("importlib").import_module("iqtree_amd.synth")
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
        orders = pkg.parsimony_orders(a.seed, a.trees, ntaxa)
        steps = max(1, ntaxa - 3)

        # the K trees one after the other
        single = []
        t.compute_parsimony_tree(orders[0])                       # warm-up: allocations, first launches
        t0 = time.perf_counter()
        for o in orders:
            single.append((t.compute_parsimony_tree(o), t.tree_string()))
        single_wall = time.perf_counter() - t0
        lib.iqhip_timing_enable(t.engine, 1)
        t.pars_timing(reset=True)
        for o in orders:
            t.compute_parsimony_tree(o)
        st = t.pars_timing()
        lib.iqhip_timing_enable(t.engine, 0)
        nwords = t.pars_shape()[1]
        base = {"shape": spec, "trees": a.trees, "nstates": n, "informative_sites": t.pars_nsites, "nwords": nwords}
        print(json.dumps(dict(base, path="one_by_one", wall_s=single_wall, device_update_ms=st["update_ms"],
                              device_scan_ms=st["scan_ms"], launches=st["update_launches"] + st["scan_launches"] + a.trees,
                              host_reads=a.trees * (steps + 1))), flush=True)

        for route in (None, "wave", "wg"):
            if route is None:
                os.environ.pop("IQHIP_PARS_BATCH_ROUTE", None)
            else:
                os.environ["IQHIP_PARS_BATCH_ROUTE"] = route
            forest = t.compute_parsimony_forest(orders)           # warm-up; and the results must be the one-tree path's
            assert [(m["score"], m["newick"]) for m in forest] == single, "the forest and the one-tree path disagree"
            wall = []
            for _ in range(a.repeat):
                t0 = time.perf_counter()
                t.compute_parsimony_forest(orders)
                wall.append(time.perf_counter() - t0)
            lib.iqhip_timing_enable(t.engine, 1)
            t.pars_timing(reset=True)
            t.pars_batch_timing(reset=True)
            t.compute_parsimony_forest(orders)
            ft, bt, fc = t.pars_timing(), t.pars_batch_timing(), t.forest_calls
            lib.iqhip_timing_enable(t.engine, 0)
            chosen = route or ("wave" if nwords <= 256 else "wg")
            print(json.dumps(dict(base, path="forest", route=route or "default", route_run=chosen, wall_s=min(wall),
                                  device_scan_ms=bt["scan_ms"], device_update_ms=ft["update_ms"],
                                  launches=bt["launches"] + ft["update_launches"] + fc["branch_scores"],
                                  host_reads=fc["scans"] + fc["branch_scores"], chunks=fc["inits"],
                                  branches_scanned=bt["branches"], segments=bt["segments"])), flush=True)
        os.environ.pop("IQHIP_PARS_BATCH_ROUTE", None)
        t.close()


if __name__ == "__main__":
    main()
