#!/usr/bin/env python3
"""Times likelihood mapping (include/iqhip.h "Likelihood mapping") on two DNA GTR+G4 shapes, 10 000 drawn quartets each:

  device   PhyloTree.quartet_likelihoods: the whole call (wall clock, best of --repeat) and, with iqhip_timing_enable, the
           device time of its cell launches and of its solve launches (HIP events, iqhip_debug_quartet_timing); quartets/s
           from the wall clock; mean work items (non-zero cells + other patterns) and derivative evaluations per quartet tree
  route    the route there was before: per quartet tree a 4-taxon PhyloTree over the host-compressed sub-alignment,
           fix_negative_branch and optimize_all_branches(10, 0.1) on the traversal kernels, timed on --route-quartets
           quartets of the same draw (`route_s_per_quartet` with, `route_compute_s_per_quartet` without the compression and the
           engine set-up) and compared with the device's logl

Shapes: `--shapes 100x10000,50x100000` (taxa x patterns of synth.make_workload).  Prints one JSON line per shape.  Not the
flagship benchmark (bench.py)."""
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
    ap.add_argument("--shapes", default="100x10000,50x100000")
    ap.add_argument("--quartets", type=int, default=10000)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--route-quartets", type=int, default=20)
    a = ap.parse_args()
    pkg = entry.load_package()
    synth = __import__("importlib").import_module("iqtree_amd.synth")
    import lmap_ref
    lib = pkg.libiqhip()
    model = synth.gtr_model(alpha=0.9, ncat=4)
    for shape in a.shapes.split(","):
        ntaxa, nptn = (int(x) for x in shape.split("x"))
        nwk, states, freq = synth.make_workload(ntaxa, nptn, model, seed=5)
        t = pkg.PhyloTree(nwk)
        t.set_alignment(4, 0, states, freq)
        t.set_model(model)
        t.attach_engine(0)
        quartets = pkg.draw_quartets(ntaxa, a.quartets, 1)
        res = t.quartet_likelihoods(quartets)                      # warm-up: allocations, first launches
        wall = []
        for _ in range(a.repeat):
            t0 = time.perf_counter()
            t.quartet_likelihoods(quartets)
            wall.append(time.perf_counter() - t0)
        lib.iqhip_timing_enable(t.engine, 1)
        t.quartet_likelihoods(quartets)
        cells_ms, solve_ms = t.quartet_timing()
        lib.iqhip_timing_enable(t.engine, 0)
        cells, nother = t.quartet_cells(quartets)
        items = np.count_nonzero(cells.reshape(len(quartets), 256), axis=1) + nother
        t.close()
        nroute = min(a.route_quartets, len(quartets))
        whole = compute = 0.0
        worst = 0.0
        for qi in range(nroute):
            for k in range(3):
                t0 = time.perf_counter()
                taxa = [quartets[qi][lmap_ref.QC[4 * k + j]] for j in range(4)]
                cols, w = lmap_ref.sub_alignment(states, freq, taxa)
                old = pkg.PhyloTree("(0:0.1,1:0.1,(2:0.1,3:0.1):0.1);")
                old.set_alignment(4, 0, cols, w)
                old.set_model(model)
                old.set_likelihood_kernel(pkg.LK_EIGEN_HIP)
                old.attach_engine(0)
                t1 = time.perf_counter()
                old.fix_negative_branch()
                old.initialize_all_partial_lh()
                old.clear_all_partial_lh()
                lnl = old.optimize_all_branches(10, 0.1)
                t2 = time.perf_counter()
                old.close()
                whole += time.perf_counter() - t0
                compute += t2 - t1
                worst = max(worst, abs(lnl - res["logl"][qi, k]) / abs(lnl))
        print(json.dumps(dict(ntaxa=ntaxa, nptn=nptn, nquartets=len(quartets), wall_s=min(wall), cells_ms=cells_ms, solve_ms=solve_ms,
                              quartets_per_s=len(quartets) / min(wall), mean_items=float(items.mean()),
                              mean_evals_per_tree=float(res["neval"].mean()), mean_sweeps_per_tree=float(res["nsweeps"].mean()),
                              route_quartets=nroute, route_s_per_quartet=whole / nroute, route_compute_s_per_quartet=compute / nroute,
                              speedup_vs_route=whole / nroute * len(quartets) / min(wall),
                              speedup_vs_route_compute=compute / nroute * len(quartets) / min(wall),
                              max_rel_logl_diff_on_route_quartets=worst)), flush=True)


if __name__ == "__main__":
    main()
