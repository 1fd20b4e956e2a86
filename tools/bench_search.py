#!/usr/bin/env python3
"""Measures the NNI tree search (iq-tree_amd/host/tree_search_host.h) on one GPU: a DNA alignment of 50 taxa x 100 000
patterns under GTR+G4 (synth.make_workload), starting ten random NNIs away from the tree the data were simulated on.

  * one optimize_nni with the restricted branch lists (speed), with every branch in every step, and with the
    branch-by-branch evaluator (batched=False): wall time, engine submissions per NNI step, candidates evaluated per step
  * one search of 10 iterations: wall time, engine submissions

Prints one JSON line.  No ratio is promised; DESIGN.md section 3.16 records what a run gave, with its date.

    python tools/bench_search.py [--taxa 50] [--patterns 100000] [--iterations 10] [--seed 1] [--device 0]
"""
import argparse
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--taxa", type=int, default=50)
    ap.add_argument("--patterns", type=int, default=100000)
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    pkg = load_package()
    synth = importlib.import_module("iqtree_amd.synth")
    model = synth.gtr_model(alpha=0.9, ncat=4)
    nwk, pat, freq = synth.make_workload(args.taxa, args.patterns, model, seed=args.seed)

    def attach(newick):
        t = pkg.PhyloTree(newick)
        t.set_mem_mode(pkg.LM_ALL_BRANCH)
        t.set_alignment(4, pkg.SEQ_DNA, pat, freq)
        t.set_model(model)
        t.set_likelihood_kernel(pkg.LK_EIGEN_HIP)
        t.attach_engine(args.device)
        return t

    t = attach(nwk)
    true_lnl = t.compute_likelihood()
    pkg.TreeSearch(t, seed=args.seed).do_random_nnis(10, 1)
    t.compute_likelihood()
    t.optimize_all_branches()
    start = t.tree_string()

    def one_optimize_nni(**kw):
        tr = attach(start)
        tr.compute_likelihood()                               # engine warm: inputs uploaded, kernels loaded
        tr.clear_all_partial_lh()
        t0 = time.perf_counter()
        lnl, count, steps, trace = tr.optimize_nni(trace=True, **kw)
        sec = time.perf_counter() - t0
        return dict(seconds=round(sec, 4), lnl=lnl, nnis=count, steps=steps,
                    submissions_per_step=[s["submissions"] for s in trace],
                    candidates_per_step=[len(s["evaluated"]) for s in trace])

    res = dict(shape=dict(taxa=args.taxa, patterns=int(pat.shape[1]), model="GTR+G4"), true_tree_lnl=true_lnl,
               optimize_nni_speed=one_optimize_nni(), optimize_nni_allnni=one_optimize_nni(speed=False),
               optimize_nni_unbatched=one_optimize_nni(batched=False))
    ts_tree = attach(start)
    ts_tree.compute_likelihood()
    n0 = ts_tree.num_submissions
    t0 = time.perf_counter()
    best = pkg.TreeSearch(ts_tree, seed=args.seed, iterations=args.iterations).search()
    res["search"] = dict(iterations=args.iterations, seconds=round(time.perf_counter() - t0, 4), best_lnl=best,
                         submissions=ts_tree.num_submissions - n0)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
