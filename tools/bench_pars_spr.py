#!/usr/bin/env python3
"""Times the parsimony SPR scan (include/iqhip.h "Parsimony SPR scan") and the search on top of it
(PhyloTree.optimize_parsimony_spr) at radius --radius, from the stepwise-addition tree of a simulated alignment:

  scan     one iqhip_pars_spr_scan of every prune point of the tree: device time of its launches (HIP events,
           iqhip_debug_pars_spr_timing, best of --repeat), the steps scored, ns per scored step, and the bytes its lanes load
           -- per step and column the side vector, and the target vector when the step is scored, planes + score word, plus
           the subtree vector once per job; counted from the job list -- over the time, as a fraction of --hbm-tbs.  Most of
           these loads are re-reads of the same few hundred vectors, so the fraction says how far the kernel is from what HBM
           alone could feed, not that HBM is the limit.
  search   optimize_parsimony_spr to convergence: rounds, moves, the score before and after, wall clock and the device time
           of all its scan launches
  host     the numpy restatement (tests/spr_ref.job_scores over fitch_ref) on the first --host-jobs jobs of the same tree:
           wall-clock ns per step, and its scores must equal the device's.  An orientation only: this is NOT the reference's
           SIMD code.  --no-host skips it.

Shapes: `--shapes dna:200x100000,protein:100x20000` (taxa x parsimony-informative sites: columns are simulated until that
many are informative; DNA: GTR+G4, protein / codon: a random reversible 20- / 64-state matrix +G).  One JSON line per shape.  No pass
threshold.  Not the flagship benchmark (bench.py)."""
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


def informative_columns(synth, F, nwk, model, n, want):
    """simulated columns, the first `want` parsimony-informative ones"""
    keep, have, seed = [], 0, 2
    while have < want:
        st = synth.simulate_alignment(nwk, model, max(1000, int(1.3 * (want - have))), seed)
        st = st[:, F.is_informative(st, n) != 0]
        keep.append(st)
        have += st.shape[1]
        seed += 1
    return np.ascontiguousarray(np.concatenate(keep, axis=1)[:, :want])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="dna:200x100000,protein:100x20000")
    ap.add_argument("--radius", type=int, default=6)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--hbm-tbs", type=float, default=8.0, help="HBM peak in TB/s the load rate is compared with")
    ap.add_argument("--host-jobs", type=int, default=2)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--no-search", action="store_true")
    a = ap.parse_args()
    pkg = entry.load_package()
    synth = __import__("importlib").import_module("iqtree_amd.synth")
    import fitch_ref as F
    import spr_ref as S
    lib = pkg.libiqhip()
    for spec in a.shapes.split(","):
        kind, shape = spec.split(":")
        ntaxa, nsite = (int(x) for x in shape.split("x"))
        if kind == "dna":
            model, n, seq_type = synth.gtr_model(alpha=0.9, ncat=4), 4, 0
        elif kind == "protein":
            model, n, seq_type = synth.random_reversible_model(20, 7, alpha=0.9, ncat=4), 20, 1
        else:
            model, n, seq_type = synth.random_reversible_model(64, 7, alpha=0.9, ncat=2), 64, 2
        nwk = synth.random_tree_newick(ntaxa, 1)
        states = informative_columns(synth, F, nwk, model, n, nsite)
        t = pkg.PhyloTree(nwk)
        t.set_alignment(n, seq_type, states, np.ones(nsite))
        t.set_model(model)
        t.attach_engine(0)
        order = [int(x) for x in np.random.default_rng(3).permutation(ntaxa)]
        start_score = t.compute_parsimony_tree(order)
        assert t.pars_nsites == nsite
        nwords = t.pars_shape()[1]
        # ---- one scan
        t.compute_all_partial_pars()
        jobs, steps, moves = t.collect_spr_jobs(a.radius)
        scores, best_step, best_score, best_job = t.pars_spr_scan(jobs, steps)     # warm-up: allocations, first launch
        lib.iqhip_timing_enable(t.engine, 1)
        scan_ms = []
        for _ in range(a.repeat):
            t.pars_spr_timing(reset=True)
            again = t.pars_spr_scan(jobs, steps, want_scores=False)
            tm = t.pars_spr_timing()
            assert again[3] == best_job and tm["launches"] == 3
            scan_ms.append(tm["scan_ms"])
        nscored = int((steps[:, 3] == 0).sum())
        assert tm["steps_scored"] == nscored
        loaded = 4.0 * nwords * (n + 1) * (len(steps) + nscored + len(jobs))
        ms = min(scan_ms)
        row = {
            "shape": spec, "nstates": n, "radius": a.radius, "informative_sites": nsite, "nwords": nwords, "jobs": len(jobs),
            "steps": len(steps), "steps_scored": nscored, "scan_launches": 3, "scan_device_ms": ms,
            "ns_per_scored_step": 1e6 * ms / nscored, "bytes_loaded": loaded, "bytes_loaded_per_step": loaded / len(steps),
            "load_rate_tbs": loaded / (ms * 1e-3) / 1e12, "load_rate_vs_hbm_peak": loaded / (ms * 1e-3) / 1e12 / a.hbm_tbs,
            "upload_bytes": 16 * (len(jobs) + len(steps)), "readback_bytes_scores": 4 * (len(steps) + 2 * len(jobs) + 1),
        }
        # ---- the numpy restatement on the first jobs of the same tree
        if not a.no_host:
            adj = S.mirror_adjacency(t)
            tips = F.tip_vectors(states, np.arange(nsite), n)
            dv = F.directed_vectors(adj, tips)
            want = S.collect_jobs(adj, ntaxa, a.radius)[:a.host_jobs]
            t0 = time.perf_counter()
            hs = [S.job_scores(job, dv) for job in want]
            host = time.perf_counter() - t0
            nh = sum(len(x) for x in hs)
            for job_row, sc in zip(jobs, hs):
                got = scores[job_row[1]:job_row[1] + job_row[2]].tolist()
                assert got == [-1 if v is None else v for v in sc]
            row.update(host_steps=nh, host_ns_per_step=1e9 * host / nh)
        # ---- the search
        if not a.no_search:
            t.pars_spr_timing(reset=True)
            t0 = time.perf_counter()
            final, rounds = t.optimize_parsimony_spr(a.radius, trace=True)
            wall = time.perf_counter() - t0
            tm = t.pars_spr_timing()
            assert final == t.compute_parsimony() and rounds[0]["score_before"] == start_score
            row.update(score_start=start_score, score_final=final, rounds=len(rounds),
                       moves=sum(r["applied"] for r in rounds), search_wall_s=wall, search_scan_device_ms=tm["scan_ms"],
                       search_scan_launches=tm["launches"])
        lib.iqhip_timing_enable(t.engine, 0)
        print(json.dumps(row), flush=True)
        t.close()


if __name__ == "__main__":
    main()
