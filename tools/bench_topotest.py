#!/usr/bin/env python3
"""Times the tree topology tests on the device (include/iqhip.h "tree topology tests") against the route a caller had
before them, for one engine: `--rows` store rows x `--nptn` DNA patterns.

  device   iqhip_multiscale_bp over `--scales` scales x `--reps` replicates (resamples drawn, multiplied and counted on
           the device), and iqhip_gen_boot_samples + iqhip_tree_tests (weighted) on `--reps` replicates
  host     ONE scale of the older route: MT19937 multinomial resamples on the host, iqhip_set_boot_samples,
           iqhip_ptnlh_rell, arg-max in numpy -- on `--host-reps` replicates (the float sample matrix of 10 000 x 100 000
           is 4 GB on the host), scaled linearly to `--reps`

Prints one JSON line.  Not the flagship benchmark (bench.py)."""
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
    ap.add_argument("--rows", type=int, default=100)
    ap.add_argument("--nptn", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=10000)
    ap.add_argument("--scales", type=int, default=10)
    ap.add_argument("--host-reps", type=int, default=1000)
    ap.add_argument("--repeat", type=int, default=3)
    a = ap.parse_args()
    pkg = entry.load_package()
    synth = __import__("importlib").import_module("iqtree_amd.synth")
    rng = np.random.default_rng(1)
    freq = rng.integers(1, 4, size=a.nptn).astype(np.float64)
    nsite = int(freq.sum())
    t = pkg.PhyloTree("(0:0.1,1:0.2,2:0.3);")
    t.set_alignment(4, pkg.SEQ_DNA, rng.integers(0, 4, size=(3, a.nptn)).astype(np.uint8), freq)
    t.set_model(synth.gtr_model(alpha=0.9, ncat=4))
    t.attach_engine(0)
    t.ptnlh_reserve(a.rows)
    base = rng.uniform(-12.0, -1.0, size=a.nptn)
    for r in range(a.rows):
        off = 0.05 * rng.uniform(-1.0, 1.0, size=a.nptn)
        t.ptnlh_upload(r, base + off - (off @ freq) / nsite)
    rows = np.arange(a.rows)
    lh = np.array([t.ptnlh_fetch(r) @ freq for r in range(a.rows)])
    scales = np.linspace(0.5, 0.5 + 0.1 * (a.scales - 1), a.scales)

    def best(fn):
        fn()                                                     # warm-up: allocations, first launches
        times = []
        for _ in range(a.repeat):
            t0 = time.perf_counter()
            fn()
            times.append(time.perf_counter() - t0)
        return min(times)

    out = dict(rows=a.rows, nptn=a.nptn, reps=a.reps, scales=a.scales, nsite=nsite)
    out["multiscale_bp_s"] = best(lambda: t.multiscale_bp(rows, scales, a.reps, 7))
    out["gen_boot_samples_s"] = best(lambda: t.gen_boot_samples(a.reps, nsite, 7))
    out["tree_tests_weighted_s"] = best(lambda: t.tree_tests(rows, lh, a.reps, weighted=True, tie_seed=7))
    out["tree_tests_s"] = best(lambda: t.tree_tests(rows, lh, a.reps, tie_seed=7))
    out["diff_variance_s"] = best(lambda: t.ptnlh_diff_variance(rows))

    host = np.random.Generator(np.random.MT19937(7))
    p = freq / nsite

    def host_route():
        W = host.multinomial(nsite, p, size=a.host_reps).astype(np.float32)
        t.set_boot_samples(W)
        R = t.ptnlh_rell(rows, a.host_reps)
        return np.bincount(np.argmax(R, axis=0), minlength=a.rows) / a.host_reps

    t0 = time.perf_counter()
    host_route()
    one = time.perf_counter() - t0
    out["host_route_one_scale_s_at_host_reps"] = one
    out["host_reps"] = a.host_reps
    out["host_route_one_scale_s_scaled"] = one * a.reps / a.host_reps
    out["ratio_host_all_scales_over_multiscale_bp"] = out["host_route_one_scale_s_scaled"] * a.scales / out["multiscale_bp_s"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
