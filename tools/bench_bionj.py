"""BIONJ on the device (iqhip_bionj) next to the vectorised numpy restatement of tests/bionj_ref.py, run by hand:
    python tools/bench_bionj.py [n ...]          (default 500 2000 8000)
Per n: a symmetrised uniform-random matrix; the device time of the whole enqueued merge loop (HIP events,
iqhip_debug_bionj_timing), the wall time of the call (uploads, 3 n^2 allocations, the log's read-back), launches per step,
and the restatement's wall time where an estimate from the previous size (cubic growth) stays under a minute.  One JSON
line per n."""
import importlib, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as g
import bionj_ref as br
pkg = g.load_package(); synth = importlib.import_module("iqtree_amd.synth")
sizes = [int(x) for x in sys.argv[1:]] or [500, 2000, 8000]
model = synth.gtr_model()
nwk, pat, freq = synth.make_workload(8, 200, model, seed=1)
t = pkg.PhyloTree(nwk); t.set_alignment(4, pkg.SEQ_DNA, pat, freq); t.set_model(model); t.attach_engine(0)
lib = pkg.libiqhip()
lib.iqhip_timing_enable(t.engine, 1)
t.bionj(br.uniform_matrix(64, 1))   # (first launches of the kernels: code upload)
prev = None   # (n, seconds) of the last restatement run
for n in sizes:
    rng = np.random.default_rng(n)
    A = rng.uniform(0.05, 1.0, (n, n))
    D = (A + A.T) / 2
    np.fill_diagonal(D, 0.0)
    reps = []
    for _ in range(2):
        t0 = time.perf_counter(); steps, last, last_len = t.bionj(D); wall = time.perf_counter() - t0
        ms, launches = t.bionj_timing()
        reps.append((ms, wall))
    ms, wall = min(reps)
    out = dict(n=n, device_ms=round(ms, 3), call_wall_ms=round(wall * 1e3, 3), launches=launches,
               launches_per_step=round(launches / max(1, n - 3), 3), us_per_step=round(ms * 1e3 / max(1, n - 3), 3),
               runs=[round(r[0], 3) for r in reps])
    est = None if prev is None else prev[1] * (n / prev[0]) ** 3
    if est is None or est < 60.0:
        t0 = time.perf_counter(); want = br.bionj(D); sec = time.perf_counter() - t0
        prev = (n, sec)
        out["numpy_ms"] = round(sec * 1e3, 1)
        out["same_pairs"] = [(int(s["a"]), int(s["b"])) for s in steps] == [s[:2] for s in want["steps"]]
        out["max_abs_diff"] = float(max(max(abs(s["la"] - w[2]), abs(s["lb"] - w[3]), abs(s["lambda"] - w[4]))
                                        for s, w in zip(steps, want["steps"])))
    else:
        out["numpy_ms"] = None
        out["numpy_estimate_s"] = round(est, 1)
    print(json.dumps(out), flush=True)
t.close()
