"""EM estimation of +R free-rate models on the device (iqhip_em_posteriors / iqhip_em_objective, PhyloTree::optimizeFreeRatesEM):
device time of one E-step and of one objective call, time of one traversal, lockstep rounds per EM step against the sum of the
Brent evaluations (what the reference's one-category-at-a-time loop spends in traversals), and next to them the host
route that existed before these kernels for the same quantities: compute_pattern_lh_cat() to the host plus numpy.
    python tools/bench_em.py [dna|protein|all]      DNA 50 taxa x 100 k patterns +R4, protein 50 x 20 k +R4
Prints one line of JSON per workload.  No threshold is fixed here."""
import copy
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g  # noqa: E402

pkg = g.load_package()
import importlib  # noqa: E402

synth = importlib.import_module("iqtree_amd.synth")
WORKLOADS = {"dna": (4, 0, 50, 100000), "protein": (20, 1, 50, 20000)}


def median_ms(fn, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out))


def run(name):
    n, seq_type, ntaxa, P = WORKLOADS[name]
    base = synth.gtr_model(alpha=0.7, ncat=4) if n == 4 else synth.random_reversible_model(n, 11, alpha=0.7, ncat=4)
    true = copy.copy(base)
    true.props = np.array([0.4, 0.3, 0.2, 0.1])
    true.rates = np.array([0.1, 0.6, 1.6, 4.6])
    nwk = synth.random_tree_newick(ntaxa, 5, 0.02, 0.2)
    # distinct random columns stand in for patterns (as bench.py's workloads do); enough sites that P patterns remain
    st = synth.simulate_alignment(nwk, true, int(P * (1.6 if n == 4 else 1.3)) + 64, 3)
    pat, freq = synth.compress_patterns(st)
    pat, freq = np.ascontiguousarray(pat[:, :P]), freq[:P].copy()
    p0, r0 = pkg.free_rate_start(4)
    start = copy.copy(true)
    start.props, start.rates = p0, r0
    t = pkg.PhyloTree(nwk)
    t.set_alignment(n, seq_type, pat, freq)
    t.set_model(start)
    t.set_likelihood_kernel(pkg.LK_EIGEN_HIP)
    t.attach_engine(0)
    lib = pkg.libiqhip()
    t.compute_likelihood()
    a, b = t.current_branch()
    t.compute_likelihood_derv(a, b)
    lib.iqhip_timing_enable(t.engine, 1)
    ms = np.zeros(2)
    dp = ms.ctypes.data_as(C.POINTER(C.c_double))
    e_ms, o_ms = [], []
    for _ in range(12):
        t.em_posteriors()
        t.em_objective(a, b)
        lib.iqhip_debug_em_timing(t.engine, dp)
        e_ms.append(ms[0])
        o_ms.append(ms[1])
    lib.iqhip_timing_enable(t.engine, 0)

    def traversal():
        t.clear_all_partial_lh()
        t.compute_likelihood()

    traversal()
    trav_ms = median_ms(traversal, 10)
    # calls as the EM loop makes them (theta rebuilt, result read back), wall clock
    cat_sum = np.zeros(4)
    csp = cat_sum.ctypes.data_as(C.POINTER(C.c_double))
    estep_call_ms = median_ms(lambda: t.lib.iqhost_em_posteriors(t.h, None, csp), 10)   # (W stays on the device)
    obj_call_ms = median_ms(lambda: t.em_objective(a, b), 10)

    # the host route: the nptn x ncat matrix to the host, posteriors and their sums in numpy
    def host_estep():
        cat = t.compute_pattern_lh_cat()
        W = freq[:, None] * cat / cat.sum(axis=1, keepdims=True)
        return W, W.sum(axis=0)

    host_estep_ms = median_ms(host_estep, 10)
    W, _ = host_estep()

    def host_objective():
        cat = t.compute_pattern_lh_cat()
        sc = t.fetch_scale_num(a, b).astype(np.float64) if t.neighbor_info(a, b)["key"] else 0.0
        return (W * (np.log(cat / start.props[None, :]) + np.asarray(sc)[..., None] * -177.44567822334599)).sum(axis=0)

    host_obj_ms = median_ms(host_objective, 10)
    t.set_model(start)
    t.clear_all_partial_lh()
    t.compute_likelihood()
    t0 = time.perf_counter()
    res = t.optimize_free_rates_em(trace=True)
    em_s = time.perf_counter() - t0
    steps = [dict(rounds=s["rounds"], evals=[int(x) for x in s["evals"]], sum_evals=int(s["evals"].sum()),
                  floored=int(s["floored"].sum())) for s in res["trace"]]
    print(json.dumps(dict(workload=name, states=n, taxa=ntaxa, patterns=int(pat.shape[1]), ncat=4,
                          estep_device_ms=float(np.median(e_ms)), objective_device_ms=float(np.median(o_ms)),
                          traversal_ms=trav_ms, estep_call_ms=estep_call_ms, objective_call_ms=obj_call_ms,
                          host_route_estep_ms=host_estep_ms, host_route_objective_ms=host_obj_ms,
                          em_seconds=em_s, em_steps=steps, lnl=res["lnl"], props=list(res["props"]), rates=list(res["rates"]))))


if __name__ == "__main__":
    which = sys.argv[1] if len(sys.argv) > 1 else "all"
    for w in (WORKLOADS if which == "all" else [which]):
        run(w)
