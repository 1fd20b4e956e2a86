"""EM estimation of mixture class weights on the device (iqhip_mix_class_lh / iqhip_mix_weights_em): device time of the
class-likelihood launch and of the EM chain, time per EM step, the bandwidth that implies against the one read of the
8 * nclass * nptn_pad bytes of the class-likelihood matrix a step makes, the chain's launches, what an enqueued step costs
once the loop has converged, and next to them the numpy restatement (tests/mixem_ref.py) on the fetched matrix.
    python tools/bench_mixem.py [sites [classes [rates]]]      default: protein, 50 taxa x 20 000 sites, 20 classes x 4 rates
Prints one line of JSON.  No threshold is fixed here."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as g  # noqa: E402

pkg = g.load_package()
import importlib  # noqa: E402

import mixem_ref  # noqa: E402

synth = importlib.import_module("iqtree_amd.synth")


def median(xs):
    return float(np.median(xs))


def run(nsites, nclass, ncat, ntaxa=50, reps=10):
    model = synth.mixture_model(20, nclass, 21, ncat=ncat)
    nwk = synth.random_tree_newick(ntaxa, 5, 0.02, 0.2)
    share = -(-nsites // nclass)
    st = np.concatenate([synth.simulate_alignment(nwk, model.classes[m], share, 30 + m) for m in range(nclass)], axis=1)
    pat, freq = synth.compress_patterns(st)
    t = pkg.PhyloTree(nwk)
    t.set_alignment(20, 1, pat, freq)
    t.set_model(model)
    t.set_likelihood_kernel(pkg.LK_EIGEN_HIP)
    t.attach_engine(0)
    t.compute_likelihood()
    lib = pkg.libiqhip()
    w0 = np.array([model.props[model.cat_class == m].sum() for m in range(nclass)])
    Lc = t.mix_class_lh()
    nptn = pat.shape[1]
    nptn_pad = -(-nptn // 16) * 16
    lib.iqhip_timing_enable(t.engine, 1)
    lh_ms = []
    for _ in range(reps):
        t.lib.iqhost_mix_class_lh(t.h, None)             # (the matrix stays on the device)
        lh_ms.append(t.mix_timing()["class_lh_ms"])

    def chain(max_steps):
        ms, res = [], None
        for _ in range(reps):
            res = t.mix_weights_em(w0, max_steps=max_steps)
            ms.append(t.mix_timing()["em_ms"])
        return median(ms), res, t.mix_timing()["launches"]

    ref_ms, ref_res, ref_launches = chain(nclass)             # what the reference runs: nclass steps
    long_steps = 2000
    long_ms, long_res, long_launches = chain(long_steps)      # to convergence, the rest of the chain idles
    k = long_res["steps"]
    conv_ms, _, _ = chain(k)                                  # the converged run without idle steps
    lib.iqhip_timing_enable(t.engine, 0)
    wall = []
    for _ in range(reps):
        t0 = time.perf_counter()
        t.mix_weights_em(w0, max_steps=nclass)
        wall.append((time.perf_counter() - t0) * 1e3)
    t0 = time.perf_counter()
    ref = mixem_ref.optimize_weights(Lc, freq, None, w0, max_steps=nclass)
    numpy_ms = (time.perf_counter() - t0) * 1e3
    step_ms = ref_ms / ref_res["steps"]
    bytes_per_step = 8.0 * nclass * nptn_pad
    print(json.dumps(dict(
        workload="protein mixture", taxa=ntaxa, sites=int(st.shape[1]), patterns=int(nptn), nptn_pad=int(nptn_pad), classes=nclass,
        rates=ncat, class_lh_device_ms=median(lh_ms),
        em_steps=ref_res["steps"], em_chain_device_ms=ref_ms, em_step_device_us=step_ms * 1e3, em_launches=int(ref_launches),
        matrix_mib=bytes_per_step / 2**20, step_gb_per_s=bytes_per_step / (step_ms * 1e-3) / 1e9,
        em_call_wall_ms=median(wall),
        converged_after=k, converged=long_res["converged"], chain_to_convergence_ms=conv_ms,
        step_to_convergence_us=conv_ms / k * 1e3, long_chain_steps=long_steps, long_chain_ms=long_ms,
        long_chain_launches=int(long_launches),
        idle_step_us=(long_ms - conv_ms) / max(1, long_steps - k) * 1e3 if k < long_steps else None,
        numpy_restatement_ms=numpy_ms, numpy_steps=ref["steps"],
        max_rel_weight_diff=float(np.max(np.abs(ref_res["weights"] - ref["prop"]) / ref["prop"])))))


if __name__ == "__main__":
    a = [int(x) for x in sys.argv[1:]]
    run(a[0] if len(a) > 0 else 20000, a[1] if len(a) > 1 else 20, a[2] if len(a) > 2 else 4)
