"""Estimation of model parameters on the device (iqhip_class_lnl, ModelOptimizer): one forward-difference stencil of the
reference's BFGS evaluated as the K classes of one candidate mixture engine against the same K points one after the other
on a plain engine (set_model + clear + compute_likelihood per point: the code path that existed before), the device time of
iqhip_class_lnl alone next to the wall time of the traversal in front of it, traversals per BFGS stencil both ways, and
the whole optimize_parameters (fixed branch lengths) both ways.
    python tools/bench_paramopt.py [dna500|dna5000|dna100000|protein2000|all]
GTR+G4 on DNA, 50 taxa x 500 / 5 000 / 100 000 patterns asked for; a random reversible 20-state matrix (LG-shaped) +I+G4,
50 x 2 000.  Prints one line of JSON per workload.  No threshold is fixed here."""
import importlib
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g  # noqa: E402

pkg = g.load_package()
synth = importlib.import_module("iqtree_amd.synth")
WORKLOADS = {"dna500": (4, 500), "dna5000": (4, 5000), "dna100000": (4, 100000), "protein2000": (20, 2000)}
LETTERS = {4: "ACGT", 20: "ARNDCQEGHILKMFPSTWYV"}


def median_ms(fn, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out))


def phylip(states, letters):
    lut = np.frombuffer(letters.encode(), dtype=np.uint8)
    rows = ["%d %s" % (t, lut[states[t]].tobytes().decode()) for t in range(states.shape[0])]
    return "%d %d\n%s\n" % (states.shape[0], states.shape[1], "\n".join(rows))


def device_tree(nwk, aln, st, fr, model):
    t = pkg.PhyloTree(nwk)
    t.set_alignment(aln.nstates, aln.seq_type, st, fr, aln.ptn_invar(model.p_invar, model.state_freq))
    t.set_model(model)
    t.set_likelihood_kernel(pkg.LK_EIGEN_HIP)
    t.attach_engine(0)
    return t


def mixture_of(models):
    """K plain models (one string each) as the K classes of a mixture: class weight 1, props = p_c"""
    return pkg.AttrDict(nclass=len(models), cat_class=np.repeat(np.arange(len(models)), models[0].ncat).astype(np.int32),
                        eval=np.concatenate([m.eval.reshape(-1) for m in models]),
                        evec=np.concatenate([m.evec.reshape(-1) for m in models]),
                        inv_evec=np.concatenate([m.inv_evec.reshape(-1) for m in models]),
                        rates=np.concatenate([m.rates for m in models]), props=np.concatenate([m.props for m in models]))


def run(name):
    n, P = WORKLOADS[name]
    ntaxa = 50
    nwk = synth.random_tree_newick(ntaxa, 5, 0.02, 0.2)
    tmp = tempfile.mkdtemp()
    if n == 4:
        truth = synth.gtr_model(rates6=(1.8, 4.2, 0.7, 1.3, 5.1, 1.0), freqs=(0.3, 0.2, 0.22, 0.28), alpha=0.6, ncat=4)
        st = synth.simulate_alignment(nwk, truth, int(P * 1.7) + 64, 3)
        head, tail, seq_type = "GTR", "+G4", "DNA"
    else:
        rng = np.random.default_rng(7)
        R = rng.gamma(shape=1.0, scale=1.0, size=(20, 20)) + 0.05
        R = (R + R.T) / 2.0
        f = rng.dirichlet(np.full(20, 5.0))
        truth = synth.reversible_model(R, f, 0.7, 4, 0.1)
        st = synth.simulate_alignment(nwk, truth, int(P * 1.1) + 64, 3)
        st[:, :P // 10] = st[0:1, :P // 10]
        head = os.path.join(tmp, "random.paml")
        with open(head, "w") as fh:
            for i in range(1, 20):
                fh.write(" ".join("%.17g" % R[i, j] for j in range(i)) + "\n")
            fh.write("\n" + " ".join("%.17g" % x for x in f) + "\n")
        tail, seq_type = "+I+G4", "AA"
    # (the patterns are whatever the alignment compresses to; the count is reported)
    keep = np.zeros(st.shape[1], dtype=bool)
    cols = {}
    for s in range(st.shape[1]):
        key = st[:, s].tobytes()
        if key in cols or len(cols) < P:
            cols.setdefault(key, True)
            keep[s] = True
    aln = pkg.Alignment(content=phylip(st[:, keep], LETTERS[n]), seq_type=seq_type)
    sts, fr, _, _ = aln.arrays()
    freqs = aln.state_freq()
    ftok = "+F{%s}" % ",".join("%.17g" % x for x in freqs / freqs.sum()) if n == 4 else ""
    ndim = 5 if n == 4 else 0
    p0 = max(aln.frac_const_sites / 2.0, 1e-6)
    rate_tok = "+G4{1}" if n == 4 else "+I{%.17g}+G4{1}" % p0

    def string(params):
        return (head + ("{%s}" % ",".join("%.17g" % x for x in params) if ndim else "")) + ftok + rate_tok

    out = dict(workload=name, states=n, taxa=ntaxa, patterns=int(aln.npattern), ncat=4, ndim=ndim)
    if ndim:
        # one stencil: the base point and its ndim forward points, h = 1e-4 |x|
        x0 = np.ones(ndim)
        pts = [x0] + [x0 + 1e-4 * np.eye(ndim)[d] for d in range(ndim)]
        models = [aln.build_model(string(p)) for p in pts]
        K = len(models)
        tm = device_tree(nwk, aln, sts, fr, models[0])
        mix = mixture_of(models)
        mix.p_invar, mix.state_freq = models[0].p_invar, models[0].state_freq
        tc = device_tree(nwk, aln, sts, fr, mix)
        tc.compute_likelihood()
        a, b = tc.current_branch()
        ones = np.ones(K)
        pkg.libiqhip().iqhip_timing_enable(tc.engine, 1)

        def batched():
            tc.set_model(mix)
            tc.clear_all_partial_lh()
            return tc.class_lnl(a, b, ones)[0]

        def sequential():
            vals = []
            for m in models:
                tm.set_model(m)
                tm.clear_all_partial_lh()
                vals.append(tm.compute_likelihood())
            return np.array(vals)

        vb, vs = batched(), sequential()
        out["stencil_max_rel_diff"] = float(np.max(np.abs(vb - vs) / np.abs(vs)))
        out["stencil_batched_ms"] = median_ms(batched, 15)
        out["stencil_sequential_ms"] = median_ms(sequential, 15)
        kern = []
        for _ in range(15):
            batched()
            kern.append(tc.class_lnl_timing())
        out["class_lnl_device_ms"] = float(np.median(kern))

        def cand_traversal():
            tc.clear_all_partial_lh()
            tc.compute_likelihood()

        def plain_traversal():
            tm.clear_all_partial_lh()
            tm.compute_likelihood()

        out["candidate_traversal_ms"] = median_ms(cand_traversal, 15)
        out["plain_traversal_ms"] = median_ms(plain_traversal, 15)
        out["K"] = K
    for batch in (True, False):
        t = device_tree(nwk, aln, sts, fr, aln.build_model(string(np.ones(ndim))))
        t.compute_likelihood()
        opt = pkg.ModelOptimizer(t, aln, string(np.ones(ndim)), batch="always" if batch else False)
        t0 = time.perf_counter()
        lnl = opt.optimize_parameters(fixed_len=True)
        sec = time.perf_counter() - t0
        tr = opt.trace
        stencils = sum(c["stencils"] for c in tr)
        key = "batched" if batch else "sequential"
        out[key] = dict(seconds=sec, lnl=lnl, rounds=opt.rounds, stencils=stencils,
                        stencil_traversals=sum(c["stencil_traversals"] for c in tr),
                        single_traversals=sum(c["single_traversals"] for c in tr),
                        model_call_traversals_per_stencil=(sum(c["stencil_traversals"] + c["single_traversals"] for c in tr
                                                               if c["what"] == "model") / stencils) if stencils else None,
                        redone=sum(c["stencils_redone"] for c in tr), model=opt.model_string())
    print(json.dumps(out))


if __name__ == "__main__":
    which = sys.argv[1] if len(sys.argv) > 1 else "all"
    for w in (WORKLOADS if which == "all" else [which]):
        run(w)
