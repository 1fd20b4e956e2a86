"""NNI evaluation (hot loop 2 of the tree search): all 2(n-3) nni1 candidates, branch by branch
(getBestNNIForBran, the reference's order) vs one batched submission (evaluateNNIsBatch).

--asc: +ASC data instead -- variable sites only plus one unobserved constant pattern per state -- on
(4 states, G4, 50 taxa, 100 k sites) and (20 states, G4, 50 taxa, 20 k sites); also times a branch-length sweep in its
per-branch and its one-submission form.  A library without the batched +ASC forms reports the per-branch forms only."""
import argparse, importlib, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import __graft_entry__ as g
pkg = g.load_package(); synth = importlib.import_module("iqtree_amd.synth")
ap = argparse.ArgumentParser()
ap.add_argument("--asc", action="store_true", help="variable sites only + n unobserved constant patterns (+ASC)")
ap.add_argument("--reps", type=int, default=5)
args = ap.parse_args()
reps = args.reps


def plain_tree(T, P):
    model = synth.gtr_model()
    nwk, pat, freq = synth.make_workload(T, P, model, seed=3)
    t = pkg.PhyloTree(nwk); t.set_mem_mode(pkg.LM_ALL_BRANCH); t.set_alignment(4, 0, pat, freq); t.set_model(model)
    t.attach_engine(0)
    return t


def asc_tree(n, T, S, mem_mode):
    model = synth.gtr_model(alpha=0.9, ncat=4) if n == 4 else synth.random_reversible_model(n, 51, alpha=0.9, ncat=4)
    nwk = synth.random_tree_newick(T, 52, 0.02, 0.15)
    pat, freq = synth.compress_patterns(synth.simulate_alignment(nwk, model, S, 53))
    const = np.all(pat == pat[0][None, :], axis=0)
    pat, freq = np.ascontiguousarray(pat[:, ~const]), freq[~const].copy()
    nsites = float(freq.sum())
    pat = np.ascontiguousarray(np.concatenate([pat, np.tile(np.arange(n, dtype=np.uint8)[None, :], (T, 1))], axis=1))
    freq = np.concatenate([freq, np.zeros(n)])
    t = pkg.PhyloTree(nwk); t.set_mem_mode(mem_mode); t.set_alignment(n, 0 if n == 4 else 1, pat, freq)
    t.set_ascertainment(n, nsites); t.set_model(model)
    t.attach_engine(0)
    return t


def timed(f, n):
    f()
    t0 = time.perf_counter()
    for _ in range(n):
        out = f()
    return (time.perf_counter() - t0) / n, out


def nni(t, label):
    t.compute_likelihood()
    try:
        tb, b = timed(t.evaluate_nnis_batch, reps)
    except pkg.HostError as err:
        tb, b = None, None
        print("%s: no batched form (%s)" % (label, err))
    t.compute_all_partial_lh()
    branches = sorted({(a, x) for a in range(t.num_nodes) for x, _ in t.neighbors(a)
                       if a < x and len(t.neighbors(a)) == 3 and len(t.neighbors(x)) == 3})
    t0 = time.perf_counter()
    for (x, y) in branches:
        t.nni_for_branch(x, y, nni5=False)
    ts = time.perf_counter() - t0
    ncand = 2 * len(branches)
    print("%s: %d candidates; nni1 branch by branch %.2f ms (%.1f us per candidate)%s" % (
        label, ncand, ts * 1e3, ts * 1e6 / ncand,
        "" if tb is None else ", batched %.2f ms (%.1f us per candidate)" % (tb * 1e3, tb * 1e6 / ncand)))
    return branches


if args.asc:
    for (n, T, S) in ((4, 50, 100000), (20, 50, 20000)):
        label = "+ASC %d states, taxa %d, sites %d" % (n, T, S)
        nni(asc_tree(n, T, S, pkg.LM_ALL_BRANCH), label)
        for sweep in (False, True):
            t = asc_tree(n, T, S, 0)
            t.set_device_newton(True); t.set_device_sweep(sweep)
            t.compute_likelihood()
            nbranch = 2 * T - 3
            s0 = t.num_submissions
            dt, _ = timed(lambda: t.optimize_all_branches(iterations=1, tolerance=1e-9), reps)
            pc = t.path_counts()
            print("    sweep (device_sweep=%d): %.2f ms per optimizeAllBranches pass, %.1f us per branch; submissions %d, paths %s" % (
                sweep, dt * 1e3, dt * 1e6 / nbranch, t.num_submissions - s0,
                {k: v for k, v in pc.items() if k.startswith("sweep") and v}))
    sys.exit(0)

for (T, P) in ((44, 355), (50, 5000), (50, 100000)):
    t = plain_tree(T, P)
    branches = nni(t, "taxa %d patterns %d" % (T, P))
    tb5, b5 = timed(t.evaluate_nnis5_batch, reps)
    t0 = time.perf_counter()
    for (x, y) in branches:
        t.nni_for_branch(x, y, nni5=True)
    ts5 = time.perf_counter() - t0
    print("    nni5 branch by branch %.2f ms (%.1f us per candidate), batched %.2f ms (%.1f us per candidate)" %
          (ts5 * 1e3, ts5 * 1e6 / len(b5), tb5 * 1e3, tb5 * 1e6 / len(b5)))
