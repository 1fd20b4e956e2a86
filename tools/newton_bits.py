"""Every bit the in-kernel branch-length solvers (k_newton, k_newton_batch, k_sweep4) return, on a fixed list of small
cases: one JSON line per solve, every double as float.hex().  Two builds of the library compute the same thing exactly
when the outputs are identical:

    IQHIP_LIB_DIR=$PWD/iq-tree_amd/lib_alt_parent python tools/newton_bits.py > parent.jsonl
    python tools/newton_bits.py > result.jsonl && diff parent.jsonl result.jsonl

Engines (about 10 taxa, +G4), chosen by tiles of the engine's pattern layout (4 states: 64 patterns, 20 states: 16):
  dna-4 / dna-8 / dna-24     at most 4 tiles (one workgroup per solve, no exchange), 5-8 (two workgroups in k_newton, the
                             8-wave workgroup in k_sweep4), more than 8
  asc-4 / asc-8 / asc-24     the same with +ASC: variable patterns only plus one unobserved constant pattern per state
  aa-12                      20 states (B = 80, theta in registers), more than 4 tiles per solve
and the dna / asc engines once more with the arrival-counter exchange (IQHIP_NEWTON_POSTS=0).  The tool asserts the tile
counts.  Per engine: the five (x1, xguess, x2, xacc, max_steps) set-ups of tests/test_solver_paths_gpu.py on a leaf and an
internal branch, on resident theta (iqhip_newton_branch) and through the fused front end (iqhip_optimize_branch); one
optimizeAllBranches pass with an upper bound of 0.05 -- the diverged-solve rule fires -- branch by branch, as one
submission, (4 states) as one submission in the per-step form, and through iqhip_optimize_sweep itself for each step's
status; and the batched NNI candidates."""
import ctypes as C
import importlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import __graft_entry__ as g

pkg = g.load_package()
synth = importlib.import_module("iqtree_amd.synth")
lib = pkg.libiqhip()

SETUPS = [(1e-6, None, 100.0, 1e-6, 100), (1e-6, 60.0, 100.0, 1e-6, 100), (1e-6, 0.01, 0.03, 1e-6, 100),
          (0.6, 0.9, 100.0, 1e-6, 100), (1e-6, 3.0, 100.0, 1e-6, 3)]
NTAXA = 10


class Result(C.Structure):
    _fields_ = [("optx", C.c_double), ("d2l", C.c_double), ("lnl", C.c_double), ("nsteps", C.c_int32), ("status", C.c_int32)]


class Step(C.Structure):
    _fields_ = [("ops", C.c_void_p), ("len_from", C.POINTER(C.c_int32)), ("nops", C.c_int32), ("_pad", C.c_int32),
                ("a", pkg.BranchEnd), ("b", pkg.BranchEnd), ("xguess", C.c_double)]


lib.iqhip_optimize_sweep.argtypes = [C.c_void_p, C.POINTER(Step), C.c_int, C.c_double, C.c_double, C.c_double, C.c_int,
                                     C.c_double, C.POINTER(C.c_double), C.POINTER(Result)]


def hx(v):
    return float(v).hex()


def emit(engine, what, **kw):
    print(json.dumps(dict(engine=engine, what=what, **kw), sort_keys=True), flush=True)


def inputs(n, nptn, asc, seed):
    """-> (newick, patterns, frequencies, n_unobs, nsites, model) with exactly nptn patterns"""
    model = synth.gtr_model(alpha=0.9, ncat=4) if n == 4 else synth.random_reversible_model(n, seed, alpha=0.9, ncat=4)
    if not asc:
        nwk, pat, freq = synth.make_workload(NTAXA, nptn, model, seed=seed)
        return nwk, pat, freq, 0, 0.0, model
    # as tests/test_asc_batch_gpu.py asc_inputs: simulate, drop the constant patterns, append one per state
    nwk = synth.random_tree_newick(NTAXA, seed + 1, 0.02, 0.15)
    pat, freq = synth.compress_patterns(synth.simulate_alignment(nwk, model, 4 * nptn, seed + 2))
    const = np.all(pat == pat[0][None, :], axis=0)
    pat, freq = pat[:, ~const][:, :nptn - n], freq[~const][:nptn - n].copy()
    assert pat.shape[1] == nptn - n
    ns = float(freq.sum())
    pat = np.ascontiguousarray(np.concatenate([pat, np.tile(np.arange(n, dtype=np.uint8)[None, :], (NTAXA, 1))], axis=1))
    return nwk, pat, np.concatenate([freq, np.zeros(n)]), n, ns, model


def tree(inp, n, mem_mode):
    nwk, pat, freq, nun, ns, model = inp
    t = pkg.PhyloTree(nwk)
    t.set_mem_mode(mem_mode)
    t.set_alignment(n, 0 if n == 4 else 1, pat, freq)
    t.set_ascertainment(nun, ns)
    t.set_model(model)
    t.set_likelihood_kernel(pkg.LK_EIGEN_HIP)
    t.attach_engine(0)
    t.set_device_newton(True)
    return t


def branches(t):
    return [(a, b) for a in range(t.num_nodes) for b, _ in t.neighbors(a) if a < b]


def two_branches(t):
    """a leaf branch and an internal branch"""
    inner = [(a, b) for (a, b) in branches(t) if len(t.neighbors(a)) == 3 and len(t.neighbors(b)) == 3]
    return [(0, t.neighbors(0)[0][0]), inner[len(inner) // 2]]


def ends(t, a, b):
    """the two iqhip_branch_end of branch (a, b); a leaf comes first, as the tip itself"""
    if len(t.neighbors(b)) == 1:
        a, b = b, a
    far = pkg.key_end(t.neighbor_info(a, b)["key"])
    return (pkg.leaf_end(a) if len(t.neighbors(a)) == 1 else pkg.key_end(t.neighbor_info(b, a)["key"])), far


def setups(name, inp, n):
    t = tree(inp, n, pkg.LM_ALL_BRANCH)
    t.compute_likelihood()
    for (a, b) in two_branches(t):
        cur = dict(t.neighbors(a))[b]
        t.reset_theta()
        t.compute_likelihood_derv(a, b)
        for (x1, xg, x2, xacc, ms) in SETUPS:
            xg = cur if xg is None else xg
            optx, d2l, ns = C.c_double(), C.c_double(), C.c_int()
            rc = lib.iqhip_newton_branch(t.engine, C.c_double(xg), C.c_double(x1), C.c_double(x2), C.c_double(xacc), ms,
                                         C.byref(optx), C.byref(d2l), C.byref(ns))
            emit(name, "newton_branch", branch=[a, b], setup=[x1, xg, x2, xacc, ms], optx=hx(optx.value), d2l=hx(d2l.value),
                 evaluations=ns.value, status=rc)
    t.compute_all_partial_lh()
    for (a, b) in two_branches(t):
        cur = dict(t.neighbors(a))[b]
        ea, eb = ends(t, a, b)
        for (x1, xg, x2, xacc, ms) in SETUPS:
            xg = cur if xg is None else xg
            optx, d2l, ns = C.c_double(), C.c_double(), C.c_int()
            rc = lib.iqhip_optimize_branch(t.engine, None, 0, ea, eb, C.c_double(xg), C.c_double(x1), C.c_double(x2),
                                           C.c_double(xacc), ms, None, C.byref(optx), C.byref(d2l), C.byref(ns))
            assert rc == 0, lib.iqhip_last_error()
            emit(name, "optimize_branch", branch=[a, b], setup=[x1, xg, x2, xacc, ms], optx=hx(optx.value), d2l=hx(d2l.value),
                 evaluations=ns.value, status=rc)
    # iqhip_optimize_sweep itself, no node updates: every step's result row, status 5 = the diverged-solve rule ran
    br = branches(t)
    steps = (Step * len(br))()
    for k, (a, b) in enumerate(br):
        steps[k].ops, steps[k].nops = None, 0
        steps[k].a, steps[k].b = ends(t, a, b)
        steps[k].xguess = dict(t.neighbors(a))[b]
    res = (Result * len(br))()
    rc = lib.iqhip_optimize_sweep(t.engine, steps, len(br), 1e-6, 0.05, 1e-6, 100, 0.95, None, res)
    assert rc == 0, lib.iqhip_last_error()
    assert any(r.status == 5 for r in res)
    for k, (a, b) in enumerate(br):
        emit(name, "optimize_sweep", branch=[a, b], optx=hx(res[k].optx), d2l=hx(res[k].d2l), evaluations=res[k].nsteps,
             status=res[k].status, diverged=int(res[k].status == 5))
    t.compute_likelihood()
    for m in t.evaluate_nnis_batch():
        emit(name, "nni", branch=[m["node1"], m["node2"]], swap=[m["node1_nei"], m["node2_nei"]], new_len=hx(m["new_len"]),
             newloglh=hx(m["newloglh"]))
    t.close()


def sweeps(name, inp, n):
    forms = [("per_branch", False, None), ("one_submission", True, None)]
    if n == 4:
        forms.append(("one_submission_per_step", True, "0"))
    for form, sweep, kernel in forms:
        if kernel is not None:
            os.environ["IQHIP_SWEEP_KERNEL"] = kernel    # (read when the engine is created)
        t = tree(inp, n, 0)
        os.environ.pop("IQHIP_SWEEP_KERNEL", None)
        t.set_device_sweep(sweep)
        t.set_branch_bounds(1e-6, 0.05)
        t.clear_all_partial_lh()
        c0 = t.num_derv_calls
        lnl = t.optimize_all_branches(iterations=1, tolerance=1e-9)
        lens = [[a, b, hx(ln)] for a in range(t.num_nodes) for b, ln in t.neighbors(a) if a < b]
        assert any(float.fromhex(v) > 0.0475 for _, _, v in lens)      # the diverged-solve rule ran
        emit(name, "sweep_" + form, lnl=hx(lnl), evaluations=t.num_derv_calls - c0, lengths=lens,
             paths={k: v for k, v in t.path_counts().items() if v and (k.startswith("sweep") or k.startswith("newton"))})
        t.close()


ENGINES = [("dna-4", 4, 250, False), ("dna-8", 4, 500, False), ("dna-24", 4, 1500, False),
           ("asc-4", 4, 250, True), ("asc-8", 4, 500, True), ("asc-24", 4, 1500, True), ("aa-12", 20, 150, False)]
TILES = {"dna-4": 4, "dna-8": 8, "dna-24": 24, "asc-4": 4, "asc-8": 8, "asc-24": 24, "aa-12": 12}


def main():
    if lib.iqhip_device_count() < 1:
        raise SystemExit("newton_bits.py: no HIP device visible")
    for name, n, nptn, asc in ENGINES:
        inp = inputs(n, nptn, asc, 7100 + nptn + n)
        assert inp[1].shape[1] == nptn
        ntiles = (nptn + 63) // 64 * 64 // (64 if n == 4 else 16)     # engine.hip configure_engine: patterns padded to 64
        assert ntiles == TILES[name], (name, ntiles)
        for posts in ((None, "0") if n == 4 else (None,)):
            if posts is not None:
                os.environ["IQHIP_NEWTON_POSTS"] = posts               # (read when the engine is created)
            label = name + ("" if posts is None else "-counter")
            setups(label, inp, n)
            sweeps(label, inp, n)
            os.environ.pop("IQHIP_NEWTON_POSTS", None)


if __name__ == "__main__":
    main()
