"""The rebuild legs of k_traverse4's fill image (DESIGN.md 3.1 "Fill image") at the headline shape, DNA 50 taxa x 100k
patterns, GTR+G4: clearAllPartialLH + computeLikelihood per step, with something changed before every step.
  leg a  one branch length alternates between two values: every step plans anew and fills its chunks in the kernel
  leg b  the model's alpha changes: the plan stays cached, its image is stale at every step and is built again (policy A)
  leg c  nothing changes (the benchmark's step), for scale
Prints one JSON line; `built` / `reused` are iqhip_debug_fill_image's counts over the timed steps (absent from a library
without the image).
    python tools/bench_fill_image.py [steps] [repeats]"""
import ctypes as C
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g  # noqa: E402

pkg = g.load_package()
synth = importlib.import_module("iqtree_amd.synth")
STEPS = int(sys.argv[1]) if len(sys.argv) > 1 else 200
REPEATS = int(sys.argv[2]) if len(sys.argv) > 2 else 3
lib = pkg.libiqhip()

nwk, pat, freq, model = synth.baseline_workload("dna")
tree = pkg.PhyloTree(nwk)
tree.set_alignment(4, synth.BASELINE_SHAPES["dna"][4], pat, freq)
tree.set_model(model)
tree.set_likelihood_kernel(pkg.LK_EIGEN_HIP)
tree.attach_engine(0)
models = [synth.gtr_model(alpha=a, ncat=model.ncat) for a in (0.9, 1.1)]
leaf = 0
nb = tree.neighbors(leaf)[0][0]
lens = (0.11, 0.13)


def counts():
    if not hasattr(lib, "iqhip_debug_fill_image"):
        return None
    a, b = C.c_int64(), C.c_int64()
    lib.iqhip_debug_fill_image.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    lib.iqhip_debug_fill_image(tree.engine, C.byref(a), C.byref(b), None)
    return a.value, b.value


def leg(change):
    for k in range(20):
        change(k)
        tree.clear_and_compute_likelihood()
    c0 = counts()
    t0 = time.perf_counter()
    for k in range(STEPS):
        change(k)
        tree.clear_and_compute_likelihood()
    dt = (time.perf_counter() - t0) / STEPS * 1e3
    c1 = counts()
    return dt, (None if c0 is None else (c1[0] - c0[0], c1[1] - c0[1]))


legs = {"a_length": lambda k: tree.set_branch_length(leaf, nb, lens[k & 1]),
        "b_model": lambda k: tree.set_model(models[k & 1]),
        "c_same": lambda k: None}
out = {"bench": "fill_image_legs", "steps": STEPS, "repeats": REPEATS}
for name, change in legs.items():
    ms, cnt = [], None
    for _ in range(REPEATS):
        dt, cnt = leg(change)
        ms.append(dt)
    out[name] = {"ms_per_step": ms, "built_reused": cnt}
tree.close()
print(json.dumps(out))
