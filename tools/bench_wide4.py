"""Wide DNA (4 states, 9 .. 32 categories or components): full traversals at 50 taxa x 100 000 patterns under a
GTR+G16 model and a 12-component mixture (3 classes x G4), on the route the environment selects: IQHIP_WIDE4=valu is
k_traverse4w, IQHIP_WIDE4=generic the padded matrix-core kernel, unset the engine's default.  Every record names the
kernel the planner chose (slot 14 of iqhip_debug_plan_shape for the same shape and environment), never the variable.
Per model: kernel time per traversal from iqhip_timing_read (HIP events around the traversal launches), pattern-node
updates per second, and the bytes the plan's descriptors move (iqhip_timing_plan_bytes) over that time.  The A/B is the
pair IQHIP_WIDE4=valu / IQHIP_WIDE4=generic, run alternately on one device.
usage: python tools/bench_wide4.py [--json] [--reps N] [--taxa T] [--patterns P]"""
import argparse, ctypes as C, importlib, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g
pkg = g.load_package(); synth = importlib.import_module("iqtree_amd.synth")

HBM_PEAK_GBS = 8000.0   # MI355X data sheet
VARIANTS = {1: "generic", 10: "k_traverse4w"}   # TravVariant (iqhip_internal.h), as iqhip_debug_plan_shape reports it


def route_of(ncat, nclass, T, P):
    """the node-update kernel a (4, ncat) engine of this environment launches: a planning-only engine of the same shape
    plans one cherry, slot 14 of its plan shape is the top launch's variant"""
    lib, e = pkg.libiqhip(), C.c_void_p()
    if lib.iqhip_debug_create_planner(C.byref(e), 4, ncat, P, T, 256, 18, nclass) != 0:
        raise SystemExit(lib.iqhip_last_error().decode())
    try:
        ops = (pkg.NodeOp * 1)(pkg.NodeOp(1, 0, 0, 0, 1, 0.1, 0.1, 0, 0))
        rec = (C.c_int64 * len(pkg.PLAN_SHAPE_SLOTS))()
        if lib.iqhip_debug_plan(e, ops, 1) != 0 or lib.iqhip_debug_plan_shape(e, rec, len(rec)) != 0:
            raise SystemExit(lib.iqhip_last_error().decode())
        return VARIANTS.get(rec[14], "variant %d" % rec[14])
    finally:
        lib.iqhip_destroy(e)


def one_model(name, model, T, P, warmup, reps):
    nwk, pat, freq = synth.make_workload(T, P, getattr(model, "classes", [model])[0], seed=3)   # (a mixture: sites of its first class)
    t = pkg.PhyloTree(nwk); t.set_alignment(4, 0, pat, freq); t.set_model(model); t.attach_engine(0)
    lib, eng = pkg.libiqhip(), t.engine

    def step():
        t.clear_all_partial_lh()
        return t.compute_likelihood()
    for _ in range(warmup):
        lnl = step()
    lib.iqhip_timing_enable(eng, 1)
    rounds = []
    for _ in range(reps):   # each repetition: 10 traversals, one reading
        for _ in range(10):
            lnl = step()
        avg_ms, launches = C.c_double(), C.c_int64()
        lib.iqhip_timing_read(eng, C.byref(avg_ms), C.byref(launches), 1)
        rounds.append(avg_ms.value * launches.value / 10.0)   # ms per traversal, all its launches together
    lib.iqhip_timing_enable(eng, 0)
    st_b, ld_b = C.c_double(), C.c_double()
    lib.iqhip_timing_plan_bytes(eng, C.byref(st_b), C.byref(ld_b))
    t.close()
    rounds.sort()
    med = rounds[len(rounds) // 2]
    nbytes = st_b.value + ld_b.value
    return dict(model=name, route=route_of(model.ncat, len(getattr(model, "classes", [model])), T, P), ntaxa=T, patterns=P, ncat=model.ncat,
                ms_per_traversal=med, ms_min=rounds[0], ms_max=rounds[-1], rounds=len(rounds),
                mpattern_node_updates_per_s=(T - 2) * P / (med * 1e-3) / 1e6, plan_bytes=nbytes,
                plan_gbs=nbytes / (med * 1e-3) / 1e9, hbm_frac=nbytes / (med * 1e-3) / 1e9 / HBM_PEAK_GBS, lnL=lnl)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", action="store_true")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--taxa", type=int, default=50)
    ap.add_argument("--patterns", type=int, default=100000)
    a = ap.parse_args()
    out = [one_model("GTR+G16", synth.gtr_model(alpha=0.9, ncat=16), a.taxa, a.patterns, a.warmup, a.reps),
           one_model("MIX3+G4", synth.mixture_model(4, 3, 17, ncat=4), a.taxa, a.patterns, a.warmup, a.reps)]
    if a.json:
        print(json.dumps(out))
    else:
        for r in out:
            print("%(model)-8s %(route)-12s taxa %(ntaxa)d patterns %(patterns)d C %(ncat)d: %(ms_per_traversal).3f ms per traversal "
                  "(min %(ms_min).3f, max %(ms_max).3f over %(rounds)d readings), %(mpattern_node_updates_per_s).0f M pattern-node updates/s, "
                  "%(plan_gbs).0f GB/s of plan bytes = %(hbm_frac).2f of HBM peak, lnL %(lnL).4f" % r)
