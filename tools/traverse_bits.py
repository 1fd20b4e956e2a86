"""Every bit the traversal kernels (k_traverse4, k_traverse4w, k_traverse_mfma, trav_mfma2_body, k_traverse_mfma_mix20,
trav_rows64_body, the node update of k_sweep4) leave behind, on a fixed list of small cases: one JSON line per case, every
double as float.hex(), long arrays as the sha256 of their bytes.  Two builds of the library compute the same thing exactly
when the outputs are identical:

    IQHIP_LIB_DIR=$PWD/iq-tree_amd/lib_alt_parent python tools/traverse_bits.py > parent.jsonl
    python tools/traverse_bits.py > result.jsonl && diff parent.jsonl result.jsonl

(a) "table": the scaling rule's truth table through the C ABI, as tests/test_multifurcation_gpu.py builds it -- three
    uploaded child vectors, a NO_SCALE product of two of them, then the node's own update with flags 0, NO_SCALE and
    SCALAR_RULE -- on one alignment that holds ordinary patterns, patterns whose children are all tiny (product below
    2^-256) with and without an invariant-site term, patterns with one child exactly zero (one of them with an
    invariant-site term) and a pattern whose product is a denormal; plus a leaf-leaf, a leaf-internal and an
    internal-internal update on real states (ambiguity codes and the unknown state included), the branch lnL, pattern_lh
    and df / ddf on top of them.  150 patterns for 4 states (three 64-pattern tiles, the last ragged), 40 for 20 / 64
    states (three 16-pattern tiles).
(b) "chain": whole traversals of a 300-taxon caterpillar and of a 300-taxon random tree (joins: parked operands) with
    branch lengths 0.4 .. 0.9, so that the patterns rescale on the way (20 / 64 states: several times) and the rescaled value is consumed from
    registers, from the parked copy and from memory: lnL, pattern_lh, every vector, counter and lh_scale_factor, df / ddf.
(c) "sweep": one optimizeAllBranches pass through k_sweep4 on that caterpillar: the lengths and the final lnL.
Every case also prints the launch the planner chooses for its op list under the case's environment (variant, leaf
tables, grid, ... of iqhip_debug_plan_shape, on a planning-only engine of the same shape): both builds ran the same kernel."""
import ctypes as C
import hashlib
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

SU = {4: 18, 20: 23, 64: 64}
SEQ_TYPE = {4: 0, 20: 1, 64: 2}
NPTN = {4: 150, 20: 40, 64: 40}
NUM_CUS = 256      # of the planning-only engine (MI355X)
DP, I16P = C.POINTER(C.c_double), C.POINTER(C.c_int16)
NO_SCALE, SCALAR_RULE = 1, 2

# (label, states, categories per class, classes, environment): how every site of the scaling tail is reached
TABLE_CASES = [
    ("t4-c1", 4, 1, 1, {}),
    ("t4-c4-ls1", 4, 4, 1, {"IQHIP_LANE_SPLIT": "1"}), ("t4-c4-ls2", 4, 4, 1, {"IQHIP_LANE_SPLIT": "2"}),
    ("t4-c8-ls1", 4, 8, 1, {"IQHIP_LANE_SPLIT": "1"}), ("t4-c8-ls2", 4, 8, 1, {"IQHIP_LANE_SPLIT": "2"}),
    ("t4w-c9", 4, 9, 1, {"IQHIP_WIDE4": "valu"}), ("t4w-c32", 4, 32, 1, {"IQHIP_WIDE4": "valu"}),
    ("t4w-mix3x4", 4, 4, 3, {"IQHIP_WIDE4": "valu"}),
    ("generic-4x9", 4, 9, 1, {"IQHIP_WIDE4": "generic"}), ("generic-64x2", 64, 2, 1, {}),
    ("generic-64-mix2x1", 64, 1, 2, {}),
    ("mfma2-20x1", 20, 1, 1, {}),
    ("mfma2-20x4-cs0-top0", 20, 4, 1, {"IQHIP_CAT_SPLIT": "0", "IQHIP_TOP_CS2": "0"}),
    ("mfma2-20x4-cs0-top1", 20, 4, 1, {"IQHIP_CAT_SPLIT": "0", "IQHIP_TOP_CS2": "1"}),
    ("mfma2-20x4-cs1-top0", 20, 4, 1, {"IQHIP_CAT_SPLIT": "1", "IQHIP_TOP_CS2": "0"}),
    ("mfma2-20x4-cs1-top1", 20, 4, 1, {"IQHIP_CAT_SPLIT": "1", "IQHIP_TOP_CS2": "1"}),
    ("mfma2-64x1-tab0", 64, 1, 1, {"IQHIP_ROW_SPLIT": "0", "IQHIP_LEAF_TABLES": "0"}),
    ("mfma2-64x1-tab1", 64, 1, 1, {"IQHIP_ROW_SPLIT": "0", "IQHIP_LEAF_TABLES": "1"}),
    ("mix20-20x2", 20, 2, 1, {}),
    ("mix20-20x8-cs0", 20, 8, 1, {"IQHIP_CAT_SPLIT": "0"}), ("mix20-20x8-cs1", 20, 8, 1, {"IQHIP_CAT_SPLIT": "1"}),
    ("mix20-mix3x4", 20, 4, 3, {}),
    ("rows64-64x1", 64, 1, 1, {"IQHIP_ROW_SPLIT": "1"}),
]
# one or two per family; 4 states: joins read the parked copy; IQHIP_HOLD_LDS: the parked copy or memory
CHAIN_CASES = [
    ("t4-c4-hold1", 4, 4, 1, {}),
    ("t4w-c9", 4, 9, 1, {"IQHIP_WIDE4": "valu"}),
    ("generic-64x2", 64, 2, 1, {}),
    ("mfma2-20x4-hold1", 20, 4, 1, {"IQHIP_CAT_SPLIT": "0", "IQHIP_TOP_CS2": "0", "IQHIP_HOLD_LDS": "1"}),
    ("mfma2-20x4-hold0", 20, 4, 1, {"IQHIP_CAT_SPLIT": "0", "IQHIP_TOP_CS2": "0", "IQHIP_HOLD_LDS": "0"}),
    ("mfma2-20x4-split", 20, 4, 1, {}),
    ("mfma2-64x1", 64, 1, 1, {"IQHIP_ROW_SPLIT": "0"}),
    ("mix20-20x2", 20, 2, 1, {}),
    ("rows64-64x1", 64, 1, 1, {"IQHIP_ROW_SPLIT": "1"}),
]
NTAXA_CHAIN = 300


def hx(v):
    return float(v).hex()


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def emit(what, label, **kw):
    print(json.dumps(dict(what=what, case=label, **kw), sort_keys=True), flush=True)


def set_env(env):
    for k in [k for k in os.environ if k.startswith("IQHIP_") and k != "IQHIP_LIB_DIR"]:
        del os.environ[k]
    os.environ.update(env)      # (read when an engine is created)


def model_for(n, ncat, nclass, seed):
    if nclass > 1:
        return synth.mixture_model(n, nclass, seed, ncat=ncat)
    return synth.gtr_model(alpha=0.9, ncat=ncat) if n == 4 else synth.random_reversible_model(n, seed, alpha=0.9, ncat=ncat)


def device_tree(nwk, n, states, freq, invar, model):
    t = pkg.PhyloTree(nwk)
    t.set_alignment(n, SEQ_TYPE[n], states, freq, invar)
    t.set_model(model)
    t.set_likelihood_kernel(pkg.LK_EIGEN_HIP)
    t.attach_engine(0)
    return t


def node_ops(rows):
    ops = (pkg.NodeOp * len(rows))()
    for k, r in enumerate(rows):
        ops[k] = pkg.NodeOp(*r)
    return ops


def launch_of(n, ncomp, nclass, nptn, ntaxa, ops, uploaded=()):
    """the launches the planner chooses for this op list under the current environment; `uploaded`: keys the list reads
    without computing them (a plan of their own makes them known to the planner first)"""
    e = C.c_void_p()
    rc = lib.iqhip_debug_create_planner(C.byref(e), n, ncomp, nptn, ntaxa, NUM_CUS, SU[n], nclass)
    assert rc == 0, lib.iqhip_last_error()
    try:
        if uploaded:
            first = node_ops([(key, 0, 0, 0, 1, 0.1, 0.1, 0, 0) for key in uploaded])
            assert lib.iqhip_debug_plan(e, first, len(first)) == 0, lib.iqhip_last_error()
        assert lib.iqhip_debug_plan(e, ops, len(ops)) == 0, lib.iqhip_last_error()
        rec = (C.c_int64 * len(pkg.PLAN_SHAPE_SLOTS))()
        assert lib.iqhip_debug_plan_shape(e, rec, len(rec)) == 0, lib.iqhip_last_error()
    finally:
        lib.iqhip_destroy(e)
    return {k: int(v) for k, v in zip(pkg.PLAN_SHAPE_SLOTS, rec) if k.startswith("top_") or k.startswith("unit_")}


# ---- (a) the truth table
K_CHILD = (9000011, 9000012, 9000013)
K_PRODUCT, K_RULE0, K_NEVER, K_SCALAR, K_LEAVES, K_LEAF_INNER, K_JOIN = range(9000500, 9000507)
ZERO_PTN, ZERO_INVAR_PTN, DENORMAL_PTN, TINY_PTN, TINY_INVAR_PTN = (7, -1), 1, 3, 5, 9


def table_ops():
    lens = (0.11, 0.07, 0.23)
    rows = [(K_PRODUCT, K_CHILD[0], K_CHILD[1], -1, -1, lens[0], lens[1], NO_SCALE, 0)]
    for key, flags in ((K_RULE0, 0), (K_NEVER, NO_SCALE), (K_SCALAR, SCALAR_RULE)):
        rows.append((key, K_PRODUCT, K_CHILD[2], -1, -1, 0.0, lens[2], flags, 0))
    rows.append((K_LEAVES, 0, 0, 0, 1, 0.05, 0.31, 0, 0))                     # leaf - leaf
    rows.append((K_LEAF_INNER, 0, K_SCALAR, 2, -1, 0.09, 0.14, 0, 0))         # leaf - internal
    rows.append((K_JOIN, K_LEAVES, K_LEAF_INNER, -1, -1, 0.21, 0.02, 0, 0))   # internal - internal
    return rows


def table_case(label, n, ncat, nclass, env):
    set_env(env)
    nptn, ntaxa = NPTN[n], 4
    model = model_for(n, ncat, nclass, 31)
    ncomp = len(model.rates)
    B = n * ncomp
    rng = np.random.default_rng(1000 * n + 10 * ncomp + nclass)
    states = rng.integers(0, n, size=(ntaxa, nptn)).astype(np.uint8)
    states[:, 11] = SU[n]                           # gaps, and (4 / 20 states) ambiguity codes: the leaf tables' other rows
    states[0, 12], states[2, 13] = SU[n], SU[n]
    if n < 64:
        states[1, 14], states[2, 15], states[0, nptn - 2] = n + 1, n + 2, n
    inv0 = np.asarray(model.inv_evec, dtype=np.float64).reshape(-1, n, n)[0]
    kids = []
    for k in range(3):
        prob = rng.uniform(1e-3, 1.0, size=(nptn, ncomp, n))
        kids.append(np.ascontiguousarray(np.einsum("ix,pcx->pci", inv0, prob).reshape(nptn, B)))
    kids[1][list(ZERO_PTN) + [ZERO_INVAR_PTN]] = 0.0
    for k in range(3):
        kids[k][DENORMAL_PTN] *= 1e-104
        kids[k][TINY_PTN] *= 1e-30
        kids[k][TINY_INVAR_PTN] = kids[k][TINY_PTN]
    sc = [rng.integers(0, 3, nptn).astype(np.int16) for _ in range(3)]
    freq = rng.integers(1, 5, nptn).astype(np.float64)
    invar = np.zeros(nptn)
    invar[ZERO_INVAR_PTN] = invar[TINY_INVAR_PTN] = 0.01
    t = device_tree(synth.random_tree_newick(ntaxa, 5), n, states, freq, invar, model)
    tree_lnl = t.compute_likelihood()               # (the engine exists and holds the model and the alignment)
    e = t.engine
    for k in range(3):
        assert lib.iqhip_upload_partial(e, K_CHILD[k], kids[k].ctypes.data_as(DP), sc[k].ctypes.data_as(I16P)) == 0, lib.iqhip_last_error()
    rows = table_ops()
    ops = node_ops(rows)
    ss = np.zeros(len(rows))
    assert lib.iqhip_update_partials(e, ops, len(rows), ss.ctypes.data_as(DP)) == 0, lib.iqhip_last_error()
    vec, cnt = {}, {}
    for name, key in (("product", K_PRODUCT), ("rule0", K_RULE0), ("never", K_NEVER), ("scalar", K_SCALAR), ("leaves", K_LEAVES),
                      ("leaf_inner", K_LEAF_INNER), ("join", K_JOIN)):
        v, s = np.zeros(nptn * B), np.zeros(nptn, dtype=np.int16)
        assert lib.iqhip_fetch_partial(e, key, v.ctypes.data_as(DP)) == 0, lib.iqhip_last_error()
        assert lib.iqhip_fetch_scale_num(e, key, s.ctypes.data_as(I16P)) == 0, lib.iqhip_last_error()
        vec[name], cnt[name] = sha(v), [int(x) for x in s]
    # the cases are in the alignment: what the three rules count at the node, pattern by pattern
    base = sc[0] + sc[1] + sc[2]
    ev = {name: np.asarray(cnt[name]) - base for name in ("rule0", "never", "scalar")}
    assert not ev["never"].any()
    for p in list(ZERO_PTN) + [ZERO_INVAR_PTN]:
        assert ev["scalar"][p] == 4
    assert ev["scalar"][DENORMAL_PTN] == 1 and ev["scalar"][TINY_PTN] == 1 and ev["scalar"][TINY_INVAR_PTN] == 0
    assert ev["rule0"][TINY_PTN] == 1 and ev["rule0"][TINY_INVAR_PTN] == 0 and ev["rule0"][ZERO_INVAR_PTN] == 0
    a, b = pkg.leaf_end(3), pkg.key_end(K_JOIN)
    lnl, df, ddf = C.c_double(), C.c_double(), C.c_double()
    assert lib.iqhip_branch_lnl(e, a, b, 0.17, C.byref(lnl)) == 0, lib.iqhip_last_error()
    plh = np.zeros(nptn)
    assert lib.iqhip_fetch_pattern_lh(e, plh.ctypes.data_as(DP)) == 0, lib.iqhip_last_error()
    assert lib.iqhip_compute_theta(e, a, b) == 0, lib.iqhip_last_error()
    assert lib.iqhip_derv(e, 0.17, C.byref(df), C.byref(ddf)) == 0, lib.iqhip_last_error()
    emit("table", label, env=env, tree_lnl=hx(tree_lnl), vectors=vec, scale_num=cnt, sum_scale=[hx(x) for x in ss], lnl=hx(lnl.value),
         pattern_lh=[hx(x) for x in plh], df=hx(df.value), ddf=hx(ddf.value), launch=launch_of(n, ncomp, nclass, nptn, ntaxa, ops, K_CHILD))
    t.close()


# ---- (b) chains, (c) the sweep
def chain_inputs(n, ncat, nclass, caterpillar):
    model = model_for(n, ncat, nclass, 41)
    nwk = synth.random_tree_newick(NTAXA_CHAIN, 77 + n, 0.4, 0.9, caterpillar)
    sim = model.classes[0] if nclass > 1 else model
    states = synth.simulate_alignment(nwk, sim, NPTN[n], 78 + n, 0.02, SU[n])
    return model, nwk, np.ascontiguousarray(states), np.arange(1, NPTN[n] + 1, dtype=np.float64) % 4 + 1


def dry_plan(nwk, n, states, freq, model):
    t = pkg.PhyloTree(nwk)
    t.set_alignment(n, SEQ_TYPE[n], states, freq)
    t.set_model(model)
    t.set_dry_run(True)
    t.clear_all_partial_lh()
    t.compute_likelihood()
    ops = node_ops([(p["dst_key"], p["left_key"], p["right_key"], p["left_leaf"], p["right_leaf"], p["left_len"], p["right_len"],
                     p["flags"], 0) for p in t.last_plan()])
    t.close()
    return ops


def chain_case(label, n, ncat, nclass, env, caterpillar):
    set_env(env)
    model, nwk, states, freq = chain_inputs(n, ncat, nclass, caterpillar)
    t = device_tree(nwk, n, states, freq, None, model)
    t.clear_all_partial_lh()
    lnl, plh = t.compute_likelihood(want_pattern_lh=True)
    a, b = t.current_branch()
    vecs, counts, factors, deepest = [], [], [], (0, 0)
    for x in range(t.num_nodes):
        for y, _ in t.neighbors(x):
            info = t.neighbor_info(x, y)
            if len(t.neighbors(y)) == 1 or not (info["computed"] & 1) or info["key"] == 0:
                continue
            vecs.append(t.fetch_partial(x, y))
            counts.append(t.fetch_scale_num(x, y))
            factors.append(info["lh_scale_factor"])
            deepest = max(deepest, (int(counts[-1].min()), int(counts[-1].max())))
    assert len(vecs) >= NTAXA_CHAIN - 2 and deepest[1] >= 1, (len(vecs), deepest)  # rescaled values were consumed (range printed)
    t.reset_theta()
    df, ddf = t.compute_likelihood_derv(a, b)
    emit("chain", label + ("-caterpillar" if caterpillar else "-random"), env=env, lnl=hx(lnl), pattern_lh=sha(plh), nvectors=len(vecs),
         vectors=sha(*vecs), scale_num=sha(*counts), scale_num_range_deepest=list(deepest), lh_scale_factors=sha(np.asarray(factors)),
         df=hx(df), ddf=hx(ddf), launch=launch_of(n, len(model.rates), nclass, NPTN[n], NTAXA_CHAIN, dry_plan(nwk, n, states, freq, model)))
    t.close()


def sweep_case():
    set_env({})
    model, nwk, states, freq = chain_inputs(4, 4, 1, True)
    t = device_tree(nwk, 4, states, freq, None, model)
    t.set_device_newton(True)
    t.set_device_sweep(True)
    t.clear_all_partial_lh()
    lnl = t.optimize_all_branches(iterations=1, tolerance=1e-9)
    lens = [[x, y, hx(ln)] for x in range(t.num_nodes) for y, ln in t.neighbors(x) if x < y]
    paths = {k: v for k, v in t.path_counts().items() if v}
    assert paths.get("sweep_persistent", 0) >= 1, paths           # k_sweep4 ran
    emit("sweep", "t4-c4-caterpillar", lnl=hx(lnl), lengths=lens, paths=paths)
    t.close()


def main():
    if lib.iqhip_device_count() < 1:
        raise SystemExit("traverse_bits.py: no HIP device visible")
    for case in TABLE_CASES:
        table_case(*case)
    for case in CHAIN_CASES:
        for caterpillar in (True, False):
            chain_case(*case, caterpillar)
    sweep_case()


if __name__ == "__main__":
    main()
