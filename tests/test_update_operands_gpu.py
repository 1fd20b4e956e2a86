"""GPU: the bits of k_traverse4's node update (kernels_valu4.hip node_update4 / leaf_cat4) at every category count, in all 24
instantiations of the kernel, against recorded values (DESIGN.md 3.1 "Operand homes").

Where the node update takes U, U^-1 and the op's dst pointer from -- the constant address space as now, pinned scalar
registers, vector registers -- is a question of speed only: every product and fma keeps its operands and its order, so no
bit may change.  The expected values are therefore RECORDED ONES: tests/golden/update_operands/ holds, per case, what the
kernel left behind in the commit BEFORE the one that added this test -- lnL and every sum_scale as float.hex(), pattern_lh,
every vector and every scale counter as the sha256 of their bytes.  The commit that added the test (the pointers to the
matrices pinned) and the four other homes it measured and dropped (profiles/r09/experiments.txt) all reproduce them.
To record again, from a build that is known to be right:

    IQHIP_RECORD_UPDATE_OPERANDS=<directory> python -m pytest -m gpu tests/test_update_operands_gpu.py

writes <directory>/<case>.json instead of comparing.

Shape: 14 taxa x 150 patterns (three 64-pattern tiles, the last ragged), GTR, a random tree whose plan has a join of two vector
children, a parked (HOLD) operand, leaf + vector ops and pair children; one column holds an IUPAC ambiguity code (the slow leaf
path multiplies by U as well) and a few cells are unknown.  Cases: 1 .. 8 categories, the even counts with one and with two lanes
per pattern (IQHIP_LANE_SPLIT), and each of them twice on one engine: the tree's own traversal with its root branch (no op has two
memory children: HAS_LOAD = false), then the same ops again through iqhip_update_partials with one more op behind them that joins
two vectors of which neither is the previous result (HAS_LOAD = true) -- all 24 instantiations of the kernel."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

from test_plan_check import planner

pytestmark = pytest.mark.gpu

NTAXA, NPTN, TREE_SEED = 14, 150, 8
AMBIG_TAXON, AMBIG_PTN, AMBIG_CODE = 0, 70, 5     # an IUPAC code (4 .. 17) in the second tile
K_EXTRA = 9100001
GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "update_operands")
RECORD_DIR = os.environ.get("IQHIP_RECORD_UPDATE_OPERANDS")
CASES = [(c, sp) for c in range(1, 9) for sp in ((1, 2) if c % 2 == 0 else (1,))]
DP, I16P = C.POINTER(C.c_double), C.POINTER(C.c_int16)


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def node_ops(pkg, rows):
    ops = (pkg.NodeOp * len(rows))()
    for k, r in enumerate(rows):
        ops[k] = pkg.NodeOp(*r)
    return ops


def inputs(synth, ncat):
    model = synth.gtr_model(alpha=0.7, ncat=ncat)
    nwk = synth.random_tree_newick(NTAXA, TREE_SEED)
    states = np.ascontiguousarray(synth.simulate_alignment(nwk, synth.gtr_model(alpha=0.7, ncat=4), NPTN, 5, 0.03, 18))
    states[AMBIG_TAXON, AMBIG_PTN] = AMBIG_CODE
    assert (states == 18).sum() >= 10
    freq = np.arange(1, NPTN + 1, dtype=np.float64) % 4 + 1
    return model, nwk, states, freq


def plan_rows(plan):
    return [(p["dst_key"], p["left_key"], p["right_key"], p["left_leaf"], p["right_leaf"], p["left_len"], p["right_len"],
             p["flags"], 0) for p in plan]


def extra_op(plan):
    """one more op: a join of two inner vectors of the plan that are not pair children (their own children are not both
    leaves), the later of them not the plan's last result -- so it reads both from memory"""
    inner = [p for p in plan[:-1] if p["left_leaf"] < 0 or p["right_leaf"] < 0]
    assert len(inner) >= 2
    return (K_EXTRA, inner[0]["dst_key"], inner[1]["dst_key"], -1, -1, 0.07, 0.13, 0, 0)


def launch_shape(pkg, ncat, rows, states):
    """what the planner makes of this op list under the case's environment"""
    lib, e = planner(pkg, 4, ncat, NPTN, NTAXA)
    try:
        plain = np.array([0 if ((states[t] >= 4) & (states[t] != 18)).any() else 1 for t in range(NTAXA)], dtype=np.uint8)
        assert lib.iqhip_debug_planner_plain_taxa(e, plain.ctypes.data_as(C.POINTER(C.c_uint8))) == 0, lib.iqhip_last_error()
        assert lib.iqhip_debug_plan(e, node_ops(pkg, rows), len(rows)) == 0, lib.iqhip_last_error()
        rec = (C.c_int64 * len(pkg.PLAN_SHAPE_SLOTS))()
        assert lib.iqhip_debug_plan_shape(e, rec, len(rec)) == 0, lib.iqhip_last_error()
        removed = (C.c_int32 * len(rows))()
        assert lib.iqhip_debug_plan_removed(e, removed, len(rows)) == 0, lib.iqhip_last_error()
    finally:
        lib.iqhip_destroy(e)
    return dict(zip(pkg.PLAN_SHAPE_SLOTS, (int(v) for v in rec))), sum(removed)


def check_shape(pkg, ncat, sp, plan, rows, states):
    """the 4-state kernel, the lane form of the case, and the op kinds the case is about"""
    shape, removed = launch_shape(pkg, ncat, rows, states)
    ntiles, wpb = (NPTN + 63) // 64, 4
    assert shape["top_variant"] == -1 and shape["stages"] == 0, shape            # k_traverse4, one launch
    assert shape["top_ngroups"] == (ntiles * sp + wpb - 1) // wpb and shape["top_grid"] == shape["top_ngroups"], shape
    assert shape["nhold"] >= 1, shape                                             # a parked operand
    assert removed >= 1                                                           # a pair child
    made = {p["dst_key"] for p in plan}
    assert any(p["left_leaf"] < 0 and p["right_leaf"] < 0 and p["left_key"] in made and p["right_key"] in made for p in plan)
    assert any((p["left_leaf"] >= 0) != (p["right_leaf"] >= 0) for p in plan)     # leaf + vector


def fetch_key(lib, t, key):
    v, s = np.zeros(t.nptn * t.block), np.zeros(t.nptn, dtype=np.int16)
    assert lib.iqhip_fetch_partial(t.engine, C.c_uint64(key), v.ctypes.data_as(DP)) == 0, lib.iqhip_last_error()
    assert lib.iqhip_fetch_scale_num(t.engine, C.c_uint64(key), s.ctypes.data_as(I16P)) == 0, lib.iqhip_last_error()
    return v, s


def everything(lib, t, keys):
    vecs, counts = zip(*(fetch_key(lib, t, k) for k in keys))
    return {"nvectors": len(keys), "vectors": sha(*vecs), "scale_num": sha(*counts), "each_vector": [sha(v) for v in vecs]}


@pytest.mark.parametrize("ncat,sp", CASES)
def test_node_update_bits_match_the_recorded_ones(pkg, synth, monkeypatch, ncat, sp):
    if ncat % 2 == 0:
        monkeypatch.setenv("IQHIP_LANE_SPLIT", str(sp))     # read when an engine is created
    lib = pkg.libiqhip()
    model, nwk, states, freq = inputs(synth, ncat)
    t = pkg.PhyloTree(nwk)
    try:
        t.set_alignment(4, pkg.SEQ_DNA, states, freq)
        t.set_model(model)
        t.set_likelihood_kernel(pkg.LK_EIGEN_HIP)
        t.attach_engine(0)
        # (1) the tree's own traversal and root branch: HAS_LOAD = false
        t.clear_all_partial_lh()
        lnl, plh = t.compute_likelihood(want_pattern_lh=True)
        plan = t.last_plan()
        keys = [p["dst_key"] for p in plan]
        got = {"lnl": float(lnl).hex(), "pattern_lh": sha(plh), "traversal": everything(lib, t, keys)}
        check_shape(pkg, ncat, sp, plan, plan_rows(plan), states)
        # (2) the same ops and one with two memory children, no root: HAS_LOAD = true
        rows = plan_rows(plan) + [extra_op(plan)]
        ss = np.full(len(rows), -1.0)
        assert lib.iqhip_update_partials(t.engine, node_ops(pkg, rows), len(rows), ss.ctypes.data_as(DP)) == 0, lib.iqhip_last_error()
        got["with_load"] = everything(lib, t, keys + [K_EXTRA])
        got["with_load"]["sum_scale"] = [float(x).hex() for x in ss]
        check_shape(pkg, ncat, sp, plan, rows, states)
        # (both instantiations agree with each other, too; the goldens hold the digests of all vectors together)
        assert got["with_load"].pop("each_vector")[:len(keys)] == got["traversal"].pop("each_vector")
    finally:
        t.close()
    name = "c%d-sp%d.json" % (ncat, sp)
    if RECORD_DIR:
        os.makedirs(RECORD_DIR, exist_ok=True)
        with open(os.path.join(RECORD_DIR, name), "w") as f:
            json.dump(got, f, indent=0, sort_keys=True)
            f.write("\n")
        return
    with open(os.path.join(GOLDEN_DIR, name)) as f:
        want = json.load(f)
    for part in ("lnl", "pattern_lh", "traversal", "with_load"):
        assert got[part] == want[part], (name, part)
