"""GPU: k_traverse4 answers leaf-leaf node updates from pair tables and writes no vector for them (DESIGN.md 3.1 "Pair
children"; plan.hip select_pair_children, CHILD_PAIR).

The bit reference needs no switch: a one-op plan is never virtualised (its only op is the plan's last), so a second engine
driven ONE OP PER SUBMISSION computes every vector and every counter array the old way.  Everything fetched from the engine
under test -- the virtual vectors included, which a fetch expands -- must have the same bytes.

Lane forms (engine.hip configure_engine): one lane per pattern (SP = 1) for an odd category count, and for an even one under
IQHIP_LANE_SPLIT=1; two lanes per pattern (SP = 2) for an even category count at these pattern counts (the default: every
wave of the alignment fits the chip at once).  FORMS lists (ncat, IQHIP_LANE_SPLIT or None)."""
import ctypes as C

import numpy as np
import pytest

from test_parity_gpu import LNL_RTOL

pytestmark = pytest.mark.gpu

DP = C.POINTER(C.c_double)
FORMS = [(1, None), (2, None), (4, None), (4, "1"), (2, "1")]
NPTN = [130, 1]   # two full 64-pattern tiles and a partial one; a single pattern


def dptr(a):
    return a.ctypes.data_as(DP)


def bind(lib):
    lib.iqhip_debug_pair_children.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    lib.iqhip_debug_pair_children.restype = C.c_int
    return lib


def pair_counts(lib, eng):
    """(ops removed so far, slabs expanded so far, ops the last plan removed)"""
    a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
    assert bind(lib).iqhip_debug_pair_children(eng, C.byref(a), C.byref(b), C.byref(c)) == 0
    return a.value, b.value, c.value


def make_tree(pkg, nwk, states, model, freq=None, n_unobs=0, nsites=0, mem_mode=None):
    t = pkg.PhyloTree(nwk)
    if mem_mode is not None:
        t.set_mem_mode(mem_mode)
    t.set_alignment(4, pkg.SEQ_DNA, states, np.ones(states.shape[1]) if freq is None else freq)
    t.set_model(model)
    t.set_likelihood_kernel(pkg.LK_EIGEN_HIP)
    t.attach_engine(0)
    if n_unobs:
        t.set_ascertainment(n_unobs, nsites)
    return t


def node_ops(pkg, plan):
    ops = (pkg.NodeOp * len(plan))()
    for k, p in enumerate(plan):
        ops[k] = pkg.NodeOp(p["dst_key"], p["left_key"], p["right_key"], p["left_leaf"], p["right_leaf"], p["left_len"],
                            p["right_len"], p["flags"], 0)
    return ops


def one_op_at_a_time(pkg, lib, eng, plan):
    """the reference: every op a submission of its own; returns sum_scale per op"""
    ss = np.zeros(len(plan))
    for k, p in enumerate(plan):
        s = C.c_double(-1.0)
        assert lib.iqhip_update_partials(eng, node_ops(pkg, [p]), 1, C.byref(s)) == 0, lib.iqhip_last_error()
        ss[k] = s.value
    return ss


def fetch(lib, t, key):
    v = np.zeros(t.nptn * t.block)
    sc = np.zeros(t.nptn, dtype=np.int16)
    assert lib.iqhip_fetch_partial(t.engine, C.c_uint64(key), dptr(v)) == 0, lib.iqhip_last_error()
    assert lib.iqhip_fetch_scale_num(t.engine, C.c_uint64(key), sc.ctypes.data_as(C.POINTER(C.c_int16))) == 0, lib.iqhip_last_error()
    return v.tobytes(), sc.tobytes()


def same_vectors(lib, a, b, plan):
    for p in plan:
        va, vb = fetch(lib, a, p["dst_key"]), fetch(lib, b, p["dst_key"])
        assert va[0] == vb[0], ("vector", p["dst"])
        assert va[1] == vb[1], ("scale_num", p["dst"])


def cherries(plan):
    return [k for k, p in enumerate(plan) if p["left_leaf"] >= 0 and p["right_leaf"] >= 0]


def states_of(synth, nwk, model, nptn, seed, missing=0.0):
    return synth.simulate_alignment(nwk, model, nptn, seed, missing, 18)


def traverse_both(pkg, synth, monkeypatch, nwk, states, ncat, split, **kw):
    """tree A evaluates its likelihood the ordinary way (one plan); the engine of tree B gets A's op list one op per
    submission.  Returns (A, B, plan, lnL of A, the reference's sum_scale per op)."""
    if split:
        monkeypatch.setenv("IQHIP_LANE_SPLIT", split)
    lib = pkg.libiqhip()
    model = synth.gtr_model(alpha=0.7, ncat=ncat)
    A, B = make_tree(pkg, nwk, states, model, **kw), make_tree(pkg, nwk, states, model, **kw)
    A.clear_all_partial_lh()
    lnl = A.compute_likelihood()
    plan = A.last_plan()
    ss_ref = one_op_at_a_time(pkg, lib, B.engine, plan)
    return A, B, plan, lnl, ss_ref


@pytest.mark.parametrize("nptn", NPTN)
@pytest.mark.parametrize("ncat,split", FORMS)
@pytest.mark.parametrize("shape", ["random", "caterpillar"])
def test_full_traversal_matches_one_op_at_a_time(pkg, synth, oracle, monkeypatch, shape, ncat, split, nptn):
    """case 1 (and 2: the random 14-taxon tree has parents of two cherries and of a cherry and a leaf; the caterpillar's one
    cherry hangs below a parent whose other child is a leaf)"""
    lib = pkg.libiqhip()
    nwk = synth.random_tree_newick(14, 8) if shape == "random" else synth.random_tree_newick(8, 11, caterpillar=True)
    states = states_of(synth, nwk, synth.gtr_model(alpha=0.7, ncat=ncat), nptn, 5)
    A, B, plan, lnl, _ = traverse_both(pkg, synth, monkeypatch, nwk, states, ncat, split)
    try:
        removed = pair_counts(lib, A.engine)[2]
        assert removed >= 1 and removed <= len(cherries(plan))
        plh_a = A.fetch_pattern_lh()
        same_vectors(lib, A, B, plan)
        # the same root branch again, now from vectors in memory (all expanded by the fetches above)
        assert A.compute_likelihood_branch(*A.current_branch()) == lnl
        assert A.fetch_pattern_lh().tobytes() == plh_a.tobytes()
        ot = oracle.OracleTree(nwk, 4, oracle.SEQ_DNA, states, np.ones(nptn), None, synth.gtr_model(alpha=0.7, ncat=ncat))
        ref, _ = ot.likelihood()
        assert abs(lnl - ref) <= LNL_RTOL * abs(ref)
        if shape == "random":
            kinds = set()
            dst_of_cherry = {plan[k]["dst_key"] for k in cherries(plan)}
            for p in plan:
                lc = p["left_leaf"] < 0 and p["left_key"] in dst_of_cherry
                rc = p["right_leaf"] < 0 and p["right_key"] in dst_of_cherry
                if lc and rc:
                    kinds.add("two")
                elif (lc and p["right_leaf"] >= 0) or (rc and p["left_leaf"] >= 0):
                    kinds.add("one+leaf")
            assert kinds == {"two", "one+leaf"}, kinds
    finally:
        A.close()
        B.close()


def test_pattern_lh_and_lnl_match_an_engine_without_pair_children(pkg, synth, monkeypatch):
    """lnL and _pattern_lh byte-identical: the reference engine evaluates the same root branch from op-by-op vectors"""
    lib = pkg.libiqhip()
    nwk = synth.random_tree_newick(12, 3)
    states = states_of(synth, nwk, synth.gtr_model(alpha=0.7, ncat=4), 130, 9, missing=0.05)
    A, B, plan, lnl, _ = traverse_both(pkg, synth, monkeypatch, nwk, states, 4, "1")
    try:
        assert pair_counts(lib, A.engine)[2] >= 1
        plh = A.fetch_pattern_lh().tobytes()
        a, b = A.current_branch()
        ln = dict(A.neighbors(a))[b]
        by_dst = {tuple(p["dst"]): p["dst_key"] for p in plan}
        nl = A.num_leaves

        def end(frm, to):   # the vector at `to` seen from `frm`; a leaf end has none
            if to < nl:
                return pkg.leaf_end(to)
            key = by_dst.get((frm, to), by_dst.get((to, frm)))
            assert key is not None
            return pkg.key_end(key)

        # whichever order the engine wants its ends in: the engine under test must reproduce its own lnL with them before the
        # reference is asked
        ends = None
        for ea, eb in ((end(a, b), end(b, a)), (end(b, a), end(a, b))):
            out = C.c_double()
            if lib.iqhip_traverse_lnl(A.engine, None, 0, ea, eb, ln, None, C.byref(out)) == 0 and out.value == lnl:
                ends = (ea, eb)
                break
        assert ends is not None, (a, b)
        out = C.c_double()
        assert lib.iqhip_traverse_lnl(B.engine, None, 0, ends[0], ends[1], ln, None, C.byref(out)) == 0, lib.iqhip_last_error()
        assert np.float64(out.value).tobytes() == np.float64(lnl).tobytes()
        assert B.fetch_pattern_lh().tobytes() == plh
    finally:
        A.close()
        B.close()


def test_missing_data_and_an_ambiguity_code_keeps_its_cherry_real(pkg, synth, monkeypatch):
    """case 3: codes with row 4 (missing data) are answered from the table; a leaf with an IUPAC code keeps its cherry real"""
    lib = pkg.libiqhip()
    nwk = synth.random_tree_newick(12, 3)
    model = synth.gtr_model(alpha=0.7, ncat=4)
    states = states_of(synth, nwk, model, 130, 9, missing=0.2)
    assert (states == 18).any()
    A, B, plan, _, _ = traverse_both(pkg, synth, monkeypatch, nwk, states, 4, None)
    try:
        n_plain = pair_counts(lib, A.engine)[2]
        assert n_plain >= 2
        same_vectors(lib, A, B, plan)
    finally:
        A.close()
        B.close()
    leaf = plan[cherries(plan)[0]]["left_leaf"]
    states2 = states.copy()
    states2[leaf, 7] = 5    # an ambiguity code (A or G)
    A, B, plan2, _, _ = traverse_both(pkg, synth, monkeypatch, nwk, states2, 4, None)
    try:
        with_leaf = [k for k in cherries(plan2) if leaf in (plan2[k]["left_leaf"], plan2[k]["right_leaf"])]
        assert len(with_leaf) == 1
        assert pair_counts(lib, A.engine)[2] == n_plain - 1
        same_vectors(lib, A, B, plan2)
    finally:
        A.close()
        B.close()


def raw_plan(cherry_lens=(0.1, 0.2)):
    """leaves 0, 1 -> 101; (101, uploaded 900) -> 102; (102, leaf 2) -> 103: the parent of the cherry is 102"""
    def op(dst, lk, rk, ll, rl, a, b):
        return dict(dst_key=dst, left_key=lk, right_key=rk, left_leaf=ll, right_leaf=rl, left_len=a, right_len=b, flags=0, dst=(dst,))
    return [op(101, 0, 0, 0, 1, *cherry_lens), op(102, 101, 900, -1, -1, 0.05, 0.07), op(103, 102, 0, -1, 2, 0.11, 0.13)]


def upload_tiny(lib, t, key, scale):
    rng = np.random.default_rng(4)
    v = rng.uniform(0.1, 1.0, size=t.nptn * t.block) * scale
    sc = np.zeros(t.nptn, dtype=np.int16)
    assert lib.iqhip_upload_partial(t.engine, C.c_uint64(key), dptr(v), sc.ctypes.data_as(C.POINTER(C.c_int16))) == 0, lib.iqhip_last_error()


@pytest.mark.parametrize("ncat,split", [(4, None), (4, "1"), (1, None)])
def test_the_parent_of_a_virtual_cherry_rescales_and_stale_rows_read_zero(pkg, synth, monkeypatch, ncat, split):
    """cases 4, 5 and 9.  The parent's other child is an uploaded vector of magnitude 2^-300, so the parent's maximum is below
    2^-256 for every pattern: it must apply the scaling rule on its real maximum (a pair child is no tip for that rule).  The
    reference here is the engine that runs one op per submission (PAIR + streamed child); the oracle-chosen tree, PAIR + previous
    result, is test_scaling_at_the_parent_of_a_virtual_cherry_against_the_oracle.
    With the cherry removed two ops are left of the three: the plan travels in the kernel arguments (kSmallPlanOps).
    Stale rows: the first submission leaves a non-zero sum_scale in row 1 of the wave-partial slab; in the second one rows 0
    and 1 belong to removed ops, whose sums must read exactly 0.0."""
    if split:
        monkeypatch.setenv("IQHIP_LANE_SPLIT", split)
    lib = pkg.libiqhip()
    nwk = synth.random_tree_newick(5, 3)
    model = synth.gtr_model(alpha=0.7, ncat=ncat)
    states = states_of(synth, nwk, model, 130, 9, missing=0.1)
    A, B = make_tree(pkg, nwk, states, model), make_tree(pkg, nwk, states, model)
    try:
        for t in (A, B):
            upload_tiny(lib, t, 900, 2.0 ** -300)
        plan = raw_plan()
        ss = np.full(3, -1.0)
        assert lib.iqhip_update_partials(A.engine, node_ops(pkg, plan), 3, dptr(ss)) == 0, lib.iqhip_last_error()
        assert pair_counts(lib, A.engine)[2] == 1
        ss_ref = one_op_at_a_time(pkg, lib, B.engine, plan)
        assert ss_ref[0] == 0.0 and ss_ref[1] < 0.0          # the parent rescaled in the reference ...
        assert ss.tobytes() == ss_ref.tobytes()                # ... and here, to the same sum; the removed op's row is 0.0
        sc = np.frombuffer(fetch(lib, B, 102)[1], dtype=np.int16)
        assert (sc == 1).all()
        same_vectors(lib, A, B, plan)
        # row 1 of the wave-partial slab now holds the parent's non-zero sum.  The same three ops (other pendant lengths) behind a
        # second cherry of leaves 3 and 4, whose consumer closes the plan: rows 0 and 1 belong to removed ops
        lead = dict(raw_plan()[0], dst_key=201, left_leaf=3, right_leaf=4)
        lead_top = dict(raw_plan()[2], dst_key=203, left_key=201, right_leaf=2)
        plan3 = [lead] + raw_plan((0.3, 0.4)) + [lead_top]
        ss3 = np.full(5, -1.0)
        assert lib.iqhip_update_partials(A.engine, node_ops(pkg, plan3), 5, dptr(ss3)) == 0, lib.iqhip_last_error()
        assert pair_counts(lib, A.engine)[2] == 2
        ss3_ref = one_op_at_a_time(pkg, lib, B.engine, plan3)
        assert ss3[0] == 0.0 and ss3[1] == 0.0 and ss3_ref[2] < 0.0
        assert ss3.tobytes() == ss3_ref.tobytes()
        same_vectors(lib, A, B, plan3)
    finally:
        A.close()
        B.close()


def deep_cherry_newick(ntaxa, seed):
    """a caterpillar of taxa 0 .. ntaxa - 6 joined with the cherry (ntaxa - 5, ntaxa - 4); above that join the leaf ntaxa - 3 and
    a second cherry, where the traversal is rooted.  Seen from there the join is an INTERNAL-INTERNAL node whose children are
    a cherry and the previous result (the long chain)"""
    rng = np.random.default_rng(seed)

    def ln():
        return "%.6f" % rng.uniform(0.02, 0.2)
    cat = "(0:%s,1:%s)" % (ln(), ln())
    for t in range(2, ntaxa - 5):
        cat = "(%s:%s,%d:%s)" % (cat, ln(), t, ln())
    return "((%d:%s,%d:%s):%s,%d:%s,((%d:%s,%d:%s):%s,%s:%s):%s);" % (
        ntaxa - 1, ln(), ntaxa - 2, ln(), ln(), ntaxa - 3, ln(), ntaxa - 5, ln(), ntaxa - 4, ln(), ln(), cat, ln(), ln())


@pytest.mark.parametrize("split", [None, "1"])
def test_scaling_at_the_parent_of_a_virtual_cherry_against_the_oracle(pkg, synth, oracle, monkeypatch, split):
    """case 4.  146 taxa, chosen on the CPU with the oracle: the chain below the join is long enough for the join's maximum to
    fall below 2^-256 in some patterns AT the join (5 of 130 with these seeds; 4 more arrive rescaled from the chain).  The
    oracle's counters say so (asserted); the engine's counters at the join are the oracle's, its summed scaling is the
    oracle's to test_parity_gpu.py's bound, and everything is bit-equal to the engine that runs one op per submission."""
    lib = pkg.libiqhip()
    nptn, ncat = 130, 4
    nwk = deep_cherry_newick(146, 3)
    model = synth.gtr_model(alpha=0.7, ncat=ncat)
    states = states_of(synth, nwk, model, nptn, 5)
    A, B, plan, lnl, _ = traverse_both(pkg, synth, monkeypatch, nwk, states, ncat, split)
    try:
        cherry_keys = {plan[k]["dst_key"] for k in cherries(plan)}
        by_key = {p["dst_key"]: p for p in plan}
        join = [p for p in plan if p["left_leaf"] < 0 and p["right_leaf"] < 0 and (p["left_key"] in cherry_keys) != (p["right_key"] in cherry_keys)]
        assert len(join) == 1
        join = join[0]
        chain = by_key[join["right_key"] if join["left_key"] in cherry_keys else join["left_key"]]
        assert pair_counts(lib, A.engine)[2] == 2        # the chain's first cherry and the one at the join
        ot = oracle.OracleTree(nwk, 4, oracle.SEQ_DNA, states, np.ones(nptn), None, model)
        _, sc_join, sf_join = ot.partial(*join["dst"])
        _, sc_chain, sf_chain = ot.partial(*chain["dst"])
        own = sc_join - sc_chain                             # (the cherry's counters are zero)
        assert (own != 0).any() and sf_join - sf_chain < 0.0, "the oracle does not rescale at the cherry's parent"
        assert np.array_equal(A.fetch_scale_num(*join["dst"]), sc_join)
        assert np.array_equal(A.fetch_scale_num(*chain["dst"]), sc_chain)
        for dst, sf in ((join["dst"], sf_join), (chain["dst"], sf_chain)):
            assert abs(A.neighbor_info(*dst)["lh_scale_factor"] - sf) <= 1e-12 * max(1.0, abs(sf))   # test_parity_gpu.py:49
        own_sum = A.neighbor_info(*join["dst"])["lh_scale_factor"] - A.neighbor_info(*chain["dst"])["lh_scale_factor"]
        assert abs(own_sum - (sf_join - sf_chain)) <= 1e-12 * abs(sf_join)
        ref, _ = ot.likelihood()
        assert abs(lnl - ref) <= LNL_RTOL * abs(ref)
        same_vectors(lib, A, B, plan)
    finally:
        A.close()
        B.close()


# patterns that count in the lifecycle test; one more column follows them.  Two full tiles, so that the extra column has a wave
# to itself in both lane forms: a wave that holds an ambiguity code evaluates ALL its leaf children on the fly (leaf_cat4's
# wave-uniform slow path), which is not the table's association, and would move its neighbours' last bits in the reference
NLIFE = 128


def lifecycle_trees(pkg, synth, model):
    """A, the engine under test, and R, an engine that can never virtualise, with the SAME numbers: both alignments get a
    129th column of frequency 0 -- plain states in A, an ambiguity code in every taxon of R, so that no row of R is plain and
    its planner removes nothing.  A pattern of frequency 0 adds exactly 0.0 to every sum (lnL, derivatives, sum_scale), in the
    same lane of the same wave on both engines, so every value reduced over patterns has the same bits, and the vectors of
    the first 128 patterns do not depend on the last."""
    nwk = synth.random_tree_newick(10, 6)
    states = states_of(synth, nwk, model, NLIFE, 9, missing=0.05)
    freq = np.concatenate([np.ones(NLIFE), np.zeros(1)])
    trees = []
    for code in (0, 5):   # 5: an ambiguity code (A or G)
        st = np.concatenate([states, np.full((states.shape[0], 1), code, dtype=np.uint8)], axis=1)
        t = make_tree(pkg, nwk, st, model, freq=freq, mem_mode=1)   # LM_ALL_BRANCH: the NNI evaluators need every directed vector
        t.set_device_newton(True)
        t.set_device_sweep(True)
        trees.append(t)
    return trees


def same_state(A, R):
    """every directed vector both trees hold: the same bytes in the patterns that count; the same branch lengths"""
    n = 0
    for a in range(A.num_nodes):
        for b, ln in A.neighbors(a):
            assert np.float64(ln).tobytes() == np.float64(dict(R.neighbors(a))[b]).tobytes(), (a, b)
            ia, ir = A.neighbor_info(a, b), R.neighbor_info(a, b)
            assert (ia["computed"] & 1) == (ir["computed"] & 1), (a, b)
            if b < A.num_leaves or not (ia["computed"] & 1) or ia["key"] == 0:
                continue
            assert A.fetch_partial(a, b)[:NLIFE].tobytes() == R.fetch_partial(a, b)[:NLIFE].tobytes(), ("vector", a, b)
            assert A.fetch_scale_num(a, b)[:NLIFE].tobytes() == R.fetch_scale_num(a, b)[:NLIFE].tobytes(), ("scale_num", a, b)
            n += 1
    assert n > 0


def same_value(x, y):
    assert np.asarray(x, dtype=np.float64).tobytes() == np.asarray(y, dtype=np.float64).tobytes(), (x, y)


def test_lifecycle_on_one_engine(pkg, synth, monkeypatch):
    """case 6, every step compared with an engine that never virtualises (lifecycle_trees): fetch of a virtual vector; the
    cached plan twice with a fetch in between; set_model between traversal and fetch; per-branch and sweep optimisation next to
    a cherry; an NNI batch; a changed cherry length with a partial recompute; a recompute that reads the still valid cherry as
    a memory child; a re-rooted evaluation"""
    lib = pkg.libiqhip()
    model = synth.gtr_model(alpha=0.7, ncat=4)
    model2 = synth.gtr_model(rates6=(1.1, 3.0, 0.7, 1.3, 3.6, 1.0), freqs=(0.30, 0.20, 0.21, 0.29), alpha=0.5, ncat=4)
    A, R = lifecycle_trees(pkg, synth, model)

    def both(f):
        x, y = f(A), f(R)
        assert repr(x) == repr(y), (x, y)
        if isinstance(x, float):
            same_value(x, y)
        assert pair_counts(lib, R.engine)[0] == 0      # the reference has removed nothing, ever
        return x

    def full(t):
        t.clear_all_partial_lh()
        return t.compute_likelihood()

    def raw_fetch_first(t, key):
        v, sc = fetch(lib, t, key)
        B = t.block
        return np.frombuffer(v).reshape(-1, B)[:NLIFE].tobytes(), np.frombuffer(sc, dtype=np.int16)[:NLIFE].tobytes()
    try:
        both(full)
        plan = A.last_plan()
        assert [p["dst_key"] for p in plan] == [p["dst_key"] for p in R.last_plan()]
        ch = plan[cherries(plan)[0]]
        removed, expanded, last = pair_counts(lib, A.engine)
        assert last >= 1 and expanded == 0
        same_value(A.fetch_pattern_lh()[:NLIFE], R.fetch_pattern_lh()[:NLIFE])
        # fetch of a virtual vector expands exactly that one
        assert raw_fetch_first(A, ch["dst_key"]) == raw_fetch_first(R, ch["dst_key"])
        assert pair_counts(lib, A.engine)[1] == 1
        # the cached plan again, a fetch in between, and again
        both(full)
        assert raw_fetch_first(A, ch["dst_key"]) == raw_fetch_first(R, ch["dst_key"])
        both(full)
        same_state(A, R)
        # set_model between the traversal and the fetch: the vector fetched is the old model's
        both(full)
        old = raw_fetch_first(R, ch["dst_key"])
        A.set_model(model2)
        assert raw_fetch_first(A, ch["dst_key"]) == old
        A.set_model(model)
        # per-branch optimisation of the branch above the cherry, on vectors of which some are still pair tables
        both(full)
        dad, node = ch["dst"]
        both(lambda t: t.optimize_one_branch(dad, node, clear_lh=False))
        same_state(A, R)
        # a sweep over all branches
        both(lambda t: t.optimize_all_branches(iterations=1))
        same_state(A, R)
        # an NNI batch (its plans have explicit segments: their cherries stay real, the vectors they read are expanded)
        both(lambda t: t.evaluate_nnis_batch())
        same_state(A, R)
        # a cherry leaf's length changed: the partial recompute removes the cherry again
        leaf = ch["left_leaf"]
        before = pair_counts(lib, A.engine)[0]
        for t in (A, R):
            t.set_branch_length(leaf, t.neighbors(leaf)[0][0], 0.37)
        both(lambda t: t.compute_likelihood())
        plan = A.last_plan()
        at = [k for k, p in enumerate(plan) if p["dst_key"] == ch["dst_key"]]
        # (where the recompute holds the cherry it is removed again, unless it closes the plan or is an end of the branch the
        # likelihood is taken on; from a root on the changed leaf's side the cherry is not needed at all)
        if at:
            stays_real = at[0] == len(plan) - 1 or set(A.current_branch()) == set(ch["dst"])
            assert (pair_counts(lib, A.engine)[0] > before) == (not stays_real)
        same_state(A, R)
        # the branch from the cherry's grandparent to the cherry's sibling changes: the grandparent's side is recomputed and
        # reads the cherry, still valid and still a pair table, as a memory child -- which expands it
        both(full)
        plan = A.last_plan()
        ch = plan[cherries(plan)[0]]
        up = next(p for p in plan if ch["dst_key"] in (p["left_key"], p["right_key"]) and (p["left_leaf"] < 0 or p["right_leaf"] < 0))
        q = ch["dst"][0]
        sib = next(b for b, _ in A.neighbors(q) if b not in (ch["dst"][1], up["dst"][0]))
        expanded = pair_counts(lib, A.engine)[1]
        for t in (A, R):
            t.set_branch_length(q, sib, 0.29)
        both(lambda t: t.compute_likelihood())
        assert ch["dst_key"] not in [p["dst_key"] for p in A.last_plan()]          # not recomputed ...
        assert pair_counts(lib, A.engine)[1] > expanded                            # ... but read from memory
        same_state(A, R)
        # a re-rooted evaluation: the likelihood on the cherry's own branch, seen from the other side
        both(lambda t: t.compute_likelihood_branch(*ch["dst"]))
        same_state(A, R)
    finally:
        A.close()
        R.close()


def test_asc_engine(pkg, synth, monkeypatch):
    """case 7: unobserved constant patterns appended (+ASC)"""
    lib = pkg.libiqhip()
    nwk = synth.random_tree_newick(9, 5)
    model = synth.gtr_model(alpha=0.9, ncat=4)
    st = synth.simulate_alignment(nwk, model, 200, 6)
    st = st[:, [s for s in range(st.shape[1]) if len(set(st[:, s].tolist())) > 1]]
    pat, freq = synth.compress_patterns(st)
    pat = np.concatenate([pat, np.tile(np.arange(4, dtype=np.uint8), (9, 1))], axis=1)
    freq = np.concatenate([freq, np.zeros(4)])
    kw = dict(freq=freq, n_unobs=4, nsites=int(freq.sum()))
    model = synth.gtr_model(alpha=0.7, ncat=4)
    A, B = make_tree(pkg, nwk, pat, model, **kw), make_tree(pkg, nwk, pat, model, **kw)
    try:
        A.clear_all_partial_lh()
        la = A.compute_likelihood()
        plan = A.last_plan()
        assert pair_counts(lib, A.engine)[2] >= 1
        one_op_at_a_time(pkg, lib, B.engine, plan)
        same_vectors(lib, A, B, plan)
        assert A.compute_likelihood_branch(*A.current_branch()) == la
    finally:
        A.close()
        B.close()


def test_multifurcating_tree_keeps_its_intermediate_products_real(pkg, synth, monkeypatch):
    """case 8: IQHIP_OP_NO_SCALE / IQHIP_OP_SCALAR_RULE leaf-leaf ops stay real"""
    lib = pkg.libiqhip()
    nwk = synth.random_multifurcating_newick(12, 43)
    model = synth.gtr_model(alpha=0.7, ncat=4)
    states = states_of(synth, nwk, model, 130, 9)
    A, B = make_tree(pkg, nwk, states, model), make_tree(pkg, nwk, states, model)
    try:
        A.clear_all_partial_lh()
        A.compute_likelihood()
        plan = A.last_plan()
        flagged = [k for k in cherries(plan) if plan[k]["flags"] & 3]
        plain = [k for k in cherries(plan) if not plan[k]["flags"] & 3]
        assert flagged, "the tree has no leaf-leaf intermediate product"
        assert pair_counts(lib, A.engine)[2] <= len(plain)
        one_op_at_a_time(pkg, lib, B.engine, plan)
        same_vectors(lib, A, B, plan)
    finally:
        A.close()
        B.close()
