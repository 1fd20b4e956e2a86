"""GPU: k_traverse4 copies each chunk's LDS regions from the engine's fill image (DESIGN.md 3.1 "Fill image"; k_fill4_image,
plan.hip fill_image_submission) instead of computing them in every workgroup.

The bit reference is test_pair_children_gpu.py's and needs no switch: a second engine driven ONE OP PER SUBMISSION.  A one-op
plan travels in the kernel arguments and never has an image, so that engine fills every chunk in the kernel.  The engine under
test submits the whole plan several times in a row: the first submission plans anew and fills in the kernel, the second finds
the plan cached, builds the image and copies it, the later ones copy the image that is there.  After each one every vector and
every scale_num array, lnL, sum_scale and the pattern likelihoods must be the reference's bytes; iqhip_debug_fill_image must
show that images were built and reused, so that no case passes by never taking the copy path."""
import ctypes as C

import numpy as np
import pytest

from test_pair_children_gpu import (cherries, dptr, fetch, make_tree, node_ops, one_op_at_a_time, pair_counts, same_vectors,
                                    states_of)

pytestmark = pytest.mark.gpu

# (ncat, IQHIP_LANE_SPLIT): one lane per pattern for 1, 3 and under "1"; two lanes per pattern for 2 and 4 at these sizes
FORMS = [(1, None), (2, None), (4, None), (4, "1"), (3, None), (8, "1")]
NPTN = [1, 130, 300]   # 300: two workgroups at one lane per pattern -- a workgroup other than the first reads the image
LDS_KB = [None, 12]    # 12: several chunks, and chunk extents that are no multiple of 1 KiB


def counters(lib, eng):
    a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
    assert lib.iqhip_debug_fill_image(eng, C.byref(a), C.byref(b), C.byref(c)) == 0, lib.iqhip_last_error()
    return a.value, b.value, c.value


def ten_taxa(synth, model, nptn, seed=6):
    """10 taxa, at least two cherries; one leaf of a cherry holds an ambiguity code, so that cherry stays a real op while the
    others are answered from pair tables"""
    nwk = synth.random_tree_newick(10, seed)
    states = states_of(synth, nwk, model, nptn, 9, missing=0.05)
    return nwk, states


def with_ambiguity(states, plan):
    ch = cherries(plan)
    assert len(ch) >= 2
    st = states.copy()
    st[plan[ch[0]]["left_leaf"], st.shape[1] // 2] = 5   # A or G
    return st


def root_ends(pkg, lib, A, B, plan, lnl):
    """the ends of A's current root branch as the engine wants them, found on B (which holds every vector): the order in which
    B reproduces `lnl` bit for bit.  Returns (end a, end b, branch length)."""
    a, b = A.current_branch()
    ln = dict(A.neighbors(a))[b]
    by_dst = {tuple(p["dst"]): p["dst_key"] for p in plan}
    nl = A.num_leaves

    def end(frm, to):
        if to < nl:
            return pkg.leaf_end(to)
        key = by_dst.get((frm, to), by_dst.get((to, frm)))
        assert key is not None
        return pkg.key_end(key)

    for ea, eb in ((end(a, b), end(b, a)), (end(b, a), end(a, b))):
        out = C.c_double()
        if lib.iqhip_traverse_lnl(B.engine, None, 0, ea, eb, ln, None, C.byref(out)) == 0 and \
                np.float64(out.value).tobytes() == np.float64(lnl).tobytes():
            return ea, eb, ln
    raise AssertionError("the reference engine does not reproduce lnL %r on the root branch" % lnl)


def full(t):
    t.clear_all_partial_lh()
    return t.compute_likelihood()


def first_plan(pkg, synth, model, nptn, **kw):
    """the op list of the 10-taxon tree and its alignment with the ambiguity code put in (the plan does not depend on states)"""
    nwk, states = ten_taxa(synth, model, nptn)
    t = pkg.PhyloTree(nwk)
    t.set_alignment(4, pkg.SEQ_DNA, states, np.ones(states.shape[1]))
    t.set_model(model)
    t.set_likelihood_kernel(pkg.LK_EIGEN_HIP)
    t.attach_engine(0)
    try:
        full(t)
        plan = t.last_plan()
    finally:
        t.close()
    return nwk, with_ambiguity(states, plan)


_aln = {}


def alignment(pkg, synth, ncat, nptn):
    if (ncat, nptn) not in _aln:
        _aln[ncat, nptn] = first_plan(pkg, synth, synth.gtr_model(alpha=0.7, ncat=ncat), nptn)
    return _aln[ncat, nptn]


@pytest.mark.parametrize("kb", LDS_KB)
@pytest.mark.parametrize("nptn", NPTN)
@pytest.mark.parametrize("ncat,split", FORMS)
def test_repeated_submissions_match_one_op_at_a_time(pkg, synth, monkeypatch, ncat, split, nptn, kb):
    if split:
        monkeypatch.setenv("IQHIP_LANE_SPLIT", split)
    if kb:
        monkeypatch.setenv("IQHIP_LDS_KB", str(kb))
    lib = pkg.libiqhip()
    model = synth.gtr_model(alpha=0.7, ncat=ncat)
    nwk, states = alignment(pkg, synth, ncat, nptn)
    A, B = make_tree(pkg, nwk, states, model), make_tree(pkg, nwk, states, model)
    try:
        lnl = full(A)                                   # submission 1: planned anew, filled in the kernel
        plan = A.last_plan()
        assert counters(lib, A.engine)[:2] == (0, 0)
        removed = pair_counts(lib, A.engine)[2]
        assert 1 <= removed < len(cherries(plan))       # a pair child in the image, and a cherry that stayed real
        ss_ref = one_op_at_a_time(pkg, lib, B.engine, plan)
        ea, eb, ln = root_ends(pkg, lib, A, B, plan, lnl)
        plh_ref = B.fetch_pattern_lh().tobytes()
        assert counters(lib, B.engine) == (0, 0, 0)     # the reference never had an image
        same_vectors(lib, A, B, plan)
        ops = node_ops(pkg, plan)
        for _ in range(3):
            ss = np.full(len(plan), -1.0)
            out = C.c_double()
            assert lib.iqhip_traverse_lnl(A.engine, ops, len(plan), ea, eb, ln, dptr(ss), C.byref(out)) == 0, lib.iqhip_last_error()
            assert np.float64(out.value).tobytes() == np.float64(lnl).tobytes()
            assert ss.tobytes() == ss_ref.tobytes()
            assert A.fetch_pattern_lh().tobytes() == plh_ref
            same_vectors(lib, A, B, plan)
        built, reused, nbytes = counters(lib, A.engine)
        assert built >= 1 and reused >= 1 and built + reused >= 2, (built, reused)
        assert nbytes > 0
    finally:
        A.close()
        B.close()


def compare_with_a_fresh_reference(pkg, lib, A, nwk, states, model, lnl, **kw):
    plan = A.last_plan()
    B = make_tree(pkg, nwk, states, model, **kw)
    try:
        one_op_at_a_time(pkg, lib, B.engine, plan)
        root_ends(pkg, lib, A, B, plan, lnl)            # (asserts lnL)
        assert A.fetch_pattern_lh().tobytes() == B.fetch_pattern_lh().tobytes()
        same_vectors(lib, A, B, plan)
    finally:
        B.close()


def test_lengths_and_model_change_between_submissions(pkg, synth, monkeypatch):
    lib = pkg.libiqhip()
    model = synth.gtr_model(alpha=0.7, ncat=4)
    model2 = synth.gtr_model(rates6=(1.1, 3.0, 0.7, 1.3, 3.6, 1.0), freqs=(0.30, 0.20, 0.21, 0.29), alpha=0.5, ncat=4)
    nwk, states = alignment(pkg, synth, 4, 130)
    A = make_tree(pkg, nwk, states, model)
    try:
        for _ in range(3):
            lnl = full(A)
        assert counters(lib, A.engine)[:2] == (1, 1)
        compare_with_a_fresh_reference(pkg, lib, A, nwk, states, model, lnl)
        # one pendant and one internal branch get another length: a new plan, then its image
        plan = A.last_plan()
        leaf = plan[cherries(plan)[1]]["left_leaf"]
        A.set_branch_length(leaf, A.neighbors(leaf)[0][0], 0.37)
        inner = next(p for p in plan if p["left_leaf"] < 0 and p["right_leaf"] < 0)
        A.set_branch_length(inner["dst"][1], next(b for b, _ in A.neighbors(inner["dst"][1]) if b >= A.num_leaves and b != inner["dst"][0]), 0.29)
        for want in ((1, 1), (2, 1), (2, 2)):
            lnl = full(A)
            assert counters(lib, A.engine)[:2] == want
            compare_with_a_fresh_reference(pkg, lib, A, nwk, states, model, lnl)
        # another model under the cached plan: the image is built again at the next submission
        A.set_model(model2)
        for want in ((3, 2), (3, 3)):
            lnl = full(A)
            assert counters(lib, A.engine)[:2] == want
            compare_with_a_fresh_reference(pkg, lib, A, nwk, states, model2, lnl)
    finally:
        A.close()


@pytest.mark.parametrize("nptn", [1, 130])
def test_staged_plan(pkg, synth, monkeypatch, nptn):
    """50 taxa on a small alignment: the plan is cut into units that run as launches of their own.  plan.hip unit_target stages
    a 4-state plan while the alignment is at most one wave per SIMD, so the smallest staged alignment is a single pattern;
    130 patterns (three tiles, a partial one) as well, so that more than one wave copies each unit's chunks.  A real engine has
    no query for its plan's shape: that the op list is staged is asserted on a planning-only engine of the same shape and the
    planner's default of 256 CUs, the device's count."""
    from test_plan_check import planner
    lib = pkg.libiqhip()
    model = synth.gtr_model(alpha=0.7, ncat=4)
    nwk = synth.random_tree_newick(50, 41)
    states = states_of(synth, nwk, model, nptn, 9, missing=0.05)
    A = make_tree(pkg, nwk, states, model)
    try:
        for _ in range(3):
            lnl = full(A)
            compare_with_a_fresh_reference(pkg, lib, A, nwk, states, model, lnl)
        assert counters(lib, A.engine)[:2] == (1, 1)
        plan = A.last_plan()
        _, e = planner(pkg, 4, 4, nptn, 50)
        try:
            assert lib.iqhip_debug_plan(e, node_ops(pkg, plan), len(plan)) == 0, lib.iqhip_last_error()
            shape = (C.c_int64 * len(pkg.PLAN_SHAPE_SLOTS))()
            assert lib.iqhip_debug_plan_shape(e, shape, len(shape)) == 0
            assert shape[5] >= 1, "the plan is not staged"
        finally:
            lib.iqhip_destroy(e)
    finally:
        A.close()


def branch_batch(pkg, lib, t, plan, ends):
    """two branch tasks in one submission of explicit segments (iqhip_optimize_branch_batch): each recomputes the vector at
    one end of the root branch into a scratch key, with a pendant length of its own, and optimises the root branch from there.
    Returns the bytes of (results, sum_scale, the two scratch vectors and their counters)."""
    ea, eb, ln = ends
    keyed, other = (ea, eb) if ea.leaf < 0 else (eb, ea)
    src = next(p for p in plan if p["dst_key"] == keyed.key)
    ops, tasks = [], (pkg.BranchTask * 2)()
    for q in range(2):
        scratch = 7000 + q
        ops.append(node_ops(pkg, [dict(src, dst_key=scratch, left_len=src["left_len"] + 0.01 * (q + 1))]))
        tasks[q] = pkg.BranchTask(C.cast(ops[q], C.c_void_p), 1, 10, pkg.key_end(scratch), other, ln, 1e-6, 10.0, 1e-6)
    res = (pkg.BranchResult * 2)()
    ss = np.full(2, -1.0)
    lib.iqhip_optimize_branch_batch.argtypes = [C.c_void_p, C.POINTER(pkg.BranchTask), C.c_int, C.POINTER(C.c_double),
                                                C.POINTER(pkg.BranchResult)]
    assert lib.iqhip_optimize_branch_batch(t.engine, tasks, 2, dptr(ss), res) == 0, lib.iqhip_last_error()
    return bytes(res), ss.tobytes(), fetch(lib, t, 7000), fetch(lib, t, 7001)


def test_explicit_segments_batch_twice(pkg, synth, monkeypatch):
    """the same batch of branch tasks three times: planned anew, image built, image reused.  The reference is a fresh engine's
    first batch, which plans anew and fills in the kernel."""
    lib = pkg.libiqhip()
    model = synth.gtr_model(alpha=0.7, ncat=4)
    nwk, states = alignment(pkg, synth, 4, 130)
    A, R, B = (make_tree(pkg, nwk, states, model) for _ in range(3))
    try:
        lnl = full(A)
        assert np.float64(full(R)).tobytes() == np.float64(lnl).tobytes()
        plan = A.last_plan()
        one_op_at_a_time(pkg, lib, B.engine, plan)
        ends = root_ends(pkg, lib, A, B, plan, lnl)
        want = branch_batch(pkg, lib, R, plan, ends)
        assert counters(lib, R.engine)[:2] == (0, 0)
        before = counters(lib, A.engine)
        for _ in range(3):
            assert branch_batch(pkg, lib, A, plan, ends) == want
        after = counters(lib, A.engine)
        assert (after[0] - before[0], after[1] - before[1]) == (1, 1), (before, after)
    finally:
        A.close()
        R.close()
        B.close()


def test_asc_engine(pkg, synth, monkeypatch):
    lib = pkg.libiqhip()
    nwk = synth.random_tree_newick(9, 5)
    model = synth.gtr_model(alpha=0.7, ncat=4)
    st = synth.simulate_alignment(nwk, synth.gtr_model(alpha=0.9, ncat=4), 200, 6)
    st = st[:, [s for s in range(st.shape[1]) if len(set(st[:, s].tolist())) > 1]]
    pat, freq = synth.compress_patterns(st)
    pat = np.concatenate([pat, np.tile(np.arange(4, dtype=np.uint8), (9, 1))], axis=1)
    freq = np.concatenate([freq, np.zeros(4)])
    kw = dict(freq=freq, n_unobs=4, nsites=int(freq.sum()))
    A, B = make_tree(pkg, nwk, pat, model, **kw), make_tree(pkg, nwk, pat, model, **kw)
    try:
        # (the tree's lnL carries the +ASC correction, which a bare root-branch evaluation on the reference does not: lnL and the
        # pattern likelihoods are held to the first submission's, which fills in the kernel; the vectors to the reference's)
        lnl = full(A)
        plh = A.fetch_pattern_lh().tobytes()
        plan = A.last_plan()
        one_op_at_a_time(pkg, lib, B.engine, plan)
        same_vectors(lib, A, B, plan)
        for _ in range(2):
            assert np.float64(full(A)).tobytes() == np.float64(lnl).tobytes()
            assert A.fetch_pattern_lh().tobytes() == plh
            same_vectors(lib, A, B, plan)
        assert counters(lib, A.engine)[:2] == (1, 1)
    finally:
        A.close()
        B.close()
