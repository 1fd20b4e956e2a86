"""The refusals of iqhip_pars_insert_scores_batch (include/iqhip.h "Fitch parsimony"): everything is checked before
anything is launched.  Without a device: the symbols, planning-only engines and a null engine.  On the device (marked
gpu): null arguments, nseg < 1, seg_start[0] != 0, an empty segment, a slot out of range or never written, a taxon that is
not a tip slot, a word other than wave / wg in IQHIP_PARS_BATCH_ROUTE, a state that iqhip_pars_init has not laid out, and
sharded and embedded engines with the codes of the other iqhip_pars_* calls."""
import ctypes as C

import numpy as np
import pytest


def test_symbols_and_engines_without_a_device(pkg):
    lib = pkg.libiqhip()
    for s in ("iqhip_pars_insert_scores_batch", "iqhip_debug_pars_batch_timing"):
        assert hasattr(lib, s) and s in pkg.IQHIP_SYMBOLS, s
    IQHIP_ERR_INVALID = pkg.ERR_INVALID
    i32 = (C.c_int32 * 4)(0, 1, 2, 3)
    ss = (C.c_int32 * 2)(0, 1)
    ms, cnt = C.c_double(), (C.c_int64 * 3)()
    assert lib.iqhip_pars_insert_scores_batch(None, i32, ss, 1, i32, None, i32, i32) != 0        # no engine
    assert lib.iqhip_debug_pars_batch_timing(None, C.byref(ms), cnt, 0) == IQHIP_ERR_INVALID
    e = C.c_void_p()
    assert lib.iqhip_debug_create_planner(C.byref(e), 4, 4, 100, 5, 256, 18, 1) == 0
    try:
        assert lib.iqhip_pars_insert_scores_batch(e, i32, ss, 1, i32, None, i32, i32) == IQHIP_ERR_INVALID
        assert b"planning-only" in lib.iqhip_last_error()
        assert lib.iqhip_debug_pars_batch_timing(e, C.byref(ms), cnt, 0) == IQHIP_ERR_INVALID
    finally:
        lib.iqhip_destroy(e)


def test_wrapper_refuses_lists_that_do_not_fit(pkg, synth):
    """the Python wrapper passes lengths on: a seg_start that does not end at the number of branches never reaches C"""
    t = pkg.PhyloTree(synth.random_tree_newick(5, 1))
    with pytest.raises(pkg.HostError):
        t.pars_insert_scores_batch([(0, 1)], [0, 2], [3])
    with pytest.raises(pkg.HostError):
        t.pars_insert_scores_batch([(0, 1)], [0, 1, 1], [3])


@pytest.mark.gpu
def test_refusals_on_the_device(pkg, synth, monkeypatch):
    """everything is checked before anything is launched: a refused call leaves no count behind"""
    from test_pars_batch_gpu import NTREE, T, problem
    from test_parsimony_gpu import alignment, code_of, make_tree
    monkeypatch.delenv("IQHIP_PARS_BATCH_ROUTE", raising=False)
    states, freq, mask, ops, ends, want = problem(4, 33)
    t = make_tree(pkg, synth, 4, states, freq)
    INVALID = pkg.ERR_INVALID
    call = t.pars_insert_scores_batch
    assert code_of(pkg, call, ends[:2], [0, 2], [NTREE]) == INVALID              # before iqhip_pars_init
    t.pars_init(mask)
    assert code_of(pkg, call, ends[:2], [0, 2], [NTREE]) == INVALID              # slots never written
    t.pars_update(ops)
    t.pars_batch_timing()
    ok = call(ends[:3], [0, 1, 3], [NTREE, NTREE + 1])
    assert code_of(pkg, call, np.zeros((0, 2)), [0], []) == INVALID               # nseg < 1
    assert code_of(pkg, call, ends[:3], [1, 2, 3], [NTREE, NTREE]) == INVALID    # seg_start[0] != 0
    assert code_of(pkg, call, ends[:3], [0, 0, 3], [NTREE, NTREE]) == INVALID    # an empty segment
    assert code_of(pkg, call, ends[:3], [0, 3, 3], [NTREE, NTREE]) == INVALID
    assert code_of(pkg, call, ends[:3], [0, 4, 3], [NTREE, NTREE]) == INVALID    # decreasing
    assert code_of(pkg, call, ends[:3], [0, 1, 3], [NTREE, T]) == INVALID        # not a tip slot
    assert code_of(pkg, call, ends[:3], [0, 1, 3], [-1, NTREE]) == INVALID
    nslots = T + t.pars_shape()[2]
    assert code_of(pkg, call, [ends[0], (0, nslots)], [0, 2], [NTREE]) == INVALID   # a slot out of range
    assert code_of(pkg, call, [ends[0], (-1, 0)], [0, 2], [NTREE]) == INVALID
    assert code_of(pkg, call, [ends[0], (0, nslots - 1)], [0, 2], [NTREE]) == INVALID   # in range, never written
    monkeypatch.setenv("IQHIP_PARS_BATCH_ROUTE", "workgroup")
    assert code_of(pkg, call, ends[:3], [0, 1, 3], [NTREE, NTREE + 1]) == INVALID
    assert "IQHIP_PARS_BATCH_ROUTE" in pkg.libiqhip().iqhip_last_error().decode()
    monkeypatch.delenv("IQHIP_PARS_BATCH_ROUTE")
    bt = t.pars_batch_timing()
    assert (bt["launches"], bt["branches"], bt["segments"]) == (2, 3, 2)
    again = call(ends[:3], [0, 1, 3], [NTREE, NTREE + 1])
    assert all(np.array_equal(a, b) for a, b in zip(ok, again))
    # null arguments, through the C interface
    lib, i32p = pkg.libiqhip(), C.POINTER(C.c_int32)
    en = np.ascontiguousarray(ends[:3], dtype=np.int32)
    ss, tx = np.array([0, 1, 3], dtype=np.int32), np.array([NTREE, NTREE], dtype=np.int32)
    out = np.zeros(2, dtype=np.int32)
    p = lambda a: a.ctypes.data_as(i32p)
    for args in ((None, p(ss), 2, p(tx), None, p(out), p(out)), (p(en), None, 2, p(tx), None, p(out), p(out)),
                 (p(en), p(ss), 2, None, None, p(out), p(out)), (p(en), p(ss), 2, p(tx), None, None, p(out)),
                 (p(en), p(ss), 2, p(tx), None, p(out), None)):
        assert lib.iqhip_pars_insert_scores_batch(t.engine, *args) == INVALID
    # new frequencies invalidate the state, as for the other parsimony calls
    t.set_ptn_freq(freq * 2)
    assert code_of(pkg, call, ends[:3], [0, 1, 3], [NTREE, NTREE + 1]) == INVALID
    t.close()
    # sharded engines and embedded state counts: the codes of the other iqhip_pars_* calls
    rng = np.random.default_rng(3)
    st8, fr8, mk8 = alignment(4, 5, 200, rng, tail=False)
    st8, fr8 = np.concatenate([st8] * 8, axis=1), np.concatenate([fr8] * 8)
    ts = make_tree(pkg, synth, 4, st8, fr8, sharded=2)
    assert code_of(pkg, ts.pars_insert_scores_batch, [(0, 1)], [0, 1], [2]) == pkg.ERR_UNSUPPORTED
    ts.close()
    t5 = make_tree(pkg, synth, 5, (st8 % 5).astype(np.uint8), fr8, model=synth.random_reversible_model(5, 4, alpha=0.7, ncat=4))
    assert code_of(pkg, t5.pars_insert_scores_batch, [(0, 1)], [0, 1], [2]) == pkg.ERR_UNSUPPORTED
    t5.close()
