"""CPU: the planner's part of k_traverse4's pair children (plan.hip select_pair_children, lay_out_lds, check_plan) on a
planning-only engine.  Such an engine has no alignment, so it is told which taxa hold plain states only
(iqhip_debug_planner_plain_taxa); without that nothing is removed and every recorded plan shape stays what it was."""
import ctypes as C

import numpy as np
import pytest

from test_plan_check import plan_of, planner

NCAT = 4
BLOCK = 4 * NCAT
PAIR_BLOCKS, LEAF_BLOCKS = 38, 6   # iqhip_internal.h child_region_blocks
LAYOUT_NSLOTS = 8                  # include/iqhip.h IQHIP_PLAN_LAYOUT_NSLOTS


def bind(lib):
    lib.iqhip_debug_planner_plain_taxa.argtypes = [C.c_void_p, C.POINTER(C.c_uint8)]
    lib.iqhip_debug_plan_removed.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.c_int]
    return lib


def plain(lib, e, ntaxa, but=()):
    flags = (C.c_uint8 * ntaxa)(*[0 if t in but else 1 for t in range(ntaxa)])
    assert bind(lib).iqhip_debug_planner_plain_taxa(e, flags) == 0, lib.iqhip_last_error()


def removed_rows(lib, e, nrows):
    out = (C.c_int32 * nrows)()
    assert bind(lib).iqhip_debug_plan_removed(e, out, nrows) == 0, lib.iqhip_last_error()
    return [k for k in range(nrows) if out[k]]


SLOT_DOUBLES = 32                  # trav_lds.h trav4_lds().slot_doubles: one state byte per thread of the workgroup


def expected_removed(ops, but=(), budget=None, block=BLOCK):
    """the rule of select_pair_children, restated: both children plain leaves, scaling rule 0, exactly one later consumer, not
    the last op; and, with `budget` (doubles, lds_budget(e)): the consumer fits a chunk of its own -- slot 0, both children's
    regions and the state slots of the table children -- with the op as a pair child.  A consumer of two candidates: both if
    they fit together, else the left one alone (the right one a vector) if that fits, else neither."""
    cand = candidates(ops, but)
    if budget is None:
        return cand
    need = {"pair": PAIR_BLOCKS * block + SLOT_DOUBLES, "leaf": LEAF_BLOCKS * block + SLOT_DOUBLES, "vector": block}

    def fits(a, b):
        return SLOT_DOUBLES + need[a] + need[b] <= budget
    by_key = {ops[k].dst_key: k for k in cand}
    out = []
    for p in ops:
        l = by_key.get(p.left_key) if p.left_leaf < 0 else None
        r = by_key.get(p.right_key) if p.right_leaf < 0 else None
        if l is not None and r is not None:
            if fits("pair", "pair"):
                out += [l, r]
            elif fits("pair", "vector"):
                out.append(l)
        elif l is not None and fits("pair", "leaf" if p.right_leaf >= 0 else "vector"):
            out.append(l)
        elif r is not None and fits("leaf" if p.left_leaf >= 0 else "vector", "pair"):
            out.append(r)
    return sorted(out)


def candidates(ops, but=()):
    out = []
    for k, o in enumerate(ops[:-1]):
        if o.left_leaf < 0 or o.right_leaf < 0 or o.flags & 3 or o.left_leaf in but or o.right_leaf in but:
            continue
        readers = [j for j, p in enumerate(ops) if (p.left_leaf < 0 and p.left_key == o.dst_key) or (p.right_leaf < 0 and p.right_key == o.dst_key)]
        writers = [j for j, p in enumerate(ops) if p.dst_key == o.dst_key]
        if len(readers) == 1 and readers[0] > k and writers == [k]:
            out.append(k)
    return out


def layout(pkg, lib, e, nops):
    raw = (C.c_int32 * (nops * LAYOUT_NSLOTS))()
    assert lib.iqhip_debug_plan_layout(e, raw, nops) == 0, lib.iqhip_last_error()
    return np.array(raw).reshape(nops, LAYOUT_NSLOTS)


@pytest.mark.parametrize("ntaxa,nptn", [(50, 100000), (200, 1000000), (1000, 5000), (14, 130)])
@pytest.mark.parametrize("multifurcating", [False, True])
def test_which_ops_are_removed_and_where_the_chunks_are_cut(pkg, synth, ntaxa, nptn, multifurcating):
    """(14 taxa x 130 patterns: the plan is cut into units; 1 000 taxa: many chunks)"""
    lib, e = planner(pkg, 4, NCAT, nptn, ntaxa)
    try:
        ops = plan_of(pkg, synth, ntaxa, 41, 4, multifurcating=multifurcating)
        assert lib.iqhip_debug_plan(e, ops, len(ops)) == 0, lib.iqhip_last_error()
        assert removed_rows(lib, e, len(ops)) == []           # nothing known about the taxa: nothing removed
        but = (ops[0].left_leaf,) if ops[0].left_leaf >= 0 else ()
        plain(lib, e, ntaxa, but)
        assert lib.iqhip_debug_plan(e, ops, len(ops)) == 0, lib.iqhip_last_error()   # (check_plan runs on every planner plan)
        want = expected_removed([ops[k] for k in range(len(ops))], but)
        got = removed_rows(lib, e, len(ops))
        assert want or multifurcating, "the tree has no removable leaf-leaf op"
        assert got == want
        if multifurcating:
            assert any(o.left_leaf >= 0 and o.right_leaf >= 0 and o.flags & 3 for o in ops)   # ... which stayed real
        shape = (C.c_int64 * len(pkg.PLAN_SHAPE_SLOTS))()
        assert lib.iqhip_debug_plan_shape(e, shape, len(shape)) == 0
        budget, lds_doubles, slots = shape[0], shape[1], shape[2]
        nleft = len(ops) - len(want)
        rows = layout(pkg, lib, e, nleft)
        # the chunks tile what is left of the plan; check_plan (always on here) has held every chunk's regions -- 38 blocks for a
        # pair child -- plus its state slots (32 doubles each) to the budget, restated here for the largest
        k, chunks = 0, 0
        while k < nleft:
            n, nslots = int(rows[k][0]), int(rows[k][1])
            assert n > 0 and nslots <= slots
            assert max(int(max(r[4], r[5])) for r in rows[k:k + n]) + BLOCK <= lds_doubles
            k += n
            chunks += 1
        assert k == nleft and chunks == shape[4]
        assert lds_doubles <= budget and (not want or lds_doubles >= PAIR_BLOCKS * BLOCK)
        if ntaxa == 50 and not multifurcating:
            assert chunks == 2   # the benchmark plan needs two chunks at the present budget
    finally:
        lib.iqhip_destroy(e)


def test_a_short_plan_keeps_its_last_op_and_travels_small(pkg, synth):
    lib, e = planner(pkg, 4, NCAT, 5000, 9)
    try:
        plain(lib, e, 9)
        ops = plan_of(pkg, synth, 9, 41, 4)
        k = next(k for k, o in enumerate(ops) if o.left_leaf >= 0 and o.right_leaf >= 0)
        one = (pkg.NodeOp * 1)(ops[k])
        assert lib.iqhip_debug_plan(e, one, 1) == 0, lib.iqhip_last_error()
        assert removed_rows(lib, e, 1) == []                  # a one-op plan: its only op is its last
    finally:
        lib.iqhip_destroy(e)


@pytest.mark.parametrize("how,message", [("pair_row", b"a pair-code row for a pair child, and only for one"),
                                         ("pair_region", b"LDS chunk over the LDS budget")])
def test_check_plan_rejects_broken_pair_children(pkg, synth, monkeypatch, how, message):
    """a pair-code row attached to a child that is read as a leaf; a pair child's region that ends past the LDS budget"""
    monkeypatch.setenv("IQHIP_DEBUG_BREAK_PLAN", how)
    lib, e = planner(pkg, 4, NCAT, 100000, 50)
    try:
        plain(lib, e, 50)
        ops = plan_of(pkg, synth, 50, 41, 4)
        assert lib.iqhip_debug_plan(e, ops, len(ops)) != 0
        assert b"plan check" in lib.iqhip_last_error() and message in lib.iqhip_last_error(), lib.iqhip_last_error()
    finally:
        lib.iqhip_destroy(e)
