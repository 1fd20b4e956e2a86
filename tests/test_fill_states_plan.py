"""CPU: the LDS layout of 4-state plans as k_traverse4's chunk fill relies on it (iqhip_debug_plan_layout on a
planning-only engine, plan check on).  The fill requests the state rows of a chunk's leaf children by slot, four slots
per instruction, from a list of row pointers indexed by slot: within a chunk the leaf children own slots 1 .. n in op
order without gaps, the list fits the kernel's array (trav_lds.h kTrav4RowSlots), and regions plus state bytes of every
chunk stay within the chunk budget and within the dynamic LDS the launch allocates."""
import ctypes as C

import pytest

from test_plan_check import plan_of, planner

ROW_SLOTS = 256          # trav_lds.h kTrav4RowSlots
FIXED_DOUBLES = 128      # trav_lds.h trav4_lds: tip vectors [32][4]; + one block of values
NCAT, WG = 4, 256
BLOCK = 4 * NCAT


def layout_of(pkg, synth, ntaxa, seed, multifurcating=False):
    """(per-op layout rows, plan shape) of the full traversal of a random tree, in the caller's environment"""
    lib, e = planner(pkg, 4, NCAT, 5000, ntaxa)
    try:
        ops = plan_of(pkg, synth, ntaxa, seed, 4, multifurcating=multifurcating)
        assert lib.iqhip_debug_plan(e, ops, len(ops)) == 0, lib.iqhip_last_error()
        shape = (C.c_int64 * len(pkg.PLAN_SHAPE_SLOTS))()
        assert lib.iqhip_debug_plan_shape(e, shape, len(shape)) == 0, lib.iqhip_last_error()
        raw = (C.c_int32 * (8 * len(ops)))()
        assert lib.iqhip_debug_plan_layout(e, raw, len(ops)) == 0, lib.iqhip_last_error()
        assert lib.iqhip_debug_plan_layout(e, raw, len(ops) + 1) != 0      # not the last plan's op count: refused
        return [tuple(raw[8 * k:8 * k + 8]) for k in range(len(ops))], dict(zip(pkg.PLAN_SHAPE_SLOTS, shape))
    finally:
        lib.iqhip_destroy(e)


def chunks_of(rows):
    k = 0
    while k < len(rows):
        n = rows[k][0]
        assert n > 0, k
        yield rows[k:k + n]
        k += n


@pytest.mark.parametrize("lds_kb", [None, 8])
def test_every_chunk_fits_its_budget_and_numbers_its_slots(pkg, synth, monkeypatch, lds_kb):
    if lds_kb is not None:
        monkeypatch.setenv("IQHIP_LDS_KB", str(lds_kb))
    budget_bytes = (lds_kb or 64) * 1024
    nchunks = 0
    for ntaxa in list(range(4, 33)) + [40, 49, 50, 64, 70, 97, 128, 150, 200]:
        for seed, mf in ((ntaxa, False), (1000 + ntaxa, ntaxa % 7 == 0)):
            rows, shape = layout_of(pkg, synth, ntaxa, seed, multifurcating=mf)
            assert shape["lds_budget"] == budget_bytes // 8 - (FIXED_DOUBLES + BLOCK)
            assert shape["top_lds_bytes"] == 8 * (FIXED_DOUBLES + BLOCK + shape["lds_doubles"] + shape["state_slots"] * WG // 8)
            # (largest regions and most slots may come from different chunks, so this can pass the chunk budget by a little)
            assert shape["top_lds_bytes"] <= 152 * 1024     # trav_lds.h kTrav4MaxLdsBytes
            for chunk in chunks_of(rows):
                nchunks += 1
                nslots, want, regs = chunk[0][1], 1, 0
                for q, (cn, cs, leaf_l, leaf_r, off_l, off_r, slot_l, slot_r) in enumerate(chunk):
                    assert slot_l == (want if leaf_l else 0)
                    want += leaf_l
                    assert slot_r == (want if leaf_r else 0)
                    want += leaf_r
                    regs = max(regs, off_l + (6 if leaf_l else 1) * BLOCK, off_r + (6 if leaf_r else 1) * BLOCK)
                assert nslots == want                       # slots 1 .. n, none missing, none twice; slot 0 the dummy
                assert nslots <= ROW_SLOTS                  # the row-pointer list
                assert nslots <= shape["state_slots"] and regs <= shape["lds_doubles"]
                assert regs + nslots * WG // 8 <= shape["lds_budget"]
    assert nchunks > (150 if lds_kb else 40)


def test_a_chunk_ends_before_its_slots_outgrow_the_row_list(pkg, synth, monkeypatch):
    """one category and the largest budget: a chunk could hold more leaf children than the list has entries"""
    monkeypatch.setenv("IQHIP_LDS_KB", "150")
    monkeypatch.setenv("IQHIP_SPLIT", "0")
    lib, e = planner(pkg, 4, 1, 5000, 400)
    try:
        ops = plan_of(pkg, synth, 400, 11, 4)
        assert lib.iqhip_debug_plan(e, ops, len(ops)) == 0, lib.iqhip_last_error()
        raw = (C.c_int32 * (8 * len(ops)))()
        assert lib.iqhip_debug_plan_layout(e, raw, len(ops)) == 0
        rows = [tuple(raw[8 * k:8 * k + 8]) for k in range(len(ops))]
    finally:
        lib.iqhip_destroy(e)
    sizes = [c[0][1] for c in chunks_of(rows)]
    assert len(sizes) >= 2 and max(sizes) <= ROW_SLOTS and max(sizes) >= ROW_SLOTS - 1
    assert sum(s - 1 for s in sizes) == sum(r[2] + r[3] for r in rows)
