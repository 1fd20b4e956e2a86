"""CPU: the bookkeeping of k_traverse4's fill image (DESIGN.md 3.1 "Fill image"; plan.hip lay_out_lds, fill_image_submission)
on a planning-only engine: one 8-taxon planner goes through a sequence of submissions and iqhip_debug_fill_image is held to a
small model of the rule after each one; the image's layout (offsets, extents, total) is checked on plans of one and of many
chunks.  check_plan runs on every plan of a planner.  tests/test_fill_image_gpu.py runs what the kernel makes of the image."""
import ctypes as C

import pytest

from test_pair_children_plan import LEAF_BLOCKS, PAIR_BLOCKS, layout, plain
from test_pair_rows_plan import chunks_of, full_plan, set_lds_kb
from test_plan_check import planner

NPTN = 500
NCAT = 4


def fill_image(lib, e):
    """(submissions that built the image, submissions that reused it, bytes of the current plan's image)"""
    a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
    assert lib.iqhip_debug_fill_image(e, C.byref(a), C.byref(b), C.byref(c)) == 0, lib.iqhip_last_error()
    return a.value, b.value, c.value


def image_chunks(lib, e):
    n = C.c_int()
    assert lib.iqhip_debug_fill_image_chunks(e, None, 0, C.byref(n)) == 0, lib.iqhip_last_error()
    out = (C.c_int64 * (2 * max(n.value, 1)))()
    assert lib.iqhip_debug_fill_image_chunks(e, out, n.value, C.byref(n)) == 0, lib.iqhip_last_error()
    return [(out[2 * i], out[2 * i + 1]) for i in range(n.value)]


class Rule:
    """Policy A restated.  The image belongs to (plan, model version): it is stale after every submission that plans anew and
    after a model change; a submission that finds its plan cached builds a stale image and copies it, or copies the one that is
    there; a submission that plans anew, a small plan and a plan with device-side lengths never touch it."""

    def __init__(self):
        self.built = self.reused = 0
        self.model, self.image_model, self.cached = 1, 0, None

    def submit(self, key, nops_planned, device_lengths=False, segs=False):
        hit = not device_lengths and self.cached == key
        if not hit:
            self.image_model = 0
            self.cached = None if device_lengths else key
        small = nops_planned <= 2 and not segs
        if hit and not small:
            if self.image_model == self.model:
                self.reused += 1
            else:
                self.built += 1
                self.image_model = self.model

    def set_model(self):
        self.model += 1

    def set_alignment(self):
        self.cached = None


def copy_ops(pkg, ops, n=None):
    n = len(ops) if n is None else n
    out = (pkg.NodeOp * n)()
    for k in range(n):
        out[k] = ops[k]
    return out


def test_the_rule_through_a_sequence_of_submissions(pkg, synth):
    ntaxa = 8
    lib, e = planner(pkg, 4, NCAT, NPTN, ntaxa)
    rule = Rule()
    try:
        plain(lib, e, ntaxa)
        ops = copy_ops(pkg, full_plan(pkg, synth, ntaxa, 3))
        nops = len(ops)

        def planned():
            shape = (C.c_int64 * len(pkg.PLAN_SHAPE_SLOTS))()
            assert lib.iqhip_debug_plan_shape(e, shape, len(shape)) == 0
            return shape

        def submit(key, lst, n, segs=None, device_lengths=False):
            sg = (C.c_int32 * len(segs))(*segs) if segs else None
            assert lib.iqhip_debug_plan_submit(e, lst, n, sg, len(segs) if segs else 0, int(device_lengths)) == 0, lib.iqhip_last_error()
            removed = (C.c_int32 * n)()
            assert lib.iqhip_debug_plan_removed(e, removed, n) == 0
            rule.submit(key, n - sum(removed), device_lengths, bool(segs))
            got = fill_image(lib, e)
            assert got[:2] == (rule.built, rule.reused), (key, got)
            return got

        # the same op list three times: in the kernel, built, reused
        assert submit("a", ops, nops)[:2] == (0, 0)
        assert submit("a", ops, nops)[:2] == (1, 0)
        got = submit("a", ops, nops)
        assert got[:2] == (1, 1) and got[2] > 0
        # one length changed: a new plan fills in the kernel; the same again builds
        ops2 = copy_ops(pkg, ops)
        ops2[nops - 1].left_len = ops2[nops - 1].left_len + 0.01
        assert submit("b", ops2, nops)[:2] == (1, 1)
        assert submit("b", ops2, nops)[:2] == (2, 1)
        # the model changed: the cached plan's image is stale, built again, then reused
        assert lib.iqhip_debug_planner_event(e, 0) == 0
        rule.set_model()
        assert submit("b", ops2, nops)[:2] == (3, 1)
        assert submit("b", ops2, nops)[:2] == (3, 2)
        # the alignment set again: planned anew
        assert lib.iqhip_debug_planner_event(e, 1) == 0
        rule.set_alignment()
        assert submit("b", ops2, nops)[:2] == (3, 2)
        assert submit("b", ops2, nops)[:2] == (4, 2)
        # explicit segments (every op a segment of its own would need distinct inputs: two segments, a subtree each, are cut
        # from the list by hand -- the first cherry and the rest do not depend on each other only if the rest does not read it;
        # so: the leaf-leaf ops, one segment each)
        leafleaf = [k for k in range(nops) if ops[k].left_leaf >= 0 and ops[k].right_leaf >= 0]
        assert len(leafleaf) >= 2
        seg_ops = (pkg.NodeOp * len(leafleaf))()
        for q, k in enumerate(leafleaf):
            seg_ops[q] = ops[k]
        segs = [1] * len(leafleaf)
        assert submit("s", seg_ops, len(leafleaf), segs=segs)[:2] == (4, 2)
        got = submit("s", seg_ops, len(leafleaf), segs=segs)
        assert got[:2] == (5, 2) and got[2] == len(leafleaf) * 2 * LEAF_BLOCKS * 4 * NCAT * 8
        assert submit("s", seg_ops, len(leafleaf), segs=segs)[:2] == (5, 3)
        # a small plan travels in the kernel arguments: never an image, however often it repeats
        for _ in range(3):
            got = submit("small", ops, 2)
            assert got == (5, 3, 0)
        # lengths on the device: never cached, never an image
        for _ in range(2):
            got = submit("p", ops, nops, device_lengths=True)
            assert got == (5, 3, 0)
        # and the first plan once more: planned anew after all that
        assert submit("a", ops, nops)[:2] == (5, 3)
        assert submit("a", ops, nops)[:2] == (6, 3)
        assert planned()[4] >= 1
    finally:
        lib.iqhip_destroy(e)


@pytest.mark.parametrize("ntaxa,seed,ncat,kb", [(8, 3, 4, None), (40, 91, 4, 8), (50, 41, 8, 16), (50, 41, 3, 12), (14, 8, 1, 8)])
def test_the_image_is_the_chunks_one_behind_the_other(pkg, synth, monkeypatch, ntaxa, seed, ncat, kb):
    """offsets 16-byte aligned, consecutive chunks at least a chunk's extent apart, `bytes` the sum of the extents, every extent
    the chunk's regions as iqhip_debug_plan_layout lays them out"""
    set_lds_kb(monkeypatch, kb)
    lib, e = planner(pkg, 4, ncat, NPTN, ntaxa)
    try:
        plain(lib, e, ntaxa)
        ops = full_plan(pkg, synth, ntaxa, seed)
        assert lib.iqhip_debug_plan(e, ops, len(ops)) == 0, lib.iqhip_last_error()
        removed = (C.c_int32 * len(ops))()
        assert lib.iqhip_debug_plan_removed(e, removed, len(ops)) == 0
        rows = layout(pkg, lib, e, len(ops) - sum(removed))
        chunks = chunks_of(rows, 4 * ncat)
        img = image_chunks(lib, e)
        assert len(img) == len(chunks)
        if kb is not None:
            assert len(chunks) > 1
        for (off, ext), (_, _, _, end) in zip(img, chunks):
            assert off % 16 == 0 and ext == end * 8
        for (off, ext), (nxt, _) in zip(img, img[1:]):
            assert nxt - off >= ext
        assert fill_image(lib, e)[2] == sum(ext for _, ext in img)
        assert any(ext % 1024 for _, ext in img) or kb is None
    finally:
        lib.iqhip_destroy(e)


def test_other_kernels_have_no_image(pkg, synth):
    for nstates, ncat, nclass in ((20, 4, 1), (4, 4, 2), (4, 12, 1)):
        lib, e = planner(pkg, nstates, ncat, 3000, 10, nclass=nclass)
        try:
            from test_plan_check import plan_of
            ops = plan_of(pkg, synth, 10, 5, nstates)
            for _ in range(3):
                assert lib.iqhip_debug_plan(e, ops, len(ops)) == 0, lib.iqhip_last_error()
            assert fill_image(lib, e) == (0, 0, 0)
        finally:
            lib.iqhip_destroy(e)
