"""CPU: the parts of the pair-children planner (plan.hip select_pair_children, pair_code_row, lay_out_lds) that only a tight
LDS budget or a long session reaches, on a planning-only engine with every taxon plain: the consumer-fit rule and the chunk
cuts around pair children at IQHIP_LDS_KB = 8 and 16, every planner switch of test_plan_check.py with pair children in the
plan, and the pair-code row table (slots, the restart, the op that stays real for lack of a row) against a model of it.
tests/test_pair_rows_gpu.py runs what the kernel makes of the same plans."""
import ctypes as C

import pytest

from test_pair_children_plan import (LEAF_BLOCKS, PAIR_BLOCKS, SLOT_DOUBLES, candidates, expected_removed, layout, plain,
                                     removed_rows)
from test_plan_check import ENVS, plan_of, planner

TREES = [(14, 8), (40, 91), (50, 41)]   # (taxa, seed); the 14-taxon tree has an op whose two children are both cherries
LDS_KB = [None, 8, 16]
NPTN = 500
S_REG_FIXED = 128                        # trav_lds.h trav4_lds(): doubles in front of the plan regions, + one block


def lds_budget(kb, ncat):
    """plan.hip lds_budget for k_traverse4, in doubles (IQHIP_LDS_KB unset: 64)"""
    return (kb or 64) * 1024 // 8 - S_REG_FIXED - 4 * ncat


def pair_rows(lib, e):
    """(slots in use, restarts, ops kept real for lack of a row)"""
    a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
    assert lib.iqhip_debug_pair_rows(e, C.byref(a), C.byref(b), C.byref(c)) == 0, lib.iqhip_last_error()
    return a.value, b.value, c.value


def as_node_ops(pkg, plan):
    ops = (pkg.NodeOp * len(plan))()
    for k, p in enumerate(plan):
        ops[k] = pkg.NodeOp(p["dst_key"], p["left_key"], p["right_key"], p["left_leaf"], p["right_leaf"], p["left_len"],
                            p["right_len"], p["flags"], 0)
    return ops


def set_lds_kb(monkeypatch, kb):
    if kb is None:
        monkeypatch.delenv("IQHIP_LDS_KB", raising=False)
    else:
        monkeypatch.setenv("IQHIP_LDS_KB", str(kb))


_plans = {}


def full_plan(pkg, synth, ntaxa, seed):
    """the full-traversal op list of random_tree_newick(ntaxa, seed), built once (nobody writes to it)"""
    if (ntaxa, seed) not in _plans:
        _plans[ntaxa, seed] = plan_of(pkg, synth, ntaxa, seed, 4)
    return _plans[ntaxa, seed]


def chunks_of(rows, block):
    """[(first op, ops, slots, doubles of regions)] of a plan's LDS chunks, from iqhip_debug_plan_layout; a table child that is
    no leaf is a pair child"""
    out, k = [], 0
    while k < len(rows):
        n, nslots = int(rows[k][0]), int(rows[k][1])
        assert n > 0, k
        end = 0
        for r in rows[k:k + n]:
            for leaf, off, slot in ((r[2], r[4], r[6]), (r[3], r[5], r[7])):
                blocks = LEAF_BLOCKS if leaf else (PAIR_BLOCKS if slot > 0 else 1)
                end = max(end, int(off) + blocks * block)
        out.append((k, n, nslots, end))
        k += n
    assert k == len(rows)
    return out


def has_pair(row):
    return (row[6] > 0 and not row[2]) or (row[7] > 0 and not row[3])


def plan_at_budget(pkg, synth, monkeypatch, ntaxa, seed, ncat, kb, nptn=NPTN, ops=None):
    """plans the tree on a fresh planner with every taxon plain: the plan is accepted (check_plan runs on every planner plan),
    the removed rows are the restated rule's, the chunks tile what is left and each stays within the budget.
    Returns (layout rows, chunks, removed rows)."""
    set_lds_kb(monkeypatch, kb)
    lib, e = planner(pkg, 4, ncat, nptn, ntaxa)
    try:
        plain(lib, e, ntaxa)
        if ops is None:
            ops = full_plan(pkg, synth, ntaxa, seed)
        assert lib.iqhip_debug_plan(e, ops, len(ops)) == 0, lib.iqhip_last_error()
        block, budget = 4 * ncat, lds_budget(kb, ncat)
        want = expected_removed([ops[k] for k in range(len(ops))], budget=budget, block=block)
        got = removed_rows(lib, e, len(ops))
        assert got == want
        shape = (C.c_int64 * len(pkg.PLAN_SHAPE_SLOTS))()
        assert lib.iqhip_debug_plan_shape(e, shape, len(shape)) == 0
        assert shape[0] == budget
        lds_doubles, slots = shape[1], shape[2]
        nleft = len(ops) - len(want)
        rows = layout(pkg, lib, e, nleft)
        chunks = chunks_of(rows, block)
        for k, n, nslots, end in chunks:
            assert nslots <= slots
            assert max(int(max(r[4], r[5])) for r in rows[k:k + n]) + block <= lds_doubles
            assert end <= lds_doubles
            assert end + nslots * SLOT_DOUBLES <= budget, (k, n, nslots, end)
        assert len(chunks) == shape[4]
        assert lds_doubles <= budget and (not want or lds_doubles >= PAIR_BLOCKS * block)
        return rows, chunks, got
    finally:
        lib.iqhip_destroy(e)


@pytest.mark.parametrize("ntaxa,seed", TREES)
@pytest.mark.parametrize("kb", LDS_KB)
@pytest.mark.parametrize("ncat", range(1, 9))
def test_budget_matrix(pkg, synth, monkeypatch, ncat, kb, ntaxa, seed):
    """every plan the planner accepted before pair children is accepted with them: a leaf-leaf op whose consumer would not fit
    a chunk with the 38-block pair region stays real"""
    ops = full_plan(pkg, synth, ntaxa, seed)
    _, _, removed = plan_at_budget(pkg, synth, monkeypatch, ntaxa, seed, ncat, kb)
    cand = candidates([ops[k] for k in range(len(ops))])
    assert cand
    block, budget = 4 * ncat, lds_budget(kb, ncat)
    if SLOT_DOUBLES + PAIR_BLOCKS * block + SLOT_DOUBLES + block > budget:
        assert removed == []          # no consumer holds a pair child: the plan of an engine without plain taxa
    if kb is None:
        assert removed == cand        # the default budget holds two pair children at every category count


def test_the_two_cherry_parent_keeps_its_right_cherry_real_at_a_tight_budget(pkg, synth, monkeypatch):
    """14 taxa, seed 8: at 8 KB x 3 categories (and 16 KB x 6) two pair regions do not fit one chunk, one and a vector do"""
    ops = full_plan(pkg, synth, 14, 8)
    lst = [ops[k] for k in range(len(ops))]
    cand = candidates(lst)
    by_key = {lst[k].dst_key: k for k in cand}
    both = [(by_key[p.left_key], by_key[p.right_key]) for p in lst if p.left_leaf < 0 and p.right_leaf < 0 and
            p.left_key in by_key and p.right_key in by_key]
    assert len(both) == 1
    left, right = both[0]
    for ncat, kb in ((3, 8), (6, 16)):
        _, _, removed = plan_at_budget(pkg, synth, monkeypatch, 14, 8, ncat, kb)
        assert left in removed and right not in removed
        assert sorted(removed + [right]) == cand


def test_the_matrix_cuts_chunks_at_pair_children(pkg, synth, monkeypatch):
    """somewhere in the matrix a plan of two or more chunks has a pair child in the first op of a chunk, and one has a pair
    child in the last op of a chunk; (8 categories, 16 KB) and (4 categories, 8 KB) on the large trees, the shapes
    tests/test_pair_rows_gpu.py runs, are among them"""
    first, last = [], []
    for ntaxa, seed in TREES:
        for kb in LDS_KB:
            for ncat in range(1, 9):
                rows, chunks, _ = plan_at_budget(pkg, synth, monkeypatch, ntaxa, seed, ncat, kb)
                if len(chunks) < 2:
                    continue
                if any(has_pair(rows[k]) for k, n, _, _ in chunks):
                    first.append((ntaxa, ncat, kb))
                if any(has_pair(rows[k + n - 1]) for k, n, _, _ in chunks):
                    last.append((ntaxa, ncat, kb))
    assert first, "no chunk of the matrix opens with a pair child"
    assert last, "no chunk of the matrix closes with a pair child"
    for case in ((40, 8, 16), (50, 8, 16), (40, 4, 8), (50, 4, 8)):
        assert case in first or case in last, (case, first, last)


@pytest.mark.parametrize("env", ENVS)
@pytest.mark.parametrize("ntaxa,nptn", [(9, 500), (50, 3000)])
@pytest.mark.parametrize("ncat", [1, 3, 4, 8])
def test_planner_environments_with_pair_children(pkg, synth, monkeypatch, ncat, ntaxa, nptn, env):
    """test_plan_check.py's switches on plans that hold pair children (its own plans mark no taxon plain)"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    lib, e = planner(pkg, 4, ncat, nptn, ntaxa)
    try:
        plain(lib, e, ntaxa)
        some = False
        for seed, mf in ((41, False), (42, False), (43, True)):
            ops = plan_of(pkg, synth, ntaxa, seed, 4, multifurcating=mf)
            lst = [ops[k] for k in range(len(ops))]
            assert lib.iqhip_debug_plan(e, ops, len(ops)) == 0, lib.iqhip_last_error()
            want = expected_removed(lst, budget=lds_budget(None, ncat), block=4 * ncat)
            assert removed_rows(lib, e, len(ops)) == want
            some = some or bool(want)
            # a sweep-sized plan of the same tree: the small-plan path (a cherry is removed only if op 1 consumes it)
            assert lib.iqhip_debug_plan(e, ops, 2) == 0, lib.iqhip_last_error()
            assert removed_rows(lib, e, 2) == expected_removed(lst[:2], budget=lds_budget(None, ncat), block=4 * ncat)
        assert some
    finally:
        lib.iqhip_destroy(e)


class SlotTable:
    """the pair-code row table restated: `n` slots; a plan's missing pairs are inserted in op order; the table starts over when
    the pairs present plus the missing ones exceed n; a pair that finds the table full keeps its op real"""

    def __init__(self, n):
        self.n, self.rows, self.restarts, self.kept_real = n, {}, 0, 0

    def plan(self, ops, rows):
        """rows: the ops the eligibility rule removes; -> those that get a code row"""
        pairs = [(ops[k].left_leaf, ops[k].right_leaf) for k in rows]
        missing = [p for p in pairs if p not in self.rows]
        if missing and len(self.rows) + len(missing) > self.n:
            self.rows.clear()
            self.restarts += 1
        out = []
        for k, p in zip(rows, pairs):
            if p not in self.rows:
                if len(self.rows) >= self.n:
                    self.kept_real += 1
                    continue
                self.rows[p] = len(self.rows)
            out.append(k)
        return out

    def state(self):
        return len(self.rows), self.restarts, self.kept_real


SLOT_SEEDS = range(1, 13)


def test_the_slot_table_follows_a_changing_tree(pkg, synth):
    """one 8-taxon planner walks through the trees of seeds 1 .. 12: 15 distinct ordered pairs against 8 slots"""
    ntaxa = 8
    lib, e = planner(pkg, 4, 4, NPTN, ntaxa)
    model = SlotTable(ntaxa)
    try:
        plain(lib, e, ntaxa)
        seen = set()
        for seed in SLOT_SEEDS:
            ops = full_plan(pkg, synth, ntaxa, seed)
            lst = [ops[k] for k in range(len(ops))]
            assert lib.iqhip_debug_plan(e, ops, len(ops)) == 0, lib.iqhip_last_error()
            rule = expected_removed(lst, budget=lds_budget(None, 4))
            seen |= {(lst[k].left_leaf, lst[k].right_leaf) for k in rule}
            assert removed_rows(lib, e, len(ops)) == model.plan(lst, rule) == rule
            assert pair_rows(lib, e) == model.state(), seed
            assert pair_rows(lib, e)[1] == (0 if seed < 8 else model.restarts), seed
            if seed == 8:
                assert model.restarts == 1
            # the same plan again -- the cached one, then planned anew -- finds every row it needs
            assert lib.iqhip_debug_plan(e, ops, len(ops)) == 0, lib.iqhip_last_error()
            assert pair_rows(lib, e) == model.state(), seed
            plain(lib, e, ntaxa)   # (drops the cached plan)
            assert lib.iqhip_debug_plan(e, ops, len(ops)) == 0, lib.iqhip_last_error()
            assert removed_rows(lib, e, len(ops)) == rule
            assert pair_rows(lib, e) == model.state(), seed
        assert len(seen) > ntaxa and model.restarts >= 1 and model.kept_real == 0
    finally:
        lib.iqhip_destroy(e)


def hand_op(dst, left, right, a, b):
    """one op of a hand-written plan: a child is a taxon (int) or the key of a vector ("k", key)"""
    ll, lk = (left, 0) if isinstance(left, int) else (-1, left[1])
    rl, rk = (right, 0) if isinstance(right, int) else (-1, right[1])
    return dict(dst_key=dst, left_key=lk, right_key=rk, left_leaf=ll, right_leaf=rl, left_len=a, right_len=b, flags=0, dst=(dst,))


def six_cherry_plan():
    """every unordered pair of four taxa as a leaf-leaf op (rows 0 .. 5: more than the table's four slots) and the five joins
    above them: 201 = (101, 102), 202 = (103, 104), 203 = (105, 106), 204 = (201, 202), 205 = (204, 203)"""
    pairs = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
    plan = [hand_op(101 + q, a, b, 0.03 + 0.02 * q, 0.21 - 0.03 * q) for q, (a, b) in enumerate(pairs)]
    k = lambda key: ("k", key)   # noqa: E731
    plan += [hand_op(201, k(101), k(102), 0.05, 0.07), hand_op(202, k(103), k(104), 0.11, 0.04),
             hand_op(203, k(105), k(106), 0.06, 0.09), hand_op(204, k(201), k(202), 0.08, 0.12),
             hand_op(205, k(204), k(203), 0.10, 0.02)]
    return plan


def both_orders_plan():
    """the cherries (0, 1) and (1, 0) with swapped lengths -- the same vector --, each under a consumer of its own:
    201 = (101, taxon 2), 202 = (taxon 3, 102), 203 = (201, 202)"""
    k = lambda key: ("k", key)   # noqa: E731
    return [hand_op(101, 0, 1, 0.13, 0.31), hand_op(102, 1, 0, 0.31, 0.13), hand_op(201, k(101), 2, 0.05, 0.07),
            hand_op(202, 3, k(102), 0.11, 0.04), hand_op(203, k(201), k(202), 0.08, 0.12)]


def test_more_leaf_leaf_ops_than_slots(pkg):
    lib, e = planner(pkg, 4, 4, NPTN, 4)
    try:
        plain(lib, e, 4)
        plan = six_cherry_plan()
        ops = as_node_ops(pkg, plan)
        assert lib.iqhip_debug_plan(e, ops, len(ops)) == 0, lib.iqhip_last_error()
        lst = [ops[k] for k in range(len(ops))]
        rule = expected_removed(lst, budget=lds_budget(None, 4))
        assert rule == [0, 1, 2, 3, 4, 5]
        model = SlotTable(4)
        assert removed_rows(lib, e, len(ops)) == model.plan(lst, rule) == [0, 1, 2, 3]
        assert pair_rows(lib, e) == model.state()
        assert pair_rows(lib, e)[0] == 4 and pair_rows(lib, e)[2] == 2
    finally:
        lib.iqhip_destroy(e)


def test_both_orders_of_a_pair_have_a_row_each(pkg):
    lib, e = planner(pkg, 4, 4, NPTN, 4)
    try:
        plain(lib, e, 4)
        ops = as_node_ops(pkg, both_orders_plan())
        assert lib.iqhip_debug_plan(e, ops, len(ops)) == 0, lib.iqhip_last_error()
        assert removed_rows(lib, e, len(ops)) == [0, 1]
        assert pair_rows(lib, e) == (2, 0, 0)
    finally:
        lib.iqhip_destroy(e)
