"""GPU: what k_traverse4 computes from the plans of tests/test_pair_rows_plan.py -- the pair-code row table through a changing
tree (rows reused, the restart, an op that stays real for lack of a row, both orders of a pair), LDS chunks cut around pair
children at a tight IQHIP_LDS_KB, and every category count the kernel is instantiated for.

The reference is test_pair_children_gpu.py's: a second engine that gets the same ops ONE PER SUBMISSION never virtualises
anything.  Every vector, every scale_num array and sum_scale of every op must have the same bytes; sum_scale of a leaf-leaf op is
exactly 0.0.  The engine under test gets its plans through iqhip_update_partials (no root pass: which ops are removed is then
the planner's rule alone, and a planning-only engine given the same ops lays the same chunks out)."""
import numpy as np
import pytest

from test_pair_children_gpu import cherries, dptr, fetch, make_tree, node_ops, one_op_at_a_time, pair_counts, same_vectors, states_of
from test_pair_children_plan import expected_removed, layout, plain, removed_rows
from test_pair_rows_plan import SlotTable, both_orders_plan, chunks_of, has_pair, lds_budget, pair_rows, six_cherry_plan
from test_parity_gpu import LNL_RTOL
from test_plan_check import planner

pytestmark = pytest.mark.gpu

NPTN = 130   # two full 64-pattern tiles and a partial one
FOUR_TAXA = "((0:0.1,1:0.2):0.05,2:0.15,3:0.12);"


def dry_plan(pkg, synth, nwk, ntaxa):
    """the op list of clearAllPartialLH(); computeLikelihood() on this tree, from a host mirror without an engine (as
    test_plan_check.py plan_of)"""
    t = pkg.PhyloTree(nwk)
    try:
        t.set_mem_mode(0)
        t.set_alignment(4, pkg.SEQ_DNA, np.full((ntaxa, 8), 18, dtype=np.uint8), np.ones(8))
        t.set_model(synth.gtr_model())
        t.set_dry_run(True)
        t.clear_all_partial_lh()
        t.compute_likelihood()
        return t.last_plan()
    finally:
        t.close()


def rule_of(pkg, plan, ncat, kb=None):
    """the rows the eligibility rule removes (every taxon plain)"""
    ops = node_ops(pkg, plan)
    return expected_removed([ops[k] for k in range(len(plan))], budget=lds_budget(kb, ncat), block=4 * ncat)


def submit_and_compare(pkg, lib, A, B, plan, nremoved):
    """the whole plan in one submission to A, op by op to B: sum_scale, vectors and counters with the same bytes; `nremoved`
    ops were answered from pair tables"""
    ss = np.full(len(plan), -1.0)
    assert lib.iqhip_update_partials(A.engine, node_ops(pkg, plan), len(plan), dptr(ss)) == 0, lib.iqhip_last_error()
    assert pair_counts(lib, A.engine)[2] == nremoved
    ss_ref = one_op_at_a_time(pkg, lib, B.engine, plan)
    assert ss.tobytes() == ss_ref.tobytes(), (ss, ss_ref)
    assert all(ss[k] == 0.0 for k in cherries(plan))
    same_vectors(lib, A, B, plan)
    assert pair_counts(lib, B.engine)[0] == 0      # the reference has removed nothing, ever


def lnl_against_oracle(pkg, oracle, nwk, states, model):
    """an ordinary tree on the same data (its engine is created under the caller's environment); returns its plan"""
    T = make_tree(pkg, nwk, states, model)
    try:
        T.clear_all_partial_lh()
        lnl = T.compute_likelihood()
        ot = oracle.OracleTree(nwk, 4, oracle.SEQ_DNA, states, np.ones(states.shape[1]), None, model)
        ref, _ = ot.likelihood()
        assert abs(lnl - ref) <= LNL_RTOL * abs(ref)
        return T.last_plan()
    finally:
        T.close()


@pytest.mark.parametrize("ncat,split", [(4, None), (4, "1"), (1, None)])
def test_a_changing_tree_on_one_engine(pkg, synth, oracle, monkeypatch, ncat, split):
    """the trees of seeds 1 .. 12 on one 8-taxon engine: 15 distinct ordered pairs against 8 slots, so rows are reused, the
    table starts over (at seed 8) and later plans rebuild their pairs into recycled slots"""
    if split:
        monkeypatch.setenv("IQHIP_LANE_SPLIT", split)
    lib = pkg.libiqhip()
    ntaxa = 8
    model = synth.gtr_model(alpha=0.7, ncat=ncat)
    nwks = {seed: synth.random_tree_newick(ntaxa, seed) for seed in range(1, 13)}
    states = states_of(synth, nwks[12], model, NPTN, 5, missing=0.05)
    A, B = make_tree(pkg, nwks[1], states, model), make_tree(pkg, nwks[1], states, model)
    table = SlotTable(ntaxa)
    try:
        def step(seed):
            plan = dry_plan(pkg, synth, nwks[seed], ntaxa)
            ops = node_ops(pkg, plan)
            got = table.plan([ops[k] for k in range(len(plan))], rule_of(pkg, plan, ncat))
            assert got
            submit_and_compare(pkg, lib, A, B, plan, len(got))
            assert pair_rows(lib, A.engine) == table.state(), seed
            return plan
        for seed in range(1, 13):
            step(seed)
        assert pair_rows(lib, A.engine)[1] >= 1 and table.kept_real == 0
        # seed 12 again: the cached plan, after the comparison above has fetched (and so expanded) its virtual vectors
        before = pair_rows(lib, A.engine)
        plan = step(12)
        assert pair_rows(lib, A.engine) == before
        key = plan[cherries(plan)[0]]["dst_key"]
        assert fetch(lib, A, key) == fetch(lib, B, key)
        # seed 1 again: its pairs were lost in the restart and are built anew
        step(1)
        assert pair_rows(lib, A.engine)[0] > before[0] or pair_rows(lib, A.engine)[1] > before[1]
        lnl_against_oracle(pkg, oracle, nwks[12], states, model)
    finally:
        A.close()
        B.close()


@pytest.mark.parametrize("nptn", [NPTN, 1])
def test_more_leaf_leaf_ops_than_slots(pkg, synth, monkeypatch, nptn):
    """six leaf-leaf ops over four taxa: four get a code row, two stay real for lack of one"""
    lib = pkg.libiqhip()
    model = synth.gtr_model(alpha=0.7, ncat=4)
    states = states_of(synth, FOUR_TAXA, model, nptn, 9, missing=0.1)
    A, B = make_tree(pkg, FOUR_TAXA, states, model), make_tree(pkg, FOUR_TAXA, states, model)
    try:
        plan = six_cherry_plan()
        assert len(plan) == 11
        submit_and_compare(pkg, lib, A, B, plan, 4)
        assert pair_rows(lib, A.engine) == (4, 1, 2)
        removed = {plan[k]["dst_key"] for k in range(4)}
        real = {plan[k]["dst_key"] for k in (4, 5)}
        joins = [(p["left_key"], p["right_key"]) for p in plan[6:]]
        assert sum(1 for l, r in joins if l in removed and r in removed) == 2
        assert sum(1 for l, r in joins if l in real and r in real) == 1
    finally:
        A.close()
        B.close()


@pytest.mark.parametrize("ncat,split", [(4, None), (4, "1"), (1, None)])
def test_both_orders_of_a_pair(pkg, synth, monkeypatch, ncat, split):
    """(0, 1) and (1, 0) with swapped lengths are the same vector from two code rows"""
    if split:
        monkeypatch.setenv("IQHIP_LANE_SPLIT", split)
    lib = pkg.libiqhip()
    model = synth.gtr_model(alpha=0.7, ncat=ncat)
    states = states_of(synth, FOUR_TAXA, model, NPTN, 9, missing=0.1)
    A, B = make_tree(pkg, FOUR_TAXA, states, model), make_tree(pkg, FOUR_TAXA, states, model)
    try:
        plan = both_orders_plan()
        submit_and_compare(pkg, lib, A, B, plan, 2)     # (both consumers, and the op above them, match the reference)
        assert pair_rows(lib, A.engine) == (2, 0, 0)
        assert fetch(lib, A, plan[0]["dst_key"]) == fetch(lib, A, plan[1]["dst_key"])
    finally:
        A.close()
        B.close()


@pytest.mark.parametrize("ntaxa,seed,ncat,kb", [(40, 91, 8, 16), (50, 41, 8, 16), (40, 91, 4, 8), (50, 41, 4, 8), (14, 8, 3, 8)])
def test_chunk_cuts_around_pair_children(pkg, synth, oracle, monkeypatch, ntaxa, seed, ncat, kb):
    """plans of 4 to 21 chunks in which chunks open and close with a pair child; 14 taxa at 8 KB x 3 categories: the parent of
    two cherries holds one pair child and one real cherry (the consumer-fit rule of select_pair_children)"""
    lib = pkg.libiqhip()
    nwk = synth.random_tree_newick(ntaxa, seed)
    model = synth.gtr_model(alpha=0.7, ncat=ncat)
    states = states_of(synth, nwk, model, NPTN, 5, missing=0.05)
    monkeypatch.setenv("IQHIP_LDS_KB", str(kb))     # read when an engine is created
    plan = lnl_against_oracle(pkg, oracle, nwk, states, model)
    A, B = make_tree(pkg, nwk, states, model), make_tree(pkg, nwk, states, model)
    plib, e = planner(pkg, 4, ncat, NPTN, ntaxa)
    try:
        # where the chunks are cut: a planning-only engine of the same shape, budget and op list
        plain(plib, e, ntaxa)
        assert plib.iqhip_debug_plan(e, node_ops(pkg, plan), len(plan)) == 0, plib.iqhip_last_error()
        removed = removed_rows(plib, e, len(plan))
        rule = rule_of(pkg, plan, ncat, kb)
        assert removed == rule and removed
        rows = layout(pkg, plib, e, len(plan) - len(removed))
        chunks = chunks_of(rows, 4 * ncat)
        assert len(chunks) >= 4
        assert any(has_pair(rows[k]) for k, n, _, _ in chunks), "no chunk opens with a pair child"
        assert any(has_pair(rows[k + n - 1]) for k, n, _, _ in chunks), "no chunk closes with a pair child"
        if ntaxa == 14:
            assert len(removed) == len(rule_of(pkg, plan, ncat)) - 1    # one cherry fits at the default budget only
        submit_and_compare(pkg, lib, A, B, plan, len(removed))
    finally:
        plib.iqhip_destroy(e)
        A.close()
        B.close()


@pytest.mark.parametrize("nptn", [NPTN, 65])
@pytest.mark.parametrize("ncat,split", [(3, None), (5, None), (6, None), (6, "1"), (7, None), (8, None), (8, "1")])
def test_every_category_count_bit_for_bit(pkg, synth, oracle, monkeypatch, ncat, split, nptn):
    """the category counts test_pair_children_gpu.py's FORMS leave out, on its 14-taxon tree (parents of two cherries and of a
    cherry and a leaf); the even counts in both lane forms"""
    if split:
        monkeypatch.setenv("IQHIP_LANE_SPLIT", split)
    lib = pkg.libiqhip()
    nwk = synth.random_tree_newick(14, 8)
    model = synth.gtr_model(alpha=0.7, ncat=ncat)
    states = states_of(synth, nwk, model, nptn, 5)
    plan = lnl_against_oracle(pkg, oracle, nwk, states, model)
    A, B = make_tree(pkg, nwk, states, model), make_tree(pkg, nwk, states, model)
    try:
        rule = rule_of(pkg, plan, ncat)
        assert len(rule) >= 3
        submit_and_compare(pkg, lib, A, B, plan, len(rule))
    finally:
        A.close()
        B.close()
