"""CPU: the restatement of Fitch parsimony the device tests compare with (tests/fitch_ref.py) against a brute-force
Sankoff minimum, the host mirror's parsimony-informative flags against the numpy rule, and iqhip_debug_pars_levels -- the
validation and level assignment iqhip_pars_update runs before it launches anything -- case by case."""
import ctypes as C
import os

import numpy as np
import pytest

import fitch_ref as F
from conftest import ROOT

IQHIP_ERR_INVALID = 2
NEW_SYMBOLS = ("iqhip_pars_init", "iqhip_pars_update", "iqhip_pars_branch_scores", "iqhip_pars_insert_scores",
               "iqhip_pars_fetch", "iqhip_debug_pars_levels")
GOLDEN = os.path.join(ROOT, "tests", "golden")


def dna_case(ntaxa, nptn, rng):
    st = F.random_states(ntaxa, nptn, 4, rng, amb_frac=0.15)
    return st, rng.integers(0, 4, size=nptn).astype(float)


def protein_case(ntaxa, nptn, rng):
    """a small alphabet, B / Z / J and STATE_UNKNOWN: the brute force of 8 taxa stays below a million labelings a column"""
    st = rng.integers(0, 6, size=(ntaxa, nptn)).astype(np.uint8)
    amb = rng.random(st.shape) < 0.2
    st[amb] = rng.integers(20, 24, size=int(amb.sum())).astype(np.uint8)
    return st, rng.integers(0, 3, size=nptn).astype(float)


@pytest.mark.parametrize("ntaxa", [4, 5, 6, 7, 8])
@pytest.mark.parametrize("kind", ["dna", "protein"])
def test_restatement_equals_sankoff_minimum(ntaxa, kind):
    rng = np.random.default_rng(100 * ntaxa + (kind == "dna"))
    n = 4 if kind == "dna" else 20
    st, fr = (dna_case(ntaxa, 40, rng) if kind == "dna" else protein_case(ntaxa, 8, rng))
    assert (st >= n).any()
    sp = F.site_patterns(fr)
    adj = F.random_tree(ntaxa, rng)
    tips = F.tip_vectors(st, sp, n)
    dv = F.directed_vectors(adj, tips)
    want = F.sankoff_min(adj, st, sp, n)
    # the same score at every branch of the tree
    for a, b in F.branches(adj):
        assert F.branch_score(dv[(a, b)], dv[(b, a)])[0] == want, (a, b)


def test_insert_score_is_the_score_of_the_tree_with_the_taxon_inserted():
    rng = np.random.default_rng(5)
    st, fr = dna_case(7, 50, rng)
    sp = F.site_patterns(fr)
    tips = F.tip_vectors(st, sp, 4)
    adj = F.random_tree(6, rng, first_internal=7)
    dv = F.directed_vectors(adj, tips)
    for a, b in F.branches(adj):
        grown = {u: list(v) for u, v in adj.items()}
        F.insert_leaf(grown, a, b, 6, 99)
        assert F.insert_score(dv[(a, b)], dv[(b, a)], (tips[6], 0)) == F.tree_score(grown, tips)


def test_stepwise_restatement_recomputes_only_what_an_insertion_invalidated():
    """fitch_ref.stepwise_addition (lazy, what tools/bench_parsimony.py times) against the plain form: every branch scored
    on vectors computed from scratch"""
    rng = np.random.default_rng(8)
    st, fr = dna_case(12, 60, rng)
    tips = F.tip_vectors(st, F.site_patterns(fr), 4)
    order = [int(x) for x in rng.permutation(12)]
    score, adj, nupd, nscan = F.stepwise_addition(tips, order)
    assert nscan == sum(2 * k - 3 for k in range(3, 12)) and nupd < 3 * nscan   # (from scratch: 3 (k - 2) updates a step)
    plain = {12: list(order[:3])}
    for k in order[:3]:
        plain[k] = [12]
    for cur in range(3, 12):
        br = F.ordered_branches(plain, order[0])
        dv = F.directed_vectors(plain, tips)
        sc = [F.insert_score(dv[(a, b)], dv[(b, a)], (tips[order[cur]], 0)) for a, b in br]
        a, b = br[int(np.argmin(sc))]
        added = 12 + cur - 2
        plain[a][plain[a].index(b)] = added
        plain[b][plain[b].index(a)] = added
        plain[added] = [order[cur], a, b]
        plain[order[cur]] = [added]
    assert adj == plain and score == F.tree_score(plain, tips)


def test_padding_bits_never_score():
    st = np.array([[0], [1], [2], [3]], dtype=np.uint8)   # one site, every taxon another state
    tips = F.tip_vectors(st, F.site_patterns([1.0]), 4)
    assert tips.shape == (4, 1, 4) and tips[0, 0, 0] == 0xFFFFFFFF and tips[1, 0, 0] == 0xFFFFFFFE
    assert F.tree_score(F.random_tree(4, np.random.default_rng(0)), tips) == 3


# ---- informative patterns ---------------------------------------------------------------------------------------------
def phylip(rows):
    return "%d %d\n" % (len(rows), len(rows[0])) + "".join("t%d %s\n" % (k, r) for k, r in enumerate(rows))


def test_is_informative_crafted_columns(pkg):
    # constant; singleton; two states twice each; R = A|G makes A x3 and G x2; informative through codes alone (A: A, R;
    # G: G, R); all unknown; unknowns count towards no state (A x2, C, T once); N is unknown: A x2, C x2
    cols = ["AAAAAA", "AAAAAC", "AACCAA", "AACRTG", "ACGRTY", "------", "AAC--T", "AACC-N"]
    want = [0, 0, 1, 1, 1, 0, 0, 1]
    rows = ["".join(c[t] for c in cols) for t in range(6)]
    aln = pkg.Alignment(content=phylip(rows), seq_type="DNA")
    st, fr, sp, _ = aln.arrays()
    flags = aln.informative()
    ref = F.is_informative(st, 4)
    assert np.array_equal(flags, ref)
    assert [int(flags[sp[k]]) for k in range(len(cols))] == want
    assert aln.num_informative_sites == int(fr[flags != 0].sum()) == sum(want)


def test_ambiguity_code_makes_or_breaks_informativeness(pkg):
    # A A C C is informative; A A C Y (Y = C|T) keeps C at two sequences; A A C T is not; A A C R (R = A|G) is not: C once
    cols = ["AACC", "AACY", "AACT", "AACR", "ARCY"]
    rows = ["".join(c[t] for c in cols) for t in range(4)]
    aln = pkg.Alignment(content=phylip(rows), seq_type="DNA")
    st, _, sp, _ = aln.arrays()
    flags = aln.informative()
    assert [int(flags[sp[k]]) for k in range(len(cols))] == [1, 1, 0, 0, 1]
    assert np.array_equal(flags, F.is_informative(st, 4))


@pytest.mark.parametrize("name,n", [("example.phy", 4), ("prot_M126_27_269.phy", 20)])
def test_is_informative_on_the_golden_alignments(pkg, name, n):
    aln = pkg.Alignment(filename=os.path.join(GOLDEN, name))
    assert aln.nstates == n
    st, fr, _, _ = aln.arrays()
    flags = aln.informative()
    assert np.array_equal(flags, F.is_informative(st, n))
    assert 0 < flags.sum() < flags.size
    assert aln.num_informative_sites == int(fr[flags != 0].sum())


# ---- levels and validation --------------------------------------------------------------------------------------------
def tree_ops(adj, ntaxa, root_branch=None):
    """post-order ops towards one branch: (ops rows, slot of every directed vector computed)"""
    a, b = root_branch or F.branches(adj)[0]
    slot, ops = {}, []

    def get(u, v):
        if u < ntaxa:
            return u
        if (u, v) not in slot:
            kids = [k for k in adj[u] if k != v]
            l, r = get(kids[0], u), get(kids[1], u)
            slot[(u, v)] = ntaxa + len(slot)
            ops.append((slot[(u, v)], l, r))
        return slot[(u, v)]

    import sys
    sys.setrecursionlimit(10000)
    get(a, b)
    get(b, a)
    return ops, slot


def test_levels_of_a_caterpillar_and_a_balanced_tree(pkg):
    ntaxa = 40
    ops, _ = tree_ops(F.caterpillar(ntaxa), ntaxa, (ntaxa - 1, 2 * ntaxa - 3))
    assert len(ops) == ntaxa - 2
    lev = pkg.pars_levels(ntaxa, len(ops), ops)
    assert sorted(lev.tolist()) == list(range(len(ops)))   # depth = nops: one op per level
    # balanced: 32 tips, pairs joined level by level into two halves
    ntaxa, ops, cur, nxt = 32, [], list(range(32)), 32
    want = []
    depth = 0
    while len(cur) > 2:
        new = []
        for k in range(0, len(cur), 2):
            ops.append((nxt, cur[k], cur[k + 1]))
            want.append(depth)
            new.append(nxt)
            nxt += 1
        cur = new
        depth += 1
    order = np.random.default_rng(3).permutation(len(ops))   # any order that keeps children before parents per chain
    order = sorted(order, key=lambda k: want[k])
    lev = pkg.pars_levels(ntaxa, len(ops), [ops[k] for k in order])
    assert lev.tolist() == [want[k] for k in order] and max(want) == 3


def refused(pkg, ntaxa, nvec, ops, valid=None, words=None):
    with pytest.raises(pkg.EngineError) as ei:
        pkg.pars_levels(ntaxa, nvec, ops, valid)
    assert ei.value.code == IQHIP_ERR_INVALID
    if words:
        assert words in str(ei.value), str(ei.value)


def test_every_refusal_of_the_validation(pkg):
    T, V = 4, 4
    assert pkg.pars_levels(T, V, [(4, 0, 1), (5, 4, 2)]).tolist() == [0, 1]
    refused(pkg, T, V, [(8, 0, 1)], words="outside")            # dst out of range
    refused(pkg, T, V, [(4, 0, 9)], words="outside")            # child out of range
    refused(pkg, T, V, [(4, -1, 1)], words="outside")
    refused(pkg, T, V, [(2, 0, 1)], words="tip slot")           # dst a tip
    refused(pkg, T, V, [(4, 4, 1)], valid=[1, 0, 0, 0], words="own children")
    refused(pkg, T, V, [(4, 0, 1), (4, 2, 3)], words="twice")   # written twice in one call
    refused(pkg, T, V, [(4, 5, 1)], words="before anything")    # read of a never-written slot
    assert pkg.pars_levels(T, V, [(4, 5, 1)], valid=[0, 1, 0, 0]).tolist() == [0]   # ... written by an earlier call: fine
    # read by op 0 (valid from an earlier call), written by the later op 1
    refused(pkg, T, V, [(4, 5, 1), (5, 2, 3)], valid=[0, 1, 0, 0], words="read by an earlier op")


def test_ops_legal_alone_but_read_before_written_as_a_whole(pkg):
    T, V = 4, 4
    first, second = (5, 4, 2), (4, 0, 1)
    assert pkg.pars_levels(T, V, [second]).tolist() == [0]
    assert pkg.pars_levels(T, V, [first], valid=[1, 0, 0, 0]).tolist() == [0]
    assert pkg.pars_levels(T, V, [second, first]).tolist() == [0, 1]
    refused(pkg, T, V, [first, second], words="before anything")   # slot 4 is read before op 1 writes it


# ---- symbols, planning-only engines -----------------------------------------------------------------------------------
def test_new_symbols_and_planner_refusals(pkg):
    lib = pkg.libiqhip()
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s), s
    assert lib.iqhip_abi_version() == 2
    assert C.sizeof(pkg.ParsOp) == 16
    e = C.c_void_p()
    assert lib.iqhip_debug_create_planner(C.byref(e), 4, 4, 100, 5, 256, 18, 1) == 0
    try:
        i32 = (C.c_int32 * 4)(0, 1, 2, 3)
        op = (pkg.ParsOp * 1)(pkg.ParsOp(5, 0, 1, 0))
        out = (C.c_uint32 * 64)()
        ns = C.c_int64()
        assert lib.iqhip_pars_init(e, None, 16, C.byref(ns)) == IQHIP_ERR_INVALID
        assert b"planning-only" in lib.iqhip_last_error()
        assert lib.iqhip_pars_update(e, op, 1) == IQHIP_ERR_INVALID
        assert lib.iqhip_pars_branch_scores(e, i32, 1, i32, None) == IQHIP_ERR_INVALID
        assert lib.iqhip_pars_insert_scores(e, i32, 1, 2, None, i32, i32) == IQHIP_ERR_INVALID
        assert lib.iqhip_pars_fetch(e, 0, out) == IQHIP_ERR_INVALID
    finally:
        lib.iqhip_destroy(e)
