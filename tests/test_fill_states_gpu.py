"""GPU: k_traverse4's chunk fill stages the leaf state bytes [wave][slot][64] with one LDS-direct load per four leaf
children, requested from a per-slot list of row pointers before the exponentials and tables and waited for at the fill's
closing barrier (kernels_valu4.hip).  Every case runs through the host mirror against the CPU oracle by the rule of
test_parity_gpu.py: lnL <= 1e-9 relative, scale counters exact, vectors 1e-10 of their maximum.  One lane per pattern
(IQHIP_LANE_SPLIT=1) unless a case says otherwise.

The alignments carry IUPAC ambiguity codes in two taxa (the wave-uniform slow path reads the staged byte), unknown
characters (N, gap) in a third (the table's fifth row) and nothing but A, C, G, T in the others, and beyond the first 64
patterns no ambiguity codes at all, so that a leaf child is slow in one wave and fast in the next."""
import ctypes as C

import numpy as np
import pytest

from test_parity_gpu import LNL_RTOL, check_all_vectors
from test_plan_check import planner

pytestmark = pytest.mark.gpu

STATE_UNKNOWN = 18


def balanced_newick(ntaxa, seed, lo=0.02, hi=0.2):
    """unrooted tree whose subtrees split their taxa in halves: cherries at the bottom, joins of two inner nodes above"""
    rng = np.random.default_rng(seed)

    def sub(ids):
        if len(ids) == 1:
            return "%d" % ids[0]
        h = len(ids) // 2
        l1, l2 = rng.uniform(lo, hi, 2)
        return "(%s:%.6f,%s:%.6f)" % (sub(ids[:h]), l1, sub(ids[h:]), l2)
    ids = list(rng.permutation(ntaxa))
    a, b = ntaxa // 3, 2 * ntaxa // 3
    l = rng.uniform(lo, hi, 3)
    return "(%s:%.6f,%s:%.6f,%s:%.6f);" % (sub(ids[:max(a, 1)]), l[0], sub(ids[max(a, 1):max(b, 2)]), l[1], sub(ids[max(b, 2):]), l[2])


def alignment(synth, nwk, model, ntaxa, nptn, seed):
    st = synth.simulate_alignment(nwk, model, nptn, seed)
    rng = np.random.default_rng(seed + 1)
    head = min(nptn, 64)
    for taxon in (1, ntaxa - 1):                      # IUPAC codes R, Y, ... (states 4 .. 17), first wave only
        m = rng.random(head) < 0.3
        st[taxon, :head][m] = rng.integers(4, STATE_UNKNOWN, m.sum())
    m = rng.random(nptn) < 0.3                        # N and gaps, every wave
    st[2, m] = STATE_UNKNOWN
    st[0, nptn - 1] = STATE_UNKNOWN                   # ... and in the last live pattern of the last tile
    return st


class Case:
    """one tree and alignment with its oracle; engines are made per environment"""

    def __init__(self, pkg, synth, oracle, nwk, ntaxa, nptn, seed):
        self.pkg, self.nwk, self.ntaxa = pkg, nwk, ntaxa
        self.model = synth.gtr_model(alpha=0.9, ncat=4)
        self.st = alignment(synth, nwk, self.model, ntaxa, nptn, seed)
        self.freq = np.arange(1, nptn + 1, dtype=np.float64)
        self.ot = oracle.OracleTree(nwk, 4, 0, self.st, self.freq, None, self.model)
        self.ref, _ = self.ot.likelihood()

    def run(self):
        """a fresh engine in the caller's environment: checked against the oracle; returns what must repeat bit for bit"""
        t = self.pkg.PhyloTree(self.nwk)
        t.set_alignment(4, 0, self.st, self.freq)
        t.set_model(self.model)
        t.set_likelihood_kernel(self.pkg.LK_EIGEN_HIP)
        t.attach_engine(0)
        try:
            t.clear_all_partial_lh()
            lnl = t.compute_likelihood()
            assert abs(lnl - self.ref) <= LNL_RTOL * abs(self.ref), (lnl, self.ref)
            assert check_all_vectors(t, self.ot) == self.ntaxa - 2
            vecs = []
            for a in range(t.num_nodes):
                for b, _ in t.neighbors(a):
                    info = t.neighbor_info(a, b)
                    if not self.ot.is_leaf(b) and (info["computed"] & 1) and info["key"] != 0:
                        vecs.append((t.fetch_partial(a, b), t.fetch_scale_num(a, b)))
            return lnl, t.fetch_pattern_lh().copy(), vecs
        finally:
            t.close()


def same_vectors(x, y):
    assert len(x[2]) == len(y[2])
    for (v, s), (w, u) in zip(x[2], y[2]):
        assert np.array_equal(v, w) and np.array_equal(s, u)


def chunk_sizes(pkg, case, nptn):
    """(ops, slots) of every LDS chunk the planner cuts for the case's full traversal, in the caller's environment"""
    t = pkg.PhyloTree(case.nwk)
    t.set_alignment(4, 0, case.st, case.freq)
    t.set_model(case.model)
    t.set_dry_run(True)
    t.clear_all_partial_lh()
    t.compute_likelihood()
    plan = t.last_plan()
    ops = (pkg.NodeOp * len(plan))()
    for k, p in enumerate(plan):
        ops[k] = pkg.NodeOp(p["dst_key"], p["left_key"], p["right_key"], p["left_leaf"], p["right_leaf"],
                            p["left_len"], p["right_len"], p["flags"], 0)
    lib, e = planner(pkg, 4, 4, nptn, case.ntaxa)
    try:
        assert lib.iqhip_debug_plan(e, ops, len(ops)) == 0, lib.iqhip_last_error()
        raw = (C.c_int32 * (8 * len(ops)))()
        assert lib.iqhip_debug_plan_layout(e, raw, len(ops)) == 0, lib.iqhip_last_error()
    finally:
        lib.iqhip_destroy(e)
    out, k = [], 0
    while k < len(ops):
        out.append((raw[8 * k], raw[8 * k + 1]))
        k += raw[8 * k]
    return out


@pytest.fixture(scope="module")
def nine(pkg, synth, oracle):
    return Case(pkg, synth, oracle, synth.random_tree_newick(9, 29), 9, 64, 290)


@pytest.fixture(scope="module")
def seventy(pkg, synth, oracle):
    return Case(pkg, synth, oracle, synth.random_tree_newick(70, 7), 70, 130, 700)


@pytest.mark.parametrize("shape", ["caterpillar", "balanced"])
@pytest.mark.parametrize("ntaxa", [4, 5, 6, 7, 8, 9])
def test_slot_residues(pkg, synth, oracle, monkeypatch, ntaxa, shape):
    """one chunk of ntaxa - 2 ops and 64 patterns: between them the cases' leaf-child counts take every residue mod 4
    (the last request of the chunk fills one, two, three or four slots), with ops of two, one and no leaf child"""
    monkeypatch.setenv("IQHIP_LANE_SPLIT", "1")
    nwk = synth.random_tree_newick(ntaxa, 300 + ntaxa, caterpillar=True) if shape == "caterpillar" else balanced_newick(ntaxa, 400 + ntaxa)
    case = Case(pkg, synth, oracle, nwk, ntaxa, 64, 500 + ntaxa)
    sizes = chunk_sizes(pkg, case, 64)
    assert len(sizes) == 1 and sizes[0][0] == ntaxa - 2 and ntaxa - 1 <= sizes[0][1] - 1 <= ntaxa
    case.run()


def test_slot_residues_cover_all_four(pkg, synth, oracle, monkeypatch):
    """(what the docstring above claims about the twelve cases, from the planner)"""
    monkeypatch.setenv("IQHIP_LANE_SPLIT", "1")
    residues, kinds = set(), set()
    for ntaxa in (4, 5, 6, 7, 8, 9):
        for nwk in (synth.random_tree_newick(ntaxa, 300 + ntaxa, caterpillar=True), balanced_newick(ntaxa, 400 + ntaxa)):
            case = Case(pkg, synth, oracle, nwk, ntaxa, 64, 500 + ntaxa)
            (nops, nslots), = chunk_sizes(pkg, case, 64)
            residues.add((nslots - 1) % 4)
            t = pkg.PhyloTree(nwk)
            t.set_alignment(4, 0, case.st, case.freq)
            t.set_model(case.model)
            t.set_dry_run(True)
            t.clear_all_partial_lh()
            t.compute_likelihood()
            kinds |= {(p["left_leaf"] >= 0) + (p["right_leaf"] >= 0) for p in t.last_plan()}
    assert residues == {0, 1, 2, 3} and kinds == {0, 1, 2}


@pytest.mark.parametrize("nptn", [65, 257])
def test_edge_tiles(pkg, synth, oracle, monkeypatch, nptn):
    """65 patterns: the second wave has one live pattern.  257: a second workgroup with one live wave, whose other waves
    request nothing and take part in the fill's barriers only."""
    monkeypatch.setenv("IQHIP_LANE_SPLIT", "1")
    Case(pkg, synth, oracle, synth.random_tree_newick(9, 31), 9, nptn, 310 + nptn).run()


def test_long_and_short_chunks(pkg, synth, oracle, monkeypatch, seventy):
    """70 taxa x 130 patterns.  As the engine plans it (a small alignment: units of subtrees, chunks of up to 17 ops);
    as ONE chunk of 68 ops and 69 leaf children -- more than the 64 ops a staging pass of the fill takes, so two passes
    and 18 requests per wave (the whole plan as one segment, IQHIP_SPLIT=0, under the largest budget: the default budget
    holds at most 62 leaf children of four categories); and under the smallest budget, many chunks with their slots reused.
    Per-pattern lnL and every vector are the same bits in all three."""
    monkeypatch.setenv("IQHIP_LANE_SPLIT", "1")
    assert max(n for n, _ in chunk_sizes(pkg, seventy, 130)) <= 64
    base = seventy.run()
    monkeypatch.setenv("IQHIP_LDS_KB", "150")
    monkeypatch.setenv("IQHIP_SPLIT", "0")
    assert chunk_sizes(pkg, seventy, 130) == [(68, 70)]
    one = seventy.run()
    monkeypatch.delenv("IQHIP_SPLIT")
    monkeypatch.setenv("IQHIP_LDS_KB", "8")
    assert len(chunk_sizes(pkg, seventy, 130)) >= 12
    many = seventy.run()
    for other in (one, many):
        assert np.array_equal(other[1], base[1])
        same_vectors(other, base)
    monkeypatch.setenv("IQHIP_SPLIT", "0")      # ... and the short chunks inside one segment: every chunk refills the same slots
    sizes = chunk_sizes(pkg, seventy, 130)
    assert len(sizes) >= 10 and sum(n for n, _ in sizes) == 68
    again = seventy.run()
    assert np.array_equal(again[1], base[1])
    same_vectors(again, base)


@pytest.mark.parametrize("which", ["nine", "seventy"])
def test_lane_split(request, monkeypatch, which):
    """two lanes per pattern stage the bytes through registers into the same [wave][slot][64] layout: vectors and counters
    are the one-lane bits; the root lnL of a pattern adds its two category halves in another order (1e-13, as
    test_parity_gpu.py test_lane_split_gives_identical_vectors)"""
    case = request.getfixturevalue(which)
    out = []
    for ls in ("1", "2"):
        monkeypatch.setenv("IQHIP_LANE_SPLIT", ls)
        out.append(case.run())
    same_vectors(out[0], out[1])
    np.testing.assert_allclose(out[1][1], out[0][1], rtol=1e-13, atol=0)
    assert abs(out[1][0] - out[0][0]) <= 1e-13 * abs(out[0][0])
    if which == "seventy":                      # the two-pass chunk with two lanes per pattern
        monkeypatch.setenv("IQHIP_LDS_KB", "150")
        monkeypatch.setenv("IQHIP_SPLIT", "0")
        same_vectors(case.run(), out[0])
