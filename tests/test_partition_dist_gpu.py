"""Joint pairwise distances of a partition group on the device (include/iqhip.h "Joint pairwise distances of a partition
group"): iqhip_partition_pair_distances against restate_joint_matrix of tests/partition_dist_ref.py with the acceptance of
tests/test_pair_dist_gpu.py (equal numbers of derivative evaluations, optimum to 1e-9, d2l to 1e-6); a one-member group
against iqhip_pair_distances bit for bit; the chunking; scaled rates; the agreement with the tree kernels; the refusals;
PhyloSuperTree.fix_negative_branch against its restatement; and PhyloSuperTree.compute_dist / compute_bionj /
fix_negative_branch and `iqhip_lnl -spp parts -bionjtree` end to end.

Every case (partition_dist_ref.part_case; G1 = DNA GTR+G4, DNA with 1 category, protein +G4; G2 = codon with 1 category,
DNA with 12 categories; 5 and 17 taxa; all rates 1 and unequal rates) holds a pair identical in every member (result x1),
a taxon unknown in every member (9 without an evaluation), a taxon with data in one member only, a pair that takes a
bisection step, a non-zero init, an init of exactly 9 and a random-state taxon with init 8.5 whose JC start would be 9; a
counter asserts that each occurred.  The guard of restate_joint_solve rejects an input whose evaluation count could
legitimately differ; the seeds were chosen on the CPU so that it rejects none."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import bionj_ref as br
import partition_dist_ref as R
from test_pair_dist_gpu import assert_matches, device_dist
from test_pair_dist_host import MAX_GENETIC_DIST, MAX_STEPS, X1, X2, XACC, all_pairs

pytestmark = pytest.mark.gpu

IQHIP_ERR_INVALID, IQHIP_ERR_UNSUPPORTED = 2, 3
HERE = os.path.dirname(os.path.abspath(__file__))
BIN = os.path.join(os.path.dirname(HERE), "iq-tree_amd", "lib", "iqhip_lnl")
EXAMPLE = os.path.join(HERE, "golden", "example.phy")
PARTS = ("GTR{1.513,2.393,1.769,1.912,2.838}+F{0.249,0.262,0.251,0.238}+G4{0.934}, first = 1-150\n"
         "HKY{2.0}+G4{0.5}, second = 151-300\n"
         "JC, third = 301-384\n")
DP, I32P = C.POINTER(C.c_double), C.POINTER(C.c_int32)


# ------------------------------------------------------------------------------------------
# groups
# ------------------------------------------------------------------------------------------
def member_tree(pkg, synth, m, ntaxa):
    t = pkg.PhyloTree(synth.random_tree_newick(ntaxa, 1))
    t.set_alignment(m["n"], m["seq_type"], m["pat"], m["freq"])
    t.set_model(m["model"])
    t.set_likelihood_kernel(pkg.LK_EIGEN_HIP)
    t.attach_engine(0)
    return t


class Group:
    """member trees with engines and their group"""

    def __init__(self, pkg, synth, members, rates=None):
        self.pkg, self.T = pkg, members[0]["pat"].shape[0]
        self.trees = [member_tree(pkg, synth, m, self.T) for m in members]
        self.g = pkg.PartitionGroup(self.trees)
        if rates is not None:
            self.g.set_rates(rates)

    def raw(self, init=None, x1=X1, x2=X2, xacc=XACC, max_steps=MAX_STEPS, dist_null=False):
        """iqhip_partition_pair_distances -> (status, dist, d2l, nsteps)"""
        T = self.T
        dist, d2l, nst = np.full((T, T), -1.0), np.full((T, T), -1.0), np.full((T, T), -1, dtype=np.int32)
        ini = None if init is None else np.ascontiguousarray(init, dtype=np.float64)
        rc = self.pkg.libiqhip().iqhip_partition_pair_distances(
            self.g.h, None if ini is None else ini.ctypes.data_as(DP), x1, x2, xacc, max_steps,
            None if dist_null else dist.ctypes.data_as(DP), d2l.ctypes.data_as(DP), nst.ctypes.data_as(I32P))
        return rc, dist, d2l, nst

    def close(self):
        self.g.close()
        for t in self.trees:
            t.close()


def same_bits(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------
# distances
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group,ntaxa,rates", R.CASES)
def test_distances_match_the_restated_joint_solve(pkg, synth, group, ntaxa, rates):
    members, init, r, ref = R.solved_part_case(synth, group, ntaxa, rates)
    T = ntaxa
    G = Group(pkg, synth, members, r)
    rc, dist, d2l, nst = G.raw(init)
    assert rc == 0, pkg.libiqhip().iqhip_last_error()
    assert_matches((dist, d2l, nst), ref, T)
    assert dist[0, T - 3] == X1                                                       # identical in every member
    assert (dist[T - 1, :T - 1] == MAX_GENETIC_DIST).all() and not nst[T - 1].any() and not d2l[T - 1].any()
    assert dist[1, T - 3] == MAX_GENETIC_DIST and nst[1, T - 3] == 0 and d2l[1, T - 3] == 0.0   # init of exactly 9
    assert nst[0, T - 2] >= 2 and nst[T - 4, T - 2] >= 2                              # init 8.5 is solved from
    # the wrapper of the Python layer gives the same matrices
    got = G.g.pair_distances(init)
    assert same_bits(got, (dist, d2l, nst))
    G.close()


@pytest.mark.parametrize("group,member", [("G1", 0), ("G1", 1), ("G1", 2), ("G2", 0), ("G2", 1)])
def test_one_member_at_rate_one_is_the_plain_call_bit_for_bit(pkg, synth, group, member):
    members, init = R.part_case(synth, group, 17)
    m = members[member]
    T = 17
    G = Group(pkg, synth, [m])
    rc, dist, d2l, nst = G.raw(init)
    assert rc == 0, pkg.libiqhip().iqhip_last_error()
    prc, pdist, pd2l, pnst = device_dist(pkg, G.trees[0], init)
    assert prc == 0
    cnt = R.member_counts([m], all_pairs(T))[0]
    solved = 0
    for k, (i, j) in enumerate(all_pairs(T)):
        start = init[i, j] if init[i, j] != 0.0 else R.restate_super_jc([cnt[k]])
        if start == MAX_GENETIC_DIST:   # returned as it is here, solved from 9 by the plain call
            assert (dist[i, j], d2l[i, j], nst[i, j]) == (MAX_GENETIC_DIST, 0.0, 0) and pnst[i, j] >= 1
            continue
        solved += 1
        assert (dist[i, j].tobytes(), d2l[i, j].tobytes(), nst[i, j]) == (pdist[i, j].tobytes(), pd2l[i, j].tobytes(), pnst[i, j]), (i, j)
    assert solved >= 60
    G.close()


def test_chunks_and_repeats_do_not_change_a_bit(pkg, synth, monkeypatch):
    members, init, r, _ = R.solved_part_case(synth, "G1", 17, "unequal")
    G = Group(pkg, synth, members, r)
    rc, *first = G.raw(init)
    assert rc == 0
    rc, *again = G.raw(init)
    assert rc == 0 and same_bits(again, first)
    for chunk in ("37", "1"):                                    # 136 pairs in 4 chunks / one pair per chunk
        monkeypatch.setenv("IQHIP_PAIR_CHUNK", chunk)
        rc, *got = G.raw(init)
        assert rc == 0 and same_bits(got, first), chunk
    G.close()


def test_a_rate_set_after_the_first_call_is_picked_up(pkg, synth):
    members, init, r1, ref1 = R.solved_part_case(synth, "G2", 5, "ones")
    _, _, r2, ref2 = R.solved_part_case(synth, "G2", 5, "unequal")
    G = Group(pkg, synth, members)
    rc, *a = G.raw(init)
    assert rc == 0
    assert_matches(a, ref1, 5)
    G.g.set_rates(r2)
    rc, *b = G.raw(init)
    assert rc == 0
    assert_matches(b, ref2, 5)
    assert a[0].tobytes() != b[0].tobytes()
    G.close()


@pytest.mark.parametrize("c", [2.0, 0.5])
def test_rates_scaled_by_c_scale_the_distances(pkg, synth, c):
    """f_c(x) = f_1(c x): the optimum of every pair moves to x* / c.  minimizeNewton returns the iterate before its first
    step shorter than xacc, which lies within 1.01 xacc of the optimum (the argument of test_pair_dist_gpu.py
    test_agrees_with_the_tree_kernels), so |c x_c - x_1| <= c 1.01 xacc + 1.01 xacc = 1.01 xacc (c + 1) for every pair with an
    interior optimum under both rate sets."""
    members, _, r, _ = R.solved_part_case(synth, "G1", 17, "unequal")
    G = Group(pkg, synth, members, r)
    rc, d1, _, n1 = G.raw(None)
    assert rc == 0
    G.g.set_rates(c * r)
    rc, dc, _, nc = G.raw(None)
    assert rc == 0
    checked = 0
    for (i, j) in all_pairs(17):
        if n1[i, j] == 0 or nc[i, j] == 0 or not (100 * X1 < d1[i, j] < 0.4 * X2):   # (interior for c = 2 and c = 0.5 alike)
            continue
        checked += 1
        print((i, j), d1[i, j], dc[i, j], abs(c * dc[i, j] - d1[i, j]))
        assert abs(c * dc[i, j] - d1[i, j]) <= 1.01 * XACC * (c + 1.0), (i, j, d1[i, j], dc[i, j])
    assert checked >= 25
    G.close()


def test_agrees_with_the_tree_kernels(pkg, synth):
    """The super tree (0:a, 1:x1, 2:c) with taxon 2 unknown in every member, no ambiguous state in taxa 0 and 1 and unequal
    rates: member p's likelihood of a pattern is pi[s0] * sum_c props[c] P_c[s0][s1](r_p (a + x1)), its function of the pair
    at r_p x up to the constant pi[s0].  So the joint optimum a* of branch (0, centre) satisfies a* + x1 = d*, the joint
    optimum of the pair; two results each within 1.01 xacc of their optimum: |a + x1 - dist[0, 1]| <= 2.02 xacc."""
    rates = np.array([0.4, 1.0, 2.5])
    parts = []
    for k, (model, n, seq_type, nsite) in enumerate(((synth.gtr_model(alpha=0.9, ncat=4), 4, 0, 500),
                                                       (synth.gtr_model(alpha=None, ncat=1), 4, 0, 63),
                                                       (synth.random_reversible_model(20, 5, alpha=0.9, ncat=4), 20, 1, 200))):
        st = synth.simulate_alignment("(0:0.15,1:0.2,2:0.1);", model, nsite, 5 + k)
        st[2] = 18 if n == 4 else 23
        pat, freq = synth.compress_patterns(st)
        parts.append(dict(nstates=n, seq_type=seq_type, pat=pat, freq=freq, model=model))
    st = pkg.PhyloSuperTree("(0:0.1,1:%r,2:0.3);" % X1, parts)
    st.part_rates = rates
    dist = st.compute_dist()
    st.compute_likelihood()
    centre = st.neighbors(0)[0][0]
    a = st.optimize_one_branch(0, centre)
    print(a, dist[0, 1])
    assert 0.05 < dist[0, 1] < 1.0
    assert abs(a + X1 - dist[0, 1]) <= 2.02 * XACC
    assert dist[0, 2] == MAX_GENETIC_DIST and dist[1, 2] == MAX_GENETIC_DIST
    st.close()


# ------------------------------------------------------------------------------------------
# refusals
# ------------------------------------------------------------------------------------------
def test_refusals(pkg, synth):
    lib = pkg.libiqhip()
    members, init, r, ref = R.solved_part_case(synth, "G1", 5, "unequal")
    G = Group(pkg, synth, members, r)

    def refused(want, word, **kw):
        rc = G.raw(**kw)[0]
        assert rc == want and word in lib.iqhip_last_error(), (rc, lib.iqhip_last_error())
        rc, *got = G.raw(init)                                   # and the group still works
        assert rc == 0
        assert_matches(got, ref, 5)

    refused(IQHIP_ERR_INVALID, b"null argument", dist_null=True)
    refused(IQHIP_ERR_INVALID, b"x1 <= x2", x1=2.0, x2=1.0)
    refused(IQHIP_ERR_INVALID, b"max_steps", max_steps=0)
    refused(IQHIP_ERR_INVALID, b"tolerance", xacc=0.0)
    refused(IQHIP_ERR_INVALID, b"bounds", x1=-1.0)
    refused(IQHIP_ERR_INVALID, b"bounds", x2=math.inf)
    for bad in (-0.5, math.nan, math.inf):
        ini = init.copy()
        ini[2, 3] = ini[3, 2] = bad
        refused(IQHIP_ERR_INVALID, b"initial distance", init=ini)
    dist = np.zeros((5, 5))
    assert lib.iqhip_partition_pair_distances(None, None, X1, X2, XACC, MAX_STEPS, dist.ctypes.data_as(DP), None, None) == IQHIP_ERR_INVALID
    assert b"null group" in lib.iqhip_last_error()

    # members with different taxon counts
    six = R.member_data(synth, "gtr_g4", 6, 40, 3, synth.random_tree_newick(6, 3, 0.02, 0.4))
    t6 = member_tree(pkg, synth, six, 6)
    mixed = pkg.PartitionGroup([G.trees[0], t6])
    with pytest.raises(pkg.EngineError) as ex:
        mixed.pair_distances(ntaxa=5)
    assert ex.value.code == IQHIP_ERR_INVALID and "number of taxa" in str(ex.value)
    mixed.close()
    t6.close()

    # a member with an embedded state count (binary data on the 4-state kernels)
    rng = np.random.default_rng(2)
    two = pkg.PhyloTree(synth.random_tree_newick(5, 1))
    two.set_alignment(2, 3, rng.integers(0, 2, size=(5, 70)).astype(np.uint8), np.ones(70))
    two.set_model(synth.random_reversible_model(2, 4, alpha=0.7, ncat=4))
    two.set_likelihood_kernel(pkg.LK_EIGEN_HIP)
    two.attach_engine(0)
    emb = pkg.PartitionGroup([G.trees[0], two])
    with pytest.raises(pkg.EngineError) as ex:
        emb.pair_distances(ntaxa=5)
    assert ex.value.code == IQHIP_ERR_UNSUPPORTED and "states" in str(ex.value)
    emb.close()
    two.close()

    rc, *got = G.raw(init)                                       # the members serve their own group as before
    assert rc == 0
    assert_matches(got, ref, 5)
    G.close()


# ------------------------------------------------------------------------------------------
# PhyloSuperTreePlen::fixNegativeBranch
# ------------------------------------------------------------------------------------------
def super_lengths(st):
    return {(a, b): l for a in range(st.num_nodes) for b, l in st.neighbors(a)}


@pytest.mark.parametrize("force", [False, True])
@pytest.mark.parametrize("group", ["G1", "G2"])
def test_fix_negative_branch(pkg, synth, group, force):
    T = 17
    members, _ = R.part_case(synth, group, T)
    rates = R.case_rates(group, "unequal")
    nwk = synth.random_tree_newick(T, 4)
    lens = re.findall(r":([0-9.eE+-]+)", nwk)
    assert len(lens) == 2 * T - 3
    neg = {1, 5, 6, 20, 30}                                      # these branches get a negative length, one a zero length
    it = iter(range(len(lens)))
    nwk = re.sub(r":([0-9.eE+-]+)", lambda m: (lambda k: ":-0.0%d" % (k + 1) if k in neg else (":0.0" if k == 9 else m.group(0)))(next(it)), nwk)
    st = pkg.PhyloSuperTree(nwk, members)
    st.part_rates = rates
    before = super_lengths(st)
    assert sum(1 for l in before.values() if l < 0.0) == 2 * len(neg)
    fixed = st.fix_negative_branch(force)
    after = super_lengths(st)
    nsites = [float(m["freq"].sum()) for m in members]
    seq_types = [m["seq_type"] for m in members]
    branches = [(a, b) for (a, b) in before if a < b]
    assert len(branches) == 2 * T - 3
    want_fixed = 0
    for (a, b) in branches:
        mlen = []
        for p, (m, t) in enumerate(zip(members, st.members)):
            l = rates[p] * before[(a, b)]                         # mapTrees: the member's own length
            if l < 0.0 or force:
                subst = t.parsimony_branch(a, b)[1]
                l = R.restate_fix_length(subst, nsites[p], m["n"])
                want_fixed += 1
            if l <= 0.0:
                l = 1e-6
            mlen.append(l)
        want = R.restate_weighted_mean(mlen, nsites, seq_types)
        assert after[(a, b)] == want and after[(b, a)] == want, (a, b, after[(a, b)], want, mlen)
        for p, t in enumerate(st.members):
            assert dict(t.neighbors(a))[b] == rates[p] * want    # the members get rate x super length again
    assert fixed == want_fixed == len(members) * (len(branches) if force else len(neg))
    assert min(after.values()) > 0.0
    assert math.isfinite(st.compute_likelihood())
    st.close()


def test_fix_negative_branch_without_a_negative_length_changes_nothing(pkg, synth):
    members, _ = R.part_case(synth, "G1", 5)
    st = pkg.PhyloSuperTree(synth.random_tree_newick(5, 4), members)
    before = super_lengths(st)
    assert st.fix_negative_branch(False) == 0
    assert super_lengths(st) == before
    st.close()


# ------------------------------------------------------------------------------------------
# end to end
# ------------------------------------------------------------------------------------------
def test_starting_tree_python_and_command_line(pkg, tmp_path):
    part = tmp_path / "parts.txt"
    part.write_text(PARTS)
    names, parts = pkg.read_partition_file(EXAMPLE, str(part))
    T = len(names)
    star = "(" + ",".join("%s:0.1" % n for n in names) + ");"
    st = pkg.PhyloSuperTree(star, parts, names=names)
    assert np.array_equal(st.part_rates, np.ones(3))
    dist, d2l = st.compute_dist(want_d2l=True)
    np.testing.assert_array_equal(dist, dist.T)
    assert not np.diag(dist).any() and (dist[~np.eye(T, dtype=bool)] >= X1).all() and d2l.shape == (T, T)

    pre = tmp_path / "x"
    r = subprocess.run([BIN, "-s", EXAMPLE, "-spp", str(part), "-bionjtree", "-pre", str(pre)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr + r.stdout
    mldist, bionj = tmp_path / "x.mldist", tmp_path / "x.bionj"
    # the .mldist text is the Python matrix in the format of test_pair_dist_gpu.test_compute_dist_python_and_command_line
    lines = mldist.read_text().split("\n")
    assert lines[0] == str(T) and lines[-1] == "" and len(lines) == T + 2
    width = max(10, max(len(s) for s in names))
    for i, ln in enumerate(lines[1:T + 1]):
        assert ln[:width + 1] == names[i].ljust(width) + " " and ln.endswith(" ")
        vals = ln[width + 1:].split(" ")
        assert vals[-1] == "" and len(vals) == T + 1
        assert vals[:T] == ["%.7f" % v for v in dist[i]], (i, vals[:3])
    # the tree is a function of the file: BIONJ on the text's matrix gives the .bionj text
    fnames, fdist = br.parse_matrix_text(mldist.read_text())
    assert fnames == list(names)
    nwk = st.compute_bionj(fdist)
    assert bionj.read_text() == nwk + "\n"
    assert st.num_leaves == T and st.num_nodes == 2 * T - 2
    assert all(t.num_nodes == 2 * T - 2 for t in st.members)
    fixed = st.fix_negative_branch(False)
    assert re.search(r"BIONJ tree: [0-9.]+ s, printed to %s\.bionj" % re.escape(str(pre)), r.stdout), r.stdout
    m = re.search(r"^(\d+) negative branch lengths fixed$", r.stdout, re.M)
    assert m and int(m.group(1)) == fixed, r.stdout
    st.read_tree(st.tree_string())                               # (the driver goes on from the tree's text, as -te would)
    total = st.compute_likelihood()
    m = re.search(r"^Log-likelihood of the input tree: (\S+)$", r.stdout, re.M)
    assert m and abs(float(m.group(1)) - total) <= 1e-9 * abs(total), (m and m.group(1), total)
    # ... and on to the optimised partition model
    m = re.search(r"^Optimal log-likelihood: (\S+)$", r.stdout, re.M)
    assert m and float(m.group(1)) >= total - 1e-6 * abs(total), r.stdout
    assert (tmp_path / "x.treefile").exists()
    st.close()


def test_command_line_bionjtree_with_search_and_refusals(tmp_path):
    part = tmp_path / "parts.txt"
    part.write_text(PARTS)
    pre = tmp_path / "s"
    out = tmp_path / "named.mldist"
    rows = open(EXAMPLE).read().split("\n")[1:11]                # the first ten sequences: a search of a few seconds
    small = tmp_path / "small.phy"
    small.write_text(" 10 384\n" + "\n".join(rows) + "\n")
    r = subprocess.run([BIN, "-s", str(small), "-q", str(part), "-bionjtree", "-mldist", str(out), "-search", "-n", "2", "-pre", str(pre)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr + r.stdout
    assert out.exists() and (tmp_path / "s.bionj").exists() and not (tmp_path / "s.mldist").exists()
    assert re.search(r"^Tree search: \d+ iterations", r.stdout, re.M), r.stdout
    # a tree next to -bionjtree or -mldist, and -bb, stay refused
    tree = str(tmp_path / "s.bionj")
    for extra in (["-te", tree, "-bionjtree"], ["-te", tree, "-mldist", str(out)], ["-t", tree, "-bionjtree"],
                  ["-bionjtree", "-bb", "100"], ["-te", tree, "-bb", "100"]):
        r = subprocess.run([BIN, "-s", EXAMPLE, "-q", str(part)] + extra, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "cannot be combined with" in r.stderr, (extra, r.stderr)
    r = subprocess.run([BIN, "-s", EXAMPLE, "-q", str(part), "-mldist", str(out)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "usage" in r.stderr              # neither a tree nor -bionjtree
