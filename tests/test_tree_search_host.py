"""Host, no GPU: the tree edits of the NNI search (do_nni, change_nni_brans, save / restore_branch_lengths, do_random_nni) on
dry-run trees against pure-Python topology arithmetic, and the pure decisions of iq-tree_amd/host/search_host.h
(select_non_conflicting, the stable sort, branches_for_nni, CandidateSet, the stop rule, bootstrap_correlation, the random
stream) against restatements (tests/nni_search_ref.py) and numpy."""
import numpy as np
import pytest

import nni_search_ref as ref

TAXA = (4, 5, 8, 13)


def make(pkg, synth, ntaxa, seed=3, mem_mode=0):
    nwk = synth.random_tree_newick(ntaxa, seed)
    t = pkg.PhyloTree(nwk)
    t.set_mem_mode(mem_mode)
    t.set_alignment(4, 0, np.zeros((ntaxa, 8), dtype=np.uint8), np.ones(8))
    t.set_model(synth.gtr_model())
    t.set_dry_run(True)
    return t


def adjacency_splits(adj, ntaxa):
    """the non-trivial splits of a tree given as adjacency lists: per internal branch the side without taxon 0"""
    out = set()

    def below(node, dad):
        if len(adj[node]) == 1:
            return {node}
        s = set()
        for nb in adj[node]:
            if nb != dad:
                s |= below(nb, node)
        return s

    for a, b in ref.internal_branches(adj):
        side = below(b, a)
        if 0 in side:
            side = set(range(ntaxa)) - side
        out.add(frozenset(side))
    return out


def swapped(adj, m):
    """the adjacency after the NNI: the subtree at node1_nei goes to node2, the one at node2_nei to node1"""
    adj = [list(a) for a in adj]
    for at, frm, to in ((m["node1"], m["node1_nei"], m["node2_nei"]), (m["node2"], m["node2_nei"], m["node1_nei"]),
                        (m["node1_nei"], m["node1"], m["node2"]), (m["node2_nei"], m["node2"], m["node1"])):
        adj[at][adj[at].index(frm)] = to
    return adj


def all_moves(adj):
    """both NNIs of every internal branch: the first other neighbour of node1 against each other neighbour of node2"""
    moves = []
    for a, b in ref.internal_branches(adj):
        s1 = [x for x in adj[a] if x != b]
        for x in (y for y in adj[b] if y != a):
            moves.append(dict(node1=a, node2=b, node1_nei=s1[0], node2_nei=x))
    return moves


@pytest.mark.parametrize("ntaxa", TAXA)
@pytest.mark.parametrize("mem_mode", (0, 1))
def test_do_nni_gives_the_neighbour_topology_and_undoes_itself(pkg, synth, ntaxa, mem_mode):
    t = make(pkg, synth, ntaxa, 10 + ntaxa, mem_mode)
    t.initialize_all_partial_lh()
    t.compute_likelihood()                                  # dry run: flags up, LM_PER_NODE buffers oriented
    start = t.tree_string()
    adj = ref.adjacency(t)
    assert len(all_moves(adj)) == 2 * (ntaxa - 3)
    for m in all_moves(adj):
        t.do_nni(m)
        assert set(pkg.newick_splits(t.tree_string(), ntaxa)) == adjacency_splits(swapped(adj, m), ntaxa)
        assert ref.adjacency(t) == swapped(adj, m)          # neighbour slots are kept: the subtrees trade places
        if mem_mode == 0:                                   # LM_PER_NODE: still one buffer per internal node
            for v in range(ntaxa, t.num_nodes):
                assert sum(1 for u, _ in t.neighbors(v) if t.neighbor_info(u, v)["key"]) == 1
        t.compute_likelihood()                              # the plan of the edited tree is valid
        t.do_nni(m)
        assert t.tree_string() == start                     # byte for byte, neighbour order included
    t.do_nni(all_moves(adj)[0], clear_lh=False)
    assert t.tree_string() != start


def test_do_nni_clears_what_looks_through_the_branch(pkg, synth):
    t = make(pkg, synth, 9, 5, mem_mode=1)
    t.set_dry_run(True)
    t.compute_likelihood()
    adj = ref.adjacency(t)
    m = all_moves(adj)[2]
    for a in range(t.num_nodes):                            # make every directed vector "valid"
        for b in adj[a]:
            if len(adj[b]) > 1:
                t.compute_partial_likelihood(a, b)
    t.do_nni(m)
    new = ref.adjacency(t)

    def below(node, dad):
        s = {node}
        for nb in new[node]:
            if nb != dad:
                s |= below(nb, node)
        return s

    for a in range(t.num_nodes):
        for b in new[a]:
            if len(new[b]) == 1:
                continue
            # the vector of a -> b summarises the subtree at b away from a: stale iff that subtree holds the central branch
            stale = {m["node1"], m["node2"]} <= below(b, a) or (a, b) in ((m["node1"], m["node2"]), (m["node2"], m["node1"]))
            assert bool(t.neighbor_info(a, b)["computed"] & 1) == (not stale), (a, b)


@pytest.mark.parametrize("ntaxa", (8, 13))
def test_apply_then_revert_in_the_same_order_restores_the_tree(pkg, synth, ntaxa):
    t = make(pkg, synth, ntaxa, 21)
    start = t.tree_string()
    moves = all_moves(ref.adjacency(t))[::2]
    for k, m in enumerate(moves):
        m["newloglh"] = -float(k)
    chosen = ref.non_touching(ref.select_non_conflicting(moves))
    assert len(chosen) >= 2
    lens = t.save_branch_lengths()
    for k, m in enumerate(chosen):
        t.do_nni(m)
        t.change_nni_brans(dict(m, new_lens=[1.0 + k, 1.1 + k, 1.2 + k, 1.3 + k, 1.4 + k]), nni5=True)
    assert t.tree_string() != start
    for m in chosen:
        t.do_nni(m)
    t.restore_branch_lengths(lens)
    assert t.tree_string() == start
    with pytest.raises(pkg.HostError, match="restoreBranchLengths"):
        t.restore_branch_lengths(lens[:-1])


@pytest.mark.parametrize("ntaxa", TAXA)
@pytest.mark.parametrize("nni5", (True, False))
def test_change_nni_brans_follows_the_evaluation_order(pkg, synth, ntaxa, nni5):
    """In a dry run the Newton solve returns at once, so nni_for_branch reports for newLen[i] the CURRENT length of the
    branch it optimises i-th; the random lengths are distinct, which names that branch by the node at its outer end."""
    t = make(pkg, synth, ntaxa, 31 + ntaxa)
    adj = ref.adjacency(t)
    length = {(a, b): ln for a in range(t.num_nodes) for b, ln in t.neighbors(a)}
    assert len(set(length.values())) == t.num_nodes - 1
    for a, b in ref.internal_branches(adj):
        for cnt, (_, nei1, nei2, lens) in enumerate(t.nni_for_branch(a, b, nni5=nni5)):
            m = dict(node1=a, node2=b, node1_nei=nei1, node2_nei=nei2, new_lens=[10.0, 11.0, 12.0, 13.0, 14.0])
            outer = []                                      # the outer end of the branch newLen[1..4] was reported for
            for i in range(1, 5 if nni5 else 1):
                outer += [x for x in adj[a] + adj[b] if x not in (a, b) and lens[i] in (length[(a, x)] if x in adj[a] else None,
                                                                                        length[(b, x)] if x in adj[b] else None)]
            assert lens[0] == length[(a, b)] and len(outer) == (4 if nni5 else 0)
            before = t.tree_string()
            t.do_nni(m)
            t.change_nni_brans(m, nni5)
            now = {(u, v): ln for u in range(t.num_nodes) for v, ln in t.neighbors(u)}
            assert now[(a, b)] == now[(b, a)] == 10.0
            for i, x in enumerate(outer):
                at = a if x in ref.adjacency(t)[a] else b
                assert now[(at, x)] == now[(x, at)] == 11.0 + i
            if not nni5:
                assert sum(1 for v in now.values() if v >= 10.0) == 2
            t.do_nni(m)                                     # undo, lengths back
            for (u, v), ln in length.items():
                t.set_branch_length(u, v, ln)
            assert t.tree_string() == before


def test_do_random_nni_takes_the_neighbours_the_coins_name(pkg, synth):
    t = make(pkg, synth, 9, 41)
    for bit1 in (0, 1):
        for bit2 in (0, 1):
            adj = ref.adjacency(t)
            a, b = ref.internal_branches(adj)[1]
            want = dict(node1=a, node2=b, node1_nei=[x for x in adj[a] if x != b][bit1], node2_nei=[x for x in adj[b] if x != a][bit2])
            assert t.do_random_nni(a, b, bit1, bit2) == want
            assert ref.adjacency(t) == swapped(adj, want)
    with pytest.raises(pkg.HostError, match="internal branch"):
        t.do_random_nni(0, t.neighbors(0)[0][0], 0, 0)
    with pytest.raises(pkg.HostError, match="does not belong"):
        t.do_nni(dict(node1=a, node2=b, node1_nei=0, node2_nei=0))


def draw_moves(rng, n, nnodes, ties):
    scores = rng.integers(0, 4, n).astype(float) if ties else rng.normal(size=n)
    return [dict(node1=int(rng.integers(0, nnodes)), node2=int(rng.integers(0, nnodes)), newloglh=float(s), tag=k)
            for k, s in enumerate(scores)]


@pytest.mark.parametrize("ties", (False, True))
def test_sort_and_select_non_conflicting(pkg, ties):
    rng = np.random.default_rng(7 + ties)
    for trial in range(40):
        moves = draw_moves(rng, int(rng.integers(0, 30)), 12, ties)
        want = sorted(moves, key=lambda m: -m["newloglh"])                     # Python's sort is stable
        got = pkg.sort_moves(moves)
        assert [m["tag"] for m in got] == [m["tag"] for m in want]
        sel = pkg.select_non_conflicting(got)
        one_liner = [m for k, m in enumerate(want)
                     if not any({m["node1"], m["node2"]} & {p["node1"], p["node2"]} for p in ref.select_non_conflicting(want[:k]))]
        assert [m["tag"] for m in sel] == [m["tag"] for m in one_liner] == [m["tag"] for m in ref.select_non_conflicting(want)]


@pytest.mark.parametrize("ntaxa", (4, 5, 8, 13, 30))
def test_branches_for_nni(pkg, synth, ntaxa):
    t = make(pkg, synth, ntaxa, 51 + ntaxa)
    adj = ref.adjacency(t)
    inner = ref.internal_branches(adj)
    rng = np.random.default_rng(ntaxa)
    for trial in range(10):
        k = int(rng.integers(1, min(4, len(inner)) + 1))
        applied = [dict(node1=inner[i][int(f)], node2=inner[i][1 - int(f)])
                   for i, f in zip(rng.choice(len(inner), k, replace=False), rng.integers(0, 2, k))]
        got = pkg.branches_for_nni([(m["node1"], m["node2"]) for m in applied], adj)
        assert got == ref.branches_for_nni(applied, adj)
        assert len({frozenset(b) for b in got}) == len(got) and {frozenset(b) for b in got} <= {frozenset(b) for b in inner}
        # every internal branch within two steps of the FIRST applied branch is listed (a later move's walk stops at
        # branches that are listed already, as the reference's does)
        ends = {applied[0]["node1"], applied[0]["node2"]}
        ring1 = {frozenset(b) for b in inner if set(b) & ends}
        ring2 = {frozenset(b) for b in inner if set(b) & set().union(*ring1)}
        assert ring2 <= {frozenset(b) for b in got}
        assert got[0] == (applied[0]["node1"], applied[0]["node2"])
    assert pkg.branches_for_nni([], adj) == []


def test_candidate_set(pkg):
    cs, rs = pkg.CandidateSet(), ref.CandidateSet()
    for tree, topo, score in (("A1", "A", -10.0), ("B1", "B", -12.0), ("A2", "A", -11.0), ("A3", "A", -9.0), ("C1", "C", -9.0)):
        assert cs.update(tree, topo, score) == rs.update(tree, topo, score)
    # A: the worse score was ignored, the better one replaced the tree; C ties with A and, inserted later, ranks first
    assert [e[1] for e in cs.top_trees()] == ["C1", "A3", "B1"] == [e[1] for e in rs.ranked()]
    assert cs.best_score == -9.0 and len(cs) == 3
    assert cs.tree_topology_exist("B") and not cs.tree_topology_exist("D")
    # getRandCandTree with fewer than popSize trees draws among those present only
    ranks = {cs.rand_cand_rank(5, pkg.search_rand(1, 2, d)) for d in range(200)}
    assert ranks == {0, 1, 2}
    assert {cs.rand_cand_rank(2, pkg.search_rand(1, 2, d)) for d in range(200)} == {0, 1}
    with pytest.raises(pkg.HostError, match="empty"):
        pkg.CandidateSet().rand_cand_rank(5, 1)
    # eviction at maxCandidates: a better new topology pushes the worst out; a worse one is inserted all the same
    small, rsmall = pkg.CandidateSet(3), ref.CandidateSet(3)
    for k, score in enumerate((-5.0, -4.0, -3.0, -2.0, -6.0)):
        assert small.update("t%d" % k, "T%d" % k, score) == rsmall.update("t%d" % k, "T%d" % k, score)
    assert [e[1] for e in small.top_trees()] == ["t3", "t2", "t1", "t4"] == [e[1] for e in rsmall.ranked()]
    assert not small.tree_topology_exist("T0")


def test_stop_rule_boundaries(pkg):
    F, U, B = pkg.SC_FIXED_ITERATION, pkg.SC_UNSUCCESS_ITERATION, pkg.SC_BOOTSTRAP_CORRELATION
    assert not pkg.stop_rule(F, 7, min_iteration=7) and pkg.stop_rule(F, 8, min_iteration=7)
    assert not pkg.stop_rule(U, 104, unsuccess_iteration=100, last_improved=5)
    assert pkg.stop_rule(U, 105, unsuccess_iteration=100, last_improved=5)
    kw = dict(unsuccess_iteration=100, last_improved=5, min_correlation=0.99, max_iteration=1000)
    assert pkg.stop_rule(B, 105, 0.99, **kw) and not pkg.stop_rule(B, 105, 0.9899, **kw)
    assert not pkg.stop_rule(B, 104, 1.0, **kw)
    assert not pkg.stop_rule(B, 1000, 0.0, **kw) and pkg.stop_rule(B, 1001, 0.0, **kw)


def test_bootstrap_correlation(pkg):
    s = [frozenset(x) for x in ((1, 2), (3, 4), (5, 6), (1, 2, 3, 4), (2, 3), (4, 5))]
    half = {s[0]: 100, s[1]: 80, s[2]: 55, s[3]: 30, s[4]: 7}
    now = {s[0]: 98, s[1]: 85, s[2]: 40, s[3]: 33, s[5]: 12}                    # s[4] left, s[5] new
    x = [100, 80, 55, 30, 7, 0]
    y = [98, 85, 40, 33, 0, 12]
    want = float(np.corrcoef(x, y)[0, 1])
    assert abs(pkg.bootstrap_correlation([half, now], 8) - want) <= 1e-14
    assert abs(ref.pearson(x, y) - want) <= 1e-14
    # the table at index (n - 1) // 2 against the last one
    other = {s[0]: 1, s[1]: 2, s[2]: 3}
    assert abs(pkg.bootstrap_correlation([other, half, other, now], 8) - want) <= 1e-14
    assert abs(pkg.bootstrap_correlation([half, other, now], 8) - float(np.corrcoef([1, 2, 3, 0, 0], [98, 85, 40, 33, 12])[0, 1])) <= 1e-14
    # trivial splits are not compared
    with_trivial = [{**half, frozenset((3,)): 100}, {**now, frozenset((7,)): 100, frozenset(range(1, 8)): 100}]
    assert abs(pkg.bootstrap_correlation(with_trivial, 8) - want) <= 1e-14
    assert pkg.bootstrap_correlation([], 8) == 0.0 and pkg.bootstrap_correlation([half], 8) == 0.0
    assert abs(pkg.bootstrap_correlation([half, half], 8) - 1.0) <= 1e-14


def test_search_random_stream(pkg):
    vals = [pkg.search_rand(5, it, d) for it in range(4) for d in range(50)]
    assert len(set(vals)) == len(vals) and all(0 <= v < 2 ** 64 for v in vals)
    assert pkg.search_rand(5, 1, 2) == pkg.search_rand(5, 1, 2) != pkg.search_rand(6, 1, 2)
    # the construction of ufboot_rand with stream 0x5E
    m64, g = (1 << 64) - 1, 0x9E3779B97F4A7C15

    def mix(z):
        z ^= z >> 30
        z = z * 0xBF58476D1CE4E5B9 & m64
        z ^= z >> 27
        z = z * 0x94D049BB133111EB & m64
        return z ^ (z >> 31)

    assert pkg.search_rand(9, 3, 4) == mix((mix((mix((9 + g * (0x5E + 1)) & m64) + g * (3 + 1)) & m64) + g * (4 + 1)) & m64)
    draws = [pkg.search_rand_int(pkg.search_rand(1, 1, d), 7) for d in range(700)]
    assert set(draws) == set(range(7)) and min(np.bincount(draws)) > 60
    assert pkg.search_rand_int(2 ** 64 - 1, 7) == 6 and pkg.search_rand_int(0, 7) == 0 and pkg.search_rand_int(12345, 1) == 0
