"""NNI tree edits on the super tree of an edge-linked partition model, without engines (attach=False): do_nni, its inverse,
do_random_nni, change_nni_brans and save / restore of lengths fan out to every member by node id, checked against topology
arithmetic on adjacency lists."""
import numpy as np

import partition_ref as pr


def build(pkg, synth, oracle):
    nwk, members = pr.mixed_group(synth, oracle)
    return pkg.PhyloSuperTree(nwk, members, attach=False)


def adjacency(t):
    return [[v for v, _ in t.neighbors(a)] for a in range(t.num_nodes)]


def lengths(t):
    return {(a, v): l for a in range(t.num_nodes) for v, l in t.neighbors(a)}


def inner_branches(t):
    return [(a, b) for a in range(t.num_nodes) for b, _ in t.neighbors(a)
            if a < b and len(t.neighbors(a)) == 3 and len(t.neighbors(b)) == 3]


def swapped(adj, mv):
    """the adjacency lists after the move: the two subtrees change places, slot for slot"""
    out = [list(x) for x in adj]
    n1, n2, x, y = mv["node1"], mv["node2"], mv["node1_nei"], mv["node2_nei"]
    out[n1][out[n1].index(x)] = y
    out[n2][out[n2].index(y)] = x
    out[x][out[x].index(n1)] = n2
    out[y][out[y].index(n2)] = n1
    return out


def test_do_nni_fans_out_and_is_its_own_inverse(pkg, synth, oracle):
    st = build(pkg, synth, oracle)
    adj0, len0 = adjacency(st), lengths(st)
    assert st.num_leaves == pr.MIXED_NTAXA and len(inner_branches(st)) == pr.MIXED_NTAXA - 3
    for m in st.members:
        assert adjacency(m) == adj0 and lengths(m) == len0
    a, b = inner_branches(st)[1]
    mv = dict(node1=a, node2=b, node1_nei=[v for v in adj0[a] if v != b][0], node2_nei=[v for v in adj0[b] if v != a][1])
    st.do_nni(mv)
    want = swapped(adj0, mv)
    assert adjacency(st) == want and want != adj0
    for m in st.members:
        assert adjacency(m) == want
        assert lengths(m) == lengths(st)        # the Neighbor objects moved with their lengths, on every tree alike
    st.do_nni(mv)
    assert adjacency(st) == adj0 and lengths(st) == len0
    for m in st.members:
        assert adjacency(m) == adj0 and lengths(m) == len0
    st.close()


def test_random_nni_lengths_and_restore(pkg, synth, oracle):
    st = build(pkg, synth, oracle)
    saved = st.save_branch_lengths()
    a, b = inner_branches(st)[2]
    for bit1 in (0, 1):
        for bit2 in (0, 1):
            before = adjacency(st)
            mv = st.do_random_nni(a, b, bit1, bit2)
            assert mv["node1_nei"] == [v for v in before[a] if v != b][bit1]
            assert mv["node2_nei"] == [v for v in before[b] if v != a][bit2]
            assert adjacency(st) == swapped(before, mv)
            for m in st.members:
                assert adjacency(m) == adjacency(st)
    # five new lengths: the central branch, then the other branches of node1 and of node2 in neighbour order
    move = dict(node1=a, node2=b, new_lens=[0.11, 0.12, 0.13, 0.14, 0.15])
    st.change_nni_brans(move, nni5=True)
    adj = adjacency(st)
    order = [(a, b)] + [(a, v) for v in adj[a] if v != b] + [(b, v) for v in adj[b] if v != a]
    for t in [st] + st.members:
        got = lengths(t)
        for (x, y), l in zip(order, move["new_lens"]):
            assert got[(x, y)] == l and got[(y, x)] == l
    # member lengths are rate x the move's lengths (super-tree units)
    st.part_rates = pr.MIXED_RATES
    move = dict(node1=a, node2=b, new_lens=[0.21, 0.22, 0.23, 0.24, 0.25])
    st.change_nni_brans(move, nni5=True)
    for t, r in zip([st] + st.members, [1.0] + pr.MIXED_RATES):
        got = lengths(t)
        for (x, y), l in zip(order, move["new_lens"]):
            assert got[(x, y)] == r * l and got[(y, x)] == r * l
    st.part_rates = [1.0] * len(pr.MIXED_RATES)
    assert not np.array_equal(st.save_branch_lengths(), saved)
    st.restore_branch_lengths(saved)
    assert np.array_equal(st.save_branch_lengths(), saved)
    for m in st.members:
        assert lengths(m) == lengths(st)
    st.clear_all_partial_lh()
    st.close()
