"""NNI on the super tree of an edge-linked partition model (host/supertree_host.h): the two / ten rounds of phylo_nni.cpp run
on the super tree with one iqhip_partition_optimize_branch_batch per round, against the branch-by-branch path built from
joint optimize_one_branch solves; and the tree edits that apply a move.  Bounds of batch against branch by branch: those
of tests/test_nni_batch_gpu.py."""
import numpy as np
import pytest

import partition_ref as pr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def group(synth, oracle):
    return pr.mixed_group(synth, oracle)


def super_tree(pkg, group, **kw):
    nwk, members = group
    st = pkg.PhyloSuperTree(nwk, members, all_branch=True, **kw)
    st.part_rates = pr.MIXED_RATES
    return st


def adjacency(t):
    return [[v for v, _ in t.neighbors(a)] for a in range(t.num_nodes)]


def test_batches_against_branch_by_branch(pkg, group):
    """case 8: evaluate_nnis_batch and evaluate_nnis5_batch against nni_for_branch per branch; an all-branch nni5 evaluation
    is exactly 10 batches of joint solves and no joint single solve (no solve diverged on this input)"""
    st = super_tree(pkg, group)
    lnl = st.compute_likelihood()
    tree0 = st.tree_string()
    c0 = st.counters()
    batch1 = st.evaluate_nnis_batch()
    c1 = st.counters()
    batch5 = st.evaluate_nnis5_batch()
    c5 = st.counters()
    assert len(batch1) == len(batch5) == 2 * (pr.MIXED_NTAXA - 3)
    assert c1["group_batches"] - c0["group_batches"] == 2 and c5["group_batches"] - c1["group_batches"] == 10
    assert c5["group_solves"] == c0["group_solves"] and c5["diverged"] == c0["diverged"]
    assert all(max(m["new_lens"]) <= 0.95 * 100.0 for m in batch5) and all(m["new_len"] <= 0.95 * 100.0 for m in batch1)
    assert st.tree_string() == tree0                                    # nothing is changed in the tree
    assert abs(st.compute_likelihood() - lnl) <= 1e-12 * abs(lnl)
    for k in range(0, len(batch1), 2):
        a, b = batch1[k]["node1"], batch1[k]["node2"]
        assert (batch5[k]["node1"], batch5[k]["node2"]) == (a, b)
        seq1 = st.nni_for_branch(a, b, nni5=False)
        seq5 = st.nni_for_branch(a, b, nni5=True)
        for c in range(2):
            newloglh, nei1, nei2, lens = seq1[c]
            m = batch1[k + c]
            assert (m["node1_nei"], m["node2_nei"]) == (nei1, nei2)
            assert abs(m["new_len"] - lens[0]) <= 1e-9 * max(1e-6, lens[0]), (a, b, c, m, lens)
            assert abs(m["newloglh"] - newloglh) <= 1e-10 * abs(newloglh), (a, b, c, m, newloglh)
            newloglh, nei1, nei2, lens = seq5[c]
            m = batch5[k + c]
            assert (m["node1_nei"], m["node2_nei"]) == (nei1, nei2)
            np.testing.assert_allclose(m["new_lens"], lens, rtol=1e-7, atol=1e-12)
            assert abs(m["newloglh"] - newloglh) <= 1e-9 * abs(newloglh), (a, b, c, m, newloglh)
    assert st.tree_string() == tree0
    assert abs(st.compute_likelihood() - lnl) <= 1e-12 * abs(lnl)
    # a listed branch has the entries of the full call; the batch can be repeated
    a, b = batch5[4]["node1"], batch5[4]["node2"]
    some = st.evaluate_nnis5_batch(branches=[(b, a)])
    assert [m["newloglh"] for m in some] == [m["newloglh"] for m in batch5[4:6]]
    assert [m["newloglh"] for m in st.evaluate_nnis_batch()] == [m["newloglh"] for m in batch1]
    st.close()


def test_applying_the_best_nni5_move(pkg, oracle, group):
    """case 9"""
    nwk, members = group
    st = super_tree(pkg, group)
    st.compute_likelihood()
    best = max(st.evaluate_nnis5_batch(), key=lambda m: m["newloglh"])
    st.do_nni(best)
    st.change_nni_brans(best, nni5=True)
    lnl = st.compute_likelihood()
    assert abs(lnl - best["newloglh"]) <= 1e-9 * abs(lnl), (lnl, best)
    new_nwk = st.tree_string()
    want = sum(oracle.OracleTree(pr.scale_newick(new_nwk, r), d["n"], d["seq_type"], d["pat"], d["freq"], d["invar"],
                                 d["model"]).likelihood()[0] for d, r in zip(members, pr.MIXED_RATES))
    assert abs(lnl - want) <= 1e-9 * abs(want), (lnl, want)
    adj = adjacency(st)
    sup_len = {(a, v): l for a in range(st.num_nodes) for v, l in st.neighbors(a)}
    for t, r in zip(st.members, pr.MIXED_RATES):
        assert adjacency(t) == adj
        for a in range(st.num_nodes):
            for v, l in t.neighbors(a):
                assert l == r * sup_len[(a, v)]
    st.close()


def test_batches_need_a_buffer_per_directed_vector(pkg, group):
    nwk, members = group
    st = pkg.PhyloSuperTree(nwk, members)
    st.compute_likelihood()
    with pytest.raises(pkg.HostError, match="setAllBranchMode"):
        st.evaluate_nnis5_batch()
    st.close()


def perturbed(pkg, group, seed):
    """the true tree after three random NNIs drawn from `seed` (the same on every call)"""
    st = super_tree(pkg, group)
    rng = np.random.default_rng(seed)
    for _ in range(3):
        adj = adjacency(st)
        inner = [(a, b) for a in range(len(adj)) for b in adj[a] if a < b and len(adj[a]) == 3 and len(adj[b]) == 3]
        a, b = inner[int(rng.integers(len(inner)))]
        st.do_random_nni(a, b, int(rng.integers(2)), int(rng.integers(2)))
    st.clear_all_partial_lh()
    return st


def move_ids(m):
    return (m["node1"], m["node2"], m["node1_nei"], m["node2_nei"])


def test_optimize_nni_from_a_perturbed_start(pkg, group):
    """case 10: the C++ trace (branches, positive, applied, scores, rollbacks) against nni_search_ref.optimize_nni driven over
    the Python super tree; the seed is the first for which the RESTATEMENT applies a move"""
    import nni_search_ref as ref
    want = None
    for seed in range(8):
        a = perturbed(pkg, group, seed)
        start = a.compute_likelihood()
        want = ref.optimize_nni(a, nni5=True, speed=True, batched=True)
        a.close()
        if any(s["applied"] and not s["rolled_back"] for s in want[3]):
            break
    assert any(s["applied"] and not s["rolled_back"] for s in want[3])
    b = perturbed(pkg, group, seed)
    assert abs(b.compute_likelihood() - start) <= 1e-12 * abs(start)
    lnl, count, steps, trace = b.optimize_nni(nni5=True, speed=True, batched=True, trace=True)
    assert (count, steps) == (want[1], want[2]) and len(trace) == len(want[3])
    for got, ref_step in zip(trace, want[3]):
        assert [tuple(x) for x in got["branches"]] == [tuple(x) for x in ref_step["branches"]]
        assert got["all_branches"] == ref_step["all_branches"] and got["rolled_back"] == ref_step["rolled_back"]
        assert [move_ids(m) for m in got["positive"]] == [move_ids(m) for m in ref_step["positive"]]
        assert [move_ids(m) for m in got["applied"]] == [move_ids(m) for m in ref_step["applied"]]
        for m, r in zip(got["positive"], ref_step["positive"]):
            assert abs(m["newloglh"] - r["newloglh"]) <= 1e-10 * abs(r["newloglh"])
        assert abs(got["score"] - ref_step["score"]) <= 1e-10 * abs(ref_step["score"])
    assert abs(lnl - want[0]) <= 1e-10 * abs(want[0]) and lnl > start
    assert abs(b.compute_likelihood() - lnl) <= 1e-10 * abs(lnl)
    b.close()


def test_three_iteration_tree_search(pkg, group):
    """case 11: a fixed iteration count with nni5 and speed against replay_search over the same kind of object (every
    candidate tree re-read by the super tree and all members); the candidate set's best tree reloads with the stored score"""
    import nni_search_ref as ref
    nwk, members = group
    def make(newick):
        t = super_tree(pkg, group)
        t.read_tree(newick)
        return t

    p = perturbed(pkg, group, 1)
    start = p.tree_string()      # both runs start from this string (a tree string rounds the lengths)
    p.close()
    st = make(start)
    ts = pkg.TreeSearch(st, seed=3, iterations=3, nni5=True, speed=True)
    best, its = ts.search(trace=True)
    assert [it["iteration"] for it in its] == [1, 2, 3, 4] and its[0]["parent"] == -1
    assert all(len(it["random_nnis"]) == int(0.5 * (pr.MIXED_NTAXA - 3)) for it in its[1:])

    scores, cand = ref.replay_search(make, start, its)
    for it, sc in zip(its, scores):
        assert abs(it["score"] - sc) <= 1e-10 * abs(sc), (it["iteration"], it["score"], sc)
    got = ts.candidates()
    assert [c[2] for c in got] == [c[2] for c in cand.ranked()]
    np.testing.assert_allclose([c[0] for c in got], [c[0] for c in cand.ranked()], rtol=1e-10)
    assert best == ts.best_score == got[0][0] == max(it["score"] for it in its)
    lnl = st.compute_likelihood()                                   # the best tree is loaded
    assert abs(lnl - best) <= 1e-10 * abs(best)
    assert st.sorted_taxon_id_string() == got[0][2]
    again = make(got[0][1])                                         # ... and reloads with the stored score
    assert abs(again.compute_likelihood() - got[0][0]) <= 1e-9 * abs(got[0][0])
    for t, r in zip(again.members, pr.MIXED_RATES):
        assert [[v for v, _ in t.neighbors(a)] for a in range(again.num_nodes)] == adjacency(again)
    again.close()
    st.close()


def test_search_refusals(pkg, synth, oracle, group):
    """case 12: UFBoot, num_init_trees > 0, a multifurcating super tree, fewer than 4 taxa, and the batched evaluation
    without a buffer per directed vector; each raises and the tree is untouched"""
    st = super_tree(pkg, group)
    tree0 = st.tree_string()
    ts = pkg.TreeSearch(st, num_init_trees=5)
    with pytest.raises(pkg.HostError, match="not available on a super tree"):
        ts.optimize_nni()
    with pytest.raises(pkg.HostError, match="not available on a super tree"):
        ts.search()
    ts.close()
    # UFBoot on a member
    m = st.members[0]
    nsite = int(round(float(np.sum(group[1][0]["freq"]))))
    m.gen_boot_samples(8, nsite, 5)
    m.ufboot_init(8, seed=5)
    for call in (lambda: st.optimize_nni(), lambda: pkg.TreeSearch(st, iterations=1).search()):
        with pytest.raises(pkg.HostError, match="UFBoot is not available on a super tree"):
            call()
    assert st.tree_string() == tree0
    st.close()
    nwk, members = group
    plain = pkg.PhyloSuperTree(nwk, members)
    with pytest.raises(pkg.HostError, match="setAllBranchMode"):
        plain.optimize_nni()
    assert plain.tree_string() == tree0
    assert plain.optimize_nni(batched=False)[0] >= plain.compute_likelihood() - 1e-6   # the branch-by-branch path needs no mode
    plain.close()
    # a multifurcating super tree: one internal branch of the mixed tree collapsed
    multi = collapse_first_inner_branch(nwk)
    poly = pkg.PhyloSuperTree(multi, members, all_branch=True)
    before = poly.tree_string()
    with pytest.raises(pkg.HostError, match="multifurcating"):
        poly.optimize_nni()
    with pytest.raises(pkg.HostError, match="multifurcating"):
        pkg.TreeSearch(poly, iterations=1).search()
    assert poly.tree_string() == before
    poly.close()
    # fewer than 4 taxa
    small_nwk = synth.random_tree_newick(3, 5, 0.05, 0.2)
    small = [pr.member_data(synth, oracle, small_nwk, 4, 4, pr.SEQ_DNA, 80, 40 + k, 1.0) for k in range(2)]
    tiny = pkg.PhyloSuperTree(small_nwk, small, all_branch=True)
    before = tiny.tree_string()
    with pytest.raises(pkg.HostError, match="at least 4 taxa"):
        tiny.optimize_nni()
    assert tiny.tree_string() == before
    tiny.close()


def collapse_first_inner_branch(nwk):
    """the Newick string with one internal branch removed: the first group that closes inside another group loses its
    parentheses and its length, its children join the enclosing node"""
    opens = []
    for i, ch in enumerate(nwk):
        if ch == "(":
            opens.append(i)
        elif ch == ")":
            start = opens.pop()
            if opens:   # an inner group
                j = i + 1
                while j < len(nwk) and nwk[j] not in ",)":
                    j += 1
                return nwk[:start] + nwk[start + 1:i] + nwk[j:]
    raise ValueError("no inner group")
