"""UFBoot bookkeeping, the parts that need no device: the numpy restatement of IQTree::saveCurrentTree's per-replicate rule
(tests/ufboot_ref.py) on hand-worked cases, the split / support / consensus functions of iq-tree_amd/host/ufboot_splits.h
through the Python wrappers against the independent restatement, the new symbols and the refusal of a planning-only
engine."""
import ctypes as C

import numpy as np
import pytest

import ufboot_ref as ref

DBL_MAX = ref.DBL_MAX


# ---- the rule ----------------------------------------------------------------------------------------------------------
def test_first_tree_against_the_start_values():
    st = ref.ufboot_start(3)
    counts, mn = ref.ufboot_rule(st, [np.array([-100.0, -90.0, -1e300])], [4], [-95.5], [1.0])
    assert counts.tolist() == [1, 0, 3] and mn == -95.5
    assert st["boot_logl"].tolist() == [-100.0, -90.0, -1e300]     # any finite sum beats -DBL_MAX + epsilon (= -DBL_MAX)
    assert st["boot_orig_logl"].tolist() == [-95.5] * 3
    assert st["boot_counts"].tolist() == [1, 1, 1]                  # "else boot_counts = 1", not 0 + 1 by the tie branch
    assert st["boot_tree"].tolist() == [4, 4, 4]
    assert ref.ufboot_rule(ref.ufboot_start(2), [], [], [], [])[1] == DBL_MAX   # no replicate holds a tree


def test_tie_band_with_rand_on_both_sides():
    # one replicate at boot_logl = -100 with count 1; a tie needs rand <= 1 / (1 + 1)
    def after(rell, rand, count=1, eps=0.5):
        st = dict(boot_logl=np.array([-100.0]), boot_orig_logl=np.array([-99.0]), boot_counts=np.array([count], dtype=np.int32),
                  boot_tree=np.array([0], dtype=np.int64))
        c, _ = ref.ufboot_rule(st, [np.array([rell])], [1], [-98.0], [rand], epsilon=eps)
        return st["boot_logl"][0], st["boot_orig_logl"][0], int(st["boot_counts"][0]), int(st["boot_tree"][0]), int(c[2])

    assert after(-100.2, 0.5) == (-100.0, -98.0, 2, 1, 1)     # inside the band, rand == 1/2: taken, count++, max() keeps -100
    assert after(-100.2, 0.5000001) == (-100.0, -99.0, 1, 0, 0)   # rand just above 1/2: not taken
    assert after(-99.8, 0.5) == (-99.8, -98.0, 2, 1, 1)       # inside the band from above: max() moves boot_logl up
    assert after(-99.8, 0.34, count=2) == (-100.0, -99.0, 2, 0, 0)   # count 2: needs rand <= 1/3
    assert after(-99.8, 1.0 / 3.0, count=2) == (-99.8, -98.0, 3, 1, 1)
    # the strict edges: rell == boot_logl + epsilon is NOT better by the first test but lies in the band;
    # rell == boot_logl - epsilon is outside the band (strict >)
    assert after(-99.5, 0.0) == (-99.5, -98.0, 2, 1, 1)
    assert after(-99.5, 0.9) == (-100.0, -99.0, 1, 0, 0)
    assert after(-100.5, 0.0) == (-100.0, -99.0, 1, 0, 0)
    assert after(-99.4999, 0.9) == (-99.4999, -98.0, 1, 1, 1)   # strictly better: count reset to 1, rand ignored
    # epsilon = 0: the band is empty, only a strictly larger sum replaces
    assert after(-100.0, 0.0, eps=0.0) == (-100.0, -99.0, 1, 0, 0)
    assert after(-99.0, 1.0, count=5, eps=0.0) == (-99.0, -98.0, 1, 1, 1)


def test_entries_apply_in_list_order():
    st = ref.ufboot_start(2)
    rell = [np.array([-10.0, -10.0]), np.array([-10.0, -8.0]), np.array([-10.2, -30.0])]
    counts, mn = ref.ufboot_rule(st, rell, [0, 1, 2], [-5.0, -6.0, -7.0], [0.9, 0.4, 0.3])
    # replicate 0: tree 0; tie with count 1, 0.4 <= 1/2: tree 1, count 2; tie with count 2, 0.3 <= 1/3: tree 2, count 3
    # replicate 1: tree 0; -8 strictly better: tree 1, count 1; -30 worse
    assert st["boot_tree"].tolist() == [2, 1] and st["boot_counts"].tolist() == [3, 1]
    assert st["boot_logl"].tolist() == [-10.0, -8.0] and st["boot_orig_logl"].tolist() == [-7.0, -6.0]
    assert counts.tolist() == [3, 0, 5] and mn == -7.0
    # the cutoff drops on logl alone, before anything is compared (:2678)
    st = ref.ufboot_start(2)
    counts, mn = ref.ufboot_rule(st, rell, [0, 1, 2], [-5.0, -6.01, -5.9], [0.9, 0.4, 0.3], logl_cutoff=-5.0)
    assert counts.tolist() == [2, 1, 3]
    assert st["boot_tree"].tolist() == [2, 0]
    margins = np.full(2, np.inf)
    ref.ufboot_rule(ref.ufboot_start(2), rell[:2], [0, 1], [-5.0, -6.0], [0.9, 0.4], margins=margins)
    np.testing.assert_allclose(margins, [0.5, 1.5])


# ---- splits, supports, consensus ------------------------------------------------------------------------------------------
TREES = ["((0,1),2,(3,(4,5)));",                 # 01|2345, 45|0123, 345|012
         "((0,2):0.1,1:0.2,(3:1e-3,(4,5)87:0.1):0.2);",   # 02|1345, 45, 345 -- lengths and labels are skipped
         "(0,(1,2),((3,5),4));",                 # 12|0345, 35|0124, 345
         "((1,0),2,((5,4),3));"]                 # = tree 0 written in another order


def fs(*taxa):
    return frozenset(taxa)


def test_newick_splits(pkg):
    assert ref.newick_splits(TREES[0], 6) == [fs(2, 3, 4, 5), fs(4, 5), fs(3, 4, 5)]
    assert ref.newick_splits(TREES[1], 6) == [fs(1, 3, 4, 5), fs(4, 5), fs(3, 4, 5)]
    for t in TREES:
        assert pkg.newick_splits(t, 6) == ref.newick_splits(t, 6), t
    assert set(pkg.newick_splits(TREES[3], 6)) == set(pkg.newick_splits(TREES[0], 6))
    # a rooted (bifurcating) top level names its one split once; names are looked up
    assert pkg.newick_splits("((0,1),(2,3));", 4) == [fs(2, 3)]
    names = ["Hs", "Pt", "Gg", "Mm", "Rn"]
    assert pkg.newick_splits("((Hs:1,Pt:1):1,Gg:1,(Mm:2,Rn:2)99:1);", 5, names) == [fs(2, 3, 4), fs(3, 4)]
    assert pkg.newick_splits("(0,1,2);", 3) == []
    # 70 taxa: the bitset spans two words
    cat = "(0,1," * 1 + "".join("(%d," % k for k in range(2, 69)) + "69" + ")" * 68 + ";"
    got = pkg.newick_splits(cat, 70)
    assert got == ref.newick_splits(cat, 70) and len(got) == 67 and fs(68, 69) in got
    for bad in ("((0,1),2,(3,(4,5));", "((0,1),2,(3,(4,4)));", "((0,1),2,(3,4));", "((0,1),2,(3,(4,7)));", "((0,1),2,(3,(4,x)));"):
        with pytest.raises(pkg.HostError):
            pkg.newick_splits(bad, 6)


def test_supports_with_an_absent_split(pkg):
    query = "((0,1),(2,3),(4,5));"      # 01 in trees 0 and 3, 23 in no tree (label 0), 45 in trees 0, 1 and 3
    assert ref.supports(TREES, query, 6) == [50, 0, 75]
    assert pkg.split_supports(TREES, query, 6) == [50, 0, 75]
    w = [3, 1, 2, 1]                    # 01: 4 of 7 = 57.1; 45: 5 of 7 = 71.4
    assert ref.supports(TREES, query, 6, w) == [57, 0, 71]
    assert pkg.split_supports(TREES, query, 6, weights=w) == [57, 0, 71]
    assert pkg.split_supports(TREES[:1] * 8, TREES[0], 6) == [100, 100, 100]
    # halves round away from zero: 1 of 8 = 12.5 -> 13, 1 of 200 = 0.5 -> 1
    assert pkg.split_supports([TREES[1]] + [TREES[0]] * 7, "((0,2),1,(3,(4,5)));", 6)[0] == 13 == ref.supports([TREES[1]] + [TREES[0]] * 7, TREES[1], 6)[0]
    assert pkg.split_supports([TREES[1]] + [TREES[0]] * 199, TREES[1], 6)[0] == 1


def test_consensus_with_an_incompatible_pair(pkg):
    # weights 3, 2, 1: 345 has 6, 45 has 5, 01|2345 has 3, 02|1345 has 2 and is incompatible with 01 -> left out;
    # 35 (1) is incompatible with 45; 12|0345 (1) is incompatible with 01
    w = [3, 2, 1]
    taken = ref.consensus_splits(TREES[:3], 6, w)
    assert taken == [(fs(3, 4, 5), 100), (fs(4, 5), 83), (fs(2, 3, 4, 5), 50)]
    want = "(0,1,(2,(3,(4,5)83)100)50);"
    assert ref.consensus(TREES[:3], 6, w) == want
    assert pkg.consensus_tree(TREES[:3], 6, weights=w) == want
    # the other way round the heavier of the incompatible pair wins
    assert pkg.consensus_tree(TREES[:3], 6, weights=[2, 3, 1]) == ref.consensus(TREES[:3], 6, [2, 3, 1]) == "(0,(1,(3,(4,5)83)100)50,2);"
    # equal weights: the tie goes to the split that appeared first (01 of tree 0, before 02 of tree 1)
    assert pkg.consensus_tree(TREES[:2], 6) == ref.consensus(TREES[:2], 6) == "(0,1,(2,(3,(4,5)100)100)50);"
    assert pkg.consensus_tree(TREES[1::-1], 6) == ref.consensus(TREES[1::-1], 6) == "(0,(1,(3,(4,5)100)100)50,2);"
    names = list("ABCDEF")
    named = ["((A,B),C,(D,(E,F)));", "((A,C),B,(D,(F,E)));"]
    assert pkg.consensus_tree(named, 6, names=names) == ref.consensus(named, 6, names=names) == "(A,B,(C,(D,(E,F)100)100)50);"
    # random tree sets against the restatement
    rng = np.random.default_rng(3)
    for ntaxa in (5, 9, 70):
        trees = []
        for _ in range(7):
            parts = [str(t) for t in rng.permutation(ntaxa)]
            while len(parts) > 3:
                i, j = sorted(rng.choice(len(parts), 2, replace=False))
                b = parts.pop(j)
                a = parts.pop(i)
                parts.append("(%s,%s)" % (a, b))
            trees.append("(" + ",".join(parts) + ");")
        w = rng.integers(1, 5, size=len(trees)).tolist()
        assert pkg.consensus_tree(trees, ntaxa, weights=w) == ref.consensus(trees, ntaxa, w)
        for q in trees[:2]:
            assert pkg.split_supports(trees, q, ntaxa, weights=w) == ref.supports(trees, q, ntaxa, w)
            assert pkg.newick_splits(q, ntaxa) == ref.newick_splits(q, ntaxa)


def test_sorted_taxon_id_string(pkg):
    """WT_TAXON_ID + WT_SORT_TAXA: printed from the root leaf's neighbour, children by ascending smallest taxon, no lengths"""
    t = pkg.PhyloTree("((5:0.1,4:0.2):0.05,(1:0.1,(3:0.2,0:0.1):0.07):0.04,2:0.3);")
    s = t.sorted_taxon_id_string()
    assert s == "(0,(1,(2,(4,5))),3);"      # the root leaf is taxon 0; its neighbour joins 0, 3 and the rest
    assert set(pkg.newick_splits(s, 6)) == set(pkg.newick_splits("((5,4),(1,(3,0)),2);", 6))
    assert ":" not in s and s.endswith(";")
    t.close()


def test_rand_is_the_documented_generator(pkg):
    """(z >> 11) 2^-53 with z = mix(mix(mix(seed + G (0xBB + 1)) + G (tree_id + 1)) + G): restated here with numpy uint64"""
    G = np.uint64(0x9E3779B97F4A7C15)

    def mix(z):
        z = np.uint64(z)
        z ^= z >> np.uint64(30)
        z *= np.uint64(0xBF58476D1CE4E5B9)
        z ^= z >> np.uint64(27)
        z *= np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))

    with np.errstate(over="ignore"):
        for seed, tid in ((0, 0), (7, 1), (2 ** 63 + 5, 123456789)):
            z = mix(mix(mix(np.uint64(seed) + G * np.uint64(0xBB + 1)) + G * np.uint64(tid + 1)) + G)
            want = float(int(z) >> 11) * 2.0 ** -53
            assert pkg.ufboot_rand(seed, tid) == want and 0.0 <= want < 1.0


# ---- ABI ---------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("iqhip_ufboot_init", "iqhip_ufboot_update", "iqhip_ufboot_fetch", "iqhip_debug_ufboot_timing")


def test_new_symbols_exist(pkg):
    lib = pkg.libiqhip()
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s), s
        assert s in pkg.IQHIP_SYMBOLS
    assert C.sizeof(pkg.UFBootTree) == 32
    host = pkg.libiqhost()
    for s in ("iqhost_ufboot_init", "iqhost_save_current_tree", "iqhost_save_nni_trees", "iqhost_summarize_bootstrap",
              "iqhost_ufboot_newick_splits", "iqhost_ufboot_split_supports", "iqhost_ufboot_consensus"):
        assert hasattr(host, s), s


def test_planning_only_engine_refuses_the_new_calls(pkg):
    lib = pkg.libiqhip()
    e = C.c_void_p()
    assert lib.iqhip_debug_create_planner(C.byref(e), 4, 4, 1000, 8, 256, 18, 1) == 0
    try:
        ent = (pkg.UFBootTree * 1)(pkg.UFBootTree(0, 0, 0, -1.0, 0.5))
        d = np.zeros(4)
        dp = d.ctypes.data_as(C.POINTER(C.c_double))
        n = C.c_int64()
        calls = [lambda: lib.iqhip_ufboot_init(e, 1),
                 lambda: lib.iqhip_ufboot_update(e, ent, 1, 0.5, 0.0, None, None),
                 lambda: lib.iqhip_ufboot_fetch(e, dp, None, None, None),
                 lambda: lib.iqhip_debug_ufboot_timing(e, dp, C.byref(n))]
        for call in calls:
            assert call() == 2                                  # IQHIP_ERR_INVALID
            assert b"planning-only" in lib.iqhip_last_error()
    finally:
        lib.iqhip_destroy(e)
