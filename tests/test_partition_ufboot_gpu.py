"""UFBoot on edge-linked partition models (include/iqhip.h "UFBoot on edge-linked partition models"): the per-pattern rows
of the group's batched joint solve, the members' RELL sums added in member order, the group's per-replicate state and the
super tree's mirror, against the oracle, against numpy float64 and against the numpy restatement of IQTree::saveCurrentTree's
rule (tests/ufboot_ref.py).

Exact cases: integer rows times integer samples -- every member's RELL sum and their sum are exact integers in any order, so
the group's state must equal the restatement BIT FOR BIT whatever the chunking.  Real rows: bit-identical to the restatement fed
with the group's own sums; equal to the restatement on numpy's product wherever no comparison sits within the product's
error bound of its threshold."""
import ctypes as C

import numpy as np
import pytest

import partition_ref as pr
import partition_ufboot_ref as pu
import ufboot_ref as ref
import test_branch_tests_gpu as bt        # swapped_newick, oracle_rows
import test_partition_batch_gpu as pb     # make_group, plain_task

pytestmark = pytest.mark.gpu

IQHIP_ERR_INVALID = 2
NROWS, NSAMPLES = 12, 257
EXACT_NPTN = (17, 70, 1100)               # 1100: two work items of the 4-state tiles, the second ragged


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def assert_state_equal(got, want, what=""):
    for f in ("boot_tree", "boot_counts"):
        np.testing.assert_array_equal(got[f], want[f], err_msg="%s %s" % (f, what))
    for f in ("boot_logl", "boot_orig_logl"):
        np.testing.assert_array_equal(bits(got[f]), bits(want[f]), err_msg="%s %s" % (f, what))


def small_engine(pkg, synth, nptn):
    rng = np.random.default_rng(nptn)
    pat = rng.integers(0, 4, size=(3, nptn)).astype(np.uint8)
    t = pkg.PhyloTree("(0:0.1,1:0.2,2:0.3);")
    t.set_alignment(4, pkg.SEQ_DNA, pat, np.ones(nptn))
    t.set_model(synth.gtr_model(alpha=0.9, ncat=4))
    t.set_likelihood_kernel(pkg.LK_EIGEN_HIP)
    t.attach_engine(0)
    return t


def set_chunk(monkeypatch, chunk):
    if chunk is None:
        monkeypatch.delenv("IQHIP_UFBOOT_CHUNK", raising=False)
    else:
        monkeypatch.setenv("IQHIP_UFBOOT_CHUNK", chunk)


# ---- 1. exact sums -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exact_group(pkg, synth):
    """three 4-state members; per member NROWS integer rows as tests/test_ufboot_gpu.py::exact_engine builds them (row 0
    random in -9 .. -1, every other row differing from it by -1 / 0 / +1 at three patterns, one duplicated row) and
    NSAMPLES integer samples in 0 .. 3"""
    trees, Ls, Ws = [], [], []
    for nptn in EXACT_NPTN:
        rng = np.random.default_rng(2000 + nptn)
        t = small_engine(pkg, synth, nptn)
        L = np.tile(rng.integers(-9, 0, size=nptn).astype(np.float64), (NROWS, 1))
        for r in range(1, NROWS):
            at = rng.choice(nptn, 3, replace=False)
            L[r, at] = np.clip(L[r, at] + rng.integers(-1, 2, size=3), -9, -1)
        L[NROWS - 1] = L[1]
        W = rng.integers(0, 4, size=(NSAMPLES, nptn)).astype(np.float32)
        t.set_boot_samples(W)
        trees.append(t)
        Ls.append(L)
        Ws.append(W.astype(np.float64))
    g = pkg.PartitionGroup(trees)
    g.ptnlh_reserve(NROWS)
    for t, L in zip(trees, Ls):
        for r in range(NROWS):
            t.ptnlh_upload(r, L[r])
    yield g, trees, Ls, Ws
    g.close()


def exact_sums(Ls, Ws, rows, ns):
    R = sum(L[rows] @ W[:ns].T for L, W in zip(Ls, Ws))
    assert np.array_equal(R, np.round(R)) and np.abs(R).max() < 2 ** 40
    return R


@pytest.mark.parametrize("ntrees", [1, 2, 37])
@pytest.mark.parametrize("nsamples", [1, 63, 64, 65, 257])
def test_exact_sums(pkg, exact_group, monkeypatch, nsamples, ntrees):
    g, trees, Ls, Ws = exact_group
    P = len(trees)
    rng = np.random.default_rng(7 * nsamples + 1000 * ntrees)
    rows, ids, logl, rand = entry_list(rng, ntrees)
    R = exact_sums(Ls, Ws, rows, nsamples)
    assert np.array_equal(g.ptnlh_rell(rows, nsamples), R)
    saw_tie = False
    for eps in (0.5, 1.0, 0.0):
        want = ref.ufboot_start(nsamples)
        wcounts, wmin = ref.ufboot_rule(want, R, ids, logl, rand, epsilon=eps)
        saw_tie = saw_tie or bool((want["boot_counts"] > 1).any())
        for chunk in (None, "1", "5"):
            set_chunk(monkeypatch, chunk)
            g.ufboot_init(nsamples)
            counts, mn = g.ufboot_update(rows, ids, logl, rand, epsilon=eps)
            assert_state_equal(g.ufboot_state(), want, "eps %g chunk %s" % (eps, chunk))
            assert counts.tolist() == wcounts.tolist() and mn == wmin
            nchunks = ntrees if chunk == "1" else -(-ntrees // 5) if chunk == "5" else 1
            assert g.ufboot_timing()[2] == (2 * P + 1) * nchunks       # per chunk: product + combine per member, one update
        set_chunk(monkeypatch, None)
        # one call over the list == one call per entry
        g.ufboot_init(nsamples)
        total = np.zeros(3, dtype=np.int64)
        for k in range(ntrees):
            c, mn = g.ufboot_update(rows[k:k + 1], ids[k:k + 1], logl[k:k + 1], rand[k:k + 1], epsilon=eps)
            total += c
        assert_state_equal(g.ufboot_state(), want, "eps %g entry by entry" % eps)
        assert total.tolist() == wcounts.tolist() and mn == wmin
    if ntrees >= 2 and nsamples > 1:
        assert saw_tie                                       # the inputs do force the tie branch


def entry_list(rng, ntrees):
    """tests/test_ufboot_gpu.py::entry_list"""
    rows = rng.integers(0, NROWS, size=ntrees)
    if ntrees >= 2:
        rows[1] = rows[0]
    if ntrees >= 5:
        rows[4] = rows[2]
    ids = 5 + np.arange(ntrees, dtype=np.int64) * 3
    ids[-1] = (1 << 40) + 7
    logl = rng.uniform(-5000.0, -4000.0, size=ntrees)
    rand = rng.uniform(0.0, 1.0, size=ntrees)
    rand[::7] = 0.5
    if ntrees >= 2:
        rand[1] = 0.25
    if ntrees >= 3:
        rand[2] = 0.0
    if ntrees >= 4:
        rand[3] = 1.0
    return rows, ids, logl, rand


def test_cutoff_drops_entries(pkg, exact_group):
    """the cases of tests/test_ufboot_gpu.py::test_cutoff_drops_entries on the group"""
    g, trees, Ls, Ws = exact_group
    rng = np.random.default_rng(11)
    rows, ids, logl, rand = entry_list(rng, 37)
    ns = 65
    R = exact_sums(Ls, Ws, rows, ns)
    cutoff = float(np.sort(logl)[12]) + 1.0                  # the 12 lowest fall below cutoff - 1
    want = ref.ufboot_start(ns)
    wcounts, wmin = ref.ufboot_rule(want, R, ids, logl, rand, logl_cutoff=cutoff)
    assert wcounts[:2].tolist() == [25, 12]
    g.ufboot_init(ns)
    counts, mn = g.ufboot_update(rows, ids, logl, rand, logl_cutoff=cutoff)
    assert_state_equal(g.ufboot_state(), want)
    assert counts.tolist() == wcounts.tolist() and mn == wmin
    # everything dropped: nothing is multiplied, the state stays, the minimum is still reported
    counts, mn2 = g.ufboot_update(rows[:3], ids[:3], [-9e5, -9e5, -9e5], rand[:3], logl_cutoff=cutoff)
    assert counts.tolist() == [0, 3, 0] and mn2 == wmin
    assert_state_equal(g.ufboot_state(), want)
    assert g.ufboot_timing()[2] == 1
    # a fresh state with everything dropped holds no tree: DBL_MAX
    g.ufboot_init(ns)
    counts, mn3 = g.ufboot_update(rows[:3], ids[:3], [-9e5, -9e5, -9e5], rand[:3], logl_cutoff=cutoff)
    assert counts.tolist() == [0, 3, 0] and mn3 == ref.DBL_MAX
    assert_state_equal(g.ufboot_state(), ref.ufboot_start(ns))


# ---- 2. rows of the batched solve ------------------------------------------------------------------------------------------
def member_with_patterns(synth, oracle, nwk, n, ncat, seq_type, nsites, seed, rate, npat):
    """partition_ref.member_data cut to exactly npat patterns (the first npat of the compressed alignment)"""
    d = pr.member_data(synth, oracle, nwk, n, ncat, seq_type, nsites, seed, rate)
    assert d["pat"].shape[1] >= npat, (d["pat"].shape, npat)
    d["pat"] = np.ascontiguousarray(d["pat"][:, :npat])
    d["freq"] = np.ascontiguousarray(d["freq"][:npat])
    d["invar"] = np.ascontiguousarray(d["invar"][:npat])
    return d


BOUNDARY_RATES = [1.0, 1.7, 0.6]
_groups = {}


def case_group(name, synth, oracle):
    """'mixed': partition_ref.mixed_group.  'boundary': DNA +G4 with 1100 patterns (two 4-state work items, the second
    ragged), protein with 530 patterns (crosses the 512-pattern matrix-core item; 530 is no multiple of 16), DNA with one
    category and 17 patterns; 8 taxa"""
    if name == "mixed":
        nwk, members = pr.mixed_group(synth, oracle)
        return nwk, members, pr.MIXED_RATES
    if name not in _groups:
        nwk = synth.random_tree_newick(8, 91, 0.05, 0.4)
        members = [member_with_patterns(synth, oracle, nwk, 4, 4, pr.SEQ_DNA, 6000, 810, BOUNDARY_RATES[0], 1100),
                   member_with_patterns(synth, oracle, nwk, 20, 1, pr.SEQ_PROTEIN, 700, 820, BOUNDARY_RATES[1], 530),
                   member_with_patterns(synth, oracle, nwk, 4, 1, pr.SEQ_DNA, 60, 830, BOUNDARY_RATES[2], 17)]
        _groups[name] = (nwk, members, BOUNDARY_RATES)
    return _groups[name]


def super_tree(pkg, nwk, members, rates):
    st = pkg.PhyloSuperTree(nwk, members, all_branch=True)
    st.part_rates = rates
    return st


def fetch_rows(st, rows):
    return [np.array([m.ptnlh_fetch(r) for r in rows]) for m in st.members]


@pytest.mark.parametrize("name", ["mixed", "boundary"])
def test_rows_of_the_batched_solve(pkg, synth, oracle, monkeypatch, name):
    nwk, members, rates = case_group(name, synth, oracle)
    st = super_tree(pkg, nwk, members, rates)
    st.compute_likelihood()
    plain = st.evaluate_nnis5_batch()
    nm = len(plain)
    assert nm == 10
    # rows 0 and nm + 1, nm + 2 hold a mark that must survive
    st.ptnlh_reserve(nm + 3)
    for m in st.members:
        for r in (0, nm + 1, nm + 2):
            m.ptnlh_upload(r, np.full(m.nptn, -7.0 - r))
    moves = st.evaluate_nnis5_batch(first_row=1)
    assert moves == plain                                    # moves, lengths and lnL bit-identical to a call without rows
    L = fetch_rows(st, range(1, nm + 1))
    for m in st.members:
        for r in (0, nm + 1, nm + 2):
            assert np.array_equal(m.ptnlh_fetch(r), np.full(m.nptn, -7.0 - r))
    # every member's row against the oracle's per-pattern values at the device's own accepted lengths
    for k, mv in enumerate(moves):
        swapped = bt.swapped_newick(st, mv)
        total = 0.0
        for p, (d, r) in enumerate(zip(members, rates)):
            part_ref, expect = bt.oracle_rows(oracle, pr.scale_newick(swapped, r), d)
            np.testing.assert_allclose(L[p][k], expect, rtol=1e-9, atol=0, err_msg="move %d member %d" % (k, p))
            mine = float(np.dot(L[p][k], d["freq"]))
            assert abs(mine - part_ref) <= 1e-9 * abs(part_ref), (k, p, mine, part_ref)   # the member's part of newloglh
            total += mine
        assert abs(total - mv["newloglh"]) <= 1e-9 * abs(mv["newloglh"]), (k, total, mv["newloglh"])
    # a row is a function of the theta slot, the counters and optx alone
    for env, value in (("IQHIP_PART_BATCH_CHUNK", "3"), ("IQHIP_PART_STEPS", "1")):
        monkeypatch.setenv(env, value)
        again = st.evaluate_nnis5_batch(first_row=1)
        monkeypatch.delenv(env)
        assert again == moves, env
        for a, b in zip(fetch_rows(st, range(1, nm + 1)), L):
            assert np.array_equal(bits(a), bits(b)), env
    # batched rows against the branch-by-branch rows, at the loosest bound tests/test_partition_nni_gpu.py uses for batch
    # against branch by branch (rtol 1e-7, that of the five lengths; the sums below are held to its 1e-9 of |lnL|)
    worst = 0.0
    for k in range(0, nm, 2):
        seq5 = st.nni_for_branch(moves[k]["node1"], moves[k]["node2"], nni5=True, first_row=nm + 3)
        B = fetch_rows(st, (nm + 3, nm + 4))
        for c in range(2):
            for p, d in enumerate(members):
                np.testing.assert_allclose(B[p][c], L[p][k + c], rtol=1e-7, atol=0)
                worst = max(worst, float(np.max(np.abs(B[p][c] - L[p][k + c]) / np.abs(L[p][k + c]))))
            got = sum(float(np.dot(B[p][c], d["freq"])) for p, d in enumerate(members))
            assert abs(got - seq5[c][0]) <= 1e-9 * abs(seq5[c][0])
    print("%s: batched against branch-by-branch rows, largest relative difference %.3e" % (name, worst))
    st.close()


def test_rows_through_the_group_call(pkg, synth, oracle, monkeypatch):
    """iqhip_partition_optimize_branch_batch_rows itself: all 13 branches of the mixed group as one batch, every fourth task
    without a row.  sum_ptn f * row is the member's part_lnl (1e-9 |lnL|); results and part_lnl have the bits of the call
    without rows; rows nobody names are untouched; a row outside one member's store refuses the call before it runs"""
    lib = pkg.libiqhip()
    nwk, members = pr.mixed_group(synth, oracle)
    G = pb.make_group(pkg, oracle, nwk, members, pr.MIXED_RATES)
    g, trees = G["group"], G["trees"]
    tasks = [pb.plain_task(pkg, G, a, b, 1e-6, G["sup"].length(a, b), 100.0, 1e-6, 100) for a, b in G["edges"]]
    arr = (pkg.BranchTask * len(tasks))(*tasks)
    rows = np.array([-1 if k % 4 == 3 else 2 + k for k in range(len(tasks))], dtype=np.int32)
    nrows = 2 + len(tasks) + 1
    g.ptnlh_reserve(nrows)
    for t in trees:
        for r in range(nrows):
            t.ptnlh_upload(r, np.full(t.nptn, -3.0 - r))
    res0, part0 = g.optimize_branch_batch(arr)
    res, part = g.optimize_branch_batch(arr, rows=rows)
    pb.same_bits(res, part, res0, part0)
    used = set(int(r) for r in rows if r >= 0)
    kept = {}
    for p, (t, d) in enumerate(zip(trees, members)):
        for r in range(nrows):
            got = t.ptnlh_fetch(r)
            if r not in used:
                assert np.array_equal(got, np.full(t.nptn, -3.0 - r)), (p, r)
        for k, r in enumerate(rows):
            if r >= 0:
                got = t.ptnlh_fetch(int(r))
                kept[(p, k)] = got
                assert abs(np.dot(got, d["freq"]) - part[k][p]) <= 1e-9 * abs(part[k][p]), (p, k)
    for env, value in (("IQHIP_PART_BATCH_CHUNK", "3"), ("IQHIP_PART_STEPS", "1")):
        monkeypatch.setenv(env, value)
        res2, part2 = g.optimize_branch_batch(arr, rows=rows)
        monkeypatch.delenv(env)
        pb.same_bits(res2, part2, res0, part0)
        for (p, k), want in kept.items():
            assert np.array_equal(bits(trees[p].ptnlh_fetch(int(rows[k]))), bits(want)), (env, p, k)
    # two tasks may not name one row: their passes would store to it in one launch
    twice = rows.copy()
    twice[6] = twice[2]
    out = (pkg.BranchResult * len(tasks))()
    assert lib.iqhip_partition_optimize_branch_batch_rows(g.h, arr, len(tasks), out, None,
                                                          twice.ctypes.data_as(C.POINTER(C.c_int32))) == IQHIP_ERR_INVALID
    assert b"same row" in lib.iqhip_last_error()
    # one member's store is larger: a row only it has is outside the group's
    trees[1].ptnlh_reserve(nrows + 4)
    bad = rows.copy()
    bad[5] = nrows + 1
    out = (pkg.BranchResult * len(tasks))()
    ip = bad.ctypes.data_as(C.POINTER(C.c_int32))
    assert lib.iqhip_partition_optimize_branch_batch_rows(g.h, arr, len(tasks), out, None, ip) == IQHIP_ERR_INVALID
    assert b"row outside the store" in lib.iqhip_last_error()
    for (p, k), want in kept.items():
        assert np.array_equal(bits(trees[p].ptnlh_fetch(int(rows[k]))), bits(want))
    g.close()


# ---- 3, 4. group sums; real rows through the update ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def real_case(pkg, synth, oracle):
    """the mixed group: the current tree's row 0 and the 10 NNI rows 1 .. 10 of evaluate_nnis5_batch on every member; per
    member NSAMPLES resamples of its own sites"""
    nwk, members = pr.mixed_group(synth, oracle)
    st = super_tree(pkg, nwk, members, pr.MIXED_RATES)
    Ws = pu.member_samples(members, NSAMPLES, pu.MARGIN_SEED)
    st.set_boot_samples(Ws)
    lnl = st.compute_likelihood()
    st.ptnlh_reserve(11)
    st.ufboot_init(1)
    st.save_current_tree(lnl)                                # the mirror puts the current tree's row into row 0 of every member
    moves = st.evaluate_nnis5_batch(first_row=1)
    assert len(moves) == 10
    rows = np.arange(11)
    logl = np.array([lnl] + [m["newloglh"] for m in moves])
    ids = np.arange(11, dtype=np.int64)
    rand = np.array([pkg.ufboot_rand(pu.TIE_SEED, k) for k in range(11)])
    Ls = fetch_rows(st, rows)
    assert abs(sum(float(L[0] @ d["freq"]) for L, d in zip(Ls, members)) - lnl) <= 1e-9 * abs(lnl)
    yield st, rows, ids, logl, rand, Ls, [W.astype(np.float64) for W in Ws]
    st.close()


@pytest.mark.parametrize("nsamples", [1, 64, 257])
def test_group_sums_are_the_member_sums_in_member_order(real_case, nsamples):
    st, rows, ids, logl, rand, Ls, Ws = real_case
    for rr in (rows, np.array([3, 3, 0, 10, 3])):
        want = None
        for m in st.members:
            mine = m.ptnlh_rell(rr, nsamples)
            want = mine if want is None else want + mine     # ((R_0 + R_1) + R_2) + R_3 in float64
        got = st.ptnlh_rell(rr, nsamples)
        assert np.array_equal(bits(got), bits(want))


@pytest.mark.parametrize("nsamples", [64, 257])
def test_real_rows_bit_identical_to_the_rule_on_the_group_sums(real_case, monkeypatch, nsamples):
    st, rows, ids, logl, rand, Ls, Ws = real_case
    R = st.ptnlh_rell(rows, nsamples)
    want = ref.ufboot_start(nsamples)
    wcounts, wmin = ref.ufboot_rule(want, R, ids, logl, rand)
    for chunk in (None, "1", "5"):
        set_chunk(monkeypatch, chunk)
        st.ufboot_init(nsamples)
        counts, mn = st.ufboot_update(rows, ids, logl, rand)
        assert_state_equal(st.ufboot_state(), want, "chunk %s" % chunk)
        assert counts.tolist() == wcounts.tolist() and mn == wmin
    assert len(set(want["boot_tree"].tolist())) > 1          # the replicates do disagree about the best tree


def test_real_rows_against_the_numpy_product(real_case):
    """The margin scheme of tests/test_ufboot_gpu.py::test_real_rows_against_the_numpy_product on R = sum_p L_p W_p^T
    (partition_ufboot_ref.margin_scheme): the group's sum differs from numpy's by at most 1e-13 * sum_p |L_p| |W_p|^T per
    element, so a replicate counts only where every comparison of the numpy run keeps a margin above that bound; there
    boot_tree, boot_counts and boot_orig_logl must be equal and boot_logl agrees within the bound.  At most 1 % of the
    replicates may be left out.  The seed (partition_ufboot_ref.MARGIN_SEED) was chosen without a device, on the oracle's rows:
    tests/test_partition_ufboot_host.py asserts that the reference computation alone leaves out none there (smallest margin
    1.137e-03, largest bound 4.848e-10); with the device's rows on an MI355X the figures are the same to the digits shown."""
    st, rows, ids, logl, rand, Ls, Ws = real_case
    ns = NSAMPLES
    want, counted, margins, bound = pu.margin_scheme(Ls, Ws, ids, logl, rand, ns)
    print("replicates left out: %d of %d; smallest margin %.3e, largest bound %.3e" % ((~counted).sum(), ns, margins.min(), bound.max()))
    assert (~counted).sum() <= ns // 100
    st.ufboot_init(ns)
    st.ufboot_update(rows, ids, logl, rand)
    got = st.ufboot_state()
    for f in ("boot_tree", "boot_counts"):
        np.testing.assert_array_equal(got[f][counted], want[f][counted], err_msg=f)
    np.testing.assert_array_equal(bits(got["boot_orig_logl"][counted]), bits(want["boot_orig_logl"][counted]))
    assert (np.abs(got["boot_logl"] - want["boot_logl"])[counted] <= bound[counted]).all()


# ---- 5. mirror ---------------------------------------------------------------------------------------------------------------
def test_mirror_feeds_the_same_entries(pkg, real_case):
    """save_current_tree + save_nni_trees == one update over {current row, the 10 NNI rows} with sequential ids and the
    documented tie draws; the kept strings are those of the ids some replicate refers to; supports and consensus of
    summarize_bootstrap are ufboot_ref's on the winners"""
    st, rows, ids, logl, rand, Ls, Ws = real_case
    ns = 65
    st.ufboot_init(ns)
    st.ufboot_update(rows[:1], ids[:1], logl[:1], rand[:1])
    st.ufboot_update(rows[1:], ids[1:], logl[1:], rand[1:])
    want = st.ufboot_state()
    st.ufboot_init(ns, seed=9)
    lnl = st.compute_likelihood()
    assert abs(lnl - logl[0]) <= 1e-9 * abs(lnl)
    c0, _ = st.save_current_tree(logl[0])
    assert c0.tolist() == [1, 0, ns]
    c1, mn = st.save_nni_trees()
    assert c1[0] == 10 and abs(mn - want["boot_orig_logl"].min()) <= 1e-9 * abs(mn)
    got = st.ufboot_state()
    np.testing.assert_array_equal(got["boot_tree"], want["boot_tree"])
    np.testing.assert_array_equal(got["boot_counts"], want["boot_counts"])
    np.testing.assert_allclose(got["boot_logl"], want["boot_logl"], rtol=1e-12)   # the rows were computed again
    info = st.ufboot_info()
    assert info["trees_fed"] == 11 and info["trees_kept"] == len(set(got["boot_tree"].tolist()))
    assert all(m.ufboot_info()["trees_fed"] == 0 for m in st.members)            # the members' own states are not touched
    s = st.summarize_bootstrap()
    assert len(s["boot_trees"]) == ns and s["distinct_trees"] == info["trees_kept"]
    base = st.sorted_taxon_id_string()
    for k in range(ns):
        if got["boot_tree"][k] == 0:
            assert s["boot_trees"][k] == base
        else:
            assert s["boot_trees"][k] != base and len(ref.newick_splits(s["boot_trees"][k], 8)) == 5
    assert sorted(p for _, _, p in s["supports"]) == sorted(ref.supports(s["boot_trees"], base, 8))
    assert s["consensus_tree"] == ref.consensus(s["boot_trees"], 8)


# ---- 6. search -----------------------------------------------------------------------------------------------------------------
class GroupReplay:
    """tests/test_tree_search_gpu.py::BootReplay on super trees: every tree the search feeds, in its order, through
    ufboot_ref.ufboot_rule on the group's RELL sums of the rows"""

    def __init__(self, pkg, nsamples, seed):
        self.pkg, self.ns, self.seed = pkg, nsamples, seed
        self.state = ref.ufboot_start(nsamples)
        self.next_id = 0
        self.cutoff = 0.0
        self.min_orig = ref.DBL_MAX

    def feed(self, tree, rows, logl):
        ids = np.arange(self.next_id, self.next_id + len(rows), dtype=np.int64)
        self.next_id += len(rows)
        rand = np.array([self.pkg.ufboot_rand(self.seed, int(k)) for k in ids])
        R = tree.ptnlh_rell(np.asarray(rows), self.ns)
        _, self.min_orig = ref.ufboot_rule(self.state, R, ids, np.asarray(logl), rand, logl_cutoff=self.cutoff)

    def next_iteration(self):
        if self.min_orig != ref.DBL_MAX:
            self.cutoff = self.min_orig

    def current(self, tree, score):
        tree.save_current_tree(score)      # (row 0 on every member; the replay tree's own state is not looked at)
        self.feed(tree, [0], [score])

    def evaluate(self, tree, listed):
        moves = tree.evaluate_nnis5_batch(first_row=1, branches=listed)
        self.feed(tree, [1 + k for k in range(len(moves))], [m["newloglh"] for m in moves])
        return moves


def test_search_feeds_the_bootstrap(pkg, synth, oracle, real_case):
    import nni_search_ref as nref
    import test_partition_nni_gpu as pn
    group = pr.mixed_group(synth, oracle)
    Ws = [W.astype(np.float32) for W in real_case[6]]
    ns = 100

    def make(newick, boot=True):
        t = super_tree(pkg, group[0], group[1], pr.MIXED_RATES)
        t.read_tree(newick)
        if boot:
            t.set_boot_samples(Ws)
            t.ufboot_init(ns, seed=11)
        return t

    p = pn.perturbed(pkg, group, 1)
    start = p.tree_string()
    p.close()
    plain = make(start, boot=False)
    ts0 = pkg.TreeSearch(plain, seed=3, iterations=3)
    best0 = ts0.search()
    st = make(start)
    ts = pkg.TreeSearch(st, seed=3, iterations=3, step_iterations=2)
    best, its = ts.search(trace=True)
    # a fixed iteration count: the bootstrap does not steer the search
    assert [it["iteration"] for it in its] == [1, 2, 3, 4]
    assert best == best0 and ts.candidates() == ts0.candidates()
    assert [k for k, _ in ts.correlation_log] == [2, 4] and len(ts.boot_splits) == 3   # snapshots at 2, 3, 4
    fed = sum(1 + len(s["evaluated"]) for it in its for s in it["steps"] if s["branches"])
    assert st.ufboot_info()["trees_fed"] == fed
    replay = GroupReplay(pkg, ns, 11)
    made = []

    def make_kept(newick):
        made.append(make(newick))
        return made[-1]

    nref.replay_search(make_kept, start, its, boot=replay)
    assert replay.next_id == fed
    got = st.ufboot_state()
    np.testing.assert_array_equal(got["boot_tree"], replay.state["boot_tree"])
    np.testing.assert_array_equal(got["boot_counts"], replay.state["boot_counts"])
    np.testing.assert_allclose(got["boot_logl"], replay.state["boot_logl"], rtol=1e-12)
    np.testing.assert_allclose(got["boot_orig_logl"], replay.state["boot_orig_logl"], rtol=1e-10)
    assert (got["boot_tree"] >= 0).all()                     # every replicate holds a tree
    assert len(st.summarize_bootstrap()["boot_trees"]) == ns
    # batched evaluation with UFBoot needs nni5, as on a plain tree
    with pytest.raises(pkg.HostError, match="needs nni5"):
        pkg.TreeSearch(st, iterations=1, nni5=False).search()
    for t in made + [st, plain]:
        t.close()


# ---- 7. state rules and refusals -------------------------------------------------------------------------------------------------
def test_state_rules_and_refusals(pkg, synth):
    lib = pkg.libiqhip()
    mem0 = pkg.debug_memory()
    a, b = small_engine(pkg, synth, 70), small_engine(pkg, synth, 17)
    for t, v in ((a, -1.0), (b, -2.0)):
        t.ptnlh_reserve(2)
        t.ptnlh_upload(0, v * np.ones(t.nptn))
        t.ptnlh_upload(1, 2.0 * v * np.ones(t.nptn))
    g = pkg.PartitionGroup([a, b])
    ent = (pkg.UFBootTree * 2)(pkg.UFBootTree(0, 0, 3, -104.0, 0.5), pkg.UFBootTree(1, 0, 4, -208.0, 0.5))
    upd = lambda: lib.iqhip_partition_ufboot_update(g.h, ent, 2, 0.5, 0.0, None, None)
    fetch = lambda: lib.iqhip_partition_ufboot_fetch(g.h, None, None, None, None)
    assert lib.iqhip_partition_ufboot_init(g.h, 1) == IQHIP_ERR_INVALID       # no samples yet
    assert upd() == IQHIP_ERR_INVALID and fetch() == IQHIP_ERR_INVALID          # before init
    assert b"iqhip_partition_ufboot_init" in lib.iqhip_last_error()
    a.set_boot_samples(np.ones((8, 70), dtype=np.float32))
    assert lib.iqhip_partition_ufboot_init(g.h, 1) == IQHIP_ERR_INVALID       # one member still has none
    b.set_boot_samples(np.ones((6, 17), dtype=np.float32))
    assert lib.iqhip_partition_ufboot_init(g.h, 0) == IQHIP_ERR_INVALID
    assert lib.iqhip_partition_ufboot_init(g.h, 7) == IQHIP_ERR_INVALID       # above ONE member's sample count
    assert upd() == IQHIP_ERR_INVALID
    g.ufboot_init(6)
    assert upd() == 0
    st = g.ufboot_state()
    assert st["boot_tree"].tolist() == [3] * 6 and st["boot_logl"].tolist() == [-104.0] * 6   # -70 - 2 * 17
    g.ufboot_init(5)                                                            # a second init resets the state
    assert_state_equal(g.ufboot_state(), ref.ufboot_start(5))
    assert upd() == 0
    # replacing ANY member's sample matrix invalidates the group's state, whichever call replaces it
    b.gen_boot_samples(6, 17, 3)
    assert upd() == IQHIP_ERR_INVALID and fetch() == IQHIP_ERR_INVALID
    g.ufboot_init(6)
    assert upd() == 0
    a.set_boot_samples(np.ones((8, 70), dtype=np.float32))
    assert upd() == IQHIP_ERR_INVALID
    rows = np.zeros(1, dtype=np.int32)
    out = np.zeros(8)
    assert lib.iqhip_partition_ptnlh_rell(g.h, rows.ctypes.data_as(C.POINTER(C.c_int32)), 1, 6,
                                          out.ctypes.data_as(C.POINTER(C.c_double))) == 0     # (the sums need no state)
    assert out[:6].tolist() == [-104.0] * 6
    g.ufboot_init(6)
    assert upd() == 0
    before = g.ufboot_state()

    def rc(eps=0.5, n=1, null=False, row=0, tree_id=9, logl=-10.0, rand=0.5):
        e1 = (pkg.UFBootTree * 1)(pkg.UFBootTree(row, 0, tree_id, logl, rand))
        return lib.iqhip_partition_ufboot_update(g.h, None if null else e1, n, eps, 0.0, None, None)

    assert rc(null=True) == IQHIP_ERR_INVALID and rc(n=0) == IQHIP_ERR_INVALID
    assert rc(row=-1) == IQHIP_ERR_INVALID and rc(tree_id=-1) == IQHIP_ERR_INVALID
    for bad in (-1e-9, 1.0000001, float("nan")):
        assert rc(rand=bad) == IQHIP_ERR_INVALID
    for bad in (float("inf"), float("-inf"), float("nan")):
        assert rc(logl=bad) == IQHIP_ERR_INVALID
    assert rc(eps=-0.1) == IQHIP_ERR_INVALID and rc(eps=float("nan")) == IQHIP_ERR_INVALID
    # a row outside ONE member's store (a has three rows now, b two): nothing is enqueued, the state is unchanged
    a.ptnlh_reserve(3)
    assert rc(row=2) == IQHIP_ERR_INVALID
    assert b"row outside the store of member 1" in lib.iqhip_last_error()
    rows[0] = 2
    assert lib.iqhip_partition_ptnlh_rell(g.h, rows.ctypes.data_as(C.POINTER(C.c_int32)), 1, 6,
                                          out.ctypes.data_as(C.POINTER(C.c_double))) == IQHIP_ERR_INVALID
    assert_state_equal(g.ufboot_state(), before)
    d = np.zeros(2)
    assert lib.iqhip_debug_partition_ufboot_timing(g.h, None, None) == IQHIP_ERR_INVALID
    assert lib.iqhip_debug_partition_ufboot_timing(g.h, d.ctypes.data_as(C.POINTER(C.c_double)), None) == 0
    # destroying the group frees what it owned and leaves the members usable
    with_group = pkg.debug_memory()
    g.close()
    assert pkg.debug_memory()[0] < with_group[0]
    assert a.ptnlh_fetch(0).tolist() == [-1.0] * 70
    assert a.ptnlh_rell([0], 8).tolist() == [[-70.0] * 8]
    a.ufboot_init(8)                                                            # a member's own state is its own
    assert a.ufboot_state()["boot_tree"].tolist() == [-1] * 8
    a.close()
    b.close()
    assert pkg.debug_memory() == mem0                                           # back at the starting value
