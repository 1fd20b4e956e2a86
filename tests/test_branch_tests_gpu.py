"""SH-aLRT and local-bootstrap branch supports on the device (include/iqhip.h "branch supports"): the store of
per-pattern log-likelihood rows filled by iqhip_optimize_branch_batch_rows / iqhip_ptnlh_put_current, the matrix-core
product iqhip_ptnlh_rell and the statistics of iqhip_branch_tests, against the oracle, against numpy float64 and against a
numpy restatement of PhyloTree::testOneBranch (tests/test_branch_tests_host.py)."""
import ctypes as C
import sys

import numpy as np
import pytest

from test_branch_tests_host import restate_branch_tests

pytestmark = pytest.mark.gpu

SEQ_BINARY = 3
IQHIP_ERR_INVALID, IQHIP_ERR_UNSUPPORTED = 2, 3


def make_case(synth, oracle, pkg, n, ncat, seq_type, ntaxa, nsites, seed, lo=0.02, hi=0.2, caterpillar=False, data_nwk=None,
              sharded=0):
    """host tree in LM_ALL_BRANCH on one engine + everything an oracle tree of another topology needs"""
    if n == 4:
        model = synth.gtr_model(alpha=0.9, ncat=ncat)
    else:
        model = synth.random_reversible_model(n, seed, alpha=0.9, ncat=ncat)
    su = oracle.state_unknown_for(n, seq_type)
    nwk = synth.random_tree_newick(ntaxa, seed, lo, hi, caterpillar)
    st = synth.simulate_alignment(data_nwk or nwk, model, nsites, seed + 1, 0.02 if n != 2 else 0.0, su)
    pat, freq = synth.compress_patterns(st)
    invar = synth.ptn_invar_for(pat, model)
    t = pkg.PhyloTree(nwk)
    t.set_mem_mode(pkg.LM_ALL_BRANCH)
    t.set_alignment(n, seq_type, pat, freq, invar)
    t.set_model(model)
    t.set_likelihood_kernel(pkg.LK_EIGEN_HIP)
    if sharded:
        t.attach_engine_sharded([0] * sharded, pkg.REDUCE_HOST)
    else:
        t.attach_engine(0)
    okw = dict(n=n, seq_type=seq_type, pat=pat, freq=freq, invar=invar, model=model)
    return t, okw, freq


def swapped_newick(t, m):
    """the NNI neighbour of move m (evaluate_nnis5_batch) with its five re-optimised lengths, rooted for printing at leaf 0"""
    adj = {a: [[b, ln] for b, ln in t.neighbors(a)] for a in range(t.num_nodes)}
    n1, n2, s1, s2 = m["node1"], m["node2"], m["node1_nei"], m["node2_nei"]

    def replace(at, old, new):
        for e in adj[at]:
            if e[0] == old:
                e[0] = new
                return
        raise AssertionError("not adjacent")

    l1 = [ln for b, ln in adj[n1] if b == s1][0]
    l2 = [ln for b, ln in adj[n2] if b == s2][0]
    replace(n1, s1, s2)
    replace(s2, n2, n1)
    replace(n2, s2, s1)
    replace(s1, n1, n2)
    for e in adj[n1]:
        if e[0] == s2:
            e[1] = l2
    for e in adj[n2]:
        if e[0] == s1:
            e[1] = l1

    def set_len(a, b, ln):
        for x, y in ((a, b), (b, a)):
            for e in adj[x]:
                if e[0] == y:
                    e[1] = ln

    # newLen: [0] the central branch, [1], [2] the branches at node1, [3], [4] those at node2, each in neighbour order
    lens = m["new_lens"]
    set_len(n1, n2, lens[0])
    for k, b in enumerate([b for b, _ in adj[n1] if b != n2]):
        set_len(n1, b, lens[1 + k])
    for k, b in enumerate([b for b, _ in adj[n2] if b != n1]):
        set_len(n2, b, lens[3 + k])
    nleaf = t.num_leaves
    sys.setrecursionlimit(max(sys.getrecursionlimit(), 20000))

    def write(node, dad):
        if node < nleaf and dad is not None:
            return "%d" % node
        return "(" + ",".join("%s:%.17g" % (write(b, node), ln) for b, ln in adj[node] if b != dad) + ")"

    start = adj[0][0][0]
    return write(start, None) + ";"


def oracle_rows(oracle, nwk, okw, **extra):
    """(lnL, per-pattern lnL with the scaling events of both ends put back) of a tree, as tests/test_rell_gpu.py"""
    ot = oracle.OracleTree(nwk, okw["n"], okw["seq_type"], okw["pat"], okw["freq"], okw["invar"], okw["model"], **extra)
    ref, (a, b) = ot.likelihood()
    _, oplh = ot.branch_lnl(a, b)
    _, sc_b, _ = ot.partial(a, b)                      # a is the leaf end
    return ref, oracle.pattern_lh_scaled(oplh, None, sc_b)


def check_rows_against_oracle(t, oracle, okw, freq, moves, first_row, which, **extra):
    for k in which:
        m = moves[k]
        ref, expect = oracle_rows(oracle, swapped_newick(t, m), okw, **extra)
        got = t.ptnlh_fetch(first_row + k)
        nobs = len(expect) - extra.get("n_unobs", 0)
        np.testing.assert_allclose(got[:nobs], expect[:nobs], rtol=1e-9, atol=0)
        assert abs(m["newloglh"] - ref) <= 1e-9 * abs(ref), (k, m["newloglh"], ref)
        assert abs(np.dot(got, freq) - m["newloglh"]) <= 1e-9 * abs(m["newloglh"])


def check_product(t, freq, M, seed, reps=(100,)):
    """iqhip_ptnlh_rell on store rows 0 .. M-1 against numpy float64 at 1e-13 * sum |L W| per element; the weights include
    zeros, a zero sample and values of 2^20"""
    rng = np.random.default_rng(seed)
    W = boot_samples(rng, freq, max(reps))
    W[rng.random(W.shape) < 0.3] = 0.0
    W[rng.random(W.shape) < 0.01] = 2.0 ** 20
    if len(W) > 5:
        W[3] = 0.0
        W[5, ::7] = 2.0 ** 20
    t.set_boot_samples(W)
    L = np.array([t.ptnlh_fetch(r) for r in range(M)])
    W64 = W.astype(np.float64)
    for n in reps:
        got = t.ptnlh_rell(np.arange(M), n)
        want = L @ W64[:n].T
        bound = 1e-13 * (np.abs(L) @ np.abs(W64[:n]).T)
        assert got.shape == want.shape == (M, n)
        assert np.all(np.abs(got - want) <= bound), float(np.max(np.abs(got - want) / np.maximum(bound, 1e-300)))
    return L, W


# ---- 1. rows against the oracle ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,ncat,seq_type,ntaxa,nsites", [(4, 4, 0, 7, 300), (20, 4, 1, 6, 200), (64, 1, 2, 6, 150),
                                                          (4, 12, 0, 6, 200), (2, 4, SEQ_BINARY, 6, 200)])
def test_rows_against_oracle(pkg, synth, oracle, n, ncat, seq_type, ntaxa, nsites):
    t, okw, freq = make_case(synth, oracle, pkg, n, ncat, seq_type, ntaxa, nsites, 7100 + n + ncat)
    t.compute_likelihood()
    moves = t.evaluate_nnis5_batch(first_row=1)
    assert len(moves) == 2 * (ntaxa - 3)
    check_rows_against_oracle(t, oracle, okw, freq, moves, 1, range(len(moves)))
    plain = t.evaluate_nnis5_batch()                    # the entry without rows gives the same moves
    assert [m["newloglh"] for m in plain] == [m["newloglh"] for m in moves]


def test_rows_deep_tree_scale_counters_at_both_ends(pkg, synth, oracle):
    """40 taxa and, because a 4-state pattern likelihood of 40 taxa cannot fall below 2^-256 (0.25^40 ~ 1e-24), a
    400-taxon random tree with long branches: near its centre the branch a candidate's lnL is evaluated on has rescaled
    vectors at both ends (two such candidates in this tree, found with the oracle's counters), and the row must carry
    both counters."""
    t, okw, freq = make_case(synth, oracle, pkg, 4, 4, 0, 40, 150, 7300, lo=0.4, hi=0.9, caterpillar=True)
    t.compute_likelihood()
    moves = t.evaluate_nnis5_batch(first_row=1)
    check_rows_against_oracle(t, oracle, okw, freq, moves, 1, range(0, len(moves), 9))
    check_product(t, freq, 1 + len(moves), 40, reps=(70,))           # 75 rows: five row tiles, the 8-tile kernel
    t.close()
    t, okw, freq = make_case(synth, oracle, pkg, 4, 4, 0, 400, 120, 7301, lo=0.5, hi=0.9)
    t.compute_likelihood()
    moves = t.evaluate_nnis5_batch(first_row=1)
    nleaf = t.num_leaves
    both = []
    for k, m in enumerate(moves):
        # the last optimised branch joins node2 with its last neighbour (the other end: everything else); the taxon sets of
        # its two ends are those of this branch of the unchanged tree when the neighbour was not part of the swap
        last = [b for b, _ in t.neighbors(m["node2"]) if b != m["node1"]][-1]
        if last < nleaf or last == m["node2_nei"]:
            continue
        if t.fetch_scale_num(m["node2"], last).max() >= 1 and t.fetch_scale_num(last, m["node2"]).max() >= 1:
            both.append(k)
    assert len(both) >= 2
    pick = both[:4]
    check_rows_against_oracle(t, oracle, okw, freq, moves, 1, pick)
    assert min(t.ptnlh_fetch(1 + k).min() for k in pick) < 2 * -177.44567822334599     # at least two scaling events
    # 795 rows: the 13-tile kernel (more than 64 KB of LDS) over four row groups, the last one ragged
    assert 1 + len(moves) == 795
    check_product(t, freq, 795, 400, reps=(37, 100))


def test_product_row_tiles_between_two_and_four(pkg, synth, oracle):
    """22 taxa: 39 rows = three row tiles, the 4-tile kernel; with the cases above and below every instantiation runs"""
    t, okw, freq = make_case(synth, oracle, pkg, 4, 4, 0, 22, 400, 7350)
    t.compute_likelihood()
    moves = t.evaluate_nnis5_batch(first_row=1)
    assert 1 + len(moves) == 39
    L, W = check_product(t, freq, 39, 22, reps=(1, 37, 100))
    assert not L[0].any() and L[1:].all(axis=1).any()


def test_rows_from_several_chunks(pkg, synth, oracle, monkeypatch):
    t, okw, freq = make_case(synth, oracle, pkg, 4, 4, 0, 11, 300, 7400)
    t.compute_likelihood()
    whole = t.evaluate_nnis5_batch(first_row=1)
    rows_whole = [t.ptnlh_fetch(1 + k) for k in range(len(whole))]
    monkeypatch.setenv("IQHIP_BATCH_CHUNK", "3")          # 8 tasks per round: chunks of 3, 3, 2 reuse the theta buffers
    moves = t.evaluate_nnis5_batch(first_row=20)
    check_rows_against_oracle(t, oracle, okw, freq, moves, 20, range(len(moves)))
    for k in range(len(moves)):
        np.testing.assert_allclose(t.ptnlh_fetch(20 + k), rows_whole[k], rtol=1e-12)
        np.testing.assert_array_equal(t.ptnlh_fetch(1 + k), rows_whole[k])      # growing the store kept the old rows


# ---- 2. batched against per-branch ------------------------------------------------------------------------------------
def boot_samples(rng, freq, nsamples):
    p = np.asarray(freq, dtype=np.float64)
    return rng.multinomial(int(p.sum()), p / p.sum(), size=nsamples).astype(np.float32)


@pytest.mark.parametrize("n,ncat,seq_type,ntaxa,nsites", [(4, 4, 0, 9, 400), (20, 4, 1, 6, 200)])
def test_batched_equals_per_branch(pkg, synth, oracle, n, ncat, seq_type, ntaxa, nsites):
    t, okw, freq = make_case(synth, oracle, pkg, n, ncat, seq_type, ntaxa, nsites, 7500 + n)
    t.set_boot_samples(boot_samples(np.random.default_rng(5), freq, 64))
    nb = ntaxa - 3
    a = t.test_all_branches(64, 40, batched=True)
    rows_a = [t.ptnlh_fetch(r) for r in range(1 + 2 * nb)]
    b = t.test_all_branches(64, 40, batched=False)
    rows_b = [t.ptnlh_fetch(r) for r in range(1 + 2 * nb)]
    assert len(a) == len(b) == nb
    assert a["node1"].tolist() == b["node1"].tolist() and a["node2"].tolist() == b["node2"].tolist()
    for ra, rb in zip(rows_a, rows_b):
        np.testing.assert_allclose(ra, rb, rtol=1e-12, atol=0)
    np.testing.assert_allclose(a["lh"], b["lh"], rtol=1e-9)
    # the same rows give the same decisions unless one sits within rounding of its threshold (none does here)
    for f in ("sh_alrt", "lbp"):
        assert a[f].tolist() == b[f].tolist()
    # abayes and alrt_stat are functions of the differences lh_k - lh_0, and the two forms' lh agree to 1e-9 |lh| each:
    # d ln(abayes) <= max |d(lh_k - lh_0)| <= 2e-9 max|lh|, d alrt_stat <= 2 * 2e-9 max|lh|
    dl = 2e-9 * np.abs(a["lh"]).max()
    np.testing.assert_allclose(a["abayes"], b["abayes"], rtol=dl, atol=0)
    np.testing.assert_allclose(a["alrt_stat"], b["alrt_stat"], rtol=0, atol=2 * dl)
    assert abs(np.dot(rows_a[0], freq) - a["lh"][0, 0]) <= 1e-9 * abs(a["lh"][0, 0])


def test_rows_null_is_the_old_entry(pkg, synth, oracle):
    t, okw, freq = make_case(synth, oracle, pkg, 4, 4, 0, 14, 3000, 7600)
    lib = pkg.libiqhip()
    lib.iqhip_optimize_branch_batch.argtypes = [C.c_void_p, C.POINTER(pkg.BranchTask), C.c_int, C.POINTER(C.c_double),
                                                C.POINTER(pkg.BranchResult)]
    t.compute_likelihood()
    t.compute_all_partial_lh()
    nleaf = t.num_leaves
    inner = [(x, y) for x in range(t.num_nodes) for y, _ in t.neighbors(x) if x < y and x >= nleaf and y >= nleaf]
    tasks = (pkg.BranchTask * len(inner))(*[
        pkg.BranchTask(None, 0, 10, pkg.key_end(t.neighbor_info(x, y)["key"]), pkg.key_end(t.neighbor_info(y, x)["key"]),
                       0.05 + 0.01 * k, 1e-6, 100.0, 1e-6) for k, (x, y) in enumerate(inner)])

    def values(res):
        return [(r.optx, r.d2l, r.lnl, r.nsteps, r.status) for r in res]

    old = (pkg.BranchResult * len(inner))()
    new = (pkg.BranchResult * len(inner))()
    with_rows = (pkg.BranchResult * len(inner))()
    assert lib.iqhip_optimize_branch_batch(t.engine, tasks, len(inner), None, old) == 0
    assert lib.iqhip_optimize_branch_batch_rows(t.engine, tasks, len(inner), None, new, None) == 0
    assert values(old) == values(new)                                       # bit-identical
    t.ptnlh_reserve(len(inner))
    rows = np.arange(len(inner), dtype=np.int32)
    rows[1] = -1                                                            # a task without a row
    assert lib.iqhip_optimize_branch_batch_rows(t.engine, tasks, len(inner), None, with_rows,
                                                rows.ctypes.data_as(C.POINTER(C.c_int32))) == 0
    assert values(with_rows) == values(old)
    assert not t.ptnlh_fetch(1).any()
    # every branch of one tree: the row of task k is the tree's pattern lnL at that branch length
    for k, (x, y) in enumerate(inner):
        if k == 1:
            continue
        assert abs(np.dot(t.ptnlh_fetch(k), freq) - old[k].lnl) <= 1e-10 * abs(old[k].lnl)


# ---- 3. the product against numpy float64 ------------------------------------------------------------------------------
@pytest.mark.parametrize("ntaxa", [4, 7, 12])                  # M = 3, 9, 19 rows (19 crosses a 16-row tile)
@pytest.mark.parametrize("nsites", [70, 1000, 5600])           # one K-step pair ... several K-chunks to combine
def test_product_against_numpy(pkg, synth, oracle, ntaxa, nsites):
    # 20 states x 1 category: nearly every site of a long-branched tree is a pattern of its own, also for 4 taxa
    t, okw, freq = make_case(synth, oracle, pkg, 20, 1, 1, ntaxa, nsites, 7700 + ntaxa, lo=0.5, hi=1.0)
    assert t.nptn >= 0.85 * nsites                      # (4 taxa: about 4900 of 5600 sites are distinct patterns)
    M = 1 + 2 * (ntaxa - 3)
    rng = np.random.default_rng(ntaxa * nsites)
    W = boot_samples(rng, freq, 100)
    W[rng.random(W.shape) < 0.3] = 0.0
    W[rng.random(W.shape) < 0.01] = 2.0 ** 20
    W[3] = 0.0
    W[5, ::7] = 2.0 ** 20
    t.set_boot_samples(W)
    assert len(t.test_all_branches(1)) == ntaxa - 3         # fills rows 0 .. M-1
    L = np.array([t.ptnlh_fetch(r) for r in range(M)])
    t.compute_likelihood()
    np.testing.assert_array_equal(L[0], t.compute_pattern_likelihood())
    W64 = W.astype(np.float64)
    for reps in (1, 37, 100):
        got = t.ptnlh_rell(np.arange(M), reps)
        want = L @ W64[:reps].T
        bound = 1e-13 * (np.abs(L) @ np.abs(W64[:reps]).T)
        assert got.shape == want.shape == (M, reps)
        assert np.all(np.abs(got - want) <= bound), float(np.max(np.abs(got - want) / np.maximum(bound, 1e-300)))
    assert not t.ptnlh_rell(np.arange(M), 100)[:, 3].any()
    # repeated rows are multiplied once and handed out to every place; the result is the same run to run
    perm = np.array([M - 1, 0, 0, 1, M - 1])
    again = t.ptnlh_rell(perm, 37)
    np.testing.assert_array_equal(again, t.ptnlh_rell(np.arange(M), 37)[perm])


# ---- 4. the statistics against the numpy restatement --------------------------------------------------------------------
def check_supports(t, sup, W, reps, lbp_reps):
    """the device's counts against restate_branch_tests fed numpy's own sums of the fetched rows"""
    times = max(reps, lbp_reps)
    W64 = W.astype(np.float64)[:times]
    row0 = t.ptnlh_fetch(0)
    for q in range(len(sup)):
        L = np.array([row0, t.ptnlh_fetch(1 + 2 * q), t.ptnlh_fetch(2 + 2 * q)])
        R = L @ W64.T
        r = restate_branch_tests(R, sup["lh"][q])
        tol = 1e-9 * (np.abs(L) @ np.abs(W64).T).max(axis=0)
        keep = r["margin"] > tol
        print("branch %d: %d of %d replicates excluded" % (q, int((~keep).sum()), times))
        assert (~keep).sum() <= 0.01 * times
        # replicates within rounding of a threshold may fall either way: the counts agree up to their number, exactly when
        # there is none
        for name, flags in (("sh_alrt", r["sh"]), ("lbp", r["lbp"])):
            lo, hi = int(flags[keep].sum()), int(flags[keep].sum() + (~keep).sum())
            got = sup[name][q] * times
            assert abs(got - round(got)) < 1e-9 and lo <= round(got) <= hi, (q, name, got, lo, hi)
        assert abs(sup["abayes"][q] - r["abayes"]) <= 1e-12 * abs(r["abayes"])
        assert abs(sup["alrt_stat"][q] - r["alrt_stat"]) <= 1e-12 * max(1.0, abs(r["alrt_stat"]))


def test_statistics_against_restatement(pkg, synth, oracle):
    t, okw, freq = make_case(synth, oracle, pkg, 4, 4, 0, 10, 500, 7800, lo=0.01, hi=0.08)
    W = boot_samples(np.random.default_rng(11), freq, 200)
    t.set_boot_samples(W)
    sup = t.test_all_branches(200, 150)
    assert len(sup) == 7
    check_supports(t, sup, W, 200, 150)
    assert 0.0 < sup["sh_alrt"].max() <= 1.0 and 0.0 < sup["lbp"].max() <= 1.0
    # fewer replicates than uploaded samples: the first ones are used; lbp_reps > reps sets the count
    sup2 = t.test_all_branches(10, 37)
    check_supports(t, sup2, W, 10, 37)
    # the C call on the same rows, run twice: the same bits
    rows3 = np.array([[0, 1 + 2 * q, 2 + 2 * q] for q in range(7)])
    r1 = t.branch_tests(rows3, sup2["lh"], 10, 37)
    r2 = t.branch_tests(rows3, sup2["lh"], 10, 37)
    np.testing.assert_array_equal(r1, r2)
    np.testing.assert_array_equal(r1[:, 0], sup2["sh_alrt"])


def test_statistics_when_a_neighbour_is_better(pkg, synth, oracle):
    """the tree is not the data's: some NNI neighbour has the higher likelihood (the reference prints a warning and
    counts all the same, phylotree.cpp:3790-3800)"""
    other = synth.random_tree_newick(9, 4242, 0.05, 0.2)
    t, okw, freq = make_case(synth, oracle, pkg, 4, 4, 0, 9, 600, 7900, lo=0.05, hi=0.2, data_nwk=other)
    W = boot_samples(np.random.default_rng(12), freq, 100)
    t.set_boot_samples(W)
    sup = t.test_all_branches(100, 100)
    better = (sup["lh"][:, 1] > sup["lh"][:, 0]) | (sup["lh"][:, 2] > sup["lh"][:, 0])
    assert better.any()
    assert np.all(sup["alrt_stat"][better] < 0) and np.all(sup["sh_alrt"][better] == 0.0)
    check_supports(t, sup, W, 100, 100)


# ---- 5. +ASC ------------------------------------------------------------------------------------------------------------
def test_branch_tests_with_ascertainment(pkg, synth, oracle):
    model = synth.gtr_model(alpha=0.7, ncat=4)
    nwk = synth.random_tree_newick(8, 8100)
    st = synth.simulate_alignment(nwk, model, 500, 8101)
    st = st[:, [s for s in range(st.shape[1]) if len(set(st[:, s].tolist())) > 1]]
    pat, freq = synth.compress_patterns(st)
    nsite = int(freq.sum())
    pat = np.concatenate([pat, np.tile(np.arange(4, dtype=np.uint8), (8, 1))], axis=1)
    freq = np.concatenate([freq, np.zeros(4)])
    t = pkg.PhyloTree(nwk)
    t.set_mem_mode(pkg.LM_ALL_BRANCH)
    t.set_alignment(4, 0, pat, freq)
    t.set_ascertainment(4, nsite)
    t.set_model(model)
    t.attach_engine(0)
    W = boot_samples(np.random.default_rng(13), freq, 100)
    assert not W[:, -4:].any()
    t.set_boot_samples(W)
    sup = t.test_all_branches(100, 100)
    nb = 8 - 3
    rows = np.array([t.ptnlh_fetch(r) for r in range(1 + 2 * nb)])
    assert np.all(rows[:, -4:] == 0.0) and np.all(rows[:, :-4] < 0.0)
    t.compute_likelihood()
    np.testing.assert_allclose(rows[0], t.compute_pattern_likelihood(), rtol=1e-12)
    for q in range(nb):
        for c in range(3):
            r = 0 if c == 0 else 2 * q + c
            assert abs(np.dot(rows[r], freq) - sup["lh"][q, c]) <= 1e-9 * abs(sup["lh"][q, c])
    check_supports(t, sup, W, 100, 100)
    # the rows of the candidates against the oracle on the swapped trees, +ASC shift included
    moves = t.evaluate_nnis5_batch(first_row=1)
    okw = dict(n=4, seq_type=0, pat=pat, freq=freq, invar=None, model=model)
    check_rows_against_oracle(t, oracle, okw, freq, moves, 1, range(0, len(moves), 3), n_unobs=4, nsites=nsite)
    # padding: the device rows behind nptn stay zero, so a product with the full matrix equals the product of the fetched part
    got = t.ptnlh_rell(np.arange(1 + 2 * nb), 100)
    want = np.array([t.ptnlh_fetch(r) for r in range(1 + 2 * nb)]) @ W.astype(np.float64).T
    np.testing.assert_allclose(got, want, rtol=1e-12)


# ---- 6. errors ----------------------------------------------------------------------------------------------------------
def test_invalid_arguments(pkg, synth, oracle):
    lib = pkg.libiqhip()
    t, okw, freq = make_case(synth, oracle, pkg, 4, 4, 0, 6, 100, 8200)
    t.compute_likelihood()
    moves = t.evaluate_nnis5_batch(first_row=1)              # store of 7 rows
    out = np.zeros(7 * 8)
    dp = out.ctypes.data_as(C.POINTER(C.c_double))
    lh3 = np.array([-100.0, -101.0, -102.0])
    lp = lh3.ctypes.data_as(C.POINTER(C.c_double))
    sup = (pkg.BranchSupport * 1)()

    def rows_ptr(v):
        a = np.array(v, dtype=np.int32)
        return a, a.ctypes.data_as(C.POINTER(C.c_int32))

    keep, ok = rows_ptr([0, 1, 2])
    # no samples uploaded
    assert lib.iqhip_branch_tests(t.engine, ok, lp, 1, 4, 0, sup) == IQHIP_ERR_INVALID
    assert b"no bootstrap samples" in lib.iqhip_last_error()
    assert lib.iqhip_ptnlh_rell(t.engine, ok, 3, 4, dp) == IQHIP_ERR_INVALID
    t.set_boot_samples(boot_samples(np.random.default_rng(1), freq, 8))
    assert lib.iqhip_branch_tests(t.engine, ok, lp, 1, 8, 8, sup) == 0
    # replicates beyond the uploaded samples
    assert lib.iqhip_branch_tests(t.engine, ok, lp, 1, 9, 0, sup) == IQHIP_ERR_INVALID
    assert lib.iqhip_branch_tests(t.engine, ok, lp, 1, 0, 9, sup) == IQHIP_ERR_INVALID
    assert lib.iqhip_ptnlh_rell(t.engine, ok, 3, 9, dp) == IQHIP_ERR_INVALID
    assert lib.iqhip_ptnlh_rell(t.engine, ok, 3, 0, dp) == IQHIP_ERR_INVALID
    # a row out of range
    for bad in ([0, 1, 7], [0, -1, 2]):
        keep2, badp = rows_ptr(bad)
        assert lib.iqhip_branch_tests(t.engine, badp, lp, 1, 8, 0, sup) == IQHIP_ERR_INVALID
        assert lib.iqhip_ptnlh_rell(t.engine, badp, 3, 8, dp) == IQHIP_ERR_INVALID
    assert lib.iqhip_ptnlh_fetch(t.engine, 7, dp) == IQHIP_ERR_INVALID
    assert lib.iqhip_ptnlh_fetch(t.engine, -1, dp) == IQHIP_ERR_INVALID
    assert lib.iqhip_ptnlh_put_current(t.engine, 7, pkg.leaf_end(0), pkg.leaf_end(1)) == IQHIP_ERR_INVALID
    assert lib.iqhip_ptnlh_reserve(t.engine, -1) == IQHIP_ERR_INVALID
    # nbranch < 1, null arguments
    assert lib.iqhip_branch_tests(t.engine, ok, lp, 0, 8, 0, sup) == IQHIP_ERR_INVALID
    assert lib.iqhip_branch_tests(t.engine, None, lp, 1, 8, 0, sup) == IQHIP_ERR_INVALID
    assert lib.iqhip_branch_tests(None, ok, lp, 1, 8, 0, sup) == IQHIP_ERR_INVALID
    assert lib.iqhip_ptnlh_rell(t.engine, ok, 0, 8, dp) == IQHIP_ERR_INVALID
    # a task row outside the store
    task = (pkg.BranchTask * 1)(pkg.BranchTask(None, 0, 10, pkg.key_end(1), pkg.key_end(2), 0.1, 1e-6, 100.0, 1e-6))
    res = (pkg.BranchResult * 1)()
    keep3, big = rows_ptr([7])
    assert lib.iqhip_optimize_branch_batch_rows(t.engine, task, 1, None, res, big) == IQHIP_ERR_INVALID
    # the host mirror
    with pytest.raises(pkg.HostError, match="more replicates"):
        t.test_all_branches(9)
    # the engine still works
    assert lib.iqhip_branch_tests(t.engine, ok, lp, 1, 8, 8, sup) == 0


def test_sharded_engine_is_unsupported(pkg, synth, oracle):
    lib = pkg.libiqhip()
    t, okw, freq = make_case(synth, oracle, pkg, 4, 4, 0, 6, 400, 8300, sharded=2)
    t.compute_likelihood()
    assert lib.iqhip_num_shards(t.engine) == 2
    t.set_boot_samples(boot_samples(np.random.default_rng(1), freq, 8))
    out = np.zeros(t.nptn * 8)
    dp = out.ctypes.data_as(C.POINTER(C.c_double))
    rows = np.array([0, 1, 2], dtype=np.int32)
    ip = rows.ctypes.data_as(C.POINTER(C.c_int32))
    sup = (pkg.BranchSupport * 1)()
    task = (pkg.BranchTask * 1)(pkg.BranchTask(None, 0, 10, pkg.key_end(1), pkg.key_end(2), 0.1, 1e-6, 100.0, 1e-6))
    res = (pkg.BranchResult * 1)()
    for rc in (lib.iqhip_ptnlh_reserve(t.engine, 3), lib.iqhip_ptnlh_put_current(t.engine, 0, pkg.leaf_end(0), pkg.key_end(1)),
               lib.iqhip_ptnlh_fetch(t.engine, 0, dp), lib.iqhip_optimize_branch_batch_rows(t.engine, task, 1, None, res, ip),
               lib.iqhip_branch_tests(t.engine, ip, dp, 1, 8, 0, sup), lib.iqhip_ptnlh_rell(t.engine, ip, 3, 8, dp)):
        assert rc == IQHIP_ERR_UNSUPPORTED
    with pytest.raises(pkg.HostError):
        t.test_all_branches(8)
