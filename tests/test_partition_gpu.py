"""Edge-linked partition models on the device: the joint branch solve of a group of engines (iqhip_partition_*,
kernels_partnewton.hip) against the restatement of tests/partition_ref.py over the CPU oracle -- the minimize_newton loop
of oracle_driver.py over sum_p r_p df_p(r_p x), sum_p r_p^2 ddf_p(r_p x).  Tolerances are those of
tests/test_newton_oracle_gpu.py for a single solve: |optx - ref| <= 1e-9 max(1, |ref|), the same number of derivative
evaluations, d2l to 1e-6; per-member lnL as tests/test_parity_gpu.py checks a branch lnL (1e-9 relative)."""
import ctypes as C
import os

import numpy as np
import pytest

import partition_ref as pr

pytestmark = pytest.mark.gpu

LNL_RTOL = 1e-9   # tests/test_parity_gpu.py
ERR_INVALID, ERR_UNSUPPORTED = 2, 3


def prepare(trees, a, b):
    """pending partials of both ends + theta of branch (a, b) on every member (the member's own derivative path)"""
    for t in trees:
        t.reset_theta()
        t.compute_likelihood_derv(a, b)


def check_solve(got, ref, where):
    optx, d2l, ns, _ = got
    ref_x, ref_d2l, pts, status = ref
    assert status == "ok", where
    assert ns == len(pts), (where, ns, pts)
    assert abs(optx - ref_x) <= 1e-9 * max(1.0, abs(ref_x)), (where, optx, ref_x)
    assert abs(d2l - ref_d2l) <= 1e-6 * max(1.0, abs(ref_d2l)), (where, d2l, ref_d2l)


@pytest.fixture(scope="module")
def mixed(pkg, synth, oracle):
    nwk, members = pr.mixed_group(synth, oracle)
    trees = [pr.device_member(pkg, nwk, d) for d in members]
    ots = [pr.oracle_member(oracle, nwk, d) for d in members]
    for t in trees:
        t.compute_likelihood()
    sup = oracle.OracleTree(nwk, 4, 0, members[0]["pat"], members[0]["freq"], None, members[0]["model"])
    g = pkg.PartitionGroup(trees)
    g.set_rates(pr.MIXED_RATES)
    yield dict(nwk=nwk, members=members, trees=trees, ots=ots, sup=sup, group=g, edges=pr.tree_edges(sup, len(sup.adj)))
    g.close()


def test_mixed_group_every_branch(mixed):
    """case 1: DNA GTR+G4 (3 tiles of 64, the last partial), DNA with one category (less than a tile), protein +G4
    (16-pattern tiles, the last partial), binary with 2 categories (the embedded route); all-unknown rows; 13 branches x 5
    setups"""
    pats = [d["pat"].shape[1] for d in mixed["members"]]
    assert 128 < pats[0] < 192 and pats[1] < 64 and pats[2] % 16 != 0, pats
    assert len(mixed["edges"]) == 13
    g, ots, rates = mixed["group"], mixed["ots"], pr.MIXED_RATES
    nchecked, worst = 0, 0.0
    for (a, b) in mixed["edges"]:
        prepare(mixed["trees"], a, b)
        th = [ot.theta(a, b) for ot in ots]
        thetas = [t for t, _ in th]
        for (x1, xg, x2, xacc, ms) in pr.NEWTON_SETUPS:
            xg = mixed["sup"].length(a, b) if xg is None else xg
            ref = pr.joint_minimize_newton(ots, rates, a, b, x1, xg, x2, xacc, ms, thetas)
            got = g.newton_branch(xg, x1, x2, xacc, ms)
            check_solve(got, ref, (a, b, x1, xg, x2, ms))
            want = pr.joint_lnl_from_theta(ots, rates, a, b, got[0], th)
            np.testing.assert_allclose(got[3], want, rtol=LNL_RTOL, atol=0)
            if ms == 100 and x2 == 100.0 and x1 == 1e-6:
                own = ots[0].minimize_newton(a, b, x1, xg, x2, xacc, ms, theta=thetas[0])[0]
                worst = max(worst, abs(np.log(ref[0] / own)))
            nchecked += 1
    assert nchecked == 65
    assert worst > np.log(1.1)   # the joint optimum is not member 0's: a solve that looks at one member fails above
    # the same per-member values from the stand-alone call
    a, b = mixed["edges"][-1]
    np.testing.assert_allclose(g.lnl_from_theta(0.07), pr.joint_lnl_from_theta(ots, rates, a, b, 0.07), rtol=LNL_RTOL, atol=0)


def test_single_member_equals_newton_branch(pkg, mixed):
    """case 2"""
    lib = pkg.libiqhip()
    for k in (0, 2, 3):
        t, ot = mixed["trees"][k], mixed["ots"][k]
        g = pkg.PartitionGroup([t])
        for (a, b) in mixed["edges"][:4]:
            prepare([t], a, b)
            xg = ot.length(a, b)
            optx, d2l, ns = C.c_double(), C.c_double(), C.c_int()
            assert lib.iqhip_newton_branch(t.engine, xg, 1e-6, 100.0, 1e-6, 100, C.byref(optx), C.byref(d2l), C.byref(ns)) == 0
            got = g.newton_branch(xg, 1e-6, 100.0, 1e-6, 100)
            assert got[2] == ns.value
            assert abs(got[0] - optx.value) <= 1e-9 * max(1.0, abs(optx.value))
            assert abs(got[1] - d2l.value) <= 1e-6 * max(1.0, abs(d2l.value))
        g.close()


def test_several_work_items_per_member(pkg, synth, oracle):
    """case 3: DNA 12 taxa x 40 000 sites (hundreds of 64-pattern tiles: many work items) with a codon member"""
    nwk = synth.random_tree_newick(12, 31, 0.02, 0.2)
    rates = [0.8, 1.7]
    members = [pr.member_data(synth, oracle, nwk, 4, 4, pr.SEQ_DNA, 40000, 600, rates[0]),
               pr.member_data(synth, oracle, nwk, 64, 1, pr.SEQ_CODON, 600, 610, rates[1])]
    assert members[0]["pat"].shape[1] > 16 * 64 * 2   # more than two work items of 16 tiles
    trees = [pr.device_member(pkg, nwk, d) for d in members]
    ots = [pr.oracle_member(oracle, nwk, d) for d in members]
    for t in trees:
        t.compute_likelihood()
    g = pkg.PartitionGroup(trees)
    g.set_rates(rates)
    sup = oracle.OracleTree(nwk, 4, 0, members[0]["pat"], members[0]["freq"], None, members[0]["model"])
    for (a, b) in pr.tree_edges(sup, len(sup.adj))[:5]:
        prepare(trees, a, b)
        th = [ot.theta(a, b) for ot in ots]
        xg = sup.length(a, b)
        ref = pr.joint_minimize_newton(ots, rates, a, b, 1e-6, xg, 100.0, 1e-6, 100, [t for t, _ in th])
        got = g.newton_branch(xg, 1e-6, 100.0, 1e-6, 100)
        check_solve(got, ref, (a, b))
        np.testing.assert_allclose(got[3], pr.joint_lnl_from_theta(ots, rates, a, b, got[0], th), rtol=LNL_RTOL, atol=0)
    g.close()


def test_many_members(pkg, synth, oracle):
    """case 4: 70 members, more than the 64 the update kernel takes per round"""
    assert 70 > 64   # kPartUpdateThreads (iqhip_internal.h)
    nwk = synth.random_tree_newick(8, 41, 0.02, 0.2)
    rng = np.random.default_rng(42)
    rates = list(rng.uniform(0.2, 3.0, 70))
    members = [pr.member_data(synth, oracle, nwk, 4, 4, pr.SEQ_DNA, int(rng.integers(40, 131)), 700 + 3 * k, rates[k])
               for k in range(70)]
    trees = [pr.device_member(pkg, nwk, d) for d in members]
    ots = [pr.oracle_member(oracle, nwk, d) for d in members]
    for t in trees:
        t.compute_likelihood()
    g = pkg.PartitionGroup(trees)
    g.set_rates(rates)
    sup = oracle.OracleTree(nwk, 4, 0, members[0]["pat"], members[0]["freq"], None, members[0]["model"])
    for (a, b) in pr.tree_edges(sup, len(sup.adj))[:3]:
        prepare(trees, a, b)
        th = [ot.theta(a, b) for ot in ots]
        xg = sup.length(a, b)
        ref = pr.joint_minimize_newton(ots, rates, a, b, 1e-6, xg, 100.0, 1e-6, 100, [t for t, _ in th])
        got = g.newton_branch(xg, 1e-6, 100.0, 1e-6, 100)
        check_solve(got, ref, (a, b))
        np.testing.assert_allclose(got[3], pr.joint_lnl_from_theta(ots, rates, a, b, got[0], th), rtol=LNL_RTOL, atol=0)
    tm = g.timing()
    assert tm["launches"] >= 1 + 2 * got[2]   # init + (derivative, update) per evaluation
    g.close()


def test_same_bits(mixed):
    """case 5: twice the same call; one step per chunk"""
    g = mixed["group"]
    a, b = mixed["edges"][3]
    prepare(mixed["trees"], a, b)
    xg = mixed["sup"].length(a, b)
    runs = [g.newton_branch(xg, 1e-6, 100.0, 1e-6, 100) for _ in range(2)]
    os.environ["IQHIP_PART_STEPS"] = "1"
    try:
        runs.append(g.newton_branch(xg, 1e-6, 100.0, 1e-6, 100))
    finally:
        del os.environ["IQHIP_PART_STEPS"]
    for r in runs[1:]:
        assert r[:3] == runs[0][:3]
        assert np.array_equal(r[3], runs[0][3])


def test_nan_member_contributes_nothing(pkg, mixed):
    """case 6: one member's theta is NaN (a host-written NaN vector at one end of the branch): phylokernel.h:647-651 per
    member, so the result is the restatement's with that member's derivatives at 0"""
    lib = pkg.libiqhip()
    trees, ots, rates = mixed["trees"], mixed["ots"], pr.MIXED_RATES
    a, b = next((a, b) for (a, b) in mixed["edges"] if not mixed["sup"].is_leaf(a) and not mixed["sup"].is_leaf(b))
    prepare(trees, a, b)
    t = trees[1]
    key_ab, key_ba = t.neighbor_info(a, b)["key"], t.neighbor_info(b, a)["key"]
    good = t.fetch_partial(a, b)
    sc = np.ascontiguousarray(t.fetch_scale_num(a, b), dtype=np.int16)
    bad = np.full_like(good, np.nan)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int16)
    try:
        assert lib.iqhip_upload_partial(t.engine, key_ab, bad.ctypes.data_as(dp), sc.ctypes.data_as(ip)) == 0
        assert lib.iqhip_compute_theta(t.engine, pkg.key_end(key_ba), pkg.key_end(key_ab)) == 0
        thetas = [ot.theta(a, b)[0] for ot in ots]
        thetas[1] = np.full_like(thetas[1], np.nan)
        xg = mixed["sup"].length(a, b)
        ref = pr.joint_minimize_newton(ots, rates, a, b, 1e-6, xg, 100.0, 1e-6, 100, thetas)
        got = mixed["group"].newton_branch(xg, 1e-6, 100.0, 1e-6, 100, want_lnl=False)
        check_solve(got, ref, (a, b))
    finally:
        good = np.ascontiguousarray(good)
        assert lib.iqhip_upload_partial(t.engine, key_ab, good.ctypes.data_as(dp), sc.ctypes.data_as(ip)) == 0
        t.reset_theta()


def test_state_and_refusals(pkg, synth, oracle, mixed):
    """case 9"""
    lib = pkg.libiqhip()
    g, trees = mixed["group"], mixed["trees"]
    (a, b), (a2, b2) = mixed["edges"][0], mixed["edges"][5]
    prepare(trees, a, b)

    def code(fn):
        with pytest.raises(pkg.EngineError) as ei:
            fn()
        return ei.value.code

    assert code(lambda: g.newton_branch(0.1, 1e-6, 100.0, 1e-6, 0)) == ERR_INVALID        # max_steps < 1
    assert code(lambda: g.newton_branch(0.1, 2.0, 1.0, 1e-6, 100)) == ERR_INVALID         # x1 > x2
    for bad in ([1.0, 0.0, 1.0, 1.0], [1.0, -2.0, 1.0, 1.0], [1.0, float("nan"), 1.0, 1.0], [1.0, float("inf"), 1.0, 1.0]):
        assert code(lambda: g.set_rates(bad)) == ERR_INVALID
    # theta built for different branches on two members
    trees[2].reset_theta()
    trees[2].compute_likelihood_derv(a2, b2)
    assert code(lambda: g.newton_branch(0.1, 1e-6, 100.0, 1e-6, 100)) == ERR_INVALID
    assert b"another branch" in lib.iqhip_last_error()
    assert code(lambda: g.lnl_from_theta(0.1)) == ERR_INVALID
    # theta missing on one member: a fresh engine that has never built one
    d = mixed["members"][1]
    fresh = pr.device_member(pkg, mixed["nwk"], d)
    fresh.compute_likelihood()
    g2 = pkg.PartitionGroup([trees[0], fresh])
    assert code(lambda: g2.newton_branch(0.1, 1e-6, 100.0, 1e-6, 100)) == ERR_INVALID
    assert b"theta not computed" in lib.iqhip_last_error()
    g2.close()
    # a member listed twice; members that cannot join
    assert code(lambda: pkg.PartitionGroup([trees[0], trees[0]])) == ERR_INVALID
    nwk = mixed["nwk"]
    n = 4
    pat = np.ascontiguousarray(np.concatenate([d["pat"], np.tile(np.arange(n, dtype=np.uint8)[None, :], (8, 1))], axis=1))
    freq = np.concatenate([d["freq"], np.zeros(n)])
    asc = pkg.PhyloTree(nwk)
    asc.set_alignment(4, 0, pat, freq)
    asc.set_ascertainment(n, float(freq.sum()))
    asc.set_model(d["model"])
    asc.attach_engine(0)
    asc.compute_likelihood()
    assert code(lambda: pkg.PartitionGroup([trees[0], asc])) == ERR_UNSUPPORTED
    mix = pkg.PhyloTree(nwk)
    mix.set_alignment(4, 0, d["pat"], d["freq"])
    mix.set_model(synth.mixture_model(4, 2, 5, alpha=0.9, ncat=2))
    mix.attach_engine(0)
    mix.compute_likelihood()
    assert code(lambda: pkg.PartitionGroup([trees[0], mix])) == ERR_UNSUPPORTED
    d0 = mixed["members"][0]                 # (a shard takes at least 64 patterns)
    sh = pkg.PhyloTree(nwk)
    sh.set_alignment(4, 0, d0["pat"], d0["freq"])
    sh.set_model(d0["model"])
    sh.attach_engine_sharded([0, 0], pkg.REDUCE_HOST)
    sh.compute_likelihood()
    assert code(lambda: pkg.PartitionGroup([trees[0], sh])) == ERR_UNSUPPORTED
    # the members work on their own after a group is destroyed
    t, ot = trees[0], mixed["ots"][0]
    g3 = pkg.PartitionGroup([t, trees[1]])
    prepare([t, trees[1]], a, b)
    g3.newton_branch(0.1, 1e-6, 100.0, 1e-6, 100)
    g3.close()
    prepare([t], a2, b2)
    xg = ot.length(a2, b2)
    ref_x, ref_d2l, pts, status = ot.minimize_newton(a2, b2, 1e-6, xg, 100.0, 1e-6, 100)
    optx, d2l, ns = C.c_double(), C.c_double(), C.c_int()
    assert lib.iqhip_newton_branch(t.engine, xg, 1e-6, 100.0, 1e-6, 100, C.byref(optx), C.byref(d2l), C.byref(ns)) == 0
    assert status == "ok" and ns.value == len(pts) and abs(optx.value - ref_x) <= 1e-9 * max(1.0, abs(ref_x))


# ---- the host mirror (host/supertree_host.h) ---------------------------------------------------------------------------
EM_RATE_RTOL = 1.4e-11   # tests/test_em_gpu.py, its Brent-optimised rates


def super_tree(pkg, mixed, rates=None, fixed_rates=True):
    st = pkg.PhyloSuperTree(mixed["nwk"], mixed["members"], fixed_rates=fixed_rates)
    if rates is not None:
        st.part_rates = rates
    return st


def fresh_oracles(oracle, mixed, rates):
    return [pr.oracle_member(oracle, mixed["nwk"], d, scale=r) for d, r in zip(mixed["members"], rates)]


def test_mirror_likelihood_and_branch_pass(pkg, oracle, mixed):
    """case 7: computeLikelihood; one optimizeAllBranches pass branch by branch against the restatement, the oracle trees
    receiving the device's accepted length after each branch; the same pass as one call"""
    rates = pr.MIXED_RATES
    st = super_tree(pkg, mixed, rates)
    ots = fresh_oracles(oracle, mixed, rates)
    want = [ot.likelihood()[0] for ot in ots]
    lnl = st.compute_likelihood()
    np.testing.assert_allclose(st.part_lnl(), want, rtol=LNL_RTOL, atol=0)
    assert abs(lnl - sum(want)) <= LNL_RTOL * abs(sum(want))
    order = st.branch_order()
    assert len(order) == 13 and sorted(tuple(sorted(e)) for e in order) == sorted(mixed["edges"])
    for (a, b) in order:
        cur = st.branch_length(a, b)
        ref = pr.joint_minimize_newton(ots, rates, a, b, 1e-6, cur, 100.0, 1e-6, 100)
        assert ref[3] == "ok"
        got = st.optimize_one_branch(a, b)
        assert abs(got - ref[0]) <= 1e-9 * max(1.0, abs(ref[0])), (a, b, got, ref[0])
        np.testing.assert_allclose(st.part_lnl(), pr.joint_lnl_from_theta(ots, rates, a, b, got), rtol=LNL_RTOL, atol=0)
        for ot, r in zip(ots, rates):
            ot.set_length(a, b, r * got)
    assert st.counters()["group_solves"] == 13
    final = sum(ot.likelihood()[0] for ot in ots)
    assert final > sum(want)
    st2 = super_tree(pkg, mixed, rates)
    lnl2 = st2.optimize_all_branches(iterations=1)
    assert abs(lnl2 - final) <= LNL_RTOL * abs(final)
    for (a, b) in order:
        assert abs(st2.branch_length(a, b) - st.branch_length(a, b)) <= 1e-9 * max(1.0, st.branch_length(a, b))
    for t, r in zip(st2.members, rates):   # r_p x is written to every member
        for (a, b) in order[:3]:
            assert t.neighbor_info(a, b)["length"] == r * st2.branch_length(a, b)
    st.close()
    st2.close()


def test_mirror_diverged_newton_reset(pkg, oracle, mixed):
    """case 7, the tight upper bound: every optimum above 0.0475 counts as diverged (phylotree.cpp:2167-2176), decided on
    the summed lnL"""
    rates = pr.MIXED_RATES
    st = super_tree(pkg, mixed, rates)
    st.set_branch_bounds(1e-6, 0.05)
    ots = fresh_oracles(oracle, mixed, rates)
    st.compute_likelihood()
    ndiv = 0
    for (a, b) in st.branch_order():
        cur = st.branch_length(a, b)
        optx, _, _, status = pr.joint_minimize_newton(ots, rates, a, b, 1e-6, cur, 0.05, 1e-6, 100)
        assert status == "ok"
        want = optx
        if optx > 0.05 * 0.95:
            opt_lh = pr.joint_lnl_from_theta(ots, rates, a, b, optx).sum()
            orig_lh = pr.joint_lnl_from_theta(ots, rates, a, b, cur).sum()
            if orig_lh > opt_lh:
                want = cur
            ndiv += 1
        got = st.optimize_one_branch(a, b)
        assert abs(got - want) <= 1e-9 * max(1.0, want), (a, b, got, want, optx)
        for ot, r in zip(ots, rates):
            ot.set_length(a, b, r * got)
    assert ndiv >= 2 and st.counters()["diverged"] == ndiv
    st.close()


def test_gene_rates(pkg, oracle, mixed):
    """case 8: optimizeGeneRate against the restatement's lockstep Brent searches"""
    members, nwk = mixed["members"], mixed["nwk"]
    nsites = [float(d["freq"].sum()) for d in members]
    st = super_tree(pkg, mixed, fixed_rates=False)
    before = st.compute_likelihood()
    res = st.optimize_gene_rates(0.001)
    cache = {}

    def lnl_at(p, s):
        if (p, s) not in cache:
            cache[(p, s)] = pr.oracle_member(oracle, nwk, members[p], scale=s).likelihood()[0]
        return cache[(p, s)]

    ref_rates, ref_scale, ref_evals, ref_rounds, ref_lnl = pr.gene_rate_step(lnl_at, [1.0] * 4, nsites, 0.001, pkg.BrentStateMachine)
    print("gene rates: device", res["rates"], "restatement", ref_rates, "evals", res["evals"], ref_evals)
    assert res["evals"] == ref_evals
    np.testing.assert_allclose(res["rates"], ref_rates, rtol=EM_RATE_RTOL, atol=0)
    assert abs(float(np.dot(res["rates"], nsites)) / sum(nsites) - 1.0) <= 1e-12
    assert res["lnl"] >= before
    assert abs(res["lnl"] - ref_lnl.sum()) <= LNL_RTOL * abs(ref_lnl.sum())
    assert res["rounds"] == max(res["evals"]) < sum(res["evals"])     # group traversals: the longest search, not the sum
    assert st.counters()["group_traversals"] == res["rounds"]
    # the super tree was scaled by the inverse of the factor the rates were divided by
    (a, b) = mixed["edges"][0]
    assert abs(st.branch_length(a, b) - ref_scale * mixed["sup"].length(a, b)) <= 1e-9 * mixed["sup"].length(a, b)
    after = st.compute_likelihood()
    assert abs(after - res["lnl"]) <= 1e-9 * abs(after)
    st.close()
    fixed = super_tree(pkg, mixed, fixed_rates=True)
    lnl = fixed.optimize_parameters()
    assert np.array_equal(fixed.part_rates, np.ones(4))
    assert lnl > before
    fixed.close()
