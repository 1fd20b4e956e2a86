"""SH-aLRT / local-bootstrap branch supports, the parts that need no device: the numpy restatement of the reference's
replicate loop (PhyloTree::testOneBranch, phylotree.cpp:4014-4053) that the GPU tests compare the engine with, the new
symbols of libiqhip.so, the refusal of a planning-only engine and the node labels (phylotree.cpp:4078-4091)."""
import ctypes as C

import numpy as np


def restate_branch_tests(R, lh):
    """phylotree.cpp:3994-4053 on the weighted sums R[3, S] (rows: current tree, NNI 1, NNI 2) and the three total lnL.
    -> dict(sh, lbp: boolean outcome per replicate; margin: the smallest decision margin per replicate; abayes, alrt_stat)"""
    R = np.asarray(R, dtype=np.float64)
    lh = np.asarray(lh, dtype=np.float64)
    aLRT = lh[0] - lh[1] if lh[1] > lh[2] else lh[0] - lh[2]
    S = R.shape[1]
    sh = np.zeros(S, dtype=bool)
    lbp = np.zeros(S, dtype=bool)
    margin = np.zeros(S)
    for i in range(S):
        lh_new = R[:, i]
        lbp[i] = lh_new[0] > lh_new[1] and lh_new[0] > lh_new[2]
        cs = lh_new - lh
        if cs[0] >= cs[1] and cs[0] >= cs[2]:
            cs_best = cs[0]
            cs_2nd = cs[1] if cs[1] > cs[2] else cs[2]
        elif cs[1] >= cs[2]:
            cs_best = cs[1]
            cs_2nd = cs[0] if cs[0] > cs[2] else cs[2]
        else:
            cs_best = cs[2]
            cs_2nd = cs[0] if cs[0] > cs[1] else cs[1]
        sh[i] = aLRT > (cs_best - cs_2nd) + 0.05
        margin[i] = min(abs(lh_new[0] - lh_new[1]), abs(lh_new[0] - lh_new[2]), abs(aLRT - (cs_best - cs_2nd) - 0.05))
    return dict(sh=sh, lbp=lbp, margin=margin, alrt_stat=2.0 * aLRT,
                abayes=1.0 / (1.0 + np.exp(lh[1] - lh[0]) + np.exp(lh[2] - lh[0])))


def test_restatement_on_a_hand_made_example():
    # three trees x five replicates; lh = (-100, -103, -101): aLRT = lh0 - lh2 = 1 (lh2 is the better neighbour)
    lh = [-100.0, -103.0, -101.0]
    R = np.array([[-100.0, -99.0, -104.0, -100.0, -101.0],
                  [-103.0, -98.0, -104.5, -108.0, -104.0],
                  [-101.0, -100.5, -105.5, -100.0, -101.0]])
    # LBP: tree 0 strictly best in replicates 0 and 2 (1: tree 1 wins; 3, 4: ties with tree 2 do not count)
    # centred sums cs = R - lh:        rep0 (0, 0, 0)    rep1 (1, 5, .5)   rep2 (-4, -1.5, -4.5) rep3 (0, -5, 1)  rep4 (-1, -1, 0)
    # best - second:                   0                 4                 4                   1                1
    # SH-aLRT: 1 > d + 0.05            yes               no                no                  no               no
    r = restate_branch_tests(R, lh)
    assert r["lbp"].tolist() == [True, False, True, False, False]
    assert r["sh"].tolist() == [True, False, False, False, False]
    assert r["alrt_stat"] == 2.0
    assert abs(r["abayes"] - 1.0 / (1.0 + np.exp(-3.0) + np.exp(-1.0))) < 1e-15
    np.testing.assert_allclose(r["margin"], [0.95, 1.0, 0.5, 0.0, 0.0], atol=1e-12)
    # tie order of the reference: cs0 == cs1 == cs2 takes tree 0 as best and cs[2] as second (cs[1] > cs[2] is false)
    r = restate_branch_tests(np.array([[-100.0], [-103.0], [-101.0]]), lh)
    assert r["sh"].tolist() == [True] and r["lbp"].tolist() == [True]
    # lh1 > lh0 (the reference warns and goes on): aLRT is negative, no replicate can pass the SH test
    r = restate_branch_tests(R, [-100.0, -99.0, -101.0])
    assert r["alrt_stat"] == -2.0 and not r["sh"].any()


NEW_SYMBOLS = ("iqhip_ptnlh_reserve", "iqhip_ptnlh_put_current", "iqhip_ptnlh_fetch", "iqhip_optimize_branch_batch_rows",
               "iqhip_branch_tests", "iqhip_ptnlh_rell")


def test_new_symbols_exist(pkg):
    lib = pkg.libiqhip()
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s), s
        assert s in pkg.IQHIP_SYMBOLS
    assert lib.iqhip_abi_version() == 2
    host = pkg.libiqhost()
    for s in ("iqhost_test_all_branches", "iqhost_evaluate_nnis5_batch_rows", "iqhost_support_tree_string"):
        assert hasattr(host, s), s


def test_planning_only_engine_refuses_the_new_calls(pkg):
    lib = pkg.libiqhip()
    e = C.c_void_p()
    assert lib.iqhip_debug_create_planner(C.byref(e), 4, 4, 1000, 8, 256, 18, 1) == 0
    try:
        out = np.zeros(1000)
        dp = out.ctypes.data_as(C.POINTER(C.c_double))
        rows = np.zeros(3, dtype=np.int32)
        ip = rows.ctypes.data_as(C.POINTER(C.c_int32))
        sup = (pkg.BranchSupport * 1)()
        task = (pkg.BranchTask * 1)(pkg.BranchTask(None, 0, 10, pkg.key_end(1), pkg.key_end(2), 0.1, 1e-6, 100.0, 1e-6))
        res = (pkg.BranchResult * 1)()
        calls = [lambda: lib.iqhip_ptnlh_reserve(e, 3),
                 lambda: lib.iqhip_ptnlh_put_current(e, 0, pkg.key_end(1), pkg.key_end(2)),
                 lambda: lib.iqhip_ptnlh_fetch(e, 0, dp),
                 lambda: lib.iqhip_optimize_branch_batch_rows(e, task, 1, None, res, ip),
                 lambda: lib.iqhip_branch_tests(e, ip, dp, 1, 10, 0, sup),
                 lambda: lib.iqhip_ptnlh_rell(e, ip, 3, 1, dp)]
        for call in calls:
            assert call() == 2                                  # IQHIP_ERR_INVALID
            assert b"planning-only" in lib.iqhip_last_error()
    finally:
        lib.iqhip_destroy(e)


def test_support_labels(pkg):
    """the reference prints `SH-aLRT[/LBP]` in percent with ostringstream precision 3 (phylotree.cpp:4078-4091) on the node
    of an internal branch that is farther from the root leaf; no device is needed for the string"""
    t = pkg.PhyloTree("((0:0.1,1:0.2):0.05,2:0.3,(3:0.1,(4:0.2,5:0.1):0.07):0.04);")
    inner = [(a, b) for a in range(t.num_nodes) for b, _ in t.neighbors(a)
             if a < b and len(t.neighbors(a)) > 1 and len(t.neighbors(b)) > 1]
    assert len(inner) == 3
    sup = np.zeros(3, dtype=pkg.SUPPORT_DTYPE)
    for q, (a, b) in enumerate(inner):
        sup["node1"][q], sup["node2"][q] = a, b
    sup["sh_alrt"] = [0.873, 1.0, 0.0]
    sup["lbp"] = [0.5, 0.12345, 1.0]
    both = t.support_tree_string(sup, True, True)
    only_sh = t.support_tree_string(sup, True, False)
    only_lbp = t.support_tree_string(sup, False, True)
    for lab in ("87.3/50", "100/12.3", "0/100"):
        assert ")" + lab + ":" in both, (lab, both)
    for lab in ("87.3", "100", "0"):
        assert ")" + lab + ":" in only_sh, (lab, only_sh)
    for lab in ("/50", "/12.3", "/100"):                        # the reference writes the separator even without SH-aLRT
        assert ")" + lab + ":" in only_lbp, (lab, only_lbp)
    # same topology and lengths as the plain string, labels only added
    import re
    assert re.sub(r"\)[0-9./]+:", "):", both) == t.tree_string()
    t.close()
