"""GPU: no allocation outlives its engine, and a failed allocation leaves nothing behind (iqhip_debug_memory,
iqhip_debug_fail_alloc).

Every device and pinned-host buffer of an engine or a partition group is a DevBuf or a PinBuf (iqhip_internal.h), and both
allocate through one pair of functions that counts bytes.  So "create, use every feature, destroy" must bring both counts
back to where they were, whatever the engine's shape, and an engine whose creation fails half way must return a null handle
with the counts where they were.  The counts are process-wide and other engines of the session may be alive: every
assertion is relative to the reading at the start of the test.

Shapes: 5 taxa and 100 patterns where the path allows it; the 20-state engine has the 8192 padded patterns from which
cherry_candidate (engine.hip) switches the cherry tables and their pair engine on, and 16 taxa: the plan of the 12-taxon
tree has no units below its top stage, whose cherries are computed, not looked up (plan.hip assign_cherry_tables); the sharded engine has the 200 patterns tests/test_feature_refusals.py uses."""
import ctypes as C
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DP = C.POINTER(C.c_double)
ERR_NOMEM = 5
CHERRY_MIN_PATTERNS = 8 * 1024   # engine.hip cherry_candidate
MAX_STEPS = 64                   # allocations a creation may make before it succeeds: a condition of the tests below


def reading(pkg):
    gc.collect()   # (a tree another test left to the collector must not free its engine in the middle of a test)
    return pkg.debug_memory()


def case(synth, n, ncat, nptn, ntaxa, seed=3):
    model = (synth.gtr_model(alpha=0.9 if ncat > 1 else None, ncat=ncat) if n == 4
             else synth.random_reversible_model(n, 3, alpha=0.9 if ncat > 1 else None, ncat=ncat))
    rng = np.random.default_rng(seed)
    return dict(n=n, seq_type={4: 0, 20: 1, 64: 2}[n], ncat=ncat, nptn=nptn, ntaxa=ntaxa, model=model,
                nwk=synth.random_tree_newick(ntaxa, 1), states=rng.integers(0, n, size=(ntaxa, nptn)).astype(np.uint8),
                freq=rng.integers(1, 4, size=nptn).astype(np.float64))


def host_tree(pkg, c):
    t = pkg.PhyloTree(c["nwk"])
    t.set_mem_mode(pkg.LM_ALL_BRANCH)
    t.set_alignment(c["n"], c["seq_type"], c["states"], c["freq"])
    t.set_model(c["model"])
    t.set_likelihood_kernel(pkg.LK_EIGEN_HIP)
    return t


def attached(pkg, c, sharded=0):
    t = host_tree(pkg, c)
    if sharded:
        t.attach_engine_sharded([0] * sharded, pkg.REDUCE_HOST)
    else:
        t.attach_engine(0)
    return t


def use_everything(pkg, t, c, plain=True):
    """every feature that owns memory of its own, once (tools/check_leaks.py does the same at a larger size)"""
    rng = np.random.default_rng(5)
    t.compute_likelihood()
    t.optimize_all_branches(iterations=1)
    t.evaluate_nnis_batch()
    t.set_boot_samples(np.stack([c["freq"], c["freq"][::-1]]).astype(np.float32))
    t.compute_rell()
    t.ptnlh_reserve(2)
    two = rng.uniform(-12.0, -1.0, (2, c["nptn"]))
    for r in range(2):
        t.ptnlh_upload(r, two[r])
    t.tree_tests([0, 1], two @ c["freq"], 2, weighted=True)
    if plain:
        t.compute_dist()
        t.compute_parsimony()
    a = rng.uniform(0.05, 1.0, (5, 5))
    t.bionj((a + a.T) / 2)


@pytest.mark.parametrize("ncat", [1, 4])
def test_dna_engine_returns_everything(pkg, synth, ncat):
    start = reading(pkg)
    c = case(synth, 4, ncat, 100, 5)
    t = attached(pkg, c)
    use_everything(pkg, t, c)
    live = pkg.debug_memory()
    assert live[0] > start[0] and live[1] > start[1]
    t.close()
    assert pkg.debug_memory() == start


def test_protein_engine_with_cherry_tables_returns_everything(pkg, synth):
    start = reading(pkg)
    c = case(synth, 20, 4, CHERRY_MIN_PATTERNS, 16)
    t = attached(pkg, c)
    t.compute_likelihood()
    built, answered = C.c_int64(0), C.c_int64(0)
    assert pkg.libiqhip().iqhip_debug_cherry_tables(t.engine, C.byref(built), C.byref(answered)) == 0
    assert built.value > 0 and answered.value > 0   # the tables exist, and with them the pair engine
    t.optimize_all_branches(iterations=1)
    t.compute_parsimony()
    t.close()
    assert pkg.debug_memory() == start


def test_codon_engine_returns_everything(pkg, synth):
    start = reading(pkg)
    c = case(synth, 64, 1, 100, 5)
    t = attached(pkg, c)
    t.compute_likelihood()
    t.optimize_all_branches(iterations=1)
    t.compute_dist()
    t.compute_parsimony()
    t.close()
    assert pkg.debug_memory() == start


def test_sharded_engine_returns_everything(pkg, synth):
    start = reading(pkg)
    c = case(synth, 4, 4, 200, 5)
    t = attached(pkg, c, sharded=2)
    t.compute_likelihood()
    t.optimize_all_branches(iterations=1)
    t.set_boot_samples(c["freq"][None, :].astype(np.float32))
    t.compute_rell()
    t.close()
    assert pkg.debug_memory() == start


def two_members(pkg, synth):
    cs = [case(synth, 4, 4, 100, 5, seed=3), case(synth, 4, 1, 70, 5, seed=4)]
    trees = [attached(pkg, c) for c in cs]
    for t in trees:   # theta of one branch on every member
        t.compute_likelihood()
        t.compute_likelihood_derv(*t.current_branch())
    return trees


def test_partition_group_returns_everything(pkg, synth):
    start = reading(pkg)
    trees = two_members(pkg, synth)
    members_only = pkg.debug_memory()
    g = pkg.PartitionGroup(trees)
    g.newton_branch(0.1, 1e-6, 100.0, 1e-6, 100)
    g.lnl_from_theta(0.07)
    assert pkg.debug_memory() != members_only
    g.close()
    assert pkg.debug_memory() == members_only   # the group owns nothing of its members
    for t in trees:
        t.close()
    assert pkg.debug_memory() == start


# ---- creation with the k-th allocation failing, k = 1, 2, .. until it succeeds ----------------------------------------
def create_with_failures(pkg, create):
    """create() -> (status, handle).  Every failed creation: a status, a null handle, the counts untouched.  Returns the
    handle of the creation that succeeded and the number that failed."""
    start = pkg.debug_memory()
    for k in range(1, MAX_STEPS + 1):
        pkg.debug_fail_alloc(k)
        try:
            rc, h = create()
        finally:
            pkg.debug_fail_alloc(0)
        if rc == 0:
            assert h.value
            return h, k - 1
        assert not h.value, k
        assert pkg.debug_memory() == start, k
    pytest.fail("creation still failed with the %dth allocation failing" % MAX_STEPS)


def raw_lnl(pkg, e, c):
    """model, alignment and the lnL of the star of taxa 0, 1, 2 through the C ABI alone -> the bits of the lnL"""
    lib = pkg.libiqhip()
    t = host_tree(pkg, c)
    tip, su = np.ascontiguousarray(t.tip_partial_lh()), t.state_unknown
    t.close()
    m = c["model"]
    a = [np.ascontiguousarray(x, dtype=np.float64) for x in (m.eval, m.evec, m.inv_evec, m.rates, m.props)]
    assert lib.iqhip_set_model(e, *[x.ctypes.data_as(DP) for x in a], su, tip.ctypes.data_as(DP)) == 0, lib.iqhip_last_error()
    states, invar = np.ascontiguousarray(c["states"]), np.zeros(c["nptn"])
    assert lib.iqhip_set_alignment(e, states.ctypes.data_as(C.POINTER(C.c_uint8)), c["freq"].ctypes.data_as(DP),
                                   invar.ctypes.data_as(DP)) == 0, lib.iqhip_last_error()
    ops = (pkg.NodeOp * 1)(pkg.NodeOp(1, 0, 0, 0, 1, 0.1, 0.2, 0, 0))
    lnl = C.c_double()
    assert lib.iqhip_traverse_lnl(e, ops, 1, pkg.leaf_end(2), pkg.key_end(1), 0.15, None, C.byref(lnl)) == 0, lib.iqhip_last_error()
    assert np.isfinite(lnl.value) and lnl.value < 0.0
    return np.float64(lnl.value).tobytes()


@pytest.mark.parametrize("sharded", [False, True])
def test_engine_creation_with_failing_allocations(pkg, synth, sharded):
    lib = pkg.libiqhip()
    c = case(synth, 4, 4, 200, 5)

    def create():
        e = C.c_void_p()
        if sharded:
            rc = lib.iqhip_create_sharded(C.byref(e), (C.c_int * 2)(0, 0), 2, pkg.REDUCE_HOST, 4, 4, c["nptn"], c["ntaxa"])
        else:
            rc = lib.iqhip_create(C.byref(e), 0, 4, 4, c["nptn"], c["ntaxa"])
        return rc, e

    start = reading(pkg)
    rc, plain = create()
    assert rc == 0, lib.iqhip_last_error()
    want = raw_lnl(pkg, plain, c)
    lib.iqhip_destroy(plain)
    assert pkg.debug_memory() == start
    e, nfailed = create_with_failures(pkg, create)
    try:
        assert nfailed >= (2 if sharded else 1)   # (a sharded engine is two engines: more allocations to fail)
        assert raw_lnl(pkg, e, c) == want
    finally:
        lib.iqhip_destroy(e)
    assert pkg.debug_memory() == start


def test_partition_creation_with_failing_allocations(pkg, synth):
    lib = pkg.libiqhip()
    start = reading(pkg)
    trees = two_members(pkg, synth)
    members_only = pkg.debug_memory()

    def create():
        g = C.c_void_p()
        handles = (C.c_void_p * 2)(*[t.engine for t in trees])
        return lib.iqhip_partition_create(C.byref(g), handles, 2), g

    def lnl_bits(g):
        out = np.zeros(2)
        assert lib.iqhip_partition_lnl_from_theta(g, 0.07, out.ctypes.data_as(DP)) == 0, lib.iqhip_last_error()
        assert np.isfinite(out).all()
        return out.tobytes()

    rc, g0 = create()
    assert rc == 0, lib.iqhip_last_error()
    want = lnl_bits(g0)
    lib.iqhip_partition_destroy(g0)
    assert pkg.debug_memory() == members_only
    g, nfailed = create_with_failures(pkg, create)
    try:
        assert nfailed >= 1
        assert lnl_bits(g) == want
    finally:
        lib.iqhip_partition_destroy(g)
    assert pkg.debug_memory() == members_only
    for t in trees:
        t.close()
    assert pkg.debug_memory() == start


# ---- growth with the allocation failing --------------------------------------------------------------------------------
def test_ptnlh_reserve_keeps_the_store_when_it_cannot_grow(pkg, synth):
    start = reading(pkg)
    c = case(synth, 4, 4, 100, 5)
    t = attached(pkg, c)
    rows = np.random.default_rng(9).uniform(-12.0, -1.0, (2, c["nptn"]))
    t.ptnlh_reserve(2)
    for r in range(2):
        t.ptnlh_upload(r, rows[r])
    before = pkg.debug_memory()
    pkg.debug_fail_alloc(1)
    try:
        with pytest.raises(pkg.HostError):
            t.ptnlh_reserve(4)
    finally:
        pkg.debug_fail_alloc(0)
    assert pkg.debug_memory() == before
    for r in range(2):
        assert t.ptnlh_fetch(r).tobytes() == rows[r].tobytes()
    t.ptnlh_reserve(4)
    for r in range(2):
        assert t.ptnlh_fetch(r).tobytes() == rows[r].tobytes()
    assert not t.ptnlh_fetch(2).any() and not t.ptnlh_fetch(3).any()   # new rows are zero-filled
    t.close()
    assert pkg.debug_memory() == start


def test_reserve_reports_a_failed_allocation(pkg, synth):
    lib = pkg.libiqhip()
    start = reading(pkg)
    c = case(synth, 4, 4, 100, 5)
    t = attached(pkg, c)
    want = t.compute_likelihood()
    for k in (1, 2):   # a slab is a vector and its scale counters: either allocation may be the one that fails
        before = pkg.debug_memory()
        pkg.debug_fail_alloc(k)
        try:
            assert lib.iqhip_reserve(t.engine, 64) == ERR_NOMEM
        finally:
            pkg.debug_fail_alloc(0)
        assert pkg.debug_memory() == before
    t.clear_all_partial_lh()
    assert t.compute_likelihood() == want
    assert lib.iqhip_reserve(t.engine, 64) == 0, lib.iqhip_last_error()
    t.clear_all_partial_lh()
    assert t.compute_likelihood() == want
    t.close()
    assert pkg.debug_memory() == start


def test_codon_engines_on_two_devices_agree(pkg, synth):
    """the dynamic-LDS opt-in of the 64-state kernels belongs to the device: the second device's engine must get it too"""
    if pkg.libiqhip().iqhip_device_count() < 2:
        pytest.skip("needs two devices")
    c = case(synth, 64, 1, 100, 5)
    lnl = []
    for device in (0, 1):
        t = host_tree(pkg, c)
        t.attach_engine(device)
        lnl.append(np.float64(t.compute_likelihood()).tobytes())
        t.close()
    assert lnl[0] == lnl[1]
