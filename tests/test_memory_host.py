"""CPU: the library's memory accounting on planning-only engines (iqhip_debug_memory, iqhip_debug_fail_alloc).

A planning-only engine makes no HIP call: its device buffers are fake addresses, which count as nothing, and the staging
copy of its plan (h_ops) is plain host memory from the same allocate / free pair every real buffer goes through, which
counts as host bytes.  So without a GPU these tests pin that the staging grows through the owner, that a failed growth is
reported and leaves the engine usable, and that nothing outlives the engine.

The counters are process-wide.  Every reading is compared with the one at the start of the test; in a process with no other
live engine, such as the run of this file alone, that reading is (0, 0)."""
import ctypes as C

import pytest

from test_plan_check import planner

NTAXA, NPTN = 5, 200
SHAPES = [(4, 4), (20, 4), (64, 1)]   # nstates, ncat


def chain(pkg, nops):
    """a caterpillar of nops node updates over the five taxa: op k joins the vector of op k - 1 with a leaf"""
    ops = (pkg.NodeOp * nops)()
    for k in range(nops):
        if k == 0:
            ops[k] = pkg.NodeOp(100, 0, 0, 0, 1, 0.1, 0.2, 0, 0)
        else:
            ops[k] = pkg.NodeOp(100 + k, 100 + k - 1, 0, -1, (k + 1) % NTAXA, 0.1, 0.2, 0, 0)
    return ops


FEW, MANY = 3, 100   # the staging starts at max(64, 2 * descriptors) descriptors (plan.hip ensure_plan_capacity): 100 ops outgrow it


@pytest.mark.parametrize("nstates,ncat", SHAPES)
def test_plan_staging_is_counted_and_freed(pkg, nstates, ncat):
    start = pkg.debug_memory()
    lib, e = planner(pkg, nstates, ncat, NPTN, NTAXA)
    try:
        assert pkg.debug_memory() == start                       # fake addresses count as nothing
        assert lib.iqhip_debug_plan(e, chain(pkg, FEW), FEW) == 0, lib.iqhip_last_error()
        small = pkg.debug_memory()
        assert small[0] == start[0] and small[1] > start[1]      # host staging, no device memory
        assert lib.iqhip_debug_plan(e, chain(pkg, MANY), MANY) == 0, lib.iqhip_last_error()
        grown = pkg.debug_memory()
        assert grown[0] == start[0] and grown[1] > small[1]      # the staging was replaced by a larger one
        assert lib.iqhip_debug_plan(e, chain(pkg, FEW), FEW) == 0, lib.iqhip_last_error()
        assert pkg.debug_memory() == grown                       # ... and is kept
    finally:
        lib.iqhip_destroy(e)
    assert pkg.debug_memory() == start


@pytest.mark.parametrize("nstates,ncat", SHAPES)
def test_failed_growth_is_reported_and_recovered(pkg, nstates, ncat):
    """iqhip_debug_fail_alloc(k) for k = 1, 2, .. until the growth succeeds, a fresh planner each time"""
    start = pkg.debug_memory()
    failed = 0
    for k in range(1, 9):
        lib, e = planner(pkg, nstates, ncat, NPTN, NTAXA)
        try:
            assert lib.iqhip_debug_plan(e, chain(pkg, FEW), FEW) == 0, lib.iqhip_last_error()
            pkg.debug_fail_alloc(k)
            rc = lib.iqhip_debug_plan(e, chain(pkg, MANY), MANY)
            pkg.debug_fail_alloc(0)
            if rc != 0:
                failed += 1
                assert lib.iqhip_debug_plan(e, chain(pkg, MANY), MANY) == 0, lib.iqhip_last_error()   # a later call succeeds
        finally:
            pkg.debug_fail_alloc(0)
            lib.iqhip_destroy(e)
        assert pkg.debug_memory() == start, k
        if rc == 0:
            break
    else:
        pytest.fail("the growth still failed at the 8th allocation")
    assert failed >= 1   # (the first allocation of the growth is the staging itself)


def test_fake_addresses_stay_distinct_and_aligned(pkg):
    """what tests/test_plan_check.py relies on, stated on the owners: plans with more and more vectors validate (check_plan
    refuses a descriptor whose pointers are not live allocations of the right kind) while no device byte is counted"""
    start = pkg.debug_memory()
    lib, e = planner(pkg, 4, 4, NPTN, NTAXA)
    try:
        for nops in (1, 7, 64, 65, 300):
            assert lib.iqhip_debug_plan(e, chain(pkg, nops), nops) == 0, lib.iqhip_last_error()
            assert pkg.debug_memory()[0] == start[0]
    finally:
        lib.iqhip_destroy(e)
    assert pkg.debug_memory() == start
