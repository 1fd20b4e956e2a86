"""Joint pairwise distances of a partition group (include/iqhip.h "Joint pairwise distances of a partition group"), the
parts that need no device: the new symbols, the properties of the restatement in tests/partition_dist_ref.py (its joint
derivatives against central differences of its joint function, the member-0 rule of the JC start), the cases
tests/test_partition_dist_gpu.py runs on the device, and the refusal of planning-only engines."""
import collections
import ctypes as C
import os
import re

import numpy as np
import pytest

import partition_dist_ref as R
from conftest import ROOT
from test_pair_dist_host import MAX_GENETIC_DIST, MAX_STEPS, X1, X2, XACC, restate_jc

IQHIP_ERR_INVALID = 2
NEW_SYMBOLS = ("iqhip_partition_pair_distances", "iqhip_debug_partition_pair_timing")


def test_symbols(pkg):
    src = open(os.path.join(ROOT, "include", "iqhip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = pkg.libiqhip()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in pkg.IQHIP_SYMBOLS and hasattr(lib, name), name
    host = pkg.libiqhost()
    for name in ("iqhost_super_compute_dist", "iqhost_super_compute_bionj", "iqhost_super_fix_negative_branch"):
        assert hasattr(host, name), name
    for name in ("compute_dist", "compute_bionj", "fix_negative_branch", "partition_pair_timing"):
        assert hasattr(pkg.PhyloSuperTree, name), name
    assert hasattr(pkg.PartitionGroup, "pair_distances")


@pytest.mark.parametrize("rates", ["ones", "unequal"])
@pytest.mark.parametrize("group", ["G1", "G2"])
def test_joint_derivatives_agree_with_central_differences(synth, group, rates):
    members, _ = R.part_case(synth, group, 5)
    r = R.case_rates(group, rates)
    counts = [c[0] for c in R.member_counts(members, [(0, 3)])]   # (taxon 3: random states, data in every member)
    models = [m["model"] for m in members]
    assert all(c.sum() > 0 for c in counts)
    for t in (0.05, 0.3, 1.5):
        df, ddf = R.joint_func_derv(counts, models, r, t)
        # the argument of test_pair_dist_host.test_derivatives_agree_with_central_differences: |D(h/2) - g'| <= |D(h) -
        # D(h/2)| (truncation, 3x headroom) + 8 eps |g| / (h/2) (rounding of the two evaluations), h = 1e-3 t
        h = 1e-3 * t
        eps = 2.0 ** -52
        for g, want in ((lambda x: R.joint_function(counts, models, r, x), df),
                        (lambda x: R.joint_func_derv(counts, models, r, x)[0], ddf)):
            D = lambda s: (g(t + s) - g(t - s)) / (2.0 * s)   # noqa: E731
            d1, d2 = D(h), D(h / 2)
            tol = abs(d1 - d2) + 8 * eps * abs(g(t)) / (h / 2)
            assert abs(d2 - want) <= tol, (group, rates, t, d2, want, tol)
            assert tol <= 1e-4 * abs(want)   # (the check is not vacuous)


def test_joint_derivatives_of_one_member_at_rate_one_are_the_members(synth):
    members, _ = R.part_case(synth, "G1", 5)
    counts = R.member_counts(members, [(0, 1)])[0][0]
    from test_pair_dist_host import restate_func_derv
    for t in (1e-6, 0.2, 9.0):
        assert R.joint_func_derv([counts], [members[0]["model"]], [1.0], t) == restate_func_derv(counts, members[0]["model"], t)


def test_jc_start_reads_the_state_count_of_member_zero():
    """a DNA and a protein member swapped: the same pooled sums, z = 4 / 3 against z = 20 / 19"""
    rng = np.random.default_rng(3)
    dna = np.diag(rng.integers(5, 20, size=4).astype(float)) + rng.integers(0, 3, size=(4, 4))
    prot = np.diag(rng.integers(5, 20, size=20).astype(float)) + rng.integers(0, 2, size=(20, 20))
    total, same = dna.sum() + prot.sum(), np.trace(dna) + np.trace(prot)
    p = (total - same) / total
    for order, n0 in (((dna, prot), 4), ((prot, dna), 20)):
        z = n0 / (n0 - 1.0)
        assert R.restate_super_jc(list(order)) == -np.log(1.0 - z * p) / z
    assert R.restate_super_jc([dna, prot]) != R.restate_super_jc([prot, dna])
    assert R.restate_super_jc([dna]) == restate_jc(dna)                       # one member: Alignment::computeJCDist
    assert R.restate_super_jc([np.zeros((4, 4)), np.zeros((20, 20))]) == MAX_GENETIC_DIST
    far = np.ones((4, 4)) - np.eye(4)                                         # no identical column: x <= 0 for z = 4 / 3 ...
    assert R.restate_super_jc([far, np.zeros((20, 20))]) == MAX_GENETIC_DIST
    assert R.restate_super_jc([np.zeros((20, 20)), far]) == MAX_GENETIC_DIST  # ... and for z = 20 / 19


def test_a_start_of_nine_is_returned_without_a_solve(synth):
    members, _ = R.part_case(synth, "G1", 5)
    counts = [c[0] for c in R.member_counts(members, [(0, 1)])]
    models = [m["model"] for m in members]
    assert R.restate_joint_solve(counts, models, [1.0, 1.0, 1.0], init=MAX_GENETIC_DIST) == (MAX_GENETIC_DIST, 0.0, [])
    x, d2l, pts = R.restate_joint_solve(counts, models, [1.0, 1.0, 1.0], init=8.5)
    assert x < 8.5 and len(pts) >= 2


@pytest.mark.parametrize("group,ntaxa,rates", R.CASES)
def test_cases_hold_what_the_device_tests_need(synth, group, ntaxa, rates):
    """every case on the CPU: no pair trips the guard, and every required situation occurs"""
    members, init = R.part_case(synth, group, ntaxa)
    assert [m["pat"].shape[1] for m in members] == list(R.NPTN[ntaxa][:len(members)])
    stats = collections.Counter()
    dist, d2l, nst = R.restate_joint_matrix(members, R.case_rates(group, rates), init, stats)
    R.assert_part_case_stats(stats, ntaxa)
    T = ntaxa
    assert dist[0, T - 3] == X1                                                   # identical in every member
    assert (dist[T - 1, :T - 1] == MAX_GENETIC_DIST).all() and not nst[T - 1].any() and not d2l[T - 1].any()
    assert dist[1, T - 3] == MAX_GENETIC_DIST and nst[1, T - 3] == 0              # init of exactly 9
    assert nst[0, T - 2] >= 2 and nst[T - 4, T - 2] >= 2                          # init 8.5 is solved from


def test_weighted_mean_counts_a_codon_member_three_times_next_to_others():
    assert R.restate_weighted_mean([0.1, 0.4], [100.0, 300.0], [0, 1]) == (0.1 * 100.0 + 0.4 * 300.0) / 400.0
    assert R.restate_weighted_mean([0.1, 0.4], [100.0, 300.0], [2, 2]) == (0.1 * 100.0 + 0.4 * 300.0) / 400.0
    assert R.restate_weighted_mean([0.1, 0.4], [100.0, 300.0], [2, 0]) == (0.1 * 100.0 + 0.4 * 300.0) / 600.0


def test_wrong_shapes_raise_before_the_c_call(pkg):
    """the shape checks of PhyloSuperTree.compute_dist / compute_bionj are exceptions, not asserts (they guard a C call
    that reads ntaxa * ntaxa doubles); tried on an object that never reaches the library"""
    class Stub(pkg.PhyloSuperTree):
        num_leaves = 5

        def __init__(self):
            self.h = None

    st = Stub()
    with pytest.raises(ValueError):
        st.compute_dist(init=np.zeros((4, 4)))
    with pytest.raises(ValueError):
        st.compute_bionj(dist=np.zeros((5, 4)))
    with pytest.raises(ValueError):
        st.compute_bionj(dist=np.zeros((5, 5)), var=np.zeros((3, 3)))


def test_planning_only_engines_are_refused(pkg):
    """What is covered: iqhip_partition_create refuses planning-only engines, so the new entry point can never see such a
    member, and a null group is invalid for both new calls.  The entry point itself is not reached with a planner."""
    lib = pkg.libiqhip()
    es = [C.c_void_p(), C.c_void_p()]
    for e in es:
        assert lib.iqhip_debug_create_planner(C.byref(e), 4, 4, 1000, 5, 256, 18, 1) == 0
    g = C.c_void_p()
    arr = (C.c_void_p * 2)(*[e.value for e in es])
    assert lib.iqhip_partition_create(C.byref(g), arr, 2) == IQHIP_ERR_INVALID
    assert b"planning-only" in lib.iqhip_last_error() and not g.value
    dist = np.zeros(25)
    dp = C.POINTER(C.c_double)
    assert lib.iqhip_partition_pair_distances(None, None, X1, X2, XACC, MAX_STEPS, dist.ctypes.data_as(dp), None, None) == IQHIP_ERR_INVALID
    assert b"null group" in lib.iqhip_last_error()
    a, b = C.c_double(), C.c_double()
    assert lib.iqhip_debug_partition_pair_timing(None, C.byref(a), C.byref(b)) == IQHIP_ERR_INVALID
    for e in es:
        lib.iqhip_destroy(e)
