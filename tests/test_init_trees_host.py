"""CPU: the addition orders of the parsimony starting trees (iqsearch::parsimonyOrders, search_host.h) against a Python
restatement of the stated construction, and the conditions on the inputs that the GPU search tests rely on, checked with
fitch_ref alone."""
import numpy as np
import pytest

import init_trees_case as case
import init_trees_ref as iref


@pytest.mark.parametrize("seed,k,ntaxa", [(0, 8, 10), (7, 3, 4), (123456789, 5, 33), (2**63 + 5, 2, 1), (1, 0, 9), (1, 4, 0)])
def test_orders_equal_the_restatement(pkg, seed, k, ntaxa):
    got = pkg.parsimony_orders(seed, k, ntaxa)
    assert got == iref.parsimony_orders(pkg, seed, k, ntaxa)
    assert len(got) == k and all(sorted(o) == list(range(ntaxa)) for o in got)      # every order is a permutation
    assert got == pkg.parsimony_orders(seed, k, ntaxa)                              # deterministic
    # order j depends on j alone: a longer list starts with the shorter one
    assert pkg.parsimony_orders(seed, k + 2, ntaxa)[:k] == got


def test_orders_follow_the_seed_and_leave_the_search_stream_alone(pkg):
    a, b = pkg.parsimony_orders(1, 8, 10), pkg.parsimony_orders(2, 8, 10)
    assert a != b and len({tuple(o) for o in a}) > 1
    # the draws are those of iteration 0 of the search stream: the last swap of order j is draw j * ntaxa + 1
    for j, o in enumerate(a):
        start = list(range(10))
        for i in range(9, 0, -1):
            r = pkg.search_rand_int(pkg.search_rand(1, 0, j * 10 + i), i + 1)
            start[i], start[r] = start[r], start[i]
        assert o == start
    # iterations >= 1 are the search's own: their values are what they were (splitmix64 keyed by seed, iteration, draw)
    G, M = 0x9E3779B97F4A7C15, (1 << 64) - 1

    def mix(z):
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
        return z ^ (z >> 31)

    for seed, it, draw in [(1, 1, 0), (1, 2, 3), (99, 7, 12)]:
        want = mix((mix((mix((seed + G * (0x5E + 1)) & M) + G * (it + 1)) & M) + G * (draw + 1)) & M)
        assert pkg.search_rand(seed, it, draw) == want


def test_negative_counts_are_refused(pkg):
    with pytest.raises(pkg.HostError):
        pkg.parsimony_orders(1, -1, 5)
    with pytest.raises(pkg.HostError):
        pkg.parsimony_orders(1, 2, -5)


@pytest.mark.parametrize("name", sorted(case.CASES))
def test_conditions_on_the_search_inputs(pkg, name):
    """the orders of the chosen seed give, by the restatement, at least two equal and at least two different topologies:
    the duplicate filter of the search has something to drop and something to keep"""
    ntaxa = case.CASES[name][2]
    orders_of = lambda seed: iref.parsimony_orders(pkg, seed, case.NUM_INIT - 1, ntaxa)
    assert case.first_good_seed(name, orders_of) == case.SEARCH_SEED[name]
    tops = case.restated_topologies(name, orders_of(case.SEARCH_SEED[name]))
    assert case.has_repeats_and_differences(tops)
    # with the eighth order as well (K = 8 orders), the same holds
    tops8 = case.restated_topologies(name, iref.parsimony_orders(pkg, case.SEARCH_SEED[name], case.NUM_INIT, ntaxa))
    assert tops8[:-1] == tops and case.has_repeats_and_differences(tops8)
    true, n, _, pat, freq = case.data(name)
    assert pat.shape[0] == ntaxa and int(np.sum(freq)) == case.CASES[name][3]
