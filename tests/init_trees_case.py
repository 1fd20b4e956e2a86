"""The inputs of the starting-population tests (test_init_trees_host.py checks their conditions without a device,
test_init_trees_gpu.py and test_init_trees_cli_gpu.py run the search on them): an alignment simulated on a random tree with
synth, and the search seed whose parsimony orders give both repeated and different topologies."""
import functools

import numpy as np

import fitch_ref as F

# name -> (nstates, ncat, ntaxa, nsites, data seed)
CASES = {"dna10": (4, 4, 10, 300, 5), "prot8": (20, 4, 8, 200, 6)}
NUM_INIT = 8          # the given tree + 7 parsimony trees
# The first seed of 0, 1, 2, ... for which the RESTATEMENT (fitch_ref.stepwise_addition on parsimony_orders' construction)
# gives at least two equal and at least two different topologies among the parsimony trees of dna10; found by
# first_good_seed below, asserted in test_init_trees_host.py.  The code under test had no say.
SEARCH_SEED = {"dna10": 0, "prot8": 1}


@functools.lru_cache(maxsize=None)
def data(name):
    """-> (true newick, nstates, model, patterns [ntaxa, nptn], frequencies)"""
    import importlib
    from conftest import load_package
    load_package()
    synth = importlib.import_module("iqtree_amd.synth")
    n, ncat, ntaxa, nsites, seed = CASES[name]
    model = synth.gtr_model(alpha=0.9, ncat=ncat) if n == 4 else synth.random_reversible_model(n, seed, alpha=0.9, ncat=ncat)
    true = synth.random_tree_newick(ntaxa, 1000 + seed)
    pat, freq = synth.compress_patterns(synth.simulate_alignment(true, model, nsites, 2000 + seed))
    return true, n, model, pat, freq


def adj_splits(adj, ntaxa):
    """the non-trivial splits of an adjacency dict, each the side without taxon 0"""
    out = set()
    for a, b in F.branches(adj):
        if a < ntaxa or b < ntaxa:
            continue
        side, stack = set(), [(a, b)]
        while stack:
            x, dad = stack.pop()
            if x < ntaxa:
                side.add(x)
            stack.extend((y, x) for y in adj[x] if y != dad)
        out.add(frozenset(side if 0 not in side else set(range(ntaxa)) - side))
    return frozenset(out)


def restated_topologies(name, orders):
    """the stepwise-addition tree of every order by fitch_ref alone -> [(score, split set)]"""
    _, n, _, pat, freq = data(name)
    tips = F.tip_vectors(pat, F.site_patterns(freq, F.is_informative(pat, n)), n)
    out = []
    for order in orders:
        score, adj, _, _ = F.stepwise_addition(tips, list(order))
        out.append((score, adj_splits(adj, pat.shape[0])))
    return out


def has_repeats_and_differences(topologies):
    keys = [t[1] for t in topologies]
    return len(set(keys)) >= 2 and len(set(keys)) < len(keys)


def first_good_seed(name, orders_of, limit=50):
    """orders_of(seed) -> the NUM_INIT - 1 orders of that seed"""
    for seed in range(limit):
        if has_repeats_and_differences(restated_topologies(name, orders_of(seed))):
            return seed
    return None
