"""CPU side of the partition-UFBoot tests: the rows of a super tree and of its nni5 neighbourhood from the oracle alone, and
the screening of the margin test's seed on them.

  oracle_nni5_rows    the current tree and, in the order PhyloTree::evaluateNNIs5Batch lists them, its 2 (n - 3) NNI
                      neighbours, each with the five branches re-optimised jointly over the members in the reference's
                      order (the two at node1, the central one, the two at node2; the second swap of a branch starts from
                      the lengths the first left) by partition_ref.joint_minimize_newton -> (logl [M], per member rows
                      [M][nptn]): log|lh + invar| with the scaling events of both branch ends put back
  member_samples      per member NSAMPLES multinomial resamples of its own sites (resampling within partitions)
  margin_scheme       tests/test_ufboot_gpu.py::test_real_rows_against_the_numpy_product on R = sum_p L_p W_p^T
"""
import copy

import numpy as np

import partition_ref as pr
import ufboot_ref as ref

MARGIN_SEED = 41      # screened by tests/test_partition_ufboot_host.py: no replicate is left out on the oracle's rows
TIE_SEED = 9


def _row(oracle, ot):
    lnl, (a, b) = ot.likelihood()
    _, plh = ot.branch_lnl(a, b)
    _, sc_b, _ = ot.partial(a, b)                      # a is the leaf end
    return lnl, oracle.pattern_lh_scaled(plh, None, sc_b)


def _swap(ot, n1, n2, a, x):
    """the subtree a at n1 and the subtree x at n2 change places, each in the other's neighbour slot, lengths travelling"""
    la, lx = ot.length(n1, a), ot.length(n2, x)
    for e in ot.adj[n1]:
        if e[0] == a:
            e[0], e[1] = x, lx
    for e in ot.adj[n2]:
        if e[0] == x:
            e[0], e[1] = a, la
    for e in ot.adj[a]:
        if e[0] == n1:
            e[0] = n2
    for e in ot.adj[x]:
        if e[0] == n2:
            e[0] = n1
    ot.clear()


def oracle_nni5_rows(oracle, nwk, members, rates, lo=1e-6, hi=100.0, max_steps=10):
    ots = [pr.oracle_member(oracle, nwk, d) for d in members]
    sup = pr.oracle_member(oracle, nwk, members[0], scale=1.0)   # the super tree's lengths
    nnodes = len(sup.adj)
    logl, rows = [], [[] for _ in members]

    def record():
        total = 0.0
        for p, ot in enumerate(ots):
            v, r = _row(oracle, ot)
            total += v
            rows[p].append(r)
        logl.append(total)

    def solve(a, b):
        optx, _, _, status = pr.joint_minimize_newton(ots, rates, a, b, lo, sup.length(a, b), hi, lo, max_steps)
        assert status == "ok" and optx <= 0.95 * hi, (a, b, optx, status)
        sup.set_length(a, b, optx)
        for ot, r in zip(ots, rates):
            ot.set_length(a, b, r * optx)

    record()
    inner = [(a, b) for a in range(nnodes) for b, _ in sup.adj[a] if a < b and not sup.is_leaf(a) and not sup.is_leaf(b)]
    for n1, n2 in inner:
        saved = [copy.deepcopy(t.adj) for t in ots + [sup]]
        first = [v for v, _ in sup.adj[n1] if v != n2][0]
        for x in [v for v, _ in sup.adj[n2] if v != n1]:
            for t in ots + [sup]:
                _swap(t, n1, n2, first, x)
            for y in [v for v, _ in sup.adj[n1] if v != n2]:
                solve(n1, y)
            solve(n1, n2)
            for y in [v for v, _ in sup.adj[n2] if v != n1]:
                solve(n2, y)
            record()
            for t in ots + [sup]:
                _swap(t, n1, n2, x, first)
        for t, adj in zip(ots + [sup], saved):
            t.adj = adj
            t.clear()
    return np.array(logl), [np.array(r) for r in rows]


def member_samples(members, nsamples, seed):
    rng = np.random.default_rng(seed)
    out = []
    for d in members:
        f = np.asarray(d["freq"], dtype=np.float64)
        out.append(rng.multinomial(int(f.sum()), f / f.sum(), size=nsamples).astype(np.float32))
    return out


def margin_scheme(Ls, Ws, ids, logl, rand, ns):
    """-> (state of the numpy run, counted [ns], margins [ns], bound [ns])"""
    W64 = [np.asarray(W[:ns], dtype=np.float64) for W in Ws]
    R = sum(L @ W.T for L, W in zip(Ls, W64))
    bound = (1e-13 * sum(np.abs(L) @ np.abs(W).T for L, W in zip(Ls, W64))).max(axis=0)
    margins = np.full(ns, np.inf)
    want = ref.ufboot_start(ns)
    ref.ufboot_rule(want, R, ids, logl, rand, margins=margins)
    return want, margins > bound, margins, bound
