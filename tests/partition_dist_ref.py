"""Restatement of the joint pairwise distances of an edge-linked partition group (include/iqhip.h "Joint pairwise
distances of a partition group"; PhyloSuperTreePlen::computeDist over SuperAlignmentPairwisePlen), and the cases of
tests/test_partition_dist_host.py and tests/test_partition_dist_gpu.py.

Built from restate_counts, restate_func_derv, restate_function and restate_jc of tests/test_pair_dist_host.py and from the
oracle's own minimize_newton, so that neither a member's function nor the update rule is restated again:

  joint_func_derv       df = sum_p r_p df_p(r_p x), ddf = sum_p r_p^2 ddf_p(r_p x), in member order
  restate_super_jc      SuperAlignment::computeDist (superalignment.cpp:384-421): the members' counts pooled, z from the
                        state count of MEMBER 0
  restate_joint_solve   the start (init, or restate_super_jc), the return at 9 without a solve, minimize_newton, and the
                        walk guard of restate_solve: an input whose stopping tests are decided within 1e-6 xacc of their
                        threshold is rejected ("change the seed")"""
import collections
import math
import os
import sys

import numpy as np

from conftest import ROOT
from test_pair_dist_host import (MAX_GENETIC_DIST, MAX_STEPS, X1, X2, XACC, all_pairs, rate_model, restate_counts,
                                 restate_func_derv, restate_function)

sys.path.insert(0, os.path.join(ROOT, "oracle"))
import oracle_driver  # noqa: E402


# ------------------------------------------------------------------------------------------
# restatements
# ------------------------------------------------------------------------------------------
def joint_func_derv(counts, models, rates, x):
    """(df, ddf) of the pair over all members; counts: one [n_p, n_p] table per member"""
    df = ddf = None
    for p, (c, m, r) in enumerate(zip(counts, models, rates)):
        a, b = restate_func_derv(c, m, x * r)
        rdf, rddf = r * a, (r * r) * b
        df = rdf if p == 0 else df + rdf
        ddf = rddf if p == 0 else ddf + rddf
    return df, ddf


def joint_function(counts, models, rates, x):
    """the negative log-likelihood whose derivatives joint_func_derv returns"""
    return sum(restate_function(c, m, x * r) for c, m, r in zip(counts, models, rates))


def restate_super_jc(counts):
    total = sum(float(c.sum()) for c in counts)
    same = sum(float(np.trace(c)) for c in counts)
    if total == 0:
        return MAX_GENETIC_DIST
    n0 = counts[0].shape[0]
    z = n0 / (n0 - 1.0)
    x = 1.0 - z * ((total - same) / total)
    return MAX_GENETIC_DIST if x <= 0 else -np.log(x) / z


class JointPairFunction:
    """stands where OracleTree.minimize_newton expects a tree: derv() returns the likelihood's derivatives (-df, -ddf)"""

    def __init__(self, counts, models, rates):
        self.counts, self.models, self.rates = counts, models, rates

    def derv(self, a, b, length=None, theta=None):
        df, ddf = joint_func_derv(self.counts, self.models, self.rates, length)
        return -df, -ddf


def restate_joint_solve(counts, models, rates, init=0.0, x1=X1, x2=X2, xacc=XACC, max_steps=MAX_STEPS, stats=None, who=None):
    """-> (optx, d2l, evaluated points); a start of 9 -> (9, 0, [])"""
    jc = restate_super_jc(counts)
    guess = jc if init == 0.0 else init
    data_in = sum(int(c.sum() > 0) for c in counts)
    if stats is not None:
        stats["solves"] += 1
        stats["init"] += int(init != 0.0 and init != MAX_GENETIC_DIST)
        stats["init_9"] += int(init == MAX_GENETIC_DIST)
        stats["unknown_everywhere"] += int(data_in == 0 and init == 0.0)
    if guess == MAX_GENETIC_DIST:
        return MAX_GENETIC_DIST, 0.0, []
    fn = JointPairFunction(counts, models, rates)
    optx, d2l, pts, status = oracle_driver.OracleTree.minimize_newton(fn, 0, 1, x1, guess, x2, xacc, max_steps, theta=0)
    assert status == "ok", (who, status)
    if stats is not None:
        xl, xh = x1, x2
        for k, x in enumerate(pts):
            f, df = joint_func_derv(counts, models, rates, x)
            if f < 0.0:
                xl = x
            else:
                xh = x
            bisect = df <= 0.0 or ((x - xh) * df - f) * ((x - xl) * df - f) >= 0.0
            dx = 0.5 * (xh - xl) if bisect else f / df
            if k + 1 < len(pts):
                assert pts[k + 1] == (xl + dx if bisect else x - dx), (who, k, pts)
                stats["bisection"] += int(bisect)
            assert abs(abs(dx) - xacc) > 1e-6 * xacc and abs(abs(f) - xacc) > 1e-6 * xacc, ("change the seed", who, x, dx, f)
        stats["identical"] += int(optx == x1)
        stats["one_member"] += int(data_in == 1 and len(counts) > 1)
        stats["random_8.5"] += int(init == 8.5 and jc == MAX_GENETIC_DIST)
        stats["interior"] += int(x1 < optx < 0.5 * x2)
    return optx, d2l, pts


def member_counts(members, pairs):
    """per member the counts of all listed pairs [npairs, n, n]"""
    return [restate_counts(m["pat"], m["freq"], m["n"], pairs) for m in members]


def restate_joint_matrix(members, rates, init=None, stats=None, x1=X1, x2=X2, xacc=XACC, max_steps=MAX_STEPS):
    """-> dist, d2l, nsteps [ntaxa, ntaxa] of the restatement"""
    T = members[0]["pat"].shape[0]
    dist, d2l, nst = np.zeros((T, T)), np.zeros((T, T)), np.zeros((T, T), dtype=np.int32)
    pairs = all_pairs(T)
    cnt = member_counts(members, pairs)
    models = [m["model"] for m in members]
    for k, (i, j) in enumerate(pairs):
        g = 0.0 if init is None else init[i, j]
        x, d, pts = restate_joint_solve([c[k] for c in cnt], models, rates, g, x1, x2, xacc, max_steps, stats=stats, who=(i, j))
        dist[i, j] = dist[j, i] = x
        d2l[i, j] = d2l[j, i] = d
        nst[i, j] = nst[j, i] = len(pts)
    return dist, d2l, nst


# ------------------------------------------------------------------------------------------
# the cases
# ------------------------------------------------------------------------------------------
GROUPS = {"G1": ("gtr_g4", "dna_1", "prot_g4"), "G2": ("codon_1", "dna_12")}
NPTN = {5: (65, 1, 64), 17: (1000, 63, 200)}            # member pattern counts, cut to the group's size
RATES = {"ones": (1.0, 1.0, 1.0), "unequal": (0.4, 1.0, 2.5)}
CASES = [(g, T, r) for g in ("G1", "G2") for T in (5, 17) for r in ("ones", "unequal")]
# chosen on the CPU so that no pair of a case trips restate_joint_solve's guard and every required situation occurs
SEEDS = {(g, T): 11 for g in GROUPS for T in NPTN}
SEEDS[("G2", 17)] = 19   # (seeds 11 .. 18: the pair only the codon member has data for starts below 9)


def member_data(synth, kind, ntaxa, nptn, seed, nwk):
    """one member: states[ntaxa, nptn] simulated on the common tree (codon members: the synthetic GY94 workload), 3 % of
    the characters ambiguous or unknown, frequencies 1 .. 3 -> dict(n, seq_type, pat, freq, model, unknown, sense)"""
    rng = np.random.default_rng(7000 + 13 * seed + nptn)
    if kind == "codon_1":
        _, states, _, model = synth.codon_gy94_workload(ntaxa, nptn, seed)
        n, seq_type, unknown = 64, 2, 64
        states = states.copy()
        sense = np.unique(states)
        states[rng.random(states.shape) < 0.03] = unknown
    else:
        model, n, seq_type = rate_model(synth, kind)
        unknown = 18 if n == 4 else 23
        states = synth.simulate_alignment(nwk, model, nptn, seed + 1 + nptn)
        sense = np.arange(n)
        amb = rng.random(states.shape) < 0.03
        states[amb] = rng.integers(n, unknown + 1, size=int(amb.sum()))
    freq = rng.integers(1, 4, size=nptn).astype(np.float64)
    return dict(n=n, nstates=n, seq_type=seq_type, pat=np.ascontiguousarray(states, dtype=np.uint8), freq=freq, model=model,
                unknown=unknown, sense=sense, rng=rng)


def part_case(synth, group, ntaxa):
    """-> (members, init[ntaxa, ntaxa]).  In EVERY member the last taxon shows only unknown states, the one before it
    independent random states, the one before that is a copy of taxon 0; taxon ntaxa - 4 has data in member 0 only.  init
    asks for a far-off start of pair (0, 1), for exactly 9 on pair (1, ntaxa - 3) and for 8.5 on the pairs (0, ntaxa - 2) and
    (ntaxa - 4, ntaxa - 2) with the random taxon: the JC start of at least one of them would be 9 (with a codon member 0,
    z = 64 / 63 leaves that to the pair only member 0 has data for)."""
    seed = SEEDS[(group, ntaxa)]
    kinds = GROUPS[group]
    nwk = synth.random_tree_newick(ntaxa, seed, 0.02, 0.4)
    members = []
    for p, kind in enumerate(kinds):
        m = member_data(synth, kind, ntaxa, NPTN[ntaxa][p], seed, nwk)
        st, rng = m["pat"], m.pop("rng")
        st[ntaxa - 1] = m["unknown"]
        st[ntaxa - 2] = rng.choice(m["sense"], size=st.shape[1])
        st[ntaxa - 3] = st[0]
        if p > 0:
            st[ntaxa - 4] = m["unknown"]
        members.append(m)
    init = np.zeros((ntaxa, ntaxa))
    for (i, j), v in (((0, 1), 3.0), ((1, ntaxa - 3), MAX_GENETIC_DIST), ((0, ntaxa - 2), 8.5), ((ntaxa - 4, ntaxa - 2), 8.5)):
        init[i, j] = init[j, i] = v
    return members, init


def case_rates(group, rates):
    return np.array(RATES[rates][:len(GROUPS[group])])


def assert_part_case_stats(stats, ntaxa):
    """what every case must contain (the module docstring of tests/test_partition_dist_gpu.py)"""
    assert stats["solves"] == ntaxa * (ntaxa - 1) // 2
    for what in ("identical", "unknown_everywhere", "one_member", "bisection", "init", "init_9", "random_8.5", "interior"):
        assert stats[what] >= 1, (what, dict(stats))


_solved = {}


def solved_part_case(synth, group, ntaxa, rates):
    """the case and its restated solution, computed once -> (members, init, rates, (dist, d2l, nsteps))"""
    key = (group, ntaxa, rates)
    if key not in _solved:
        members, init = part_case(synth, group, ntaxa)
        r = case_rates(group, rates)
        stats = collections.Counter()
        ref = restate_joint_matrix(members, r, init, stats)
        assert_part_case_stats(stats, ntaxa)
        _solved[key] = (members, init, r, ref)
    return _solved[key]


# ------------------------------------------------------------------------------------------
# PhyloSuperTreePlen::fixNegativeBranch
# ------------------------------------------------------------------------------------------
def restate_fix_length(subst, nsite, nstates, min_branch_length=1e-6):
    """the member rule (phylotree.cpp:2664-2690): the branch's substitution count over the sites, Jukes-Cantor corrected
    (math.log: the C library's, as on the host)"""
    bl = subst / nsite if subst > 0 else 1.0 / nsite
    z = nstates / (nstates - 1)
    x = 1.0 - z * bl
    if x > 0:
        bl = -math.log(x) / z
    return max(bl, min_branch_length)


def restate_weighted_mean(member_lengths, nsites, seq_types):
    """PhyloSuperTree::computeBranchLengths (phylosupertree.cpp:1353-1398) for a branch that occurs once in every member:
    sum_p len_p nsite_p / sum_p nsite_p in member order; with codon AND other members a codon member counts 3 nsite_p in
    the denominator (rescale_codon_brlen)"""
    rescale = any(s == 2 for s in seq_types) and any(s != 2 for s in seq_types)
    length, occ = 0.0, 0.0
    for l, ns, s in zip(member_lengths, nsites, seq_types):
        length += l * ns
        occ += ns * 3 if (s == 2 and rescale) else ns
    return length / occ if occ != 0.0 else length
