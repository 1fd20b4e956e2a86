"""fp64 numpy restatement of BIONJ as include/iqhip.h ("BIONJ") writes it out, the inputs of the BIONJ tests and a
Newick-to-splits helper.  Not a test module.

bionj(dist, var=None, rule="first", sums="numpy") follows the header step for step.  rule="first" is the header's pair
rule (the first pair in scan order within 1e-6 of the minimum), rule="reference" is Best_pair's running minimum, a Python
loop (use it at n <= 65).  sums selects how S and the lambda sum are added: "numpy" (pairwise), "fsum" (exactly rounded) or
"reversed" (sequential from the far end)."""
import math
import re

import numpy as np

PAIR_EPS = 1e-6   # Best_pair's 0.000001


def symmetrise(m):
    m = np.asarray(m, dtype=np.float64)
    out = (m + m.T) / 2.0
    np.fill_diagonal(out, 0.0)
    return out


def _sum(values, sums):
    if sums == "numpy":
        return float(np.sum(values))
    if sums == "fsum":
        return math.fsum(values)
    if sums == "reversed":
        tot = 0.0
        for v in values[::-1]:
            tot += float(v)
        return tot
    raise ValueError(sums)


def _row_sums(sub, sums):
    if sums == "numpy":
        return sub.sum(axis=1)   # (the diagonal is 0.0)
    return np.array([_sum(row, sums) for row in sub])


def bionj(dist, var=None, rule="first", sums="numpy"):
    """-> dict(steps=[(a, b, la, lb, lambda)], last=[l0, l1, l2], last_len=[..], margin=[per step], near=[per step],
    guard=[per step]).  margin: the smallest Q above m + 1e-6, minus m (inf when there is none); near: some Q lies in
    (m + 1e-6, m + 2e-6], where the two pair rules may part; guard: the distance of the closest Q to the threshold
    m + 1e-6 itself, where rounding could move a pair across it."""
    D = symmetrise(dist)
    V = D.copy() if var is None else symmetrise(var)
    n = D.shape[0]
    assert n >= 3 and D.shape == (n, n) and V.shape == (n, n)
    act = np.arange(n)
    steps, margin, near, guard = [], [], [], []
    while act.size > 3:
        r = act.size
        sub = D[np.ix_(act, act)]
        S = _row_sums(sub, sums)
        Q = (r - 2) * sub - S[:, None] - S[None, :]   # Q[x, y], x the row: ((r - 2) D_xy - S_x) - S_y
        low = np.tril(np.ones((r, r), dtype=bool), -1)
        q = Q[low]
        m = q.min()
        above = q[q > m + PAIR_EPS]
        margin.append(float(above.min() - m) if above.size else math.inf)
        near.append(bool(((q > m + PAIR_EPS) & (q <= m + 2 * PAIR_EPS)).any()))
        guard.append(float(np.abs(q - (m + PAIR_EPS)).min()))
        if rule == "first":
            px, py = np.argwhere(low & (Q <= m + PAIR_EPS))[0]   # (row-major: x ascending, then y ascending)
        elif rule == "reference":
            qmin, px, py = 1.0e300, 0, 0
            for x in range(r):
                for y in range(x):
                    if Q[x, y] < qmin - PAIR_EPS:
                        qmin, px, py = Q[x, y], x, y
        else:
            raise ValueError(rule)
        a, b = int(act[px]), int(act[py])
        vab = V[a, b]
        la = 0.5 * (D[a, b] + (S[px] - S[py]) / (r - 2))
        lb = 0.5 * (D[a, b] + (S[py] - S[px]) / (r - 2))
        others = act[(act != a) & (act != b)]
        if vab == 0.0:
            lam = 0.5
        else:
            lam = 0.5 + _sum(V[b, others] - V[a, others], sums) / (2.0 * (r - 2) * vab)
        lam = min(1.0, max(0.0, lam))
        nd = lam * (D[a, others] - la) + (1.0 - lam) * (D[b, others] - lb)
        nv = lam * V[a, others] + (1.0 - lam) * V[b, others] - lam * (1.0 - lam) * vab
        D[a, others] = D[others, a] = nd
        V[a, others] = V[others, a] = nv
        steps.append((a, b, float(la), float(lb), float(lam)))
        act = act[act != b]
    l0, l1, l2 = (int(x) for x in act)
    last_len = [0.5 * (D[l0, l1] + D[l0, l2] - D[l1, l2]), 0.5 * (D[l1, l0] + D[l1, l2] - D[l0, l2]),
                0.5 * (D[l2, l1] + D[l2, l0] - D[l1, l0])]
    return dict(steps=steps, last=[l0, l1, l2], last_len=[float(x) for x in last_len], margin=margin, near=near, guard=guard)


# ------------------------------------------------------------------------------------------
# splits
# ------------------------------------------------------------------------------------------
def _key(members, n):
    s = frozenset(members)
    return frozenset(range(n)) - s if 0 in s else s


def log_splits(steps, last, last_len, n):
    """the unrooted splits of a step log: {the side without taxon 0 (frozenset of taxon ids): length}"""
    cluster = {i: {i} for i in range(n)}
    out = {}

    def add(members, length):
        k = _key(members, n)
        out[k] = out.get(k, 0.0) + length

    for a, b, la, lb, _ in steps:
        add(cluster[a], la)
        add(cluster[b], lb)
        cluster[a] = cluster[a] | cluster.pop(b)
    for l, length in zip(last, last_len):
        add(cluster[int(l)], length)
    return out


def newick_splits(newick, names):
    """the same from a Newick string whose leaf labels are `names` (index = taxon id)"""
    ids = {str(nm): i for i, nm in enumerate(names)}
    n = len(names)
    tokens = re.findall(r"[(),;]|[^(),;:\s]+|:\s*[-+0-9.eE]+", newick)
    out = {}
    pos = 0

    def parse():
        nonlocal pos
        members = set()
        if tokens[pos] == "(":
            pos += 1
            while True:
                members |= parse()
                if tokens[pos] == ",":
                    pos += 1
                    continue
                assert tokens[pos] == ")", tokens[pos]
                pos += 1
                break
            if pos < len(tokens) and tokens[pos] not in "(),;" and not tokens[pos].startswith(":"):
                pos += 1   # (an internal label)
        else:
            members.add(ids[tokens[pos]])
            pos += 1
        if pos < len(tokens) and tokens[pos].startswith(":"):
            k = _key(members, n)
            out[k] = out.get(k, 0.0) + float(tokens[pos][1:])
            pos += 1
        return members

    assert parse() == set(range(n)), "the tree does not hold every taxon once"
    return out


def max_split_diff(got, want):
    """the split sets must be equal -> the largest difference of their lengths"""
    assert set(got) == set(want), (sorted(map(sorted, set(got) ^ set(want))))
    return max(abs(got[k] - want[k]) for k in want)


# ------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------
def uniform_matrix(n, seed):
    rng = np.random.default_rng(1000 * n + seed)
    A = rng.uniform(0.05, 1, (n, n))
    D = np.round((A + A.T) / 2, 7)
    np.fill_diagonal(D, 0.0)
    return D


def duplicates_matrix(n, seed=1):
    """a uniform m x m matrix, m = n // 2, expanded by a row map that repeats rows: taxa i and i + m (and i + 2 m) are
    duplicates of each other at distance 0"""
    m = n // 2
    base = uniform_matrix(m, seed)
    rows = np.arange(n) % m
    return base[np.ix_(rows, rows)].copy()


def balanced_matrix(depth, edge):
    """path lengths between the 2^depth leaves of a perfectly balanced rooted binary tree with every edge `edge`"""
    n = 1 << depth
    D = np.zeros((n, n))
    for i in range(n):
        for j in range(n):
            if i != j:
                D[i, j] = 2 * edge * (i ^ j).bit_length()
    return D


def star_matrix(n, d):
    D = np.full((n, n), float(d))
    np.fill_diagonal(D, 0.0)
    return D


def matrix_text(D, names):
    """the text BioNj::create reads (and Alignment::printDist writes): 7 decimals"""
    lines = [str(len(names))]
    for i, nm in enumerate(names):
        lines.append(nm + " " + " ".join("%.7f" % v for v in D[i]))
    return "\n".join(lines) + "\n"


def parse_matrix_text(text):
    tok = text.split()
    n = int(tok[0])
    names, rows = [], []
    for i in range(n):
        part = tok[1 + i * (n + 1): 1 + (i + 1) * (n + 1)]
        names.append(part[0])
        rows.append([float(v) for v in part[1:]])
    return names, np.array(rows)
