"""A numpy restatement of bit-parallel Fitch parsimony, written from the algorithm: the expected values of
tests/test_parsimony_host.py and tests/test_parsimony_gpu.py.

Sites: pattern p contributes ptn_freq[p] consecutive sites when informative[p] != 0, in pattern order; 32 sites make a word
column.  A vector is planes[nwords, nstates] uint32 (bit b of planes[w, i]: site 32 w + b allows state i) plus the number
of substitutions inside its subtree.  The padding bits of the last word carry plane 0 at every tip, so they never score.
  update       z = x & y;  w = ~OR_i z_i;  z_i |= w & (x_i | y_i);  score = x.score + y.score + popcount(w)
  branch       score = a.score + c.score + popcount(~OR_i(a_i & c_i)); subst = the popcount alone
  insertion    m = update(a, c) without its score; score = a.score + c.score + popcount(w_ac) + popcount(~OR_i(m_i & t_i))
sankoff_min is independent of all bit tricks: per site the minimum number of changes over all labelings of the internal
nodes, a leaf costing nothing on its edge when the neighbour's label is one of the states its code allows.
Trees are adjacency dicts {node: [neighbours]}, leaves 0 .. ntaxa-1 of degree 1, internal nodes of degree 3."""
import itertools

import numpy as np

SEQ_DNA, SEQ_PROTEIN, SEQ_CODON = 0, 1, 2
AMBI_AA = (4 + 8, 32 + 64, 512 + 1024)   # B = N|D, Z = Q|E, J = I|L


def state_unknown(nstates):
    return {4: 18, 20: 23, 64: 64}[nstates]


def state_masks(nstates):
    """the states every state code allows, as a python int bit mask per code (codes 0 .. STATE_UNKNOWN)"""
    full = (1 << nstates) - 1
    m = [1 << s for s in range(nstates)]
    if nstates == 4:
        m += [s - 3 for s in range(4, 18)]
    elif nstates == 20:
        m += list(AMBI_AA)
    m.append(full)
    assert len(m) == state_unknown(nstates) + 1
    return m


def site_patterns(ptn_freq, informative=None):
    """pattern index of every site"""
    f = np.asarray(ptn_freq)
    assert np.all(f >= 0) and np.all(f == np.floor(f))
    keep = np.ones(f.size, dtype=bool) if informative is None else np.asarray(informative) != 0
    return np.repeat(np.arange(f.size), np.where(keep, f, 0).astype(np.int64))


def tip_vectors(states, site_ptn, nstates):
    """planes[ntaxa, nwords, nstates] uint32"""
    states = np.asarray(states)
    masks = state_masks(nstates)
    nsites = len(site_ptn)
    nwords = max(1, (nsites + 31) // 32)
    allow = np.zeros((len(masks), nstates), dtype=np.uint32)
    for s, m in enumerate(masks):
        for i in range(nstates):
            allow[s, i] = (m >> i) & 1
    bits = np.zeros((states.shape[0], nwords * 32, nstates), dtype=np.uint32)
    bits[:, :nsites, :] = allow[states[:, site_ptn]]
    bits[:, nsites:, 0] = 1   # the dummy states of the padding
    shifts = np.arange(32, dtype=np.uint32)
    b = bits.reshape(states.shape[0], nwords, 32, nstates)
    return np.bitwise_or.reduce(b << shifts[None, None, :, None], axis=2).astype(np.uint32)


def popcount(a):
    a = np.asarray(a, dtype=np.uint32)
    return int(np.unpackbits(a.view(np.uint8)).sum())


def update(x, y):
    """(planes, score) of the parent of x = (planes, score) and y"""
    z = x[0] & y[0]
    w = ~np.bitwise_or.reduce(z, axis=1)
    z = z | (w[:, None] & (x[0] | y[0]))
    return z.astype(np.uint32), x[1] + y[1] + popcount(w)


def branch_score(a, c):
    """-> (score, subst) of the branch whose two directed vectors are a and c"""
    subst = popcount(~np.bitwise_or.reduce(a[0] & c[0], axis=1))
    return a[1] + c[1] + subst, subst


def insert_score(a, c, t):
    """score of the tree with tip vector t inserted into branch (a, c)"""
    m, s = update(a, c)
    return s + popcount(~np.bitwise_or.reduce(m & t[0], axis=1))


# ---- trees ------------------------------------------------------------------------------------------------------------
def random_tree(ntaxa, rng, order=None, first_internal=None):
    """random unrooted binary tree by random stepwise insertion; internal nodes first_internal (default ntaxa) upwards"""
    order = list(range(ntaxa)) if order is None else list(order)
    top = ntaxa if first_internal is None else first_internal
    adj = {order[0]: [top], order[1]: [top], order[2]: [top], top: [order[0], order[1], order[2]]}
    nxt = top + 1
    for t in order[3:]:
        edges = branches(adj)
        a, b = edges[int(rng.integers(len(edges)))]
        insert_leaf(adj, a, b, t, nxt)
        nxt += 1
    return adj


def insert_leaf(adj, a, b, leaf, new_node):
    adj[a][adj[a].index(b)] = new_node
    adj[b][adj[b].index(a)] = new_node
    adj[new_node] = [a, b, leaf]
    adj[leaf] = [new_node]


def caterpillar(ntaxa):
    adj = {0: [ntaxa], 1: [ntaxa], ntaxa: [0, 1, ntaxa + 1]}
    for k in range(2, ntaxa - 1):
        node = ntaxa + k - 1
        adj[k] = [node]
        adj[node] = [node - 1, k, node + 1]
    last = 2 * ntaxa - 3
    adj[ntaxa - 1] = [last]
    adj[last][2] = ntaxa - 1
    return adj


def branches(adj):
    """every branch once, as (a, b) with a < b, sorted"""
    return sorted((a, b) for a in adj for b in adj[a] if a < b)


def newick(adj, lengths=None):
    """rooted for printing at the internal node next to leaf 0"""
    def sub(u, dad):
        ln = "" if lengths is None else ":%.17g" % lengths[(min(u, dad), max(u, dad))]
        kids = [v for v in adj[u] if v != dad]
        if not kids:
            return "%d%s" % (u, ln)
        return "(" + ",".join(sub(v, u) for v in kids) + ")" + ln
    top = adj[0][0]
    return "(" + ",".join(sub(v, top) for v in adj[top]) + ");"


def directed_vectors(adj, tips):
    """{(u, v): (planes, score)}: the subtree that hangs at u when looking from its neighbour v, for every directed branch"""
    out = {}

    def get(u, v):
        if (u, v) not in out:
            kids = [k for k in adj[u] if k != v]
            if not kids:
                out[(u, v)] = (tips[u], 0)
            else:
                assert len(kids) == 2
                out[(u, v)] = update(get(kids[0], u), get(kids[1], u))
        return out[(u, v)]

    import sys
    sys.setrecursionlimit(max(sys.getrecursionlimit(), 4 * len(adj) + 100))
    for u in adj:
        for v in adj[u]:
            get(u, v)
    return out


def tree_score(adj, tips):
    a, b = branches(adj)[0]
    dv = directed_vectors(adj, tips)
    return branch_score(dv[(a, b)], dv[(b, a)])[0]


def sankoff_min(adj, states, site_ptn, nstates):
    """sum over the sites of the minimum number of changes over ALL labelings of the internal nodes.  The labels of a site
    run over the states that at least one CONSTRAINING leaf allows there (a leaf whose code allows every state, STATE_UNKNOWN,
    costs nothing under any labeling): a label outside that set can be replaced by the label of a neighbouring node without
    adding a change, so the minimum is reached inside the set.  With no constraining leaf the site costs nothing."""
    masks = state_masks(nstates)
    full = (1 << nstates) - 1
    ntaxa = np.asarray(states).shape[0]
    internal = sorted(u for u in adj if len(adj[u]) > 1)
    pos = {u: k for k, u in enumerate(internal)}
    total = 0
    cache = {}
    for p in site_ptn:
        col = tuple(int(s) for s in np.asarray(states)[:, p])
        if col not in cache:
            union = 0
            for a in adj:
                if a < ntaxa and masks[col[a]] != full:
                    union |= masks[col[a]]
            cand = [i for i in range(nstates) if (union >> i) & 1] or [0]
            assert len(cand) ** len(internal) <= 2_000_000, "brute force too large"
            lab = np.array(list(itertools.product(cand, repeat=len(internal))), dtype=np.int64)
            cost = np.zeros(lab.shape[0], dtype=np.int64)
            for a, b in branches(adj):
                if a < ntaxa:   # leaf a, internal b
                    allowed = np.array([(masks[col[a]] >> i) & 1 for i in range(nstates)], dtype=np.int64)
                    cost += 1 - allowed[lab[:, pos[b]]]
                else:
                    cost += lab[:, pos[a]] != lab[:, pos[b]]
            cache[col] = int(cost.min())
        total += cache[col]
    return total


def ordered_branches(adj, root):
    """MTree::getBranches: depth first from the root in neighbour order, each branch as (lower id, higher id)"""
    out, stack = [], [(root, None, iter(adj[root]))]
    while stack:
        node, dad, it = stack[-1]
        nb = next(it, None)
        if nb is None:
            stack.pop()
        elif nb != dad:
            out.append((min(node, nb), max(node, nb)))
            stack.append((nb, node, iter(adj[nb])))
    return out


def stepwise_addition(tips, order):
    """stepwise addition by maximum parsimony, the same steps as computeParsimonyTree: per step the vectors an insertion
    invalidated are recomputed (and no others), every branch of getBranches order is scored with insert_score and the
    FIRST minimum is taken; node ids and neighbour order as the reference's tree surgery leaves them
    -> (score, adj, number of updates, number of branches scored)"""
    ntaxa = len(order)
    adj = {ntaxa: list(order[:3])}
    for k in order[:3]:
        adj[k] = [ntaxa]
    root, dv, nupd, nscan, best = order[0], {}, 0, 0, None

    def vec(u, v):   # the subtree at u seen from v (iterative post-order over what is missing)
        nonlocal nupd
        if u < ntaxa:
            return (tips[u], 0)
        todo = [(u, v)]
        while todo:
            x, y = todo[-1]
            if (x, y) in dv:
                todo.pop()
                continue
            kids = [k for k in adj[x] if k != y]
            need = [(k, x) for k in kids if k >= ntaxa and (k, x) not in dv]
            if need:
                todo.extend(need)
                continue
            a, b = [(tips[k], 0) if k < ntaxa else dv[(k, x)] for k in kids]
            dv[(x, y)] = update(a, b)
            nupd += 1
            todo.pop()
        return dv[(u, v)]

    for cur in range(3, ntaxa):
        br = ordered_branches(adj, root)
        new = (tips[order[cur]], 0)
        scores = [insert_score(vec(a, b), vec(b, a), new) for a, b in br]
        nscan += len(br)
        k = int(np.argmin(scores))
        best = scores[k]
        a, b = br[k]
        added = ntaxa + cur - 2
        adj[a][adj[a].index(b)] = added
        adj[b][adj[b].index(a)] = added
        adj[added] = [order[cur], a, b]
        adj[order[cur]] = [added]
        # what a and b showed each other now belongs to the added node; every vector that looks towards it is stale
        for x, y in ((a, b), (b, a)):
            if (x, y) in dv:
                dv[(x, added)] = dv.pop((x, y))
        stack = [(a, added), (b, added)]
        while stack:
            x, dad = stack.pop()
            for nb in adj[x]:
                if nb != dad:
                    dv.pop((x, nb), None)
                    stack.append((nb, x))
    # fixNegativeBranch(true): every remaining vector, then the substitution count of every branch
    subst = {(a, b): branch_score(vec(a, b), vec(b, a)) for a, b in ordered_branches(adj, root)}
    if best is None:
        best = next(iter(subst.values()))[0]
    return best, adj, nupd, nscan


def is_informative(states, nstates):
    """per pattern: at least two states, each shown by at least two taxa; an ambiguity code counts towards every state it
    allows, STATE_UNKNOWN towards none"""
    states = np.asarray(states)
    masks = state_masks(nstates)
    su = state_unknown(nstates)
    allow = np.zeros((len(masks), nstates), dtype=np.int64)
    for s, m in enumerate(masks):
        if s != su:
            for i in range(nstates):
                allow[s, i] = (m >> i) & 1
    num_app = allow[states].sum(axis=0)          # [nptn, nstates]
    return ((num_app >= 2).sum(axis=1) >= 2).astype(np.uint8)


# ---- alignments for the tests -----------------------------------------------------------------------------------------
def random_states(ntaxa, nptn, nstates, rng, amb_frac=0.10, alphabet=None):
    """random state codes with amb_frac of the cells an ambiguity code or STATE_UNKNOWN (where the alphabet has codes)"""
    k = nstates if alphabet is None else alphabet
    st = rng.integers(0, k, size=(ntaxa, nptn)).astype(np.uint8)
    amb = rng.random((ntaxa, nptn)) < amb_frac
    su = state_unknown(nstates)
    codes = np.arange(nstates, su + 1)
    st[amb] = rng.choice(codes, size=int(amb.sum())).astype(np.uint8)
    return st
