"""Restatements for the UFBoot tests, written from the reference's text and independent of the C++:

* ufboot_rule      IQTree::saveCurrentTree's per-replicate rule (iqtree.cpp:2738-2750) in numpy: sequential over the entries,
                   vectorised over the replicates, every comparison worded as there.
* newick_splits / split_counts / supports / consensus      the splits of Newick strings, the weighted split counts of a
                   tree set (MTreeSet::convertSplits, SW_COUNT), createBootstrapSupport's numbers (mexttree.cpp:416-461)
                   and the greedy consensus (findMaxCompatibleSplits, splitgraph.cpp:673-706; ties: first appearance).
A split is the frozenset of the taxa on the side WITHOUT taxon 0.
"""
import numpy as np

DBL_MAX = np.finfo(np.float64).max


def ufboot_start(nsamples):
    """iqtree.cpp:308-312"""
    return dict(boot_logl=np.full(nsamples, -DBL_MAX), boot_orig_logl=np.full(nsamples, -DBL_MAX),
                boot_counts=np.zeros(nsamples, dtype=np.int32), boot_tree=np.full(nsamples, -1, dtype=np.int64))


def ufboot_rule(state, rell, tree_ids, logl, rand, epsilon=0.5, logl_cutoff=0.0, margins=None):
    """Applies the entries in order to `state` (in place).  rell[i] = the nsamples RELL sums of entry i.  Returns
    (counts = [applied, dropped, slots replaced], min_orig_logl).  margins (optional array, nsamples): receives per
    replicate the smallest |rell - (boot_logl +- epsilon)| any comparison of an applied entry saw."""
    bl, bo, bc, bt = state["boot_logl"], state["boot_orig_logl"], state["boot_counts"], state["boot_tree"]
    applied = dropped = replaced = 0
    for i in range(len(tree_ids)):
        if logl_cutoff != 0.0 and logl[i] < logl_cutoff - 1.0:   # :2678
            dropped += 1
            continue
        applied += 1
        r = np.asarray(rell[i], dtype=np.float64)
        if margins is not None:
            with np.errstate(over="ignore"):
                np.minimum(margins, np.minimum(np.abs(r - (bl + epsilon)), np.abs(r - (bl - epsilon))), out=margins)
        better = r > bl + epsilon
        tie = ~better & (r > bl - epsilon)
        better = better | (tie & (rand[i] <= 1.0 / (bc + 1)))
        inc = better & (r <= bl + epsilon)
        bc[better & inc] += 1
        bc[better & ~inc] = 1
        bl[better] = np.maximum(bl[better], r[better])
        bo[better] = logl[i]
        bt[better] = tree_ids[i]
        replaced += int(better.sum())
    held = bt >= 0
    return np.array([applied, dropped, replaced], dtype=np.int64), (float(bo[held].min()) if held.any() else DBL_MAX)


# ---- splits ------------------------------------------------------------------------------------------------------------
def _parse(newick, names=None):
    """nested lists of taxon ids; lengths, internal labels and [comments] are dropped"""
    lookup = None if names is None else {n: i for i, n in enumerate(names)}
    pos = 0
    text = newick.strip()

    def skip_tail():
        nonlocal pos
        while pos < len(text) and text[pos] not in ",();":
            if text[pos] == "[":
                pos = text.index("]", pos)
            pos += 1

    def node():
        nonlocal pos
        if text[pos] == "(":
            pos += 1
            kids = [node()]
            while text[pos] == ",":
                pos += 1
                kids.append(node())
            assert text[pos] == ")", (newick, pos)
            pos += 1
            skip_tail()
            return kids
        start = pos
        while text[pos] not in ":,();[":
            pos += 1
        label = text[start:pos].strip()
        skip_tail()
        return int(label) if lookup is None else lookup[label]

    tree = node()
    assert text[pos] == ";", (newick, pos)
    return tree


def newick_splits(newick, ntaxa, names=None):
    """the non-trivial splits in the post-order of the string"""
    out = []
    everyone = frozenset(range(ntaxa))

    def walk(nd, top):
        if not isinstance(nd, list):
            return frozenset([nd])
        mine = frozenset()
        for k in nd:
            mine |= walk(k, False)
        if not top:
            s = everyone - mine if 0 in mine else mine
            if 2 <= len(s) <= ntaxa - 2 and s not in out:
                out.append(s)
        return mine

    assert walk(_parse(newick, names), True) == everyone
    return out


def split_counts(trees, ntaxa, weights=None, names=None):
    """(splits in first-appearance order, {split: summed weight}, sum of the weights)"""
    order, count = [], {}
    weights = [1] * len(trees) if weights is None else list(weights)
    for t, w in zip(trees, weights):
        for s in newick_splits(t, ntaxa, names):
            if s not in count:
                order.append(s)
                count[s] = 0
            count[s] += w
    return order, count, sum(weights)


def _round_half_away(x):
    return int(np.floor(x + 0.5)) if x >= 0 else -int(np.floor(-x + 0.5))


def supports(trees, query, ntaxa, weights=None, names=None):
    """round(100 count / sum of the weights) for every split of `query`, 0 where no tree has the split"""
    _, count, total = split_counts(trees, ntaxa, weights, names)
    return [_round_half_away(100.0 * count.get(s, 0) / total) for s in newick_splits(query, ntaxa, names)]


def compatible(a, b):
    return not (a & b) or a <= b or b <= a


def consensus_splits(trees, ntaxa, weights=None, names=None):
    """findMaxCompatibleSplits: descending weight, ties to the first appearance, taken when compatible with all taken"""
    order, count, total = split_counts(trees, ntaxa, weights, names)
    ranked = sorted(range(len(order)), key=lambda k: (-count[order[k]], k))
    taken = []
    for k in ranked:
        if len(taken) >= ntaxa - 3:
            break
        if all(compatible(order[k], t) for t in taken):
            taken.append(order[k])
    return [(s, _round_half_away(100.0 * count[s] / total)) for s in taken]


def consensus(trees, ntaxa, weights=None, names=None):
    """the consensus tree as a string: rooted at taxon 0's node, children by ascending smallest taxon, supports as labels"""
    clades = consensus_splits(trees, ntaxa, weights, names)
    label = {s: str(p) for s, p in clades}
    sets = [s for s, _ in clades]

    def write(members, inside):
        kids = [s for s in sets if s < members and not any(s < o < members for o in sets)] if inside else \
               [s for s in sets if not any(s < o for o in sets)]
        loose = sorted(members - frozenset().union(*kids)) if kids else sorted(members)
        parts = [(min(s), "(" + write(s, True) + ")" + label[s]) for s in kids]
        parts += [(t, str(t) if names is None else names[t]) for t in loose]
        return ",".join(p for _, p in sorted(parts))

    return "(" + write(frozenset(range(ntaxa)), False) + ");"
