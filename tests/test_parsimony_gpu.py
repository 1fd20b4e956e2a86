"""GPU: Fitch parsimony on the device (include/iqhip.h "Fitch parsimony") against the numpy restatement of
tests/fitch_ref.py -- everything is integer arithmetic and every comparison is exact equality.

Tips (every size at which the packing takes another path: one site, a word less one, a word, a word and one, two words, two
words and one, and 2049 sites = the smallest count with more than one wave of word columns), updates and branch scores on
random trees, deep and wide op lists in one launch / split over calls / with permuted slots, the insertion scan with its
first-minimum rule, the lifetime of the state and the refusals; then the host mirror on top: the stepwise-addition tree step
by step against a replay of the reference's tree surgery, fixNegativeBranch's lengths, the hand-over to the likelihood
kernels, and iqhip_lnl -parstree / -pars."""
import numpy as np
import pytest

import fitch_ref as F

pytestmark = pytest.mark.gpu

SEQ = {4: 0, 20: 1, 64: 2}


def model_for(synth, n):
    return synth.gtr_model(alpha=0.9, ncat=4) if n == 4 else synth.random_reversible_model(n, 3, alpha=0.9, ncat=2)


def make_tree(pkg, synth, n, states, freq, model=None, sharded=0, nwk=None):
    t = pkg.PhyloTree(nwk or synth.random_tree_newick(states.shape[0], 1))
    t.set_alignment(n, SEQ.get(n, 3), states, freq)
    t.set_model(model or model_for(synth, n))
    t.set_likelihood_kernel(pkg.LK_EIGEN_HIP)
    if sharded:
        t.attach_engine_sharded([0] * sharded, pkg.REDUCE_HOST)
    else:
        t.attach_engine(0)
    return t


def alignment(n, ntaxa, nsites, rng, tail=True):
    """patterns with integer frequencies that add up to nsites over the informative-masked ones, 10 % ambiguity codes or
    unknowns, a tail of zero-frequency patterns and a mixed mask -> states, freq, mask"""
    nkeep = max(1, min(nsites, 40 if nsites > 100 else nsites))
    fr_keep = np.full(nkeep, nsites // nkeep, dtype=np.float64)
    fr_keep[: nsites - int(fr_keep.sum())] += 1
    assert fr_keep.sum() == nsites
    nskip, nzero = 5, (4 if tail else 0)
    mask = np.concatenate([np.ones(nkeep, np.uint8), np.zeros(nskip, np.uint8)])
    freq = np.concatenate([fr_keep, rng.integers(1, 5, size=nskip).astype(float)])
    perm = rng.permutation(mask.size)
    mask, freq = mask[perm], freq[perm]
    mask = np.concatenate([mask, np.ones(nzero, np.uint8)])       # the unobserved +ASC patterns: frequency 0
    freq = np.concatenate([freq, np.zeros(nzero)])
    states = F.random_states(ntaxa, mask.size, n, rng, amb_frac=0.10)
    return states, freq, mask


def all_directed_ops(adj, ntaxa):
    """ops for every directed vector in an order that has children first -> (ops rows, {(u, v): slot})"""
    slot, ops = {}, []
    import sys
    sys.setrecursionlimit(20000)

    def get(u, v):
        if u < ntaxa:
            return u
        if (u, v) not in slot:
            kids = [k for k in adj[u] if k != v]
            l, r = get(kids[0], u), get(kids[1], u)
            slot[(u, v)] = ntaxa + len(slot)
            ops.append((slot[(u, v)], l, r))
        return slot[(u, v)]

    for u in sorted(adj):
        for v in adj[u]:
            get(u, v)
    return ops, slot


def slot_of(slot, u, v, ntaxa):
    return u if u < ntaxa else slot[(u, v)]


# ---- tips -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nsites", [1, 31, 32, 33, 64, 65, 2049])
@pytest.mark.parametrize("n", [4, 20, 64])
def test_tip_vectors_equal_the_restatement(pkg, synth, n, nsites):
    rng = np.random.default_rng(n * 7919 + nsites)
    ntaxa = 5
    states, freq, mask = alignment(n, ntaxa, nsites, rng)
    assert (states >= n).any() and (freq[-4:] == 0).all() and 0 < mask.sum() < mask.size
    t = make_tree(pkg, synth, n, states, freq)
    assert t.pars_init(mask, 0) == nsites
    want = F.tip_vectors(states, F.site_patterns(freq, mask), n)
    for k in range(ntaxa):
        planes, score = t.pars_fetch(k)
        np.testing.assert_array_equal(planes, want[k])
        assert score == 0
    # without a mask every pattern counts
    assert t.pars_init(None, 0) == int(freq.sum())
    np.testing.assert_array_equal(t.pars_fetch(ntaxa - 1)[0], F.tip_vectors(states, F.site_patterns(freq), n)[ntaxa - 1])
    t.close()


# ---- updates and branch scores ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nsites", [33, 2049])
@pytest.mark.parametrize("ntaxa", [3, 4, 5, 17, 64])
@pytest.mark.parametrize("n", [4, 20, 64])
def test_updates_and_branch_scores(pkg, synth, n, ntaxa, nsites):
    rng = np.random.default_rng(n * 104729 + ntaxa * 131 + nsites)
    states, freq, mask = alignment(n, ntaxa, nsites, rng)   # 10 % ambiguity codes / unknowns at every state count
    assert (states >= n).any()
    sp = F.site_patterns(freq, mask)
    tips = F.tip_vectors(states, sp, n)
    adj = F.random_tree(ntaxa, rng)
    ops, slot = all_directed_ops(adj, ntaxa)
    assert len(ops) == 3 * (ntaxa - 2)
    t = make_tree(pkg, synth, n, states, freq)
    assert t.pars_init(mask) == nsites
    t.pars_update(ops)
    dv = F.directed_vectors(adj, tips)
    for (u, v), s in slot.items():
        planes, score = t.pars_fetch(s)
        np.testing.assert_array_equal(planes, dv[(u, v)][0], err_msg=str((u, v)))
        assert score == dv[(u, v)][1], (u, v)
    br = F.branches(adj)
    br = [br[k] if rng.random() < 0.5 else br[k][::-1] for k in rng.permutation(len(br))]   # scrambled, either direction
    ends = [(slot_of(slot, a, b, ntaxa), slot_of(slot, b, a, ntaxa)) for a, b in br]
    score, subst = t.pars_branch_scores(ends)
    want = [F.branch_score(dv[(a, b)], dv[(b, a)]) for a, b in br]
    assert score.tolist() == [w[0] for w in want] and subst.tolist() == [w[1] for w in want]
    assert len(set(score.tolist())) == 1          # the score of a tree is the same at every branch
    if ntaxa <= 8:   # (at most 3 internal nodes here: the brute force is a few thousand labelings a column)
        assert int(score[0]) == F.sankoff_min(adj, states, sp, n)
    t.close()


# ---- depth and levels ---------------------------------------------------------------------------------------------------
def balanced(ntaxa):
    """a balanced unrooted tree: the two halves are joined by one branch"""
    adj, cur, nxt = {}, list(range(ntaxa)), ntaxa
    while len(cur) > 2:
        new = []
        for k in range(0, len(cur), 2):
            adj[nxt] = [cur[k], cur[k + 1]]
            for c in (cur[k], cur[k + 1]):
                adj.setdefault(c, []).append(nxt)
            new.append(nxt)
            nxt += 1
        cur = new
    adj[cur[0]].append(cur[1])
    adj[cur[1]].append(cur[0])
    return adj


@pytest.mark.parametrize("shape", ["caterpillar300", "balanced256"])
def test_deep_and_wide_op_lists_in_one_launch(pkg, synth, shape):
    ntaxa = 300 if shape == "caterpillar300" else 256
    rng = np.random.default_rng(ntaxa)
    states, freq, mask = alignment(4, ntaxa, 2049, rng)
    sp = F.site_patterns(freq, mask)
    tips = F.tip_vectors(states, sp, 4)
    adj = F.caterpillar(ntaxa) if shape == "caterpillar300" else balanced(ntaxa)
    # the ops towards one branch: for the caterpillar the far end (298 levels of one op), for the balanced tree the middle
    root = (ntaxa - 1, 2 * ntaxa - 3) if shape == "caterpillar300" else tuple(sorted(adj)[-2:])
    slot, ops = {}, []
    import sys
    sys.setrecursionlimit(20000)

    def get(u, v):
        if u < ntaxa:
            return u
        if (u, v) not in slot:
            kids = [k for k in adj[u] if k != v]
            l, r = get(kids[0], u), get(kids[1], u)
            slot[(u, v)] = ntaxa + len(slot)
            ops.append((slot[(u, v)], l, r))
        return slot[(u, v)]

    ra, rb = get(root[0], root[1]), get(root[1], root[0])
    lev = pkg.pars_levels(ntaxa, len(ops), ops)
    if shape == "caterpillar300":
        assert len(ops) == 298 and sorted(lev.tolist()) == list(range(298))
    else:
        assert len(ops) == 254 and np.bincount(lev).tolist() == [128, 64, 32, 16, 8, 4, 2]
    dv = F.directed_vectors(adj, tips)
    want = F.branch_score(dv[(root[0], root[1])], dv[(root[1], root[0])])
    t = make_tree(pkg, synth, 4, states, freq)
    nvec = len(ops)

    def run(op_rows, pieces, a, b, fetch):
        t.pars_init(mask, nvec)
        bounds = np.linspace(0, len(op_rows), pieces + 1).astype(int)
        for k in range(pieces):
            t.pars_update(op_rows[bounds[k]:bounds[k + 1]])
        sc, sb = t.pars_branch_scores([(a, b)])
        return (int(sc[0]), int(sb[0])), [t.pars_fetch(s) for s in fetch]

    probe = [ops[0][0], ops[len(ops) // 2][0], ops[-1][0]]
    one, v1 = run(ops, 1, ra, rb, probe)
    assert one == want
    for (u, v), s in slot.items():
        if s in probe:
            got = v1[probe.index(s)]
            np.testing.assert_array_equal(got[0], dv[(u, v)][0])
            assert got[1] == dv[(u, v)][1]
    several, v2 = run(ops, 7, ra, rb, probe)
    perm = rng.permutation(nvec) + ntaxa                      # the same ops with the caller's slots renumbered
    ren = lambda s: int(s) if s < ntaxa else int(perm[s - ntaxa])
    permuted, v3 = run([(ren(d), ren(l), ren(r)) for d, l, r in ops], 1, ren(ra), ren(rb), [ren(s) for s in probe])
    assert one == several == permuted
    for a, b, c in zip(v1, v2, v3):
        np.testing.assert_array_equal(a[0], b[0])
        np.testing.assert_array_equal(a[0], c[0])
        assert a[1] == b[1] == c[1]
    t.close()


# ---- insertion scan -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ntaxa", [3, 4, 16, 63])
@pytest.mark.parametrize("n", [4, 20, 64])
def test_insertion_scan(pkg, synth, n, ntaxa):
    rng = np.random.default_rng(n * 17 + ntaxa)
    states, freq, mask = alignment(n, ntaxa + 3, 2049 if ntaxa == 16 else 65, rng)
    new, unknown, twin = ntaxa, ntaxa + 1, ntaxa + 2            # the held-out taxon, an all-unknown one, a copy of leaf 1
    states[unknown] = F.state_unknown(n)
    states[2] = states[1]                                       # two equal leaves in the tree ...
    states[twin] = states[1]                                    # ... and a third copy to insert: next to either costs nothing
    sp = F.site_patterns(freq, mask)
    tips = F.tip_vectors(states, sp, n)
    T = ntaxa + 3
    adj = F.random_tree(ntaxa, rng, first_internal=T)
    ops, slot = all_directed_ops(adj, T)
    t = make_tree(pkg, synth, n, states, freq)
    t.pars_init(mask)
    t.pars_update(ops)
    br = F.branches(adj)
    br = [br[k] for k in rng.permutation(len(br))]
    ends = [(slot_of(slot, a, b, T), slot_of(slot, b, a, T)) for a, b in br]
    for taxon in (new, unknown, twin):
        want = []
        for a, b in br:
            grown = {u: list(v) for u, v in adj.items()}
            F.insert_leaf(grown, a, b, taxon, 10 * T)
            want.append(F.tree_score(grown, tips))
        score, best, best_score = t.pars_insert_scores(ends, taxon)
        assert score.tolist() == want
        assert best == int(np.argmin(want)) and best_score == min(want)          # np.argmin: the first minimum
        assert t.pars_insert_scores(ends, taxon, want_scores=False) == (None, best, best_score)
        if taxon == unknown:
            assert len(set(want)) == 1 and best == 0
        if taxon == twin:
            assert want.count(min(want)) >= 2   # (a new taxon never lowers the score; beside leaf 1 or leaf 2 it adds nothing)
    t.close()


# ---- lifetime and refusals ----------------------------------------------------------------------------------------------
def code_of(pkg, fn, *a):
    with pytest.raises(pkg.EngineError) as ei:
        fn(*a)
    return ei.value.code


def test_lifetime_and_refusals(pkg, synth):
    rng = np.random.default_rng(11)
    states, freq, mask = alignment(4, 5, 200, rng, tail=False)
    states = np.concatenate([states] * 8, axis=1)     # (a shard holds at least 64 patterns)
    freq, mask = np.concatenate([freq] * 8), np.concatenate([mask] * 8)
    adj = F.random_tree(5, rng)
    ops, slot = all_directed_ops(adj, 5)
    t = make_tree(pkg, synth, 4, states, freq)
    INVALID, UNSUPPORTED = pkg.ERR_INVALID, pkg.ERR_UNSUPPORTED
    assert code_of(pkg, t.pars_update, ops) == INVALID            # before init
    assert code_of(pkg, t.pars_fetch, 0) == INVALID
    assert code_of(pkg, t.pars_init, mask, -1) == INVALID
    t.pars_init(mask)
    # a read of a never-written slot: refused before anything is launched, and nothing was written
    assert code_of(pkg, t.pars_update, [(ops[0][0], ops[0][1], ops[0][2]), (20, 19, 0)]) == INVALID
    assert code_of(pkg, t.pars_fetch, ops[0][0]) == INVALID
    assert code_of(pkg, t.pars_branch_scores, [(0, 19)]) == INVALID
    assert code_of(pkg, t.pars_branch_scores, np.zeros((0, 2))) == INVALID      # nbranch < 1
    t.pars_update(ops)
    ends = [(0, slot[(adj[0][0], 0)])]
    first = t.pars_branch_scores(ends)
    assert code_of(pkg, t.pars_insert_scores, ends, 5) == INVALID               # not a tip slot
    assert code_of(pkg, t.pars_insert_scores, ends, -1) == INVALID
    # new frequencies invalidate the state; a re-init recovers
    f2 = freq.copy()
    f2[mask != 0] *= 2
    t.set_ptn_freq(f2)
    assert code_of(pkg, t.pars_branch_scores, ends) == INVALID
    assert code_of(pkg, t.pars_update, ops) == INVALID
    assert t.pars_init(mask) == 2 * int(freq[mask != 0].sum())
    t.pars_update(ops)
    second = t.pars_branch_scores(ends)
    assert int(second[0][0]) == 2 * int(first[0][0])
    for bad in (0.5, -1.0):
        f3 = freq.copy()
        f3[int(np.flatnonzero(mask)[0])] = bad
        t.set_ptn_freq(f3)
        assert code_of(pkg, t.pars_init, mask) == INVALID
    t.close()
    # a mixture engine reads only the tip table: the plain engine's scores
    tm = make_tree(pkg, synth, 4, states, freq, model=synth.mixture_model(4, 3, 9, ncat=4))
    tm.pars_init(mask)
    tm.pars_update(ops)
    got = tm.pars_branch_scores(ends)
    assert (int(got[0][0]), int(got[1][0])) == (int(first[0][0]), int(first[1][0]))
    tm.close()
    ts = make_tree(pkg, synth, 4, states, freq, sharded=2)
    assert code_of(pkg, ts.pars_init, mask) == UNSUPPORTED
    ts.close()
    t5 = make_tree(pkg, synth, 5, (states % 5).astype(np.uint8), freq, model=synth.random_reversible_model(5, 4, alpha=0.7, ncat=4))
    assert code_of(pkg, t5.pars_init, mask) == UNSUPPORTED
    t5.close()


# ---- stepwise addition ----------------------------------------------------------------------------------------------------
ordered_branches = F.ordered_branches


def restated_lengths(adj, dv, n, nsite, min_len=1e-6):
    """fixNegativeBranch(true) with the same double expressions"""
    import math
    out = {}
    for a, b in F.branches(adj):
        subst = F.branch_score(dv[(a, b)], dv[(b, a)])[1]
        bl = (subst / nsite) if subst > 0 else (1.0 / nsite)
        z = n / (n - 1)
        x = 1.0 - (z * bl)
        if x > 0:
            bl = -math.log(x) / z
        out[(a, b)] = max(bl, min_len)
    return out


@pytest.mark.parametrize("ntaxa", [4, 5, 12, 40])
@pytest.mark.parametrize("n", [4, 20, 64])
def test_stepwise_addition_tree(pkg, synth, n, ntaxa):
    rng = np.random.default_rng(n * 1000 + ntaxa)
    states, freq, _ = alignment(n, ntaxa, 300, rng)
    if n != 4:   # few states per column, or hardly any protein / codon column is informative
        states = np.where(states < n, states % 4, states).astype(np.uint8)
    inf = F.is_informative(states, n)
    sp = F.site_patterns(freq, inf)
    assert 0 < len(sp) <= freq.sum()
    tips = F.tip_vectors(states, sp, n)
    order = [int(x) for x in rng.permutation(ntaxa)]
    t = make_tree(pkg, synth, n, states, freq)
    score, steps = t.compute_parsimony_tree(order, trace=True)
    assert t.pars_nsites == len(sp) and len(steps) == ntaxa - 3
    # replay: the reference's surgery on an ordered adjacency list, node ids as the reference numbers them
    adj = {ntaxa: list(order[:3])}
    for k in order[:3]:
        adj[k] = [ntaxa]
    root = order[0]
    last = None
    for cur, st in zip(range(3, ntaxa), steps):
        assert st["branches"] == ordered_branches(adj, root)
        dv = F.directed_vectors(adj, tips)
        want = [F.insert_score(dv[(a, b)], dv[(b, a)], (tips[order[cur]], 0)) for a, b in st["branches"]]
        assert st["scores"] == want
        assert st["chosen"] == int(np.argmin(want))           # the first minimum
        a, b = st["branches"][st["chosen"]]
        added = ntaxa + cur - 2
        adj[a][adj[a].index(b)] = added
        adj[b][adj[b].index(a)] = added
        adj[added] = [order[cur], a, b]
        adj[order[cur]] = [added]
        last = want[st["chosen"]]
    dv = F.directed_vectors(adj, tips)
    if last is None:
        last = F.tree_score(adj, tips)
    assert score == last == F.tree_score(adj, tips)
    assert t.get_branches() == ordered_branches(adj, root)
    assert t.compute_parsimony() == last
    # the lengths of fixNegativeBranch(true), exactly
    want_len = restated_lengths(adj, dv, n, float(freq.sum()))
    for (a, b), ln in want_len.items():
        assert dict(t.neighbors(a))[b] == ln == dict(t.neighbors(b))[a], (a, b)
    a, b = t.get_branches()[len(want_len) // 2]
    sc, sb = t.parsimony_branch(a, b)
    assert (sc, sb) == F.branch_score(dv[(a, b)], dv[(b, a)])
    # from scratch
    t.clear_all_partial_lh()
    assert t.compute_parsimony() == last
    assert t.fix_negative_branch(True) == 2 * ntaxa - 3
    for (a, b), ln in want_len.items():
        assert dict(t.neighbors(a))[b] == ln
    # the likelihood kernels take over the tree
    t.initialize_all_partial_lh()
    lnl = t.compute_likelihood()
    fresh = make_tree(pkg, synth, n, states, freq, nwk=t.tree_string())
    fresh.initialize_all_partial_lh()
    fresh.clear_all_partial_lh()
    ref = fresh.compute_likelihood()
    assert np.isfinite(ref) and abs(lnl - ref) <= 1e-9 * abs(ref), (lnl, ref)   # LNL_RTOL of tests/test_parity_gpu.py
    fresh.close()
    t.close()


# ---- command line ---------------------------------------------------------------------------------------------------------
def test_parstree_command_line(pkg, tmp_path):
    import os
    import re
    import subprocess
    here = os.path.dirname(os.path.abspath(__file__))
    binary = os.path.join(os.path.dirname(here), "iq-tree_amd", "lib", "iqhip_lnl")
    example = os.path.join(here, "golden", "example.phy")
    model = "GTR{1.513,2.393,1.769,1.912,2.838}+F{0.249,0.262,0.251,0.238}+G4{0.934}"
    pre = str(tmp_path / "p")
    r = subprocess.run([binary, "-s", example, "-m", model, "-parstree", "-seed", "1", "-pre", pre],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"Parsimony score: (\d+) \(based on (\d+) informative sites\)", r.stdout)
    assert m, r.stdout
    nwk = open(pre + ".parstree").read().strip()
    aln = pkg.Alignment(example)
    st, fr, _, _ = aln.arrays()
    assert int(m.group(2)) == aln.num_informative_sites
    t = pkg.PhyloTree(nwk, aln.seq_names)
    t.set_alignment(4, 0, st, fr)
    t.set_model(aln.build_model(model))
    t.set_likelihood_kernel(pkg.LK_EIGEN_HIP)
    t.attach_engine(0)
    assert t.compute_parsimony() == int(m.group(1))
    t.close()
    lnl = re.findall(r"Log-likelihood[^:]*: (\S+)", r.stdout)
    assert len(lnl) == 2
    r2 = subprocess.run([binary, "-s", example, "-m", model, "-te", pre + ".parstree", "-pars", "-pre", pre + "2"],
                        capture_output=True, text=True, timeout=120)
    assert r2.returncode == 0, r2.stdout + r2.stderr
    assert re.findall(r"Log-likelihood[^:]*: (\S+)", r2.stdout) == lnl
    m2 = re.search(r"Parsimony score: (\d+) \(based on (\d+) informative sites\)", r2.stdout)
    assert m2 and m2.groups() == m.groups()
