"""GPU: the engine's growable scratch buffers (iqhip_internal.h DevBuf) across growth and across engine lifetimes.

A buffer that grows drops its contents and changes its address.  The other suites mostly use one size per engine, so they do
not pin that a grown buffer is used correctly afterwards.  Here each feature runs small -> large -> small on ONE engine, and
all three results must equal, bit for bit, those of a fresh engine that was given only that call.  A second test runs
create -> every feature once -> close three times and then compares a fourth engine's results with the first's: a double
free or a pointer that outlived its engine shows as a different result, nothing is provoked.

The engine: 9 taxa, 65 patterns (one past the 64-pattern pad), 4 states +G4 and 20 states +G4."""
import numpy as np
import pytest

import fitch_ref as F
from test_parsimony_gpu import all_directed_ops, slot_of

pytestmark = pytest.mark.gpu

NTAXA, NPTN, NROWS, NBOOT = 9, 65, 40, 100
FEATURES = ["tree_tests", "ptnlh_rell", "branch_tests", "pair_counts", "pars_branch_scores"]


def inputs(n):
    """the alignment, the store rows and the parsimony op list of the n-state case (the same for every engine)"""
    rng = np.random.default_rng(1000 + n)
    states = F.random_states(NTAXA, NPTN, n, rng, amb_frac=0.10)
    freq = rng.integers(1, 6, size=NPTN).astype(np.float64)
    rows = rng.uniform(-12.0, -1.0, size=(NROWS, NPTN))
    adj = F.random_tree(NTAXA, rng)
    ops, slot = all_directed_ops(adj, NTAXA)
    ends = [(slot_of(slot, a, b, NTAXA), slot_of(slot, b, a, NTAXA)) for a, b in F.branches(adj)]
    return dict(n=n, states=states, freq=freq, rows=rows, lh=rows @ freq, ops=ops, ends=ends)


def make_engine(pkg, synth, inp):
    n = inp["n"]
    t = pkg.PhyloTree(synth.random_tree_newick(NTAXA, 1))
    t.set_alignment(n, pkg.SEQ_DNA if n == 4 else pkg.SEQ_PROTEIN, inp["states"], inp["freq"])
    t.set_model(synth.gtr_model(alpha=0.9, ncat=4) if n == 4 else synth.random_reversible_model(20, 3, alpha=0.9, ncat=4))
    t.set_likelihood_kernel(pkg.LK_EIGEN_HIP)
    t.attach_engine(0)
    return t


def prepare(t, inp, feature):
    """what a feature's call needs on an engine: the row store and the sample matrix, or the parsimony vectors"""
    done = t.__dict__.setdefault("_prepared", set())
    kind = "pars" if feature == "pars_branch_scores" else "none" if feature == "pair_counts" else "store"
    if kind in done:
        return
    done.add(kind)
    if kind == "store":
        t.ptnlh_reserve(NROWS)
        for r in range(NROWS):
            t.ptnlh_upload(r, inp["rows"][r])
        t.gen_boot_samples(NBOOT, int(inp["freq"].sum()), 7)
    elif kind == "pars":
        t.pars_init()
        t.pars_update(inp["ops"])


def call(t, inp, feature, large):
    """one call of a feature at its small or its large size -> the bytes of everything it returned"""
    prepare(t, inp, feature)
    if feature == "ptnlh_rell":       # 2 rows x 8 samples; 33 rows, one of them a repeat, x 100 samples
        rows, ns = (list(range(32)) + [5], NBOOT) if large else ([3, 1], 8)
        out = [t.ptnlh_rell(rows, ns)]
    elif feature == "branch_tests":   # 1 branch over 2 rows x 8 samples; 11 branches = 33 entries with repeats x 100 samples
        rows3 = (list(range(32)) + [5]) if large else [3, 1, 3]
        out = [t.branch_tests(rows3, inp["lh"][rows3], 100 if large else 8, 100 if large else 8)]
    elif feature == "tree_tests":     # weighted: 2 trees x 8 samples; 17 trees x 100 samples
        rows, ns = (list(range(20, 37)), NBOOT) if large else ([4, 9], 8)
        out = [t.tree_tests(rows, inp["lh"][rows], ns, weighted=True, tie_seed=11)]
    elif feature == "pair_counts":    # 3 pairs; all 36
        pairs = [(i, j) for i in range(NTAXA) for j in range(i + 1, NTAXA)]
        assert len(pairs) == 36
        out = [t.pair_counts(pairs if large else [(7, 2), (0, 8), (4, 5)])]
    else:                             # one end pair; every branch
        assert feature == "pars_branch_scores" and len(inp["ends"]) == 2 * NTAXA - 3
        out = list(t.pars_branch_scores(inp["ends"] if large else inp["ends"][6:7]))
    return b"".join(np.ascontiguousarray(a).tobytes() for a in out)


_inputs, _fresh = {}, {}


def fresh_result(pkg, synth, n, feature, large):
    """the feature's result on an engine that is given only that call (computed once per case)"""
    inp = _inputs.setdefault(n, inputs(n))
    key = (n, feature, large)
    if key not in _fresh:
        t = make_engine(pkg, synth, inp)
        _fresh[key] = call(t, inp, feature, large)
        t.close()
    return inp, _fresh[key]


@pytest.fixture(scope="module", params=[4, 20])
def shared(request, pkg, synth):
    """ONE engine per state count for all features of test_small_large_small"""
    inp = _inputs.setdefault(request.param, inputs(request.param))
    t = make_engine(pkg, synth, inp)
    yield request.param, t
    t.close()


@pytest.mark.parametrize("feature", FEATURES)
def test_small_large_small(pkg, synth, shared, feature):
    n, t = shared
    inp, want_small = fresh_result(pkg, synth, n, feature, False)
    _, want_large = fresh_result(pkg, synth, n, feature, True)
    assert len(want_large) > len(want_small) > 0
    assert call(t, inp, feature, False) == want_small     # first use: every buffer is allocated
    assert call(t, inp, feature, True) == want_large      # the buffers grow: new addresses, old contents dropped
    assert call(t, inp, feature, False) == want_small     # the grown buffers, used below their capacity
    assert call(t, inp, feature, True) == want_large      # ... and at it, without growing


@pytest.mark.parametrize("n", [4, 20])
def test_engine_lifetimes(pkg, synth, n):
    inp = _inputs.setdefault(n, inputs(n))

    def cycle():
        t = make_engine(pkg, synth, inp)
        got = [call(t, inp, f, True) for f in FEATURES]
        t.close()
        return got

    first = cycle()
    assert first == [fresh_result(pkg, synth, n, f, True)[1] for f in FEATURES]
    cycle()
    cycle()
    assert cycle() == first
