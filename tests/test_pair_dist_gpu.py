"""Pairwise maximum-likelihood distances on the device (include/iqhip.h "pairwise maximum-likelihood distances"):
iqhip_pair_counts against restate_counts (exactly), iqhip_pair_distances against restate_solve of
tests/test_pair_dist_host.py with the acceptance of tests/test_solver_paths_gpu.py (equal numbers of derivative
evaluations, optimum to 1e-9, d2l to 1e-6), the chunking, the agreement with the tree kernels, the refusals, and
PhyloTree.compute_dist / `iqhip_lnl -mldist` end to end.

Every distance case (test_pair_dist_host.dist_case) holds two identical sequences (optimum at x1), a sequence of unknown
states only (distance 9 after one evaluation), a sequence of independent random states (JC start 9, the solve ends in the
upper half of the bracket), a pair that takes a bisection step and a non-zero initial distance; a counter asserts that
each occurred.  The guard of restate_solve rejects an input whose evaluation count could legitimately differ; the seeds
were chosen on the CPU so that it rejects none."""
import collections
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from test_pair_dist_host import (KINDS, MAX_GENETIC_DIST, MAX_STEPS, SHAPES, X1, X2, XACC, all_pairs, assert_case_stats,
                                 dist_case, restate_counts, restate_matrix)

pytestmark = pytest.mark.gpu

IQHIP_ERR_INVALID, IQHIP_ERR_UNSUPPORTED = 2, 3
HERE = os.path.dirname(os.path.abspath(__file__))
BIN = os.path.join(os.path.dirname(HERE), "iq-tree_amd", "lib", "iqhip_lnl")
EXAMPLE = os.path.join(HERE, "golden", "example.phy")
MODEL = "GTR{1.513,2.393,1.769,1.912,2.838}+F{0.249,0.262,0.251,0.238}+G4{0.934}"
DP, I32P = C.POINTER(C.c_double), C.POINTER(C.c_int32)


# ------------------------------------------------------------------------------------------
# engines
# ------------------------------------------------------------------------------------------
class RawEngine:
    """an engine made through the C ABI alone (two taxa make no tree for the host mirror)"""

    def __init__(self, pkg, synth, n, ntaxa, states, freq):
        self.lib, self.n = pkg.libiqhip(), n
        model = synth.gtr_model(alpha=0.9, ncat=4) if n == 4 else synth.random_reversible_model(n, 3, alpha=0.9, ncat=2)
        unknown = {4: 18, 20: 23, 64: 64}[n]
        self.e = C.c_void_p()
        assert self.lib.iqhip_create(C.byref(self.e), 0, n, model.ncat, states.shape[1], ntaxa) == 0, self.lib.iqhip_last_error()
        tip = np.ones((unknown + 1, n))
        tip[:n] = np.eye(n)
        arr = [np.ascontiguousarray(x, dtype=np.float64) for x in (model.eval, model.evec, model.inv_evec, model.rates, model.props, tip)]
        assert self.lib.iqhip_set_model(self.e, *[a.ctypes.data_as(DP) for a in arr[:5]], unknown, arr[5].ctypes.data_as(DP)) == 0
        st = np.ascontiguousarray(states, dtype=np.uint8)
        fr, iv = np.ascontiguousarray(freq, dtype=np.float64), np.zeros(states.shape[1])
        assert self.lib.iqhip_set_alignment(self.e, st.ctypes.data_as(C.POINTER(C.c_uint8)), fr.ctypes.data_as(DP),
                                            iv.ctypes.data_as(DP)) == 0, self.lib.iqhip_last_error()

    def pair_counts(self, pairs):
        pr = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
        out = np.full((pr.shape[0], self.n, self.n), -1.0)
        rc = self.lib.iqhip_pair_counts(self.e, pr.ctypes.data_as(I32P), pr.shape[0], out.ctypes.data_as(DP))
        assert rc == 0, self.lib.iqhip_last_error()
        return out

    def close(self):
        self.lib.iqhip_destroy(self.e)


def tree_engine(pkg, synth, n, seq_type, states, freq, model, sharded=0):
    t = pkg.PhyloTree(synth.random_tree_newick(states.shape[0], 1))
    t.set_alignment(n, seq_type, states, freq)
    t.set_model(model)
    t.set_likelihood_kernel(pkg.LK_EIGEN_HIP)
    if sharded:
        t.attach_engine_sharded([0] * sharded, pkg.REDUCE_HOST)
    else:
        t.attach_engine(0)
    return t


def device_dist(pkg, t, init=None, x1=X1, x2=X2, xacc=XACC, max_steps=MAX_STEPS):
    """iqhip_pair_distances -> (status, dist, d2l, nsteps)"""
    T = t.num_leaves
    dist, d2l, nst = np.full((T, T), -1.0), np.full((T, T), -1.0), np.full((T, T), -1, dtype=np.int32)
    ini = None if init is None else np.ascontiguousarray(init, dtype=np.float64)
    rc = pkg.libiqhip().iqhip_pair_distances(t.engine, None if ini is None else ini.ctypes.data_as(DP), x1, x2, xacc, max_steps,
                                             dist.ctypes.data_as(DP), d2l.ctypes.data_as(DP), nst.ctypes.data_as(I32P))
    return rc, dist, d2l, nst


# ------------------------------------------------------------------------------------------
# counts
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nptn", [1, 63, 64, 65, 1000])
@pytest.mark.parametrize("ntaxa", [2, 3, 5, 17])
@pytest.mark.parametrize("n", [4, 20, 64])
def test_counts_equal_the_restatement(pkg, synth, monkeypatch, n, ntaxa, nptn):
    rng = np.random.default_rng(n * 100003 + ntaxa * 1009 + nptn)
    unknown = {4: 18, 20: 23, 64: 64}[n]
    states = rng.integers(0, n, size=(ntaxa, nptn))
    # close sequences: most columns show one state in every taxon, as real alignments do
    same = rng.random(nptn) < 0.6
    states[:, same] = states[0, same]
    amb = rng.random(states.shape) < 0.1
    states[amb] = rng.integers(n, unknown + 1, size=int(amb.sum()))
    states = states.astype(np.uint8)
    freq = rng.integers(0, 10, size=nptn).astype(np.float64)
    freq[nptn - nptn // 8:] = 0.0                               # a tail of zero-frequency patterns (+ASC)
    eng = RawEngine(pkg, synth, n, ntaxa, states, freq)
    pairs = np.array([(i, j) for i in range(ntaxa) for j in range(ntaxa) if i != j])
    pairs = pairs[rng.permutation(len(pairs))]                  # scrambled, both (i, j) and (j, i)
    assert len(pairs) == 2 * [1, 3, 10, 136][[2, 3, 5, 17].index(ntaxa)]
    got = eng.pair_counts(pairs)
    want = restate_counts(states, freq, n, pairs)
    np.testing.assert_array_equal(got, want)
    where = {tuple(p): k for k, p in enumerate(pairs.tolist())}
    for (i, j), k in where.items():
        np.testing.assert_array_equal(got[k], got[where[(j, i)]].T)
    again = eng.pair_counts(pairs)
    assert again.tobytes() == got.tobytes()
    monkeypatch.setenv("IQHIP_PAIR_CHUNK", "7")                 # (read per call) several chunks, tiles cut by their ends
    assert eng.pair_counts(pairs).tobytes() == got.tobytes()
    # the upper triangle alone, in order: the list iqhip_pair_distances counts
    upper = np.array(all_pairs(ntaxa))
    np.testing.assert_array_equal(eng.pair_counts(upper), restate_counts(states, freq, n, upper))
    eng.close()


# ------------------------------------------------------------------------------------------
# distances
# ------------------------------------------------------------------------------------------
_cases = {}


def solved_case(pkg, synth, kind, shape):
    """the case, and its restated solution computed once"""
    if (kind, shape) not in _cases:
        n, seq_type, states, freq, model, init = dist_case(pkg, synth, kind, *shape)
        stats = collections.Counter()
        ref = restate_matrix(states, freq, model, init, stats)
        assert_case_stats(stats, shape[0])
        _cases[(kind, shape)] = (n, seq_type, states, freq, model, init, ref)
    return _cases[(kind, shape)]


def assert_matches(got, ref, T):
    (dist, d2l, nst), (rdist, rd2l, rnst) = got, ref
    for (i, j) in all_pairs(T):
        print((i, j), dist[i, j], rdist[i, j], d2l[i, j], rd2l[i, j], nst[i, j], rnst[i, j])
        assert nst[i, j] == rnst[i, j], (i, j, nst[i, j], rnst[i, j])
        assert abs(dist[i, j] - rdist[i, j]) <= 1e-9 * max(1.0, abs(rdist[i, j])), (i, j, dist[i, j], rdist[i, j])
        assert abs(d2l[i, j] - rd2l[i, j]) <= 1e-6 * max(1.0, abs(rd2l[i, j])), (i, j, d2l[i, j], rd2l[i, j])
    for m in (dist, d2l, nst):
        np.testing.assert_array_equal(m, m.T)
        assert not np.diag(m).any()


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("kind", KINDS)
def test_distances_match_the_restated_solve(pkg, synth, kind, shape):
    n, seq_type, states, freq, model, init, ref = solved_case(pkg, synth, kind, shape)
    T = shape[0]
    t = tree_engine(pkg, synth, n, seq_type, states, freq, model)
    rc, dist, d2l, nst = device_dist(pkg, t, init)
    assert rc == 0, pkg.libiqhip().iqhip_last_error()
    assert_matches((dist, d2l, nst), ref, T)
    assert dist[0, T - 3] == X1                                   # identical sequences
    assert (dist[T - 1, :T - 1] == MAX_GENETIC_DIST).all() and (nst[T - 1, :T - 1] == 1).all()   # no overlap
    # the non-zero initial distance is honoured: from the JC start the same pair takes another walk to the same optimum
    # (each result lies within xacc of it) and stops at other bits; every other pair is untouched
    rc, dist0, _, _ = device_dist(pkg, t, None)
    assert rc == 0 and dist0[0, 1] != dist[0, 1] and abs(dist0[0, 1] - dist[0, 1]) <= 2 * XACC
    mask = np.ones((T, T), dtype=bool)
    mask[0, 1] = mask[1, 0] = False
    assert dist0[mask].tobytes() == dist[mask].tobytes()
    t.close()


def test_chunks_do_not_change_a_bit(pkg, synth, monkeypatch):
    n, seq_type, states, freq, model, init, _ = solved_case(pkg, synth, "gtr_g4", SHAPES[1])
    t = tree_engine(pkg, synth, n, seq_type, states, freq, model)
    rc, dist, d2l, nst = device_dist(pkg, t, init)
    assert rc == 0
    for chunk in ("37", "1"):                                    # 136 pairs in 4 chunks / one pair per chunk
        monkeypatch.setenv("IQHIP_PAIR_CHUNK", chunk)
        rc, dist_c, d2l_c, nst_c = device_dist(pkg, t, init)
        assert rc == 0
        assert dist_c.tobytes() == dist.tobytes() and d2l_c.tobytes() == d2l.tobytes() and nst_c.tobytes() == nst.tobytes()
    t.close()


def test_asc_engine_ignores_the_unobserved_patterns(pkg, synth):
    """+ASC: the unobserved constant patterns are appended with frequency 0 and contribute nothing to any pair"""
    n, seq_type, states, freq, model, init, ref = solved_case(pkg, synth, "gtr_g4", SHAPES[0])
    T = SHAPES[0][0]
    unobs = np.repeat(np.arange(4, dtype=np.uint8)[None, :], T, axis=0)
    t = pkg.PhyloTree(synth.random_tree_newick(T, 1))
    t.set_alignment(n, seq_type, np.concatenate([states, unobs], axis=1), np.concatenate([freq, np.zeros(4)]))
    t.set_ascertainment(4, float(freq.sum()))
    t.set_model(model)
    t.set_likelihood_kernel(pkg.LK_EIGEN_HIP)
    t.attach_engine(0)
    rc, dist, d2l, nst = device_dist(pkg, t, init)
    assert rc == 0, pkg.libiqhip().iqhip_last_error()
    assert_matches((dist, d2l, nst), ref, T)
    t.close()


def test_agrees_with_the_tree_kernels(pkg, synth):
    """(0:a, 1:x1, 2:c) with taxon 2 unknown everywhere and no ambiguous state in taxa 0 and 1: the tree's likelihood of a
    pattern is pi[s0] * sum_c props[c] P_c[s0][s1](a + x1), the pair's function up to the constant pi[s0].  So the optimum
    a* of branch (0, centre) satisfies a* + x1 = d*, the optimum of the pair.  minimizeNewton returns the iterate before
    its first step shorter than xacc, which is within |dx| (1 + O(dx)) < xacc (1 + 1e-2) of the optimum; two such results:
    |a + x1 - dist[0, 1]| <= 2.02 xacc, xacc = x1 = 1e-6."""
    model = synth.gtr_model(alpha=0.9, ncat=4)
    st = synth.simulate_alignment("(0:0.15,1:0.2,2:0.1);", model, 500, 5)
    st[2] = 18
    pat, freq = synth.compress_patterns(st)
    t = pkg.PhyloTree("(0:0.1,1:%r,2:0.3);" % X1)
    t.set_alignment(4, 0, pat, freq)
    t.set_model(model)
    t.set_likelihood_kernel(pkg.LK_EIGEN_HIP)
    t.attach_engine(0)
    dist = t.compute_dist()
    t.clear_all_partial_lh()
    t.compute_likelihood()
    centre = t.neighbors(0)[0][0]
    a = t.optimize_one_branch(0, centre)
    print(a, dist[0, 1])
    assert 0.1 < dist[0, 1] < 1.0
    assert abs(a + X1 - dist[0, 1]) <= 2.02 * XACC
    t.close()


# ------------------------------------------------------------------------------------------
# refusals
# ------------------------------------------------------------------------------------------
def refused(pkg, t, want, word, pairs=(0, 1), **kw):
    lib = pkg.libiqhip()
    rc = device_dist(pkg, t, **kw)[0]
    assert rc == want and word in lib.iqhip_last_error(), (rc, lib.iqhip_last_error())
    pr = np.array(pairs, dtype=np.int32)
    out = np.zeros(len(pr) // 2 * 64 * 64)
    return lib.iqhip_pair_counts(t.engine, pr.ctypes.data_as(I32P), len(pr) // 2, out.ctypes.data_as(DP))


def test_refusals(pkg, synth):
    lib = pkg.libiqhip()
    rng = np.random.default_rng(2)
    states = rng.integers(0, 4, size=(5, 200)).astype(np.uint8)   # (a shard holds at least 64 patterns)
    freq = np.ones(200)
    # mixture model
    t = tree_engine(pkg, synth, 4, 0, states, freq, synth.mixture_model(4, 3, 9, ncat=4))
    assert refused(pkg, t, IQHIP_ERR_UNSUPPORTED, b"mixture") == IQHIP_ERR_UNSUPPORTED and b"mixture" in lib.iqhip_last_error()
    t.close()
    # sharded engine
    t = tree_engine(pkg, synth, 4, 0, states, freq, synth.gtr_model(), sharded=2)
    assert refused(pkg, t, IQHIP_ERR_UNSUPPORTED, b"sharded") == IQHIP_ERR_UNSUPPORTED and b"sharded" in lib.iqhip_last_error()
    t.close()
    # embedded state count: iqhip_create(2, ...)
    t = pkg.PhyloTree(synth.random_tree_newick(5, 1))
    t.set_alignment(2, 3, (states & 1).astype(np.uint8), freq)
    t.set_model(synth.random_reversible_model(2, 4, alpha=0.7, ncat=4))
    t.set_likelihood_kernel(pkg.LK_EIGEN_HIP)
    t.attach_engine(0)
    assert refused(pkg, t, IQHIP_ERR_UNSUPPORTED, b"states") == IQHIP_ERR_UNSUPPORTED and b"states" in lib.iqhip_last_error()
    t.close()
    # arguments
    t = tree_engine(pkg, synth, 4, 0, states, freq, synth.gtr_model())
    assert refused(pkg, t, IQHIP_ERR_INVALID, b"max_steps", pairs=(0, 5), max_steps=0) == IQHIP_ERR_INVALID
    assert b"outside" in lib.iqhip_last_error()
    assert refused(pkg, t, IQHIP_ERR_INVALID, b"x1 <= x2", pairs=(-1, 0), x1=2.0, x2=1.0) == IQHIP_ERR_INVALID
    assert device_dist(pkg, t)[0] == 0                           # and the engine still works
    t.close()


# ------------------------------------------------------------------------------------------
# end to end
# ------------------------------------------------------------------------------------------
def test_compute_dist_python_and_command_line(pkg, synth, tmp_path):
    aln = pkg.Alignment(EXAMPLE)
    st, fr, _, _ = aln.arrays()
    model = aln.build_model(MODEL)
    T = st.shape[0]
    nwk = synth.random_tree_newick(T, 12)
    t = pkg.PhyloTree(nwk)
    t.set_alignment(4, 0, st, fr)
    t.set_model(model)
    t.attach_engine(0)
    dist, d2l = t.compute_dist(want_d2l=True)
    rdist, rd2l, _ = restate_matrix(st, fr, model)
    for (i, j) in all_pairs(T):
        assert abs(dist[i, j] - rdist[i, j]) <= 1e-9 * max(1.0, abs(rdist[i, j])), (i, j, dist[i, j], rdist[i, j])
        assert abs(d2l[i, j] - rd2l[i, j]) <= 1e-6 * max(1.0, abs(rd2l[i, j])), (i, j, d2l[i, j], rd2l[i, j])
    np.testing.assert_array_equal(dist, dist.T)
    assert not np.diag(dist).any()
    np.testing.assert_array_equal(t.pair_counts([(3, 7), (7, 3)]), restate_counts(st, fr, 4, [(3, 7), (7, 3)]))
    t.close()
    names = aln.seq_names
    tf = tmp_path / "t.nwk"
    tf.write_text(re.sub(r"([(,])(\d+):", lambda m: "%s%s:" % (m.group(1), names[int(m.group(2))]), nwk) + "\n")
    out = tmp_path / "x.mldist"
    r = subprocess.run([BIN, "-s", EXAMPLE, "-te", str(tf), "-m", MODEL, "-pre", str(tmp_path / "x"), "-blfix", "-mldist", str(out)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr + r.stdout
    lines = out.read_text().split("\n")
    assert lines[0] == str(T) and lines[-1] == "" and len(lines) == T + 2
    width = max(10, max(len(s) for s in names))
    for i, ln in enumerate(lines[1:T + 1]):
        assert ln[:width + 1] == names[i].ljust(width) + " " and ln.endswith(" ")
        vals = ln[width + 1:].split(" ")
        assert vals[-1] == "" and len(vals) == T + 1
        assert vals[:T] == ["%.7f" % v for v in dist[i]], (i, vals[:3])
