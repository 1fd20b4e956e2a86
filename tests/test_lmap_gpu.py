"""Likelihood mapping on the device (include/iqhip.h "Likelihood mapping") against tests/lmap_ref.py:
iqhip_quartet_cells exactly; iqhip_quartet_likelihoods over all 15 quartets of each 6-taxon case of lmap_ref.CASES with equal
numbers of sweeps and of derivative evaluations, logl to 1e-8 relative (the sweep tolerance of tests/test_sweep_gpu.py) and
lengths to rtol 1e-7 / atol 1e-12 (tests/test_solver_paths_gpu.py); the same quartets through the existing route (a 4-taxon
PhyloTree per quartet tree on the traversal kernels); bit-identical results across calls and chunkings; every refusal;
likelihood_mapping and `iqhip_lnl -lmap` end to end.

Every likelihood case holds two identical sequences (lengths ending at x1), a sequence of independent random states
(diverged solves / lengths in the upper bracket), a gap-only taxon, ambiguity codes, three columns of unknowns only (the
all-unknown item, with a constant cell, under +I), quartet trees that need more than one sweep and, with iterations = 1,
trees that stop at the limit; counters assert that each occurred.  lmap_ref's guard flags a quartet tree whose discrete
decisions could legitimately differ between two correct implementations; the seeds of lmap_ref.CASES were chosen on the CPU
with lmap_ref alone so that it flags none."""
import ctypes as C
import functools
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import lmap_ref

pytestmark = pytest.mark.gpu

IQHIP_ERR_INVALID, IQHIP_ERR_UNSUPPORTED = 2, 3
HERE = os.path.dirname(os.path.abspath(__file__))
BIN = os.path.join(os.path.dirname(HERE), "iq-tree_amd", "lib", "iqhip_lnl")
EXAMPLE = os.path.join(HERE, "golden", "example.phy")
MODEL = "GTR{1.513,2.393,1.769,1.912,2.838}+F{0.249,0.262,0.251,0.238}+G4{0.934}"   # tests/test_pair_dist_gpu.py
DP, I32P = C.POINTER(C.c_double), C.POINTER(C.c_int32)
X1, X2 = lmap_ref.X1, lmap_ref.X2
QUARTETS6 = list(itertools.combinations(range(6), 4))


def tree_engine(pkg, synth, states, freq, model, nstates=4, seq_type=0, sharded=0, n_unobs=0):
    t = pkg.PhyloTree(synth.random_tree_newick(states.shape[0], 1))
    t.set_alignment(nstates, seq_type, states, freq)
    if n_unobs:
        t.set_ascertainment(n_unobs, float(np.sum(freq)))
    t.set_model(model)
    t.set_likelihood_kernel(pkg.LK_EIGEN_HIP)
    if sharded:
        t.attach_engine_sharded([0] * sharded, pkg.REDUCE_HOST)
    else:
        t.attach_engine(0)
    return t


def raw_likelihoods(pkg, t, quartets, const_invar=None, x1=X1, x2=X2, xacc=X1, max_steps=100, diverge=0.95, iterations=10,
                    tolerance=0.1, null_results=False):
    """iqhip_quartet_likelihoods through the C ABI -> (status, records); the records start as a pattern of 0xA5 bytes"""
    q = np.ascontiguousarray(quartets, dtype=np.int32).reshape(-1, 4)
    out = np.frombuffer(b"\xa5" * (pkg.QUARTET_RESULT_DTYPE.itemsize * max(1, q.shape[0])), dtype=pkg.QUARTET_RESULT_DTYPE).copy()
    ci = None if const_invar is None else np.ascontiguousarray(const_invar, dtype=np.float64)
    rc = pkg.libiqhip().iqhip_quartet_likelihoods(t.engine, q.ctypes.data_as(I32P) if q.size else None, q.shape[0],
                                                  None if ci is None else ci.ctypes.data_as(DP), x1, x2, xacc, max_steps, diverge,
                                                  iterations, tolerance, None if null_results else out.ctypes.data_as(C.c_void_p))
    return rc, out


# ------------------------------------------------------------------------------------------
# 1. cells
# ------------------------------------------------------------------------------------------
def random_alignment(rng, ntaxa, nptn, amb=0.1):
    st = rng.integers(0, 4, size=(ntaxa, nptn))
    same = rng.random(nptn) < 0.6
    st[:, same] = st[0, same]
    if amb:
        m = rng.random(st.shape) < amb
        st[m] = rng.integers(4, 19, size=int(m.sum()))
    freq = rng.integers(0, 9, size=nptn).astype(np.float64)      # some patterns of frequency 0: dropped
    freq[0] = max(freq[0], 1.0)
    return st.astype(np.uint8), freq


def check_cells(pkg, synth, states, freq, quartets):
    t = tree_engine(pkg, synth, states, freq, synth.gtr_model())
    cells, nother = t.quartet_cells(quartets)
    t.close()
    lengths = []
    for q, c, n in zip(quartets, cells, nother):
        rc, rother = lmap_ref.cells_ref(states, freq, q)
        assert np.array_equal(c, rc), q
        assert n == len(rother), (q, n, len(rother))
        lengths.append(int(n))
    return lengths


@pytest.mark.parametrize("nptn", [1, 63, 64, 65, 150])
def test_cells_equal_the_restatement(pkg, synth, nptn):
    rng = np.random.default_rng(1000 + nptn)
    states, freq = random_alignment(rng, 7, nptn)
    quartets = [tuple(int(x) for x in rng.permutation(7)[:4]) for _ in range(9)] + [(0, 1, 2, 3), (6, 5, 4, 3)]
    check_cells(pkg, synth, states, freq, quartets)


def test_cells_other_list_empty_full_and_long(pkg, synth):
    rng = np.random.default_rng(7)
    states, freq = random_alignment(rng, 6, 150, amb=0.0)
    freq[:] = rng.integers(1, 9, size=150)
    assert check_cells(pkg, synth, states, freq, [(0, 1, 2, 3), (5, 3, 1, 0)]) == [0, 0]           # no other pattern at all
    states[4] = 18                                                                                 # a gap-only taxon
    assert check_cells(pkg, synth, states, freq, [(0, 4, 2, 3), (0, 1, 2, 3)]) == [150, 0]         # every pattern / none
    states, freq = random_alignment(rng, 6, 400, amb=0.0)
    freq[:] = rng.integers(1, 9, size=400)
    gappy = rng.random(400) < 0.8
    states[2, gappy] = rng.integers(4, 19, size=int(gappy.sum()))                                  # one gappy taxon
    n = check_cells(pkg, synth, states, freq, [(0, 1, 2, 3), (2, 5, 4, 0), (0, 1, 3, 4)])
    assert n[0] > 256 and n[1] == n[0] and n[2] == 0


# ------------------------------------------------------------------------------------------
# 2. likelihoods against the restatement
# ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def reference(name, iterations):
    """the restatement of every quartet tree of a case, computed once"""
    from conftest import load_package
    import importlib
    import sys
    load_package()
    synth = importlib.import_module("iqtree_amd.synth")
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))
    import oracle_driver as od
    case = lmap_ref.lmap_case(synth, name)
    out = {}
    for q in QUARTETS6:
        for k in range(3):
            out[(q, k)] = lmap_ref.quartet_tree_ref(od, case["states"], case["freq"], q, k, case["model"], case["nsite"], iterations,
                                                    0.1, case["const_invar"])
    return case, out


def compare(res, ref, what):
    for qi, q in enumerate(QUARTETS6):
        for k in range(3):
            r = ref[(q, k)]
            assert not r["guard"], ("change the seed", what, q, k, r["guard"])
            assert res["status"][qi, k] == 0
            print(what, q, k, "sweeps", res["nsweeps"][qi, k], r["nsweeps"], "evals", res["neval"][qi, k], r["neval"], "logl",
                  res["logl"][qi, k], r["logl"])
            assert (res["nsweeps"][qi, k], res["neval"][qi, k]) == (r["nsweeps"], r["neval"]), (what, q, k)
            assert abs(res["logl"][qi, k] - r["logl"]) <= 1e-8 * abs(r["logl"]), (what, q, k, res["logl"][qi, k], r["logl"])
            np.testing.assert_allclose(res["len"][qi, k], r["len"], rtol=1e-7, atol=1e-12, err_msg=str((what, q, k)))


@pytest.mark.parametrize("name", list(lmap_ref.CASES))
def test_likelihoods_equal_the_restatement(pkg, synth, name):
    case, ref = reference(name, 10)
    _, ref1 = reference(name, 1)
    states, freq = case["states"], case["freq"]
    # what the case holds
    assert np.array_equal(states[0], states[1]) and np.all(states[5] == 18)
    assert np.any((states[2:4] >= 4) & (states[2:4] < 18)) and np.any(np.all(states == 18, axis=0))
    stats = {key: sum(r["stats"][key] for r in ref.values()) for key in ("lower", "upper", "diverged")}
    assert stats["lower"] >= 1 and stats["upper"] + stats["diverged"] >= 1, stats
    assert sum(r["nsweeps"] > 1 for r in ref.values()) >= 1 and sum(r["stats"]["limit"] for r in ref1.values()) >= 1
    if case["const_invar"] is not None:
        cc = np.concatenate([lmap_ref.const_char_of(lmap_ref.sub_alignment(states, freq, q)[0]) for q in QUARTETS6])
        assert np.any(cc == 4) and np.any((cc >= 0) & (cc < 4))
    t = tree_engine(pkg, synth, states, freq, case["model"])
    assert t.ncat == {"jc": 1, "gtr_g4": 4, "gtr_i_g4": 4, "hky_r3": 3, "wide10": 10}[name]
    res = t.quartet_likelihoods(QUARTETS6, const_invar=case["const_invar"])
    res1 = t.quartet_likelihoods(QUARTETS6, iterations=1, const_invar=case["const_invar"])
    t.close()
    compare(res, ref, name)
    compare(res1, ref1, name + " (one sweep)")
    assert np.all(res1["nsweeps"] == 1)


# ------------------------------------------------------------------------------------------
# 3. the same quartets on the traversal kernels
# ------------------------------------------------------------------------------------------
def test_likelihoods_equal_the_existing_route(pkg, synth):
    case, _ = reference("gtr_g4", 10)
    states, freq, model = case["states"], case["freq"], case["model"]
    quartets = [QUARTETS6[i] for i in (0, 4, 7, 11, 14)]
    t = tree_engine(pkg, synth, states, freq, model)
    res = t.quartet_likelihoods(quartets)
    # one Newton step per solve and one sweep: every solve hands back the length it started from
    rc, start = raw_likelihoods(pkg, t, quartets, max_steps=1, iterations=1)
    assert rc == 0
    t.close()
    for qi, q in enumerate(quartets):
        for k in range(3):
            taxa = [q[lmap_ref.QC[4 * k + j]] for j in range(4)]
            cols, w = lmap_ref.sub_alignment(states, freq, taxa)
            # the sub-alignment keeps the site count of the whole alignment: nsite of the starting lengths
            assert w.sum() == freq.sum()
            old = pkg.PhyloTree("(0:0.1,1:0.1,(2:0.1,3:0.1):0.1);")
            old.set_alignment(4, 0, cols, w)
            old.set_model(model)
            old.set_likelihood_kernel(pkg.LK_EIGEN_HIP)
            old.attach_engine(0)
            old.set_device_sweep(False)
            assert old.fix_negative_branch() == 5
            lens = [dict(old.neighbors(a))[b] for a, b in ((0, 4), (1, 4), (2, 5), (3, 5), (4, 5))]
            np.testing.assert_allclose(start["len"][qi, k], lens, rtol=1e-12, atol=0, err_msg=str((q, k)))
            old.initialize_all_partial_lh()
            old.clear_all_partial_lh()
            lnl = old.optimize_all_branches(10, 0.1)
            old.close()
            print(q, k, "logl", res["logl"][qi, k], lnl)
            assert abs(res["logl"][qi, k] - lnl) <= 1e-8 * abs(lnl), (q, k, res["logl"][qi, k], lnl)


# ------------------------------------------------------------------------------------------
# 4. reproducibility
# ------------------------------------------------------------------------------------------
def test_results_are_bit_identical_across_calls_and_chunkings(pkg, synth, monkeypatch):
    case, _ = reference("gtr_i_g4", 10)
    t = tree_engine(pkg, synth, case["states"], case["freq"], case["model"])
    quartets = QUARTETS6 + [tuple(reversed(q)) for q in QUARTETS6[:5]]
    monkeypatch.delenv("IQHIP_QUARTET_CHUNK", raising=False)
    first = t.quartet_likelihoods(quartets, const_invar=case["const_invar"])
    cells = t.quartet_cells(quartets)
    assert first.tobytes() == t.quartet_likelihoods(quartets, const_invar=case["const_invar"]).tobytes()
    for chunk in ("1", "7"):
        monkeypatch.setenv("IQHIP_QUARTET_CHUNK", chunk)     # (read per call)
        assert first.tobytes() == t.quartet_likelihoods(quartets, const_invar=case["const_invar"]).tobytes(), chunk
        again = t.quartet_cells(quartets)
        assert np.array_equal(cells[0], again[0]) and np.array_equal(cells[1], again[1])
    t.close()
    assert np.all(first["_pad"] == 0)


# ------------------------------------------------------------------------------------------
# 5. refusals
# ------------------------------------------------------------------------------------------
def refused(pkg, t, code, text, **kw):
    quartets = kw.pop("quartets", [(0, 1, 2, 3)])
    rc, out = raw_likelihoods(pkg, t, quartets, **kw)
    assert rc == code, (rc, code, pkg.libiqhip().iqhip_last_error())
    assert text in pkg.libiqhip().iqhip_last_error(), (text, pkg.libiqhip().iqhip_last_error())
    assert out.tobytes() == b"\xa5" * out.nbytes                 # nothing was launched: the results are untouched
    q = np.ascontiguousarray(quartets, dtype=np.int32).reshape(-1, 4)
    cells, nother = np.full((max(1, q.shape[0]), 256), -1.0), np.full(max(1, q.shape[0]), -1, dtype=np.int32)
    rc2 = pkg.libiqhip().iqhip_quartet_cells(t.engine, q.ctypes.data_as(I32P) if q.size else None, q.shape[0],
                                             cells.ctypes.data_as(DP), nother.ctypes.data_as(I32P))
    return rc2, cells, nother


def test_refusals(pkg, synth):
    lib = pkg.libiqhip()
    rng = np.random.default_rng(3)
    states, freq = random_alignment(rng, 6, 200)                 # (a shard holds at least 64 patterns)
    freq[:] = 1.0
    # 20 states
    t = tree_engine(pkg, synth, rng.integers(0, 20, size=(6, 50)).astype(np.uint8), np.ones(50),
                    synth.random_reversible_model(20, 3, alpha=0.9, ncat=4), nstates=20, seq_type=1)
    assert refused(pkg, t, IQHIP_ERR_UNSUPPORTED, b"4 states")[0] == IQHIP_ERR_UNSUPPORTED
    t.close()
    # mixture model
    t = tree_engine(pkg, synth, states, freq, synth.mixture_model(4, 3, 9, ncat=4))
    assert refused(pkg, t, IQHIP_ERR_UNSUPPORTED, b"mixture")[0] == IQHIP_ERR_UNSUPPORTED
    t.close()
    # +ASC: the four constant patterns appended as unobserved
    asc = np.concatenate([states, np.tile(np.arange(4, dtype=np.uint8), (6, 1))], axis=1)
    t = tree_engine(pkg, synth, asc, np.concatenate([freq, np.zeros(4)]), synth.gtr_model(), n_unobs=4)
    assert refused(pkg, t, IQHIP_ERR_UNSUPPORTED, b"ASC")[0] == IQHIP_ERR_UNSUPPORTED
    t.close()
    # sharded engine
    t = tree_engine(pkg, synth, states, freq, synth.gtr_model(), sharded=2)
    assert refused(pkg, t, IQHIP_ERR_UNSUPPORTED, b"sharded")[0] == IQHIP_ERR_UNSUPPORTED
    t.close()
    # embedded state count: iqhip_create(2, ...)
    t = tree_engine(pkg, synth, rng.integers(0, 2, size=(6, 40)).astype(np.uint8), np.ones(40),
                    synth.random_reversible_model(2, 4, alpha=0.7, ncat=4), nstates=2, seq_type=3)
    assert refused(pkg, t, IQHIP_ERR_UNSUPPORTED, b"4 states")[0] == IQHIP_ERR_UNSUPPORTED
    t.close()
    # arguments
    t = tree_engine(pkg, synth, states, freq, synth.gtr_model())
    inv = IQHIP_ERR_INVALID
    assert refused(pkg, t, inv, b"nq >= 1", quartets=[])[0] == inv
    assert refused(pkg, t, inv, b"outside", quartets=[(0, 1, 2, 6)])[0] == inv
    assert refused(pkg, t, inv, b"outside", quartets=[(0, 1, 2, 3), (-1, 1, 2, 3)])[0] == inv
    assert refused(pkg, t, inv, b"twice", quartets=[(0, 1, 2, 3), (4, 1, 2, 4)])[0] == inv
    assert refused(pkg, t, inv, b"x1 <= x2", x1=2.0, x2=1.0)[0] == 0
    assert refused(pkg, t, inv, b"max_steps", max_steps=0)[0] == 0
    assert refused(pkg, t, inv, b"iterations", iterations=0)[0] == 0
    assert refused(pkg, t, inv, b"tolerance", tolerance=-0.1)[0] == 0
    assert refused(pkg, t, inv, b"tolerance", tolerance=float("nan"))[0] == 0
    rc, _ = raw_likelihoods(pkg, t, [(0, 1, 2, 3)], null_results=True)
    assert rc == inv and b"null" in lib.iqhip_last_error()
    assert lib.iqhip_quartet_likelihoods(None, None, 1, None, X1, X2, X1, 100, 0.95, 10, 0.1, None) == inv
    assert lib.iqhip_quartet_cells(t.engine, None, 1, None, None) == inv
    # a non-integer pattern frequency
    f2 = freq.copy()
    f2[3] = 1.5
    t.set_ptn_freq(f2)
    with pytest.raises(pkg.HostError, match="integers"):
        t.quartet_cells([(0, 1, 2, 3)])                          # (the mirror pushes its inputs, then the engine refuses)
    assert refused(pkg, t, inv, b"integers")[0] == inv
    t.set_ptn_freq(freq)
    assert t.quartet_cells([(0, 1, 2, 3)])[0].sum() + t.quartet_cells([(0, 1, 2, 3)])[1][0] == 200
    rc, out = raw_likelihoods(pkg, t, [(0, 1, 2, 3)])            # and the engine still works
    assert rc == 0 and np.all(out["nsweeps"] >= 1) and np.all(np.isfinite(out["logl"]))
    t.close()
    # planning-only engine; an engine without alignment and model
    e = C.c_void_p()
    assert lib.iqhip_debug_create_planner(C.byref(e), 4, 4, 100, 6, 256, 18, 1) == 0, lib.iqhip_last_error()
    q = np.array([0, 1, 2, 3], dtype=np.int32)
    out = np.zeros(1, dtype=pkg.QUARTET_RESULT_DTYPE)
    args = (q.ctypes.data_as(I32P), 1, None, X1, X2, X1, 100, 0.95, 10, 0.1, out.ctypes.data_as(C.c_void_p))
    assert lib.iqhip_quartet_likelihoods(e, *args) == inv and b"planning" in lib.iqhip_last_error()
    lib.iqhip_destroy(e)
    assert lib.iqhip_create(C.byref(e), 0, 4, 4, 100, 6) == 0, lib.iqhip_last_error()
    assert lib.iqhip_quartet_likelihoods(e, *args) == inv and b"first" in lib.iqhip_last_error()
    lib.iqhip_destroy(e)


# ------------------------------------------------------------------------------------------
# 6. likelihood_mapping
# ------------------------------------------------------------------------------------------
def test_likelihood_mapping_on_seven_taxa(pkg, synth):
    model = synth.gtr_model()
    nwk = synth.random_tree_newick(7, 21, lo=0.05, hi=0.5)
    states, freq = synth.compress_patterns(synth.simulate_alignment(nwk, model, 250, 22, 0.03, 18))
    t = tree_engine(pkg, synth, states, freq, model)
    lm = t.likelihood_mapping()
    assert np.array_equal(lm.seq_id, pkg.all_quartets(7)) and lm.seq_id.shape == (35, 4)
    direct = t.quartet_likelihoods(lm.seq_id)
    assert np.array_equal(lm.logl, direct["logl"])
    area, corner = np.zeros(7, dtype=np.int64), np.zeros(3, dtype=np.int64)
    seq = np.zeros((8, 10), dtype=np.int64)
    for q in range(35):
        w, c, a = lmap_ref.region_ref(lm.logl[q])
        assert np.array_equal(lm.qweight[q], w) and (lm.corner[q], lm.area[q]) == (c, a)
        area[a] += 1
        corner[c] += 1
        for row in list(lm.seq_id[q]) + [7]:
            seq[row, a] += 1
            seq[row, 7 + c] += 1
    assert np.array_equal(lm.areacount, area) and np.array_equal(lm.cornercount, corner) and np.array_equal(lm.seq_count, seq)
    assert lm.areacount.sum() == 35 and lm.cornercount.sum() == 35 and lm.seq_count[:7, :7].sum() == 4 * 35
    assert t.likelihood_mapping(nquartets=35).seq_id.shape == (35, 4)           # >= C(7, 4): all unique quartets
    drawn = t.likelihood_mapping(nquartets=10, seed=3)
    assert np.array_equal(drawn.seq_id, pkg.draw_quartets(7, 10, 3))
    assert np.array_equal(drawn.logl, t.quartet_likelihoods(pkg.draw_quartets(7, 10, 3))["logl"])
    assert drawn.areacount.sum() == 10
    cells_ms, solve_ms = t.quartet_timing()
    assert cells_ms == 0.0 and solve_ms == 0.0                                  # (timing was never enabled)
    t.close()
    small = pkg.PhyloTree("(0:0.1,1:0.1,2:0.1);")
    small.set_alignment(4, 0, states[:3], freq)
    small.set_model(model)
    small.set_likelihood_kernel(pkg.LK_EIGEN_HIP)
    small.attach_engine(0)
    with pytest.raises(pkg.HostError, match="at least 4 taxa"):
        small.likelihood_mapping()
    small.close()


# ------------------------------------------------------------------------------------------
# 7. the command line
# ------------------------------------------------------------------------------------------
def test_command_line(pkg, synth, tmp_path):
    aln = pkg.Alignment(EXAMPLE)
    st, fr, _, _ = aln.arrays()
    model = aln.build_model(MODEL)
    T = st.shape[0]
    nwk = synth.random_tree_newick(T, 12)
    names = aln.seq_names
    tf = tmp_path / "t.nwk"
    tf.write_text(re.sub(r"([(,])(\d+):", lambda m: "%s%s:" % (m.group(1), names[int(m.group(2))]), nwk) + "\n")
    r = subprocess.run([BIN, "-s", EXAMPLE, "-te", str(tf), "-m", MODEL, "-pre", str(tmp_path / "x"), "-blfix", "-lmap", "200",
                        "-seed", "1", "-wql"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr + r.stdout
    assert "Computing 200 quartet likelihoods" in r.stdout
    t = pkg.PhyloTree(nwk)
    t.set_alignment(4, 0, st, fr)
    t.set_model(model)
    t.attach_engine(0)
    quartets = pkg.draw_quartets(T, 200, 1)
    res = t.quartet_likelihoods(quartets)
    t.close()
    lines = (tmp_path / "x.lmap.quartetlh").read_text().split("\n")
    assert lines[0] == "SeqIDs\tlh1\tlh2\tlh3\tweight1\tweight2\tweight3" and lines[-1] == "" and len(lines) == 202
    for q, ln in enumerate(lines[1:201]):
        w = lmap_ref.region_ref(res["logl"][q])[0]
        want = ["(%d,%d,%d,%d)" % tuple(quartets[q] + 1)] + ["%g" % v for v in list(res["logl"][q]) + list(w)]
        assert ln.split("\t") == want, (q, ln, want)
    counts = [int(x) for x in re.findall(r"Quartets in region \d: (\d+)", r.stdout)]
    summary = [int(x) for x in re.findall(r"Number of (?:fully resolved |partly resolved|unresolved     ) quartets: (\d+) \(", r.stdout)]
    assert len(counts) == 7 and len(summary) == 3 and sum(summary) == 200 == sum(counts)
    assert summary == [sum(counts[:3]), sum(counts[3:6]), counts[6]]
    areas = np.bincount([lmap_ref.region_ref(res["logl"][q])[2] for q in range(200)], minlength=7)
    assert counts == list(areas)
    pf = tmp_path / "p.nex"
    pf.write_text("JC, all = 1-100\n")
    r = subprocess.run([BIN, "-s", EXAMPLE, "-te", str(tf), "-q", str(pf), "-lmap", "200"], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "-lmap" in r.stderr and "cannot be combined" in r.stderr
