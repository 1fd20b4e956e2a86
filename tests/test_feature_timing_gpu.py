"""The timing read-outs of the drivers an engine and a partition group share (iqhip_timing_enable): UFBoot and the pairwise
distances on one engine and on the group, the group's joint Newton solve and its batch.  With timing on, every reading is
finite and > 0 and the launch counts are those tests/test_ufboot_gpu.py, tests/test_partition_ufboot_gpu.py,
tests/test_partition_gpu.py and tests/test_partition_batch_gpu.py assert; with timing never switched on, every reading is
exactly 0.0.  Several chunks per call throughout (IQHIP_UFBOOT_CHUNK, IQHIP_PAIR_CHUNK): a reading is a sum over chunks.

One group of 2 members on 6 taxa, DNA: 1 category with 70 patterns, 4 categories with 130 patterns (a second 64-pattern
tile); 8 bootstrap samples."""
import ctypes as C
import math

import numpy as np
import pytest

import partition_ref as pr
import test_partition_batch_gpu as pb           # make_group, plain_task, single_solve
from test_pair_dist_gpu import device_dist
from test_partition_ufboot_gpu import member_with_patterns

pytestmark = pytest.mark.gpu

NTAXA, NSAMPLES, NROWS = 6, 8, 3
RATES = [1.0, 1.6]
SHAPES = [(1, 70), (4, 130)]                    # (categories, patterns)


def run_all(pkg, synth, oracle, monkeypatch, timing):
    """the six calls on a fresh group -> {name: (ms0, ms1, launches or None)} and what the launch counts follow from"""
    lib = pkg.libiqhip()
    nwk = synth.random_tree_newick(NTAXA, 61, 0.05, 0.4)
    members = [member_with_patterns(synth, oracle, nwk, 4, ncat, pr.SEQ_DNA, 3000, 900 + 10 * k, RATES[k], npat)
               for k, (ncat, npat) in enumerate(SHAPES)]
    G = pb.make_group(pkg, oracle, nwk, members, RATES)
    g, trees = G["group"], G["trees"]
    assert [t.nptn for t in trees] == [npat for _, npat in SHAPES] and trees[0].num_leaves == NTAXA
    P = len(trees)
    for t in trees:
        assert lib.iqhip_timing_enable(t.engine, 1 if timing else 0) == 0
    rng = np.random.default_rng(5)
    g.ptnlh_reserve(NROWS)
    for t in trees:
        for r in range(NROWS):
            t.ptnlh_upload(r, rng.uniform(-9.0, -1.0, size=t.nptn))
        t.set_boot_samples(rng.integers(0, 4, size=(NSAMPLES, t.nptn)).astype(np.float32))
    rows, ids, logl, rand = [0, 1, 2], [1, 2, 3], [-10.0, -11.0, -12.0], [0.5, 0.5, 0.5]
    got = {}
    # UFBoot: 3 trees in chunks of 2 -> two rounds
    monkeypatch.setenv("IQHIP_UFBOOT_CHUNK", "2")
    one = trees[1]
    one.ufboot_init(NSAMPLES)
    one.ufboot_update(rows, ids, logl, rand)
    got["engine ufboot"] = one.ufboot_timing()
    g.ufboot_init(NSAMPLES)
    g.ufboot_update(rows, ids, logl, rand)
    got["group ufboot"] = g.ufboot_timing()
    monkeypatch.delenv("IQHIP_UFBOOT_CHUNK")
    # pairwise distances: 15 pairs in chunks of 4 -> four chunks
    monkeypatch.setenv("IQHIP_PAIR_CHUNK", "4")
    assert device_dist(pkg, one)[0] == 0
    a, b = C.c_double(-1.0), C.c_double(-1.0)
    assert lib.iqhip_debug_pair_timing(one.engine, C.byref(a), C.byref(b)) == 0
    got["engine pairs"] = (a.value, b.value, None)
    g.pair_distances()
    got["group pairs"] = g.pair_timing() + (None,)
    monkeypatch.delenv("IQHIP_PAIR_CHUNK")
    # the joint Newton solve of one branch, then a batch of two
    sup = G["sup"]
    tasks = [pb.plain_task(pkg, G, x, y, 1e-6, sup.length(x, y), 100.0, 1e-6, 100) for x, y in G["edges"][:2]]
    nsteps = pb.single_solve(pkg, G, tasks[0])[2]
    tm = g.timing()
    got["group newton"] = (tm["derv_ms"], tm["update_ms"], tm["launches"])
    res, _ = g.optimize_branch_batch((pkg.BranchTask * 2)(*tasks))
    assert [r["status"] for r in res] == [0, 0]
    tm = g.timing()
    got["group batch"] = (tm["derv_ms"], tm["update_ms"], tm["launches"])
    g.close()
    for t in trees:
        t.close()
    return got, P, nsteps, max(r["nsteps"] for r in res)


def check_launches(got, P, nsteps, most):
    assert got["engine ufboot"][2] == 3 * 2                          # tests/test_ufboot_gpu.py: 3 per chunk
    assert got["group ufboot"][2] == (2 * P + 1) * 2                 # tests/test_partition_ufboot_gpu.py: 2 P + 1 per chunk
    assert got["group newton"][2] >= 1 + 2 * nsteps                  # tests/test_partition_gpu.py
    assert 2 * most + 2 <= got["group batch"][2] <= 2 * (most + 3) + 2 * 3   # tests/test_partition_batch_gpu.py


def test_readings_with_timing_on(pkg, synth, oracle, monkeypatch):
    got, P, nsteps, most = run_all(pkg, synth, oracle, monkeypatch, True)
    assert len(got) == 6
    for name, (ms0, ms1, _) in sorted(got.items()):
        print("%-14s %.6f ms  %.6f ms" % (name, ms0, ms1))
    for name, (ms0, ms1, _) in got.items():
        assert math.isfinite(ms0) and ms0 > 0.0 and math.isfinite(ms1) and ms1 > 0.0, (name, ms0, ms1)
    check_launches(got, P, nsteps, most)


def test_readings_are_zero_with_timing_off(pkg, synth, oracle, monkeypatch):
    got, P, nsteps, most = run_all(pkg, synth, oracle, monkeypatch, False)
    assert len(got) == 6
    for name, (ms0, ms1, _) in got.items():
        assert ms0 == 0.0 and ms1 == 0.0, (name, ms0, ms1)
    check_launches(got, P, nsteps, most)
