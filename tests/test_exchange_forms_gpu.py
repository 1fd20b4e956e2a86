"""The posted and the arrival-counter exchange (wg_exchange.h; IQHIP_NEWTON_POSTS=0 selects the counter) on the engines
test_newton_exchange_gpu.py leaves out: a +ASC DNA engine -- every workgroup adds the unobserved patterns' correction to the
exchanged sums -- and a 20-state +G4 engine (16-pattern tiles, B = 80, theta held in registers).  Both forms add the same
workgroup partials in the same order, so optimum, d2l, evaluation count, the lengths of a sweep and the batched NNI
candidates must agree bit for bit.  Each engine has 5 to 16 tiles: several workgroups take part in every solve."""
import pytest

from test_asc_batch_gpu import asc_inputs, asc_tree
from test_newton_oracle_gpu import device_newton
from test_solver_paths_gpu import SETUPS, engine_tiles, uncompressed
from test_sweep_gpu import lengths

pytestmark = pytest.mark.gpu


def asc_dna(pkg, synth, oracle):
    return asc_tree(pkg, asc_inputs(synth, 4, 4, 0, 12, 1500), 4, 0, mem_mode=pkg.LM_ALL_BRANCH), 64


def protein(pkg, synth, oracle):
    return uncompressed(20, 4, 1, 9, 150, 7300)(pkg, synth, oracle, mem_mode=pkg.LM_ALL_BRANCH)[0], 16


def solver_bits(pkg, synth, oracle, make):
    t, tile = make(pkg, synth, oracle)
    ntiles = engine_tiles(t.nptn, tile)
    assert 5 <= ntiles <= 16, ntiles                 # more than one workgroup of 4 waves per solve
    t.set_device_newton(True)
    t.compute_likelihood()
    inner = [(a, b) for (a, b) in lengths(t) if len(t.neighbors(a)) == 3 and len(t.neighbors(b)) == 3]
    out = {"nni": [(m["new_len"], m["newloglh"]) for m in t.evaluate_nnis_batch()], "solves": []}
    for (a, b) in ((0, t.neighbors(0)[0][0]), inner[len(inner) // 2]):
        t.reset_theta()
        t.compute_likelihood_derv(a, b)
        for (x1, xg, x2, xacc, ms) in SETUPS:
            xg = lengths(t)[(min(a, b), max(a, b))] if xg is None else xg
            out["solves"].append((a, b, ms) + device_newton(pkg, t, xg, x1, x2, xacc, ms))
        # the solve with max_steps = 3 is ended by the limit: one more step allowed, one more evaluation made
        assert out["solves"][-1][2] == 3 and out["solves"][-1][5] == 3, out["solves"][-1]
        assert device_newton(pkg, t, 3.0, 1e-6, 100.0, 1e-6, 4)[2] == 4
    pc = t.path_counts()
    assert pc["newton_one_launch"] > 0 and pc["newton_chain"] == 0 and pc["newton_fallback"] == 0, pc
    out["lnl"] = t.optimize_all_branches(iterations=1, tolerance=1e-3)    # theta built by the first evaluation of every solve
    out["lengths"] = lengths(t)
    t.close()
    return out


@pytest.mark.parametrize("make", [asc_dna, protein])
def test_posted_and_counted_exchange_agree(pkg, synth, oracle, monkeypatch, make):
    monkeypatch.delenv("IQHIP_NEWTON_POSTS", raising=False)
    posted = solver_bits(pkg, synth, oracle, make)
    monkeypatch.setenv("IQHIP_NEWTON_POSTS", "0")    # (read when the engine is created)
    counted = solver_bits(pkg, synth, oracle, make)
    assert len(posted["solves"]) == 2 * len(SETUPS) and len(posted["nni"]) > 0
    for p, c in zip(posted["solves"], counted["solves"]):
        print("solve", p, c)
        assert p == c                                 # optx, d2l and the number of evaluations, bit for bit
    assert posted["nni"] == counted["nni"]
    assert posted["lnl"] == counted["lnl"] and posted["lengths"] == counted["lengths"]
