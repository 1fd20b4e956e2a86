"""GPU parity over the paths the device branch-length solvers take (kernels_newton.hip wg_partial / k_newton /
k_newton_batch, solve.hip, kernels_sweep.hip) -- the solvers' counterpart of test_kernel_paths_gpu.py.  The paths are keyed
on B = nstates * ncat of the engine and on tiles per wave, independently of the traversal kernels:

  * theta held in registers across the evaluations of a solve (ThetaRegs): ntiles <= 4 * grid and B <= 80 on a 16-pattern
    engine (B <= 20 on a 64-pattern one); below the bound the registers are partly filled (`e < B` guards)
  * the generic 16-pattern path walks a pattern's rows in chunks of 80: B > 80 iterates, the last chunk partial or full
  * several tiles per wave in k_newton once (ntiles + 3) / 4 exceeds the grid cap: 2 * num_cus with the posted exchange,
    num_cus with the arrival counter (IQHIP_NEWTON_POSTS=0, or max_steps + 5 > 128 post epochs)
  * k_newton_batch: several tiles per wave as soon as ntasks * wgs_needed > capacity (solve.hip iqhip_optimize_branch_batch)
  * the fused front end (theta built inside the first evaluation, from a leaf or from two vectors) per layout

Every solve is compared with the oracle's minimize_newton (oracle_driver.OracleTree: the reference's loop over the oracle's
derivative kernel): same number of derivative evaluations, optimum to 1e-9, d2l to 1e-6 -- the tolerances of
test_newton_oracle_gpu.py.  The conditions the cases must meet (every solve 'ok'; a bisection step, a result on either
bound and a solve ended by the step limit in every case; no |dx| or |f| within 1e-6 relative of xacc, where the evaluation
count could legitimately differ) are properties of the oracle alone and are asserted beside the comparisons."""
import collections
import copy

import numpy as np
import pytest

import test_binary_gpu
import test_other_states_gpu
from test_asc_batch_gpu import asc_inputs, asc_oracle, asc_tree, oracle_candidates
from test_mixture import make_mix
from test_newton_oracle_gpu import device_newton
from test_parity_gpu import LNL_RTOL, make_case
from test_sweep_gpu import lengths, run_both

pytestmark = pytest.mark.gpu

X1, X2, XACC = 1e-6, 100.0, 1e-6     # the mirror's branch bounds and tolerance (phylo_host.h, tools.cpp defaults)
# (x1, xguess, x2, xacc, max_steps) of test_device_newton_matches_oracle_newton: the reference's call, a far-off start, an
# upper bound below the optimum, a lower bound above it, a step limit that ends the loop early
SETUPS = [(1e-6, None, 100.0, 1e-6, 100), (1e-6, 60.0, 100.0, 1e-6, 100), (1e-6, 0.01, 0.03, 1e-6, 100),
          (0.6, 0.9, 100.0, 1e-6, 100), (1e-6, 3.0, 100.0, 1e-6, 3)]
CONDITIONS = ("bisection", "upper", "lower", "limit")


def num_cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def engine_tiles(nptn, tile):
    """ntiles of an engine (engine.hip configure_engine: patterns padded to 64)"""
    return (nptn + 63) // 64 * 64 // tile


# ------------------------------------------------------------------------------------------
# the oracle side: expected solves and what each of them did
# ------------------------------------------------------------------------------------------
def oracle_solve(ot, a, b, x1, xguess, x2, xacc, max_steps, theta, stats):
    """ot.minimize_newton -> (optx, d2l, number of evaluations).  The solve is followed point by point (bracket, kind of
    step, |dx|, |f|) for the conditions of the module docstring; `stats` counts what happened."""
    optx, d2l, pts, status = ot.minimize_newton(a, b, x1, xguess, x2, xacc, max_steps, theta=theta)
    assert status == "ok", (a, b, x1, xguess, x2, max_steps, status)
    xl, xh = x1, x2
    for k, x in enumerate(pts):
        df, ddf = ot.derv(a, b, length=x, theta=theta)
        f, df = -df, -ddf
        if f < 0.0:
            xl = x
        else:
            xh = x
        bisect = df <= 0.0 or ((x - xh) * df - f) * ((x - xl) * df - f) >= 0.0
        dx = 0.5 * (xh - xl) if bisect else f / df
        if k + 1 < len(pts):
            assert pts[k + 1] == (xl + dx if bisect else x - dx), (k, pts, bisect)   # (this walk is the oracle's)
            stats["bisection"] += int(bisect)
        # an evaluation count may differ from the oracle's only where a stopping test is decided by the last bits
        assert abs(abs(dx) - xacc) > 1e-6 * xacc and abs(abs(f) - xacc) > 1e-6 * xacc, ("change the seed", a, b, x, dx, f)
    stats["upper"] += int(x2 - optx <= 2 * xacc)
    stats["lower"] += int(optx - x1 <= 2 * xacc)
    if len(pts) == max_steps:   # ended by the limit, unless one more step would not have been evaluated either
        stats["limit"] += int(len(ot.minimize_newton(a, b, x1, xguess, x2, xacc, max_steps + 1, theta=theta)[2]) > max_steps)
    stats["solves"] += 1
    return optx, d2l, len(pts)


def two_branches(ot):
    """a leaf branch and an internal branch (check_paths' choice)"""
    inner = [(x, y) for x in sorted(ot.adj) for y, _ in ot.adj[x] if not ot.is_leaf(x) and not ot.is_leaf(y)]
    return [(0, ot.adj[0][0][0]), inner[len(inner) // 2]]


def expected_solves(ot, a, b, stats, max_steps=100):
    """the five set-ups on branch (a, b) of the oracle, theta built once: [(x1, xguess, x2, xacc, max_steps, optx, d2l, n)]"""
    theta, _ = ot.theta(a, b)
    out = []
    for (x1, xg, x2, xacc, ms) in SETUPS:
        xg = ot.length(a, b) if xg is None else xg
        ms = max_steps if ms == 100 else ms
        out.append((x1, xg, x2, xacc, ms) + oracle_solve(ot, a, b, x1, xg, x2, xacc, ms, theta, stats))
    return out


def expected_one_branch(ot, a, b, stats, max_steps=100):
    """optimizeOneBranch (phylotree.cpp:2148-2192) on the oracle: the solve from the current length, then the
    diverged-solve rule"""
    cur = ot.length(a, b)
    optx, _, _ = oracle_solve(ot, a, b, X1, cur, X2, XACC, max_steps, ot.theta(a, b)[0], stats)
    if optx > 0.95 * X2 and ot.lnl_from_theta(a, b, length=cur)[0] > ot.lnl_from_theta(a, b, length=optx)[0]:
        return cur
    return optx


def assert_conditions(stats):
    for c in CONDITIONS:
        assert stats[c] >= 1, (c, dict(stats))


# ------------------------------------------------------------------------------------------
# check_solvers
# ------------------------------------------------------------------------------------------
def run_setups(pkg, t, want, slot):
    """every expected solve of `want` = {(a, b): expected_solves} through iqhip_newton_branch on resident theta"""
    pc0 = t.path_counts()
    n = 0
    for (a, b), solves in want.items():
        t.reset_theta()
        t.compute_likelihood_derv(a, b)   # pending partials of both ends + theta of this branch on the device
        for (x1, xg, x2, xacc, ms, ref_x, ref_d2l, npts) in solves:
            optx, d2l, ns = device_newton(pkg, t, xg, x1, x2, xacc, ms)
            print(slot, (a, b), (x1, xg, x2, ms), optx, ref_x, d2l, ref_d2l, ns, npts)
            assert ns == npts, (a, b, x1, xg, x2, ms, ns, npts)
            assert abs(optx - ref_x) <= 1e-9 * max(1.0, abs(ref_x)), (a, b, x1, xg, x2, ms, optx, ref_x)
            assert abs(d2l - ref_d2l) <= 1e-6 * max(1.0, abs(ref_d2l)), (a, b, x1, xg, x2, ms, d2l, ref_d2l)
            n += 1
    pc = t.path_counts()
    other = "newton_chain" if slot == "newton_one_launch" else "newton_one_launch"
    assert pc[slot] - pc0[slot] == n and pc[other] == pc0[other] and pc["newton_fallback"] == 0, (pc0, pc)
    return n


def check_solvers(pkg, make, monkeypatch, branches=two_branches, max_steps=100, chain=True):
    """`make() -> (tree with an engine, its oracle)`.  On the branches of the case: (1) resident theta, one launch of
    k_newton per solve, the five set-ups; (2) the fused front end through optimize_one_branch, the result fed into the
    oracle before the next branch; (3) the same set-ups on a second engine created under IQHIP_NEWTON=chain."""
    stats = collections.Counter()
    t, ot = make()
    t.set_device_newton(True)
    t.compute_likelihood()
    brs = branches(ot)
    want = {br: expected_solves(ot, br[0], br[1], stats, max_steps) for br in brs}
    nchecked = run_setups(pkg, t, want, "newton_one_launch")
    if chain:
        monkeypatch.setenv("IQHIP_NEWTON", "chain")      # (read when the engine is created)
        tc, _ = make()
        monkeypatch.delenv("IQHIP_NEWTON")
        tc.compute_likelihood()
        assert run_setups(pkg, tc, want, "newton_chain") == nchecked
        tc.close()
    for (a, b) in brs:
        t.clear_all_partial_lh()
        t.compute_likelihood()
        pc0 = t.path_counts()
        got = t.optimize_one_branch(a, b, max_nr_step=max_steps)
        ref = expected_one_branch(ot, a, b, stats, max_steps)
        print("fused", (a, b), got, ref)
        assert abs(got - ref) <= 1e-9 * max(1.0, ref), (a, b, got, ref)
        pc = t.path_counts()
        assert pc["newton_one_launch"] == pc0["newton_one_launch"] + 1 and pc["newton_chain"] == pc["newton_fallback"] == 0, pc
        ot.set_length(a, b, got)
    assert nchecked == len(SETUPS) * len(brs) and stats["solves"] == nchecked + len(brs)
    assert_conditions(stats)
    t.close()
    return stats


# ------------------------------------------------------------------------------------------
# cases: make(pkg, synth, oracle, mem_mode) -> (tree, oracle tree); the same inputs on every call
# ------------------------------------------------------------------------------------------
def plain(n, ncat, seq_type, ntaxa, nptn, seed, missing=0.03):
    def make(pkg, synth, oracle, mem_mode=0):
        return make_case(synth, oracle, pkg, ntaxa, nptn, n, ncat, seed, seq_type=seq_type, missing=missing, mem_mode=mem_mode)[:2]
    return make


def engine_tree(pkg, nwk, n, seq_type, pat, freq, model, mem_mode=0):
    t = pkg.PhyloTree(nwk)
    t.set_mem_mode(mem_mode)
    t.set_alignment(n, seq_type, pat, freq)
    t.set_model(model)
    t.set_likelihood_kernel(pkg.LK_EIGEN_HIP)
    t.attach_engine(0)
    return t


def mixture(n, seq_type, nclass, ncat, fused, ntaxa, nptn, seed):
    def make(pkg, synth, oracle, mem_mode=0):
        model, nwk, pat, freq, ot = make_mix(synth, oracle, n, nclass, ncat, fused, ntaxa, nptn, seed, seq_type)
        assert model.ncat == (nclass if fused else nclass * ncat)
        return engine_tree(pkg, nwk, n, seq_type, pat, freq, model, mem_mode), ot
    return make


def embedded(n, ncat, ntaxa, nsites, seed):
    def make(pkg, synth, oracle, mem_mode=0):
        return test_other_states_gpu.build(pkg, synth, oracle, n, ncat, ntaxa, nsites, seed, mem_mode=mem_mode)
    return make


def binary(ncat, seed):
    def make(pkg, synth, oracle, mem_mode=0):
        return test_binary_gpu.make_case(synth, oracle, pkg, 12, 3000, ncat, seed, missing=0.05)[:2]
    return make


def asc_mixture_inputs(synth, n, nclass, ncat, ntaxa, nsites, seed):
    """asc_inputs for a mixture: variable sites only, then one unobserved constant pattern per state"""
    model = synth.mixture_model(n, nclass, seed, ncat=ncat)
    nwk = synth.random_tree_newick(ntaxa, seed + 1, 0.02, 0.15)
    pat, freq = synth.compress_patterns(synth.simulate_alignment(nwk, model.classes[0], nsites, seed + 2))
    const = np.all(pat == pat[0][None, :], axis=0)
    pat, freq = np.ascontiguousarray(pat[:, ~const]), freq[~const].copy()
    ns = float(freq.sum())
    pat = np.ascontiguousarray(np.concatenate([pat, np.tile(np.arange(n, dtype=np.uint8)[None, :], (ntaxa, 1))], axis=1))
    return nwk, pat, np.concatenate([freq, np.zeros(n)]), n, ns, model


def with_asc(n, seq_type, inputs_of):
    def make(pkg, synth, oracle, mem_mode=0):
        inputs = inputs_of(synth)
        nobs, nptn = inputs[1].shape[1] - n, inputs[1].shape[1]
        assert nobs // 16 < (nptn - 1) // 16          # the unobserved patterns lie in more than one 16-pattern tile
        return asc_tree(pkg, inputs, n, seq_type, mem_mode=mem_mode), asc_oracle(oracle, inputs, n, seq_type)
    return make


def uncompressed(n, ncat, seq_type, ntaxa, nptn, seed):
    """simulated columns as they come, every frequency 1: exactly nptn patterns"""
    def make(pkg, synth, oracle, mem_mode=0):
        model = synth.gtr_model(alpha=0.9, ncat=ncat) if n == 4 else synth.random_reversible_model(n, seed, alpha=0.9, ncat=ncat)
        nwk = synth.random_tree_newick(ntaxa, seed)
        st = synth.simulate_alignment(nwk, model, nptn, seed + 1, 0.02, oracle.state_unknown_for(n, seq_type))
        freq = np.ones(nptn)
        return (engine_tree(pkg, nwk, n, seq_type, st, freq, model, mem_mode),
                oracle.OracleTree(nwk, n, seq_type, st, freq, None, model))
    return make


MIX20_3x2 = mixture(20, 1, 3, 2, False, 9, 300, 5301)
MIX4_2x4 = mixture(4, 0, 2, 4, False, 9, 300, 5502)
ASC_20x5 = with_asc(20, 1, lambda synth: asc_inputs(synth, 20, 5, 1, 9, 300))
ASC_MIX20_3x2 = with_asc(20, 1, lambda synth: asc_mixture_inputs(synth, 20, 3, 2, 9, 300, 5801))

# id -> (make, engine B = kernel states x categories, 16-pattern layout)
SOLVER_CASES = collections.OrderedDict(
    # 20 states, plain: registers partly filled (B = 20 / 40 / 60), the boundary (80), a partial second chunk (100), two
    # full chunks (160), four (320)
    [("20x%d" % c, (plain(20, c, 1, 9, 300, 5100 + c), 20 * c, True)) for c in (1, 2, 3, 4, 5, 8, 16)] +
    # 64 states, plain: the generic path, several chunks
    [("64x2", (plain(64, 2, 2, 8, 250, 5202), 128, True)), ("64x16", (plain(64, 16, 2, 8, 150, 5216, missing=0.02), 1024, True))] +
    # 20-state mixtures: per-component eigenvalues and rates in eval_at; 96 components = 46 KB of LDS
    [("mix20-3x2", (MIX20_3x2, 120, True)), ("mix20-24x4", (mixture(20, 1, 24, 4, False, 7, 150, 5324), 1920, True)),
     ("mix20-96x1", (mixture(20, 1, 96, 1, True, 7, 150, 5396), 1920, True)),
     ("mix64-8x2", (mixture(64, 2, 8, 2, False, 7, 150, 5408), 1024, True))] +
    # 4-state mixtures: 4 states in the 16-pattern layout (B <= 80: registers, 2 / 3 / 8 of 20 per lane filled)
    [("mix4-2x1", (mixture(4, 0, 2, 1, True, 9, 300, 5501), 8, True)), ("mix4-2x4", (MIX4_2x4, 32, True)),
     ("mix4-3x1", (mixture(4, 0, 3, 1, True, 9, 300, 5503), 12, True))] +
    # state counts embedded in the 4-, 20- and 64-state kernels: zero-padded rows of the block
    [("n3x4", (embedded(3, 4, 10, 400, 5603), 16, False)), ("n5x4", (embedded(5, 4, 10, 500, 5605), 80, True)),
     ("n5x5", (embedded(5, 5, 10, 500, 5655), 100, True)), ("n21x1", (embedded(21, 1, 9, 300, 5621), 64, True)),
     ("n61x1", (embedded(61, 1, 8, 300, 5661), 64, True))] +
    [("binary-1", (binary(1, 5701), 4, False)), ("binary-4", (binary(4, 5704), 16, False))] +
    # +ASC where asc_unobserved_sums walks more than 80 rows per pattern
    [("asc-20x5", (ASC_20x5, 100, True)), ("asc-mix20-3x2", (ASC_MIX20_3x2, 120, True))])


@pytest.mark.parametrize("case", list(SOLVER_CASES))
def test_solvers_at_every_model_shape(pkg, synth, oracle, case, monkeypatch):
    make, B, tile16 = SOLVER_CASES[case]
    made = []

    def once():
        made.append(make(pkg, synth, oracle))
        return made[-1]
    stats = check_solvers(pkg, once, monkeypatch)
    ot = made[0][1]
    # the path: one workgroup per solve or one tile per wave, so theta stays in registers exactly when B allows it
    kernel_n = 4 if ot.n <= 4 else 20 if ot.n <= 20 else 64
    assert B == kernel_n * ot.ncat and tile16 == (kernel_n != 4 or ot.nclass > 1)
    ntiles = engine_tiles(ot.nptn, 16 if tile16 else 64)
    assert ntiles <= 4 * min((ntiles + 3) // 4, num_cus())
    print("case", case, "B", B, "tiles", ntiles, "registers", B <= (80 if tile16 else 20), dict(stats))


# ------------------------------------------------------------------------------------------
# several tiles per wave in k_newton: more tiles than 4 waves x the grid cap
# ------------------------------------------------------------------------------------------
TILE_CASES = [  # n, ncat, seq_type, grid cap in workgroups per CU, env, max_steps
    (20, 1, 1, 2, {}, 100),                             # posted exchange
    (20, 1, 1, 1, {"IQHIP_NEWTON_POSTS": "0"}, 100),    # arrival counter
    (20, 1, 1, 1, {}, 200),                             # max_steps + 5 > 128 post epochs: the counter form by itself
    (20, 4, 1, 2, {}, 100),
    (20, 4, 1, 1, {"IQHIP_NEWTON_POSTS": "0"}, 100),
    (20, 4, 1, 1, {}, 200),
    (4, 4, 0, 1, {"IQHIP_NEWTON_POSTS": "0"}, 100),     # 64-pattern layout
    (4, 4, 0, 1, {}, 200),
]


def tile_case(n, ncat, seq_type, cap, ncu):
    """-> (tile, nptn, make) with 4 * cap * ncu + 1 tiles, the last one ragged"""
    tile = 64 if n == 4 else 16
    nptn = tile * (4 * cap * ncu + 1) - 5
    return tile, nptn, uncompressed(n, ncat, seq_type, 8, nptn, 5900 + n + ncat + cap)


@pytest.mark.parametrize("n,ncat,seq_type,cap,env,max_steps", TILE_CASES,
                         ids=["%dx%d-cap%d-%s" % (c[0], c[1], c[3], "steps200" if c[5] == 200 else "posts0" if c[4] else "posts")
                              for c in TILE_CASES])
def test_newton_with_several_tiles_per_wave(pkg, synth, oracle, n, ncat, seq_type, cap, env, max_steps, monkeypatch):
    """ntiles = 4 * cap * num_cus + 1: at least one wave of the capped grid owns two tiles (`tile += nwg * 4`), and theta
    is re-read from memory although B <= 80 (B <= 20 would be the 64-pattern bound: 4 x 4 is under it too).  One branch per
    case, a leaf branch for one category (theta built from `tipc`) and an internal one otherwise; no chain engine."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    tile, nptn, make = tile_case(n, ncat, seq_type, cap, num_cus())
    ntiles = engine_tiles(nptn, tile)
    posts = not env and max_steps + 5 <= 128
    assert cap == (2 if posts else 1)
    grid = min((ntiles + 3) // 4, cap * num_cus())
    assert ntiles > 4 * grid and n * ncat <= (20 if n == 4 else 80)
    stats = check_solvers(pkg, lambda: make(pkg, synth, oracle), monkeypatch, max_steps=max_steps, chain=False,
                          branches=lambda ot: two_branches(ot)[:1] if ncat == 1 else two_branches(ot)[1:])
    print("tiles", n, ncat, cap, max_steps, "nptn", nptn, "tiles", ntiles, "grid", grid, dict(stats))


# ------------------------------------------------------------------------------------------
# batched NNI candidates against the oracle, without +ASC
# ------------------------------------------------------------------------------------------
def clone(ot):
    """the same oracle tree with an adjacency of its own"""
    o2 = copy.copy(ot)
    o2.adj = {k: [list(e) for e in v] for k, v in ot.adj.items()}
    o2.cache = {}
    return o2


BATCH_CASES = collections.OrderedDict([
    ("4x3", plain(4, 3, 0, 9, 300, 6003, missing=0.02)), ("20x1", plain(20, 1, 1, 9, 300, 6001, missing=0.02)),
    ("20x5", plain(20, 5, 1, 9, 300, 6005, missing=0.02)), ("64x2", plain(64, 2, 2, 9, 200, 6002, missing=0.02)),
    ("mix20-3x2", MIX20_3x2), ("mix4-2x4", MIX4_2x4), ("n5x4", embedded(5, 4, 9, 500, 6054))])


def check_batch(t, ot, ntaxa):
    """every nni1 candidate of the tree: the oracle's minimize_newton on the swapped tree with the NNI step limit, and that
    tree's lnL at the batch's length"""
    t.compute_likelihood()
    c0 = t.num_derv_calls
    batch = t.evaluate_nnis_batch()
    nevals = t.num_derv_calls - c0
    assert len(batch) == 2 * (ntaxa - 3)
    ref = oracle_candidates(lambda: clone(ot), batch)
    assert all(r[0] <= 0.95 * X2 for r in ref)                     # no candidate takes the diverged-solve detour
    for m, (optx, pts, lnl) in zip(batch, ref):
        print("batch", m, optx, len(pts), lnl)
        assert abs(m["new_len"] - optx) <= 1e-9 * max(1.0, abs(optx)), (m, optx)
        assert abs(m["newloglh"] - lnl) <= LNL_RTOL * abs(lnl), (m, lnl)
    assert nevals == sum(len(r[1]) for r in ref), (nevals, [len(r[1]) for r in ref])
    return batch


@pytest.mark.parametrize("case", list(BATCH_CASES))
def test_batched_candidates_against_the_oracle(pkg, synth, oracle, case):
    t, ot = BATCH_CASES[case](pkg, synth, oracle, mem_mode=pkg.LM_ALL_BRANCH)
    assert ot.ntaxa == 9
    check_batch(t, ot, 9)


def test_batched_candidates_with_several_tiles_per_wave(pkg, synth, oracle):
    """20 x 4 with ntasks * wgs_needed > capacity (solve.hip iqhip_optimize_branch_batch: 3 workgroups per CU while the LDS
    of a workgroup, (3 * block + 8) doubles + 64 bytes, allows it; G = capacity / ntasks workgroups per task): each task's
    4 * G waves own more than one tile.  The mirror submits the first swaps of all branches, then the second swaps:
    ntaxa - 3 tasks per launch."""
    ntasks, block = 9 - 3, 80
    wg_per_cu = max(1, min(3, 150 * 1024 // ((3 * block + 8) * 8 + 64)))
    capacity = num_cus() * wg_per_cu
    G = capacity // ntasks
    nptn = 16 * (4 * G + 1) - 5
    ntiles = engine_tiles(nptn, 16)
    wgs_needed = (ntiles + 3) // 4
    assert ntasks <= capacity and ntasks * wgs_needed > capacity and ntiles > 4 * G
    t, ot = uncompressed(20, 4, 1, 9, nptn, 6100)(pkg, synth, oracle, mem_mode=pkg.LM_ALL_BRANCH)
    check_batch(t, ot, 9)


def test_nni5_batch_at_a_second_chunk(pkg, synth, oracle):
    """20 x 5 (B = 100): the nni5 batch against the evaluator that goes branch by branch"""
    t, ot = BATCH_CASES["20x5"](pkg, synth, oracle, mem_mode=pkg.LM_ALL_BRANCH)
    lnl = t.compute_likelihood()
    tree0 = t.tree_string()
    batch = t.evaluate_nnis5_batch()
    assert len(batch) == 2 * (9 - 3) and t.tree_string() == tree0
    assert abs(t.compute_likelihood() - lnl) <= 1e-12 * abs(lnl)
    for k in range(0, len(batch), 2):
        a, b = batch[k]["node1"], batch[k]["node2"]
        seq = t.nni_for_branch(a, b, nni5=True)
        for c in range(2):
            newloglh, nei1, nei2, lens = seq[c]
            m = batch[k + c]
            assert (m["node1_nei"], m["node2_nei"]) == (nei1, nei2)
            print("nni5", (a, b, c), m["new_lens"], lens, m["newloglh"], newloglh)
            np.testing.assert_allclose(m["new_lens"], lens, rtol=1e-7, atol=1e-12)
            assert abs(m["newloglh"] - newloglh) <= 1e-9 * abs(newloglh)


# ------------------------------------------------------------------------------------------
# sweeps: one submission against the per-branch form, on engines that take the per-step form
# ------------------------------------------------------------------------------------------
SWEEP_CASES = collections.OrderedDict([
    ("20x5", plain(20, 5, 1, 9, 300, 6205, missing=0.02)), ("64x2", plain(64, 2, 2, 8, 250, 6202, missing=0.02)),
    ("mix20-3x2", MIX20_3x2), ("mix4-2x4", MIX4_2x4), ("n5x4", embedded(5, 4, 10, 500, 6254))])


@pytest.mark.parametrize("case", list(SWEEP_CASES))
def test_sweeps_in_the_per_step_form(pkg, synth, oracle, case):
    made = []

    def make():
        made.append(SWEEP_CASES[case](pkg, synth, oracle))
        return made[-1][0]
    out = run_both(make, iterations=2, start=0.15)
    (l0, len0, c0, s0, _), (l1, len1, c1, s1, t1) = out[False], out[True]
    assert len0.keys() == len1.keys()
    for k in len0:
        assert len0[k] == len1[k], (k, len0[k], len1[k])     # same evaluated points, same kernels: same bits
    assert l0 == l1
    assert c0 == c1                                          # derivative evaluations
    nbranch = len(len0)
    assert s1 < s0 and s0 - s1 >= nbranch - 1                # one submission per sweep instead of one per branch
    pc = t1.path_counts()
    assert pc["sweep_per_step"] > 0 and pc["sweep_persistent"] == 0 and pc["sweep_sequential"] == 0, pc
    assert pc["newton_chain"] == 0 and pc["newton_fallback"] == 0, pc
    ot = made[-1][1]
    ot2 = oracle.OracleTree(t1.tree_string(), ot.n, ot.seq_type, ot.states, ot.freq, ot.invar, ot.model)
    ref, _ = ot2.likelihood()
    print("sweep", case, l1, ref, c1, s0, s1, pc)
    assert abs(l1 - ref) <= 1e-8 * abs(ref)
    assert len(lengths(t1)) == nbranch == 2 * ot.ntaxa - 3
