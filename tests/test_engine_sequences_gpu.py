"""GPU: ONE long-lived engine through interleaved feature calls (tests/engine_sequences.py has the catalogue, the state
record and the two comparators).

After every action the live engine's result is compared with a fresh engine built in exactly the recorded state and given
only that action (bits, or 1e-12 after a lazy partial recompute: the grades are explained in engine_sequences.py), and with
the independent references the suite already has: the next lnL against the oracle at LNL_RTOL, every Newton solve against the
oracle's minimizeNewton (same evaluation count, optimum 1e-9, d2l 1e-6), the consumers against numpy / em_ref / mixem_ref /
lmap_ref / fitch_ref at their own tests' tolerances.

Every engine is created with IQHIP_CHECK_PLAN=1: each plan it uploads is validated on the host as well.  A failing sequence
prints the prefix of action ids that led to the failure; pasted into engine_sequences.fixed_sequences() it becomes a new
fixed sequence."""
import numpy as np
import pytest

import engine_sequences as ES
from test_cherry_tables_gpu import counters as cherry_counters
from test_parity_gpu import LNL_RTOL

pytestmark = pytest.mark.gpu

FIXED = ES.fixed_sequences()


@pytest.fixture(scope="module")
def ctx(pkg, synth, oracle):
    c = ES.Ctx(pkg, synth, oracle)
    yield c
    print("fresh engines built: %d for %d distinct (state, action) pairs" % (c.fresh_built, len(c.fresh_cache)))


@pytest.fixture(autouse=True)
def checked_plans(monkeypatch):
    monkeypatch.setenv("IQHIP_CHECK_PLAN", "1")      # (read when an engine is created)


def drive(ctx, state, seq, at_end=None, **kw):
    r = ES.Runner(ctx, state, **kw)
    try:
        r.run_all(seq)
        if at_end:
            at_end(r.t)
    finally:
        r.close()
    print(state.kind, state.route, "actions", dict(r.counts), "references", dict(r.refs), "solves", dict(r.stats))
    return r


def newton_actions(seq):
    return [a for a in seq if ES.split_id(a)[0] in ("newton_posted", "newton_counter", "newton_limit")]


# What each fixed sequence aims at (iqhip_internal.h line numbers of the engine's fields):
#   parities-*      newton_launches & 1 picks d_newton_barrier, newton_post_launches & 1 the half of d_newton_posts (:679,
#                   :684), each k_newton launch resets the other parity's slots of its own grid; k_newton_batch has
#                   batch_launches / batch_post_launches / batch_posts_used[2] (:689-697), k_sweep4 its parity buffers
#                   (d_sweep_posts, solve.hip:366).  posted, counter, posted, posted, batch, counter, batch, batch, sweep,
#                   posted -- once as written (even) and once with one more posted solve in front (odd), so that every launch
#                   meets both parities and every change of form happens at both.
#   layout-dna      the 4-state layout switch of set_model_common (engine.hip:441-457): 64-pattern tiles -> 16-pattern tiles
#                   while the model is a mixture -> back; it re-arms d_newton_posts and newton_post_launches, drops plan_cache
#                   (:724) and theta_valid (:471).  The whole pass under plain, mixture, plain; mix.model_version (:614):
#                   mix_weights_em is refused again after every model change.
#   model-change-*  model_version / tab_model_version (:515), em.valid (:604), mix.model_version (:614), cherry_model_synced
#                   (:538: the pair engine of the distances follows set_model), the host copies h_evec0 / h_tip0 / h_props /
#                   h_cls / pd.coef: every consumer, a new eigen-system, every consumer again.
#   reweight-*      freq_prefix_valid (:577: gen_boot_samples draws from the prefix sums of ptn_freq; the drawn samples are
#                   checked against the generator's restatement), h_freq and the device row store: set_ptn_freq (a resample
#                   with zeros) between every pair of consumers, then the original frequencies and the first results again.
#                   pars_ready (:656) and the mirror's pars_initialized: `pars` runs through the mirror with no
#                   initialisation of the test's own, so after set_ptn_freq the mirror must lay the sites out again by
#                   itself; `pars_stale` asserts that the raw calls are refused with the documented message until
#                   pars_init is repeated.  Scores against fitch_ref on the new frequencies.
#   cherry-*        cherry_slots[].model_version (:521) and the leaf / cherry tables' tab_model_version (:515): 20 x 4 with
#                   nptn_pad = 8192, where a node with two leaf children is answered from a table.  lnL and every vector,
#                   bit-equal to a fresh engine, after a model change, a Newton solve and a new length on a cherry's pendant
#                   branch, the NNI batch, the model set back, the pendant length set by hand.
#   stale-matrix-*  mix.model_version (:614) against a set_model the mirror has not pushed yet: see fixed_sequences().
#   recycling-dna   key2slab / keymap_version (:728-733) and plan_cache under LM_PER_NODE: re-rooting on every branch steals
#                   buffers, all keys are released, one length changes, every branch again.
@pytest.mark.parametrize("sid", list(FIXED))
def test_fixed_sequence(ctx, sid):
    kind, mem_mode, seq = FIXED[sid]
    cherries = []
    r = drive(ctx, ctx.start(kind, mem_mode), seq, at_end=lambda t: cherries.append(cherry_counters(ctx.pkg, t)))
    nn = len(newton_actions(seq))
    assert r.refs["oracle_newton"] == nn and r.stats["solves"] == nn
    if kind == "prot_cherry":
        # (conditions on the input: the engine did answer cherries from tables, and rebuilt them along the way; the branch
        # the sequence solves and changes is a cherry's pendant one)
        built, ops = cherries[0]
        assert built >= 2 and ops >= built, (built, ops)          # test_cherry_tables_gpu.py:63
        assert ES.is_cherry_pendant(ctx, ES.CHERRY_PENDANT)
    else:
        assert cherries[0] == (0, 0)
    assert r.refs["oracle_lnl"] == sum(1 for a in seq if a.startswith("lnl@"))
    if sid.startswith("parities"):
        assert nn == (6 if sid.endswith("even") else 7) and r.counts["nni"] == 3 and r.counts["sweep"] == 1
    if sid == "layout-dna":
        n = len(ES.LAYOUT_PASS)
        assert len(seq) == 3 * n + 6
        # the third pass (plain again) repeats the first to the bit
        ES.first_pass_equals(r.results, seq, range(0, n), range(2 * n + 6, 3 * n + 6))
        assert r.refs["mixem_ref"] == 1 and r.refs["em_ref"] == 2
    if sid.startswith("reweight"):
        n = len(ES.REWEIGHT_SET)
        ES.first_pass_equals(r.results, seq, range(0, n), range(len(seq) - n, len(seq)))
        assert r.counts["pars_stale"] == 1 and r.refs["fitch_raw"] == 1 and r.refs["fitch_ref"] == r.counts["pars"] >= 5
    if sid.startswith("stale-matrix"):
        assert r.refs["mixem_ref"] == 2 and r.counts["mixem_stale"] == 1
    if sid.startswith("model-change"):
        want = "mixem_ref" if kind == "prot_mix" else "em_ref"
        assert r.refs[want] == 2 and r.refs["fitch_ref"] == 2 and r.refs["fitch_raw"] == 2 and r.refs["numpy_store"] == 2
        assert r.refs["tree_tests_restatement"] == 2 and r.refs["branch_tests_restatement"] == 2
        if kind == "prot_mix":
            assert r.refs["textbook_class_lnl"] == 2
        else:
            assert r.refs["pair_dist_restatement"] == 2 and r.refs["lmap_ref_lh"] == (2 if kind == "dna" else 0)


# Timing toggled (iqhip_internal.h:738 `timing`): iqhip_timing_enable flipped before every second action of the Newton
# parity sequence and of the model-change sequence must change no result.
@pytest.mark.parametrize("sid", ["parities-prot-odd", "model-change-prot", "model-change-dna"])
def test_timing_toggled_changes_no_result(ctx, sid):
    kind, mem_mode, seq = FIXED[sid]
    plain = drive(ctx, ctx.start(kind, mem_mode), seq)
    toggled = drive(ctx, ctx.start(kind, mem_mode), seq, toggle_timing=True)
    assert len(plain.results) == len(toggled.results) == len(seq)
    for aid, a, b in zip(seq, plain.results, toggled.results):
        assert list(a) == list(b), aid
        for k in a:
            assert a[k].tobytes() == b[k].tobytes(), (aid, k)


# Topology replaced under a live engine: plan_cache (:724), the key map (:728-733), pars_ready (:656), the pair engine's
# model (cherry_model_synced :538, pd.coef) and the mirror's vectors must follow compute_parsimony_tree and compute_bionj.
# Both run right behind a change they depend on (new frequencies; a new model), after the feature has already run once on
# the old input.  Each resulting tree is compared with its restatement (fitch_ref.stepwise_addition; bionj_ref.bionj on the
# restated distances' device counterpart) and, as a string, with the tree a fresh engine in the same state builds.  The new
# tree's node numbers are the mirror's own (not those of a tree parsed from its string), so for the batch the oracle is
# given the live tree's adjacency and numbers.
def test_topology_replaced_under_a_live_engine(ctx, oracle):
    import bionj_ref as br
    import fitch_ref as F
    from test_bionj_gpu import DEVICE_TOL, GUARD, assert_log_matches
    from test_pair_dist_host import restate_matrix
    from test_solver_paths_gpu import check_batch
    state = ctx.start("dna", ES.LM_ALL_BRANCH)
    inp = ctx.inputs("dna")
    T, order = inp["ntaxa"], list(range(inp["ntaxa"] - 1, -1, -1))
    t = ctx.tree(state)

    def oracle_tree(st):
        ot = oracle.OracleTree(t.tree_string(), inp["n"], inp["seq_type"], inp["states"], np.array(st.freq), None, ctx.model(st))
        by_string = ot.likelihood()[0]
        ot.adj = {a: [[b, ln] for b, ln in t.neighbors(a)] for a in range(t.num_nodes)}
        ot.cache = {}
        assert abs(ot.likelihood()[0] - by_string) <= 1e-12 * abs(by_string)     # (the same tree under both numberings)
        return ot, by_string

    def fresh(st, build):
        f = ctx.tree(st)
        try:
            build(f)
            return f.tree_string()
        finally:
            f.close()

    try:
        lnl0, (_, ref0) = t.compute_likelihood(), oracle_tree(state)
        assert abs(lnl0 - ref0) <= LNL_RTOL * abs(ref0)
        t.evaluate_nnis_batch()                                   # the batch keys and every vector of the old tree exist
        t.compute_parsimony()                                     # the parsimony sites of the old frequencies are laid out
        t.compute_dist()                                          # the pair engine holds the old model

        # ---- new frequencies, then the stepwise-addition tree
        state = state._replace(freq=ES.resampled_freq(state, 2))
        freq = np.array(state.freq)
        t.set_ptn_freq(freq)
        t.clear_all_partial_lh()
        score = t.compute_parsimony_tree(order)
        tips = F.tip_vectors(inp["states"], F.site_patterns(freq, F.is_informative(inp["states"], inp["n"])), inp["n"])
        want_score, adj, _, _ = F.stepwise_addition(tips, order)
        assert score == want_score == F.tree_score(adj, tips) == t.compute_parsimony()      # test_parsimony_gpu.py:370-372
        assert {a: sorted(b for b, _ in t.neighbors(a)) for a in range(t.num_nodes)} == {a: sorted(adj[a]) for a in adj}
        assert t.tree_string() == fresh(state, lambda f: f.compute_parsimony_tree(order))
        old = F.tip_vectors(inp["states"], F.site_patterns(np.ones(inp["nptn"]), F.is_informative(inp["states"], inp["n"])), inp["n"])
        assert F.stepwise_addition(old, order)[0] != want_score   # (the input tells stale sites from new ones)
        lnl1, (ot1, ref1) = t.compute_likelihood(), oracle_tree(state)
        assert abs(lnl1 - ref1) <= LNL_RTOL * abs(ref1), (lnl1, ref1)
        check_batch(t, ot1, T)                                    # every candidate against the oracle's minimizeNewton
        assert abs(t.compute_likelihood() - lnl1) <= 1e-12 * abs(lnl1)                 # test_solver_paths_gpu.py:399

        # ---- a new model, then the BIONJ tree of its distances
        state = state._replace(model="gtr2")
        t.set_model(ctx.model(state))
        t.clear_all_partial_lh()
        nwk, steps, last, last_len = t.compute_bionj()
        dist = t.compute_dist()
        rdist, _, _ = restate_matrix(inp["states"], freq, ctx.model(state), None)
        assert np.all(np.abs(dist - rdist) <= 1e-9 * np.maximum(1.0, np.abs(rdist)))   # test_pair_dist_gpu.py assert_matches
        old_dist, _, _ = restate_matrix(inp["states"], freq, ctx.model(ctx.start("dna")), None)
        assert np.max(np.abs(old_dist - rdist)) > 1e-6            # (the input tells a stale model from the new one)
        want = br.bionj(dist)
        assert min(want["guard"]) >= GUARD                        # test_bionj_gpu.py:198-202
        assert_log_matches((steps, last, last_len), want, DEVICE_TOL)
        ids = [str(i) for i in range(T)]
        want_splits = br.log_splits(want["steps"], want["last"], want["last_len"], T)
        assert br.max_split_diff(br.newick_splits(nwk, ids), want_splits) <= 0.5e-8 + DEVICE_TOL
        assert set(br.newick_splits(t.tree_string(), ids)) == set(want_splits)
        assert t.tree_string() == fresh(state, lambda f: f.compute_bionj())
        t.fix_negative_branch(False)
        lnl2, (ot2, ref2) = t.compute_likelihood(), oracle_tree(state)
        assert abs(lnl2 - ref2) <= LNL_RTOL * abs(ref2), (lnl2, ref2)
        check_batch(t, ot2, T)
        pc0 = t.path_counts()
        lnl3 = t.optimize_all_branches(iterations=1, tolerance=1e-9)
        pc = t.path_counts()
        assert pc["sweep_persistent"] == pc0["sweep_persistent"] + 1 and pc["sweep_per_step"] == 0, pc
        ref3 = oracle_tree(state)[1]
        assert lnl3 > lnl2 and abs(lnl3 - ref3) <= 1e-8 * abs(ref3), (lnl3, ref3)      # test_sweep_gpu.py:87
    finally:
        t.close()


# Seeded sequences: 40 actions drawn from the kind's catalogue, a pure function of (kind, seed); the third seed runs in
# LM_PER_NODE.  dna_wide runs under both IQHIP_WIDE4 routes.
SEEDED = [(kind, seed, route) for kind in ES.SEEDED_KINDS for seed in ES.SEEDS
          for route in (("generic", "valu") if kind == "dna_wide" else ("",))]


@pytest.mark.parametrize("kind,seed,route", SEEDED, ids=["%s-%d%s" % (k, s, "-" + r if r else "") for k, s, r in SEEDED])
def test_seeded_sequence(ctx, monkeypatch, kind, seed, route):
    if route:
        monkeypatch.setenv("IQHIP_WIDE4", route)
    seq = ES.seeded_sequence(kind, seed)
    ES.sequence_conditions(ctx, kind)                         # (the generator's, not the engine's)
    r = drive(ctx, ctx.start(kind, ES.seeded_mem_mode(seed), route), seq)
    assert sum(r.counts.values()) == ES.SEQ_LEN
    nn = len(newton_actions(seq))
    assert r.refs["oracle_newton"] == nn and r.stats["solves"] == nn and r.refs["oracle_lnl"] == r.counts["lnl"]
    for ref in ("numpy_rell", "numpy_store", "fitch_ref"):
        assert r.refs[ref] >= 1, (ref, dict(r.refs))
