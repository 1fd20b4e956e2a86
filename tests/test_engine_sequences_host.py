"""CPU: the inputs of test_engine_sequences_gpu.py are what that suite needs them to be -- properties of the generator and of
the oracle alone, checked without an engine.

  * the seeded draw is a pure function of (kind, seed), and the committed seeds meet the suite's conditions: at least 3
    state-changing actions, 3 solves of two forms and 4 consumer calls per sequence, every eligible action at least twice
    over a kind's seeds
  * every fixed sequence names only actions of the catalogue, with arguments they accept
  * the oracle-only conditions of the Newton actions (test_solver_paths_gpu.py oracle_solve: status "ok", no stopping test
    decided within 1e-6 relative of xacc) hold along every sequence, the state record replayed through oracle.OracleTree
  * the traversal-level actions of every sequence, replayed on the dry-run mirror, give plans that pass the plan check of a
    planning-only engine"""
import pytest

import engine_sequences as ES


@pytest.fixture(scope="module")
def ctx(pkg, synth, oracle):
    return ES.Ctx(pkg, synth, oracle)


def all_sequences():
    """id -> (kind, memory mode, sequence): the fixed ones and the seeded ones"""
    out = ES.fixed_sequences()
    for kind in ES.SEEDED_KINDS:
        for seed in ES.SEEDS:
            out["seeded-%s-%d" % (kind, seed)] = (kind, ES.seeded_mem_mode(seed), ES.seeded_sequence(kind, seed))
    return out


def test_the_draw_is_a_pure_function_of_kind_and_seed():
    for kind in ES.SEEDED_KINDS:
        seqs = [ES.seeded_sequence(kind, s) for s in ES.SEEDS]
        assert seqs == [ES.seeded_sequence(kind, s) for s in ES.SEEDS]
        assert len({tuple(s) for s in seqs}) == len(ES.SEEDS)
    assert ES.seeded_sequence("dna", 1) != ES.seeded_sequence("prot", 1)


@pytest.mark.parametrize("kind", ES.SEEDED_KINDS)
def test_committed_seeds_meet_the_conditions(ctx, kind):
    ran = ES.sequence_conditions(ctx, kind)
    print(kind, "actions that run their feature over the seeds:", dict(ran))


def test_sequences_name_only_actions_of_the_catalogue():
    for sid, (kind, mem_mode, seq) in all_sequences().items():
        models = ES.MODEL_NAMES[kind]
        assert kind in ES.KINDS and mem_mode in (ES.LM_PER_NODE, ES.LM_ALL_BRANCH) and len(seq) > 0
        for aid in seq:
            name, arg = ES.split_id(aid)
            assert name in ES.ACTIONS, (sid, aid)
            assert (arg in models) if name == "set_model" else isinstance(arg, int), (sid, aid)
    # every action of the catalogue is used by some sequence, and every category by every seeded one
    used = {ES.split_id(a)[0] for _, _, seq in all_sequences().values() for a in seq}
    assert used == set(ES.ACTIONS)


def test_the_cherry_sequence_works_on_a_cherry(ctx):
    assert ES.is_cherry_pendant(ctx, ES.CHERRY_PENDANT)
    n, _, ntaxa, nptn, _ = ES.KINDS["prot_cherry"]
    assert (n, ntaxa - 2) == (20, 8) and (nptn + 63) // 64 * 64 == 8192 and (nptn - 1 + 63) // 64 * 64 < 8192


SEQUENCE_IDS = list(all_sequences())


@pytest.mark.parametrize("sid", SEQUENCE_IDS)
def test_oracle_conditions_hold_along_the_sequence(ctx, sid):
    kind, mem_mode, seq = all_sequences()[sid]
    state, stats = ES.oracle_replay(ctx, ctx.start(kind, mem_mode), seq)
    nsolves = sum(1 for a in seq if ES.split_id(a)[0] in ("newton_posted", "newton_counter", "newton_limit", "one_branch"))
    assert stats["solves"] == nsolves, (stats, nsolves)
    assert len(state.lengths) == 2 * ES.KINDS[kind][2] - 3 and all(ES.X1 <= x <= ES.X2 for x in state.lengths)


@pytest.mark.parametrize("sid", SEQUENCE_IDS)
def test_plans_of_the_sequence_pass_the_plan_check(ctx, sid, monkeypatch):
    monkeypatch.setenv("IQHIP_CHECK_PLAN", "1")
    kind, mem_mode, seq = all_sequences()[sid]
    ntrav = sum(1 for a in seq if ES.split_id(a)[0] in ES.TRAVERSALS)
    assert ES.plan_replay(ctx, ctx.start(kind, mem_mode), seq) == ntrav
