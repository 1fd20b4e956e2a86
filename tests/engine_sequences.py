"""One long-lived engine driven through interleaved feature calls (helper of test_engine_sequences_{gpu,host}.py).

Every other GPU suite builds an engine for one feature and closes it.  A real caller (the reference's PhyloTree, the
command-line tool) keeps ONE engine through traversals, solves, sweeps, model changes, reweighting and the consumer
features, and the engine carries state between them: residency flags and cached plans (theta_valid, model_version,
plan_cache, keymap_version, tab_model_version, freq_prefix_valid, pars_ready, em.valid, mix.model_version), the launch
parities of the in-kernel solvers (newton_launches, newton_post_launches, batch_launches, the sweep's parity buffers), the
4-state layout switch of set_model_common, the host copies behind the setters and the shared result vector.

  State     everything that defines what an engine should compute: tree string, branch lengths (exact doubles), model,
            ptn_freq, ptn_invar, memory mode, engine kind (+ the IQHIP_WIDE4 route of a wide engine).
  ACTIONS   id -> Action(apply, category, grade).  apply(ctx, tree, state, arg) runs the call with the prerequisite it
            needs itself and returns {name: array}; a state-changing action also returns the new State.
  fresh()   the first comparator: a NEW engine built in exactly the recorded state is given only that action; results are
            cached by a digest of (state, action).
  Runner    drives one live engine, compares every action with fresh() by its grade and with the independent references
            the suite already has (oracle lnL, the oracle's Newton loop, numpy, em_ref and the textbook pruning, mixem_ref,
            lmap_ref cells and quartet trees, fitch_ref, and the restatements of the pair distances, the class lnL, the
            sample generator, the tree tests and the branch tests; bionj_ref in the topology test).

Grades
  "bits"  byte equality: the quantity is promised to have the same bits on every run (its inputs are vectors, which are
          bit-equal whatever plan computed them, and its own reduction order is fixed).
  "lnl"   a value reduced from the root branch of a traversal: byte equality when both engines ran the same plan (the live
          engine evaluates right after clear_all_partial_lh, as the fresh one does), else 1e-12 relative -- the bound
          test_parity_gpu.py::test_many_taxa_plan_chunks_and_key_reuse uses for a tree re-evaluated on recycled buffers.

Every tolerance below is the one of the existing test named beside it; this file introduces none."""
import collections
import ctypes as C
import hashlib

import numpy as np

import em_ref
import fitch_ref as F
import lmap_ref
import mixem_ref
import textbook
from test_branch_tests_host import restate_branch_tests
from test_newton_oracle_gpu import device_newton
from test_parity_gpu import LNL_RTOL
from test_parsimony_gpu import all_directed_ops, slot_of
from test_pair_dist_host import restate_matrix
from test_solver_paths_gpu import X1, X2, XACC, oracle_solve
from test_tree_tests_host import STREAM_RELL, restate_gen, restate_tree_tests, tie_uniforms

LM_PER_NODE, LM_ALL_BRANCH = 0, 1
LAZY_RTOL = 1e-12           # test_parity_gpu.py:600
NBOOT, NROWS = 8, 6
# (max_steps) of the three resident-theta solves: max_steps + 5 <= kNewtonPostEpochs (128) takes the posted exchange, above it
# the arrival counter (solve.hip); 3 ends the loop on the step limit (the fifth set-up of test_newton_oracle_gpu.py)
POSTED_STEPS, COUNTER_STEPS, LIMIT_STEPS = 100, 150, 3

# kind -> nstates, seq_type, ntaxa, npatterns (uncompressed columns: the pattern count is exact), seed
KINDS = collections.OrderedDict([
    ("dna", (4, 0, 9, 330, 7100)),         # 6 tiles of 64: 2 workgroups in k_newton; 24 tiles of 16 while a mixture
    ("dna_wide", (4, 0, 9, 130, 7200)),    # 12 categories: 16-pattern tiles, both IQHIP_WIDE4 routes
    ("prot", (20, 1, 8, 150, 7300)),       # 10 tiles, 3 workgroups
    ("prot_mix", (20, 1, 8, 150, 7400)),   # 3 classes x 2 rates
    ("codon", (64, 2, 7, 70, 7500)),
    # cherry tables (engine.hip cherry_candidate: 20 x 4, nptn_pad >= 8192; plan.hip:386: only plans of >= 8 ops use them, which
    # a tree needs 10 taxa for): the smallest pattern count that pads to 8192.  Fixed sequence only
    ("prot_cherry", (20, 1, 10, 8129, 7600)),
])
SEEDED_KINDS = [k for k in KINDS if k != "prot_cherry"]
CHERRY_PENDANT = 3      # index in edges_of() of (leaf 3, node 14): leaf 5 hangs at node 14 as well


MODEL_NAMES = {"dna": ["gtr", "gtr2", "mix"], "dna_wide": ["gtr", "gtr2"], "prot": ["m", "m2"], "prot_mix": ["mix", "mix2"],
               "codon": ["m", "m2"], "prot_cherry": ["m", "m2"]}


def models_of(synth, kind):
    """name -> model, the first one is the kind's starting model.  ncat cannot change on an attached engine, so a DNA
    mixture has 2 classes x 2 rates = the 4 components of the plain model"""
    n, _, _, _, seed = KINDS[kind]
    if kind == "dna":
        return collections.OrderedDict([
            ("gtr", synth.gtr_model(alpha=0.9, ncat=4)),
            ("gtr2", synth.gtr_model(rates6=(1.1, 3.0, 0.7, 1.3, 3.6, 1.0), freqs=(0.30, 0.20, 0.21, 0.29), alpha=0.5, ncat=4)),
            ("mix", synth.mixture_model(4, 2, seed, ncat=2))])
    if kind == "dna_wide":
        return collections.OrderedDict([
            ("gtr", synth.gtr_model(alpha=0.9, ncat=12)),
            ("gtr2", synth.gtr_model(rates6=(1.1, 3.0, 0.7, 1.3, 3.6, 1.0), freqs=(0.30, 0.20, 0.21, 0.29), alpha=0.5, ncat=12))])
    if kind == "prot_mix":
        return collections.OrderedDict([("mix", synth.mixture_model(20, 3, seed, ncat=2)),
                                        ("mix2", synth.mixture_model(20, 3, seed + 1, alpha=0.6, ncat=2))])
    ncat = 1 if kind == "codon" else 4
    return collections.OrderedDict([("m", synth.random_reversible_model(n, seed, alpha=0.9, ncat=ncat)),
                                    ("m2", synth.random_reversible_model(n, seed + 1, alpha=0.6, ncat=ncat))])


def edges_of(t):
    """every branch once as (a, b), a < b, sorted: the order of State.lengths (and of the oracle's branches)"""
    return sorted((a, b) for a in range(t.num_nodes) for b, _ in t.neighbors(a) if a < b)


def lengths_of(t):
    return tuple(ln for _, ln in sorted(((a, b), ln) for a in range(t.num_nodes) for b, ln in t.neighbors(a) if a < b))


class State(collections.namedtuple("State", "kind route nwk lengths model freq invar mem_mode")):
    """freq / invar are tuples of doubles, lengths follows edges_of() of a tree parsed from nwk"""

    def digest(self):
        h = hashlib.sha256()
        h.update(repr((self.kind, self.route, self.nwk, self.model, self.mem_mode)).encode())
        for v in (self.lengths, self.freq, self.invar):
            h.update(np.asarray(v, dtype=np.float64).tobytes())
        return h.hexdigest()


class Ctx:
    """the packages and the fixed inputs of every kind (alignment, models, parsimony op list), built once"""

    def __init__(self, pkg, synth, oracle):
        self.pkg, self.synth, self.oracle = pkg, synth, oracle
        self._inputs = {}
        self.fresh_cache = {}
        self.fresh_built = 0
        self._oracles = {}
        self._refs = {}

    def cached(self, key, make):
        """a restatement computed once per distinct input"""
        if key not in self._refs:
            self._refs[key] = make()
        return self._refs[key]

    def inputs(self, kind):
        if kind not in self._inputs:
            n, seq_type, ntaxa, nptn, seed = KINDS[kind]
            models = models_of(self.synth, kind)
            base = next(iter(models.values()))
            nwk = self.synth.random_tree_newick(ntaxa, seed)
            su = self.oracle.state_unknown_for(n, seq_type)
            sim = base.classes[0] if hasattr(base, "classes") else base
            states = self.synth.simulate_alignment(nwk, sim, nptn, seed + 1, 0.02, su)
            assert states.shape == (ntaxa, nptn)
            rng = np.random.default_rng(seed + 2)
            adj = F.random_tree(ntaxa, rng)
            ops, slot = all_directed_ops(adj, ntaxa)
            ends = [(slot_of(slot, a, b, ntaxa), slot_of(slot, b, a, ntaxa)) for a, b in F.branches(adj)]
            rows = rng.uniform(-12.0, -1.0, size=(NROWS, nptn))
            assert list(models) == MODEL_NAMES[kind]
            self._inputs[kind] = dict(n=n, seq_type=seq_type, ntaxa=ntaxa, nptn=nptn, seed=seed, nwk=nwk, states=states,
                                      models=models, pars_adj=adj, pars_ops=ops, pars_slot=slot, pars_ends=ends, rows=rows,
                                      su=su)
        return self._inputs[kind]

    def start(self, kind, mem_mode=LM_ALL_BRANCH, route=""):
        inp = self.inputs(kind)
        t = self.pkg.PhyloTree(inp["nwk"])
        lengths = lengths_of(t)
        t.close()
        return State(kind, route, inp["nwk"], lengths, next(iter(inp["models"])), (1.0,) * inp["nptn"], (0.0,) * inp["nptn"],
                     mem_mode)

    def model(self, state):
        return self.inputs(state.kind)["models"][state.model]

    def tree(self, state, engine=True):
        """a tree in exactly this state: an engine of its own (engine=True) or the dry-run mirror that only records plans"""
        inp = self.inputs(state.kind)
        t = self.pkg.PhyloTree(state.nwk)
        t.set_mem_mode(state.mem_mode)
        t.set_alignment(inp["n"], inp["seq_type"], inp["states"], np.array(state.freq), np.array(state.invar))
        t.set_model(self.model(state))
        t.set_likelihood_kernel(self.pkg.LK_EIGEN_HIP)
        edges = edges_of(t)
        assert len(edges) == len(state.lengths)
        for (a, b), ln in zip(edges, state.lengths):
            t.set_branch_length(a, b, ln, clear_reverse=False)
        if engine:
            t.attach_engine(0)
        else:
            t.set_dry_run(True)
        t.set_device_newton(True)
        t.set_device_sweep(True)
        return t

    def oracle_tree(self, state):
        key = state.digest()
        if key not in self._oracles:
            if len(self._oracles) > 64:
                self._oracles.clear()
            inp = self.inputs(state.kind)
            ot = self.oracle.OracleTree(state.nwk, inp["n"], inp["seq_type"], inp["states"], np.array(state.freq),
                                        np.array(state.invar), self.model(state))
            edges = sorted((a, b) for a in ot.adj for b, _ in ot.adj[a] if a < b)
            assert len(edges) == len(state.lengths)
            for (a, b), ln in zip(edges, state.lengths):
                ot.set_length(a, b, ln)
            self._oracles[key] = ot
        ot = self._oracles[key]
        ot.clear()
        return ot


# ------------------------------------------------------------------------------------------
# what a state change does to the record (pure functions of the state: the host replay uses them without an engine)
# ------------------------------------------------------------------------------------------
def new_length(state, k):
    old = state.lengths[k % len(state.lengths)]
    return 0.02 + 0.18 * ((old * 977.0 + 0.37 * k) % 1.0)


def resampled_freq(state, arg):
    """a multinomial resample of the ORIGINAL sites (every frequency 1): about a third of the patterns get 0.  arg 0 puts
    the original frequencies back"""
    nptn = len(state.freq)
    if arg == 0:
        return (1.0,) * nptn
    rng = np.random.default_rng(9000 + arg)
    f = rng.multinomial(nptn, np.full(nptn, 1.0 / nptn)).astype(np.float64)
    assert np.count_nonzero(f == 0.0) >= nptn // 4
    return tuple(f.tolist())


def new_invar(ctx, state, arg):
    """ptn_invar of p-inv = arg / 20 under the kind's first model (phylotreesse.cpp:543-569); arg 0: none"""
    inp = ctx.inputs(state.kind)
    out = np.zeros(inp["nptn"])
    if arg:
        base = next(iter(inp["models"].values()))
        st = inp["states"]
        const = np.all(st == st[0][None, :], axis=0) & (st[0] < inp["n"])
        out[const] = (arg % 10) / 20.0 * np.asarray(base.freqs)[st[0][const]]
    return tuple(out.tolist())


def boot_samples(state):
    """float32 [NBOOT, nptn] multinomial pattern weights of the state's frequencies (set_boot_samples)"""
    f = np.array(state.freq)
    rng = np.random.default_rng(31)
    return rng.multinomial(int(f.sum()), f / f.sum(), size=NBOOT).astype(np.float32)


def class_weights(model):
    return np.array([model.props[model.cat_class == m].sum() for m in range(model.nclass)])


def is_mixture(ctx, state):
    return int(getattr(ctx.model(state), "nclass", 1)) > 1


# ------------------------------------------------------------------------------------------
# the catalogue.  apply(ctx, t, state, arg) -> {name: array} or ({name: array}, new state)
# ------------------------------------------------------------------------------------------
Action = collections.namedtuple("Action", "apply category grade")
ACTIONS = collections.OrderedDict()
STATE, TRAV, SOLVE, CONSUME = "state", "traversal", "solver", "consumer"


def action(name, category, grade):
    def deco(fn):
        ACTIONS[name] = Action(fn, category, grade)
        return fn
    return deco


def split_id(aid):
    name, _, arg = aid.partition("@")
    return name, (int(arg) if arg.lstrip("-").isdigit() else arg)


def arr(x, dtype=np.float64):
    return np.ascontiguousarray(x, dtype=dtype)


def refused(ctx, fn, *a, **kw):
    """the call must be refused by the library, with its message -> {"refused": message bytes}"""
    try:
        fn(*a, **kw)
    except ctx.pkg.HostError as e:
        return {"refused": np.frombuffer(str(e).encode(), dtype=np.uint8).copy()}
    raise AssertionError("%s was not refused" % getattr(fn, "__name__", fn))


def with_state(t, state, **changes):
    return state._replace(lengths=lengths_of(t), **changes)


# ---- state-changing actions.  Every one ends with the vectors cleared the way the mirror's callers do it: the setters of
#      the mirror mark inputs dirty and leave the partial vectors to the caller (phylo_host.cpp setPtnFreq / setMixtureModel),
#      as the reference's do.  grade "bits": they return nothing, the next actions carry the comparison.
@action("set_len_r", STATE, "bits")
def _(ctx, t, state, k):
    """one branch, clear_reverse=True: the reverse vectors of both ends are dropped (iqhost_set_branch_length)"""
    a, b = edges_of(t)[k % len(state.lengths)]
    t.set_branch_length(a, b, new_length(state, k), clear_reverse=True)
    return {}, with_state(t, state)


@action("set_len_n", STATE, "bits")
def _(ctx, t, state, k):
    """one branch, clear_reverse=False followed by clear_all_partial_lh (test_sweep_gpu.py run_both)"""
    a, b = edges_of(t)[k % len(state.lengths)]
    t.set_branch_length(a, b, new_length(state, k), clear_reverse=False)
    t.clear_all_partial_lh()
    return {}, with_state(t, state)


@action("set_model", STATE, "bits")
def _(ctx, t, state, name):
    """a new eigen-system and alpha; "mix" on the dna kind is the 4-state layout switch (engine.hip set_model_common)"""
    new = state._replace(model=name)
    t.set_model(ctx.model(new))
    t.clear_all_partial_lh()
    return {}, new


@action("set_freq", STATE, "bits")
def _(ctx, t, state, arg):
    f = resampled_freq(state, arg)
    t.set_ptn_freq(np.array(f))
    t.clear_all_partial_lh()
    return {}, state._replace(freq=f)


@action("set_invar", STATE, "bits")
def _(ctx, t, state, arg):
    v = new_invar(ctx, state, arg)
    t.set_ptn_invar(np.array(v))
    t.clear_all_partial_lh()
    return {}, state._replace(invar=v)


@action("clear_all", STATE, "bits")
def _(ctx, t, state, arg):
    t.clear_all_partial_lh()
    return {}, state


@action("release", STATE, "bits")
def _(ctx, t, state, arg):
    """every key released, then all vectors cleared (test_parity_gpu.py test_many_taxa_plan_chunks_and_key_reuse)"""
    lib = ctx.pkg.libiqhip()
    keys = {t.neighbor_info(a, b)["key"] for a in range(t.num_nodes) for b, _ in t.neighbors(a)} - {0}
    for k in sorted(keys):
        assert lib.iqhip_release(t.engine, k) == 0, lib.iqhip_last_error()
    t.clear_all_partial_lh()
    return {}, state


@action("timing", STATE, "bits")
def _(ctx, t, state, on):
    """iqhip_timing_enable on (1) / off (0): a property of the live engine only, it must change no result"""
    assert ctx.pkg.libiqhip().iqhip_timing_enable(t.engine, int(on)) == 0
    return {}, state


@action("reset_lengths", STATE, "bits")
def _(ctx, t, state, arg):
    """every branch back to the length the kind starts with (run_both's loop: clear_reverse=False, then all vectors cleared)"""
    start = ctx.start(state.kind).lengths
    for (a, b), ln in zip(edges_of(t), start):
        t.set_branch_length(a, b, ln, clear_reverse=False)
    t.clear_all_partial_lh()
    return {}, state._replace(lengths=start)


CLEARING = ("set_len_n", "set_model", "set_freq", "set_invar", "clear_all", "release", "reset_lengths")   # end with clear_all_partial_lh


# ---- traversal-level actions
def current_branch(t, state, k):
    """branch k becomes the mirror's current branch (iqhost_compute_derv sets current_it), theta of it resident"""
    a, b = edges_of(t)[k % len(state.lengths)]
    t.reset_theta()
    t.compute_likelihood_derv(a, b)
    return a, b


@action("lnl", TRAV, "lnl")
def _(ctx, t, state, arg):
    """grade lnl: one reduction over the root branch of whatever plan is pending (kernels_valu4 / kernels_mfma lnL tail)"""
    return {"lnl": arr([t.compute_likelihood()])}


@action("lnl_branch", TRAV, "lnl")
def _(ctx, t, state, k):
    """re-rooting: the same tree evaluated on another branch.  grade lnl: the fresh engine's plan is the full traversal
    towards that branch, the live engine's only what is pending"""
    a, b = edges_of(t)[k % len(state.lengths)]
    return {"lnl": arr([t.compute_likelihood_branch(a, b)])}


@action("derv_buffer", TRAV, "lnl")
def _(ctx, t, state, k):
    """compute_likelihood_derv + compute_likelihood_from_buffer as a pair.  grade lnl: both reduce theta of the branch,
    which the derivative launch builds together with whatever node updates are pending"""
    a, b = edges_of(t)[k % len(state.lengths)]
    t.reset_theta()          # the mirror's theta_computed is one flag for the whole tree, the caller drops it per branch
    df, ddf = t.compute_likelihood_derv(a, b)
    return {"derv": arr([df, ddf]), "lnl": arr([t.compute_likelihood_from_buffer()])}


@action("vectors", TRAV, "bits")
def _(ctx, t, state, arg):
    """every vector an evaluation on the first branch computes, with its scale counters (compute_likelihood() alone would
    evaluate on the live engine's current branch).  grade bits: a vector's arithmetic depends on its two children and the
    model only, whatever plan it is part of (k_traverse4 / k_traverse_mfma walk one op at a time); the runner compares the
    vectors the fresh engine has, the live one may hold more"""
    t.compute_likelihood_branch(*edges_of(t)[0])
    out = collections.OrderedDict()
    for a in range(t.num_nodes):
        for b, _ in t.neighbors(a):
            info = t.neighbor_info(a, b)
            if t.num_leaves > b or not (info["computed"] & 1) or info["key"] == 0:
                continue
            out["v%d_%d" % (a, b)] = t.fetch_partial(a, b)
            out["s%d_%d" % (a, b)] = arr(t.fetch_scale_num(a, b), np.int16)
    return out


@action("ptn_lh", TRAV, "lnl")
def _(ctx, t, state, k):
    """compute_pattern_likelihood on a given branch: the derivative call makes it the mirror's current branch, the
    evaluation that follows runs there.  grade lnl per pattern: the values come out of the lnL launch"""
    current_branch(t, state, k)
    lnl = t.compute_likelihood()
    return {"lnl": arr([lnl]), "ptn_lh": t.compute_pattern_likelihood()}


@action("ptn_lh_cat", TRAV, "lnl")
def _(ctx, t, state, k):
    """compute_pattern_lh_cat on a given branch (the call rebuilds theta of the current branch itself).  grade lnl: theta
    comes out of the derivative launch together with whatever node updates are pending, as in derv_buffer"""
    current_branch(t, state, k)
    return {"ptn_lh_cat": t.compute_pattern_lh_cat()}


@action("rell", TRAV, "bits")
def _(ctx, t, state, arg):
    """set_boot_samples + compute_rell on a full evaluation.  grade bits: both engines run the same plan (all vectors are
    cleared first) and k_rell sums the patterns in a fixed order (kernels_rell.hip)"""
    t.set_boot_samples(boot_samples(state))
    t.clear_all_partial_lh()
    lnl = t.compute_likelihood()
    return {"lnl": arr([lnl]), "rell": t.compute_rell(), "ptn_lh": t.compute_pattern_likelihood()}


# ---- solver actions
def newton_on_theta(ctx, t, state, k, max_steps, xguess=None):
    """device_newton of test_newton_oracle_gpu.py: theta of the branch resident, one k_newton launch"""
    a, b = edges_of(t)[k % len(state.lengths)]
    t.compute_likelihood()
    t.reset_theta()
    t.compute_likelihood_derv(a, b)
    xg = state.lengths[k % len(state.lengths)] if xguess is None else xguess
    pc0 = t.path_counts()
    optx, d2l, ns = device_newton(ctx.pkg, t, xg, X1, X2, XACC, max_steps)
    pc = t.path_counts()
    assert pc["newton_one_launch"] == pc0["newton_one_launch"] + 1 and pc["newton_chain"] == pc["newton_fallback"] == 0, pc
    return {"newton": arr([optx, d2l, ns])}


# grade bits for the three: theta is a product of two bit-equal vectors, every evaluation reduces it in the fixed order of
# kernels_newton.hip wg_partial + the exchange (wg_exchange.h), so a solve repeats to the bit (test_exchange_forms_gpu.py)
@action("newton_posted", SOLVE, "bits")
def _(ctx, t, state, k):
    return newton_on_theta(ctx, t, state, k, POSTED_STEPS)


@action("newton_counter", SOLVE, "bits")
def _(ctx, t, state, k):
    return newton_on_theta(ctx, t, state, k, COUNTER_STEPS)


@action("newton_limit", SOLVE, "bits")
def _(ctx, t, state, k):
    return newton_on_theta(ctx, t, state, k, LIMIT_STEPS, xguess=3.0)


@action("one_branch", SOLVE, "lnl")
def _(ctx, t, state, k):
    """optimize_one_branch, the fused front end: theta is built inside the first evaluation together with the pending node
    updates, so grade lnl.  The new length enters the state"""
    a, b = edges_of(t)[k % len(state.lengths)]
    pc0 = t.path_counts()
    got = t.optimize_one_branch(a, b)
    pc = t.path_counts()
    assert pc["newton_one_launch"] == pc0["newton_one_launch"] + 1 and pc["newton_chain"] == pc["newton_fallback"] == 0, pc
    return {"length": arr([got])}, with_state(t, state)


def sweep_is_persistent(ctx, state):
    """solve.hip:414: one k_sweep4 launch for a plain 4-state engine on the VALU kernels"""
    return state.kind == "dna" and not is_mixture(ctx, state)


@action("sweep", SOLVE, "lnl")
def _(ctx, t, state, arg):
    """optimize_all_branches, one iteration, in one submission.  grade lnl: the first step's plan is what is pending"""
    pc0 = t.path_counts()
    lnl = t.optimize_all_branches(iterations=1, tolerance=1e-9)
    pc = t.path_counts()
    ran, other = ("sweep_persistent", "sweep_per_step") if sweep_is_persistent(ctx, state) else ("sweep_per_step", "sweep_persistent")
    assert pc[ran] > pc0[ran] and pc[other] == pc0[other] and pc["sweep_sequential"] == 0 and pc["newton_chain"] == 0, (pc0, pc)
    return {"lnl": arr([lnl]), "lengths": arr(lengths_of(t))}, with_state(t, state)


def batch_arrays(batch, key):
    ids = arr([[m["node1"], m["node2"], m["node1_nei"], m["node2_nei"]] for m in batch], np.int32)
    return {"ids": ids, "lens": arr([m[key] for m in batch]), "newloglh": arr([m["newloglh"] for m in batch])}


@action("nni", SOLVE, "bits")
def _(ctx, t, state, arg):
    """evaluate_nnis_batch (k_newton_batch).  grade bits: computeAllPartialLh makes every vector resident first, every task
    then builds its two vectors and theta itself (solve.hip iqhip_optimize_branch_batch).  In LM_PER_NODE the mirror
    refuses (test_nni_batch_gpu.py:44)"""
    if state.mem_mode != LM_ALL_BRANCH:
        out = refused(ctx, t.evaluate_nnis_batch)
        assert b"LM_ALL_BRANCH" in out["refused"].tobytes()
        return out
    return batch_arrays(t.evaluate_nnis_batch(), "new_len")


@action("nni5", SOLVE, "bits")
def _(ctx, t, state, arg):
    """evaluate_nnis5_batch: ten submissions of k_newton_batch over resident vectors; grade bits as nni"""
    if state.mem_mode != LM_ALL_BRANCH:
        out = refused(ctx, t.evaluate_nnis5_batch)
        assert b"LM_ALL_BRANCH" in out["refused"].tobytes()
        return out
    tree0 = t.tree_string()
    out = batch_arrays(t.evaluate_nnis5_batch(), "new_lens")
    assert t.tree_string() == tree0
    return out


# ---- consumer actions.  grade bits for all: each reads vectors / theta of a pinned branch (bit-equal on both engines) or
#      the alignment alone, and sums in a fixed order (the features' own tests assert identical bits on a second call)
def pin_theta(t, state, k):
    a, b = edges_of(t)[k % len(state.lengths)]
    t.compute_likelihood()
    t.reset_theta()
    t.compute_likelihood_derv(a, b)     # current branch = (a, b), theta resident
    return a, b


@action("em", CONSUME, "bits")
def _(ctx, t, state, k):
    """+R EM E-step, objective and site rates (classlh.hip kEmNeeds: refused while the model is a mixture)"""
    a, b = pin_theta(t, state, k)
    if is_mixture(ctx, state):
        out = refused(ctx, t.em_posteriors)
        assert b"iqhip_em_posteriors" in out["refused"].tobytes()
        return out
    cat = t.compute_pattern_lh_cat()    # (of the current branch: the E-step's input, for the reference)
    W, s = t.em_posteriors()
    f, fl = t.em_objective(a, b)
    r, c = t.site_rates()
    return {"cat": cat, "W": W, "cat_sum": s, "F": f, "floored": arr(fl, np.int64), "rate": r, "best": arr(c, np.int32)}


@action("mixem", CONSUME, "bits")
def _(ctx, t, state, k):
    """mix_class_lh + mix_weights_em + mix_posteriors (classlh.hip kMixNeeds: refused unless the model is a mixture)"""
    pin_theta(t, state, k)
    if not is_mixture(ctx, state):
        out = refused(ctx, t.mix_class_lh)
        assert b"iqhip_mix_class_lh" in out["refused"].tobytes()
        return out
    Lc = t.mix_class_lh()
    em = t.mix_weights_em(class_weights(ctx.model(state)), trace=True)
    return {"Lc": Lc, "weights": em["weights"], "trace": em["trace"], "steps": arr([em["steps"], em["converged"]], np.int64),
            "post": t.mix_posteriors()}


@action("mixem_stale", CONSUME, "bits")
def _(ctx, t, state, arg):
    """mix_weights_em with no mix_class_lh since the model was set: refused on every engine, a plain one ("unsupported")
    and a mixture whose matrix belongs to the previous model (mix.model_version, classlh.hip iqhip_mix_weights_em).  Only
    for fixed sequences that place it right behind a set_model"""
    nclass = int(getattr(ctx.model(state), "nclass", 1))
    out = refused(ctx, t.mix_weights_em, np.full(nclass, 1.0 / nclass))
    assert b"iqhip_mix_weights_em" in out["refused"].tobytes()
    refused(ctx, t.mix_posteriors)
    # (the texts differ by history -- "one class", "needs iqhip_mix_class_lh first" -- so only the refusal is compared)
    return {"refused": np.frombuffer(b"iqhip_mix_weights_em", dtype=np.uint8).copy()}


@action("class_lnl", CONSUME, "bits")
def _(ctx, t, state, k):
    a, b = pin_theta(t, state, k)
    if not is_mixture(ctx, state):
        out = refused(ctx, t.class_lnl, a, b, np.ones(1))
        assert b"no mixture" in out["refused"].tobytes()        # (the mirror's own check, phylo_em.cpp classLnl)
        return out
    lnl, fl = t.class_lnl(a, b, class_weights(ctx.model(state)))    # (the weights folded into the components' props)
    return {"class_lnl": lnl, "floored": arr(fl, np.int64)}


def upload_rows(ctx, t, state):
    rows = ctx.inputs(state.kind)["rows"]
    t.ptnlh_reserve(NROWS)
    for r in range(NROWS):
        t.ptnlh_upload(r, rows[r])
    return rows


@action("store", CONSUME, "bits")
def _(ctx, t, state, arg):
    """the row store: ptnlh_reserve, uploaded rows, ptnlh_rell against the samples of set_boot_samples"""
    upload_rows(ctx, t, state)
    t.set_boot_samples(boot_samples(state))
    return {"R": t.ptnlh_rell([3, 1, 5, 1], NBOOT), "row": t.ptnlh_fetch(4)}


TREE_ROWS = [4, 0, 2]


@action("tree_tests", CONSUME, "bits")
def _(ctx, t, state, arg):
    """tree_tests on uploaded rows with device-drawn samples: gen_boot_samples draws from the prefix sums of ptn_freq
    (freq_prefix_valid must follow set_ptn_freq)"""
    rows = upload_rows(ctx, t, state)
    f = np.array(state.freq)
    t.gen_boot_samples(NBOOT, int(f.sum()), 7)
    sel = TREE_ROWS
    return {"R": t.ptnlh_rell(sel, NBOOT), "tests": t.tree_tests(sel, (rows @ f)[sel], NBOOT, tie_seed=11)}


@action("branch_tests", CONSUME, "bits")
def _(ctx, t, state, arg):
    """test_all_branches with a few replicates: ptnlh_put_current of the tree, the batched neighbours, iqhip_branch_tests"""
    t.set_boot_samples(boot_samples(state))
    if state.mem_mode != LM_ALL_BRANCH:
        out = refused(ctx, t.test_all_branches, NBOOT)
        assert b"LM_ALL_BRANCH" in out["refused"].tobytes()
        return out
    t.clear_all_partial_lh()          # the tree's own lnL (row 0, lh[:, 0]) from the same plan on both engines
    sup = t.test_all_branches(NBOOT)
    return {"supports": sup, "rows": np.array([t.ptnlh_fetch(r) for r in range(1 + 2 * len(sup))])}


def ALL_PAIRS(ntaxa):
    return [(i, j) for i in range(ntaxa) for j in range(i + 1, ntaxa)]


@action("pair_counts", CONSUME, "bits")
def _(ctx, t, state, arg):
    pairs = ALL_PAIRS(t.num_leaves)
    if is_mixture(ctx, state):
        out = refused(ctx, t.pair_counts, pairs)
        assert b"iqhip_pair_counts" in out["refused"].tobytes()
        return out
    return {"counts": t.pair_counts(pairs)}


@action("dist", CONSUME, "bits")
def _(ctx, t, state, arg):
    if is_mixture(ctx, state):
        return refused(ctx, t.compute_dist)
    d, d2l = t.compute_dist(want_d2l=True)
    return {"dist": d, "d2l": d2l}


def quartets_of(ntaxa):
    """5 quartets of distinct taxa"""
    rng = np.random.default_rng(77)
    return [tuple(sorted(int(x) for x in rng.choice(ntaxa, size=4, replace=False))) for _ in range(5)]


def quartets_ok(ctx, state):
    return ctx.inputs(state.kind)["n"] == 4 and not is_mixture(ctx, state)


@action("quartet_cells", CONSUME, "bits")
def _(ctx, t, state, arg):
    qs = quartets_of(t.num_leaves)
    if not quartets_ok(ctx, state):
        out = refused(ctx, t.quartet_cells, qs)
        assert b"iqhip_quartet_cells" in out["refused"].tobytes()
        return out
    cells, nother = t.quartet_cells(qs)
    return {"cells": cells, "nother": arr(nother, np.int32)}


@action("quartet_lh", CONSUME, "bits")
def _(ctx, t, state, arg):
    qs = quartets_of(t.num_leaves)
    if not quartets_ok(ctx, state):
        return refused(ctx, t.quartet_likelihoods, qs)
    return {"quartets": t.quartet_likelihoods(qs)}


PARS_MESSAGE = b"needs iqhip_pars_init first (the alignment or its frequencies changed since)"     # pars.hip pars_require


@action("pars", CONSUME, "bits")
def _(ctx, t, state, arg):
    """compute_parsimony and parsimony_branch through the mirror, with NO initialisation of the test's own: after
    set_ptn_freq the mirror has dropped pars_initialized (phylo_host.cpp setPtnFreq) and needParsimony lays the sites out
    again by itself; the engine has dropped pars_ready (engine.hip iqhip_set_ptn_freq) and would refuse the old layout"""
    a, b = edges_of(t)[0]
    sc, sb = t.parsimony_branch(a, b)
    return {"tree_score": arr([t.compute_parsimony()], np.int64), "branch": arr([sc, sb], np.int64),
            "nsites": arr([t.pars_nsites], np.int64)}


@action("pars_raw", CONSUME, "bits")
def _(ctx, t, state, arg):
    """the raw calls on a fixed op list: pars_init + pars_update + pars_branch_scores.  They take the engine's slots, which
    the mirror's own vectors live in, so the engine is handed back to the mirror with initialize_all_partial_pars"""
    inp = ctx.inputs(state.kind)
    nsites = t.pars_init()
    t.pars_update(inp["pars_ops"])
    sc, sb = t.pars_branch_scores(inp["pars_ends"])
    t.initialize_all_partial_pars()
    return {"nsites": arr([nsites], np.int64), "score": arr(sc, np.int32), "subst": arr(sb, np.int32)}


@action("pars_stale", CONSUME, "bits")
def _(ctx, t, state, arg):
    """right behind a set_freq (fixed sequences only): the raw pars_update and pars_branch_scores are refused with the
    documented message until pars_init is repeated (pars_ready), whatever initialised the engine before; then pars_init, and
    they work again"""
    inp = ctx.inputs(state.kind)
    out = refused(ctx, t.pars_update, inp["pars_ops"])
    assert PARS_MESSAGE in out["refused"].tobytes(), out["refused"].tobytes()
    assert PARS_MESSAGE in refused(ctx, t.pars_branch_scores, inp["pars_ends"])["refused"].tobytes()
    nsites = t.pars_init()
    t.pars_update(inp["pars_ops"])
    sc, sb = t.pars_branch_scores(inp["pars_ends"])
    t.initialize_all_partial_pars()
    return {"nsites": arr([nsites], np.int64), "score": arr(sc, np.int32), "subst": arr(sb, np.int32)}


FIXED_ONLY = ("mixem_stale", "pars_stale", "reset_lengths")    # need their place in a sequence: not drawn


def drawn_actions():
    """the action names every seeded sequence draws from.  The list is the same for every kind: a feature a kind's engine
    does not accept stays in as the action that asserts its refusal (RUNS says which those are)"""
    return [n for n in ACTIONS if n not in FIXED_ONLY]


def runs(ctx, state, name):
    """the action runs its feature in this state (False: it asserts the refusal)"""
    mix, n = is_mixture(ctx, state), ctx.inputs(state.kind)["n"]
    if name in ("em", "pair_counts", "dist"):
        return not mix
    if name in ("mixem", "class_lnl"):
        return mix
    if name in ("quartet_cells", "quartet_lh"):
        return n == 4 and not mix
    if name in ("nni", "nni5", "branch_tests"):
        return state.mem_mode == LM_ALL_BRANCH
    return True


# ------------------------------------------------------------------------------------------
# the first comparator: a fresh engine per distinct (state, action)
# ------------------------------------------------------------------------------------------
def run_action(ctx, t, state, aid):
    name, arg = split_id(aid)
    out = ACTIONS[name].apply(ctx, t, state, arg)
    res, new = out if isinstance(out, tuple) else (out, state)
    return collections.OrderedDict((k, np.ascontiguousarray(v)) for k, v in res.items()), new


def fresh(ctx, state, aid):
    key = (state.digest(), aid)
    if key not in ctx.fresh_cache:
        t = ctx.tree(state)
        try:
            ctx.fresh_cache[key] = run_action(ctx, t, state, aid)[0]
        finally:
            t.close()
        ctx.fresh_built += 1
    return ctx.fresh_cache[key]


def compare(aid, grade, same_plan, got, want, where):
    """got: the live engine's, want: the fresh engine's"""
    name, _ = split_id(aid)
    if name == "vectors":      # the live engine may hold more vectors than one evaluation computes
        assert set(want) <= set(got) and len(want) > 0, (where, sorted(want), sorted(got))
        got = {k: got[k] for k in want}
    assert list(got) == list(want), (where, list(got), list(want))
    for k in want:
        g, w = got[k], want[k]
        assert g.shape == w.shape and g.dtype == w.dtype, (where, k, g.shape, w.shape)
        if grade == "bits" or same_plan or g.dtype.kind != "f":
            assert g.tobytes() == w.tobytes(), (where, k, "not the fresh engine's bits", g.ravel()[:4], w.ravel()[:4])
        else:
            np.testing.assert_allclose(g, w, rtol=LAZY_RTOL, atol=0, err_msg=str((where, k)))


# ------------------------------------------------------------------------------------------
# the second comparator: the independent references of the existing suites
# ------------------------------------------------------------------------------------------
def check_reference(ctx, state, aid, got, stats):
    """state: the one the action ran in.  -> the name of the reference that was applied, or None"""
    name, arg = split_id(aid)
    inp = ctx.inputs(state.kind)
    if "refused" in got:
        return None
    freq = np.array(state.freq)
    if name == "lnl":
        ref, _ = ctx.oracle_tree(state).likelihood()
        assert abs(got["lnl"][0] - ref) <= LNL_RTOL * abs(ref), (aid, got["lnl"][0], ref)       # test_parity_gpu.py LNL_RTOL
        return "oracle_lnl"
    if name in ("newton_posted", "newton_counter", "newton_limit"):
        # test_solver_paths_gpu.py run_setups: same evaluation count, optimum to 1e-9, d2l to 1e-6
        ot = ctx.oracle_tree(state)
        a, b = sorted((x, y) for x in ot.adj for y, _ in ot.adj[x] if x < y)[arg % len(state.lengths)]
        ms = {"newton_posted": POSTED_STEPS, "newton_counter": COUNTER_STEPS, "newton_limit": LIMIT_STEPS}[name]
        xg = 3.0 if name == "newton_limit" else ot.length(a, b)
        ref_x, ref_d2l, npts = oracle_solve(ot, a, b, X1, xg, X2, XACC, ms, ot.theta(a, b)[0], stats)
        optx, d2l, ns = got["newton"]
        assert ns == npts, (aid, ns, npts)
        assert abs(optx - ref_x) <= 1e-9 * max(1.0, abs(ref_x)), (aid, optx, ref_x)
        assert abs(d2l - ref_d2l) <= 1e-6 * max(1.0, abs(ref_d2l)), (aid, d2l, ref_d2l)
        return "oracle_newton"
    if name == "rell":
        # test_mixture.py:188: numpy on the fetched pattern likelihoods, 1e-9
        w = boot_samples(state).astype(np.float64)
        want = w @ got["ptn_lh"]
        assert np.all(np.abs(got["rell"] - want) <= 1e-9 * np.abs(got["rell"])), (aid, got["rell"], want)
        return "numpy_rell"
    if name == "em":
        # test_em_gpu.py test_e_step: W = freq * cat / sum(cat) on compute_pattern_lh_cat, rtol 1e-10; em_ref.pattern_rates
        cat, W, model = got["cat"], got["W"], ctx.model(state)
        expect = freq[:, None] * cat / cat.sum(axis=1, keepdims=True)
        np.testing.assert_allclose(W, expect, rtol=1e-10, atol=0)
        np.testing.assert_allclose(got["cat_sum"], expect.sum(axis=0), rtol=1e-10, atol=0)
        np.testing.assert_allclose(got["cat_sum"], W.sum(axis=0), rtol=1e-10, atol=0)
        live = freq > 0          # (a pattern of frequency 0 has no posterior weights to take a rate from)
        ref_rate, ref_cat = em_ref.pattern_rates(cat, model.rates)
        np.testing.assert_allclose(got["rate"][live], ref_rate[live], rtol=1e-10, atol=0)
        assert np.array_equal(got["best"][live], ref_cat[live])
        if not any(state.invar):
            # test_em_gpu.py test_objective: F[c] = <W[:, c], log L of the one-category tree of rate c> on the textbook pruning
            # (that test has no +I case, so none is restated here either)
            from test_em_gpu import TEXTBOOK_ATOL, TEXTBOOK_RTOL, with_rates
            adj, col = ctx.oracle_tree(state).adj, W.sum(axis=0)
            assert np.all(got["floored"] == 0)
            for c in range(len(model.rates)):
                logl = textbook.site_log_likelihoods(adj, inp["states"], with_rates(model, [1.0], [model.rates[c]]), inp["seq_type"],
                                                     inp["su"])
                ref = float(np.dot(W[:, c], logl))
                assert abs(got["F"][c] / col[c] - ref / col[c]) <= TEXTBOOK_ATOL + TEXTBOOK_RTOL * abs(ref / col[c]), (aid, c)
        return "em_ref"
    if name == "mixem":
        # test_mixem_gpu.py test_em_matches_the_restatement_on_the_device_matrix: rtol 1e-10
        model = ctx.model(state)
        ref = mixem_ref.optimize_weights(got["Lc"], freq, np.array(state.invar), class_weights(model), max_steps=model.nclass)
        assert got["steps"][0] == ref["steps"] and got["steps"][1] == ref["converged"]
        np.testing.assert_allclose(got["weights"], ref["prop"], rtol=1e-10, atol=0)
        return "mixem_ref"
    if name == "quartet_cells":
        # test_lmap_gpu.py:85: equal cells, the same number of other patterns
        for q, c, n in zip(quartets_of(inp["ntaxa"]), got["cells"], got["nother"]):
            rc, rother = lmap_ref.cells_ref(inp["states"], freq, q)
            assert np.array_equal(c, rc) and n == len(rother), (aid, q)
        return "lmap_ref"
    if name == "pars":
        # test_parsimony_gpu.py:340-382: the mirror's scores count the parsimony-informative sites, on the NEW frequencies
        sp = F.site_patterns(freq, F.is_informative(inp["states"], inp["n"]))
        tips = F.tip_vectors(inp["states"], sp, inp["n"])
        ot = ctx.oracle_tree(state)
        adj = {u: [v for v, _ in ot.adj[u]] for u in ot.adj}
        assert got["nsites"][0] == len(sp) and got["tree_score"][0] == F.tree_score(adj, tips), aid
        a, b = sorted((x, y) for x in adj for y in adj[x] if x < y)[0]
        dv = F.directed_vectors(adj, tips)
        assert tuple(got["branch"]) == F.branch_score(dv[(a, b)], dv[(b, a)]), aid
        return "fitch_ref"
    if name in ("pars_raw", "pars_stale"):
        # test_parsimony_gpu.py test_updates_and_branch_scores: equal scores, every site of the new frequencies
        tips = F.tip_vectors(inp["states"], F.site_patterns(freq), inp["n"])
        dv = F.directed_vectors(inp["pars_adj"], tips)
        want = [F.branch_score(dv[(a, b)], dv[(b, a)]) for a, b in F.branches(inp["pars_adj"])]
        assert got["score"].tolist() == [w[0] for w in want] and got["subst"].tolist() == [w[1] for w in want], aid
        assert got["nsites"][0] == int(freq.sum())
        return "fitch_raw"
    if name == "dist":
        # test_pair_dist_gpu.py assert_matches: the restated solve of every pair, optimum 1e-9, d2l 1e-6
        rdist, rd2l, _ = ctx.cached(("dist", state.kind, state.model, state.freq),
                                    lambda: restate_matrix(inp["states"], freq, ctx.model(state), None, collections.Counter()))
        for (i, j) in ALL_PAIRS(inp["ntaxa"]):
            assert abs(got["dist"][i, j] - rdist[i, j]) <= 1e-9 * max(1.0, abs(rdist[i, j])), (aid, i, j)
            assert abs(got["d2l"][i, j] - rd2l[i, j]) <= 1e-6 * max(1.0, abs(rd2l[i, j])), (aid, i, j)
        assert np.array_equal(got["dist"], got["dist"].T) and not np.diag(got["dist"]).any()
        return "pair_dist_restatement"
    if name == "quartet_lh":
        # test_lmap_gpu.py compare: sweeps and evaluations equal, logl 1e-8, lengths rtol 1e-7 / atol 1e-12
        res = got["quartets"]
        for qi, q in enumerate(quartets_of(inp["ntaxa"])):
            for k in range(3):
                r = ctx.cached(("quartet", state.kind, state.model, state.freq, q, k),
                               lambda: lmap_ref.quartet_tree_ref(ctx.oracle, inp["states"], freq, q, k, ctx.model(state),
                                                                 float(freq.sum()), 10, 0.1, None))
                assert not r["guard"], ("change the seed", aid, q, k, r["guard"])
                assert res["status"][qi, k] == 0
                assert (res["nsweeps"][qi, k], res["neval"][qi, k]) == (r["nsweeps"], r["neval"]), (aid, q, k)
                assert abs(res["logl"][qi, k] - r["logl"]) <= 1e-8 * abs(r["logl"]), (aid, q, k, res["logl"][qi, k], r["logl"])
                np.testing.assert_allclose(res["len"][qi, k], r["len"], rtol=1e-7, atol=1e-12, err_msg=str((aid, q, k)))
        return "lmap_ref_lh"
    if name == "class_lnl":
        if any(state.invar):      # (test_class_lnl_gpu.py restates +I per class only; the resident ptn_invar is not restated)
            return None
        # test_class_lnl_gpu.py test_folded_class_weights: every class's own model on the textbook pruning, rtol 1e-9
        from test_class_lnl_gpu import RTOL, textbook_lnl
        model, w = ctx.model(state), class_weights(ctx.model(state))
        plain = [ctx.synth.Model(c.Q, c.freqs, c.eval, c.evec, c.inv_evec, c.rates, c.props / w[m], 0.0, c.name)
                 for m, c in enumerate(model.classes)]
        ref = ctx.cached(("class_lnl", state.digest()),
                         lambda: textbook_lnl(ctx.oracle_tree(state), inp["states"], freq, plain, inp["seq_type"], inp["su"]))
        assert np.all(got["floored"] == 0)
        np.testing.assert_allclose(got["class_lnl"], ref, rtol=RTOL, atol=0)
        return "textbook_class_lnl"
    if name == "tree_tests":
        # test_tree_tests_gpu.py: the generator's restatement on the state's frequencies, the product at check_product's
        # bound, restate_tree_tests on the device's sums with equal p-values
        samples = restate_gen(freq, NBOOT, 0, int(freq.sum()), 7, STREAM_RELL).astype(np.float64)
        rows = inp["rows"][TREE_ROWS]
        assert not samples[:, freq == 0].any() and samples.sum(axis=1).tolist() == [int(freq.sum())] * NBOOT
        assert np.all(np.abs(got["R"] - rows @ samples.T) <= 1e-13 * (np.abs(rows) @ samples.T)), aid
        want = restate_tree_tests(got["R"], (inp["rows"] @ freq)[TREE_ROWS], 0.5, None, tie_uniforms(11, len(TREE_ROWS), NBOOT))
        for field, key in (("rell_bp", "bp"), ("kh_pvalue", "kh"), ("sh_pvalue", "sh"), ("rell_confident", "rell_confident"),
                           ("elw_confident", "elw_confident")):
            assert got["tests"][field].tolist() == want[key].tolist(), (aid, field)
        return "tree_tests_restatement"
    if name == "branch_tests":
        # test_branch_tests_gpu.py check_supports / :390: restate_branch_tests fed numpy's sums of the fetched rows
        sup, L, w = got["supports"], got["rows"], boot_samples(state).astype(np.float64)
        for q in range(len(sup)):
            Lq = L[[0, 1 + 2 * q, 2 + 2 * q]]
            for c in range(3):
                assert abs(np.dot(Lq[c], freq) - sup["lh"][q, c]) <= 1e-9 * abs(sup["lh"][q, c]), (aid, q, c)
            r = restate_branch_tests(Lq @ w.T, sup["lh"][q])
            keep = r["margin"] > 1e-9 * (np.abs(Lq) @ np.abs(w).T).max(axis=0)
            lo, hi = int(r["sh"][keep].sum()), int(r["sh"][keep].sum() + (~keep).sum())
            count = sup["sh_alrt"][q] * NBOOT
            assert abs(count - round(count)) < 1e-9 and lo <= round(count) <= hi, (aid, q, count, lo, hi)
            assert abs(sup["abayes"][q] - r["abayes"]) <= 1e-12 * abs(r["abayes"])
            assert abs(sup["alrt_stat"][q] - r["alrt_stat"]) <= 1e-12 * max(1.0, abs(r["alrt_stat"]))
        return "branch_tests_restatement"
    if name == "store":
        # test_branch_tests_gpu.py check_product: numpy float64 at 1e-13 * sum |L W| per element
        rows, w = inp["rows"][[3, 1, 5, 1]], boot_samples(state).astype(np.float64)
        want = rows @ w.T
        assert np.all(np.abs(got["R"] - want) <= 1e-13 * (np.abs(rows) @ np.abs(w).T)), aid
        assert np.array_equal(got["row"], inp["rows"][4])
        return "numpy_store"
    if name == "pair_counts":
        st = inp["states"].astype(np.int64)
        for (i, j), c in zip(ALL_PAIRS(inp["ntaxa"]), got["counts"]):
            want = np.zeros((inp["n"], inp["n"]))
            ok = (st[i] < inp["n"]) & (st[j] < inp["n"])
            np.add.at(want, (st[i][ok], st[j][ok]), freq[ok])
            assert np.array_equal(c, want), (aid, i, j)        # test_pair_dist_host.py restate_counts: integers, exact
        return "numpy_counts"
    return None


# ------------------------------------------------------------------------------------------
# the runner
# ------------------------------------------------------------------------------------------
class Runner:
    """one live engine; run(aid) applies an action, compares it with the fresh engine and the references, advances the
    state.  `toggle_timing` flips iqhip_timing_enable before every second action.  The first failure ends the sequence; its
    message carries the prefix of action ids that led to it."""

    def __init__(self, ctx, state, toggle_timing=False):
        self.ctx, self.state = ctx, state
        self.t = ctx.tree(state)
        self.same_plan = True            # nothing is computed yet: the next evaluation runs the fresh engine's plan
        self.done, self.results = [], []
        self.stats = collections.Counter()
        self.refs = collections.Counter()
        self.counts = collections.Counter()
        self.toggle, self.timing_on = toggle_timing, False

    def close(self):
        self.t.close()

    def run(self, aid):
        ctx = self.ctx
        name, _ = split_id(aid)
        act = ACTIONS[name]
        if self.toggle and len(self.done) % 2 == 1:
            self.timing_on = not self.timing_on
            assert ctx.pkg.libiqhip().iqhip_timing_enable(self.t.engine, int(self.timing_on)) == 0
        before = self.state
        self.done.append(aid)
        where = "after %r" % (self.done,)
        try:
            got, new = run_action(ctx, self.t, before, aid)
            compare(aid, act.grade, self.same_plan, got, fresh(ctx, before, aid), where)
            ref = check_reference(ctx, before, aid, got, self.stats)
        except AssertionError as e:
            raise AssertionError("%s: %s" % (where, e)) from e
        if ref:
            self.refs[ref] += 1
        if "refused" in got:
            assert new == before and lengths_of(self.t) == before.lengths, where
        if name != "timing":
            self.same_plan = name in CLEARING
        self.state = new
        self.counts[name] += 1
        self.results.append(got)
        return got

    def run_all(self, aids):
        for aid in aids:
            self.run(aid)
        return self


# ------------------------------------------------------------------------------------------
# seeded sequences: a pure function of (kind, seed)
# ------------------------------------------------------------------------------------------
SEEDS = (2, 3, 5)      # chosen so that sequence_conditions() and the oracle-only conditions hold for every kind
SEQ_LEN = 40


def seeded_mem_mode(seed):
    """the third seed runs in LM_PER_NODE (buffer stealing; the batch actions assert the mirror's refusal there)"""
    return LM_PER_NODE if seed == SEEDS[-1] else LM_ALL_BRANCH


# the form of the exchange a solver action launches; the two batch actions launch k_newton_batch in LM_ALL_BRANCH only (in
# LM_PER_NODE they assert the mirror's refusal and count for no form)
FORMS = {"newton_posted": "posted", "newton_counter": "counter", "newton_limit": "posted", "one_branch": "posted",
         "sweep": "sweep", "nni": "batch", "nni5": "batch"}


def draw_arg(rng, ctx_models, name, nbranch, model_now):
    if name == "set_model":
        others = [m for m in ctx_models if m != model_now]
        return others[int(rng.integers(len(others)))]
    if name == "set_freq":
        return int(rng.integers(0, 4))
    if name == "set_invar":
        return int(rng.integers(0, 5))
    if name == "timing":
        return int(rng.integers(0, 2))
    if name in ("set_len_r", "set_len_n", "lnl_branch", "derv_buffer", "ptn_lh", "ptn_lh_cat", "newton_posted", "newton_counter",
                "newton_limit", "one_branch", "em", "mixem", "class_lnl"):
        return int(rng.integers(nbranch))
    return 0


def seeded_sequence(kind, seed):
    """every eligible action once, the rest drawn, in a drawn order: [action id]"""
    rng = np.random.default_rng([KINDS[kind][4], seed])
    names = drawn_actions()
    assert len(names) <= SEQ_LEN
    picks = list(names) + [names[int(rng.integers(len(names)))] for _ in range(SEQ_LEN - len(names))]
    picks = [picks[i] for i in rng.permutation(len(picks))]
    models = MODEL_NAMES[kind]
    nbranch = 2 * KINDS[kind][2] - 3
    model_now, out = models[0], []
    for name in picks:
        arg = draw_arg(rng, models, name, nbranch, model_now)
        if name == "set_model":
            model_now = arg
        out.append("%s@%s" % (name, arg))
    return out


def sequence_conditions(ctx, kind):
    """the conditions on the generator's output (properties of the generator alone), counting an action only where it RUNS
    its feature in the state the sequence has reached -- an asserted refusal counts for nothing: per sequence at least 3
    state-changing actions, 3 solves of two forms and 4 consumer calls; over the kind's seeds every action that the kind can
    run at all at least twice"""
    total, can_run = collections.Counter(), set()
    for seed in SEEDS:
        seq = seeded_sequence(kind, seed)
        state = ctx.start(kind, seeded_mem_mode(seed))
        ran = []
        for aid in seq:
            name, arg = split_id(aid)
            if runs(ctx, state, name):
                ran.append(name)
            if name == "set_model":
                state = state._replace(model=arg)
        for model in MODEL_NAMES[kind]:
            for mem_mode in (LM_ALL_BRANCH, LM_PER_NODE):
                st = state._replace(model=model, mem_mode=mem_mode)
                can_run.update(n for n in drawn_actions() if runs(ctx, st, n))
        cats = collections.Counter(ACTIONS[n].category for n in ran)
        solves = [n for n in ran if ACTIONS[n].category == SOLVE]
        assert len(seq) == SEQ_LEN
        assert cats[STATE] >= 3 and len(solves) >= 3 and len({FORMS[n] for n in solves}) >= 2 and cats[CONSUME] >= 4, (kind, seed, cats)
        total.update(ran)
    for n in sorted(can_run):
        assert total[n] >= 2, (kind, n, total[n])
    return total


# ------------------------------------------------------------------------------------------
# fixed sequences (each aims at one piece of shared state; see test_engine_sequences_gpu.py)
# ------------------------------------------------------------------------------------------
def parity_sequence(extra_front):
    """posted, counter, posted, posted, batch, counter, batch, batch, sweep, posted; every solve on another branch"""
    kinds = ["newton_posted", "newton_counter", "newton_posted", "newton_posted", "nni", "newton_counter", "nni", "nni", "sweep",
             "newton_posted"]
    if extra_front:
        kinds = ["newton_posted"] + kinds
    out, k = [], 0
    for n in kinds:
        if n.startswith("newton"):
            out.append("%s@%d" % (n, k))
            k += 1
        else:
            out.append(n + "@0")
    return out


LAYOUT_PASS = ["clear_all@0", "lnl@0", "vectors@0", "newton_posted@1", "newton_counter@4", "nni@0", "sweep@0", "ptn_lh@2", "rell@0",
               # while a mixture: em, dist and quartet_lh assert their refusals, then mixem runs; while plain the other way
               # round (parsimony accepts both: pars.hip pars_require has no model condition)
               "em@3", "dist@0", "quartet_lh@0", "pars@0", "mixem@3"]


def layout_sequence():
    """the pass under plain, mixture, plain; the sweep moved the lengths, so they are put back before each model change and
    the third pass starts in the state of the first"""
    return (LAYOUT_PASS + ["reset_lengths@0", "set_model@mix", "mixem_stale@0"] + LAYOUT_PASS +
            ["reset_lengths@0", "set_model@gtr", "mixem_stale@0"] + LAYOUT_PASS)


CONSUMERS = ["em@2", "mixem@2", "class_lnl@2", "store@0", "tree_tests@0", "branch_tests@0", "pair_counts@0", "dist@0",
             "quartet_cells@0", "quartet_lh@0", "pars@0", "pars_raw@0"]


def model_change_sequence(kind):
    models = MODEL_NAMES[kind]
    return CONSUMERS + ["set_model@" + models[1], "mixem_stale@0"] + CONSUMERS + ["lnl@0", "newton_posted@1"]


REWEIGHT_SET = ["lnl@0", "rell@0", "em@1", "tree_tests@0", "pair_counts@0", "quartet_cells@0", "pars@0"]


def reweight_sequences():
    """set_freq between every ordered pair drawn from REWEIGHT_SET, cut into two ids; each ends with the original
    frequencies put back and the whole set once more"""
    pairs = [(x, y) for i, x in enumerate(REWEIGHT_SET) for y in REWEIGHT_SET[i + 1:]]
    halves = [pairs[:len(pairs) // 2], pairs[len(pairs) // 2:]]
    out = []
    for half in halves:
        seq = list(REWEIGHT_SET)
        for n, (x, y) in enumerate(half):
            seq += [x, "set_freq@%d" % (1 + n % 3), y]
        # parsimony on both sides of a reweighting: the mirror has laid the sites out (pars), the frequencies change, the
        # raw calls are refused until pars_init (pars_stale: the engine's pars_ready), and after the next change the
        # mirror lays them out again by itself (pars: the mirror's pars_initialized)
        seq += ["pars@0", "set_freq@2", "pars_stale@0", "pars@0", "set_freq@3", "pars@0"]
        seq += ["set_freq@0"] + REWEIGHT_SET
        out.append(seq)
    return out


def recycling_sequence(nbranch):
    """LM_PER_NODE: every branch in turn (re-orientation steals buffers), all keys released, one length changed, every
    branch again; a Newton solve after each third evaluation"""
    def walk():
        seq = []
        for k in range(nbranch):
            seq.append("lnl_branch@%d" % k)
            if k % 3 == 2:
                seq.append("newton_posted@%d" % k)
        return seq
    return ["lnl@0"] + walk() + ["release@0", "set_len_r@4"] + walk() + ["lnl@0"]


def is_cherry_pendant(ctx, k):
    """branch k of the prot_cherry tree joins a leaf to a node that carries a second leaf, neither of them leaf 0 (where
    the traversal starts: test_cherry_tables_gpu.py sibling_leaves)"""
    t = ctx.pkg.PhyloTree(ctx.inputs("prot_cherry")["nwk"])
    a, b = edges_of(t)[k]
    nl = t.num_leaves
    ok = 0 < a < nl and any(c != a and 0 < c < nl for c, _ in t.neighbors(b))
    t.close()
    return ok


def cherry_sequence():
    """lnL and all vectors after each of: a model change, a Newton solve and a new length on a cherry's pendant branch,
    the NNI batch (swapped subtrees make new cherries), the model set back, the pendant length set by hand"""
    k = CHERRY_PENDANT
    look = ["lnl@0", "vectors@0"]
    return (look + ["set_model@m2"] + look + ["newton_posted@%d" % k, "one_branch@%d" % k] + look + ["nni@0", "set_model@m"] + look +
            ["set_len_n@%d" % k] + look + ["set_len_r@%d" % k] + look)


def first_pass_equals(results, seq, first, again):
    """the results of the index range `again` equal, to the bit, those of `first` (same action ids)"""
    assert [seq[i] for i in first] == [seq[i] for i in again]
    for i, j in zip(first, again):
        for k in results[i]:
            assert results[i][k].tobytes() == results[j][k].tobytes(), (seq[i], i, j, k)


# ------------------------------------------------------------------------------------------
# replays without a GPU (test_engine_sequences_host.py)
# ------------------------------------------------------------------------------------------
def oracle_replay(ctx, state, seq):
    """the state record through oracle.OracleTree alone: every Newton action's oracle-only conditions (oracle_solve:
    status "ok", no stopping test decided within 1e-6 relative of xacc), the lengths following the oracle's own solves
    (optimize_one_branch: test_solver_paths_gpu.py expected_one_branch; a sweep: lmap_ref.optimize_all_branches)
    -> (final state, Counter of what the solves did)"""
    from test_solver_paths_gpu import expected_one_branch
    stats = collections.Counter()
    for aid in seq:
        name, arg = split_id(aid)
        nb = len(state.lengths)
        if name in ("set_len_r", "set_len_n"):
            ln = list(state.lengths)
            ln[arg % nb] = new_length(state, arg)
            state = state._replace(lengths=tuple(ln))
        elif name == "reset_lengths":
            state = state._replace(lengths=ctx.start(state.kind).lengths)
        elif name == "set_model":
            state = state._replace(model=arg)
        elif name == "set_freq":
            state = state._replace(freq=resampled_freq(state, arg))
        elif name == "set_invar":
            state = state._replace(invar=new_invar(ctx, state, arg))
        elif name in ("newton_posted", "newton_counter", "newton_limit", "one_branch", "sweep"):
            ot = ctx.oracle_tree(state)
            edges = sorted((x, y) for x in ot.adj for y, _ in ot.adj[x] if x < y)
            if name == "sweep":
                res = lmap_ref.optimize_all_branches(ot, 1, 1e-9, x1=X1, x2=X2, max_steps=100)
                assert not res["guard"], (aid, res["guard"])
                stats["sweeps"] += 1
            elif name == "one_branch":
                a, b = edges[arg % nb]
                ot.set_length(a, b, expected_one_branch(ot, a, b, stats))
            else:
                a, b = edges[arg % nb]
                ms = {"newton_posted": POSTED_STEPS, "newton_counter": COUNTER_STEPS, "newton_limit": LIMIT_STEPS}[name]
                xg = 3.0 if name == "newton_limit" else ot.length(a, b)
                oracle_solve(ot, a, b, X1, xg, X2, XACC, ms, ot.theta(a, b)[0], stats)
            state = state._replace(lengths=tuple(ot.length(a, b) for a, b in edges))
    return state, stats


TRAVERSALS = {"lnl": 0, "vectors": 1, "rell": 0, "lnl_branch": 1, "ptn_lh": 2, "ptn_lh_cat": 2, "derv_buffer": 2}


def plan_replay(ctx, state, seq):
    """the traversal-level actions of a sequence on the dry-run mirror (it records the plan of every submission instead of
    sending it); every recorded plan is given to a planning-only engine of the state's shape, whose plan check is always on
    -> number of plans checked"""
    pkg = ctx.pkg
    lib = pkg.libiqhip()
    inp = ctx.inputs(state.kind)
    t = ctx.tree(state, engine=False)
    planner, nchecked = [None, None], 0

    def planner_for(st):
        model = ctx.model(st)
        if planner[1] != st.model:
            if planner[0] is not None:
                lib.iqhip_destroy(planner[0])
            e = C.c_void_p()
            rc = lib.iqhip_debug_create_planner(C.byref(e), inp["n"], len(model.rates), inp["nptn"], inp["ntaxa"], 256, inp["su"],
                                                int(getattr(model, "nclass", 1)))
            assert rc == 0, lib.iqhip_last_error()
            planner[0], planner[1] = e, st.model
        return planner[0]

    try:
        for aid in seq:
            name, arg = split_id(aid)
            if name in ("set_len_r", "set_len_n", "reset_lengths", "set_model", "set_freq", "set_invar", "clear_all"):
                state = run_action(ctx, t, state, aid)[1]
                continue
            if name not in TRAVERSALS:
                continue
            a, b = edges_of(t)[(arg if isinstance(arg, int) else 0) % len(state.lengths)]
            if name == "rell":
                t.clear_all_partial_lh()
            # the mirror keeps the plan of its last submission only, and the derivative call may make two (one per side of
            # the branch): it is replayed as the evaluation on that branch, one plan, followed by the derivative
            calls = [[t.compute_likelihood], [lambda: t.compute_likelihood_branch(a, b)],
                     [lambda: t.compute_likelihood_branch(a, b), lambda: t.compute_likelihood_derv(a, b)]][TRAVERSALS[name]]
            for call in calls:
                call()
                plan = t.last_plan()
                ops = (pkg.NodeOp * max(1, len(plan)))()
                for k, p in enumerate(plan):
                    ops[k] = pkg.NodeOp(p["dst_key"], p["left_key"], p["right_key"], p["left_leaf"], p["right_leaf"],
                                        p["left_len"], p["right_len"], p["flags"], 0)
                assert lib.iqhip_debug_plan(planner_for(state), ops, len(plan)) == 0, (aid, lib.iqhip_last_error())
            nchecked += 1
    finally:
        if planner[0] is not None:
            lib.iqhip_destroy(planner[0])
        t.close()
    return nchecked


def fixed_sequences():
    """id -> (kind, memory mode, [action id]) of every hand-written sequence"""
    out = collections.OrderedDict()
    for kind in ("dna", "prot"):
        for extra in (0, 1):
            out["parities-%s-%s" % (kind, "odd" if extra else "even")] = (kind, LM_ALL_BRANCH, parity_sequence(extra))
    out["layout-dna"] = ("dna", LM_ALL_BRANCH, layout_sequence())
    for kind in ("dna", "prot", "prot_mix"):
        out["model-change-%s" % kind] = (kind, LM_ALL_BRANCH, model_change_sequence(kind))
    for kind in ("dna", "prot"):
        for h, seq in enumerate(reweight_sequences()):
            out["reweight-%s-%d" % (kind, h)] = (kind, LM_ALL_BRANCH, seq)
    out["cherry-prot_cherry"] = ("prot_cherry", LM_ALL_BRANCH, cherry_sequence())
    out["recycling-dna"] = ("dna", LM_PER_NODE, recycling_sequence(2 * KINDS["dna"][2] - 3))
    # found by model-change-prot_mix, its shortest failing prefix: the mirror's mixWeightsEM (and iqhost_mix_posteriors) called
    # the engine without pushing a pending set_model, so the engine compared mix.model_version with the version of the model
    # it still had and ran the EM on the previous model's matrix.  Both now push their inputs first (phylo_em.cpp)
    out["stale-matrix-prot_mix"] = ("prot_mix", LM_ALL_BRANCH, ["mixem@2", "set_model@mix2", "mixem_stale@0", "mixem@2"])
    return out
