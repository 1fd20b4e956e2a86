"""GPU parity over the kernel paths the engine dispatches (engine.hip configure_engine, kernels_mfma.hip launch_traverse):
every category count of the 4-state kernels with both lane splits, the 20- and 64-state
category counts with and without a pipelined instantiation (the one-class mix20 kernel, its component split, the generic
64-state kernel), the documented component caps, and the matrix-core tile edges with each size-chosen variant forced both
ways.  Each case checks lnL, pattern_lh, pattern_lh_cat, every vector and counter, branch lnL, df / ddf and the lnL from
theta against the oracle (test_parity_gpu.check_paths)."""
import numpy as np
import pytest

from test_mixture import make_mix
from test_parity_gpu import check_paths, make_case
from test_sweep_gpu import lengths, run_both

pytestmark = pytest.mark.gpu


def set_env(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def num_cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


# ------------------------------------------------------------------------------------------
# 4 states: k_traverse4 / k_theta4 / k_theta_reduce4 for C = 1..8
# ------------------------------------------------------------------------------------------
DNA_CASES = [(c, None) for c in (1, 3, 5, 7)] + [(c, ls) for c in (2, 4, 6, 8) for ls in ("1", "2")]


@pytest.mark.parametrize("ncat,lane_split", DNA_CASES)
def test_dna_category_counts(pkg, synth, oracle, ncat, lane_split, monkeypatch):
    if lane_split:
        monkeypatch.setenv("IQHIP_LANE_SPLIT", lane_split)
    t, ot, model, *_ = make_case(synth, oracle, pkg, 10, 600, 4, ncat, 1300 + ncat, missing=0.03)
    check_paths(t, ot, model, 10)


@pytest.mark.parametrize("ncat", [3, 8])
def test_dna_workgroup_sizes(pkg, synth, oracle, ncat):
    """11 tiles on workgroups of four waves (kTravWg = 256): 11 waves, or 22 with two lanes per pattern -- the last workgroup is ragged"""
    t, ot, model, *_ = make_case(synth, oracle, pkg, 11, 700, 4, ncat, 1400 + ncat, missing=0.03)
    check_paths(t, ot, model, 11)


@pytest.mark.parametrize("ncat", [3, 8])
def test_persistent_sweep_with_theta_in_memory(pkg, synth, oracle, ncat):
    """k_sweep4<C, reg = false> (kernels_sweep.hip launch_sweep4): more tiles than the persistent grid has waves, so theta
    is re-read from memory.  The pattern count is the smallest that gets there, from sweep4_grid / sweep4_waves: 4 waves
    per workgroup once there are more than 8 tiles, at most 2 workgroups per CU."""
    ntiles = 4 * 2 * num_cus() + 1
    nptn = 64 * ntiles - 17
    grid = min((ntiles + 3) // 4, 2 * num_cus())
    assert ntiles > grid * 4
    model = synth.gtr_model(alpha=0.9, ncat=ncat)
    nwk = synth.random_tree_newick(8, 1500 + ncat)
    st = synth.simulate_alignment(nwk, model, nptn, 1501 + ncat, 0.02, 18)
    freq = np.ones(nptn)

    def make():
        t = pkg.PhyloTree(nwk)
        t.set_alignment(4, 0, st, freq)
        t.set_model(model)
        t.set_likelihood_kernel(pkg.LK_EIGEN_HIP)
        t.attach_engine(0)
        return t
    out = run_both(make, iterations=1, start=0.15)
    (l0, len0, c0, _, _), (l1, len1, c1, _, t1) = out[False], out[True]
    assert len0 == len1 and l0 == l1 and c0 == c1
    pc = t1.path_counts()
    assert pc["sweep_persistent"] >= 1 and pc["sweep_per_step"] == 0, pc
    ot = oracle.OracleTree(t1.tree_string(), 4, 0, st, freq, None, model)
    ref, _ = ot.likelihood()
    assert abs(l1 - ref) <= 1e-8 * abs(ref)
    assert len(lengths(t1)) == 2 * 8 - 3


# ------------------------------------------------------------------------------------------
# 20 and 64 states, plain models: every category count the engine dispatches differently
# ------------------------------------------------------------------------------------------
PROTEIN_CASES = [(c, {}) for c in (1, 2, 3, 5)] + [(c, {"IQHIP_CAT_SPLIT": cs}) for c in (4, 8, 12, 16) for cs in ("0", "1")]


@pytest.mark.parametrize("ncat,env", PROTEIN_CASES, ids=lambda v: str(v) if not isinstance(v, dict) else
                         "-".join("%s=%s" % kv for kv in v.items()) or "default")
def test_protein_category_counts(pkg, synth, oracle, ncat, env, monkeypatch):
    """ncat 1 and 4: the pipelined kernels (4: cat_split forced both ways); every other count: k_traverse_mfma_mix20 with
    one class, with (ncat % 4 == 0) and without its component split"""
    set_env(monkeypatch, env)
    t, ot, model, *_ = make_case(synth, oracle, pkg, 9, 300, 20, ncat, 1600 + ncat, seq_type=1, missing=0.03)
    check_paths(t, ot, model, 9)


CODON_CASES = [(1, {"IQHIP_ROW_SPLIT": "0"}), (1, {"IQHIP_ROW_SPLIT": "1"})] + [(c, {}) for c in (2, 3, 4, 8, 16)]


@pytest.mark.parametrize("ncat,env", CODON_CASES, ids=lambda v: str(v) if not isinstance(v, dict) else
                         "-".join("%s=%s" % kv for kv in v.items()) or "default")
def test_codon_category_counts(pkg, synth, oracle, ncat, env, monkeypatch):
    """ncat 1: the pipelined kernel (row_split forced both ways); ncat > 1: the generic k_traverse_mfma<64, false>, up to
    the cap of 16"""
    set_env(monkeypatch, env)
    t, ot, model, *_ = make_case(synth, oracle, pkg, 8, 250, 64, ncat, 1700 + ncat, seq_type=2, missing=0.03)
    check_paths(t, ot, model, 8)


# ------------------------------------------------------------------------------------------
# the documented caps (engine.hip iqhip_create): 96 components for 20 states, 16 for 64
# ------------------------------------------------------------------------------------------
CAP_CASES = [  # n, seq_type, nclass, ncat, fused, nptn, env
    (20, 1, 24, 4, False, 200, {}),                              # 96 components, mix20 component split (small alignment)
    (20, 1, 24, 4, False, 1500, {"IQHIP_CAT_SPLIT": "0"}),       # ... and the unsplit launch
    (20, 1, 96, 1, True, 200, {}),
    (20, 1, 96, 1, True, 1500, {"IQHIP_CAT_SPLIT": "0"}),
    (64, 2, 8, 2, False, 150, {}),                               # 16 components
    (64, 2, 8, 2, False, 1200, {}),
]


@pytest.mark.parametrize("n,seq_type,nclass,ncat,fused,nptn,env", CAP_CASES)
def test_mixtures_at_the_component_caps(pkg, synth, oracle, n, seq_type, nclass, ncat, fused, nptn, env, monkeypatch):
    set_env(monkeypatch, env)
    model, nwk, pat, freq, ot = make_mix(synth, oracle, n, nclass, ncat, fused, 7, nptn, 1800 + nclass + nptn, seq_type)
    assert model.ncat == (96 if n == 20 else 16)
    t = pkg.PhyloTree(nwk)
    t.set_alignment(n, seq_type, pat, freq)
    t.set_model(model)
    t.attach_engine(0)
    check_paths(t, ot, model, 7, pattern_lh_cat=False)


@pytest.mark.parametrize("nptn", [150, 1200])
def test_codon_plain_model_at_the_cap(pkg, synth, oracle, nptn):
    t, ot, model, *_ = make_case(synth, oracle, pkg, 7, nptn, 64, 16, 1900 + nptn, seq_type=2, missing=0.02)
    check_paths(t, ot, model, 7)


# ------------------------------------------------------------------------------------------
# matrix-core tile edges: 16-pattern tiles, padding to 64; every size-chosen variant forced both ways
# ------------------------------------------------------------------------------------------
EDGE_VARIANTS = [  # n, ncat, env
    (20, 1, {}),
    (20, 4, {"IQHIP_CAT_SPLIT": "1"}),
    (20, 4, {"IQHIP_CAT_SPLIT": "0", "IQHIP_TOP_CS2": "0"}),
    (20, 4, {"IQHIP_CAT_SPLIT": "0", "IQHIP_TOP_CS2": "1"}),
    (20, 8, {"IQHIP_CAT_SPLIT": "0"}),
    (20, 8, {"IQHIP_CAT_SPLIT": "1"}),
    (64, 1, {"IQHIP_ROW_SPLIT": "0"}),
    (64, 1, {"IQHIP_ROW_SPLIT": "1"}),
    (64, 2, {}),
]
EDGE_NPTN = [1, 2, 15, 16, 17, 63, 64, 65, 127, 129]


@pytest.mark.parametrize("nptn", EDGE_NPTN)
@pytest.mark.parametrize("n,ncat,env", EDGE_VARIANTS, ids=lambda v: str(v) if not isinstance(v, dict) else
                         "-".join("%s=%s" % kv for kv in v.items()) or "default")
def test_matrix_core_tile_edges(pkg, synth, oracle, n, ncat, env, nptn, monkeypatch):
    set_env(monkeypatch, env)
    seq_type = 1 if n == 20 else 2
    model = synth.random_reversible_model(n, 2000 + n + ncat, alpha=0.9, ncat=ncat)
    su = oracle.state_unknown_for(n, seq_type)
    nwk = synth.random_tree_newick(7, 2001 + nptn)
    st = np.ascontiguousarray(synth.simulate_alignment(nwk, model, max(nptn, 4), 2002 + nptn, 0.03, su)[:, :nptn])
    freq = np.arange(1, nptn + 1, dtype=np.float64)
    ot = oracle.OracleTree(nwk, n, seq_type, st, freq, None, model)
    t = pkg.PhyloTree(nwk)
    t.set_alignment(n, seq_type, st, freq)
    t.set_model(model)
    t.attach_engine(0)
    check_paths(t, ot, model, 7)
