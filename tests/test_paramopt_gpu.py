"""GPU: estimation of model parameters on the device (ModelOptimizer, model_opt_host.h): the reference's BFGS with its
forward-difference stencils batched as the classes of a candidate mixture engine (iqhip_class_lnl), Brent for alpha and
p-inv, the loop of ModelFactory::optimizeParameters.  Reference: tests/modelopt_ref.py, the same routines restated in Python
on textbook likelihoods.
DNA: 12 taxa, 1 500 sites simulated under GTR+G4, start rates 1 and alpha 1, fixed branch lengths.
  1. first stencil: the gradient the batched path hands to the machine against the reference's, per component within
     2 * 1e-9 * |lnL| / h (the lnL bound of the class values and the step; nothing measured).
  2. invariants: the lnL in the trace never falls by more than 1e-6; the end is more than 1.0 above the start; traversals per
     stencil = ceil(ndim / (K - 1)) (6 points, K = 6: one); no stencil redone.
  3. against the reference run: relative difference of the six estimates and the difference in lnL, bounds at ten times the
     values measured once on the MI355X (MEASURED_DNA below), ceilings 5e-3 and 0.01.
  4. batch=True and batch=False end within the same bounds of each other; the batched run takes fewer traversals.
  5. two batched runs give identical bits.
  6. protein: 10 taxa x 400 sites, a random reversible matrix (written as a PAML file) +I+G4, optimize_rates() against the
     reference, same rule for the bounds.
  7. with branch lengths (fixed_len=False): lnL monotone, the end not below the fixed-length one, the loop stops by its gain
     rule within 99 rounds."""
import math

import numpy as np
import pytest

import modelopt_ref

pytestmark = pytest.mark.gpu

# Bounds of check 3 / 4 / 6: ten times the differences measured once on the MI355X between the device run and the restated
# run, under the ceilings 5e-3 (parameters, relative) and 0.01 (lnL): two correct runs may part ways on near-equal
# line-search values, and logl_epsilon = 0.01 is the loop's own resolution (the precedent: EM_RATE_RTOL, test_em_gpu.py).
# Measured (also in DESIGN.md section 3.12):
#   DNA, device against the restated run:      parameters 5.277e-09 relative, lnL 5.230e-09
#   DNA, batched against sequential:           parameters 1.439e-08 relative, lnL 7.443e-09   (held to the DNA bounds)
#   protein, device against the restated run:  parameters 1.355e-07 relative, lnL 8.359e-09
PARAM_RTOL_CEILING, LNL_ATOL_CEILING = 5e-3, 0.01
MEASURED_DNA = dict(param_rel=5.277e-09, lnl_abs=5.230e-09)
MEASURED_PROTEIN = dict(param_rel=1.355e-07, lnl_abs=8.359e-09)


def bounds(measured):
    return min(PARAM_RTOL_CEILING, 10.0 * measured["param_rel"]), min(LNL_ATOL_CEILING, 10.0 * measured["lnl_abs"])


# The data set.  Preconditions on the REFERENCE run alone, checked on the CPU before any device run: (a) it ends in the
# interior (asserted below), and (b) it does not part ways with itself: repeated with every likelihood value perturbed by a
# pseudo-random relative 3e-15 (what two correct implementations differ by), the restated run with this seed returns the same
# estimates to 6 digits in two trials.  Seeds 9100 and 9110 of the same recipe fail (b): their perturbed runs move the
# estimates by 1e-2 and 5e-3 (a BFGS termination test or a line-search acceptance flips, and the runs end an iteration
# apart on a flat surface), so no implementation could be held to the ceiling there; 9120 and 9130 pass.
DNA_SEED = 9120
DNA_LETTERS = "ACGT"
AA_LETTERS = "ARNDCQEGHILKMFPSTWYV"


def phylip(states, letters):
    ntaxa, nsites = states.shape
    lines = ["%d %d" % (ntaxa, nsites)]
    for t in range(ntaxa):
        lines.append("%d %s" % (t, "".join(letters[s] for s in states[t])))
    return "\n".join(lines) + "\n"


def fmt(v):
    return ",".join("%.17g" % x for x in v)


def device_tree(pkg, nwk, aln, model_string):
    """a tree holding aln's patterns with the model of the string (all values given), engine attached"""
    st, fr, _, _ = aln.arrays()
    m = aln.build_model(model_string)
    t = pkg.PhyloTree(nwk)
    t.set_alignment(aln.nstates, aln.seq_type, st, fr, aln.ptn_invar(m.p_invar, m.state_freq))
    t.set_model(m)
    t.set_likelihood_kernel(pkg.LK_EIGEN_HIP)
    t.attach_engine(0)
    return t, st, fr


@pytest.fixture(scope="module")
def dna(pkg, synth, oracle):
    truth = synth.gtr_model(rates6=(1.8, 4.2, 0.7, 1.3, 5.1, 1.0), freqs=(0.3, 0.2, 0.22, 0.28), alpha=0.6, ncat=4)
    nwk = synth.random_tree_newick(12, DNA_SEED, 0.03, 0.25)
    states = synth.simulate_alignment(nwk, truth, 1500, DNA_SEED + 1, 0.0, 18)
    aln = pkg.Alignment(content=phylip(states, DNA_LETTERS), seq_type="DNA")
    freqs = aln.state_freq()
    freqs = freqs / freqs.sum()
    base = "+F{%s}+G4" % fmt(freqs)
    start = "GTR{1,1,1,1,1}+F{%s}+G4{1}" % fmt(freqs)
    t, st, fr = device_tree(pkg, nwk, aln, start)
    ot = oracle.OracleTree(nwk, 4, 0, st, fr, None, truth)
    pb = modelopt_ref.Problem(synth, ot.adj, st, fr, 0, 18, modelopt_ref.gtr_exch, freqs, 4, True, False, aln.frac_const_sites)
    grads = []
    modelopt_ref.optimize_model(pb, [1.0] * 5, 1.0, 0.0, gradients=grads)      # (the first call of the reference loop)
    ref = modelopt_ref.optimize_parameters(pb, [1.0] * 5, 1.0, 0.0)
    # the device runs
    lnl0 = t.compute_likelihood()
    opt = pkg.ModelOptimizer(t, aln, "GTR" + base, batch=True)
    lnl = opt.optimize_parameters(fixed_len=True)
    return dict(nwk=nwk, aln=aln, base=base, start=start, t=t, pb=pb, ref=ref, ref_grad0=grads[0], lnl0=lnl0, opt=opt, lnl=lnl,
                trace=opt.trace, values=opt.values(), string=opt.model_string(), rounds=opt.rounds)


def rel_diff(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.abs(b)))


def estimates(values):
    return list(values["params"]) + [values["alpha"]]


def test_first_stencil_gradient(dna):
    call = dna["trace"][0]
    assert call["what"] == "model" and call["K"] == 6 and len(call["grad0"]) == 5
    assert np.array_equal(call["x0"], np.ones(5))
    ref = np.array(dna["ref_grad0"])
    lnl = abs(call["values0"][0])
    bound = 2.0 * 1e-9 * lnl / call["h0"]
    print("gradient device %s reference %s bound %s" % (call["grad0"], ref, bound))
    assert np.all(np.abs(call["grad0"] - ref) <= bound)
    assert abs(-call["values0"][0] - dna["pb"].lnl([1.0] * 5, 1.0, 0.0)) <= 1e-9 * lnl


def test_invariants(dna):
    trace = dna["trace"]
    prev = dna["lnl0"]
    for c in trace:
        print(c["what"], c["requests"], c["stencils"], c["stencil_traversals"], c["single_traversals"], c["lnl_before"], c["lnl_after"])
        assert c["lnl_before"] >= prev - 1e-6 and c["lnl_after"] >= c["lnl_before"] - 1e-6
        prev = c["lnl_after"]
        assert c["stencils_redone"] == 0
        if c["what"] == "model":
            assert c["K"] == 6 and c["stencils"] >= 1
            assert c["stencil_traversals"] == c["stencils"] * math.ceil(5 / (c["K"] - 1))
        else:
            assert c["stencils"] == 0 and c["stencil_traversals"] == 0
    assert dna["lnl"] > dna["lnl0"] + 1.0
    assert abs(dna["t"].compute_likelihood() - dna["lnl"]) <= 0.01 + 1e-6     # (the loop returns the value of its last accepted round)
    assert 2 <= dna["rounds"] + 1 < 99


def test_against_the_reference_run(dna):
    ref = dna["ref"]
    # precondition, CPU: the reference run ends in the interior, so the unrestated boundary restart never applies
    for p in ref["params"]:
        assert 1e-4 + 1e-4 < p < 100.0 - 1e-4
    assert 0.02 + 1e-4 < ref["alpha"] < 1000.0 - 1e-4
    got, want = estimates(dna["values"]), list(ref["params"]) + [ref["alpha"]]
    final = dna["t"].compute_likelihood()
    d_par, d_lnl = rel_diff(got, want), abs(final - ref["lnl"])
    print("device %s lnL %.6f\nreference %s lnL %.6f\nMEASURED dna: param_rel %.3e lnl_abs %.3e" % (got, final, want, ref["lnl"],
                                                                                                d_par, d_lnl))
    rtol, atol = bounds(MEASURED_DNA)
    assert d_par <= rtol and d_lnl <= atol
    # the printed string holds the estimates in full precision
    m = dna["aln"].build_model(dna["string"])
    assert m.ncat == 4 and dna["string"].startswith("GTR{") and "+G4{" in dna["string"]


def test_batched_and_sequential_agree(dna, pkg):
    t, _, _ = device_tree(pkg, dna["nwk"], dna["aln"], dna["start"])
    seq = pkg.ModelOptimizer(t, dna["aln"], "GTR" + dna["base"], batch=False)
    seq.optimize_parameters(fixed_len=True)
    final_seq, final = t.compute_likelihood(), dna["t"].compute_likelihood()
    d_par, d_lnl = rel_diff(estimates(seq.values()), estimates(dna["values"])), abs(final_seq - final)
    trav_seq = sum(c["single_traversals"] + c["stencil_traversals"] for c in seq.trace)
    trav = sum(c["single_traversals"] + c["stencil_traversals"] for c in dna["trace"])
    print("MEASURED batch vs sequential: param_rel %.3e lnl_abs %.3e, traversals %d batched / %d sequential" % (d_par, d_lnl, trav, trav_seq))
    rtol, atol = bounds(MEASURED_DNA)
    assert d_par <= rtol and d_lnl <= atol
    assert all(c["K"] == 0 and c["stencil_traversals"] == 0 for c in seq.trace)
    assert trav < trav_seq


def test_reproducible(dna, pkg):
    t, _, _ = device_tree(pkg, dna["nwk"], dna["aln"], dna["start"])
    again = pkg.ModelOptimizer(t, dna["aln"], "GTR" + dna["base"], batch=True)
    lnl = again.optimize_parameters(fixed_len=True)
    assert lnl == dna["lnl"] and again.model_string() == dna["string"]
    assert np.array_equal(estimates(again.values()), estimates(dna["values"]))


def test_with_branch_lengths(dna, pkg):
    t, _, _ = device_tree(pkg, dna["nwk"], dna["aln"], dna["start"])
    opt = pkg.ModelOptimizer(t, dna["aln"], "GTR" + dna["base"], batch=True)
    lnl0 = t.compute_likelihood()
    lnl = opt.optimize_parameters(fixed_len=False)
    prev = lnl0
    for c in opt.trace:
        assert c["lnl_before"] >= prev - 1e-6 and c["lnl_after"] >= c["lnl_before"] - 1e-6     # branch sweeps in between only raise it
        prev = c["lnl_after"]
        assert c["stencils_redone"] == 0
    final = t.compute_likelihood()
    print("with branch lengths: %.6f (fixed lengths %.6f), %d rounds" % (final, dna["t"].compute_likelihood(), opt.rounds))
    assert final >= dna["t"].compute_likelihood() - 1e-6 and abs(final - lnl) <= 1e-6 * abs(final)
    assert opt.rounds + 1 < 99


def test_protein_rates(pkg, synth, oracle, tmp_path):
    rng = np.random.default_rng(9200)
    R = rng.gamma(shape=1.0, scale=1.0, size=(20, 20)) + 0.05
    R = (R + R.T) / 2.0
    freqs = rng.dirichlet(np.full(20, 5.0))
    truth = synth.reversible_model(R, freqs, 0.7, 4, 0.15)
    paml = tmp_path / "random.paml"
    with open(paml, "w") as f:
        for i in range(1, 20):
            f.write(" ".join("%.17g" % R[i, j] for j in range(i)) + "\n")
        f.write("\n" + " ".join("%.17g" % x for x in freqs) + "\n")
    nwk = synth.random_tree_newick(10, 9201, 0.05, 0.3)
    states = synth.simulate_alignment(nwk, truth, 400, 9202, 0.0, 23)
    states[:, :60] = states[0:1, :60]                        # constant columns: p-inv has something to find
    aln = pkg.Alignment(content=phylip(states, AA_LETTERS), seq_type="AA")
    a0, p0 = 3.0, 0.02                                       # given in braces: starting values, away from the estimate
    t, st, fr = device_tree(pkg, nwk, aln, "%s+I{%.17g}+G4{%.17g}" % (paml, p0, a0))
    ot = oracle.OracleTree(nwk, 20, 1, st, fr, None, truth)
    file_freq = freqs / freqs.sum()
    pb = modelopt_ref.Problem(synth, ot.adj, st, fr, 1, 23, lambda params: R, file_freq, 4, True, True, aln.frac_const_sites)
    alpha, pinv, ref_lnl = modelopt_ref.optimize_rates(pb, (), a0, p0)
    assert 0.02 + 1e-4 < alpha < 1000.0 - 1e-4 and 1e-6 + 1e-4 < pinv < aln.frac_const_sites - 1e-4     # interior
    opt = pkg.ModelOptimizer(t, aln, "%s+I{%.17g}+G4{%.17g}" % (paml, p0, a0))
    assert opt.optimize_model() == 0.0                       # no free rate parameter
    lnl0 = t.compute_likelihood()
    assert abs(lnl0 - pb.lnl((), a0, p0)) <= 1e-9 * abs(lnl0)
    lnl = opt.optimize_rates()
    v = opt.values()
    d_par, d_lnl = rel_diff([v["alpha"], v["p_invar"]], [alpha, pinv]), abs(lnl - ref_lnl)
    print("protein: device alpha %.8f p-inv %.8f lnL %.6f; reference %.8f %.8f %.6f\nMEASURED protein: param_rel %.3e lnl_abs %.3e"
          % (v["alpha"], v["p_invar"], lnl, alpha, pinv, ref_lnl, d_par, d_lnl))
    rtol, atol = bounds(MEASURED_PROTEIN)
    assert d_par <= rtol and d_lnl <= atol
    assert lnl > lnl0 + 1.0 and [c["what"] for c in opt.trace] == ["alpha", "pinv"]
    assert "Proportion of invariable sites: " in opt.write_info() and "Gamma shape alpha: " in opt.write_info()
