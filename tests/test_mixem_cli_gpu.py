"""`iqhip_lnl ... -m 'MIX{...}+G4{..}' [-mixweights]` (cli/iqhip_lnl.cpp): a mixture given on the command line evaluates to the
likelihood of the Python path, and -mixweights prints the class weights PhyloTree.optimize_mixture_weights() estimates."""
import os
import re
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BIN = os.path.join(ROOT, "iq-tree_amd", "lib", "iqhip_lnl")
EXAMPLE = os.path.join(HERE, "golden", "example.phy")
MIX = "MIX{JC,HKY{2.0},GTR{1.5,2.4,1.8,1.9,2.8}+F{0.2,0.3,0.24,0.26}}+G4{0.8}"
LNL_RTOL = 1e-9   # tests/test_parity_gpu.py: two evaluations of one tree that may sum in different orders


def named_tree(nwk, names):
    return re.sub(r"([(,])(\d+):", lambda m: "%s%s:" % (m.group(1), names[int(m.group(2))]), nwk)


def run_cli(args):
    r = subprocess.run([BIN] + args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr + r.stdout
    return r.stdout


def read_report(prefix):
    out = {}
    for line in open(prefix + ".iqhip"):
        k, _, v = line.strip().partition(" ")
        out[k] = v
    return out


@pytest.fixture(scope="module")
def setup(pkg, synth, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("mixcli")
    aln = pkg.Alignment(EXAMPLE)
    nwk = named_tree(synth.random_tree_newick(44, 12), aln.seq_names)
    tf = tmp / "t.nwk"
    tf.write_text(nwk + "\n")
    st, fr, _, _ = aln.arrays()
    model = aln.build_model(MIX)
    t = pkg.PhyloTree(nwk, names=aln.seq_names)
    t.set_alignment(4, 0, st, fr)
    t.set_model(model)
    t.set_likelihood_kernel(pkg.LK_EIGEN_HIP)
    t.attach_engine(0)
    return dict(tmp=tmp, aln=aln, tree_file=str(tf), t=t, model=model, lnl=t.compute_likelihood())


def test_mixture_string_gives_the_python_lnl(setup):
    pre = str(setup["tmp"] / "plain")
    out = run_cli(["-s", EXAMPLE, "-te", setup["tree_file"], "-m", MIX, "-blfix", "-pre", pre])
    rep = read_report(pre)
    print("lnL command line %s, Python %.12f" % (rep["lnL"], setup["lnl"]))
    assert abs(float(rep["lnL"]) - setup["lnl"]) <= LNL_RTOL * abs(setup["lnl"])
    assert abs(float(rep["lnL_input_tree"]) - setup["lnl"]) <= LNL_RTOL * abs(setup["lnl"])
    assert "Log-likelihood of the input tree:" in out and rep["model"] == MIX


def test_mixweights_prints_the_estimated_weights(setup):
    t = setup["t"]
    pre = str(setup["tmp"] / "mw")
    out = run_cli(["-s", EXAMPLE, "-te", setup["tree_file"], "-m", MIX, "-blfix", "-mixweights", "-pre", pre])
    # the command line's loop with -blfix: the EM again while it gains more than 0.01
    cur, res = setup["lnl"], None
    for _ in range(2, 100):
        res = t.optimize_mixture_weights()
        if res["lnl"] > cur + 0.01:
            cur = res["lnl"]
        else:
            break
    m = re.search(r"^Mixture weights:((?: \S+){3})$", out, re.M)
    assert m, out
    printed = np.array([float(x) for x in m.group(1).split()])
    print("printed", printed, "Python", res["weights"])
    np.testing.assert_allclose(printed, res["weights"], rtol=5.1e-6, atol=0)      # %g prints six significant digits
    assert np.max(np.abs(res["weights"] - 1.0 / 3)) > 1e-3 and abs(res["weights"].sum() - 1.0) < 1e-9
    rep = read_report(pre)
    assert abs(float(rep["lnL"]) - res["lnl"]) <= LNL_RTOL * abs(res["lnl"]) and float(rep["lnL"]) > setup["lnl"]
    # the printed model string carries the class rates and the estimated weights and reproduces the likelihood
    mm = re.search(r"^Model with estimated weights: (\S+)$", out, re.M)
    assert mm and rep["model"] == mm.group(1) and mm.group(1).startswith("MIX{JC:") and mm.group(1).endswith("}+G4{0.8}")
    tf = setup["tmp"] / "final.nwk"                          # (all class rates are 1 here: the lengths were not rescaled)
    tf.write_text(rep["tree"] + "\n")
    again = str(setup["tmp"] / "again")
    run_cli(["-s", EXAMPLE, "-te", str(tf), "-m", mm.group(1), "-blfix", "-pre", again])
    assert abs(float(read_report(again)["lnL"]) - float(rep["lnL"])) <= 1e-6


def test_mixweights_with_class_rates(setup):
    """classes of unequal rates: the printed rates are rescaled to mean 1 under the estimated weights and the branch lengths
    with them, so the printed model on the printed tree is the model the run ended with"""
    mix = "MIX{JC:0.5,HKY{2.0}:2,GTR{1.5,2.4,1.8,1.9,2.8}+F{0.2,0.3,0.24,0.26}:1.2}+G4{0.8}"
    pre = str(setup["tmp"] / "mwr")
    out = run_cli(["-s", EXAMPLE, "-te", setup["tree_file"], "-m", mix, "-blfix", "-mixweights", "-pre", pre])
    rep = read_report(pre)
    mm = re.search(r"^Model with estimated weights: (\S+)$", out, re.M)
    assert mm and rep["model"] == mm.group(1)
    fields = re.findall(r":([^:,}]+):([^:,}]+)[,}]", mm.group(1).split("}+G4")[0] + "}")
    rates = np.array([float(a) for a, _ in fields])
    w = np.array([float(b) for _, b in fields])
    printed = np.array([float(x) for x in re.search(r"^Mixture weights:((?: \S+){3})$", out, re.M).group(1).split()])
    print("rates", rates, "weights", w)
    assert rates.size == 3 and abs(w.sum() - 1.0) < 1e-12 and abs(float(np.dot(w, rates)) - 1.0) < 1e-12
    np.testing.assert_allclose(rates / rates[0], np.array([0.5, 2.0, 1.2]) / 0.5, rtol=1e-12)   # the ratios are the given ones
    np.testing.assert_allclose(printed, w, rtol=5.1e-6, atol=0)
    assert np.max(np.abs(w - 1.0 / 3)) > 1e-3 and float(rep["lnL"]) > float(rep["lnL_input_tree"])
    tf = setup["tmp"] / "mwr_final.nwk"
    tf.write_text(rep["tree"] + "\n")
    again = str(setup["tmp"] / "mwr_again")
    run_cli(["-s", EXAMPLE, "-te", str(tf), "-m", mm.group(1), "-blfix", "-pre", again])
    assert abs(float(read_report(again)["lnL"]) - float(rep["lnL"])) <= 1e-6
