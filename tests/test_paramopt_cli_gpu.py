"""GPU: iqhip_lnl -optmodel.  `-m GTR+I+G4 -optmodel` on the example alignment prints the reference's four lines and a model
string with the estimates; feeding that string back without -optmodel (on the tree the run printed, lengths fixed)
reproduces the printed lnL to 1e-6; -blfix leaves the branch lengths alone."""
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BIN = os.path.join(ROOT, "iq-tree_amd", "lib", "iqhip_lnl")
EXAMPLE = os.path.join(HERE, "golden", "example.phy")


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


def line_value(out, head):
    lines = [l for l in out.splitlines() if l.startswith(head)]
    assert len(lines) == 1, (head, out)
    return lines[0][len(head):].strip()


def branch_lengths(nwk):
    return sorted(float(x) for x in re.findall(r":([0-9.eE+-]+)", nwk))


@pytest.fixture(scope="module")
def tree_file(pkg, synth, tmp_path_factory):
    aln = pkg.Alignment(EXAMPLE)
    nwk = named_tree(synth.random_tree_newick(44, 12), aln.seq_names)
    tf = tmp_path_factory.mktemp("optmodel") / "t.nwk"
    tf.write_text(nwk + "\n")
    return str(tf), nwk


def check_output(out):
    """the four lines and the model string -> (lnL, model string)"""
    lnl = float(line_value(out, "Optimal log-likelihood:"))
    alpha = float(line_value(out, "Gamma shape alpha:"))
    pinv = float(line_value(out, "Proportion of invariable sites:"))
    rates = line_value(out, "Rate parameters:")
    assert re.fullmatch(r"A-C: \S+  A-G: \S+  A-T: \S+  C-G: \S+  C-T: \S+  G-T: 1", rates), rates
    model = line_value(out, "Model with estimated parameters:")
    m = re.fullmatch(r"GTR\{([^}]*)\}\+I\{([^}]*)\}\+G4\{([^}]*)\}", model)
    assert m, model
    assert len(m.group(1).split(",")) == 5
    assert abs(float(m.group(2)) - pinv) <= 1e-5 * pinv and abs(float(m.group(3)) - alpha) <= 1e-5 * alpha   # (6 digits printed)
    assert 0.02 < alpha < 1000.0 and 1e-6 <= pinv < 1.0
    assert "1. Initial log-likelihood:" in out
    return lnl, model


def test_optmodel_estimates_and_the_string_reads_back(tree_file, tmp_path):
    tf, _ = tree_file
    pre = str(tmp_path / "opt")
    out = run_cli(["-s", EXAMPLE, "-te", tf, "-m", "GTR+I+G4", "-optmodel", "-pre", pre])
    lnl, model = check_output(out)
    rep = read_report(pre)
    assert rep["model"] == model and float(rep["lnL"]) == lnl
    assert lnl > float(rep["lnL_input_tree"]) + 1.0          # rates 1, alpha 1, p-inv frac_const / 2 on the input tree
    # the string, without -optmodel, on the tree the run printed
    tf2 = tmp_path / "opt.nwk"
    tf2.write_text(rep["tree"] + "\n")
    pre2 = str(tmp_path / "back")
    run_cli(["-s", EXAMPLE, "-te", str(tf2), "-m", model, "-blfix", "-pre", pre2])
    back = float(read_report(pre2)["lnL"])
    print("optmodel lnL %.9f, read back %.9f" % (lnl, back))
    assert abs(back - lnl) <= 1e-6


def test_optmodel_honours_blfix(tree_file, tmp_path):
    tf, nwk = tree_file
    pre = str(tmp_path / "fix")
    out = run_cli(["-s", EXAMPLE, "-te", tf, "-m", "GTR+I+G4", "-optmodel", "-blfix", "-pre", pre])
    lnl, model = check_output(out)
    rep = read_report(pre)
    assert branch_lengths(rep["tree"]) == branch_lengths(nwk)            # untouched
    assert lnl > float(rep["lnL_input_tree"]) + 1.0
    pre2 = str(tmp_path / "back")
    run_cli(["-s", EXAMPLE, "-te", tf, "-m", model, "-blfix", "-pre", pre2])
    assert abs(float(read_report(pre2)["lnL"]) - lnl) <= 1e-6
    # braces are starting values: the same optimum from another start, within the loop's resolution
    pre3 = str(tmp_path / "start")
    out3 = run_cli(["-s", EXAMPLE, "-te", tf, "-m", "GTR{2,2,2,2,2}+I{0.05}+G4{0.5}", "-optmodel", "-blfix", "-pre", pre3])
    lnl3, _ = check_output(out3)
    assert abs(lnl3 - lnl) <= 0.1
