"""The stand-alone driver's edge-linked partition model: `iqhip_lnl -s aln -q|-spp parts.txt -te tree` on the mixed group
of tests/partition_ref.py written as ONE PHYLIP file (DNA, protein and binary columns) plus a partition file.  The printed
rates, per-partition lnL and total agree with the Python view of the same mirror fed by the same reader."""
import os
import re
import subprocess

import numpy as np
import pytest

import partition_ref as pr

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
BIN = os.path.join(os.path.dirname(HERE), "iq-tree_amd", "lib", "iqhip_lnl")


def run_cli(args):
    return subprocess.run([BIN] + args, capture_output=True, text=True, timeout=300)


def read_report(prefix):
    total, parts = None, []
    for line in open(prefix + ".iqhip"):
        w = line.split()
        if w[0] == "lnL":
            total = float(w[1])
        elif w[0] == "partition":
            parts.append((w[1], float(w[3]), float(w[5])))
    return total, parts


@pytest.fixture(scope="module")
def files(synth, oracle, tmp_path_factory):
    return pr.mixed_files(tmp_path_factory.mktemp("partition_cli"), synth, oracle)


@pytest.mark.parametrize("flag", ["-q", "-spp"])
def test_partition_model_run(pkg, files, tmp_path, flag):
    aln, part, tree, _ = files
    pre = str(tmp_path / "run")
    r = run_cli(["-s", aln, flag, part, "-te", tree, "-pre", pre])
    assert r.returncode == 0, r.stderr + r.stdout
    out = r.stdout
    # the same run through the Python view of the mirror
    names, parts = pkg.read_partition_file(aln, part)
    st = pkg.PhyloSuperTree(open(tree).read(), parts, names=names, fixed_rates=flag == "-q")
    st.optimize_parameters(False, 0.001, 0.001)
    total = st.compute_likelihood()
    lnls, rates = st.part_lnl(), st.part_rates
    rep_total, rep_parts = read_report(pre)
    assert abs(rep_total - total) <= 1e-9 * abs(total)
    assert [p[0] for p in rep_parts] == pr.MIXED_NAMES
    np.testing.assert_allclose([p[1] for p in rep_parts], rates, rtol=1e-9, atol=0)
    np.testing.assert_allclose([p[2] for p in rep_parts], lnls, rtol=1e-9, atol=0)
    m = re.search(r"^Optimal log-likelihood: (\S+)$", out, re.M)
    assert m and abs(float(m.group(1)) - total) <= 1e-6 * abs(total)
    lines = re.findall(r"^Partition (\S+): (\d+) sites, (\d+) patterns, lnL (\S+)$", out, re.M)
    assert [l[0] for l in lines] == pr.MIXED_NAMES
    assert [int(l[1]) for l in lines] == [d["nsite"] for d in parts] == [300, 70, 200, 90]
    assert [int(l[2]) for l in lines] == [d["pat"].shape[1] for d in parts]
    np.testing.assert_allclose([float(l[3]) for l in lines], lnls, rtol=0, atol=1e-6)
    rl = re.search(r"^Partition-specific rates:  (.*)$", out, re.M)
    if flag == "-q":
        assert rl is None and np.array_equal(rates, np.ones(4))
    else:
        np.testing.assert_allclose([float(x) for x in rl.group(1).split()], rates, rtol=1e-5, atol=0)   # 6 significant digits
        nsite = np.array([d["nsite"] for d in parts], dtype=float)
        assert abs(float(np.dot(rates, nsite)) / nsite.sum() - 1.0) <= 1e-12 and rates.max() / rates.min() > 1.1
    # .treefile parses and carries the super tree's lengths
    t = pkg.PhyloTree(open(pre + ".treefile").read(), names)
    assert t.num_leaves == 8
    t2 = pkg.PhyloTree(st.tree_string(), names)
    for a in range(t.num_nodes):
        assert [(b, l) for b, l in t.neighbors(a)] == [(b, l) for b, l in t2.neighbors(a)]
    st.close()


def test_refused_option_combinations(files):
    aln, part, tree, _ = files
    base = ["-s", aln, "-q", part, "-te", tree]
    for extra in (["-m", "JC"], ["-alrt", "100"], ["-z", tree, "-zb", "10"], ["-bb", "100"], ["-mldist", "x.mldist"], ["-pars"],
                  ["-parstree"], ["-bionjtree"], ["-emrates"], ["-mixweights"], ["-optmodel"]):
        for b in (base, ["-s", aln, "-spp", part, "-te", tree]):
            r = run_cli(b + extra)
            assert r.returncode != 0 and "cannot be combined with" in r.stderr, (extra, r.stderr)
    r = run_cli(["-s", aln, "-q", part, "-spp", part, "-te", tree])
    assert r.returncode != 0
