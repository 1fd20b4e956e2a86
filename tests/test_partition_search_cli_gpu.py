"""The stand-alone driver's NNI tree search on an edge-linked partition model: `iqhip_lnl -s aln -spp parts -t tree -n 2` on
the mixed group of tests/partition_ref.py -- optimizeParameters, the search on the super tree, optimizeParameters again, the
per-partition lines, `Optimal log-likelihood:` and <prefix>.treefile -- and the combinations that stay refused."""
import os
import re
import subprocess

import pytest

import partition_ref as pr

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
BIN = os.path.join(os.path.dirname(HERE), "iq-tree_amd", "lib", "iqhip_lnl")


def run_cli(args):
    return subprocess.run([BIN] + args, capture_output=True, text=True, timeout=300)


@pytest.fixture(scope="module")
def files(synth, oracle, tmp_path_factory):
    return pr.mixed_files(tmp_path_factory.mktemp("partition_search_cli"), synth, oracle)


def optimal(out):
    m = re.search(r"^Optimal log-likelihood: (\S+)$", out, re.M)
    assert m, out
    return float(m.group(1))


def test_search_on_the_partition_model(pkg, files, tmp_path):
    aln, part, tree, names = files
    pre = str(tmp_path / "search")
    r = run_cli(["-s", aln, "-spp", part, "-t", tree, "-n", "2", "-pre", pre])
    assert r.returncode == 0, r.stderr + r.stdout
    lines = re.findall(r"^Partition (\S+): (\d+) sites, (\d+) patterns, lnL (\S+)$", r.stdout, re.M)
    assert [l[0] for l in lines] == pr.MIXED_NAMES
    assert re.search(r"^Tree search: 3 iterations", r.stdout, re.M), r.stdout
    fixed = run_cli(["-s", aln, "-spp", part, "-te", tree, "-pre", str(tmp_path / "fixed")])
    assert fixed.returncode == 0, fixed.stderr
    assert optimal(r.stdout) >= optimal(fixed.stdout) - 1e-6 * abs(optimal(fixed.stdout))
    nwk = open(pre + ".treefile").read().strip()
    assert sorted(re.findall(r"[(,]([A-Za-z]\w*):", nwk)) == sorted(names) and len(names) == 8
    # the same through -te ... -search
    r2 = run_cli(["-s", aln, "-spp", part, "-te", tree, "-search", "-n", "2", "-pre", str(tmp_path / "again")])
    assert r2.returncode == 0 and optimal(r2.stdout) == optimal(r.stdout)


def test_refused_with_the_search(files):
    aln, part, tree, _ = files
    for args in (["-q", part, "-te", tree, "-search", "-bb", "100"], ["-spp", part, "-te", tree, "-search", "-numpars", "10"]):
        r = run_cli(["-s", aln] + args)
        assert r.returncode != 0 and "cannot be combined with" in r.stderr, (args, r.stderr)
