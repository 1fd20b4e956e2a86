"""`iqhip_lnl ... -search / -t` (cli/iqhip_lnl.cpp): the NNI tree search from a tree file, from the BIONJ and the parsimony
starting tree, with the ultrafast bootstrap fed by the search, and the refusals."""
import os
import re
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BIN = os.path.join(ROOT, "iq-tree_amd", "lib", "iqhip_lnl")
MODEL = "GTR{1.5,2.4,1.8,1.9,2.8}+F{0.25,0.26,0.25,0.24}+G4{0.9}"
NTAXA, NSITE = 10, 1000


def run_cli(args, ok=True):
    r = subprocess.run([BIN] + args, capture_output=True, text=True, timeout=300)
    if ok:
        assert r.returncode == 0, r.stderr + r.stdout
    return r


@pytest.fixture(scope="module")
def case(synth, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("search")
    model = synth.gtr_model(alpha=0.9, ncat=4)
    true = synth.random_tree_newick(NTAXA, 91)
    st = synth.simulate_alignment(true, model, NSITE, 92)
    names = ["t%d" % i for i in range(NTAXA)]
    aln = tmp / "a.phy"
    aln.write_text("%d %d\n" % (NTAXA, NSITE) + "".join("%-10s %s\n" % (names[i], "".join("ACGT"[x] for x in st[i])) for i in range(NTAXA)))
    start = tmp / "start.nwk"                               # a random topology, not the one the data come from
    start.write_text(re.sub(r"([(,])(\d+)", lambda m: m.group(1) + names[int(m.group(2))], synth.random_tree_newick(NTAXA, 93)) + "\n")
    return dict(tmp=tmp, aln=str(aln), start=str(start), true=true, names=names)


def printed(out, what):
    m = re.search(r"^%s\s*(-?[\d.]+(?:e[-+]?\d+)?)$" % re.escape(what), out, re.M)
    assert m, (what, out)
    return float(m.group(1))


def test_search_from_a_tree_file(pkg, case):
    pre = str(case["tmp"] / "s")
    out = run_cli(["-s", case["aln"], "-m", MODEL, "-t", case["start"], "-n", "3", "-seed", "1", "-pre", pre]).stdout
    start_lnl = printed(out, "Log-likelihood after branch-length optimisation:")
    best = printed(out, "Optimal log-likelihood:")
    assert best > start_lnl                                 # a random start: the search does improve it
    assert re.search(r"^Tree search: 4 iterations, \d+ candidate trees", out, re.M)
    for m in re.finditer(r"^BETTER TREE FOUND at iteration (\d+): (-[\d.]+)$", out, re.M):
        assert 2 <= int(m.group(1)) <= 4 and float(m.group(2)) <= best + 1e-3
    assert abs(printed(out, "BEST SCORE FOUND :") - best) < 6e-4
    # the tree file holds the tree of the printed optimum
    again = run_cli(["-s", case["aln"], "-m", MODEL, "-te", pre + ".treefile", "-blfix", "-pre", str(case["tmp"] / "re")]).stdout
    assert abs(printed(again, "Log-likelihood of the input tree:") - best) < 5e-4
    assert len(pkg.newick_splits(open(pre + ".treefile").read().strip(), NTAXA, case["names"])) == NTAXA - 3
    # -te <file> -search is the same run
    out2 = run_cli(["-s", case["aln"], "-m", MODEL, "-te", case["start"], "-search", "-n", "3", "-seed", "1", "-pre", pre + "2"]).stdout
    assert printed(out2, "Optimal log-likelihood:") == best
    assert open(pre + "2.treefile").read() == open(pre + ".treefile").read()
    # every 10th iteration is reported
    out3 = run_cli(["-s", case["aln"], "-m", MODEL, "-t", case["start"], "-n", "10", "-seed", "1", "-pre", pre + "3"]).stdout
    assert re.search(r"^Iteration 10 / LogL: -[\d.]+$", out3, re.M) and printed(out3, "Optimal log-likelihood:") >= best - 1e-6


@pytest.mark.parametrize("start", ["-bionjtree", "-parstree"])
def test_search_from_a_built_starting_tree(pkg, case, start):
    pre = str(case["tmp"] / start[1:])
    out = run_cli(["-s", case["aln"], "-m", MODEL, start, "-search", "-n", "2", "-seed", "2", "-pre", pre]).stdout
    best = printed(out, "Optimal log-likelihood:")
    assert best >= printed(out, "Log-likelihood after branch-length optimisation:") - 1e-6
    assert len(pkg.newick_splits(open(pre + ".treefile").read().strip(), NTAXA, case["names"])) == NTAXA - 3


def test_search_feeds_the_bootstrap(pkg, case):
    pre = str(case["tmp"] / "bb")
    out = run_cli(["-s", case["aln"], "-m", MODEL, "-t", case["start"], "-bb", "200", "-nstep", "4", "-n", "8", "-seed", "3", "-wbt",
                   "-pre", pre]).stdout
    corr = re.findall(r"^NOTE: Bootstrap correlation coefficient of split occurrence frequencies: (\S+)$", out, re.M)
    assert len(corr) == 2 and all(-1.0 <= float(c) <= 1.0 for c in corr)
    m = re.search(r"^UFBoot: (\d+) candidate trees, (\d+) distinct bootstrap trees$", out, re.M)
    assert m and int(m.group(1)) > 9 * (1 + 2 * (NTAXA - 3)) // 2          # the search fed it, not one neighbourhood
    boot = open(pre + ".ufboot").read().splitlines()
    # (a topology the search meets again is fed again under a new tree id: the ids count as distinct, the strings repeat)
    assert len(boot) == 200 and 1 <= len(set(boot)) <= int(m.group(2))
    best = open(pre + ".treefile").read().strip()
    sup = open(pre + ".suptree").read().strip()
    assert set(pkg.newick_splits(sup, NTAXA, case["names"])) == set(pkg.newick_splits(best, NTAXA, case["names"]))
    labels = [int(x) for x in re.findall(r"\)(\d+)", sup)]
    assert len(labels) == NTAXA - 3 and all(0 <= x <= 100 for x in labels)
    assert open(pre + ".contree").read().strip() == pkg.consensus_tree(boot, NTAXA, names=case["names"])


def test_refusals(case):
    r = run_cli(["-s", case["aln"], "-t", case["start"]], ok=False)
    assert r.returncode == 2 and "needs a model" in r.stderr
    r = run_cli(["-s", case["aln"], "-m", MODEL, "-t", case["start"], "-n", "-1"], ok=False)
    assert r.returncode == 2 and "non-negative number of iterations" in r.stderr
    r = run_cli(["-s", case["aln"], "-m", MODEL, "-t", case["start"], "-nstep", "3"], ok=False)
    assert r.returncode == 2 and "-nstep" in r.stderr
