"""`iqhip_lnl -search -numpars N [-toppars M] [-sprrad R]` (cli/iqhip_lnl.cpp): the starting population of the search from
the command line -- the three lines it prints, with the counts and the final score of the Python API on the same inputs --
and the usage errors."""
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
BIN = os.path.join(os.path.dirname(HERE), "iq-tree_amd", "lib", "iqhip_lnl")
MODEL = "GTR{1.5,2.4,1.8,1.9,2.8}+F{0.25,0.26,0.25,0.24}+G4{0.9}"
NTAXA, NSITE = 10, 300


def run_cli(args):
    return subprocess.run([BIN] + args, capture_output=True, text=True, timeout=300)


@pytest.fixture(scope="module")
def case(synth, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("numpars")
    true = synth.random_tree_newick(NTAXA, 191)
    st = synth.simulate_alignment(true, synth.gtr_model(alpha=0.9, ncat=4), NSITE, 192)
    names = ["t%d" % i for i in range(NTAXA)]
    aln = tmp / "a.phy"
    aln.write_text("%d %d\n" % (NTAXA, NSITE) + "".join("%-10s %s\n" % (names[i], "".join("ACGT"[x] for x in st[i])) for i in range(NTAXA)))
    start = tmp / "start.nwk"
    start.write_text(re.sub(r"([(,])(\d+)", lambda m: m.group(1) + names[int(m.group(2))], synth.random_tree_newick(NTAXA, 193)) + "\n")
    return dict(tmp=tmp, aln=str(aln), start=str(start), names=names)


def api_search(pkg, case, seed, **kw):
    aln = pkg.Alignment(case["aln"])
    st, fr, _, _ = aln.arrays()
    t = pkg.PhyloTree(open(case["start"]).read().strip(), aln.seq_names)
    t.set_mem_mode(pkg.LM_ALL_BRANCH)
    t.set_alignment(4, 0, st, fr)
    t.set_model(aln.build_model(MODEL))
    t.set_likelihood_kernel(pkg.LK_EIGEN_HIP)
    t.attach_engine(0)
    ts = pkg.TreeSearch(t, seed=seed, **kw)
    best, its = ts.search(trace=True)
    return ts, best, its, t.compute_likelihood()


def test_numpars_prints_the_counts_of_the_api(pkg, case):
    pre = str(case["tmp"] / "n")
    r = run_cli(["-s", case["aln"], "-m", MODEL, "-te", case["start"], "-blfix", "-search", "-numpars", "6", "-toppars", "2", "-n", "1",
                 "-seed", "1", "-pre", pre])
    assert r.returncode == 0, r.stderr + r.stdout
    ts, best, its, lnl = api_search(pkg, case, 1, iterations=1, num_init_trees=6, num_nni_trees=2)
    distinct = 6 - ts.init_duplicates
    assert len(ts.init_trees) == distinct and len(its) == 3
    lines = r.stdout.splitlines()
    want = ["Generating 5 parsimony trees... %d distinct starting trees" % distinct,
            "Computing log-likelihood of %d initial trees" % distinct, "Optimizing top 2 initial trees with NNI..."]
    at = [lines.index(w) for w in want]                       # each is printed, and in this order ...
    assert at == sorted(at)
    m = re.search(r"^Tree search: (\d+) iterations, (\d+) candidate trees", r.stdout, re.M)
    assert m and int(m.group(1)) == 3 and int(m.group(2)) == len(ts.candidates())
    assert at[-1] < next(k for k, l in enumerate(lines) if l.startswith("Tree search:"))   # ... before the search reports
    got = float(re.search(r"^Optimal log-likelihood: (\S+)$", r.stdout, re.M).group(1))
    assert abs(got - lnl) <= 1e-10 * abs(lnl) and abs(got - best) <= 1e-10 * abs(best)
    for mm in re.finditer(r"^BETTER TREE FOUND at iteration (\d+): (-[\d.]+)$", r.stdout, re.M):
        it = its[int(mm.group(1)) - 1]
        assert it["new_best"] and abs(float(mm.group(2)) - it["score"]) < 1e-3
    assert set(pkg.newick_splits(open(pre + ".treefile").read().strip(), NTAXA, case["names"])) == \
        set(pkg.newick_splits(ts.candidates()[0][1], NTAXA, case["names"]))


def test_toppars_follows_numpars_and_sprrad_is_taken(pkg, case):
    # -numpars below -toppars (20 by default) lowers -toppars: every distinct tree is optimised
    r = run_cli(["-s", case["aln"], "-m", MODEL, "-te", case["start"], "-blfix", "-search", "-numpars", "3", "-sprrad", "2", "-n", "0",
                 "-seed", "4", "-pre", str(case["tmp"] / "t")])
    assert r.returncode == 0, r.stderr + r.stdout
    ts, best, its, lnl = api_search(pkg, case, 4, iterations=0, num_init_trees=3, num_nni_trees=3, init_spr_radius=2)
    distinct = 3 - ts.init_duplicates
    assert "Generating 2 parsimony trees... %d distinct starting trees" % distinct in r.stdout
    assert "Optimizing top %d initial trees with NNI..." % distinct in r.stdout and len(its) == distinct
    got = float(re.search(r"^Optimal log-likelihood: (\S+)$", r.stdout, re.M).group(1))
    assert abs(got - lnl) <= 1e-10 * abs(lnl)


def test_usage_errors(case):
    base = ["-s", case["aln"], "-m", MODEL, "-te", case["start"]]
    r = run_cli(base + ["-numpars", "6"])                     # without -search
    assert r.returncode == 2 and "usage:" in r.stderr
    for bad in (["-numpars", "0"], ["-numpars", "x"], ["-toppars", "-2"]):
        r = run_cli(base + ["-search"] + bad)
        assert r.returncode == 2 and "positive number of trees" in r.stderr
    r = run_cli(base + ["-sprrad", "2"])                      # -sprrad alone still needs a parsimony tree to work on
    assert r.returncode == 2
