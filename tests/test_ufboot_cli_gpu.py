"""`iqhip_lnl -s aln -te tree -m MODEL -bb N -seed S -wbt` (cli/iqhip_lnl.cpp): the ultrafast bootstrap's bookkeeping over
the -te tree and its NNI neighbourhood, the support tree, the consensus tree and the .ufboot file; the supports recomputed
from the .ufboot lines by the independent restatement (tests/ufboot_ref.py), the same winners through the Python view, and
byte-identical files from a second run."""
import os
import re
import subprocess

import pytest

import ufboot_ref as ref

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BIN = os.path.join(ROOT, "iq-tree_amd", "lib", "iqhip_lnl")
EXAMPLE = os.path.join(HERE, "golden", "example.phy")
MODEL = "GTR{1.513,2.393,1.769,1.912,2.838}+F{0.249,0.262,0.251,0.238}+G4{0.934}"
NREP, SEED = 200, 7


def named_tree(nwk, names):
    return re.sub(r"([(,])(\d+)", lambda m: m.group(1) + names[int(m.group(2))], nwk)


def run_cli(args):
    r = subprocess.run([BIN] + args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr + r.stdout
    return r.stdout


@pytest.fixture(scope="module")
def bb_cli(pkg, synth, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("ufboot")
    aln = pkg.Alignment(EXAMPLE)
    tf = tmp / "t.nwk"
    tf.write_text(named_tree(synth.random_tree_newick(44, 12), aln.seq_names) + "\n")
    pre = str(tmp / "bb")
    out = run_cli(["-s", EXAMPLE, "-te", str(tf), "-m", MODEL, "-bb", str(NREP), "-seed", str(SEED), "-wbt", "-pre", pre])
    return dict(aln=aln, tree_file=str(tf), pre=pre, out=out, tmp=tmp)


def labelled_splits(newick, names):
    """{split: label} of the internal nodes that carry a label"""
    n = len(names)
    ids = {nm: i for i, nm in enumerate(names)}
    out = {}
    stack = []
    for tok in re.finditer(r"\(|\)([^:,();]*)|([^:,();]+)|:[^,();]*|,|;", newick.strip()):
        t = tok.group(0)
        if t == "(":
            stack.append(set())
        elif t[0] == ")":
            grp = stack.pop()
            if stack:
                stack[-1] |= grp
                s = frozenset(range(n)) - grp if 0 in grp else frozenset(grp)
                if 2 <= len(s) <= n - 2 and tok.group(1) != "":
                    out[s] = tok.group(1)
        elif tok.group(2) is not None:
            stack[-1].add(ids[t])
    return out


def test_files_and_supports(bb_cli):
    aln, pre, out = bb_cli["aln"], bb_cli["pre"], bb_cli["out"]
    names = aln.seq_names
    n = len(names)
    m = re.search(r"^UFBoot: (\d+) candidate trees, (\d+) distinct bootstrap trees$", out, re.M)
    assert m and int(m.group(1)) == 1 + 2 * (n - 3)
    boot = open(pre + ".ufboot").read().splitlines()
    assert len(boot) == NREP
    assert len(set(boot)) == int(m.group(2)) and int(m.group(2)) >= 1
    for line in set(boot):
        assert len(ref.newick_splits(line, n, names)) == n - 3          # every winner parses and is binary
    sup_tree = open(pre + ".suptree").read().strip()
    labels = labelled_splits(sup_tree, names)
    assert len(labels) == n - 3
    assert set(labels) == set(ref.newick_splits(open(bb_cli["tree_file"]).read().strip(), n, names))
    _, count, total = ref.split_counts(boot, n, names=names)
    assert total == NREP
    for s, lab in labels.items():
        assert re.fullmatch(r"\d+", lab) and 0 <= int(lab) <= 100, lab
        assert int(lab) == ref._round_half_away(100.0 * count.get(s, 0) / NREP), (sorted(s), lab)
    con = open(pre + ".contree").read().strip()
    assert con == ref.consensus(boot, n, names=names)
    assert set(ref.newick_splits(con, n, names)) == {s for s, _ in ref.consensus_splits(boot, n, names=names)}


def test_python_path_gives_the_same_winners(pkg, bb_cli):
    aln = bb_cli["aln"]
    st, fr, _, _ = aln.arrays()
    t = pkg.PhyloTree(open(bb_cli["tree_file"]).read().strip(), names=aln.seq_names)
    t.set_mem_mode(pkg.LM_ALL_BRANCH)
    t.set_alignment(4, 0, st, fr)
    t.set_model(aln.build_model(MODEL))
    t.set_likelihood_kernel(pkg.LK_EIGEN_HIP)
    t.attach_engine(0)
    t.compute_likelihood()
    t.optimize_all_branches()
    t.clear_all_partial_lh()
    lnl = t.compute_likelihood()
    t.gen_boot_samples(NREP, aln.nsite, SEED, stream=0xA0)
    t.ufboot_init(NREP, seed=SEED)
    t.clear_all_partial_lh()
    lnl = t.compute_likelihood()
    t.ufboot_next_iteration()
    t.save_current_tree(lnl)
    t.save_nni_trees()
    s = t.summarize_bootstrap()
    boot = open(bb_cli["pre"] + ".ufboot").read().splitlines()
    assert [named_tree(x, aln.seq_names) for x in s["boot_trees"]] == boot
    assert s["consensus_tree"] == open(bb_cli["pre"] + ".contree").read().strip()
    cli_labels = sorted(int(x) for x in labelled_splits(open(bb_cli["pre"] + ".suptree").read().strip(), aln.seq_names).values())
    assert sorted(p for _, _, p in s["supports"]) == cli_labels


def test_tree_set_feeds_one_iteration_per_tree(pkg, synth, bb_cli):
    """-z: the -te tree first, then every tree of the file, each with its NNI neighbourhood; the supports sit on the -te
    tree and are the shares of the .ufboot lines, whichever tree the winners came from"""
    aln = bb_cli["aln"]
    names = aln.seq_names
    n = len(names)
    zf = bb_cli["tmp"] / "set.nwk"
    zf.write_text("".join(named_tree(synth.random_tree_newick(44, s), names) + "\n" for s in (12, 13)))
    pre = str(bb_cli["tmp"] / "set")
    out = run_cli(["-s", EXAMPLE, "-te", bb_cli["tree_file"], "-m", MODEL, "-bb", "64", "-seed", "3", "-z", str(zf), "-wbt", "-pre", pre])
    m = re.search(r"^UFBoot: (\d+) candidate trees, (\d+) distinct bootstrap trees$", out, re.M)
    assert m and int(m.group(1)) == 3 * (1 + 2 * (n - 3))
    boot = open(pre + ".ufboot").read().splitlines()
    assert len(boot) == 64 and len(set(boot)) == int(m.group(2))
    labels = labelled_splits(open(pre + ".suptree").read().strip(), names)
    assert set(labels) == set(ref.newick_splits(open(bb_cli["tree_file"]).read().strip(), n, names))
    _, count, _ = ref.split_counts(boot, n, names=names)
    for s, lab in labels.items():
        assert int(lab) == ref._round_half_away(100.0 * count.get(s, 0) / 64), (sorted(s), lab)
    assert open(pre + ".contree").read().strip() == ref.consensus(boot, n, names=names)
    assert "TOPOTEST" not in out                                        # -z without -zb runs no topology tests


def test_second_run_is_byte_identical(bb_cli):
    pre2 = str(bb_cli["tmp"] / "again")
    out2 = run_cli(["-s", EXAMPLE, "-te", bb_cli["tree_file"], "-m", MODEL, "-bb", str(NREP), "-seed", str(SEED), "-wbt", "-pre", pre2])
    for ext in (".suptree", ".contree", ".ufboot"):
        assert open(bb_cli["pre"] + ext, "rb").read() == open(pre2 + ext, "rb").read(), ext
    line = lambda o: re.search(r"^UFBoot: .*$", o, re.M).group(0)
    assert line(out2) == line(bb_cli["out"])
