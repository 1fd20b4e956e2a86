"""`iqhip_lnl ... -alrt N [-lbp N] [-seed S]` (cli/iqhip_lnl.cpp): the multinomial site resamples of its own generator,
the sample upload with +ASC patterns present, the branch tests and the labelled tree appended to the report."""
import re

import numpy as np
import pytest

from test_cli_gpu import EXAMPLE, named_tree, read_report, run_cli

pytestmark = pytest.mark.gpu
LABEL = re.compile(r"\)([0-9.e+-]+)/([0-9.e+-]+):")


def test_cli_branch_supports_with_asc(pkg, synth, oracle, tmp_path):
    aln = pkg.Alignment(EXAMPLE)
    st, fr, _, _ = aln.arrays()
    names = aln.seq_names
    nwk = synth.random_tree_newick(44, 12)
    tf = tmp_path / "t.nwk"
    tf.write_text(named_tree(nwk, names) + "\n")
    rows = st[:, [p for p in range(st.shape[1]) if len(set(st[:, p].tolist())) > 1 and st[:, p].max() < 4]][:, :120]
    phy = tmp_path / "var.phy"
    phy.write_text(" 44 %d\n" % rows.shape[1] + "".join("%s %s\n" % (names[i], "".join("ACGT"[s] for s in rows[i])) for i in range(44)))
    model = "HKY{2.0}+F{0.3,0.2,0.2,0.3}+G4{0.7}+ASC"
    reps = 200

    def run(seed, name):
        pre = str(tmp_path / name)
        out = run_cli(["-s", str(phy), "-te", str(tf), "-m", model, "-blfix", "-alrt", str(reps), "-lbp", str(reps), "-seed",
                       str(seed), "-pre", pre])
        assert "4 unobservable constant patterns" in out and "on 41 internal branches" in out
        rep = read_report(pre)
        assert rep["support_tree"] in out
        return rep

    rep = run(5, "a")
    labels = LABEL.findall(rep["support_tree"])
    assert len(labels) == 41                                          # every internal branch, SH-aLRT/LBP
    sh = np.array([float(a) for a, _ in labels])
    lbp = np.array([float(b) for _, b in labels])
    assert np.all((sh >= 0) & (sh <= 100)) and np.all((lbp >= 0) & (lbp <= 100)) and lbp.max() > 0
    # percentages of 200 replicates, printed with three significant digits: multiples of 0.5
    assert np.allclose(sh * 2, np.round(sh * 2), atol=0.21) and np.allclose(lbp * 2, np.round(lbp * 2), atol=0.21)
    assert LABEL.sub("):", rep["support_tree"]) == rep["tree"]         # labels only added
    assert run(5, "b")["support_tree"] == rep["support_tree"]          # same seed, same draws
    assert run(6, "c")["support_tree"] != rep["support_tree"]
    # the library on the same data with numpy's multinomial draws: the same supports up to resampling noise
    a2 = pkg.Alignment(str(phy))
    m2 = a2.build_model(model)
    nsite = a2.nsite
    a2.append_unobserved_const_patterns()
    s2, f2, _, _ = a2.arrays()
    t = pkg.PhyloTree(nwk)
    t.set_mem_mode(pkg.LM_ALL_BRANCH)
    t.set_alignment(4, 0, s2, f2)
    t.set_ascertainment(4, nsite)
    t.set_model(m2)
    t.attach_engine(0)
    p = np.asarray(f2, dtype=np.float64)
    t.set_boot_samples(np.random.default_rng(1).multinomial(nsite, p / p.sum(), size=reps).astype(np.float32))
    sup = t.test_all_branches(reps, reps)
    assert len(sup) == 41
    lib_labels = LABEL.findall(t.support_tree_string(sup, True, True))
    lsh = np.array([float(a) for a, _ in lib_labels])
    llbp = np.array([float(b) for _, b in lib_labels])
    noise = 100 * 5 * np.sqrt(2 * 0.25 / reps)                        # five standard deviations of a difference of two fractions
    assert np.all(np.abs(lsh - sh) <= noise) and np.all(np.abs(llbp - lbp) <= noise)
