"""Edge-linked partition models, the parts that need no device: the partition-file parser and site extractor
(host/partition_spec.h, readPartitionRaxml) against the plain-Python restatement of tests/partition_ref.py, the
all-unknown row of a taxon without data, the refusals of the group ABI that need no engine, and the restatement's own
per-member NaN rule."""
import ctypes as C

import numpy as np
import pytest

import partition_ref as pr

GOOD = [
    ("JC, g1 = 1-100\n", 100),
    ("GTR{1.5,2.4,1.8,1.9,2.8}+F{0.25,0.26,0.25,0.24}+G4{0.8}, gene1 = 1-100, 250-400, 401-500\\3\nJC, g2 = 101-249\n", 500),
    ("  LG+G4{0.5} ,  third pos = 3 - 300 \\ 3 , 7\t9\r\n\nHKY{2.0}, rest=1-300\\3 2-300\\3\n", 300),
    ("POISSON, single = 17\nJC2, bin = 18-20 1\n", 20),
]
BAD = [
    ("JC g = 1-10", 100),            # no ',' after the model
    ("JC, g 1-10", 100),             # no '='
    ("JC, = 1-10", 100),             # no name
    (", g = 1-10", 100),             # no model
    ("JC, g = 1-101", 100),          # beyond the alignment
    ("JC, g = 0-10", 100),           # before it
    ("JC, g = 10-1", 100),           # empty range
    ("JC, g = ", 100),               # no site
    ("JC, g = , ", 100),
    ("JC, g = 1-10\\0", 100),        # step < 1
    ("JC, g = 1-x", 100),
    ("JC, g = 1-10 abc", 100),
    ("GTR{1,2, g = 1-10", 100),      # the brace never closes: no ',' outside braces
    ("", 100),
    ("\n\n", 100),
]


@pytest.mark.parametrize("text,nsite", GOOD)
def test_parser_matches_the_python_parser(pkg, text, nsite):
    want = pr.parse_partition_file(text, nsite)
    got = pkg.parse_partition_spec(text, nsite)
    assert got == want
    assert all(m == m.strip() and n == n.strip() for m, n, _ in got)


def test_model_string_is_kept_verbatim(pkg):
    m = "GTR{1.5,2.4,1.8,1.9,2.8}+F{0.25,0.26,0.25,0.24}+I{0.1}+G4{0.8}"
    (model, name, sites), = pkg.parse_partition_spec("%s, a b = 2-4" % m, 10)
    assert model == m and name == "a b" and sites == [1, 2, 3]


@pytest.mark.parametrize("text,nsite", BAD)
def test_bad_partition_files_are_refused(pkg, text, nsite):
    with pytest.raises(pr.PartitionFileError):
        pr.parse_partition_file(text, nsite)
    with pytest.raises(pkg.HostError):
        pkg.parse_partition_spec(text, nsite)


ALN = """5 24
t1 ACGTACGTACGT0101ARNDARND
t2 ACGTACGAACGT0111ARNDCRND
t3 ACGAACGTACGT1010NKNDARNE
t4 ------------0110--------
t5 ACGTNCGTACGA----ARNDARND
"""
PARTS = "HKY{2.0}+G4{0.7}, dna = 1-12\\2, 2-12\\2\nJC2+F{0.4,0.6}, bin = 13-16\nPOISSON, prot = 17-24\n"


def test_site_extraction_and_unknown_rows(pkg):
    names, parts = pkg.read_partition_file(None, None, aln_content=ALN, part_content=PARTS)
    assert names == ["t1", "t2", "t3", "t4", "t5"]
    rows = [line.split()[1] for line in ALN.strip().splitlines()[1:]]
    spec = pr.parse_partition_file(PARTS, 24)
    code = {0: dict(zip("ACGT", range(4)), **{"-": 18, "N": 18}), 3: {"0": 0, "1": 1, "-": 2},
            1: dict(zip(pr.LETTERS[pr.SEQ_PROTEIN], range(20)), **{"-": 23})}
    assert [d["seq_type"] for d in parts] == [0, 3, 1] and [d["nstates"] for d in parts] == [4, 2, 20]
    for d, (model, name, sites) in zip(parts, spec):
        assert d["name"] == name and d["model_string"] == model and d["nsite"] == len(sites)
        chars = pr.extract_sites([list(r) for r in rows], sites)
        want = np.array([[code[d["seq_type"]][c] for c in row] for row in chars], dtype=np.uint8)
        st, fr, sp, _ = d["alignment"].arrays()
        assert np.array_equal(st[:, sp], want)                      # site by site, every taxon kept
        assert fr.sum() == len(sites) and np.array_equal(st, d["pat"])
    # a taxon without data in a partition is an all-unknown row, not a dropped sequence
    assert parts[0]["pat"].shape[0] == 5 and np.all(parts[0]["pat"][3] == 18)
    assert np.all(parts[2]["pat"][3] == 23) and np.all(parts[1]["pat"][4] == 2)
    assert parts[0]["model"].ncat == 4 and parts[1]["model"].ncat == 1
    np.testing.assert_allclose(parts[1]["model"].state_freq, [0.4, 0.6])
    with pytest.raises(pkg.HostError):      # a mixture cannot join
        pkg.read_partition_file(None, None, aln_content=ALN, part_content="MIX{JC,HKY{2.0}}, dna = 1-12\n")
    with pytest.raises(pkg.HostError):      # codon partitions need whole triplets
        pkg.read_partition_file(None, None, aln_content=ALN, part_content="GY{2.0,0.5}+F1X4, c = 1-11\n")


def test_group_abi_refusals_without_a_device(pkg):
    lib = pkg.libiqhip()
    assert lib.iqhip_abi_version() == 2
    g = C.c_void_p()
    one = (C.c_void_p * 1)(None)
    assert lib.iqhip_partition_create(None, one, 1) == 2
    assert lib.iqhip_partition_create(C.byref(g), None, 1) == 2 and not g.value
    assert lib.iqhip_partition_create(C.byref(g), one, 0) == 2 and not g.value
    assert lib.iqhip_partition_create(C.byref(g), one, -3) == 2
    assert lib.iqhip_partition_create(C.byref(g), one, 1) == 2 and b"null engine" in lib.iqhip_last_error()
    r = (C.c_double * 1)(1.0)
    assert lib.iqhip_partition_set_rates(None, r) == 2
    x, d, n = C.c_double(), C.c_double(), C.c_int()
    assert lib.iqhip_partition_newton_branch(None, 0.1, 1e-6, 100.0, 1e-6, 100, C.byref(x), C.byref(d), C.byref(n), None) == 2
    assert lib.iqhip_partition_lnl_from_theta(None, 0.1, r) == 2
    assert lib.iqhip_partition_lnl_from_theta(None, 0.1, None) == 2
    assert lib.iqhip_partition_traverse_lnl(None, None, 0, pkg.leaf_end(0), pkg.key_end(1), 0.1, None, r) == 2
    assert lib.iqhip_debug_partition_timing(None, None, None) == 2
    lib.iqhip_partition_destroy(None)


def test_restatement_applies_the_nan_rule_per_member(synth, oracle):
    """a member whose theta is NaN contributes df = ddf = 0 (phylokernel.h:647-651 before the weighted sum): the joint
    solve equals the solve over the other members, and differs from the solve over all of them"""
    nwk, members = pr.mixed_group(synth, oracle)
    ots = [pr.oracle_member(oracle, nwk, d) for d in members]
    rates = pr.MIXED_RATES
    a, b = pr.tree_edges(ots[0], len(ots[0].adj))[4]
    thetas = [ot.theta(a, b)[0] for ot in ots]
    full = pr.joint_minimize_newton(ots, rates, a, b, 1e-6, 0.1, 100.0, 1e-6, 100, thetas)
    broken = list(thetas)
    broken[2] = np.full_like(thetas[2], np.nan)
    got = pr.joint_minimize_newton(ots, rates, a, b, 1e-6, 0.1, 100.0, 1e-6, 100, broken)
    rest = [0, 1, 3]
    want = pr.joint_minimize_newton([ots[k] for k in rest], [rates[k] for k in rest], a, b, 1e-6, 0.1, 100.0, 1e-6, 100,
                                    [thetas[k] for k in rest])
    assert got[3] == want[3] == full[3] == "ok"
    assert got[0] == want[0] and got[2] == want[2]
    assert abs(got[0] - full[0]) > 1e-6
