"""BIONJ without a device: the fp64 restatement of tests/bionj_ref.py against the reference's recorded output
(tests/golden/bionj_cases.json, written by tests/make_bionj_golden.py), the conditions the fixtures must meet, the pure host
Newick builder of the host mirror (bionj_newick) and the spread between summation orders that the tolerance of
tests/test_bionj_gpu.py rests on."""
import json
import os

import numpy as np
import pytest

import bionj_ref as br

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "bionj_cases.json")) as _f:
    GOLDEN = json.load(_f)
GOLDEN_NAMES = ["uniform_n%d_s%d" % (n, s) for n in (5, 8, 13, 24, 40) for s in (0, 1)] + [
    "uniform_n65_s1", "duplicates_n9", "duplicates_n16", "balanced_n16_e0.125", "star_n9_d0.5"]

# the reference computes in float and prints 8 decimals: 3 x the 3.3e-7 measured between it and an fp64 evaluation
GOLDEN_LENGTH_TOL = 1e-6
# every fixture keeps the runner-up pair this far above the minimum of Q at every step (the fixture's condition)
FIXTURE_MARGIN = 5e-5
# largest difference of any la, lb, lambda or final length between two summation orders of the restatement
ORDER_SPREAD_BOUND = 1e-15


def golden_case(case):
    names, D = br.parse_matrix_text(case["matrix"])
    return names, D, br.newick_splits(case["newick"], names)


def test_the_fixture_holds_the_listed_cases():
    assert [c["name"] for c in GOLDEN] == GOLDEN_NAMES
    assert os.path.getsize(os.path.join(HERE, "golden", "bionj_cases.json")) < 120 * 1024


@pytest.mark.parametrize("rule", ["first", "reference"])
def test_restatement_gives_the_recorded_trees(rule):
    worst = 0.0
    for case in GOLDEN:
        names, D, want = golden_case(case)
        r = br.bionj(D, rule=rule)
        got = br.log_splits(r["steps"], r["last"], r["last_len"], len(names))
        d = br.max_split_diff(got, want)
        print("%-22s rule %-9s max |length - reference| %.3e" % (case["name"], rule, d))
        worst = max(worst, d)
    print("largest difference of a split length: %.3e" % worst)
    assert worst <= GOLDEN_LENGTH_TOL


def test_fixtures_keep_their_margin():
    for case in GOLDEN:
        _, D, _ = golden_case(case)
        r = br.bionj(D)
        ref = br.bionj(D, rule="reference")
        assert [s[:2] for s in r["steps"]] == [s[:2] for s in ref["steps"]], case["name"]
        assert not any(r["near"]), case["name"]
        if r["margin"]:
            print("%-22s smallest margin %.3e" % (case["name"], min(r["margin"])))
            assert min(r["margin"]) >= FIXTURE_MARGIN, case["name"]


def test_newick_builder_hand_written_log(pkg):
    steps = [(3, 1, 0.1, 0.2, 0.5), (4, 3, -0.05, 0.3, 1.0)]
    got = pkg.bionj_newick(steps, [0, 2, 4], [0.25, 0.125, 1.5], ["A", "B", "C", "D", "E"])
    assert got == "(A:0.25000000,C:0.12500000,(E:-0.05000000,(D:0.10000000,B:0.20000000):0.30000000):1.50000000);"
    # three taxa: no merge
    assert pkg.bionj_newick([], [0, 1, 2], [1, 2, 3], ["x", "y", "z"]) == "(x:1.00000000,y:2.00000000,z:3.00000000);"
    # a log that merges a row twice, rows that are not ascending, a wrong number of steps
    with pytest.raises(pkg.HostError):
        pkg.bionj_newick([(3, 1, 0.1, 0.2, 0.5), (1, 0, 0.1, 0.2, 0.5)], [0, 2, 4], [0, 0, 0], list("ABCDE"))
    with pytest.raises(pkg.HostError):
        pkg.bionj_newick(steps, [2, 0, 4], [0, 0, 0], list("ABCDE"))
    with pytest.raises(pkg.HostError):
        pkg.bionj_newick(steps[:1], [0, 2, 4], [0, 0, 0], list("ABCDE"))


def test_newick_builder_on_the_restatements_logs(pkg):
    for case in GOLDEN:
        names, D, _ = golden_case(case)
        r = br.bionj(D)
        steps = np.zeros(len(r["steps"]), dtype=pkg.BIONJ_STEP_DTYPE)
        for k, s in enumerate(r["steps"]):
            steps[k] = s
        nwk = pkg.bionj_newick(steps, r["last"], r["last_len"], names)
        got = br.newick_splits(nwk, names)
        want = br.log_splits(r["steps"], r["last"], r["last_len"], len(names))
        assert br.max_split_diff(got, want) <= 0.5e-8 + 1e-15, case["name"]   # (%10.8f rounds to the nearest 1e-8)


def log_spread(a, b):
    assert [s[:2] for s in a["steps"]] == [s[:2] for s in b["steps"]] and a["last"] == b["last"]
    x, y = np.array([s[2:] for s in a["steps"]]), np.array([s[2:] for s in b["steps"]])
    return max(np.abs(x - y).max(), np.abs(np.array(a["last_len"]) - np.array(b["last_len"])).max())


def test_summation_order_spread():
    """numpy's pairwise sums against exactly rounded ones: the same pairs, and numbers that differ by at most
    ORDER_SPREAD_BOUND (2.3e-16 measured) -- the tolerance of tests/test_bionj_gpu.py is 1000 x this bound."""
    worst = 0.0
    for n in (24, 65, 130, 257):
        D = br.uniform_matrix(n, 1)
        d = log_spread(br.bionj(D, sums="numpy"), br.bionj(D, sums="fsum"))
        print("n = %3d spread %.3e" % (n, d))
        worst = max(worst, d)
    assert worst <= ORDER_SPREAD_BOUND
