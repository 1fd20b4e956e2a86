"""UFBoot on an edge-linked partition model: ONE group update (iqhip_partition_ufboot_update) over the 195 candidate rows of
a 100-taxon super tree -- the current tree and its 194 nni5 neighbours, rows written by the group's batched joint solves --
against the route a caller had before: one iqhip_ptnlh_rell per member, the copies of the members' M x S sums to the host,
their sum in numpy and the rule in numpy (tests/ufboot_ref.py).  Four DNA GTR+G4 partitions of about 25 000 patterns each,
1 000 replicates resampled within partitions on the device.
    python tools/bench_partition_ufboot.py [taxa [sites per partition [replicates [reps]]]]     default 100 25000 1000 5
Reported: the device time of the members' products and of the update kernel (HIP events, iqhip_timing_enable on the first
member), the kernels enqueued, the wall time of the whole call; for the old route the wall time of the members'
iqhip_ptnlh_rell calls, of the host sum and of the numpy rule; whether both routes end in the same state; and what the rows
cost a batched group solve: the wall time of evaluate_nnis5_batch with rows (the last of the five rounds of each swap goes
through iqhip_partition_optimize_branch_batch_rows) against the same call without.  Prints one line of JSON.  No threshold
is fixed here."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as g  # noqa: E402

pkg = g.load_package()
import importlib  # noqa: E402

import partition_ref as pr  # noqa: E402
import ufboot_ref  # noqa: E402

synth = importlib.import_module("iqtree_amd.synth")
oracle = g.load_oracle()
RATES = [1.0, 0.4, 2.3, 0.7]


def median(xs):
    return float(np.median(xs))


def run(ntaxa, nsites, nsamples, reps):
    nwk = synth.random_tree_newick(ntaxa, 9, 0.02, 0.2)
    data = [pr.member_data(synth, oracle, nwk, 4, 4, pr.SEQ_DNA, nsites, 900 + 10 * k, RATES[k]) for k in range(len(RATES))]
    st = pkg.PhyloSuperTree(nwk, data, all_branch=True)
    st.part_rates = RATES
    st.gen_boot_samples(nsamples, 3)
    lnl = st.compute_likelihood()
    # the cost of the rows: the same evaluation with and without (the first pass of each allocates)
    wall = {"plain": [], "rows": []}
    for k in range(reps + 1):
        t0 = time.perf_counter()
        plain = st.evaluate_nnis5_batch()
        wall["plain"].append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        moves = st.evaluate_nnis5_batch(first_row=1)
        wall["rows"].append((time.perf_counter() - t0) * 1e3)
    same_moves = moves == plain
    M = 1 + len(moves)
    st.ufboot_init(1)
    st.save_current_tree(lnl)                                # row 0
    rows = np.arange(M)
    ids = np.arange(M, dtype=np.int64)
    logl = np.array([lnl] + [m["newloglh"] for m in moves])
    rand = np.array([pkg.ufboot_rand(1, k) for k in range(M)])
    lib = pkg.libiqhip()
    lib.iqhip_timing_enable(st.members[0].engine, 1)
    prod_ms, upd_ms, wall_ms, launches = [], [], [], 0
    for _ in range(reps + 1):                                # (the first pass allocates the scratch)
        st.ufboot_init(nsamples)
        t0 = time.perf_counter()
        counts, mn = st.ufboot_update(rows, ids, logl, rand)
        wall_ms.append((time.perf_counter() - t0) * 1e3)
        p, u, launches = st.ufboot_timing()
        prod_ms.append(p)
        upd_ms.append(u)
    lib.iqhip_timing_enable(st.members[0].engine, 0)
    got = st.ufboot_state()
    rell_ms, sum_ms, rule_ms = [], [], []
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        parts = [m.ptnlh_rell(rows, nsamples) for m in st.members]
        rell_ms.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        R = parts[0]
        for x in parts[1:]:
            R = R + x
        sum_ms.append((time.perf_counter() - t0) * 1e3)
        state = ufboot_ref.ufboot_start(nsamples)
        t0 = time.perf_counter()
        wcounts, wmn = ufboot_ref.ufboot_rule(state, R, ids, logl, rand)
        rule_ms.append((time.perf_counter() - t0) * 1e3)
    same = all(np.array_equal(got[f], state[f]) for f in got) and counts.tolist() == wcounts.tolist() and mn == wmn
    print(json.dumps(dict(
        workload="DNA GTR+G4 x %d partitions" % len(RATES), taxa=ntaxa, rows=M, patterns=[int(d["pat"].shape[1]) for d in data],
        replicates=nsamples, products_device_ms=median(prod_ms[1:]), update_kernel_device_us=median(upd_ms[1:]) * 1e3,
        launches=int(launches), update_call_wall_ms=median(wall_ms[1:]), slots_replaced=int(counts[2]),
        distinct_winners=int(len(set(got["boot_tree"].tolist()))),
        old_route_member_rell_wall_ms=median(rell_ms[1:]), old_route_host_sum_wall_ms=median(sum_ms[1:]),
        old_route_numpy_rule_wall_ms=median(rule_ms[1:]),
        old_route_wall_ms=median(rell_ms[1:]) + median(sum_ms[1:]) + median(rule_ms[1:]),
        sums_to_host_mib=len(RATES) * M * nsamples * 8 / 2**20, same_state=bool(same),
        nni5_batch_wall_ms=median(wall["plain"][1:]), nni5_batch_with_rows_wall_ms=median(wall["rows"][1:]),
        rows_written_mib=sum(int(m.nptn) for m in st.members) * len(moves) * 8 / 2**20, same_moves=bool(same_moves))))
    st.close()
    if not (same and same_moves):
        sys.exit(1)


if __name__ == "__main__":
    a = [int(x) for x in sys.argv[1:]]
    run(a[0] if len(a) > 0 else 100, a[1] if len(a) > 1 else 25000, a[2] if len(a) > 2 else 1000, a[3] if len(a) > 3 else 5)
