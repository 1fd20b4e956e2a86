"""UFBoot bookkeeping on the device (iqhip_ufboot_update): ONE update over the 2 (n - 3) + 1 candidate rows of an n-taxon
tree -- the current tree and its NNI neighbourhood -- against the route a caller had before: iqhip_ptnlh_rell, the copy of
the M x S sums to the host and the rule in numpy (tests/ufboot_ref.py).  Reported: the device time of the matrix-core
product and of the update kernel (HIP events), the kernels enqueued, the wall time of the whole call, and for the old route
the wall time of iqhip_ptnlh_rell (product + copy + scatter) and of the numpy rule.  Both routes must end in the same state.
    python tools/bench_ufboot.py [taxa [patterns [replicates]]]      default: DNA, 100 taxa, 100 000 patterns, 1 000 replicates
The rows are uploaded (uniform in -12 .. -1 with the spread of a per-pattern lnL; neighbouring rows differ in 2 % of the
patterns): neither route's time depends on their values.  Prints one line of JSON.  No threshold is fixed here."""
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

import ufboot_ref  # noqa: E402

synth = importlib.import_module("iqtree_amd.synth")


def median(xs):
    return float(np.median(xs))


def run(ntaxa, nptn, nsamples, reps=5):
    rng = np.random.default_rng(1)
    M = 2 * (ntaxa - 3) + 1
    t = pkg.PhyloTree("(0:0.1,1:0.2,2:0.3);")
    t.set_alignment(4, pkg.SEQ_DNA, rng.integers(0, 4, size=(3, nptn)).astype(np.uint8), rng.integers(1, 4, size=nptn).astype(np.float64))
    t.set_model(synth.gtr_model(alpha=0.9, ncat=4))
    t.set_likelihood_kernel(pkg.LK_EIGEN_HIP)
    t.attach_engine(0)
    t.ptnlh_reserve(M)
    base = rng.uniform(-12.0, -1.0, size=nptn)
    for r in range(M):
        row = base.copy()
        at = rng.choice(nptn, max(1, nptn // 50), replace=False)
        row[at] = rng.uniform(-12.0, -1.0, size=at.size)
        t.ptnlh_upload(r, row)
    t.gen_boot_samples(nsamples, nptn * 2, 3)
    rows = np.arange(M)
    ids = np.arange(M, dtype=np.int64)
    logl = rng.uniform(-3.0e5, -2.9e5, size=M)
    rand = np.array([pkg.ufboot_rand(1, k) for k in range(M)])
    lib = pkg.libiqhip()
    lib.iqhip_timing_enable(t.engine, 1)
    prod_ms, upd_ms, wall_ms, launches = [], [], [], 0
    for _ in range(reps + 1):                                  # (the first pass allocates the scratch)
        t.ufboot_init(nsamples)
        t0 = time.perf_counter()
        counts, mn = t.ufboot_update(rows, ids, logl, rand)
        wall_ms.append((time.perf_counter() - t0) * 1e3)
        p, u, launches = t.ufboot_timing()
        prod_ms.append(p)
        upd_ms.append(u)
    lib.iqhip_timing_enable(t.engine, 0)
    got = t.ufboot_state()
    rell_ms, rule_ms = [], []
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        R = t.ptnlh_rell(rows, nsamples)
        rell_ms.append((time.perf_counter() - t0) * 1e3)
        st = ufboot_ref.ufboot_start(nsamples)
        t0 = time.perf_counter()
        wcounts, wmn = ufboot_ref.ufboot_rule(st, R, ids, logl, rand)
        rule_ms.append((time.perf_counter() - t0) * 1e3)
    same = all(np.array_equal(got[f], st[f]) for f in got) and counts.tolist() == wcounts.tolist() and mn == wmn
    print(json.dumps(dict(
        workload="DNA", taxa=ntaxa, rows=M, patterns=nptn, replicates=nsamples,
        product_device_ms=median(prod_ms[1:]), update_kernel_device_us=median(upd_ms[1:]) * 1e3, launches=int(launches),
        update_call_wall_ms=median(wall_ms[1:]), slots_replaced=int(counts[2]),
        distinct_winners=int(len(set(got["boot_tree"].tolist()))),
        old_route_ptnlh_rell_wall_ms=median(rell_ms[1:]), old_route_numpy_rule_wall_ms=median(rule_ms[1:]),
        old_route_wall_ms=median(rell_ms[1:]) + median(rule_ms[1:]), sums_to_host_mib=M * nsamples * 8 / 2**20,
        same_state=bool(same))))
    if not same:
        sys.exit(1)


if __name__ == "__main__":
    a = [int(x) for x in sys.argv[1:]]
    run(a[0] if len(a) > 0 else 100, a[1] if len(a) > 1 else 100000, a[2] if len(a) > 2 else 1000)
