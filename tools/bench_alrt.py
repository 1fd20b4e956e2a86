"""SH-aLRT / local-bootstrap branch tests on the device (iqhip_branch_tests): time of the one-product form against the
M-launch form (one iqhip_rell per distinct per-pattern vector, the best the engine offered before), and the achieved
fraction of the fp64 matrix peak and of HBM bandwidth of pass 1, from the operand bytes.  Default shape: 100 taxa,
100k DNA patterns, 1000 replicates.  Prints one JSON line.
    python tools/bench_alrt.py [ntaxa] [npatterns] [replicates]"""
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g  # noqa: E402

pkg = g.load_package()
synth = importlib.import_module("iqtree_amd.synth")
T = int(sys.argv[1]) if len(sys.argv) > 1 else 100
P = int(sys.argv[2]) if len(sys.argv) > 2 else 100000
NS = int(sys.argv[3]) if len(sys.argv) > 3 else 1000
PEAK_F64_MATRIX = 78.6e12     # MI355X, fp64 matrix, flop/s
PEAK_HBM = 8.0e12             # bytes/s

model = synth.gtr_model()
nwk = synth.random_tree_newick(T, 1, 0.05, 0.3)
st = synth.simulate_alignment(nwk, model, int(P * 1.02) + 64, 3)
pat, freq = synth.compress_patterns(st)
if pat.shape[1] < P:
    raise SystemExit("only %d patterns: raise the site count" % pat.shape[1])
pat, freq = np.ascontiguousarray(pat[:, :P]), freq[:P].copy()
t = pkg.PhyloTree(nwk)
t.set_mem_mode(pkg.LM_ALL_BRANCH)
t.set_alignment(4, 0, pat, freq)
t.set_model(model)
t.attach_engine(0)
rng = np.random.default_rng(1)
w = rng.poisson(freq, size=(NS, P)).astype(np.float32)      # (timing only: Poisson counts instead of a multinomial draw)
t.set_boot_samples(w)
t0 = time.perf_counter()
sup = t.test_all_branches(NS, NS)                            # fills the store: row 0 and two rows per internal branch
t_all = time.perf_counter() - t0
nb = len(sup)
M = 1 + 2 * nb
rows3 = np.array([[0, 1 + 2 * q, 2 + 2 * q] for q in range(nb)])
t.branch_tests(rows3, sup["lh"], NS, NS)
reps = 10
t0 = time.perf_counter()
for _ in range(reps):
    out = t.branch_tests(rows3, sup["lh"], NS, NS)
dt_tests = (time.perf_counter() - t0) / reps
# pass 1 on its own: iqhip_ptnlh_rell = row upload + product + combine + the read-back of the M x NS sums (1.6 MB)
t.ptnlh_rell(np.arange(M), NS)
t0 = time.perf_counter()
for _ in range(reps):
    t.ptnlh_rell(np.arange(M), NS)
dt_product = (time.perf_counter() - t0) / reps
# the M-launch form: one iqhip_rell (k_pattern_lh_scaled + k_rell + the read-back of the scores) per distinct vector.
# iqhip_rell only multiplies the vector of the last lnL evaluation, so the current branch's vector stands in for every
# row: same length and the same 400 MB of sample matrix per call, but the 0.8 MB vector stays cache-resident -- the
# baseline is flattered by that, by at most 0.2 % of its traffic
t.compute_likelihood()
t.compute_rell()
t0 = time.perf_counter()
for _ in range(M):
    r = t.compute_rell()
dt_launches = time.perf_counter() - t0
ppad = (P + 63) // 64 * 64
flop = 2.0 * M * ppad * NS
operand_bytes = 4.0 * NS * ppad + 8.0 * M * ppad
print(json.dumps(dict(bench="alrt", ntaxa=T, npatterns=P, replicates=NS, rows=M, branch_tests_ms=dt_tests * 1e3,
                      m_launch_ms=dt_launches * 1e3, speedup=dt_launches / dt_tests,
                      test_all_branches_s=t_all, gflop=flop / 1e9, operand_gb=operand_bytes / 1e9,
                      ptnlh_rell_ms=dt_product * 1e3,
                      frac_fp64_matrix_peak=flop / dt_product / PEAK_F64_MATRIX,
                      frac_hbm_peak=operand_bytes / dt_product / PEAK_HBM,
                      fractions_of="host wall time of iqhip_ptnlh_rell: row-list upload, product, combine, read-back of the sums",
                      branch_tests_includes="host deduplication, two uploads, product, combine, statistics, read-back",
                      baseline="M x iqhip_rell on the current branch's vector (iqhip_rell cannot address store rows)",
                      m_launch_gb=(4.0 * NS * ppad + 8.0 * ppad) * M / 1e9,
                      sh_alrt_mean=float(sup["sh_alrt"].mean()), lbp_mean=float(sup["lbp"].mean()))))
