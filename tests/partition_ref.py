"""Restatement of the edge-linked partition model (PhyloSuperTreePlen, -q / -spp) over the CPU oracle, plus the shared
data of the partition tests.

  joint_minimize_newton   Optimization::minimizeNewton (optimization.cpp:388-465), the loop of
                          oracle_driver.OracleTree.minimize_newton, over PhyloSuperTreePlen::computeFuncDerv
                          (phylosupertreeplen.cpp:530-578): df = sum_p r_p df_p(r_p x), ddf = sum_p r_p^2 ddf_p(r_p x), with
                          the reference's NaN / inf rule (phylokernel.h:647-651) applied per member before the sum
  joint_lnl_from_theta    every member's computeLikelihoodFromBuffer at r_p x
  gene_rate_step          PartitionModelPlen::optimizeGeneRate (phylosupertreeplen.cpp:219-254): the P
                          optimizeTreeLengthScaling Brent searches (phylotree.cpp:2103-2118) in lockstep, then the
                          normalisation
  parse_partition_file / extract_sites   RAxML-style partition files (readPartitionRaxml, phylosupertree.cpp:150-266;
                          extractSiteID, alignment.cpp:2169-2200), plain Python

Every member is an OracleTree on the FULL super-tree topology whose lengths are the super tree's times r_p; a taxon without
data in a partition is an all-unknown row."""
import os
import re

import numpy as np

SEQ_DNA, SEQ_PROTEIN, SEQ_CODON, SEQ_BINARY = 0, 1, 2, 3


def scale_newick(nwk, r):
    """every branch length of the Newick string times r (17 significant digits: the product survives the round trip)"""
    r = float(r)
    return re.sub(r":([0-9.eE+-]+)", lambda m: ":" + repr(float(m.group(1)) * r), nwk)


def joint_derv(ots, rates, a, b, x, thetas):
    df = ddf = 0.0
    for ot, r, th in zip(ots, rates, thetas):
        d1, d2 = ot.derv(a, b, length=r * x, theta=th)
        if np.isnan(d1) or np.isinf(d1):
            d1, d2 = 0.0, 0.0
        df += r * d1
        ddf += r * r * d2
    return df, ddf


def joint_minimize_newton(ots, rates, a, b, x1, xguess, x2, xacc, max_steps, thetas=None):
    """-> (optx, d2l, evaluated points, status) as OracleTree.minimize_newton"""
    if thetas is None:
        thetas = [ot.theta(a, b)[0] for ot in ots]
    evaluated = []

    def func_derv(x):
        evaluated.append(x)
        df, ddf = joint_derv(ots, rates, a, b, x, thetas)
        if not np.isfinite(df):
            df, ddf = 0.0, 0.0
        return -df, -ddf

    rts = min(max(xguess, x1), x2)
    f, df = func_derv(rts)
    d2l = df
    if not (np.isfinite(f) and np.isfinite(df)):
        return rts, d2l, evaluated, "nonfinite"
    if df >= 0.0 and abs(f) < xacc:
        return rts, d2l, evaluated, "ok"
    if f < 0.0:
        xl, xh = rts, x2
    else:
        xh, xl = rts, x1
    dx = abs(xh - xl)
    for j in range(1, max_steps + 1):
        rts_old = rts
        if df <= 0.0 or ((rts - xh) * df - f) * ((rts - xl) * df - f) >= 0.0:
            dx = 0.5 * (xh - xl)
            rts = xl + dx
            d2l = df
            if xl == rts:
                return rts, d2l, evaluated, "ok"
        else:
            dx = f / df
            temp = rts
            rts -= dx
            d2l = df
            if temp == rts:
                return rts, d2l, evaluated, "ok"
        if abs(dx) < xacc or j == max_steps:
            return rts_old, d2l, evaluated, "ok"
        f, df = func_derv(rts)
        if not (np.isfinite(f) and np.isfinite(df)):
            return rts_old, d2l, evaluated, "nonfinite"
        if df > 0.0 and abs(f) < xacc:
            return rts, df, evaluated, "ok"
        if f < 0.0:
            xl = rts
        else:
            xh = rts
    return 0.0, 0.0, evaluated, "maxsteps"


def joint_lnl_from_theta(ots, rates, a, b, x, thetas=None):
    out = []
    for k, (ot, r) in enumerate(zip(ots, rates)):
        if thetas is None:
            th, sf = ot.theta(a, b)
        else:
            th, sf = thetas[k]
        out.append(ot.lnl_from_theta(a, b, length=r * x, theta=th, sf=sf)[0])
    return np.array(out)


def gene_rate_step(lnl_at, rates, nsites, gradient_epsilon, brent):
    """lnl_at(p, s): member p's log-likelihood with the super tree's lengths times s.  brent: the BrentStateMachine class.
    -> (new rates after the normalisation, factor the super tree is scaled by, evaluations per member, lockstep rounds,
    per-member lnL at the optimum)"""
    total = float(sum(nsites))
    tol = max(0.001, gradient_epsilon)
    ms = [brent(min(r, 1.0 / n), r, max(total / n, r), tol) for r, n in zip(rates, nsites)]
    rounds = 0
    while not all(m.done for m in ms):
        rounds += 1
        for p, m in enumerate(ms):
            if not m.done:
                m.update(-lnl_at(p, m.x))
    res = [m.result() for m in ms]
    new = np.array([r[0] for r in res])
    s = float(np.dot(new, nsites)) / total
    return new * (1.0 / s), s, [r[2] for r in res], rounds, np.array([-r[1] for r in res])


# ---- partition files ------------------------------------------------------------------------------------------------
class PartitionFileError(ValueError):
    pass


def _split_model(line):
    """the model field ends at the first comma outside braces (a -m string carries commas inside them)"""
    depth = 0
    for i, ch in enumerate(line):
        if ch == "{":
            depth += 1
        elif ch == "}":
            depth -= 1
        elif ch == "," and depth == 0:
            return line[:i], line[i + 1:]
    raise PartitionFileError("no ',' after the model")


def parse_positions(spec, nsite):
    """'1-100, 250-400 401-500\\3' -> 0-based site indices, in order (extractSiteID)"""
    spec = re.sub(r"\s*([-\\])\s*", r"\1", spec.replace(",", " ").strip())
    sites = []
    for tok in spec.split():
        m = re.fullmatch(r"(\d+)(?:-(\d+)(?:\\(\d+))?)?", tok)
        if not m:
            raise PartitionFileError("bad range %r" % tok)
        lo = int(m.group(1))
        hi = int(m.group(2)) if m.group(2) else lo
        step = int(m.group(3)) if m.group(3) else 1
        if lo < 1 or hi > nsite:
            raise PartitionFileError("position outside the alignment in %r" % tok)
        if lo > hi:
            raise PartitionFileError("empty range %r" % tok)
        if step < 1:
            raise PartitionFileError("bad step in %r" % tok)
        sites.extend(range(lo - 1, hi, step))
    if not sites:
        raise PartitionFileError("partition without a site")
    return sites


def parse_partition_file(text, nsite):
    """-> [(model string verbatim, name, [0-based sites])]"""
    parts = []
    for raw in text.splitlines():
        line = raw.strip()
        if not line:
            continue
        model, rest = _split_model(line)
        if "=" not in rest:
            raise PartitionFileError("no '=' in %r" % raw)
        name, spec = rest.split("=", 1)
        model, name = model.strip(), name.strip()
        if not model or not name:
            raise PartitionFileError("missing model or name in %r" % raw)
        parts.append((model, name, parse_positions(spec, nsite)))
    if not parts:
        raise PartitionFileError("no partition")
    return parts


def extract_sites(columns, sites):
    """columns[taxon][site] (any 2-D array) -> the chosen sites, in order"""
    return np.ascontiguousarray(np.asarray(columns)[:, sites])


# ---- shared data: the mixed group of the partition tests ------------------------------------------------------------
MIXED_RATES = [1.0, 0.4, 2.3, 0.7]
MIXED_UNKNOWN_TAXA = [[], [2, 5], [0], [6, 7, 1]]
MIXED_NTAXA = 8
NEWTON_SETUPS = [(1e-6, None, 100.0, 1e-6, 100), (1e-6, 60.0, 100.0, 1e-6, 100), (1e-6, 0.01, 0.03, 1e-6, 100),
                 (0.6, 0.9, 100.0, 1e-6, 100), (1e-6, 3.0, 100.0, 1e-6, 3)]   # tests/test_newton_oracle_gpu.py


def member_data(synth, oracle, nwk, n, ncat, seq_type, nsites, seed, rate, unknown_taxa=(), missing=0.02, model=None):
    """one member: sites simulated on the super tree scaled by `rate`, `missing` cells and all-unknown rows knocked out"""
    if model is None:
        if n == 4:
            model = synth.gtr_model(alpha=0.9, ncat=ncat)
        else:
            model = synth.random_reversible_model(n, seed, alpha=0.9 if ncat > 1 else None, ncat=ncat)
    su = oracle.state_unknown_for(n, seq_type)
    st = synth.simulate_alignment(scale_newick(nwk, rate), model, nsites, seed + 1, missing, su)
    for t in unknown_taxa:
        st[t, :] = su
    pat, freq = synth.compress_patterns(st)
    return dict(n=n, ncat=ncat, seq_type=seq_type, model=model, sites=st, pat=pat, freq=freq,
                invar=synth.ptn_invar_for(pat, model), rate=rate, nsite=nsites, su=su)


_cache = {}


def mixed_group(synth, oracle):
    """8 taxa; DNA GTR+G4 300 sites, DNA 1 category 70 sites, protein +G4 200 sites, binary 2 categories 90 sites"""
    if "mixed" not in _cache:
        nwk = synth.random_tree_newick(MIXED_NTAXA, 77, 0.02, 0.2)
        shapes = [(4, 4, SEQ_DNA, 300), (4, 1, SEQ_DNA, 70), (20, 4, SEQ_PROTEIN, 200), (2, 2, SEQ_BINARY, 90)]
        members = [member_data(synth, oracle, nwk, n, c, s, ns, 500 + 10 * k, MIXED_RATES[k], MIXED_UNKNOWN_TAXA[k])
                   for k, (n, c, s, ns) in enumerate(shapes)]
        _cache["mixed"] = (nwk, members)
    return _cache["mixed"]


def oracle_member(oracle, nwk, d, scale=None):
    """the member's OracleTree on the super tree scaled by its rate (or by `scale`)"""
    return oracle.OracleTree(scale_newick(nwk, d["rate"] if scale is None else scale), d["n"], d["seq_type"], d["pat"],
                             d["freq"], d["invar"], d["model"])


def device_member(pkg, nwk, d, scale=None):
    t = pkg.PhyloTree(scale_newick(nwk, d["rate"] if scale is None else scale))
    t.set_alignment(d["n"], d["seq_type"], d["pat"], d["freq"], d["invar"])
    t.set_model(d["model"])
    t.set_likelihood_kernel(pkg.LK_EIGEN_HIP)
    t.attach_engine(0)
    return t


def tree_edges(ot, nnodes):
    return [(a, b) for a in range(nnodes) for b, _ in ot.adj[a] if a < b]


# ---- the mixed group as files: one PHYLIP alignment of all four data types + a partition file + a named tree -----------
LETTERS = {SEQ_DNA: "ACGT", SEQ_PROTEIN: "ARNDCQEGHILKMFPSTWYV", SEQ_BINARY: "01"}
MIXED_MODEL_STRINGS = ["GTR{1.5,2.4,1.8,1.9,2.8}+F{0.25,0.26,0.25,0.24}+G4{0.9}", "GTR{1.5,2.4,1.8,1.9,2.8}+F{0.25,0.26,0.25,0.24}",
                       "POISSON+G4{0.9}", "GTR2+F{0.4,0.6}+G2{0.9}"]
MIXED_NAMES = ["dna_g4", "dna_1cat", "protein", "binary"]


def sites_as_text(d):
    """the member's site columns as one string per taxon ('-' for the unknown state)"""
    letters = LETTERS[d["seq_type"]]
    return ["".join(letters[s] if s < len(letters) else "-" for s in row) for row in d["sites"]]


def named_tree(nwk, names):
    return re.sub(r"([(,])(\d+):", lambda m: "%s%s:" % (m.group(1), names[int(m.group(2))]), nwk)


def mixed_files(directory, synth, oracle):
    """-> (alignment path, partition file path, tree path, taxon names)"""
    nwk, members = mixed_group(synth, oracle)
    names = ["t%d" % i for i in range(MIXED_NTAXA)]
    rows = ["".join(parts) for parts in zip(*[sites_as_text(d) for d in members])]
    aln = os.path.join(str(directory), "mixed.phy")
    with open(aln, "w") as f:
        f.write("%d %d\n" % (len(names), len(rows[0])))
        for n, r in zip(names, rows):
            f.write("%s %s\n" % (n, r))
    part = os.path.join(str(directory), "mixed.parts")
    with open(part, "w") as f:
        first = 1
        for d, ms, nm in zip(members, MIXED_MODEL_STRINGS, MIXED_NAMES):
            f.write("%s, %s = %d-%d\n" % (ms, nm, first, first + d["nsite"] - 1))
            first += d["nsite"]
    tree = os.path.join(str(directory), "mixed.nwk")
    with open(tree, "w") as f:
        f.write(named_tree(nwk, names) + "\n")
    return aln, part, tree, names
