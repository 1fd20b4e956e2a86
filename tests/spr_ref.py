"""A numpy restatement of the parsimony SPR scan and search, written from the algorithm on top of fitch_ref.py: the expected
values of tests/test_pars_spr_host.py and tests/test_pars_spr_gpu.py.

A move prunes the subtree at node s seen from its neighbour p (p goes with it: p's other neighbours q1, q2 are joined) and
regrafts it into a branch (a, b) of the rest.  collect_jobs enumerates, per internal node p (ascending) and neighbour s (in
neighbour order), the branches within `radius` of the merged branch q1 -- q2 in depth-first pre-order, as steps:
  parent < 0       U = V(side)                       (depth 0: what lies beyond the merged branch, seen from its other end)
  otherwise        U = update(U[parent], V(side))    (the pruned tree's directed vector on the prune-point side of (a, b))
  score            insert_score(U, V(target), S) + S.score, with a subtree S in the place of fitch_ref's tip
V(x) = (node, seen from): directed vectors of the UNPRUNED tree that do not contain S.  The first root step is the current
tree; the second (the same branch from the other end) is not scored.  Depth 1 = the branches next to the merged branch.
search() runs the rounds: all prune points against the same tree, the FIRST minimum in job and step order, applied when it
is below the current score.  Trees are fitch_ref's ordered adjacency dicts; apply_move edits the neighbour lists in place
(positions kept), which fixes the enumeration order of the next round."""
import numpy as np

import fitch_ref as F

NO_SCORE = 1


def collect_jobs(adj, ntaxa, radius):
    """-> [dict(p, s, steps=[dict(parent, side, target, move=(a, b), depth, scored)])]; jobs with no step of depth >= 1 are
    left out"""
    jobs = []
    for p in sorted(u for u in adj if len(adj[u]) > 1):
        assert len(adj[p]) == 3
        for s in adj[p]:
            q1, q2 = [k for k in adj[p] if k != s]
            steps = []

            def go(a, dad, parent, depth):
                if a < ntaxa or depth > radius:
                    return
                x, y = [k for k in adj[a] if k != dad]
                for tgt, side in ((x, y), (y, x)):
                    k = len(steps)
                    steps.append(dict(parent=parent, side=(side, a), target=(tgt, a), move=(a, tgt), depth=depth, scored=True))
                    go(tgt, a, k, depth + 1)

            steps.append(dict(parent=-1, side=(q2, p), target=(q1, p), move=(q1, q2), depth=0, scored=True))
            go(q1, p, 0, 1)
            second = len(steps)
            steps.append(dict(parent=-1, side=(q1, p), target=(q2, p), move=(q2, q1), depth=0, scored=False))
            go(q2, p, second, 1)
            if len(steps) > 2:
                jobs.append(dict(p=p, s=s, steps=steps))
    return jobs


def job_scores(job, dv):
    """the score of every step of a job (None where not scored) from the directed vectors of the unpruned tree"""
    S = dv[(job["s"], job["p"])]
    U, out = [], []
    for st in job["steps"]:
        y = dv[st["side"]]
        u = y if st["parent"] < 0 else F.update(U[st["parent"]], y)
        U.append(u)
        out.append(F.insert_score(u, dv[st["target"]], S) + S[1] if st["scored"] else None)
    return out


def apply_move(adj, p, s, a, b):
    """a copy of adj with the subtree at s (seen from p) regrafted, with p, into the branch (a, b)"""
    new = {u: list(v) for u, v in adj.items()}
    q1, q2 = [k for k in new[p] if k != s]
    assert {a, b} != {q1, q2} and p not in (a, b)
    i1, i2 = new[p].index(q1), new[p].index(q2)
    new[q1][new[q1].index(p)] = q2
    new[q2][new[q2].index(p)] = q1
    new[a][new[a].index(b)] = p
    new[b][new[b].index(a)] = p
    new[p][i1], new[p][i2] = a, b
    return new


def search(adj, tips, ntaxa, radius, max_rounds=None):
    """-> (score, final adj, [per round dict(score_before, job, step, score, steps_scored, move=(p, s, a, b), applied)])"""
    rounds, current = [], None
    while max_rounds is None or len(rounds) < max_rounds:
        jobs = collect_jobs(adj, ntaxa, radius)
        if not jobs:
            break
        dv = F.directed_vectors(adj, tips)
        best = None
        nscored = 0
        for j, job in enumerate(jobs):
            for k, sc in enumerate(job_scores(job, dv)):
                if sc is None:
                    continue
                nscored += 1
                if best is None or sc < best[0]:
                    best = (sc, j, k)
        before = job_scores(dict(jobs[0], steps=jobs[0]["steps"][:1]), dv)[0]
        sc, j, k = best
        job = jobs[j]
        applied = sc < before
        rounds.append(dict(score_before=before, job=j, step=k, score=sc, steps_scored=nscored,
                           move=(job["p"], job["s"]) + job["steps"][k]["move"], applied=applied))
        current = sc if applied else before
        if not applied:
            break
        assert job["steps"][k]["depth"] >= 1
        adj = apply_move(adj, job["p"], job["s"], *job["steps"][k]["move"])
    if current is None:
        current = F.tree_score(adj, tips)
    return current, adj, rounds


def program(jobs, slot_of):
    """the jobs as the rows iqhip_pars_spr_scan takes: (jobs[njobs, 4], steps[nsteps, 4]); slot_of(node, seen_from) -> slot"""
    jrows, srows = [], []
    for job in jobs:
        jrows.append((slot_of(job["s"], job["p"]), len(srows), len(job["steps"]), 0))
        for st in job["steps"]:
            srows.append((st["parent"], slot_of(*st["side"]), slot_of(*st["target"]), 0 if st["scored"] else NO_SCORE))
    return np.array(jrows, dtype=np.int32).reshape(-1, 4), np.array(srows, dtype=np.int32).reshape(-1, 4)


def first_minima(jobs_rows, scores):
    """(best_step[njobs], best_score[njobs], best_job) of a returned score array: first minima, -1 / INT32_MAX / -1 for none"""
    bs, bsc = [], []
    for _, first, n, _ in jobs_rows:
        sc = [(int(v), k) for k, v in enumerate(scores[first:first + n]) if v >= 0]
        v, k = min(sc) if sc else (0x7fffffff, -1)
        bs.append(k)
        bsc.append(v)
    real = [(v, j) for j, v in enumerate(bsc) if v != 0x7fffffff]
    return bs, bsc, (min(real)[1] if real else -1)


def mirror_adjacency(tree):
    """the ordered adjacency dict of a host-mirror PhyloTree"""
    return {u: [v for v, _ in tree.neighbors(u)] for u in range(2 * tree.num_leaves - 2)}
