"""Python restatement of the reference's NNI search -- IQTree::optimizeNNI (iqtree.cpp:2125-2288), doRandomNNIs
(:1302-1339) and the snni branch of doTreeSearch (:1834-2098) -- written from the reference's text over calls that existed
before the C++ search (evaluate_nnis[5]_batch, nni_for_branch, optimize_all_branches, compute_likelihood, ...) plus the thin
tree-edit primitives do_nni / change_nni_brans / save_branch_lengths / restore_branch_lengths / do_random_nni, which the host
tests check on their own against topology arithmetic.  The decisions (positive moves, sort, non-conflicting set, branch lists,
candidate set, stop rule) are plain Python here; tests compare the C++ loop's trace with this one's."""
import math

LOGLH_EPSILON = 0.001
MODEPS = 0.01
NNI_MAX_NR_STEP = 10


def adjacency(tree):
    return [[b for b, _ in tree.neighbors(v)] for v in range(tree.num_nodes)]


def internal_branches(adj):
    """ascending node id, node1 < node2: the order of PhyloTree::internalBranches"""
    return [(a, b) for a in range(len(adj)) for b in adj[a] if a < b and len(adj[a]) > 1 and len(adj[b]) > 1]


def select_non_conflicting(moves):
    taken = []
    for m in moves:
        if not any({m["node1"], m["node2"]} & {t["node1"], t["node2"]} for t in taken):
            taken.append(m)
    return taken


def non_touching(moves):
    """the moves, in order, whose four nodes (both ends, both swapped subtree roots) are free of every earlier kept move's:
    such moves can be applied and reverted in any order"""
    kept, used = [], set()
    for m in moves:
        four = {m["node1"], m["node2"], m["node1_nei"], m["node2_nei"]}
        if not four & used:
            kept.append(m)
            used |= four
    return kept


def branches_for_nni(applied, adj):
    """getBranchesForNNI over getInnerBranches(depth 2), breadth-limited walk restated with an explicit recursion"""
    out = []

    def exists(a, b):
        return (a, b) in out or (b, a) in out

    def inner(depth, node, dad):
        if depth == 0:
            return
        for nb in adj[node]:
            if nb != dad and len(adj[nb]) > 1 and not exists(node, nb):
                out.append((node, nb))
                inner(depth - 1, nb, node)

    for m in applied:
        if not exists(m["node1"], m["node2"]):
            out.append((m["node1"], m["node2"]))
        inner(2, m["node1"], m["node2"])
        inner(2, m["node2"], m["node1"])
    return out


def evaluate(tree, branches, nni5, batched):
    """both candidates of every listed branch (node1 < node2), in list order"""
    branches = [(min(a, b), max(a, b)) for a, b in branches]
    if batched:
        full = tree.evaluate_nnis5_batch() if nni5 else tree.evaluate_nnis_batch()
        by = {}
        for m in full:
            by.setdefault((m["node1"], m["node2"]), []).append(m)
        moves = [m for br in branches for m in by[br]]
    else:
        moves = []
        for a, b in branches:
            for newloglh, nei1, nei2, lens in tree.nni_for_branch(a, b, nni5=nni5):
                moves.append(dict(node1=a, node2=b, node1_nei=nei1, node2_nei=nei2, newloglh=newloglh, new_lens=list(lens)))
    for m in moves:
        if "new_lens" not in m:
            m["new_lens"] = [m["new_len"], 0.0, 0.0, 0.0, 0.0]
    return moves


def optimize_nni(tree, nni5=True, speed=True, batched=True, boot=None):
    """-> (curScore, nni_count, nni_steps, trace); starts with compute_likelihood() as PhyloTree.optimize_nni does.
    boot: an object with current(tree, score) -- saveCurrentTree's place -- and evaluate(tree, listed) -> moves, which stands
    in for the evaluation and sees every candidate in evaluation order (the UFBoot replay of the GPU tests)"""
    cur = tree.compute_likelihood()
    ntaxa = tree.num_leaves
    roll_back = False
    nni_count = 0
    num_nnis = 0
    branches = []
    trace = []
    non_conf = []
    nni_steps = 1
    while nni_steps <= ntaxa:
        old = cur
        st = dict(branches=[], all_branches=False, positive=[], applied=[], score=cur, rolled_back=False)
        if not roll_back:
            if boot:
                boot.current(tree, cur)
            lenvec = tree.save_branch_lengths()
            adj = adjacency(tree)
            st["all_branches"] = not branches
            listed = internal_branches(adj) if not branches else [(min(a, b), max(a, b)) for a, b in branches]
            moves = boot.evaluate(tree, listed) if boot else evaluate(tree, listed, nni5, batched)
            plus = []
            for q in range(0, len(moves), 2):
                best = moves[q] if moves[q]["newloglh"] > moves[q + 1]["newloglh"] else moves[q + 1]
                if best["newloglh"] > cur + LOGLH_EPSILON:
                    plus.append(best)
            plus.sort(key=lambda m: -m["newloglh"])   # stable
            st["branches"] = listed
            st["positive"] = plus
            if not plus:
                trace.append(st)
                break
            non_conf = select_non_conflicting(plus)
            num_nnis = len(non_conf)
        # the reference's moves hold neighbour iterators (slots): a move whose end an earlier move of the step re-hung swaps
        # what its slots hold by then
        before = adjacency(tree)
        slots = [(before[m["node1"]].index(m["node1_nei"]), before[m["node2"]].index(m["node2_nei"])) for m in non_conf[:num_nnis]]
        applied = []
        for m, (s1, s2) in zip(non_conf[:num_nnis], slots):
            now = adjacency(tree)
            m = dict(m, node1_nei=now[m["node1"]][s1], node2_nei=now[m["node2"]][s2])
            tree.do_nni(m)
            applied.append(m)
            tree.change_nni_brans(m, nni5)
        branches = branches_for_nni(applied, adjacency(tree)) if speed else []
        cur = tree.optimize_all_branches(1, LOGLH_EPSILON, NNI_MAX_NR_STEP)
        st["applied"] = applied
        st["score"] = cur
        if cur >= non_conf[0]["newloglh"] - LOGLH_EPSILON:
            nni_count += num_nnis
            roll_back = False
        else:
            for m in reversed(applied):     # last first: the order that also undoes adjacent moves
                tree.do_nni(m)
            tree.restore_branch_lengths(lenvec)
            tree.clear_all_partial_lh()
            roll_back = True
            num_nnis = 1
            cur = old
            st["rolled_back"] = True
        trace.append(st)
        if cur - old < 0.1:
            break
        nni_steps += 1
    return cur, nni_count, nni_steps, trace


class CandidateSet:
    """candidateset.cpp:158-201 on a list kept in ascending score, equal scores in insertion order"""

    def __init__(self, max_candidates=1000):
        self.trees = []   # (score, tree, topology)
        self.max_candidates = max_candidates

    def _insert(self, entry):
        k = 0
        while k < len(self.trees) and self.trees[k][0] <= entry[0]:
            k += 1
        self.trees.insert(k, entry)

    def update(self, tree, topology, score):
        known = [e for e in self.trees if e[2] == topology]
        if known:
            if known[0][0] < score:
                for k in range(len(self.trees) - 1, -1, -1):
                    if self.trees[k][2] == topology:
                        del self.trees[k]
                        break
                self._insert((score, tree, topology))
            return False
        if self.trees and self.trees[0][0] < score and len(self.trees) >= self.max_candidates:
            del self.trees[0]
        self._insert((score, tree, topology))
        return True

    def best_score(self):
        return self.trees[-1][0] if self.trees else -1.7976931348623157e308

    def by_rank(self, rank):
        return self.trees[len(self.trees) - 1 - rank]

    def ranked(self):
        return list(reversed(self.trees))


def replay_search(make_tree, start_newick, iterations, nni5=True, speed=True, boot=None):
    """doTreeSearch with the parent ranks and random NNIs taken from `iterations` (the C++ trace): the same per-iteration
    scores and the same candidate set must come out.  make_tree(newick) builds an attached tree; boot: see optimize_nni,
    with next_iteration() at the start of every search iteration."""
    cand = CandidateSet()
    out = []
    tree = make_tree(start_newick)
    score, *_ = optimize_nni(tree, nni5, speed, boot=boot)
    cand.update(tree.tree_string(), tree.sorted_taxon_id_string(), score)
    out.append(score)
    for it in iterations[1:]:
        if boot:
            boot.next_iteration()
        tree = make_tree(cand.by_rank(it["parent"])[1])
        for a, b, bit1, bit2 in it["random_nnis"]:
            tree.do_random_nni(a, b, bit1, bit2)
        tree.clear_all_partial_lh()
        score, *_ = optimize_nni(tree, nni5, speed, boot=boot)
        if score > cand.best_score() + MODEPS:
            score = tree.optimize_all_branches(100, LOGLH_EPSILON)
        cand.update(tree.tree_string(), tree.sorted_taxon_id_string(), score)
        out.append(score)
    return out, cand


def pearson(x, y):
    mx, my = sum(x) / len(x), sum(y) / len(y)
    sxy = sum((a - mx) * (b - my) for a, b in zip(x, y))
    return sxy / math.sqrt(sum((a - mx) ** 2 for a in x) * sum((b - my) ** 2 for b in y))
