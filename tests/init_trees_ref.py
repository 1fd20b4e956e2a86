"""Python restatement of the starting population of the tree search -- createInitTrees + initCandidateTreeSet
(iqtree.cpp:577-773) as TreeSearch restates them with num_init_trees > 0 -- over tests/nni_search_ref.py (imported, not
edited) and calls that existed before the forest: search_rand / search_rand_int for the addition orders,
compute_parsimony_tree and optimize_parsimony_spr for every parsimony tree ALONE, optimize_all_branches for the scores.
The stochastic loop that follows is replay_loop: nni_search_ref.replay_search without its starting iteration."""
import nni_search_ref as ref


def parsimony_orders(pkg, seed, k, ntaxa):
    """order j: Fisher-Yates, for i = ntaxa-1 .. 1 swap i with search_rand_int(search_rand(seed, 0, j * ntaxa + i), i + 1)"""
    out = []
    for j in range(k):
        o = list(range(ntaxa))
        for i in range(ntaxa - 1, 0, -1):
            r = pkg.search_rand_int(pkg.search_rand(seed, 0, j * ntaxa + i), i + 1)
            o[i], o[r] = o[r], o[i]
        out.append(o)
    return out


def init_candidate_set(pkg, make_tree, start_newick, seed, num_init, num_nni, spr_radius=0, boot=None):
    """-> (init trees [(score, tree, topology)] in generation order, duplicates, kept [(score, tree, topology)] best first,
    scores of the iterations 1 .. M, their optimize_nni traces, the candidate set after them)"""
    cand = ref.CandidateSet()
    init, seen, dup = [], set(), 0

    def add(tree, topology):
        score = tree.optimize_all_branches(2)
        entry = (score, tree.tree_string(), topology)
        cand.update(entry[1], topology, score)
        init.append(entry)
        seen.add(topology)

    t = make_tree(start_newick)
    add(t, t.sorted_taxon_id_string())
    for order in parsimony_orders(pkg, seed, num_init - 1, t.num_leaves):
        p = make_tree(start_newick)
        p.compute_parsimony_tree(order)
        if spr_radius:
            p.optimize_parsimony_spr(spr_radius)
        q = make_tree(p.tree_string())
        topology = q.sorted_taxon_id_string()
        if topology in seen:
            dup += 1
            continue
        add(q, topology)
    kept = cand.ranked()[:max(1, min(num_nni, len(cand.trees)))]
    cand = ref.CandidateSet()
    scores, traces = [], []
    for _, newick, _ in kept:
        tree = make_tree(newick)
        score, _, _, steps = ref.optimize_nni(tree, boot=boot)
        traces.append(steps)
        if score > cand.best_score() + ref.MODEPS:
            score = tree.optimize_all_branches(100, ref.LOGLH_EPSILON)
        cand.update(tree.tree_string(), tree.sorted_taxon_id_string(), score)
        scores.append(score)
    return init, dup, kept, scores, traces, cand


def replay_loop(make_tree, cand, iterations, boot=None):
    """the loop of doTreeSearch on the candidate set `cand`, with the parent ranks and random NNIs of `iterations` (the
    entries of the C++ trace after the starting trees) -> their scores and optimize_nni traces; cand is updated"""
    out, traces = [], []
    for it in iterations:
        if boot:
            boot.next_iteration()
        tree = make_tree(cand.by_rank(it["parent"])[1])
        for a, b, bit1, bit2 in it["random_nnis"]:
            tree.do_random_nni(a, b, bit1, bit2)
        tree.clear_all_partial_lh()
        score, _, _, steps = ref.optimize_nni(tree, boot=boot)
        traces.append(steps)
        if score > cand.best_score() + ref.MODEPS:
            score = tree.optimize_all_branches(100, ref.LOGLH_EPSILON)
        cand.update(tree.tree_string(), tree.sorted_taxon_id_string(), score)
        out.append(score)
    return out, traces
