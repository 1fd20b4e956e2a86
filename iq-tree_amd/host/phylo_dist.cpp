// phylo_dist.cpp -- pairwise ML distances, likelihood mapping and BIONJ (see phylo_host.h)
#include "phylo_host.h"

#include <stdio.h>

#include <algorithm>

namespace iqhost {

// ---- pairwise ML distances, phylotree.cpp:2432-2541
void PhyloTree::computeDist(const double *init, double *dist, double *d2l) {
    needDevice("computeDist");
    noCallerCollective("computeDist");
    pushInputs();
    check(iqhip_pair_distances(engine, init, min_branch_length, MAX_GENETIC_DIST, min_branch_length, 100, dist, d2l, nullptr),
          "iqhip_pair_distances");
}

void PhyloTree::pairCounts(const int32_t *pairs, int npairs, double *counts) {
    needDevice("pairCounts");
    pushInputs();
    check(iqhip_pair_counts(engine, pairs, npairs, counts), "iqhip_pair_counts");
}

// ---- likelihood mapping, quartet.cpp:676-1152, 1340-1505 (include/iqhip.h "Likelihood mapping"; lmap_host.h)
void PhyloTree::quartetCells(const int32_t *quartets, int nq, double *cells, int32_t *nother) {
    needDevice("quartetCells");
    pushInputs();
    check(iqhip_quartet_cells(engine, quartets, nq, cells, nother), "iqhip_quartet_cells");
}

void PhyloTree::computeQuartetLikelihoods(const int32_t *quartets, int nq, iqhip_quartet_result *results, int iterations,
                                          double tolerance, const double *const_invar) {
    needDevice("computeQuartetLikelihoods");
    noCallerCollective("computeQuartetLikelihoods");
    pushInputs();
    check(iqhip_quartet_likelihoods(engine, quartets, nq, const_invar, min_branch_length, max_branch_length, min_branch_length,
                                    100, 0.95, iterations, tolerance, results),
          "iqhip_quartet_likelihoods");
}

void PhyloTree::doLikelihoodMapping(int64_t nquartets, uint64_t seed, LmapResult &out, const double *const_invar) {
    if (leafNum < 4) throw std::runtime_error("likelihood mapping needs at least 4 taxa");
    if (nquartets < 0) throw std::runtime_error("doLikelihoodMapping: negative number of quartets");
    std::vector<int32_t> quartets;
    if (nquartets == 0 || nquartets >= lmap::numQuartets(leafNum)) lmap::allQuartets(leafNum, quartets);
    else lmap::drawQuartets(leafNum, nquartets, seed, quartets);
    const size_t nq = quartets.size() / 4;
    if (nq > 2147483647u) throw std::runtime_error("doLikelihoodMapping: too many quartets for one call");
    std::vector<iqhip_quartet_result> res(nq);
    computeQuartetLikelihoods(quartets.data(), (int)nq, res.data(), 10, 0.1, const_invar);
    out = LmapResult();
    out.info.resize(nq);
    out.seq_count.assign((size_t)(leafNum + 1) * 10, 0);
    for (size_t q = 0; q < nq; q++) {
        lmap::QuartetInfo &qi = out.info[q];
        for (int k = 0; k < 4; k++) qi.seqID[k] = quartets[4 * q + k];
        for (int k = 0; k < 3; k++) qi.logl[k] = res[q].logl[k];
        lmap::region(qi.logl, qi.qweight, &qi.corner, &qi.area);
        out.areacount[qi.area]++;
        out.cornercount[qi.corner]++;
        for (int col : {qi.area, 7 + qi.corner}) {
            out.seq_count[(size_t)leafNum * 10 + col]++;
            for (int k = 0; k < 4; k++) out.seq_count[(size_t)qi.seqID[k] * 10 + col]++;
        }
    }
}

// ---- BIONJ, phylotree.cpp:2619-2635 over bionj.h (include/iqhip.h "BIONJ")
std::string PhyloTree::bionjNewick(const iqhip_bionj_step *steps, int n, const int32_t *last, const double *last_len,
                                   const std::vector<std::string> &names) {
    if (n < 3 || (int)names.size() != n) throw std::runtime_error("bionjNewick: one name per taxon, at least 3 taxa");
    if (!last || !last_len || (n > 3 && !steps)) throw std::runtime_error("bionjNewick: null argument");
    auto fmt = [](double len) {
        char buf[400];
        snprintf(buf, sizeof buf, "%10.8f", len);
        return std::string(buf);
    };
    std::vector<std::string> sub(names);
    std::vector<char> gone((size_t)n, 0);
    for (int k = 0; k < n - 3; k++) {
        const int a = steps[k].a, b = steps[k].b;
        if (a < 0 || a >= n || b < 0 || b >= n || a == b || gone[(size_t)a] || gone[(size_t)b])
            throw std::runtime_error("bionjNewick: step " + std::to_string(k) + " merges a row that is not active");
        sub[(size_t)a] = "(" + sub[(size_t)a] + ":" + fmt(steps[k].la) + "," + sub[(size_t)b] + ":" + fmt(steps[k].lb) + ")";
        sub[(size_t)b].clear();
        gone[(size_t)b] = 1;
    }
    std::string out = "(";
    for (int k = 0; k < 3; k++) {
        const int l = last[k];
        if (l < 0 || l >= n || gone[(size_t)l] || (k > 0 && l <= last[k - 1]))
            throw std::runtime_error("bionjNewick: the last three rows must be active and ascending");
        out += sub[(size_t)l] + ":" + fmt(last_len[k]) + (k < 2 ? "," : ");");
    }
    return out;
}

void PhyloTree::computeBioNJ(const double *dist, const double *var, std::string *newick, iqhip_bionj_step *steps_out,
                             int32_t *last_out, double *last_len_out) {
    needDevice("computeBioNJ");
    const int n = leafNum;
    if (n < 3) throw std::runtime_error("computeBioNJ needs at least 3 taxa");
    for (int k = 0; k < n; k++)
        if (k >= (int)nodes.size() || !nodes[(size_t)k]) throw std::runtime_error("computeBioNJ: the taxa are not known yet");
    const std::vector<std::string> names = leafNames();
    std::vector<iqhip_bionj_step> steps((size_t)std::max(1, n - 3));
    int32_t last[3];
    double last_len[3];
    check(iqhip_bionj(engine, n, dist, var, steps.data(), last, last_len), "iqhip_bionj");
    const std::string nwk = bionjNewick(steps.data(), n, last, last_len, names);
    const bool non_empty_tree = root != nullptr;
    readTreeString(nwk, names);   // (a tree read with taxon ids as labels has the ids as its names)
    if (non_empty_tree) initializeAllPartialLh();
    if (newick) *newick = nwk;
    if (steps_out) std::copy(steps.begin(), steps.begin() + (n - 3), steps_out);
    if (last_out) std::copy(last, last + 3, last_out);
    if (last_len_out) std::copy(last_len, last_len + 3, last_len_out);
}

}  // namespace iqhost
