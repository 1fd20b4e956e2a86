// iqhip_lnl -- stand-alone driver of the MI355X likelihood path, the counterpart of the reference's
// "evaluate one fixed tree" command line:
//     iqtree -s A.phy -te T.nwk -m 'GTR{a,b,c,d,e}+F{..}+G4{alpha}' [-blfix] -n 0 [-wsl] -pre X
// Everything it does goes through the same host mirror and C ABI as the tests: read the alignment
// (alignment_host), build the model inputs (model_host), read the tree, setLikelihoodKernel(HIP),
// computeLikelihood(), optionally optimizeAllBranches(), write X.iqhip (full-precision numbers) and
// X.sitelh.  With -alrt N [-lbp N] [-seed S] it then runs the SH-aLRT / local-bootstrap branch tests on the device
// (PhyloTree::testAllBranches) and prints the tree with SH-aLRT[/LBP] node labels; the site resamples are multinomial
// draws of its own generator (std::mt19937_64), not the reference's RNG stream.
// With -z <treefile> -zb N [-zw] [-au] [-seed S] it runs the tree topology tests of the reference's evaluateTrees on the
// trees of <treefile> (Newick, one after the other; -blfix keeps their branch lengths): one line per tree with logL,
// bp-RELL, p-KH, p-SH, [p-WKH, p-WSH,] c-ELW and +/- marks (confidence set; p >= 0.05), and with -au the bootstrap
// proportions of the AU test's ten scales r = 0.5 .. 1.4 (the AU p-value itself is not computed).  The resamples are drawn
// on the device by the engine's own generator (include/iqhip.h), not the reference's RNG stream.
// With -mldist <file> it computes the maximum-likelihood distance of every pair of sequences under the model on the device
// (PhyloTree::computeDist; it needs the model only, not the tree's lengths) and writes the matrix in the format of
// Alignment::printDist: the number of taxa, then per taxon its name left-aligned in max(10, longest name) columns, a blank
// and the distances in fixed notation with 7 decimals, each followed by a blank.
// With -parstree and no -te it builds the starting tree itself: stepwise addition by maximum parsimony on the device
// (PhyloTree::computeParsimonyTree; the addition order is a shuffle of the taxa drawn from -seed with std::mt19937_64, not
// the reference's RNG stream), branch lengths from fixNegativeBranch(true); it prints "Parsimony score: N (based on M
// informative sites)", writes <prefix>.parstree and goes on as if that file had been given with -te.  With -te, -pars
// prints the same line for the given tree.
// -sprrad R (1 .. 10) after -parstree or -pars runs the parsimony SPR search of radius R on that tree
// (PhyloTree::optimizeParsimonySPR: per round every prune point is scanned on the device and the best move is applied) and
// prints "Parsimony score after SPR: N (K rounds)" below the first line, K counting the round that found nothing;
// <prefix>.parstree then holds the improved tree.  Without -sprrad nothing changes (the reference's default radius of 6 is
// not applied on its own).
// With -bionjtree and no -te it builds the BIONJ starting tree (PhyloTree::computeBioNJ): the distances are computed and
// written as for -mldist (to <prefix>.mldist unless -mldist names the file), that text is read back -- the tree is a
// function of the file, as in the reference, whose BioNj::create reads it -- iqhip_bionj runs on the device, the tree is
// written to <prefix>.bionj with the reference's %10.8f lengths, fixNegativeBranch(false) replaces the negative ones and
// the run goes on as if the tree had been given with -te.  -te, -parstree and -bionjtree exclude each other.
// With -emrates (the model must have a +R<k> component) the weights and rates of the free-rate model are estimated by EM on
// the device (PhyloTree::optimizeFreeRatesEM) inside the loop of ModelFactory::optimizeParameters
// (model/modelfactory.cpp:952-1040) with the substitution model fixed: initial lnL; per round i = 2, 3, ...
// optimizeAllBranches(min(i, 3)) unless -blfix, then the EM, until the gain is not above 0.01 (params.modeps); a final
// optimizeAllBranches(100); rescaleRates; all branch lengths times the mean rate.  A bare +R<k> without braces is accepted
// with this flag only and starts from RateFree::setNCategory's point (equal weights, Gamma(1) mean rates).  It prints the
// reference's "Site proportion and rates:  (w,r) ..." line and the model string with the estimated +R<k>{...}, which is
// also what <prefix>.iqhip records.
// With -wsr it writes <prefix>.rate in the format of RateHeterogeneity::writeSiteRates (model/rateheterogeneity.cpp:56-81):
// per site the empirical-Bayes posterior mean rate, the best category (ties: the first, where the reference draws) and that
// category's rate, and prints the "Empirical proportions for each category:" line.  For +G and +R models alike.
// -m also takes the reference's MIX{m1[:rate[:weight]],m2,...} over the model names above, each class with its own {params}
// and +F{..}, followed by the rate suffixes (ModelMixture::initMixture): weights 1 / k unless given, normalised to sum 1,
// class rates rescaled to a global rate of 1, components in [class][rate] order.  With -mixweights the class weights are
// estimated by EM on the device (PhyloTree::optimizeMixtureWeights = ModelMixture::optimizeWeights) inside the same
// parameter / branch-length loop as -emrates; it prints the reference's "Mixture weights: w1 w2 ..." line and the model
// string with the estimated :rate:weight fields, which is also what <prefix>.iqhip records.  Before that the class rates are
// divided by their mean under the new weights and all branch lengths multiplied by it (likelihood unchanged), so the printed
// string, read back, is the model of the printed tree.  -mixweights refuses +I (the category rates would follow p_invar);
// -emrates, -wsr and +ASC refuse mixtures.
// With -optmodel the parameters of the model are estimated (ModelOptimizer, model_opt_host.h = ModelFactory::optimizeParameters
// over ModelGTR / RateGamma / RateInvar / RateGammaInvar::optimizeParameters): the rate parameters of the DNA models by the
// reference's BFGS, whose forward-difference stencils run as the classes of one candidate mixture engine (one traversal per
// stencil), the Gamma shape and the proportion of invariable sites by Brent, branch lengths in between unless -blfix.  With
// this flag the substitution model, +I and +G<k> may come without braces (-m GTR+I+G4) and start from the reference's
// defaults: rates 1, alpha 1, p-inv = half the fraction of constant sites; values in braces are starting values.  It prints
// the reference's "Optimal log-likelihood:", "Rate parameters:", "Proportion of invariable sites:" and "Gamma shape alpha:"
// lines and the model string with the estimates, which is also what <prefix>.iqhip records.  MIX{}, +R, +ASC and +FO are
// refused with this flag; without it a string that leaves values out is refused as before.
// With -bb N [-beps E] [-seed S] [-z <treefile>] [-wbt] it runs the ultrafast bootstrap's bookkeeping on the candidate trees of
// ONE search iteration per tree: N resamples of all sites are drawn on the device (iqhip_gen_boot_samples, stream 0xA0 of
// -seed); the -te tree goes first, then every tree of -z in file order; each is fed itself (after branch optimisation
// unless -blfix; PhyloTree::saveCurrentTree) and then its whole NNI neighbourhood through one update
// (PhyloTree::saveNNITrees), the log-likelihood cutoff following iqtree.cpp:1887-1888 between the trees.  It prints
// "UFBoot: K candidate trees, D distinct bootstrap trees", writes <prefix>.suptree (the -te tree with the supports
// round(100 count / N) as node labels) and <prefix>.contree (the greedy consensus of the winners) and, with -wbt,
// <prefix>.ufboot: the winner of every replicate in replicate order, topology only, children by ascending smallest taxon.
// E is params.ufboot_epsilon (0.5).  Without -search what is fed is what the given trees offer.  With -bb a -z file needs
// no -zb.
// With -search (or -t <file> = -te <file> -search) it runs the NNI tree search (TreeSearch, tree_search_host.h =
// IQTree::doTreeSearch with optimizeNNI) from the starting tree the command line gives (-te, -parstree, -bionjtree) after
// what comes before it (branch lengths, or -optmodel's estimates: the search takes the model as given): -n N a fixed number
// of iterations after the starting tree's, else it stops after -numstop N (100) iterations without a better tree; -pers P
// (0.5) the perturbation strength, -popsize K (5), -nni1 / -nni5, -allnni (every branch in every NNI step), -seed S the
// search's own random stream.  With -bb N the bootstrap is fed by the search, every evaluated tree as it is evaluated, and
// the search ends when the split frequencies of the bootstrap trees correlate by -bcor C (0.99) at a multiple of -nstep S
// (100) and -numstop iterations brought no better tree, or after -nm MAXIT (1000).  It prints "Iteration k / LogL: x" every
// 10th iteration, "BETTER TREE FOUND at iteration k: x", "NOTE: Bootstrap correlation coefficient of split occurrence
// frequencies: c" and "Optimal log-likelihood:", and writes <prefix>.treefile.  -search sets LM_ALL_BRANCH.
// With -search -numpars N [-toppars M] [-sprrad R] (the reference's flag names; its defaults are 100 and 20) the search
// starts as the reference's does (initCandidateTreeSet): the starting tree plus N - 1 stepwise-addition parsimony trees built
// in lockstep on the device (pars_forest_host.h; with -sprrad followed by SPR rounds of radius R), duplicate topologies
// dropped, every tree scored with two rounds of branch optimisation, the best M (20; lowered to N when N is smaller, as
// tools.cpp:2523-2525 does) optimised by NNI as the iterations 1 .. M.  It prints "Generating N-1 parsimony trees... D
// distinct starting trees", "Computing log-likelihood of D initial trees" and "Optimizing top M initial trees with NNI...".
// -n then counts the iterations after those M.  Without -numpars the search starts from the one tree, as before.
// With -q <partition file> (edge-linked, all partition rates 1) or -spp <partition file> (edge-linked, proportional: the
// rates start at 1 and are estimated) instead of -m it evaluates an edge-linked partition model (PhyloSuperTree,
// supertree_host.h): the file is RAxML-style, `MODEL, name = 1-100, 250-400, 401-500\3`, MODEL a string in the -m syntax
// above (JC2 / GTR2 name binary columns); every partition keeps every taxon.  PartitionModelPlen::optimizeParameters runs
// with the substitution parameters as given (-blfix: fixed branch lengths too).  It prints "Partition-specific rates:  r1
// r2 ..." (-spp only), one line "Partition <name>: <nsite> sites, <nptn> patterns, lnL <value>" per partition and "Optimal
// log-likelihood: <sum>", and writes <prefix>.treefile with the super tree's lengths.  With -bionjtree [-mldist <file>] and
// no -te / -t the starting tree is built first (PhyloSuperTreePlen::computeDist, computeBioNJ, fixNegativeBranch): from a
// star tree, all rates 1 and the models as the file gives them, every pair of sequences is solved jointly over the
// partitions on the device, the matrix is written (<prefix>.mldist unless -mldist names the file) and read back, the BIONJ
// tree goes to <prefix>.bionj, fixNegativeBranch(false) runs, the lines of the plain -bionjtree path and "Log-likelihood of
// the input tree" are printed, and the run goes on as -te <prefix>.bionj does (with -search: as -t).  -q / -spp exclude -m,
// -alrt, -z, -bb, -pars*, -emrates, -mixweights, -optmodel and -lmap, and -bionjtree / -mldist next to -te / -t.
// With -lmap N [-wql] [-seed S] it runs likelihood mapping (PhyloTree::doLikelihoodMapping) under the model after the tree's
// lnL and branch optimisation: N quartets drawn from -seed (N = 0 or N >= C(n,4): every unique quartet), the three trees of
// each optimised on the device in one call.  It prints "Computing N quartet likelihoods", "Quartets in region k: .." for
// the seven regions and the three summary lines (fully resolved = regions 1-3, partly resolved = 4-6, unresolved = 7, with
// percentages); -wql writes <prefix>.lmap.quartetlh in the reference's format: "SeqIDs lh1 lh2 lh3 weight1 weight2 weight3"
// tab-separated, ids 1-based as (a,b,c,d).  4-state data; refused for mixtures, +ASC and with -q / -spp.  No cluster file,
// no SVG / EPS plot.
// There is no CPU path: without a GPU it fails with the engine's error.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <fstream>
#include <random>
#include <sstream>
#include <string>
#include <vector>

#include "../iq-tree_amd/host/alignment_host.h"
#include "../iq-tree_amd/host/model_host.h"
#include "../iq-tree_amd/host/model_opt_host.h"
#include "../iq-tree_amd/host/phylo_host.h"
#include "../iq-tree_amd/host/supertree_host.h"
#include "../iq-tree_amd/host/tree_search_host.h"

using namespace iqhost;

// the "+R<k>" / "+R<k>{...}" component of a model string: [begin, end) without the '+', and k (0: none given = 4);
// false when the string has none
static bool findFreeRate(const std::string &m, size_t &begin, size_t &end, int &k, bool &bare) {
    size_t pos = m.find('+');
    while (pos != std::string::npos) {
        size_t stop = pos + 1;
        int depth = 0;
        while (stop < m.size() && (m[stop] != '+' || depth > 0)) {
            if (m[stop] == '{') depth++;
            if (m[stop] == '}') depth--;
            stop++;
        }
        const std::string tok = m.substr(pos + 1, stop - pos - 1);
        if (!tok.empty() && (tok[0] == 'R' || tok[0] == 'r')) {
            size_t i = 1;
            int n = 0;
            while (i < tok.size() && isdigit((unsigned char)tok[i])) n = 10 * n + (tok[i++] - '0');
            if (i == tok.size() || tok[i] == '{') {
                begin = pos + 1;
                end = stop;
                k = n == 0 ? 4 : n;
                bare = i == tok.size();
                return true;
            }
        }
        pos = stop < m.size() ? stop : std::string::npos;
    }
    return false;
}

static std::string freeRateToken(const std::vector<double> &props, const std::vector<double> &rates) {
    std::string t = "R" + std::to_string(props.size()) + "{";
    char buf[64];
    for (size_t c = 0; c < props.size(); c++) {
        snprintf(buf, sizeof buf, "%s%.17g,%.17g", c ? "," : "", props[c], rates[c]);
        t += buf;
    }
    return t + "}";
}

// "MIX{...}" at the head of a model string rewritten with the given class rates and weights as :rate:weight fields
static std::string mixtureString(const std::string &m, const std::vector<double> &rates, const std::vector<double> &weights) {
    size_t close = 4;
    int depth = 1;
    while (close < m.size() && depth > 0) {
        if (m[close] == '{') depth++;
        if (m[close] == '}') depth--;
        close++;
    }
    std::string out = m.substr(0, 4);
    size_t start = 4, cls = 0;
    depth = 0;
    for (size_t i = 4; i < close; i++) {
        if (m[i] == '{') depth++;
        const bool last = i + 1 == close;
        if (m[i] == '}' && !last) depth--;
        if ((m[i] == ',' && depth == 0) || last) {
            std::string item = m.substr(start, i - start);
            int d = 0;
            for (size_t k = 0; k < item.size(); k++) {
                if (item[k] == '{') d++;
                if (item[k] == '}') d--;
                if (item[k] == ':' && d == 0) {
                    item.resize(k);
                    break;
                }
            }
            char buf[80];
            snprintf(buf, sizeof buf, ":%.17g:%.17g", rates[cls], weights[cls]);
            out += (cls ? "," : "") + item + buf;
            cls++;
            start = i + 1;
        }
    }
    return out + "}" + m.substr(close);
}

// the Newick strings of a tree set file, one after the other
static std::vector<std::string> readTreeSet(const std::string &file) {
    std::ifstream zin(file.c_str());
    if (!zin) throw std::runtime_error("cannot open tree set file " + file);
    std::stringstream zss;
    zss << zin.rdbuf();
    std::vector<std::string> newicks;
    std::string cur;
    for (char c : zss.str()) {
        cur += c;
        if (c == ';') {
            if (cur.find('(') != std::string::npos) newicks.push_back(cur);
            cur.clear();
        }
    }
    return newicks;
}

static void writeText(const std::string &file, const std::string &text) {
    std::ofstream out(file.c_str());
    if (!out) throw std::runtime_error("cannot write " + file);
    out << text;
}

// the distance matrix in the reference's .mldist format (alignment.cpp:2586-2606)
static void writeMldist(const std::string &file, const std::vector<std::string> &names, const std::vector<double> &dist,
                        double min_branch_length) {
    const int nseq = (int)names.size();
    size_t max_len = 10;
    for (int i = 0; i < nseq; i++) max_len = std::max(max_len, names[i].size());
    std::ofstream out(file.c_str());
    if (!out) throw std::runtime_error("cannot write " + file);
    out << nseq << std::endl;
    out.precision(std::max((int)ceil(-log10(min_branch_length)) + 1, 6));   // alignment.cpp:2592
    out << std::fixed;
    for (int i = 0; i < nseq; i++) {
        out.width((std::streamsize)max_len);
        out << std::left << names[i] << " ";
        for (int j = 0; j < nseq; j++) out << dist[(size_t)i * nseq + j] << " ";
        out << std::endl;
    }
}

// ... and the matrix as the file holds it
static void readMldist(const std::string &file, const std::vector<std::string> &names, std::vector<double> &dist) {
    const int nseq = (int)names.size();
    dist.assign((size_t)nseq * nseq, 0.0);
    std::ifstream in(file.c_str());
    int n_in = 0;
    if (!(in >> n_in) || n_in != nseq) throw std::runtime_error("cannot read " + file);
    std::string name;
    for (int i = 0; i < nseq; i++) {
        if (!(in >> name) || name != names[i]) throw std::runtime_error("unexpected sequence name in " + file);
        for (int j = 0; j < nseq; j++)
            if (!(in >> dist[(size_t)i * nseq + j])) throw std::runtime_error("cannot read " + file);
    }
}

// a topology string of taxon ids with the ids replaced by the sequence names
static std::string namedTopology(const std::string &ids, const std::vector<std::string> &names) {
    std::string out;
    for (size_t i = 0; i < ids.size();) {
        if (isdigit((unsigned char)ids[i])) {
            size_t j = i;
            while (j < ids.size() && isdigit((unsigned char)ids[j])) j++;
            out += names.at((size_t)atoi(ids.substr(i, j - i).c_str()));
            i = j;
        } else
            out += ids[i++];
    }
    return out;
}

// what -search / -t hands to the NNI tree search
struct SearchOptions {
    bool on = false, nni5 = true, allnni = false, n_given = false;
    long long n_iter = -1;
    int numstop = 100, popsize = 5;
    double pers = 0.5;
    unsigned long long seed = 1;
};

// -q / -spp: the edge-linked partition model on a fixed topology, or with -search / -t the NNI tree search on the super tree
// between two optimizeParameters (rates with -spp, and lengths); the partition rates and models are taken as given inside
// the search loop
// With -bionjtree and no -te / -t the starting tree is built as the plain path builds it (PhyloSuperTreePlen::computeDist,
// computeBioNJ, fixNegativeBranch): from a star tree, all rates 1 and the models as the partition file gives them, the joint
// ML distance of every pair is written to mldist_file and read back, the BIONJ tree of that text goes to <prefix>.bionj,
// fixNegativeBranch(false) replaces the negative lengths, and the run goes on as -te <prefix>.bionj does
static int runPartitionModel(const std::string &aln_file, const std::string &part_file, const std::string &tree_file,
                             const std::string &prefix, bool proportional, bool blfix, int dev, const SearchOptions &so,
                             bool bionjtree, const std::string &mldist_file) {
    std::vector<std::string> names;
    std::vector<PartitionInput> parts;
    readPartitionRaxml(aln_file, part_file, names, parts);
    std::stringstream tss;
    if (bionjtree) {   // a star of all taxa: only the taxa matter until the tree is built
        tss << "(";
        for (size_t i = 0; i < names.size(); i++) tss << (i ? "," : "") << names[i] << ":0.1";
        tss << ");";
    } else {
        std::ifstream tin(tree_file.c_str());
        if (!tin) throw std::runtime_error("cannot open tree file " + tree_file);
        tss << tin.rdbuf();
    }
    PhyloSuperTree tree;
    tree.readTreeString(tss.str(), names);
    if (tree.super.leafNum != (int)names.size()) throw std::runtime_error("Tree and alignment have different numbers of taxa");
    for (const PartitionInput &in : parts) tree.addPartition(in);
    tree.fixed_rates = !proportional;
    if (so.on) tree.setAllBranchMode();   // the batched NNI evaluation needs every directed vector
    tree.attachEngines(dev);
    printf("Edge-linked partition model with %d partitions (%s)\n", tree.size(), proportional ? "-spp" : "-q");
    if (bionjtree) {
        const int nseq = (int)names.size();
        std::vector<double> dist((size_t)nseq * nseq);
        auto t0 = std::chrono::steady_clock::now();
        tree.computeDist(dist.data(), nullptr);
        double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        writeMldist(mldist_file, names, dist, tree.min_branch_length);
        printf("ML distances of %d pairs: %.4f s, printed to %s\n", nseq * (nseq - 1) / 2, sec, mldist_file.c_str());
        readMldist(mldist_file, names, dist);   // the tree is a function of the file, as in the reference
        t0 = std::chrono::steady_clock::now();
        std::string nwk;
        tree.computeBioNJ(dist.data(), nullptr, &nwk);
        sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        writeText(prefix + ".bionj", nwk + "\n");
        printf("BIONJ tree: %.4f s, printed to %s.bionj\n", sec, prefix.c_str());
        const int fixed = tree.fixNegativeBranch(false);   // phyloanalysis.cpp:1832-1837
        printf("%d negative branch lengths fixed\n", fixed);
        tree.readTreeString(tree.getTreeString(), names);   // from here on what -te does with a tree file
        printf("Log-likelihood of the input tree: %.17g\n", tree.computeLikelihood());
    }
    tree.optimizeParameters(blfix, 0.001, 0.001);   // params.modeps defaults
    if (so.on) {
        TreeSearch ts(&tree);
        ts.nni5 = so.nni5;
        ts.speednni = !so.allnni;
        ts.popSize = so.popsize;
        ts.initPS = so.pers;
        ts.seed = so.seed;
        ts.stop_rule.unsuccess_iteration = so.numstop;
        ts.stop_rule.stop_condition = so.n_given ? iqsearch::SC_FIXED_ITERATION : iqsearch::SC_UNSUCCESS_ITERATION;
        ts.stop_rule.min_iteration = (int)so.n_iter;
        ts.on_iteration = [&](const TreeSearch &, const TreeSearch::Iteration &it) {
            if (it.iteration % 10 == 0) printf("Iteration %d / LogL: %.4f\n", it.iteration, it.score);
            if (it.new_best && it.iteration > 1) printf("BETTER TREE FOUND at iteration %d: %.4f\n", it.iteration, it.score);
        };
        auto t0 = std::chrono::steady_clock::now();
        ts.doTreeSearch();
        const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        printf("Tree search: %d iterations, %d candidate trees, %ld batches of joint solves: %.4f s\n", ts.stop_rule.cur_iteration,
               (int)ts.candidates.size(), tree.num_group_batches, sec);
        tree.optimizeParameters(blfix, 0.001, 0.001);
    }
    const double total = tree.computeLikelihood();
    if (proportional) {   // PartitionModelPlen::writeInfo
        std::ostringstream os;
        os << "Partition-specific rates: ";
        for (double r : tree.part_rate) os << " " << r;
        printf("%s\n", os.str().c_str());
    }
    for (int p = 0; p < tree.size(); p++)
        printf("Partition %s: %d sites, %d patterns, lnL %.6f\n", tree.part_name[(size_t)p].c_str(), parts[(size_t)p].aln.getNSite(),
               parts[(size_t)p].aln.getNPattern(), tree.cur_score[(size_t)p]);
    printf("Optimal log-likelihood: %.6f\n", total);
    writeText(prefix + ".treefile", tree.getTreeString() + "\n");
    std::ostringstream rep;
    rep.precision(17);
    rep << "lnL " << total << "\n";
    for (int p = 0; p < tree.size(); p++)
        rep << "partition " << tree.part_name[(size_t)p] << " rate " << tree.part_rate[(size_t)p] << " lnL " << tree.cur_score[(size_t)p] << "\n";
    writeText(prefix + ".iqhip", rep.str());
    return 0;
}

static void usage() {
    fprintf(stderr,
            "usage: iqhip_lnl -s <alignment> -te <newick file> -m <model> [-st DNA|AA|CODON[n]] [-pre <prefix>]\n"
            "                 [-blfix] [-wsl] [-dev <gpu>] [-reps <n>] [-nolhmemsave] [-alrt <n>] [-lbp <n>] [-seed <s>]\n"
            "                 [-z <tree set file> -zb <n> [-zw] [-au]] [-mldist <file>] [-pars [-sprrad <r>]] [-emrates] [-wsr]\n"
            "                 [-lmap <n quartets, 0 = all> [-wql]]\n"
            "                 [-mixweights] [-optmodel] [-bb <n> [-beps <e>] [-z <tree set file>] [-wbt]]\n"
            "                 [-search | -t <newick file>] [-n <iterations>] [-numstop <n>] [-pers <p>] [-popsize <k>] [-nni1|-nni5] [-allnni]\n"
            "                 (NNI tree search from the starting tree; with -bb <n>: [-bcor <c>] [-nstep <s>] [-nm <max iterations>])\n"
            "                 [-numpars <n> [-toppars <m>] [-sprrad <r>]]   (with -search: n starting trees, n - 1 of them parsimony trees,\n"
            "                  the best m optimised by NNI before the search loop)\n"
            "       iqhip_lnl -s <alignment> -parstree [-sprrad <r>] -m <model> [-seed <s>] ...   (parsimony starting tree instead of -te)\n"
            "       iqhip_lnl -s <alignment> -bionjtree -m <model> ...              (BIONJ starting tree instead of -te)\n"
            "       iqhip_lnl -s <alignment> -q|-spp <partition file> -te <newick file> | -bionjtree [-mldist <file>]\n"
            "                 [-blfix] [-pre <prefix>] [-dev <gpu>]\n"
            "                 [-search | -t <newick file>] [-n <iterations>] [-numstop <n>] [-pers <p>] [-popsize <k>] [-nni1] [-allnni]\n"
            "                 (edge-linked partition model instead of -m; lines 'MODEL, name = 1-100, 250-400, 401-500\\3';\n"
            "                  -q: all partition rates 1, -spp: rates estimated)\n"
            "  model: e.g. 'GTR{1.5,2.4,1.8,1.9,2.8}+F{0.25,0.26,0.25,0.24}+I{0.1}+G4{0.9}', 'HKY{2}+G4{0.5}', JC,\n"
            "         POISSON+G4{1}, <paml matrix file>+G4{0.9}, 'GY{kappa,omega}+F1X4', any of them +ASC;\n"
            "         +R3{w1,r1,w2,r2,w3,r3}, or with -emrates (weights and rates estimated by EM) also a bare +R3;\n"
            "         with -optmodel (parameters estimated) also GTR+I+G4, HKY+G4{0.7}, <paml matrix file>+I+G4: braces are starting values;\n"
            "         'MIX{JC,HKY{2.0}:1.5,GTR{..}+F{..}:0.5:0.2}+G4{0.8}' (class[:rate[:weight]]); -mixweights estimates the weights by EM\n");
}

int main(int argc, char **argv) {
    std::string aln_file, tree_file, model_str, seq_type, prefix;
    bool blfix = false, wsl = false, all_branch = false;
    int dev = 0, reps = 0, alrt = 0, lbp = 0;
    unsigned long long seed = 1;
    std::string treeset_file, mldist_file, part_file;
    bool part_proportional = false;
    long long lmap = -1;   // -lmap <n>: likelihood mapping over n drawn quartets (0: all unique quartets)
    bool wql = false;
    int zb = 0, sprrad = 0, bb = 0;
    double beps = 0.5;
    bool wbt = false;
    bool search = false, nni5 = true, allnni = false;   // -search: the NNI tree search from the starting tree
    long long n_iter = -1;
    bool n_given = false;
    int numstop = 100, popsize = 5, nstep = 100, nm = 1000;
    int numpars = 0, toppars = 20;   // -numpars / -toppars: the starting population of the search (0: the one tree)
    double pers = 0.5, bcor = 0.99;
    bool zw = false, au = false, parstree = false, pars = false, bionjtree = false, emrates = false, wsr = false, mixweights = false, optmodel = false;
    for (int i = 1; i < argc; i++) {
        std::string a = argv[i];
        auto next = [&]() -> std::string {
            if (i + 1 >= argc) { usage(); exit(2); }
            return argv[++i];
        };
        if (a == "-s") aln_file = next();
        else if (a == "-te") tree_file = next();
        else if (a == "-m") model_str = next();
        else if (a == "-st") seq_type = next();
        else if (a == "-pre") prefix = next();
        else if (a == "-blfix") blfix = true;
        else if (a == "-wsl") wsl = true;
        else if (a == "-nolhmemsave") all_branch = true;
        else if (a == "-dev") dev = atoi(next().c_str());
        else if (a == "-reps") reps = atoi(next().c_str());
        else if (a == "-alrt") alrt = atoi(next().c_str());
        else if (a == "-lbp") lbp = atoi(next().c_str());
        else if (a == "-z") treeset_file = next();
        else if (a == "-zb") zb = atoi(next().c_str());
        else if (a == "-bb") bb = atoi(next().c_str());
        else if (a == "-beps") beps = atof(next().c_str());
        else if (a == "-wbt") wbt = true;
        else if (a == "-zw") zw = true;
        else if (a == "-au") au = true;
        else if (a == "-mldist") mldist_file = next();
        else if (a == "-parstree") parstree = true;
        else if (a == "-pars") pars = true;
        else if (a == "-bionjtree") bionjtree = true;
        else if (a == "-emrates") emrates = true;
        else if (a == "-wsr") wsr = true;
        else if (a == "-mixweights") mixweights = true;
        else if (a == "-optmodel") optmodel = true;
        else if (a == "-lmap") {
            lmap = atoll(next().c_str());
            if (lmap < 0) { usage(); return 2; }
        }
        else if (a == "-wql") wql = true;
        else if (a == "-q" || a == "-spp") {
            if (!part_file.empty()) { usage(); return 2; }
            part_file = next();
            part_proportional = a == "-spp";
        }
        else if (a == "-sprrad") {
            sprrad = atoi(next().c_str());
            if (sprrad < 1 || sprrad > IQHIP_PARS_SPR_MAX_RADIUS) { usage(); return 2; }
        }
        else if (a == "-seed") seed = strtoull(next().c_str(), nullptr, 10);
        else if (a == "-n") {   // with -search / -t: a fixed number of search iterations; else accepted for compatibility (-n 0)
            char *end = nullptr;
            const std::string v = next();
            n_iter = strtoll(v.c_str(), &end, 10);
            n_given = true;
            if (v.empty() || *end || n_iter < 0) {
                fprintf(stderr, "error: -n needs a non-negative number of iterations\n");
                return 2;
            }
        }
        else if (a == "-search") search = true;
        else if (a == "-t") { tree_file = next(); search = true; }
        else if (a == "-numstop") numstop = atoi(next().c_str());
        else if (a == "-numpars" || a == "-toppars") {
            char *end = nullptr;
            const std::string v = next();
            const long long k = strtoll(v.c_str(), &end, 10);
            if (v.empty() || *end || k < 1 || k > 1000000) {
                fprintf(stderr, "error: %s needs a positive number of trees\n", a.c_str());
                return 2;
            }
            (a == "-numpars" ? numpars : toppars) = (int)k;
        }
        else if (a == "-pers") pers = atof(next().c_str());
        else if (a == "-popsize") popsize = atoi(next().c_str());
        else if (a == "-nni1") nni5 = false;
        else if (a == "-nni5") nni5 = true;
        else if (a == "-allnni") allnni = true;
        else if (a == "-bcor") bcor = atof(next().c_str());
        else if (a == "-nstep") nstep = atoi(next().c_str());
        else if (a == "-nm") nm = atoi(next().c_str());
        else { usage(); return 2; }
    }
    if (search && model_str.empty() && part_file.empty()) {
        fprintf(stderr, "error: -search / -t needs a model (-m): the search takes the model as given\n");
        return 2;
    }
    if (!part_file.empty()) {
        const char *with = numpars > 0 ? "-numpars" : !model_str.empty() ? "-m" : alrt > 0 || lbp > 0 ? "-alrt / -lbp" : !treeset_file.empty() || zb > 0 ? "-z" : bb > 0 ? "-bb"
                           : !mldist_file.empty() && !tree_file.empty() ? "-mldist and a tree (-te / -t): the distances belong to -bionjtree"
                           : pars || parstree || sprrad > 0 ? "-pars / -parstree / -sprrad"
                           : bionjtree && !tree_file.empty() ? "-bionjtree and a tree (-te / -t)" : emrates ? "-emrates" : mixweights ? "-mixweights" : optmodel ? "-optmodel" : lmap >= 0 ? "-lmap" : nullptr;
        if (with) {
            fprintf(stderr, "error: -q / -spp cannot be combined with %s (the models come from the partition file; the tree comes from -te / -t or from -bionjtree)\n", with);
            return 2;
        }
        if (aln_file.empty() || (tree_file.empty() && !bionjtree)) { usage(); return 2; }
        if (prefix.empty()) prefix = part_file;
        if (bionjtree && mldist_file.empty()) mldist_file = prefix + ".mldist";
        try {
            SearchOptions so;
            so.on = search; so.nni5 = nni5; so.allnni = allnni; so.n_given = n_given; so.n_iter = n_iter;
            so.numstop = numstop; so.popsize = popsize; so.pers = pers; so.seed = seed;
            return runPartitionModel(aln_file, part_file, tree_file, prefix, part_proportional, blfix, dev, so, bionjtree, mldist_file);
        } catch (const std::exception &ex) {
            fprintf(stderr, "error: %s\n", ex.what());
            return 1;
        }
    }
    if (aln_file.empty() || model_str.empty() || (int)!tree_file.empty() + (int)parstree + (int)bionjtree != 1) { usage(); return 2; }
    if (prefix.empty()) prefix = aln_file;
    if (bionjtree && mldist_file.empty()) mldist_file = prefix + ".mldist";
    if (alrt < 0 || lbp < 0) { usage(); return 2; }
    if (sprrad > 0 && !parstree && !pars && numpars == 0) { usage(); return 2; }
    if (numpars > 0 && !search) { usage(); return 2; }   // the starting population belongs to the search
    if (numpars > 0 && numpars < toppars) toppars = numpars;
    if (bb < 0 || !(beps >= 0.0) || (bb == 0 && wbt)) { usage(); return 2; }
    if (zb < 0 || (!treeset_file.empty() && zb < 1 && bb == 0) || (treeset_file.empty() && (zb > 0 || zw || au))) { usage(); return 2; }
    if (wql && lmap < 0) { usage(); return 2; }
    if (search) {
        if (numstop < 1 || popsize < 1 || !(pers >= 0.0 && pers <= 1.0) || nstep < 2 || nstep % 2 || nm < 1 || !(bcor >= 0.0 && bcor <= 1.0)) {
            fprintf(stderr, "error: -numstop, -popsize, -nm need positive numbers, -pers and -bcor values in [0, 1], -nstep an even number >= 2\n");
            return 2;
        }
        if (bb > 0 && !treeset_file.empty() && zb == 0) {
            fprintf(stderr, "error: with -search the bootstrap is fed by the search, not by -z\n");
            return 2;
        }
    }
    if (alrt > 0 || lbp > 0 || bb > 0 || search) all_branch = true;  // the batched NNI evaluation needs every directed vector
    try {
        Alignment aln;
        aln.readFile(aln_file, seq_type);
        printf("Alignment has %d sequences with %d columns and %d patterns\n", aln.getNSeq(), aln.getNSite(), aln.getNPattern());
        if (emrates) {
            size_t r0, r1;
            int k;
            bool bare;
            if (!findFreeRate(model_str, r0, r1, k, bare)) throw std::runtime_error("-emrates needs a +R<k> model");
            if (bare) {   // RateFree::setNCategory's starting point stands in for the missing values
                std::vector<double> p0, rt0;
                PhyloTree::freeRateStart(k, p0, rt0);
                model_str = model_str.substr(0, r0) + freeRateToken(p0, rt0) + model_str.substr(r1);
            }
        }
        ModelSpec spec = parseModelString(model_str, optmodel);
        if (optmodel) {
            if (emrates || mixweights) throw std::runtime_error("-optmodel excludes -emrates and -mixweights");
            ModelOptimizer::checkScope(spec);
            ModelOptimizer::startingValues(spec, aln);
        }
        ModelInputs mi;
        buildModel(spec, aln, mi);  // frequencies from the observed patterns only
        const int nsite = aln.getNSite();
        const bool mixture = mi.nclass > 1;
        if (mixweights && !mixture) throw std::runtime_error("-mixweights needs a MIX{...} model");
        // (the reference's setPInvar also replaces the category rates: 1 / (1 - p) for +I alone, the Gamma rates over 1 - p with
        // +G; the re-send of weights and ptn_invar does not restate that)
        if (mixweights && spec.p_invar > 0.0)
            throw std::runtime_error("-mixweights: +I is not supported (the category rates would follow p_invar)");
        if (mixture && (emrates || wsr)) throw std::runtime_error("-emrates and -wsr are not available for mixture models");
        if (mixture && spec.ascertainment) throw std::runtime_error("Mixture model +ASC is not supported yet");
        if (mixture && !mldist_file.empty()) throw std::runtime_error("-mldist and -bionjtree are not available for mixture models");
        if (lmap >= 0 && (mixture || spec.ascertainment)) throw std::runtime_error("-lmap is not available for mixture models and +ASC");
        if (lmap >= 0 && aln.num_states != 4) throw std::runtime_error("-lmap: 4-state data only");
        if (spec.ascertainment) {
            const int k = aln.appendUnobservedConstPatterns();
            printf("Ascertainment bias correction: %d unobservable constant patterns\n", k);
        }
        std::stringstream tss;
        if (parstree || bionjtree) {   // a star of all taxa: only the taxa matter until the tree is built
            tss << "(";
            for (int i = 0; i < aln.getNSeq(); i++) tss << (i ? "," : "") << aln.seq_names[i] << ":0.1";
            tss << ");";
        } else {
            std::ifstream tin(tree_file.c_str());
            if (!tin) throw std::runtime_error("cannot open tree file " + tree_file);
            tss << tin.rdbuf();
        }

        PhyloTree tree;
        tree.readTreeString(tss.str(), aln.seq_names);
        if (tree.leafNum != aln.getNSeq()) throw std::runtime_error("Tree and alignment have different numbers of taxa");
        std::vector<uint8_t> states;
        std::vector<double> freq, invar;
        aln.statesByLeaf(states);
        aln.ptnFreq(freq);
        aln.ptnInvar(mi.p_invar, mi.state_freq.data(), invar);
        tree.setAlignment(aln.num_states, aln.seq_type, aln.getNPattern(), states.data(), freq.data(), invar.data());
        if (spec.ascertainment) tree.setAscertainment(aln.n_unobserved, (double)nsite);
        if (mixture)
            tree.setMixtureModel(mi.nclass, mi.ncat, mi.cat_class.data(), mi.eig.eval.data(), mi.eig.evec.data(),
                                 mi.eig.inv_evec.data(), mi.rates.data(), mi.props.data());
        else
            tree.setModel(mi.ncat, mi.eig.eval.data(), mi.eig.evec.data(), mi.eig.inv_evec.data(), mi.rates.data(), mi.props.data());
        tree.lh_mem_save = all_branch ? LM_ALL_BRANCH : LM_PER_NODE;
        tree.setLikelihoodKernel(LK_EIGEN_HIP);
        tree.attachEngine(dev);
        if (parstree) {
            std::vector<int> order((size_t)aln.getNSeq());
            for (size_t i = 0; i < order.size(); i++) order[i] = (int)i;
            std::mt19937_64 gen(seed);
            for (size_t i = order.size(); i > 1; i--) std::swap(order[i - 1], order[(size_t)(gen() % i)]);
            auto t0 = std::chrono::steady_clock::now();
            const int score = tree.computeParsimonyTree(order.data());
            const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            printf("Parsimony score: %d (based on %lld informative sites)\n", score, (long long)tree.pars_nsites);
            if (sprrad > 0) {   // the SPR rounds that follow the additions in the reference's default starting tree
                std::vector<PhyloTree::SprRound> rounds;
                const int improved = tree.optimizeParsimonySPR(sprrad, -1, &rounds);
                tree.fixNegativeBranch(true);
                printf("Parsimony score after SPR: %d (%d rounds)\n", improved, (int)rounds.size());
            }
            const std::string nwk = tree.getTreeString();
            std::ofstream out((prefix + ".parstree").c_str());
            if (!out) throw std::runtime_error("cannot write " + prefix + ".parstree");
            out << nwk << std::endl;
            printf("Parsimony tree: %.4f s, printed to %s.parstree\n", sec, prefix.c_str());
            tree.readTreeString(nwk, aln.seq_names);   // from here on exactly what -te <prefix>.parstree does
        } else if (pars) {
            const int score = tree.computeParsimony();
            printf("Parsimony score: %d (based on %lld informative sites)\n", score, (long long)tree.pars_nsites);
            if (sprrad > 0) {   // improve the given tree; its branch lengths are merged / split where a move cuts
                std::vector<PhyloTree::SprRound> rounds;
                const int improved = tree.optimizeParsimonySPR(sprrad, -1, &rounds);
                printf("Parsimony score after SPR: %d (%d rounds)\n", improved, (int)rounds.size());
                const std::string nwk = tree.getTreeString();
                std::ofstream out((prefix + ".parstree").c_str());
                if (!out) throw std::runtime_error("cannot write " + prefix + ".parstree");
                out << nwk << std::endl;
                printf("Improved tree printed to %s.parstree\n", prefix.c_str());
                tree.readTreeString(nwk, aln.seq_names);
            }
        }
        if (!mldist_file.empty()) {
            const int nseq = aln.getNSeq();
            std::vector<double> dist((size_t)nseq * nseq), d2l((size_t)nseq * nseq);
            auto t0 = std::chrono::steady_clock::now();
            tree.computeDist(nullptr, dist.data(), d2l.data());
            const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            writeMldist(mldist_file, aln.seq_names, dist, tree.min_branch_length);
            printf("ML distances of %d pairs: %.4f s, printed to %s\n", nseq * (nseq - 1) / 2, sec, mldist_file.c_str());
        }
        if (bionjtree) {
            std::vector<double> dist;
            readMldist(mldist_file, aln.seq_names, dist);   // the matrix as the file holds it
            auto t0 = std::chrono::steady_clock::now();
            std::string nwk;
            tree.computeBioNJ(dist.data(), nullptr, &nwk);
            const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            std::ofstream out((prefix + ".bionj").c_str());
            if (!out) throw std::runtime_error("cannot write " + prefix + ".bionj");
            out << nwk << std::endl;
            printf("BIONJ tree: %.4f s, printed to %s.bionj\n", sec, prefix.c_str());
            const int fixed = tree.fixNegativeBranch(false);   // phyloanalysis.cpp:1832-1837
            printf("%d negative branch lengths fixed\n", fixed);
            tree.readTreeString(tree.getTreeString(), aln.seq_names);   // from here on what -te does with a tree file
        }
        tree.initializeAllPartialLh();
        tree.clearAllPartialLH();
        std::vector<double> pattern_lh(aln.getNPattern());
        double lnl = tree.computeLikelihood(pattern_lh.data());
        printf("Log-likelihood of the input tree: %.17g\n", lnl);
        const double lnl_input = lnl;
        if (emrates) {
            if (spec.p_invar > 0.0) throw std::runtime_error("-emrates: +I+R is not supported");
            const double logl_epsilon = 0.01;   // params.modeps (tools.cpp)
            int em_steps = 0, em_rounds = 0;
            ModelOptimizer::parameterLoop(tree, blfix, logl_epsilon, lnl, [&]() {
                std::vector<PhyloTree::EmStep> steps;
                const double new_lh = tree.optimizeFreeRatesEM(&steps);
                em_steps += (int)steps.size();
                for (const PhyloTree::EmStep &st : steps) em_rounds += st.rounds;
                return new_lh;
            }, true);
            // rescaleRates, then branch lengths in substitutions per site (modelfactory.cpp:1035-1040)
            std::vector<double> props = tree.getProps(), rates = tree.getRates();
            double mean_rate = 0.0;
            for (size_t c = 0; c < rates.size(); c++) mean_rate += props[c] * rates[c];
            for (double &r : rates) r /= mean_rate;
            tree.setRateCategories(rates.data(), props.data());
            if (mean_rate != 1.0) tree.scaleLength(mean_rate);
            tree.clearAllPartialLH();
            lnl = tree.computeLikelihood(pattern_lh.data());
            mi.rates = rates;
            mi.props = props;
            size_t r0, r1;
            int k;
            bool bare;
            findFreeRate(model_str, r0, r1, k, bare);
            model_str = model_str.substr(0, r0) + freeRateToken(props, rates) + model_str.substr(r1);
            printf("EM: %d steps, %d lockstep rounds\n", em_steps, em_rounds);
            printf("Site proportion and rates: ");
            for (size_t c = 0; c < rates.size(); c++) printf(" (%g,%g)", props[c], rates[c]);
            printf("\nModel with estimated rates: %s\n", model_str.c_str());
            printf("Optimal log-likelihood: %.17g\n", lnl);
        } else if (mixweights) {
            // the loop of ModelFactory::optimizeParameters with the substitution models fixed, as for -emrates
            const double logl_epsilon = 0.01;   // params.modeps
            int em_steps = 0;
            ModelOptimizer::parameterLoop(tree, blfix, logl_epsilon, lnl, [&]() {
                int steps = 0;
                const double new_lh = tree.optimizeMixtureWeights(nullptr, &steps);
                em_steps += steps;
                return new_lh;
            }, true);
            // The class rates were normalised with the weights the run started from.  As the reference does when it writes the
            // model (modelmixture.cpp:1552-1563) and as -emrates does for +R: rates over their new mean, all branch lengths
            // times it -- the likelihood is unchanged and the printed string reads back as the model the tree holds
            const std::vector<double> w = tree.getMixtureWeights();
            mi.props = tree.getProps();
            double mean_rate = 0.0;
            for (int m = 0; m < mi.nclass; m++) mean_rate += w[m] * mi.class_rates[m];
            if (mean_rate != 1.0) {
                const size_t n = (size_t)mi.nstates;
                for (int m = 0; m < mi.nclass; m++) {
                    mi.class_rates[m] /= mean_rate;
                    for (size_t i = 0; i < n; i++) mi.eig.eval[(size_t)m * n + i] /= mean_rate;
                }
                tree.setMixtureModel(mi.nclass, mi.ncat, mi.cat_class.data(), mi.eig.eval.data(), mi.eig.evec.data(),
                                     mi.eig.inv_evec.data(), mi.rates.data(), mi.props.data());
                tree.scaleLength(mean_rate);
            }
            tree.clearAllPartialLH();
            lnl = tree.computeLikelihood(pattern_lh.data());
            model_str = mixtureString(model_str, mi.class_rates, w);
            printf("EM: %d steps\n", em_steps);
            printf("Mixture weights:");
            for (double x : w) printf(" %g", x);
            printf("\nModel with estimated weights: %s\n", model_str.c_str());
            printf("Optimal log-likelihood: %.17g\n", lnl);
        } else if (optmodel) {
            ModelOptimizer opt(tree, aln, spec, true);
            opt.optimizeParameters(blfix, DEFAULT_LOGL_EPSILON, DEFAULT_GRADIENT_EPSILON, true);
            tree.clearAllPartialLH();
            lnl = tree.computeLikelihood(pattern_lh.data());
            mi = opt.getInputs();
            model_str = opt.modelString();
            int stencils = 0, stencil_trav = 0, single_trav = 0, redone = 0;
            for (const ModelOptimizer::Call &c : opt.trace) {
                stencils += c.stencils;
                stencil_trav += c.stencil_traversals;
                single_trav += c.single_traversals;
                redone += c.stencils_redone;
            }
            printf("Parameters optimization took %d rounds: %d stencils in %d batched traversals (%d redone), %d single traversals\n",
                   opt.rounds, stencils, stencil_trav, redone, single_trav);
            printf("%s", opt.writeInfo().c_str());
            printf("Model with estimated parameters: %s\n", model_str.c_str());
            printf("Optimal log-likelihood: %.17g\n", lnl);
        } else if (!blfix) {
            lnl = tree.optimizeAllBranches();
            printf("Log-likelihood after branch-length optimisation: %.17g\n", lnl);
            tree.clearAllPartialLH();
            lnl = tree.computeLikelihood(pattern_lh.data());
        }
        if (search) {   // IQTree::doTreeSearch from the tree and the model as they stand now
            if (bb > 0 && (mixture || spec.ascertainment)) throw std::runtime_error("-bb is not available for mixture models and +ASC");
            TreeSearch ts(&tree);
            ts.nni5 = nni5;
            ts.speednni = !allnni;
            ts.popSize = popsize;
            ts.initPS = pers;
            ts.seed = seed;
            ts.stop_rule.unsuccess_iteration = numstop;
            ts.stop_rule.stop_condition = n_given ? iqsearch::SC_FIXED_ITERATION : iqsearch::SC_UNSUCCESS_ITERATION;
            ts.stop_rule.min_iteration = (int)n_iter;
            if (bb > 0) {   // every tree the search evaluates feeds the bootstrap; the correlation rule ends the search
                tree.genBootSamples(bb, nsite, seed, 0xA0u);
                tree.initUFBoot(bb, seed);
                tree.ufboot_epsilon = beps;
                ts.stop_rule.stop_condition = iqsearch::SC_BOOTSTRAP_CORRELATION;
                ts.stop_rule.min_correlation = bcor;
                ts.stop_rule.max_iteration = n_given ? std::min((int)n_iter, nm) : nm;
                ts.step_iterations = nstep;
            }
            ts.on_iteration = [&](const TreeSearch &s, const TreeSearch::Iteration &it) {
                if (it.iteration % 10 == 0) printf("Iteration %d / LogL: %.4f\n", it.iteration, it.score);
                if (it.new_best && it.iteration > 1) printf("BETTER TREE FOUND at iteration %d: %.4f\n", it.iteration, it.score);
                if (!s.correlation_log.empty() && s.correlation_log.back().first == it.iteration) {
                    printf("Log-likelihood cutoff on original alignment: %.6f\n", tree.ufboot_logl_cutoff);
                    printf("NOTE: Bootstrap correlation coefficient of split occurrence frequencies: %g\n", s.correlation_log.back().second);
                }
            };
            if (numpars > 0) {
                ts.numInitTrees = numpars;
                ts.numNNITrees = toppars;
                ts.initSprRadius = sprrad;
                ts.on_init_phase = [&](const TreeSearch &, int phase, int count) {
                    if (phase == 0) printf("Generating %d parsimony trees... %d distinct starting trees\n", numpars - 1, count);
                    else if (phase == 1) printf("Computing log-likelihood of %d initial trees\n", count);
                    else printf("Optimizing top %d initial trees with NNI...\n", count);
                };
            }
            auto t0 = std::chrono::steady_clock::now();
            const long sub0 = tree.num_submissions;
            ts.doTreeSearch();
            const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            tree.clearAllPartialLH();
            lnl = tree.computeLikelihood(pattern_lh.data());
            printf("Tree search: %d iterations, %d candidate trees, %ld engine submissions: %.4f s\n", ts.stop_rule.cur_iteration,
                   (int)ts.candidates.size(), tree.num_submissions - sub0, sec);
            printf("Optimal log-likelihood: %.17g\n", lnl);
            writeText(prefix + ".treefile", tree.getTreeString() + "\n");
            printf("Best tree printed to %s.treefile\n", prefix.c_str());
        }
        double df = 0.0, ddf = 0.0;
        tree.theta_computed = false;
        tree.computeLikelihoodDerv(tree.current_it, tree.current_it_back->node, df, ddf);
        double upd_per_s = 0.0;
        if (reps > 0) {
            auto t0 = std::chrono::steady_clock::now();
            for (int r = 0; r < reps; r++) {
                tree.clearAllPartialLH();
                lnl = tree.computeLikelihood();
            }
            const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            upd_per_s = (double)reps * (tree.leafNum - 2) * (double)aln.getNPattern() / sec;
            printf("%d traversals in %.4f s: %.1f M pattern-node updates/s\n", reps, sec, upd_per_s / 1e6);
        }
        {
            std::ofstream out((prefix + ".iqhip").c_str());
            char buf[128];
            out << "model " << model_str << "\n";
            out << "nseq " << aln.getNSeq() << " nsite " << nsite << " npattern " << aln.getNPattern() - aln.n_unobserved << "\n";
            snprintf(buf, sizeof buf, "%.17g", lnl_input); out << "lnL_input_tree " << buf << "\n";
            snprintf(buf, sizeof buf, "%.17g", lnl);       out << "lnL " << buf << "\n";
            snprintf(buf, sizeof buf, "%.17g", df);        out << "df " << buf << "\n";
            snprintf(buf, sizeof buf, "%.17g", ddf);       out << "ddf " << buf << "\n";
            out << "rates";
            for (double r : mi.rates) { snprintf(buf, sizeof buf, " %.17g", r); out << buf; }
            out << "\ntree " << tree.getTreeString() << "\n";
        }
        if (lmap >= 0) {   // likelihood mapping (doLikelihoodMapping, quartet.cpp:1340-1505), under the model and not the tree
            const int nseq = aln.getNSeq();
            const long long all = (long long)lmap::numQuartets(nseq);
            const long long nq = (lmap == 0 || lmap >= all) ? all : lmap;
            std::vector<double> const_invar;
            if (mi.p_invar > 0.0) {
                for (int x = 0; x < 4; x++) const_invar.push_back(mi.p_invar * mi.state_freq[(size_t)x]);
                const_invar.push_back(mi.p_invar);
            }
            printf("Computing %lld quartet likelihoods\n", nq);
            PhyloTree::LmapResult r;
            auto t0 = std::chrono::steady_clock::now();
            tree.doLikelihoodMapping(lmap, seed, r, const_invar.empty() ? nullptr : const_invar.data());
            const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            printf("Likelihood mapping of %lld quartets: %.4f s\n", nq, sec);
            for (int k = 0; k < 7; k++) printf("Quartets in region %d: %lld\n", k + 1, (long long)r.areacount[k]);
            const long long resolved = r.areacount[0] + r.areacount[1] + r.areacount[2];
            const long long partly = r.areacount[3] + r.areacount[4] + r.areacount[5];
            const long long unresolved = r.areacount[6], total = resolved + partly + unresolved;
            printf("Number of fully resolved  quartets: %lld (%g%%)\n", resolved, 100.0 * resolved / total);
            printf("Number of partly resolved quartets: %lld (%g%%)\n", partly, 100.0 * partly / total);
            printf("Number of unresolved      quartets: %lld (%g%%)\n", unresolved, 100.0 * unresolved / total);
            if (wql) {   // quartet.cpp:1455-1467: 1-based ids, the stream's default number format
                const std::string name = prefix + ".lmap.quartetlh";
                std::ofstream out(name.c_str());
                if (!out) throw std::runtime_error("cannot write " + name);
                out << "SeqIDs\tlh1\tlh2\tlh3\tweight1\tweight2\tweight3" << std::endl;
                for (const lmap::QuartetInfo &q : r.info)
                    out << "(" << q.seqID[0] + 1 << "," << q.seqID[1] + 1 << "," << q.seqID[2] + 1 << "," << q.seqID[3] + 1 << ")"
                        << "\t" << q.logl[0] << "\t" << q.logl[1] << "\t" << q.logl[2] << "\t" << q.qweight[0] << "\t"
                        << q.qweight[1] << "\t" << q.qweight[2] << std::endl;
                printf("likelihood mapping results written to %s\n", name.c_str());
            }
        }
        if (wsr) {
            tree.clearAllPartialLH();
            tree.computeLikelihood();
            std::vector<double> ptn_rate;
            std::vector<int> ptn_cat;
            tree.computePatternRates(ptn_rate, ptn_cat);
            const std::vector<double> &cat_rate = tree.getRates();
            std::ofstream out((prefix + ".rate").c_str());
            if (!out) throw std::runtime_error("cannot write " + prefix + ".rate");
            out.setf(std::ios::fixed, std::ios::floatfield);
            out.precision(5);
            out << "Site\tRate\tCategory\tCategorized_rate" << std::endl;
            std::vector<int> count(cat_rate.size(), 0);
            for (int i = 0; i < nsite; i++) {
                const int ptn = aln.site_pattern[i];
                out << i + 1 << "\t";
                if (ptn_rate[ptn] >= 100.0) out << "100.0"; else out << ptn_rate[ptn];   // MAX_SITE_RATE
                out << "\t" << ptn_cat[ptn] + 1 << "\t" << cat_rate[ptn_cat[ptn]] << std::endl;
                count[ptn_cat[ptn]]++;
            }
            printf("Empirical proportions for each category:");
            for (int c : count) printf(" %g", (double)c / nsite);
            printf("\nSite rates printed to %s.rate\n", prefix.c_str());
        }
        if (alrt > 0 || lbp > 0) {
            // bootstrap weightings: nsite sites drawn with replacement, counted per pattern (the unobserved +ASC patterns
            // have frequency 0 and are never drawn)
            const int times = alrt > lbp ? alrt : lbp;
            const size_t np = (size_t)aln.getNPattern();
            std::vector<float> samples((size_t)times * np, 0.0f);
            std::mt19937_64 gen(seed);
            std::discrete_distribution<size_t> pick(freq.begin(), freq.end());
            for (int r = 0; r < times; r++)
                for (int k = 0; k < nsite; k++) samples[(size_t)r * np + pick(gen)] += 1.0f;
            tree.setBootSamples(samples.data(), times);
            std::vector<PhyloTree::BranchSupport> sup;
            auto t0 = std::chrono::steady_clock::now();
            tree.testAllBranches(alrt, lbp, sup, true);
            const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            printf("Branch tests (%d SH-aLRT, %d local bootstrap replicates) on %d internal branches: %.4f s\n", alrt, lbp,
                   (int)sup.size(), sec);
            const std::string labelled = tree.supportTreeString(sup, alrt > 0, lbp > 0);
            printf("Tree with %s%s supports: %s\n", alrt > 0 ? "SH-aLRT" : "", lbp > 0 ? "/LBP" : "", labelled.c_str());
            std::ofstream out((prefix + ".iqhip").c_str(), std::ios::app);
            out << "support_tree " << labelled << "\n";
        }
        if (bb > 0) {
            if (mixture || spec.ascertainment) throw std::runtime_error("-bb is not available for mixture models and +ASC");
            std::vector<std::string> newicks;
            if (!treeset_file.empty()) newicks = readTreeSet(treeset_file);
            auto t0 = std::chrono::steady_clock::now();
            if (!search) {
                tree.genBootSamples(bb, nsite, seed, 0xA0u);
                tree.initUFBoot(bb, seed);
                tree.ufboot_epsilon = beps;
            }
            const std::string te_tree = tree.getTreeString();
            for (size_t k = 0; !search && k <= newicks.size(); k++) {
                double cur = lnl;
                if (k > 0) {
                    tree.readTreeString(newicks[k - 1], aln.seq_names);
                    if (tree.leafNum != aln.getNSeq()) throw std::runtime_error("-z: a tree with another number of taxa");
                    tree.initializeAllPartialLh();
                    tree.clearAllPartialLH();
                    cur = tree.computeLikelihood();
                    if (!blfix) {
                        tree.optimizeAllBranches();
                        tree.clearAllPartialLH();
                        cur = tree.computeLikelihood();
                    }
                } else {
                    tree.clearAllPartialLH();
                    cur = tree.computeLikelihood();
                }
                tree.ufbootNextIteration();
                tree.saveCurrentTree(cur);
                tree.saveNNITrees();
            }
            if (!search && !newicks.empty()) {   // the supports go onto the -te tree
                tree.readTreeString(te_tree, aln.seq_names);
                tree.initializeAllPartialLh();
            }
            PhyloTree::UFBootSummary sum;
            tree.summarizeBootstrap(sum);
            const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            printf("UFBoot: %lld candidate trees, %d distinct bootstrap trees\n", (long long)tree.ufboot_next_id, sum.distinct_trees);
            printf("UFBoot bookkeeping (%d replicates, %d trees and their NNI neighbourhoods): %.4f s\n", bb, (int)newicks.size() + 1, sec);
            printf("Log-likelihood cutoff on original alignment: %.6f\n", tree.ufboot_min_orig_logl);
            writeText(prefix + ".suptree", sum.support_tree + "\n");
            writeText(prefix + ".contree", sum.consensus_tree + "\n");
            printf("Tree with UFBoot supports written to %s.suptree, consensus tree to %s.contree\n", prefix.c_str(), prefix.c_str());
            if (wbt) {
                std::string all;
                for (const std::string &t : sum.boot_trees) all += namedTopology(t, aln.seq_names) + "\n";
                writeText(prefix + ".ufboot", all);
                printf("UFBoot trees printed to %s.ufboot\n", prefix.c_str());
            }
        }
        if (!treeset_file.empty() && zb > 0) {
            const std::vector<std::string> newicks = readTreeSet(treeset_file);
            std::vector<double> scales;
            if (au) scales = {0.5, 0.6, 0.7, 0.8, 0.9, 1.0, 1.1, 1.2, 1.3, 1.4};
            std::vector<PhyloTree::TreeTest> res;
            std::vector<double> au_bp;
            auto t0 = std::chrono::steady_clock::now();
            tree.evaluateTrees(newicks, blfix, zb, zw, scales, seed, res, au_bp);
            const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            printf("Tree topology tests (%d trees, %d RELL replicates%s): %.4f s\n", (int)res.size(), zb,
                   au ? ", AU replicates at 10 scales" : "", sec);
            printf("Tree      logL    bp-RELL    p-KH     p-SH    %sc-ELW\n", zw ? "p-WKH    p-WSH    " : "");
            for (size_t t = 0; t < res.size(); t++) {
                const iqhip_tree_test &r = res[t].t;
                printf("TOPOTEST %3d %.6f  %.4f %c  %.4f %c  %.4f %c  ", (int)t + 1, res[t].logl, r.rell_bp,
                       r.rell_confident ? '+' : '-', r.kh_pvalue, r.kh_pvalue < 0.05 ? '-' : '+', r.sh_pvalue,
                       r.sh_pvalue < 0.05 ? '-' : '+');
                if (zw)
                    printf("%.4f %c  %.4f %c  ", r.wkh_pvalue, r.wkh_pvalue < 0.05 ? '-' : '+', r.wsh_pvalue,
                           r.wsh_pvalue < 0.05 ? '-' : '+');
                printf("%.4f %c\n", r.elw_value, r.elw_confident ? '+' : '-');
            }
            if (au) {
                printf("AU bootstrap proportions per scale r (STEP 2 of the AU test; no AU p-value is computed)\nAUSCALE   r");
                for (double r : scales) printf(" %6.1f", r);
                printf("\n");
                for (size_t t = 0; t < res.size(); t++) {
                    printf("AUBP    %3d", (int)t + 1);
                    for (size_t k = 0; k < scales.size(); k++) printf(" %.4f", au_bp[k * res.size() + t]);
                    printf("\n");
                }
            }
        }
        if (wsl) {
            writeSiteLh(prefix + ".sitelh", aln, pattern_lh.data());
            printf("Site log-likelihoods printed to %s.sitelh\n", prefix.c_str());
        }
        printf("BEST SCORE FOUND : %.3f\n", lnl);
    } catch (const std::exception &ex) {
        fprintf(stderr, "ERROR: %s\n", ex.what());
        return 2;  // outError(): exit(2), tools.cpp:99-106
    }
    return 0;
}
