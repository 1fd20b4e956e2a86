// supertree_host.h -- host mirror of the edge-linked partition model: the slice of PhyloSuperTreePlen /
// PartitionModelPlen (phylosupertreeplen.cpp) that sits on the likelihood kernels, on top of a partition group of engines
// (include/iqhip.h, iqhip_partition_*).
//
// P PhyloTrees of identical topology (copyTopology of the super tree), each with its own alignment, model and engine.
// Every member runs the FULL super-tree topology: a taxon without data in a partition stays in its alignment as an
// all-unknown row (the reference drops it with removeGappySeq and links the trees with linkTrees / mapTrees; the
// likelihood is the same, and a branch with only such taxa behind it has df = ddf = 0 exactly).  Member p's branch
// lengths are the super tree's times part_rate[p] -- written by this class whenever either changes.
//
//   computeLikelihood      PhyloSuperTreePlen::computeFunction (:474-511): the sum of the members' likelihoods
//   optimizeOneBranch      :425-472 over PhyloTree::optimizeOneBranch (phylotree.cpp:2148-2192): per member the pending
//                          partials and theta through its own computeLikelihoodDerv path, then ONE
//                          iqhip_partition_newton_branch on sum_p r_p df_p(r_p x); the diverged-Newton reset
//                          (phylotree.cpp:2167-2176) on the summed lnL through iqhip_partition_lnl_from_theta
//   optimizeAllBranches    :415-423 over PhyloTree::optimizeAllBranches (phylotree.cpp:2232-2332): the reference's
//                          branch order and stopping rule on the super tree
//   optimizeGeneRate       PartitionModelPlen::optimizeGeneRate (:219-254): the P optimizeTreeLengthScaling Brent
//                          searches (phylotree.cpp:2103-2118) in lockstep (BrentMachine), one
//                          iqhip_partition_traverse_lnl per round, then the normalisation
//   optimizeParameters     PartitionModelPlen::optimizeParameters (:107-200).  DEVIATION: the per-partition
//                          substitution parameters are taken as given (no optimizeParametersOnly, no linked alpha):
//                          rates and branch lengths only
//   initUFBoot / saveCurrentTree / saveNNITrees / summarizeBootstrap   PhyloSuperTreePlen::getBestNNIForBran's
//                          computePatternLikelihood + saveCurrentTree (:1367-1372): PhyloTree's own bookkeeping run on
//                          `super`, its device calls sent to the group (iqhip_partition_ufboot_*); sites are resampled
//                          within partitions (superalignment.cpp:360-370), every member keeps its own sample matrix
//   computeDist / computeBioNJ / fixNegativeBranch   the starting tree of a run without -te: PhyloSuperTreePlen::computeDist
//                          (:361-371, every pair solved jointly over the members: iqhip_partition_pair_distances),
//                          PhyloTree::computeBioNJ on that matrix, PhyloSuperTreePlen::fixNegativeBranch (:1710-1729)
#pragma once
#include <string>
#include <vector>

#include "alignment_host.h"
#include "model_host.h"
#include "partition_spec.h"
#include "phylo_host.h"

struct iqhip_partition;

namespace iqhost {

// One partition as read from a partition file: the sites cut from the one alignment (extractSites), pattern-compressed
// anew, and the model its string names.  EVERY taxon is kept; one without data in the partition is an all-unknown row
// (the reference drops it with removeGappySeq; the likelihood is the same).
struct PartitionInput {
    std::string name, model;
    Alignment aln;
    ModelInputs inputs;
};
// the data type a partition's model string asks for: "DNA" (JC F81 K80 HKY TN GTR), "CODON" (GY), "BIN" (JC2 GTR2), else "AA"
std::string partitionSequenceType(const std::string &model);
// RAxML-style partition file (partition_spec.h; readPartitionRaxml, phylosupertree.cpp:150-266) over ONE alignment file
// (PHYLIP or FASTA, its columns of whatever data types the models name).  Mixtures and +ASC are refused: such members
// cannot join a partition group.
void readPartitionRaxml(const std::string &aln_file, const std::string &part_file, std::vector<std::string> &seq_names,
                        std::vector<PartitionInput> &parts);
void readPartitionStrings(const std::string &aln_content, const std::string &part_content, std::vector<std::string> &seq_names,
                          std::vector<PartitionInput> &parts);

class PhyloSuperTree : private PhyloTree::NNIBackend {
public:
    typedef PhyloTree::NNIMove NNIMove;
    typedef PhyloTree::BranchList BranchList;
    PhyloSuperTree();
    ~PhyloSuperTree();
    PhyloSuperTree(const PhyloSuperTree &) = delete;
    PhyloSuperTree &operator=(const PhyloSuperTree &) = delete;

    // before the first partition: the super tree.  Later: a candidate tree of the search on the same taxa -- `super` and every
    // member re-read it (node ids and neighbour order agree), engines, models and rates stay, member lengths = rate x super
    // lengths, every member vector is dropped
    void readTreeString(const std::string &newick, const std::vector<std::string> &names);
    std::string getTreeString() const { return super.getTreeString(); }
    // a new member of the super tree's topology; the caller gives it its alignment and model (setAlignment, setModel)
    PhyloTree *addPartition(const std::string &name);
    PhyloTree *addPartition(const PartitionInput &in);   // ... with the alignment and model of a partition file's entry
    // one engine per member on `device` + the group; member lengths = rate x super lengths
    void attachEngines(int device);

    PhyloTree super;                      // topology and lengths; it never gets an engine
    std::vector<PhyloTree *> parts;
    std::vector<std::string> part_name;
    std::vector<double> part_rate;        // 1 after addPartition
    std::vector<double> cur_score;        // part_info[part].cur_score
    bool fixed_rates = true;              // -q; false: -spp
    iqhip_partition *group = nullptr;
    double min_branch_length = 1e-6, max_branch_length = 100.0;
    int num_param_iterations = 100;       // params.num_param_iterations

    int size() const { return (int)parts.size(); }
    void setRates(const double *rates);   // also rescales the members' lengths
    double computeLikelihood();
    // returns the accepted length of the super-tree branch (node ids a, b)
    double optimizeOneBranch(int a, int b, bool clearLH = true, int maxNRStep = 100);
    double optimizeAllBranches(int my_iterations = 100, double tolerance = 0.001, int maxNRStep = 100);
    double optimizeGeneRate(double gradient_epsilon);
    double optimizeParameters(bool fixed_len, double logl_epsilon, double gradient_epsilon);
    // the thin call: theta of (a, b) on every member, then iqhip_partition_newton_branch with these arguments
    void partitionNewtonBranch(int a, int b, double xguess, double x1, double x2, double xacc, int max_steps, double *optx,
                               double *d2l, int *nsteps, double *part_lnl);
    double totalNSite() const;
    void setBranchBounds(double lo, double hi);   // of the super tree and every member
    // the branches in the order optimizeAllBranches visits them (node ids)
    void branchOrder(std::vector<int> &n1, std::vector<int> &n2);

    // ---- NNI on the super tree: the single-tree operation applied to `super` and, by node id, to every member.  Moves
    //      and their five lengths are in super-tree units; member lengths are rate x super length.
    // every member (and the super tree, for its keys) keeps a buffer per directed vector: what the batched evaluations
    // need.  Before the engines are attached.
    void setAllBranchMode();
    void doNNI(const NNIMove &move);                        // PhyloTree::doNNI(move, clearLH = true) on all of them
    void changeNNIBrans(const NNIMove &move, bool nni5);    // ... and the vectors that look through the five branches go stale
    NNIMove doOneRandomNNI(int a, int b, int bit1, int bit2);
    void saveBranchLengths(std::vector<double> &lenvec) const { super.saveBranchLengths(lenvec); }
    void restoreBranchLengths(const std::vector<double> &lenvec);   // and the members' lengths; every member vector dropped
    void clearAllPartialLH();
    // The branch-by-branch path (PhyloTree::getBestNNIForBran, phylotree.cpp:2873-3066) from existing calls only: each swap
    // is made on every tree, the central branch (nni5: the two at node1, the central one, the two at node2) solved jointly
    // with optimizeOneBranch in the reference's order, the summed lnL taken, and the swap undone; the second swap starts
    // from the lengths the first left, and all lengths are restored at the end.  Every member vector is dropped.
    // ptnlh_rows (optional, 2 entries): the row of every member's store that receives the per-pattern values of the two
    // neighbours (phylosupertreeplen.cpp:1367-1372)
    NNIMove getBestNNIForBran(int a, int b, bool nni5, NNIMove moves[2], const int *ptnlh_rows = nullptr);
    // the two / ten rounds of phylo_nni.cpp run on `super`, one iqhip_partition_optimize_branch_batch per round; a
    // candidate whose solve diverged (optx > 0.95 max_branch_length) takes the branch-by-branch path.  setAllBranchMode.
    void evaluateNNIsBatch(std::vector<NNIMove> &moves, const BranchList *branches = nullptr);
    // ptnlh_rows (optional, 2 per branch in move order): the last of the five rounds goes through
    // iqhip_partition_optimize_branch_batch_rows, so candidate k's per-pattern values land in row ptnlh_rows[k] of every member
    void evaluateNNIs5Batch(std::vector<NNIMove> &moves, const int *ptnlh_rows, const BranchList *branches);
    void evaluateNNIs5Batch(std::vector<NNIMove> &moves, const BranchList *branches = nullptr) { evaluateNNIs5Batch(moves, nullptr, branches); }

    // ---- UFBoot on the super tree (PhyloSuperTreePlen::getBestNNIForBran's computePatternLikelihood + saveCurrentTree).
    //      Sites are resampled WITHIN partitions (superalignment.cpp:360-370): every member keeps its own sample matrix.  The
    //      per-replicate state is the GROUP's (iqhip_partition_ufboot_*); the bookkeeping -- ids, tie draws, the strings of
    //      taken candidates, winners, split counts -- is PhyloTree's own, run on `super` with the device calls sent here.
    //      The members' own ufboot_nsamples stay 0.
    // member p: nsamples replicates of its own site count, drawn with stream p
    void genBootSamples(int nsamples, uint64_t seed);
    void setBootSamples(int part, const float *samples, int nsamples);   // [nsamples][member's nptn]
    void reservePtnlhRows(int nrows);
    void initUFBoot(int nsamples, uint64_t seed) { needGroup(); super.initUFBoot(nsamples, seed); }
    // the current tree's row on every member (row 0), then one update
    void saveCurrentTree(double logl) { needGroup(); super.saveCurrentTree(logl); }
    void saveNNITrees() { needGroup(); super.saveNNITrees(); }
    void saveNNITrees(const std::vector<NNIMove> &evaluated) { needGroup(); super.saveNNITrees(evaluated); }
    void ufbootNextIteration() { super.ufbootNextIteration(); }
    void summarizeBootstrap(PhyloTree::UFBootSummary &out) { needGroup(); super.summarizeBootstrap(out); }

    // ---- the starting tree of a partitioned alignment (include/iqhip.h, "Joint pairwise distances of a partition group")
    // PhyloSuperTreePlen::computeDist for all pairs: iqhip_partition_pair_distances with x1 = xacc = min_branch_length, x2 =
    // MAX_GENETIC_DIST and 100 Newton steps at the current rates.  dist, d2l (or nullptr): [leafNum][leafNum]; init: the same
    // shape or nullptr, an entry of 0 = the pair's JC start (SuperAlignment::computeDist)
    void computeDist(double *dist, double *d2l, const double *init = nullptr);
    // PhyloTree::computeBioNJ: iqhip_bionj on member 0's engine, PhyloTree::bionjNewick, and the tree read into the super tree
    // and every member (rates and models stay; member lengths = rate x super lengths, negative ones included:
    // fixNegativeBranch(false) is the caller's next step, as in the reference)
    void computeBioNJ(const double *dist, const double *var, std::string *newick = nullptr);
    // PhyloSuperTreePlen::fixNegativeBranch (:1710-1729): every member runs PhyloTree::fixNegativeBranch(force) on its own
    // lengths (rate x super length); if any branch was fixed, each super-tree branch becomes sum_p len_p nsite_p / sum_p
    // nsite_p in member order (PhyloSuperTree::computeBranchLengths, phylosupertree.cpp:1353-1398; with codon AND other
    // members a codon member counts 3 nsite_p in the denominator: rescale_codon_brlen), and the members get rate x super
    // length again.  Returns the number of fixed member branches.
    // DEVIATION: a taxon without data in a partition is an all-unknown row here, not a pruned sub-tree: every branch occurs
    // once in every member, and such a member's parsimony count for a branch behind which it has no data is 0.
    int fixNegativeBranch(bool force);
    void pairTiming(double *counts_ms, double *solve_ms) const;   // iqhip_debug_partition_pair_timing

    // counters (tests, bench): joint solves, batches of joint solves, group traversals, diverged-Newton resets; of the last
    // optimizeGeneRate: Brent evaluations per member and lockstep rounds
    long num_group_solves = 0, num_group_batches = 0, num_group_traversals = 0, num_diverged = 0;
    std::vector<int> gene_rate_evals;
    int gene_rate_rounds = 0;

private:
    // PhyloTree::NNIBackend for `super`
    void pendingVectors(const std::vector<PhyloNode *> &n1, const std::vector<PhyloNode *> &n2, bool all) override;
    void submitTasks(const std::vector<iqhip_branch_task> &tasks, std::vector<iqhip_branch_result> &res, const int32_t *rows) override;
    void bestNNIForBran(int node1, int node2, bool nni5, NNIMove moves[2], const int *ptnlh_rows) override {
        getBestNNIForBran(node1, node2, nni5, moves, ptnlh_rows);
    }
    void ufbootInit(int nsamples) override;
    void ufbootReserveRows(int nrows) override { reservePtnlhRows(nrows); }
    void ufbootPutCurrentRow(int row) override;
    void ufbootUpdate(const iqhip_ufboot_tree *ent, int n, double epsilon, double logl_cutoff, int64_t counts[3],
                      double *min_orig_logl) override;
    void ufbootFetchTrees(int64_t *boot_tree) override;
    void needGroup() const;
    void pushLengths();                   // member lengths = rate x super lengths; all member vectors dropped
    void prepareBranch(int a, int b);     // current_it + pending partials + theta of (a, b) on every member
    void hip(int rc, const char *what) const;
    double sumScores() const;
};

}  // namespace iqhost
