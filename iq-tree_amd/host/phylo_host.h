// phylo_host.h -- host-side mirror of the slice of IQ-TREE's PhyloTree that sits directly on
// top of the likelihood kernels.  It exists so that (a) the drop-in boundary can be exercised
// exactly the way the reference's callers exercise it (setLikelihoodKernel(); clearAllPartialLH();
// computeLikelihood(); computeLikelihoodDerv(); ...) on a box that has no reference sources,
// and (b) the adapter logic shipped in integration/phylotree_hip.cpp (recursion, lazy flags,
// LM_PER_NODE re-orientation, lh_scale_factor bookkeeping) is tested code.
//
// Names and argument meaning follow the reference (file:line = /root/reference):
//   PhyloNeighbor fields            phylonode.h:102-127
//   setLikelihoodKernel + 4 ptrs    phylotreesse.cpp:60-357, phylotree.h:658-659,697-698,742-743,979-980
//   initializeAllPartialLh          phylotree.cpp:667-716,834-987   (LM_PER_NODE / LM_ALL_BRANCH)
//   computeLikelihood               phylotree.cpp:1031-1072
//   clear*PartialLh                 phylonode.cpp:15-65, phylotree.cpp:495-502
//   computeTipPartialLikelihood     phylotreesse.cpp:359-529
//   optimizeOneBranch/AllBranches   phylotree.cpp:2120-2332, optimization.cpp:388-465
// The compute kernels themselves are NOT here: the four *HIP member functions only build a
// plan and call libiqhip.so (include/iqhip.h).  There is no CPU kernel in this library; asking
// for LK_EIGEN / LK_EIGEN_SSE throws.
#pragma once
#include <stdint.h>

#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../../include/iqhip.h"
#include "lmap_host.h"

namespace ufboot {
struct SplitCounts;   // ufboot_splits.h
}
namespace iqhip_adapter { template <class X> struct Plan; }   // include/iqhip_adapter.h

namespace iqhost {

typedef short int UBYTE;  // phylonode.h:17

enum LikelihoodKernel { LK_EIGEN = 0, LK_EIGEN_SSE = 1, LK_EIGEN_HIP = 2 };  // tools.h:397-399 (+HIP)
enum LhMemSave { LM_PER_NODE = 0, LM_ALL_BRANCH = 1 };                       // tools.cpp:907,2461
enum SeqType { SEQ_DNA = 0, SEQ_PROTEIN = 1, SEQ_CODON = 2, SEQ_OTHER = 3 };

struct PhyloNode;

struct PhyloNeighbor {
    PhyloNode *node = nullptr;  // the node this neighbor points TO
    double length = 0.0;
    int id = -1;                // branch id
    int partial_lh_computed = 0;  // bit0 = likelihood vector valid, bit1 = parsimony vector valid (phylonode.h:104)
    int pars_slot = -1;           // the engine slot that stands for partial_pars (phylonode.h); a leaf's is its taxon id
    uint64_t partial_lh = 0;      // opaque device key; 0 == NULL (phylonode.h:112)
    double lh_scale_factor = 0.0; // phylonode.h:117
    inline void clearPartialLh() { partial_lh_computed = 0; }
    void clearForwardPartialLh(PhyloNode *dad);  // phylonode.cpp:15-20
};

struct PhyloNode {
    int id = -1;  // leaves: taxon id (alignment row); internal: >= leafNum
    std::string name;
    std::vector<PhyloNeighbor *> neighbors;
    double height = 0.0;
    bool isLeaf() const { return neighbors.size() <= 1; }
    int degree() const { return (int)neighbors.size(); }
    PhyloNeighbor *findNeighbor(const PhyloNode *n) const {
        for (PhyloNeighbor *x : neighbors)
            if (x->node == n) return x;
        return nullptr;
    }
    void clearReversePartialLh(PhyloNode *dad);              // phylonode.cpp:42-50
    void clearAllPartialLh(bool make_null, PhyloNode *dad);  // phylonode.cpp:52-65
};

// a recorded node update (also what the CPU-only tests inspect in dry-run mode); dst / left / right are NULL for
// the intermediate products of a multifurcating node
struct PlanOp {
    PhyloNeighbor *dst, *left, *right;
    iqhip_node_op op;
};

struct MirrorPolicy;  // mirror_policy.h: this tree's answers to include/iqhip_adapter.h

class PhyloTree {
public:
    typedef void (PhyloTree::*ComputePartialLikelihoodType)(PhyloNeighbor *, PhyloNode *);
    typedef double (PhyloTree::*ComputeLikelihoodBranchType)(PhyloNeighbor *, PhyloNode *);
    typedef double (PhyloTree::*ComputeLikelihoodFromBufferType)();
    typedef void (PhyloTree::*ComputeLikelihoodDervType)(PhyloNeighbor *, PhyloNode *, double &, double &);

    PhyloTree();
    ~PhyloTree();
    PhyloTree(const PhyloTree &) = delete;
    PhyloTree &operator=(const PhyloTree &) = delete;

    // ---- tree ----------------------------------------------------------------------------
    // Newick with branch lengths; leaf labels are looked up in `names` (alignment order) or,
    // when names is empty, parsed as integer taxon ids.  A bifurcating top level is unrooted.
    void readTreeString(const std::string &newick, const std::vector<std::string> &names);
    std::string getTreeString() const;
    // the same tree as src, field by field: node ids, names, the order of every node's neighbours, branch ids and lengths
    // (no printed string in between).  Drops this tree's vectors as readTreeString does
    void copyTopology(const PhyloTree &src);
    // lengths only, looked up by node id; throws when the topologies differ.  The caller invalidates the vectors
    void copyBranchLengths(const PhyloTree &src);
    int leafNum = 0, nodeNum = 0, branchNum = 0;
    PhyloNode *root = nullptr;  // a leaf, as in the reference (phylotree.cpp:1034)
    std::vector<PhyloNode *> nodes;  // index == id
    PhyloNode *findFarthestLeaf(PhyloNode *node = nullptr, PhyloNode *dad = nullptr);  // mtree.cpp:2052

    // ---- data + model (the kernel's inputs, SURVEY 8a a5,a6,a13) -------------------------
    void setAlignment(int nstates, SeqType seq_type, int64_t nptn, const uint8_t *states /*[leaf][ptn]*/,
                      const double *ptn_freq, const double *ptn_invar);
    // +ASC (ModelFactory::unobserved_ptns, model/modelfactory.cpp:359-370): the last n_unobserved
    // patterns of setAlignment are the unobserved constant patterns; nsites = aln->getNSite()
    void setAscertainment(int64_t n_unobserved, double nsites);
    // new pattern weights / invariant-site terms on an attached engine (computePtnFreq / computePtnInvar,
    // phylotreesse.cpp:531-569: the reference recomputes them with every model change)
    void setPtnFreq(const double *ptn_freq);
    void setPtnInvar(const double *ptn_invar);
    int64_t n_unobserved = 0;
    double asc_nsites = 0.0;
    void setModel(int ncat, const double *eval, const double *evec, const double *inv_evec,
                  const double *rates, const double *props);
    // Mixture models (ModelMixture; phylokernelmixture.h / phylokernelmixrate.h): ncat_ components in the
    // reference's block order [class][rate], component q on eigen-system cat_class[q]; eval / evec /
    // inv_evec are the nclass systems concatenated, props[q] = class weight x category proportion
    void setMixtureModel(int nclass, int ncat, const int *cat_class, const double *eval, const double *evec,
                         const double *inv_evec, const double *rates, const double *props);
    int nmixture = 1;
    int num_states = 0, ncat = 0, STATE_UNKNOWN = 0;
    SeqType seq_type = SEQ_DNA;
    int64_t nptn = 0;
    std::vector<double> tip_partial_lh;
    void computeTipPartialLikelihood();  // phylotreesse.cpp:459-527

    // ---- kernel dispatch -----------------------------------------------------------------
    void setLikelihoodKernel(LikelihoodKernel lk);  // phylotreesse.cpp:60
    LikelihoodKernel sse = LK_EIGEN_HIP;
    LhMemSave lh_mem_save = LM_PER_NODE;
    // device: >= 0 creates an engine on that GPU; dry_run records plans without any device
    void attachEngine(int device);
    // pattern-sharded engines (include/iqhip.h "pattern sharding over GPUs"): one handle over several GPUs of this
    // process, or this process's engine joined to the other ranks' (one process per GPU); nothing else changes for
    // the callers below -- every host-visible sum is all-reduced inside the engine
    void attachEngineSharded(const int *device_ids, int ndev, int reduce_mode);
    void attachComm(int nranks, int rank, const void *unique_id);
    void setDryRun(bool on) { dry_run = on; }
    // sends what changed since the last submission (model, alignment, weights) to the engine now; callers of the raw
    // engine calls (the thin pars_* wrappers) need it, every member function below does it itself
    void syncInputs() { pushInputs(); }
    bool heavy_first = true;  // plan order of independent subtrees (see collectPlan)
    // optimizeOneBranch: run the whole Newton-Raphson solve on the device (iqhip_newton_branch)
    // instead of one computeLikelihoodDerv round trip per step; off -> the reference's host loop
    bool device_newton = true;
    bool device_sweep = true;   // optimizeAllBranches: a whole sweep as one engine submission (iqhip_optimize_sweep)
    long num_derv_calls = 0;  // derivative evaluations (host loop: calls; device loop: reported steps)
    iqhip_engine *engine = nullptr;
    int engine_device = -1;   // the GPU of attachEngine
    // Pattern-sharded runs (one process per GPU): when set, every host-visible result vector
    // {lnL | df,ddf | sum_scale per op} is left on the device, handed to this hook (which
    // all-reduces it in place over RCCL on the engine's stream) and only then read back.
    typedef void (*AllReduceHook)(void *device_ptr, int ndoubles, void *ctx);
    void setAllReduceHook(AllReduceHook fn, void *ctx) { allreduce_hook = fn; allreduce_ctx = ctx; }

    void computePartialLikelihood(PhyloNeighbor *dad_branch, PhyloNode *dad);       // :335
    double computeLikelihoodBranch(PhyloNeighbor *dad_branch, PhyloNode *dad);      // :339
    void computeLikelihoodDerv(PhyloNeighbor *dad_branch, PhyloNode *dad, double &df, double &ddf);  // :344
    double computeLikelihoodFromBuffer();                                           // :349

    // ---- buffers / flags -----------------------------------------------------------------
    void initializeAllPartialLh();  // phylotree.cpp:667
    void deleteAllPartialLh();      // phylotree.cpp:718
    void clearAllPartialLH();       // phylotree.cpp:495
    bool central_partial_lh = false;
    bool theta_computed = false;
    PhyloNeighbor *current_it = nullptr, *current_it_back = nullptr;

    // ---- callers (hot loops 1 and 2 of SURVEY section 3) -----------------------------------
    double computeLikelihood(double *pattern_lh = nullptr);  // phylotree.cpp:1031
    double curScore = 0.0;
    double min_branch_length = 1e-6, max_branch_length = 100.0;  // tools.cpp defaults
    void optimizeOneBranch(PhyloNode *node1, PhyloNode *node2, bool clearLH = true, int maxNRStep = 100);
    double optimizeAllBranches(int my_iterations = 100, double tolerance = 0.001, int maxNRStep = 100);

    // ---- NNI evaluation (phylotree.cpp:2873-3066): both swaps around an internal branch, the central
    //      branch (and with nni5 the four adjacent ones) re-optimised on scratch buffers, tree restored
    struct NNIMove {
        int node1 = -1, node2 = -1;
        int node1_nei = -1, node2_nei = -1;  // the two subtrees (by their root node id) that were swapped
        double newloglh = 0.0;
        double newLen[5] = {0, 0, 0, 0, 0};
        int ptnlh_row = -1;  // row of the engine's per-pattern store holding this neighbour's pattern lnL (the reference's ptnlh)
    };
    // ptnlh_rows (optional, 2 entries): store rows that receive the per-pattern lnL of the two neighbours
    // (iqhip_ptnlh_put_current after the final computeLikelihoodFromBuffer, phylotree.cpp:3019-3020)
    NNIMove getBestNNIForBran(PhyloNode *node1, PhyloNode *node2, bool nni5, NNIMove moves[2],
                              const int *ptnlh_rows = nullptr);
    static const int NNI_MAX_NR_STEP = 10;  // phylotree.h
    // computeAllPartialLh (phylotree.cpp:504-514): every directed vector valid (needs LM_ALL_BRANCH)
    void computeAllPartialLh();
    // IQTree::evaluateNNIs with nni1 for EVERY internal branch, all 2(n-3) candidates side by side in one
    // iqhip_optimize_branch_batch submission (same swaps, same Newton solve, same lnL as getBestNNIForBran
    // gives one branch at a time).  moves: 2 per internal branch, in branch order.  Needs LM_ALL_BRANCH.
    // branches (optional): only these internal branches become tasks, in list order and each normalised to
    // node1->id < node2->id; the entries of a listed branch are those the full call gives for it.  With a list only the
    // directed vectors those branches read are made valid (computePartialLhAround), not all of them
    typedef std::vector<std::pair<int, int>> BranchList;
    void evaluateNNIsBatch(std::vector<NNIMove> &moves, const BranchList *branches = nullptr);
    // the same with nni5 (the reference's default, params.nni5): per candidate the two branches at node1, the
    // central branch and the two at node2 are optimised in that order (phylotree.cpp:2984-3024); five rounds of
    // batched tasks per swap, ten submissions per tree instead of ~10 per branch
    // ptnlh_rows (optional, 2 per internal branch in move order): the last round goes through
    // iqhip_optimize_branch_batch_rows, so every candidate's per-pattern lnL lands in its store row on the device
    // ptnlh_rows with a branch list: 2 per LISTED branch in move order
    void evaluateNNIs5Batch(std::vector<NNIMove> &moves, const int *ptnlh_rows = nullptr, const BranchList *branches = nullptr);
    // Who runs the tasks of a batched NNI evaluation for a tree WITHOUT an engine of its own: the super tree of an
    // edge-linked partition model (supertree_host.h) sets itself here, and the candidate and task construction, the two
    // nni1 rounds and the five nni5 rounds of phylo_nni.cpp serve it unchanged.  The tree's Neighbor keys must be the keys
    // the backend's engines know; results[t].lnl is the whole log-likelihood (the scale-factor terms included), so the
    // scaffold adds nothing to it: the Neighbors of such a tree carry lh_scale_factor 0 and the per-op sums are 0.
    struct NNIBackend {
        virtual ~NNIBackend() {}
        // every directed vector valid (all), or the four around each listed branch; the tree's keys and next_key in step
        virtual void pendingVectors(const std::vector<PhyloNode *> &n1, const std::vector<PhyloNode *> &n2, bool all) = 0;
        // rows (or nullptr): per task the row of the backend's per-pattern stores that takes its values (< 0: none)
        virtual void submitTasks(const std::vector<iqhip_branch_task> &tasks, std::vector<iqhip_branch_result> &res,
                                 const int32_t *rows) = 0;
        // the branch-by-branch path; ptnlh_rows (or nullptr): the store rows of the two neighbours
        virtual void bestNNIForBran(int node1, int node2, bool nni5, NNIMove moves[2], const int *ptnlh_rows) = 0;
        // the device side of the UFBoot bookkeeping below, for the tree without an engine: the state, the store rows and
        // the sample matrices are the backend's
        virtual void ufbootInit(int nsamples) = 0;
        virtual void ufbootReserveRows(int nrows) = 0;
        virtual void ufbootPutCurrentRow(int row) = 0;   // the current tree's per-pattern values into `row`
        virtual void ufbootUpdate(const iqhip_ufboot_tree *ent, int n, double epsilon, double logl_cutoff, int64_t counts[3],
                                  double *min_orig_logl) = 0;
        virtual void ufbootFetchTrees(int64_t *boot_tree) = 0;
    };
    NNIBackend *nni_backend = nullptr;
    // the internal branches in the order both NNI evaluations list them (node1->id < node2->id)
    void internalBranches(std::vector<PhyloNode *> &n1, std::vector<PhyloNode *> &n2) const;
    // the four subtree vectors around each listed branch (what its NNI candidates read), one submission; LM_ALL_BRANCH
    void computePartialLhAround(const std::vector<PhyloNode *> &n1, const std::vector<PhyloNode *> &n2);

    // ---- tree edits of the NNI search (phylotree.cpp:2726-2871) --------------------------------------------------------
    // doNNI: the subtrees at node1_nei and node2_nei change places wherever they hang on node1 / node2 now, so the same
    // move a second time restores the tree, neighbour order included.  The Neighbor objects move with their lengths.
    // clearLH: both central vectors and everything that looks through the branch from outside go stale (:2826-2832).
    // LM_PER_NODE: each end's buffer is first moved onto the central Neighbor that points to it (:2799-2803).
    void doNNI(const NNIMove &move, bool clearLH = true);
    // newLen[0] to the central branch and, with nni5, newLen[1..4] to the other branches of node1 then node2 in neighbour
    // order AFTER the swap -- the order in which getBestNNIForBran / evaluateNNIs5Batch fill newLen
    void changeNNIBrans(const NNIMove &move, bool nni5);
    // one length per Neighbor object in creation order; the objects keep their branch through doNNI
    void saveBranchLengths(std::vector<double> &lenvec) const;
    void restoreBranchLengths(const std::vector<double> &lenvec);   // the caller clears the vectors (clearAllPartialLH)
    // doOneRandomNNI with its two coin flips as arguments: bit 0 takes the first other neighbour of the node, bit 1 the
    // second.  No vector is cleared (the reference's caller recomputes everything); returns the move that was made
    NNIMove doOneRandomNNI(PhyloNode *node1, PhyloNode *node2, int bit1, int bit2);
    // node id -> neighbour ids in neighbour order (search_host.h's Adjacency)
    std::vector<std::vector<int>> adjacency() const;

    // ---- SH-aLRT / local bootstrap (PhyloTree::testAllBranches, phylotree.cpp:3984-4103) on the device:
    //      computeLikelihood -> store row 0; both NNI neighbours of every internal branch with five branches re-optimised
    //      -> rows 1 + 2 q + cnt; one iqhip_branch_tests on the samples of setBootSamples (ONE sample matrix for all
    //      branches, see include/iqhip.h).  batched: evaluateNNIs5Batch (needs LM_ALL_BRANCH); else getBestNNIForBran
    //      branch by branch.  Returns the tree's lnL.
    struct BranchSupport {
        int node1 = -1, node2 = -1;
        double lh[3] = {0, 0, 0};
        double sh_alrt = 0, lbp = 0, abayes = 0, alrt_stat = 0;
    };
    double testAllBranches(int reps, int lbp_reps, std::vector<BranchSupport> &out, bool batched = true);
    // Newick with "SH-aLRT[/LBP]" labels (percent, precision 3) on the internal nodes, in the reference's label order
    // (phylotree.cpp:4078-4091); the label of an internal branch sits on its node farther from the root
    std::string supportTreeString(const std::vector<BranchSupport> &sup, bool with_sh, bool with_lbp) const;
    static std::string supportLabel(double sh_alrt, double lbp, bool with_sh, bool with_lbp);

    // ---- tree topology tests (evaluateTrees, phylotesting.cpp:2053-2442; -z trees -zb N [-zw] [-au]) on the device.
    //      Per tree: read the topology (the Newick reader above; same taxa as the current tree), computeLikelihood,
    //      optimizeAllBranches unless fixed_lengths, iqhip_ptnlh_put_current into store row tid, keep the total lnL.  Then
    //      iqhip_gen_boot_samples (nsite draws per replicate, stream 0xA0 of `seed`), iqhip_tree_tests (tie draws of `seed`)
    //      and, with au_scales, iqhip_multiscale_bp with nsamples replicates per scale: au_bp[k * ntrees + tid].
    //      Harness code like testAllBranches; the tree is left at the last topology.
    struct TreeTest {
        double logl = 0.0;
        iqhip_tree_test t = {};
    };
    void evaluateTrees(const std::vector<std::string> &newicks, bool fixed_lengths, int nsamples, bool weighted,
                       const std::vector<double> &au_scales, uint64_t seed, std::vector<TreeTest> &out,
                       std::vector<double> &au_bp, double epsilon = 0.5);

    // ---- pairwise ML distances (PhyloTree::computeDist(dist_mat, var_mat), phylotree.cpp:2476-2541) on the device: one
    //      iqhip_pair_distances with x1 = xacc = min_branch_length, x2 = MAX_GENETIC_DIST and 100 Newton steps, as
    //      AlignmentPairwise::optimizeDist calls minimizeNewton.  dist, d2l: leafNum * leafNum (symmetric, zero diagonal);
    //      init: nullptr or leafNum * leafNum initial distances (0: the pair's JC distance).  The caller forms var_mat
    //      from d2l for its ls_var_type.  Needs no tree beyond the taxa.  pairCounts: AlignmentPairwise's pair_freq.
    static constexpr double MAX_GENETIC_DIST = 9.0;
    void computeDist(const double *init, double *dist, double *d2l);
    void pairCounts(const int32_t *pairs, int npairs, double *counts);

    // ---- likelihood mapping (-lmap; PhyloTree::computeQuartetLikelihoods / doLikelihoodMapping, quartet.cpp:676-1152,
    //      1340-1505) on the device.  computeQuartetLikelihoods: ONE iqhip_quartet_likelihoods call for the nq quartets
    //      (4 taxon ids each, order kept) with x1 = xacc = min_branch_length, x2 = max_branch_length, 100 Newton steps and
    //      the diverged-solve fraction 0.95, as optimizeOneBranch; the reference's optimizeAllBranches(10, 0.1) per quartet
    //      tree are the defaults.  const_invar: nullptr or {p_inv pi[0..3], p_inv} of a +I model.  Needs no tree beyond the
    //      taxa.  quartetCells: the 256 cells and the number of other patterns per quartet.
    //      doLikelihoodMapping: nquartets = 0 or >= C(leafNum, 4): all unique quartets in the reference's order, otherwise
    //      nquartets draws of lmap::drawQuartets(seed); per quartet lmap::region; area / corner counts overall and per
    //      sequence (seq_count[(leafNum + 1) * 10]: row = sequence, the last row all quartets; columns 0..6 regions, 7..9
    //      corners, as countarr of the reference).  Throws below 4 taxa.  Cluster files and the plots are out of scope.
    struct LmapResult {
        std::vector<lmap::QuartetInfo> info;
        int64_t areacount[7] = {0, 0, 0, 0, 0, 0, 0}, cornercount[3] = {0, 0, 0};
        std::vector<int64_t> seq_count;
    };
    void quartetCells(const int32_t *quartets, int nq, double *cells, int32_t *nother);
    void computeQuartetLikelihoods(const int32_t *quartets, int nq, iqhip_quartet_result *results, int iterations = 10,
                                   double tolerance = 0.1, const double *const_invar = nullptr);
    void doLikelihoodMapping(int64_t nquartets, uint64_t seed, LmapResult &out, const double *const_invar = nullptr);

    // ---- BIONJ (PhyloTree::computeBioNJ, phylotree.cpp:2619-2635, over BioNj::create) on the device: one iqhip_bionj on
    //      dist (and var, or nullptr for V = D), leafNum * leafNum each; the step log becomes the reference's Newick string
    //      (bionjNewick, names = the current leaf labels), which replaces the tree through readTreeString -- as the reference
    //      reads its .bionj file back -- followed by initializeAllPartialLh() when there was a tree before.  Lengths may be
    //      negative: fixNegativeBranch(false) is the caller's next step, as in the reference.
    //      steps_out (leafNum - 3), last_out (3), last_len_out (3): optional copies of what iqhip_bionj returned.
    void computeBioNJ(const double *dist, const double *var, std::string *newick = nullptr, iqhip_bionj_step *steps_out = nullptr,
                      int32_t *last_out = nullptr, double *last_len_out = nullptr);
    // pure host: merging b into a makes sub[a] = "(" sub[a] ":" la "," sub[b] ":" lb ")", the end is
    // "(" sub[l0] ":" .. "," sub[l1] ":" .. "," sub[l2] ":" .. ");", every length printed with %10.8f (bionj.h:741,752,526)
    static std::string bionjNewick(const iqhip_bionj_step *steps, int n, const int32_t *last, const double *last_len,
                                   const std::vector<std::string> &names);

    // ---- Fitch parsimony (PhyloTree::setParsimonyKernel, phylotreesse.cpp:34-61; phylotreepars.cpp) on the device.  The
    //      two kernels are iqhip_pars_update and iqhip_pars_branch_scores; a vector is named by the engine slot in
    //      PhyloNeighbor::pars_slot, bit 1 of partial_lh_computed is its flag.  Only the parsimony-informative patterns
    //      are packed, as in the reference (alignment.cpp:624-650).  Trees must be strictly bifurcating (:150).
    void setParsimonyKernel(LikelihoodKernel lk);   // called by setLikelihoodKernel, as the reference's last line
    void initializeAllPartialPars();                // phylotree.cpp:590-650: iqhip_pars_init + one slot per directed vector
    // collects every vector below dad_branch whose flag is down into ONE iqhip_pars_update (as collectPlan does)
    void computePartialParsimony(PhyloNeighbor *dad_branch, PhyloNode *dad);
    int computeParsimonyBranch(PhyloNeighbor *dad_branch, PhyloNode *dad, int *branch_subst = nullptr);
    int computeParsimony();                         // phylotreepars.cpp: the score at the root branch
    void computeAllPartialPars();                   // :284-294, one submission
    // phylotree.cpp:2654-2694: all substitution counts from ONE iqhip_pars_branch_scores, then the Jukes-Cantor
    // correction and the min_branch_length clamp on the host; returns the number of branches set
    int fixNegativeBranch(bool force);
    // phylotreepars.cpp:309-426 with the addition order as an input (the reference shuffles): discards the topology and
    // all likelihood vectors, builds the stepwise-addition tree -- per step one update submission and one
    // iqhip_pars_insert_scores over getBranches order (mtree.cpp:905-919) -- and runs fixNegativeBranch(true).
    // Afterwards the tree is ready for initializeAllPartialLh().  Returns the parsimony score.
    struct ParsStep {
        std::vector<int> node1, node2, score;   // the branches scanned (ids, node1 < node2) and, with trace, their scores
        int chosen = -1, best_score = 0;
    };
    int computeParsimonyTree(const int *taxon_order, std::vector<ParsStep> *trace = nullptr);
    // ---- parsimony SPR search (the SPR rounds of pllComputeRandomizedStepwiseAdditionParsimonyTree,
    //      pll/fastDNAparsimony.c:1857-1942 over rearrangeParsimony / addTraverseParsimony / testInsertParsimony,
    //      :1169-1427) on iqhip_pars_spr_scan.
    // DEVIATION from the reference: PLL visits the nodes one after the other and applies the first node's best improvement
    // at once; here EVERY prune point of the tree is scanned against the same tree in one launch and the single best move
    // (the first minimum in job and step order) is applied per round.  Both end in a tree that no SPR within the radius
    // improves; the trees may differ.
    struct SprMove {
        int prune = -1, subtree = -1;   // the subtree at node `subtree` seen from its neighbour `prune` is cut off ...
        int node1 = -1, node2 = -1;     // ... and regrafted, together with node `prune`, into the branch node1 -- node2
        int depth = 0;                  // 0: the branch the pruning merged (node1, node2 = prune's other neighbours)
    };
    // one job per (internal node p ascending, neighbour s of p in neighbour order): p's other neighbours q1, q2; two root
    // steps for the merged branch (the first scored: the current tree; the second NO_SCORE), the first followed by the walk
    // outward from q1, the second by the walk from q2, to depth <= radius (depth 1 = the branches next to the merged
    // branch: addTraverseParsimony with mintrav = 1, maxtrav = radius).  moves[k] = what step k stands for.  Jobs without a
    // step of depth >= 1 are left out.  Needs no device: without an initialised parsimony state the slots are assigned here.
    void collectSprJobs(int radius, std::vector<iqhip_pars_spr_job> &jobs, std::vector<iqhip_pars_spr_step> &steps,
                        std::vector<SprMove> &moves);
    struct SprRound {
        int score_before = 0, job = -1, step = -1, score = 0, steps_scored = 0;
        SprMove move;
        bool applied = false;
    };
    // per round: computeAllPartialPars (one update submission), collectSprJobs, ONE iqhip_pars_spr_scan; the scan's global
    // first minimum is applied on the host tree when it is below the current score (it then has depth >= 1: every scored
    // root step is the current tree, which is also checked), else the search stops.  max_rounds < 0: until no move improves.
    // The last trace entry of a converged search is the round that found nothing (applied = false).  Returns the score;
    // all likelihood vectors are dropped when a move is applied, branch lengths are split / merged (fixNegativeBranch(true)
    // gives parsimony lengths), node ids stay.
    int optimizeParsimonySPR(int radius, int max_rounds = -1, std::vector<SprRound> *trace = nullptr);
    void applySprMove(const SprMove &mv);   // prune-and-regraft on the host tree, reusing node `prune`
    void getBranches(std::vector<PhyloNode *> &n1, std::vector<PhyloNode *> &n2, PhyloNode *node = nullptr,
                     PhyloNode *dad = nullptr) const;   // mtree.cpp:905-919
    std::vector<uint8_t> pars_informative;          // per pattern, computed by initializeAllPartialPars
    int64_t pars_nsites = 0;                        // informative sites
    bool pars_initialized = false;

    // ---- consumers of the per-pattern lnL (phylotree.cpp:1200-1230, iqtree.cpp:2676-2750) ----------
    // computePatternLikelihood: lnL per pattern of the last computeLikelihood(), scaling events of
    // both ends of current_it put back -- computed on the device, one D2H of nptn doubles
    void computePatternLikelihood(double *ptn_lh);
    // _pattern_lh_cat[ptn*ncat + c] of the current branch (phylotree.cpp:1119-1124 -> scalar kernels), unscaled
    void computePatternLhCat(double *ptn_lh_cat);
    // ---- EM estimation of +R free-rate models (RateFree::optimizeWithEM, model/ratefree.cpp:450-579) on the device ------
    // The reference optimises the rate of category c by Brent's method on a tree-length scaling of a one-category copy of
    // the tree whose pattern weights are the posteriors of c -- C x (3 .. ~20) one-category traversals per EM step, one after
    // the other.  A one-category tree with all lengths scaled by s IS a category of rate s, so here the C Brent searches
    // (BrentMachine, brent_host.h) advance in lockstep on the C-category engine: per round every unfinished machine puts its
    // trial point into rates[c], ONE traversal runs, and ONE iqhip_em_objective returns all C objective values.  An EM step
    // costs 1 + max_c(evals_c) traversals instead of sum_c evals_c, and no nptn x ncat matrix crosses to the host.
    // Rates are NOT renormalised here (the reference's sum += prop[c] * rates[c] is computed and never used): that is the
    // caller's rescaleRates.  Refuses +I+R (p_invar > 0), mixtures and +ASC.  Returns the lnL at the estimated parameters.
    struct EmStep {
        std::vector<double> props, rates;   // after the step (unchanged when the step broke off before assigning them)
        double lnl_before = 0.0;
        std::vector<int> evals;             // Brent evaluations per category
        int rounds = 0;                     // lockstep rounds = traversals spent on the rates
        std::vector<int64_t> floored;       // floored objective terms per category, summed over the rounds (include/iqhip.h)
    };
    double optimizeFreeRatesEM(std::vector<EmStep> *trace = nullptr);
    // one E-step on current_it (theta is rebuilt): cat_sum[ncat]; W stays on the device (iqhip_em_fetch_posteriors)
    void emPosteriors(double *cat_sum);
    // the M-step objectives of all categories for the branch dad_branch (theta is rebuilt), after an E-step
    void emObjective(PhyloNeighbor *dad_branch, PhyloNode *dad, double *f, int64_t *floored);
    // RateGamma::computePatternRates (model/rategamma.cpp:235-258): one E-step plus iqhip_em_site_rates; ties go to the
    // first best category
    void computePatternRates(std::vector<double> &rates_out, std::vector<int> &cat_out);
    // RateFree::setNCategory (model/ratefree.cpp:81-90): equal weights and the discrete-Gamma mean rates of shape 1
    static void freeRateStart(int k, std::vector<double> &props, std::vector<double> &rates);
    // the category rates and weights of the current model; setRateCategories replaces them (same eigen-system; every
    // likelihood vector is stale afterwards: clearAllPartialLH)
    const std::vector<double> &getRates() const { return m_rates; }
    const std::vector<double> &getProps() const { return m_props; }
    void setRateCategories(const double *rates, const double *props);
    void scaleLength(double norm);   // mtree.cpp: every branch length times norm

    // ---- EM estimation of mixture class weights (ModelMixture::optimizeWeights, model/modelmixture.cpp:1355-1416) -------
    // computePatternLhCat(WSL_MIXTURE) (phylotree.cpp:1108-1160): theta of current_it is rebuilt and the per-class pattern
    // likelihoods are left on the device (iqhip_mix_class_lh); out: nullptr or nptn * nmixture doubles [ptn][class]
    enum SiteLoglType { WSL_MIXTURE = 3 };
    void computePatternLhCat(SiteLoglType wsl, double *out);
    // the class weights inside the component weights: w[m] = sum of m_props over the components of class m (ascending)
    std::vector<double> getMixtureWeights() const;
    // optimizeWeights restated: evaluate on the current branch, run the EM on the device with max_steps = nmixture, rescale
    // the component weights (props[q] *= w_new[m] / w_old[m]) and, with +I (p_invar != nullptr and *p_invar > 0; updated),
    // ptn_invar (linear in p_invar), re-send the model, clear all vectors; returns computeLikelihood().
    // nsteps / converged (or nullptr): what the EM reported
    double optimizeMixtureWeights(double *p_invar = nullptr, int *nsteps = nullptr, int *converged = nullptr);
    // the EM alone on the matrix of the last computePatternLhCat(WSL_MIXTURE) (iqhip_mix_weights_em); the tree is unchanged
    void mixWeightsEM(int max_steps, double *weights, double *p_invar, int *nsteps, int *converged, double *trace);
    // ---- per-class log-likelihoods: K candidate models as the K classes of a mixture (iqhip_class_lnl) -------------------
    // theta of dad_branch is rebuilt; lnl[nmixture] = the log-likelihood of every class's model alone on this tree.
    // class_weight[nmixture]: the weight folded into each class's props (1 for candidates); class_invar: nullptr (the
    // resident ptn_invar for every class) or [nmixture][nptn]; floored: nullptr or [nmixture]
    void classLnl(PhyloNeighbor *dad_branch, PhyloNode *dad, const double *class_weight, const double *class_invar, double *lnl,
                  int64_t *floored);
    // PhyloTree::computePatternStateFreq (phylotree.cpp:1162-1196): class_freq [nmixture][nstates] -> ptn_state_freq
    // [nptn][nstates]
    void computePatternStateFreq(const double *class_freq, double *ptn_state_freq);
    double getAlnNSite() const;   // the sum of the pattern frequencies

    // UFBoot: boot_samples uploaded once; computeRELL = saveCurrentTree's dot products, on the device
    void setBootSamples(const float *samples /*[nsamples][nptn]*/, int nsamples);
    // the same matrix drawn on the device (iqhip_gen_boot_samples): nsamples replicates of ndraws sites each
    void genBootSamples(int nsamples, int64_t ndraws, uint64_t seed, uint32_t stream, int64_t first_replicate = 0);
    void computeRELL(std::vector<double> &rell);
    int num_boot_samples = 0;

    // ---- ultrafast bootstrap bookkeeping (IQTree::saveCurrentTree / saveNNITrees / summarizeBootstrap, iqtree.cpp:2676-2801,
    //      2803-2880) on iqhip_ufboot_update.  The per-replicate state lives in the engine; the mirror keeps tree id -> Newick
    //      (taxon ids, taxa sorted: WT_TAXON_ID + WT_SORT_TAXA) for the ids some replicate still refers to.  Tree ids are
    //      sequential from 0.  A tree's rand is (z >> 11) 2^-53 with z of the generator of include/iqhip.h for
    //      (seed, stream 0xBB, rho = tree id, j = 0).  Store rows 0 .. 2 (leafNum - 3) are scratch: row 0 the current tree,
    //      row 1 + k NNI candidate k.
    void initUFBoot(int nsamples, uint64_t seed);   // on the first nsamples rows of the sample matrix (setBootSamples / genBootSamples)
    // one saveCurrentTree(cur_logl) for the tree of the last computeLikelihood(): its row, then one update
    void saveCurrentTree(double logl);
    // evaluateNNIs5Batch with store rows, then ONE update over all 2 (leafNum - 3) candidates in move order, logl = newloglh;
    // a candidate's string is made from (current tree, move) only when a replicate took it.  Needs LM_ALL_BRANCH
    void saveNNITrees();
    // the update alone, for moves that were ALREADY evaluated on the current tree with store rows (ptnlh_row >= 0 each):
    // every candidate is fed, positive or not, in the given order (phylotree.cpp:3019-3024), so one evaluation serves the
    // search and the bootstrap
    void saveNNITrees(const std::vector<NNIMove> &evaluated);
    // iqtree.cpp:1887-1888, the start of a search iteration: logl_cutoff = the minimum of boot_orig_logl
    void ufbootNextIteration();
    static double ufbootRand(uint64_t seed, int64_t tree_id);
    // WT_TAXON_ID + WT_SORT_TAXA of the current tree, or of its NNI neighbour `mv`
    std::string sortedTaxonIdString(const NNIMove *mv = nullptr) const;
    struct UFBootSummary {
        std::vector<int> node1, node2, support;   // per internal branch (internalBranches order): round(100 count / nsamples)
        std::string support_tree;                  // the current tree with the supports as labels (supportTreeString's layout)
        std::string consensus_tree;                // greedy consensus of the winners (ufboot_splits.h), supports as labels
        std::vector<std::string> boot_trees;       // the winner of every replicate, in replicate order
        int distinct_trees = 0;
    };
    void summarizeBootstrap(UFBootSummary &out);
    // the weighted split counts of the current winners alone (what the search's correlation rule snapshots)
    void ufbootSplitCounts(ufboot::SplitCounts &sc);
    int ufboot_nsamples = 0;
    uint64_t ufboot_seed = 0;
    int64_t ufboot_next_id = 0;          // = candidate trees fed so far
    double ufboot_epsilon = 0.5;         // params.ufboot_epsilon
    double ufboot_logl_cutoff = 0.0, ufboot_min_orig_logl = 0.0;
    int64_t ufboot_counts[3] = {0, 0, 0};   // of the last update (include/iqhip.h)
    std::vector<std::pair<int64_t, std::string>> ufboot_trees;   // id (ascending) -> Newick of the ids still referred to

    // ---- host views ----------------------------------------------------------------------
    void fetchScaleNum(PhyloNeighbor *nei, UBYTE *out);
    void fetchPartialLh(PhyloNeighbor *nei, double *out);
    void fetchPatternLh(double *out);

    std::vector<PlanOp> last_plan;  // the most recent submission (tests / tracing)
    long num_partial_lh_computations = 0;  // phylokernel.h:85 (counts leaf visits too)
    long num_submissions = 0;

    // ---- partition models (supertree_host.h) ----------------------------------------------------------------------
    // What computeLikelihoodBranch(dad_branch, dad) would submit, WITHOUT submitting it: the pending node updates of both
    // ends (their flags go up, as if they had run), len_branch[2k], [2k+1] = the branch ids whose lengths are op k's
    // left_len / right_len (-1: the zero-length hand-over inside a multifurcating node), the two ends of the branch and
    // its id.  The caller runs the ops itself (iqhip_partition_traverse_lnl); the lh_scale_factor of the planned vectors
    // is NOT maintained on that route, so the caller ends with clearAllPartialLH().
    void collectBranchPlan(PhyloNeighbor *dad_branch, PhyloNode *dad, std::vector<iqhip_node_op> &ops,
                           std::vector<int> &len_branch, iqhip_branch_end &a, iqhip_branch_end &b, int &root_branch);

private:
    friend struct MirrorPolicy;
    friend class PhyloSuperTree;
    ComputePartialLikelihoodType computePartialLikelihoodPointer = nullptr;
    ComputeLikelihoodBranchType computeLikelihoodBranchPointer = nullptr;
    ComputeLikelihoodFromBufferType computeLikelihoodFromBufferPointer = nullptr;
    ComputeLikelihoodDervType computeLikelihoodDervPointer = nullptr;

    // the four kernels registered for LK_EIGEN_HIP
    void computePartialLikelihoodHIP(PhyloNeighbor *dad_branch, PhyloNode *dad);
    double computeLikelihoodBranchHIP(PhyloNeighbor *dad_branch, PhyloNode *dad);
    void computeLikelihoodDervHIP(PhyloNeighbor *dad_branch, PhyloNode *dad, double &df, double &ddf);
    double computeLikelihoodFromBufferHIP();

    // plan building, flag handling, re-orientation, scale-factor bookkeeping and the bodies of the four kernels are
    // include/iqhip_adapter.h instantiated with MirrorPolicy -- the same templates integration/phylotree_hip.cpp
    // instantiates with the reference's types
    iqhip_branch_end branchEnd(PhyloNeighbor *nei) const;
    void check(int rc, const char *what) const;
    void pushInputs();
    void finishAttach();   // what attachEngine and attachEngineSharded do once the engine exists
    void rebuildTheta(PhyloNeighbor *dad_branch, PhyloNode *dad);
    // "<who> needs an attached engine": needEngine accepts a dry-run tree that has an engine, needDevice does not
    void needEngine(const char *who) const;
    void needDevice(const char *who) const;
    void noCallerCollective(const char *who) const;   // "<who>: not available with a caller-owned collective"
    std::vector<std::string> leafNames() const;        // by taxon id; a leaf without a name goes by its id
    // the Newick string from the root's neighbour with label[node id] behind every internal node
    std::string labelledTreeString(const std::vector<std::string> &label) const;
    // the tail of computeAllPartialLh and computePartialLhAround: the collected node updates as one submission
    void submitPendingVectors(iqhip_adapter::Plan<MirrorPolicy> &plan, const char *who);
    // both batched NNI evaluators: the refusals, the branches, their vectors, the inputs (false: an empty list); then rounds of
    // branch solves (rows: nullptr or a store row per task; sum_scale: per op in task order; diverged: optx > 0.95 max length)
    bool beginNNIBatch(const char *who, const BranchList *branches, std::vector<PhyloNode *> &bn1, std::vector<PhyloNode *> &bn2);
    void branchByBranch(PhyloNode *node1, PhyloNode *node2, bool nni5, NNIMove moves[2], const int *ptnlh_rows);
    void submitBranchTasks(const std::vector<iqhip_branch_task> &tasks, const int32_t *rows, std::vector<double> &sum_scale,
                           std::vector<iqhip_branch_result> &res, std::vector<char> &diverged);

    double computeFuncDerv(double value, double &df, double &ddf);
    double minimizeNewton(double x1, double xguess, double x2, double xacc, double &d2l, int maxNRStep);
    void getPreOrderBranches(std::vector<PhyloNode *> &n1, std::vector<PhyloNode *> &n2, PhyloNode *node,
                             PhyloNode *dad);

    typedef void (PhyloTree::*ComputePartialParsimonyType)(PhyloNeighbor *, PhyloNode *);
    typedef int (PhyloTree::*ComputeParsimonyBranchType)(PhyloNeighbor *, PhyloNode *, int *);
    ComputePartialParsimonyType computePartialParsimonyPointer = nullptr;
    ComputeParsimonyBranchType computeParsimonyBranchPointer = nullptr;
    void computePartialParsimonyHIP(PhyloNeighbor *dad_branch, PhyloNode *dad);
    int computeParsimonyBranchHIP(PhyloNeighbor *dad_branch, PhyloNode *dad, int *branch_subst);
    void collectParsOps(PhyloNeighbor *dad_branch, PhyloNode *dad, std::vector<iqhip_pars_op> &ops);
    void submitParsOps(std::vector<iqhip_pars_op> &ops);
    void needParsimony(const char *what);
    void assignParsSlots();
    int pars_next_slot = 0;
    // The first slot of this tree's vectors; -1: leafNum, a tree that has the arena to itself.  A member of a
    // ParsimonyForest (pars_forest_host.h) has no engine of its own: it owns the 3 * leafNum - 6 slots from its base in the
    // owner's arena and never initialises the arena.
    int pars_slot_base = -1;
    friend class ParsimonyForest;
    // the pieces of initializeAllPartialPars, computeAllPartialPars, fixNegativeBranch and computeParsimonyTree that touch
    // the topology only, so that a forest drives many trees through them with ONE engine call per step
    int64_t parsInformativeSites();   // fills pars_informative; the number of parsimony sites iqhip_pars_init will lay out
    void collectAllParsOps(std::vector<iqhip_pars_op> &ops);
    // the branches in fixNegativeBranch's recursion order, (neighbour, the node it hangs at)
    void fixBranchList(std::vector<PhyloNeighbor *> &all, std::vector<PhyloNode *> &from) const;
    // subst: one count per branch of `all` that is negative or forced, in order; nsite = getAlnNSite()
    int applyParsLengths(const std::vector<PhyloNeighbor *> &all, const std::vector<PhyloNode *> &from, const int32_t *subst,
                         bool force, double nsite);
    void startParsimonyTree(const int *taxon_order, const std::vector<std::string> &names);   // the 3-taxon star, no slots
    std::vector<std::string> pars_names;   // leaf names by taxon id while a stepwise-addition tree is being built
    PhyloNode *newParsNode(int id);
    PhyloNeighbor *newParsNeighbor(PhyloNode *from, PhyloNode *to);
    // the branches of getBranches order with the ops their two vectors still need and their slots (a, c per branch)
    void collectInsertScan(std::vector<PhyloNode *> &nodes1, std::vector<PhyloNode *> &nodes2, std::vector<iqhip_pars_op> &ops,
                           std::vector<int32_t> &ends);
    void insertParsimonyTaxon(PhyloNode *target_node, PhyloNode *target_dad, int taxon, int cur);   // phylotreepars.cpp:382-405
    void finishParsimonyTree();   // node and branch counts, branch ids in traversal order
    void renumberBranches();
    void ufbootWinners(UFBootSummary &out, ufboot::SplitCounts &sc);
    void needUFBootDevice(const char *who) const;   // needDevice, or an NNI backend that stands in for the engine
    bool ufbootFeed(std::vector<iqhip_ufboot_tree> &ent, std::vector<int64_t> &boot_tree);

    AllReduceHook allreduce_hook = nullptr;
    void *allreduce_ctx = nullptr;
    bool dry_run = false;
    bool inputs_dirty = true;   // anything to push before the next submission
    bool model_dirty = true, aln_dirty = true, weights_dirty = false;
    uint64_t next_key = 1;
    uint64_t nni_keys[6] = {0, 0, 0, 0, 0, 0};
    std::vector<uint64_t> nni_batch_keys;  // scratch vectors of evaluateNNIsBatch (2 per candidate)  // nni_partial_lh scratch (phylotree.cpp:852-860)
    std::vector<uint8_t> aln_states;
    std::vector<double> ptn_freq, ptn_invar, m_eval, m_evec, m_inv_evec, m_rates, m_props;
    std::vector<int> m_cat_class;
    std::vector<PhyloNeighbor *> all_neighbors;
    void freeTree();
};

}  // namespace iqhost
