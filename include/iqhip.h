/*
 * iqhip.h -- C ABI of the MI355X (gfx950) likelihood engine `libiqhip.so`.
 *
 * Drop-in boundary for ONE path of IQ-TREE 1.4.3: the Felsenstein-pruning likelihood
 * kernels that sit behind PhyloTree's four member-function pointers
 *   computePartialLikelihoodPointer   phylotree.h:658-659   (kernel: phylokernel.h:70-483)
 *   computeLikelihoodBranchPointer    phylotree.h:697-698   (kernel: phylokernel.h:733-1020)
 *   computeLikelihoodFromBufferPointer phylotree.h:742-743  (kernel: phylokernel.h:1022-1192)
 *   computeLikelihoodDervPointer      phylotree.h:979-980   (kernel: phylokernel.h:485-730)
 * selected by PhyloTree::setLikelihoodKernel (phylotreesse.cpp:60-311).  The reference-side
 * adapter (four PhyloTree member functions that do the recursion / flag handling and call
 * this ABI) is shown in INTEGRATION.md and integration/phylotree_hip.cpp.
 *
 * Conventions
 *   - plain C, POD arguments, every call returns an int status (IQHIP_OK == 0); the text of
 *     the last error of the calling thread is available from iqhip_last_error().  The
 *     reference has no error codes on this path (outError()/assert, tools.cpp:99-106); the
 *     adapter turns a non-zero status into outError().
 *   - one engine == one PhyloTree on one GPU.  No process-global state: engines of
 *     different trees may be driven from different host threads (phylosupertree.cpp:970).
 *   - all vectors stay resident in HBM.  A partial-likelihood vector is addressed by an
 *     opaque 64-bit KEY chosen by the caller -- the adapter uses the value of the host
 *     pointer PhyloNeighbor::partial_lh (phylonode.h:112), which the tree search re-points
 *     freely (phylotree.cpp:2921-2922, phylokernel.h:127-143); the engine maps key -> device
 *     slab lazily.  The companion scale_num array (phylonode.h:122, `short` per pattern)
 *     lives with the same key.
 *   - host-layout arrays use the reference's layout: partial_lh[ptn*block + c*nstates + i],
 *     evec[x*n+i] = U[x][i], inv_evec[i*n+x] = U^-1[i][x]; the device layout
 *     is private and converted by the fetch/upload calls.
 *   - patterns shard over GPUs (every pattern is independent; only scalar sums cross).  Two forms,
 *     both with ONE collective per evaluation -- ncclAllReduce (SUM, f64) over RCCL of the few result doubles:
 *       one process, several GPUs (what the single-process reference needs): iqhip_create_sharded returns an
 *         engine that fronts one shard per device; every call below works on it unchanged;
 *       one process per GPU (MPI / torch.distributed programs): each rank creates its own engine on its pattern
 *         range and joins a communicator with iqhip_comm_unique_id / iqhip_comm_init_rank; from then on every
 *         synchronous call all-reduces its result in place on the device before the host reads it, so all ranks
 *         return identical values.
 */
#ifndef IQHIP_H_
#define IQHIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IQHIP_ABI_VERSION 2

enum {
    IQHIP_OK = 0,
    IQHIP_ERR_NO_DEVICE = 1,   /* no HIP device / runtime failure at create */
    IQHIP_ERR_INVALID = 2,     /* bad argument (shape, key, leaf id, order of calls) */
    IQHIP_ERR_UNSUPPORTED = 3, /* nstates outside 2..64, too many categories, ... */
    IQHIP_ERR_HIP = 4,         /* a HIP runtime call failed; see iqhip_last_error() */
    IQHIP_ERR_NOMEM = 5
};

typedef struct iqhip_engine iqhip_engine;

/* One internal-node update = one call of computePartialLikelihoodEigenSIMD's pattern loop
 * (phylokernel.h:183-479).  A child is a leaf when *_leaf >= 0 (taxon id = row of the
 * alignment passed to iqhip_set_alignment); otherwise *_key names a computed vector.
 * Child order is free: the engine applies the reference's own "leaf goes left" swap
 * (phylokernel.h:116-121) where it matters. */
typedef struct iqhip_node_op {
    uint64_t dst_key;
    uint64_t left_key;
    uint64_t right_key;
    int32_t left_leaf;
    int32_t right_leaf;
    double left_len;  /* PhyloNeighbor::length of the left child branch  */
    double right_len; /* ... of the right child branch */
    uint32_t flags;   /* IQHIP_OP_* */
    uint32_t _pad;
} iqhip_node_op;
/* IQHIP_OP_NO_SCALE: never rescale this result.  A node of degree > 3 (the reference's scalar kernel multiplies ALL
 * children, applies U^-1 and tests for underflow once, phylotreesse.cpp:702-806) is submitted as a chain of binary
 * updates whose intermediate products travel over zero-length branches and carry this flag (iqhip_adapter.h). */
/* IQHIP_OP_SCALAR_RULE: the node's own (last) update of such a chain applies the SCALAR kernel's scaling rule
 * (phylotreesse.cpp:774-801): as the SIMD rule, plus -- before the ptn_invar test -- `lh_max == 0.0` ("very shitty data"):
 * the pattern's vector becomes tip_partial_lh[STATE_UNKNOWN] in every category, scale_num += 4 and
 * sum_scale += 4 * LOG_SCALING_THRESHOLD * ptn_freq.  Binary nodes go through the reference's SIMD kernel, which has no
 * such branch (phylokernel.h:461-474), and carry neither flag. */
enum { IQHIP_OP_NO_SCALE = 1, IQHIP_OP_SCALAR_RULE = 2 };

/* One end of a branch for the lnL / theta calls. leaf >= 0 -> taxon id, else key. */
typedef struct iqhip_branch_end {
    uint64_t key;
    int32_t leaf;
    int32_t _pad;
} iqhip_branch_end;

const char *iqhip_last_error(void);
int iqhip_abi_version(void);
int iqhip_device_count(void);

/* nstates in 2 .. 64.  4, 20, 64 are the reference's SIMD dispatch cases (phylotreeavx.cpp:34-134), 2 its <Vec2d, 2, 2> case
 * (phylotreesse.cpp:262-276); every other count (morphological / multi-state data) goes to the reference's scalar kernels
 * (phylotreesse.cpp:281-309) and here runs on the next kernel size up (4 / 20 / 64) through an exact embedding, with the
 * scalar kernel's scaling rule at every node.  All of them keep the reference's shapes at this boundary (n x n eigen-system,
 * tip table of STATE_UNKNOWN + 1 rows, vectors of nstates*ncat doubles per pattern); embedded counts (everything but 4, 20,
 * 64) have STATE_UNKNOWN = nstates and no mixtures.
 * nptn = aln->size() + unobserved patterns of this shard; ntaxa = leafNum.
 * ncat: 1..32 for exactly 4 states (9..32: "wide DNA", e.g. +R10, +G16, MIX{JC,HKY,GTR}+G4 -- such an engine keeps the
 * 16-pattern tile layout from creation; IQHIP_WIDE4, read at creation, picks its node update: generic (the default), the padded
 * matrix-core kernel, or valu, k_traverse4w on the same plans; any other word is IQHIP_ERR_INVALID); 1..8 for 2- and 3-state data, which run on the 4-state kernels through the
 * embedding (nstates = 3 with ncat = 9 is IQHIP_ERR_UNSUPPORTED); 1..16 on the 64-state kernels; 1..96 on the 20-state
 * kernels (the (class, rate) components of a mixture model count as categories, see iqhip_set_mixture_model). */
int iqhip_create(iqhip_engine **out, int device, int nstates, int ncat, int64_t nptn,
                 int ntaxa);
void iqhip_destroy(iqhip_engine *e);

/* ---- pattern sharding over GPUs -------------------------------------------------------------------------------
 * The reference sums over patterns inside one process (phylokernel.h:251,335,410,592-643,951-962); these calls
 * are what replaces those sums when the patterns live on several GPUs.
 *
 * iqhip_create_sharded: ONE engine handle over ndev GPUs.  Shard g holds the contiguous pattern range
 * [nptn*g/ndev, nptn*(g+1)/ndev) rounded down to multiples of 64 (iqhip_shard_range) of every vector; the model
 * tables are replicated.  All other arguments as iqhip_create; the handle is used with every entry point of this
 * header exactly like a single-device engine (the *_async / result-buffer calls excepted: it reduces itself).
 * reduce_mode: IQHIP_REDUCE_RCCL -- per evaluation one grouped ncclAllReduce on the shards' streams (devices must
 * be distinct); IQHIP_REDUCE_HOST -- every shard writes its result doubles to pinned host memory and the host adds
 * them in shard order (also allows shards that share a device). */
enum { IQHIP_REDUCE_RCCL = 0, IQHIP_REDUCE_HOST = 1 };
int iqhip_create_sharded(iqhip_engine **out, const int *device_ids, int ndev, int reduce_mode, int nstates, int ncat,
                         int64_t nptn, int ntaxa);
int iqhip_num_shards(iqhip_engine *e); /* 1 for a plain engine */
int iqhip_shard_range(iqhip_engine *e, int shard, int64_t *first, int64_t *count, int *device);
/* One process per GPU: rank 0 obtains the 128-byte id (ncclGetUniqueId), the caller distributes it (MPI_Bcast,
 * torch.distributed, a file), every rank attaches its engine.  nptn of each engine is that rank's pattern count.
 * Afterwards all ranks must make the same sequence of compute calls (each contains the collective). */
#define IQHIP_COMM_ID_BYTES 128
int iqhip_comm_unique_id(void *id_out /* IQHIP_COMM_ID_BYTES */);
int iqhip_comm_init_rank(iqhip_engine *e, int nranks, int rank, const void *id /* IQHIP_COMM_ID_BYTES */);
int iqhip_comm_size(iqhip_engine *e); /* ranks / shards that share the patterns; 1 = not sharded */

/* Optional: run on the caller's HIP stream (hipStream_t) instead of the engine's own. */
int iqhip_set_stream(iqhip_engine *e, void *hip_stream);
/* Pre-allocate device slabs for `nvectors` partial-likelihood vectors (the reference's
 * central_partial_lh arena, phylotree.cpp:867-873). Optional; slabs are created on demand. */
int iqhip_reserve(iqhip_engine *e, int nvectors);
/* Forget a key (PhyloTree::deleteAllPartialLh / aligned_free of an NNI scratch buffer). */
int iqhip_release(iqhip_engine *e, uint64_t key);
/* Move a vector to a new key without touching device data (LM_PER_NODE re-orientation is a
 * pointer move on the host, phylokernel.h:127-143, so the key usually does not change). */
int iqhip_rekey(iqhip_engine *e, uint64_t old_key, uint64_t new_key);

/* Alignment side inputs (phylotreesse.cpp:531-569, pattern.h:24, alignment.cpp:470-472).
 * states: ntaxa rows of nptn state bytes (row = taxon id);  ptn_freq, ptn_invar: nptn. */
int iqhip_set_alignment(iqhip_engine *e, const uint8_t *states, const double *ptn_freq,
                        const double *ptn_invar);
int iqhip_set_ptn_freq(iqhip_engine *e, const double *ptn_freq);   /* bootstrap re-weighting */
int iqhip_set_ptn_invar(iqhip_engine *e, const double *ptn_invar); /* +I changed */

/* +ASC (ascertainment-bias correction): the LAST n_unobserved patterns passed to
 * iqhip_set_alignment are the unobserved constant patterns (ModelFactory::unobserved_ptns,
 * phylokernel.h:87; frequency 0, ptn_invar = p_invar*pi) and nsites = aln->getNSite().  The lnL and
 * derivative calls then apply phylokernel.h:868-909,968-1016 (branch), :655-725 (derivatives) and
 * :1124-1187 (from buffer), also inside iqhip_newton_branch / iqhip_optimize_sweep / iqhip_optimize_branch_batch.  0
 * switches it off.  Not available with the *_async calls (the caller owns the collective there).  Sharded engines (iqhip_create_sharded): the unobserved patterns
 * must fit the last shard; prob_const / df_const / ddf_const are reduced with the result.  Comm engines
 * (iqhip_comm_init_rank): the rank holding the unobserved patterns (the last one) passes their number, every other
 * rank passes (0, nsites). */
int iqhip_set_ascertainment(iqhip_engine *e, int64_t n_unobserved, double nsites);

/* Model side inputs (model/modelsubst.h:248-258, model/rateheterogeneity.h:95-141,
 * phylotreesse.cpp:359-529): eval[n], evec[n*n], inv_evec[n*n], rates[ncat], props[ncat],
 * tip_partial_lh[(state_unknown+1)*n]. Invalidates nothing by itself: like the reference,
 * the caller clears partial_lh_computed flags (clearAllPartialLH). */
int iqhip_set_model(iqhip_engine *e, const double *eval, const double *evec,
                    const double *inv_evec, const double *rates, const double *props,
                    int state_unknown, const double *tip_partial_lh);

/* Mixture models (computeMixturePartialLikelihoodEigenSIMD & co, phylokernelmixture.h:20-460; fused
 * mixture-rate models, phylokernelmixrate.h:22-450).  The engine's ncat categories are the (class, rate)
 * components in the reference's block order [class][rate] (block = nstates*ncat*nmixture there,
 * phylokernelmixture.h:55-56): component q uses eigen-system cat_class[q], rate rates[q] and weight
 * props[q] (= class weight x category proportion).  eval / evec / inv_evec are the nclass systems
 * concatenated (model->getEigenvalues() etc. of ModelMixture); tip_partial_lh is [state][class][n]
 * (phylotreesse.cpp:395-458, phylokernelmixture.h:151).  4, 20 and 64 states; any nclass in 1..ncat, so a 4-state engine
 * of 12 components takes MIX{JC,HKY,GTR}+G4, and plain -> mixture -> plain on one engine works (the caller invalidates all
 * vectors at a model change, as always). */
int iqhip_set_mixture_model(iqhip_engine *e, int nclass, const int32_t *cat_class /* [ncat] */,
                            const double *eval, const double *evec, const double *inv_evec,
                            const double *rates /* [ncat] */, const double *props /* [ncat] */,
                            int state_unknown, const double *tip_partial_lh);

/* Execute a post-ordered list of node updates (children before parents) in ONE submission.
 * sum_scale[k] receives op k's own sum_scale (phylokernel.h:389,471: LOG_SCALING_THRESHOLD *
 * sum of ptn_freq over the patterns rescaled at this node); the caller keeps
 * lh_scale_factor = left + right + sum_scale exactly as phylokernel.h:157,395,477. */
int iqhip_update_partials(iqhip_engine *e, const iqhip_node_op *ops, int nops,
                          double *sum_scale);

/* computeLikelihoodBranchEigenSIMD's pattern loop (phylokernel.h:779-966) on branch (a,b)
 * of length len.  At most one end may be a leaf.  *lnl = sum_ptn freq*log|lh_ptn| WITHOUT
 * the two lh_scale_factor terms (the caller adds them, phylokernel.h:751).  _pattern_lh is
 * kept on the device (iqhip_fetch_pattern_lh). */
int iqhip_branch_lnl(iqhip_engine *e, iqhip_branch_end a, iqhip_branch_end b, double len,
                     double *lnl);

/* Fused form of the reference's hot loop 1 (clearAllPartialLH(); computeLikelihood()):
 * the node updates and the branch lnL in one device pass. */
int iqhip_traverse_lnl(iqhip_engine *e, const iqhip_node_op *ops, int nops,
                       iqhip_branch_end a, iqhip_branch_end b, double len,
                       double *sum_scale, double *lnl);

/* theta_all = a .* b (phylokernel.h:535-579); kept on the device. */
int iqhip_compute_theta(iqhip_engine *e, iqhip_branch_end a, iqhip_branch_end b);
/* df, ddf at branch length len from theta (phylokernel.h:516-532,583-651). */
int iqhip_derv(iqhip_engine *e, double len, double *df, double *ddf);
/* lnL (without lh_scale_factors) from theta (phylokernel.h:1040-1122); writes _pattern_lh. */
int iqhip_lnl_from_theta(iqhip_engine *e, double len, double *lnl);

/* the whole Newton-Raphson solve of Optimization::minimizeNewton
 * (optimization.cpp:388-450) for the branch whose theta is resident, in ONE launch: the loop
 * "computeFuncDerv; update; test" of optimizeOneBranch (phylotree.cpp:2148-2192) runs on the device
 * with the reference's update rule, bracketing and stopping tests (x1/x2 = min/max branch length,
 * xacc = min branch length, max_steps = maxNRStep).  Returns the optimised length (*optx), the last
 * second derivative (*d2l, as minimizeNewton's d2l) and the number of derivative evaluations.
 * On a sharded engine every derivative evaluation needs the all-reduce of {df, ddf}, so the solve is a chain of
 * enqueued steps instead of one kernel (derivative kernel -> all-reduce -> 1-thread update kernel that applies the
 * same rule to device-resident state); the host reads the state once per few steps, not once per step. */
int iqhip_newton_branch(iqhip_engine *e, double xguess, double x1, double x2, double xacc,
                        int max_steps, double *optx, double *d2l, int *nsteps);
/* optimizeOneBranch in one submission and one host round trip: the pending node updates of both
 * ends of the branch (as iqhip_update_partials), theta (as iqhip_compute_theta) and the Newton
 * solve (as iqhip_newton_branch).  nops may be 0. */
int iqhip_optimize_branch(iqhip_engine *e, const iqhip_node_op *ops, int nops, iqhip_branch_end a,
                          iqhip_branch_end b, double xguess, double x1, double x2, double xacc,
                          int max_steps, double *sum_scale, double *optx, double *d2l, int *nsteps);

/* The same update rule as a host-side state machine (128 opaque bytes), for callers that own the collective: evaluate
 * {df, ddf} at *first_x / *next_x (iqhip_derv_async + their own all-reduce), feed the sums to _update until *done.
 * status as iqhip_branch_result.status.  No likelihood arithmetic happens in these three calls. */
#define IQHIP_NEWTON_STATE_BYTES 128
int iqhip_newton_host_init(void *state, double xguess, double x1, double x2, double xacc, int max_steps, double *first_x);
int iqhip_newton_host_update(void *state, double df_sum, double ddf_sum, double *next_x, int *done);
int iqhip_newton_host_result(const void *state, double *optx, double *d2l, int *nsteps, int *status);

/* Asynchronous use (a caller that owns the collective itself, e.g. a torch.distributed program that all-reduces a
 * tensor it bound as the result buffer; engines with a communicator and sharded engines do this internally and
 * refuse these calls).  The *_async forms enqueue the same work but leave the
 * result on the device: `iqhip_result_device_ptr` is a device array of
 * iqhip_result_capacity() doubles laid out as
 *    [0] = lnl or df, [1] = ddf, [2 .. 2+nops) = sum_scale per op
 * which the caller may all-reduce in place (ncclAllReduce / torch.distributed, SUM, f64)
 * on the engine's stream before iqhip_result_read copies it to the host. */
int iqhip_bind_result_buffer(iqhip_engine *e, void *device_ptr, int capacity_doubles);
void *iqhip_result_device_ptr(iqhip_engine *e);
int iqhip_result_capacity(iqhip_engine *e);
int iqhip_traverse_lnl_async(iqhip_engine *e, const iqhip_node_op *ops, int nops,
                             iqhip_branch_end a, iqhip_branch_end b, double len);
int iqhip_derv_async(iqhip_engine *e, double len);
int iqhip_update_partials_async(iqhip_engine *e, const iqhip_node_op *ops, int nops); /* result[2+k] = sum_scale */
int iqhip_lnl_from_theta_async(iqhip_engine *e, double len);                          /* result[0] = lnl */
int iqhip_result_read(iqhip_engine *e, double *out, int ndoubles); /* syncs the stream */
int iqhip_synchronize(iqhip_engine *e);

/* Lazy device->host views of what the reference keeps in host memory
 * (phylotree.cpp:1062,1218-1227 read scale_num and _pattern_lh on the host). */
int iqhip_fetch_scale_num(iqhip_engine *e, uint64_t key, int16_t *out /* nptn */);
int iqhip_fetch_pattern_lh(iqhip_engine *e, double *out /* nptn */);
int iqhip_fetch_partial(iqhip_engine *e, uint64_t key, double *out /* nptn*block, ref layout */);
int iqhip_fetch_theta(iqhip_engine *e, double *out /* nptn*block, ref layout */);
/* Batched branch optimisation: ntasks INDEPENDENT branches in one submission -- the NNI candidates of a tree
 * (IQTree::evaluateNNIs -> PhyloTree::getBestNNIForBran, phylotree.cpp:2873-3066, evaluates them one after the
 * other; on the device they run side by side).  Task t first runs its own node updates ops[0..nops) (they may
 * read any existing vector, must write vectors no other task touches -- the nni_partial_lh scratch buffers,
 * phylotree.cpp:2901-2924), then optimises the length of branch (a, b) as iqhip_optimize_branch does and
 * evaluates computeLikelihoodFromBuffer at the optimum.  results[t].lnl excludes the lh_scale_factor terms;
 * sum_scale receives the per-op values of all tasks, concatenated in task order.  +ASC engines included: results[t].lnl
 * then carries -nsites * log(1 - prob_const) of its own branch.
 * On a sharded engine (iqhip_create_sharded, iqhip_comm_init_rank) the tasks advance side by side as well: per Newton
 * step one derivative launch for all tasks and ONE all-reduce of 2 * ntasks doubles (chunks of 64 tasks, the same on
 * every rank); with +ASC 5 * ntasks doubles ({df, ddf, prob_const, df_const, ddf_const} per task). */
typedef struct iqhip_branch_task {
    const iqhip_node_op *ops;
    int32_t nops;
    int32_t max_steps;
    iqhip_branch_end a, b;
    double xguess, x1, x2, xacc;
} iqhip_branch_task;
typedef struct iqhip_branch_result {
    double optx, d2l, lnl;
    int32_t nsteps;
    int32_t status; /* 0 ok, 2 non-finite derivative, 3 step limit reached (optx is still the last iterate), 5 (sweeps) diverged-solve rule applied */
} iqhip_branch_result;
int iqhip_optimize_branch_batch(iqhip_engine *e, const iqhip_branch_task *tasks, int ntasks,
                                double *sum_scale /* sum of nops, may be NULL */, iqhip_branch_result *results);

/* A whole branch-length sweep in one submission: PhyloTree::optimizeAllBranches' loop `for every branch in pre-order:
 * optimizeOneBranch(node1, node2, clearLH = true, maxNRStep)` (phylotree.cpp:2252-2332, 2148-2192).  Step j runs the node
 * updates that are pending at both ends of its branch, builds theta and solves for the branch length exactly as
 * iqhip_optimize_branch does; the length of a child branch that an EARLIER step of the same sweep optimised is not known
 * to the host when the sweep is submitted, so the op refers to it by step number: len_from[2k] / len_from[2k+1] >= 0
 * replaces ops[k].left_len / right_len by the accepted length of that step (the engine reads it from device memory when
 * the op runs); -1 keeps the value in the op.  The caller lists the steps as if every step changed its branch
 * (optimizeOneBranch's clearReversePartialLh on both sides of the branch).
 * diverge_frac > 0 applies optimizeOneBranch's "newton raphson diverged, reset" rule (phylotree.cpp:2167-2176, 0.95 there)
 * inside the sweep: a result above diverge_frac * x2 is kept only if the branch lnL there is not below the lnL at
 * xguess; results[j].status = 5 reports that the rule ran.  results[j].lnl is not filled.  sum_scale receives the per-op
 * values of all steps, concatenated.  Two launches per step, one host round trip per sweep (+ASC engines included: both
 * lnL of the diverged-solve rule carry their own -nsites * log(1 - prob_const)); on sharded engines (every Newton step
 * contains an all-reduce) the steps run one after the other inside this call. */
typedef struct iqhip_sweep_step {
    const iqhip_node_op *ops;
    const int32_t *len_from; /* NULL or 2 * nops entries */
    int32_t nops;
    int32_t _pad;
    iqhip_branch_end a, b;
    double xguess; /* the branch's current length */
} iqhip_sweep_step;
int iqhip_optimize_sweep(iqhip_engine *e, const iqhip_sweep_step *steps, int nsteps, double x1, double x2, double xacc,
                         int max_steps, double diverge_frac, double *sum_scale /* sum of nops, may be NULL */,
                         iqhip_branch_result *results);

/* Consumers of the device-resident _pattern_lh (so -wsl / UFBoot need no full-vector round trip per tree).
 * iqhip_fetch_pattern_lh_scaled: PhyloTree::computePatternLikelihood (phylotree.cpp:1200-1230) for the
 *   branch (a,b) the last lnL evaluation ran on: _pattern_lh + (scale_num_a + scale_num_b)*log(2^-256).
 * iqhip_set_boot_samples: UFBoot's boot_samples (iqtree.h:670, BootValType = float), [nsamples][nptn],
 *   uploaded once.  iqhip_rell: the RELL scores of IQTree::saveCurrentTree (iqtree.cpp:2726-2736),
 *   rell[s] = dotProduct(pattern_lh, boot_samples[s]) (phylokernel.h:55-61), accumulated in double.
 *   The _async form leaves the scores in the result vector [0, nsamples) for a sharded caller to
 *   all-reduce before iqhip_result_read. */
/* _pattern_lh_cat of the reference's scalar kernels (phylotreesse.cpp:1190-1237; consumer
 * RateGamma::computePatternRates, model/rategamma.cpp:241-262): per pattern and category
 * sum_i exp(eval_i r_c len) prop_c theta[ptn][c][i] for the branch of the last iqhip_compute_theta,
 * unscaled, out[ptn*ncat + c]. */
int iqhip_pattern_lh_cat(iqhip_engine *e, double len, double *out /* nptn*ncat */);

/* EM estimation of +R free-rate weights and rates (RateFree::optimizeWithEM, model/ratefree.cpp:450-579) and empirical-Bayes
 * site rates (RateGamma::computePatternRates, model/rategamma.cpp:235-258) on the device.  With L_pc the quantity
 * iqhip_pattern_lh_cat returns for the branch of the last iqhip_compute_theta at length len:
 * iqhip_em_posteriors (the E-step): W[p][c] = ptn_freq[p] L_pc / sum_c L_pc stays on the device in an engine-owned
 *   category-major matrix; cat_sum[c] = sum_p W[p][c].  It also leaves per pattern the posterior mean rate
 *   sum_c r_c L_pc / sum_c L_pc and the best category, the FIRST maximum of L_pc (the reference breaks ties with its random
 *   number generator).
 * iqhip_em_fetch_posteriors / iqhip_em_site_rates: what the last E-step left, copied to the host.
 * iqhip_em_objective: with the rates and weights the engine holds NOW and the theta resident NOW,
 *   f[c] = sum_p W[p][c] (log(L_pc / prop_c) + (max(sc_a[p], 0) + max(sc_b[p], 0)) LOG_SCALING_THRESHOLD),
 *   sc_a / sc_b the scale counters of the branch's two ends, W the matrix of the last E-step.  f[c] is the log-likelihood of
 *   the reference's one-category tree with pattern weights W[.][c] and all lengths scaled by rates[c]
 *   (optimizeTreeLengthScaling, phylotree.cpp:2106-2133), so one traversal of the C-category engine evaluates the C
 *   objectives of the M-step at once.  A term with W == 0 contributes 0.
 *   UNDERFLOW RULE: the engine rescales a pattern only when ALL of its categories are small, so a fast category can
 *   underflow where the reference's one-category tree would have rescaled.  A term with W > 0 whose L_pc is not a positive
 *   normal number takes log(DBL_MIN) in place of the logarithm and is counted in floored[c] (NULL: not reported); callers
 *   treat a non-zero count as "this objective value is a bound, not the value".
 * All sums are formed in a fixed order without atomics: the same bits on every run.
 * Plain engines of 4, 20 or 64 states only: IQHIP_ERR_UNSUPPORTED for mixture models, sharded engines and communicator
 * ranks, +ASC (the reference switches EM off there as well) and embedded state counts; IQHIP_ERR_INVALID for a null
 * argument, theta not resident, a negative or NaN len, a weight <= 0 (objective), no E-step yet (objective, fetch, site
 * rates) and planning-only engines.
 * iqhip_debug_em_timing: with iqhip_timing_enable, ms[0] / ms[1] = the device time (HIP events, milliseconds) of the launches
 *   of the last iqhip_em_posteriors / iqhip_em_objective call (kernel plus the fold of the sums). */
int iqhip_em_posteriors(iqhip_engine *e, double len, double *cat_sum /* ncat */);
int iqhip_em_fetch_posteriors(iqhip_engine *e, double *out /* nptn*ncat, [ptn][cat] */);
int iqhip_em_site_rates(iqhip_engine *e, double *ptn_rate /* nptn */, int32_t *ptn_cat /* nptn */);
int iqhip_em_objective(iqhip_engine *e, iqhip_branch_end a, iqhip_branch_end b, double len, double *f /* ncat */,
                       int64_t *floored /* ncat or NULL */);
int iqhip_debug_em_timing(iqhip_engine *e, double *ms /* 2 */);

/* EM estimation of mixture class weights (ModelMixture::optimizeWeights, model/modelmixture.cpp:1355-1416; Wang, Li, Susko and
 * Roger 2008), per-pattern class posteriors and PhyloTree::computePatternStateFreq (phylotree.cpp:1162-1196) on the device.
 * iqhip_mix_class_lh: with L_pq the quantity iqhip_pattern_lh_cat returns for the branch of the last iqhip_compute_theta at
 *   length len, Lc[p][m] = sum of L_pq over the components q with cat_class[q] == m, in ascending q starting from the first
 *   (computePatternLhCat(WSL_MIXTURE), phylotree.cpp:1132-1143; cat_class is an arbitrary map).  The matrix stays on the
 *   device, class-major and unscaled -- every consumer below uses per-pattern ratios only; out (or NULL) receives a copy.
 * iqhip_mix_weights_em: the reference's loop on the matrix of the last iqhip_mix_class_lh, at most max_steps steps (the
 *   reference passes nclass), with no tree traversal in between.  One step, over the patterns with ptn_freq > 0:
 *     s_p = v ptn_invar[p] + sum_m g[m] Lc[p][m]    (ascending m, starting from the invariant term)
 *     new_m = (sum_p g[m] Lc[p][m] ptn_freq[p] / s_p) / nsites
 *     converged = all |w[m] - new_m| < 1e-4;   g[m] *= new_m / w[m];   w[m] = new_m;   p_invar_new = 1 - sum_m w[m]
 *   and with +I: converged &= |p_invar - p_invar_new| < 1e-4; v = p_invar_new / (the p_invar passed in); p_invar = p_invar_new.
 *   g and v start at 1.  All max_steps steps are enqueued on the engine's stream without a host read in between -- the
 *   steps behind the converged one do nothing -- and the step count, the flag, the weights and the log are read once.
 *   weights: in, the class weights inside the engine's props; out, the estimate.  trace (or NULL): row k < *nsteps =
 *   {w[0 .. nclass), p_invar} after step k, the rows behind them 0.  max_steps is at most IQHIP_MIX_MAX_STEPS: the log
 *   (max_steps rows of nclass + 1 doubles, 3 MB at 96 classes) lives on the device for the run and is read back whole.  The call changes nothing the likelihood kernels read: the caller re-sends the
 *   model (props[q] *= w_new[m] / w_old[m] through iqhip_set_mixture_model, then iqhip_set_ptn_invar) and invalidates all
 *   vectors as at any model change.
 *   +I: with p_invar != NULL and *p_invar > 0 the engine's resident ptn_invar is taken to belong to *p_invar; computePtnInvar
 *   is linear in p_invar, so the factor v is exact up to rounding.
 *   DEVIATIONS from the reference: (1) with p_invar NULL or 0 there is no +I handling (the reference would store the
 *   rounding noise of 1 - sum w as p_invar); (2) the reference rescales its matrix in place by new / old after every step,
 *   here the matrix is never rewritten and the cumulative factors g carry the product -- equal up to rounding, not in bits;
 *   (3) the random number generator of computePatternRates is not involved.
 * iqhip_mix_posteriors: post[p][m] = Lc[p][m] * (1 / sum_m Lc[p][m]) -- no invariant term, as phylotree.cpp:1174-1182 -- and,
 *   with the classes' state frequencies class_freq[m][i], state_freq[p][i] = sum_m class_freq[m][i] post[p][m].
 * All sums are formed in a fixed order without atomics, in a decomposition that follows from the pattern and class counts
 * alone: the same bits on every run and on every device.
 * Mixture engines of 4, 20 or 64 states.  IQHIP_ERR_UNSUPPORTED: one class, sharded engines and communicator ranks, +ASC
 * (the reference: "Mixture model +ASC is not supported yet"), embedded state counts.  IQHIP_ERR_INVALID: a null argument,
 * planning-only engines, theta not resident, a negative or NaN len, max_steps outside 1 .. IQHIP_MIX_MAX_STEPS, nsites <= 0, a weight <= 0 or not
 * finite, *p_invar outside [0, 1), EM or posteriors before iqhip_mix_class_lh or after the engine's model changed.
 * iqhip_debug_mix_timing: with iqhip_timing_enable, ms[0] / ms[1] = the device time (HIP events, milliseconds) of the last
 *   class-lh launch / of the last EM chain; launches (or NULL) = the kernels that chain enqueued, 2 max_steps. */
#define IQHIP_MIX_MAX_STEPS 4096
int iqhip_mix_class_lh(iqhip_engine *e, double len, double *out /* nptn*nclass [ptn][class], or NULL: device only */);
int iqhip_mix_weights_em(iqhip_engine *e, int max_steps, double nsites, double *weights /* nclass, in/out */,
                         double *p_invar /* NULL or in/out */, int *nsteps, int *converged,
                         double *trace /* NULL or max_steps*(nclass+1) */);
int iqhip_mix_posteriors(iqhip_engine *e, const double *class_freq /* nclass*nstates or NULL */,
                         double *post /* nptn*nclass or NULL */, double *state_freq /* nptn*nstates or NULL */);
int iqhip_debug_mix_timing(iqhip_engine *e, double *ms /* 2 */, int64_t *launches);
/* Per-class log-likelihoods of a mixture engine: K candidate models as the K classes of one engine (class m = candidate m:
 * its own eigen-system and tip_partial_lh slice, its components' rates and props), one traversal, K values.
 * iqhip_class_lnl reads the theta resident for the branch (a, b).  With Lc[p][m] what iqhip_mix_class_lh defines (the
 * components of class m in ascending q, the same table and the same arithmetic per component):
 *   lnl[m] = sum over p with ptn_freq[p] > 0 of
 *            ptn_freq[p] (log(Lc[p][m] / class_weight[m] + inv_m[p]) + (max(sc_a[p], 0) + max(sc_b[p], 0)) LOG_SCALING_THRESHOLD)
 *   inv_m[p] = class_invar[m][p] when the pointer is given, else the engine's resident ptn_invar[p] for every class (a
 *   stencil over substitution parameters with fixed frequencies and fixed p-inv).  This is the expression the branch lnL
 *   forms for a plain model with the two scale counters put back (as iqhip_em_objective): lnl[m] is the log-likelihood of
 *   class m's model alone on this tree.  class_weight[m] is the weight the caller folded into that class's props; it may
 *   be 1 (iqhip_set_mixture_model does not require the weights to sum to 1).
 *   UNDERFLOW RULE as iqhip_em_objective: the engine rescales a pattern only when ALL components are small.  A term whose
 *   argument is not a positive normal number takes log(DBL_MIN) and is counted in floored[m] (NULL: not reported).
 *   The nptn x nclass matrix is not written: every workgroup reduces its tile to one partial per class and a fold kernel adds
 *   the rows in a fixed order.  No atomics; the decomposition follows from the padded pattern count and nclass alone: a
 *   repeated call returns the same bits.
 * Engines whose model came through iqhip_set_mixture_model (one class is allowed), 4, 20 or 64 states, the wide 4-state
 * engines included.  IQHIP_ERR_UNSUPPORTED: a model set through iqhip_set_model, +ASC, sharded engines and communicator
 * ranks, embedded state counts.  IQHIP_ERR_INVALID: a null argument, a planning-only engine, theta not resident for that
 * branch, a negative or NaN len, a class_weight <= 0 or not finite.
 * iqhip_debug_class_lnl_timing: with iqhip_timing_enable, *ms = the device time (HIP events, milliseconds) of the two
 *   launches of the last iqhip_class_lnl call. */
int iqhip_class_lnl(iqhip_engine *e, iqhip_branch_end a, iqhip_branch_end b, double len,
                    const double *class_weight /* nclass */, const double *class_invar /* NULL or nclass*nptn, [class][ptn] */,
                    double *lnl /* nclass */, int64_t *floored /* nclass or NULL */);
int iqhip_debug_class_lnl_timing(iqhip_engine *e, double *ms);
int iqhip_fetch_pattern_lh_scaled(iqhip_engine *e, iqhip_branch_end a, iqhip_branch_end b, double *out /* nptn */);
int iqhip_set_boot_samples(iqhip_engine *e, const float *samples, int nsamples);
int iqhip_rell(iqhip_engine *e, iqhip_branch_end a, iqhip_branch_end b, double *rell /* nsamples */);
int iqhip_rell_async(iqhip_engine *e, iqhip_branch_end a, iqhip_branch_end b);
/* ---- SH-aLRT and local-bootstrap branch supports (PhyloTree::testAllBranches / testOneBranch / computeNNIPatternLh /
 * resampleLh, phylotree.cpp:3779-3809, 3984-4103) --------------------------------------------------------------------
 * The engine keeps a STORE of per-pattern log-likelihood rows on the device (nptn_pad doubles each).  A row holds exactly
 * what iqhip_fetch_pattern_lh_scaled returns for a branch at a length: the scale counters of both ends put back, 0 for
 * the unobserved +ASC patterns and the padding, the +ASC shift as there.  Rows are filled without leaving the device:
 *   iqhip_ptnlh_put_current        row <- the branch (a, b) the last lnL evaluation ran on (the current tree's row, and the
 *                                  candidates of a branch-by-branch getBestNNIForBran)
 *   iqhip_optimize_branch_batch_rows  iqhip_optimize_branch_batch, and for every task t with rows[t] >= 0 the per-pattern
 *                                  log-likelihood of its branch at results[t].optx goes to row rows[t] (the reference's
 *                                  nniMoves[cnt].ptnlh, phylotree.cpp:3019-3020).  rows == NULL: iqhip_optimize_branch_batch.
 *   iqhip_ptnlh_reserve grows the store (existing rows keep their contents), iqhip_ptnlh_fetch copies one row to the host.
 * iqhip_ptnlh_rell: the raw RELL sums R[i][s] = sum_p row(rows[i])[p] * boot_samples[s][p] for the first nsamples samples of
 *   iqhip_set_boot_samples: ONE tall-skinny fp64 product R = L W^T on the matrix cores (every distinct row is multiplied
 *   once, the sample matrix is read from HBM once), K-split over workgroups and combined in a fixed order: the same bits
 *   run to run.
 * iqhip_branch_tests: per branch b the three rows rows3[3b .. 3b+2] = {current tree, NNI 1, NNI 2} and their total
 *   log-likelihoods lh3[3b .. 3b+2] (lh_scale_factor terms included; the caller has them); the comparisons of
 *   phylotree.cpp:4018-4044 run on the device for the first max(reps_sh, reps_lbp) samples, and only nbranch result
 *   structs leave it.  Both fractions are over max(reps_sh, reps_lbp) replicates, as testOneBranch returns them.
 * DEVIATION from the reference: it draws a fresh resample per (branch, replicate); here ONE sample matrix serves every
 *   branch of a call.  Each branch's support has the same distribution, supports of different branches share their draws.
 *   A caller who wants independent draws uploads new samples and calls per branch.
 * Out of scope: sharded engines (iqhip_create_sharded) and engines with a communicator return IQHIP_ERR_UNSUPPORTED from
 *   all of these calls (iqhip_optimize_branch_batch_rows with rows == NULL excepted), planning-only engines
 *   IQHIP_ERR_INVALID; the parametric aLRT probability (Statistics_To_Probabilities) stays with the caller, who needs
 *   only alrt_stat for it. */
typedef struct iqhip_branch_support {
    double sh_alrt;   /* fraction of the max(reps_sh, reps_lbp) replicates, as testOneBranch returns it */
    double lbp;       /* local bootstrap fraction */
    double abayes;    /* 1 / (1 + exp(lh1-lh0) + exp(lh2-lh0)) */
    double alrt_stat; /* 2 * (lh0 - max(lh1, lh2)) */
} iqhip_branch_support;
int iqhip_ptnlh_reserve(iqhip_engine *e, int nrows);
int iqhip_ptnlh_put_current(iqhip_engine *e, int row, iqhip_branch_end a, iqhip_branch_end b);
int iqhip_ptnlh_fetch(iqhip_engine *e, int row, double *out /* nptn */);
int iqhip_optimize_branch_batch_rows(iqhip_engine *e, const iqhip_branch_task *tasks, int ntasks, double *sum_scale,
                                     iqhip_branch_result *results, const int32_t *rows /* ntasks or NULL */);
int iqhip_branch_tests(iqhip_engine *e, const int32_t *rows3, const double *lh3, int nbranch, int reps_sh, int reps_lbp,
                       iqhip_branch_support *out);
int iqhip_ptnlh_rell(iqhip_engine *e, const int32_t *rows, int nrows, int nsamples, double *out /* nrows*nsamples */);

/* ---- Tree topology tests: RELL-BP, KH, SH, weighted KH / SH, c-ELW and the bootstrap proportions of the AU test
 * (evaluateTrees / performAUTest, phylotesting.cpp:1916-2050, 2053-2442; options -z trees -zb N [-zw] [-au]) ------------
 * The caller fills one store row per candidate tree (iqhip_ptnlh_put_current after optimising the tree, or
 * iqhip_ptnlh_upload) and keeps the trees' total log-likelihoods; the rows stay on the device, the RELL sums are the
 * matrix-core product of iqhip_ptnlh_rell, the comparisons run per replicate on the device and a few doubles per tree
 * leave it.
 * iqhip_ptnlh_upload: host -> one store row (nptn doubles, the padding zeroed), the counterpart of iqhip_ptnlh_fetch.
 * iqhip_gen_boot_samples: draws rows [0, nsamples) of the engine's sample matrix ON THE DEVICE; it allocates the matrix
 *   as iqhip_set_boot_samples does and replaces its content, and iqhip_rell, iqhip_ptnlh_rell, iqhip_branch_tests and
 *   iqhip_tree_tests then work on the generated samples.  Row i is replicate rho = first_replicate + i; for every draw
 *   j < ndraws
 *       z = mix(mix(mix(seed + G (stream + 1)) + G (rho + 1)) + G (j + 1)),   G = 0x9E3779B97F4A7C15,
 *       mix = the splitmix64 finaliser (z ^= z >> 30, z *= 0xBF58476D1CE4E5B9, z ^= z >> 27, z *= 0x94D049BB133111EB,
 *             z ^= z >> 31), all modulo 2^64,
 *       site = mulhi64(z, nsite), nsite = sum ptn_freq; pattern = the first p whose inclusive integer prefix sum of
 *       ptn_freq exceeds site; count[pattern] += 1
 *   -- the distribution of the reference's per-site loop (alignment.cpp:2319-2350; its multinomial branch has the same).
 *   Patterns of frequency 0 (the unobserved +ASC patterns, the padding) never receive a draw.  Counts are integer
 *   atomics converted to float afterwards: the same arguments give the same matrix on every run, and generating [0, n)
 *   at once equals generating any split of it.  ptn_freq must hold non-negative integers (IQHIP_ERR_INVALID otherwise);
 *   ndraws <= 2^24 (a float holds no larger count exactly).
 * iqhip_ptnlh_diff_variance: computeLogLDiffVariance (phylotree.cpp:1390-1416) for all pairs of the row list: the
 *   weighted mean of the difference, then sum f (d - mean)^2 nsite / (nsite - 1); symmetric, diagonal 0, nsite <= 1 gives 0.
 * iqhip_tree_tests: phylotesting.cpp:2218-2411 on the first nsamples rows of the sample matrix for the trees whose rows
 *   and total log-likelihoods are given (rows may repeat; each distinct row is multiplied once).  avg_lh is summed in
 *   replicate order, so every comparison sees the reference's bits for the same sums.  epsilon is params.ufboot_epsilon
 *   of the RELL-BP tie rule (:2230-2239); its random_double() is (z >> 11) 2^-53 with z of the generator above for
 *   (tie_seed, stream 0xB9, rho = replicate, j = tree).  weighted != 0 adds the weighted KH / SH tests (:2323-2370) with
 *   weights 1 / sqrt(iqhip_ptnlh_diff_variance); otherwise wkh_pvalue = wsh_pvalue = -1.  The two 95 % confidence sets
 *   (:2248-2255, :2404-2411) are formed on the host from the returned shares; among equal shares the tree with the
 *   highest index enters first (the reference's order among equal shares is that of its quicksort).
 * iqhip_multiscale_bp: STEP 2 of performAUTest: for every scale k, nsamples replicates of ndraws = (int)round(scales[k]
 *   nsite) draws (replicates rho = 0 .. nsamples-1 of stream k of `seed`), generated, multiplied and counted chunk by
 *   chunk on the device -- no sample matrix crosses the bus; bp[k * ntrees + tid] = fraction of the replicates in which
 *   tree tid is the first with the strictly largest sum (:1974-1979).  The chunk keeps the sample matrix within 256 MB
 *   (IQHIP_BOOT_CHUNK, read per call, overrides the replicates per chunk); the K-split of the products follows from the
 *   pattern and CU counts only, so the counts do not depend on the chunk size.  The sample matrix is left with the last
 *   chunk.  STEP 3 / 4 of the AU test (the weighted-least-squares / maximum-likelihood fit of (d, c) and the normal
 *   quantiles) stay with the caller, as Statistics_To_Probabilities does for the aLRT.
 * DEVIATIONS from the reference: the resamples and the tie draws come from the counter-based generator above, not from
 *   the reference's RNG stream (as for -alrt); the AU replicates of all trees share one sample matrix, as they do there.
 * Out of scope: sharded engines and communicator ranks return IQHIP_ERR_UNSUPPORTED from all five calls, planning-only
 *   engines IQHIP_ERR_INVALID.  IQHIP_ERR_INVALID also for rows outside the store, fewer than two trees, more replicates
 *   than the matrix holds (iqhip_tree_tests) and a scale <= 0. */
typedef struct iqhip_tree_test {
    double rell_bp, kh_pvalue, sh_pvalue, wkh_pvalue, wsh_pvalue, elw_value;
    int32_t rell_confident, elw_confident;
} iqhip_tree_test;
int iqhip_ptnlh_upload(iqhip_engine *e, int row, const double *in /* nptn */);
int iqhip_gen_boot_samples(iqhip_engine *e, int nsamples, int64_t first_replicate, int64_t ndraws, uint64_t seed,
                           uint32_t stream);
int iqhip_ptnlh_diff_variance(iqhip_engine *e, const int32_t *rows, int nrows, double *var /* nrows*nrows */);
int iqhip_tree_tests(iqhip_engine *e, const int32_t *rows, const double *lh, int ntrees, int nsamples, double epsilon,
                     int weighted, uint64_t tie_seed, iqhip_tree_test *out /* ntrees */);
int iqhip_multiscale_bp(iqhip_engine *e, const int32_t *rows, int ntrees, const double *scales, int nscales, int nsamples,
                        uint64_t seed, double *bp /* nscales*ntrees, bp[k*ntrees+tid] */);

/* ---- Ultrafast bootstrap: the online RELL bookkeeping per candidate tree (IQTree::saveCurrentTree, iqtree.cpp:2676-2786;
 * option -bb) -----------------------------------------------------------------------------------------------------------
 * The reference calls saveCurrentTree for the current tree of every search iteration (iqtree.cpp:2135-2136) and for every
 * NNI candidate getBestNNIForBran evaluates (phylotree.cpp:3022-3023): the tree's RELL score in every replicate is compared
 * with the best score that replicate has seen, and the replicate's tree is replaced under an epsilon / random-tie rule.
 * Here the per-replicate state lives on the device next to the sample matrix and the store rows; a call applies a whole
 * list of candidate trees and only a few words leave the device.
 * iqhip_ufboot_init: engine-owned state for the first nsamples rows of the sample matrix, started as iqtree.cpp:308-312:
 *   boot_logl = boot_orig_logl = -DBL_MAX, boot_counts = 0, boot_tree = -1.  A second init resets the state.  Replacing
 *   the sample matrix (iqhip_set_boot_samples, iqhip_gen_boot_samples, iqhip_multiscale_bp) invalidates it: update and
 *   fetch return IQHIP_ERR_INVALID until the next init.
 * iqhip_ufboot_update: one entry = one saveCurrentTree(cur_logl): row = the store row with the tree's per-pattern lnL,
 *   logl = cur_logl, rand = the ONE random_double() the reference draws per call and shares over all replicates (in
 *   [0, 1]), tree_id >= 0 = the caller's tag for the tree string.  Entries with logl_cutoff != 0 && logl < logl_cutoff - 1.0
 *   are dropped on the host (:2678).  The others are applied IN LIST ORDER; for every replicate s < nsamples, with
 *   rell = R[row][s] of iqhip_ptnlh_rell (:2738-2750):
 *       better = rell > boot_logl[s] + epsilon
 *       if (!better && rell > boot_logl[s] - epsilon) better = (rand <= 1.0 / (boot_counts[s] + 1))
 *       if (better) {
 *           if (rell <= boot_logl[s] + epsilon) boot_counts[s]++; else boot_counts[s] = 1;
 *           boot_logl[s] = max(boot_logl[s], rell); boot_orig_logl[s] = logl; boot_tree[s] = tree_id;
 *       }
 *   counts (or NULL) = {entries applied, entries dropped by the cutoff, replicate slots replaced}; *min_orig_logl (or NULL)
 *   = the minimum of boot_orig_logl over the replicates that hold a tree, DBL_MAX when none does -- the reference's next
 *   logl_cutoff (iqtree.cpp:1888).  Both come back in one small read; the sums never leave the device.
 *   The list is processed in chunks of consecutive entries so that the product's staging stays within 256 MB
 *   (IQHIP_UFBOOT_CHUNK, read per call, overrides the entries per chunk).  A sum depends on its row, its sample, the
 *   padded pattern count, nsamples and the CU count only, so the state after a call is bit-identical for every chunk size
 *   and to the rule applied to iqhip_ptnlh_rell(rows, nsamples) at the same nsamples.
 * iqhip_ufboot_fetch: the state, nsamples entries each (any pointer may be NULL).
 * iqhip_debug_ufboot_timing: *launches = the kernels the last update enqueued; with iqhip_timing_enable, ms[0] / ms[1] =
 *   the device time (HIP events, milliseconds) of its products / of its update kernels.
 * DEVIATION from the reference: it is built with BOOT_VAL_FLOAT -- the pattern lnL is cast to float and the dot product
 *   runs in float.  Here the rows stay fp64 and the product is fp64, as for -alrt and the topology tests; epsilon
 *   (params.ufboot_epsilon, 0.5 by default) is many orders of magnitude above the difference.  The tie draws are the
 *   caller's; they do not follow the reference's RNG stream.
 * IQHIP_ERR_UNSUPPORTED: sharded engines and communicator ranks.  IQHIP_ERR_INVALID: planning-only engines; init with
 *   nsamples < 1 or above the number of uploaded samples; a null `trees`, ntrees < 1, a row outside the store, tree_id < 0,
 *   rand outside [0, 1] or NaN, a non-finite logl, epsilon < 0 or NaN, any call before init.  Everything is validated on
 *   the host before the first launch. */
typedef struct iqhip_ufboot_tree {
    int32_t row, _pad;
    int64_t tree_id;
    double logl, rand;
} iqhip_ufboot_tree; /* 32 bytes */
int iqhip_ufboot_init(iqhip_engine *e, int nsamples);
int iqhip_ufboot_update(iqhip_engine *e, const iqhip_ufboot_tree *trees, int ntrees, double epsilon, double logl_cutoff,
                        int64_t *counts /* 3 or NULL */, double *min_orig_logl /* or NULL */);
int iqhip_ufboot_fetch(iqhip_engine *e, double *boot_logl, double *boot_orig_logl, int32_t *boot_counts, int64_t *boot_tree);
int iqhip_debug_ufboot_timing(iqhip_engine *e, double *ms /* 2: product, update */, int64_t *launches);

/* ---- Pairwise maximum-likelihood distances (PhyloTree::computeDist, phylotree.cpp:2432-2541; per pair AlignmentPairwise,
 * alignmentpairwise.cpp:29-312, and Optimization::minimizeNewton) -- the likelihood computation the reference runs before
 * a tree exists; the matrix feeds BIONJ and is written as .mldist.  Everything it needs is resident in any engine: the state
 * rows and ptn_freq of iqhip_set_alignment, the eigen-system, rates and proportions of iqhip_set_model.
 * iqhip_pair_counts: AlignmentPairwise's constructor: counts[k*n*n + a*n + b] = sum of ptn_freq over the patterns where taxon
 *   pairs[2k] shows state a and taxon pairs[2k+1] shows state b, a, b < nstates (n = nstates).  Patterns where either state
 *   is >= nstates (ambiguity codes, gaps, STATE_UNKNOWN) are skipped -- addPattern returns before its ambiguity branch
 *   (alignmentpairwise.cpp:68-79).  Integer-valued frequencies give exact counts, the same bits on every run.
 * iqhip_pair_distances: PhyloTree::computeDist(dist_mat, var_mat) for all pairs in one submission.  init: ntaxa*ntaxa initial
 *   distances or NULL; an entry of 0 (or NULL) means "start from the JC distance of the pair" (Alignment::computeJCDist,
 *   alignment.cpp:2552-2584, MAX_GENETIC_DIST = 9 when there is no overlap or the correction diverges), as
 *   phylotree.cpp:2434-2439.  dist: ntaxa*ntaxa, symmetric, diagonal 0.  d2l: NULL or ntaxa*ntaxa, minimizeNewton's d2l per
 *   pair (symmetric, diagonal 0), from which the caller forms var_mat for its ls_var_type (phylotree.cpp:2505-2514).
 *   nsteps: NULL or ntaxa*ntaxa derivative evaluations per pair.  The reference calls minimizeNewton with x1 = xacc =
 *   min_branch_length, x2 = MAX_GENETIC_DIST and max_steps = 100; a pair with no overlapping characters then returns 9 after
 *   one evaluation (f = df = 0).  The update rule, bracketing, stopping tests and d2l are those of iqhip_newton_branch; a
 *   pair that ends in one of minimizeNewton's two errors makes the call return IQHIP_ERR_INVALID with the matrices filled.
 *   The function of a pair is computeFuncDerv's default branch (alignmentpairwise.cpp:253-279) over computeTransDerv
 *   (modelgtr.cpp:301-338): per category c, e_k = exp(t rates[c] eval[k]), P_ij = sum_k evec[i,k] inv_evec[k,j] e_k, P' and
 *   P'' with one and two more factors eval[k]; a negative P_ij becomes 0 (the derivatives are left as they are);
 *   S = sum_c props[c] P, S' = sum_c props[c] rates[c] P', S'' = sum_c props[c] rates[c]^2 P''; over the cells with
 *   count > 0 and S_ij > 0: df = -sum count S'/S, ddf = -sum count (S''/S - (S'/S)^2).  The invariant-site term is not part
 *   of the function, as in the reference.
 * DEVIATION from the reference: it adds the categories unweighted.  S'/S and S''/S do not change under a common factor, so
 *   with equal proportions (with or without +I) this is the reference's function; with unequal proportions (+R) it is the
 *   weighted form the model means.
 * Supported: plain engines of 4, 20 and 64 states with any category count the engine accepts (the 9..32-category DNA engines
 *   included) and +ASC engines (the unobserved patterns carry frequency 0).  IQHIP_ERR_UNSUPPORTED: mixture models, sharded
 *   engines and communicator ranks, embedded state counts.  IQHIP_ERR_INVALID: planning-only engines, a call before the
 *   alignment or the model is set, pair indices outside [0, ntaxa), x1 > x2, max_steps < 1.
 *   Without a GPU there is no engine to call them on: iqhip_create returns IQHIP_ERR_NO_DEVICE, as for every compute call.
 * The pairs are processed in chunks whose counts fit 64 MB (IQHIP_PAIR_CHUNK, read per call, overrides the pairs per
 *   chunk); a chunk is counted and solved before the next one overwrites its counts, and no result depends on the chunking.
 * iqhip_debug_pair_timing: with iqhip_timing_enable, the device time (HIP events, milliseconds) the last
 *   iqhip_pair_distances call spent in its count launches and in its solve launches. */
int iqhip_pair_counts(iqhip_engine *e, const int32_t *pairs /* 2*npairs */, int npairs, double *counts);
int iqhip_pair_distances(iqhip_engine *e, const double *init, double x1, double x2, double xacc, int max_steps,
                         double *dist, double *d2l, int32_t *nsteps);
int iqhip_debug_pair_timing(iqhip_engine *e, double *counts_ms, double *solve_ms);

/* ---- Likelihood mapping (-lmap; PhyloTree::computeQuartetLikelihoods, quartet.cpp:676-1152): for every quartet (a, b, c, d)
 * of taxa the maximised log-likelihoods of its three trees, from what is resident in any plain 4-state engine: the state
 * rows and ptn_freq of iqhip_set_alignment, the eigen-system, rates, proportions and tip rows of iqhip_set_model.
 * quartets: 4 * nq taxon ids, four distinct ones per quartet, in the caller's order (never sorted).
 * iqhip_quartet_cells: the quartet's columns collapsed.  cells[q * 256 + ((s0 * 4 + s1) * 4 + s2) * 4 + s3] = the sum of
 *   ptn_freq over the patterns that show the unambiguous states (s0, s1, s2, s3) in the four taxa; nother[q] = the number of
 *   all other patterns with a frequency > 0 (an ambiguity code, a gap or STATE_UNKNOWN among the four states).  This is what
 *   the reference gets by re-compressing the sub-alignment (extractSubAlignment, alignment.cpp:1892-1935).  Integer-valued
 *   frequencies give exact sums, the same bits on every run.
 * iqhip_quartet_likelihoods: per quartet and topology k = 0, 1, 2 the tree (p0, p1, (p2, p3)) with p_j = quartet[qc[4 k + j]],
 *   qc = {0,1,2,3, 0,2,1,3, 0,3,1,2} (quartet.cpp:925), i.e. 12|34, 13|24, 14|23.  Its five branches are numbered
 *     0 .. 3 = the pendant branch of p0 .. p3, 4 = the internal branch;
 *   len[k][j] is the optimised length of branch j.
 *   Starting lengths: fixNegativeBranch(true) (phylotree.cpp:2654-2694): Fitch on the four leaves over the parsimony-
 *     informative columns (Alignment::isInformative on the four states: an ambiguity code counts towards every state it allows,
 *     STATE_UNKNOWN towards none; in Fitch an ambiguity code is its set of states and STATE_UNKNOWN the full set),
 *     branch_subst = the weighted number of columns whose two Fitch sets across the branch are disjoint, length =
 *     (branch_subst > 0 ? branch_subst : 1) / nsite with nsite = the sum of ALL pattern frequencies of the engine, then the JC
 *     correction -log(1 - z length) / z, z = 4/3, where its argument is positive, and the lower bound x1.
 *   optimizeAllBranches(iterations, tolerance) (phylotree.cpp:2252-2332): the initial lnL on branch 2; up to `iterations`
 *     sweeps over the branches in the TRAVERSAL TABLE order {2, 3, 4, 0, 1} -- computeBestTraversal for the Newick string
 *     above: the farthest leaf from p0 is p2, the pre-order from p2 takes neighbours by ascending edge-count height, so p2's
 *     own branch, p3's, the internal one, then p0's and p1's; it depends on neither the lengths nor the data.  Per branch
 *     optimizeOneBranch: minimizeNewton(x1, current, x2, xacc, max_steps) with the update rule of iqhip_newton_branch, then
 *     the diverged-solve rule: optx > diverge_frac * x2 keeps the better of the lnL at optx and at the old length.  After a
 *     sweep the lnL on the last branch (1); a lnL below the previous one restores the lengths saved before the sweep and
 *     returns the lnL recomputed there (on branch 2); old <= new <= old + tolerance stops.  nsweeps = sweeps run, neval =
 *     derivative evaluations of all its solves, status = 0 or minimizeNewton's error (2 non-finite derivative, 3 step limit)
 *     of the first solve that hit one -- the call then returns IQHIP_ERR_INVALID with the results filled.
 *   The function is the engine's (K1-K9 on four leaves): per category the cherry vectors U^-1 ((E tip) o (E tip)), for a
 *     pendant branch the far side U^-1 ((E tip) o (E_uv partial)), lh = invar + sum_c prop_c sum_i exp(eval_i rate_c t) theta_i,
 *     lnL = sum w log|lh|, df and ddf as phylokernel.h:599-646.  A leaf of STATE_UNKNOWN contributes exactly 1.0 (the K2 rule).
 *     No scaling: with four leaves and lengths in [1e-6, 100] no vector gets near 2^-256.
 *   const_invar: NULL (no +I) or 5 values, p_inv * pi[x] for x < 4 and [4] = p_inv.  The invariant term of a column follows
 *     Alignment::computeConst on its four states: the states allowed by all four; exactly one common state x gives
 *     const_invar[x], all four (a column of STATE_UNKNOWN only) const_invar[4], anything else 0.
 * Supported: plain 4-state engines (iqhip_set_model) with any category count they accept, +G and +R alike.
 *   IQHIP_ERR_UNSUPPORTED: 20- and 64-state engines, embedded state counts, mixtures, +ASC, sharded engines and communicator
 *   ranks.  IQHIP_ERR_INVALID: planning-only engines, a call before the alignment or the model is set, null arguments, nq < 1,
 *   a taxon outside [0, ntaxa) or twice in a quartet, x1 > x2, max_steps < 1, iterations < 1, tolerance < 0 or NaN, a pattern
 *   frequency that is not a non-negative integer below 2^53.  Everything is validated on the host before the first launch.
 * The quartets run in chunks whose cell tables and other-lists (nptn entries each, the worst case) fit 64 MB;
 *   IQHIP_QUARTET_CHUNK (read per call) overrides the quartets per chunk.  No result depends on the chunking.
 * iqhip_debug_quartet_timing: with iqhip_timing_enable, the device time (HIP events, milliseconds) the last
 *   iqhip_quartet_likelihoods call spent in its cell launches and in its solve launches. */
typedef struct iqhip_quartet_result {   /* per quartet */
    double  logl[3];        /* topology k = 0,1,2: 12|34, 13|24, 14|23 in quartet order */
    double  len[3][5];      /* optimised lengths, branch numbers as above */
    int32_t nsweeps[3], neval[3], status[3], _pad;
} iqhip_quartet_result; /* 184 bytes */
int iqhip_quartet_cells(iqhip_engine *e, const int32_t *quartets /* 4*nq */, int nq,
                        double *cells /* nq*256 */, int32_t *nother /* nq */);
int iqhip_quartet_likelihoods(iqhip_engine *e, const int32_t *quartets, int nq,
                              const double *const_invar /* 5 or NULL: p_inv*pi[x], x<4; [4] = p_inv */,
                              double x1, double x2, double xacc, int max_steps, double diverge_frac,
                              int iterations, double tolerance, iqhip_quartet_result *results);
int iqhip_debug_quartet_timing(iqhip_engine *e, double *cells_ms, double *solve_ms);

/* ---- BIONJ (PhyloTree::computeBioNJ, phylotree.cpp:2619-2635; BioNj::create, bionj.h) -- the tree the reference builds from
 * the distance matrix above before any search.  The engine supplies the device and the stream only: n is free and need not
 * be the engine's taxon count, and no model or alignment has to be set.
 * All arithmetic is fp64, indices are 0-based, A is the set of active rows and r = |A|.
 *   Initialisation: D_ij = (dist[i][j] + dist[j][i]) / 2, the diagonal is ignored.  V = var symmetrised the same way, or
 *     V = D when var is NULL (the reference reads both from the same file, so V = D is its behaviour).
 *   While r > 3:
 *     S_i = sum over j in A, j != i of D_ij                                  (recomputed every step, Compute_sums_Sx)
 *     Q_xy = (r - 2) D_xy - S_x - S_y for active x > y;  m = min Q
 *     (a, b) = the first pair, in the reference's scan order (x ascending, then y < x ascending), with Q_xy <= m + 1e-6;
 *       hence a > b
 *     vab = V_ab;  la = 0.5 (D_ab + (S_a - S_b) / (r - 2));  lb = 0.5 (D_ab + (S_b - S_a) / (r - 2))
 *     lambda = 0.5 if vab == 0, else 0.5 + sum over i in A \ {a, b} of (V_bi - V_ai) / (2 (r - 2) vab), clamped to [0, 1]
 *     for i in A \ {a, b}:  D_ai <- lambda (D_ai - la) + (1 - lambda) (D_bi - lb)
 *                           V_ai <- lambda V_ai + (1 - lambda) V_bi - lambda (1 - lambda) vab
 *     steps[k] = {a, b, la, lb, lambda}; b leaves A; r <- r - 1
 *   Finish: the three rows left are last[0] < last[1] < last[2] = l0, l1, l2 with the lengths
 *     last_len = {0.5 (D_01 + D_02 - D_12), 0.5 (D_10 + D_12 - D_02), 0.5 (D_21 + D_20 - D_10)}.
 *   The tree: merging b into a makes sub[a] = "(" sub[a] ":" la "," sub[b] ":" lb ")"; the end is
 *     "(" sub[l0] ":" .. "," sub[l1] ":" .. "," sub[l2] ":" .. ");" (iqhost_bionj_newick of the host mirror writes it).
 * DEVIATION from the reference: Best_pair (bionj.h:426-452) keeps a running minimum and replaces it only when
 *   Q < Qmin - 1e-6, a serial, order-dependent rule.  Its state is 1e300 until the scan reaches the first pair within 1e-6 of
 *   m; it accepts that pair and can accept nothing after it unless some Q lies in (m + 1e-6, m + 2e-6] -- so the rule above
 *   picks the same pair whenever no Q lies in that interval.  Unlike a bare arg-min it does not depend on the summation
 *   order when pairs tie exactly in exact arithmetic (duplicate sequences, star-like data).  The reference computes in
 *   float; which of several exactly tied pairs it merges first is decided by its rounding noise, so compare split sets with
 *   their lengths, never Newick strings.
 * Negative lengths are returned as they come (the reference prints them too).  The same input gives the same bits on every
 *   run: no floating-point atomics, every sum in a fixed order, the kernels are built without contraction.
 * The whole merge loop is enqueued on the engine's stream without a host read in between (four launches per step: row
 *   minima of Q, the pick with la / lb / lambda and the log entry, the update of row and column a, the row sums); the host
 *   reads the log once.  D, V and a staging matrix (3 n^2 doubles) are allocated per call and freed before it returns.
 * IQHIP_ERR_INVALID: n < 3, a NULL dist / last / last_len, NULL steps with n > 3, a non-finite off-diagonal entry of dist or
 *   var, a planning-only engine.  IQHIP_ERR_UNSUPPORTED: sharded engines and communicator ranks; n > 65536 (the pairs no
 *   longer fit a 32-bit index).  IQHIP_ERR_NOMEM: the three matrices do not fit.  n == 3 runs no merge and returns the
 *   finish only.
 * iqhip_debug_bionj_timing: *launches = the kernel launches of the last iqhip_bionj call; with iqhip_timing_enable, *ms =
 *   the device time (HIP events, milliseconds) from its first launch to its last (otherwise 0). */
typedef struct iqhip_bionj_step { int32_t a, b; double la, lb, lambda; } iqhip_bionj_step;   /* 32 bytes */
int iqhip_bionj(iqhip_engine *e, int n, const double *dist /* n*n */, const double *var /* n*n or NULL */,
                iqhip_bionj_step *steps /* n-3 */, int32_t *last /* 3 */, double *last_len /* 3 */);
int iqhip_debug_bionj_timing(iqhip_engine *e, double *ms, int64_t *launches);

/* ---- Fitch parsimony (PhyloTree::setParsimonyKernel, phylotreesse.cpp:34-61: computePartialParsimonyPointer and
 * computeParsimonyBranchPointer, the bit-parallel kernels of phylotreepars.cpp:18-282) -- what the reference runs before a
 * tree exists to build its stepwise-addition starting trees (computeParsimonyTree, phylotreepars.cpp:309-426) and, through
 * fixNegativeBranch(true) (phylotree.cpp:2654-2694), the first branch lengths.  Everything is integer arithmetic; every
 * result is exact.  The state lives in a plain engine and is built from the state rows and ptn_freq of
 * iqhip_set_alignment and the tip table and eigenvectors of iqhip_set_model.
 * iqhip_pars_init: lays out the sites and writes the tip vectors (phylotreepars.cpp:39-146).  Pattern p contributes
 *   ptn_freq[p] consecutive sites when informative[p] != 0 (NULL: every pattern), in pattern order; frequencies must be
 *   non-negative integers (IQHIP_ERR_INVALID otherwise), frequency 0 -- the unobserved +ASC patterns -- contributes
 *   nothing.  The reference first sorts the informative patterns by their number of characters (orderPatternByNumChars);
 *   all scores are sums over sites, so the order changes no result and is not reproduced.  *nsites = the site count;
 *   nwords = ceil(nsites / 32), at least 1.  Bit-plane i of a taxon's site is set exactly when its state code allows state i:
 *   the indicator of a code is recovered from the engine's tip table row, which is in eigen-space (U^-1 times the
 *   indicator), as round(U * row) -- the DNA codes 4..17 give the mask `state - 3`, B/Z/J the ambi_aa pairs,
 *   STATE_UNKNOWN every plane, without a sequence-type switch.  The padding bits of the last word get plane 0 at every
 *   tip (the reference's dummy states, :74-75) and can never score.
 *   Slots 0 .. ntaxa-1 are the tip vectors, slots ntaxa .. ntaxa+nvectors-1 the caller's (the reference's arena holds
 *   4 * (ntaxa - 1) blocks, phylotree.cpp:601).  A vector is nwords * nstates words plus its subtree score, kept as one
 *   uint32 per word column (x_score[w] + y_score[w] + popcount(w)), so that an update needs no reduction.
 * iqhip_pars_update: the node update of phylotreepars.cpp:169-211 for a whole op list, in one launch at any tree depth
 *   (the ops are levelled on the host; a column of a vector depends on the same column of its children only).  Checked
 *   on the host before anything is launched: every slot in range, dst not a tip slot and not one of its own children, no
 *   slot written twice in a call, every slot read a tip or written by an earlier op of the call or by an earlier call
 *   (one valid flag per slot), no slot read by an op and written by a later one.  IQHIP_ERR_INVALID otherwise.
 * iqhip_pars_branch_scores: computeParsimonyBranchFast (:218-282) for nbranch branches, ends[2b], ends[2b+1] = the slots
 *   of the two directed vectors of branch b: score = sum_w (a_score[w] + c_score[w] + popcount(~OR_i(a_i & c_i))),
 *   subst = the popcount part.  The reference's early exit at a lower bound (:251) truncates only scores that lose anyway;
 *   full scores are returned here.
 * iqhip_pars_insert_scores: the scan of one stepwise-addition step (addTaxonMPFast, :428-465): for branch (a, c) and tip
 *   slot `taxon`, m = fitch(a, c) in registers, score = sum_w (a_score + c_score + popcount(w_ac) + popcount(~OR_i(m_i & t_i)))
 *   -- the score of the tree with the taxon inserted into that branch.  *best = the FIRST minimum in list order (the
 *   reference accepts a candidate on score < best_pars_score only, :371), *best_score its score; score: NULL or nbranch.
 * iqhip_pars_shape: what the last iqhip_pars_init laid out: the site count, nwords and nvectors (any of them may be NULL).
 * iqhip_pars_fetch: a vector in the reference's layout, out[w * nstates + i], and out[nwords * nstates] = its subtree score.
 * iqhip_debug_pars_levels: iqhip_pars_update's validation and level assignment alone (no engine, no device): valid[k] != 0
 *   means slot ntaxa + k was written by an earlier call (NULL: none); level[k] = 0 for an op whose children are tips or
 *   earlier calls' vectors, else 1 + the larger level of the ops that write its children.
 * iqhip_set_alignment and iqhip_set_ptn_freq after iqhip_pars_init invalidate the parsimony state: the later calls return
 *   IQHIP_ERR_INVALID until the next iqhip_pars_init, which also resets the valid flags.
 * IQHIP_ERR_UNSUPPORTED: sharded engines and communicator ranks, embedded state counts (anything but 4, 20, 64).
 * IQHIP_ERR_INVALID: planning-only engines, init before the alignment or the model is set, every other call before init,
 *   nvectors < 0, nbranch < 1, `taxon` not a tip slot.  Mixture engines are accepted (class 0's tip table is read).
 * iqhip_debug_pars_timing: since the last reset, ms[0] / ms[1] = the device time (HIP events, milliseconds; counted while
 *   iqhip_timing_enable is on) of the iqhip_pars_update launches / of the iqhip_pars_insert_scores launches, and counts =
 *   {update launches, scan launches (scores + first minimum), ops updated, branches scanned}.
 * iqhip_pars_insert_scores_batch: one stepwise-addition step of MANY trees that share one arena (the reference builds its
 *   100 starting trees under "#pragma omp parallel for", iqtree.cpp:591-601; here tree k's step s is segment k of one call).
 *   The branches [seg_start[g], seg_start[g + 1]) of `ends` form segment g and are scored against the tip slot taxon[g] with
 *   exactly iqhip_pars_insert_scores' formula; best[g] = the FIRST minimum of segment g in list order as an index WITHIN the
 *   segment, best_score[g] that minimum; score: NULL or seg_start[nseg] entries -- without it 2 * nseg integers come back.
 *   Two launches per call (scores, then one workgroup per segment for the minima), no atomics, a fixed order: every run gives
 *   the same bits.  Two routes over one scoring function, chosen from nwords alone: a wave per branch (four branches per
 *   workgroup) while nwords <= 256, a workgroup per branch above; the threshold has NOT been measured.
 *   IQHIP_PARS_BATCH_ROUTE = wave | wg, read per call, forces a route; any other word is IQHIP_ERR_INVALID.
 *   IQHIP_ERR_INVALID, before anything is launched: a null argument (all but `score`), nseg < 1, seg_start[0] != 0,
 *   seg_start not strictly increasing (an empty segment), a slot out of range or never written, a taxon[g] that is not a
 *   tip slot.  Engines are refused as by the other iqhip_pars_* calls.
 * iqhip_debug_pars_batch_timing: since the last reset, *ms = the device time of the batch scans (while iqhip_timing_enable
 *   is on), counts = {launches, branches, segments}.  The counters of iqhip_debug_pars_timing do not count batch calls. */
typedef struct iqhip_pars_op { int32_t dst, left, right, _pad; } iqhip_pars_op; /* slots */
int iqhip_pars_init(iqhip_engine *e, const uint8_t *informative /* nptn or NULL */, int nvectors, int64_t *nsites);
int iqhip_pars_update(iqhip_engine *e, const iqhip_pars_op *ops, int nops);
int iqhip_pars_branch_scores(iqhip_engine *e, const int32_t *ends /* 2*nbranch slots */, int nbranch, int32_t *score,
                             int32_t *subst /* either may be NULL */);
int iqhip_pars_insert_scores(iqhip_engine *e, const int32_t *ends, int nbranch, int32_t taxon,
                             int32_t *score /* nbranch or NULL */, int32_t *best, int32_t *best_score);
int iqhip_pars_shape(iqhip_engine *e, int64_t *nsites, int64_t *nwords, int *nvectors);
int iqhip_pars_fetch(iqhip_engine *e, int32_t slot, uint32_t *out /* nwords*nstates + 1 */);
int iqhip_debug_pars_levels(int ntaxa, int nvectors, const uint8_t *valid /* nvectors or NULL */, const iqhip_pars_op *ops,
                            int nops, int32_t *level);
int iqhip_debug_pars_timing(iqhip_engine *e, double *ms /* 2 */, int64_t *counts /* 4 */, int reset);
int iqhip_pars_insert_scores_batch(iqhip_engine *e, const int32_t *ends /* 2*nbranch slots */,
                                   const int32_t *seg_start /* nseg+1, seg_start[nseg] = nbranch */, int nseg,
                                   const int32_t *taxon /* nseg tip slots */, int32_t *score /* nbranch or NULL */,
                                   int32_t *best /* nseg */, int32_t *best_score /* nseg */);
int iqhip_debug_pars_batch_timing(iqhip_engine *e, double *ms /* 1 */, int64_t *counts /* 3: launches, branches, segments */,
                                  int reset);

/* ---- Parsimony SPR scan (the scan inside pllComputeRandomizedStepwiseAdditionParsimonyTree's SPR rounds,
 * pll/fastDNAparsimony.c:1169-1427 rearrangeParsimony / addTraverseParsimony / testInsertParsimony): the score of every
 * regraft position within a radius, for many prune points, in ONE launch over the vectors that iqhip_pars_update left.
 *
 * A job is one prune point: `subtree` = the slot of the pruned subtree's directed vector S, and nsteps steps from
 * steps[first_step] in depth-first pre-order.  Step k of a job (parent is relative to the job):
 *   U_k = V(side)                         when parent < 0 (depth 0: the far end of the branch the pruning merged)
 *   U_k = fitch(U_parent, V(side))        otherwise (depth = the parent's + 1), score column U_parent + V(side) + popcount(cost)
 *   score_k = sum_w (U_k.score + V(target).score + S.score + popcount(w(U_k, V(target))) + popcount(~OR_i(m_i & S_i))),
 *             m = fitch(U_k, V(target)), unless flags has IQHIP_PARS_SPR_NO_SCORE
 * -- iqhip_pars_insert_scores' formula with a subtree in the place of the tip, plus the subtree's own score: the exact Fitch
 * length of the tree with S regrafted into that branch.  U_k is, in the pruned tree, the directed vector of everything on
 * the prune-point side of the target branch; V(side) and V(target) are vectors of the unpruned tree that do not contain S
 * and are read as stored.  The parent of a step must be the MOST RECENT earlier step of the job one level up, so that a
 * stack indexed by depth holds every U that is still needed; depth <= IQHIP_PARS_SPR_MAX_RADIUS.  The U never leave the
 * chip: only scores are written.
 * score (nsteps or NULL): -1 at NO_SCORE steps and at steps that belong to no job.  best_step[j] / best_score[j]: the
 * FIRST minimum over job j's scored steps in step order, as an index within the job (-1 and INT32_MAX when none is
 * scored).  *best_job: the first job in job order that holds the global minimum (-1 when nothing is scored).  All sums are
 * integer, so the results are exact and the same on every run.
 * iqhip_debug_pars_spr_check: the validation that iqhip_pars_spr_scan runs before it launches anything, alone (no engine,
 *   no device): every slot in [0, ntaxa + nvectors) and a tip or marked valid; the step ranges of the jobs inside
 *   [0, nsteps) and disjoint; 0 <= parent < k or parent < 0, the stack rule, the depth bound; no unknown flag.  depth:
 *   nsteps entries or NULL (-1 at steps of no job).
 * njobs == 0 succeeds and launches nothing.  Refusals as for the other iqhip_pars_* calls; anything the check finds is
 *   IQHIP_ERR_INVALID.
 * iqhip_debug_pars_spr_timing: since the last reset, *ms = the device time of the scan launches (while iqhip_timing_enable
 *   is on), counts = {launches, steps scored}. */
enum { IQHIP_PARS_SPR_NO_SCORE = 1 };
#define IQHIP_PARS_SPR_MAX_RADIUS 10
typedef struct iqhip_pars_spr_step { int32_t parent, side, target, flags; } iqhip_pars_spr_step;
typedef struct iqhip_pars_spr_job { int32_t subtree, first_step, nsteps, _pad; } iqhip_pars_spr_job;
int iqhip_pars_spr_scan(iqhip_engine *e, const iqhip_pars_spr_job *jobs, int njobs, const iqhip_pars_spr_step *steps,
                        int nsteps, int32_t *score /* nsteps or NULL */, int32_t *best_step /* njobs */,
                        int32_t *best_score /* njobs */, int32_t *best_job);
int iqhip_debug_pars_spr_check(int ntaxa, int nvectors, const uint8_t *valid /* nvectors or NULL */,
                               const iqhip_pars_spr_job *jobs, int njobs, const iqhip_pars_spr_step *steps, int nsteps,
                               int32_t *depth /* nsteps or NULL */);
int iqhip_debug_pars_spr_timing(iqhip_engine *e, double *ms /* 1 */, int64_t *counts /* 2 */, int reset);

/* Host -> device (tests; SPR/NNI code that fills a buffer on the host). */
int iqhip_upload_partial(iqhip_engine *e, uint64_t key, const double *partial_lh,
                         const int16_t *scale_num);

/* Measurement hook for bench.py: average device time (ms) per launch of the traversal kernel over the
 * launches since the last reset (a staged plan is two launches per traversal), measured with HIP
 * events on the engine's stream. */
int iqhip_timing_enable(iqhip_engine *e, int on);
int iqhip_timing_read(iqhip_engine *e, double *avg_ms, int64_t *launches, int reset);
/* Bytes the traversal launches of the LAST submission store to / load from global memory, derived from its device
 * descriptors (result vectors + counters; children that are neither register-resident nor parked; leaf state rows; the
 * root-branch pass).  `stored` is exact; `loaded` is an upper bound of the fabric reads (same-launch re-reads may hit
 * the L2 / Infinity Cache).  bench.py prices a launch with it when no PMC pass of the shape is on file. */
int iqhip_timing_plan_bytes(iqhip_engine *e, double *stored, double *loaded);
/* Engines with a communicator (iqhip_comm_init_rank): average duration in microseconds of the engine's own all-reduces
 * since the last reset, HIP events on its stream around each ncclAllReduce while timing is enabled -- from the moment the
 * stream reaches the collective to its completion, i.e. including the wait for slower ranks. */
int iqhip_timing_collective_read(iqhip_engine *e, double *avg_us, int64_t *count, int reset);

/* Cherry tables (20 states x 4 categories, >= 8192 patterns; IQHIP_CHERRY_TABLES=0 switches them off): a node whose two
 * children are leaves (computePartialLikelihood's leaf-leaf case, phylokernel.h:187-260) takes one of (STATE_UNKNOWN+1)^2
 * values per pattern, so the engine computes that table once per (pair of taxa, pendant lengths, model) -- with the same
 * kernels on a pseudo-alignment of all state pairs, hence the same bits -- and the traversal copies rows instead of issuing
 * the node's three matrix products.  Counters since the engine was created: tables built, node updates answered. */
int iqhip_debug_cherry_tables(iqhip_engine *e, int64_t *tables_built, int64_t *ops_from_tables);

/* Which Newton and sweep forms an engine ran, counted since it was created; out[k] for k < min(n, IQHIP_PATH_NSLOTS):
 *   IQHIP_PATH_NEWTON_ONE_LAUNCH  Newton solves as one launch of k_newton (iqhip_newton_branch, iqhip_optimize_branch and
 *                                 every step of a per-step sweep)
 *   IQHIP_PATH_NEWTON_CHAIN       Newton solves as the enqueued chain (IQHIP_NEWTON=chain or a communicator rank)
 *   IQHIP_PATH_SWEEP_PERSISTENT   sweeps as one launch of the 4-state persistent kernel k_sweep4
 *   IQHIP_PATH_SWEEP_PER_STEP     sweeps as two launches per step enqueued back to back
 *   IQHIP_PATH_SWEEP_SEQUENTIAL   sweeps (or their remainders) one step at a time with a host round trip each
 *   IQHIP_PATH_NEWTON_FALLBACK    one-launch solves whose grid barrier gave up and that the enqueued chain finished
 * IQHIP_NEWTON, IQHIP_SWEEP and IQHIP_SWEEP_KERNEL are read when the engine is created.  A sharded engine counts its
 * sweeps on the front; its Newton solves run the front's own loop over the shards and are not counted. */
#define IQHIP_PATH_NEWTON_ONE_LAUNCH 0
#define IQHIP_PATH_NEWTON_CHAIN 1
#define IQHIP_PATH_SWEEP_PERSISTENT 2
#define IQHIP_PATH_SWEEP_PER_STEP 3
#define IQHIP_PATH_SWEEP_SEQUENTIAL 4
#define IQHIP_PATH_NEWTON_FALLBACK 5
#define IQHIP_PATH_NSLOTS 6
int iqhip_debug_path_counts(iqhip_engine *e, int64_t *out, int n);

/* Debugging aid, no reference counterpart: a PLANNING-ONLY engine makes no HIP call and owns no device memory (its
 * vectors are distinct fake addresses).  iqhip_debug_plan turns an op list into the device descriptors exactly as
 * iqhip_update_partials would (key -> slab map, canonical child order, staging, LDS chunks, K2 table slots, look-ahead
 * sentinels) and validates the kernels' contract on them: every pointer of every descriptor, used or not, is a live
 * allocation of the right kind (the traversal kernels request op k+1's inputs unconditionally).  The same check runs on
 * a real engine before every plan upload when IQHIP_CHECK_PLAN=1.  Every other entry point fails on a planner.
 * A planner keeps the plan cache a real engine keeps: iqhip_debug_plan with the op list of the call before it (same keys,
 * leaves, lengths; nothing created, released or invalidated in between) finds the plan cached, plans nothing and checks
 * nothing again, and counts what a cached submission counts (pair slabs marked again, cherry ops, the fill image below).
 * iqhip_debug_planner_plain_taxa and iqhip_debug_planner_event(e, 1) drop the cached plan. */
int iqhip_debug_create_planner(iqhip_engine **out, int nstates /* 4, 20, 64 */, int ncat, int64_t nptn, int ntaxa,
                               int num_cus, int state_unknown, int nclass);
int iqhip_debug_plan(iqhip_engine *e, const iqhip_node_op *ops, int nops);
/* Read-only: the shape of the planner's last plan and the launches it would get, out[k] for k < IQHIP_PLAN_SHAPE_NSLOTS
 * (n must be at least that):
 *   0..5    LDS budget of a chunk (doubles), plan regions of the largest chunk (doubles), leaf-state slots, parked operands,
 *           LDS chunks, stages of units
 *   6..13   units per stage (the first 8 stages)
 *   14..20  the top-stage launch: kernel variant (the engine's TravVariant, 10 = TRAV_WIDE4 = k_traverse4w; -1: the 4-state kernel), leaf tables, full-role
 *           workgroups of a mixed-role launch, workgroups per segment, grid, dynamic LDS bytes, offset of the parking places
 *           (doubles, -1: none)
 *   21..27  the same for the first stage of units (zeros: the plan has none) */
#define IQHIP_PLAN_SHAPE_NSLOTS 28
int iqhip_debug_plan_shape(iqhip_engine *e, int64_t *out, int n);
/* Read-only: the LDS layout of the planner's last plan, out[k * IQHIP_PLAN_LAYOUT_NSLOTS + f] for op k < nops (the op
 * count of that plan): ops of the chunk (first op of a chunk, else 0), leaf-state slots of the chunk with the dummy slot
 * (first op, else 0), left / right child is a leaf, offsets of the two children's regions (doubles), leaf-state slots of
 * the two children */
#define IQHIP_PLAN_LAYOUT_NSLOTS 8
int iqhip_debug_plan_layout(iqhip_engine *e, int32_t *out, int nops);

/* Pair children (4-state engines of at most 8 categories).  A node update whose two children are leaves with
 * plain rows (states 0 .. 3 and STATE_UNKNOWN only), submitted with scaling rule 0 in a plan whose one later op consumes it, is
 * not run: its consumer reads a 25-row table, and the vector behind its key exists as that table until someone reads it --
 * every call that reads a vector by key (fetches, branch ends, solvers, sweeps, NNI evaluators, a later plan) sees the vector
 * and the all-zero scale_num the update would have written, sum_scale of such an op is exactly 0.0, and iqhip_set_model /
 * iqhip_set_alignment keep the vectors of the submissions made before them.  Memory: the first plan that removes an update
 * allocates one device buffer of ntaxa * nptn_pad bytes (pair-code rows), as large as the state matrix.
 * iqhip_debug_pair_children: node updates removed so far, vectors expanded for a reader so far, updates the last plan removed.
 * iqhip_debug_pair_rows (any engine, a planning-only one included): slots of the pair-code row table in use; how often the table
 * started over because a plan's missing pairs did not fit beside the rows present (not counted: the clear that goes with the
 * buffer's allocation, nor the one on an alignment change); leaf-leaf updates so far that met every condition and stayed real
 * because the table had no slot left for their pair.  Any pointer may be NULL.
 * iqhip_debug_planner_plain_taxa (planning-only engines, which have no alignment): plain[t] != 0 -- taxon t's row is plain;
 * NULL -- nothing known, nothing is removed (the state after iqhip_debug_create_planner).
 * iqhip_debug_plan_removed (planning-only engines): out[k] = 1 when row k of the last plan's op list was removed. */
int iqhip_debug_pair_children(iqhip_engine *e, int64_t *ops_removed, int64_t *slabs_expanded, int64_t *last_plan_removed);
int iqhip_debug_pair_rows(iqhip_engine *e, int64_t *slots_in_use, int64_t *restarts, int64_t *kept_real_for_lack_of_a_row);
int iqhip_debug_planner_plain_taxa(iqhip_engine *e, const uint8_t *plain);
int iqhip_debug_plan_removed(iqhip_engine *e, int32_t *out, int nrows);

/* The fill image of the 4-state traversal (4-state engines of at most 8 categories).  What a chunk fill leaves in
 * LDS besides the leaf states depends on the plan and the model only.  When a submission finds its plan cached (the same op list,
 * lengths included, as the one before), the engine builds those LDS contents once into a device buffer, chunk by chunk, and the
 * traversal's workgroups copy them; a later submission of the same plan under the same model copies them again.  A new plan,
 * iqhip_set_model and iqhip_set_alignment make the image stale; plans whose lengths lie on the device, plans of a few ops that
 * travel in the kernel arguments, and a submission that plans anew never use one.  Results are bit-identical either way.
 * iqhip_debug_fill_image (any engine, a planning-only one included): submissions so far that built the image (planning-only:
 * would have), submissions that copied an image already built, bytes of the current plan's image (0: it can have none).  Any
 * pointer may be NULL.
 * Planning-only engines: iqhip_debug_plan_submit is iqhip_debug_plan with explicit segments (nsegs > 0: segment sizes) or with
 * every branch length on the device (device_lengths != 0); iqhip_debug_planner_event(e, 0) does to the planner's state what
 * iqhip_set_model does, (e, 1) what iqhip_set_alignment does; iqhip_debug_fill_image_chunks: out[2 i], out[2 i + 1] = byte
 * offset and byte extent of chunk i of the last plan's image (at most cap pairs), *nchunks = the plan's chunks. */
int iqhip_debug_fill_image(iqhip_engine *e, int64_t *built, int64_t *reused, int64_t *bytes);
int iqhip_debug_plan_submit(iqhip_engine *e, const iqhip_node_op *ops, int nops, const int32_t *segs, int nsegs, int device_lengths);
int iqhip_debug_planner_event(iqhip_engine *e, int what);
int iqhip_debug_fill_image_chunks(iqhip_engine *e, int64_t *out, int cap, int *nchunks);

/* Debugging aids, no reference counterpart: the library's memory accounting.  Every device and pinned-host allocation of
 * every engine and partition group in this process goes through one allocate / free pair, which counts bytes.
 * iqhip_debug_memory: what is live now -- device memory, and pinned or host staging memory (the plain host staging of a
 *   planning-only engine counts here; its fake device addresses count as nothing).  Either pointer may be NULL.  After
 *   every engine and group has been destroyed both are 0.
 * iqhip_debug_fail_alloc: the nth allocation from now (1-based) returns out-of-memory without a HIP call, the ones
 *   before and after it are served; 0 clears a pending failure.  Process-wide, like the counts. */
void iqhip_debug_memory(int64_t *device_bytes, int64_t *host_bytes);
void iqhip_debug_fail_alloc(int nth);

/* ---- Edge-linked partition models (-q / -spp; PhyloSuperTreePlen::computeFuncDerv, phylosupertreeplen.cpp:530-578):
 * a GROUP of existing single-device engines, one per partition, all running the super tree's topology (a taxon without
 * data in a partition stays in its alignment as an all-unknown row), whose branch lengths are the super tree's times
 * the partition's rate r_p.  The group owns nothing of its members: destroying it leaves them usable, and a member must
 * outlive the group.  All members sit on one device.
 * iqhip_partition_create: IQHIP_ERR_UNSUPPORTED for sharded engines, communicator ranks, +ASC members and mixture
 *   members; IQHIP_ERR_INVALID for planning-only engines, members without alignment or model, nparts < 1, a member
 *   listed twice, a null argument, members on different devices.  Every state count and category count iqhip_create
 *   accepts is accepted (embedded counts and wide DNA included).
 * iqhip_partition_set_rates: r_p, finite and > 0 (IQHIP_ERR_INVALID otherwise); 1 for every member after create (-q).
 * iqhip_partition_newton_branch: Optimization::minimizeNewton on f(x) = -sum_p r_p df_p(r_p x), f'(x) = -sum_p r_p^2
 *   ddf_p(r_p x).  Every member must hold a valid theta (iqhip_compute_theta, or a call that leaves one) for the SAME
 *   branch, i.e. the same two iqhip_branch_end values on every member -- leaf ids and keys: the members of a group share
 *   one key space, as trees of one topology built alike do; IQHIP_ERR_INVALID otherwise.  A member whose df is NaN or
 *   infinite contributes df = ddf = 0 (phylokernel.h:647-651, applied per partition before the weighted sum).  Bounds,
 *   update rule, stopping tests, d2l and nsteps (derivative evaluations) are those of iqhip_newton_branch, and so are the
 *   two errors of minimizeNewton.  part_lnl (nparts doubles or NULL) receives every member's computeLikelihoodFromBuffer at
 *   r_p * optx, its scale-factor term included (taken from the scale counters of the two branch ends).
 *   The solve is an enqueued chain on the group's stream: a state-machine init, then per evaluation one launch over all
 *   members' thetas and one single-workgroup update; the host reads the 128-byte state once per chunk of steps
 *   (IQHIP_PART_STEPS, read per call, overrides the steps per chunk; the result does not depend on it).  All sums run in
 *   a fixed order: the same call gives the same bits.  The group's stream waits for the members' streams and they wait
 *   for it (events, no host synchronisation per member).
 * iqhip_partition_lnl_from_theta: the same per-member values at a given x >= 0.
 * iqhip_partition_traverse_lnl: one op list and root branch for every member, member p with every length multiplied by
 *   scale[p] (NULL: the rates); everything is enqueued on the members' streams and the nparts log-likelihoods are read
 *   after one synchronisation.  part_lnl[p] is member p's whole log-likelihood (scale-factor term included); the per-op
 *   sum_scale rows are not returned.  The evaluation of PhyloSuperTreePlen::computeFunction and of
 *   optimizeTreeLengthScaling for all partitions in lockstep.
 * iqhip_partition_optimize_branch_batch: ntasks INDEPENDENT joint solves side by side -- the NNI candidates of a super tree
 *   -- with the task struct of iqhip_optimize_branch_batch.  Task t first runs its node updates ops[0..nops) on every
 *   member, member p with every op length multiplied by r_p (they may read any existing vector and must write vectors no
 *   other task touches; the keys are the same on every member), then solves the length x of branch (a, b) as
 *   iqhip_partition_newton_branch does, on thetas built into per-task slots: xguess, x1, x2, x and optx are in super-tree
 *   units, member p is evaluated at r_p * x.  The NaN / inf rule per member, update rule, bounds, stopping tests, d2l and
 *   nsteps are those of the single solve; minimizeNewton's two failures come back in results[t].status (2, 3) as in
 *   iqhip_optimize_branch_batch, not as an error of the call.  (A solve that runs into max_steps ends at j == max_steps with
 *   the last accepted iterate, status 0 and nsteps == max_steps, exactly as iqhip_partition_newton_branch returns it.)  part_lnl[t * nparts + p] (or NULL) is member p's
 *   computeLikelihoodFromBuffer at r_p * optx of task t, its scale-factor term included (from the scale counters of the
 *   two branch ends, on the device); results[t].lnl is their sum in member order, formed on the host -- so no sum_scale
 *   bookkeeping is needed for scratch vectors, and none is returned.
 *   Per chunk of tasks: one submission of the gathered node updates and the theta slots on every member's stream, then on
 *   the group's stream ONE enqueued chain for all tasks: per evaluation one derivative launch over (work item x task) and
 *   one update launch with a workgroup per task; the states are read once per chunk of steps (IQHIP_PART_STEPS), and the
 *   lnL pass rides behind each chunk.  No grid barrier, no atomics, fixed summation order: a task's result has the bits of
 *   iqhip_partition_newton_branch on the same theta, whatever the chunking.  Tasks per chunk: at most 64, and all
 *   members' theta slots together within a quarter of the free device memory; IQHIP_PART_BATCH_CHUNK (read per call)
 *   lowers it.  The members are left as iqhip_optimize_branch_batch with the same ops leaves them: the theta of
 *   iqhip_compute_theta and its validity are untouched.  IQHIP_ERR_INVALID for a null group, task array or result array,
 *   ntasks < 1, a bad ops array, bounds the single solve refuses, a key a member does not know; the member conditions of
 *   every group call apply.
 * iqhip_debug_partition_timing: *launches = kernels the group's last call enqueued on its own stream; with
 *   iqhip_timing_enable on the FIRST member, ms[0] / ms[1] = device time (HIP events) of the derivative launches / of the
 *   update launches of the last iqhip_partition_newton_branch or iqhip_partition_optimize_branch_batch. */
typedef struct iqhip_partition iqhip_partition;
int iqhip_partition_create(iqhip_partition **out, iqhip_engine *const *members, int nparts);
void iqhip_partition_destroy(iqhip_partition *g);
int iqhip_partition_set_rates(iqhip_partition *g, const double *rate /* nparts */);
int iqhip_partition_newton_branch(iqhip_partition *g, double xguess, double x1, double x2, double xacc, int max_steps,
                                  double *optx, double *d2l, int *nsteps, double *part_lnl /* nparts or NULL */);
int iqhip_partition_lnl_from_theta(iqhip_partition *g, double x, double *part_lnl /* nparts */);
int iqhip_partition_traverse_lnl(iqhip_partition *g, const iqhip_node_op *ops, int nops, iqhip_branch_end a,
                                 iqhip_branch_end b, double len, const double *scale /* nparts or NULL */,
                                 double *part_lnl /* nparts */);
int iqhip_partition_optimize_branch_batch(iqhip_partition *g, const iqhip_branch_task *tasks, int ntasks,
                                          iqhip_branch_result *results,
                                          double *part_lnl /* ntasks * nparts, [task][member], or NULL */);
int iqhip_debug_partition_timing(iqhip_partition *g, double *ms /* 2: derivative launches, update launches */,
                                 int64_t *launches);

/* ---- UFBoot on edge-linked partition models: per-pattern rows of the batched joint solve, RELL sums and the bootstrap's
 *      bookkeeping on the group (PhyloSuperTreePlen::getBestNNIForBran, phylosupertreeplen.cpp:1367-1372;
 *      PhyloSuperTree::computePatternLikelihood, phylosupertree.cpp:981-990; SuperAlignment::createBootstrapAlignment,
 *      superalignment.cpp:360-370) ----
 * Row r of the group is row r of EVERY member's store of per-pattern log-likelihood rows (iqhip_ptnlh_*); every member keeps
 * its own sample matrix, filled on the member with iqhip_set_boot_samples / iqhip_gen_boot_samples (ndraws = the member's
 * own site count: sites are resampled within partitions).  The RELL score of a super tree in replicate s is
 *     sum_p sum_ptn W_p[s][ptn] * L_p[row][ptn]
 * formed as the members' own products (the fp64 matrix-core product of iqhip_ptnlh_rell, each on its member's stream with
 * its own K-split) added IN MEMBER ORDER, ((R_0 + R_1) + R_2) + ..., on the group's stream.
 *
 * iqhip_partition_ptnlh_reserve: iqhip_ptnlh_reserve(nrows) on every member.
 * iqhip_partition_optimize_branch_batch_rows: iqhip_partition_optimize_branch_batch (rows == NULL is exactly that call),
 *   and for every task t with rows[t] >= 0 every member p receives in row rows[t] of its own store the per-pattern
 *   log-likelihood of the task's branch at r_p * optx.  A row means what iqhip_optimize_branch_batch_rows documents:
 *   log|lh + invar| with the reference's NaN / inf repair, the scale counters of both branch ends put back, 0 in the
 *   padding; members are never +ASC, so there is no shift.  The row is written by the lnL pass that rides behind every
 *   chunk of steps, in the launch that forms the task's lnL sums: the pattern's value before the multiplication by its
 *   frequency, a plain store, exactly once per task.  It is a function of the theta slot, the counters and optx alone: the
 *   same bits for every IQHIP_PART_BATCH_CHUNK and IQHIP_PART_STEPS; results and part_lnl have the bits of the call
 *   without rows.  IQHIP_ERR_INVALID, before anything is enqueued, for a row >= 0 outside any member's store
 *   and for a row >= 0 that two tasks name (the rows of one call are distinct).
 * iqhip_partition_ptnlh_rell: out[i * nsamples + s] = the member-order sum above for rows[i] and replicate s.  Member p's
 *   term has the bits of iqhip_ptnlh_rell(member p, rows, nrows, nsamples).
 * iqhip_partition_ufboot_init: the per-replicate state of iqhip_ufboot_init (boot_logl = boot_orig_logl = -DBL_MAX,
 *   boot_counts = 0, boot_tree = -1), owned by the group; the members' own UFBoot states are not touched.  Every member must
 *   hold at least nsamples samples.  The state belongs to the members' sample matrices as they are now: once any member's
 *   matrix is replaced or refilled (iqhip_set_boot_samples, iqhip_gen_boot_samples, iqhip_multiscale_bp) every call below is
 *   IQHIP_ERR_INVALID until the next init.
 * iqhip_partition_ufboot_update: iqhip_ufboot_update on the group -- the same entry struct, the same host-side cutoff
 *   (an entry with logl_cutoff != 0 and logl < logl_cutoff - 1 is dropped), the entries applied IN LIST ORDER, the same
 *   three counts {applied, dropped, replaced slots} and minimum.  `rell` of an entry is the member-order sum, formed inside
 *   the update kernel: no summed matrix is materialised.  Entries per chunk: all members' staging together within 256 MB;
 *   IQHIP_UFBOOT_CHUNK (read per call) overrides.  A member's K-split follows from nsamples, its pattern count and the CU
 *   count alone, so the state is bit-identical for every chunk size, and to the rule applied to
 *   iqhip_partition_ptnlh_rell at the same nsamples.
 * iqhip_partition_ufboot_fetch: the four state arrays, nsamples entries each (any may be NULL).
 * iqhip_debug_partition_ufboot_timing: of the last update, *launches = kernels enqueued; with iqhip_timing_enable on the
 *   FIRST member, ms[0] = device time of the members' products (summed over members), ms[1] = of the update kernels.
 * Everything is validated on the host before the first launch.  IQHIP_ERR_INVALID: a null group or list; nrows / ntrees < 1;
 *   a row outside a member's store; tree_id < 0; rand outside [0, 1] or NaN; a non-finite logl; epsilon < 0 or NaN; update
 *   or fetch before init (or after a member's sample matrix was replaced); nsamples < 1 or above any member's sample count.
 *   The member conditions of every group call apply. */
int iqhip_partition_ptnlh_reserve(iqhip_partition *g, int nrows);
int iqhip_partition_optimize_branch_batch_rows(iqhip_partition *g, const iqhip_branch_task *tasks, int ntasks,
                                               iqhip_branch_result *results,
                                               double *part_lnl /* ntasks * nparts, [task][member], or NULL */,
                                               const int32_t *rows /* ntasks (row, or < 0: none) or NULL */);
int iqhip_partition_ptnlh_rell(iqhip_partition *g, const int32_t *rows, int nrows, int nsamples,
                               double *out /* nrows * nsamples */);
int iqhip_partition_ufboot_init(iqhip_partition *g, int nsamples);
int iqhip_partition_ufboot_update(iqhip_partition *g, const iqhip_ufboot_tree *trees, int ntrees, double epsilon,
                                  double logl_cutoff, int64_t *counts /* 3 or NULL */, double *min_orig_logl /* or NULL */);
int iqhip_partition_ufboot_fetch(iqhip_partition *g, double *boot_logl, double *boot_orig_logl, int32_t *boot_counts,
                                 int64_t *boot_tree);
int iqhip_debug_partition_ufboot_timing(iqhip_partition *g, double *ms /* 2: products, update */, int64_t *launches);

/* ---- Joint pairwise distances of a partition group (PhyloSuperTreePlen::computeDist, phylosupertreeplen.cpp:361-371, per
 * pair SuperAlignmentPairwisePlen, :18-45): what an edge-linked partition run computes before it has a tree; the matrix
 * feeds iqhip_bionj and is written as .mldist.
 * iqhip_partition_pair_distances: the arguments and the [T][T] symmetric outputs dist, d2l (or NULL), nsteps (or NULL) are
 *   those of iqhip_pair_distances; T = the members' common taxon count; an init entry of 0 (or init NULL) means "use the JC
 *   start".  For the pair (i, j), counts_p being member p's iqhip_pair_counts table and r_p the group's current rate
 *   (iqhip_partition_set_rates):
 *   Start: init[i][j] when non-zero, otherwise SuperAlignment::computeDist (superalignment.cpp:384-421): total = sum_p sum
 *     counts_p, same = sum_p trace(counts_p); total == 0 -> 9; z = n_0 / (n_0 - 1) with n_0 the state count of MEMBER 0
 *     (the reference reads partitions[0]->num_states, whatever the other partitions hold); x = 1 - z (total - same) / total;
 *     x <= 0 -> 9, else -log(x) / z.  Integer-valued pattern frequencies make the sums exact in any order.
 *   DIFFERENCE from iqhip_pair_distances: a start equal to 9 (MAX_GENETIC_DIST; an init entry of exactly 9 included) is
 *     returned as it is, without a solve: dist = 9, d2l = 0, nsteps = 0 (phylosupertree.cpp:697, phylosupertreeplen.cpp:365).
 *     The plain call solves from 9.
 *   Solve: Optimization::minimizeNewton (the rule of iqhip_newton_branch) on df = sum_p r_p df_p(r_p x), ddf = sum_p r_p^2
 *     ddf_p(r_p x), summed in member order, (df_p, ddf_p) being exactly what iqhip_pair_distances evaluates for member p
 *     alone (non-zero cells only, P < 0 -> 0, S > 0, props-weighted category sums).  A member in which the pair shares no
 *     column contributes 0: the reference's "taxon absent from the partition".  A one-member group at rate 1 gives the
 *     bits of iqhip_pair_distances on that member for every pair whose start is not 9.
 *   Returns as iqhip_pair_distances: IQHIP_ERR_INVALID with the matrices filled when a pair ends in one of minimizeNewton's
 *     two errors.
 *   One wave per pair, no host round trip per step; the pairs go in chunks whose counts, all members together (sum_p n_p^2
 *     x 8 bytes per pair), fit 64 MB (IQHIP_PAIR_CHUNK, read per call, overrides the pairs per chunk).  The same bits on
 *     every run and for every chunk size.
 * IQHIP_ERR_UNSUPPORTED: a member iqhip_pair_distances refuses (embedded state counts, mixtures; sharded and +ASC members
 *   cannot be in a group at all); members whose shapes put the LDS of the solve, 8 (max_p nstates_p ncat_p + 2 max_p
 *   nstates_p) bytes, above 64 KB (a codon member with more than 126 categories).  IQHIP_ERR_INVALID: a null g or dist, members with different taxon counts, x1 > x2,
 *   xacc <= 0, max_steps < 1, a negative or non-finite init entry.  All checked before the first launch: after a refused
 *   call the group works as before.
 * iqhip_debug_partition_pair_timing: with iqhip_timing_enable on the FIRST member, the device time (HIP events,
 *   milliseconds) the last call spent in the members' count launches (summed over members, which run side by side) and in
 *   its solve launches; iqhip_debug_partition_timing's *launches = the kernels that call enqueued. */
int iqhip_partition_pair_distances(iqhip_partition *g, const double *init, double x1, double x2, double xacc, int max_steps,
                                   double *dist, double *d2l, int32_t *nsteps);
int iqhip_debug_partition_pair_timing(iqhip_partition *g, double *counts_ms, double *solve_ms);

#ifdef __cplusplus
}
#endif
#endif /* IQHIP_H_ */
