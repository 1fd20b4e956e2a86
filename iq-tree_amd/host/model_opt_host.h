// model_opt_host.h -- estimation of model parameters on top of the device likelihood: the substitution rates of the DNA models
// by the reference's BFGS, the Gamma shape and the proportion of invariable sites by Brent, and the loop around them.
// Restated (file:line = /root/reference):
//   ModelGTR::optimizeParameters / targetFunk / setBounds     model/modelgtr.cpp:556-604, 510-519, 534-554
//   RateGamma::optimizeParameters / computeFunction           model/rategamma.cpp:209-223, 156-163
//   RateInvar::optimizeParameters / computeFunction           model/rateinvar.cpp:87-100, 65-71
//   RateGammaInvar::optimizeParameters, non-joint branch      model/rategammainvar.cpp:118-139
//   ModelFactory::optimizeParametersOnly / optimizeParameters model/modelfactory.cpp:767-781, 937-1065
// over BfgsMachine (bfgs_host.h) and BrentMachine (brent_host.h).  Starting values where the model string gives none:
// rates 1 (ModelGTR::ModelGTR, model/modelgtr.cpp:61), alpha 1 (RateGamma::RateGamma with the default shape -1:
// max(MIN_GAMMA_SHAPE, |shape|), model/rategamma.cpp:32), p-inv max(frac_const_sites / 2, MIN_PINVAR) (RateInvar::RateInvar,
// model/rateinvar.cpp:26).  Values given in braces are starting values (the reference would fix them).
//
// THE BATCH.  dfpmin spends ndim + 1 of its roughly ndim + 2 .. 4 likelihood evaluations per iteration on the forward
// difference stencil of derivativeFunk, and every point of a stencil sits on the same tree.  A stencil request of the
// BfgsMachine therefore goes to a CANDIDATE TREE: a second PhyloTree of this optimiser on the same device and alignment,
// whose engine holds K * C components, K = min(ndim + 1, maxModelComponents(nstates) / C).  Class m of its mixture model is
// candidate m -- its own eigen-system and tip_partial_lh slice, the C category rates, props = p_c, class weight 1 -- so ONE
// clearAllPartialLH + traversal + theta and ONE iqhip_class_lnl return K log-likelihoods.  Topology and branch lengths are
// copied from the main tree by node id before each stencil.  A stencil of more than K points is cut into chunks; every
// chunk carries the base point as class 0, so every difference f(x + h e_i) - f(x) is formed from two values of one launch;
// a short last chunk repeats the base point.  Single requests (line search), Brent and the final evaluation run on the main
// tree, so lnsrch's fold is a main-tree value after the first iteration.  batch = false, K < 2, or an alignment of more than
// batch_max_patterns patterns (BATCH_MAX_PATTERNS, the measured crossover) sends every point to the main tree one after the
// other: the reference's order.  A non-zero floored count (iqhip_class_lnl's underflow rule) makes
// the optimiser redo that stencil sequentially; the trace counts it.
// OUT OF SCOPE: +FO, joint_optimize / optimizeAllParameters, -fai restarts, testAlpha, codon kappa /
// omega, L-BFGS-B, the boundary restart of minimizeMultiDimen, mixtures, +R (-emrates), +ASC, sharded engines.
#pragma once
#include <functional>
#include <string>
#include <vector>

#include "alignment_host.h"
#include "model_host.h"
#include "phylo_host.h"

namespace iqhost {

constexpr double MIN_RATE = 1e-4, MAX_RATE = 100.0, TOL_RATE = 1e-4;                      // model/modelgtr.h:30-32
constexpr double MIN_GAMMA_SHAPE = 0.02, MAX_GAMMA_SHAPE = 1000.0, TOL_GAMMA_SHAPE = 0.001;  // model/rategamma.h:27-29
constexpr double MIN_PINVAR = 1e-6, TOL_PINVAR = 1e-6;                                    // model/rateinvar.h:26-27
constexpr double DEFAULT_GRADIENT_EPSILON = 0.0001;   // model/modelfactory.h:169 (optimizeParameters' default)
constexpr double DEFAULT_LOGL_EPSILON = 0.01;         // params.modeps, tools.cpp:871
// batch = true batches the stencils of alignments of at most this many patterns: the largest measured size at which the
// batched stencil beat the K points one after the other (the table of tools/bench_paramopt.py: 1.5x
// at 500 patterns, 1.3x at 5 000; at 100 000 the 24-component traversal is bandwidth-bound and the batch lost 2.3x)
constexpr int64_t BATCH_MAX_PATTERNS = 5000;

class ModelOptimizer {
public:
    // one optimiser call as the trace records it
    struct Call {
        std::string what;                // "model", "alpha", "pinv"
        int requests = 0;                // requests of the machine (BFGS: stencils + singles; Brent: evaluations)
        int stencils = 0;                // stencil requests
        int stencil_traversals = 0;      // traversals of the candidate tree (one per chunk)
        int single_traversals = 0;       // traversals of the main tree
        int stencils_redone = 0;         // stencils evaluated again, sequentially, after a floored term
        int K = 0;                       // candidates per traversal (0: sequential)
        double lnl_before = 0.0, lnl_after = 0.0;
        std::vector<double> x0, grad0, h0, values0;   // the first stencil: base point, the gradient handed to the machine, steps, values
    };

    // tree: alignment set, engine attached, a model of spec's category count set.  The constructor fills the values the
    // string left out and sends that model.  Throws for what is out of scope.
    ModelOptimizer(PhyloTree &tree, const Alignment &aln, ModelSpec spec, bool batch = true);
    ~ModelOptimizer();
    ModelOptimizer(const ModelOptimizer &) = delete;
    ModelOptimizer &operator=(const ModelOptimizer &) = delete;

    // refusals and starting values, no device: throws for MIX{}, +R, +ASC, +FO; fills missing values
    static void checkScope(const ModelSpec &spec);
    static void startingValues(ModelSpec &spec, const Alignment &aln);
    // free rate parameters (0 for models without, and for codon models whose parameters are not estimated here)
    static int numParams(const ModelSpec &spec) { const int k = numRateParams(spec); return k < 0 ? 0 : k; }
    // candidates per traversal for ndim parameters and C rate categories
    static int candidatesPerTraversal(int ndim, int ncat, int nstates);

    double optimizeModel(double gradient_epsilon = DEFAULT_GRADIENT_EPSILON);    // ModelGTR::optimizeParameters; 0.0: nothing to do
    double optimizeRates(double gradient_epsilon = DEFAULT_GRADIENT_EPSILON);    // the site_rate's optimizeParameters; 0.0: no +G / +I
    double optimizeParametersOnly(double gradient_epsilon = DEFAULT_GRADIENT_EPSILON);
    double optimizeParameters(bool fixed_len = false, double logl_epsilon = DEFAULT_LOGL_EPSILON,
                              double gradient_epsilon = DEFAULT_GRADIENT_EPSILON, bool write_info = false);
    int rounds = 0;   // of the last optimizeParameters (the reference's i - 1)

    // the loop of ModelFactory::optimizeParameters (model/modelfactory.cpp:952-1033) around any "optimise the parameters,
    // return the lnL" step: initial lnL cur_lh; for i = 2 .. 99: optimizeAllBranches(min(i, 3), logl_epsilon) unless
    // fixed_len, the step; stop when the step returns 0 (nothing to optimise) or its gain is not above logl_epsilon, with
    // the final optimizeAllBranches(100, logl_epsilon).  write_info prints the reference's progress lines.  -> cur_lh
    static double parameterLoop(PhyloTree &tree, bool fixed_len, double logl_epsilon, double cur_lh,
                                const std::function<double()> &optimize_only, bool write_info, int *rounds = nullptr);

    std::string modelString() const;    // full precision, braces filled
    std::string writeInfo() const;      // the reference's writeInfo lines of the model and the site rates
    const ModelSpec &getSpec() const { return spec; }
    const ModelInputs &getInputs() const { return mi; }
    bool batch;
    int64_t batch_max_patterns = BATCH_MAX_PATTERNS;   // (the bench raises it to measure the batch above the crossover)
    std::vector<Call> trace;

private:
    PhyloTree &tree;
    const Alignment &aln;
    ModelSpec spec;          // the model the main tree holds now
    ModelInputs mi;
    std::string original;    // tokens of the model string, for modelString()
    PhyloTree *cand = nullptr;
    int cand_K = 0;
    std::vector<double> cand_invar;
    Call *cur_call = nullptr;

    double evalMain(const ModelSpec &s);                         // the reference's targetFunk / computeFunction on the main tree
    void stencilSequential(const ModelSpec &base, const std::vector<double> &points, int npoints, double *values);
    bool stencilBatched(const ModelSpec &base, const std::vector<double> &points, int npoints, int K, double *values);
    double brent(const char *what, double xmin, double xguess, double xmax, double tol, const std::function<void(ModelSpec &, double)> &set);
};

}  // namespace iqhost
