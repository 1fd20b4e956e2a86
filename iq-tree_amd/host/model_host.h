// model_host.h -- producers of the likelihood kernels' model inputs.
//
// The kernels take an eigen-system (eval, U = evec, U^-1 = inv_evec), category rates and
// proportions.  In the reference these come from (file:line = /root/reference):
//   ModelGTR::decomposeRateMatrix            model/modelgtr.cpp:608-722
//   EigenDecomposition::eigensystem_sym      eigendecomposition.cpp:167-296  (normalise Q to one
//       substitution per unit time :306-346, drop zero-frequency states :348-371, symmetrise with
//       sqrt(pi) :373-394, symmetric eigen-solver, U = V/sqrt(pi), U^-1 = V^T*sqrt(pi))
//   RateGamma::computeRates / computeRatesMean   model/rategamma.cpp:86-150 (+ the four published
//       routines it cites: AS 291 lnGamma, AS 32 incomplete gamma, AS 70 normal point, AS 91 chi2 point)
//   ModelCodon (GY94 rate attributes / kappa-omega scaling)   model/modelcodon.cpp:468-540, 671-700
//   Alignment::computeCodonFreq (F1X4 / F3X4)   alignment.cpp:2990-3080
// This is host-side C++ (the reference's is too); nothing here runs on the likelihood hot path.
// The symmetric eigen-solver is a cyclic Jacobi iteration, not the reference's tred2/tqli pair:
// eigenvector order and signs differ, the likelihood does not depend on either.
#pragma once
#include <string>
#include <vector>

namespace iqhost {

struct EigenSystem {
    int n = 0;
    std::vector<double> eval, evec, inv_evec;  // evec[x*n+i] = U[x][i]; inv_evec[i*n+x] = U^-1[i][x]
};

// rate_matrix: n*n exchangeabilities (symmetric, diagonal ignored) -- or, with
// ignore_state_freq, the complete off-diagonal rates q_ij (codon models that already folded the
// nucleotide frequencies in).  state_freq need not be normalised.
void decomposeRateMatrix(const double *rate_matrix, const double *state_freq, int n, EigenSystem &out,
                         bool ignore_state_freq = false);

// RateGamma::computeRates: mean (default) or median discrete-Gamma rates, divided by (1 - p_invar)
void discreteGammaRates(double gamma_shape, int ncategory, bool cut_median, double p_invar, double *rates);
double cmpLnGamma(double alpha);
double cmpIncompleteGamma(double x, double alpha, double ln_gamma_alpha);
double cmpPointNormal(double prob);
double cmpPointChi2(double prob, double v);

// Standard genetic code in the reference's codon numbering (A,C,G,T = 0..3, codon = 16a+4b+c)
const char *geneticCode(int ncbi_table);

// A parsed `-m` string, e.g. "GTR{1.5,2.4,1.8,1.9,2.8}+F{0.25,0.26,0.25,0.24}+I{0.1}+G4{0.9}",
// "HKY{2.0}+G4{0.5}", "JC", "POISSON+G4{1.0}", "GY{2.0,0.5}+F1X4", "file.paml+G4{0.9}", "...+ASC".
struct ModelSpec {
    std::string name;                 // JC F81 K80 HKY TN GTR POISSON GY JC2 GTR2 (binary data) <paml file>
    std::vector<double> params;       // rate parameters in the reference's order
    enum FreqType { FREQ_DEFAULT, FREQ_EQUAL, FREQ_USER, FREQ_EMPIRICAL, FREQ_CODON_1x4, FREQ_CODON_3x4 } freq_type = FREQ_DEFAULT;
    std::vector<double> user_freq;
    int ncat = 1;
    double gamma_shape = 1.0;
    bool gamma_median = false;
    double p_invar = 0.0;
    // +R<k>{w1,r1,...,wk,rk} (model/ratefree.cpp:25-55): free-rate categories, weights summing to 1, rates already
    // rescaled to mean 1; empty: discrete Gamma
    std::vector<double> free_props, free_rates;
    bool ascertainment = false;
    // MIX{m1[:rate[:weight]],m2,...} (ModelMixture::initMixture, model/modelmixture.cpp:1132-1230): name == "MIX", one spec
    // per class (substitution model and frequencies only), the class rates rescaled so that sum_m w_m rate_m = 1 and the
    // weights normalised to sum 1 (1 / k each when none is given); the rate suffixes of the whole string apply to every class
    std::vector<ModelSpec> mix_classes;
    std::vector<double> mix_rates, mix_weights;
    bool mix_weights_given = false;   // some class carried a :weight (the reference's fix_prop)
    // what the string named, and which values it left out (parseModelString with allow_missing; the model optimiser,
    // model_opt_host.h, fills them with the reference's starting values): +I / +G given at all; no {} behind the
    // substitution model although it has rate parameters, behind +I, behind +G; +FO (frequencies to be estimated)
    bool has_invar = false, has_gamma = false;
    bool params_missing = false, pinvar_missing = false, gamma_missing = false;
    bool freq_optimized = false;
    std::string source;               // the string as parsed
};
// components (classes x rate categories) an engine of this state count takes
int maxModelComponents(int nstates);
// allow_missing: a substitution model, +I or +G<k> may come without braces (the *_missing flags); without it such a string is
// refused
ModelSpec parseModelString(const std::string &s, bool allow_missing = false);
// free rate parameters of a substitution model by name, in the reference's order (ModelDNA::init, model/modeldna.cpp; a
// protein matrix has none): JC / F81 / POISSON / a PAML file 0, K80 / HKY 1, TN 2, GTR 5; -1: not a model with rate
// parameters this library optimises (GY, MIX)
int numRateParams(const ModelSpec &spec);
// the category rates and proportions of spec's rate heterogeneity (discrete Gamma, +I, +R) -> out.ncat / rates / props / p_invar
void buildRateCategories(const ModelSpec &spec, struct ModelInputs &out);

struct ModelInputs {      // what PhyloTree::setModel / iqhip_set_model consume
    int nstates = 0, ncat = 1;
    EigenSystem eig;
    std::vector<double> state_freq, rates, props;
    double p_invar = 0.0;
    // mixtures (nclass > 1): eig holds the classes' systems one after the other (eval [nclass][n], evec / inv_evec
    // [nclass][n][n], the eigenvalues of class m times its rate, as total_num_subst scales them in the reference); ncat
    // counts the components, in [class][rate] order: cat_class[q] = q / (rate categories), props[q] = w_m * p_c;
    // state_freq = sum_m w_m class_freq[m] (what ptn_invar is built from)
    int nclass = 1;
    std::vector<int> cat_class;
    std::vector<double> class_freq, class_rates, class_weights;   // [nclass][n], [nclass], [nclass]
};

class Alignment;
// builds the rate matrix named by `spec` for the alignment's data type, takes frequencies from the
// spec or the alignment, decomposes, and produces the category rates
void buildModel(const ModelSpec &spec, const Alignment &aln, ModelInputs &out);

}  // namespace iqhost
