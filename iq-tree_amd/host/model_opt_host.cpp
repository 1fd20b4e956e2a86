// model_opt_host.cpp -- see model_opt_host.h
#include "model_opt_host.h"

#include <math.h>
#include <stdio.h>

#include <algorithm>
#include <sstream>
#include <stdexcept>

#include "bfgs_host.h"
#include "brent_host.h"

namespace iqhost {

namespace {

std::string upperCase(std::string s) {
    for (char &c : s) c = (char)toupper((unsigned char)c);
    return s;
}

// the '+'-separated tokens of a model string, braces respected
std::vector<std::string> modelTokens(const std::string &s) {
    std::vector<std::string> toks;
    size_t start = 0;
    int depth = 0;
    for (size_t i = 0; i <= s.size(); i++) {
        if (i < s.size() && s[i] == '{') depth++;
        if (i < s.size() && s[i] == '}') depth--;
        if (i == s.size() || (s[i] == '+' && depth == 0)) {
            toks.push_back(s.substr(start, i - start));
            start = i + 1;
        }
    }
    return toks;
}

std::string num(double v) {
    char buf[40];
    snprintf(buf, sizeof buf, "%.17g", v);
    return buf;
}

bool sameRates(const ModelSpec &a, const ModelSpec &b) { return a.gamma_shape == b.gamma_shape && a.p_invar == b.p_invar; }

}  // namespace

void ModelOptimizer::checkScope(const ModelSpec &spec) {
    if (!spec.mix_classes.empty()) throw std::runtime_error("model optimisation: MIX{} models are not supported (-mixweights estimates their weights)");
    if (!spec.free_rates.empty())
        throw std::runtime_error("model optimisation: +R models are not supported (-emrates estimates their weights and rates)");
    if (spec.ascertainment) throw std::runtime_error("model optimisation: +ASC is not supported");
    if (spec.freq_optimized) throw std::runtime_error("model optimisation: +FO (estimated frequencies) is not supported");
}

void ModelOptimizer::startingValues(ModelSpec &spec, const Alignment &aln) {
    const int k = numParams(spec);
    if (spec.params.empty() && k > 0) spec.params.assign((size_t)k, 1.0);   // model/modelgtr.cpp:61
    if (spec.gamma_missing) spec.gamma_shape = 1.0;                         // model/rategamma.cpp:32 with the default shape -1
    if (spec.pinvar_missing) spec.p_invar = std::max(aln.frac_const_sites / 2.0, MIN_PINVAR);   // model/rateinvar.cpp:26
    spec.params_missing = spec.gamma_missing = spec.pinvar_missing = false;
}

int ModelOptimizer::candidatesPerTraversal(int ndim, int ncat, int nstates) {
    return std::min(ndim + 1, maxModelComponents(nstates) / std::max(1, ncat));
}

ModelOptimizer::ModelOptimizer(PhyloTree &tree_, const Alignment &aln_, ModelSpec spec_, bool batch_)
    : batch(batch_), tree(tree_), aln(aln_), spec(spec_) {
    checkScope(spec);
    if (!tree.engine) throw std::runtime_error("ModelOptimizer: the tree has no engine");
    if (tree.n_unobserved > 0) throw std::runtime_error("model optimisation: +ASC is not supported");
    if (tree.ncat != spec.ncat || tree.nmixture != 1)
        throw std::runtime_error("ModelOptimizer: the tree holds a model of another category count");
    original = spec.source;
    startingValues(spec, aln);
    // send the starting model (buildModel + setModel + setPtnInvar)
    buildModel(spec, aln, mi);
    tree.setModel(mi.ncat, mi.eig.eval.data(), mi.eig.evec.data(), mi.eig.inv_evec.data(), mi.rates.data(), mi.props.data());
    std::vector<double> invar;
    aln.ptnInvar(mi.p_invar, mi.state_freq.data(), invar);
    tree.setPtnInvar(invar.data());
    tree.clearAllPartialLH();
}

ModelOptimizer::~ModelOptimizer() { delete cand; }

// targetFunk (modelgtr.cpp:510-519) / computeFunction (rategamma.cpp:156-163): re-send and clear only when the point differs
// from the one the tree holds
double ModelOptimizer::evalMain(const ModelSpec &s) {
    const bool params_changed = s.params != spec.params, rates_changed = !sameRates(s, spec);
    if (params_changed || rates_changed) {
        if (params_changed) buildModel(s, aln, mi);
        else buildRateCategories(s, mi);
        tree.setModel(mi.ncat, mi.eig.eval.data(), mi.eig.evec.data(), mi.eig.inv_evec.data(), mi.rates.data(), mi.props.data());
        if (s.p_invar != spec.p_invar) {
            std::vector<double> invar;
            aln.ptnInvar(mi.p_invar, mi.state_freq.data(), invar);
            tree.setPtnInvar(invar.data());
        }
        tree.clearAllPartialLH();
        spec.params = s.params;
        spec.gamma_shape = s.gamma_shape;
        spec.p_invar = s.p_invar;
        if (cur_call) cur_call->single_traversals++;
    }
    return tree.computeLikelihood();
}

void ModelOptimizer::stencilSequential(const ModelSpec &base, const std::vector<double> &points, int npoints, double *values) {
    const size_t n = base.params.size();
    ModelSpec s = base;
    for (int r = 0; r < npoints; r++) {
        s.params.assign(points.begin() + (size_t)r * n, points.begin() + (size_t)(r + 1) * n);
        values[r] = -evalMain(s);
    }
}

// -> false when a term was floored (the caller evaluates the stencil again, sequentially)
bool ModelOptimizer::stencilBatched(const ModelSpec &base, const std::vector<double> &points, int npoints, int K, double *values) {
    const size_t n = base.params.size(), C = (size_t)base.ncat;
    // the candidates' inputs: eigen-systems of all points (the base point once)
    std::vector<ModelInputs> in((size_t)npoints);
    ModelSpec s = base;
    for (int r = 0; r < npoints; r++) {
        s.params.assign(points.begin() + (size_t)r * n, points.begin() + (size_t)(r + 1) * n);
        buildModel(s, aln, in[(size_t)r]);
    }
    std::vector<double> invar;
    aln.ptnInvar(in[0].p_invar, in[0].state_freq.data(), invar);
    std::vector<int> cat_class((size_t)K * C);
    for (size_t q = 0; q < cat_class.size(); q++) cat_class[q] = (int)(q / C);
    const std::vector<double> ones((size_t)K, 1.0);
    std::vector<double> lnl((size_t)K);
    std::vector<int64_t> floored((size_t)K);
    double base_first = 0.0;
    for (int first = 1, chunk = 0; first < npoints || chunk == 0; first += K - 1, chunk++) {
        // class 0: the base point; classes 1 ..: the forward points first, first + 1, ...; a short chunk repeats the base
        std::vector<double> eval, evec, ievec, rates, props;
        std::vector<int> point_of((size_t)K, 0);
        for (int m = 1; m < K; m++)
            if (first + m - 1 < npoints) point_of[(size_t)m] = first + m - 1;
        for (int m = 0; m < K; m++) {
            const ModelInputs &x = in[(size_t)point_of[(size_t)m]];
            eval.insert(eval.end(), x.eig.eval.begin(), x.eig.eval.end());
            evec.insert(evec.end(), x.eig.evec.begin(), x.eig.evec.end());
            ievec.insert(ievec.end(), x.eig.inv_evec.begin(), x.eig.inv_evec.end());
            rates.insert(rates.end(), x.rates.begin(), x.rates.end());
            props.insert(props.end(), x.props.begin(), x.props.end());   // p_c: class weight 1
        }
        if (cand && cand_K != K) {
            delete cand;
            cand = nullptr;
        }
        if (!cand) {
            cand = new PhyloTree();
            cand->copyTopology(tree);
            std::vector<uint8_t> states;
            std::vector<double> freq;
            aln.statesByLeaf(states);
            aln.ptnFreq(freq);
            cand->setAlignment(aln.num_states, aln.seq_type, aln.getNPattern(), states.data(), freq.data(), invar.data());
            cand->setMixtureModel(K, (int)(K * C), cat_class.data(), eval.data(), evec.data(), ievec.data(), rates.data(), props.data());
            cand->lh_mem_save = LM_PER_NODE;
            cand->setLikelihoodKernel(LK_EIGEN_HIP);
            cand->attachEngine(tree.engine_device);
            cand->initializeAllPartialLh();
            cand_K = K;
            cand_invar = invar;
        } else
            cand->setMixtureModel(K, (int)(K * C), cat_class.data(), eval.data(), evec.data(), ievec.data(), rates.data(), props.data());
        if (chunk == 0) {
            cand->copyBranchLengths(tree);
            if (cand_invar != invar) {
                cand->setPtnInvar(invar.data());
                cand_invar = invar;
            }
        }
        cand->clearAllPartialLH();
        cand->classLnl(cand->root->neighbors[0], cand->root, ones.data(), nullptr, lnl.data(), floored.data());
        if (cur_call) cur_call->stencil_traversals++;
        for (int m = 0; m < K; m++)
            if (floored[(size_t)m] != 0) return false;
        if (chunk == 0) {
            base_first = lnl[0];
            values[0] = -base_first;
        }
        for (int m = 1; m < K; m++) {
            const int r = point_of[(size_t)m];
            if (r == 0) continue;
            // both values of a difference come from one launch (the base of a later chunk has the bits of the first: same
            // class slot, same data, fixed-order sums; should it ever differ, the difference is what is kept)
            values[r] = lnl[0] == base_first ? -lnl[(size_t)m] : -(base_first + (lnl[(size_t)m] - lnl[0]));
        }
    }
    return true;
}

double ModelOptimizer::optimizeModel(double gradient_epsilon) {
    const int ndim = numParams(spec);
    if (ndim == 0) return 0.0;   // modelgtr.cpp:560
    trace.emplace_back();
    Call &call = trace.back();
    cur_call = &call;
    call.what = "model";
    call.lnl_before = tree.computeLikelihood();
    // (targetFunk returns 1e12 while the last state's frequency is below 1e-4, modelgtr.cpp:512; the frequencies are fixed here)
    const bool bad_freq = mi.state_freq.back() < 1e-4;
    const std::vector<double> lower((size_t)ndim, MIN_RATE), upper((size_t)ndim, MAX_RATE);   // setBounds :534-542, bound_check false
    const bool use_batch = batch && (int64_t)aln.getNPattern() <= batch_max_patterns;
    const int K = use_batch ? candidatesPerTraversal(ndim, spec.ncat, aln.num_states) : 0;
    call.K = K >= 2 ? K : 0;
    BfgsMachine m;
    m.init(ndim, spec.params.data(), lower.data(), upper.data(), nullptr, std::max(gradient_epsilon, TOL_RATE));
    std::vector<double> values((size_t)ndim + 1);
    const ModelSpec base = spec;   // (frequencies, rate heterogeneity: fixed during this call)
    while (m.request != BfgsMachine::DONE) {
        call.requests++;
        const int np = m.npoints();
        if (bad_freq) {
            for (int r = 0; r < np; r++) values[(size_t)r] = 1.0e+12;
        } else if (m.request == BfgsMachine::STENCIL) {
            call.stencils++;
            ModelSpec b = base;
            b.gamma_shape = spec.gamma_shape;
            b.p_invar = spec.p_invar;
            bool done = false;
            if (K >= 2) {
                done = stencilBatched(b, m.points, np, K, values.data());
                if (!done) call.stencils_redone++;
            }
            if (!done) stencilSequential(b, m.points, np, values.data());
        } else {
            ModelSpec s = base;
            s.params = m.points;
            values[0] = -evalMain(s);
        }
        const bool first = m.request == BfgsMachine::STENCIL && call.stencils == 1;
        if (first) {
            call.x0.assign(m.points.begin(), m.points.begin() + ndim);
            call.h0 = m.h;
            call.values0.assign(values.begin(), values.begin() + np);
        }
        m.update(values.data());
        if (first) call.grad0 = m.g;
    }
    double score = -m.fret;
    // getVariables / decomposeRateMatrix / computeLikelihood when the point differs from the one evaluated last (:586-596)
    ModelSpec fin = base;
    fin.params = m.x;
    if (fin.params != spec.params) score = evalMain(fin);
    call.lnl_after = score;
    cur_call = nullptr;
    return score;
}

// minimizeOneDimen over computeFunction, then computeFunction at the optimum (rategamma.cpp:217-222, rateinvar.cpp:94-99)
double ModelOptimizer::brent(const char *what, double xmin, double xguess, double xmax, double tol,
                             const std::function<void(ModelSpec &, double)> &set) {
    trace.emplace_back();
    Call &call = trace.back();
    cur_call = &call;
    call.what = what;
    call.lnl_before = tree.computeLikelihood();
    BrentMachine bm;
    double x = bm.init(xmin, xguess, xmax, tol);
    while (!bm.done) {
        ModelSpec s = spec;
        set(s, x);
        call.requests++;
        x = bm.update(-evalMain(s));
    }
    ModelSpec s = spec;
    set(s, bm.optx);
    const double lh = evalMain(s);
    call.lnl_after = lh;
    cur_call = nullptr;
    return lh;
}

double ModelOptimizer::optimizeRates(double gradient_epsilon) {
    auto alpha = [&]() {
        return brent("alpha", MIN_GAMMA_SHAPE, spec.gamma_shape, MAX_GAMMA_SHAPE, std::max(gradient_epsilon, TOL_GAMMA_SHAPE),
                     [](ModelSpec &s, double v) { s.gamma_shape = v; });
    };
    auto pinv = [&]() {
        return brent("pinv", MIN_PINVAR, spec.p_invar, std::min(aln.frac_const_sites, 1.0 - MIN_PINVAR),
                     std::max(gradient_epsilon, TOL_PINVAR), [](ModelSpec &s, double v) { s.p_invar = v; });
    };
    if (spec.has_gamma && spec.has_invar) {   // rategammainvar.cpp:118-139: alpha, then p-inv
        alpha();
        return pinv();
    }
    if (spec.has_gamma) return alpha();
    if (spec.has_invar) return pinv();
    return 0.0;   // RateHeterogeneity::optimizeParameters
}

double ModelOptimizer::optimizeParametersOnly(double gradient_epsilon) {   // modelfactory.cpp:769-775
    const double model_lh = optimizeModel(gradient_epsilon);
    const double rate_lh = optimizeRates(gradient_epsilon);
    return rate_lh == 0.0 ? model_lh : rate_lh;
}

double ModelOptimizer::parameterLoop(PhyloTree &tree, bool fixed_len, double logl_epsilon, double cur_lh,
                                     const std::function<double()> &optimize_only, bool write_info, int *rounds) {
    if (write_info) printf("1. Initial log-likelihood: %.6f\n", cur_lh);
    int i;
    for (i = 2; i < 100; i++) {   // params.num_param_iterations
        if (!fixed_len) tree.optimizeAllBranches(std::min(i, 3), logl_epsilon);
        const double new_lh = optimize_only();
        if (new_lh == 0.0) {   // nothing to optimise (:1004-1007)
            if (!fixed_len) cur_lh = tree.optimizeAllBranches(100, logl_epsilon);
            break;
        }
        if (new_lh > cur_lh + logl_epsilon) {
            cur_lh = new_lh;
            if (write_info) printf("%d. Current log-likelihood: %.6f\n", i, cur_lh);
        } else {
            if (!fixed_len) cur_lh = tree.optimizeAllBranches(100, logl_epsilon);
            break;
        }
    }
    if (rounds) *rounds = i - 1;
    return cur_lh;
}

double ModelOptimizer::optimizeParameters(bool fixed_len, double logl_epsilon, double gradient_epsilon, bool write_info) {
    const double cur_lh = tree.computeLikelihood();
    // (rescaleRates: the mean rate of a Gamma / +I model is 1 by construction, nothing to rescale, :1036-1040)
    return parameterLoop(tree, fixed_len, logl_epsilon, cur_lh, [&]() { return optimizeParametersOnly(gradient_epsilon); },
                         write_info, &rounds);
}

std::string ModelOptimizer::modelString() const {
    std::vector<std::string> toks = modelTokens(original);
    std::string out;
    for (size_t t = 0; t < toks.size(); t++) {
        std::string tok = toks[t];
        const std::string u = upperCase(tok);
        const size_t open = tok.find('{');
        if (t == 0) {
            if (numParams(spec) > 0) {
                tok = tok.substr(0, open) + "{";
                for (size_t k = 0; k < spec.params.size(); k++) tok += (k ? "," : "") + num(spec.params[k]);
                tok += "}";
            }
        } else if (u[0] == 'I' && (u.size() == 1 || open == 1))
            tok = "I{" + num(spec.p_invar) + "}";
        else if (u[0] == 'G')
            tok = tok.substr(0, open) + "{" + num(spec.gamma_shape) + "}";
        out += (t ? "+" : "") + tok;
    }
    return out;
}

std::string ModelOptimizer::writeInfo() const {
    std::ostringstream out;
    if (aln.num_states == 4 && aln.seq_type == SEQ_DNA) {   // ModelGTR::writeInfo, modelgtr.cpp:184-203
        double r[6] = {1, 1, 1, 1, 1, 1};
        const int k = numParams(spec);
        if (k == 1) r[1] = r[4] = spec.params[0];
        else if (k == 2) { r[1] = spec.params[0]; r[4] = spec.params[1]; }
        else if (k == 5) for (int j = 0; j < 5; j++) r[j] = spec.params[(size_t)j];
        out << "Rate parameters:  A-C: " << r[0] << "  A-G: " << r[1] << "  A-T: " << r[2] << "  C-G: " << r[3] << "  C-T: " << r[4]
            << "  G-T: " << r[5] << "\n";
        out << "Base frequencies:   A: " << mi.state_freq[0] << "  C: " << mi.state_freq[1] << "  G: " << mi.state_freq[2]
            << "  T: " << mi.state_freq[3] << "\n";
    }
    if (spec.has_invar) out << "Proportion of invariable sites: " << spec.p_invar << "\n";   // RateInvar::writeInfo
    if (spec.has_gamma) out << "Gamma shape alpha: " << spec.gamma_shape << "\n";             // RateGamma::writeInfo
    return out.str();
}

}  // namespace iqhost
