// phylo_em.cpp -- the +R EM, site rates, the mixture-weight EM and per-class log-likelihoods (see phylo_host.h)
#include "phylo_host.h"
#include "brent_host.h"
#include "model_host.h"

#include <math.h>

#include <algorithm>

namespace iqhost {

// ---- EM for +R free-rate models, empirical-Bayes site rates (kernels_em.hip; model/ratefree.cpp:450-579)
void PhyloTree::setRateCategories(const double *rates, const double *props) {
    if (m_rates.empty()) throw std::runtime_error("setRateCategories before setModel");
    m_rates.assign(rates, rates + ncat);
    m_props.assign(props, props + ncat);
    inputs_dirty = model_dirty = true;
    theta_computed = false;
}

void PhyloTree::scaleLength(double norm) {
    for (PhyloNeighbor *nb : all_neighbors) nb->length *= norm;
    theta_computed = false;
}

void PhyloTree::freeRateStart(int k, std::vector<double> &props, std::vector<double> &rates) {
    if (k < 1) throw std::runtime_error("freeRateStart: at least one category");
    props.assign((size_t)k, 1.0 / k);
    rates.assign((size_t)k, 1.0);
    discreteGammaRates(1.0, k, false, 0.0, rates.data());
}

void PhyloTree::emPosteriors(double *cat_sum) {
    needEngine("emPosteriors");
    if (!current_it) throw std::runtime_error("emPosteriors before computeLikelihood");
    rebuildTheta(current_it, current_it_back->node);
    check(iqhip_em_posteriors(engine, current_it->length, cat_sum), "iqhip_em_posteriors");
}

void PhyloTree::emObjective(PhyloNeighbor *dad_branch, PhyloNode *dad, double *f, int64_t *floored) {
    needEngine("emObjective");
    PhyloNeighbor *back = dad_branch->node->findNeighbor(dad);
    if (!back) throw std::runtime_error("emObjective: not a branch");
    current_it = dad_branch;
    current_it_back = back;
    rebuildTheta(dad_branch, dad);
    check(iqhip_em_objective(engine, branchEnd(dad_branch), branchEnd(back), dad_branch->length, f, floored),
          "iqhip_em_objective");
}

void PhyloTree::computePatternRates(std::vector<double> &rates_out, std::vector<int> &cat_out) {
    std::vector<double> cat_sum((size_t)ncat);
    emPosteriors(cat_sum.data());
    rates_out.assign((size_t)nptn, 0.0);
    std::vector<int32_t> cat((size_t)nptn);
    check(iqhip_em_site_rates(engine, rates_out.data(), cat.data()), "iqhip_em_site_rates");
    cat_out.assign(cat.begin(), cat.end());
}

double PhyloTree::optimizeFreeRatesEM(std::vector<EmStep> *trace) {
    needEngine("optimizeFreeRatesEM");
    if (nmixture > 1) throw std::runtime_error("optimizeFreeRatesEM: mixture models are not supported (ModelMixture::optimizeWithEM)");
    if (n_unobserved > 0) throw std::runtime_error("optimizeFreeRatesEM: +ASC is not supported (the reference switches EM off for it)");
    for (double v : ptn_invar)
        if (v != 0.0) throw std::runtime_error("optimizeFreeRatesEM: +I+R (p_invar > 0) is not supported");
    const double MIN_PROP = 1e-4;
    const int nmix = ncat;
    const double nsite = getAlnNSite();
    std::vector<double> prop(m_props), rates(m_rates), new_prop((size_t)nmix), f((size_t)nmix);
    std::vector<int64_t> floored((size_t)nmix);
    if (trace) trace->clear();
    for (int step = 0; step < nmix; step++) {
        EmStep rec;
        rec.evals.assign((size_t)nmix, 0);
        rec.floored.assign((size_t)nmix, 0);
        // E-step on the current parameters (computePatternLhCat: a likelihood evaluation, then theta of its branch)
        rec.lnl_before = computeLikelihood();
        emPosteriors(new_prop.data());
        // M-step, weights
        int maxpropid = 0;
        for (int c = 0; c < nmix; c++) {
            new_prop[c] = new_prop[c] / nsite;
            if (new_prop[c] > new_prop[maxpropid]) maxpropid = c;
        }
        bool zero_prop = false;
        for (int c = 0; c < nmix; c++)
            if (new_prop[c] < MIN_PROP) {
                new_prop[maxpropid] -= (MIN_PROP - new_prop[c]);
                new_prop[c] = MIN_PROP;
                zero_prop = true;
            }
        if (zero_prop) {   // the reference breaks BEFORE the weights are assigned
            rec.props = prop;
            rec.rates = rates;
            if (trace) trace->push_back(rec);
            break;
        }
        bool converged = true;
        for (int c = 0; c < nmix; c++) {
            converged = converged && (fabs(prop[c] - new_prop[c]) < 1e-4);
            prop[c] = new_prop[c];
        }
        // M-step, rates: optimizeTreeLengthScaling(MIN_PROP, rates[c], 1 / prop[c], 0.001) for all c in lockstep
        std::vector<BrentMachine> bm((size_t)nmix);
        std::vector<double> trial(rates);
        int running = 0;
        for (int c = 0; c < nmix; c++) {
            const double scaling = rates[c];
            trial[c] = bm[c].init(std::min(scaling, MIN_PROP), scaling, std::max(1.0 / prop[c], scaling), std::max(0.001, 0.001));
            running++;
        }
        while (running > 0) {
            setRateCategories(trial.data(), prop.data());
            clearAllPartialLH();
            computeLikelihood();
            emObjective(current_it, current_it_back->node, f.data(), floored.data());
            rec.rounds++;
            for (int c = 0; c < nmix; c++) {
                if (bm[c].done) continue;
                rec.floored[c] += floored[c];
                const double next = bm[c].update(-f[c]);
                rec.evals[c]++;
                if (bm[c].done) {
                    running--;
                    trial[c] = bm[c].optx;   // a finished machine keeps its accepted rate
                } else
                    trial[c] = next;
            }
        }
        double sum = 0.0;
        for (int c = 0; c < nmix; c++) {
            const double scaling = bm[c].optx;
            converged = converged && (fabs(rates[c] - scaling) < 1e-4);
            rates[c] = scaling;
            sum += prop[c] * rates[c];   // (computed and never used, as in the reference)
        }
        (void)sum;
        setRateCategories(rates.data(), prop.data());
        clearAllPartialLH();
        rec.props = prop;
        rec.rates = rates;
        if (trace) trace->push_back(rec);
        if (converged) break;
    }
    setRateCategories(rates.data(), prop.data());
    clearAllPartialLH();
    return computeLikelihood();
}

// ---- EM for mixture class weights (kernels_mixem.hip; model/modelmixture.cpp:1355-1416)
double PhyloTree::getAlnNSite() const {
    double nsite = 0.0;
    for (double f : ptn_freq) nsite += f;
    return nsite;
}

void PhyloTree::computePatternLhCat(SiteLoglType wsl, double *out) {
    needEngine("computePatternLhCat");
    if (wsl != WSL_MIXTURE) throw std::runtime_error("computePatternLhCat: only WSL_MIXTURE takes this form");
    if (!current_it) throw std::runtime_error("computePatternLhCat before computeLikelihood");
    rebuildTheta(current_it, current_it_back->node);
    check(iqhip_mix_class_lh(engine, current_it->length, out), "iqhip_mix_class_lh");
}

std::vector<double> PhyloTree::getMixtureWeights() const {
    std::vector<double> w((size_t)nmixture, 0.0);
    std::vector<char> seen((size_t)nmixture, 0);
    for (int q = 0; q < ncat; q++) {
        const int m = m_cat_class[q];
        w[m] = seen[m] ? w[m] + m_props[q] : m_props[q];
        seen[m] = 1;
    }
    return w;
}

void PhyloTree::mixWeightsEM(int max_steps, double *weights, double *p_invar, int *nsteps, int *converged, double *trace) {
    needEngine("mixWeightsEM");
    // a model or weights set since the last submission reach the engine first: it refuses the matrix of another model
    // (mix.model_version), which it cannot do for a model it has not been sent yet
    pushInputs();
    check(iqhip_mix_weights_em(engine, max_steps, getAlnNSite(), weights, p_invar, nsteps, converged, trace), "iqhip_mix_weights_em");
}

double PhyloTree::optimizeMixtureWeights(double *p_invar, int *nsteps, int *converged) {
    needEngine("optimizeMixtureWeights");
    if (nmixture < 2) throw std::runtime_error("optimizeMixtureWeights: the model is no mixture");
    if (!current_it) computeLikelihood();
    computePatternLhCat(WSL_MIXTURE, nullptr);
    const std::vector<double> w_old = getMixtureWeights();
    std::vector<double> w(w_old);
    const double pinv_old = p_invar ? *p_invar : 0.0;
    int n = 0, conv = 0;
    mixWeightsEM(nmixture, w.data(), p_invar, &n, &conv, nullptr);
    if (nsteps) *nsteps = n;
    if (converged) *converged = conv;
    for (int q = 0; q < ncat; q++) m_props[q] *= w[m_cat_class[q]] / w_old[m_cat_class[q]];
    if (p_invar && pinv_old > 0.0) {   // computePtnInvar is linear in p_invar
        const double v = *p_invar / pinv_old;
        for (double &x : ptn_invar) x *= v;
        weights_dirty = true;
    }
    inputs_dirty = model_dirty = true;
    theta_computed = false;
    clearAllPartialLH();
    return computeLikelihood();
}

void PhyloTree::computePatternStateFreq(const double *class_freq, double *ptn_state_freq) {
    needEngine("computePatternStateFreq");
    if (!class_freq || !ptn_state_freq) throw std::runtime_error("computePatternStateFreq: null argument");
    computePatternLhCat(WSL_MIXTURE, nullptr);
    check(iqhip_mix_posteriors(engine, class_freq, nullptr, ptn_state_freq), "iqhip_mix_posteriors");
}

void PhyloTree::classLnl(PhyloNeighbor *dad_branch, PhyloNode *dad, const double *class_weight, const double *class_invar,
                         double *lnl, int64_t *floored) {
    needEngine("classLnl");
    if (nmixture < 2) throw std::runtime_error("classLnl: the model is no mixture (candidates are the classes of a mixture)");
    PhyloNeighbor *back = dad_branch->node->findNeighbor(dad);
    if (!back) throw std::runtime_error("classLnl: not a branch");
    current_it = dad_branch;
    current_it_back = back;
    rebuildTheta(dad_branch, dad);
    check(iqhip_class_lnl(engine, branchEnd(dad_branch), branchEnd(back), dad_branch->length, class_weight, class_invar, lnl,
                          floored),
          "iqhip_class_lnl");
}

}  // namespace iqhost
