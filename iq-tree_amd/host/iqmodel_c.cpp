// iqmodel_c.cpp -- flat C view of the model / alignment producers (model_host.h, alignment_host.h)
// for ctypes; test and tool plumbing, not part of the drop-in boundary.
#include <string.h>

#include <memory>
#include <string>
#include <vector>

#include "alignment_host.h"
#include "model_host.h"
#include "partition_spec.h"
#include "supertree_host.h"

using namespace iqhost;

static thread_local std::string g_model_err;

#define IQM_TRY(body)                    \
    try {                                \
        body;                            \
        return 0;                        \
    } catch (const std::exception &ex) { \
        g_model_err = ex.what();         \
        return 1;                        \
    }

extern "C" {

const char *iqmodel_last_error(void) { return g_model_err.c_str(); }

int iqmodel_decompose(const double *rate_matrix, const double *state_freq, int n, int ignore_state_freq,
                      double *eval, double *evec, double *inv_evec) {
    IQM_TRY({
        EigenSystem es;
        decomposeRateMatrix(rate_matrix, state_freq, n, es, ignore_state_freq != 0);
        memcpy(eval, es.eval.data(), sizeof(double) * n);
        memcpy(evec, es.evec.data(), sizeof(double) * n * n);
        memcpy(inv_evec, es.inv_evec.data(), sizeof(double) * n * n);
    });
}
int iqmodel_gamma_rates(double shape, int ncat, int median, double p_invar, double *rates) {
    IQM_TRY(discreteGammaRates(shape, ncat, median != 0, p_invar, rates));
}
double iqmodel_ln_gamma(double a) { return cmpLnGamma(a); }
double iqmodel_incomplete_gamma(double x, double a) { return cmpIncompleteGamma(x, a, cmpLnGamma(a)); }
double iqmodel_point_normal(double p) { return cmpPointNormal(p); }
double iqmodel_point_chi2(double p, double v) { return cmpPointChi2(p, v); }
const char *iqmodel_genetic_code(int table) { return geneticCode(table); }

// ---- alignment ---------------------------------------------------------------------------
int iqaln_read(void **out, const char *filename_or_null, const char *content_or_null, const char *seq_type) {
    *out = nullptr;
    Alignment *a = new Alignment();
    try {
        if (filename_or_null) a->readFile(filename_or_null, seq_type ? seq_type : "");
        else a->readString(content_or_null, seq_type ? seq_type : "");
        *out = a;
        return 0;
    } catch (const std::exception &ex) {
        g_model_err = ex.what();
        delete a;
        return 1;
    }
}
void iqaln_destroy(void *h) { delete (Alignment *)h; }
int iqaln_nseq(void *h) { return ((Alignment *)h)->getNSeq(); }
int iqaln_nsite(void *h) { return ((Alignment *)h)->getNSite(); }
int iqaln_npattern(void *h) { return ((Alignment *)h)->getNPattern(); }
int iqaln_nstates(void *h) { return ((Alignment *)h)->num_states; }
int iqaln_seq_type(void *h) { return (int)((Alignment *)h)->seq_type; }
int iqaln_state_unknown(void *h) { return ((Alignment *)h)->STATE_UNKNOWN; }
double iqaln_frac_const_sites(void *h) { return ((Alignment *)h)->frac_const_sites; }
const char *iqaln_seq_name(void *h, int i) { return ((Alignment *)h)->seq_names[i].c_str(); }
int iqaln_append_unobserved(void *h, int *n_out) { IQM_TRY(*n_out = ((Alignment *)h)->appendUnobservedConstPatterns()); }
int iqaln_get(void *h, uint8_t *states, double *ptn_freq, int *site_pattern, int *const_char) {
    IQM_TRY({
        Alignment *a = (Alignment *)h;
        std::vector<uint8_t> s;
        std::vector<double> f;
        a->statesByLeaf(s);
        a->ptnFreq(f);
        if (states) memcpy(states, s.data(), s.size());
        if (ptn_freq) memcpy(ptn_freq, f.data(), f.size() * sizeof(double));
        if (site_pattern) memcpy(site_pattern, a->site_pattern.data(), a->site_pattern.size() * sizeof(int));
        if (const_char)
            for (size_t p = 0; p < a->patterns.size(); p++) const_char[p] = a->patterns[p].is_const ? a->patterns[p].const_char : -1;
    });
}
int iqaln_num_informative_sites(void *h) { return ((Alignment *)h)->num_informative_sites; }
int iqaln_informative(void *h, uint8_t *out) {
    IQM_TRY({
        Alignment *a = (Alignment *)h;
        for (size_t p = 0; p < a->patterns.size(); p++) out[p] = a->patterns[p].is_informative ? 1 : 0;
    });
}
int iqaln_ptn_invar(void *h, double p_invar, const double *state_freq, double *out) {
    IQM_TRY({
        std::vector<double> v;
        ((Alignment *)h)->ptnInvar(p_invar, state_freq, v);
        memcpy(out, v.data(), v.size() * sizeof(double));
    });
}
int iqaln_state_freq(void *h, double *out) { IQM_TRY(((Alignment *)h)->computeStateFreq(out)); }
int iqaln_codon_freq(void *h, int f3x4, double *state_freq, double *ntfreq) {
    IQM_TRY(((Alignment *)h)->computeCodonFreq(f3x4 != 0, state_freq, ntfreq));
}
int iqaln_write_sitelh(void *h, const char *filename, const double *pattern_lh) {
    IQM_TRY(writeSiteLh(filename, *(Alignment *)h, pattern_lh));
}

// ---- -m string -> kernel inputs -------------------------------------------------------------
// out arrays sized by the caller: eval[n], evec[n*n], inv_evec[n*n], state_freq[n], rates[64], props[64]
int iqmodel_build(void *aln, const char *model_string, int *ncat, double *p_invar, int *asc, double *eval,
                  double *evec, double *inv_evec, double *state_freq, double *rates, double *props) {
    IQM_TRY({
        ModelSpec spec = parseModelString(model_string);
        if (!spec.mix_classes.empty()) throw std::runtime_error("a MIX{} model takes iqmodel_build_mixture");
        if (spec.ncat > 64) throw std::runtime_error("too many rate categories");
        ModelInputs mi;
        buildModel(spec, *(Alignment *)aln, mi);
        const int n = mi.nstates;
        *ncat = mi.ncat;
        *p_invar = mi.p_invar;
        *asc = spec.ascertainment;
        memcpy(eval, mi.eig.eval.data(), sizeof(double) * n);
        memcpy(evec, mi.eig.evec.data(), sizeof(double) * n * n);
        memcpy(inv_evec, mi.eig.inv_evec.data(), sizeof(double) * n * n);
        memcpy(state_freq, mi.state_freq.data(), sizeof(double) * n);
        memcpy(rates, mi.rates.data(), sizeof(double) * mi.ncat);
        memcpy(props, mi.props.data(), sizeof(double) * mi.ncat);
    });
}

// MIX{...} strings.  iqmodel_mixture_dims: the class and component counts (nclass = 1, ncat = the rate categories for a
// plain model); iqmodel_build_mixture: out arrays sized from them -- eval [nclass * n], evec / inv_evec [nclass * n * n],
// class_freq [nclass * n], state_freq [n] (the weighted mean), cat_class / rates / props [ncat], class_rates /
// class_weights [nclass]
int iqmodel_mixture_dims(void *aln, const char *model_string, int *nclass, int *ncat) {
    IQM_TRY({
        const ModelSpec spec = parseModelString(model_string);
        const int M = spec.mix_classes.empty() ? 1 : (int)spec.mix_classes.size();
        const int limit = maxModelComponents(((Alignment *)aln)->num_states);
        if (!spec.mix_classes.empty() && (long long)M * spec.ncat > limit)
            throw std::runtime_error("MIX{}: " + std::to_string((long long)M * spec.ncat) + " components; an engine of " +
                                     std::to_string(((Alignment *)aln)->num_states) + " states takes at most " + std::to_string(limit));
        *nclass = M;
        *ncat = M * spec.ncat;
    });
}
int iqmodel_build_mixture(void *aln, const char *model_string, double *p_invar, int *asc, double *eval, double *evec,
                          double *inv_evec, double *class_freq, double *state_freq, int *cat_class, double *rates,
                          double *props, double *class_rates, double *class_weights) {
    IQM_TRY({
        ModelSpec spec = parseModelString(model_string);
        if (spec.mix_classes.empty()) throw std::runtime_error("iqmodel_build_mixture: not a MIX{} model");
        ModelInputs mi;
        buildModel(spec, *(Alignment *)aln, mi);
        const size_t n = (size_t)mi.nstates;
        const size_t M = (size_t)mi.nclass;
        const size_t C = (size_t)mi.ncat;
        *p_invar = mi.p_invar;
        *asc = spec.ascertainment;
        memcpy(eval, mi.eig.eval.data(), sizeof(double) * M * n);
        memcpy(evec, mi.eig.evec.data(), sizeof(double) * M * n * n);
        memcpy(inv_evec, mi.eig.inv_evec.data(), sizeof(double) * M * n * n);
        memcpy(class_freq, mi.class_freq.data(), sizeof(double) * M * n);
        memcpy(state_freq, mi.state_freq.data(), sizeof(double) * n);
        memcpy(cat_class, mi.cat_class.data(), sizeof(int) * C);
        memcpy(rates, mi.rates.data(), sizeof(double) * C);
        memcpy(props, mi.props.data(), sizeof(double) * C);
        memcpy(class_rates, mi.class_rates.data(), sizeof(double) * M);
        memcpy(class_weights, mi.class_weights.data(), sizeof(double) * M);
    });
}

// ---- partition files (partition_spec.h, supertree_host.h) ----------------------------------------------------------------
// the parser alone: *out = a list of PartitionSpec for iqpart_spec_*; nsite = sites of the alignment the positions refer to
int iqpart_spec_parse(void **out, const char *text, int nsite) {
    *out = nullptr;
    IQM_TRY(*out = new std::vector<PartitionSpec>(parsePartitionFile(text ? text : "", nsite)));
}
void iqpart_spec_free(void *h) { delete (std::vector<PartitionSpec> *)h; }
int iqpart_spec_count(void *h) { return (int)((std::vector<PartitionSpec> *)h)->size(); }
const char *iqpart_spec_model(void *h, int k) { return (*(std::vector<PartitionSpec> *)h)[(size_t)k].model.c_str(); }
const char *iqpart_spec_name(void *h, int k) { return (*(std::vector<PartitionSpec> *)h)[(size_t)k].name.c_str(); }
int iqpart_spec_nsites(void *h, int k) { return (int)(*(std::vector<PartitionSpec> *)h)[(size_t)k].sites.size(); }
int iqpart_spec_sites(void *h, int k, int *out) {
    IQM_TRY({
        const std::vector<int> &v = (*(std::vector<PartitionSpec> *)h).at((size_t)k).sites;
        for (size_t i = 0; i < v.size(); i++) out[i] = v[i];
    });
}
// the whole reader: one alignment (file or content) + one partition file (file or content) -> a list of PartitionInput
int iqpart_read(void **out, const char *aln_file, const char *aln_content, const char *part_file, const char *part_content) {
    *out = nullptr;
    IQM_TRY({
        std::vector<std::string> names;
        std::unique_ptr<std::vector<PartitionInput>> parts(new std::vector<PartitionInput>());
        if (aln_file && part_file) readPartitionRaxml(aln_file, part_file, names, *parts);
        else if (aln_content && part_content) readPartitionStrings(aln_content, part_content, names, *parts);
        else throw std::runtime_error("iqpart_read: give both files or both contents");
        *out = parts.release();
    });
}
void iqpart_free(void *h) { delete (std::vector<PartitionInput> *)h; }
int iqpart_count(void *h) { return (int)((std::vector<PartitionInput> *)h)->size(); }
const char *iqpart_model(void *h, int k) { return (*(std::vector<PartitionInput> *)h)[(size_t)k].model.c_str(); }
const char *iqpart_name(void *h, int k) { return (*(std::vector<PartitionInput> *)h)[(size_t)k].name.c_str(); }
// a copy of partition k's alignment as an iqaln_* handle of its own (iqaln_destroy frees it)
int iqpart_alignment(void *h, int k, void **aln) {
    *aln = nullptr;
    IQM_TRY(*aln = new Alignment((*(std::vector<PartitionInput> *)h).at((size_t)k).aln));
}

}  // extern "C"
