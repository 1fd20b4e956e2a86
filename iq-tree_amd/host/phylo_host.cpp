// phylo_host.cpp -- see phylo_host.h.  Host logic only; all arithmetic on partial-likelihood
// vectors happens in libiqhip.so.  This unit: tree, inputs, engine, dispatch, buffers, likelihood and branch lengths; the
// features on top have a unit each (phylo_nni, phylo_support, phylo_dist, phylo_pars, phylo_em, phylo_ufboot .cpp).
#include <time.h>
#include "phylo_host.h"
#include "mirror_policy.h"

#include <assert.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>

namespace iqhost {

// log(2^-256), phylotree.h:53
static const double LOG_SCALING_THRESHOLD = log(0x1p-256);

// =========================================================================================
// flags (phylonode.cpp:15-65)
// =========================================================================================
void PhyloNeighbor::clearForwardPartialLh(PhyloNode *dad) {
    clearPartialLh();
    for (PhyloNeighbor *nb : node->neighbors)
        if (nb->node != dad) nb->clearForwardPartialLh(node);
}

void PhyloNode::clearReversePartialLh(PhyloNode *dad) {
    for (PhyloNeighbor *nb : neighbors)
        if (nb->node != dad) {
            nb->node->findNeighbor(this)->partial_lh_computed = 0;
            nb->node->clearReversePartialLh(this);
        }
}

void PhyloNode::clearAllPartialLh(bool make_null, PhyloNode *dad) {
    PhyloNeighbor *nei = findNeighbor(dad);
    nei->partial_lh_computed = 0;
    if (make_null) nei->partial_lh = 0;
    nei = dad->findNeighbor(this);
    nei->partial_lh_computed = 0;
    if (make_null) nei->partial_lh = 0;
    for (PhyloNeighbor *nb : neighbors)
        if (nb->node != dad) nb->node->clearAllPartialLh(make_null, this);
}

// =========================================================================================
// tree
// =========================================================================================
PhyloTree::PhyloTree() { setLikelihoodKernel(LK_EIGEN_HIP); }

PhyloTree::~PhyloTree() {
    if (engine) iqhip_destroy(engine);
    freeTree();
}

void PhyloTree::freeTree() {
    for (PhyloNeighbor *nb : all_neighbors) delete nb;
    for (PhyloNode *n : nodes) delete n;
    all_neighbors.clear();
    nodes.clear();
    root = nullptr;
    current_it = current_it_back = nullptr;
    pars_initialized = false;   // (the new tree's vectors have no slots yet)
}

namespace {
struct NwkNode {
    std::string label;
    double len = 0.0;
    bool has_len = false;
    std::vector<NwkNode *> kids;
    ~NwkNode() { for (NwkNode *k : kids) delete k; }
};

struct NwkParser {
    const std::string &s;
    size_t pos = 0;
    explicit NwkParser(const std::string &str) : s(str) {}
    void skip() { while (pos < s.size() && isspace((unsigned char)s[pos])) pos++; }
    NwkNode *parse() {
        skip();
        NwkNode *n = new NwkNode();
        if (pos < s.size() && s[pos] == '(') {
            pos++;
            for (;;) {
                n->kids.push_back(parse());
                skip();
                if (pos >= s.size()) { delete n; throw std::runtime_error("newick: unexpected end"); }
                if (s[pos] == ',') { pos++; continue; }
                if (s[pos] == ')') { pos++; break; }
                delete n;
                throw std::runtime_error("newick: expected ',' or ')'");
            }
        }
        skip();
        size_t b = pos;
        while (pos < s.size() && !strchr(":,();", s[pos]) && !isspace((unsigned char)s[pos])) pos++;
        n->label = s.substr(b, pos - b);
        skip();
        if (pos < s.size() && s[pos] == ':') {
            pos++;
            skip();
            char *end = nullptr;
            n->len = strtod(s.c_str() + pos, &end);
            if (end == s.c_str() + pos) { delete n; throw std::runtime_error("newick: bad branch length"); }
            pos = end - s.c_str();
            n->has_len = true;
        }
        return n;
    }
};
}  // namespace

void PhyloTree::readTreeString(const std::string &newick, const std::vector<std::string> &names) {
    deleteAllPartialLh();
    freeTree();
    NwkParser P(newick);
    NwkNode *top = P.parse();
    struct Guard { NwkNode *p; ~Guard() { delete p; } } guard{top};

    // count leaves
    std::vector<NwkNode *> stack{top};
    int nleaf = 0;
    while (!stack.empty()) {
        NwkNode *n = stack.back();
        stack.pop_back();
        if (n->kids.empty()) nleaf++;
        for (NwkNode *k : n->kids) stack.push_back(k);
    }
    if (nleaf < 3) throw std::runtime_error("tree needs at least 3 taxa");
    if (!names.empty() && (int)names.size() != nleaf)
        throw std::runtime_error("newick leaf count differs from the number of sequences");
    leafNum = nleaf;
    nodes.assign(nleaf, nullptr);
    int branch_id = 0;

    auto connect = [&](PhyloNode *a, PhyloNode *b, double len) {
        PhyloNeighbor *ab = new PhyloNeighbor(), *ba = new PhyloNeighbor();
        ab->node = b; ab->length = len; ab->id = branch_id;
        ba->node = a; ba->length = len; ba->id = branch_id;
        branch_id++;
        a->neighbors.push_back(ab);
        b->neighbors.push_back(ba);
        all_neighbors.push_back(ab);
        all_neighbors.push_back(ba);
    };
    auto leaf_id = [&](const std::string &label) -> int {
        if (names.empty()) {
            char *end = nullptr;
            long v = strtol(label.c_str(), &end, 10);
            if (label.empty() || *end) throw std::runtime_error("leaf label '" + label + "' is not a taxon id");
            return (int)v;
        }
        for (size_t i = 0; i < names.size(); i++)
            if (names[i] == label) return (int)i;
        throw std::runtime_error("leaf label '" + label + "' not found in alignment");
    };
    // recursive build; returns the PhyloNode of a newick node
    struct Builder {
        PhyloTree *t; decltype(connect) &conn; decltype(leaf_id) &lid;
        PhyloNode *build(NwkNode *n) {
            PhyloNode *pn = new PhyloNode();
            if (n->kids.empty()) {
                int id = lid(n->label);
                if (id < 0 || id >= t->leafNum || t->nodes[id]) {
                    delete pn;
                    throw std::runtime_error("duplicate or out-of-range taxon '" + n->label + "'");
                }
                pn->id = id;
                pn->name = n->label;
                t->nodes[id] = pn;
            } else {
                pn->id = (int)t->nodes.size();
                pn->name = n->label;
                t->nodes.push_back(pn);
                for (NwkNode *k : n->kids) {
                    PhyloNode *c = build(k);
                    conn(pn, c, k->len);
                }
            }
            return pn;
        }
    } builder{this, connect, leaf_id};

    if (top->kids.size() == 2) {
        // rooted input: drop the degree-2 root, join its two children by one branch
        NwkNode *a = top->kids[0], *b = top->kids[1];
        if (a->kids.empty() && b->kids.empty()) throw std::runtime_error("tree needs at least 3 taxa");
        PhyloNode *na = builder.build(a), *nb = builder.build(b);
        connect(na, nb, a->len + b->len);
    } else {
        builder.build(top);
    }
    for (PhyloNode *n : nodes)
        if (!n) throw std::runtime_error("a taxon of the alignment is missing from the tree");
    nodeNum = (int)nodes.size();
    branchNum = branch_id;
    for (PhyloNode *n : nodes)
        if (!n->isLeaf() && n->degree() < 3) throw std::runtime_error("internal node of degree < 3");
    root = nodes[0];  // the reference roots at the first taxon by default (setRootNode)
    current_it = current_it_back = nullptr;
    theta_computed = false;
}

void PhyloTree::copyTopology(const PhyloTree &src) {
    if (&src == this) return;
    deleteAllPartialLh();
    freeTree();
    leafNum = src.leafNum;
    nodeNum = src.nodeNum;
    branchNum = src.branchNum;
    nodes.assign(src.nodes.size(), nullptr);
    for (size_t i = 0; i < src.nodes.size(); i++) {
        PhyloNode *pn = new PhyloNode();
        pn->id = src.nodes[i]->id;
        pn->name = src.nodes[i]->name;
        nodes[i] = pn;
    }
    for (size_t i = 0; i < src.nodes.size(); i++)
        for (const PhyloNeighbor *snb : src.nodes[i]->neighbors) {
            PhyloNeighbor *nb = new PhyloNeighbor();
            nb->node = nodes[(size_t)snb->node->id];
            nb->length = snb->length;
            nb->id = snb->id;
            nodes[i]->neighbors.push_back(nb);
            all_neighbors.push_back(nb);
        }
    root = src.root ? nodes[(size_t)src.root->id] : nullptr;
    current_it = current_it_back = nullptr;
    theta_computed = false;
}

void PhyloTree::copyBranchLengths(const PhyloTree &src) {
    if (src.nodes.size() != nodes.size()) throw std::runtime_error("copyBranchLengths: the trees differ");
    for (size_t i = 0; i < nodes.size(); i++) {
        const std::vector<PhyloNeighbor *> &a = nodes[i]->neighbors, &b = src.nodes[i]->neighbors;
        if (a.size() != b.size()) throw std::runtime_error("copyBranchLengths: the trees differ");
        for (size_t k = 0; k < a.size(); k++) {
            if (a[k]->node->id != b[k]->node->id) throw std::runtime_error("copyBranchLengths: the trees differ");
            a[k]->length = b[k]->length;
        }
    }
    theta_computed = false;
}

std::string PhyloTree::getTreeString() const {   // (the labelled writer of phylo_support.cpp with no labels)
    return root ? labelledTreeString(std::vector<std::string>(nodes.size())) : ";";
}

PhyloNode *PhyloTree::findFarthestLeaf(PhyloNode *node, PhyloNode *dad) {
    if (!node) node = root;
    if (dad && node->isLeaf()) {
        node->height = 0.0;
        return node;
    }
    PhyloNode *res = nullptr;
    node->height = 0.0;
    for (PhyloNeighbor *nb : node->neighbors)
        if (nb->node != dad) {
            PhyloNode *leaf = findFarthestLeaf(nb->node, node);
            if (node->height < nb->node->height + 1) {
                node->height = nb->node->height + 1;
                res = leaf;
            }
        }
    return res;
}

// =========================================================================================
// inputs
// =========================================================================================
void PhyloTree::setAlignment(int nstates, SeqType st, int64_t nptn_, const uint8_t *states,
                             const double *freq, const double *invar) {
    if (engine) throw std::runtime_error("setAlignment after attachEngine is not supported");
    if (leafNum <= 0) throw std::runtime_error("readTreeString first");
    num_states = nstates;
    seq_type = st;
    nptn = nptn_;
    // alignment.cpp:470-472
    STATE_UNKNOWN = (st == SEQ_DNA && nstates == 4) ? 18 : (st == SEQ_PROTEIN && nstates == 20) ? 23 : nstates;
    aln_states.assign(states, states + (size_t)leafNum * nptn);
    ptn_freq.assign(freq, freq + nptn);
    ptn_invar.assign(invar, invar + nptn);
    inputs_dirty = aln_dirty = true;
}

void PhyloTree::setPtnFreq(const double *f) {
    if (nptn <= 0) throw std::runtime_error("setAlignment first");
    ptn_freq.assign(f, f + nptn);
    inputs_dirty = weights_dirty = true;
    pars_initialized = false;   // (the parsimony sites follow the frequencies)
}

void PhyloTree::setPtnInvar(const double *v) {
    if (nptn <= 0) throw std::runtime_error("setAlignment first");
    ptn_invar.assign(v, v + nptn);
    inputs_dirty = weights_dirty = true;
}

void PhyloTree::setAscertainment(int64_t n_unobs, double nsites) {
    if (n_unobs < 0 || n_unobs >= nptn) throw std::runtime_error("setAscertainment: bad pattern count");
    n_unobserved = n_unobs;
    asc_nsites = nsites;
    inputs_dirty = aln_dirty = true;
}

void PhyloTree::setModel(int ncat_, const double *eval, const double *evec, const double *inv_evec,
                         const double *rates, const double *props) {
    setMixtureModel(1, ncat_, nullptr, eval, evec, inv_evec, rates, props);
}

void PhyloTree::setMixtureModel(int nclass, int ncat_, const int *cat_class, const double *eval, const double *evec,
                                const double *inv_evec, const double *rates, const double *props) {
    if (num_states <= 0) throw std::runtime_error("setAlignment first");
    if (engine && ncat_ != ncat) throw std::runtime_error("ncat cannot change after attachEngine");
    if (nclass < 1 || (nclass > 1 && !cat_class)) throw std::runtime_error("bad mixture description");
    const int n = num_states;
    ncat = ncat_;
    nmixture = nclass;
    m_eval.assign(eval, eval + (size_t)nclass * n);
    m_evec.assign(evec, evec + (size_t)nclass * n * n);
    m_inv_evec.assign(inv_evec, inv_evec + (size_t)nclass * n * n);
    m_rates.assign(rates, rates + ncat);
    m_props.assign(props, props + ncat);
    m_cat_class.assign(ncat, 0);
    if (nclass > 1) m_cat_class.assign(cat_class, cat_class + ncat);
    computeTipPartialLikelihood();
    inputs_dirty = model_dirty = true;
    theta_computed = false;
}

// phylotreesse.cpp:359-529; for mixtures tip_partial_lh[state][class][i] (:395-458)
void PhyloTree::computeTipPartialLikelihood() {
    const int n = num_states, M = nmixture;
    tip_partial_lh.assign((size_t)(STATE_UNKNOWN + 1) * M * n, 0.0);
    for (int m = 0; m < M; m++) {
        const double *inv_evec = m_inv_evec.data() + (size_t)m * n * n;
        auto tip = [&](int state) { return &tip_partial_lh[((size_t)state * M + m) * n]; };
        for (int state = 0; state < n; state++)
            for (int i = 0; i < n; i++) tip(state)[i] = inv_evec[i * n + state];
        for (int i = 0; i < n; i++) {  // unknown character: sum over all states
            double lh_unknown = 0.0;
            for (int x = 0; x < n; x++) lh_unknown += inv_evec[i * n + x];
            tip(STATE_UNKNOWN)[i] = lh_unknown;
        }
        if (seq_type == SEQ_DNA && n == 4) {
            for (int state = 4; state < 18; state++) {  // IUPAC ambiguity = bitmask state-3
                const int cstate = state - n + 1;
                for (int i = 0; i < n; i++) {
                    double lh = 0.0;
                    for (int x = 0; x < n; x++)
                        if (cstate & (1 << x)) lh += inv_evec[i * n + x];
                    tip(state)[i] = lh;
                }
            }
        } else if (seq_type == SEQ_PROTEIN && n == 20) {
            const int ambi_aa[3] = {4 + 8, 32 + 64, 512 + 1024};  // B, Z, U
            for (int k = 0; k < 3; k++)
                for (int i = 0; i < n; i++) {
                    double lh = 0.0;
                    for (int x = 0; x < 11; x++)
                        if (ambi_aa[k] & (1 << x)) lh += inv_evec[i * n + x];
                    tip(20 + k)[i] = lh;
                }
        }
    }
}

void PhyloTree::check(int rc, const char *what) const {
    if (rc != IQHIP_OK) throw std::runtime_error(std::string(what) + ": " + iqhip_last_error());
}

void PhyloTree::needEngine(const char *who) const {
    if (!engine) throw std::runtime_error(std::string(who) + " needs an attached engine");
}

void PhyloTree::needDevice(const char *who) const {
    if (!engine || dry_run) throw std::runtime_error(std::string(who) + " needs an attached engine");
}

void PhyloTree::noCallerCollective(const char *who) const {
    if (allreduce_hook) throw std::runtime_error(std::string(who) + ": not available with a caller-owned collective");
}

void PhyloTree::attachEngine(int device) {
    if (engine) throw std::runtime_error("engine already attached");
    if (m_eval.empty() || aln_states.empty()) throw std::runtime_error("setAlignment and setModel first");
    check(iqhip_create(&engine, device, num_states, ncat, nptn, leafNum), "iqhip_create");
    engine_device = device;
    finishAttach();
}

void PhyloTree::attachEngineSharded(const int *device_ids, int ndev, int reduce_mode) {
    if (engine) throw std::runtime_error("engine already attached");
    if (m_eval.empty() || aln_states.empty()) throw std::runtime_error("setAlignment and setModel first");
    check(iqhip_create_sharded(&engine, device_ids, ndev, reduce_mode, num_states, ncat, nptn, leafNum),
          "iqhip_create_sharded");
    finishAttach();
}

void PhyloTree::finishAttach() {   // a new engine gets every input and the vector arena
    inputs_dirty = model_dirty = aln_dirty = true;
    pushInputs();
    // the reference's arena: leafNum-2 vectors (LM_PER_NODE) or 3*leafNum-6 (phylotree.cpp:867-873)
    int nvec = (lh_mem_save == LM_PER_NODE) ? (leafNum - 2) : (3 * leafNum - 6);
    check(iqhip_reserve(engine, nvec), "iqhip_reserve");
}

void PhyloTree::attachComm(int nranks, int rank, const void *unique_id) {
    if (!engine) throw std::runtime_error("attachEngine first");
    check(iqhip_comm_init_rank(engine, nranks, rank, unique_id), "iqhip_comm_init_rank");
}

std::vector<std::string> PhyloTree::leafNames() const {
    std::vector<std::string> names((size_t)leafNum);
    for (int i = 0; i < leafNum; i++) names[(size_t)i] = nodes[(size_t)i]->name.empty() ? std::to_string(i) : nodes[(size_t)i]->name;
    return names;
}

void PhyloTree::pushInputs() {
    if (!engine || !inputs_dirty) return;
    // a model change re-sends the model only: the alignment (megabytes of state rows) stays where it is
    if (model_dirty) {
        if (nmixture > 1)
            check(iqhip_set_mixture_model(engine, nmixture, m_cat_class.data(), m_eval.data(), m_evec.data(),
                                          m_inv_evec.data(), m_rates.data(), m_props.data(), STATE_UNKNOWN,
                                          tip_partial_lh.data()),
                  "iqhip_set_mixture_model");
        else
            check(iqhip_set_model(engine, m_eval.data(), m_evec.data(), m_inv_evec.data(), m_rates.data(),
                                  m_props.data(), STATE_UNKNOWN, tip_partial_lh.data()),
                  "iqhip_set_model");
    }
    if (aln_dirty) {
        check(iqhip_set_alignment(engine, aln_states.data(), ptn_freq.data(), ptn_invar.data()),
              "iqhip_set_alignment");
        check(iqhip_set_ascertainment(engine, n_unobserved, asc_nsites), "iqhip_set_ascertainment");
    } else if (weights_dirty) {
        check(iqhip_set_ptn_freq(engine, ptn_freq.data()), "iqhip_set_ptn_freq");
        check(iqhip_set_ptn_invar(engine, ptn_invar.data()), "iqhip_set_ptn_invar");
    }
    inputs_dirty = model_dirty = aln_dirty = weights_dirty = false;
}

// =========================================================================================
// dispatch (phylotreesse.cpp:60-357)
// =========================================================================================
void PhyloTree::setLikelihoodKernel(LikelihoodKernel lk) {
    sse = lk;
    if (lk != LK_EIGEN_HIP) {
        computePartialLikelihoodPointer = nullptr;
        computeLikelihoodBranchPointer = nullptr;
        computeLikelihoodDervPointer = nullptr;
        computeLikelihoodFromBufferPointer = nullptr;
        throw std::runtime_error(
            "setLikelihoodKernel: this build ships no CPU kernel; only LK_EIGEN_HIP is available");
    }
    computePartialLikelihoodPointer = &PhyloTree::computePartialLikelihoodHIP;
    computeLikelihoodBranchPointer = &PhyloTree::computeLikelihoodBranchHIP;
    computeLikelihoodDervPointer = &PhyloTree::computeLikelihoodDervHIP;
    computeLikelihoodFromBufferPointer = &PhyloTree::computeLikelihoodFromBufferHIP;
    setParsimonyKernel(lk);
}

void PhyloTree::setParsimonyKernel(LikelihoodKernel) {  // phylotreesse.cpp:34-58 (one device form for every kernel choice)
    computePartialParsimonyPointer = &PhyloTree::computePartialParsimonyHIP;
    computeParsimonyBranchPointer = &PhyloTree::computeParsimonyBranchHIP;
}

void PhyloTree::computePartialLikelihood(PhyloNeighbor *dad_branch, PhyloNode *dad) {
    (this->*computePartialLikelihoodPointer)(dad_branch, dad);
}
double PhyloTree::computeLikelihoodBranch(PhyloNeighbor *dad_branch, PhyloNode *dad) {
    return (this->*computeLikelihoodBranchPointer)(dad_branch, dad);
}
void PhyloTree::computeLikelihoodDerv(PhyloNeighbor *dad_branch, PhyloNode *dad, double &df, double &ddf) {
    (this->*computeLikelihoodDervPointer)(dad_branch, dad, df, ddf);
}
double PhyloTree::computeLikelihoodFromBuffer() {
    assert(current_it && current_it_back);
    if (computeLikelihoodFromBufferPointer) return (this->*computeLikelihoodFromBufferPointer)();
    return (this->*computeLikelihoodBranchPointer)(current_it, current_it_back->node);
}

// =========================================================================================
// buffers (phylotree.cpp:667-716, 834-987)
// =========================================================================================
void PhyloTree::initializeAllPartialLh() {
    if (!root) throw std::runtime_error("no tree");
    // depth-first from the root leaf, as initializeAllPartialLh(index, indexlh, node, dad)
    struct Rec {
        PhyloTree *t;
        void go(PhyloNode *node, PhyloNode *dad) {
            if (dad) {
                PhyloNeighbor *nei = node->findNeighbor(dad);   // node -> dad
                PhyloNeighbor *nei2 = dad->findNeighbor(node);  // dad -> node
                if (t->lh_mem_save == LM_PER_NODE) {
                    nei->partial_lh = 0;
                    nei2->partial_lh = node->isLeaf() ? 0 : t->next_key++;
                } else {
                    nei->partial_lh = nei->node->isLeaf() ? 0 : t->next_key++;
                    nei2->partial_lh = nei2->node->isLeaf() ? 0 : t->next_key++;
                }
            }
            for (PhyloNeighbor *nb : node->neighbors)
                if (nb->node != dad) go(nb->node, node);
        }
    } rec{this};
    rec.go(root, nullptr);
    central_partial_lh = true;
}

void PhyloTree::deleteAllPartialLh() {
    for (PhyloNeighbor *nb : all_neighbors) {
        if (nb->partial_lh && engine) iqhip_release(engine, nb->partial_lh);
        nb->partial_lh = 0;
        nb->partial_lh_computed = 0;
    }
    central_partial_lh = false;
}

void PhyloTree::clearAllPartialLH() {
    if (!root) return;
    root->neighbors[0]->node->clearAllPartialLh(false, root);
    current_it = current_it_back = nullptr;
}

iqhip_branch_end PhyloTree::branchEnd(PhyloNeighbor *nei) const { return iqhip_adapter::branchEnd<MirrorPolicy>(nei); }

void PhyloTree::computePartialLikelihoodHIP(PhyloNeighbor *dad_branch, PhyloNode *dad) {
    MirrorPolicy::Plan plan;
    iqhip_adapter::computePartialLikelihood<MirrorPolicy>(this, dad_branch, dad, &plan);
    if (plan.empty()) last_plan.clear();
}

double PhyloTree::computeLikelihoodBranchHIP(PhyloNeighbor *dad_branch, PhyloNode *dad) {
    return iqhip_adapter::computeLikelihoodBranch<MirrorPolicy>(this, dad_branch, dad);
}

void PhyloTree::computeLikelihoodDervHIP(PhyloNeighbor *dad_branch, PhyloNode *dad, double &df, double &ddf) {
    iqhip_adapter::computeLikelihoodDerv<MirrorPolicy>(this, dad_branch, dad, df, ddf);
}

double PhyloTree::computeLikelihoodFromBufferHIP() {
    assert(current_it && current_it_back);
    return iqhip_adapter::computeLikelihoodFromBuffer<MirrorPolicy>(this);
}

void PhyloTree::collectBranchPlan(PhyloNeighbor *dad_branch, PhyloNode *dad, std::vector<iqhip_node_op> &ops,
                                  std::vector<int> &len_branch, iqhip_branch_end &a, iqhip_branch_end &b, int &root_branch) {
    PhyloNode *node;
    PhyloNeighbor *node_branch;
    MirrorPolicy::ensureBuffers(this);
    iqhip_adapter::orientBranch<MirrorPolicy>(dad_branch, dad, node_branch, node);
    MirrorPolicy::Plan plan;
    if ((dad_branch->partial_lh_computed & 1) == 0) iqhip_adapter::collectPlan<MirrorPolicy>(this, dad_branch, dad, plan);
    if ((node_branch->partial_lh_computed & 1) == 0) iqhip_adapter::collectPlan<MirrorPolicy>(this, node_branch, node, plan);
    pushInputs();
    ops = plan.ops;
    len_branch.assign(2 * plan.size(), -1);
    for (size_t q = 0; q < len_branch.size(); q++)
        if (plan.len_nb[q]) len_branch[q] = plan.len_nb[q]->id;
    a = branchEnd(node_branch);
    b = branchEnd(dad_branch);
    root_branch = dad_branch->id;
}

// =========================================================================================
// callers
// =========================================================================================
double PhyloTree::computeLikelihood(double *pattern_lh) {
    if (!root || !root->isLeaf()) throw std::runtime_error("computeLikelihood: no rooted-at-leaf tree");
    if (!current_it) {
        PhyloNode *leaf = findFarthestLeaf();
        current_it = leaf->neighbors[0];
        current_it_back = current_it->node->findNeighbor(leaf);
    }
    double score = computeLikelihoodBranch(current_it, current_it_back->node);
    if (pattern_lh) {
        fetchPatternLh(pattern_lh);
        if (current_it->lh_scale_factor < 0.0) {  // phylotree.cpp:1059-1069
            std::vector<UBYTE> sc((size_t)nptn);
            fetchScaleNum(current_it, sc.data());
            for (int64_t i = 0; i < nptn - n_unobserved; i++)
                pattern_lh[i] += std::max(sc[i], UBYTE(0)) * LOG_SCALING_THRESHOLD;
        }
    }
    curScore = score;
    return score;
}

double PhyloTree::computeFuncDerv(double value, double &df, double &ddf) {
    current_it->length = value;
    current_it_back->length = value;
    computeLikelihoodDerv(current_it, current_it_back->node, df, ddf);
    df = -df;
    ddf = -ddf;
    return 0.0;
}

// optimization.cpp:388-465 restated (Newton-Raphson with bisection safeguard on f = -dlnL/dt)
double PhyloTree::minimizeNewton(double x1, double xguess, double x2, double xacc, double &d2l, int maxNRStep) {
    double df, dx, f, temp, xh, xl, rts, rts_old;
    rts = xguess;
    if (rts < x1) rts = x1;
    if (rts > x2) rts = x2;
    computeFuncDerv(rts, f, df);
    d2l = df;
    if (!isfinite(f) || !isfinite(df)) throw std::runtime_error("Wrong computeFuncDerv");
    if (df >= 0.0 && fabs(f) < xacc) return rts;
    if (f < 0.0) { xl = rts; xh = x2; } else { xh = rts; xl = x1; }
    dx = fabs(xh - xl);
    for (int j = 1; j <= maxNRStep; j++) {
        rts_old = rts;
        if ((df <= 0.0) || (((rts - xh) * df - f) * ((rts - xl) * df - f) >= 0.0)) {
            dx = 0.5 * (xh - xl);
            rts = xl + dx;
            d2l = df;
            if (xl == rts) return rts;
        } else {
            dx = f / df;
            temp = rts;
            rts -= dx;
            d2l = df;
            if (temp == rts) return rts;
        }
        if (fabs(dx) < xacc || (j == maxNRStep)) return rts_old;
        computeFuncDerv(rts, f, df);
        if (!isfinite(f) || !isfinite(df)) throw std::runtime_error("Wrong computeFuncDerv");
        if (df > 0.0 && fabs(f) < xacc) { d2l = df; return rts; }
        if (f < 0.0) xl = rts; else xh = rts;
    }
    throw std::runtime_error("Maximum number of iterations exceeded in minimizeNewton");
}

void PhyloTree::optimizeOneBranch(PhyloNode *node1, PhyloNode *node2, bool clearLH, int maxNRStep) {
    current_it = node1->findNeighbor(node2);
    current_it_back = node2->findNeighbor(node1);
    assert(current_it && current_it_back);
    const double current_len = current_it->length;
    theta_computed = false;
    double d2l;
    double optx;
    if (device_newton && engine && !dry_run && !allreduce_hook) {
        // one engine call: pending node updates of both ends + theta + the whole minimizeNewton solve (on a sharded
        // engine as an enqueued chain of steps with an in-stream all-reduce each); allreduce_hook is the legacy
        // caller-owned collective, which has to come back to the host between steps
        int nsteps = 0;
        optx = iqhip_adapter::minimizeNewtonOnBranch<MirrorPolicy>(this, current_len, maxNRStep, &nsteps);
        (void)d2l;
    } else {
        optx = minimizeNewton(min_branch_length, current_len, max_branch_length, min_branch_length, d2l, maxNRStep);
    }
    if (optx > max_branch_length * 0.95) {  // newton raphson diverged, reset (phylotree.cpp:2167-2176)
        // (both solvers leave the branch at the last evaluated length, as the reference's computeFuncDerv does)
        double opt_lh = computeLikelihoodFromBuffer();
        current_it->length = current_it_back->length = current_len;
        double orig_lh = computeLikelihoodFromBuffer();
        if (orig_lh > opt_lh) optx = current_len;
    }
    current_it->length = optx;
    current_it_back->length = optx;
    if (clearLH && current_len != optx) {
        node1->clearReversePartialLh(node2);
        node2->clearReversePartialLh(node1);
    }
}

void PhyloTree::getPreOrderBranches(std::vector<PhyloNode *> &n1, std::vector<PhyloNode *> &n2,
                                    PhyloNode *node, PhyloNode *dad) {
    if (dad) { n1.push_back(node); n2.push_back(dad); }
    std::vector<PhyloNeighbor *> neivec = node->neighbors;  // mtree.cpp:2102-2113: ascending height
    for (size_t i = 0; i < neivec.size(); i++)
        for (size_t j = i + 1; j < neivec.size(); j++)
            if (neivec[i]->node->height > neivec[j]->node->height) std::swap(neivec[i], neivec[j]);
    for (PhyloNeighbor *nb : neivec)
        if (nb->node != dad) getPreOrderBranches(n1, n2, nb->node, node);
}

double PhyloTree::optimizeAllBranches(int my_iterations, double tolerance, int maxNRStep) {
    std::vector<PhyloNode *> nodes1, nodes2;
    PhyloNode *farleaf = findFarthestLeaf();
    findFarthestLeaf(farleaf);  // phylotree.cpp:2241-2250
    getPreOrderBranches(nodes1, nodes2, farleaf, nullptr);
    double tree_lh = computeLikelihoodBranch(nodes1[0]->findNeighbor(nodes2[0]), nodes1[0]);
    for (int i = 0; i < my_iterations; i++) {
        std::vector<double> lenvec;
        for (PhyloNeighbor *nb : all_neighbors) lenvec.push_back(nb->length);
        if (device_sweep && device_newton && engine && !dry_run && !allreduce_hook) {
            // the whole loop as one engine submission (iqhip_adapter::optimizeBranchSweep -> iqhip_optimize_sweep)
            theta_computed = false;
            int nevals = 0;
            timespec ts0, ts1;
            static const bool dbg = getenv("IQHIP_DEBUG_SWEEP") != nullptr;
            if (dbg) clock_gettime(CLOCK_MONOTONIC, &ts0);
            iqhip_adapter::optimizeBranchSweep<MirrorPolicy>(this, nodes1.data(), nodes2.data(), (int)nodes1.size(), maxNRStep,
                                                            0.95, &nevals);
            if (dbg) {
                clock_gettime(CLOCK_MONOTONIC, &ts1);
                fprintf(stderr, "[iqhost] optimizeBranchSweep: %.1f us in all\n", (ts1.tv_sec - ts0.tv_sec) * 1e6 + (ts1.tv_nsec - ts0.tv_nsec) * 1e-3);
            }
            num_derv_calls += nevals;
            num_submissions++;
        } else {
            for (size_t j = 0; j < nodes1.size(); j++) optimizeOneBranch(nodes1[j], nodes2[j], true, maxNRStep);
        }
        double new_tree_lh = computeLikelihoodFromBuffer();
        if (new_tree_lh < tree_lh) {  // rare: restore and stop (phylotree.cpp:2303-2319)
            clearAllPartialLH();
            for (size_t k = 0; k < all_neighbors.size(); k++) all_neighbors[k]->length = lenvec[k];
            new_tree_lh = computeLikelihood();
            curScore = new_tree_lh;
            return new_tree_lh;
        }
        if (tree_lh <= new_tree_lh && new_tree_lh <= tree_lh + tolerance) { curScore = new_tree_lh; return new_tree_lh; }
        tree_lh = new_tree_lh;
    }
    curScore = tree_lh;
    return tree_lh;
}

// =========================================================================================
// host views
// =========================================================================================
void PhyloTree::fetchScaleNum(PhyloNeighbor *nei, UBYTE *out) {
    needEngine("fetchScaleNum");
    if (!nei->partial_lh) throw std::runtime_error("neighbor has no buffer");
    check(iqhip_fetch_scale_num(engine, nei->partial_lh, out), "iqhip_fetch_scale_num");
}
void PhyloTree::fetchPartialLh(PhyloNeighbor *nei, double *out) {
    needEngine("fetchPartialLh");
    if (!nei->partial_lh) throw std::runtime_error("neighbor has no buffer");
    check(iqhip_fetch_partial(engine, nei->partial_lh, out), "iqhip_fetch_partial");
}
void PhyloTree::fetchPatternLh(double *out) {
    needEngine("fetchPatternLh");
    check(iqhip_fetch_pattern_lh(engine, out), "iqhip_fetch_pattern_lh");
}

void PhyloTree::computePatternLikelihood(double *ptn_lh) {
    needEngine("computePatternLikelihood");
    if (!current_it) throw std::runtime_error("computePatternLikelihood before computeLikelihood");
    check(iqhip_fetch_pattern_lh_scaled(engine, branchEnd(current_it), branchEnd(current_it_back), ptn_lh),
          "iqhip_fetch_pattern_lh_scaled");
}

void PhyloTree::rebuildTheta(PhyloNeighbor *dad_branch, PhyloNode *dad) {   // through a derivative evaluation on that branch
    double df, ddf;
    theta_computed = false;
    computeLikelihoodDerv(dad_branch, dad, df, ddf);
}

void PhyloTree::computePatternLhCat(double *ptn_lh_cat) {
    needEngine("computePatternLhCat");
    if (!current_it) throw std::runtime_error("computePatternLhCat before computeLikelihood");
    rebuildTheta(current_it, current_it_back->node);
    check(iqhip_pattern_lh_cat(engine, current_it->length, ptn_lh_cat), "iqhip_pattern_lh_cat");
}

}  // namespace iqhost
