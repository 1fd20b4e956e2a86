// phylo_host.cpp -- see phylo_host.h.  Host logic only; all arithmetic on partial-likelihood
// vectors happens in libiqhip.so.
#include <time.h>
#include "phylo_host.h"
#include "ufboot_splits.h"
#include "brent_host.h"
#include "model_host.h"
#include "alignment_host.h"

#include <assert.h>
#include <float.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <sstream>

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

static void writeNewick(std::ostringstream &os, const PhyloNode *node, const PhyloNode *dad) {
    if (node->isLeaf() && dad) {
        if (node->name.empty()) os << node->id;  // leaf labels as read (MTree::printTree writes names)
        else os << node->name;
        return;
    }
    os << "(";
    bool first = true;
    for (PhyloNeighbor *nb : node->neighbors)
        if (nb->node != dad) {
            if (!first) os << ",";
            first = false;
            writeNewick(os, nb->node, node);
            os.precision(17);
            os << ":" << nb->length;
        }
    os << ")";
}

std::string PhyloTree::getTreeString() const {
    std::ostringstream os;
    if (!root) return ";";
    // print from the internal node next to the root leaf so the output is a trifurcation
    const PhyloNode *start = root->neighbors[0]->node;
    writeNewick(os, start, nullptr);
    os << ";";
    return os.str();
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

void PhyloTree::attachEngine(int device) {
    if (engine) throw std::runtime_error("engine already attached");
    if (m_eval.empty() || aln_states.empty()) throw std::runtime_error("setAlignment and setModel first");
    check(iqhip_create(&engine, device, num_states, ncat, nptn, leafNum), "iqhip_create");
    engine_device = device;
    inputs_dirty = model_dirty = aln_dirty = true;
    pushInputs();
    // the reference's arena: leafNum-2 vectors (LM_PER_NODE) or 3*leafNum-6 (phylotree.cpp:867-873)
    int nvec = (lh_mem_save == LM_PER_NODE) ? (leafNum - 2) : (3 * leafNum - 6);
    check(iqhip_reserve(engine, nvec), "iqhip_reserve");
}

void PhyloTree::attachEngineSharded(const int *device_ids, int ndev, int reduce_mode) {
    if (engine) throw std::runtime_error("engine already attached");
    if (m_eval.empty() || aln_states.empty()) throw std::runtime_error("setAlignment and setModel first");
    check(iqhip_create_sharded(&engine, device_ids, ndev, reduce_mode, num_states, ncat, nptn, leafNum),
          "iqhip_create_sharded");
    inputs_dirty = model_dirty = aln_dirty = true;
    pushInputs();
    int nvec = (lh_mem_save == LM_PER_NODE) ? (leafNum - 2) : (3 * leafNum - 6);
    check(iqhip_reserve(engine, nvec), "iqhip_reserve");
}

void PhyloTree::attachComm(int nranks, int rank, const void *unique_id) {
    if (!engine) throw std::runtime_error("attachEngine first");
    check(iqhip_comm_init_rank(engine, nranks, rank, unique_id), "iqhip_comm_init_rank");
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

// =========================================================================================
// The adapter (include/iqhip_adapter.h) instantiated for this mirror.  The policy answers the adapter's questions
// about the tree types and wraps the engine calls with what only the mirror has: dry-run mode (CPU tests record
// plans without a device), the legacy caller-owned collective (allreduce_hook) and the call counters.
// =========================================================================================
}  // namespace iqhost

#include "../../include/iqhip_adapter.h"

namespace iqhost {

struct MirrorPolicy : iqhip_adapter::EngineCalls<MirrorPolicy, PhyloTree> {
    typedef iqhip_adapter::EngineCalls<MirrorPolicy, PhyloTree> Base;
    typedef iqhip_adapter::Plan<MirrorPolicy> Plan;
    typedef PhyloTree Tree;
    typedef PhyloNode Node;
    typedef PhyloNeighbor Neighbor;
    static Node *node(Neighbor *nb) { return nb->node; }
    static double length(Neighbor *nb) { return nb->length; }
    static void setLength(Neighbor *nb, double len) { nb->length = len; }
    static bool isLeaf(Node *n) { return n->isLeaf(); }
    static int degree(Node *n) { return n->degree(); }
    static int leafId(Node *n) { return n->id; }
    static int numNeighbors(Node *n) { return (int)n->neighbors.size(); }
    static Neighbor *neighborAt(Node *n, int k) { return n->neighbors[k]; }
    static Neighbor *findNeighbor(Node *at, Node *to) { return at->findNeighbor(to); }
    static int &computed(Neighbor *nb) { return nb->partial_lh_computed; }
    static double &scaleFactor(Neighbor *nb) { return nb->lh_scale_factor; }
    static uint64_t key(Neighbor *nb) { return nb->partial_lh; }
    static void stealBuffer(Neighbor *to, Neighbor *from) { to->partial_lh = from->partial_lh; from->partial_lh = 0; }
    static bool perNodeMode(Tree *t) { return t->lh_mem_save == LM_PER_NODE; }
    static bool heavyFirst(Tree *t) { return t->heavy_first; }
    static void ensureBuffers(Tree *t) { if (!t->central_partial_lh) t->initializeAllPartialLh(); }
    static void sync(Tree *t) { t->pushInputs(); }
    static iqhip_engine *engine(Tree *t) { return t->engine; }
    static void fail(Tree *, const char *what, const char *detail) {
        throw std::runtime_error(std::string(what) + ": " + detail);
    }
    static void countComputation(Tree *t) { t->num_partial_lh_computations++; }
    static bool &thetaComputed(Tree *t) { return t->theta_computed; }
    static Neighbor *currentIt(Tree *t) { return t->current_it; }
    static Neighbor *currentItBack(Tree *t) { return t->current_it_back; }
    static void clearReversePartialLh(Node *n, Node *dad) { n->clearReversePartialLh(dad); }
    static void setCurrent(Tree *t, Neighbor *it, Neighbor *back) { t->current_it = it; t->current_it_back = back; }
    static void optimizeSweep(Tree *t, const iqhip_sweep_step *steps, int nsteps, int max_steps, double diverge_frac,
                              double *sum_scale, iqhip_branch_result *results) {
        needEngine(t);
        Base::optimizeSweep(t, steps, nsteps, max_steps, diverge_frac, sum_scale, results);
    }
    static double minBranchLength(Tree *t) { return t->min_branch_length; }
    static double maxBranchLength(Tree *t) { return t->max_branch_length; }

    static void record(Tree *t, const Plan &plan) {
        t->last_plan.clear();
        for (size_t k = 0; k < plan.ops.size(); k++) {
            PlanOp p;
            p.dst = plan.dst[k];
            const bool binary = plan.dst[k] && plan.nkids(k) == 2;
            p.left = binary ? plan.kid(k, 0) : nullptr;
            p.right = binary ? plan.kid(k, 1) : nullptr;
            p.op = plan.ops[k];
            t->last_plan.push_back(p);
        }
    }
    static void needEngine(Tree *t) {
        if (!t->engine) throw std::runtime_error("HIP likelihood kernel selected but no engine attached");
    }
    static void updatePartials(Tree *t, Plan &plan, double *sum_scale) {
        record(t, plan);
        if (t->dry_run) return;
        needEngine(t);
        Base::updatePartials(t, plan, sum_scale);
        t->num_submissions++;
    }
    static double traverseLnl(Tree *t, Plan &plan, iqhip_branch_end a, iqhip_branch_end b, double len, double *sum_scale) {
        record(t, plan);
        const int nops = (int)plan.ops.size();
        if (t->dry_run) {
            if (!t->allreduce_hook) return 0.0;
            // CPU rehearsal of the caller-owned collective (tests, gloo): the hook receives a HOST vector laid out
            // like the device result {lnl, -, sum_scale[k]...}, fills in this rank's share and all-reduces it; no
            // likelihood arithmetic happens in this library.
            std::vector<double> res(2 + plan.ops.size(), 0.0);
            t->allreduce_hook(res.data(), (int)res.size(), t->allreduce_ctx);
            for (int k = 0; k < nops; k++) sum_scale[k] = res[2 + k];
            return res[0];
        }
        needEngine(t);
        double lnl;
        if (t->allreduce_hook) {  // caller-owned collective (the engine's own: iqhip_comm_init_rank / iqhip_create_sharded)
            chk(t, iqhip_traverse_lnl_async(t->engine, plan.empty() ? nullptr : plan.ops.data(), nops, a, b, len),
                "iqhip_traverse_lnl_async");
            const int nres = 2 + nops;
            t->allreduce_hook(iqhip_result_device_ptr(t->engine), nres, t->allreduce_ctx);
            std::vector<double> res(nres);
            chk(t, iqhip_result_read(t->engine, res.data(), nres), "iqhip_result_read");
            lnl = res[0];
            for (int k = 0; k < nops; k++) sum_scale[k] = res[2 + k];
        } else {
            lnl = Base::traverseLnl(t, plan, a, b, len, sum_scale);
        }
        t->num_submissions++;
        return lnl;
    }
    static void computeTheta(Tree *t, iqhip_branch_end a, iqhip_branch_end b) {
        if (t->dry_run) return;
        needEngine(t);
        Base::computeTheta(t, a, b);
    }
    static void derv(Tree *t, double len, double &df, double &ddf) {
        t->num_derv_calls++;
        if (t->dry_run) return;
        needEngine(t);
        if (t->allreduce_hook) {
            chk(t, iqhip_derv_async(t->engine, len), "iqhip_derv_async");
            t->allreduce_hook(iqhip_result_device_ptr(t->engine), 2, t->allreduce_ctx);
            double res[2];
            chk(t, iqhip_result_read(t->engine, res, 2), "iqhip_result_read");
            df = res[0];
            ddf = res[1];
            if (isnan(df) || isinf(df)) df = ddf = 0.0;  // phylokernel.h:647-651
        } else {
            Base::derv(t, len, df, ddf);
        }
    }
    static double lnlFromTheta(Tree *t, double len) {
        if (t->dry_run) return 0.0;
        needEngine(t);
        return Base::lnlFromTheta(t, len);
    }
    static double optimizeBranch(Tree *t, Plan &plan, iqhip_branch_end a, iqhip_branch_end b, double xguess, int max_steps,
                                 double *sum_scale, int *nsteps) {
        record(t, plan);
        needEngine(t);
        const double optx = Base::optimizeBranch(t, plan, a, b, xguess, max_steps, sum_scale, nsteps);
        t->num_submissions++;
        t->num_derv_calls += *nsteps;
        return optx;
    }
};

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
// NNI evaluation, phylotree.cpp:2873-3066 (upper-bound shortcut left out; the ptnlh output goes to the engine's store)
// =========================================================================================
static void updateNeighborNode(PhyloNode *at, PhyloNode *oldn, PhyloNode *newn) {
    for (PhyloNeighbor *nb : at->neighbors)
        if (nb->node == oldn) { nb->node = newn; return; }
    throw std::runtime_error("updateNeighbor: not adjacent");
}

PhyloTree::NNIMove PhyloTree::getBestNNIForBran(PhyloNode *node1, PhyloNode *node2, bool nni5, NNIMove moves[2],
                                                const int *ptnlh_rows) {
    if (node1->isLeaf() || node2->isLeaf() || node1->degree() != 3 || node2->degree() != 3)
        throw std::runtime_error("getBestNNIForBran needs an internal branch of a binary tree");
    if (!central_partial_lh) initializeAllPartialLh();
    const int IT_NUM = nni5 ? 6 : 2;
    if (!nni_keys[0])
        for (int i = 0; i < 6; i++) nni_keys[i] = next_key++;
    // the neighbour slots that get a scratch copy (:2901-2924)
    std::vector<PhyloNeighbor **> slot;
    auto slot_of = [](PhyloNode *at, PhyloNode *to) -> PhyloNeighbor ** {
        for (auto &nb : at->neighbors)
            if (nb->node == to) return &nb;
        throw std::runtime_error("not adjacent");
    };
    slot.push_back(slot_of(node1, node2));
    slot.push_back(slot_of(node2, node1));
    if (nni5) {
        for (PhyloNeighbor *nb : node1->neighbors) if (nb->node != node2) slot.push_back(slot_of(nb->node, node1));
        for (PhyloNeighbor *nb : node2->neighbors) if (nb->node != node1) slot.push_back(slot_of(nb->node, node2));
    }
    std::vector<PhyloNeighbor *> saved(IT_NUM);
    for (int id = 0; id < IT_NUM; id++) {
        saved[id] = *slot[id];
        PhyloNeighbor *tmp = new PhyloNeighbor();
        tmp->node = saved[id]->node;
        tmp->length = saved[id]->length;
        tmp->id = saved[id]->id;
        tmp->partial_lh = nni_keys[id];
        *slot[id] = tmp;
    }
    PhyloNeighbor *node12_it = node1->findNeighbor(node2), *node21_it = node2->findNeighbor(node1);

    // the two moves: first non-node2 neighbour of node1 against each non-node1 neighbour of node2 (:2951-2960)
    size_t i1 = 0;
    while (node1->neighbors[i1]->node == node2) i1++;
    std::vector<size_t> i2s;
    for (size_t j = 0; j < node2->neighbors.size(); j++)
        if (node2->neighbors[j]->node != node1) i2s.push_back(j);
    const double backupScore = curScore;
    for (int cnt = 0; cnt < 2; cnt++) {
        const size_t i2 = i2s[cnt];
        PhyloNeighbor *node1_nei = node1->neighbors[i1], *node2_nei = node2->neighbors[i2];
        moves[cnt] = NNIMove();
        moves[cnt].node1 = node1->id;
        moves[cnt].node2 = node2->id;
        moves[cnt].node1_nei = node1_nei->node->id;
        moves[cnt].node2_nei = node2_nei->node->id;
        // do the NNI swap (:2976-2980)
        node1->neighbors[i1] = node2_nei;
        updateNeighborNode(node2_nei->node, node2, node1);
        node2->neighbors[i2] = node1_nei;
        updateNeighborNode(node1_nei->node, node1, node2);
        node12_it->clearPartialLh();
        node21_it->clearPartialLh();
        int i = 1;
        if (nni5) {
            for (PhyloNeighbor *nb : std::vector<PhyloNeighbor *>(node1->neighbors))
                if (nb->node != node2) {
                    nb->node->findNeighbor(node1)->clearPartialLh();
                    optimizeOneBranch(node1, nb->node, false, NNI_MAX_NR_STEP);
                    moves[cnt].newLen[i++] = node1->findNeighbor(nb->node)->length;
                }
            node21_it->clearPartialLh();
        }
        optimizeOneBranch(node1, node2, false, NNI_MAX_NR_STEP);
        moves[cnt].newLen[0] = node1->findNeighbor(node2)->length;
        if (nni5) {
            for (PhyloNeighbor *nb : std::vector<PhyloNeighbor *>(node2->neighbors))
                if (nb->node != node1) {
                    nb->node->findNeighbor(node2)->clearPartialLh();
                    optimizeOneBranch(node2, nb->node, false, NNI_MAX_NR_STEP);
                    moves[cnt].newLen[i++] = node2->findNeighbor(nb->node)->length;
                }
            node12_it->clearPartialLh();
        }
        moves[cnt].newloglh = computeLikelihoodFromBuffer();
        if (ptnlh_rows && ptnlh_rows[cnt] >= 0) {  // computePatternLikelihood(nniMoves[cnt].ptnlh), phylotree.cpp:3019-3020
            if (!engine || dry_run) throw std::runtime_error("getBestNNIForBran: store rows need an attached engine");
            check(iqhip_ptnlh_put_current(engine, ptnlh_rows[cnt], branchEnd(current_it), branchEnd(current_it_back)),
                  "iqhip_ptnlh_put_current");
            moves[cnt].ptnlh_row = ptnlh_rows[cnt];
        }
        // swap back (:3027-3030)
        node1->neighbors[i1] = node1_nei;
        updateNeighborNode(node1_nei->node, node2, node1);
        node2->neighbors[i2] = node2_nei;
        updateNeighborNode(node2_nei->node, node1, node2);
    }
    // restore the Neighbor objects (:3036-3044)
    for (int id = IT_NUM - 1; id >= 0; id--) {
        if (*slot[id] == current_it) current_it = saved[id];
        if (*slot[id] == current_it_back) current_it_back = saved[id];
        delete *slot[id];
        *slot[id] = saved[id];
    }
    // restore the length of the 4 branches around node1, node2 (:3048-3051)
    for (PhyloNeighbor *nb : node1->neighbors) if (nb->node != node2) nb->length = nb->node->findNeighbor(node1)->length;
    for (PhyloNeighbor *nb : node2->neighbors) if (nb->node != node1) nb->length = nb->node->findNeighbor(node2)->length;
    theta_computed = false;
    curScore = backupScore;
    return moves[0].newloglh > moves[1].newloglh ? moves[0] : moves[1];
}

void PhyloTree::computeAllPartialLh() {
    if (lh_mem_save != LM_ALL_BRANCH) throw std::runtime_error("computeAllPartialLh needs LM_ALL_BRANCH");
    if (!central_partial_lh) initializeAllPartialLh();
    // one plan for every pending directed vector (each has its own buffer in this mode), one submission
    MirrorPolicy::Plan plan;
    for (PhyloNode *node : nodes)
        for (PhyloNeighbor *nb : node->neighbors)
            if (!nb->node->isLeaf() && (nb->partial_lh_computed & 1) == 0)
                iqhip_adapter::collectPlan<MirrorPolicy>(this, nb, node, plan);
    MirrorPolicy::record(this, plan);
    if (plan.empty()) return;
    if (!dry_run && allreduce_hook) throw std::runtime_error("computeAllPartialLh: not available with a caller-owned collective");
    std::vector<double> sum_scale(plan.size(), 0.0);
    pushInputs();
    MirrorPolicy::updatePartials(this, plan, sum_scale.data());
    iqhip_adapter::applyScaleFactors<MirrorPolicy>(plan, sum_scale.data());
}

void PhyloTree::computePartialLhAround(const std::vector<PhyloNode *> &n1, const std::vector<PhyloNode *> &n2) {
    if (lh_mem_save != LM_ALL_BRANCH) throw std::runtime_error("computePartialLhAround needs LM_ALL_BRANCH");
    if (!central_partial_lh) initializeAllPartialLh();
    MirrorPolicy::Plan plan;   // as computeAllPartialLh, for the vectors of the listed branches only
    for (size_t q = 0; q < n1.size(); q++)
        for (int side = 0; side < 2; side++) {
            PhyloNode *node = side ? n2[q] : n1[q], *other = side ? n1[q] : n2[q];
            for (PhyloNeighbor *nb : node->neighbors)
                if (nb->node != other && !nb->node->isLeaf() && (nb->partial_lh_computed & 1) == 0)
                    iqhip_adapter::collectPlan<MirrorPolicy>(this, nb, node, plan);
        }
    MirrorPolicy::record(this, plan);
    if (plan.empty()) return;
    if (!dry_run && allreduce_hook) throw std::runtime_error("computePartialLhAround: not available with a caller-owned collective");
    std::vector<double> sum_scale(plan.size(), 0.0);
    pushInputs();
    MirrorPolicy::updatePartials(this, plan, sum_scale.data());
    iqhip_adapter::applyScaleFactors<MirrorPolicy>(plan, sum_scale.data());
}

// the branches of a batched NNI evaluation: all internal ones, or the caller's list with each branch normalised to
// node1->id < node2->id (the orientation internalBranches gives, so that a listed branch has the full call's entries)
static void nniBranches(const PhyloTree *t, const PhyloTree::BranchList *branches, const char *who, std::vector<PhyloNode *> &n1,
                        std::vector<PhyloNode *> &n2) {
    if (!branches) t->internalBranches(n1, n2);
    else {
        n1.clear();
        n2.clear();
        for (const auto &br : *branches) {
            const int a = std::min(br.first, br.second), b = std::max(br.first, br.second);
            if (a < 0 || b >= (int)t->nodes.size() || a == b || !t->nodes[(size_t)a]->findNeighbor(t->nodes[(size_t)b]) ||
                t->nodes[(size_t)a]->isLeaf() || t->nodes[(size_t)b]->isLeaf())
                throw std::runtime_error(std::string(who) + ": a listed branch is not an internal branch of the tree");
            n1.push_back(t->nodes[(size_t)a]);
            n2.push_back(t->nodes[(size_t)b]);
        }
    }
    for (size_t q = 0; q < n1.size(); q++)
        if (n1[q]->degree() != 3 || n2[q]->degree() != 3) throw std::runtime_error(std::string(who) + " needs a binary tree");
}

void PhyloTree::evaluateNNIsBatch(std::vector<NNIMove> &moves, const BranchList *branches) {
    if (!engine || dry_run) throw std::runtime_error("evaluateNNIsBatch needs an attached engine");
    if (allreduce_hook) throw std::runtime_error("evaluateNNIsBatch: runs with a caller-owned collective use getBestNNIForBran");
    std::vector<PhyloNode *> bn1, bn2;
    nniBranches(this, branches, "evaluateNNIsBatch", bn1, bn2);
    if (branches && bn1.empty()) { moves.clear(); return; }
    if (branches) computePartialLhAround(bn1, bn2);
    else computeAllPartialLh();
    pushInputs();
    struct Cand {
        PhyloNode *node1, *node2;
        PhyloNeighbor *n1a, *n1b, *n2x, *n2o;  // n1a <-> n2x are swapped
        iqhip_node_op ops[2];
    };
    std::vector<Cand> cands;
    for (size_t bq = 0; bq < bn1.size(); bq++) {
        PhyloNode *node1 = bn1[bq], *node2 = bn2[bq];
        std::vector<PhyloNeighbor *> s1, s2;
        for (PhyloNeighbor *nb : node1->neighbors) if (nb->node != node2) s1.push_back(nb);
        for (PhyloNeighbor *nb : node2->neighbors) if (nb->node != node1) s2.push_back(nb);
        for (int cnt = 0; cnt < 2; cnt++) {  // phylotree.cpp:2951-2960: first neighbour of node1 against each of node2's
            Cand c;
            c.node1 = node1; c.node2 = node2;
            c.n1a = s1[0]; c.n1b = s1[1]; c.n2x = s2[cnt]; c.n2o = s2[1 - cnt];
            cands.push_back(c);
        }
    }
    while (nni_batch_keys.size() < 2 * cands.size()) nni_batch_keys.push_back(next_key++);
    auto child = [&](PhyloNeighbor *nb, uint64_t &key, int32_t &leaf, double &len) {
        if (nb->node->isLeaf()) { key = 0; leaf = nb->node->id; }
        else { key = nb->partial_lh; leaf = -1; }
        len = nb->length;
    };
    std::vector<iqhip_branch_task> tasks(cands.size());
    for (size_t t = 0; t < cands.size(); t++) {
        Cand &c = cands[t];
        // after the swap node2's subtree (seen from node1) joins n1a and n2o, node1's joins n2x and n1b
        memset(c.ops, 0, sizeof c.ops);
        c.ops[0].dst_key = nni_batch_keys[2 * t];
        child(c.n1a, c.ops[0].left_key, c.ops[0].left_leaf, c.ops[0].left_len);
        child(c.n2o, c.ops[0].right_key, c.ops[0].right_leaf, c.ops[0].right_len);
        c.ops[1].dst_key = nni_batch_keys[2 * t + 1];
        child(c.n2x, c.ops[1].left_key, c.ops[1].left_leaf, c.ops[1].left_len);
        child(c.n1b, c.ops[1].right_key, c.ops[1].right_leaf, c.ops[1].right_len);
        iqhip_branch_task &k = tasks[t];
        k.ops = c.ops;
        k.nops = 2;
        k.max_steps = NNI_MAX_NR_STEP;
        k.a = iqhip_branch_end{nni_batch_keys[2 * t], -1, 0};
        k.b = iqhip_branch_end{nni_batch_keys[2 * t + 1], -1, 0};
        k.xguess = c.node1->findNeighbor(c.node2)->length;
        k.x1 = min_branch_length;
        k.x2 = max_branch_length;
        k.xacc = min_branch_length;
    }
    // the tasks hold pointers into cands: do not touch cands from here on.
    // Two rounds: the reference evaluates the second swap of a branch starting from the length the first swap's
    // optimisation left on that branch (the Neighbor copies are restored only after both, phylotree.cpp:3036-3051),
    // so the first swaps of all branches run side by side, then the second swaps with those lengths as guesses.
    std::vector<double> sum_scale(2 * cands.size(), 0.0);
    std::vector<iqhip_branch_result> res(cands.size());
    for (int round = 0; round < 2; round++) {
        std::vector<iqhip_branch_task> sub;
        for (size_t t = round; t < tasks.size(); t += 2) {
            if (round == 1) tasks[t].xguess = res[t - 1].optx;
            sub.push_back(tasks[t]);
        }
        std::vector<double> ss(2 * sub.size(), 0.0);
        std::vector<iqhip_branch_result> rr(sub.size());
        check(iqhip_optimize_branch_batch(engine, sub.data(), (int)sub.size(), ss.data(), rr.data()),
              "iqhip_optimize_branch_batch");
        num_submissions++;
        for (size_t q = 0; q < sub.size(); q++) {
            const size_t t = 2 * q + round;
            res[t] = rr[q];
            sum_scale[2 * t] = ss[2 * q];
            sum_scale[2 * t + 1] = ss[2 * q + 1];
        }
    }
    moves.assign(cands.size(), NNIMove());
    for (size_t t = 0; t < cands.size(); t++) {
        const Cand &c = cands[t];
        NNIMove &m = moves[t];
        m.node1 = c.node1->id;
        m.node2 = c.node2->id;
        m.node1_nei = c.n1a->node->id;
        m.node2_nei = c.n2x->node->id;
        m.newLen[0] = res[t].optx;
        num_derv_calls += res[t].nsteps;
        if (res[t].status == 2) throw std::runtime_error("Wrong computeFuncDerv (non-finite derivative)");
        const double sf = c.n1a->lh_scale_factor + c.n2o->lh_scale_factor + sum_scale[2 * t] +
                          c.n2x->lh_scale_factor + c.n1b->lh_scale_factor + sum_scale[2 * t + 1];
        m.newloglh = res[t].lnl + sf;
        const bool first_diverged = (t & 1) && res[t - 1].optx > max_branch_length * 0.95;
        if (res[t].optx > max_branch_length * 0.95 || first_diverged) {
            // diverged Newton (phylotree.cpp:2167-2176: optimizeOneBranch compares lnL at the optimum with lnL at the old
            // length and may restore the latter): rare; the one-branch path for this candidate -- and for the second swap
            // of a branch whose first swap diverged, because its starting length is whatever that comparison left
            NNIMove two[2];
            getBestNNIForBran(c.node1, c.node2, false, two);
            m = two[t & 1];
        }
    }
}

void PhyloTree::internalBranches(std::vector<PhyloNode *> &n1, std::vector<PhyloNode *> &n2) const {
    n1.clear();
    n2.clear();
    for (PhyloNode *node1 : nodes)
        for (PhyloNeighbor *nb12 : node1->neighbors) {
            PhyloNode *node2 = nb12->node;
            if (node1->isLeaf() || node2->isLeaf() || node1->id > node2->id) continue;
            n1.push_back(node1);
            n2.push_back(node2);
        }
}

void PhyloTree::evaluateNNIs5Batch(std::vector<NNIMove> &moves, const int *ptnlh_rows, const BranchList *branches_in) {
    if (!engine || dry_run) throw std::runtime_error("evaluateNNIs5Batch needs an attached engine");
    if (allreduce_hook) throw std::runtime_error("evaluateNNIs5Batch: runs with a caller-owned collective use getBestNNIForBran");
    std::vector<PhyloNode *> bn1, bn2;
    nniBranches(this, branches_in, "evaluateNNIs5Batch", bn1, bn2);
    if (branches_in && bn1.empty()) { moves.clear(); return; }
    if (branches_in) computePartialLhAround(bn1, bn2);
    else computeAllPartialLh();
    pushInputs();
    // an outward subtree vector around the branch: fixed while the candidate is evaluated
    struct Ext { uint64_t key; int32_t leaf; double sf; };
    auto ext_of = [](PhyloNeighbor *nb) {
        Ext x;
        if (nb->node->isLeaf()) { x.key = 0; x.leaf = nb->node->id; x.sf = 0.0; }
        else { x.key = nb->partial_lh; x.leaf = -1; x.sf = nb->lh_scale_factor; }
        return x;
    };
    struct Branch {  // one internal branch: the five Neighbor lengths carry over from the first swap to the second
        PhyloNode *node1, *node2;
        PhyloNeighbor *n1[2], *n2[2];
        double len1[2], len2[2], l0;
    };
    std::vector<Branch> branches;
    for (size_t bq = 0; bq < bn1.size(); bq++) {
        PhyloNode *node1 = bn1[bq], *node2 = bn2[bq];
        Branch b;
        b.node1 = node1; b.node2 = node2;
        int i = 0, j = 0;
        for (PhyloNeighbor *nb : node1->neighbors) if (nb->node != node2) { b.n1[i] = nb; b.len1[i++] = nb->length; }
        for (PhyloNeighbor *nb : node2->neighbors) if (nb->node != node1) { b.n2[j] = nb; b.len2[j++] = nb->length; }
        b.l0 = node1->findNeighbor(node2)->length;
        branches.push_back(b);
    }
    const size_t nb = branches.size();
    while (nni_batch_keys.size() < 4 * nb) nni_batch_keys.push_back(next_key++);
    moves.assign(2 * nb, NNIMove());
    struct Work {
        Ext X[2], Y[2];           // subtrees at node1 (X1 = moved in, X2) and at node2 in optimisation order
        double lX[2], lY[2], l0;
        double *outX[2], *outY[2];  // where the optimised lengths go back to (the Branch's Neighbor slots)
        uint64_t s0, s1, s2, s3;
        double sf0, sf1, sf2, sf3;
        iqhip_node_op ops[2];
        bool diverged;
    };
    auto mkop = [](uint64_t dst, const Ext *a, uint64_t akey, double alen, const Ext *b, uint64_t bkey, double blen) {
        iqhip_node_op o;
        memset(&o, 0, sizeof o);
        o.dst_key = dst;
        o.left_key = a ? a->key : akey;  o.left_leaf = a ? a->leaf : -1;  o.left_len = alen;
        o.right_key = b ? b->key : bkey; o.right_leaf = b ? b->leaf : -1; o.right_len = blen;
        return o;
    };
    for (int cnt = 0; cnt < 2; cnt++) {
        std::vector<Work> work(nb);
        for (size_t q = 0; q < nb; q++) {
            Branch &b = branches[q];
            Work &w = work[q];
            // swap n1[0] <-> n2[cnt]: node1 now holds {n2[cnt], n1[1]}, node2 holds n1[0] at n2[cnt]'s index
            w.X[0] = ext_of(b.n2[cnt]); w.lX[0] = b.len2[cnt];     w.outX[0] = &b.len2[cnt];
            w.X[1] = ext_of(b.n1[1]);   w.lX[1] = b.len1[1];       w.outX[1] = &b.len1[1];
            const int moved_pos = cnt, other = 1 - cnt;  // neighbour-index order at node2 (phylotree.cpp:3008-3016)
            Ext R = ext_of(b.n1[0]), S = ext_of(b.n2[other]);
            if (moved_pos < other) { w.Y[0] = R; w.lY[0] = b.len1[0]; w.outY[0] = &b.len1[0]; w.Y[1] = S; w.lY[1] = b.len2[other]; w.outY[1] = &b.len2[other]; }
            else { w.Y[0] = S; w.lY[0] = b.len2[other]; w.outY[0] = &b.len2[other]; w.Y[1] = R; w.lY[1] = b.len1[0]; w.outY[1] = &b.len1[0]; }
            w.l0 = b.l0;
            w.s0 = nni_batch_keys[4 * q]; w.s1 = nni_batch_keys[4 * q + 1];
            w.s2 = nni_batch_keys[4 * q + 2]; w.s3 = nni_batch_keys[4 * q + 3];
            w.diverged = false;
            NNIMove &m = moves[2 * q + cnt];
            m.node1 = b.node1->id; m.node2 = b.node2->id;
            m.node1_nei = b.n1[0]->node->id; m.node2_nei = b.n2[cnt]->node->id;
        }
        for (int round = 0; round < 5; round++) {
            std::vector<iqhip_branch_task> tasks(nb);
            for (size_t q = 0; q < nb; q++) {
                Work &w = work[q];
                iqhip_branch_task &k = tasks[q];
                memset(&k, 0, sizeof k);
                k.ops = w.ops;
                k.max_steps = NNI_MAX_NR_STEP;
                k.x1 = min_branch_length; k.x2 = max_branch_length; k.xacc = min_branch_length;
                const Ext &Ya = w.Y[0], &Yb = w.Y[1];
                switch (round) {
                    case 0:  // branch node1 - X1: u12 = f(Y...), w = f(u12, X2)
                        w.ops[0] = mkop(w.s0, &Ya, 0, w.lY[0], &Yb, 0, w.lY[1]);
                        w.ops[1] = mkop(w.s1, nullptr, w.s0, w.l0, &w.X[1], 0, w.lX[1]);
                        k.nops = 2; k.a = iqhip_branch_end{w.X[0].key, w.X[0].leaf, 0}; k.b = iqhip_branch_end{w.s1, -1, 0};
                        k.xguess = w.lX[0];
                        break;
                    case 1:  // branch node1 - X2
                        w.ops[0] = mkop(w.s1, nullptr, w.s0, w.l0, &w.X[0], 0, w.lX[0]);
                        k.nops = 1; k.a = iqhip_branch_end{w.X[1].key, w.X[1].leaf, 0}; k.b = iqhip_branch_end{w.s1, -1, 0};
                        k.xguess = w.lX[1];
                        break;
                    case 2:  // central branch
                        w.ops[0] = mkop(w.s2, &w.X[0], 0, w.lX[0], &w.X[1], 0, w.lX[1]);
                        k.nops = 1; k.a = iqhip_branch_end{w.s0, -1, 0}; k.b = iqhip_branch_end{w.s2, -1, 0};
                        k.xguess = w.l0;
                        break;
                    case 3:  // branch node2 - Y1
                        w.ops[0] = mkop(w.s3, nullptr, w.s2, w.l0, &Yb, 0, w.lY[1]);
                        k.nops = 1; k.a = iqhip_branch_end{Ya.key, Ya.leaf, 0}; k.b = iqhip_branch_end{w.s3, -1, 0};
                        k.xguess = w.lY[0];
                        break;
                    default:  // branch node2 - Y2
                        w.ops[0] = mkop(w.s3, nullptr, w.s2, w.l0, &Ya, 0, w.lY[0]);
                        k.nops = 1; k.a = iqhip_branch_end{Yb.key, Yb.leaf, 0}; k.b = iqhip_branch_end{w.s3, -1, 0};
                        k.xguess = w.lY[1];
                        break;
                }
            }
            std::vector<double> ss(2 * nb + 2, 0.0);
            std::vector<iqhip_branch_result> rr(nb);
            if (round == 4 && ptnlh_rows) {  // the lnL of the last round is the candidate's: keep its per-pattern values
                std::vector<int32_t> rows(nb);
                for (size_t q = 0; q < nb; q++) rows[q] = ptnlh_rows[2 * q + cnt];
                check(iqhip_optimize_branch_batch_rows(engine, tasks.data(), (int)nb, ss.data(), rr.data(), rows.data()),
                      "iqhip_optimize_branch_batch_rows");
                for (size_t q = 0; q < nb; q++) moves[2 * q + cnt].ptnlh_row = rows[q];
            } else
                check(iqhip_optimize_branch_batch(engine, tasks.data(), (int)nb, ss.data(), rr.data()),
                      "iqhip_optimize_branch_batch");
            num_submissions++;
            size_t sp = 0;
            for (size_t q = 0; q < nb; q++) {
                Work &w = work[q];
                const iqhip_branch_result &r = rr[q];
                if (r.status == 2) throw std::runtime_error("Wrong computeFuncDerv (non-finite derivative)");
                if (r.optx > max_branch_length * 0.95) w.diverged = true;
                num_derv_calls += r.nsteps;
                NNIMove &m = moves[2 * q + cnt];
                switch (round) {
                    case 0:
                        w.sf0 = w.Y[0].sf + w.Y[1].sf + ss[sp];
                        w.sf1 = w.sf0 + w.X[1].sf + ss[sp + 1];
                        sp += 2;
                        w.lX[0] = r.optx; m.newLen[1] = r.optx;
                        break;
                    case 1:
                        w.sf1 = w.sf0 + w.X[0].sf + ss[sp++];
                        w.lX[1] = r.optx; m.newLen[2] = r.optx;
                        break;
                    case 2:
                        w.sf2 = w.X[0].sf + w.X[1].sf + ss[sp++];
                        w.l0 = r.optx; m.newLen[0] = r.optx;
                        break;
                    case 3:
                        w.sf3 = w.sf2 + w.Y[1].sf + ss[sp++];
                        w.lY[0] = r.optx; m.newLen[3] = r.optx;
                        break;
                    default:
                        w.sf3 = w.sf2 + w.Y[0].sf + ss[sp++];
                        w.lY[1] = r.optx; m.newLen[4] = r.optx;
                        m.newloglh = r.lnl + w.Y[1].sf + w.sf3;
                        break;
                }
            }
        }
        // the lengths the swap left on the five Neighbor objects are the second swap's starting point
        for (size_t q = 0; q < nb; q++) {
            Work &w = work[q];
            *w.outX[0] = w.lX[0]; *w.outX[1] = w.lX[1];
            *w.outY[0] = w.lY[0]; *w.outY[1] = w.lY[1];
            branches[q].l0 = w.l0;
            if (w.diverged) {  // diverged Newton (phylotree.cpp:2167-2176): rare; take the branch-by-branch path
                NNIMove two[2];
                getBestNNIForBran(branches[q].node1, branches[q].node2, true, two, ptnlh_rows ? ptnlh_rows + 2 * q : nullptr);
                moves[2 * q] = two[0];
                moves[2 * q + 1] = two[1];
            }
        }
    }
}

// =========================================================================================
// tree edits of the NNI search, phylotree.cpp:2726-2871
// =========================================================================================
namespace {
// the slot of `at`'s neighbour list that holds one of the two subtrees of the move
PhyloNeighbor **swapSlot(PhyloNode *at, PhyloNode *other_end, int id_a, int id_b) {
    for (PhyloNeighbor *&nb : at->neighbors)
        if (nb->node != other_end && (nb->node->id == id_a || nb->node->id == id_b)) return &nb;
    throw std::runtime_error("doNNI: the move does not belong to this tree");
}
// PhyloNeighbor::reorientPartialLh (phylonode.cpp:22-39): `nb` points to a node whose one buffer may sit on another Neighbor
void reorientPartialLh(PhyloNeighbor *nb, PhyloNode *dad) {
    if (nb->partial_lh) return;
    for (PhyloNeighbor *kid : nb->node->neighbors) {
        if (kid->node == dad) continue;
        PhyloNeighbor *backnei = kid->node->findNeighbor(nb->node);
        if (backnei->partial_lh) {
            nb->partial_lh = backnei->partial_lh;
            backnei->partial_lh = 0;
            backnei->partial_lh_computed &= ~1;
            return;
        }
    }
    throw std::runtime_error("doNNI: partial_lh is not re-oriented");
}
}  // namespace

void PhyloTree::doNNI(const NNIMove &move, bool clearLH) {
    if (move.node1 < 0 || move.node2 < 0 || move.node1 >= (int)nodes.size() || move.node2 >= (int)nodes.size())
        throw std::runtime_error("doNNI: bad node id");
    PhyloNode *node1 = nodes[(size_t)move.node1], *node2 = nodes[(size_t)move.node2];
    PhyloNeighbor *node12_it = node1->findNeighbor(node2), *node21_it = node2->findNeighbor(node1);
    if (!node12_it || !node21_it || node1->degree() != 3 || node2->degree() != 3)
        throw std::runtime_error("doNNI needs an internal branch of a binary tree");
    PhyloNeighbor **slot1 = swapSlot(node1, node2, move.node1_nei, move.node2_nei);
    PhyloNeighbor **slot2 = swapSlot(node2, node1, move.node1_nei, move.node2_nei);
    if ((*slot1)->node == (*slot2)->node) throw std::runtime_error("doNNI: the move does not belong to this tree");
    if (lh_mem_save == LM_PER_NODE && central_partial_lh) {  // reorient partial_lh before swap (:2799-2803)
        reorientPartialLh(node12_it, node1);
        reorientPartialLh(node21_it, node2);
    }
    PhyloNeighbor *node1_nei = *slot1, *node2_nei = *slot2;
    *slot1 = node2_nei;
    updateNeighborNode(node2_nei->node, node2, node1);
    *slot2 = node1_nei;
    updateNeighborNode(node1_nei->node, node1, node2);
    if (clearLH) {
        node12_it->clearPartialLh();
        node21_it->clearPartialLh();
        node2->clearReversePartialLh(node1);
        node1->clearReversePartialLh(node2);
    }
    theta_computed = false;
}

void PhyloTree::changeNNIBrans(const NNIMove &move, bool nni5) {
    if (move.node1 < 0 || move.node2 < 0 || move.node1 >= (int)nodes.size() || move.node2 >= (int)nodes.size())
        throw std::runtime_error("changeNNIBrans: bad node id");
    PhyloNode *node1 = nodes[(size_t)move.node1], *node2 = nodes[(size_t)move.node2];
    PhyloNeighbor *n12 = node1->findNeighbor(node2), *n21 = node2->findNeighbor(node1);
    if (!n12 || !n21) throw std::runtime_error("changeNNIBrans: the move does not belong to this tree");
    n12->length = n21->length = move.newLen[0];
    if (!nni5) return;
    int i = 1;
    for (PhyloNeighbor *nb : node1->neighbors)
        if (nb->node != node2) nb->length = nb->node->findNeighbor(node1)->length = move.newLen[i++];
    for (PhyloNeighbor *nb : node2->neighbors)
        if (nb->node != node1) nb->length = nb->node->findNeighbor(node2)->length = move.newLen[i++];
}

void PhyloTree::saveBranchLengths(std::vector<double> &lenvec) const {
    lenvec.clear();
    for (const PhyloNeighbor *nb : all_neighbors) lenvec.push_back(nb->length);
}

void PhyloTree::restoreBranchLengths(const std::vector<double> &lenvec) {
    if (lenvec.size() != all_neighbors.size()) throw std::runtime_error("restoreBranchLengths: the lengths are not this tree's");
    for (size_t k = 0; k < all_neighbors.size(); k++) all_neighbors[k]->length = lenvec[k];
}

PhyloTree::NNIMove PhyloTree::doOneRandomNNI(PhyloNode *node1, PhyloNode *node2, int bit1, int bit2) {
    if (node1->isLeaf() || node2->isLeaf() || node1->degree() != 3 || node2->degree() != 3 || !node1->findNeighbor(node2))
        throw std::runtime_error("doOneRandomNNI needs an internal branch of a binary tree");
    auto pick = [](PhyloNode *at, PhyloNode *other, int bit) {   // :2732-2758: a draw of 0 takes the first, else the next
        std::vector<PhyloNeighbor *> s;
        for (PhyloNeighbor *nb : at->neighbors)
            if (nb->node != other) s.push_back(nb);
        return s[bit ? 1 : 0];
    };
    NNIMove mv;
    mv.node1 = node1->id;
    mv.node2 = node2->id;
    mv.node1_nei = pick(node1, node2, bit1)->node->id;
    mv.node2_nei = pick(node2, node1, bit2)->node->id;
    doNNI(mv, false);
    return mv;
}

std::vector<std::vector<int>> PhyloTree::adjacency() const {
    std::vector<std::vector<int>> adj(nodes.size());
    for (const PhyloNode *nd : nodes)
        for (const PhyloNeighbor *nb : nd->neighbors) adj[(size_t)nd->id].push_back(nb->node->id);
    return adj;
}

// =========================================================================================
// SH-aLRT / local bootstrap, phylotree.cpp:3984-4103
// =========================================================================================
double PhyloTree::testAllBranches(int reps, int lbp_reps, std::vector<BranchSupport> &out, bool batched) {
    if (!engine || dry_run) throw std::runtime_error("testAllBranches needs an attached engine");
    if (allreduce_hook) throw std::runtime_error("testAllBranches: not available with a caller-owned collective");
    if (reps < 0 || lbp_reps < 0 || std::max(reps, lbp_reps) < 1) throw std::runtime_error("testAllBranches: no replicates");
    if (std::max(reps, lbp_reps) > num_boot_samples) throw std::runtime_error("testAllBranches: more replicates than setBootSamples uploaded");
    if (batched && lh_mem_save != LM_ALL_BRANCH) throw std::runtime_error("testAllBranches(batched) needs LM_ALL_BRANCH");
    std::vector<PhyloNode *> n1, n2;
    internalBranches(n1, n2);
    const size_t nb = n1.size();
    if (nb == 0) throw std::runtime_error("testAllBranches: the tree has no internal branch");
    const double lh0 = computeLikelihood();
    check(iqhip_ptnlh_reserve(engine, (int)(1 + 2 * nb)), "iqhip_ptnlh_reserve");
    check(iqhip_ptnlh_put_current(engine, 0, branchEnd(current_it), branchEnd(current_it_back)), "iqhip_ptnlh_put_current");
    std::vector<int> rows(2 * nb);
    for (size_t k = 0; k < 2 * nb; k++) rows[k] = (int)(1 + k);
    std::vector<NNIMove> moves;
    if (batched) {
        evaluateNNIs5Batch(moves, rows.data());
    } else {
        moves.resize(2 * nb);
        for (size_t q = 0; q < nb; q++) {
            NNIMove two[2];
            getBestNNIForBran(n1[q], n2[q], true, two, &rows[2 * q]);
            moves[2 * q] = two[0];
            moves[2 * q + 1] = two[1];
        }
    }
    std::vector<int32_t> rows3(3 * nb);
    std::vector<double> lh3(3 * nb);
    for (size_t q = 0; q < nb; q++) {
        rows3[3 * q] = 0;
        lh3[3 * q] = lh0;
        for (int cnt = 0; cnt < 2; cnt++) {
            const NNIMove &m = moves[2 * q + cnt];
            if (m.node1 != n1[q]->id || m.node2 != n2[q]->id || m.ptnlh_row != rows[2 * q + cnt])
                throw std::runtime_error("testAllBranches: NNI moves out of order");
            rows3[3 * q + 1 + cnt] = m.ptnlh_row;
            lh3[3 * q + 1 + cnt] = m.newloglh;
        }
    }
    std::vector<iqhip_branch_support> res(nb);
    check(iqhip_branch_tests(engine, rows3.data(), lh3.data(), (int)nb, reps, lbp_reps, res.data()), "iqhip_branch_tests");
    out.assign(nb, BranchSupport());
    for (size_t q = 0; q < nb; q++) {
        BranchSupport &b = out[q];
        b.node1 = n1[q]->id;
        b.node2 = n2[q]->id;
        for (int k = 0; k < 3; k++) b.lh[k] = lh3[3 * q + k];
        b.sh_alrt = res[q].sh_alrt;
        b.lbp = res[q].lbp;
        b.abayes = res[q].abayes;
        b.alrt_stat = res[q].alrt_stat;
    }
    return lh0;
}

// =========================================================================================
// tree topology tests, phylotesting.cpp:2053-2442
// =========================================================================================
void PhyloTree::evaluateTrees(const std::vector<std::string> &newicks, bool fixed_lengths, int nsamples, bool weighted,
                              const std::vector<double> &au_scales, uint64_t seed, std::vector<TreeTest> &out,
                              std::vector<double> &au_bp, double epsilon) {
    if (!engine || dry_run) throw std::runtime_error("evaluateTrees needs an attached engine");
    if (allreduce_hook) throw std::runtime_error("evaluateTrees: not available with a caller-owned collective");
    if (newicks.size() < 2) throw std::runtime_error("evaluateTrees: at least two trees");
    if (nsamples < 1) throw std::runtime_error("evaluateTrees: no replicates");
    const int ntrees = (int)newicks.size();
    std::vector<std::string> names((size_t)leafNum);
    for (int i = 0; i < leafNum; i++) names[i] = nodes[i]->name.empty() ? std::to_string(i) : nodes[i]->name;
    const int leaves = leafNum;
    check(iqhip_ptnlh_reserve(engine, ntrees), "iqhip_ptnlh_reserve");
    out.assign((size_t)ntrees, TreeTest());
    std::vector<int32_t> rows((size_t)ntrees);
    std::vector<double> lh((size_t)ntrees);
    for (int tid = 0; tid < ntrees; tid++) {
        readTreeString(newicks[tid], names);
        if (leafNum != leaves) throw std::runtime_error("evaluateTrees: a tree with another number of taxa");
        initializeAllPartialLh();
        clearAllPartialLH();
        double lnl = computeLikelihood();
        if (!fixed_lengths) {
            optimizeAllBranches();
            clearAllPartialLH();
            lnl = computeLikelihood();
        }
        check(iqhip_ptnlh_put_current(engine, tid, branchEnd(current_it), branchEnd(current_it_back)), "iqhip_ptnlh_put_current");
        rows[tid] = tid;
        lh[tid] = out[tid].logl = lnl;
    }
    double nsite = 0.0;
    for (double f : ptn_freq) nsite += f;
    genBootSamples(nsamples, (int64_t)nsite, seed, 0xA0u);
    std::vector<iqhip_tree_test> res((size_t)ntrees);
    check(iqhip_tree_tests(engine, rows.data(), lh.data(), ntrees, nsamples, epsilon, weighted ? 1 : 0, seed, res.data()),
          "iqhip_tree_tests");
    for (int tid = 0; tid < ntrees; tid++) out[tid].t = res[tid];
    au_bp.clear();
    if (!au_scales.empty()) {
        au_bp.assign(au_scales.size() * (size_t)ntrees, 0.0);
        check(iqhip_multiscale_bp(engine, rows.data(), ntrees, au_scales.data(), (int)au_scales.size(), nsamples, seed,
                                  au_bp.data()),
              "iqhip_multiscale_bp");
    }
}

// =========================================================================================
// pairwise ML distances, phylotree.cpp:2432-2541
// =========================================================================================
void PhyloTree::computeDist(const double *init, double *dist, double *d2l) {
    if (!engine || dry_run) throw std::runtime_error("computeDist needs an attached engine");
    if (allreduce_hook) throw std::runtime_error("computeDist: not available with a caller-owned collective");
    pushInputs();
    check(iqhip_pair_distances(engine, init, min_branch_length, MAX_GENETIC_DIST, min_branch_length, 100, dist, d2l, nullptr),
          "iqhip_pair_distances");
}

void PhyloTree::pairCounts(const int32_t *pairs, int npairs, double *counts) {
    if (!engine || dry_run) throw std::runtime_error("pairCounts needs an attached engine");
    pushInputs();
    check(iqhip_pair_counts(engine, pairs, npairs, counts), "iqhip_pair_counts");
}

// =========================================================================================
// likelihood mapping, quartet.cpp:676-1152, 1340-1505 (include/iqhip.h "Likelihood mapping"; lmap_host.h)
// =========================================================================================
void PhyloTree::quartetCells(const int32_t *quartets, int nq, double *cells, int32_t *nother) {
    if (!engine || dry_run) throw std::runtime_error("quartetCells needs an attached engine");
    pushInputs();
    check(iqhip_quartet_cells(engine, quartets, nq, cells, nother), "iqhip_quartet_cells");
}

void PhyloTree::computeQuartetLikelihoods(const int32_t *quartets, int nq, iqhip_quartet_result *results, int iterations,
                                          double tolerance, const double *const_invar) {
    if (!engine || dry_run) throw std::runtime_error("computeQuartetLikelihoods needs an attached engine");
    if (allreduce_hook) throw std::runtime_error("computeQuartetLikelihoods: not available with a caller-owned collective");
    pushInputs();
    check(iqhip_quartet_likelihoods(engine, quartets, nq, const_invar, min_branch_length, max_branch_length, min_branch_length,
                                    100, 0.95, iterations, tolerance, results),
          "iqhip_quartet_likelihoods");
}

void PhyloTree::doLikelihoodMapping(int64_t nquartets, uint64_t seed, LmapResult &out, const double *const_invar) {
    if (leafNum < 4) throw std::runtime_error("likelihood mapping needs at least 4 taxa");
    if (nquartets < 0) throw std::runtime_error("doLikelihoodMapping: negative number of quartets");
    std::vector<int32_t> quartets;
    if (nquartets == 0 || nquartets >= lmap::numQuartets(leafNum)) lmap::allQuartets(leafNum, quartets);
    else lmap::drawQuartets(leafNum, nquartets, seed, quartets);
    const size_t nq = quartets.size() / 4;
    if (nq > 2147483647u) throw std::runtime_error("doLikelihoodMapping: too many quartets for one call");
    std::vector<iqhip_quartet_result> res(nq);
    computeQuartetLikelihoods(quartets.data(), (int)nq, res.data(), 10, 0.1, const_invar);
    out = LmapResult();
    out.info.resize(nq);
    out.seq_count.assign((size_t)(leafNum + 1) * 10, 0);
    for (size_t q = 0; q < nq; q++) {
        lmap::QuartetInfo &qi = out.info[q];
        for (int k = 0; k < 4; k++) qi.seqID[k] = quartets[4 * q + k];
        for (int k = 0; k < 3; k++) qi.logl[k] = res[q].logl[k];
        lmap::region(qi.logl, qi.qweight, &qi.corner, &qi.area);
        out.areacount[qi.area]++;
        out.cornercount[qi.corner]++;
        for (int col : {qi.area, 7 + qi.corner}) {
            out.seq_count[(size_t)leafNum * 10 + col]++;
            for (int k = 0; k < 4; k++) out.seq_count[(size_t)qi.seqID[k] * 10 + col]++;
        }
    }
}

// =========================================================================================
// BIONJ, phylotree.cpp:2619-2635 over bionj.h (include/iqhip.h "BIONJ")
// =========================================================================================
std::string PhyloTree::bionjNewick(const iqhip_bionj_step *steps, int n, const int32_t *last, const double *last_len,
                                   const std::vector<std::string> &names) {
    if (n < 3 || (int)names.size() != n) throw std::runtime_error("bionjNewick: one name per taxon, at least 3 taxa");
    if (!last || !last_len || (n > 3 && !steps)) throw std::runtime_error("bionjNewick: null argument");
    auto fmt = [](double len) {
        char buf[400];
        snprintf(buf, sizeof buf, "%10.8f", len);
        return std::string(buf);
    };
    std::vector<std::string> sub(names);
    std::vector<char> gone((size_t)n, 0);
    for (int k = 0; k < n - 3; k++) {
        const int a = steps[k].a, b = steps[k].b;
        if (a < 0 || a >= n || b < 0 || b >= n || a == b || gone[(size_t)a] || gone[(size_t)b])
            throw std::runtime_error("bionjNewick: step " + std::to_string(k) + " merges a row that is not active");
        sub[(size_t)a] = "(" + sub[(size_t)a] + ":" + fmt(steps[k].la) + "," + sub[(size_t)b] + ":" + fmt(steps[k].lb) + ")";
        sub[(size_t)b].clear();
        gone[(size_t)b] = 1;
    }
    std::string out = "(";
    for (int k = 0; k < 3; k++) {
        const int l = last[k];
        if (l < 0 || l >= n || gone[(size_t)l] || (k > 0 && l <= last[k - 1]))
            throw std::runtime_error("bionjNewick: the last three rows must be active and ascending");
        out += sub[(size_t)l] + ":" + fmt(last_len[k]) + (k < 2 ? "," : ");");
    }
    return out;
}

void PhyloTree::computeBioNJ(const double *dist, const double *var, std::string *newick, iqhip_bionj_step *steps_out,
                             int32_t *last_out, double *last_len_out) {
    if (!engine || dry_run) throw std::runtime_error("computeBioNJ needs an attached engine");
    const int n = leafNum;
    if (n < 3) throw std::runtime_error("computeBioNJ needs at least 3 taxa");
    std::vector<std::string> names((size_t)n);
    for (int k = 0; k < n; k++) {
        if (k >= (int)nodes.size() || !nodes[(size_t)k]) throw std::runtime_error("computeBioNJ: the taxa are not known yet");
        names[(size_t)k] = nodes[(size_t)k]->name.empty() ? std::to_string(k) : nodes[(size_t)k]->name;
    }
    std::vector<iqhip_bionj_step> steps((size_t)std::max(1, n - 3));
    int32_t last[3];
    double last_len[3];
    check(iqhip_bionj(engine, n, dist, var, steps.data(), last, last_len), "iqhip_bionj");
    const std::string nwk = bionjNewick(steps.data(), n, last, last_len, names);
    const bool non_empty_tree = root != nullptr;
    readTreeString(nwk, names);   // (a tree read with taxon ids as labels has the ids as its names)
    if (non_empty_tree) initializeAllPartialLh();
    if (newick) *newick = nwk;
    if (steps_out) std::copy(steps.begin(), steps.begin() + (n - 3), steps_out);
    if (last_out) std::copy(last, last + 3, last_out);
    if (last_len_out) std::copy(last_len, last_len + 3, last_len_out);
}

// =========================================================================================
// Fitch parsimony (phylotreepars.cpp; include/iqhip.h "Fitch parsimony")
// =========================================================================================
void PhyloTree::needParsimony(const char *what) {
    if (!engine || dry_run) throw std::runtime_error(std::string(what) + " needs an attached engine");
    if (!pars_initialized) initializeAllPartialPars();
}

int64_t PhyloTree::parsInformativeSites() {
    // parsimony-informative patterns: Alignment::isInformative, the rule of computeConst, asked of this tree's data type
    Alignment rule;
    rule.seq_type = seq_type;
    rule.num_states = num_states;
    rule.STATE_UNKNOWN = STATE_UNKNOWN;
    pars_informative.assign((size_t)nptn, 0);
    int64_t total = 0;
    for (int64_t p = 0; p < nptn; p++) {
        pars_informative[(size_t)p] = rule.isInformative(aln_states.data() + p, leafNum, (size_t)nptn);
        if (pars_informative[(size_t)p]) total += (int64_t)ptn_freq[(size_t)p];
    }
    return total;
}

void PhyloTree::initializeAllPartialPars() {
    if (!engine || dry_run) throw std::runtime_error("initializeAllPartialPars needs an attached engine");
    if (!root) throw std::runtime_error("no tree");
    pushInputs();
    parsInformativeSites();
    check(iqhip_pars_init(engine, pars_informative.data(), 4 * (leafNum - 1), &pars_nsites), "iqhip_pars_init");
    assignParsSlots();
    pars_initialized = true;
}

void PhyloTree::assignParsSlots() {   // one slot per directed vector that is not a tip's; every parsimony flag goes down
    pars_next_slot = pars_slot_base < 0 ? leafNum : pars_slot_base;
    for (PhyloNeighbor *nb : all_neighbors) {
        nb->pars_slot = nb->node->isLeaf() ? nb->node->id : pars_next_slot++;
        nb->partial_lh_computed &= ~2;
    }
}

void PhyloTree::collectParsOps(PhyloNeighbor *dad_branch, PhyloNode *dad, std::vector<iqhip_pars_op> &ops) {
    PhyloNode *node = dad_branch->node;
    if (node->isLeaf() || (dad_branch->partial_lh_computed & 2)) return;
    PhyloNeighbor *kid[2] = {nullptr, nullptr};
    int nkid = 0;
    for (PhyloNeighbor *nb : node->neighbors)
        if (nb->node != dad) {
            if (nkid == 2) throw std::runtime_error("parsimony needs a strictly bifurcating tree");
            kid[nkid++] = nb;
        }
    if (nkid != 2) throw std::runtime_error("parsimony needs a strictly bifurcating tree");
    collectParsOps(kid[0], node, ops);
    collectParsOps(kid[1], node, ops);
    ops.push_back(iqhip_pars_op{dad_branch->pars_slot, kid[0]->pars_slot, kid[1]->pars_slot, 0});
    dad_branch->partial_lh_computed |= 2;
}

void PhyloTree::submitParsOps(std::vector<iqhip_pars_op> &ops) {
    if (ops.empty()) return;
    check(iqhip_pars_update(engine, ops.data(), (int)ops.size()), "iqhip_pars_update");
    ops.clear();
}

void PhyloTree::computePartialParsimony(PhyloNeighbor *dad_branch, PhyloNode *dad) {
    (this->*computePartialParsimonyPointer)(dad_branch, dad);
}
int PhyloTree::computeParsimonyBranch(PhyloNeighbor *dad_branch, PhyloNode *dad, int *branch_subst) {
    return (this->*computeParsimonyBranchPointer)(dad_branch, dad, branch_subst);
}

void PhyloTree::computePartialParsimonyHIP(PhyloNeighbor *dad_branch, PhyloNode *dad) {
    needParsimony("computePartialParsimony");
    std::vector<iqhip_pars_op> ops;
    collectParsOps(dad_branch, dad, ops);
    submitParsOps(ops);
}

int PhyloTree::computeParsimonyBranchHIP(PhyloNeighbor *dad_branch, PhyloNode *dad, int *branch_subst) {
    needParsimony("computeParsimonyBranch");
    PhyloNeighbor *node_branch = dad_branch->node->findNeighbor(dad);
    std::vector<iqhip_pars_op> ops;
    collectParsOps(dad_branch, dad, ops);
    collectParsOps(node_branch, dad_branch->node, ops);
    submitParsOps(ops);
    const int32_t ends[2] = {dad_branch->pars_slot, node_branch->pars_slot};
    int32_t score = 0, subst = 0;
    check(iqhip_pars_branch_scores(engine, ends, 1, &score, &subst), "iqhip_pars_branch_scores");
    if (branch_subst) *branch_subst = subst;
    return score;
}

int PhyloTree::computeParsimony() {
    if (!root) throw std::runtime_error("no tree");
    return computeParsimonyBranch(root->neighbors[0], root);
}

void PhyloTree::computeAllPartialPars() {
    needParsimony("computeAllPartialPars");
    std::vector<iqhip_pars_op> ops;
    collectAllParsOps(ops);
    submitParsOps(ops);
}

void PhyloTree::collectAllParsOps(std::vector<iqhip_pars_op> &ops) {
    std::vector<PhyloNode *> n1, n2;
    getBranches(n1, n2);
    for (size_t k = 0; k < n1.size(); k++) {
        collectParsOps(n1[k]->findNeighbor(n2[k]), n1[k], ops);
        collectParsOps(n2[k]->findNeighbor(n1[k]), n2[k], ops);
    }
}

void PhyloTree::getBranches(std::vector<PhyloNode *> &n1, std::vector<PhyloNode *> &n2, PhyloNode *node, PhyloNode *dad) const {
    if (!node) node = root;
    for (PhyloNeighbor *nb : node->neighbors)
        if (nb->node != dad) {
            const bool lower = node->id < nb->node->id;
            n1.push_back(lower ? node : nb->node);
            n2.push_back(lower ? nb->node : node);
            getBranches(n1, n2, nb->node, node);
        }
}

void PhyloTree::fixBranchList(std::vector<PhyloNeighbor *> &all, std::vector<PhyloNode *> &from) const {
    // the branches in the reference's recursion order: (node, neighbour) from the root downwards
    struct Rec {
        std::vector<PhyloNeighbor *> &all;
        std::vector<PhyloNode *> &from;
        void go(PhyloNode *node, PhyloNode *dad) {
            for (PhyloNeighbor *nb : node->neighbors)
                if (nb->node != dad) {
                    all.push_back(nb);
                    from.push_back(node);
                    go(nb->node, node);
                }
        }
    } rec{all, from};
    rec.go(root, nullptr);
}

int PhyloTree::fixNegativeBranch(bool force) {
    if (!root) throw std::runtime_error("no tree");
    std::vector<PhyloNeighbor *> all;
    std::vector<PhyloNode *> from;
    fixBranchList(all, from);
    std::vector<int32_t> ends;
    size_t ntodo = 0;
    for (size_t k = 0; k < all.size(); k++)
        if (all[k]->length < 0.0 || force) ntodo++;
    std::vector<int32_t> subst(ntodo);
    if (ntodo) {
        computeAllPartialPars();
        for (size_t k = 0; k < all.size(); k++)
            if (all[k]->length < 0.0 || force) {
                ends.push_back(all[k]->pars_slot);
                ends.push_back(all[k]->node->findNeighbor(from[k])->pars_slot);
            }
        check(iqhip_pars_branch_scores(engine, ends.data(), (int)ntodo, nullptr, subst.data()), "iqhip_pars_branch_scores");
    }
    double nsite = 0.0;   // getAlnNSite()
    for (double f : ptn_freq) nsite += f;
    return applyParsLengths(all, from, subst.data(), force, nsite);
}

int PhyloTree::applyParsLengths(const std::vector<PhyloNeighbor *> &all, const std::vector<PhyloNode *> &from, const int32_t *subst,
                                bool force, double nsite) {
    int fixed = 0;
    size_t q = 0;
    for (size_t k = 0; k < all.size(); k++) {
        PhyloNeighbor *nb = all[k], *back = nb->node->findNeighbor(from[k]);
        if (nb->length < 0.0 || force) {
            const int branch_subst = subst[q++];
            double branch_length = (branch_subst > 0) ? ((double)branch_subst / nsite) : (1.0 / nsite);
            const double z = (double)num_states / (num_states - 1);
            const double x = 1.0 - (z * branch_length);
            if (x > 0) branch_length = -log(x) / z;
            if (branch_length < min_branch_length) branch_length = min_branch_length;
            nb->length = back->length = branch_length;
            fixed++;
        }
        if (nb->length <= 0.0) nb->length = back->length = min_branch_length;
    }
    if (fixed) {   // new lengths: every likelihood vector is stale (the parsimony flags stay)
        for (PhyloNeighbor *nb : all_neighbors) nb->partial_lh_computed &= ~1;
        current_it = current_it_back = nullptr;
        theta_computed = false;
    }
    return fixed;
}

void PhyloTree::startParsimonyTree(const int *taxon_order, const std::vector<std::string> &names) {
    const int size = leafNum;
    {
        std::vector<char> seen((size_t)size, 0);
        for (int k = 0; k < size; k++) {
            if (taxon_order[k] < 0 || taxon_order[k] >= size || seen[(size_t)taxon_order[k]])
                throw std::runtime_error("computeParsimonyTree: the addition order is not a permutation of the taxa");
            seen[(size_t)taxon_order[k]] = 1;
        }
    }
    deleteAllPartialLh();
    freeTree();
    nodes.assign((size_t)(2 * size - 2), nullptr);
    pars_names = names;
    // the initial tree of 3 taxa around node `size`
    PhyloNode *centre = newParsNode(size);
    for (int k = 0; k < 3; k++) {
        PhyloNode *leaf = newParsNode(taxon_order[k]);
        newParsNeighbor(centre, leaf);
        newParsNeighbor(leaf, centre);
    }
    root = nodes[(size_t)taxon_order[0]];
}

PhyloNode *PhyloTree::newParsNode(int id) {
    PhyloNode *nd = new PhyloNode();
    nd->id = id;
    if (id < leafNum && id < (int)pars_names.size()) nd->name = pars_names[(size_t)id];
    nodes[(size_t)id] = nd;
    return nd;
}

PhyloNeighbor *PhyloTree::newParsNeighbor(PhyloNode *from, PhyloNode *to) {
    PhyloNeighbor *nb = new PhyloNeighbor();
    nb->node = to;
    nb->length = -1.0;
    from->neighbors.push_back(nb);
    all_neighbors.push_back(nb);
    return nb;
}

void PhyloTree::collectInsertScan(std::vector<PhyloNode *> &nodes1, std::vector<PhyloNode *> &nodes2, std::vector<iqhip_pars_op> &ops,
                                  std::vector<int32_t> &ends) {
    nodes1.clear();
    nodes2.clear();
    getBranches(nodes1, nodes2);
    for (size_t k = 0; k < nodes1.size(); k++) {
        PhyloNeighbor *a = nodes2[k]->findNeighbor(nodes1[k]), *c = nodes1[k]->findNeighbor(nodes2[k]);
        collectParsOps(a, nodes2[k], ops);
        collectParsOps(c, nodes1[k], ops);
        ends.push_back(a->pars_slot);
        ends.push_back(c->pars_slot);
    }
}

void PhyloTree::insertParsimonyTaxon(PhyloNode *target_node, PhyloNode *target_dad, int taxon, int cur) {
    // insert added_node in the middle of target_node -- target_dad (:382-405); its neighbours: the new taxon, then
    // target_node, then target_dad
    PhyloNode *new_taxon = newParsNode(taxon), *added_node = newParsNode(leafNum + cur - 2);
    PhyloNeighbor *to_taxon = newParsNeighbor(added_node, new_taxon);
    PhyloNeighbor *from_taxon = newParsNeighbor(new_taxon, added_node);
    PhyloNeighbor *dad_side = target_dad->findNeighbor(target_node), *node_side = target_node->findNeighbor(target_dad);
    PhyloNeighbor *to_node = newParsNeighbor(added_node, target_node), *to_dad = newParsNeighbor(added_node, target_dad);
    // added_node -> target_node inherits what target_dad saw of target_node, and the other way round
    to_node->pars_slot = dad_side->pars_slot;
    to_node->partial_lh_computed = dad_side->partial_lh_computed;
    to_dad->pars_slot = node_side->pars_slot;
    to_dad->partial_lh_computed = node_side->partial_lh_computed;
    dad_side->node = added_node;    // updateNeighbor: in place, the position in the neighbour list is kept
    node_side->node = added_node;
    to_taxon->pars_slot = new_taxon->id;
    // (the reference copies the scan's fitch(a, c) into this vector; here its flag stays down and the next
    // submission computes it with everything else)
    from_taxon->pars_slot = pars_next_slot++;
    dad_side->clearPartialLh();
    dad_side->pars_slot = pars_next_slot++;
    node_side->clearPartialLh();
    node_side->pars_slot = pars_next_slot++;
    target_dad->clearReversePartialLh(added_node);
    target_node->clearReversePartialLh(added_node);
}

void PhyloTree::finishParsimonyTree() {
    nodeNum = 2 * leafNum - 2;
    branchNum = 2 * leafNum - 3;
    {   // branch ids in traversal order from the root
        int next_id = 0;
        std::vector<PhyloNode *> n1, n2;
        getBranches(n1, n2);
        for (size_t k = 0; k < n1.size(); k++) {
            n1[k]->findNeighbor(n2[k])->id = n2[k]->findNeighbor(n1[k])->id = next_id++;
        }
    }
    current_it = current_it_back = nullptr;
    theta_computed = false;
}

int PhyloTree::computeParsimonyTree(const int *taxon_order, std::vector<ParsStep> *trace) {
    if (!engine || dry_run) throw std::runtime_error("computeParsimonyTree needs an attached engine");
    const int size = leafNum;
    if (size < 3) throw std::runtime_error("computeParsimonyTree needs at least 3 taxa");
    std::vector<std::string> names((size_t)size);
    for (int k = 0; k < size && k < (int)nodes.size(); k++)
        if (nodes[(size_t)k]) names[(size_t)k] = nodes[(size_t)k]->name;
    startParsimonyTree(taxon_order, names);
    pars_initialized = false;
    initializeAllPartialPars();   // (the three vectors that point at the centre take slots; leaves are their own)
    if (trace) trace->clear();
    int best_pars_score = 0;
    std::vector<iqhip_pars_op> ops;
    for (int cur = 3; cur < size; cur++) {
        std::vector<PhyloNode *> nodes1, nodes2;
        // every vector the scan reads, in one submission
        std::vector<int32_t> ends;
        collectInsertScan(nodes1, nodes2, ops, ends);
        submitParsOps(ops);
        ParsStep step;
        int32_t best = 0, best_score = 0;
        if (trace) step.score.resize(nodes1.size());
        check(iqhip_pars_insert_scores(engine, ends.data(), (int)nodes1.size(), taxon_order[cur], trace ? step.score.data() : nullptr,
                                       &best, &best_score),
              "iqhip_pars_insert_scores");
        best_pars_score = best_score;
        if (trace) {
            for (size_t k = 0; k < nodes1.size(); k++) {
                step.node1.push_back(nodes1[k]->id);
                step.node2.push_back(nodes2[k]->id);
            }
            step.chosen = best;
            step.best_score = best_score;
            trace->push_back(step);
        }
        insertParsimonyTaxon(nodes1[(size_t)best], nodes2[(size_t)best], taxon_order[cur], cur);
    }
    finishParsimonyTree();
    fixNegativeBranch(true);
    if (size == 3) best_pars_score = computeParsimony();
    return best_pars_score;
}

// ---- parsimony SPR search ------------------------------------------------------------------------------------------------
void PhyloTree::collectSprJobs(int radius, std::vector<iqhip_pars_spr_job> &jobs, std::vector<iqhip_pars_spr_step> &steps,
                               std::vector<SprMove> &moves) {
    if (!root) throw std::runtime_error("no tree");
    if (radius < 1 || radius > IQHIP_PARS_SPR_MAX_RADIUS) throw std::runtime_error("collectSprJobs: radius outside 1 .. 10");
    if (!pars_initialized) {
        if (engine && !dry_run) initializeAllPartialPars();
        else assignParsSlots();
    }
    jobs.clear();
    steps.clear();
    moves.clear();
    struct Walk {
        int radius, first;
        PhyloNode *p, *s;
        std::vector<iqhip_pars_spr_step> &steps;
        std::vector<SprMove> &moves;
        // the branches beyond node a (reached from dad); step `parent` holds everything on dad's side of dad -- a
        void go(PhyloNode *a, PhyloNode *dad, int parent, int depth) {
            if (a->isLeaf() || depth > radius) return;
            PhyloNeighbor *kid[2] = {nullptr, nullptr};
            int nkid = 0;
            for (PhyloNeighbor *nb : a->neighbors)
                if (nb->node != dad) {
                    if (nkid == 2) throw std::runtime_error("parsimony needs a strictly bifurcating tree");
                    kid[nkid++] = nb;
                }
            if (nkid != 2) throw std::runtime_error("parsimony needs a strictly bifurcating tree");
            for (int c = 0; c < 2; c++) {
                const int k = (int)steps.size() - first;
                steps.push_back(iqhip_pars_spr_step{parent, kid[1 - c]->pars_slot, kid[c]->pars_slot, 0});
                moves.push_back(SprMove{p->id, s->id, a->id, kid[c]->node->id, depth});
                go(kid[c]->node, a, k, depth + 1);
            }
        }
    };
    for (PhyloNode *p : nodes) {
        if (!p || p->isLeaf()) continue;
        if (p->degree() != 3) throw std::runtime_error("parsimony needs a strictly bifurcating tree");
        for (int i = 0; i < 3; i++) {
            PhyloNeighbor *to_s = p->neighbors[(size_t)i], *to_q1 = p->neighbors[(size_t)(i == 0 ? 1 : 0)],
                          *to_q2 = p->neighbors[(size_t)(i == 2 ? 1 : 2)];
            PhyloNode *q1 = to_q1->node, *q2 = to_q2->node;
            const int first = (int)steps.size();
            Walk w{radius, first, p, to_s->node, steps, moves};
            steps.push_back(iqhip_pars_spr_step{-1, to_q2->pars_slot, to_q1->pars_slot, 0});
            moves.push_back(SprMove{p->id, to_s->node->id, q1->id, q2->id, 0});
            // (q1 is reached over the merged branch: its far side is q2, and p itself is not q1's neighbour any more)
            w.go(q1, p, 0, 1);
            const int second = (int)steps.size() - first;
            steps.push_back(iqhip_pars_spr_step{-1, to_q1->pars_slot, to_q2->pars_slot, IQHIP_PARS_SPR_NO_SCORE});
            moves.push_back(SprMove{p->id, to_s->node->id, q2->id, q1->id, 0});
            w.go(q2, p, second, 1);
            const int n = (int)steps.size() - first;
            if (n == 2) {   // two leaves beyond p: nowhere to go
                steps.resize((size_t)first);
                moves.resize((size_t)first);
                continue;
            }
            jobs.push_back(iqhip_pars_spr_job{to_s->pars_slot, first, n, 0});
        }
    }
}

void PhyloTree::applySprMove(const SprMove &mv) {
    const int nn = (int)nodes.size();
    auto node_of = [&](int id) -> PhyloNode * {
        if (id < 0 || id >= nn || !nodes[(size_t)id]) throw std::runtime_error("applySprMove: no such node");
        return nodes[(size_t)id];
    };
    PhyloNode *p = node_of(mv.prune), *s = node_of(mv.subtree), *a = node_of(mv.node1), *b = node_of(mv.node2);
    if (p->degree() != 3 || !p->findNeighbor(s)) throw std::runtime_error("applySprMove: the subtree does not hang at the prune node");
    PhyloNeighbor *to_q[2] = {nullptr, nullptr};
    int nq = 0;
    for (PhyloNeighbor *nb : p->neighbors)
        if (nb->node != s) to_q[nq++] = nb;
    PhyloNode *q1 = to_q[0]->node, *q2 = to_q[1]->node;
    // the target: a branch of the tree as it stands that neither touches the prune node nor lies inside the pruned subtree
    // (every branch of the pruned tree but the merged one); everything is checked before anything changes
    PhyloNeighbor *a_b = a->findNeighbor(b), *b_a = b->findNeighbor(a);
    if (a == p || b == p || !a_b || !b_a) throw std::runtime_error("applySprMove: the target is not a branch of the pruned tree");
    {
        std::vector<std::pair<PhyloNode *, PhyloNode *>> todo{{s, p}};
        while (!todo.empty()) {
            PhyloNode *x = todo.back().first, *dad = todo.back().second;
            todo.pop_back();
            if (x == a || x == b) throw std::runtime_error("applySprMove: the target lies inside the pruned subtree");
            for (PhyloNeighbor *nb : x->neighbors)
                if (nb->node != dad) todo.push_back({nb->node, x});
        }
    }
    deleteAllPartialLh();   // (topology change: every likelihood vector and every parsimony flag)
    // merge q1 -- p -- q2 into q1 -- q2 (in place: the positions in the neighbour lists are kept)
    PhyloNeighbor *q1_p = q1->findNeighbor(p), *q2_p = q2->findNeighbor(p);
    const double merged = to_q[0]->length + to_q[1]->length;
    q1_p->node = q2;
    q2_p->node = q1;
    q1_p->length = q2_p->length = merged;
    // split a -- b with p
    const double half = a_b->length * 0.5;
    a_b->node = p;
    b_a->node = p;
    to_q[0]->node = a;
    to_q[1]->node = b;
    a_b->length = b_a->length = to_q[0]->length = to_q[1]->length = half;
    {   // branch ids in traversal order from the root
        int next_id = 0;
        std::vector<PhyloNode *> n1, n2;
        getBranches(n1, n2);
        for (size_t k = 0; k < n1.size(); k++) n1[k]->findNeighbor(n2[k])->id = n2[k]->findNeighbor(n1[k])->id = next_id++;
    }
    assignParsSlots();   // (a neighbour that pointed at a leaf may point at an internal node now, and the other way round)
    current_it = current_it_back = nullptr;
    theta_computed = false;
}

int PhyloTree::optimizeParsimonySPR(int radius, int max_rounds, std::vector<SprRound> *trace) {
    if (!engine || dry_run) throw std::runtime_error("optimizeParsimonySPR needs an attached engine");
    if (radius < 1 || radius > IQHIP_PARS_SPR_MAX_RADIUS) throw std::runtime_error("optimizeParsimonySPR: radius outside 1 .. 10");
    if (trace) trace->clear();
    std::vector<iqhip_pars_spr_job> jobs;
    std::vector<iqhip_pars_spr_step> steps;
    std::vector<SprMove> moves;
    std::vector<int32_t> score, best_step, best_score;
    int current = -1;
    for (int round = 0; max_rounds < 0 || round < max_rounds; round++) {
        computeAllPartialPars();
        collectSprJobs(radius, jobs, steps, moves);
        if (jobs.empty()) break;   // (4 taxa or fewer branches than a move needs)
        score.resize(steps.size());
        best_step.resize(jobs.size());
        best_score.resize(jobs.size());
        int32_t best_job = -1;
        check(iqhip_pars_spr_scan(engine, jobs.data(), (int)jobs.size(), steps.data(), (int)steps.size(), score.data(),
                                  best_step.data(), best_score.data(), &best_job),
              "iqhip_pars_spr_scan");
        SprRound r;
        r.score_before = score[(size_t)jobs[0].first_step];
        for (const iqhip_pars_spr_job &job : jobs)   // every scored root step is the tree as it stands
            if (score[(size_t)job.first_step] != r.score_before)
                throw std::runtime_error("optimizeParsimonySPR: the prune points disagree about the score of the current tree");
        for (int32_t v : score) r.steps_scored += v >= 0;
        if (best_job < 0) throw std::runtime_error("optimizeParsimonySPR: nothing was scored");
        r.job = best_job;
        r.step = best_step[(size_t)best_job];
        r.score = best_score[(size_t)best_job];
        r.move = moves[(size_t)jobs[(size_t)best_job].first_step + (size_t)r.step];
        r.applied = r.score < r.score_before;
        if (r.applied && r.move.depth < 1) throw std::runtime_error("optimizeParsimonySPR: a root step beats the current tree");
        current = r.applied ? r.score : r.score_before;
        if (r.applied) applySprMove(r.move);
        if (trace) trace->push_back(r);
        if (!r.applied) break;
    }
    return current >= 0 ? current : computeParsimony();
}

std::string PhyloTree::supportLabel(double sh_alrt, double lbp, bool with_sh, bool with_lbp) {
    std::ostringstream ss;  // phylotree.cpp:4078-4091 (node names are empty here)
    ss.precision(3);
    if (with_sh) ss << sh_alrt * 100;
    if (with_lbp) ss << "/" << lbp * 100;
    return ss.str();
}

static void writeSupportNewick(std::ostringstream &os, const PhyloNode *node, const PhyloNode *dad,
                               const std::vector<std::string> &label) {
    if (node->isLeaf() && dad) {
        if (node->name.empty()) os << node->id;
        else os << node->name;
        return;
    }
    os << "(";
    bool first = true;
    for (PhyloNeighbor *nb : node->neighbors)
        if (nb->node != dad) {
            if (!first) os << ",";
            first = false;
            writeSupportNewick(os, nb->node, node, label);
            os.precision(17);
            os << ":" << nb->length;
        }
    os << ")" << label[node->id];
}

std::string PhyloTree::supportTreeString(const std::vector<BranchSupport> &sup, bool with_sh, bool with_lbp) const {
    // testAllBranches walks from the root leaf and names `node` of every internal (node, dad): the far end of the branch,
    // which is also where a Newick string printed from the root's neighbour puts the label of that branch
    if (!root) return ";";
    std::vector<std::string> label(nodes.size());
    std::vector<std::pair<PhyloNode *, PhyloNode *>> stack;
    stack.push_back({root, nullptr});
    while (!stack.empty()) {
        PhyloNode *node = stack.back().first, *dad = stack.back().second;
        stack.pop_back();
        if (dad && !node->isLeaf() && !dad->isLeaf())
            for (const BranchSupport &b : sup)
                if ((b.node1 == node->id && b.node2 == dad->id) || (b.node2 == node->id && b.node1 == dad->id))
                    label[node->id] = supportLabel(b.sh_alrt, b.lbp, with_sh, with_lbp);
        for (PhyloNeighbor *nb : node->neighbors)
            if (nb->node != dad) stack.push_back({nb->node, node});
    }
    std::ostringstream os;
    writeSupportNewick(os, root->neighbors[0]->node, nullptr, label);
    os << ";";
    return os.str();
}

// =========================================================================================
// host views
// =========================================================================================
void PhyloTree::fetchScaleNum(PhyloNeighbor *nei, UBYTE *out) {
    if (!engine) throw std::runtime_error("no engine");
    if (!nei->partial_lh) throw std::runtime_error("neighbor has no buffer");
    check(iqhip_fetch_scale_num(engine, nei->partial_lh, out), "iqhip_fetch_scale_num");
}
void PhyloTree::fetchPartialLh(PhyloNeighbor *nei, double *out) {
    if (!engine) throw std::runtime_error("no engine");
    if (!nei->partial_lh) throw std::runtime_error("neighbor has no buffer");
    check(iqhip_fetch_partial(engine, nei->partial_lh, out), "iqhip_fetch_partial");
}
void PhyloTree::fetchPatternLh(double *out) {
    if (!engine) throw std::runtime_error("no engine");
    check(iqhip_fetch_pattern_lh(engine, out), "iqhip_fetch_pattern_lh");
}

void PhyloTree::computePatternLikelihood(double *ptn_lh) {
    if (!engine) throw std::runtime_error("no engine");
    if (!current_it) throw std::runtime_error("computePatternLikelihood before computeLikelihood");
    check(iqhip_fetch_pattern_lh_scaled(engine, branchEnd(current_it), branchEnd(current_it_back), ptn_lh),
          "iqhip_fetch_pattern_lh_scaled");
}

void PhyloTree::computePatternLhCat(double *ptn_lh_cat) {
    if (!engine) throw std::runtime_error("no engine");
    if (!current_it) throw std::runtime_error("computePatternLhCat before computeLikelihood");
    double df, ddf;
    theta_computed = false;
    computeLikelihoodDerv(current_it, current_it_back->node, df, ddf);  // (re)builds theta of current_it
    check(iqhip_pattern_lh_cat(engine, current_it->length, ptn_lh_cat), "iqhip_pattern_lh_cat");
}

// =========================================================================================
// EM for +R free-rate models, empirical-Bayes site rates (kernels_em.hip; model/ratefree.cpp:450-579)
// =========================================================================================
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
    if (!engine) throw std::runtime_error("no engine");
    if (!current_it) throw std::runtime_error("emPosteriors before computeLikelihood");
    double df, ddf;
    theta_computed = false;
    computeLikelihoodDerv(current_it, current_it_back->node, df, ddf);  // (re)builds theta of current_it
    check(iqhip_em_posteriors(engine, current_it->length, cat_sum), "iqhip_em_posteriors");
}

void PhyloTree::emObjective(PhyloNeighbor *dad_branch, PhyloNode *dad, double *f, int64_t *floored) {
    if (!engine) throw std::runtime_error("no engine");
    PhyloNeighbor *back = dad_branch->node->findNeighbor(dad);
    if (!back) throw std::runtime_error("emObjective: not a branch");
    current_it = dad_branch;
    current_it_back = back;
    double df, ddf;
    theta_computed = false;
    computeLikelihoodDerv(dad_branch, dad, df, ddf);
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
    if (!engine) throw std::runtime_error("no engine");
    if (nmixture > 1) throw std::runtime_error("optimizeFreeRatesEM: mixture models are not supported (ModelMixture::optimizeWithEM)");
    if (n_unobserved > 0) throw std::runtime_error("optimizeFreeRatesEM: +ASC is not supported (the reference switches EM off for it)");
    for (double v : ptn_invar)
        if (v != 0.0) throw std::runtime_error("optimizeFreeRatesEM: +I+R (p_invar > 0) is not supported");
    const double MIN_PROP = 1e-4;
    const int nmix = ncat;
    double nsite = 0.0;   // getAlnNSite
    for (double f : ptn_freq) nsite += f;
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

// =========================================================================================
// EM for mixture class weights (kernels_mixem.hip; model/modelmixture.cpp:1355-1416)
// =========================================================================================
double PhyloTree::getAlnNSite() const {
    double nsite = 0.0;
    for (double f : ptn_freq) nsite += f;
    return nsite;
}

void PhyloTree::computePatternLhCat(SiteLoglType wsl, double *out) {
    if (!engine) throw std::runtime_error("no engine");
    if (wsl != WSL_MIXTURE) throw std::runtime_error("computePatternLhCat: only WSL_MIXTURE takes this form");
    if (!current_it) throw std::runtime_error("computePatternLhCat before computeLikelihood");
    double df, ddf;
    theta_computed = false;
    computeLikelihoodDerv(current_it, current_it_back->node, df, ddf);  // (re)builds theta of current_it
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
    if (!engine) throw std::runtime_error("no engine");
    // a model or weights set since the last submission reach the engine first: it refuses the matrix of another model
    // (mix.model_version), which it cannot do for a model it has not been sent yet
    pushInputs();
    check(iqhip_mix_weights_em(engine, max_steps, getAlnNSite(), weights, p_invar, nsteps, converged, trace), "iqhip_mix_weights_em");
}

double PhyloTree::optimizeMixtureWeights(double *p_invar, int *nsteps, int *converged) {
    if (!engine) throw std::runtime_error("no engine");
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
    if (!engine) throw std::runtime_error("no engine");
    if (!class_freq || !ptn_state_freq) throw std::runtime_error("computePatternStateFreq: null argument");
    computePatternLhCat(WSL_MIXTURE, nullptr);
    check(iqhip_mix_posteriors(engine, class_freq, nullptr, ptn_state_freq), "iqhip_mix_posteriors");
}

void PhyloTree::classLnl(PhyloNeighbor *dad_branch, PhyloNode *dad, const double *class_weight, const double *class_invar,
                         double *lnl, int64_t *floored) {
    if (!engine) throw std::runtime_error("no engine");
    if (nmixture < 2) throw std::runtime_error("classLnl: the model is no mixture (candidates are the classes of a mixture)");
    PhyloNeighbor *back = dad_branch->node->findNeighbor(dad);
    if (!back) throw std::runtime_error("classLnl: not a branch");
    current_it = dad_branch;
    current_it_back = back;
    double df, ddf;
    theta_computed = false;
    computeLikelihoodDerv(dad_branch, dad, df, ddf);   // (re)builds theta of dad_branch
    check(iqhip_class_lnl(engine, branchEnd(dad_branch), branchEnd(back), dad_branch->length, class_weight, class_invar, lnl,
                          floored),
          "iqhip_class_lnl");
}

void PhyloTree::setBootSamples(const float *samples, int nsamples) {
    if (!engine) throw std::runtime_error("no engine");
    pushInputs();
    check(iqhip_set_boot_samples(engine, samples, nsamples), "iqhip_set_boot_samples");
    num_boot_samples = nsamples;
}

void PhyloTree::genBootSamples(int nsamples, int64_t ndraws, uint64_t seed, uint32_t stream, int64_t first_replicate) {
    if (!engine) throw std::runtime_error("no engine");
    pushInputs();
    check(iqhip_gen_boot_samples(engine, nsamples, first_replicate, ndraws, seed, stream), "iqhip_gen_boot_samples");
    num_boot_samples = nsamples;
}

void PhyloTree::computeRELL(std::vector<double> &rell) {
    if (!engine) throw std::runtime_error("no engine");
    if (!current_it) throw std::runtime_error("computeRELL before computeLikelihood");
    rell.assign((size_t)num_boot_samples, 0.0);
    if (allreduce_hook) {  // pattern shards: partial dot products are summed over the ranks
        check(iqhip_rell_async(engine, branchEnd(current_it), branchEnd(current_it_back)), "iqhip_rell_async");
        allreduce_hook(iqhip_result_device_ptr(engine), num_boot_samples, allreduce_ctx);
        check(iqhip_result_read(engine, rell.data(), num_boot_samples), "iqhip_result_read");
    } else
        check(iqhip_rell(engine, branchEnd(current_it), branchEnd(current_it_back), rell.data()), "iqhip_rell");
}

// =========================================================================================
// ultrafast bootstrap bookkeeping, iqtree.cpp:2676-2801 (saveCurrentTree / saveNNITrees), 2803-2880 (summarizeBootstrap)
// =========================================================================================
double PhyloTree::ufbootRand(uint64_t seed, int64_t tree_id) {
    // include/iqhip.h, iqhip_gen_boot_samples: z = mix(mix(mix(seed + G (stream + 1)) + G (rho + 1)) + G (j + 1))
    const uint64_t G = 0x9E3779B97F4A7C15ull;
    auto mix = [](uint64_t z) {
        z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
        z ^= z >> 27; z *= 0x94D049BB133111EBull;
        z ^= z >> 31;
        return z;
    };
    const uint64_t z = mix(mix(mix(seed + G * (0xBBull + 1)) + G * ((uint64_t)tree_id + 1)) + G * 1);
    return (double)(z >> 11) * 0x1.0p-53;
}

void PhyloTree::initUFBoot(int nsamples, uint64_t seed) {
    if (!engine || dry_run) throw std::runtime_error("initUFBoot needs an attached engine");
    if (allreduce_hook) throw std::runtime_error("initUFBoot: not available with a caller-owned collective");
    pushInputs();
    check(iqhip_ufboot_init(engine, nsamples), "iqhip_ufboot_init");
    ufboot_nsamples = nsamples;
    ufboot_seed = seed;
    ufboot_next_id = 0;
    ufboot_logl_cutoff = 0.0;
    ufboot_min_orig_logl = DBL_MAX;
    ufboot_counts[0] = ufboot_counts[1] = ufboot_counts[2] = 0;
    ufboot_trees.clear();
}

void PhyloTree::ufbootNextIteration() {
    if (ufboot_min_orig_logl != DBL_MAX) ufboot_logl_cutoff = ufboot_min_orig_logl;
}

namespace {
// (smallest taxon id, string) of the subtree at `node` seen from `dad` in an adjacency list; children by smallest taxon id
std::pair<int, std::string> sortedSubtree(const std::vector<std::vector<int>> &adj, int node, int dad) {
    if (adj[node].size() <= 1 && dad >= 0) return {node, std::to_string(node)};
    std::vector<std::pair<int, std::string>> kids;
    for (int c : adj[node])
        if (c != dad) kids.push_back(sortedSubtree(adj, c, node));
    std::sort(kids.begin(), kids.end(), [](const std::pair<int, std::string> &a, const std::pair<int, std::string> &b) { return a.first < b.first; });
    std::string s = "(";
    for (size_t k = 0; k < kids.size(); k++) s += (k ? "," : "") + kids[k].second;
    return {kids.empty() ? node : kids[0].first, s + ")"};
}
}  // namespace

std::string PhyloTree::sortedTaxonIdString(const NNIMove *mv) const {
    if (!root || root->neighbors.empty()) return ";";
    std::vector<std::vector<int>> adj(nodes.size());
    for (const PhyloNode *nd : nodes)
        for (const PhyloNeighbor *nb : nd->neighbors) adj[(size_t)nd->id].push_back(nb->node->id);
    if (mv) {   // the subtree at node1_nei goes to node2, the one at node2_nei to node1
        auto swap_in = [&](int at, int from, int to) {
            for (int &x : adj[(size_t)at])
                if (x == from) { x = to; return; }
            throw std::runtime_error("sortedTaxonIdString: the move does not belong to this tree");
        };
        swap_in(mv->node1, mv->node1_nei, mv->node2_nei);
        swap_in(mv->node2, mv->node2_nei, mv->node1_nei);
        swap_in(mv->node1_nei, mv->node1, mv->node2);
        swap_in(mv->node2_nei, mv->node2, mv->node1);
    }
    // MTree::printTree: from the root leaf's neighbour, the root leaf among its children
    return sortedSubtree(adj, root->neighbors[0]->node->id, -1).second + ";";
}

// keeps id -> Newick for the ids of boot_tree only
static void ufbootKeepReferred(std::vector<std::pair<int64_t, std::string>> &trees, const std::vector<int64_t> &boot_tree) {
    std::vector<int64_t> ids(boot_tree);
    std::sort(ids.begin(), ids.end());
    ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
    std::vector<std::pair<int64_t, std::string>> kept;
    for (auto &t : trees)
        if (std::binary_search(ids.begin(), ids.end(), t.first)) kept.push_back(std::move(t));
    trees.swap(kept);
}

void PhyloTree::saveCurrentTree(double logl) {
    if (!engine || dry_run) throw std::runtime_error("saveCurrentTree needs an attached engine");
    if (ufboot_nsamples < 1) throw std::runtime_error("saveCurrentTree before initUFBoot");
    if (!current_it) throw std::runtime_error("saveCurrentTree before computeLikelihood");
    check(iqhip_ptnlh_reserve(engine, 1), "iqhip_ptnlh_reserve");
    check(iqhip_ptnlh_put_current(engine, 0, branchEnd(current_it), branchEnd(current_it_back)), "iqhip_ptnlh_put_current");
    iqhip_ufboot_tree t;
    memset(&t, 0, sizeof t);
    t.row = 0;
    t.tree_id = ufboot_next_id++;
    t.logl = logl;
    t.rand = ufbootRand(ufboot_seed, t.tree_id);
    check(iqhip_ufboot_update(engine, &t, 1, ufboot_epsilon, ufboot_logl_cutoff, ufboot_counts, &ufboot_min_orig_logl),
          "iqhip_ufboot_update");
    if (ufboot_counts[2] == 0) return;
    std::vector<int64_t> boot_tree((size_t)ufboot_nsamples);
    check(iqhip_ufboot_fetch(engine, nullptr, nullptr, nullptr, boot_tree.data()), "iqhip_ufboot_fetch");
    ufboot_trees.push_back({t.tree_id, sortedTaxonIdString()});
    ufbootKeepReferred(ufboot_trees, boot_tree);
}

void PhyloTree::saveNNITrees() {
    if (!engine || dry_run) throw std::runtime_error("saveNNITrees needs an attached engine");
    if (ufboot_nsamples < 1) throw std::runtime_error("saveNNITrees before initUFBoot");
    if (lh_mem_save != LM_ALL_BRANCH) throw std::runtime_error("saveNNITrees needs LM_ALL_BRANCH");
    std::vector<PhyloNode *> n1, n2;
    internalBranches(n1, n2);
    const size_t nc = 2 * n1.size();
    if (nc == 0) return;
    check(iqhip_ptnlh_reserve(engine, (int)(1 + nc)), "iqhip_ptnlh_reserve");
    std::vector<int> rows(nc);
    for (size_t k = 0; k < nc; k++) rows[k] = (int)(1 + k);
    std::vector<NNIMove> moves;
    evaluateNNIs5Batch(moves, rows.data());
    for (size_t k = 0; k < nc; k++)
        if (moves[k].ptnlh_row != rows[k]) throw std::runtime_error("saveNNITrees: NNI moves out of order");
    saveNNITrees(moves);
}

void PhyloTree::saveNNITrees(const std::vector<NNIMove> &moves) {
    if (!engine || dry_run) throw std::runtime_error("saveNNITrees needs an attached engine");
    if (ufboot_nsamples < 1) throw std::runtime_error("saveNNITrees before initUFBoot");
    const size_t nc = moves.size();
    if (nc == 0) return;
    std::vector<iqhip_ufboot_tree> ent(nc);
    const int64_t first_id = ufboot_next_id;
    for (size_t k = 0; k < nc; k++) {
        if (moves[k].ptnlh_row < 0) throw std::runtime_error("saveNNITrees: a move was evaluated without a store row");
        iqhip_ufboot_tree &t = ent[k];
        memset(&t, 0, sizeof t);
        t.row = moves[k].ptnlh_row;
        t.tree_id = ufboot_next_id++;
        t.logl = moves[k].newloglh;
        t.rand = ufbootRand(ufboot_seed, t.tree_id);
    }
    check(iqhip_ufboot_update(engine, ent.data(), (int)nc, ufboot_epsilon, ufboot_logl_cutoff, ufboot_counts, &ufboot_min_orig_logl),
          "iqhip_ufboot_update");
    if (ufboot_counts[2] == 0) return;
    std::vector<int64_t> boot_tree((size_t)ufboot_nsamples);
    check(iqhip_ufboot_fetch(engine, nullptr, nullptr, nullptr, boot_tree.data()), "iqhip_ufboot_fetch");
    std::vector<char> taken(nc, 0);
    for (int64_t id : boot_tree)
        if (id >= first_id) taken[(size_t)(id - first_id)] = 1;
    for (size_t k = 0; k < nc; k++)
        if (taken[k]) ufboot_trees.push_back({first_id + (int64_t)k, sortedTaxonIdString(&moves[k])});
    ufbootKeepReferred(ufboot_trees, boot_tree);
}

// the winner of every replicate (out.boot_trees, out.distinct_trees) and the split counts of the winners
void PhyloTree::ufbootWinners(UFBootSummary &out, ufboot::SplitCounts &sc) {
    if (!engine || dry_run) throw std::runtime_error("summarizeBootstrap needs an attached engine");
    if (ufboot_nsamples < 1) throw std::runtime_error("summarizeBootstrap before initUFBoot");
    const size_t S = (size_t)ufboot_nsamples;
    std::vector<int64_t> boot_tree(S);
    check(iqhip_ufboot_fetch(engine, nullptr, nullptr, nullptr, boot_tree.data()), "iqhip_ufboot_fetch");
    out = UFBootSummary();
    sc = ufboot::SplitCounts(leafNum);
    out.boot_trees.resize(S);
    // trees.convertSplits(taxname, sg, hash_ss, SW_COUNT, ...): every winner once, weighted by its replicates, in the order
    // the replicates first name it
    std::vector<int64_t> order;
    std::vector<int64_t> weight;
    std::vector<const std::string *> text;
    for (size_t s = 0; s < S; s++) {
        const int64_t id = boot_tree[s];
        const auto at = std::lower_bound(ufboot_trees.begin(), ufboot_trees.end(), id,
                                         [](const std::pair<int64_t, std::string> &t, int64_t v) { return t.first < v; });
        if (at == ufboot_trees.end() || at->first != id) throw std::runtime_error("summarizeBootstrap: a replicate holds no tree");
        out.boot_trees[s] = at->second;
        size_t k = 0;
        while (k < order.size() && order[k] != id) k++;
        if (k == order.size()) {
            order.push_back(id);
            weight.push_back(0);
            text.push_back(&at->second);
        }
        weight[k]++;
    }
    out.distinct_trees = (int)order.size();
    std::vector<ufboot::Split> splits;
    for (size_t k = 0; k < order.size(); k++) {
        ufboot::newickSplits(*text[k], leafNum, splits);
        sc.addTree(splits, weight[k]);
    }
}

void PhyloTree::ufbootSplitCounts(ufboot::SplitCounts &sc) {
    UFBootSummary winners;
    ufbootWinners(winners, sc);
}

void PhyloTree::summarizeBootstrap(UFBootSummary &out) {
    ufboot::SplitCounts sc(leafNum);
    ufbootWinners(out, sc);
    const size_t S = (size_t)ufboot_nsamples;
    // createBootstrapSupport: the split of every internal branch of the current tree
    std::vector<PhyloNode *> n1, n2;
    internalBranches(n1, n2);
    std::vector<std::string> label(nodes.size());
    std::vector<std::vector<int>> below(nodes.size());   // taxa below `node` seen from its dad, from the root leaf
    std::vector<std::pair<PhyloNode *, PhyloNode *>> pre;
    pre.push_back({root, nullptr});
    for (size_t k = 0; k < pre.size(); k++)
        for (PhyloNeighbor *nb : pre[k].first->neighbors)
            if (nb->node != pre[k].second) pre.push_back({nb->node, pre[k].first});
    std::vector<int> support_of(nodes.size(), -1);
    std::vector<PhyloNode *> dad_of(nodes.size(), nullptr);
    for (const auto &pr : pre) dad_of[(size_t)pr.first->id] = pr.second;
    for (size_t k = pre.size(); k-- > 0;) {
        PhyloNode *node = pre[k].first, *dad = pre[k].second;
        std::vector<int> &mine = below[(size_t)node->id];
        if (node->isLeaf()) mine.push_back(node->id);
        if (dad) {
            if (!node->isLeaf() && !dad->isLeaf()) {
                ufboot::Split sp(ufboot::splitWords(leafNum), 0);
                for (int t : mine) ufboot::splitSet(sp, t);
                ufboot::splitNormalise(sp, leafNum);
                support_of[(size_t)node->id] = ufboot::splitSupport(sc, sp, (int64_t)S);
                label[(size_t)node->id] = std::to_string(support_of[(size_t)node->id]);
            }
            std::vector<int> &up = below[(size_t)dad->id];
            up.insert(up.end(), mine.begin(), mine.end());
            std::vector<int>().swap(mine);
        }
    }
    for (size_t q = 0; q < n1.size(); q++) {
        out.node1.push_back(n1[q]->id);
        out.node2.push_back(n2[q]->id);
        // the label of an internal branch sits on its node farther from the root
        out.support.push_back(support_of[(size_t)(dad_of[(size_t)n2[q]->id] == n1[q] ? n2[q] : n1[q])->id]);
    }
    std::ostringstream os;
    writeSupportNewick(os, root->neighbors[0]->node, nullptr, label);
    os << ";";
    out.support_tree = os.str();
    std::vector<std::string> names((size_t)leafNum);
    for (int i = 0; i < leafNum; i++) names[(size_t)i] = nodes[(size_t)i]->name.empty() ? std::to_string(i) : nodes[(size_t)i]->name;
    out.consensus_tree = ufboot::consensusTree(sc, names);
}

}  // namespace iqhost
