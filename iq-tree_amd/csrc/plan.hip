// plan.hip -- host side of libiqhip.so: the planner.  build_plan turns the op list of one submission into the DevOp
// descriptors the traversal kernels walk (+ segment table and K2 job list) and iqhip_engine::plan, one pass per job.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <unordered_set>

#include "iqhip_internal.h"

using namespace iqhip;

namespace {

int fail(int code, const std::string &msg) { return set_error(code, msg); }
constexpr int kSentinels = 2;  // descriptors behind the last op: >= the kernels' deepest look-ahead (streamed child: 1 op)

// DevOps needed to hold `bytes` (the segment table and the job list ride in the descriptor buffer)
int devops_for(size_t bytes) { return (int)((bytes + sizeof(DevOp) - 1) / sizeof(DevOp)); }

// the staging of one op list (cut_units)
struct Units {
    std::vector<int> order;                  // order[p] = caller index of the op at position p
    std::vector<int> seg_of;                 // position -> its unit (1, 2, ...); 0: the top stage
    std::vector<std::pair<int, int>> units;  // {begin, nops} in the new order, stage after stage
    std::vector<int> stage_units;            // units per stage (launch)
    int top_begin = 0;                       // first position of the top stage
};

// the segment table behind the sentinels: {top_begin, top_nops, unit1_begin, unit1_nops, ...}
int segment_table_ops(const Units &u) { return devops_for(sizeof(int) * 2 * (1 + u.units.size())); }

// d_ops and its pinned staging copy h_ops (plain host memory for a planning-only engine) for `nops` DevOps
int ensure_plan_capacity(iqhip_engine *e, int nops) {
    if ((size_t)nops <= std::min(e->d_ops.cap, e->h_ops.cap)) return IQHIP_OK;
    const size_t cap = (size_t)std::max(64, nops * 2);
    e->plan_cache.uploaded.clear();
    HIPCHK(e->d_ops.ensure(e, cap));
    if (e->h_ops.ensure(e, cap) != hipSuccess) return fail(IQHIP_ERR_NOMEM, "plan staging");
    return IQHIP_OK;
}

// every pointer a valid target, nothing used: the starting point of each descriptor, and the look-ahead sentinels
void dummy_op(const iqhip_engine *e, DevOp &d) {
    memset(&d, 0, sizeof(d));
    d.dst = e->dummy.plh.p;
    d.dst_sc = e->dummy.sc.p;
    d.pf = d.ld = e->dummy.plh.p;
    d.pf_sc = d.ld_sc = e->dummy.sc.p;
    d.sl = d.sr = e->d_states.p;
    d.tabL = d.tabR = e->d_leaf_tab.p;
    d.pair_row_l = d.pair_row_r = -1;
}

// Same op list as last time and no key created / released / moved since: the descriptors on the device are still the
// right ones (hot loop 1 re-evaluates one tree many times).
bool plan_is_cached(const iqhip_engine *e, const iqhip_node_op *ops, int nops, const std::vector<int> *explicit_segs,
                    const double *const *len_ptrs) {
    const PlanCache &c = e->plan_cache;
    const size_t in_bytes = sizeof(iqhip_node_op) * (size_t)nops;
    // (a removed op whose result this submission's root pass reads: plan again, with that op real)
    for (int q = 0; q < e->n_root_end_keys; q++) {
        const auto it = e->key2slab.find(e->root_end_keys[q]);
        for (const Plan::Virtual &v : e->plan.virt)
            if (it != e->key2slab.end() && it->second == v.slab) return false;
    }
    return !len_ptrs && nops > 0 && c.version == e->keymap_version && c.ops_in.size() == in_bytes &&
           memcmp(c.ops_in.data(), ops, in_bytes) == 0 && !c.uploaded.empty() &&
           (explicit_segs ? c.segs == *explicit_segs : c.segs.empty()) &&
           (!e->plan.uses_cherry || e->plan.cherry_model == e->model_version);
}

// caller-defined independent segments (a batch of branch tasks): one set of workgroups each, no top stage
int cut_explicit(const iqhip_node_op *ops, int nops, const std::vector<int> &segs, Units &u) {
    std::unordered_set<uint64_t> dsts;
    for (int k = 0; k < nops; k++)
        if (!dsts.insert(ops[k].dst_key).second)
            return fail(IQHIP_ERR_INVALID, "batched node updates must write distinct vectors");
    int pos = 0;
    for (const int n : segs) {
        if (n <= 0) continue;
        if (pos + n > nops) break;   // (refused below)
        u.units.push_back({pos, n});
        for (int q = 0; q < n; q++) u.seg_of[pos + q] = (int)u.units.size();
        pos += n;
    }
    if (pos != nops) return fail(IQHIP_ERR_INVALID, "segment sizes do not add up to the op count");
    u.stage_units.push_back((int)u.units.size());
    u.top_begin = nops;
    return IQHIP_OK;
}

// unit size of the automatic staging (0: none)
int unit_target(const iqhip_engine *e, int nops) {
    if (e->split_target >= 0) return e->split_target;
    const int64_t simds = (int64_t)e->num_cus * 4;
    // the matrix-core kernels (16-pattern tiles, long per-tile op lists) when there are fewer than 6 tile-waves per
    // SIMD; unit size so that the first launch has ~4 waves per SIMD.  Measured at the BASELINE shapes: protein 1.28 ->
    // 1.10 ms, codon 0.64 -> 0.49 ms; the 4-state kernel is store-bound and loses (0.161 -> 0.172..0.184 ms), so it
    // stays unsplit.
    int target = 0;
    if (e->mfma && e->ntiles < 6 * simds && nops >= 12)
        target = (int)std::min<int64_t>(nops / 2, std::max<int64_t>(3, ((int64_t)nops * e->ntiles + 4 * simds - 1) / (4 * simds)));
    // 4-state kernel: only while the whole alignment is at most one wave per SIMD, where a traversal is a latency-bound
    // chain (50 taxa GTR+G4: 5k patterns 0.082 -> 0.045 ms, 20k 0.086 -> 0.060 ms; 60k patterns 0.109 -> 0.126 ms, so
    // not there)
    if (!e->mfma && e->ntiles * e->lane_split <= simds && nops >= 12) target = std::max(6, nops / 4);
    return target;
}

// lc[k] / rc[k]: the op whose result is op k's left / right child (-1: a leaf or an outside vector).  False when re-ordering
// is unsafe: a vector is both an outside input and a destination (LM_PER_NODE buffer stealing), written or consumed twice.
bool producer_links(const iqhip_node_op *ops, int nops, std::vector<int> &lc, std::vector<int> &rc) {
    std::unordered_map<uint64_t, int> prod;
    std::unordered_set<uint64_t> ext_in;
    std::vector<char> consumed(nops, 0);
    lc.assign(nops, -1);
    rc.assign(nops, -1);
    for (int k = 0; k < nops; k++) {
        const iqhip_node_op &o = ops[k];
        for (int side = 0; side < 2; side++) {
            if ((side ? o.right_leaf : o.left_leaf) >= 0) continue;
            const uint64_t key = side ? o.right_key : o.left_key;
            auto it = prod.find(key);
            if (it == prod.end()) { ext_in.insert(key); continue; }
            if (consumed[it->second]++) return false;
            (side ? rc : lc)[k] = it->second;
        }
        if (!prod.emplace(o.dst_key, k).second) return false;
    }
    for (int k = 0; k < nops; k++)
        if (ext_in.count(ops[k].dst_key)) return false;
    return true;
}

// Level by level: among the ops not yet placed, the maximal subtrees of 2..target ops (vectors of earlier levels count
// as outside inputs) become the units of the next launch; what is left after the last level walks sequentially.  Every
// level is a launch of tiles x units waves, so the sequential tail -- where an alignment with slightly more tiles than
// SIMDs runs at half speed -- shrinks from "everything above the first cut" to a few ops.
void cut_subtrees(int nops, int target, int max_levels, const std::vector<int> &lc, const std::vector<int> &rc, Units &u) {
    std::vector<char> placed(nops, 0);
    std::vector<int> new_order;
    new_order.reserve(nops);
    const int min_top = std::max(2, std::min(target, 6));
    for (int level = 0; level < max_levels && nops - (int)new_order.size() > min_top; level++) {
        std::vector<int> rem;  // unplaced ops in post-order
        for (int k = 0; k < nops; k++)
            if (!placed[k]) rem.push_back(k);
        const int R = (int)rem.size();
        std::vector<int> pos_of(nops, -1), l2(R, -1), r2(R, -1), sz(R, 1);
        std::vector<char> cont(R, 1), cons(R, 0);
        for (int q = 0; q < R; q++) pos_of[rem[q]] = q;
        for (int q = 0; q < R; q++) {
            const int k = rem[q];
            if (lc[k] >= 0 && !placed[lc[k]]) { l2[q] = pos_of[lc[k]]; cons[l2[q]] = 1; sz[q] += sz[l2[q]]; }
            if (rc[k] >= 0 && !placed[rc[k]]) { r2[q] = pos_of[rc[k]]; cons[r2[q]] = 1; sz[q] += sz[r2[q]]; }
            // post-order contiguity within the unplaced sequence: the subtree of q is exactly [q - sz + 1, q]
            const int a = std::max(l2[q], r2[q]), b2 = std::min(l2[q], r2[q]);
            bool c2 = true;
            if (a >= 0) c2 = (a == q - 1) && cont[a];
            if (b2 >= 0) c2 = c2 && (b2 == a - sz[a]) && cont[b2];
            cont[q] = c2;
        }
        std::vector<int> stack;
        for (int q = R - 1; q >= 0; q--)
            if (!cons[q]) stack.push_back(q);
        std::vector<std::pair<int, int>> found;  // {root position, size}
        while (!stack.empty()) {
            const int q = stack.back();
            stack.pop_back();
            if (sz[q] <= target && sz[q] >= 2 && cont[q]) {
                found.push_back({q, sz[q]});
            } else {
                if (l2[q] >= 0) stack.push_back(l2[q]);
                if (r2[q] >= 0) stack.push_back(r2[q]);
            }
        }
        if (found.size() < 2) break;
        std::stable_sort(found.begin(), found.end(),
                         [](const std::pair<int, int> &x, const std::pair<int, int> &y2) { return x.second > y2.second; });
        for (const std::pair<int, int> &f : found) {
            u.units.push_back({(int)new_order.size(), f.second});
            for (int q = f.first - f.second + 1; q <= f.first; q++) {
                u.seg_of[new_order.size()] = (int)u.units.size();
                placed[rem[q]] = 1;
                new_order.push_back(rem[q]);
            }
        }
        u.stage_units.push_back((int)found.size());
    }
    if (u.units.empty()) return;
    u.top_begin = (int)new_order.size();
    for (int k = 0; k < nops; k++)
        if (!placed[k]) { u.seg_of[new_order.size()] = 0; new_order.push_back(k); }
    u.order = std::move(new_order);
}

// The staging.  A launch gives every 64/16-pattern tile one wave that walks the whole op list, so an alignment with few
// tiles leaves SIMDs idle or unevenly loaded (a tile is an indivisible unit of nops updates).  Independent subtrees of
// the plan are therefore cut out as "units" that run on their own workgroups in a first launch (tiles x units waves),
// and only the ops above them ("top") walk sequentially in a second launch.  Writes nothing to the engine.
int cut_units(const iqhip_engine *e, const iqhip_node_op *ops, int nops, const std::vector<int> *explicit_segs, Units &u) {
    u.order.resize(nops);
    for (int k = 0; k < nops; k++) u.order[k] = k;
    u.seg_of.assign(nops, 0);
    if (explicit_segs) {
        const int rc = cut_explicit(ops, nops, *explicit_segs, u);
        if (rc) return rc;
    } else {
        const int target = unit_target(e, nops);
        std::vector<int> lc, rc;
        if (target > 0 && target < nops && nops >= 4 && producer_links(ops, nops, lc, rc))
            cut_subtrees(nops, target, e->max_levels, lc, rc, u);
    }
    if (e->debug_plan) {
        fprintf(stderr, "[iqhip] plan: %d ops, %zu stages of units (", nops, u.stage_units.size());
        size_t ui = 0;
        for (int n : u.stage_units) {
            for (int q = 0; q < n; q++) fprintf(stderr, "%d ", u.units[ui++].second);
            fprintf(stderr, "| ");
        }
        fprintf(stderr, ") top %d ops\n", nops - u.top_begin);
    }
    return IQHIP_OK;
}

// A removed leaf-leaf op as its consumer sees it
struct PairDef { int32_t taxon_l, taxon_r; double len_l, len_r; int row; const uint8_t *codes; };
// What select_pair_children leaves: the ops that stay, in the caller's order, with the caller's row of each, and the removed
// ones by the key of their result
struct Kept {
    std::vector<iqhip_node_op> ops;
    std::vector<int> row;
    std::unordered_map<uint64_t, PairDef> pairs;
};

uint64_t pair_key(int32_t tl, int32_t tr) { return ((uint64_t)(uint32_t)tl << 32) | (uint32_t)tr; }

// *row: the pair-code row of an ordered pair of taxa, built if the pair has none yet (nullptr: no slot left, the op stays real)
int pair_code_row(iqhip_engine *e, int32_t tl, int32_t tr, const uint8_t **row) {
    const size_t P = (size_t)e->nptn_pad, nslots = e->d_pair_rows.cap / P;
    *row = nullptr;
    auto it = e->pair_row_of.find(pair_key(tl, tr));
    if (it != e->pair_row_of.end()) { *row = e->d_pair_rows.p + (size_t)it->second * P; return IQHIP_OK; }
    if (e->pair_row_of.size() >= nslots) { e->pair_ops_without_row++; return IQHIP_OK; }
    const int slot = (int)e->pair_row_of.size();
    uint8_t *out = e->d_pair_rows.p + (size_t)slot * P;
    if (!e->planner) HIPCHK(launch_pair_codes(e, e->d_states.p + (size_t)tl * P, e->d_states.p + (size_t)tr * P, out));
    e->pair_row_of[pair_key(tl, tr)] = slot;
    *row = out;
    return IQHIP_OK;
}

// Leaf-leaf node updates that k_traverse4 need not run (DESIGN.md 3.1 "Pair children"): the vector of such a node depends on
// the pair of leaf states only, so its one consumer reads a 25-row table instead (CHILD_PAIR), the op leaves the list and its
// slab is marked virtual.  An op is removed when: both children are leaves whose rows hold only states 0 .. 3 and
// STATE_UNKNOWN; its scaling rule is 0; exactly one later op of this plan consumes its result, nothing else writes that key
// and it is not the plan's last op; the plan is cut automatically and takes its lengths from the host (no explicit segments,
// no sweep pointers); and its consumer still fits a chunk of its own with that child as a pair child -- both children's regions,
// their state slots and slot 0 within lds_budget(e) (a pair child's region is 38 blocks, a leaf's 6: at a tight IQHIP_LDS_KB an
// op that fits with a real cherry below it would not with the table).  A consumer of two such ops: both removed if the two pair
// regions fit together; else the left one removed and the right one real if that fits; else both real.
// Consumer and producer then share a segment, because the producer no longer exists.
// Returns whether anything was removed (then `kept` is the list to plan).
int select_pair_children(iqhip_engine *e, const iqhip_node_op *ops, int nops, const std::vector<int> *explicit_segs,
                         const double *const *len_ptrs, Kept &kept, bool *any) {
    *any = false;
    if (e->mfma || e->wide4 || e->n != 4 || e->n_user != 4 || e->embed2 || e->scalar_rule_all || explicit_segs || len_ptrs ||
        nops < 2 || e->taxon_plain.size() != (size_t)e->ntaxa)
        return IQHIP_OK;
    std::unordered_map<uint64_t, int> writes, reads, first_read;
    for (int k = 0; k < nops; k++) {
        writes[ops[k].dst_key]++;
        for (int side = 0; side < 2; side++) {
            if ((side ? ops[k].right_leaf : ops[k].left_leaf) >= 0) continue;
            const uint64_t key = side ? ops[k].right_key : ops[k].left_key;
            if (!reads[key]++) first_read[key] = k;
        }
    }
    std::vector<char> removed((size_t)nops, 0);
    int nremoved = 0;
    for (int k = 0; k + 1 < nops; k++) {
        const iqhip_node_op &o = ops[k];
        if (o.left_leaf < 0 || o.right_leaf < 0 || o.left_leaf >= e->ntaxa || o.right_leaf >= e->ntaxa) continue;
        if (o.flags & (IQHIP_OP_NO_SCALE | IQHIP_OP_SCALAR_RULE)) continue;
        if (!e->taxon_plain[o.left_leaf] || !e->taxon_plain[o.right_leaf]) continue;
        if (!(o.left_len >= 0.0) || !(o.right_len >= 0.0)) continue;   // (refused by fill_descriptors)
        if (writes[o.dst_key] != 1 || reads[o.dst_key] != 1 || first_read[o.dst_key] <= k) continue;
        // (a root-branch end of this submission is read from memory by the root pass: cheaper left real than expanded every time)
        if (std::find(e->root_end_keys, e->root_end_keys + e->n_root_end_keys, o.dst_key) != e->root_end_keys + e->n_root_end_keys) continue;
        removed[k] = 1;
        nremoved++;
    }
    if (!nremoved) return IQHIP_OK;
    // the consumers' fit: what lay_out_lds charges an op that opens a chunk (a vector child: one block, no state slot)
    const int B = e->block, budget = lds_budget(e), slot_sz = trav4_lds(B).slot_doubles;
    auto child_need = [&](int32_t kind) { return child_region_blocks(kind) * B + (child_is_table(kind) ? slot_sz : 0); };
    std::unordered_map<uint64_t, int> candidate;   // key -> the op that may be removed
    for (int k = 0; k < nops; k++)
        if (removed[k]) candidate[ops[k].dst_key] = k;
    for (int k = 0; k < nops; k++) {
        const iqhip_node_op &o = ops[k];
        const auto li = o.left_leaf < 0 ? candidate.find(o.left_key) : candidate.end();
        const auto ri = o.right_leaf < 0 ? candidate.find(o.right_key) : candidate.end();
        const int l = li == candidate.end() ? -1 : li->second, r = ri == candidate.end() ? -1 : ri->second;
        if (l < 0 && r < 0) continue;
        const int32_t lkind = o.left_leaf >= 0 ? CHILD_LEAF : CHILD_PF, rkind = o.right_leaf >= 0 ? CHILD_LEAF : CHILD_PF;
        auto fits = [&](int32_t a, int32_t b) { return slot_sz + child_need(a) + child_need(b) <= budget; };
        bool keep_l = l >= 0, keep_r = r >= 0;   // (as pair children)
        if (l >= 0 && r >= 0) {
            if (!fits(CHILD_PAIR, CHILD_PAIR)) { keep_r = false; keep_l = fits(CHILD_PAIR, CHILD_PF); }
        } else if (l >= 0) {
            keep_l = fits(CHILD_PAIR, rkind);
        } else {
            keep_r = fits(lkind, CHILD_PAIR);
        }
        if (l >= 0 && !keep_l) { removed[l] = 0; nremoved--; }
        if (r >= 0 && !keep_r) { removed[r] = 0; nremoved--; }
    }
    if (!nremoved) return IQHIP_OK;
    // the code rows: one buffer of ntaxa slots (a tree has at most ntaxa / 2 leaf-leaf nodes); a search that has walked through
    // more pairs than that starts over -- kernels still reading the old rows are ahead of the new builds on the stream
    const size_t P = (size_t)e->nptn_pad;
    if (e->d_pair_rows.cap < (size_t)e->ntaxa * P) {
        HIPCHK(e->d_pair_rows.ensure(e, (size_t)e->ntaxa * P));
        e->pair_row_of.clear();
    }
    size_t nmissing = 0;   // pairs of this plan that have no row yet (a pair occurs once in a tree)
    for (int k = 0; k < nops; k++)
        nmissing += removed[k] && !e->pair_row_of.count(pair_key(ops[k].left_leaf, ops[k].right_leaf));
    if (e->pair_row_of.size() + nmissing > e->d_pair_rows.cap / P) {
        e->pair_row_of.clear();
        e->pair_row_restarts++;
    }
    for (int k = 0; k < nops; k++) {
        if (removed[k]) {
            const iqhip_node_op &o = ops[k];
            const uint8_t *codes;
            int rc = pair_code_row(e, o.left_leaf, o.right_leaf, &codes);
            if (rc) return rc;
            if (codes) {
                int didx;
                rc = slab_for_key(e, o.dst_key, true, &didx);   // (the slab keeps its allocation)
                if (rc) return rc;
                kept.pairs[o.dst_key] = {o.left_leaf, o.right_leaf, o.left_len, o.right_len, k, codes};
                e->plan.virt.push_back({didx, o.left_leaf, o.right_leaf, o.left_len, o.right_len});
                continue;
            }
        }
        kept.ops.push_back(ops[k]);
        kept.row.push_back(k);
    }
    *any = !kept.pairs.empty();
    if (e->debug_plan) fprintf(stderr, "[iqhip] plan: %zu of %d ops removed as pair children\n", kept.pairs.size(), nops);
    return IQHIP_OK;
}

// the slabs of the plan's removed ops are virtual from this submission on (a cached plan too: every submission "computes" them)
void mark_virtual_slabs(iqhip_engine *e) {
    for (const Plan::Virtual &v : e->plan.virt) {
        Slab &s = e->slabs[v.slab];
        s.virt = true;
        s.taxon_l = v.taxon_l; s.taxon_r = v.taxon_r;
        s.len_l = v.len_l; s.len_r = v.len_r;
    }
    e->pair_ops_removed += (int64_t)e->plan.virt.size();
}

// One DevOp per op, in the staged order: children resolved to slabs / state rows and put in the kernels' canonical
// form.  *last_dst: the slab the last op writes (-1: none).  rows / pairs: select_pair_children's (nullptr: nothing removed)
int fill_descriptors(iqhip_engine *e, const iqhip_node_op *ops, int nops, const Units &u, const double *const *len_ptrs,
                     int *last_dst, const Kept *kept) {
    int prev_dst = -1;
    for (int k = 0; k < nops; k++) {
        const iqhip_node_op &o = ops[u.order[k]];
        DevOp &d = e->h_ops.p[k];
        dummy_op(e, d);
        d.out_row = kept ? kept->row[u.order[k]] : u.order[k];
        d.no_scale = (o.flags & IQHIP_OP_NO_SCALE) ? 1 : (((o.flags & IQHIP_OP_SCALAR_RULE) || e->scalar_rule_all) ? 2 : 0);
        if (k > 0 && u.seg_of[k] != u.seg_of[k - 1]) prev_dst = -1;  // another workgroup: no register hand-over
        if (!(o.left_len >= 0.0) || !(o.right_len >= 0.0))
            return fail(IQHIP_ERR_INVALID, "negative or NaN branch length");
        const double *lp, *rp; const int16_t *lsc, *rsc;
        const uint8_t *lst, *rst; int32_t lkind, rkind;
        // (a removed op's result is never looked up as a slab: that would expand it)
        const PairDef *lpair = nullptr, *rpair = nullptr;
        if (kept && o.left_leaf < 0 && kept->pairs.count(o.left_key)) lpair = &kept->pairs.at(o.left_key);
        if (kept && o.right_leaf < 0 && kept->pairs.count(o.right_key)) rpair = &kept->pairs.at(o.right_key);
        int rc = IQHIP_OK;
        if (lpair) { lp = nullptr; lsc = nullptr; lst = lpair->codes; lkind = CHILD_PAIR; }
        else rc = resolve_child(e, o.left_key, o.left_leaf, prev_dst, &lp, &lsc, &lst, &lkind);
        if (rc) return rc;
        if (rpair) { rp = nullptr; rsc = nullptr; rst = rpair->codes; rkind = CHILD_PAIR; }
        else rc = resolve_child(e, o.right_key, o.right_leaf, prev_dst, &rp, &rsc, &rst, &rkind);
        if (rc) return rc;
        int didx;
        rc = slab_for_key(e, o.dst_key, true, &didx);
        if (rc) return rc;
        if ((!child_is_table(lkind) && lp == e->slabs[didx].plh.p) || (!child_is_table(rkind) && rp == e->slabs[didx].plh.p))
            return fail(IQHIP_ERR_INVALID, "node update writes onto one of its own children");
        if (lkind == CHILD_PREV && rkind == CHILD_PREV)
            return fail(IQHIP_ERR_INVALID, "node update uses the same vector for both children");
        double llen = o.left_len, rlen = o.right_len;
        const double *llen_p = len_ptrs ? len_ptrs[2 * u.order[k]] : nullptr, *rlen_p = len_ptrs ? len_ptrs[2 * u.order[k] + 1] : nullptr;
        d.dst = e->slabs[didx].plh.p;
        d.dst_sc = e->slabs[didx].sc.p;
        if (e->mfma && !e->mfma_pipelined) {
            // generic matrix-core kernel: both children are read from memory (pf = left, ld = right)
            if (lkind != CHILD_LEAF) { lkind = CHILD_LOAD; d.pf = lp; d.pf_sc = lsc; } else d.sl = lst;
            if (rkind != CHILD_LEAF) { rkind = CHILD_LOAD; d.ld = rp; d.ld_sc = rsc; } else d.sr = rst;
        } else {
            // canonical form (the Hadamard product commutes): left in {LEAF, PF}, right in
            // {LEAF, PREV}; the only other shape is (PF, LOAD): two memory children, neither of
            // them the previous result -- the kernel reads the second one synchronously.
            auto swap_children = [&]() {
                std::swap(lp, rp); std::swap(lsc, rsc); std::swap(lst, rst);
                std::swap(lkind, rkind); std::swap(llen, rlen); std::swap(llen_p, rlen_p); std::swap(lpair, rpair);
            };
            if (lkind == CHILD_PREV) swap_children();                              // PREV goes right
            else if (child_is_table(lkind) && rkind == CHILD_LOAD) swap_children();  // memory child goes left
            if (lkind == CHILD_LOAD) lkind = CHILD_PF;
            if (rkind == CHILD_LOAD) (u.seg_of[k] ? e->plan.units_have_load : e->plan.has_load) = true;  // (PF, LOAD)
            if (lkind == CHILD_PF) { d.pf = lp; d.pf_sc = lsc; d.real_mask |= 1; }
            if (rkind == CHILD_LOAD) { d.ld = rp; d.ld_sc = rsc; }
            if (child_is_table(lkind)) d.sl = lst;
            if (child_is_table(rkind)) d.sr = rst;
            if (lpair) { d.pair_len[0] = lpair->len_l; d.pair_len[1] = lpair->len_r; d.pair_row_l = lpair->row; }
            if (rpair) { d.pair_len[2] = rpair->len_l; d.pair_len[3] = rpair->len_r; d.pair_row_r = rpair->row; }
        }
        d.left_kind = lkind; d.right_kind = rkind;
        d.left_len = llen; d.right_len = rlen;
        d.left_len_p = llen_p; d.right_len_p = rlen_p;
        prev_dst = didx;
    }
    *last_dst = prev_dst;
    return IQHIP_OK;
}

// HOLD analysis (4-state kernel): a streamed left child produced by op j of this plan can stay in registers until its
// join k if no op in (j, k) streams, loads or parks anything itself (the usual case after heavier-first ordering: the
// other subtree is a short chain).  20 states, one wave per tile: the parking place is LDS; the launch reserves it when
// plan.nhold > 0.
void park_operands(iqhip_engine *e, int nops, const std::vector<int> &seg_of) {
    const bool hold_regs = !e->mfma;
    const bool hold_in_lds = e->mfma && e->mfma_pipelined && e->hold_lds && e->n == 20 && !e->cat_split;
    std::unordered_map<const double *, int> producer;   // vector -> the op of this plan that writes it
    for (int k = 0; k < nops && (hold_regs || hold_in_lds); k++) {
        DevOp &d = e->h_ops.p[k];
        const auto it = d.left_kind == CHILD_PF ? producer.find(d.pf) : producer.end();
        const int j = it == producer.end() ? -1 : it->second;
        producer[d.dst] = k;
        if (j < 0) continue;
        bool ok = !e->h_ops.p[j].push_hold && seg_of[j] == seg_of[k];
        if (hold_in_lds && top_stage_may_share_tiles(e) && seg_of[k] == 0) ok = false;   // (no parking place there)
        for (int q = j + 1; q < k && ok; q++) {
            const DevOp &m = e->h_ops.p[q];
            ok = m.left_kind != CHILD_PF && m.left_kind != CHILD_HOLD && m.right_kind != CHILD_LOAD && !m.push_hold;
        }
        if (!ok) continue;
        e->h_ops.p[j].push_hold = 1;
        d.left_kind = CHILD_HOLD;
        d.pf = e->dummy.plh.p;
        d.pf_sc = e->dummy.sc.p;
        d.real_mask &= ~1;
        e->plan.nhold++;
    }
    if (e->debug_plan) {
        int npf = 0;
        for (int k = 0; k < nops; k++) npf += (e->h_ops.p[k].left_kind == CHILD_PF) + (e->h_ops.p[k].right_kind == CHILD_LOAD);
        fprintf(stderr, "[iqhip] plan: %d children read back from memory, %d parked\n", npf, e->plan.nhold);
    }
}

// K2 tables of the leaf children (pipelined matrix-core kernels): slot = taxon, rebuilt by k_leaf_tables before the
// traversal only where the pendant branch length (or the model) changed since the slot was last built
int assign_leaf_tables(iqhip_engine *e, int nops) {
    if (!(e->mfma && e->mfma_pipelined && e->leaf_tables)) return IQHIP_OK;
    const size_t per = leaf_table_doubles(e);
    leaf_tables_follow_model(e);   // (the new plan has no tables yet: after a model change every slot is stale)
    struct Use { double len; const double *len_p; int slot; };
    std::unordered_map<int, std::vector<Use>> seen;  // taxon -> lengths used in this plan
    int noverflow = 0;
    std::vector<TabJob> dirty, clean;
    std::vector<std::pair<int, int>> uses;  // (op index, side) -> slot, resolved to pointers after (re)allocation
    std::vector<int> use_slot;
    for (int k = 0; k < nops; k++) {
        const DevOp &d = e->h_ops.p[k];
        for (int side = 0; side < 2; side++) {
            if ((side ? d.right_kind : d.left_kind) != CHILD_LEAF) continue;
            const uint8_t *row = side ? d.sr : d.sl;
            const int taxon = (int)((row - e->d_states.p) / e->nptn_pad);
            const double *len_p = side ? d.right_len_p : d.left_len_p;   // (sweeps: the length is on the device)
            const double len = len_p ? NAN : (side ? d.right_len : d.left_len);
            std::vector<Use> &u = seen[taxon];
            int slot = -1;
            for (const Use &x : u)
                if (x.len_p == len_p && (len_p || x.len == len)) slot = x.slot;
            if (slot < 0) {
                slot = u.empty() ? taxon : e->ntaxa + noverflow++;
                u.push_back({len, len_p, slot});
                const TabJob j = {len, reinterpret_cast<double *>((size_t)slot), len_p, 0.0};  // (tab: the slot number for now)
                const bool cached = !len_p && slot < e->ntaxa && (size_t)slot < e->tab_len.size() && e->tab_len[slot] == len;
                (cached ? clean : dirty).push_back(j);
            }
            uses.push_back({k, side});
            use_slot.push_back(slot);
        }
    }
    const size_t need = (size_t)e->ntaxa + (size_t)noverflow;
    if (need > e->d_leaf_tab.cap / per) {
        HIPCHK(e->d_leaf_tab.ensure(e, (need + 16) * per));
        e->plan_cache.uploaded.clear();
        // a new buffer holds no tables: everything this plan uses is dirty
        dirty.insert(dirty.end(), clean.begin(), clean.end());
        clean.clear();
        e->tab_len.assign(e->d_leaf_tab.cap / per, NAN);
    }
    if (e->tab_len.size() < e->d_leaf_tab.cap / per) e->tab_len.resize(e->d_leaf_tab.cap / per, NAN);
    // non-leaf children point at slot 0: the kernels may request a row unconditionally (one step ahead)
    for (int k = 0; k < nops; k++) e->h_ops.p[k].tabL = e->h_ops.p[k].tabR = e->d_leaf_tab.p;
    for (size_t q = 0; q < uses.size(); q++) {
        DevOp &d = e->h_ops.p[uses[q].first];
        (uses[q].second ? d.tabR : d.tabL) = e->d_leaf_tab.p + (size_t)use_slot[q] * per;
    }
    for (std::vector<TabJob> *v : {&dirty, &clean})
        for (TabJob &j : *v) {
            const size_t slot = (size_t)j.tab;
            j.tab = e->d_leaf_tab.p + slot * per;
            e->tab_len[slot] = slot < (size_t)e->ntaxa ? j.len : NAN;  // overflow slots are never reused
            e->plan.tab_jobs.push_back(j);
        }
    e->plan.tab_dirty = (int)dirty.size();
    e->plan.nleaf_tabs = (int)e->plan.tab_jobs.size();
    return IQHIP_OK;
}

// cherry tables: an op whose two children are leaves reads its result out of the table of its pair of taxa
int assign_cherry_tables(iqhip_engine *e, int nops, const std::vector<int> &seg_of) {
    // (planning-only engine: the tables are never built, their slots are fake addresses like every other buffer)
    const bool have_pair = e->planner ? e->cherry_s2 > 0 : (e->pair && e->cherry_model_synced);
    if (!(cherry_candidate(e) && e->mfma_pipelined && have_pair && nops >= 8)) return IQHIP_OK;
    const size_t per = (size_t)e->cherry_npairs * e->block;
    const size_t want = (size_t)2 * e->ntaxa + 16;
    const bool fresh = e->d_cherry_tab.cap < want * per;   // (a new buffer holds no tables)
    if (fresh) HIPCHK(e->d_cherry_tab.ensure(e, want * per));
    const size_t cherry_cap = e->d_cherry_tab.cap / per;    // slots allocated
    // room for every cherry a plan can hold; a search that has walked through more pairs than that starts over
    if (fresh || e->cherry_slots.size() + (size_t)e->ntaxa / 2 + 1 > cherry_cap) {
        e->cherry_slot_of.clear();
        e->cherry_slots.clear();
    }
    const uint64_t stamp = ++e->cherry_stamp;
    for (int k = 0; k < nops; k++) {
        DevOp &d = e->h_ops.p[k];
        if (d.left_kind != CHILD_LEAF || d.right_kind != CHILD_LEAF || d.left_len_p || d.right_len_p) continue;
        // (the top stage's two-waves-per-tile / row-split kernels compute their cherries)
        if ((top_stage_may_share_tiles(e) || top_stage_may_mix_roles64(e)) && seg_of[k] == 0) continue;
        const uint64_t tl = (uint64_t)((d.sl - e->d_states.p) / e->nptn_pad), tr = (uint64_t)((d.sr - e->d_states.p) / e->nptn_pad);
        const uint64_t key = (tl << 32) | tr;
        auto it = e->cherry_slot_of.find(key);
        int slot;
        if (it == e->cherry_slot_of.end()) {
            if (e->cherry_slots.size() >= cherry_cap) continue;
            slot = (int)e->cherry_slots.size();
            e->cherry_slots.emplace_back();
            e->cherry_slot_of[key] = slot;
        } else {
            slot = it->second;
        }
        iqhip_engine::CherrySlot &cs = e->cherry_slots[slot];
        const bool same = cs.len_l == d.left_len && cs.len_r == d.right_len;
        if (cs.stamp == stamp && !same) continue;   // (the same pair with other lengths in one plan: computed the ordinary way)
        if (!same || cs.model_version != e->model_version) {
            cs.len_l = d.left_len;
            cs.len_r = d.right_len;
            cs.model_version = 0;   // until built (submit_traverse)
            if (cs.stamp != stamp) e->plan.cherry_jobs.push_back(slot);
        }
        cs.stamp = stamp;
        d.cherry = e->d_cherry_tab.p + (size_t)slot * per;
        e->plan.uses_cherry = true;
    }
    return IQHIP_OK;
}

// LDS layout of the per-(op, child) regions, cut into chunks that fit the budget
int lay_out_lds(iqhip_engine *e, int nops, const std::vector<int> &seg_of) {
    const int B = e->block, budget = lds_budget(e);
    const bool tables_in_lds = e->mfma && e->mfma_pipelined && e->n == 20 && e->plan.nleaf_tabs > 0;
    // a LEAF child's region: 4 states -- exponentials + the 5-row K2 table; 20 states with leaf tables -- the child's
    // whole K2 table [ncat][STATE_UNKNOWN][n], copied from the table buffer when the chunk is filled
    // (wide DNA: as the 4-state kernel, on both of its routes -- the generic kernel reads the exponentials only)
    const int leaf_sz = (!e->mfma || e->wide4) ? child_region_blocks(CHILD_LEAF) * B : (tables_in_lds ? (int)leaf_table_doubles(e) : B);
    const int pair_sz = child_region_blocks(CHILD_PAIR) * B;   // (k_traverse4 only: no other plan holds a PAIR child)
    const int slot_sz = e->mfma ? 0 : trav4_lds(B).slot_doubles;   // (slot 0: the non-leaf children's)
    int chunk_start = 0, used = slot_sz, regs = 0, max_used = 0, slots = 1, max_slots = 1;
    // k_traverse4's fill image: the chunks' regions one behind the other, each chunk its own extent (a multiple of the block:
    // 16-byte aligned); every op of a chunk carries the chunk's offset
    int64_t image = 0;
    bool image_ok = !e->mfma && e->fill_image.on;
    auto close_chunk = [&](int end) {
        e->h_ops.p[chunk_start].chunk_nops = end - chunk_start;
        e->h_ops.p[chunk_start].chunk_slots = slots;
        if (e->mfma) return;
        for (int q = chunk_start; q < end; q++) e->h_ops.p[q].image_off = (int32_t)image;
        image += regs;
    };
    for (int k = 0; k < nops; k++) {
        DevOp &d = e->h_ops.p[k];
        if (d.left_len_p || d.right_len_p) image_ok = false;   // (lengths the host does not know)
        const int szl = d.left_kind == CHILD_LEAF ? leaf_sz : (d.left_kind == CHILD_PAIR ? pair_sz : B);
        const int szr = d.right_kind == CHILD_LEAF ? leaf_sz : (d.right_kind == CHILD_PAIR ? pair_sz : B);
        // 4-state path: each leaf / pair child also stages one state byte per thread in LDS
        const int nleaf = child_is_table(d.left_kind) + child_is_table(d.right_kind);
        const int need = szl + szr + nleaf * slot_sz;
        // (an op must fit a chunk of its own, slot 0 included: what check_plan holds every chunk to)
        if (slot_sz + need > budget) return fail(IQHIP_ERR_UNSUPPORTED, "nstates*ncat too large for the LDS plan regions");
        // (k_traverse4 keeps one row pointer per slot of the chunk in a fixed array)
        const bool rows_full = !e->mfma && slots + nleaf > kTrav4RowSlots;
        if ((used + need > budget || rows_full || seg_of[k] != seg_of[k - (k > 0)]) && k > chunk_start) {
            close_chunk(k);
            chunk_start = k; used = slot_sz; regs = 0; slots = 1;
        }
        d.lds_left = regs; d.lds_right = regs + szl;
        regs += szl + szr;
        used += need;
        if (regs > max_used) max_used = regs;
        d.sl_slot = child_is_table(d.left_kind) ? slots++ : 0;
        d.sr_slot = child_is_table(d.right_kind) ? slots++ : 0;
        if (slots > max_slots) max_slots = slots;
    }
    if (nops > 0) close_chunk(nops);
    if (image * (int64_t)sizeof(double) > INT32_MAX) image_ok = false;   // (the kernel's 32-bit byte offsets)
    e->plan.image_doubles = image;
    e->plan.image_ok = image_ok && image > 0;
    e->plan.state_slots = max_slots;
    e->plan.lds_doubles = max_used;
    return IQHIP_OK;
}

// The kernels' contract on a plan, checked on the host before the descriptors go to the device (IQHIP_CHECK_PLAN=1; always
// for a planning-only engine).  The traversal kernels issue the requests of op k+1 unconditionally while op k computes
// (streamed child, its counters, leaf state rows, K2 table rows), so EVERY pointer of EVERY descriptor -- the look-ahead
// sentinels behind the last op included -- must be a dereferenceable address of the right kind even when the op does not
// use it: a null tabL / tabR of a non-leaf child was a GPU memory fault in round 2 that this check finds without a GPU.
int check_plan(iqhip_engine *e, int nops, int nsentinels) {
    std::unordered_set<const void *> vecs, scs;
    for (const Slab &sl : e->slabs) { vecs.insert(sl.plh.p); scs.insert(sl.sc.p); }
    vecs.insert(e->dummy.plh.p);
    scs.insert(e->dummy.sc.p);
    const size_t per = (e->mfma && e->mfma_pipelined) ? leaf_table_doubles(e) : 0;
    char msg[256];
    auto bad = [&](int k, const char *what) {
        snprintf(msg, sizeof msg, "plan check: op %d of %d (+%d sentinels): %s", k, nops, nsentinels, what);
        return fail(IQHIP_ERR_INVALID, msg);
    };
    auto state_row = [&](const uint8_t *p) {
        if (!p || !e->d_states.p || p < e->d_states.p) return false;
        const size_t off = (size_t)(p - e->d_states.p);
        return off % (size_t)e->nptn_pad == 0 && off / (size_t)e->nptn_pad < (size_t)e->ntaxa;
    };
    auto pair_row = [&](const uint8_t *p) {
        if (!p || !e->d_pair_rows.p || p < e->d_pair_rows.p) return false;
        const size_t off = (size_t)(p - e->d_pair_rows.p);
        return off % (size_t)e->nptn_pad == 0 && off / (size_t)e->nptn_pad < e->pair_row_of.size();
    };
    auto table = [&](const double *p) {
        if (e->plan.nleaf_tabs == 0 && !e->d_leaf_tab.p) return p == nullptr;  // kernel variant without tables
        if (!p || !e->d_leaf_tab.p || p < e->d_leaf_tab.p || per == 0) return false;
        const size_t off = (size_t)(p - e->d_leaf_tab.p);
        return off % per == 0 && off / per < e->d_leaf_tab.cap / per;
    };
    for (int k = 0; k < nops + nsentinels; k++) {
        const DevOp &d = e->h_ops.p[k];
        if (!vecs.count(d.dst) || d.dst == nullptr) return bad(k, "dst is not a vector slab");
        if (!scs.count(d.dst_sc)) return bad(k, "dst_sc is not a counter slab");
        if (!vecs.count(d.pf)) return bad(k, "pf (streamed child) is not a vector slab / the dummy slab");
        if (!scs.count(d.pf_sc)) return bad(k, "pf_sc is not a counter slab / the dummy");
        if (!vecs.count(d.ld)) return bad(k, "ld (second memory child) is not a vector slab / the dummy slab");
        if (!scs.count(d.ld_sc)) return bad(k, "ld_sc is not a counter slab / the dummy");
        // (a pair-code row holds codes 0 .. 24: read as leaf states it would index past a 5-row table)
        const bool pl = k < nops && d.left_kind == CHILD_PAIR, pr = k < nops && d.right_kind == CHILD_PAIR;
        if ((pl || pr) && (e->mfma || e->wide4)) return bad(k, "pair child in a plan of another kernel than k_traverse4");
        if (!(pl ? pair_row(d.sl) : state_row(d.sl)) || !(pr ? pair_row(d.sr) : state_row(d.sr)))
            return bad(k, "sl / sr is not a row of the state matrix (a pair-code row for a pair child, and only for one)");
        if ((pl && !(d.pair_len[0] >= 0.0 && d.pair_len[1] >= 0.0)) || (pr && !(d.pair_len[2] >= 0.0 && d.pair_len[3] >= 0.0)))
            return bad(k, "pair child with a negative or NaN pendant branch length");
        if ((pl != (d.pair_row_l >= 0)) || (pr != (d.pair_row_r >= 0)) || d.pair_row_l >= e->plan.nrows || d.pair_row_r >= e->plan.nrows)
            return bad(k, "pair_row is not the row of a removed op");
        if (!table(d.tabL) || !table(d.tabR)) return bad(k, "tabL / tabR is not a K2 table slot");
        if (d.cherry) {
            const size_t cper = (size_t)e->cherry_npairs * e->block;
            if (!e->d_cherry_tab.p || cper == 0 || d.cherry < e->d_cherry_tab.p || (size_t)(d.cherry - e->d_cherry_tab.p) % cper != 0 ||
                (size_t)(d.cherry - e->d_cherry_tab.p) / cper >= e->d_cherry_tab.cap / cper || k >= nops || d.left_kind != CHILD_LEAF ||
                d.right_kind != CHILD_LEAF)
                return bad(k, "cherry is not a cherry-table slot of an op with two leaf children");
        }
        if (k >= nops) continue;  // sentinels: pointers only
        if (d.dst == e->dummy.plh.p || d.dst_sc == e->dummy.sc.p) return bad(k, "a real op writes the dummy slab");
        const bool lk = d.left_kind == CHILD_LEAF || d.left_kind == CHILD_PAIR || d.left_kind == CHILD_PF || d.left_kind == CHILD_HOLD ||
                        (d.left_kind == CHILD_LOAD && e->mfma && !e->mfma_pipelined);
        const bool rk = d.right_kind == CHILD_LEAF || d.right_kind == CHILD_PAIR || d.right_kind == CHILD_PREV || d.right_kind == CHILD_LOAD;
        if (!lk || !rk) return bad(k, "child kinds are not in canonical form");
        if (d.left_kind == CHILD_PF && (d.pf == e->dummy.plh.p || !(d.real_mask & 1))) return bad(k, "streamed child without a real vector");
        if (d.left_kind != CHILD_PF && !(e->mfma && !e->mfma_pipelined) && (d.real_mask & 1)) return bad(k, "real_mask set without a streamed child");
        if (d.right_kind == CHILD_LOAD && d.ld == e->dummy.plh.p) return bad(k, "second memory child without a real vector");
        if (d.dst == d.pf || d.dst == d.ld) return bad(k, "op writes one of its own children");
        if (!(d.left_len >= 0.0) || !(d.right_len >= 0.0)) return bad(k, "negative or NaN branch length");
        if (d.out_row < 0 || d.out_row >= e->plan.nrows) return bad(k, "out_row outside the caller's op list");
        if (d.lds_left < 0 || d.lds_right < 0 || d.lds_left > e->plan.lds_doubles || d.lds_right > e->plan.lds_doubles)
            return bad(k, "LDS region outside the launch's allocation");
        if (d.sl_slot < 0 || d.sr_slot < 0 || d.sl_slot >= e->plan.state_slots || d.sr_slot >= e->plan.state_slots)
            return bad(k, "leaf-state slot outside the launch's allocation");
        if (d.chunk_nops < 0 || k + d.chunk_nops > nops) return bad(k, "LDS chunk runs past the plan");
        if (e->wide4) {   // k_traverse4w: both children in the memory form, a leaf's region holds its table as well
            if ((d.left_kind != CHILD_LEAF && d.left_kind != CHILD_LOAD) || (d.right_kind != CHILD_LEAF && d.right_kind != CHILD_LOAD))
                return bad(k, "wide 4-state op is not in the (memory, memory) form");
            if ((d.left_kind == CHILD_LOAD && d.pf == e->dummy.plh.p) || (d.right_kind == CHILD_LOAD && d.ld == e->dummy.plh.p))
                return bad(k, "memory child without a real vector");
            const int szl = (d.left_kind == CHILD_LEAF ? 6 : 1) * e->block, szr = (d.right_kind == CHILD_LEAF ? 6 : 1) * e->block;
            if (d.lds_left + szl > e->plan.lds_doubles || d.lds_right + szr > e->plan.lds_doubles ||
                (d.lds_left < d.lds_right + szr && d.lds_right < d.lds_left + szl))
                return bad(k, "LDS regions of the two children overlap or leave the launch's allocation");
            if (d.no_scale < 0 || d.no_scale > 2) return bad(k, "unknown scaling rule");
        }
    }
    // chunks tile the plan; the segment table stays inside it
    for (int k = 0; k < nops;) {
        const DevOp &c = e->h_ops.p[k];
        if (c.chunk_nops <= 0) return bad(k, "op is not covered by an LDS chunk");
        if (!e->mfma) {
            // k_traverse4 requests the state rows of slots 1 .. chunk_slots - 1, four per instruction, from the row pointers
            // the fill stages per slot: the chunk's leaf children own those slots in op order, none twice and none missing,
            // the list fits the kernel's array, and regions plus state bytes fit what the launch allocates
            int next = 1, regs = 0;
            for (int q = k; q < k + c.chunk_nops; q++) {
                const DevOp &d = e->h_ops.p[q];
                if (d.sl_slot != (child_is_table(d.left_kind) ? next : 0)) return bad(q, "leaf-state slots of the chunk are not 1 .. n in op order");
                next += child_is_table(d.left_kind);
                if (d.sr_slot != (child_is_table(d.right_kind) ? next : 0)) return bad(q, "leaf-state slots of the chunk are not 1 .. n in op order");
                next += child_is_table(d.right_kind);
                const int szl = child_region_blocks(d.left_kind) * e->block, szr = child_region_blocks(d.right_kind) * e->block;
                if (d.lds_left < d.lds_right + szr && d.lds_right < d.lds_left + szl) return bad(q, "LDS regions of the two children overlap");
                regs = std::max(regs, std::max(d.lds_left + szl, d.lds_right + szr));
            }
            // the chunk's part of the fill image: 16-byte aligned, inside the image, the same offset on every op of the chunk
            for (int q = k; q < k + c.chunk_nops; q++)
                if (e->h_ops.p[q].image_off != c.image_off) return bad(q, "image_off differs within a chunk");
            if (c.image_off < 0 || c.image_off % 2 != 0 || (int64_t)c.image_off + regs > e->plan.image_doubles)
                return bad(k, "the chunk's fill image is misaligned or outside the image");
            if (c.chunk_slots != next) return bad(k, "chunk_slots is not the chunk's slot count");
            if (next > kTrav4RowSlots) return bad(k, "more leaf-state slots than the kernel's row-pointer list holds");
            if (next > e->plan.state_slots || regs > e->plan.lds_doubles) return bad(k, "LDS chunk outside the launch's allocation");
            if (regs + next * trav4_lds(e->block).slot_doubles > lds_budget(e)) return bad(k, "LDS chunk over the LDS budget");
        }
        k += c.chunk_nops;
    }
    const int *tab = reinterpret_cast<const int *>(e->h_ops.p + e->plan.table_off);
    int covered = 0;
    for (int u = 0; u <= e->plan.nunits; u++) {
        const int b = tab[2 * u], n = tab[2 * u + 1];
        if (b < 0 || n < 0 || b + n > nops) return bad(b, "segment outside the plan");
        covered += n;
    }
    if (covered != nops) return bad(nops, "segments do not cover the plan exactly once");
    return IQHIP_OK;
}

// The descriptors of a repeated plan (model-parameter optimisation re-evaluates the same tree) are already on the
// device: skip the upload, never the computation.
int upload_plan(iqhip_engine *e, size_t nbytes) {
    std::vector<char> &up = e->plan_cache.uploaded;
    const char *h = reinterpret_cast<const char *>(e->h_ops.p);
    if (e->planner) {   // (nothing to upload to; `uploaded` is what d_ops would hold, so that a repeated plan is found cached)
        up.assign(h, h + nbytes);
        return IQHIP_OK;
    }
    if (e->plan.small) {
        // (rides in the kernel arguments, which the launch copies out of h_ops; `uploaded` is what d_ops would hold)
    } else if (up.size() == nbytes && memcmp(up.data(), h, nbytes) == 0) {
        return IQHIP_OK;
    } else if (e->plan_arena_on && e->plan_arena_used + nbytes <= e->h_plan_arena.cap) {
        // a sweep enqueues many plans before the device has run the first: each upload goes out of a slice of its own
        // of a pinned arena, so that re-using h_ops for the next plan never has to wait for the device (that wait -- the
        // staging event below -- made the host fall in step with the device eight times per 97-branch protein sweep)
        char *slice = e->h_plan_arena.p + e->plan_arena_used;
        memcpy(slice, h, nbytes);
        e->plan_arena_used += (nbytes + 255) / 256 * 256;
        HIPCHK(hipMemcpyAsync(e->d_ops.p, slice, nbytes, hipMemcpyHostToDevice, e->stream));
    } else {
        HIPCHK(hipMemcpyAsync(e->d_ops.p, e->h_ops.p, nbytes, hipMemcpyHostToDevice, e->stream));
        HIPCHK(hipEventRecord(e->staging_free, e->stream));
        e->staging_busy = true;
    }
    up.assign(h, h + nbytes);
    return IQHIP_OK;
}

// sentinels, segment table and K2 job list behind the descriptors; the cache key; the small-plan decision; check; upload
// (ops_in: the caller's list, the cache key; nops: the ops that were planned -- select_pair_children may have removed some)
int finish_and_upload(iqhip_engine *e, int nops, const iqhip_node_op *ops_in, int nops_in, Units &u, const std::vector<int> *explicit_segs,
                      const double *const *len_ptrs, int last_dst) {
    Plan &p = e->plan;
    for (int q = 0; q < kSentinels; q++) dummy_op(e, e->h_ops.p[nops + q]);  // targets of the look-ahead requests
    e->h_ops.p[nops].image_off = (int32_t)p.image_doubles;   // (k_traverse4: a chunk's extent is the distance to the next chunk's offset)
    p.table_off = nops + kSentinels;
    const int table_ops = segment_table_ops(u);
    int *tab = reinterpret_cast<int *>(e->h_ops.p + p.table_off);
    memset(tab, 0, sizeof(DevOp) * (size_t)table_ops);
    tab[0] = u.top_begin; tab[1] = nops - u.top_begin;
    for (size_t i = 0; i < u.units.size(); i++) { tab[2 + 2 * i] = u.units[i].first; tab[3 + 2 * i] = u.units[i].second; }
    p.nunits = (int)u.units.size();
    p.stage_units = std::move(u.stage_units);
    p.top_nops = nops - u.top_begin;
    p.jobs_off = p.table_off + table_ops;
    const int jobs_ops = devops_for(sizeof(TabJob) * p.tab_jobs.size());
    if (jobs_ops > 0) {
        memset(e->h_ops.p + p.jobs_off, 0, sizeof(DevOp) * (size_t)jobs_ops);
        memcpy(e->h_ops.p + p.jobs_off, p.tab_jobs.data(), sizeof(TabJob) * p.tab_jobs.size());
    }
    PlanCache &c = e->plan_cache;
    c.ops_in.assign((const char *)ops_in, (const char *)(ops_in + nops_in));
    c.segs = explicit_segs ? *explicit_segs : std::vector<int>();
    c.version = len_ptrs ? 0 : e->keymap_version;  // (slabs created while building are included; a sweep step's plan is never re-used)
    c.dst = last_dst;
    // a small plan rides in the kernel arguments (the launch copies it out of h_ops)
    p.small = e->small_plans && kernel_takes_small_plan(e) && !explicit_segs && u.units.empty() && nops > 0 && nops + kSentinels <= kSmallPlanOps;
    p.small_nops = nops;
    if (e->planner && nops > 0) {   // negative tests (IQHIP_DEBUG_BREAK_PLAN): break one descriptor the way round 2's fault did
        const std::string &br = e->debug_break_plan;
        if (br == "tab") e->h_ops.p[nops - 1].tabL = nullptr;
        else if (br == "sentinel") e->h_ops.p[nops + kSentinels - 1].pf = nullptr;
        else if (br == "states") e->h_ops.p[0].sr = nullptr;
        else if (br == "pair_row") {   // a pair-code row on a child that is read as a leaf
            for (int k = 0; k < nops; k++)
                if (e->h_ops.p[k].left_kind == CHILD_LEAF && !e->pair_row_of.empty()) { e->h_ops.p[k].sl = e->d_pair_rows.p; break; }
        } else if (br == "pair_region") {   // a pair child's region (and the launch's allocation with it) moved past the LDS budget
            for (int k = 0; k < nops; k++)
                if (e->h_ops.p[k].left_kind == CHILD_PAIR) {
                    e->h_ops.p[k].lds_left = lds_budget(e);
                    e->plan.lds_doubles = lds_budget(e) + child_region_blocks(CHILD_PAIR) * e->block;
                    break;
                }
        }
        else if (br == "cherry")
            for (int k = 0; k < nops; k++)
                if (e->h_ops.p[k].cherry) { e->h_ops.p[k].cherry += 8; break; }   // (inside the buffer, not on a table)
    }
    if (e->check_plans) {
        const int rc = check_plan(e, nops, kSentinels);
        if (rc) { c.invalidate(); return rc; }
    }
    return upload_plan(e, sizeof(DevOp) * (size_t)(p.jobs_off + jobs_ops));
}

}  // namespace

namespace iqhip {

// Resolve one child of a node op. prev_dst = slab index written by the previous op (-1: none).
int resolve_child(iqhip_engine *e, uint64_t key, int32_t leaf, int prev_dst, const double **plh, const int16_t **sc,
                  const uint8_t **states, int32_t *kind) {
    *plh = nullptr; *sc = nullptr; *states = nullptr;
    if (leaf >= 0) {
        if (leaf >= e->ntaxa) return fail(IQHIP_ERR_INVALID, "leaf id out of range");
        *states = e->d_states.p + (size_t)leaf * e->nptn_pad;
        *kind = CHILD_LEAF;
        return IQHIP_OK;
    }
    int idx;
    int rc = slab_for_key(e, key, false, &idx);
    if (rc) return rc;
    *plh = e->slabs[idx].plh.p;
    *sc = e->slabs[idx].sc.p;
    *kind = (idx == prev_dst) ? CHILD_PREV : CHILD_LOAD;
    return IQHIP_OK;
}

int build_branch(iqhip_engine *e, iqhip_branch_end a, iqhip_branch_end b, double len, int prev_dst, DevBranch *br) {
    if (!(len >= 0.0)) return fail(IQHIP_ERR_INVALID, "negative or NaN branch length");
    if (a.leaf >= 0 && b.leaf >= 0)
        return fail(IQHIP_ERR_INVALID, "branch with two leaf ends (2-taxon tree) is not supported");
    if (b.leaf >= 0) std::swap(a, b);  // the reference puts the leaf on the `dad` side (:739-746)
    const uint8_t *st_unused;
    int rc = resolve_child(e, a.key, a.leaf, prev_dst, &br->a, &br->a_sc, &br->a_states, &br->a_kind);
    if (rc) return rc;
    rc = resolve_child(e, b.key, b.leaf, prev_dst, &br->b, &br->b_sc, &st_unused, &br->b_kind);
    if (rc) return rc;
    br->len = len;
    return IQHIP_OK;
}

// Policy A (DESIGN.md 3.1 "Fill image"): a plan that was found cached is going to be submitted again -- its image is built
// if it is stale (another model since, or never built) and the launches copy it; a plan that was planned anew fills in the
// kernel and launches nothing.  Never: plans with device-side lengths (not cached, image_ok), plans that travel in the
// kernel arguments, the pair engine's cherry submissions (fill_image.on).
int fill_image_submission(iqhip_engine *e) {
    iqhip_engine::FillImage &f = e->fill_image;
    f.use = false;
    if (e->mfma || !f.on || !f.plan_hit || !e->plan.image_ok || e->plan.small) return IQHIP_OK;
    if (f.model == e->model_version && f.buf.cap >= (size_t)e->plan.image_doubles) {
        f.reused++;
    } else {
        if (f.buf.cap < (size_t)e->plan.image_doubles) HIPCHK(f.buf.ensure(e, (size_t)e->plan.image_doubles + 1024));
        if (!e->planner) HIPCHK(launch_fill4_image(e, e->plan.small_nops));
        f.model = e->model_version;
        f.built++;
    }
    f.use = true;
    return IQHIP_OK;
}

bool leaf_tables_follow_model(iqhip_engine *e) {
    if (e->tab_model_version == e->model_version) return false;
    std::fill(e->tab_len.begin(), e->tab_len.end(), NAN);
    const size_t per = leaf_table_doubles(e);
    for (const TabJob &j : e->plan.tab_jobs) {
        const size_t slot = (size_t)(j.tab - e->d_leaf_tab.p) / per;
        if (slot < (size_t)e->ntaxa) e->tab_len[slot] = j.len;
    }
    e->tab_model_version = e->model_version;
    return true;
}

// Slack in two budgets below: charged to the chunk, allocated by no launch and read by no kernel.  Kept because a
// larger budget would move chunk boundaries (and with them speed).
constexpr int kRows64BudgetSlack = 128;   // on top of rows64_lds(), also in the role maximum of the 64-state pipelined kernels

int lds_budget(const iqhip_engine *e) {
    const int B = e->block, nx = e->state_unknown + 1 - e->n;
    if (!e->mfma) return e->lds_budget_bytes / 8 - trav4_lds(B).s_reg;
    // (a 20-state engine on k_traverse_mfma_mix20, whose fixed part is mix20_lds().sReg = 0, is charged the generic kernel's
    // images all the same: slack as above)
    if (e->wide4) {   // both routes get the same chunks: the larger of the two kernels' fixed parts
        const int kb = e->mfma_lds_kb >= 0 ? e->mfma_lds_kb : kWide4LdsKb;
        return kb * 1024 / 8 - std::max(wide4_lds(e->nclass, B).sReg, generic_lds(4, nx).sReg);
    }
    int fixed = !e->mfma_pipelined ? generic_lds(e->n, nx).sReg
                : e->row_split     ? rows64_lds(nx).sReg + kRows64BudgetSlack
                                   : mfma2_lds(e->n, nx).sReg;
    // (64 states: a launch may mix both roles, k_traverse_mfma_top64)
    if (e->mfma_pipelined && e->n == 64) fixed = std::max(fixed, rows64_lds(nx).sReg + kRows64BudgetSlack);
    // two workgroups per CU (160 KB LDS): <= 78 KB each, images included (a third workgroup for the 20-state kernel was
    // measured: no gain, more chunks); IQHIP_MFMA_LDS_KB overrides
    // (20 states: + 2.6 KB of static arrays per workgroup, the fill's descriptor copies)
    const int total_kb = e->mfma_lds_kb >= 0 ? e->mfma_lds_kb : (e->n == 20 ? 75 : 78);
    if (e->plan.nhold > 0) fixed += mfma2_park_doubles(B);   // the waves' parking places (CHILD_HOLD in LDS)
    int budget = (total_kb * 1024) / 8 - fixed;
    // the generic kernel's images leave two workgroups per CU too little for one op with two vector children once
    // n * ncat > 864 (64 states, 14 .. 16 categories or components): one workgroup per CU, all the dynamic LDS the
    // matrix-core kernels allow
    if (e->mfma_lds_kb < 0 && !e->mfma_pipelined && budget < 2 * B) budget = kTravMaxLdsBytes / 8 - fixed;
    return budget;
}

// Which kernel a launch of `nsegs` segments runs, with its grid and dynamic LDS; reads the engine's shape and switches
// and the current plan, makes no HIP call.
TravLaunch choose_traverse_mfma(const iqhip_engine *e, bool top_stage, int nsegs) {
    const int n = e->n, C = e->ncat, nx = e->state_unknown + 1 - n, regs = e->plan.lds_doubles;
    const int64_t tiles = e->ntiles;
    TravLaunch L = {TRAV_NONE, false, 0, 0, 0, 0, -1};
    int fixed = 0, waves_per_tile = 1;
    if (!e->mfma_pipelined) {   // both children from memory: mixtures, category counts without a pipelined instantiation
        // (20 states: the mixture kernel -- with one class for a plain model: 16+4-row MFMA split, A fragments in
        // registers -- beats the padded generic kernel, which is not instantiated for 20 states)
        if (e->wide4 && !e->wide4_generic) {
            L.variant = TRAV_WIDE4;
            fixed = wide4_lds(e->nclass, e->block).sReg;
        } else if (n == 20) {
            L.variant = e->mix_split ? TRAV_MIX20_SPLIT : TRAV_MIX20;
            waves_per_tile = e->mix_split ? 4 : 1;
            fixed = mix20_lds().sReg;
        } else if (n == 64 || n == 4) {   // (4: mixtures, and wide DNA under IQHIP_WIDE4=generic; a plain model of at most 8 categories never comes here)
            L.variant = TRAV_GENERIC;
            fixed = generic_lds(n, nx).sReg;
        }
    } else if ((n == 20 && (C == 4 || C == 1)) || (n == 64 && C == 1)) {   // plan in canonical (PF, PREV) form
        L.tab = e->plan.nleaf_tabs > 0 || e->leaf_tables;
        L.variant = TRAV_M2;
        fixed = mfma2_lds(n, nx).sReg;
        if (n == 64) {
            // whole rounds of one chain per SIMD go to full-chain workgroups, a small remainder to row-split ones
            const int64_t per_round = (int64_t)e->num_cus * 4, rounds = tiles / per_round, rest = tiles - rounds * per_round;
            if (e->row_split) {
                L.variant = TRAV_ROWS64;
                waves_per_tile = 4;
                fixed = rows64_lds(nx).sReg;
            } else if (top_stage && nsegs == 1 && top_stage_may_mix_roles64(e) && rounds >= 1 && rest > 0 && rest <= per_round / 2) {
                L.variant = TRAV_TOP64;
                L.nfull = (int)(rounds * e->num_cus);
                L.ngroups = (int)(tiles - (int64_t)L.nfull * 4);
                fixed = top64_fixed_doubles(nx);
            }
        } else if (C == 4 && e->cat_split) {
            L.variant = TRAV_M2_CAT_SPLIT;
            waves_per_tile = 4;
        } else if (C == 4 && !L.tab && top_stage && top_stage_may_share_tiles(e)) {
            // whole rounds of two-waves-per-tile workgroups (three per CU); a small remainder as one wave per category
            const int64_t per_round = (int64_t)e->num_cus * 3 * 2, rounds = tiles / per_round, rest = tiles - rounds * per_round;
            L.variant = TRAV_M2_TOP_CS2;
            waves_per_tile = 2;
            if (e->mixed_top && nsegs == 1 && rounds >= 1 && rest > 0 && rest <= per_round / 4) {
                L.variant = TRAV_TOP20;
                L.nfull = (int)(rounds * e->num_cus * 3);
                L.ngroups = (int)(tiles - (int64_t)L.nfull * 2);
            }
        }
    }
    if (L.variant == TRAV_NONE) return L;
    if (L.nfull > 0) L.grid = L.nfull + L.ngroups;
    else {
        L.ngroups = (int)((tiles * waves_per_tile + kTravWg / 64 - 1) / (kTravWg / 64));
        L.grid = L.ngroups * nsegs;
    }
    L.lds_bytes = (size_t)(fixed + regs) * sizeof(double);
    if (L.variant == TRAV_M2 && n < 64 && e->plan.nhold > 0) {   // parking places: one tile vector per wave
        L.hold_off = fixed + regs;
        L.lds_bytes += (size_t)mfma2_park_doubles(e->block) * sizeof(double);
    }
    return L;
}

int build_plan(iqhip_engine *e, const iqhip_node_op *ops, int nops, int *last_dst, const std::vector<int> *explicit_segs,
               const double *const *len_ptrs) {
    if (nops + 2 > e->result_cap) return fail(IQHIP_ERR_INVALID, "too many node updates in one submission");
    e->fill_image.plan_hit = false;
    if (plan_is_cached(e, ops, nops, explicit_segs, len_ptrs)) {
        *last_dst = e->plan_cache.dst;
        mark_virtual_slabs(e);
        e->fill_image.plan_hit = true;
        return IQHIP_OK;
    }
    e->fill_image.model = 0;   // (the image belongs to the plan that is replaced here)
    e->plan_cache.version = 0;
    if (e->staging_busy) {  // the previous submission may still be copying h_ops
        HIPCHK(hipEventSynchronize(e->staging_free));
        e->staging_busy = false;
    }
    e->plan = Plan();
    e->plan.cherry_model = e->model_version;
    e->plan.nrows = nops;
    const iqhip_node_op *const ops_in = ops;
    const int nops_in = nops;
    Kept kept;
    bool removed = false;
    int rc = select_pair_children(e, ops, nops, explicit_segs, len_ptrs, kept, &removed);
    if (rc) return rc;
    if (removed) { ops = kept.ops.data(); nops = (int)kept.ops.size(); }
    Units u;
    rc = cut_units(e, ops, nops, explicit_segs, u);
    // (room for the K2 table job list behind the segment table: at most two leaf children per op)
    if (!rc) rc = ensure_plan_capacity(e, nops + kSentinels + segment_table_ops(u) + devops_for(sizeof(TabJob) * (size_t)(2 * nops + 1)));
    if (!rc) rc = fill_descriptors(e, ops, nops, u, len_ptrs, last_dst, removed ? &kept : nullptr);
    if (!rc) park_operands(e, nops, u.seg_of);
    if (!rc) rc = assign_leaf_tables(e, nops);
    if (!rc) rc = assign_cherry_tables(e, nops, u.seg_of);
    if (!rc) rc = lay_out_lds(e, nops, u.seg_of);
    if (!rc) rc = finish_and_upload(e, nops, ops_in, nops_in, u, explicit_segs, len_ptrs, *last_dst);
    if (!rc) mark_virtual_slabs(e);
    return rc;
}

}  // namespace iqhip
