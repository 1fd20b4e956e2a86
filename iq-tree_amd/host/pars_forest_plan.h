// pars_forest_plan.h -- the arithmetic of a parsimony forest that needs no tree and no engine: which arena slots a member
// owns, how many members fit one arena, and how the members' branch lists become the segments of ONE
// iqhip_pars_insert_scores_batch.  Plain C++ (tools/asan_pars_forest.sh runs it under ASan + UBSan).
#pragma once
#include <stdint.h>

#include <stdexcept>
#include <string>
#include <vector>

namespace iqforest {

// A stepwise-addition tree of T taxa has 3 T - 6 directed vectors that are not a tip's: 3 around the first centre, 3 more
// per inserted taxon.  The tips are slots 0 .. T-1 and are shared by every member.
inline int memberVectors(int ntaxa) { return ntaxa >= 3 ? 3 * ntaxa - 6 : 0; }
inline int slotBase(int ntaxa, int k) { return ntaxa + k * memberVectors(ntaxa); }
inline int64_t arenaVectors(int ntaxa, int members) { return (int64_t)members * memberVectors(ntaxa); }

// The bytes of device memory one member's vectors take: per vector nwords * (nstates planes + 1 score column) words.
inline int64_t memberBytes(int ntaxa, int nstates, int64_t nsites) {
    const int64_t nwords = nsites > 0 ? (nsites + 31) / 32 : 1;
    return (int64_t)memberVectors(ntaxa) * nwords * (nstates + 1) * 4;
}

// The default budget of one arena: 1 GiB of the device's 288 GB.  100 DNA trees of 50 taxa x 100 k sites take 0.9 GB and
// so stay one chunk; larger forests are built in several chunks, which changes no result.
constexpr int64_t kForestArenaBudget = (int64_t)1 << 30;

// members per chunk: as many as the budget holds, at least 1, at most K and at most what keeps every slot an int32;
// forced > 0 (IQHIP_PARS_FOREST_CHUNK) replaces the budget
inline int chunkMembers(int K, int ntaxa, int nstates, int64_t nsites, int forced, int64_t budget = kForestArenaBudget) {
    if (K < 1) return 0;
    const int64_t per = memberBytes(ntaxa, nstates, nsites);
    int64_t m = forced > 0 ? forced : (per > 0 ? budget / per : K);
    const int64_t slot_cap = memberVectors(ntaxa) > 0 ? ((int64_t)2147483647 - ntaxa) / memberVectors(ntaxa) : K;
    if (m > slot_cap) m = slot_cap;
    if (m < 1) m = 1;
    if (m > K) m = K;
    return (int)m;
}

// IQHIP_PARS_FOREST_CHUNK: unset or empty -> 0 (the budget decides); a positive integer; anything else is refused
inline int parseChunk(const char *text) {
    if (!text || !*text) return 0;
    long v = 0;
    for (const char *c = text; *c; c++) {
        if (*c < '0' || *c > '9' || v > 100000000) throw std::runtime_error(std::string("IQHIP_PARS_FOREST_CHUNK must be a positive integer, not '") + text + "'");
        v = v * 10 + (*c - '0');
    }
    if (v < 1) throw std::runtime_error(std::string("IQHIP_PARS_FOREST_CHUNK must be a positive integer, not '") + text + "'");
    return (int)v;
}

// The members' branch-end lists one after the other, with where each begins: the arguments of the batch scan.
struct Segments {
    std::vector<int32_t> ends, seg_start, taxon;
    void clear() {
        ends.clear();
        seg_start.assign(1, 0);
        taxon.clear();
    }
    // member_ends: 2 slots per branch; an empty list is refused (the scan has no empty segments)
    void add(const std::vector<int32_t> &member_ends, int32_t tip) {
        if (member_ends.empty() || member_ends.size() % 2) throw std::runtime_error("forest: a member without branches");
        if (seg_start.empty()) seg_start.assign(1, 0);
        ends.insert(ends.end(), member_ends.begin(), member_ends.end());
        seg_start.push_back((int32_t)(ends.size() / 2));
        taxon.push_back(tip);
    }
    int nseg() const { return (int)taxon.size(); }
};

}  // namespace iqforest
