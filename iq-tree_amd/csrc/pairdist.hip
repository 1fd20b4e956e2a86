// pairdist.hip -- driver of the pairwise ML distances (PhyloTree::computeDist).  Host code only; the kernels are in
// kernels_dist.hip.
#include <stdlib.h>
#include <cmath>

#include "iqhip_internal.h"

using namespace iqhip;

// ---- pairwise ML distances (PhyloTree::computeDist, phylotree.cpp:2432-2541; kernels_dist.hip) -----------------------
// single-device plain engines of 4 / 20 / 64 states with model and alignment; mixtures are refused behind that: a mixture
// without an alignment is an invalid call here, not an unsupported model
namespace iqhip {
int pair_require(iqhip_engine *e, const char *what) {
    int rc = require(e, what, REQ_SINGLE_DEVICE | REQ_PLAIN_STATES | REQ_STATES_4_20_64 | REQ_MODEL_ALN);
    return rc ? rc : require(e, what, REQ_NO_MIXTURE);
}
}  // namespace iqhip

// pairs per chunk: the counts of a chunk stay within 64 MB; IQHIP_PAIR_CHUNK (read per call) overrides
static int64_t pair_chunk(const iqhip_engine *e, int64_t npairs) {
    int64_t chunk = std::max<int64_t>(1, ((int64_t)64 << 20) / (8 * (int64_t)e->n * e->n));
    if (const char *pc = getenv("IQHIP_PAIR_CHUNK")) chunk = std::max(1, atoi(pc));
    return std::max<int64_t>(1, std::min(chunk, npairs));
}

// tiles of 4 x 4 taxa for the m pairs of a chunk: pair k goes to slot k.  Pairs of one block of taxa share a tile, whatever
// their order in the list; a pair listed twice opens a new tile
namespace iqhip {
void pair_tiles(const int32_t *pairs, int64_t m, int ntaxa, std::vector<PairTile> &tiles) {
    std::unordered_map<uint64_t, size_t> open;
    for (int64_t k = 0; k < m; k++) {
        const int i = pairs[2 * k], j = pairs[2 * k + 1];
        const uint64_t key = ((uint64_t)(i >> 2) << 32) | (uint64_t)(j >> 2);
        const int cell = (i & 3) * 4 + (j & 3);
        auto it = open.find(key);
        if (it == open.end() || tiles[it->second].out[cell] >= 0) {
            PairTile t;
            for (int x = 0; x < 4; x++) {
                t.ra[x] = std::min((i & ~3) + x, ntaxa - 1);
                t.rb[x] = std::min((j & ~3) + x, ntaxa - 1);
            }
            for (int c = 0; c < 16; c++) t.out[c] = -1;
            open[key] = tiles.size();
            tiles.push_back(t);
            it = open.find(key);
        }
        tiles[it->second].out[cell] = (int32_t)k;
    }
}

// the pairs i < j block by block of 4 x 4 taxa, so that the pairs of a tile are neighbours in the list (and in a chunk)
void pair_list(int T, std::vector<int32_t> &pairs) {
    pairs.clear();
    pairs.reserve((size_t)T * (T - 1));
    for (int I = 0; I < T; I += 4)
        for (int J = I; J < T; J += 4)
            for (int i = I; i < std::min(I + 4, T); i++)
                for (int j = std::max(J, i + 1); j < std::min(J + 4, T); j++) {
                    pairs.push_back(i);
                    pairs.push_back(j);
                }
}
}  // namespace iqhip

extern "C" int iqhip_pair_counts(iqhip_engine *e, const int32_t *pairs, int npairs, double *counts) {
    int rc = pair_require(e, "iqhip_pair_counts");
    if (rc) return rc;
    if (!pairs || !counts || npairs < 0) return fail(IQHIP_ERR_INVALID, "iqhip_pair_counts: bad pair list");
    for (int64_t k = 0; k < 2 * (int64_t)npairs; k++)
        if (pairs[k] < 0 || pairs[k] >= e->ntaxa) return fail(IQHIP_ERR_INVALID, "iqhip_pair_counts: pair index outside [0, ntaxa)");
    HIPCHK(use_device(e));
    const size_t nn = (size_t)e->n * e->n;
    const int64_t chunk = pair_chunk(e, npairs);
    for (int64_t first = 0; first < npairs; first += chunk) {
        const int64_t m = std::min<int64_t>(chunk, npairs - first);
        std::vector<PairTile> tiles;
        pair_tiles(pairs + 2 * first, m, e->ntaxa, tiles);
        HIPCHK(e->pd.tiles.ensure(e, tiles.size()));
        HIPCHK(e->pd.counts.ensure(e, (size_t)m * nn));
        HIPCHK(hipStreamSynchronize(e->stream));   // (pageable source: the copy must not outlive `tiles`)
        HIPCHK(hipMemcpyAsync(e->pd.tiles.p, tiles.data(), sizeof(PairTile) * tiles.size(), hipMemcpyHostToDevice, e->stream));
        HIPCHK(launch_pair_counts(e, e->pd.tiles.p, (int)tiles.size(), e->pd.counts.p));
        HIPCHK(hipMemcpyAsync(counts + (size_t)first * nn, e->pd.counts.p, sizeof(double) * (size_t)m * nn, hipMemcpyDeviceToHost,
                              e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
    }
    return IQHIP_OK;
}

extern "C" int iqhip_pair_distances(iqhip_engine *e, const double *init, double x1, double x2, double xacc, int max_steps,
                                    double *dist, double *d2l, int32_t *nsteps) {
    int rc = pair_require(e, "iqhip_pair_distances");
    if (rc) return rc;
    if (!dist) return fail(IQHIP_ERR_INVALID, "iqhip_pair_distances: null argument");
    if (!(x1 >= 0.0) || x1 > x2 || !std::isfinite(x2) || !(xacc > 0.0) || max_steps < 1)
        return fail(IQHIP_ERR_INVALID, "iqhip_pair_distances: bad bounds / tolerance / step count (x1 <= x2, max_steps >= 1)");
    const int T = e->ntaxa, n = e->n;
    const int64_t npairs = (int64_t)T * (T - 1) / 2;
    std::vector<int32_t> pairs;
    pair_list(T, pairs);
    std::vector<double> h_init;
    if (init) {
        h_init.resize((size_t)npairs);
        for (int64_t k = 0; k < npairs; k++) {
            const double v = init[(size_t)pairs[2 * k] * T + pairs[2 * k + 1]];
            if (!(v >= 0.0) || !std::isfinite(v)) return fail(IQHIP_ERR_INVALID, "iqhip_pair_distances: an initial distance is negative or not finite");
            h_init[(size_t)k] = v;
        }
    }
    for (size_t k = 0; k < (size_t)T * T; k++) {
        dist[k] = 0.0;
        if (d2l) d2l[k] = 0.0;
        if (nsteps) nsteps[k] = 0;
    }
    if (npairs == 0) return IQHIP_OK;
    HIPCHK(use_device(e));
    const size_t nn = (size_t)n * n, n3 = nn * n;
    const int64_t chunk = pair_chunk(e, npairs);
    // all tiles up front, chunk by chunk (a chunk's slots start at 0): the chunk loop below makes no host round trip
    std::vector<PairTile> tiles;
    std::vector<size_t> tile_first;
    for (int64_t first = 0; first < npairs; first += chunk) {
        tile_first.push_back(tiles.size());
        pair_tiles(pairs.data() + 2 * first, std::min<int64_t>(chunk, npairs - first), T, tiles);
    }
    tile_first.push_back(tiles.size());
    HIPCHK(e->pd.tiles.ensure(e, tiles.size()));
    HIPCHK(e->pd.counts.ensure(e, (size_t)chunk * nn));
    HIPCHK(e->pd.coef.ensure(e, n3));
    HIPCHK(e->pd.init.ensure(e, (size_t)npairs));
    HIPCHK(e->pd.out.ensure(e, (size_t)4 * npairs));
    HIPCHK(hipStreamSynchronize(e->stream));
    HIPCHK(hipMemcpyAsync(e->pd.tiles.p, tiles.data(), sizeof(PairTile) * tiles.size(), hipMemcpyHostToDevice, e->stream));
    if (init) HIPCHK(hipMemcpyAsync(e->pd.init.p, h_init.data(), sizeof(double) * h_init.size(), hipMemcpyHostToDevice, e->stream));
    HIPCHK(launch_pair_coef(e, e->pd.coef.p));
    PairSolveArgs a;
    a.counts = e->pd.counts.p;
    a.coef = e->pd.coef.p;
    a.eval = e->d_eval;
    a.rates = e->d_rates;
    a.props = e->d_props;
    a.init = init ? e->pd.init.p : nullptr;
    a.out = e->pd.out.p;
    a.n = n;
    a.ncat = e->ncat;
    a.max_steps = max_steps;
    a.x1 = x1;
    a.x2 = x2;
    a.xacc = xacc;
    // iqhip_timing_enable: device time of the count and the solve launches, summed over the chunks
    PhaseTimer timer(e, 2);
    e->pd.ms[0] = e->pd.ms[1] = 0.0;
    int64_t first = 0;
    for (size_t c = 0; first < npairs; c++, first += chunk) {
        const int m = (int)std::min<int64_t>(chunk, npairs - first);
        a.first_pair = first;
        timer.mark();
        HIPCHK(launch_pair_counts(e, e->pd.tiles.p + tile_first[c], (int)(tile_first[c + 1] - tile_first[c]), e->pd.counts.p));
        timer.mark();
        HIPCHK(launch_pair_solve(e, a, m));
        timer.mark();
    }
    std::vector<double> out((size_t)4 * npairs);
    HIPCHK(hipMemcpyAsync(out.data(), e->pd.out.p, sizeof(double) * out.size(), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    timer.read(e->pd.ms);
    int worst = 0;
    for (int64_t k = 0; k < npairs; k++) {
        const size_t ij = (size_t)pairs[2 * k] * T + pairs[2 * k + 1], ji = (size_t)pairs[2 * k + 1] * T + pairs[2 * k];
        const NewtonResult r(out.data() + 4 * k);
        dist[ij] = dist[ji] = r.optx;
        if (d2l) d2l[ij] = d2l[ji] = r.d2l;
        if (nsteps) nsteps[ij] = nsteps[ji] = r.nsteps;
        if (r.status && !worst) worst = r.status;
    }
    return newton_status(worst);   // (minimizeNewton's two nrerror() exits; the matrices are filled all the same)
}

extern "C" int iqhip_debug_pair_timing(iqhip_engine *e, double *counts_ms, double *solve_ms) {
    if (!e || !e->shards.empty()) return fail(IQHIP_ERR_INVALID, "iqhip_debug_pair_timing: needs a single-device engine");
    if (counts_ms) *counts_ms = e->pd.ms[0];
    if (solve_ms) *solve_ms = e->pd.ms[1];
    return IQHIP_OK;
}
