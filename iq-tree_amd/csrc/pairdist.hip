// pairdist.hip -- drivers of the pairwise ML distances: of one engine (PhyloTree::computeDist; kernels in kernels_dist.hip)
// and, jointly over its members, of a partition group (SuperAlignmentPairwisePlen; kernel in kernels_partdist.hip).  Host
// code only.  Both calls check their arguments, list the pairs, cut them into chunks of tiles and scatter the results with
// the same code.
#include <stdlib.h>
#include <cmath>

#include "partition.h"
#include "partpair_layout.h"

using namespace iqhip;

namespace {

// ---- pairwise ML distances (PhyloTree::computeDist, phylotree.cpp:2432-2541; kernels_dist.hip) -----------------------
// single-device plain engines of 4 / 20 / 64 states with model and alignment; mixtures are refused behind that: a mixture
// without an alignment is an invalid call here, not an unsupported model
int pair_require(iqhip_engine *e, const char *what) {
    int rc = require(e, what, REQ_SINGLE_DEVICE | REQ_PLAIN_STATES | REQ_STATES_4_20_64 | REQ_MODEL_ALN);
    return rc ? rc : require(e, what, REQ_NO_MIXTURE);
}

// the pairs per chunk a caller asks for through the environment, read per call; 0: the call's own bound
int pair_chunk_override() {
    const char *pc = getenv("IQHIP_PAIR_CHUNK");
    return pc ? std::max(1, atoi(pc)) : 0;
}

// pairs per chunk of one engine: the counts of a chunk stay within 64 MB
int64_t pair_chunk(const iqhip_engine *e, int64_t npairs) {
    const int over = pair_chunk_override();
    const int64_t chunk = over ? over : std::max<int64_t>(1, ((int64_t)64 << 20) / (8 * (int64_t)e->n * e->n));
    return std::max<int64_t>(1, std::min(chunk, npairs));
}

// tiles of 4 x 4 taxa for the m pairs of a chunk: pair k goes to slot k.  Pairs of one block of taxa share a tile, whatever
// their order in the list; a pair listed twice opens a new tile
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

// ---- what iqhip_pair_distances and iqhip_partition_pair_distances share ----------------------------------------------------
int pair_check_args(const char *what, const double *dist, double x1, double x2, double xacc, int max_steps) {
    if (!dist) return fail(IQHIP_ERR_INVALID, std::string(what) + ": null argument");
    if (!(x1 >= 0.0) || x1 > x2 || !std::isfinite(x2) || !(xacc > 0.0) || max_steps < 1)
        return fail(IQHIP_ERR_INVALID, std::string(what) + ": bad bounds / tolerance / step count (x1 <= x2, max_steps >= 1)");
    return IQHIP_OK;
}

// the pairs of a call over T taxa in the order it solves them, and per pair its initial distance (empty: none given)
struct PairCall {
    int T;
    int64_t npairs;
    std::vector<int32_t> pairs;
    std::vector<double> init;
};

// lists the pairs, takes their initial distances out of the caller's matrix (checked) and zeroes the caller's results
int pair_call(const char *what, int T, const double *init, double *dist, double *d2l, int32_t *nsteps, PairCall &c) {
    c.T = T;
    c.npairs = (int64_t)T * (T - 1) / 2;
    pair_list(T, c.pairs);
    if (init) {
        c.init.resize((size_t)c.npairs);
        for (int64_t k = 0; k < c.npairs; k++) {
            const double v = init[(size_t)c.pairs[2 * k] * T + c.pairs[2 * k + 1]];
            if (!(v >= 0.0) || !std::isfinite(v)) return fail(IQHIP_ERR_INVALID, std::string(what) + ": an initial distance is negative or not finite");
            c.init[(size_t)k] = v;
        }
    }
    for (size_t k = 0; k < (size_t)T * T; k++) {
        dist[k] = 0.0;
        if (d2l) d2l[k] = 0.0;
        if (nsteps) nsteps[k] = 0;
    }
    return IQHIP_OK;
}

// all tiles of the call up front, chunk by chunk (a chunk's slots start at 0), so that the chunk loop makes no host round
// trip: chunk c's are tiles[tile_first[c] .. tile_first[c + 1])
void pair_chunk_tiles(const PairCall &c, int64_t chunk, std::vector<PairTile> &tiles, std::vector<size_t> &tile_first) {
    for (int64_t first = 0; first < c.npairs; first += chunk) {
        tile_first.push_back(tiles.size());
        pair_tiles(c.pairs.data() + 2 * first, std::min<int64_t>(chunk, c.npairs - first), c.T, tiles);
    }
    tile_first.push_back(tiles.size());
}

// out [npairs][4] = {optx, d2l, evaluations, status} into the caller's symmetric matrices -> the first pair's failure
// (minimizeNewton's two nrerror() exits; the matrices are filled all the same)
int pair_scatter(const PairCall &c, const double *out, double *dist, double *d2l, int32_t *nsteps) {
    const size_t T = (size_t)c.T;
    int worst = 0;
    for (int64_t k = 0; k < c.npairs; k++) {
        const size_t ij = (size_t)c.pairs[2 * k] * T + c.pairs[2 * k + 1], ji = (size_t)c.pairs[2 * k + 1] * T + c.pairs[2 * k];
        const NewtonResult r(out + 4 * k);
        dist[ij] = dist[ji] = r.optx;
        if (d2l) d2l[ij] = d2l[ji] = r.d2l;
        if (nsteps) nsteps[ij] = nsteps[ji] = r.nsteps;
        if (r.status && !worst) worst = r.status;
    }
    return newton_status(worst);
}

}  // namespace

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
    const char *what = "iqhip_pair_distances";
    int rc = pair_require(e, what);
    if (rc) return rc;
    if ((rc = pair_check_args(what, dist, x1, x2, xacc, max_steps))) return rc;
    PairCall c;
    if ((rc = pair_call(what, e->ntaxa, init, dist, d2l, nsteps, c))) return rc;
    const int64_t npairs = c.npairs;
    if (npairs == 0) return IQHIP_OK;
    HIPCHK(use_device(e));
    const int n = e->n;
    const size_t nn = (size_t)n * n, n3 = nn * n;
    const int64_t chunk = pair_chunk(e, npairs);
    std::vector<PairTile> tiles;
    std::vector<size_t> tile_first;
    pair_chunk_tiles(c, chunk, tiles, tile_first);
    HIPCHK(e->pd.tiles.ensure(e, tiles.size()));
    HIPCHK(e->pd.counts.ensure(e, (size_t)chunk * nn));
    HIPCHK(e->pd.coef.ensure(e, n3));
    HIPCHK(e->pd.init.ensure(e, (size_t)npairs));
    HIPCHK(e->pd.out.ensure(e, (size_t)4 * npairs));
    HIPCHK(hipStreamSynchronize(e->stream));
    HIPCHK(hipMemcpyAsync(e->pd.tiles.p, tiles.data(), sizeof(PairTile) * tiles.size(), hipMemcpyHostToDevice, e->stream));
    if (init) HIPCHK(hipMemcpyAsync(e->pd.init.p, c.init.data(), sizeof(double) * c.init.size(), hipMemcpyHostToDevice, e->stream));
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
    for (size_t k = 0; first < npairs; k++, first += chunk) {
        const int m = (int)std::min<int64_t>(chunk, npairs - first);
        a.first_pair = first;
        timer.mark();
        HIPCHK(launch_pair_counts(e, e->pd.tiles.p + tile_first[k], (int)(tile_first[k + 1] - tile_first[k]), e->pd.counts.p));
        timer.mark();
        HIPCHK(launch_pair_solve(e, a, m));
        timer.mark();
    }
    std::vector<double> out((size_t)4 * npairs);
    HIPCHK(hipMemcpyAsync(out.data(), e->pd.out.p, sizeof(double) * out.size(), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    timer.read(e->pd.ms);
    return pair_scatter(c, out.data(), dist, d2l, nsteps);
}

extern "C" int iqhip_debug_pair_timing(iqhip_engine *e, double *counts_ms, double *solve_ms) {
    if (!e || !e->shards.empty()) return fail(IQHIP_ERR_INVALID, "iqhip_debug_pair_timing: needs a single-device engine");
    if (counts_ms) *counts_ms = e->pd.ms[0];
    if (solve_ms) *solve_ms = e->pd.ms[1];
    return IQHIP_OK;
}

// ---- joint pairwise distances (include/iqhip.h, "Joint pairwise distances of a partition group") ------------------------------
// Per chunk of pairs: every member's launch_pair_counts on its own stream into its own pd.counts, then ONE k_partpair_solve
// on the group's stream behind the members' events, then the members wait for the group (the next chunk's counts overwrite
// what the solve read; the stream rule of partition.h, chunk by chunk).  P + 1 launches per chunk, P more per call for the
// members' coefficient tables; no host round trip.
extern "C" int iqhip_partition_pair_distances(iqhip_partition *g, const double *init, double x1, double x2, double xacc,
                                              int max_steps, double *dist, double *d2l, int32_t *nsteps) {
    const char *what = "iqhip_partition_pair_distances";
    if (!g) return fail(IQHIP_ERR_INVALID, std::string(what) + ": null group");
    int rc = pair_check_args(what, dist, x1, x2, xacc, max_steps);
    if (rc) return rc;
    if ((rc = use_group(g, what))) return rc;
    const int P = g->nparts, T = g->m[0]->ntaxa;
    std::vector<int> nstates;
    int e_doubles = 0, max_n = 0;
    for (int p = 0; p < P; p++) {
        iqhip_engine *e = g->m[p];
        if ((rc = pair_require(e, what))) return rc;
        if (e->ntaxa != T)
            return fail(IQHIP_ERR_INVALID, std::string(what) + ": member " + std::to_string(p) + " has another number of taxa than member 0");
        nstates.push_back(e->n);
        e_doubles = std::max(e_doubles, e->n * e->ncat);
        max_n = std::max(max_n, e->n);
    }
    if (partpair_solve_lds_bytes(e_doubles, max_n) > kPartMaxLdsBytes)
        return fail(IQHIP_ERR_UNSUPPORTED, std::string(what) + ": nstates * ncat of a member exceeds the solve's LDS");
    PairCall c;
    if ((rc = pair_call(what, T, init, dist, d2l, nsteps, c))) return rc;
    const int64_t npairs = c.npairs;
    g->pdist.ms[0] = g->pdist.ms[1] = 0.0;
    g->launches = 0;
    if (npairs == 0) return IQHIP_OK;
    // pairs per chunk: all members' counts of a chunk together within 64 MB
    const PartPairLayout lay = partpair_layout(nstates.data(), P, npairs, pair_chunk_override());
    const int64_t chunk = lay.chunk;
    const size_t sum_nn = lay.sum_nn;
    std::vector<PairTile> tiles;   // (the same list serves every member)
    std::vector<size_t> tile_first;
    pair_chunk_tiles(c, chunk, tiles, tile_first);
    HIPCHK(g->pdist.desc.ensure(g->stream, (size_t)P));
    HIPCHK(g->pdist.cells.ensure(g->stream, (size_t)chunk * sum_nn));
    HIPCHK(g->pdist.nnz.ensure(g->stream, (size_t)chunk * P));
    HIPCHK(g->pdist.init.ensure(g->stream, (size_t)npairs));
    HIPCHK(g->pdist.out.ensure(g->stream, (size_t)4 * npairs));
    // every buffer first: up to here nothing is enqueued, and a failure returns at once
    for (int p = 0; p < P; p++) {
        iqhip_engine *e = g->m[p];
        const size_t nn = (size_t)e->n * e->n;
        HIPCHK(e->pd.tiles.ensure(e, tiles.size()));
        HIPCHK(e->pd.counts.ensure(e, (size_t)chunk * nn));
        HIPCHK(e->pd.coef.ensure(e, nn * e->n));
        HIPCHK(hipStreamSynchronize(e->stream));
    }
    // From the first copy on `tiles` and `c.init` (pageable) are sources of enqueued copies: whatever fails below, the call
    // leaves through the drain at its end, never straight out
    const auto enqueue_setup = [&]() -> int {
        for (int p = 0; p < P; p++) {
            iqhip_engine *e = g->m[p];
            HIPCHK(hipMemcpyAsync(e->pd.tiles.p, tiles.data(), sizeof(PairTile) * tiles.size(), hipMemcpyHostToDevice, e->stream));
            HIPCHK(launch_pair_coef(e, e->pd.coef.p));
            PartPairDesc &D = g->pdist.desc.h.p[p];
            D.counts = e->pd.counts.p;
            D.coef = e->pd.coef.p;
            D.eval = e->d_eval;
            D.rates = e->d_rates;
            D.props = e->d_props;
            D.cells = g->pdist.cells.p + lay.cell_first[(size_t)p];
            D.n = e->n;
            D.ncat = e->ncat;
            D.rate = g->rate[p];
        }
        g->launches += P;
        HIPCHK(hipSetDevice(g->device));
        HIPCHK(hipMemcpyAsync(g->pdist.desc.d.p, g->pdist.desc.h.p, sizeof(PartPairDesc) * (size_t)P, hipMemcpyHostToDevice, g->stream));
        if (init) HIPCHK(hipMemcpyAsync(g->pdist.init.p, c.init.data(), sizeof(double) * c.init.size(), hipMemcpyHostToDevice, g->stream));
        return IQHIP_OK;
    };
    rc = enqueue_setup();
    PartPairArgs a;
    a.desc = g->pdist.desc.d.p;
    a.nnz = g->pdist.nnz.p;
    a.init = init ? g->pdist.init.p : nullptr;
    a.out = g->pdist.out.p;
    a.nparts = P;
    a.max_steps = max_steps;
    a.e_doubles = e_doubles;
    a.max_n = max_n;
    a.x1 = x1;
    a.x2 = x2;
    a.xacc = xacc;
    const bool timing = g->m[0]->timing;
    PhaseTimer t_counts(timing, g->stream, 1), t_solve(timing, g->stream, 1);
    hipError_t s = hipSuccess;
    int64_t first = 0;
    for (size_t k = 0; first < npairs && s == hipSuccess && rc == IQHIP_OK; k++, first += chunk) {
        const int m = (int)std::min<int64_t>(chunk, npairs - first);
        a.first_pair = first;
        // (a member's stream waits for the solve of the chunk before: its counts are not overwritten under it)
        for (int p = 0; p < P && s == hipSuccess; p++) {
            iqhip_engine *e = g->m[p];
            t_counts.mark(e->stream);
            s = launch_pair_counts(e, e->pd.tiles.p + tile_first[k], (int)(tile_first[k + 1] - tile_first[k]), e->pd.counts.p);
            t_counts.mark(e->stream);
        }
        if (s != hipSuccess || (rc = wait_for_members(g))) break;
        t_solve.mark();
        s = launch_partpair_solve(g->stream, a, m);
        t_solve.mark();
        const int rc2 = members_wait(g);
        if (!rc) rc = rc2;
        g->launches += P + 1;
    }
    std::vector<double> out((size_t)4 * npairs);
    if (s == hipSuccess && rc == IQHIP_OK)
        s = hipMemcpyAsync(out.data(), g->pdist.out.p, sizeof(double) * out.size(), hipMemcpyDeviceToHost, g->stream);
    // (whatever happened: the host waits for everything enqueued, the members' streams included; the staging is free again)
    hipError_t drained = hipStreamSynchronize(g->stream);
    for (int p = 0; p < P; p++) {
        const hipError_t d = hipStreamSynchronize(g->m[p]->stream);
        if (drained == hipSuccess) drained = d;
    }
    if (rc) return rc;
    HIPCHK(s);
    HIPCHK(drained);
    t_counts.read(&g->pdist.ms[0]);
    t_solve.read(&g->pdist.ms[1]);
    return pair_scatter(c, out.data(), dist, d2l, nsteps);
}

extern "C" int iqhip_debug_partition_pair_timing(iqhip_partition *g, double *counts_ms, double *solve_ms) {
    if (!g) return fail(IQHIP_ERR_INVALID, "iqhip_debug_partition_pair_timing: null group");
    if (counts_ms) *counts_ms = g->pdist.ms[0];
    if (solve_ms) *solve_ms = g->pdist.ms[1];
    return IQHIP_OK;
}
