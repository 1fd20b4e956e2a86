// lmap_host.h -- the host side of likelihood mapping (-lmap; quartet.cpp of the reference): what is done with the three
// log-likelihoods of a quartet, and which quartets are evaluated.  Plain C++, no device call; the likelihoods themselves come
// from iqhip_quartet_likelihoods (PhyloTree::computeQuartetLikelihoods in phylo_dist.cpp).
//   order3        the descending order of three values with the reference's ties (quartet.cpp:974-1005; the same comparison
//                 tree sorts the three squared distances, :1070-1100)
//   weights       the Bayesian weights exp(l_k - l_max) / sum with TP_MAX_EXP_DIFF = 40 (:1007-1031)
//   region        the corner 0..2 of the best tree (:1033-1042) and the region 0..6 of the triangle (:1044-1128): the weights
//                 are compared with (1,0,0), (1/2,1/2,0) and (1/3,1/3,1/3) placed on the best, the two best, all three
//                 trees; the nearest of the three decides, its trees as bits 1, 2, 4: 1,2,4 -> regions 0,1,2 (resolved),
//                 3,6,5 -> regions 3,4,5 (partly resolved), 7 -> region 6 (unresolved)
//   allQuartets   every unique quartet i0 < i1 < i2 < i3 in nested-loop order (:771-782, one group), C(n,4) of them
//   drawQuartets  `count` random quartets: four distinct taxa drawn one after the other, each redrawn while it repeats an
//                 earlier one (:847-887, one group); the order drawn is kept, never sorted.
// DEVIATION from the reference: the draws do not follow its random stream.  They come from the mirror's counter-based
//   generator (include/iqhip.h, iqhip_gen_boot_samples: z = mix(mix(mix(seed + G (stream + 1)) + G (rho + 1)) + G (j + 1)))
//   with stream 0xCC, rho = the quartet's number and j = the number of the draw inside the quartet, taxon = floor(u n) for
//   u = (z >> 11) 2^-53: quartet q of a seed is the same whatever count is asked for.
#pragma once

#include <math.h>
#include <stdint.h>

#include <stdexcept>
#include <vector>

namespace iqhost {
namespace lmap {

constexpr double TP_MAX_EXP_DIFF = 40.0;
constexpr uint64_t kDrawStream = 0xCC;

struct QuartetInfo {   // quartet.h QuartetInfo
    int32_t seqID[4];
    double logl[3];
    double qweight[3];
    int corner, area;
};

inline void order3(const double v[3], int o[3]) {
    if (v[0] > v[1]) {
        if (v[2] > v[0]) { o[0] = 2; o[1] = 0; o[2] = 1; }
        else if (v[2] < v[1]) { o[0] = 0; o[1] = 1; o[2] = 2; }
        else { o[0] = 0; o[1] = 2; o[2] = 1; }
    } else {
        if (v[2] > v[1]) { o[0] = 2; o[1] = 1; o[2] = 0; }
        else if (v[2] < v[0]) { o[0] = 1; o[1] = 0; o[2] = 2; }
        else { o[0] = 1; o[1] = 2; o[2] = 0; }
    }
}

inline void weights(const double logl[3], double w[3], int order[3]) {
    order3(logl, order);
    for (int k = 1; k < 3; k++) {
        const double d = logl[order[k]] - logl[order[0]];
        w[order[k]] = d < -TP_MAX_EXP_DIFF ? 0.0 : exp(d);
    }
    w[order[0]] = 1.0;
    const double sum = w[0] + w[1] + w[2];
    for (int k = 0; k < 3; k++) w[k] = w[k] / sum;
}

inline void region(const double logl[3], double w[3], int *corner, int *area) {
    int o[3];
    weights(logl, w, o);
    static const int bits[3] = {1, 2, 4};
    *corner = o[0];   // (the best tree's bit 1, 2, 4 -> corner 0, 1, 2)
    const double third = 1.0 / 3.0;
    double sq[3], t1, t2, t3;
    int disc[3];
    t1 = 1.0 - w[o[0]];
    sq[0] = t1 * t1 + w[o[1]] * w[o[1]] + w[o[2]] * w[o[2]];
    disc[0] = bits[o[0]];
    t1 = 0.5 - w[o[0]];
    t2 = 0.5 - w[o[1]];
    sq[1] = t1 * t1 + t2 * t2 + w[o[2]] * w[o[2]];
    disc[1] = bits[o[0]] + bits[o[1]];
    t1 = third - w[o[0]];
    t2 = third - w[o[1]];
    t3 = third - w[o[2]];
    sq[2] = t1 * t1 + t2 * t2 + t3 * t3;
    disc[2] = 7;
    int so[3];
    order3(sq, so);
    static const int area_of[8] = {-1, 0, 1, 3, 2, 5, 4, 6};   // by the bits of the nearest distribution
    *area = area_of[disc[so[2]]];
}

inline int64_t numQuartets(int64_t n) { return n < 4 ? 0 : n * (n - 1) / 2 * (n - 2) / 3 * (n - 3) / 4; }

inline void allQuartets(int n, std::vector<int32_t> &out) {
    out.clear();
    for (int i0 = 0; i0 < n - 3; i0++)
        for (int i1 = i0 + 1; i1 < n - 2; i1++)
            for (int i2 = i1 + 1; i2 < n - 1; i2++)
                for (int i3 = i2 + 1; i3 < n; i3++) {
                    out.push_back(i0);
                    out.push_back(i1);
                    out.push_back(i2);
                    out.push_back(i3);
                }
}

inline uint64_t mix64(uint64_t z) {
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27; z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}

inline void drawQuartets(int n, int64_t count, uint64_t seed, std::vector<int32_t> &out) {
    if (n < 4) throw std::runtime_error("likelihood mapping needs at least 4 taxa");
    if (count < 0) throw std::runtime_error("drawQuartets: negative count");
    const uint64_t G = 0x9E3779B97F4A7C15ull;
    const uint64_t base = mix64(seed + G * (kDrawStream + 1));
    out.assign((size_t)4 * (size_t)count, 0);
    for (int64_t q = 0; q < count; q++) {
        const uint64_t qbase = mix64(base + G * ((uint64_t)q + 1));
        uint64_t j = 0;
        int32_t *t = out.data() + 4 * q;
        for (int k = 0; k < 4; k++) {
            bool again = true;
            while (again) {
                const uint64_t z = mix64(qbase + G * (++j));
                int v = (int)((double)(z >> 11) * 0x1.0p-53 * n);
                if (v >= n) v = n - 1;
                t[k] = v;
                again = false;
                for (int i = 0; i < k; i++) again = again || t[i] == v;
            }
        }
    }
}

}  // namespace lmap
}  // namespace iqhost
