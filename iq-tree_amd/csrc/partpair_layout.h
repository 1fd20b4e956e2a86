// partpair_layout.h -- how a call of iqhip_partition_pair_distances (pairdist.hip) cuts its pairs into chunks and lays the
// members' cell lists out.  Plain C++ without a device, so that tools/asan_partition_dist.sh runs it under ASan + UBSan as a
// stand-alone program.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace iqhip {

// One call's chunks.  A pair needs n_p^2 counts (8 bytes) and n_p^2 cell slots (2 bytes) of member p; the counts of a chunk,
// all members together, stay within 64 MB.  chunk_override > 0 (pairdist.hip pair_chunk_override) takes its place.  Member p's block of the
// group's cell buffer [chunk * sum_nn] starts at element cell_first[p] = chunk * sum_{q < p} n_q^2 and holds chunk * n_p^2
struct PartPairLayout {
    int64_t chunk = 1;                // pairs per chunk, 1 <= chunk <= max(1, npairs)
    size_t sum_nn = 0;                // sum_p n_p^2
    std::vector<size_t> cell_first;   // [nparts]
};

inline PartPairLayout partpair_layout(const int *nstates, int nparts, int64_t npairs, int64_t chunk_override) {
    PartPairLayout L;
    for (int p = 0; p < nparts; p++) L.sum_nn += (size_t)nstates[p] * (size_t)nstates[p];
    L.chunk = std::max<int64_t>(1, ((int64_t)64 << 20) / (8 * (int64_t)std::max<size_t>(1, L.sum_nn)));
    if (chunk_override > 0) L.chunk = chunk_override;
    L.chunk = std::max<int64_t>(1, std::min(L.chunk, npairs));
    size_t before = 0;
    for (int p = 0; p < nparts; p++) {
        L.cell_first.push_back((size_t)L.chunk * before);
        before += (size_t)nstates[p] * (size_t)nstates[p];
    }
    return L;
}

}  // namespace iqhip
