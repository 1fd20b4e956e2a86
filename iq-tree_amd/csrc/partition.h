// partition.h -- the partition group of the edge-linked partition model (-q / -spp; include/iqhip.h, "Edge-linked
// partition models") and what its drivers share.  The group's life cycle, the joint branch solves and traverse_lnl are in
// partition.hip, its rows, RELL sums and UFBoot in ufboot.hip, its joint pairwise distances in pairdist.hip.
#pragma once
#include <vector>

#include "iqhip_internal.h"

namespace iqhip {
constexpr size_t kPartMaxLdsBytes = 64 * 1024;
}

struct iqhip_partition {
    int device = 0, nparts = 0;
    std::vector<iqhip_engine *> m;
    std::vector<double> rate;
    hipStream_t stream = nullptr;
    std::vector<hipEvent_t> ev;      // one per member, recorded on its stream
    hipEvent_t ev_done = nullptr;    // recorded on the group's stream behind its last launch
    iqhip::PairBuf<char> table;             // [nparts] PartDesc ++ [nitems] PartItem
    std::vector<char> uploaded;             // the bytes of `table` the device holds
    iqhip::PairBuf<iqhip::PartScale> scale;
    iqhip::PairBuf<double> out;             // per member: lnL sums / scale-factor terms
    iqhip::PairBuf<iqhip::NewtonState> state;
    iqhip::DevBuf<double> d_partials;       // [nitems][2]
    // iqhip_partition_optimize_branch_batch, per chunk of tasks
    iqhip::PairBuf<iqhip::NewtonState> bstate;     // [tasks]
    iqhip::PairBuf<char> btable;            // [nparts] PartSlots ++ [tasks][nparts][2] scale-counter pointers ++ [tasks][nparts] row pointers
    iqhip::PairBuf<double> bout;            // [tasks][nparts]
    iqhip::DevBuf<double> d_bpartials;      // [tasks][nitems][2]
    iqhip::DevBuf<int32_t> d_blnl;          // [tasks]: the task's lnL sums are in d_bpartials
    int nitems = 0, lds_doubles = 0;
    // iqhip_debug_partition_timing: the derivative launches, the update launches of the last solve or batch
    double ms[2] = {0.0, 0.0};
    int64_t launches = 0;
    // RELL sums and UFBoot bookkeeping of the group (iqhip_partition_ptnlh_rell, iqhip_partition_ufboot_*): the state an
    // engine keeps, owned by the group (ms: the members' products, the update kernels); ufb_sums: the device table of the
    // members' bt.sums pointers; ufb_rell: the summed matrix of iqhip_partition_ptnlh_rell; ufb_gen: every member's
    // sample-matrix generation at init
    iqhip::UfbootState ufb;
    iqhip::PairBuf<const double *> ufb_sums;
    iqhip::DevBuf<double> ufb_rell;
    std::vector<uint64_t> ufb_gen;
    // iqhip_partition_pair_distances: the members' descriptors, the compacted cell lists [chunk][sum_p n_p^2] (member p's at
    // chunk * sum_{q < p} n_q^2) and their lengths [chunk][nparts] of one chunk of pairs, per pair the initial distance and
    // the result {optx, d2l, evaluations, status}
    struct {
        iqhip::PairBuf<iqhip::PartPairDesc> desc;
        iqhip::DevBuf<uint16_t> cells;
        iqhip::DevBuf<int32_t> nnz;
        iqhip::DevBuf<double> init, out;
        double ms[2] = {0.0, 0.0};   // iqhip_debug_partition_pair_timing: the members' count launches, the solve launches
    } pdist;
};

namespace iqhip {
// every call on a group starts here: the group exists, its members are still what a member must be, its device is current
int use_group(iqhip_partition *g, const char *what);
// the group's stream waits for everything enqueued on the members' streams so far ...
int wait_for_members(iqhip_partition *g);
// ... and the members' streams for everything enqueued on the group's
int members_wait(iqhip_partition *g);
// every row of a list lies inside every member's store: row r of the group is row r of each member
int group_rows_ok(const iqhip_partition *g, const char *what, const int32_t *rows, int nrows);
}  // namespace iqhip
