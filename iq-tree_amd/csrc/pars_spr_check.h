// pars_spr_check.h -- the validation of an SPR scan program (include/iqhip.h "Parsimony SPR scan"): plain C++ without any
// device code, so that a stand-alone host program can run it under sanitizers (tools/asan_pars_spr.sh).
#pragma once
#include <stdint.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/iqhip.h"

namespace iqhip {

// Validation of a job / step program (include/iqhip.h "Parsimony SPR scan").  depth: nsteps entries or NULL; max_depth: the
// deepest step or NULL.  Returns an empty string or what is wrong.
inline std::string pars_spr_check(int ntaxa, int nvectors, const uint8_t *valid, const iqhip_pars_spr_job *jobs, int njobs,
                                  const iqhip_pars_spr_step *steps, int nsteps, int32_t *depth, int *max_depth) {
    if (ntaxa < 1 || nvectors < 0) return "bad slot counts";
    if (njobs < 0 || (njobs > 0 && !jobs)) return "bad job list";
    if (nsteps < 0 || (nsteps > 0 && !steps)) return "bad step list";
    const int64_t nslots = (int64_t)ntaxa + nvectors;
    auto bad_slot = [&](int32_t s) -> const char * {
        if (s < 0 || s >= nslots) return "slot outside [0, ntaxa + nvectors)";
        if (s >= ntaxa && !(valid && valid[s - ntaxa])) return "slot has never been written";
        return nullptr;
    };
    std::vector<int32_t> dep((size_t)nsteps, -1);
    int deepest = 0;
    for (int j = 0; j < njobs; j++) {
        const iqhip_pars_spr_job &job = jobs[j];
        const std::string name = "job " + std::to_string(j);
        if (const char *why = bad_slot(job.subtree)) return name + ": subtree " + why;
        if (job.first_step < 0 || job.nsteps < 0 || (int64_t)job.first_step + job.nsteps > nsteps)
            return name + ": steps outside [0, nsteps)";
        int32_t last_at[IQHIP_PARS_SPR_MAX_RADIUS + 1];
        std::fill(last_at, last_at + IQHIP_PARS_SPR_MAX_RADIUS + 1, -1);
        for (int k = 0; k < job.nsteps; k++) {
            const size_t g = (size_t)job.first_step + (size_t)k;
            const iqhip_pars_spr_step &st = steps[g];
            const std::string sname = name + " step " + std::to_string(k);
            if (dep[g] >= 0) return sname + ": belongs to an earlier job too";
            if (st.flags & ~(int32_t)IQHIP_PARS_SPR_NO_SCORE) return sname + ": unknown flag";
            if (const char *why = bad_slot(st.side)) return sname + ": side " + why;
            if (const char *why = bad_slot(st.target)) return sname + ": target " + why;
            int d = 0;
            if (st.parent >= 0) {
                if (st.parent >= k) return sname + ": parent is not an earlier step of the job";
                d = dep[(size_t)job.first_step + (size_t)st.parent] + 1;
                if (d > IQHIP_PARS_SPR_MAX_RADIUS) return sname + ": deeper than IQHIP_PARS_SPR_MAX_RADIUS";
                if (last_at[d - 1] != st.parent) return sname + ": parent is not the most recent step one level up";
            }
            dep[g] = d;
            last_at[d] = k;
            deepest = std::max(deepest, d);
        }
    }
    if (depth) std::copy(dep.begin(), dep.end(), depth);
    if (max_depth) *max_depth = deepest;
    return std::string();
}

}  // namespace iqhip
