// Stand-alone host program for tools/asan_pars_spr.sh: runs the validation of an SPR scan program
// (iq-tree_amd/csrc/pars_spr_check.h, what iqhip_pars_spr_scan runs before it launches anything) under AddressSanitizer and
// UBSan on the CPU -- a legal program, one mutation of each rule, the integer edge cases of the job ranges, and random
// programs whose every field is drawn from a range that reaches past the legal one.  No device, no Python.
#include <stdio.h>
#include <stdlib.h>

#include <random>
#include <string>
#include <vector>

#include "../iq-tree_amd/csrc/pars_spr_check.h"

static int failures = 0;

static void expect(bool ok, const char *what) {
    if (!ok) {
        fprintf(stderr, "FAILED: %s\n", what);
        failures++;
    }
}

int main() {
    const int T = 6, V = 12;
    const std::vector<uint8_t> valid((size_t)V, 1);
    const std::vector<iqhip_pars_spr_step> steps = {{-1, 1, 2, 0}, {0, 6, 3, 0}, {1, 7, 4, 0}, {0, 8, 5, 0}, {3, 9, 0, 1}};
    const std::vector<iqhip_pars_spr_job> jobs = {{10, 0, 5, 0}};
    std::vector<int32_t> depth(steps.size());
    int deepest = -1;
    auto run = [&](const std::vector<iqhip_pars_spr_job> &j, const std::vector<iqhip_pars_spr_step> &s, const uint8_t *v,
                   int32_t *d = nullptr) {
        return iqhip::pars_spr_check(T, V, v, j.data(), (int)j.size(), s.data(), (int)s.size(), d, &deepest);
    };
    expect(run(jobs, steps, valid.data(), depth.data()).empty() && deepest == 2, "the legal program passes");
    expect(depth == std::vector<int32_t>({0, 1, 2, 1, 2}), "its depths");
    auto mutated = [&](int k, int field, int32_t value) {
        std::vector<iqhip_pars_spr_step> s = steps;
        (&s[(size_t)k].parent)[field] = value;
        return s;
    };
    expect(!run(jobs, mutated(2, 0, 2), valid.data()).empty(), "a forward parent");
    expect(!run(jobs, mutated(4, 0, 1), valid.data()).empty(), "a stale parent");
    expect(!run(jobs, mutated(1, 1, T + V), valid.data()).empty(), "a slot past the end");
    expect(!run(jobs, mutated(1, 2, -1), valid.data()).empty(), "a negative slot");
    expect(!run(jobs, mutated(1, 2, INT32_MIN), valid.data()).empty(), "INT32_MIN as a slot");
    expect(!run(jobs, mutated(0, 3, 2), valid.data()).empty(), "an unknown flag");
    expect(!run(jobs, mutated(0, 3, INT32_MIN), valid.data()).empty(), "the sign bit as a flag");
    expect(!run(jobs, steps, nullptr).empty(), "no valid flags at all");
    expect(!run({{10, 0, 3, 0}, {11, 2, 3, 0}}, steps, valid.data()).empty(), "overlapping jobs");
    expect(!run({{10, INT32_MAX, INT32_MAX, 0}}, steps, valid.data()).empty(), "a job range that overflows 32 bits");
    expect(!run({{10, 4, 2, 0}}, steps, valid.data()).empty(), "a job range past the end");
    expect(!run({{10, -1, 2, 0}}, steps, valid.data()).empty(), "a negative first step");
    expect(!run({{10, 0, -1, 0}}, steps, valid.data()).empty(), "a negative step count");
    std::vector<iqhip_pars_spr_step> chain = {{-1, 1, 2, 0}};
    for (int k = 0; k < IQHIP_PARS_SPR_MAX_RADIUS; k++) chain.push_back({k, 1, 2, 0});
    expect(run({{0, 0, (int32_t)chain.size(), 0}}, chain, valid.data()).empty() && deepest == IQHIP_PARS_SPR_MAX_RADIUS, "depth 10");
    chain.push_back({IQHIP_PARS_SPR_MAX_RADIUS, 1, 2, 0});
    expect(!run({{0, 0, (int32_t)chain.size(), 0}}, chain, valid.data()).empty(), "depth 11");
    expect(iqhip::pars_spr_check(T, V, nullptr, nullptr, 0, nullptr, 0, nullptr, nullptr).empty(), "nothing at all");
    // random programs: most are refused, none may read or write out of bounds
    std::mt19937 gen(1);
    int accepted = 0;
    for (int rep = 0; rep < 20000; rep++) {
        const int ns = (int)(gen() % 24), nj = (int)(gen() % 4);
        std::vector<iqhip_pars_spr_step> s((size_t)ns);
        std::vector<iqhip_pars_spr_job> j((size_t)nj);
        std::vector<uint8_t> v((size_t)V);
        for (auto &x : v) x = gen() % 8 != 0;
        int k = 0;
        for (auto &x : s) {
            x = {(int32_t)(gen() % 6 == 0 ? -1 : (int)(gen() % (unsigned)(k + 2)) - 1), (int32_t)(gen() % (T + V + 2)) - 1,
                 (int32_t)(gen() % (T + V + 2)) - 1, (int32_t)(gen() % 16 == 0 ? gen() % 4 : gen() % 2)};
            k++;
        }
        int at = 0;
        for (auto &x : j) {
            const int n = ns > at ? (int)(gen() % (unsigned)(ns - at + 2)) : (int)(gen() % 2);
            x = {(int32_t)(gen() % (T + V + 1)), (int32_t)(gen() % 16 == 0 ? (int)(gen() % 30) - 3 : at), n, 0};
            at += n;
        }
        std::vector<int32_t> d((size_t)ns, -7);
        const std::string err = iqhip::pars_spr_check(T, V, v.data(), j.data(), nj, s.data(), ns, d.data(), &deepest);
        if (err.empty()) {
            accepted++;
            for (const auto &x : j)
                for (int q = 0; q < x.nsteps; q++) {
                    const int32_t dq = d[(size_t)x.first_step + (size_t)q];
                    expect(dq >= 0 && dq <= IQHIP_PARS_SPR_MAX_RADIUS && dq <= deepest, "an accepted step has a legal depth");
                }
        }
    }
    expect(accepted > 50, "some random programs are legal");
    printf("pars_spr_check: %d failures, %d of 20000 random programs accepted\n", failures, accepted);
    return failures ? 1 : 0;
}
