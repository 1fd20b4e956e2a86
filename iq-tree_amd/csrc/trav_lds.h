// trav_lds.h -- how each traversal kernel family divides its dynamic LDS, in doubles from the start of smem[].  The
// kernel bodies take their pointers from these functions, the launch chooser (plan.hip choose_traverse_mfma) its byte
// counts and the planner (plan.hip lds_budget) what is left for a chunk's plan regions: one description each.  Every
// family ends with the plan regions at sReg (Plan::lds_doubles of them); what follows those is named per family.
// nx = state_unknown + 1 - n: the tip vectors of the states beyond the n plain ones.
#pragma once
#include <hip/hip_runtime.h>

namespace iqhip {

constexpr int kTravWg = 256;                        // threads per workgroup of every traversal kernel
constexpr int kTravMaxLdsBytes = 150 * 1024;        // dynamic LDS every matrix-core traversal kernel is allowed ...
constexpr int kTravGenericMaxLdsBytes = 160 * 1024; // ... and k_traverse_mfma, which has no static arrays
constexpr int kTrav4MaxLdsBytes = 150 * 1024;       // k_traverse4: 160 KB minus the static arrays (9.4 KB: fold_tail 3.1 KB, the fill's descriptor copies 4.4 KB -- pair lengths included -- and row pointers 2 KB)

__host__ __device__ constexpr int tipx_doubles(int n, int nx) { return nx * n; }   // the [nx][n] tip vectors of the states beyond n

// k_traverse_mfma<N>: zero-padded A images of U and U^-1, [MT][KS][64] each
struct GenericLds { int sU, sUi, sTipx, sReg; };
__host__ __device__ constexpr GenericLds generic_lds(int n, int nx) {
    const int img = ((n + 15) / 16) * (n / 4) * 64;
    return {0, img, 2 * img, 2 * img + tipx_doubles(n, nx)};
}

// trav_mfma2_body<N>: 64 states keep the fragment images [MTF][KS][64] (+ [KS][64] tail rows when N = 16m + 4) in LDS,
// 20 states in registers; tip rows of the plain states as an [N][N] copy while that is at most 4 KB (tip_copy)
struct Mfma2Lds { int sU, sUi, sU4, sUi4, sUiT, sTipx, sReg; bool tip_copy; };
__host__ __device__ constexpr Mfma2Lds mfma2_lds(int n, int nx) {
    const int ks = n / 4;
    const int img1 = n < 64 ? 0 : (n / 16) * ks * 64, img4 = (n < 64 || n % 16 != 4) ? 0 : ks * 64;
    const bool tip_copy = n * n * 8 <= 4096;
    const int tipx = 2 * img1 + 2 * img4 + (tip_copy ? n * n : 0);
    return {0, img1, 2 * img1, 2 * img1 + img4, 2 * img1 + 2 * img4, tipx, tipx + tipx_doubles(n, nx), tip_copy};
}
// ... behind the plan regions, when the plan parks operands (Plan::nhold > 0): one tile vector per wave of the workgroup
__host__ __device__ constexpr int mfma2_park_doubles(int block) { return (kTravWg / 64) * 16 * block; }

// trav_rows64_body: all tip rows, then the previous result and the Hadamard product as k-step slices, [2 parities][16][64] each
struct Rows64Lds { int sTip, sX, sT, sReg; };
__host__ __device__ constexpr Rows64Lds rows64_lds(int nx) {
    const int tip = (64 + nx) * 64, slices = 2 * 16 * 64;
    return {0, tip, tip + slices, tip + 2 * slices};
}

// k_traverse_mfma_mix20: the A fragments live in registers, nothing but the plan regions
struct Mix20Lds { int sReg; };
__host__ __device__ constexpr Mix20Lds mix20_lds() { return {0}; }

// k_traverse_mfma_top64 runs both 64-state bodies in one launch: the larger of the two roles' fixed parts
// (k_traverse_mfma_top20's two roles are both trav_mfma2_body<20>)
__host__ __device__ constexpr int top64_fixed_doubles(int nx) {
    return mfma2_lds(64, nx).sReg > rows64_lds(nx).sReg ? mfma2_lds(64, nx).sReg : rows64_lds(nx).sReg;
}

// k_traverse4w (4 states, 9 .. 32 categories): U and U^-1 of every class, [nclass][U 16 | U^-1 16]; the per-category tip
// vectors of the four plain states, [4][block], for the fill of the leaf tables; then the plan regions -- a leaf child's is
// [ex block][table 5 * block] as in k_traverse4, an inner child's [ex block]
struct Wide4Lds { int sW, sTipc, sReg; };
__host__ __device__ constexpr Wide4Lds wide4_lds(int nclass, int block) { return {0, 32 * nclass, 32 * nclass + 4 * block}; }
constexpr int kWide4LdsKb = 40;   // per workgroup, fixed part included: four workgroups (16 waves) per CU

// k_traverse4: tip vectors [32][4], one block of values, the plan regions, then the leaf-state slots -- one byte per
// thread each, i.e. kTravWg / 8 doubles; slot 0 is shared by all non-leaf children.  The state bytes lie [wave][slot][64]
// (slot < Plan::state_slots): a wave's slots are contiguous, so one LDS-direct dword load fills four of them, each group
// of 16 lanes fetching the 64 bytes of one leaf child (kernels_valu4.hip, the chunk fill's state requests).
// The fill image (iqhip_engine::fill_image, built by k_fill4_image) mirrors the plan regions and nothing else: chunk i of the
// plan lies at DevOp::image_off doubles (16-byte aligned) and is the chunk's s_reg byte for byte -- every region at its
// lds_left / lds_right, sized by child_region_blocks -- over the chunk's own extent, which is at most Plan::lds_doubles; the
// copy in k_traverse4 writes [s_reg, s_reg + extent) and never the state slots behind the regions.
// The row pointers those requests read, s_row[slot], are a static array of kTrav4RowSlots pointers inside the kernel,
// not part of the dynamic LDS: budget, chunk cuts and launch bytes of a plan do not depend on it.  lay_out_lds ends a
// chunk before its slots would outgrow the array and check_plan holds every chunk to it.
constexpr int kTrav4RowSlots = 256;
struct Trav4Lds { int s_tip, s_val, s_reg, slot_doubles; };
__host__ __device__ constexpr Trav4Lds trav4_lds(int block) { return {0, 128, 128 + block, kTravWg / 8}; }
__host__ __device__ constexpr size_t trav4_lds_bytes(int block, int lds_doubles, int state_slots) {
    return ((size_t)trav4_lds(block).s_reg + (size_t)lds_doubles + (size_t)state_slots * trav4_lds(block).slot_doubles) * sizeof(double);
}

}  // namespace iqhip
