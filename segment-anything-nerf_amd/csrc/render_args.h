// render_args.h -- what the files of the fused render share: raymarch.hip
// (render_impl, the workspace, the step kernels), prop_stages.hip,
// final_stage.hip and sgrid.hip.
#pragma once

#include <cmath>

#include "samnerf_common.h"

using namespace samnerf;

// Everything a kernel takes by value stays in an anonymous namespace, here as
// in the stage files, and so do the kernels: their mangled names
// (_ZN12_GLOBAL__N_1..., argument types included) are what six rounds of
// profiles/*.csv and tools/valu_cpi.py name (the proposal kernels' since gained
// one last template argument, the seeded-perturb switch PHX: "Lb0E" before the
// closing "EE" of the earlier names; tools/valu_cpi.py and tools/prop_budget.py
// carry the new ones).  Each stage file therefore fills
// its own argument struct; the host functions that cross files (namespace
// samnerf, below) take plain pointers and samnerf:: types only.
namespace {

constexpr uint32_t kRow = 164;     // head input row: f_sam 128 | f_image 31 | image 3 | depth 1 | pad

// torch.linspace(start, end, steps) element j (CPU float algorithm; see
// samnerf_linspace_host).
struct Lin {
    float start, end, step;
    uint32_t steps;
    __device__ __forceinline__ float operator()(int j) const {
        return (uint32_t)j < steps / 2u ? __builtin_fmaf(step, (float)j, start)
                                        : __builtin_fmaf(-step, (float)(steps - 1u - j), end);
    }
};

Lin make_lin(float start, float end, uint32_t steps) {
    Lin l;
    l.start = start;
    l.end = end;
    l.steps = steps;
    l.step = steps > 1 ? (end - start) / (float)(steps - 1u) : 0.0f;
    return l;
}

// XCD-aware block order.  Blocks are dispatched round-robin over the 8 XCDs
// (block b runs on XCD b % 8), each with its own 4 MB L2.  A launch over n
// ray chunks uses xcd_blocks(n) blocks and block b takes chunk xcd_chunk(b,
// n): XCD x gets the contiguous chunks [x*per, (x+1)*per) -- a band of the
// view -- so the grid cells that neighbouring rays share meet in one L2
// instead of eight.  Chunks >= n are empty.
__host__ __device__ constexpr uint32_t xcd_per(uint32_t n) { return (n + 7u) / 8u; }
__host__ __device__ constexpr uint32_t xcd_blocks(uint32_t n) { return xcd_per(n) * 8u; }
__device__ __forceinline__ uint32_t xcd_chunk(uint32_t b, uint32_t n) {
    return (b & 7u) * xcd_per(n) + (b >> 3);
}

// Grid-space coordinate u = (x + bound) / (2 bound) (grid.py:156) with the
// reference's rounding.  When 2*bound is a power of two the host passes its
// exact reciprocal (inv_b2 != 0) and the division becomes a multiplication
// with the identical result; otherwise it is an IEEE division.
struct GridScale {
    float bound, b2, inv_b2;
    __device__ __forceinline__ float operator()(float x) const {
        return inv_b2 != 0.0f ? (x + bound) * inv_b2 : (x + bound) / b2;
    }
};

GridScale make_grid_scale(float bound) {
    GridScale g;
    g.bound = bound;
    g.b2 = 2.0f * bound;
    int e = 0;
    const float m = std::frexp(g.b2, &e);                 // b2 = m * 2^e, m in [0.5, 1)
    g.inv_b2 = (m == 0.5f && std::isfinite(g.b2)) ? std::ldexp(1.0f, 1 - e) : 0.0f;
    return g;
}

// Gather forms (SAMNERF_LOOKUP, lookup_mode): direct packed / direct per-
// corner reference / de-duplicated box; auto picks per stage.
constexpr int kLookPacked = 0, kLookRef = 1, kLookBox4 = 3;
constexpr int kLookAuto = 4;     // host-side only

constexpr int kAeff = 240;          // columns of the adaptive heads' effective matrix
constexpr int kFSlots = 16;         // grid_mlp f16x3 fragment slots (final_stage.hip), 64 lanes x (8 f16 hi + 8 f16 lo) each

}  // namespace

namespace samnerf {

struct Workspace {
    float* snf;
    float4* rec;       // [N][2] slot-ordered ray records (k_snf, PropArgs::rec)
    float* bins1;
    float* bins2;
    float* wtmp;
    float* u_f;
    float* w_f;
    float* rows;
    float* packed;
    uint4* gpack;      // f16x3 grid_mlp fragments [2][kFSlots][64] (head_mode 0)
    int* gexp;         // their tensors' log2 scales [3]
    float* geo_f;      // [32][16][N] grid_mlp output rows per sample (with_mask, kind 0)
    float* mpacked;    // mask head weight stream (with_mask, kind 0)
    float* aeff;       // [K][240] adaptive heads' effective matrix (with_mask, kinds 1-2)
    float* mlog;       // [N][K] adaptive heads' logits (with_mask, kinds 1-2)
    float* xsum;       // [N][kAeff] their per-ray input sums (with_mask, kinds 1-2; training)
    size_t bytes;
};

// raymarch.hip
Workspace carve(const samnerf_model* m, uint32_t N, void* base);
int make_grid_desc(const samnerf_grid& g, uint32_t C, uint32_t L, GridDesc<16>& d, const char* name);
int lookup_mode();
bool pack_weights(const samnerf_model* m);
bool box4_ok(const GridDesc<16>& g);

// render_impl's stage marks (samnerf_set_stage_events), or null
typedef void (*StageMark)(uint32_t stage, hipStream_t s);

// prop_stages.hip: k_snf, then proposal stages 0 and 1.  What differs between
// a render (render_impl) and a training step (proposal_forward):
struct ProposalRun {
    const float* rays_o;
    const float* rays_d;
    const float* cnf;        // [n_cnf][2] camera near / far, or null
    uint32_t n_cnf;
    RayTiles tiles;          // slot -> ray
    int look;                // gather form (lookup_mode, or kLookPacked)
    StageMark mark;          // stage marks 0 and 1, or null
    float* snf;              // [2][N]
    float4* rec;             // [N][2] slot-ordered ray records, or null
    struct Stage {
        GridDesc<16> grid;
        float* bins_out;     // [TN][N]: the next stage's bins
        float* ds;           // [T][N]
        int32_t* inds_out;   // [TN][N] or null (parity taps)
        float* w_out;        // [T][N] or null (parity taps, training)
    } st[2];
};
// forms[i]: stage i's compiled level classes (KD | KH << 8, 0: the run-time
// form), written where k_prop_sigma ran
void run_proposal_stages(const samnerf_model* m, uint32_t N, const ProposalRun& r, hipStream_t s,
                         uint32_t forms[2]);

// final_stage.hip: stage 2 (k_pack_grid_mlp, k_mask_eff, k_final)
struct FinalRun {
    const float* rays_o;
    const float* rays_d;
    RayTiles tiles;
    GridDesc<16> grid;       // the main grid, L16 C2
    const float* bins_in;    // [33][N]
    float bg;                // scalar background, or
    const float* bg_rgb;     // [n_bg][3] colours in ray order (samnerf_set_background), n_bg 1 or N
    uint32_t n_bg;
    float* image;            // per-ray outputs, ray order (FinalArgs)
    float* depth;
    float* wsum;
    uint32_t img_ld, scal_ld;
    float* rows;             // [N, kRow] head-input rows, or null
    bool sam_rows;           // the s_grid composite follows (no sum_after_mlp)
    float* sigma_tap;        // parity taps (FinalArgs), null in every product render
    uint32_t* rows_tap;
    uint32_t tap_stride;
    StageMark mark;          // stage mark 2, or null
};
// form: k_final's layout (final_layout), written when k_final was launched
int run_final(const samnerf_model* m, uint32_t N, const FinalRun& r, const Workspace& w, hipStream_t s,
              uint32_t& form);

// sgrid.hip: f_sam into the head-input rows, the form by `look` and N
void launch_sgrid(uint32_t N, RayTiles tiles, const GridDesc<16>& grid, const float* u_in, const float* w_in,
                  float* rows, uint32_t* rows_tap, uint32_t tap_stride, int look, hipStream_t s);

}  // namespace samnerf
