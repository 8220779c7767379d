// final_stage.hip -- stage 2 of the fused render (the map of the pipeline is
// in raymarch.hip): k_final with its weight packing (k_pack_grid_mlp), the
// adaptive mask heads' effective matrix (k_mask_eff), and the host path that
// picks k_final's form (run_final).
#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "f16x3.h"
#include "gather_c2.h"
#include "raymarch_device.h"
#include "render_args.h"
#include "samnerf_common.h"
#include "sh_device.h"

using namespace samnerf;

namespace {

struct FinalArgs {
    const float* rays_o;
    const float* rays_d;
    uint32_t N;
    GridScale gs;
    float bg;               // scalar background, used when bg_rgb (below) is null
    // The main grid's level descriptors by value (kernarg), copied into LDS
    // at kernel start; each half-wave reads its slot's descriptor from there.
    // Round 1 read them from a copy in the workspace (written by a one-thread
    // kernel before each render): the kernel's stores may alias that table,
    // so the compiler could not use the scalar cache, and the per-half-wave
    // select became one 64-lane 16-B load per descriptor -- ~33 extra VMEM
    // instructions per wave and sample competing with the gathers for the
    // texture-address path (profiles/r2b PMC: 90 VMEM reads per wave-sample),
    // and the source of the prefetch nondeterminism.  Kernarg
    // scalar loads + selects in the loop measured slower (1.23 vs 0.92 ms:
    // SGPR-bound reloads, lgkmcnt waits); LDS: 0.82 ms.
    GridDesc<16> grid;
    uint32_t kdense[2], khashed[2];   // wave-uniform slot classes of k-blocks 0 / 1 (host-side)
    // LAY 1's hashed slots (round 6): byte offset of the slot's half-wave-0
    // level (emb + hoff8 is a uniform SGPR base); half-wave 1's level is the
    // next one, hbit = its byte distance 8 S (S = the levels' common power-of-
    // two size, above every masked row bit), hm8 = 8 (S - 1)  (final_layout
    // admits LAY 1 only when every hashed slot is laid out so)
    uint32_t hoff8[2][4];
    uint32_t hbit, hm8;
    const float* grid_emb;  // == grid.emb, as a kernel argument so gathers are global_load (not flat)
    const float* G0;   // grid_mlp [64,32]
    const float* G1;   // [64,64]
    const float* G2;   // [16,64]
    const uint4* gpack;     // f16x3: the grid_mlp fragments [hi / lo][kFSlots][64] (k_pack_grid_mlp)
    const int* gexp;        // f16x3: log2 scale of G0 / G1 / G2's fragments
    const float* V0;   // view_mlp [32,31]
    const float* V1;   // [32,32]
    const float* V2;   // [3,32]
    const float* bins_in;   // [T+1][N]
    const float* snf;       // [2][N]
    float* u_out;      // [T][3][N] grid-space sample positions
    float* w_out;      // [T][N] final weights
    float* image;      // [N,3], row stride img_ld
    float* depth;      // [N], stride scal_ld
    float* wsum;       // [N], stride scal_ld
    uint32_t img_ld, scal_ld;   // 3 / 1, or the gather tile's row (samnerf_render_forward_tile)
    float* rows;       // [N, kRow] or null
    RayTiles tiles;    // slot -> ray: rays_o / rays_d and the per-ray outputs are in ray order
    // N1 (flagged, non-parity; samnerf_model.t_thresh): optical depth
    // -ln(t_thresh) past which a ray is opaque; a wave whose rays all are
    // stops marching.  INFINITY: off (the default, the reference's semantics).
    float exit_depth;
    float* geo_out;    // GEO: [T][16][N] the grid_mlp output rows of every sample (mask head input)
    // AD (adaptive mask heads): the head is linear in the per-sample grid
    // features and MLP intermediates, so sum_k w_k head(x_k) = E . sum_k w_k x_k
    const float* aeff; // [K][240] E, blocks g 32 | h1 64 | h2 64 | o3 16 | v1 32 | v2 32 (k_mask_eff)
    float* mlog;       // [N][K] instance_mask_logits (ray order)
    float* xsum;       // [N][kAeff] the per-ray sums sum_k w_k x_k in E's column order (ray
                       // order), the adaptive head's input for its training (mask_head_train.hip)
    uint32_t mask_out;
    // parity taps (samnerf_taps; null in every product render): sigma of
    // every sample [T][N], and the corner rows of every level of the samples
    // of slots r % tap_stride == 0, [N / tap_stride][T][16][8]
    float* sigma_tap;
    uint32_t* rows_tap;
    uint32_t tap_stride;
    // samnerf_set_background's background / bg_rgb / n_bg (appended: the arguments above
    // keep their kernarg offsets)
    uint32_t last_inf;      // 1: 'last_sample' (the last sample's ds is +inf), 0: transparent
    uint32_t n_bg;          // rows of bg_rgb: 1 (one colour) or N (per ray)
    const float* bg_rgb;    // [n_bg][3] in ray order, or null: the scalar bg
};

// ---- grid_mlp on f16x3 MFMAs (v_mfma_f32_32x32x16_f16, fp32 accumulate).
// Transposed orientation: A = weights (rows = hidden units), B = activations
// (columns = 32 rays), so a layer's accumulator is the next layer's B operand
// as it stands.  Lane (j, h) of a 32x32 accumulator holds rows rho(q) + 4h,
// rho(q) = (q&3) + 8(q>>2); k-block kb of a 64-wide input takes registers
// 8(kb&1)..8(kb&1)+7 of tile kb>>1, and the weights are stored permuted to
// match (hidden_unit).  Each product is split x = hi + lo (fp16 RNE, on
// power-of-two scaled operands) and A.B = A_lo.B_hi + A_hi.B_lo + A_hi.B_hi
// (f16x3.h): fp32-equivalent, at 3 MFMAs of 32 cycles per 16-deep k-block
// instead of 8 fp32 MFMAs of 64.

constexpr int kF1 = 0;               // grid_mlp.0: slot kb*2 + ob      (kb < 2)  W[64,32]
constexpr int kF2 = 4;               // grid_mlp.1: slot 4 + kb*2 + ob  (kb < 4)  W[64,64]
constexpr int kF3 = 12;              // grid_mlp.2: slot 12 + kb        (kb < 4)  W[16,64]
// view_mlp on v_mfma_f32_32x32x2_f32 (once per ray): [q 16][lane] each
constexpr int kV1 = 0;               // view_mlp.0  q<8: geo acc rows, q>=8: sh pairs
constexpr int kV2 = 1024;            // view_mlp.1  W[32,32]
constexpr int kV3 = 2048;            // view_mlp.2  W[3,32]
constexpr int kVTotal = 3072;

__device__ __forceinline__ int rho(int q) { return (q & 3) + 8 * (q >> 2); }

// input unit of a 64-wide layer fed by accumulator tiles (kb, half h, element m)
__device__ __forceinline__ int hidden_unit(int kb, int h, int m) {
    return (kb >> 1) * 32 + rho(8 * (kb & 1) + m) + 4 * h;
}

// Level gathered by half-wave h in slot q of k-block kb (its B operand of the
// first layer holds that level's two channels at k = 2q, 2q + 1).  Adjacent
// levels share a slot: the dense levels (the coarse ones) then pair up in
// both half-waves, so their slots take gather_issue_c2's uniform dense path.
__host__ __device__ constexpr int final_level(int kb, int h, int q) { return 8 * kb + 2 * q + h; }

__device__ float grid_weight(const FinalArgs& a, int slot, int lane, int m) {
    const int i = lane & 31, h = lane >> 5;
    if (slot < kF2) {                          // input k = 2*level + channel, level = final_level(kb, h, m / 2)
        const int kb = slot >> 1, ob = slot & 1;
        return a.G0[(ob * 32 + i) * 32 + 2 * final_level(kb, h, m >> 1) + (m & 1)];
    }
    if (slot < kF3) {
        const int t = slot - kF2, kb = t >> 1, ob = t & 1;
        return a.G1[(ob * 32 + i) * 64 + hidden_unit(kb, h, m)];
    }
    const int kb = slot - kF3;
    return i < 16 ? a.G2[i * 64 + hidden_unit(kb, h, m)] : 0.0f;
}

__device__ float view_weight(const FinalArgs& a, int idx) {
    const int lane = idx & 63, i = lane & 31, h = lane >> 5;
    if (idx < kV2) {                           // f_image = [geo (units 1..15), sh * wsum]
        const int r = idx >> 6;
        if (r < 8) {
            const int unit = rho(r) + 4 * h;   // grid_mlp output row; unit 0 is sigma
            return unit >= 1 ? a.V0[i * 31 + unit - 1] : 0.0f;
        }
        return a.V0[i * 31 + 15 + 2 * (r - 8) + h];
    }
    if (idx < kV3) {
        const int r = (idx - kV2) >> 6;
        return a.V1[i * 32 + rho(r) + 4 * h];
    }
    const int r = (idx - kV3) >> 6;
    return i < 3 ? a.V2[i * 32 + rho(r) + 4 * h] : 0.0f;
}

// Exact-fp32 grid_mlp (head_mode 1) on v_mfma_f32_32x32x2_f32: one weight
// per lane and k-step, A[i][k = h] for the lane (i, h), 128 k-steps:
//   layer 1  step = ob*16 + kb*8 + m        (m: register of the gathered f[8])
//   layer 2  step = 32 + ob*32 + t*16 + q   (q: register of accumulator tile t)
//   layer 3  step = 96 + t*16 + q
// Each MFMA is the fma chain of its two k terms in k order (exact fp32).
constexpr int kXSteps = 128;

__device__ float grid_weight_exact(const FinalArgs& a, int step, int lane) {
    const int i = lane & 31, h = lane >> 5;
    if (step < 32) {
        const int ob = step >> 4, kb = (step >> 3) & 1, m = step & 7;
        return a.G0[(ob * 32 + i) * 32 + 2 * final_level(kb, h, m >> 1) + (m & 1)];
    }
    if (step < 96) {
        const int s = step - 32, ob = s >> 5, t = (s >> 4) & 1, q = s & 15;
        return a.G1[(ob * 32 + i) * 64 + t * 32 + rho(q) + 4 * h];
    }
    const int s = step - 96, t = s >> 4, q = s & 15;
    return i < 16 ? a.G2[i * 64 + t * 32 + rho(q) + 4 * h] : 0.0f;
}

#define MFMA32(A, B, C) __builtin_amdgcn_mfma_f32_32x32x2f32((A), (B), (C), 0, 0, 0)

// grid_mlp fragments for the f16x3 form (head_mode 0, f16x3.h), once per
// render (one workgroup): each weight tensor scaled by the power of two that
// puts its max |w| in [2^13, 2^14) (scale_exp_of_max), in grid_weight's slot layout, hi then lo;
// gexp[l] = log2 of tensor l's scale.  (A per-tensor scale: the scaled
// accumulators of a sample column then differ from the true values by one
// factor, so each layer's outputs are rescaled straight from their max.)
__global__ void __launch_bounds__(256) k_pack_grid_mlp(FinalArgs a, uint4* gpack, int* gexp) {
    __shared__ float wm[3][4];
    __shared__ int ke[3];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float m0 = 0.0f, m1 = 0.0f, m2 = 0.0f;
    // unrolled: the 28 loads per thread issue together (one memory round trip)
#pragma unroll
    for (int i = tid; i < 64 * 32; i += 256) m0 = fmaxf(m0, fabsf(a.G0[i]));
#pragma unroll
    for (int i = tid; i < 64 * 64; i += 256) m1 = fmaxf(m1, fabsf(a.G1[i]));
#pragma unroll
    for (int i = tid; i < 16 * 64; i += 256) m2 = fmaxf(m2, fabsf(a.G2[i]));
    m0 = wave_max64(m0);
    m1 = wave_max64(m1);
    m2 = wave_max64(m2);
    if (lane == 0) {
        wm[0][wave] = m0;
        wm[1][wave] = m1;
        wm[2][wave] = m2;
    }
    __syncthreads();
    if (tid < 3) {
        const float m = fmaxf(fmaxf(wm[tid][0], wm[tid][1]), fmaxf(wm[tid][2], wm[tid][3]));
        ke[tid] = scale_exp_of_max(m);
        gexp[tid] = ke[tid];
    }
    __syncthreads();
    for (int idx = tid; idx < kFSlots * 64; idx += 256) {
        const int slot = idx >> 6, layer = slot < kF2 ? 0 : slot < kF3 ? 1 : 2;
        float v[8];
#pragma unroll
        for (int m = 0; m < 8; ++m) v[m] = grid_weight(a, slot, idx & 63, m);
        split8_f16(v, exp2i(ke[layer]), gpack[idx], gpack[kFSlots * 64 + idx]);
    }
}

// One wave marches 32 (ray, slot) columns: with S slots per ray, lane (j, h)
// owns slot j / R of ray j % R (R = 32 / S rays per wave), i.e. samples
// slot, slot + S, slot + 2S, ...  For k-block kb it gathers both channels of
// levels final_level(kb, h, 0..3) = 8kb + h, 8kb + 2 + h, .. -- exactly its B
// operand of the first layer (grid_weight permutes the weight columns to
// match) -- so the hash grid feeds the matrix cores
// with no data movement.  grid_mlp 32->64->64->16 runs on f16x3 MFMAs,
// view_mlp 31->32->32->3 (once per ray) on fp32 MFMAs.  Compositing: each
// step the S slots of a ray exchange their optical depths by shuffle and
// every lane forms the ray's exclusive cumulative sum in sample order (the
// reference's sequential double cumsum, exactly), so the stored weights are
// final; per-slot partial sums of w, w*t and w*features are added at the end.
// S > 1 only serves small N (one rank's share of a view): S-times more waves,
// while a wave still gathers at adjacent samples of neighbouring rays.
// Occupancy: the S = 1 form without the cross-sample prefetch runs at 3 waves
// per SIMD (168 VGPRs, 10 spilled): more waves hide the gather latency better
// than the prefetch did at 2 (0.797 vs 0.826 ms per view); the S = 2 / 4 forms
// spill 20+ registers at 3 waves and stay at 2 (0.139 vs 0.158 ms at 32K rays).
#ifndef SAMNERF_DIAG_FINAL_WAVES
#define SAMNERF_DIAG_FINAL_WAVES 3
#endif
template <int S_, bool PLAIN_ = true>
constexpr int final_waves() { return (S_ == 1 && PLAIN_) ? SAMNERF_DIAG_FINAL_WAVES : 2; }

// EXIT: the N1 early-exit form, its own instantiation at 2 waves per SIMD:
// the exit in the sample loop raised the 3-wave form's spills from 10 to 22
// VGPRs (and cost the default kernel 0.80 -> 0.92 ms per view while it was a
// run-time check in the one instantiation)
// GEO: also store every sample's grid_mlp output rows (geo_feat) for the
// mask head (its own instantiation, only for renders of a mask model).
// SA: --sum_after_mlp (renderer.py:339-342): the view MLP runs on every
// sample's colour features, image = sigmoid(sum_k w_k view_mlp(colour_k)).
// AD: the adaptive mask heads (1 'density', 2 'rgb', S = 1 only): per-ray
// weighted sums of the grid features and the grid_mlp (and, SA, view_mlp)
// intermediates, then instance_mask_logits = E . sums (the head is linear).
// The EXIT / GEO / SA forms run at 2 waves per SIMD, the AD forms at 1.
template <int S_, bool PLAIN_, int AD_>
constexpr int final_waves_of() { return AD_ ? 1 : final_waves<S_, PLAIN_>(); }

// LAY: the main grid's level layout as the kernel sees it.
//   0  run time: slot classes from the kernel arguments (kdense / khashed),
//      the grid scale's division / multiplication picked per call;
//   1  the reference architecture's grid (network.py:82-86: L16 C2, 2^19
//      rows per level, base resolution 16 -> levels 0-4 dense, 5-15 hashed)
//      with a power-of-two grid scale: k-block 0's slots are dense, dense,
//      mixed, hashed, k-block 1's all hashed -- compile-time constants, so the
//      sample loop is straight-line code (no per-slot uniform branches for the
//      scheduler to stop at, no per-slot selects) and the grid scale is one
//      multiply.  The host picks 1 when the model's descriptors match
//      (final_layout), else 0; both give the same bits.
// TAP: the parity-tap stores (sigma of every sample, the corner rows) are
// compiled in.  Product renders run TAP = false: the tap address arithmetic
// and its branches are not in their sample loop at all.
constexpr uint32_t kLay1Dense[2] = {0x3u, 0x0u}, kLay1Hashed[2] = {0x8u, 0xFu};

template <int T, int S, bool EXACT, bool EXIT = false, bool GEO = false, bool SA = false, int AD = 0,
          int LAY = 0, bool TAP = true>
__global__ void __launch_bounds__(256)
__attribute__((amdgpu_waves_per_eu(final_waves_of<S, !EXIT && !GEO && !SA, AD>(),
                                   final_waves_of<S, !EXIT && !GEO && !SA, AD>())))
k_final(FinalArgs a) {
    static_assert(AD == 0 || S == 1, "adaptive mask forms: one segment");
    static_assert(AD != 2 || SA, "the 'rgb' adaptive head reads the per-sample view MLP (sum_after_mlp)");
    static_assert(S == 1 || S == 2 || S == 4, "segments per ray");
    static_assert(kXSteps * 64 == 2 * kFSlots * 64 * 4, "exact weights reuse the f16x3 slots");
    constexpr int R = 32 / S, TS = T / S;
    __shared__ uint4 Fbuf[2 * kFSlots * 64];          // f16x3: hi | lo fragments; exact: fp32 steps
    // The view MLP's weights are staged in LDS although it runs once per ray
    // outside the SA forms: read from global memory (L2) instead, a block's
    // LDS drops from 45 to 33 KiB and 4 blocks share a CU, but the 4-wave form
    // (128 VGPRs, 12 dwords spilled) measured slower, 0.735 -> 0.75 ms per
    // view (profiles/r5_final_vg4_ab.txt; a build switch through round 6)
    __shared__ float Vl[kVTotal];
    __shared__ LevelDesc sLv[16];
    if (threadIdx.x < 16) sLv[threadIdx.x] = a.grid.lv[threadIdx.x];
    uint4* const Fh = Fbuf;
    uint4* const Fl = Fbuf + kFSlots * 64;
    float* const Fx = reinterpret_cast<float*>(Fbuf);
    if constexpr (EXACT) {
        for (int idx = threadIdx.x; idx < kXSteps * 64; idx += 256)
            Fx[idx] = grid_weight_exact(a, idx >> 6, idx & 63);
    } else {
        for (int idx = threadIdx.x; idx < 2 * kFSlots * 64; idx += 256) Fbuf[idx] = a.gpack[idx];
    }
    for (int idx = threadIdx.x; idx < kVTotal; idx += 256) Vl[idx] = view_weight(a, idx);
    // f16x3: log2 scales of the three weight tensors' fragments
    const int ke0 = EXACT ? 0 : a.gexp[0], ke1 = EXACT ? 0 : a.gexp[1], ke2 = EXACT ? 0 : a.gexp[2];
    __syncthreads();

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int hh = lane >> 5, jj = lane & 31;
    const int seg = jj / R;                              // slot of this column
    const uint32_t chunk = xcd_chunk(blockIdx.x, (a.N + 4u * R - 1u) / (4u * R));
    const uint32_t ray0 = chunk * (4u * R) + wave * (uint32_t)R;
    if (ray0 >= a.N) return;                             // wave-uniform
    const uint32_t r = ray0 + (uint32_t)(jj % R);        // this column's slot
    const bool live = r < a.N;
    const uint32_t rr = live ? r : a.N - 1;
    const bool sample_writer = live && hh == 0;          // u_out / w_out of this segment
    const bool writer = sample_writer && seg == 0;       // per-ray outputs
    const uint32_t N = a.N;
    const float2* __restrict__ emb = reinterpret_cast<const float2*>(a.grid_emb);

    float o[3], d[3];
    {
        const uint32_t ray = a.tiles(rr);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            o[c] = a.rays_o[(size_t)ray * 3 + c];
            d[c] = a.rays_d[(size_t)ray * 3 + c];
        }
    }
    const float sn = a.snf[rr], sf = a.snf[N + rr];
    float rb_prev = real_bin(sn, sf, a.bins_in[(size_t)seg * N + rr]);
    double cum = 0.0, wsum = 0.0, depth = 0.0;            // cum: optical depth before this step
    float fg[8];                                          // sum_k w_k * grid_mlp rows (acc layout)
#pragma unroll
    for (int q = 0; q < 8; ++q) fg[q] = 0.0f;
    float sh[16];                                         // SH(4) of the normalised direction
    auto sh_of_ray = [&]() {
        float dx = d[0], dy = d[1], dz = d[2];
        normalize3(dx, dy, dz);
        normalize3(dx, dy, dz);
        sh_values<4>(dx, dy, dz, sh);
    };
    float rgb[3] = {0.0f, 0.0f, 0.0f};                    // SA: sum_k w_k * view_mlp(colour_k)
    if constexpr (SA) sh_of_ray();
    // AD: sum_k w_k x_k of the adaptive heads' inputs, this lane's components
    float gacc[AD ? 16 : 1], h1acc[AD ? 32 : 1], h2acc[AD ? 32 : 1], v1acc[AD == 2 ? 16 : 1],
        v2acc[AD == 2 ? 16 : 1];
    if constexpr (AD > 0) {
#pragma unroll
        for (int q = 0; q < 16; ++q) gacc[q] = 0.0f;
#pragma unroll
        for (int q = 0; q < 32; ++q) h1acc[q] = h2acc[q] = 0.0f;
    }
    if constexpr (AD == 2) {
#pragma unroll
        for (int q = 0; q < 16; ++q) v1acc[q] = v2acc[q] = 0.0f;
    }

    // level descriptors of k-block kb for this half-wave (LDS reads,
    // re-evaluated where used rather than held in VGPRs)
    auto levels = [&](int kb, LevelDesc* dl) {
#pragma unroll
        for (int q = 0; q < 4; ++q) dl[q] = sLv[final_level(kb, hh, q)];
    };
    // wave-uniform slot classes (kernel arguments)
    auto kinds = [&](int kb) {
        if constexpr (LAY == 1) return SlotKinds{kLay1Dense[kb], kLay1Hashed[kb]};
        else return SlotKinds{a.kdense[kb], a.khashed[kb]};
    };
    // grid-space coordinate (LAY 1: the host checked inv_b2 != 0)
    auto gscale = [&](float x) { return LAY == 1 ? (x + a.gs.bound) * a.gs.inv_b2 : a.gs(x); };
    // rb_prev of sample i is rb_next of sample i - 1 when S == 1 (same bits;
    // saves a division), recomputed from the bins otherwise
    // the sample's position from its two raw bins (b0 read only when S > 1:
    // for S == 1 rbp is the previous sample's rbn, or the pre-loop rb_prev)
    auto position_of = [&](int i, float b0, float b1, float& rbp, float& rbn, float& ux, float& uy,
                           float& uz) {
        const int k = i * S + seg;
        if (S > 1) rbp = real_bin(sn, sf, b0);
        rbn = real_bin(sn, sf, b1);
        const float t = (rbn + rbp) / 2.0f;
        float x = o[0] + d[0] * t, y = o[1] + d[1] * t, z = o[2] + d[2] * t;
        contract3(x, y, z);
        ux = gscale(x);
        uy = gscale(y);
        uz = gscale(z);
    };
    // the sample's positions for k_sgrid (stored after its first gathers are
    // issued: the stores share vmcnt with the loads, so stores issued first
    // would hold up the first gather's consumption by their write latency)
    auto store_position = [&](int i, float ux, float uy, float uz) {
        const int k = i * S + seg;
        if (sample_writer) {
            a.u_out[((size_t)k * 3 + 0) * N + r] = ux;
            a.u_out[((size_t)k * 3 + 1) * N + r] = uy;
            a.u_out[((size_t)k * 3 + 2) * N + r] = uz;
        }
    };
    auto position = [&](int i, float& rbp, float& rbn, float& ux, float& uy, float& uz) {
        const int k = i * S + seg;
        position_of(i, S > 1 ? a.bins_in[(size_t)k * N + rr] : 0.0f, a.bins_in[(size_t)(k + 1) * N + rr], rbp,
                    rbn, ux, uy, uz);
    };
    // the next sample's raw bins are loaded one sample ahead, so the gathers
    // of a sample start without a dependent global load in front (the load
    // of sample i + 1's bins is in flight behind sample i's work)
    float nb0 = 0.0f, nb1 = 0.0f;
    {
        if (S > 1) nb0 = a.bins_in[(size_t)seg * N + rr];
        nb1 = a.bins_in[(size_t)(seg + 1) * N + rr];
    }

    int exit_at = TS;                                     // EXIT: first step not marched
    // 'last_sample': the last sample's delta * sigma is +inf (renderer.py:314);
    // transparent: no sample's is (k_inf = -1).  Wave-uniform, from a kernel
    // argument: a scalar register compared in place of the constant T - 1.
    const int k_inf = a.last_inf ? T - 1 : -1;
    for (int i = 0; i < TS; ++i) {
        const int k = i * S + seg;
        float rb_next, ux, uy, uz;
        {
            const float b0 = nb0, b1 = nb1;
            if (i + 1 < TS) {
                const int kn = (i + 1) * S + seg;
                if (S > 1) nb0 = a.bins_in[(size_t)kn * N + rr];
                nb1 = a.bins_in[(size_t)(kn + 1) * N + rr];
            }
            position_of(i, b0, b1, rb_prev, rb_next, ux, uy, uz);
        }
        const float t = (rb_next + rb_prev) / 2.0f;
        // weight fragments are re-read from LDS each sample rather than
        // hoisted into VGPRs for the whole loop (opaque offset defeats LICM)
        int wo = lane;
        asm volatile("" : "+v"(wo));
        const uint4* FH = Fh + wo;
        const uint4* FL = Fl + wo;
        const float* FX = Fx + wo;

        floatx16 h1a = {}, h1b = {};
        float fk[AD ? 16 : 1];                           // AD: this sample's grid features (by k-block)
        // f16x3 (f16x3.h): each layer's B operands are scaled by the power of
        // two that puts the sample column's max |input| in [2^13, 2^14);
        // e_h1 / e_h2 / e_o3 = log2 of the factor a layer's accumulators carry
        // over the true values (input scales + weight-tensor scales).  Layer 1
        // (round 5) gathers both k-blocks first and takes ONE scale from the
        // column's max over all 32 inputs (16 levels x 2 channels): the dense
        // and hashed levels share it, so a level far below the column max keeps
        // fewer significant bits in its fp16 halves -- down to 2^-27 of the max
        // it stays normal fp16, and the f16x3 products stay within the error
        // bound of an exact fp32 GEMM
        // (tests/test_gpu_render.py::test_final_joint_scale_over_wide_level_ranges
        // against the exact-fp32 form on levels 2^-20 .. 1 apart).  The
        // one-block-at-a-time form (the second block rescaled the accumulators
        // by an exact power of two when its max needed a scale two or more
        // binades lower; fp32-equivalent too, other bits) held layer 1's 32
        // accumulators through the second gather; a build switch through
        // round 6.
        int k1 = 0, e_h1 = 0, e_h2 = 0;
        // this half-wave's 8 features of k-block kb (levels 8 kb + hh + 2 q)
        auto gather_kb = [&](int kb, float* f, bool first) {
            LevelDesc dl[4];
            levels(kb, dl);
            uint32_t* rt = nullptr;                      // parity taps only
            if (TAP && a.rows_tap && live && r % a.tap_stride == 0u)
                rt = a.rows_tap + ((size_t)(r / a.tap_stride) * T + k) * 128u + (8 * kb + hh) * 8;
            GatherC2<4> g;
            HashSlots hs;
            if constexpr (LAY == 1) {
#pragma unroll
                for (int q = 0; q < 4; ++q) hs.base[q] = reinterpret_cast<const char*>(a.grid_emb) + a.hoff8[kb][q];
                hs.hx = hh ? a.hbit : 0u;
                hs.m8 = a.hm8;
            }
            gather_issue_c2<4>(emb, dl, ux, uy, uz, g, kinds(kb), rt, 16, LAY == 1 ? &hs : nullptr);
            if (first) store_position(i, ux, uy, uz);
            gather_finish_c2<4, S == 1>(g, f);
        };
        if constexpr (EXACT) {
#pragma unroll
            for (int kbi = 0; kbi < 2; ++kbi) {
                // k-block 1 (levels 8-15) first, then 0: the accumulation order
                // of every round (a cross-sample prefetch of k-block 1 set it)
                const int kb = 1 - kbi;
                float f[8];
                gather_kb(kb, f, kbi == 0);
                if constexpr (AD > 0) {
#pragma unroll
                    for (int m = 0; m < 8; ++m) fk[kb * 8 + m] = f[m];
                }
#pragma unroll
                for (int m = 0; m < 8; ++m) {
                    h1a = MFMA32(FX[(kb * 8 + m) * 64], f[m], h1a);
                    h1b = MFMA32(FX[(16 + kb * 8 + m) * 64], f[m], h1b);
                }
            }
        } else {
            // f16x3, layer 1 in one piece: both k-blocks gathered first --
            // k-block 0 (the dense pair loads, 24 loads) before k-block 1 (32),
            // so only its 8 features wait through the second gather -- then
            // ONE scale from the column's max over all 32 inputs, and the 12
            // MFMAs in the k-block 1, 0 order of every round
            float f0[8], f1[8];
            gather_kb(0, f0, true);
            gather_kb(1, f1, false);
            if constexpr (AD > 0) {
#pragma unroll
                for (int m = 0; m < 8; ++m) {
                    fk[m] = f0[m];
                    fk[8 + m] = f1[m];
                }
            }
            float m = 0.0f;
#pragma unroll
            for (int e = 0; e < 8; e += 2) m = max_abs3(max_abs3(m, f0[e], f0[e + 1]), f1[e], f1[e + 1]);
            k1 = scale_exp_of_max(max_halves(m));
            const float sc = exp2i(k1);
            uint4 bh, bl;
            split8_f16(f1, sc, bh, bl);
            h1a = mfma_f16x3(FH[(kF1 + 2) * 64], FL[(kF1 + 2) * 64], bh, bl, h1a);
            h1b = mfma_f16x3(FH[(kF1 + 3) * 64], FL[(kF1 + 3) * 64], bh, bl, h1b);
            split8_f16(f0, sc, bh, bl);
            h1a = mfma_f16x3(FH[kF1 * 64], FL[kF1 * 64], bh, bl, h1a);
            h1b = mfma_f16x3(FH[(kF1 + 1) * 64], FL[(kF1 + 1) * 64], bh, bl, h1b);
        }
        if constexpr (!EXACT) e_h1 = k1 + ke0;
        float s2 = 1.0f;
        if constexpr (!EXACT) {                          // max of relu(h1): the raw max, floored at 0
            int mb = 0;                                  // max of relu(h1) on the float bits
#pragma unroll
            for (int i = 0; i < 16; ++i) mb = max_relu3(mb, h1a[i], h1b[i]);
            const float m = max_halves(__builtin_bit_cast(float, mb));
            const int k2 = scale_exp_of_max(m);
            s2 = exp2i(k2);
            e_h2 = e_h1 + k2 + ke1;
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            h1a[i] = relu_bits(h1a[i]);
            h1b[i] = relu_bits(h1b[i]);
        }
        floatx16 h2a = {}, h2b = {};
        if constexpr (EXACT) {
#pragma unroll
            for (int t = 0; t < 2; ++t) {
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    const float v = t ? h1b[q] : h1a[q];
                    h2a = MFMA32(FX[(32 + t * 16 + q) * 64], v, h2a);
                    h2b = MFMA32(FX[(64 + t * 16 + q) * 64], v, h2b);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        } else {
#pragma unroll
            for (int kb = 0; kb < 4; ++kb) {
                float v[8];
#pragma unroll
                for (int m = 0; m < 8; ++m) v[m] = (kb >> 1) ? h1b[8 * (kb & 1) + m] : h1a[8 * (kb & 1) + m];
                uint4 bh, bl;
                split8_f16(v, s2, bh, bl);
                h2a = mfma_f16x3(FH[(kF2 + 2 * kb) * 64], FL[(kF2 + 2 * kb) * 64], bh, bl, h2a);
                h2b = mfma_f16x3(FH[(kF2 + 2 * kb + 1) * 64], FL[(kF2 + 2 * kb + 1) * 64], bh, bl, h2b);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        float s3 = 1.0f;
        int e_o3 = 0;
        if constexpr (!EXACT) {
            int mb = 0;
#pragma unroll
            for (int i = 0; i < 16; ++i) mb = max_relu3(mb, h2a[i], h2b[i]);
            const float m = max_halves(__builtin_bit_cast(float, mb));
            const int k3 = scale_exp_of_max(m);
            s3 = exp2i(k3);
            e_o3 = e_h2 + k3 + ke2;
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            h2a[i] = relu_bits(h2a[i]);
            h2b[i] = relu_bits(h2b[i]);
        }
        floatx16 o3 = {};
        if constexpr (EXACT) {
#pragma unroll
            for (int t = 0; t < 2; ++t) {
#pragma unroll
                for (int q = 0; q < 16; ++q) o3 = MFMA32(FX[(96 + t * 16 + q) * 64], t ? h2b[q] : h2a[q], o3);
                __builtin_amdgcn_sched_barrier(0);
            }
        } else {
#pragma unroll
            for (int kb = 0; kb < 4; ++kb) {
                float v[8];
#pragma unroll
                for (int m = 0; m < 8; ++m) v[m] = (kb >> 1) ? h2b[8 * (kb & 1) + m] : h2a[8 * (kb & 1) + m];
                uint4 bh, bl;
                split8_f16(v, s3, bh, bl);
                o3 = mfma_f16x3(FH[(kF3 + kb) * 64], FL[(kF3 + kb) * 64], bh, bl, o3);
                __builtin_amdgcn_sched_barrier(0);
            }
            // back to the true outputs (rows 0..15 = registers 0..7 of both halves)
            const float inv = exp2i(-e_o3);
#pragma unroll
            for (int q = 0; q < 8; ++q) o3[q] = o3[q] * inv;
        }

        // sigma pre-activation = row 0, held by the lower half-wave
        float s_lo, s_hi;
        halves(o3[0], s_lo, s_hi);                       // s_lo: row 0 of this column in both halves
        // expf, not __expf: the fast form measured 2 % faster on k_final but
        // changes the bits (a build switch
        // through round 6)
        const float sigma = expf(s_lo);
        // composite (renderer.py:300-307): w_k = alpha_k * exp(-sum_{j<k} ds_j),
        // the sum in double and in sample order across the ray's S slots
        const float ds = k == k_inf ? INFINITY : (rb_next - rb_prev) * sigma;
        double before = cum;
#pragma unroll
        for (int s2 = 0; s2 < S; ++s2) {
            const float d2 = S > 1 ? __shfl(ds, (jj % R) + R * s2 + 32 * hh) : ds;
            if (s2 < seg) before += (double)d2;
            cum += (double)d2;
        }
        const float w = nan_to_num((1.0f - expf(-ds)) * expf(-(float)before));
        if (sample_writer) a.w_out[(size_t)k * N + r] = w;
        if (TAP && a.sigma_tap && sample_writer) a.sigma_tap[(size_t)k * N + r] = sigma;
        wsum += (double)w;
        depth += (double)(w * t);
#pragma unroll
        for (int q = 0; q < 8; ++q) fg[q] = fg[q] + w * o3[q];
        if constexpr (AD > 0) {
#pragma unroll
            for (int m = 0; m < 16; ++m) gacc[m] = gacc[m] + w * fk[m];
            // f16x3: the accumulators carry 2^e_h1 / 2^e_h2 (w * 2^-e is exact)
            const float w1 = EXACT ? w : w * exp2i(-e_h1), w2 = EXACT ? w : w * exp2i(-e_h2);
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                h1acc[q] = h1acc[q] + w1 * h1a[q];
                h1acc[16 + q] = h1acc[16 + q] + w1 * h1b[q];
                h2acc[q] = h2acc[q] + w2 * h2a[q];
                h2acc[16 + q] = h2acc[16 + q] + w2 * h2b[q];
            }
        }
        if (GEO && live) {                               // rows rho(q) + 4 hh of this sample
#pragma unroll
            for (int q = 0; q < 8; ++q) a.geo_out[((size_t)k * 16 + rho(q) + 4 * hh) * N + r] = o3[q];
        }
        if constexpr (SA) {                              // view MLP on this sample's colour
            floatx16 p1 = {};
#pragma unroll
            for (int q = 0; q < 8; ++q) p1 = MFMA32(Vl[kV1 + q * 64 + lane], o3[q], p1);
#pragma unroll
            for (int s2 = 0; s2 < 8; ++s2) p1 = MFMA32(Vl[kV1 + (8 + s2) * 64 + lane], sh[2 * s2 + hh], p1);
#pragma unroll
            for (int q = 0; q < 16; ++q) p1[q] = relu_bits(p1[q]);
            floatx16 p2 = {};
#pragma unroll
            for (int q = 0; q < 16; ++q) p2 = MFMA32(Vl[kV2 + q * 64 + lane], p1[q], p2);
#pragma unroll
            for (int q = 0; q < 16; ++q) p2[q] = relu_bits(p2[q]);
            floatx16 p3 = {};
#pragma unroll
            for (int q = 0; q < 16; ++q) p3 = MFMA32(Vl[kV3 + q * 64 + lane], p2[q], p3);
#pragma unroll
            for (int c = 0; c < 3; ++c) rgb[c] = rgb[c] + w * p3[c];   // rows 0..2, lower half
            if constexpr (AD == 2) {                     // view_mlp intermediates (post-ReLU)
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    v1acc[q] = v1acc[q] + w * p1[q];
                    v2acc[q] = v2acc[q] + w * p2[q];
                }
            }
        }
        rb_prev = rb_next;
        // N1 early exit: once the transmittance of every ray of the wave is
        // below t_thresh, the samples left (whose weights sum to that
        // transmittance, the last one absorbing the rest) are dropped: their
        // weights are stored as 0 (k_sgrid skips all-zero samples) and their
        // positions as the grid centre (in range for any gather).  Nothing of
        // the sample is held past its MFMAs for this (holding the position
        // spilled 16 more VGPRs at 3 waves per SIMD).
        if (EXIT && i + 1 < TS) {
            const bool open = live && !(cum > (double)a.exit_depth);
            if (__builtin_amdgcn_ballot_w64(open) == 0) {
                exit_at = i + 1;
                break;
            }
        }
    }
    if (EXIT && sample_writer) {
        for (int i2 = exit_at; i2 < TS; ++i2) {
            const int k2 = i2 * S + seg;
            a.w_out[(size_t)k2 * N + r] = 0.0f;
            a.u_out[((size_t)k2 * 3 + 0) * N + r] = 0.5f;
            a.u_out[((size_t)k2 * 3 + 1) * N + r] = 0.5f;
            a.u_out[((size_t)k2 * 3 + 2) * N + r] = 0.5f;
        }
    }

    if constexpr (S > 1) {                               // add the slots' partial sums
        double pw = 0.0, pd = 0.0;
        float pf[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) pf[q] = 0.0f;
#pragma unroll
        for (int s2 = 0; s2 < S; ++s2) {
            const int src = (jj % R) + R * s2 + 32 * hh;
            pw += __shfl(wsum, src);
            pd += __shfl(depth, src);
#pragma unroll
            for (int q = 0; q < 8; ++q) pf[q] += __shfl(fg[q], src);
        }
        wsum = pw;
        depth = pd;
#pragma unroll
        for (int q = 0; q < 8; ++q) fg[q] = pf[q];
        if constexpr (SA) {
            float pr[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int s2 = 0; s2 < S; ++s2) {
                const int src = (jj % R) + R * s2 + 32 * hh;
#pragma unroll
                for (int c = 0; c < 3; ++c) pr[c] += __shfl(rgb[c], src);
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) rgb[c] = pr[c];
        }
    }

    // view MLP on the accumulated colour features: rows 1..15 of fg are
    // f_image[0..14] (geo), f_image[15..30] = sh * sum(w) (colour = cat(geo, sh)
    // with sh constant along the ray, renderer.py:338; a rounding-level
    // reassociation of the reference's sum of products)
    if constexpr (!SA) sh_of_ray();
    const float ws = (float)wsum, dp = (float)depth;
    floatx16 v3 = {};
    if constexpr (!SA) {
        floatx16 v1 = {};
#pragma unroll
        for (int q = 0; q < 8; ++q) v1 = MFMA32(Vl[kV1 + q * 64 + lane], fg[q], v1);
#pragma unroll
        for (int s = 0; s < 8; ++s) v1 = MFMA32(Vl[kV1 + (8 + s) * 64 + lane], sh[2 * s + hh] * ws, v1);
#pragma unroll
        for (int i = 0; i < 16; ++i) v1[i] = relu_bits(v1[i]);
        floatx16 v2 = {};
#pragma unroll
        for (int q = 0; q < 16; ++q) v2 = MFMA32(Vl[kV2 + q * 64 + lane], v1[q], v2);
#pragma unroll
        for (int i = 0; i < 16; ++i) v2[i] = relu_bits(v2[i]);
#pragma unroll
        for (int q = 0; q < 16; ++q) v3 = MFMA32(Vl[kV3 + q * 64 + lane], v2[q], v3);
    }

    if constexpr (AD > 0) {
        // instance_mask_logits[c] = E[c] . sums: this lane's components, then
        // the other half-wave's (lane ^ 32 holds the ray's other rows)
        const uint32_t K = a.mask_out;
        for (uint32_t c = 0; c < K; ++c) {
            const float* E = a.aeff + (size_t)c * kAeff;
            float sacc = 0.0f;
#pragma unroll
            for (int m = 0; m < 16; ++m)
                sacc += E[2 * final_level(m >> 3, hh, (m & 7) >> 1) + (m & 1)] * gacc[m];
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int u = rho(q) + 4 * hh;
                sacc += E[32 + u] * h1acc[q] + E[64 + u] * h1acc[16 + q];
                sacc += E[96 + u] * h2acc[q] + E[128 + u] * h2acc[16 + q];
                if constexpr (AD == 2) sacc += E[176 + u] * v1acc[q] + E[208 + u] * v2acc[q];
            }
#pragma unroll
            for (int q = 0; q < 8; ++q) sacc += E[160 + rho(q) + 4 * hh] * fg[q];
            sacc = sum_halves(sacc);
            if (live && hh == 0) a.mlog[(size_t)a.tiles(r) * K + c] = sacc;
        }
        if (live && a.xsum) {                            // this lane's components of X (training)
            float* X = a.xsum + (size_t)a.tiles(r) * kAeff;
#pragma unroll
            for (int m = 0; m < 16; ++m) X[2 * final_level(m >> 3, hh, (m & 7) >> 1) + (m & 1)] = gacc[m];
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int u = rho(q) + 4 * hh;
                X[32 + u] = h1acc[q];
                X[64 + u] = h1acc[16 + q];
                X[96 + u] = h2acc[q];
                X[128 + u] = h2acc[16 + q];
                if constexpr (AD == 2) {
                    X[176 + u] = v1acc[q];
                    X[208 + u] = v2acc[q];
                }
            }
#pragma unroll
            for (int q = 0; q < 8; ++q) X[160 + rho(q) + 4 * hh] = fg[q];
        }
    }
    if (!live || seg != 0) return;
    const uint32_t ray = a.tiles(r);                     // per-ray outputs in ray order
    float* row = a.rows ? a.rows + (size_t)ray * kRow : nullptr;
    if (row) {                                 // geo units owned by this half-wave
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int unit = rho(q) + 4 * hh;
            if (unit >= 1) row[128 + unit - 1] = fg[q];
        }
    }
    if (hh != 0) return;
    float img[3];
    // the background colour of this RAY (not slot: view_width tiling permutes
    // them): one colour for all (n_bg = 1), one per ray, or the scalar
    const float* bgp = a.bg_rgb ? a.bg_rgb + (size_t)(a.n_bg == 1u ? 0u : ray) * 3 : nullptr;
    // the scalar as a value before the choice: `bgp ? bgp[c] : a.bg` becomes
    // one load through a select of the two ADDRESSES, the argument struct's
    // own among them, and the whole struct is then copied to scratch (~900
    // bytes per lane in every form of the kernel)
    const float bg0 = a.bg;
#pragma unroll
    for (int c = 0; c < 3; ++c) {                // rows 0..2 of v3 = registers 0..2, lower half
        const float bg_c = bgp ? bgp[c] : bg0;
        img[c] = sigmoidf(SA ? rgb[c] : v3[c]) + (1.0f - ws) * bg_c;
        a.image[(size_t)ray * a.img_ld + c] = img[c];
    }
    a.depth[(size_t)ray * a.scal_ld] = dp;
    a.wsum[(size_t)ray * a.scal_ld] = ws;
    if (row) {
#pragma unroll
        for (int i = 0; i < 16; ++i) row[143 + i] = sh[i] * ws;
        row[159] = img[0];
        row[160] = img[1];
        row[161] = img[2];
        row[162] = dp;
        row[163] = 0.0f;
    }
}

// k_final's cross-sample prefetch of k-block 1's gathers (rounds 1-3, a
// diagnostic form only since round 2: for S = 1 three waves per SIMD without
// it beat two with it, 0.797 vs 0.826 ms per view; for S = 2 / 4 it spilled,
// 0.288 vs 0.260 ms at 32,768 rays) was removed in round 4: its f16x3 forms
// rendered one sample of one 16-lane group differently in about one launch in
// four, mostly the first of a process (|d sigma| up to 7e-3 relative; the
// exact-fp32 prefetch form and every product form bit-stable over the same
// runs; not traced to a cause -- tools/pf_diag.py).
// k_final's wave-uniform slot paths (dense pair loads, select-free hashed
// rows): on by default; SAMNERF_FINAL_CLASSES=0 takes the lane-varying form
// everywhere (same bits: the A/B parity test).
uint32_t final_classes() {
    const char* v = diag_env("SAMNERF_FINAL_CLASSES");
    return (v && atoi(v) == 0) ? 0u : 1u;
}

// k_final's LAY (1: the reference grid's slot classes and a power-of-two
// grid scale, compile-time; 0: run time).  SAMNERF_FINAL_LAY=0 (diagnostic
// build) forces the run-time form, for the bit-identity test.
int final_layout(const FinalArgs& fa) {
    const char* v = diag_env("SAMNERF_FINAL_LAY");
    if (v && atoi(v) == 0) return 0;
    for (int kb = 0; kb < 2; ++kb)
        if (fa.kdense[kb] != kLay1Dense[kb] || fa.khashed[kb] != kLay1Hashed[kb]) return 0;
    if (fa.hbit == 0u) return 0;                      // hashed slots not laid out for HashSlots
    return fa.gs.inv_b2 != 0.0f ? 1 : 0;
}

// LAY 1's HashSlots layout (FinalArgs::hoff8 / hbit / hm8): every hashed slot
// holds two consecutive levels of one power-of-two size S (the reference's
// 2^19 hash tables) with res <= S; else hbit = 0 and LAY 1 is not used.
void set_hash_slots(FinalArgs& fa, const GridDesc<16>& g) {
    fa.hbit = fa.hm8 = 0u;
    uint32_t S = 0u;
    for (int kb = 0; kb < 2; ++kb)
        for (int q = 0; q < 4; ++q) {
            fa.hoff8[kb][q] = 0u;
            if (!((fa.khashed[kb] >> q) & 1u)) continue;
            const LevelDesc& a = g.lv[final_level(kb, 0, q)];
            const LevelDesc& b = g.lv[final_level(kb, 1, q)];
            if (!S) S = a.size;
            if (a.size != S || b.size != S || (S & (S - 1u)) || b.off != a.off + S || a.res > S || b.res > S ||
                (uint64_t)S * 8u > (1ull << 31) || (uint64_t)b.off * 8u >= (1ull << 32))
                return;                               // (hoff8 is a 32-bit byte offset)
            fa.hoff8[kb][q] = a.off * 8u;
        }
    if (!S) return;
    fa.hbit = S * 8u;
    fa.hm8 = (S - 1u) * 8u;
}

// The adaptive mask heads (network.py:143-191, renderer.py:399-434) are
// chains of bias-free Linears on concatenations [intermediate ; m]: linear in
// the per-sample inputs, so sum_k w_k head(x_k) = E . sum_k w_k x_k with E the
// product of the chain, K x 240 (blocks g 32 | h1 64 | h2 64 | o3 16 | v1 32 |
// v2 32).  One block multiplies it out from the output layer back:
// P = W_last W_prev, then per concatenating layer [A | B]: E_block = P A,
// P = P B.  (A reassociation of the reference's layer-by-layer products:
// rounding-level differences.)
struct EffArgs {
    const float* w[8];
    uint32_t K;
    int kind;          // 1 density (6 layers), 2 rgb (8 layers)
    float* aeff;
};

__global__ void __launch_bounds__(256) k_mask_eff(EffArgs a) {
    __shared__ float P[2][32 * 96];
    const int tid = threadIdx.x;
    const int K = (int)a.K, nl = a.kind == 2 ? 8 : 6;
    int cur = 0;
    for (int e = tid; e < K * 96; e += 256) P[0][e] = a.w[nl - 1][e];
    __syncthreads();
    // out[r][c] = sum_i P[r][i] W[i][c0 + c] (W: 96 rows of `ld` columns)
    auto mul = [&](const float* W, int ld, int c0, int nc, float* out, int out_ld) {
        for (int e = tid; e < K * nc; e += 256) {
            const int r = e / nc, c = e % nc;
            float acc = 0.0f;
            for (int i = 0; i < 96; ++i) acc = __builtin_fmaf(P[cur][r * 96 + i], W[i * ld + c0 + c], acc);
            out[r * out_ld + c] = acc;
        }
        __syncthreads();
    };
    auto next = [&](const float* W, int ld, int c0) {
        mul(W, ld, c0, 96, P[cur ^ 1], 96);
        cur ^= 1;
    };
    float* E = a.aeff;
    next(a.w[nl - 2], 96, 0);                            // P = W_last W_{last-1}
    if (a.kind == 2) {
        mul(a.w[5], 128, 0, 32, E + 208, kAeff);         // [v2 | m4]
        next(a.w[5], 128, 32);
        mul(a.w[4], 128, 0, 32, E + 176, kAeff);         // [v1 | m3]
        next(a.w[4], 128, 32);
    } else {
        for (int e = tid; e < K * 64; e += 256) E[(e / 64) * kAeff + 176 + e % 64] = 0.0f;
    }
    mul(a.w[3], 112, 0, 16, E + 160, kAeff);             // [o3 | m2]
    next(a.w[3], 112, 16);
    mul(a.w[2], 160, 0, 64, E + 96, kAeff);              // [h2 | m1]
    next(a.w[2], 160, 64);
    mul(a.w[1], 160, 0, 64, E + 32, kAeff);              // [h1 | m0]
    next(a.w[1], 160, 64);
    mul(a.w[0], 32, 0, 32, E, kAeff);                    // m0 = W0 g
}

// One k_final instantiation over N rays in S segments each (32 / S rays per
// wave, 4 waves per block).
template <int S, bool EXACT, bool EXIT = false, bool GEO = false, bool SA = false, int AD = 0, int LAY = 0,
          bool TAP = true>
void launch_k_final(uint32_t N, hipStream_t s, const FinalArgs& fa) {
    k_final<32, S, EXACT, EXIT, GEO, SA, AD, LAY, TAP><<<xcd_blocks(div_up(N, 128 / S)), 256, 0, s>>>(fa);
}

// The run-time layout (LAY 0, taps compiled in) by segment count.
template <bool EXACT, bool EXIT, bool GEO, bool SA>
void launch_final_lay0(int seg, uint32_t N, hipStream_t s, const FinalArgs& fa) {
    if (seg == 1) launch_k_final<1, EXACT, EXIT, GEO, SA>(N, s, fa);
    else if (seg == 2) launch_k_final<2, EXACT, EXIT, GEO, SA>(N, s, fa);
    else launch_k_final<4, EXACT, EXIT, GEO, SA>(N, s, fa);
}

// LAY 1 without taps, the product form of a reference-shaped grid.
template <int S, bool EXACT, bool GEO = false, bool SA = false, int AD = 0>
void launch_final_lay1(uint32_t N, hipStream_t s, const FinalArgs& fa) {
    launch_k_final<S, EXACT, false, GEO, SA, AD, 1, false>(N, s, fa);
}

// k_final's form for this render; EXACT = the exact-fp32 grid_mlp of head_mode
// 1.  LAY 1 (the reference grid's compile-time slot layout) wherever the grid
// matches it; the taps' forms keep the run-time layout, except the plain S = 1
// form (the taps' renders are whole views), which has a LAY 1 tap form.
// Returns the layout launched (samnerf_last_forms [2]).
template <bool EXACT>
uint32_t launch_final(int seg, uint32_t N, hipStream_t s, const FinalArgs& fa, bool sa, int ad) {
    const bool tap = fa.sigma_tap || fa.rows_tap;
    const bool lay = final_layout(fa) == 1;
    const bool lay1 = lay && !tap;
    if (ad) {                                            // adaptive mask heads: S = 1
        if (ad == 2) {
            if (lay1) launch_final_lay1<1, EXACT, false, true, 2>(N, s, fa);
            else launch_k_final<1, EXACT, false, false, true, 2>(N, s, fa);
        } else if (sa) {
            if (lay1) launch_final_lay1<1, EXACT, false, true, 1>(N, s, fa);
            else launch_k_final<1, EXACT, false, false, true, 1>(N, s, fa);
        } else {
            if (lay1) launch_final_lay1<1, EXACT, false, false, 1>(N, s, fa);
            else launch_k_final<1, EXACT, false, false, false, 1>(N, s, fa);
        }
        return lay1 ? 1u : 0u;
    }
    if (sa) {                                            // --sum_after_mlp (RGB / mask models)
        if (fa.geo_out) launch_final_lay0<EXACT, false, true, true>(seg, N, s, fa);
        else launch_final_lay0<EXACT, false, false, true>(seg, N, s, fa);
        return 0u;
    }
    if (fa.geo_out) {                                    // mask model: geo_feat per sample
        if (seg == 1 && lay1) {
            launch_final_lay1<1, EXACT, true>(N, s, fa);
            return 1u;
        }
        launch_final_lay0<EXACT, false, true, false>(seg, N, s, fa);
        return 0u;
    }
    // N1: the wave-level exit.  Compacting the open rays between passes over
    // sample chunks measured slower on the opaque-sphere 512^2 view: k_final
    // 0.97 ms in one pass, 1.37 ms in 2, 1.53 ms in 4
    // (profiles/r3_n1_compaction.txt).
    if (fa.exit_depth < INFINITY) {
        launch_final_lay0<EXACT, true, false, false>(seg, N, s, fa);
        return 0u;
    }
    if (lay1) {                                          // the plain forms
        if (seg == 1) launch_final_lay1<1, EXACT>(N, s, fa);
        else if (seg == 2) launch_final_lay1<2, EXACT>(N, s, fa);
        else launch_final_lay1<4, EXACT>(N, s, fa);
        return 1u;
    }
    if (lay && seg == 1) {
        launch_k_final<1, EXACT, false, false, false, 0, 1, true>(N, s, fa);
        return 1u;
    }
    launch_final_lay0<EXACT, false, false, false>(seg, N, s, fa);
    return 0u;
}

}  // namespace

namespace samnerf {

int run_final(const samnerf_model* m, uint32_t N, const FinalRun& r, const Workspace& w, hipStream_t s,
              uint32_t& form) {
    FinalArgs fa{};
    fa.rays_o = r.rays_o;
    fa.rays_d = r.rays_d;
    fa.N = N;
    fa.tiles = r.tiles;
    fa.gs = make_grid_scale(m->grid_bound);
    fa.bg = r.bg;
    fa.bg_rgb = r.bg_rgb;
    fa.n_bg = r.n_bg;
    fa.last_inf = current_background().background == 0 ? 1u : 0u;
    fa.grid = r.grid;
    fa.grid_emb = r.grid.emb;
    const GridDesc<16>& gg = r.grid;
    // slot q of k-block kb holds levels final_level(kb, 0 / 1, q): dense in
    // both half-waves -> pair loads, hashed in both -> select-free rows
    for (int kb = 0; kb < 2; ++kb) {
        fa.kdense[kb] = fa.khashed[kb] = 0u;
        for (int q = 0; q < 4 && final_classes(); ++q) {
            const bool ha = gg.lv[final_level(kb, 0, q)].flags & kHashed;
            const bool hb = gg.lv[final_level(kb, 1, q)].flags & kHashed;
            fa.kdense[kb] |= (!ha && !hb) ? 1u << q : 0u;
            fa.khashed[kb] |= (ha && hb) ? 1u << q : 0u;
        }
    }
    set_hash_slots(fa, gg);
    fa.G0 = m->grid_mlp[0];
    fa.G1 = m->grid_mlp[1];
    fa.G2 = m->grid_mlp[2];
    fa.V0 = m->view_mlp[0];
    fa.V1 = m->view_mlp[1];
    fa.V2 = m->view_mlp[2];
    fa.bins_in = r.bins_in;
    fa.snf = w.snf;
    fa.u_out = w.u_f;
    fa.w_out = w.w_f;
    fa.image = r.image;
    fa.depth = r.depth;
    fa.wsum = r.wsum;
    fa.img_ld = r.img_ld;
    fa.scal_ld = r.scal_ld;
    fa.exit_depth = m->t_thresh > 0.0f ? -logf(m->t_thresh) : INFINITY;
    fa.sigma_tap = r.sigma_tap;
    fa.rows_tap = r.rows_tap;
    fa.tap_stride = r.tap_stride;
    int ad = 0;
    if (m->with_mask) {
        if (m->t_thresh > 0.0f)
            return fail(SAMNERF_EINVAL, "render_forward: the mask head and t_thresh do not combine");
        if (m->mask_kind < 0 || m->mask_kind > 2)
            return fail(SAMNERF_EINVAL, "render_forward: mask_kind %d", m->mask_kind);
        if (m->mask_out < 1 || m->mask_out > 32)
            return fail(SAMNERF_EINVAL, "render_forward: mask_out %u outside 1..32", m->mask_out);
        const int nl = m->mask_kind == 0 ? 3 : m->mask_kind == 1 ? 6 : 8;
        for (int i = 0; i < nl; ++i)
            if (!m->mask_w[i]) return fail(SAMNERF_EINVAL, "render_forward: null mask_mlp weight %d", i);
        if (m->mask_kind == 0) {
            fa.geo_out = w.geo_f;
        } else {
            if (m->mask_kind == 2 && !m->sum_after_mlp)
                return fail(SAMNERF_EINVAL, "render_forward: the adaptive 'rgb' head needs sum_after_mlp");
            EffArgs ea{};
            for (int i = 0; i < nl; ++i) ea.w[i] = m->mask_w[i];
            ea.K = m->mask_out;
            ea.kind = m->mask_kind;
            ea.aeff = w.aeff;
            k_mask_eff<<<1, 256, 0, s>>>(ea);
            fa.aeff = w.aeff;
            fa.mlog = w.mlog;
            fa.xsum = m->with_mask == 2 ? w.xsum : nullptr;   // training render: the head's inputs
            fa.mask_out = m->mask_out;
            ad = m->mask_kind;
        }
    }
    fa.rows = r.rows;
    if (r.mark) r.mark(2, s);
    // segments per ray: enough waves to fill the resident slots (2 per SIMD)
    // (SAMNERF_FINAL_S = 1 | 2 | 4 overrides, for measurement)
    const char* fs = diag_env("SAMNERF_FINAL_S");
    const int seg = fs ? atoi(fs) : (N >= 65536u ? 1 : N >= 32768u ? 2 : 4);
    if (m->sum_after_mlp && (m->t_thresh > 0.0f || r.sam_rows))
        return fail(SAMNERF_EINVAL, "render_forward: sum_after_mlp renders RGB (+ mask) only: no SAM "
                    "features (the reference's branch crashes, SURVEY 0.2) and no t_thresh");
    if (m->head_mode == 1) {
        form = launch_final<true>(seg, N, s, fa, m->sum_after_mlp != 0, ad);
    } else {
        fa.gpack = w.gpack;
        fa.gexp = w.gexp;
        if (pack_weights(m)) k_pack_grid_mlp<<<1, 256, 0, s>>>(fa, w.gpack, w.gexp);
        form = launch_final<false>(seg, N, s, fa, m->sum_after_mlp != 0, ad);
    }
    return SAMNERF_OK;
}

}  // namespace samnerf
