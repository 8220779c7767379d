// sgrid.hip -- the s_grid stage of the fused render (the map of the pipeline
// is in raymarch.hip): the forward forms k_sgrid / k_sgrid_box4 with their
// choice (launch_sgrid), and the distillation step's backward with its
// deterministic variant.
#include <cstdlib>

#include "f16x3.h"
#include "render_args.h"
#include "samnerf_common.h"
#include "wave_box.h"

using namespace samnerf;

namespace {

struct SgridArgs {
    uint32_t N;
    RayTiles tiles;      // slot -> ray of the rows
    GridDesc<16> grid;
    const float* u_in;   // [T][3][N]
    const float* w_in;   // [T][N]
    float* rows;         // [N, kRow]
    // parity taps (samnerf_taps.srows; null in every product render): the
    // corner rows of every level of the samples of slots r % tap_stride == 0,
    // [N / tap_stride][T][16][8] (k_sgrid_box4)
    uint32_t* rows_tap;
    uint32_t tap_stride;
    // diagnostic build only (SAMNERF_SGRID_PATHS = hex device address of 8
    // uint64): per (wave, sample, level) of k_sgrid_box4, [0] uniform-cell,
    // [1] staged box, [2] direct gathers; [3] wave-samples skipped (all
    // weights 0); [4] box slots and [5] box cells of the staged boxes; null
    // in every other render
    unsigned long long* paths;
};

// f_sam = sum_k w_k * s_grid(x_k).  A block is one level x 64 neighbouring
// rays x 4 sample quarters: thread (q, ray) sums samples q*T/4 .. q*T/4 + T/4
// - 1 (its next sample's position/weight prefetched behind the current
// gather), and the quarters are added through LDS.  A wave is 64 rays at one
// (level, sample), so corner rows are shared across lanes.
// MODE: kLookPacked (lookup_level3), kLookRef (lookup_level3_ref, scalar
// accumulation); k_sgrid_box4 below is the de-duplicated form.  All give
// identical bits.

template <int T, int MODE>
__global__ void __launch_bounds__(256) k_sgrid(SgridArgs a) {
    constexpr int TQ = T / 4;
    __shared__ float part[3][8][64];
    const uint32_t lane = threadIdx.x & 63u, q = threadIdx.x >> 6;
    const uint32_t r = xcd_chunk(blockIdx.x, (a.N + 63u) / 64u) * 64u + lane;   // gridDim.x % 8 == 0
    const uint32_t level = blockIdx.y;
    const bool live = r < a.N;
    const uint32_t N = a.N, rr = live ? r : N - 1;
    const LevelDesc lv = a.grid.lv[level];
    float acc[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) acc[c] = 0.0f;
    const int k0 = (int)q * TQ;
    float ux = a.u_in[((size_t)k0 * 3 + 0) * N + rr];
    float uy = a.u_in[((size_t)k0 * 3 + 1) * N + rr];
    float uz = a.u_in[((size_t)k0 * 3 + 2) * N + rr];
    float w = a.w_in[(size_t)k0 * N + rr];
    for (int k = k0; k < k0 + TQ; ++k) {
        const int kn = k + 1 < k0 + TQ ? k + 1 : k;          // prefetch (clamped)
        const float nx = a.u_in[((size_t)kn * 3 + 0) * N + rr];
        const float ny = a.u_in[((size_t)kn * 3 + 1) * N + rr];
        const float nz = a.u_in[((size_t)kn * 3 + 2) * N + rr];
        const float nw = a.w_in[(size_t)kn * N + rr];
        float f[8];
        // a sample with weight 0 on every ray of the wave adds nothing (N1's
        // dropped samples; acc + 0 * f == acc for the finite features)
        if (__builtin_amdgcn_ballot_w64(w != 0.0f) == 0) {
        } else if constexpr (MODE == kLookRef) {
            lookup_level3_ref<8>(a.grid.emb, lv, ux, uy, uz, f);
#pragma unroll
            for (int c = 0; c < 8; ++c) acc[c] = acc[c] + w * f[c];
        } else {
            lookup_level3<8>(a.grid.emb, lv, ux, uy, uz, f);
            const f2v wv = {w, w};            // acc + w * f, two channels per packed mul / add
#pragma unroll
            for (int c = 0; c < 8; c += 2) {
                const f2v s = f2v{acc[c], acc[c + 1]} + wv * f2v{f[c], f[c + 1]};
                acc[c] = s.x;
                acc[c + 1] = s.y;
            }
        }
        ux = nx;
        uy = ny;
        uz = nz;
        w = nw;
    }
    if (q > 0) {
#pragma unroll
        for (int c = 0; c < 8; ++c) part[q - 1][c][lane] = acc[c];
    }
    __syncthreads();
    if (q > 0 || !live) return;
#pragma unroll
    for (int c = 0; c < 8; ++c) acc[c] = ((acc[c] + part[0][c][lane]) + part[1][c][lane]) + part[2][c][lane];
    float4* dst = reinterpret_cast<float4*>(a.rows + (size_t)a.tiles(r) * kRow + level * 8u);
    dst[0] = make_float4(acc[0], acc[1], acc[2], acc[3]);
    dst[1] = make_float4(acc[4], acc[5], acc[6], acc[7]);
}

// k_sgrid with de-duplicated gathers (SAMNERF_LOOKUP=box4, wave_box.h).  A
// block is 64 neighbouring rays x 4 sample quarters at one group of 4
// levels (gridDim.y = 4): wave q sums samples q*T/4 .. q*T/4 + T/4 - 1 for
// levels 4g .. 4g+3 (32 accumulators per lane).  Per sample the wave reduces
// its positions' range once, lanes 0-3 evaluate the 4 levels' padded corner
// boxes, and per level the wave loads each distinct corner row once into its
// 8 KiB LDS slice and reads the 8 corners of every lane from there: the
// vector-memory path carries one address per distinct row instead of 16 per
// lane.  Same rows, weights, FMA order and quarter split as k_sgrid, so the
// bits are identical.
constexpr uint32_t kBoxSlots = 256;          // 32 B slots per wave (8 KiB)

// 4 waves per SIMD (128 VGPRs, 7 spilled) instead of the 3 the compiler's
// default 142 VGPRs allow: the VALU-bound box gathers hide their LDS and
// staging latency better -- 0.835 -> 0.72 ms per view, 0.126 -> 0.112 ms at
// one rank's 32K rays (round 2)
#ifndef SAMNERF_DIAG_SGRID_WAVES
#define SAMNERF_DIAG_SGRID_WAVES 4
#endif
// TAP: the parity-tap instantiation (samnerf_taps.srows): the same kernel plus
// the corner-row stores, its own instantiation because the tap code raised the
// product form's spills (20 -> 60 bytes of scratch at 4 waves per SIMD); the
// tapped render's outputs are checked bit-identical to the product's.
// Uniform cells (round 5): a level whose box is one cell for the whole wave
// reads that cell's 8 corner rows through the scalar cache
// (lookup_level3_uniform) -- the coarse levels, where a wave's 64 neighbouring
// rays at one sample share a cell most of the time; the box path's LDS reads
// (8 corners x 32 B per lane) bound the kernel.  Against every level through
// the box: 0.686 -> 0.63 ms per view (a build switch through
// round 6).

template <int T, bool TAP = false>
__global__ void __launch_bounds__(256)
#if SAMNERF_DIAG_SGRID_WAVES
__attribute__((amdgpu_waves_per_eu(SAMNERF_DIAG_SGRID_WAVES, SAMNERF_DIAG_SGRID_WAVES)))
#endif
k_sgrid_box4(SgridArgs a) {
    constexpr int TQ = T / 4;
    __shared__ float4 smem[4][kBoxSlots * 2];          // per wave: the box slice
    const uint32_t lane = threadIdx.x & 63u, q = threadIdx.x >> 6;
    const uint32_t r = xcd_chunk(blockIdx.x, (a.N + 63u) / 64u) * 64u + lane;
    const uint32_t g = blockIdx.y;                      // levels 4g .. 4g+3
    const bool live = r < a.N;
    const uint32_t N = a.N, rr = live ? r : N - 1;
    const LevelDesc L[4] = {a.grid.lv[4 * g], a.grid.lv[4 * g + 1], a.grid.lv[4 * g + 2],
                            a.grid.lv[4 * g + 3]};
    const uint32_t li = lane & 3u;                      // this lane's level for the box pass
    const LevelDesc mine = {li == 0 ? L[0].off : li == 1 ? L[1].off : li == 2 ? L[2].off : L[3].off,
                            li == 0 ? L[0].size : li == 1 ? L[1].size : li == 2 ? L[2].size : L[3].size,
                            li == 0 ? L[0].res : li == 1 ? L[1].res : li == 2 ? L[2].res : L[3].res,
                            0u,
                            li == 0 ? L[0].fres : li == 1 ? L[1].fres : li == 2 ? L[2].fres : L[3].fres,
                            li == 0 ? L[0].ftop : li == 1 ? L[1].ftop : li == 2 ? L[2].ftop : L[3].ftop};
    float* slice = reinterpret_cast<float*>(smem[q]);
    const char* base = reinterpret_cast<const char*>(a.grid.emb);
    float acc[4][8];
#pragma unroll
    for (int l = 0; l < 4; ++l)
#pragma unroll
        for (int c = 0; c < 8; ++c) acc[l][c] = 0.0f;
    const int k0 = (int)q * TQ;
    // 32-bit byte offsets (the host launches this form only for 384 N < 2^32):
    // uniform base + lane offset loads, no 64-bit address arithmetic per sample
    const char* ub = reinterpret_cast<const char*>(a.u_in);
    const char* wb = reinterpret_cast<const char*>(a.w_in);
    const uint32_t N4 = N * 4u;
    auto ld = [](const char* b, uint32_t off) { return *reinterpret_cast<const float*>(b + off); };
    float ux = ld(ub, ((uint32_t)k0 * 3u + 0u) * N4 + rr * 4u);
    float uy = ld(ub, ((uint32_t)k0 * 3u + 1u) * N4 + rr * 4u);
    float uz = ld(ub, ((uint32_t)k0 * 3u + 2u) * N4 + rr * 4u);
    float w = ld(wb, (uint32_t)k0 * N4 + rr * 4u);
    for (int k = k0; k < k0 + TQ; ++k) {
        const uint32_t kn = (uint32_t)(k + 1 < k0 + TQ ? k + 1 : k);          // prefetch (clamped)
        const float nx = ld(ub, (kn * 3u + 0u) * N4 + rr * 4u);
        const float ny = ld(ub, (kn * 3u + 1u) * N4 + rr * 4u);
        const float nz = ld(ub, (kn * 3u + 2u) * N4 + rr * 4u);
        const float nw = ld(wb, kn * N4 + rr * 4u);
        // samples with weight 0 on all 64 rays (N1's dropped samples) add nothing
#ifdef SAMNERF_DIAG_VARIANTS
        if (a.paths && lane == 0u && __builtin_amdgcn_ballot_w64(w != 0.0f) == 0) atomicAdd(a.paths + 3, 1ull);
#endif
        if (__builtin_amdgcn_ballot_w64(w != 0.0f) != 0) {
            const f2v wv = {w, w};
            auto add = [&](int l, const float* f) {
#pragma unroll
                for (int c = 0; c < 8; c += 2) {
                    const f2v s2 = f2v{acc[l][c], acc[l][c + 1]} + wv * f2v{f[c], f[c + 1]};
                    acc[l][c] = s2.x;
                    acc[l][c + 1] = s2.y;
                }
            };
            const URange ur = wave_urange(ux, uy, uz);
            const bool ordered = wave_positions_ordered(ux, uy, uz);
            uint32_t p0, p1, p2;
            pbox_lane(mine, ur, p0, p1, p2);
            // per level: the box's rows staged through registers into the
            // wave's slice, then every lane's 8 corners read from LDS; a box
            // over kBoxSlots slots gathers directly.  (Round 4 measured a
            // one-pass form -- the 4 boxes by LDS DMA into the one slice, one
            // memory round trip per sample, a level whose box did not fit
            // beside the others gathering directly -- at 0.86 against 0.665 ms
            // per view, interleaved A/B of whole builds.)
#pragma unroll
            for (int l = 0; l < 4; ++l) {
                const PBox b = pbox_read(p0, p1, p2, l);
                float f[8];
                uint32_t* rt = nullptr;                     // parity taps only
                if (TAP && live && r % a.tap_stride == 0u)
                    rt = a.rows_tap + ((size_t)(r / a.tap_stride) * T + k) * 128u + (4 * g + l) * 8;
#ifdef SAMNERF_DIAG_VARIANTS
                if (a.paths && lane == 0u) {
                    const int path = (b.uni && ordered) ? 0 : b.slots <= kBoxSlots ? 1 : 2;
                    atomicAdd(a.paths + path, 1ull);
                    if (path == 1) {
                        atomicAdd(a.paths + 4, (unsigned long long)b.slots);
                        atomicAdd(a.paths + 5, (unsigned long long)(b.ex * b.ey * b.ez));
                    }
                }
#endif
                if (b.uni && ordered) {
                    // one cell for the whole wave: its 8 corner rows through the
                    // scalar cache, no box staging, no LDS reads (round 5)
                    const uint32_t dx = b.ex - 1u, dy = b.ey - 1u, dz = b.ez - 1u;
                    uint32_t rows[8];
#pragma unroll
                    for (int c = 0; c < 8; ++c)
                        rows[c] = dense_or_hash_row(b.x0 + (c & 1) * dx, b.y0 + ((c >> 1) & 1) * dy,
                                                    b.z0 + (c >> 2) * dz, L[l]);
                    if (rt) {
#pragma unroll
                        for (int c = 0; c < 8; ++c) rt[c] = rows[c];
                    }
                    lookup_level3_uniform<8>(a.grid.emb, L[l], rows, ux, uy, uz, f);
                } else if (b.slots <= kBoxSlots) {
                    wave_lds_sync();                        // previous level's reads done
                    stage_pbox<8>(base, L[l], b, slice, lane);
                    wave_lds_sync();
                    if (ordered)
                        lookup_level3_pbox<8, false>(a.grid.emb, L[l], b, slice, ux, uy, uz, f, rt);
                    else
                        lookup_level3_pbox<8, true>(a.grid.emb, L[l], b, slice, ux, uy, uz, f, rt);
                } else {
                    if (rt) tap_direct_rows<8>(L[l], ux, uy, uz, rt);
                    lookup_level3<8>(a.grid.emb, L[l], ux, uy, uz, f);
                }
                add(l, f);
            }
        }
        ux = nx;
        uy = ny;
        uz = nz;
        w = nw;
    }
    // quarters 1-3 hand their sums to quarter 0 through the (now free) slices
    __syncthreads();
    float* part = reinterpret_cast<float*>(smem);          // [3][32][64]
    if (q > 0) {
#pragma unroll
        for (int l = 0; l < 4; ++l)
#pragma unroll
            for (int c = 0; c < 8; ++c) part[((q - 1) * 32 + l * 8 + c) * 64 + lane] = acc[l][c];
    }
    __syncthreads();
    if (q > 0 || !live) return;
    float* dst = a.rows + (size_t)a.tiles(r) * kRow + g * 32u;
#pragma unroll
    for (int l = 0; l < 4; ++l) {
        float v[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const int i = l * 8 + c;
            v[c] = ((acc[l][c] + part[(0 * 32 + i) * 64 + lane]) + part[(1 * 32 + i) * 64 + lane]) +
                   part[(2 * 32 + i) * 64 + lane];
        }
        reinterpret_cast<float4*>(dst + l * 8)[0] = make_float4(v[0], v[1], v[2], v[3]);
        reinterpret_cast<float4*>(dst + l * 8)[1] = make_float4(v[4], v[5], v[6], v[7]);
    }
}

// Backward of k_sgrid for the distillation step: grad_emb[row] += w_k *
// corner_weight * g[ray, level*8 + c].  One thread per (ray, level, channel):
// a wave is 8 neighbouring rays x 8 channels, so one atomic wave-instruction
// adds 8 rows of 32 contiguous bytes.
//
// The global float atomics are the cost: they execute at the memory side at
// roughly one wave-instruction per 50 ns per CU whatever the lanes hold
// (MI355X_MICROARCH.md); 8 are issued per wave and sample, one per corner,
// duplicates among the 8 rays merged by a butterfly.  Summing the wave's
// corners over their box of cells in LDS first measured slower on a cfg-5
// step (0.70 vs 0.56 ms), merging along the ray too (1.62 / 1.50 vs 1.29 ms),
// and splitting a ray's samples over 4-16 blocks no faster (DESIGN.md,
// retired forms).

// DET (samnerf_sgrid_backward_det): the per-corner form's adds go
// to a 64-bit fixed-point accumulator instead of the fp32 table -- integer
// atomics are associative, so every total is the same whatever order the
// waves reach it in -- at the scale 2^det_shift (sgrid_det_shift: |any row's
// total| * 2^shift < 2^61); k_sgrid_det_finish adds the totals to the fp32
// gradient.  The per-wave butterfly merge is a fixed order, so it stays.
struct DetAcc {
    unsigned long long* acc;   // [rows][8] int64 (two's complement), null: the fp32 atomics
    const uint32_t* hdr;       // hdr[0]: max |grad_fsam| (float bits), k_sgrid_det_max;
                               // hdr[1]: non-zero when grad_fsam holds a NaN or an Inf
    int log2n;                 // ceil(log2 N)
};

// A gradient with a NaN or an Inf has no fixed-point scale (frexpf(inf) is
// unspecified and a NaN converts to INT64_MIN), and the reference's atomics
// (gridencoder.cu:252-349) propagate it into every row the ray reaches: such
// a call takes the fp32 atomic form (wave-uniform: one header word), whose
// sums carry the NaN / Inf like the reference's.  Bits repeat only for finite
// gradients, which is all the deterministic mode promises.
__device__ __forceinline__ bool sgrid_det_nonfinite(const DetAcc& d) { return d.hdr[1] != 0u; }

// 2^shift of the fixed point: max |g| < 2^e and at most N rays of weights
// summing to <= 1 reach a row, so |total| < 2^(log2n + e) and |total| 2^shift
// < 2^61 (two bits of margin)
__device__ __forceinline__ int sgrid_det_shift(const DetAcc& d) {
    int e = 0;
    frexpf(__uint_as_float(d.hdr[0]), &e);
    return 61 - d.log2n - e;
}

template <int T, bool DET = false>
__global__ void __launch_bounds__(256)
k_sgrid_backward(uint32_t N, RayTiles tiles, GridDesc<16> g, const float* __restrict__ u_in,
                 const float* __restrict__ w_in, const float* __restrict__ grad, uint32_t gstride,
                 float* __restrict__ gemb, DetAcc det = {}) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t r = (uint32_t)(t >> 3), ch = (uint32_t)(t & 7u), lane = threadIdx.x & 63u;
    const uint32_t level = blockIdx.y;
    if (((t & ~(uint64_t)63) >> 3) >= N) return;          // whole wave past the end
    const bool live = r < N;                                // lanes stay for the reductions
    const uint32_t rr = live ? r : N - 1;
    const LevelDesc d = g.lv[level];
    const float gv = live ? grad[(size_t)tiles(rr) * gstride + level * 8u + ch] : 0.0f;
    float* base = gemb + (size_t)d.off * 8u + ch;
    const uint32_t top = d.res - 1u;
    const bool fixed = DET && !sgrid_det_nonfinite(det);  // uniform: the header word
    const double dscale = fixed ? ldexp(1.0, sgrid_det_shift(det)) : 0.0;
    unsigned long long* const dbase = fixed ? det.acc + (size_t)d.off * 8u + ch : nullptr;
    for (int k = 0; k < T; ++k) {
        const float ux = u_in[((size_t)k * 3 + 0) * N + rr];
        const float uy = u_in[((size_t)k * 3 + 1) * N + rr];
        const float uz = u_in[((size_t)k * 3 + 2) * N + rr];
        const float wk = w_in[(size_t)k * N + rr];
        if (__builtin_amdgcn_ballot_w64(wk != 0.0f) == 0) continue;   // N1's dropped samples
        const float wg = wk * gv;
        uint32_t cx, cy, cz;
        float fx, fy, fz;
        locate_axis(ux, d, cx, fx);
        locate_axis(uy, d, cy, fy);
        locate_axis(uz, d, cz, fz);
        const uint32_t nx = min(cx + 1u, top), ny = min(cy + 1u, top), nz = min(cz + 1u, top);
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const float wx = (c & 1) ? fx : 1.0f - fx;
            const float wy = (c & 2) ? fy : 1.0f - fy;
            const float wz = (c & 4) ? fz : 1.0f - fz;
            const uint32_t row = dense_or_hash_row((c & 1) ? nx : cx, (c & 2) ? ny : cy,
                                                   (c & 4) ? nz : cz, d);
            float val = ((wx * wy) * wz) * wg;
            // merge equal rows of the wave's 8 rays over a 3-level butterfly
            // so one lane per row and channel issues the atomic
            bool alive = live;
#pragma unroll
            for (int sd = 8; sd < 64; sd <<= 1) {
                const uint32_t orow = __shfl_xor(row, sd);
                const float oval = __shfl_xor(val, sd);
                const int oalive = __shfl_xor((int)alive, sd);
                if (alive && oalive && orow == row) {
                    if (lane & sd) alive = false;
                    else val += oval;
                }
            }
            if (alive) {
                if (DET && fixed)
                    atomicAdd(dbase + (size_t)row * 8u,
                              (unsigned long long)__double2ll_rn((double)val * dscale));
                else
                    atomicAdd(base + (size_t)row * 8u, val);
            }
        }
    }
}

// max |grad_fsam[ray, 0:128]| into hdr[0] and a non-finite flag into hdr[1]
// (both zeroed by the host): float bits of non-negative values order as
// unsigned integers, so the atomic max is exact
__global__ void __launch_bounds__(256)
k_sgrid_det_max(const float* __restrict__ grad, uint32_t N, uint32_t gstride, uint32_t* hdr) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    float m = 0.0f;
    bool bad = false;
    if (t < (uint64_t)N * 32u) {                     // 4 features per thread
        const float4 v = *reinterpret_cast<const float4*>(grad + (size_t)(t >> 5) * gstride + (t & 31u) * 4u);
        m = fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w)));
        bad = !(isfinite(v.x) && isfinite(v.y) && isfinite(v.z) && isfinite(v.w));
    }
    m = wave_max64(m);
    const bool any_bad = __builtin_amdgcn_ballot_w64(bad) != 0;
    if ((threadIdx.x & 63u) == 0u) {
        if (m > 0.0f && isfinite(m)) atomicMax(hdr, __float_as_uint(m));
        if (any_bad) atomicOr(hdr + 1, 1u);
    }
}

// the fixed-point totals into the fp32 gradient (accumulated into, as the
// atomic form), the accumulator left zero for the next call
__global__ void __launch_bounds__(256)
k_sgrid_det_finish(DetAcc det, float* __restrict__ gemb, uint64_t n) {
    if (sgrid_det_nonfinite(det)) return;            // the fp32 atomics ran: the accumulator is untouched
    const double inv = ldexp(1.0, -sgrid_det_shift(det));
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (uint64_t)gridDim.x * blockDim.x) {
        const long long v = (long long)det.acc[i];
        if (v != 0) {
            gemb[i] = gemb[i] + (float)((double)v * inv);
            det.acc[i] = 0ull;
        }
    }
}

// Default k_sgrid form by launch size: the de-duplicated box gathers win
// on a full view (TA-bound direct gathers): 0.83 vs 1.05 ms at 262,144 rays.
// Since the integer-bit range reduction and v_med3 clamp they also win on one
// rank's share of a sharded view: 0.120 vs 0.132 ms at 32,768 rays, 0.228 vs
// 0.262 at 65,536 (bands of the 512x512 view, bench --rank-share 8 / 4).
// Below 32,768 rays (not measured) the direct form stays.
constexpr uint32_t kBox4MinRays = 32768;

}  // namespace

namespace samnerf {

void launch_sgrid(uint32_t N, RayTiles tiles, const GridDesc<16>& grid, const float* u_in, const float* w_in,
                  float* rows, uint32_t* rows_tap, uint32_t tap_stride, int look, hipStream_t s) {
    SgridArgs sa{};
    sa.N = N;
    sa.tiles = tiles;
    sa.grid = grid;
    sa.u_in = u_in;
    sa.w_in = w_in;
    sa.rows = rows;
    sa.rows_tap = rows_tap;
    sa.tap_stride = tap_stride;
    const char* pp = diag_env("SAMNERF_SGRID_PATHS");
    sa.paths = pp ? reinterpret_cast<unsigned long long*>(strtoull(pp, nullptr, 16)) : nullptr;
    const dim3 sg(xcd_blocks(div_up(N, 64)), 16);
    const dim3 sb(xcd_blocks(div_up(N, 64)), 4);
    if (look == kLookRef) {
        k_sgrid<32, kLookRef><<<sg, 256, 0, s>>>(sa);
    } else if ((look == kLookBox4 || (look == kLookAuto && N >= kBox4MinRays)) && box4_ok(grid) &&
               (uint64_t)N * 384u < (1ull << 32)) {
        if (sa.rows_tap) k_sgrid_box4<32, true><<<sb, 256, 0, s>>>(sa);
        else k_sgrid_box4<32><<<sb, 256, 0, s>>>(sa);
    } else {
        k_sgrid<32, kLookPacked><<<sg, 256, 0, s>>>(sa);
    }
}

}  // namespace samnerf

extern "C" {

// rows of the s_grid table (the deterministic backward's accumulator holds 8
// int64 per row, then an 8-entry header)
static uint64_t sgrid_rows(const samnerf_model* m) {
    return m && m->with_sam && m->s_grid.offsets_host ? (uint64_t)m->s_grid.offsets_host[m->s_grid.num_levels]
                                                      : 0u;
}

size_t samnerf_sgrid_accum_size(const samnerf_model* m) {
    const uint64_t rows = sgrid_rows(m);
    return rows ? (size_t)(rows * 8u + 8u) * sizeof(int64_t) : 0u;
}

int samnerf_sgrid_backward_det(const samnerf_model* m, const float* grad_fsam, uint32_t N,
                               float* grad_embeddings, int64_t* accum, size_t accum_bytes,
                               const void* workspace, size_t workspace_bytes, samnerf_stream_t stream) {
    if (!m || !grad_fsam || !grad_embeddings || !workspace || !accum)
        return fail(SAMNERF_EINVAL, "sgrid_backward_det: null pointer");
    if (!m->with_sam) return fail(SAMNERF_EINVAL, "sgrid_backward_det: model has no s_grid");
    Workspace w = carve(m, N, const_cast<void*>(workspace));
    if (workspace_bytes < w.bytes)
        return fail(SAMNERF_EWORKSPACE, "sgrid_backward_det: workspace too small");
    if (accum_bytes < samnerf_sgrid_accum_size(m))
        return fail(SAMNERF_EWORKSPACE, "sgrid_backward_det: accumulator needs %zu bytes, got %zu",
                    samnerf_sgrid_accum_size(m), accum_bytes);
    if (N == 0) return SAMNERF_OK;
    GridDesc<16> gs;
    int rc = make_grid_desc(m->s_grid, 8, 16, gs, "s_grid");
    if (rc) return rc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const uint64_t n = sgrid_rows(m) * 8u;
    DetAcc det;
    det.acc = reinterpret_cast<unsigned long long*>(accum);
    uint32_t* hdr = reinterpret_cast<uint32_t*>(accum + n);
    det.hdr = hdr;
    det.log2n = 0;
    while ((1ull << det.log2n) < (uint64_t)N) ++det.log2n;
    if (hipMemsetAsync(hdr, 0, 2 * sizeof(uint32_t), s) != hipSuccess)
        return fail(SAMNERF_ELAUNCH, "sgrid_backward_det: header reset failed");
    k_sgrid_det_max<<<div_up((uint64_t)N * 32u, 256), 256, 0, s>>>(grad_fsam, N, kRow, hdr);
    k_sgrid_backward<32, true><<<dim3(div_up((uint64_t)N * 8, 256), 16, 1), 256, 0, s>>>(
        N, make_ray_tiles(N, m->view_width), gs, w.u_f, w.w_f, grad_fsam, kRow, grad_embeddings, det);
    k_sgrid_det_finish<<<2048, 256, 0, s>>>(det, grad_embeddings, n);
    return check_launch("sgrid_backward_det");
}

int samnerf_sgrid_backward(const samnerf_model* m, const float* grad_fsam, uint32_t N,
                           float* grad_embeddings, const void* workspace, size_t workspace_bytes,
                           samnerf_stream_t stream) {
    if (!m || !grad_fsam || !grad_embeddings || !workspace)
        return fail(SAMNERF_EINVAL, "sgrid_backward: null pointer");
    if (!m->with_sam) return fail(SAMNERF_EINVAL, "sgrid_backward: model has no s_grid");
    Workspace w = carve(m, N, const_cast<void*>(workspace));
    if (workspace_bytes < w.bytes)
        return fail(SAMNERF_EWORKSPACE, "sgrid_backward: workspace too small");
    if (N == 0) return SAMNERF_OK;
    GridDesc<16> gs;
    int rc = make_grid_desc(m->s_grid, 8, 16, gs, "s_grid");
    if (rc) return rc;
    k_sgrid_backward<32><<<dim3(div_up((uint64_t)N * 8, 256), 16, 1), 256, 0,
                           reinterpret_cast<hipStream_t>(stream)>>>(
        N, make_ray_tiles(N, m->view_width), gs, w.u_f, w.w_f, grad_fsam, kRow, grad_embeddings);
    return check_launch("sgrid_backward");
}

}  // extern "C"
