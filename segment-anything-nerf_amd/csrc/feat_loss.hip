// feat_loss.hip -- the loss of Trainer.train_step's SAM-distillation branch
// (nerf/utils.py:1094-1108) between the render and the optimiser: the rendered
// feature rows [h*w][256] resized to the teacher's [256][Hg][Wg] map
// (F.interpolate, bilinear, align_corners=False), the mean squared error, and
// its gradient to the rows.  The reference runs them as some eight ATen
// launches that copy the map between the two layouts and, at any size but the
// teacher's, add the resize's gradient with float atomics; here they are three
// launches forward and one backward, with no float atomic: the same inputs
// give the same bits.
//
//   k_fl_taps      per axis: the two taps and weights of every destination cell
//                  (bilinear_tap, the one place the taps are formed) and, for
//                  the backward, where the destination cells of each source
//                  cell begin -> workspace
//   k_fl_forward   one destination row x 32 columns x 128 channels per
//                  workgroup: the teacher's tile comes in along Wg and is
//                  turned through LDS, the rows are read along the channels;
//                  resized (along Wg), the scaled differences [Hg*Wg][256]
//                  (along the channels) and the workgroup's sum of squares
//   k_fl_sum       the workgroups' sums strided by 256, then as a tree
//   k_fl_backward  a gather: one wave per source cell adds its destination
//                  cells' differences, rows in order and columns in order
//
// i0(d) does not decrease with d, so the destination cells whose taps touch
// source cell s -- those with i0 in {s - 1, s} -- are one run [ge[max(s-1,0)],
// ge[s+1]) where ge[v] is the first d with i0(d) >= v.  A source cell with an
// empty run is written as +0.
#include <cmath>

#include "block_reduce.h"
#include "samnerf_common.h"

using namespace samnerf;

namespace {

constexpr uint32_t kT = 256;                 // threads of every workgroup here
constexpr uint32_t kC = 256;                 // the feature width
constexpr uint32_t kMaxSide = 1024;
constexpr uint32_t kTW = 32;                 // destination columns of a tile
constexpr uint32_t kTC = 128;                // channels of a tile
constexpr uint32_t kLD = kTC + 4;            // tile row in LDS: one 16-byte access of padding
constexpr uint32_t kCH = kC / kTC;           // channel tiles

// The taps of destination cell d of an axis resized from n_in to n_out cells:
// upsample_bilinear2d's source index (align_corners=False, the scale from the
// sizes), all in fp32.  src < n_in - 1/2, so i0 <= n_in - 1; the min only
// keeps an index inside the axis whatever the rounding.
__host__ __device__ inline void bilinear_tap(uint32_t n_in, uint32_t n_out, uint32_t d, uint32_t& i0,
                                             uint32_t& i1, float& l1) {
    const float scale = (float)n_in / (float)n_out;
    float src = scale * ((float)d + 0.5f) - 0.5f;
    src = src < 0.0f ? 0.0f : src;
    uint32_t i = (uint32_t)(int)src;
    i = i < n_in - 1u ? i : n_in - 1u;
    i0 = i;
    i1 = i + (i < n_in - 1u ? 1u : 0u);
    l1 = src - (float)i;
}

// one destination cell of one axis in the workspace
struct alignas(16) Tap {
    uint32_t i0, i1;
    float l0, l1;
};

struct Layout {
    float* diff;        // [Hg*Wg][256]  (resized - gt) * 2 / (256 Hg Wg)
    float* part;        // [blocks]      the forward workgroups' sums of squares
    Tap* ty;            // [Hg]
    Tap* tx;            // [Wg]
    uint32_t* gy;       // [h + 1]  first destination row with i0 >= v
    uint32_t* gx;       // [w + 1]
    uint32_t blocks_x, blocks;
    size_t bytes;
};

Layout layout(void* ws, uint32_t h, uint32_t w, uint32_t Hg, uint32_t Wg) {
    Layout l{};
    Carver c(ws);
    l.blocks_x = div_up(Wg, kTW) * kCH;
    l.blocks = l.blocks_x * Hg;
    l.diff = c.take((size_t)Hg * Wg * kC);
    l.part = c.take(l.blocks);
    l.ty = c.take<Tap>((size_t)4 * Hg);
    l.tx = c.take<Tap>((size_t)4 * Wg);
    l.gy = c.take<uint32_t>(h + 1);
    l.gx = c.take<uint32_t>(w + 1);
    l.bytes = c.bytes();
    return l;
}

struct Params {
    uint32_t h, w, Hg, Wg;
    float scale;        // 2 / (256 Hg Wg)
    float count;        // 256 Hg Wg
    const float* pred;
    const float* gt;
    float* resized;
    float* loss;
    const float* grad_loss;
    float* grad_pred;
    Layout l;
};

__device__ __forceinline__ void taps_axis(uint32_t n_in, uint32_t n_out, uint32_t d, Tap* taps, uint32_t* ge) {
    if (d >= n_out) return;
    Tap t;
    bilinear_tap(n_in, n_out, d, t.i0, t.i1, t.l1);
    t.l0 = 1.0f - t.l1;
    taps[d] = t;
    // every v in [0, n_in] is written by exactly one d: those in (i0(d-1), i0(d)]
    // by d, those above the last i0 by the last d
    uint32_t first = 0;
    if (d > 0) {
        uint32_t p0, p1;
        float pl;
        bilinear_tap(n_in, n_out, d - 1u, p0, p1, pl);
        first = p0 + 1u;
    }
    for (uint32_t v = first; v <= t.i0; ++v) ge[v] = d;
    if (d == n_out - 1u)
        for (uint32_t v = t.i0 + 1u; v <= n_in; ++v) ge[v] = n_out;
}

__global__ void __launch_bounds__(kT) k_fl_taps(Params P) {
    const uint32_t d = blockIdx.x * kT + threadIdx.x;
    taps_axis(P.h, P.Hg, d, P.l.ty, P.l.gy);
    taps_axis(P.w, P.Wg, d, P.l.tx, P.l.gx);
}

__device__ __forceinline__ float4 lerp2(float a, float b, const float4& u, const float4& v) {
    return make_float4(a * u.x + b * v.x, a * u.y + b * v.y, a * u.z + b * v.z, a * u.w + b * v.w);
}

__global__ void __launch_bounds__(kT) k_fl_forward(Params P) {
    __shared__ float4 tile4[kTW * kLD / 4];
    __shared__ float sh[kT / 64];
    float* tile = reinterpret_cast<float*>(tile4);
    const uint32_t t = threadIdx.x;
    const uint32_t dx0 = (blockIdx.x / kCH) * kTW, c0 = (blockIdx.x % kCH) * kTC, dy = blockIdx.y;
    const uint32_t Hg = P.Hg, Wg = P.Wg;
    // the teacher's tile: a thread takes four channels of one column, a wave
    // load two runs of 32 columns; the 16-byte LDS stores of 8 neighbouring
    // columns are 132 words apart and cover the 32 banks once
    {
        const uint32_t dxl = t & (kTW - 1u), dx = dx0 + dxl;
        if (dx < Wg) {
#pragma unroll
            for (uint32_t i = 0; i < kTC / 4 / (kT / kTW); ++i) {
                const uint32_t cq = (t / kTW) + (kT / kTW) * i;
                const float* g = P.gt + ((size_t)(c0 + 4u * cq) * Hg + dy) * Wg + dx;
                const size_t plane = (size_t)Hg * Wg;
                tile4[(dxl * kLD + 4u * cq) / 4] = make_float4(g[0], g[plane], g[2 * plane], g[3 * plane]);
            }
        }
    }
    __syncthreads();
    // along the channels: 32 lanes cover the tile's 128, a wave two columns
    const Tap ty = P.l.ty[dy];
    const float4* pred4 = reinterpret_cast<const float4*>(P.pred);
    float4* diff4 = reinterpret_cast<float4*>(P.l.diff);
    const uint32_t c4 = t & (kTC / 4 - 1u), cw = c0 / 4 + c4;
    float acc = 0.0f;
#pragma unroll
    for (uint32_t i = 0; i < kTW / (kT / (kTC / 4)); ++i) {
        const uint32_t dxl = t / (kTC / 4) + (kT / (kTC / 4)) * i, dx = dx0 + dxl;
        if (dx >= Wg) continue;
        const Tap tx = P.l.tx[dx];
        const size_t r0 = (size_t)ty.i0 * P.w, r1 = (size_t)ty.i1 * P.w;
        const float4 v00 = pred4[(r0 + tx.i0) * (kC / 4) + cw], v01 = pred4[(r0 + tx.i1) * (kC / 4) + cw];
        const float4 v10 = pred4[(r1 + tx.i0) * (kC / 4) + cw], v11 = pred4[(r1 + tx.i1) * (kC / 4) + cw];
        const float4 a = lerp2(tx.l0, tx.l1, v00, v01), b = lerp2(tx.l0, tx.l1, v10, v11);
        const float4 r = lerp2(ty.l0, ty.l1, a, b);
        float4& cell = tile4[(dxl * kLD + 4u * c4) / 4];
        const float4 g = cell;
        const float4 d = make_float4(r.x - g.x, r.y - g.y, r.z - g.z, r.w - g.w);
        acc += d.x * d.x;
        acc += d.y * d.y;
        acc += d.z * d.z;
        acc += d.w * d.w;
        diff4[((size_t)dy * Wg + dx) * (kC / 4) + cw] =
            make_float4(d.x * P.scale, d.y * P.scale, d.z * P.scale, d.w * P.scale);
        cell = r;
    }
    acc = block_sum_tree(acc, sh);                     // its barriers also order the tile's stores
    if (t == 0) P.l.part[blockIdx.y * gridDim.x + blockIdx.x] = acc;
    if (!P.resized) return;
    // back along Wg
    const uint32_t dxl = t & (kTW - 1u), dx = dx0 + dxl;
    if (dx >= Wg) return;
#pragma unroll
    for (uint32_t i = 0; i < kTC / 4 / (kT / kTW); ++i) {
        const uint32_t cq = (t / kTW) + (kT / kTW) * i;
        const float4 r = tile4[(dxl * kLD + 4u * cq) / 4];
        float* o = P.resized + ((size_t)(c0 + 4u * cq) * Hg + dy) * Wg + dx;
        const size_t plane = (size_t)Hg * Wg;
        o[0] = r.x;
        o[plane] = r.y;
        o[2 * plane] = r.z;
        o[3 * plane] = r.w;
    }
}

__global__ void __launch_bounds__(kT) k_fl_sum(Params P) {
    __shared__ float sh[kT / 64];
    float v = 0.0f;
    for (uint32_t i = threadIdx.x; i < P.l.blocks; i += kT) v += P.l.part[i];
    v = block_sum_tree(v, sh);
    if (threadIdx.x == 0) *P.loss = v / P.count;
}

// the weight of destination cell t in source cell s's gradient
__device__ __forceinline__ float tap_weight(const Tap& t, uint32_t s) {
    return (t.i0 == s ? t.l0 : 0.0f) + (t.i1 == s ? t.l1 : 0.0f);
}

__global__ void __launch_bounds__(kT) k_fl_backward(Params P) {
    const uint32_t cell = blockIdx.x * (kT / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (cell >= P.h * P.w) return;
    const uint32_t sy = cell / P.w, sx = cell - sy * P.w;
    const uint32_t ylo = P.l.gy[sy ? sy - 1u : 0u], yhi = P.l.gy[sy + 1u];
    const uint32_t xlo = P.l.gx[sx ? sx - 1u : 0u], xhi = P.l.gx[sx + 1u];
    const float4* diff4 = reinterpret_cast<const float4*>(P.l.diff);
    float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    // the weights are the wave's: a tap with no weight (every second one of
    // an identity resize) is skipped by all 64 lanes
    for (uint32_t dy = ylo; dy < yhi; ++dy) {
        const float wy = tap_weight(P.l.ty[dy], sy);
        if (wy == 0.0f) continue;
        for (uint32_t dx = xlo; dx < xhi; ++dx) {
            const float wx = tap_weight(P.l.tx[dx], sx);
            if (wx == 0.0f) continue;
            const float wgt = wy * wx;
            const float4 v = diff4[((size_t)dy * P.Wg + dx) * (kC / 4) + lane];
            acc.x += wgt * v.x;
            acc.y += wgt * v.y;
            acc.z += wgt * v.z;
            acc.w += wgt * v.w;
        }
    }
    const float gl = *P.grad_loss;
    reinterpret_cast<float4*>(P.grad_pred)[(size_t)cell * (kC / 4) + lane] =
        make_float4(gl * acc.x, gl * acc.y, gl * acc.z, gl * acc.w);
}

bool side_ok(uint32_t n) { return n >= 1 && n <= kMaxSide; }

const char* validate(uint32_t h, uint32_t w, uint32_t Hg, uint32_t Wg) {
    if (!side_ok(h) || !side_ok(w)) return "h and w must lie in [1, 1024]";
    if (!side_ok(Hg) || !side_ok(Wg)) return "Hg and Wg must lie in [1, 1024]";
    return nullptr;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

Params params(uint32_t h, uint32_t w, uint32_t Hg, uint32_t Wg, void* ws) {
    Params P{};
    P.h = h; P.w = w; P.Hg = Hg; P.Wg = Wg;
    P.count = (float)kC * (float)Hg * (float)Wg;       // at most 2^28: exact
    P.scale = 2.0f / P.count;
    P.l = layout(ws, h, w, Hg, Wg);
    return P;
}

}  // namespace

extern "C" size_t samnerf_feat_loss_workspace_size(uint32_t h, uint32_t w, uint32_t Hg, uint32_t Wg) {
    if (validate(h, w, Hg, Wg)) return 0;
    return layout(nullptr, h, w, Hg, Wg).bytes;
}

extern "C" int samnerf_feat_loss_forward(const float* pred, uint32_t h, uint32_t w, const float* gt, uint32_t Hg,
                                         uint32_t Wg, float* resized, float* loss, void* ws, size_t ws_bytes,
                                         samnerf_stream_t stream) {
    if (const char* why = validate(h, w, Hg, Wg)) return fail(SAMNERF_EINVAL, "feat_loss_forward: %s", why);
    if (!pred || !gt || !loss || !ws) return fail(SAMNERF_EINVAL, "feat_loss_forward: null pred / gt / loss / ws");
    if (!aligned16(pred) || !aligned16(ws))
        return fail(SAMNERF_EINVAL, "feat_loss_forward: pred and ws must be 16-byte aligned");
    Params P = params(h, w, Hg, Wg, ws);
    if (ws_bytes < P.l.bytes)
        return fail(SAMNERF_EWORKSPACE, "feat_loss_forward: workspace of %zu bytes, %zu needed", ws_bytes, P.l.bytes);
    P.pred = pred; P.gt = gt; P.resized = resized; P.loss = loss;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    int rc;
    k_fl_taps<<<div_up(Hg > Wg ? Hg : Wg, kT), kT, 0, s>>>(P);
    if ((rc = check_launch("feat_loss taps"))) return rc;
    k_fl_forward<<<dim3(P.l.blocks_x, Hg), kT, 0, s>>>(P);
    if ((rc = check_launch("feat_loss forward"))) return rc;
    k_fl_sum<<<1, kT, 0, s>>>(P);
    return check_launch("feat_loss sum");
}

extern "C" int samnerf_feat_loss_backward(const float* grad_loss, uint32_t h, uint32_t w, uint32_t Hg, uint32_t Wg,
                                          float* grad_pred, void* ws, size_t ws_bytes, samnerf_stream_t stream) {
    if (const char* why = validate(h, w, Hg, Wg)) return fail(SAMNERF_EINVAL, "feat_loss_backward: %s", why);
    if (!grad_loss || !grad_pred || !ws)
        return fail(SAMNERF_EINVAL, "feat_loss_backward: null grad_loss / grad_pred / ws");
    if (!aligned16(grad_pred) || !aligned16(ws))
        return fail(SAMNERF_EINVAL, "feat_loss_backward: grad_pred and ws must be 16-byte aligned");
    Params P = params(h, w, Hg, Wg, ws);
    if (ws_bytes < P.l.bytes)
        return fail(SAMNERF_EWORKSPACE, "feat_loss_backward: workspace of %zu bytes, %zu needed", ws_bytes,
                    P.l.bytes);
    P.grad_loss = grad_loss; P.grad_pred = grad_pred;
    k_fl_backward<<<div_up((uint64_t)h * w, kT / 64), kT, 0, reinterpret_cast<hipStream_t>(stream)>>>(P);
    return check_launch("feat_loss backward");
}

extern "C" int samnerf_bilinear_taps_host(uint32_t n_in, uint32_t n_out, uint32_t* i0, uint32_t* i1, float* l1) {
    if (!side_ok(n_in) || !side_ok(n_out)) return fail(SAMNERF_EINVAL, "bilinear_taps_host: sizes must lie in [1, 1024]");
    if (!i0 || !i1 || !l1) return fail(SAMNERF_EINVAL, "bilinear_taps_host: null i0 / i1 / l1");
    for (uint32_t d = 0; d < n_out; ++d) bilinear_tap(n_in, n_out, d, i0[d], i1[d], l1[d]);
    return SAMNERF_OK;
}
