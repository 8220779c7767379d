// incoherent.hip -- the incoherent-region masks of --with_mask training: the
// table the sampler draws its local patches from and the loss weights its rays
// by.  The reference builds it at load from the ground-truth masks
// (colmap_provider.py:798-801) and, under --use_dynamic_incoherent, again every
// incoherent_update_iter steps from the mask head's own renders
// (Trainer.update_incoherent_mask, utils.py:1757-1780, with render_mask,
// :1716-1737, and get_incoherent_mask, :283-298).
//
//   k_incoherent_ids    per rendered ray: render_mask's softmax over the K
//                       instance columns (instance_row.h), pred = [sum of the
//                       first K - 1, last], and the argmax of those two as a byte
//   k_incoherent_masks  the whole get_incoherent_mask chain for n views in one
//                       launch: bilinear down by sfact, bilinear back up,
//                       |mask - recovered|, bilinear down again, cells >= 0.01
//                       set to 1, nearest up; the bool table and / or the float
//                       map
//
// The chain at a size divisible by sfact (a power of two).  ATen's source
// index of a bilinear resize is max(scale * (dst + 0.5) - 0.5, 0) with the upper
// neighbour clamped at the border.  Down by s = 2^k that is s c + s / 2 - 1/2: a
// coarse cell is the mean of the two middle pixels of its s x s block on each
// axis, and both down-samplings read those same 2 x 2 pixels.  So of a coarse
// cell's block only these four pixels reach the result: their mask values and
// the recovered mask at them, which is a bilinear mix of the cell's 3 x 3
// clamped coarse neighbourhood.  A workgroup takes a kTile x kTile tile of
// coarse cells of one view and stages the coarse means of the tile and its
// one-cell halo in LDS -- (kTile + 2)^2 floats whatever sfact is, each from the
// cell's four pixels -- then every thread finishes its own cell, and the
// workgroup writes the tile's pixels row by row, lane = byte.
//
// Every value is a small dyadic rational (ids below 2^14, weights multiples of
// 1 / (2 s)), so each fp32 product and sum is exact and the result does not
// depend on the order: the kernel equals ATen's CPU and GPU kernels bit for
// bit.  At a size that sfact does not divide the reference's bool is set by
// the rounding residue of ATen's kernels; such sizes are refused here.
#include <cmath>

#include "instance_row.h"
#include "samnerf_common.h"

using namespace samnerf;

namespace {

constexpr uint32_t kT = 256;
constexpr uint32_t kTile = SAMNERF_INCOHERENT_TILE;   // coarse cells per tile edge
constexpr uint32_t kHalo = kTile + 2;

static_assert(kTile * kTile == kT, "one thread per coarse cell of the tile");

// ------------------------------------------------------------------- ids --

struct IdsParams {
    uint32_t N, K, Kp, n_inst;
    const float* logits;
    uint8_t* ids;
    float* pred;
};

__global__ void __launch_bounds__(kT) k_incoherent_ids(IdsParams P) {
    extern __shared__ float sz[];             // [kT][Kp], Kp odd: no bank conflict
    const uint32_t t = threadIdx.x, K = P.K, Kp = P.Kp;
    const size_t base = (size_t)blockIdx.x * kT;
    const uint32_t cnt = (uint32_t)min((size_t)kT, (size_t)P.N - base);
    rows_to_tile(sz, P.logits, base * K, cnt, K, Kp, kT);
    __syncthreads();
    if (t >= cnt) return;
    const float* z = sz + t * Kp;
    const size_t i = base + t;
    if (P.n_inst > 1) {
        const RowNorm n = row_norm<1>(z, K);
        // inst_mask[..., :-1].sum(-1): the same tree over the first K - 1 probabilities
        float tr[kMaxK];
#pragma unroll
        for (uint32_t k = 0; k < kMaxK; ++k) tr[k] = k + 1 < K ? row_prob(z, k, n) : 0.0f;
        const float others = tree_sum32(tr);
        const float last = row_prob(z, K - 1, n);
        // argmax of [others, last]: 1 only where last is strictly greater; a
        // tie and a NaN (softmax of a NaN or infinite logit) give 0
        P.ids[i] = last > others ? 1 : 0;
        if (P.pred) { P.pred[2 * i] = others; P.pred[2 * i + 1] = last; }
    } else {
        // one column: the argmax over a dimension of size one
        P.ids[i] = 0;
        if (P.pred) P.pred[i] = row_sigmoid(z[0]);
    }
}

const char* validate_ids(const samnerf_incoherent_ids_args* a) {
    if (!a) return "null args";
    if (a->K < 1 || a->K > kMaxK) return "K (n_inst + redundant_instance) must lie in [1, 32]";
    if (a->n_inst < 1 || a->n_inst > a->K) return "n_inst must lie in [1, K]";
    if (a->n_inst == 1 && a->K != 1)
        return "n_inst == 1 takes K == 1 (redundant columns beside a single instance are not covered)";
    if (a->N == 0) return nullptr;
    if (!a->logits) return "null logits";
    if (!a->ids) return "null ids";
    return nullptr;
}

// ----------------------------------------------------------------- masks --

struct MaskParams {
    uint32_t n, H, W, hc, wc, tiles_x, tiles_y, keep_size;
    float down, up;                           // the resizes' scales: in / out
    const void* masks;
    uint8_t* table;
    float* uncertain;
};

// ATen's area_pixel_compute_source_index, align_corners = false
__device__ __forceinline__ float src_index(float scale, uint32_t dst) {
    return fmaxf(scale * ((float)dst + 0.5f) - 0.5f, 0.0f);
}

struct Tap { uint32_t i0, i1; float w0, w1; };

__device__ __forceinline__ Tap tap_of(float scale, uint32_t dst, uint32_t in) {
    const float s = src_index(scale, dst);
    Tap t;
    t.i0 = min((uint32_t)s, in - 1u);
    t.i1 = t.i0 + (t.i0 < in - 1u ? 1u : 0u);
    t.w1 = s - (float)t.i0;
    t.w0 = 1.0f - t.w1;
    return t;
}

template <typename T>
__global__ void __launch_bounds__(kT) k_incoherent_masks(MaskParams P) {
    __shared__ float small[kHalo * kHalo];    // the coarse means of the tile and its halo
    __shared__ float unc[kTile * kTile];      // mask_uncertain of the tile's cells
    const uint32_t t = threadIdx.x;
    const uint32_t per_view = P.tiles_x * P.tiles_y;
    const uint32_t view = blockIdx.x / per_view, tile = blockIdx.x - view * per_view;
    const uint32_t ty = tile / P.tiles_x, tx = tile - ty * P.tiles_x;
    const uint32_t cy0 = ty * kTile, cx0 = tx * kTile;
    const T* m = static_cast<const T*>(P.masks) + (size_t)view * P.H * P.W;

    // halo cell (hy, hx) is coarse cell (cy0 - 1 + hy, cx0 - 1 + hx); cells off
    // the view are never read (the taps clamp at the border)
    for (uint32_t e = t; e < kHalo * kHalo; e += kT) {
        const uint32_t hy = e / kHalo, hx = e - hy * kHalo;
        const int cy = (int)(cy0 + hy) - 1, cx = (int)(cx0 + hx) - 1;
        float v = 0.0f;
        if (cy >= 0 && cx >= 0 && (uint32_t)cy < P.hc && (uint32_t)cx < P.wc) {
            const Tap y = tap_of(P.down, (uint32_t)cy, P.H), x = tap_of(P.down, (uint32_t)cx, P.W);
            const T* r0 = m + (size_t)y.i0 * P.W;
            const T* r1 = m + (size_t)y.i1 * P.W;
            v = y.w0 * (x.w0 * (float)r0[x.i0] + x.w1 * (float)r0[x.i1]) +
                y.w1 * (x.w0 * (float)r1[x.i0] + x.w1 * (float)r1[x.i1]);
        }
        small[e] = v;
    }
    __syncthreads();

    const uint32_t ly = t / kTile, lx = t - ly * kTile;
    const uint32_t cy = cy0 + ly, cx = cx0 + lx;
    if (cy < P.hc && cx < P.wc) {
        const Tap y = tap_of(P.down, cy, P.H), x = tap_of(P.down, cx, P.W);
        const uint32_t py[2] = {y.i0, y.i1}, px[2] = {x.i0, x.i1};
        float res[2][2];
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            // the recovered mask at row py[a]: its coarse rows lie within cy - 1 .. cy + 1
            const Tap uy = tap_of(P.up, py[a], P.hc);
            const uint32_t h0 = min(uy.i0 + 1u - cy0, kHalo - 1u), h1 = min(uy.i1 + 1u - cy0, kHalo - 1u);
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                const Tap ux = tap_of(P.up, px[b], P.wc);
                const uint32_t g0 = min(ux.i0 + 1u - cx0, kHalo - 1u), g1 = min(ux.i1 + 1u - cx0, kHalo - 1u);
                const float rec = uy.w0 * (ux.w0 * small[h0 * kHalo + g0] + ux.w1 * small[h0 * kHalo + g1]) +
                                  uy.w1 * (ux.w0 * small[h1 * kHalo + g0] + ux.w1 * small[h1 * kHalo + g1]);
                res[a][b] = fabsf((float)m[(size_t)py[a] * P.W + px[b]] - rec);
            }
        }
        float u = y.w0 * (x.w0 * res[0][0] + x.w1 * res[0][1]) + y.w1 * (x.w0 * res[1][0] + x.w1 * res[1][1]);
        if (u >= 0.01f) u = 1.0f;
        unc[t] = u;
        if (!P.keep_size) {
            const size_t o = ((size_t)view * P.hc + cy) * P.wc + cx;
            if (P.table) P.table[o] = u != 0.0f;
            if (P.uncertain) P.uncertain[o] = u;
        }
    }
    if (!P.keep_size) return;
    __syncthreads();

    // nearest up: the tile's pixels row by row, ATen's src = min(floor(dst * scale), in - 1)
    const uint32_t s = P.H / P.hc;
    const uint32_t y0 = cy0 * s, x0 = cx0 * s;
    const uint32_t th = min(kTile * s, P.H - y0), tw = min(kTile * s, P.W - x0);
    for (uint32_t e = t; e < th * tw; e += kT) {
        const uint32_t ry = e / tw, rx = e - ry * tw;
        const uint32_t Y = y0 + ry, X = x0 + rx;
        const uint32_t sy = min((uint32_t)floorf((float)Y * P.up), P.hc - 1u);
        const uint32_t sx = min((uint32_t)floorf((float)X * P.up), P.wc - 1u);
        const float u = unc[min(sy - cy0, kTile - 1u) * kTile + min(sx - cx0, kTile - 1u)];
        const size_t o = ((size_t)view * P.H + Y) * P.W + X;
        if (P.table) P.table[o] = u != 0.0f;
        if (P.uncertain) P.uncertain[o] = u;
    }
}

const char* validate_masks(const samnerf_incoherent_masks_args* a) {
    if (!a) return "null args";
    if (a->sfact == 0 || (a->sfact & (a->sfact - 1u))) return "sfact must be a power of two";
    if (a->H == 0 || a->W == 0) return "H and W must be at least 1";
    if (a->H / a->sfact == 0 || a->W / a->sfact == 0) return "H / sfact and W / sfact must be at least 1";
    if (a->H % a->sfact || a->W % a->sfact)
        return "H and W must be divisible by sfact (elsewhere the reference's result is the rounding residue of "
               "its resize kernels: run its torch ops)";
    if ((uint64_t)a->H * a->W > 0x7fffffffull) return "H * W must stay below 2^31";
    if (a->input_type != SAMNERF_INCOHERENT_INT64 && a->input_type != SAMNERF_INCOHERENT_UINT8)
        return "unknown input_type";
    if (a->n == 0) return nullptr;
    if (!a->masks) return "null masks";
    if (!a->table && !a->uncertain) return "null table and uncertain: nothing to write";
    return nullptr;
}

}  // namespace

extern "C" int samnerf_incoherent_ids(const samnerf_incoherent_ids_args* args, samnerf_stream_t stream) {
    if (const char* why = validate_ids(args)) return fail(SAMNERF_EINVAL, "incoherent_ids: %s", why);
    const samnerf_incoherent_ids_args& a = *args;
    if (a.N == 0) return 0;
    IdsParams P{};
    P.N = a.N; P.K = a.K; P.Kp = a.K | 1u; P.n_inst = a.n_inst;
    P.logits = a.logits; P.ids = a.ids; P.pred = a.pred_mask;
    const size_t lds = (size_t)kT * P.Kp * 4;                          // <= 33 KiB
    k_incoherent_ids<<<div_up(a.N, kT), kT, lds, reinterpret_cast<hipStream_t>(stream)>>>(P);
    return check_launch("incoherent ids");
}

extern "C" int samnerf_incoherent_masks(const samnerf_incoherent_masks_args* args, samnerf_stream_t stream) {
    if (const char* why = validate_masks(args)) return fail(SAMNERF_EINVAL, "incoherent_masks: %s", why);
    const samnerf_incoherent_masks_args& a = *args;
    if (a.n == 0) return 0;
    MaskParams P{};
    P.n = a.n; P.H = a.H; P.W = a.W; P.hc = a.H / a.sfact; P.wc = a.W / a.sfact;
    P.tiles_x = div_up(P.wc, kTile); P.tiles_y = div_up(P.hc, kTile);
    P.keep_size = a.keep_size != 0;
    P.down = (float)a.H / (float)P.hc;                                 // = sfact on both axes
    P.up = (float)P.hc / (float)a.H;
    P.masks = a.masks; P.table = a.table; P.uncertain = a.uncertain;
    const uint64_t blocks = (uint64_t)a.n * P.tiles_x * P.tiles_y;
    if (blocks > 0x7fffffffull) return fail(SAMNERF_EINVAL, "incoherent_masks: n * tiles must stay below 2^31");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (a.input_type == SAMNERF_INCOHERENT_INT64)
        k_incoherent_masks<int64_t><<<(uint32_t)blocks, kT, 0, s>>>(P);
    else
        k_incoherent_masks<uint8_t><<<(uint32_t)blocks, kT, 0, s>>>(P);
    return check_launch("incoherent masks");
}
