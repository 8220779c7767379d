// present.hip -- from a render's outputs to the GUI's display buffer: the mask
// views of Trainer.test_step (nerf/utils.py:1263-1306 with the overlay
// functions of :55-94), the SAM overlay and click squares (:46-52, :97-105),
// test_gui's nearest resize (:1698-1702) and NeRFGUI.prepare_buffer with the
// spp mean (nerf/gui.py:134-140, :171-177).  The reference runs them as a
// dozen ATen launches, two full-frame host copies and numpy passes; here they
// are one launch for an image buffer at the render's size, two for a resized
// one or a depth buffer.
//
// Everything is fp32, one rounding per product and sum, in the reference's op
// order (the build's -ffp-contract=off keeps a * b + c two operations).  The
// probabilities and their argmax are instance_row.h's row -- the bits of
// ATen's softmax on the GPU.  No float atomics: min and max of the depth are
// order-free (block_reduce.h), two stages of fixed shape.
//
// The click squares follow Python's slice rules, as the reference's
// mask[y - r:y + r, x - r:x + r] applies them: an end past the image is
// clipped, and a negative start wraps round to the far edge, so a click
// within r of the top or left edge selects an empty range and draws nothing.
//
//   k_present_frame   per rendered pixel: probabilities, argmax, colour, SAM
//                     overlay, click squares; the frame goes to the buffer
//                     (same size: blended there) or to the workspace
//   k_present_resize  per buffer pixel: its source pixel of the workspace
//                     frame and of the depth, blended into the buffer
//   k_present_minmax  up to 256 workgroups: min, max, any-NaN of the resized
//                     depth, one partial each
//   k_present_depth   per buffer pixel: the partials reduced again by every
//                     workgroup, the normalised depth blended into the buffer
//
// A [N,3] frame is 12-byte pixels: a workgroup moves its 256 pixels' 768
// contiguous dwords between memory and LDS with lane = dword, and each thread
// takes its pixel from LDS (stride 3: no bank conflict).  The logits and the
// probabilities move the same way, the LDS row padded to an odd length
// (instance_row.h rows_to_tile / tile_to_rows).
#include <cmath>

#include "block_reduce.h"
#include "instance_row.h"
#include "samnerf_common.h"

using namespace samnerf;

namespace {

constexpr uint32_t kT = 256;
constexpr uint32_t kWaves = kT / 64;
constexpr uint32_t kMaxParts = 256;           // workgroups of k_present_minmax
constexpr int kRadius = 2;                    // overlay_point's default

struct Params {
    uint32_t rH, rW, H, W, n_src, n_dst, K, Kp, n_inst, n_points, n_parts;
    int mask_type, id;                        // id: the render id, -1 = none
    int use_image, to_buffer, blend;
    float spp, spp1, sy, sx;                  // (float)spp, (float)(spp + 1), the resize's scales
    const float* image;
    const float* depth;
    const float* logits;
    const float* cmap;
    const uint8_t* sam;
    const int32_t* points;
    float* frame;                             // the buffer, or the workspace frame
    float* buffer;
    float* probs;
    int64_t* ids;
    float* depth_out;
    float* parts;                             // [n_parts][3]: min, max, any NaN
};

// Python's a[lo:hi] on an axis of n: whether index v is selected
__device__ __forceinline__ bool in_slice(int v, int lo, int hi, int n) {
    if (lo < 0) lo += n;
    if (hi < 0) hi += n;
    lo = min(max(lo, 0), n);
    hi = min(max(hi, 0), n);
    return v >= lo && v < hi;
}

// ATen's nearest source index (UpSample.h nearest_neighbor_compute_source_index)
__device__ __forceinline__ uint32_t nearest_src(uint32_t dst, float scale, uint32_t in) {
    return min((uint32_t)floorf((float)dst * scale), in - 1u);
}

__device__ __forceinline__ uint32_t src_pixel(const Params& P, uint32_t j) {
    if (P.rH == P.H && P.rW == P.W) return j;
    const uint32_t oy = j / P.W, ox = j - oy * P.W;
    return nearest_src(oy, P.sy, P.rH) * P.rW + nearest_src(ox, P.sx, P.rW);
}

// The workgroup's `cnt` new pixels stand in sm[0 .. 3 cnt): into the buffer at
// pixel `base`, lane = dword.
__device__ __forceinline__ void store_pixels(const Params& P, float* dst, const float* sm, uint32_t base,
                                             uint32_t cnt, bool blend) {
    float* out = dst + (size_t)base * 3;
    for (uint32_t e = threadIdx.x; e < cnt * 3; e += kT) {
        float v = sm[e];
        if (blend) v = (out[e] * P.spp + v) / P.spp1;
        out[e] = v;
    }
}

__global__ void __launch_bounds__(kT) k_present_frame(Params P) {
    extern __shared__ float sm[];
    const uint32_t t = threadIdx.x, base = blockIdx.x * kT, i = base + t;
    const uint32_t cnt = min(kT, P.n_src - base), K = P.K, Kp = P.Kp;
    float* srgb = sm;                         // [kT][3]
    float* sz = sm + kT * 3;                  // [kT][Kp]
    if (P.use_image)
        for (uint32_t e = t; e < cnt * 3; e += kT) srgb[e] = P.image[(size_t)base * 3 + e];
    rows_to_tile(sz, P.logits, (size_t)base * K, cnt, K, Kp, kT);
    __syncthreads();
    if (t < cnt) {
        float im[3] = {0.0f, 0.0f, 0.0f}, c[3];
        if (P.use_image) { im[0] = srgb[3 * t]; im[1] = srgb[3 * t + 1]; im[2] = srgb[3 * t + 2]; }
        if (K) {
            float pid = 0.0f;
            const RowBest b = instance_row<1>(sz + t * Kp, K, P.n_inst, [&](uint32_t k, float v) {
                if ((int)k == P.id) pid = v;
            });
            const float best = b.best;
            const uint32_t arg = b.arg;
            if (P.ids) P.ids[i] = (int64_t)arg;
            const float* ca = P.cmap + 3 * arg;                // arg < K <= n_colors
            const float a7 = (float)0.7, a3 = (float)(1.0 - 0.7);
            if (P.mask_type == SAMNERF_PRESENT_HEATMAP) {
                const float* cc = P.id >= 0 ? P.cmap + 3 * P.id : ca;
                const float m = P.id >= 0 ? pid : best;
                for (int ch = 0; ch < 3; ++ch) c[ch] = cc[ch] * m;
            } else if (P.mask_type == SAMNERF_PRESENT_COMPOSITION) {
                const bool other = P.id >= 0 && (int)arg != P.id;
                for (int ch = 0; ch < 3; ++ch) c[ch] = im[ch] * a7 + (other ? im[ch] : ca[ch]) * a3;
            } else {
                const bool shown = P.id < 0 || (int)arg == P.id;
                for (int ch = 0; ch < 3; ++ch) c[ch] = shown ? ca[ch] : 0.0f;
            }
        } else {
            for (int ch = 0; ch < 3; ++ch) c[ch] = im[ch];
        }
        if (P.sam) {
            const float a7 = (float)0.7, a3 = (float)(1.0 - 0.7);
            const bool on = P.sam[i] != 0;
            for (int ch = 0; ch < 3; ++ch) c[ch] = c[ch] * a7 + (on ? (ch == 0 ? 1.0f : 0.0f) : c[ch]) * a3;
        }
        if (P.n_points) {
            const int y = (int)(i / P.rW), x = (int)(i - (uint32_t)y * P.rW);
            bool hit = false;
            for (uint32_t p = 0; p < P.n_points; ++p) {
                const int px = P.points[2 * p], py = P.points[2 * p + 1];
                hit = hit || (in_slice(y, py - kRadius, py + kRadius, (int)P.rH) &&
                              in_slice(x, px - kRadius, px + kRadius, (int)P.rW));
            }
            if (hit) { c[0] = 0.0f; c[1] = 1.0f; c[2] = 0.0f; }
        }
        srgb[3 * t] = c[0]; srgb[3 * t + 1] = c[1]; srgb[3 * t + 2] = c[2];     // this thread's own slots
        if (P.to_buffer && P.depth_out) P.depth_out[i] = P.depth[i];
    }
    __syncthreads();
    if (P.frame) store_pixels(P, P.frame, srgb, base, cnt, P.blend != 0);
    if (P.probs) tile_to_rows(P.probs, (size_t)base * K, sz, cnt, K, Kp, kT);
}

__global__ void __launch_bounds__(kT) k_present_resize(Params P) {
    __shared__ float sm[kT * 3];
    const uint32_t t = threadIdx.x, base = blockIdx.x * kT, j = base + t;
    const uint32_t cnt = min(kT, P.n_dst - base);
    if (t < cnt) {
        const uint32_t s = src_pixel(P, j);
        const float* f = P.frame + (size_t)s * 3;
        sm[3 * t] = f[0]; sm[3 * t + 1] = f[1]; sm[3 * t + 2] = f[2];
        if (P.depth_out) P.depth_out[j] = P.depth[s];
    }
    __syncthreads();
    store_pixels(P, P.buffer, sm, base, cnt, P.blend != 0);
}

struct Range { float mn, mx, nan; };

// min / max / any-NaN over the workgroup; every thread gets the result
__device__ __forceinline__ Range block_range(Range r, float* sh) {
    const auto op = [](uint32_t j, float a, float b) { return j == 0 ? fminf(a, b) : fmaxf(a, b); };
    float v[3] = {r.mn, r.mx, r.nan};
    wave_all(v, op);
    waves_put(v, sh);
    __syncthreads();
    float a[3] = {sh[0], sh[1], sh[2]};
    waves_fold(a, sh, kWaves, op);
    return Range{a[0], a[1], a[2]};
}

__global__ void __launch_bounds__(kT) k_present_minmax(Params P) {
    __shared__ float sh[3 * kWaves];
    Range r{INFINITY, -INFINITY, 0.0f};       // fminf / fmaxf skip a NaN: it is noted apart
    for (uint32_t j = blockIdx.x * kT + threadIdx.x; j < P.n_dst; j += P.n_parts * kT) {
        const float d = P.depth[src_pixel(P, j)];
        r.mn = fminf(r.mn, d);
        r.mx = fmaxf(r.mx, d);
        if (d != d) r.nan = 1.0f;
    }
    r = block_range(r, sh);
    if (threadIdx.x == 0) {
        float* o = P.parts + 3 * blockIdx.x;
        o[0] = r.mn; o[1] = r.mx; o[2] = r.nan;
    }
}

__global__ void __launch_bounds__(kT) k_present_depth(Params P) {
    __shared__ float sh[3 * kWaves];
    __shared__ float sm[kT * 3];
    const uint32_t t = threadIdx.x, base = blockIdx.x * kT, j = base + t;
    const uint32_t cnt = min(kT, P.n_dst - base);
    Range r{INFINITY, -INFINITY, 0.0f};
    if (t < P.n_parts) r = Range{P.parts[3 * t], P.parts[3 * t + 1], P.parts[3 * t + 2]};   // n_parts <= kT
    r = block_range(r, sh);
    if (r.nan != 0.0f) r.mn = r.mx = NAN;     // numpy's min / max
    if (t < cnt) {
        const float d = P.depth[src_pixel(P, j)];
        const float v = (d - r.mn) / (r.mx - r.mn + 1e-6f);
        sm[3 * t] = v; sm[3 * t + 1] = v; sm[3 * t + 2] = v;
        if (P.depth_out) P.depth_out[j] = d;
    }
    __syncthreads();
    store_pixels(P, P.buffer, sm, base, cnt, P.blend != 0);
}

bool resized(const samnerf_present_args& a) { return a.rH != a.H || a.rW != a.W; }

const char* validate(const samnerf_present_args* a) {
    if (!a) return "null args";
    if (a->rH == 0 || a->rW == 0 || a->H == 0 || a->W == 0) return "rH, rW, H, W must be at least 1";
    const uint64_t ns = (uint64_t)a->rH * a->rW, nd = (uint64_t)a->H * a->W;
    if (a->K > kMaxK) return "K (n_inst + redundant_instance) must lie in [1, 32], or be 0 for no mask view";
    if (ns * (a->K > 3 ? a->K : 3) > 0x7fffffffull || nd * 3 > 0x7fffffffull)
        return "rH * rW * max(K, 3) and H * W * 3 must stay below 2^31";
    if (a->mode != SAMNERF_PRESENT_IMAGE && a->mode != SAMNERF_PRESENT_DEPTH) return "unknown mode";
    if (!a->buffer) return "null buffer";
    if (a->K) {
        if (a->n_inst < 1 || a->n_inst > a->K) return "n_inst must lie in [1, K]";
        if (!a->logits || !a->color_map) return "a mask view needs logits and color_map";
        if (a->mask_type < SAMNERF_PRESENT_HEATMAP || a->mask_type > SAMNERF_PRESENT_MASK) return "unknown mask_type";
        if (a->n_colors < a->K) return "color_map has fewer than K rows: an argmax would index past it";
        if (a->instance_id >= 0 && (uint32_t)a->instance_id < a->n_inst && (uint32_t)a->instance_id >= a->n_colors)
            return "instance_id indexes past color_map";
    } else if (a->probs || a->ids) {
        return "probs and ids need logits";
    }
    if (a->n_points > SAMNERF_PRESENT_MAX_POINTS) return "more than 64 points";
    if (a->n_points && !a->points) return "null points";
    const bool needs_image = a->K == 0 || a->mask_type == SAMNERF_PRESENT_COMPOSITION;
    if (a->mode == SAMNERF_PRESENT_IMAGE && needs_image && !a->image) return "this view needs the rendered image";
    if ((a->mode == SAMNERF_PRESENT_DEPTH || a->depth_out) && !a->depth) return "the depth buffer and depth_out need depth";
    return nullptr;
}

size_t workspace_words(const samnerf_present_args& a) {
    if (a.mode == SAMNERF_PRESENT_DEPTH) return (size_t)3 * kMaxParts;
    return resized(a) ? (size_t)a.rH * a.rW * 3 : 0;
}

}  // namespace

extern "C" size_t samnerf_present_workspace_size(const samnerf_present_args* args) {
    if (validate(args)) return 0;
    return workspace_words(*args) * 4;
}

extern "C" int samnerf_present_frame(const samnerf_present_args* args, void* ws, size_t ws_bytes,
                                     samnerf_stream_t stream) {
    if (const char* why = validate(args)) return fail(SAMNERF_EINVAL, "present_frame: %s", why);
    const samnerf_present_args& a = *args;
    const size_t need = workspace_words(a) * 4;
    if (need && (!ws || ws_bytes < need))
        return fail(SAMNERF_EWORKSPACE, "present_frame: workspace of %zu bytes, %zu needed", ws ? ws_bytes : (size_t)0,
                    need);
    Params P{};
    P.rH = a.rH; P.rW = a.rW; P.H = a.H; P.W = a.W;
    P.n_src = a.rH * a.rW; P.n_dst = a.H * a.W;
    P.K = a.K; P.Kp = a.K | 1u; P.n_inst = a.n_inst; P.n_points = a.n_points;
    P.mask_type = a.mask_type;
    P.id = (a.K && a.instance_id >= 0 && (uint32_t)a.instance_id < a.n_inst) ? a.instance_id : -1;
    P.blend = a.spp != 0;
    P.spp = (float)a.spp; P.spp1 = (float)(a.spp + 1u);
    P.sy = (float)a.rH / (float)a.H; P.sx = (float)a.rW / (float)a.W;
    P.image = a.image; P.depth = a.depth; P.logits = a.logits; P.cmap = a.color_map;
    P.sam = a.sam_mask; P.points = a.points;
    P.buffer = a.buffer; P.probs = a.probs; P.ids = a.ids; P.depth_out = a.depth_out;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const bool image_mode = a.mode == SAMNERF_PRESENT_IMAGE;
    int rc;
    if (image_mode || a.probs || a.ids) {
        // a depth buffer needs no frame: only the side outputs of the logits
        P.use_image = image_mode && (a.K == 0 || a.mask_type == SAMNERF_PRESENT_COMPOSITION);
        P.to_buffer = image_mode && !resized(a);
        P.frame = !image_mode ? nullptr : (P.to_buffer ? a.buffer : static_cast<float*>(ws));
        Params F = P;
        if (!P.to_buffer) F.blend = 0;
        const size_t lds = ((size_t)kT * 3 + (size_t)kT * (a.K ? P.Kp : 0)) * 4;       // <= 36 KiB
        k_present_frame<<<div_up(P.n_src, kT), kT, lds, s>>>(F);
        if ((rc = check_launch("present frame"))) return rc;
    }
    if (image_mode) {
        if (!resized(a)) return 0;
        P.frame = static_cast<float*>(ws);
        k_present_resize<<<div_up(P.n_dst, kT), kT, 0, s>>>(P);
        return check_launch("present resize");
    }
    P.parts = static_cast<float*>(ws);
    P.n_parts = min(kMaxParts, div_up(P.n_dst, kT));
    k_present_minmax<<<P.n_parts, kT, 0, s>>>(P);
    if ((rc = check_launch("present depth range"))) return rc;
    k_present_depth<<<div_up(P.n_dst, kT), kT, 0, s>>>(P);
    return check_launch("present depth");
}
