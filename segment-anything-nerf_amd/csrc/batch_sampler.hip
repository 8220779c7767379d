// batch_sampler.hip -- a training step's input on the device: which pixels a
// step renders (the N > 0 branches of the reference's get_rays,
// nerf/utils.py:174-242) and everything its collate gathers at them
// (nerf/colmap_provider.py:1084-1175, utils.py:247-275).
//
//   k_batch_gather        rays, pixel indices, coarse cells and every ground-
//                         truth table read at (image, pixel) pairs
//   k_batch_draw_uniform  mode R: an image and a pixel per ray
//   k_batch_draw_patches  mode P: random p x p patches of one image
//   k_batch_draw_centred  mode C: a patch centred on a weighted draw per map row
//   k_batch_draw_error    mode E: n cells of one map without replacement
//   k_batch_fill_*        the raw draws of a (seed, offset) as arrays
//
// Every draw kernel has two sources for its raw draws: arrays (the reference's
// torch stream, or samnerf_batch_draw_fill's replay) or Philox4x32-10 under
// (seed, offset) through philox.h; the contract is in include/samnerf_hip.h.
// Plain vector loads and stores; the only atomics are integer LDS counters of
// k_batch_draw_error's histograms, whose sums do not depend on their order.
#include <float.h>

#include "block_reduce.h"
#include "philox.h"
#include "samnerf_common.h"

using namespace samnerf;

namespace {

constexpr uint32_t kStageDraw = 3u;  // an item's two integers and two uniforms
constexpr uint32_t kStageKey = 4u;   // the keys of a map row: stages 4..7

// An integer in [0, R) from one word: bias at most R / 2^32
SAMNERF_HD uint32_t draw_int(uint32_t word, uint32_t R) { return (uint32_t)(((uint64_t)word * R) >> 32); }

// The four words of item `item`
SAMNERF_HD Philox4 draw_quad(const PerturbKey& k, uint32_t item) { return perturb_quad(k, kStageDraw, item, 0u); }

// The four words of cells 4 quad .. 4 quad + 3 of map row `row` (quad < 2^18)
SAMNERF_HD Philox4 key_quad(const PerturbKey& k, uint32_t row, uint32_t quad) {
    return perturb_quad(k, kStageKey + (quad >> 16), row, quad & 0xffffu);
}

// e = -log(u), u = ((word >> 8) + 0.5) * 2^-24 in (0, 1).  The upper half of
// the range is taken through 1 - u, which fp32 holds exactly where it does not
// hold u (above 2^23 the half would round away and the top value reach 1).
__device__ __forceinline__ float key_e(uint32_t word) {
    const uint32_t k = word >> 8;
    if (k < (1u << 23)) return -logf(((float)k + 0.5f) * 0x1p-24f);
    return -log1pf(-(((float)(0xffffffu - k) + 0.5f) * 0x1p-24f));
}

// The key w / e as the bit pattern the selection orders by (non-negative
// floats order as unsigned integers): 0 for a weight that is not positive and
// finite, at least 1 for one that is, so it outranks every excluded cell.
__device__ __forceinline__ uint32_t key_bits(float w, uint32_t word) {
    if (!(w > 0.0f) || w > FLT_MAX) return 0u;
    return max(__float_as_uint(w / key_e(word)), 1u);
}

// A key handed in as an array: anything but a positive number counts as 0
__device__ __forceinline__ uint32_t given_key_bits(float k) { return k > 0.0f ? __float_as_uint(k) : 0u; }

__device__ __forceinline__ float load_weight(const void* w, uint32_t bytes, size_t i) {
    return bytes == 4u ? static_cast<const float*>(w)[i] : (float)static_cast<const uint8_t*>(w)[i];
}

// ------------------------------------------------------------------ gather --

struct GatherArgs {
    samnerf_batch_source s;
    samnerf_batch_out o;
    const int64_t* index;      // [n] or [1]
    const int64_t* pixels;     // [n] row * W + col of the ray image
    uint32_t n_index, n;
    uint32_t H, W;             // the ray image (s.H x s.W unless the intrinsics are fixed-fov)
    uint32_t coarse;           // side of the map of inds_coarse (0: not written)
    float csx, csy;            // coarse / H, coarse / W
    float inc_scale, err_scale;
};

// One thread per ray.  A ray whose image or pixel is out of range writes
// nothing; a map cell outside its map (the reference scales columns by
// size / H, colmap_provider.py:1118-1123, which overruns a row when W > H) is
// not read.
__global__ void __launch_bounds__(256) k_batch_gather(GatherArgs a) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= a.n) return;
    const int64_t img64 = a.index[a.n_index == 1u ? 0u : t], pix64 = a.pixels[t];
    if ((uint64_t)img64 >= a.s.n_img || (uint64_t)pix64 >= (uint64_t)a.H * a.W) return;
    const uint32_t img = (uint32_t)img64, pix = (uint32_t)pix64;
    const uint32_t row = pix / a.W, col = pix % a.W;
    if (a.o.i) a.o.i[t] = col;
    if (a.o.j) a.o.j[t] = row;
    if (a.o.rays_o && a.o.rays_d) {
        // utils.py:164-168, :247-259
        const float* P = a.s.poses + (size_t)img * 16u;
        const float* K = a.s.intrinsics + (a.s.n_intr == 1u ? 0u : (size_t)img * 4u);
        const float i = (float)col + 0.5f, j = (float)row + 0.5f;
        const float xs = (i - K[2]) / K[0];
        const float ys = -((j - K[3]) / K[1]);
        const float zs = -1.0f;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            a.o.rays_d[(size_t)t * 3u + k] =
                __builtin_fmaf(zs, P[4 * k + 2], __builtin_fmaf(ys, P[4 * k + 1], xs * P[4 * k]));
            a.o.rays_o[(size_t)t * 3u + k] = P[4 * k + 3];
        }
    }
    if (a.o.inds_coarse && a.coarse) {
        // utils.py:269-275
        const int64_t cx = (int64_t)((float)row * a.csx), cy = (int64_t)((float)col * a.csy);
        a.o.inds_coarse[t] = cx * a.coarse + cy;
    }
    const size_t at = ((size_t)img * a.s.H + row) * a.s.W + col;
    if (a.s.images && a.o.images) {
        // colmap_provider.py:1086
        for (uint32_t c = 0; c < a.s.C; ++c) {
            const float v = a.s.images_float ? static_cast<const float*>(a.s.images)[at * a.s.C + c]
                                             : (float)static_cast<const uint8_t*>(a.s.images)[at * a.s.C + c];
            a.o.images[(size_t)t * a.s.C + c] = v / 255.0f;
        }
    }
    if (a.s.masks && a.o.masks) a.o.masks[t] = a.s.masks[at];
    if (a.s.incoherent_masks && a.o.incoherent_masks) {
        // colmap_provider.py:1118-1123
        const uint64_t S = a.s.incoherent_size;
        const uint64_t c = (uint64_t)((float)row * a.inc_scale) * S + (uint64_t)((float)col * a.inc_scale);
        if (c < S * S) {
            const size_t e = (size_t)img * S * S + c;
            if (a.s.incoherent_bytes == 4u)
                static_cast<float*>(a.o.incoherent_masks)[t] = static_cast<const float*>(a.s.incoherent_masks)[e];
            else
                static_cast<uint8_t*>(a.o.incoherent_masks)[t] = static_cast<const uint8_t*>(a.s.incoherent_masks)[e];
        }
    }
    if (a.s.error_map && a.o.error_maps) {
        // colmap_provider.py:1140-1145
        const uint64_t S = a.s.error_size;
        const uint64_t c = (uint64_t)((float)row * a.err_scale) * S + (uint64_t)((float)col * a.err_scale);
        if (c < S * S) a.o.error_maps[t] = a.s.error_map[(size_t)img * S * S + c];
    }
    if (a.s.cam_near_far && a.o.cam_near_far) {
        a.o.cam_near_far[(size_t)t * 2u] = a.s.cam_near_far[(size_t)img * 2u];
        a.o.cam_near_far[(size_t)t * 2u + 1u] = a.s.cam_near_far[(size_t)img * 2u + 1u];
    }
}

// ------------------------------------------------------------------- draws --

struct DrawArgs {
    PerturbKey key;
    uint32_t n_img, H, W;
    uint32_t n;                // R, E: rays; P: patches; C: map rows
    uint32_t p;                // P, C: patch side
    uint32_t M;                // C, E: map side
    float sx, sy;              // C, E: H / M, W / M
    const void* weights;       // [n_img][M * M]
    uint32_t weight_bytes;
    const int64_t* rows;       // C, E: the image of each map row, or null (C seeded: drawn)
    const int64_t* int0;       // array form, else null
    const int64_t* int1;
    const float* keys;
    const float* u0;
    const float* u1;
    int64_t* index;
    int64_t* pixels;
    int64_t* cells;
};

// Mode R (utils.py:234-236 with colmap_provider.py:975 / :978): image =
// randint(n_img), pixel = randint(H * W), per ray
__global__ void __launch_bounds__(256) k_batch_draw_uniform(DrawArgs a) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= a.n) return;
    int64_t img, pix;
    if (a.int0) {
        img = a.int0[t], pix = a.int1[t];
    } else {
        const Philox4 w = draw_quad(a.key, t);
        img = draw_int(w.v[0], a.n_img), pix = draw_int(w.v[1], a.H * a.W);
    }
    a.index[t] = img;
    a.pixels[t] = pix;
}

// Pixel k of the p x p patch whose top-left corner is (x0, y0), in the
// reference's order (utils.py:206-219: offsets (k / p, k % p))
__device__ __forceinline__ int64_t patch_pixel(int64_t x0, int64_t y0, uint32_t k, uint32_t p, uint32_t W) {
    return (x0 + (int64_t)(k / p)) * (int64_t)W + y0 + (int64_t)(k % p);
}

// Mode P (utils.py:196-219): corner row = randint(H - p), col = randint(W - p)
// per patch; one thread per pixel of a patch
__global__ void __launch_bounds__(256) k_batch_draw_patches(DrawArgs a) {
    const uint32_t pp = a.p * a.p;
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= a.n * pp) return;
    const uint32_t patch = t / pp, k = t % pp;
    int64_t x0, y0;
    if (a.int0) {
        x0 = a.int0[patch], y0 = a.int1[patch];
    } else {
        const Philox4 w = draw_quad(a.key, patch);
        x0 = draw_int(w.v[0], a.H - a.p), y0 = draw_int(w.v[1], a.W - a.p);
    }
    a.pixels[t] = patch_pixel(x0, y0, k, a.p, a.W);
}

// Mode C (utils.py:180-194, :206-219): block b draws the centre of map row b
// -- the cell of largest key, the lower cell winning a tie -- as a block
// arg-max over (key bits, ~cell) packed in 64 bits, the row streamed from
// memory once (M up to 1024: 4 MiB of keys, never staged).
__global__ void __launch_bounds__(256) k_batch_draw_centred(DrawArgs a) {
    __shared__ uint64_t wbest[4];
    const uint32_t b = blockIdx.x, tid = threadIdx.x;
    const uint32_t cells = a.M * a.M;
    int64_t img;
    if (a.rows)
        img = a.rows[b];
    else
        img = draw_int(draw_quad(a.key, b).v[0], a.n_img);
    if ((uint64_t)img >= a.n_img) return;        // uniform over the block
    uint64_t best = 0;
    for (uint32_t q = tid; q * 4u < cells; q += 256u) {
        Philox4 w{};
        if (!a.keys) w = key_quad(a.key, b, q);
#pragma unroll
        for (uint32_t e = 0; e < 4; ++e) {
            const uint32_t c = q * 4u + e;
            if (c >= cells) break;
            const uint32_t bits = a.keys ? given_key_bits(a.keys[(size_t)b * cells + c])
                                         : key_bits(load_weight(a.weights, a.weight_bytes, (size_t)img * cells + c), w.v[e]);
            const uint64_t v = (uint64_t)bits << 32 | (0xffffffffu - c);
            best = v > best ? v : best;
        }
    }
    const auto larger = [](uint64_t a, uint64_t b) { return b > a ? b : a; };
    waves_put(wave_all(best, larger), wbest);
    __syncthreads();
    best = waves_fold(wbest, 4u, larger);
    const uint32_t c = 0xffffffffu - (uint32_t)best;          // < cells: every thread's candidates are
    const uint32_t crow = c / a.M, ccol = c % a.M;
    // utils.py:188-194: float32, the corner clamped to [0, H - p - 1]
    const float px = (float)crow * a.sx, py = (float)ccol * a.sy;
    const float half = (float)(a.p / 2u);
    const int64_t x0 = (int64_t)fminf(fmaxf(px - half, 0.0f), (float)((int64_t)a.H - a.p - 1));
    const int64_t y0 = (int64_t)fminf(fmaxf(py - half, 0.0f), (float)((int64_t)a.W - a.p - 1));
    const uint32_t pp = a.p * a.p;
    if (tid == 0u && a.cells) a.cells[b] = c;
    for (uint32_t k = tid; k < pp; k += 256u) {
        a.pixels[(size_t)b * pp + k] = patch_pixel(x0, y0, k, a.p, a.W);
        if (a.index) a.index[(size_t)b * pp + k] = img;
    }
}

constexpr uint32_t kECells = 16384u, kEThreads = 1024u, kEPer = kECells / kEThreads;

// Mode E (utils.py:222-233): n cells of one 128 x 128 map without replacement
// -- the n largest keys, ties to the lower cell, written in ascending cell
// order -- and a pixel inside each.  One workgroup; the 16,384 key patterns
// stay in LDS (64 KiB).  The n-th largest pattern T comes from a radix select,
// four 8-bit digits from the top, each a 256-bin histogram of the patterns
// that share the digits found so far; then every thread counts, over its 16
// consecutive cells, the patterns above T and equal to T, one block scan gives
// each its place, and the cells above T and the first (n - above) equal to T
// are written.  Exactly n cells are written whatever the map holds.
__global__ void __launch_bounds__(kEThreads) k_batch_draw_error(DrawArgs a) {
    __shared__ __attribute__((aligned(16))) uint32_t sk[kECells];
    __shared__ uint32_t hist[256];
    __shared__ uint32_t wsum[kEThreads / 64u];
    __shared__ uint32_t sel[2];
    const uint32_t tid = threadIdx.x;
    const int64_t img = a.rows[0];
    if ((uint64_t)img >= a.n_img) return;        // uniform over the block
    const uint32_t base = tid * kEPer;
#pragma unroll
    for (uint32_t q = 0; q < kEPer / 4u; ++q) {
        const uint32_t c = base + 4u * q;
        uint4 bits;
        if (a.keys) {
            const float4 k = *reinterpret_cast<const float4*>(a.keys + c);
            bits = make_uint4(given_key_bits(k.x), given_key_bits(k.y), given_key_bits(k.z), given_key_bits(k.w));
        } else {
            const Philox4 w = key_quad(a.key, 0u, c >> 2);
            const size_t at = (size_t)img * kECells + c;
            bits = make_uint4(key_bits(load_weight(a.weights, a.weight_bytes, at), w.v[0]),
                              key_bits(load_weight(a.weights, a.weight_bytes, at + 1u), w.v[1]),
                              key_bits(load_weight(a.weights, a.weight_bytes, at + 2u), w.v[2]),
                              key_bits(load_weight(a.weights, a.weight_bytes, at + 3u), w.v[3]));
        }
        *reinterpret_cast<uint4*>(&sk[c]) = bits;
    }
    __syncthreads();
    uint32_t prefix = 0u, remaining = a.n;       // 1 <= n <= 16384 (host)
#pragma unroll
    for (uint32_t pass = 0; pass < 4u; ++pass) {
        const uint32_t shift = 24u - 8u * pass;
        if (tid < 256u) hist[tid] = 0u;
        __syncthreads();
        for (uint32_t it = 0; it < kEPer; ++it) {
            const uint32_t bits = sk[it * kEThreads + tid];
            if (pass == 0u || (bits >> (shift + 8u)) == prefix) atomicAdd(&hist[(bits >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (tid < 64u) {
            // lane l holds bins 255 - 4 l .. 252 - 4 l, the largest digit first
            const uint32_t b0 = 255u - 4u * tid;
            const uint32_t h0 = hist[b0], h1 = hist[b0 - 1u], h2 = hist[b0 - 2u], h3 = hist[b0 - 3u];
            const uint32_t s = h0 + h1 + h2 + h3;
            uint32_t incl = s;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const uint32_t o = __shfl_up(incl, d, 64);
                if ((int)tid >= d) incl += o;
            }
            const uint32_t excl = incl - s;
            if (excl < remaining && remaining <= incl) {      // one lane: the matching patterns are >= remaining
                const uint32_t r = remaining - excl;
                uint32_t d = b0, above = excl;
                if (r > h0) d = b0 - 1u, above += h0;
                if (r > h0 + h1) d = b0 - 2u, above += h1;
                if (r > h0 + h1 + h2) d = b0 - 3u, above += h2;
                sel[0] = d;
                sel[1] = above;
            }
        }
        __syncthreads();
        prefix = prefix << 8 | sel[0];
        remaining -= sel[1];
    }
    const uint32_t T = prefix, need_eq = remaining;
    uint32_t v[kEPer];
#pragma unroll
    for (uint32_t q = 0; q < kEPer / 4u; ++q) {
        const uint4 x = *reinterpret_cast<const uint4*>(&sk[base + 4u * q]);
        v[4 * q] = x.x, v[4 * q + 1] = x.y, v[4 * q + 2] = x.z, v[4 * q + 3] = x.w;
    }
    uint32_t packed = 0u;                        // above T in the low half, equal in the high: each <= 16384
#pragma unroll
    for (uint32_t e = 0; e < kEPer; ++e) packed += (v[e] > T ? 1u : 0u) + (v[e] == T ? 0x10000u : 0u);
    uint32_t incl = packed;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(incl, d, 64);
        if ((int)(tid & 63u) >= d) incl += o;
    }
    if ((tid & 63u) == 63u) wsum[tid >> 6] = incl;
    __syncthreads();
    uint32_t excl = incl - packed;
    for (uint32_t w = 0; w < (tid >> 6); ++w) excl += wsum[w];
    uint32_t eq_rank = excl >> 16;
    uint32_t pos = (excl & 0xffffu) + min(eq_rank, need_eq);
#pragma unroll
    for (uint32_t e = 0; e < kEPer; ++e) {
        const bool eq = v[e] == T;
        const bool chosen = v[e] > T || (eq && eq_rank < need_eq);
        eq_rank += eq ? 1u : 0u;
        if (!chosen) continue;
        if (pos < a.n) {
            const uint32_t c = base + e;
            float rx, ry;
            if (a.u0) {
                rx = a.u0[pos], ry = a.u1[pos];
            } else {
                const Philox4 w = draw_quad(a.key, pos);
                rx = philox_uniform(w.v[2]), ry = philox_uniform(w.v[3]);
            }
            // utils.py:226-230
            const int64_t x = min((int64_t)((float)(c >> 7) * a.sx + rx * a.sx), (int64_t)a.H - 1);
            const int64_t y = min((int64_t)((float)(c & 127u) * a.sy + ry * a.sy), (int64_t)a.W - 1);
            a.cells[pos] = c;
            a.pixels[pos] = x * (int64_t)a.W + y;
        }
        ++pos;
    }
}

// -------------------------------------------------------------------- fill --

struct FillArgs {
    PerturbKey key;
    uint32_t items, range0, range1;
    int64_t* int0;
    int64_t* int1;
    float* u0;
    float* u1;
    const void* weights;
    uint32_t weight_bytes, n_img, B, cells;
    const int64_t* rows;
    float* keys;
};

__global__ void __launch_bounds__(256) k_batch_fill_items(FillArgs a) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= a.items) return;
    const Philox4 w = draw_quad(a.key, t);
    if (a.int0) a.int0[t] = draw_int(w.v[0], a.range0);
    if (a.int1) a.int1[t] = draw_int(w.v[1], a.range1);
    if (a.u0) a.u0[t] = philox_uniform(w.v[2]);
    if (a.u1) a.u1[t] = philox_uniform(w.v[3]);
}

// One thread per (row, quad of cells)
__global__ void __launch_bounds__(256) k_batch_fill_keys(FillArgs a) {
    const uint32_t quads = (a.cells + 3u) / 4u;
    const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (t >= (uint64_t)a.B * quads) return;
    const uint32_t b = (uint32_t)(t / quads), q = (uint32_t)(t % quads);
    const int64_t img = a.rows ? a.rows[b] : (int64_t)draw_int(draw_quad(a.key, b).v[0], a.n_img);
    const Philox4 w = key_quad(a.key, b, q);
#pragma unroll
    for (uint32_t e = 0; e < 4; ++e) {
        const uint32_t c = q * 4u + e;
        if (c >= a.cells) break;
        uint32_t bits = 0u;
        if ((uint64_t)img < a.n_img)
            bits = key_bits(load_weight(a.weights, a.weight_bytes, (size_t)img * a.cells + c), w.v[e]);
        a.keys[(size_t)b * a.cells + c] = __uint_as_float(bits);
    }
}

bool weight_bytes_ok(uint32_t b) { return b == 1u || b == 4u; }

}  // namespace

extern "C" {

int samnerf_batch_gather(const samnerf_batch_source* src, const int64_t* index, uint32_t n_index,
                         const int64_t* pixels, uint32_t n, uint32_t H, uint32_t W, uint32_t coarse_size,
                         const samnerf_batch_out* out, samnerf_stream_t stream) {
    if (!src || !out || !index || !pixels) return fail(SAMNERF_EINVAL, "batch_gather: null pointer");
    if (n == 0) return SAMNERF_OK;
    if (n_index != 1u && n_index != n) return fail(SAMNERF_EINVAL, "batch_gather: index must hold 1 or n entries");
    if (src->n_img == 0 || H == 0 || W == 0 || (uint64_t)H * W > 0xffffffffull)
        return fail(SAMNERF_EINVAL, "batch_gather: empty source or H * W beyond 2^32");
    if ((out->rays_o == nullptr) != (out->rays_d == nullptr))
        return fail(SAMNERF_EINVAL, "batch_gather: rays_o and rays_d come together");
    if (out->rays_o && (!src->poses || !src->intrinsics || (src->n_intr != 1u && src->n_intr != src->n_img)))
        return fail(SAMNERF_EINVAL, "batch_gather: rays need poses and 1 or n_img rows of intrinsics");
    const bool tables = (src->images && out->images) || (src->masks && out->masks);
    if (tables && (H > src->H || W > src->W))
        return fail(SAMNERF_EINVAL, "batch_gather: a %u x %u ray image reads outside the %u x %u tables", H, W,
                    src->H, src->W);
    if (src->images && out->images && (src->C < 1u || src->C > 4u))
        return fail(SAMNERF_EINVAL, "batch_gather: C must be 1..4");
    if (src->incoherent_masks && out->incoherent_masks &&
        (!weight_bytes_ok(src->incoherent_bytes) || src->incoherent_size == 0 || src->H == 0))
        return fail(SAMNERF_EINVAL, "batch_gather: incoherent masks need 1- or 4-byte cells and a size");
    if (src->error_map && out->error_maps && (src->error_size == 0 || src->H == 0))
        return fail(SAMNERF_EINVAL, "batch_gather: the error map needs a size");
    GatherArgs a{};
    a.s = *src, a.o = *out;
    a.index = index, a.pixels = pixels, a.n_index = n_index, a.n = n;
    a.H = H, a.W = W;
    a.coarse = coarse_size;
    // a long tensor times a Python float: the scalar rounded to float32
    a.csx = (float)((double)coarse_size / H), a.csy = (float)((double)coarse_size / W);
    if (src->H) {
        a.inc_scale = (float)((double)src->incoherent_size / src->H);
        a.err_scale = (float)((double)src->error_size / src->H);
    }
    k_batch_gather<<<div_up(n, 256), 256, 0, reinterpret_cast<hipStream_t>(stream)>>>(a);
    return check_launch("batch_gather");
}

int samnerf_batch_draw(const samnerf_batch_draw_args* d, samnerf_stream_t stream) {
    if (!d) return fail(SAMNERF_EINVAL, "batch_draw: null pointer");
    if (d->n == 0) return SAMNERF_OK;
    if (!d->pixels) return fail(SAMNERF_EINVAL, "batch_draw: pixels is null");
    if (d->n_img == 0 || d->H == 0 || d->W == 0 || (uint64_t)d->H * d->W > 0xffffffffull)
        return fail(SAMNERF_EINVAL, "batch_draw: empty source or H * W beyond 2^32");
    DrawArgs a{};
    a.key = make_perturb_key(d->seed, d->offset);
    a.n_img = d->n_img, a.H = d->H, a.W = d->W, a.n = d->n, a.p = d->patch, a.M = d->M;
    a.weights = d->weights, a.weight_bytes = d->weight_bytes, a.rows = d->rows;
    a.index = d->index, a.pixels = d->pixels, a.cells = d->cells;
    const bool seeded = d->seeded != 0;
    if (!seeded) a.int0 = d->int0, a.int1 = d->int1, a.keys = d->keys, a.u0 = d->u0, a.u1 = d->u1;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const bool patchy = d->mode == SAMNERF_BATCH_PATCHES || d->mode == SAMNERF_BATCH_CENTRED;
    if (patchy) {
        // utils.py:193-202: corners in [0, H - p) and clamped to H - p - 1
        if (d->patch < 1u || d->patch >= d->H || d->patch >= d->W)
            return fail(SAMNERF_EINVAL, "batch_draw: patch %u does not fit a %u x %u image", d->patch, d->H, d->W);
        if ((uint64_t)d->n * d->patch * d->patch > 0x7fffffffull)
            return fail(SAMNERF_EINVAL, "batch_draw: too many rays");
    }
    const bool weighted = d->mode == SAMNERF_BATCH_CENTRED || d->mode == SAMNERF_BATCH_ERROR;
    if (weighted) {
        if (d->M < 1u || d->M > 1024u) return fail(SAMNERF_EINVAL, "batch_draw: M = %u outside 1..1024", d->M);
        if (seeded ? (!d->weights || !weight_bytes_ok(d->weight_bytes)) : !d->keys)
            return fail(SAMNERF_EINVAL, "batch_draw: needs weights (1- or 4-byte cells) when seeded, keys otherwise");
        a.sx = (float)((double)d->H / d->M), a.sy = (float)((double)d->W / d->M);
    }
    switch (d->mode) {
    case SAMNERF_BATCH_UNIFORM:
        if (!d->index || (!seeded && (!d->int0 || !d->int1)))
            return fail(SAMNERF_EINVAL, "batch_draw: mode R needs index and, unseeded, int0 and int1");
        k_batch_draw_uniform<<<div_up(d->n, 256), 256, 0, s>>>(a);
        break;
    case SAMNERF_BATCH_PATCHES:
        if (!seeded && (!d->int0 || !d->int1)) return fail(SAMNERF_EINVAL, "batch_draw: mode P unseeded needs int0 and int1");
        k_batch_draw_patches<<<div_up((uint64_t)d->n * d->patch * d->patch, 256), 256, 0, s>>>(a);
        break;
    case SAMNERF_BATCH_CENTRED:
        if (!seeded && !d->rows) return fail(SAMNERF_EINVAL, "batch_draw: mode C unseeded needs rows");
        k_batch_draw_centred<<<d->n, 256, 0, s>>>(a);
        break;
    case SAMNERF_BATCH_ERROR:
        // utils.py:226 divides by a literal 128
        if (d->M != 128u) return fail(SAMNERF_EINVAL, "batch_draw: mode E takes M = 128 only (utils.py:226)");
        if (d->n > kECells) return fail(SAMNERF_EINVAL, "batch_draw: mode E draws at most %u cells", kECells);
        if (!d->rows || !d->cells || (!seeded && (!d->u0 || !d->u1)))
            return fail(SAMNERF_EINVAL, "batch_draw: mode E needs rows, cells and, unseeded, u0 and u1");
        if (!seeded && (reinterpret_cast<uintptr_t>(d->keys) & 15u))
            return fail(SAMNERF_EINVAL, "batch_draw: keys must be 16-byte aligned");
        k_batch_draw_error<<<1, kEThreads, 0, s>>>(a);
        break;
    default:
        return fail(SAMNERF_EINVAL, "batch_draw: unknown mode %d", d->mode);
    }
    return check_launch("batch_draw");
}

int samnerf_batch_draw_fill(uint64_t seed, uint64_t offset, uint32_t items, uint32_t range0, uint32_t range1,
                            int64_t* int0, int64_t* int1, float* u0, float* u1, const void* weights,
                            uint32_t weight_bytes, uint32_t n_img, const int64_t* rows, uint32_t B,
                            uint32_t cells, float* keys, samnerf_stream_t stream) {
    FillArgs a{};
    a.key = make_perturb_key(seed, offset);
    a.items = items, a.range0 = range0, a.range1 = range1;
    a.int0 = int0, a.int1 = int1, a.u0 = u0, a.u1 = u1;
    a.weights = weights, a.weight_bytes = weight_bytes, a.n_img = n_img, a.B = B, a.cells = cells;
    a.rows = rows, a.keys = keys;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (items && (int0 || int1 || u0 || u1)) {
        k_batch_fill_items<<<div_up(items, 256), 256, 0, s>>>(a);
        if (int rc = check_launch("batch_draw_fill")) return rc;
    }
    if (keys && B && cells) {
        if (!weights || !weight_bytes_ok(weight_bytes) || n_img == 0 || cells > 1024u * 1024u)
            return fail(SAMNERF_EINVAL, "batch_draw_fill: keys need weights (1- or 4-byte cells) of at most 1024^2 cells");
        const uint64_t blocks = ((uint64_t)B * ((cells + 3u) / 4u) + 255u) / 256u;
        if (blocks > 0x7fffffffull) return fail(SAMNERF_EINVAL, "batch_draw_fill: too many rows");
        k_batch_fill_keys<<<(uint32_t)blocks, 256, 0, s>>>(a);
        return check_launch("batch_draw_fill");
    }
    return SAMNERF_OK;
}

int samnerf_batch_draw_host(uint64_t seed, uint64_t offset, uint32_t item, uint32_t range0, uint32_t range1,
                            int64_t* ints_host, float* uniforms_host) {
    if (!ints_host || !uniforms_host) return fail(SAMNERF_EINVAL, "batch_draw_host: null pointer");
    const Philox4 w = draw_quad(make_perturb_key(seed, offset), item);
    ints_host[0] = draw_int(w.v[0], range0);
    ints_host[1] = draw_int(w.v[1], range1);
    uniforms_host[0] = philox_uniform(w.v[2]);
    uniforms_host[1] = philox_uniform(w.v[3]);
    return SAMNERF_OK;
}

}  // extern "C"
