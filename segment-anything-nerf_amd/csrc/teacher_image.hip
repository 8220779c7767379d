// teacher_image.hip -- the SAM teacher's input from a render that is already
// on the device (Trainer.train_step's cache-miss half, nerf/utils.py:1083-1085,
// and eval_step's, :1203-1208): what the reference does on the host between
// the render and image_encoder --
//     (pred_rgb.cpu().numpy() * 255).astype(uint8)
//     ResizeLongestSide(1024).apply_image     PIL's 8-bit bilinear resize
//     Sam.preprocess                           (x - mean) / std, zero padding
// -- as three launches on the caller's stream: no copy to the host, no
// allocation, no synchronisation.
//
//   k_ti_coeffs   one thread per output index of each axis: PIL's precompute_
//                 coeffs in double (the expressions of include/samnerf_hip.h,
//                 truncating casts), the first tap, the tap count and the
//                 22-bit integer weights -> workspace
//   k_ti_rows     the horizontal pass, quantising each tap as it is read
//                 (quantise.h): fp32 [H][W][3] -> uint8 [H][ow][3] in the
//                 workspace
//   k_ti_cols     the vertical pass, one thread per (y, x) of the S x S plane:
//                 the uint8 image [oh][ow][3] and / or the normalised planes
//                 [3][S][S], +0 right of and below the image; a wave's stores
//                 run along x
//
// A pass is acc = 2^21 + sum k * pixel in int32 and clamp(acc >> 22, 0, 255);
// the weights of an index sum to 2^22 up to half a unit each, so acc stays
// below 255 * (2^22 + 2^12) + 2^21 < 2^31.  3 MB in and 12 MB out at SAM's
// size: the work is bound by its launches, not by the memory system, and the
// passes are kept as simple as that allows.
#include <cmath>

#include "quantise.h"
#include "samnerf_common.h"

using namespace samnerf;

namespace {

constexpr uint32_t kT = 256;
constexpr uint32_t kMaxSide = 8192;
constexpr int kBits = 22;                    // PIL's PRECISION_BITS = 32 - 8 - 2

// one axis of the resize in the workspace
struct Axis {
    uint32_t n_in, n_out, ksize;             // ksize: the taps a table row holds
    int2* bounds;                            // [n_out]  first tap, tap count
    int32_t* kk;                             // [n_out][ksize]
};

// 2 ceil(support) + 1, as PIL sizes its table: no index has more taps
uint32_t taps_per_index(uint32_t n_in, uint32_t n_out) {
    const double scale = (double)n_in / (double)n_out;
    const double support = scale < 1.0 ? 1.0 : scale;
    return (uint32_t)(int)ceil(support) * 2u + 1u;
}

struct Layout {
    Axis x, y;
    uint8_t* rows;                           // [H][ow][3]
    size_t bytes;
};

Layout layout(void* ws, uint32_t H, uint32_t W, uint32_t oh, uint32_t ow) {
    Layout l{};
    Carver c(ws);
    l.x.n_in = W; l.x.n_out = ow; l.x.ksize = taps_per_index(W, ow);
    l.y.n_in = H; l.y.n_out = oh; l.y.ksize = taps_per_index(H, oh);
    l.x.bounds = c.take<int2>((size_t)2 * ow);
    l.y.bounds = c.take<int2>((size_t)2 * oh);
    l.x.kk = c.take<int32_t>((size_t)ow * l.x.ksize);
    l.y.kk = c.take<int32_t>((size_t)oh * l.y.ksize);
    l.rows = c.take<uint8_t>(((size_t)H * ow * 3 + 3) / 4);
    l.bytes = c.bytes();
    return l;
}

struct Params {
    uint32_t H, W, oh, ow, S;
    float mean[3], std[3];
    const float* rgb;
    uint8_t* out_u8;
    float* out_input;
    Layout l;
};

__device__ __forceinline__ void coeffs_axis(const Axis& A, uint32_t xx) {
    if (xx >= A.n_out) return;
    const double scale = (double)A.n_in / (double)A.n_out;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = fs, ss = 1.0 / fs;
    const double center = ((double)xx + 0.5) * scale;
    int xmin = (int)(center - support + 0.5);
    xmin = xmin < 0 ? 0 : xmin;
    int xmax = (int)(center + support + 0.5);
    xmax = xmax > (int)A.n_in ? (int)A.n_in : xmax;
    int n = xmax - xmin;
    n = n < 0 ? 0 : (n > (int)A.ksize ? (int)A.ksize : n);      // never taken: 1 <= n <= ksize
    int32_t* k = A.kk + (size_t)xx * A.ksize;
    double ww = 0.0;
    for (int x = 0; x < n; ++x) {
        const double a = fabs(((double)(x + xmin) - center + 0.5) * ss);
        ww += a < 1.0 ? 1.0 - a : 0.0;
    }
    // the weights again rather than a table of doubles: the same expressions
    // give the same values
    for (int x = 0; x < n; ++x) {
        const double a = fabs(((double)(x + xmin) - center + 0.5) * ss);
        double w = a < 1.0 ? 1.0 - a : 0.0;
        if (ww != 0.0) w = w / ww;
        k[x] = (int32_t)(0.5 + w * 4194304.0);
    }
    A.bounds[xx] = make_int2(xmin, n);
}

__global__ void __launch_bounds__(kT) k_ti_coeffs(Params P) {
    const uint32_t i = blockIdx.x * kT + threadIdx.x;
    coeffs_axis(P.l.x, i);
    coeffs_axis(P.l.y, i);
}

__device__ __forceinline__ uint8_t clip8(int32_t acc) {
    const int32_t v = acc >> kBits;
    return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

__global__ void __launch_bounds__(kT) k_ti_rows(Params P) {
    const uint32_t xx = blockIdx.x * kT + threadIdx.x, y = blockIdx.y;
    if (xx >= P.ow) return;
    const int2 b = P.l.x.bounds[xx];
    const int32_t* k = P.l.x.kk + (size_t)xx * P.l.x.ksize;
    const float* src = P.rgb + ((size_t)y * P.W + (uint32_t)b.x) * 3u;
    int32_t a0 = 1 << (kBits - 1), a1 = a0, a2 = a0;
    for (int t = 0; t < b.y; ++t) {
        const int32_t kv = k[t];
        a0 += kv * (int32_t)to_u8(src[3 * t]);
        a1 += kv * (int32_t)to_u8(src[3 * t + 1]);
        a2 += kv * (int32_t)to_u8(src[3 * t + 2]);
    }
    uint8_t* o = P.l.rows + ((size_t)y * P.ow + xx) * 3u;
    o[0] = clip8(a0);
    o[1] = clip8(a1);
    o[2] = clip8(a2);
}

__global__ void __launch_bounds__(kT) k_ti_cols(Params P) {
    const uint32_t x = blockIdx.x * kT + threadIdx.x, y = blockIdx.y;
    const uint32_t side = P.out_input ? P.S : P.ow;         // the launch covers side x (S or oh)
    if (x >= side) return;
    const bool inside = y < P.oh && x < P.ow;
    float v[3] = {0.0f, 0.0f, 0.0f};
    if (inside) {
        const int2 b = P.l.y.bounds[y];
        const int32_t* k = P.l.y.kk + (size_t)y * P.l.y.ksize;
        const uint8_t* src = P.l.rows + ((size_t)(uint32_t)b.x * P.ow + x) * 3u;
        const size_t pitch = (size_t)P.ow * 3u;
        int32_t a0 = 1 << (kBits - 1), a1 = a0, a2 = a0;
        for (int t = 0; t < b.y; ++t) {
            const int32_t kv = k[t];
            const uint8_t* p = src + (size_t)t * pitch;
            a0 += kv * (int32_t)p[0];
            a1 += kv * (int32_t)p[1];
            a2 += kv * (int32_t)p[2];
        }
        const uint8_t q[3] = {clip8(a0), clip8(a1), clip8(a2)};
        if (P.out_u8) {
            uint8_t* o = P.out_u8 + ((size_t)y * P.ow + x) * 3u;
            o[0] = q[0];
            o[1] = q[1];
            o[2] = q[2];
        }
        // Sam.preprocess: one fp32 subtraction and one correctly rounded
        // fp32 division, not a multiply by the reciprocal
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = ((float)q[c] - P.mean[c]) / P.std[c];
    }
    if (P.out_input) {
        const size_t plane = (size_t)P.S * P.S, at = (size_t)y * P.S + x;
        P.out_input[at] = v[0];
        P.out_input[plane + at] = v[1];
        P.out_input[2 * plane + at] = v[2];
    }
}

bool side_ok(uint32_t n) { return n >= 1 && n <= kMaxSide; }

constexpr float kMean[3] = {123.675f, 116.28f, 103.53f};      // Sam.pixel_mean, pixel_std
constexpr float kStd[3] = {58.395f, 57.12f, 57.375f};

}  // namespace

extern "C" int samnerf_teacher_image_shape(uint32_t H, uint32_t W, uint32_t target, uint32_t* oh, uint32_t* ow) {
    if (!side_ok(H) || !side_ok(W) || !side_ok(target))
        return fail(SAMNERF_EINVAL, "teacher_image_shape: H, W and target must lie in [1, 8192]");
    if (!oh || !ow) return fail(SAMNERF_EINVAL, "teacher_image_shape: null oh / ow");
    // ResizeLongestSide.get_preprocess_shape, in double as Python computes it
    const double scale = (double)target * 1.0 / (double)(H > W ? H : W);
    *oh = (uint32_t)(int)((double)H * scale + 0.5);
    *ow = (uint32_t)(int)((double)W * scale + 0.5);
    return SAMNERF_OK;
}

extern "C" size_t samnerf_teacher_image_workspace_size(uint32_t H, uint32_t W, uint32_t oh, uint32_t ow) {
    if (!side_ok(H) || !side_ok(W) || !side_ok(oh) || !side_ok(ow)) return 0;
    return layout(nullptr, H, W, oh, ow).bytes;
}

extern "C" int samnerf_teacher_image(const float* rgb, uint32_t H, uint32_t W, uint32_t oh, uint32_t ow, uint32_t S,
                                     const float* mean, const float* std, uint8_t* out_u8, float* out_input,
                                     void* workspace, size_t workspace_bytes, samnerf_stream_t stream) {
    if (!side_ok(H) || !side_ok(W) || !side_ok(oh) || !side_ok(ow))
        return fail(SAMNERF_EINVAL, "teacher_image: H, W, oh and ow must lie in [1, 8192]");
    if (!rgb) return fail(SAMNERF_EINVAL, "teacher_image: null rgb");
    if (!out_u8 && !out_input) return fail(SAMNERF_EINVAL, "teacher_image: out_u8 and out_input are both null");
    if (out_input && (!side_ok(S) || S < (oh > ow ? oh : ow)))
        return fail(SAMNERF_EINVAL, "teacher_image: S = %u must lie in [max(oh, ow), 8192] = [%u, 8192]", S,
                    oh > ow ? oh : ow);
    Params P{};
    P.l = layout(workspace, H, W, oh, ow);
    if (!workspace || workspace_bytes < P.l.bytes)
        return fail(SAMNERF_EINVAL, "teacher_image: workspace of %zu bytes, %zu needed", workspace ? workspace_bytes : 0,
                    P.l.bytes);
    P.H = H; P.W = W; P.oh = oh; P.ow = ow; P.S = S;
    for (int c = 0; c < 3; ++c) {
        P.mean[c] = mean ? mean[c] : kMean[c];
        P.std[c] = std ? std[c] : kStd[c];
    }
    P.rgb = rgb; P.out_u8 = out_u8; P.out_input = out_input;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    int rc;
    k_ti_coeffs<<<div_up(oh > ow ? oh : ow, kT), kT, 0, s>>>(P);
    if ((rc = check_launch("teacher_image coefficients"))) return rc;
    k_ti_rows<<<dim3(div_up(ow, kT), H), kT, 0, s>>>(P);
    if ((rc = check_launch("teacher_image rows"))) return rc;
    const uint32_t gx = out_input ? S : ow, gy = out_input ? S : oh;
    k_ti_cols<<<dim3(div_up(gx, kT), gy), kT, 0, s>>>(P);
    return check_launch("teacher_image columns");
}
