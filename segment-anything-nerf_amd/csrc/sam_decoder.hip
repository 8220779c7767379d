// sam_decoder.hip -- SAM's prompt encoder and mask decoder for point prompts:
// what SamPredictor.predict_torch runs between the image embedding and the
// masks (prompt tokens, the two-way transformer, the upscaling, the
// hypernetwork products, the IoU head) and its postprocess, written from the
// published description of the model (include/samnerf_hip.h has the
// equations).  The image tokens are [g*g][256], token-major: the layout of the
// render's samvit, so a rendered map goes in as it is.
//
// Every product is an exact fp32 FMA with fp32 accumulation; sinf, cosf, expf
// and erff are the accurate library functions; every sum runs in a fixed
// order and nothing is added with an atomic: a call repeats bit for bit.
//
// A call is 44 launches:
//   k_sd_src      features (+ bilinear resize to the long side g, zero pad)
//                 + no_mask_embed -> k [N][256]
//   k_sd_tokens   iou / mask / point / padding tokens -> query_pe, q
//   k_sd_lin      a row-tiled fp32 GEMM Y = act((A + A2) Wt + b) + R over up
//                 to eight jobs a launch: the q / k / v projections of an
//                 attention go out together, the 2,048-wide MLP's second
//                 layer as eight slices of the hidden dimension whose
//                 partial sums the next norm adds in slice order
//   k_sd_attn_tok few queries over many keys (token self-attention, token ->
//                 image): online-softmax partials (max, sum, acc) per thread,
//                 merged over the wave as a butterfly and over the waves in
//                 index order; the image's keys in eight slices, a workgroup
//                 each, whose partials k_sd_attn_merge combines in slice order
//   k_sd_attn_img one thread per image token and head over the T token keys
//   k_sd_ln       LayerNorm of a row (a wave each), of the sum of its parts
//   k_sd_up       per image token: LayerNorm2d, GELU, the second transposed
//                 convolution, GELU and the four hypernetwork products; the
//                 [32][4g][4g] tensor is never written
// and samnerf_sam_masks is one more: both resizes of the postprocess as 16 taps
// per output pixel, the S x S intermediate never written.
#include <atomic>
#include <cmath>
#include <vector>

#include "samnerf_common.h"

using namespace samnerf;

namespace {

constexpr uint32_t kT = 256;          // threads of every workgroup here
constexpr uint32_t kC = 256;          // SAM's transformer width
constexpr uint32_t kHeads = 8;
constexpr uint32_t kHid = 2048;       // the MLP's hidden width
constexpr uint32_t kMaxTok = 64;      // T = P + 6 <= 64
constexpr uint32_t kMaxP = 58;
constexpr uint32_t kSplit = 8;        // slices of the MLP's hidden dimension
constexpr uint32_t kMaxJobs = 8;
constexpr uint32_t kKeySlices = 8;    // of the token -> image attention; g*g is a multiple of 64
constexpr uint32_t kW2Row = 4 * 36;   // k_sd_up's LDS row: 4 sub-pixels x (32 + 4 pad)

// ---------------------------------------------------------------- layout --

struct Lin {
    size_t w, b;          // float offsets in the pack: Wt [in][out], b [out]
    uint32_t in, out;
};
struct Attn {
    Lin q, k, v, o;
};
struct Layer {
    Attn self, t2i, i2t;
    size_t nw[4], nb[4];
    Lin lin1, lin2;
};
enum Kind { kCopy, kTranspose, kConvT, kTile4 };
struct Entry {
    size_t raw, pack;
    uint32_t rows, cols;  // kTranspose: raw [rows][cols] -> pack [cols][rows]
    Kind kind;            // kConvT: raw [cols][rows/4][4] -> pack [cols][4][rows/4]; kTile4: raw [cols] four times
};
struct Layout {
    size_t G, pt[2], nap, nomask, iou, mtok;
    Layer L[2];
    Attn fin;
    size_t nfw, nfb;
    Lin up0;              // [256] -> [4][64]
    size_t uplnw, uplnb;
    size_t up1w, up1b;    // [64][4][32], [4][32]
    Lin hyp[4][3], iouh[3];
    size_t ipe;           // [g*g][256]
    size_t raw_count, pack_count;
    std::vector<Entry> entries;
};

struct Walker {
    Layout& l;
    size_t raw = 0, pack = 0;
    size_t put(uint32_t rows, uint32_t cols, Kind kind) {
        const size_t n_raw = kind == kTile4 ? cols : (size_t)rows * cols;
        const size_t n_pack = kind == kTile4 ? (size_t)4 * cols : n_raw;
        l.entries.push_back({raw, pack, rows, cols, kind});
        const size_t at = pack;
        raw += n_raw;
        pack += (n_pack + 3) & ~(size_t)3;         // every piece 16-byte aligned
        return at;
    }
    size_t vec(uint32_t n) { return put(1, n, kCopy); }
    Lin lin(uint32_t in, uint32_t out) {
        Lin r;
        r.in = in;
        r.out = out;
        r.w = put(out, in, kTranspose);
        r.b = vec(out);
        return r;
    }
    Attn attn(uint32_t inner) { return {lin(kC, inner), lin(kC, inner), lin(kC, inner), lin(inner, kC)}; }
};

// The raw order (include/samnerf_hip.h) and the pack's, walked once.
Layout make_layout(uint32_t g) {
    Layout l{};
    Walker w{l};
    l.G = w.put(2, 128, kCopy);
    l.pt[0] = w.vec(kC);
    l.pt[1] = w.vec(kC);
    l.nap = w.vec(kC);
    l.nomask = w.vec(kC);
    l.iou = w.vec(kC);
    l.mtok = w.put(4, kC, kCopy);
    for (int i = 0; i < 2; ++i) {
        Layer& L = l.L[i];
        L.self = w.attn(kC);
        L.t2i = w.attn(kC / 2);
        L.i2t = w.attn(kC / 2);
        for (int n = 0; n < 4; ++n) {
            L.nw[n] = w.vec(kC);
            L.nb[n] = w.vec(kC);
        }
        L.lin1 = w.lin(kC, kHid);
        L.lin2 = w.lin(kHid, kC);
    }
    l.fin = w.attn(kC / 2);
    l.nfw = w.vec(kC);
    l.nfb = w.vec(kC);
    l.up0.in = kC;
    l.up0.out = 256;
    l.up0.w = w.put(256, kC, kConvT);              // raw [256][64][2][2] -> [256][4][64]
    l.up0.b = w.put(1, 64, kTile4);
    l.uplnw = w.vec(64);
    l.uplnb = w.vec(64);
    l.up1w = w.put(128, 64, kConvT);               // raw [64][32][2][2] -> [64][4][32]
    l.up1b = w.put(1, 32, kTile4);
    for (int i = 0; i < 4; ++i) {
        l.hyp[i][0] = w.lin(kC, kC);
        l.hyp[i][1] = w.lin(kC, kC);
        l.hyp[i][2] = w.lin(kC, 32);
    }
    l.iouh[0] = w.lin(kC, kC);
    l.iouh[1] = w.lin(kC, kC);
    l.iouh[2] = w.lin(kC, 4);
    l.raw_count = w.raw;
    l.ipe = w.pack;
    l.pack_count = w.pack + (size_t)g * g * kC;
    return l;
}

bool grid_ok(uint32_t g) { return g >= 8 && g <= 64 && g % 8 == 0; }
bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// The taps of destination cell d of an axis resized from n_in to n_out cells:
// feat_loss.hip's bilinear_tap (the library's one definition, samnerf_hip.h).
__host__ __device__ inline void bilinear_tap(uint32_t n_in, uint32_t n_out, uint32_t d, uint32_t& i0, uint32_t& i1,
                                             float& l1) {
    const float scale = (float)n_in / (float)n_out;
    float src = scale * ((float)d + 0.5f) - 0.5f;
    src = src < 0.0f ? 0.0f : src;
    uint32_t i = (uint32_t)(int)src;
    i = i < n_in - 1u ? i : n_in - 1u;
    i0 = i;
    i1 = i + (i < n_in - 1u ? 1u : 0u);
    l1 = src - (float)i;
}

// ------------------------------------------------------------------ pack --

__global__ void __launch_bounds__(kT) k_sd_pack(const float* __restrict__ raw, float* __restrict__ pack, uint32_t rows,
                                                uint32_t cols, int kind) {
    const uint32_t n = kind == kTile4 ? 4u * cols : rows * cols;
    for (uint32_t i = blockIdx.x * kT + threadIdx.x; i < n; i += gridDim.x * kT) {
        uint32_t src = i;
        if (kind == kTranspose) {                      // pack [cols][rows]
            const uint32_t c = i / rows, r = i - c * rows;
            src = r * cols + c;
        } else if (kind == kConvT) {                   // pack [cols][4][rows / 4], raw [cols][rows / 4][4]
            const uint32_t no = rows / 4u;
            const uint32_t c = i / rows, rem = i - c * rows, ij = rem / no, o = rem - ij * no;
            src = (c * no + o) * 4u + ij;
        } else if (kind == kTile4) {
            src = i % cols;
        }
        pack[i] = raw[src];
    }
}

// pe(c), c = (cx, cy) in [0, 1]^2: channel ch of cat(sin v, cos v),
// v = ((2 cx - 1) G[0][j] + (2 cy - 1) G[1][j]) * 2 pi
__device__ __forceinline__ float pos_code(const float* __restrict__ G, float cx, float cy, uint32_t ch) {
    const uint32_t j = ch & 127u;
    const float x = 2.0f * cx - 1.0f, y = 2.0f * cy - 1.0f;
    const float v = (x * G[j] + y * G[128u + j]) * 6.283185307179586f;
    return ch < 128u ? sinf(v) : cosf(v);
}

__global__ void __launch_bounds__(kT) k_sd_image_pe(const float* __restrict__ G, float* __restrict__ ipe, uint32_t g) {
    const uint32_t n = blockIdx.x, y = n / g, x = n - y * g;
    ipe[(size_t)n * kC + threadIdx.x] =
        pos_code(G, ((float)x + 0.5f) / (float)g, ((float)y + 0.5f) / (float)g, threadIdx.x);
}

// ---------------------------------------------------------- src, tokens --

struct SrcArgs {
    const float* feat;
    const float* nomask;
    float* k;
    uint32_t g, h, w, vh, vw;   // h == 0: feat is [g*g][256]; else [h][w][256] resized to vh x vw, zero padded
};

__global__ void __launch_bounds__(kT) k_sd_src(SrcArgs a) {
    const uint32_t n = blockIdx.x * 4u + (threadIdx.x >> 6), c4 = threadIdx.x & 63u;
    if (n >= a.g * a.g) return;
    const float4 e = reinterpret_cast<const float4*>(a.nomask)[c4];
    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (a.h == 0u) {
        const float* p = a.feat + (size_t)n * kC + 4u * c4;
        v = make_float4(p[0], p[1], p[2], p[3]);
    } else {
        const uint32_t y = n / a.g, x = n - y * a.g;
        if (y < a.vh && x < a.vw) {
            uint32_t y0, y1, x0, x1;
            float ly, lx;
            bilinear_tap(a.h, a.vh, y, y0, y1, ly);
            bilinear_tap(a.w, a.vw, x, x0, x1, lx);
            const float my = 1.0f - ly, mx = 1.0f - lx;
            const float* p00 = a.feat + ((size_t)y0 * a.w + x0) * kC + 4u * c4;
            const float* p01 = a.feat + ((size_t)y0 * a.w + x1) * kC + 4u * c4;
            const float* p10 = a.feat + ((size_t)y1 * a.w + x0) * kC + 4u * c4;
            const float* p11 = a.feat + ((size_t)y1 * a.w + x1) * kC + 4u * c4;
            float r[4];
#pragma unroll
            for (int i = 0; i < 4; ++i)
                r[i] = my * (mx * p00[i] + lx * p01[i]) + ly * (mx * p10[i] + lx * p11[i]);
            v = make_float4(r[0], r[1], r[2], r[3]);
        }
    }
    reinterpret_cast<float4*>(a.k)[(size_t)n * 64u + c4] = make_float4(v.x + e.x, v.y + e.y, v.z + e.z, v.w + e.w);
}

struct TokArgs {
    const float* pack;
    size_t G, pt0, pt1, nap, iou, mtok;
    float* tok;
    float* q;
    uint32_t P, S;
    int32_t x[kMaxP], y[kMaxP], label[kMaxP];
};

__global__ void __launch_bounds__(kT) k_sd_tokens(TokArgs a) {
    const uint32_t row = blockIdx.x, c = threadIdx.x;
    float v;
    if (row == 0u) {
        v = a.pack[a.iou + c];
    } else if (row < 5u) {
        v = a.pack[a.mtok + (size_t)(row - 1u) * kC + c];
    } else if (row < 5u + a.P) {
        const uint32_t p = row - 5u;
        const float S = (float)a.S;
        v = pos_code(a.pack + a.G, ((float)a.x[p] + 0.5f) / S, ((float)a.y[p] + 0.5f) / S, c) +
            a.pack[(a.label[p] ? a.pt1 : a.pt0) + c];
    } else {
        v = a.pack[a.nap + c];
    }
    a.tok[(size_t)row * kC + c] = v;
    a.q[(size_t)row * kC + c] = v;
}

// ------------------------------------------------------------------ GEMM --

struct LinJob {
    const float* A;     // [M][lda], 16-byte aligned rows
    const float* A2;    // [M][lda] added to A, or null
    const float* Wt;    // [K][O]
    const float* b;     // [O] or null
    const float* R;     // [M][O] added after the activation, or null
    float* Y;           // [M][O]
    uint32_t M, K, O, lda, relu;
};
struct LinJobs {
    LinJob j[kMaxJobs];
};

// TM rows x 64 columns a workgroup, K in steps of 32 through LDS with the next
// step's loads in flight over the FMAs; a thread holds TM / 16 rows x 4 columns.
// Every output is one chain of FMAs over k = 0 .. K - 1.
template <int TM>
__global__ void __launch_bounds__(kT) k_sd_lin(LinJobs J) {
    constexpr int KC = 32, TN = 64, RM = TM / 16;
    constexpr int A4 = TM * KC / 4, NA = (A4 + 255) / 256, NW = KC * TN / 4 / 256;
    const LinJob& j = J.j[blockIdx.z];
    const uint32_t row0 = blockIdx.y * TM, col0 = blockIdx.x * TN;
    if (row0 >= j.M || col0 >= j.O) return;
    __shared__ float4 As4[KC * (TM + 4) / 4];
    __shared__ float4 Ws4[KC * TN / 4];
    float* As = reinterpret_cast<float*>(As4);
    const uint32_t t = threadIdx.x, ty = t >> 4, tx = t & 15u;
    float4 ra[NA], rw[NW];
    auto load = [&](uint32_t k0) {
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            const uint32_t idx = t + 256u * i;
            float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (idx < (uint32_t)A4) {
                const uint32_t r = row0 + idx / (KC / 4), k = k0 + (idx % (KC / 4)) * 4u;
                if (r < j.M) {
                    v = *reinterpret_cast<const float4*>(j.A + (size_t)r * j.lda + k);
                    if (j.A2) {
                        const float4 u = *reinterpret_cast<const float4*>(j.A2 + (size_t)r * j.lda + k);
                        v = make_float4(v.x + u.x, v.y + u.y, v.z + u.z, v.w + u.w);
                    }
                }
            }
            ra[i] = v;
        }
#pragma unroll
        for (int i = 0; i < NW; ++i) {
            const uint32_t idx = t + 256u * i, k = k0 + idx / (TN / 4), col = col0 + (idx % (TN / 4)) * 4u;
            rw[i] = col < j.O ? *reinterpret_cast<const float4*>(j.Wt + (size_t)k * j.O + col)
                              : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        }
    };
    float acc[RM][4];
#pragma unroll
    for (int r = 0; r < RM; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[r][c] = 0.0f;
    load(0);
    for (uint32_t k0 = 0; k0 < j.K; k0 += KC) {
        __syncthreads();                                   // the last step's readers are done
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            const uint32_t idx = t + 256u * i;
            if (idx < (uint32_t)A4) {
                const uint32_t r = idx / (KC / 4), k = (idx % (KC / 4)) * 4u;
                As[(k + 0u) * (TM + 4) + r] = ra[i].x;
                As[(k + 1u) * (TM + 4) + r] = ra[i].y;
                As[(k + 2u) * (TM + 4) + r] = ra[i].z;
                As[(k + 3u) * (TM + 4) + r] = ra[i].w;
            }
        }
#pragma unroll
        for (int i = 0; i < NW; ++i) Ws4[t + 256u * i] = rw[i];
        __syncthreads();
        if (k0 + KC < j.K) load(k0 + KC);
#pragma unroll
        for (int kk = 0; kk < KC; ++kk) {
            const float4 w = Ws4[kk * (TN / 4) + tx];
            float a[RM];
            if constexpr (RM == 4) {
                const float4 v = As4[(kk * (TM + 4) + ty * 4) / 4];
                a[0] = v.x; a[1] = v.y; a[2] = v.z; a[3] = v.w;
            } else {
#pragma unroll
                for (int r = 0; r < RM; ++r) a[r] = As[kk * (TM + 4) + ty * RM + r];
            }
#pragma unroll
            for (int r = 0; r < RM; ++r) {
                acc[r][0] = __builtin_fmaf(a[r], w.x, acc[r][0]);
                acc[r][1] = __builtin_fmaf(a[r], w.y, acc[r][1]);
                acc[r][2] = __builtin_fmaf(a[r], w.z, acc[r][2]);
                acc[r][3] = __builtin_fmaf(a[r], w.w, acc[r][3]);
            }
        }
    }
    const uint32_t col = col0 + tx * 4u;
    if (col >= j.O) return;
    float4 b = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (j.b) b = *reinterpret_cast<const float4*>(j.b + col);
#pragma unroll
    for (int r = 0; r < RM; ++r) {
        const uint32_t row = row0 + ty * RM + r;
        if (row >= j.M) continue;
        float4 v = make_float4(acc[r][0] + b.x, acc[r][1] + b.y, acc[r][2] + b.z, acc[r][3] + b.w);
        if (j.relu) v = make_float4(fmaxf(v.x, 0.0f), fmaxf(v.y, 0.0f), fmaxf(v.z, 0.0f), fmaxf(v.w, 0.0f));
        if (j.R) {
            const float4 u = *reinterpret_cast<const float4*>(j.R + (size_t)row * j.O + col);
            v = make_float4(v.x + u.x, v.y + u.y, v.z + u.z, v.w + u.w);
        }
        *reinterpret_cast<float4*>(j.Y + (size_t)row * j.O + col) = v;
    }
}

// ------------------------------------------------------------- attention --

// One softmax partial: the running maximum, the sum of exp(s - m) and the
// weighted values.  merge() is the flash-attention combination; a partial
// that saw no key has m = -inf and weight 0.
__device__ __forceinline__ float part_weight(float m, float mn) { return m == -INFINITY ? 0.0f : expf(m - mn); }

// QB queries x one head x one slice of the keys a workgroup (gridDim.z slices
// of Nk / gridDim.z keys); thread t takes keys t, t + 256, ... of the slice in
// that order, the loads of U of them in flight at once.  One slice: the
// result goes to out.  Several: the slice's partial (acc [DH], max, sum) goes
// to part [slice][T][8][DH + 2] and k_sd_attn_merge combines them in slice
// order -- a few queries over 4,096 keys would otherwise run on T / QB x 8
// workgroups, each reading every key's head slice.
template <int DH, int QB, int U>
__global__ void __launch_bounds__(kT) k_sd_attn_tok(const float* __restrict__ Q, const float* __restrict__ K,
                                                    const float* __restrict__ V, float* __restrict__ out,
                                                    float* __restrict__ part, uint32_t T, uint32_t Nk) {
    constexpr uint32_t inner = kHeads * DH;
    __shared__ float sh[4][QB][DH + 2];
    const uint32_t h = blockIdx.y, q0 = blockIdx.x * QB, t = threadIdx.x;
    float q[QB][DH], acc[QB][DH], m[QB], l[QB];
#pragma unroll
    for (int qi = 0; qi < QB; ++qi) {
        const uint32_t row = q0 + qi < T ? q0 + qi : T - 1u;
        load_row<DH>(Q + (size_t)row * inner + h * DH, q[qi]);
        m[qi] = -INFINITY;
        l[qi] = 0.0f;
#pragma unroll
        for (int d = 0; d < DH; ++d) acc[qi][d] = 0.0f;
    }
    const float root = sqrtf((float)DH);
    const uint32_t per = Nk / gridDim.z, k_lo = blockIdx.z * per, k_hi = k_lo + per;
    for (uint32_t j0 = k_lo + t; j0 < k_hi; j0 += U * kT) {
        float k[U][DH], v[U][DH];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t jk = j0 + u * kT < k_hi ? j0 + u * kT : k_hi - 1u;
            load_row<DH>(K + (size_t)jk * inner + h * DH, k[u]);
            load_row<DH>(V + (size_t)jk * inner + h * DH, v[u]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (j0 + u * kT >= k_hi) break;
#pragma unroll
            for (int qi = 0; qi < QB; ++qi) {
                float s = 0.0f;
#pragma unroll
                for (int d = 0; d < DH; ++d) s = __builtin_fmaf(q[qi][d], k[u][d], s);
                s = s / root;
                const float mn = fmaxf(m[qi], s);
                const float c = part_weight(m[qi], mn), p = expf(s - mn);
                l[qi] = l[qi] * c + p;
#pragma unroll
                for (int d = 0; d < DH; ++d) acc[qi][d] = __builtin_fmaf(p, v[u][d], acc[qi][d] * c);
                m[qi] = mn;
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int qi = 0; qi < QB; ++qi) {
            const float mo = __shfl_xor(m[qi], o, 64), lo = __shfl_xor(l[qi], o, 64);
            const float mn = fmaxf(m[qi], mo);
            const float c1 = part_weight(m[qi], mn), c2 = part_weight(mo, mn);
            l[qi] = l[qi] * c1 + lo * c2;
#pragma unroll
            for (int d = 0; d < DH; ++d) acc[qi][d] = acc[qi][d] * c1 + __shfl_xor(acc[qi][d], o, 64) * c2;
            m[qi] = mn;
        }
    }
    if ((t & 63u) == 0u) {
#pragma unroll
        for (int qi = 0; qi < QB; ++qi) {
#pragma unroll
            for (int d = 0; d < DH; ++d) sh[t >> 6][qi][d] = acc[qi][d];
            sh[t >> 6][qi][DH] = m[qi];
            sh[t >> 6][qi][DH + 1] = l[qi];
        }
    }
    __syncthreads();
    if (t < QB * DH) {
        const uint32_t qi = t / DH, d = t % DH;
        float mm = sh[0][qi][DH], ll = sh[0][qi][DH + 1], a = sh[0][qi][d];
        for (int w = 1; w < 4; ++w) {
            const float mo = sh[w][qi][DH], mn = fmaxf(mm, mo);
            const float c1 = part_weight(mm, mn), c2 = part_weight(mo, mn);
            ll = ll * c1 + sh[w][qi][DH + 1] * c2;
            a = a * c1 + sh[w][qi][d] * c2;
            mm = mn;
        }
        if (q0 + qi >= T) return;
        if (gridDim.z == 1u) {
            out[(size_t)(q0 + qi) * inner + h * DH + d] = a / ll;
        } else {
            float* p = part + (((size_t)blockIdx.z * T + q0 + qi) * kHeads + h) * (DH + 2);
            p[d] = a;
            if (d == 0u) {
                p[DH] = mm;
                p[DH + 1] = ll;
            }
        }
    }
}

// The key slices' partials of the token -> image attention in slice order: a
// workgroup a query, a thread one of its 8 x 16 outputs.
__global__ void __launch_bounds__(128) k_sd_attn_merge(const float* __restrict__ part, float* __restrict__ out,
                                                       uint32_t T, uint32_t slices) {
    constexpr uint32_t DH = 16;
    const uint32_t q = blockIdx.x, h = threadIdx.x >> 4, d = threadIdx.x & 15u;
    const size_t stride = (size_t)T * kHeads * (DH + 2);
    const float* p = part + ((size_t)q * kHeads + h) * (DH + 2);
    float mm = p[DH], ll = p[DH + 1], a = p[d];
    for (uint32_t z = 1; z < slices; ++z) {
        p += stride;
        const float mo = p[DH], mn = fmaxf(mm, mo);
        const float c1 = part_weight(mm, mn), c2 = part_weight(mo, mn);
        ll = ll * c1 + p[DH + 1] * c2;
        a = a * c1 + p[d] * c2;
        mm = mn;
    }
    out[(size_t)q * 128u + h * DH + d] = a / ll;
}

// Image -> token: a thread is one image token and one head (16 wide) over the
// T token keys in index order.
__global__ void __launch_bounds__(kT) k_sd_attn_img(const float* __restrict__ Q, const float* __restrict__ K,
                                                    const float* __restrict__ V, float* __restrict__ out, uint32_t N,
                                                    uint32_t T) {
    constexpr uint32_t DH = 16, inner = 128;
    __shared__ float4 Ks[kMaxTok * 4], Vs[kMaxTok * 4];
    const uint32_t h = blockIdx.y, t = threadIdx.x;
    for (uint32_t i = t; i < T * 4u; i += kT) {
        const size_t at = (size_t)(i >> 2) * inner + h * DH + (i & 3u) * 4u;
        Ks[i] = *reinterpret_cast<const float4*>(K + at);
        Vs[i] = *reinterpret_cast<const float4*>(V + at);
    }
    __syncthreads();
    const uint32_t n = blockIdx.x * kT + t;
    if (n >= N) return;
    float q[DH], acc[DH];
    load_row<DH>(Q + (size_t)n * inner + h * DH, q);
#pragma unroll
    for (int d = 0; d < (int)DH; ++d) acc[d] = 0.0f;
    float m = -INFINITY, l = 0.0f;
    const float* kf = reinterpret_cast<const float*>(Ks);
    const float* vf = reinterpret_cast<const float*>(Vs);
    for (uint32_t tt = 0; tt < T; ++tt) {
        float s = 0.0f;
#pragma unroll
        for (int d = 0; d < (int)DH; ++d) s = __builtin_fmaf(q[d], kf[tt * DH + d], s);
        s = s / 4.0f;
        const float mn = fmaxf(m, s);
        const float c = part_weight(m, mn), p = expf(s - mn);
        l = l * c + p;
#pragma unroll
        for (int d = 0; d < (int)DH; ++d) acc[d] = __builtin_fmaf(p, vf[tt * DH + d], acc[d] * c);
        m = mn;
    }
    float4* o = reinterpret_cast<float4*>(out + (size_t)n * inner + h * DH);
#pragma unroll
    for (int d = 0; d < 4; ++d)
        o[d] = make_float4(acc[4 * d] / l, acc[4 * d + 1] / l, acc[4 * d + 2] / l, acc[4 * d + 3] / l);
}

// --------------------------------------------------------------- LayerNorm --

// A wave a row of 256: x = the parts added in index order, then the norm
// (biased variance, eps 1e-5).  Y may be X.
__global__ void __launch_bounds__(kT) k_sd_ln(const float* X, uint32_t parts, size_t part_stride,
                                              const float* __restrict__ w, const float* __restrict__ b, float* Y,
                                              uint32_t M) {
    const uint32_t row = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (row >= M) return;
    float4 x = reinterpret_cast<const float4*>(X + (size_t)row * kC)[lane];
    for (uint32_t p = 1; p < parts; ++p) {
        const float4 u = reinterpret_cast<const float4*>(X + p * part_stride + (size_t)row * kC)[lane];
        x = make_float4(x.x + u.x, x.y + u.y, x.z + u.z, x.w + u.w);
    }
    float s = (x.x + x.y) + (x.z + x.w);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    const float mean = s / 256.0f;
    const float4 d = make_float4(x.x - mean, x.y - mean, x.z - mean, x.w - mean);
    float v = (d.x * d.x + d.y * d.y) + (d.z * d.z + d.w * d.w);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    const float rstd = 1.0f / sqrtf(v / 256.0f + 1e-5f);
    const float4 ww = reinterpret_cast<const float4*>(w)[lane], bb = reinterpret_cast<const float4*>(b)[lane];
    reinterpret_cast<float4*>(Y + (size_t)row * kC)[lane] =
        make_float4(d.x * rstd * ww.x + bb.x, d.y * rstd * ww.y + bb.y, d.z * rstd * ww.z + bb.z,
                    d.w * rstd * ww.w + bb.w);
}

// --------------------------------------------------------------- upscale --

__device__ __forceinline__ float gelu(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752440f)); }

// u1 [N][4][64]: the first transposed convolution of every image token, pixel
// ij = 2 i + j of its 2 x 2 block.  A thread is (token, ij, sub-pixel): the
// pixel's LayerNorm2d (eps 1e-6) and GELU, the 32 channels of its sub-pixel
// of the second transposed convolution, GELU, the four hypernetwork products.
__global__ void __launch_bounds__(kT) k_sd_up(const float* __restrict__ u1, const float* __restrict__ lnw,
                                              const float* __restrict__ lnb, const float* __restrict__ w2,
                                              const float* __restrict__ b2, const float* __restrict__ hyp,
                                              float* __restrict__ low, uint32_t g) {
    __shared__ float4 W4[64 * kW2Row / 4];
    __shared__ float4 H4[4 * 32 / 4], B4[32 / 4];
    __shared__ float Xs[64][68];                              // (token, ij) rows, 4 floats of padding
    const uint32_t t = threadIdx.x;
    for (uint32_t i = t; i < 64u * 128u / 4u; i += kT) {       // w2 [64][4][32]
        const uint32_t c = i / 32u, rem = i % 32u, sub = rem / 8u, o4 = rem % 8u;
        W4[(c * kW2Row + sub * 36u) / 4u + o4] = reinterpret_cast<const float4*>(w2)[i];
    }
    if (t < 32u) H4[t] = reinterpret_cast<const float4*>(hyp)[t];
    if (t < 8u) B4[t] = reinterpret_cast<const float4*>(b2)[t];      // the bias of one sub-pixel: b2 is tiled
    // g * g is a multiple of 64, so every workgroup has its 16 tokens
    const uint32_t pair = t >> 2, sub = t & 3u;
    const uint32_t n = blockIdx.x * 16u + (pair >> 2), ij = pair & 3u;
    {
        // the pixel's norm: the four threads of a pixel take 16 channels each
        float v[16];
        const float4* src = reinterpret_cast<const float4*>(u1 + ((size_t)n * 4u + ij) * 64u + sub * 16u);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float4 q = src[i];
            v[4 * i] = q.x; v[4 * i + 1] = q.y; v[4 * i + 2] = q.z; v[4 * i + 3] = q.w;
        }
        float s = 0.0f;
#pragma unroll
        for (int i = 0; i < 16; ++i) s += v[i];
        s += __shfl_xor(s, 1, 64);
        s += __shfl_xor(s, 2, 64);
        const float mean = s / 64.0f;
        float var = 0.0f;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            v[i] -= mean;
            var = __builtin_fmaf(v[i], v[i], var);
        }
        var += __shfl_xor(var, 1, 64);
        var += __shfl_xor(var, 2, 64);
        const float rstd = 1.0f / sqrtf(var / 64.0f + 1e-6f);
#pragma unroll 4
        for (int i = 0; i < 16; ++i) {
            const uint32_t c = sub * 16u + i;
            Xs[pair][c] = gelu(lnw[c] * (v[i] * rstd) + lnb[c]);
        }
    }
    __syncthreads();
    float a[32];
#pragma unroll
    for (int o = 0; o < 32; ++o) a[o] = 0.0f;
#pragma unroll 2
    for (int c = 0; c < 64; ++c) {
        const float x = Xs[pair][c];
        const float4* wr = &W4[(c * kW2Row + sub * 36u) / 4u];
#pragma unroll
        for (int o4 = 0; o4 < 8; ++o4) {
            const float4 w = wr[o4];
            a[4 * o4 + 0] = __builtin_fmaf(x, w.x, a[4 * o4 + 0]);
            a[4 * o4 + 1] = __builtin_fmaf(x, w.y, a[4 * o4 + 1]);
            a[4 * o4 + 2] = __builtin_fmaf(x, w.z, a[4 * o4 + 2]);
            a[4 * o4 + 3] = __builtin_fmaf(x, w.w, a[4 * o4 + 3]);
        }
    }
    float m[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    const float* hf = reinterpret_cast<const float*>(H4);
    const float* bf = reinterpret_cast<const float*>(B4);
#pragma unroll
    for (int o = 0; o < 32; ++o) {
        const float y = gelu(a[o] + bf[o]);
#pragma unroll
        for (int k = 0; k < 4; ++k) m[k] = __builtin_fmaf(hf[k * 32 + o], y, m[k]);
    }
    const uint32_t ty = n / g, tx = n - ty * g, side = 4u * g;
    const uint32_t oy = 4u * ty + 2u * (ij >> 1) + (sub >> 1), ox = 4u * tx + 2u * (ij & 1u) + (sub & 1u);
#pragma unroll
    for (int k = 0; k < 4; ++k) low[((size_t)k * side + oy) * side + ox] = m[k];
}

// ----------------------------------------------------------- postprocess --

struct MaskArgs {
    const float* low;     // [M][L][L], L = 4 g
    float* logits;        // [M][H][W] or null
    uint8_t* mask;        // [M][H][W] or null
    uint32_t L, S, ih, iw, H, W;
};

// One output pixel: the 2 x 2 taps of the resize (ih, iw) -> (H, W), each a
// 2 x 2 tap of the resize L -> S.  The crop to (ih, iw) only bounds the taps.
__global__ void __launch_bounds__(kT) k_sd_masks(MaskArgs a) {
    const uint32_t i = blockIdx.x * kT + threadIdx.x;
    if (i >= a.H * a.W) return;
    const uint32_t Y = i / a.W, X = i - Y * a.W;
    uint32_t sy[2], sx[2];
    float wy[2], wx[2];
    bilinear_tap(a.ih, a.H, Y, sy[0], sy[1], wy[1]);
    bilinear_tap(a.iw, a.W, X, sx[0], sx[1], wx[1]);
    wy[0] = 1.0f - wy[1];
    wx[0] = 1.0f - wx[1];
    uint32_t y0[2], y1[2], x0[2], x1[2];
    float ly[2], lx[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        bilinear_tap(a.L, a.S, sy[k], y0[k], y1[k], ly[k]);
        bilinear_tap(a.L, a.S, sx[k], x0[k], x1[k], lx[k]);
    }
    const float* p = a.low + (size_t)blockIdx.y * a.L * a.L;
    float v[2][2];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const float mx = 1.0f - lx[c], my = 1.0f - ly[r];
            v[r][c] = my * (mx * p[y0[r] * a.L + x0[c]] + lx[c] * p[y0[r] * a.L + x1[c]]) +
                      ly[r] * (mx * p[y1[r] * a.L + x0[c]] + lx[c] * p[y1[r] * a.L + x1[c]]);
        }
    const float out = wy[0] * (wx[0] * v[0][0] + wx[1] * v[0][1]) + wy[1] * (wx[0] * v[1][0] + wx[1] * v[1][1]);
    const size_t at = (size_t)blockIdx.y * a.H * a.W + i;
    if (a.logits) a.logits[at] = out;
    if (a.mask) a.mask[at] = out > 0.0f ? 1 : 0;
}

// ------------------------------------------------------------- workspace --

struct Work {
    float *tok, *q, *x1, *tq, *tk, *tv, *ta, *ap, *hid, *part, *kim, *kx, *ik, *iv, *iq, *ia, *u1, *h1, *h2, *hyp;
    size_t bytes;
};

Work carve(void* ws, uint32_t g) {
    Work w{};
    Carver c(ws);
    const size_t N = (size_t)g * g, tokens = (size_t)kMaxTok * kC;
    w.tok = c.take(tokens);
    w.q = c.take(tokens);
    w.x1 = c.take(tokens);
    w.tq = c.take(tokens);
    w.tk = c.take(tokens);
    w.tv = c.take(tokens);
    w.ta = c.take(tokens);
    w.ap = c.take((size_t)kKeySlices * kMaxTok * kHeads * 18);
    w.hid = c.take((size_t)kMaxTok * kHid);
    w.part = c.take(kSplit * tokens);
    w.kim = c.take(N * kC);
    w.kx = c.take(N * kC);
    w.ik = c.take(N * 128);
    w.iv = c.take(N * 128);
    w.iq = c.take(N * 128);
    w.ia = c.take(N * 128);
    w.u1 = c.take(N * kC);
    w.h1 = c.take(5 * kC);
    w.h2 = c.take(5 * kC);
    w.hyp = c.take(4 * 32);
    w.bytes = c.bytes();
    return w;
}

std::atomic<int> g_launches{0};

// The launches of one call: counted, and the first failure kept.
struct Launcher {
    hipStream_t s;
    const float* pack;
    int rc = 0, count = 0;

    void done(const char* what) {
        ++count;
        if (!rc) rc = check_launch(what);
    }
    LinJob job(const float* A, const float* A2, const Lin& L, const float* R, float* Y, uint32_t M,
               bool relu = false) const {
        return {A, A2, pack + L.w, pack + L.b, R, Y, M, L.in, L.out, L.in, relu ? 1u : 0u};
    }
    void lin(const LinJob* jobs, uint32_t n) {
        if (rc) return;
        LinJobs J{};
        uint32_t maxM = 0, maxO = 0;
        for (uint32_t i = 0; i < n; ++i) {
            J.j[i] = jobs[i];
            maxM = jobs[i].M > maxM ? jobs[i].M : maxM;
            maxO = jobs[i].O > maxO ? jobs[i].O : maxO;
        }
        if (maxM > kMaxTok)
            k_sd_lin<32><<<dim3(div_up(maxO, 64), div_up(maxM, 32), n), kT, 0, s>>>(J);
        else
            k_sd_lin<16><<<dim3(div_up(maxO, 64), div_up(maxM, 16), n), kT, 0, s>>>(J);
        done("sam_decoder lin");
    }
    void ln(const float* X, uint32_t parts, size_t stride, size_t w, size_t b, float* Y, uint32_t M) {
        if (rc) return;
        k_sd_ln<<<div_up(M, 4), kT, 0, s>>>(X, parts, stride, pack + w, pack + b, Y, M);
        done("sam_decoder ln");
    }
};

const char* validate_points(const int32_t* labels, uint32_t P) {
    if (P < 1 || P > kMaxP) return "P must lie in [1, 58]";
    for (uint32_t i = 0; i < P; ++i)
        if (labels[i] != 0 && labels[i] != 1) return "labels must be 0 or 1";
    return nullptr;
}

}  // namespace

extern "C" size_t samnerf_sam_decoder_raw_count(void) { return make_layout(8).raw_count; }

extern "C" size_t samnerf_sam_decoder_pack_size(uint32_t g) {
    return grid_ok(g) ? make_layout(g).pack_count * sizeof(float) : 0;
}

extern "C" int samnerf_sam_decoder_pack(const float* raw, size_t raw_count, uint32_t g, void* pack, size_t pack_bytes,
                                        samnerf_stream_t stream) {
    if (!grid_ok(g)) return fail(SAMNERF_EINVAL, "sam_decoder_pack: g must be a multiple of 8 in [8, 64]");
    if (!raw || !pack) return fail(SAMNERF_EINVAL, "sam_decoder_pack: null raw / pack");
    if (!aligned16(pack)) return fail(SAMNERF_EINVAL, "sam_decoder_pack: pack must be 16-byte aligned");
    const Layout l = make_layout(g);
    if (raw_count != l.raw_count)
        return fail(SAMNERF_EINVAL, "sam_decoder_pack: raw holds %zu floats, %zu expected", raw_count, l.raw_count);
    if (pack_bytes < l.pack_count * sizeof(float))
        return fail(SAMNERF_EWORKSPACE, "sam_decoder_pack: pack of %zu bytes, %zu needed", pack_bytes,
                    l.pack_count * sizeof(float));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    float* p = static_cast<float*>(pack);
    int rc;
    for (const Entry& e : l.entries) {
        const size_t n = e.kind == kTile4 ? (size_t)4 * e.cols : (size_t)e.rows * e.cols;
        k_sd_pack<<<div_up(n, kT) < 1024u ? div_up(n, kT) : 1024u, kT, 0, s>>>(raw + e.raw, p + e.pack, e.rows, e.cols,
                                                                              (int)e.kind);
        if ((rc = check_launch("sam_decoder pack"))) return rc;
    }
    k_sd_image_pe<<<g * g, kT, 0, s>>>(p + l.G, p + l.ipe, g);
    return check_launch("sam_decoder image_pe");
}

extern "C" size_t samnerf_sam_decoder_workspace_size(uint32_t g) { return grid_ok(g) ? carve(nullptr, g).bytes : 0; }

extern "C" int samnerf_sam_decoder_launches(void) { return g_launches.load(); }

extern "C" int samnerf_sam_decoder(const void* pack, size_t pack_bytes, uint32_t g, const float* features, uint32_t h,
                                   uint32_t w, const int32_t* points, const int32_t* labels, uint32_t P,
                                   float* low_res, float* iou, void* ws, size_t ws_bytes, samnerf_stream_t stream) {
    if (!grid_ok(g)) return fail(SAMNERF_EINVAL, "sam_decoder: g must be a multiple of 8 in [8, 64]");
    if (!pack || !features || !points || !labels || !low_res || !iou)
        return fail(SAMNERF_EINVAL, "sam_decoder: null pack / features / points / labels / low_res / iou");
    if (!ws) return fail(SAMNERF_EINVAL, "sam_decoder: null workspace");
    if (const char* why = validate_points(labels, P)) return fail(SAMNERF_EINVAL, "sam_decoder: %s", why);
    if ((h == 0) != (w == 0) || h > 1024 || w > 1024)
        return fail(SAMNERF_EINVAL, "sam_decoder: h and w are both 0 (features [g*g][256]) or both in [1, 1024]");
    if (!aligned16(pack) || !aligned16(ws) || !aligned16(iou))
        return fail(SAMNERF_EINVAL, "sam_decoder: pack, iou and workspace must be 16-byte aligned");
    const Layout l = make_layout(g);
    if (pack_bytes < l.pack_count * sizeof(float))
        return fail(SAMNERF_EINVAL, "sam_decoder: pack of %zu bytes, %zu expected for g = %u", pack_bytes,
                    l.pack_count * sizeof(float), g);
    const Work W = carve(ws, g);
    if (ws_bytes < W.bytes)
        return fail(SAMNERF_EWORKSPACE, "sam_decoder: workspace of %zu bytes, %zu needed", ws_bytes, W.bytes);
    const float* pk = static_cast<const float*>(pack);
    const uint32_t N = g * g, T = P + 6u;
    Launcher run{reinterpret_cast<hipStream_t>(stream), pk};
    hipStream_t s = run.s;

    SrcArgs sa{features, pk + l.nomask, W.kim, g, h, w, 0, 0};
    if (h) {                                            // sam_bridge.prepare_sam_features' sizes, in double
        const double r = w > h ? (double)g / w : (double)g / h;
        sa.vh = (uint32_t)(int)(h * r);
        sa.vw = (uint32_t)(int)(w * r);
        if (sa.vh < 1 || sa.vw < 1 || sa.vh > g || sa.vw > g)
            return fail(SAMNERF_EINVAL, "sam_decoder: a %u x %u map resizes to %u x %u", h, w, sa.vh, sa.vw);
    }
    k_sd_src<<<div_up(N, 4), kT, 0, s>>>(sa);
    run.done("sam_decoder src");

    TokArgs ta{};
    ta.pack = pk;
    ta.G = l.G; ta.pt0 = l.pt[0]; ta.pt1 = l.pt[1]; ta.nap = l.nap; ta.iou = l.iou; ta.mtok = l.mtok;
    ta.tok = W.tok; ta.q = W.q; ta.P = P; ta.S = 16u * g;
    for (uint32_t i = 0; i < P; ++i) {
        ta.x[i] = points[2 * i];
        ta.y[i] = points[2 * i + 1];
        ta.label[i] = labels[i];
    }
    k_sd_tokens<<<T, kT, 0, s>>>(ta);
    run.done("sam_decoder tokens");

    const float* ipe = pk + l.ipe;
    const size_t tokens = (size_t)kMaxTok * kC;
    // token -> image attention of `a`, the residual and the norm: q <- norm(q + attn)
    auto token_to_image = [&](const Attn& a, size_t nw, size_t nb) {
        const LinJob j[3] = {run.job(W.q, W.tok, a.q, nullptr, W.tq, T), run.job(W.kim, ipe, a.k, nullptr, W.ik, N),
                             run.job(W.kim, nullptr, a.v, nullptr, W.iv, N)};
        run.lin(j, 3);
        if (!run.rc) {
            k_sd_attn_tok<16, 2, 4><<<dim3(div_up(T, 2), kHeads, kKeySlices), kT, 0, s>>>(W.tq, W.ik, W.iv, W.ta, W.ap,
                                                                                          T, N);
            run.done("sam_decoder token->image attention");
        }
        if (!run.rc) {
            k_sd_attn_merge<<<T, 128, 0, s>>>(W.ap, W.ta, T, kKeySlices);
            run.done("sam_decoder attention merge");
        }
        const LinJob o = run.job(W.ta, nullptr, a.o, W.q, W.x1, T);
        run.lin(&o, 1);
        run.ln(W.x1, 1, 0, nw, nb, W.q, T);
    };
    for (int li = 0; li < 2; ++li) {
        const Layer& L = l.L[li];
        const float* qpe = li ? W.tok : nullptr;
        {
            const LinJob j[3] = {run.job(W.q, qpe, L.self.q, nullptr, W.tq, T),
                                 run.job(W.q, qpe, L.self.k, nullptr, W.tk, T),
                                 run.job(W.q, nullptr, L.self.v, nullptr, W.tv, T)};
            run.lin(j, 3);
            if (!run.rc) {
                k_sd_attn_tok<32, 1, 1><<<dim3(T, kHeads), kT, 0, s>>>(W.tq, W.tk, W.tv, W.ta, nullptr, T, T);
                run.done("sam_decoder self attention");
            }
            const LinJob o = run.job(W.ta, nullptr, L.self.o, li ? W.q : nullptr, W.x1, T);
            run.lin(&o, 1);
            run.ln(W.x1, 1, 0, L.nw[0], L.nb[0], W.q, T);
        }
        token_to_image(L.t2i, L.nw[1], L.nb[1]);
        {
            const LinJob up = run.job(W.q, nullptr, L.lin1, nullptr, W.hid, T, true);
            run.lin(&up, 1);
            LinJob j[kSplit];
            for (uint32_t k = 0; k < kSplit; ++k) {
                const uint32_t k0 = k * (kHid / kSplit);
                j[k] = {W.hid + k0, nullptr, pk + L.lin2.w + (size_t)k0 * kC, k ? nullptr : pk + L.lin2.b,
                        k ? nullptr : W.q, W.part + k * tokens, T, kHid / kSplit, kC, kHid, 0u};
            }
            run.lin(j, kSplit);
            run.ln(W.part, kSplit, tokens, L.nw[2], L.nb[2], W.q, T);
        }
        {
            const LinJob j[3] = {run.job(W.kim, ipe, L.i2t.q, nullptr, W.iq, N),
                                 run.job(W.q, W.tok, L.i2t.k, nullptr, W.tk, T),
                                 run.job(W.q, nullptr, L.i2t.v, nullptr, W.tv, T)};
            run.lin(j, 3);
            if (!run.rc) {
                k_sd_attn_img<<<dim3(div_up(N, kT), kHeads), kT, 0, s>>>(W.iq, W.tk, W.tv, W.ia, N, T);
                run.done("sam_decoder image->token attention");
            }
            const LinJob o = run.job(W.ia, nullptr, L.i2t.o, W.kim, W.kx, N);
            run.lin(&o, 1);
            run.ln(W.kx, 1, 0, L.nw[3], L.nb[3], W.kim, N);
        }
    }
    token_to_image(l.fin, l.nfw, l.nfb);
    // the four hypernetwork MLPs and the IoU head, a layer a launch
    {
        LinJob j[5];
        for (uint32_t i = 0; i < 5; ++i)
            j[i] = run.job(W.q + (size_t)(i < 4 ? 1 + i : 0) * kC, nullptr, i < 4 ? l.hyp[i][0] : l.iouh[0], nullptr,
                           W.h1 + i * kC, 1, true);
        run.lin(j, 5);
        for (uint32_t i = 0; i < 5; ++i)
            j[i] = run.job(W.h1 + i * kC, nullptr, i < 4 ? l.hyp[i][1] : l.iouh[1], nullptr, W.h2 + i * kC, 1, true);
        run.lin(j, 5);
        for (uint32_t i = 0; i < 5; ++i)
            j[i] = run.job(W.h2 + i * kC, nullptr, i < 4 ? l.hyp[i][2] : l.iouh[2], nullptr,
                           i < 4 ? W.hyp + i * 32 : iou, 1);
        run.lin(j, 5);
    }
    {
        const LinJob up = run.job(W.kim, nullptr, l.up0, nullptr, W.u1, N);
        run.lin(&up, 1);
        if (!run.rc) {
            k_sd_up<<<div_up(N, 16), kT, 0, s>>>(W.u1, pk + l.uplnw, pk + l.uplnb, pk + l.up1w, pk + l.up1b, W.hyp,
                                                 low_res, g);
            run.done("sam_decoder upscale");
        }
    }
    if (!run.rc) g_launches.store(run.count);
    return run.rc;
}

extern "C" int samnerf_sam_masks(const float* low_res, uint32_t M, uint32_t g, uint32_t in_h, uint32_t in_w, uint32_t H,
                                 uint32_t W, float* logits, uint8_t* mask, samnerf_stream_t stream) {
    if (!grid_ok(g)) return fail(SAMNERF_EINVAL, "sam_masks: g must be a multiple of 8 in [8, 64]");
    if (!low_res || (!logits && !mask)) return fail(SAMNERF_EINVAL, "sam_masks: null low_res, or no output");
    const uint32_t S = 16u * g;
    if (M < 1 || M > 4) return fail(SAMNERF_EINVAL, "sam_masks: M must lie in [1, 4]");
    if (in_h < 1 || in_w < 1 || in_h > S || in_w > S)
        return fail(SAMNERF_EINVAL, "sam_masks: input_size must lie in [1, %u]", S);
    if (H < 1 || W < 1 || H > 8192 || W > 8192) return fail(SAMNERF_EINVAL, "sam_masks: H and W must lie in [1, 8192]");
    MaskArgs a{low_res, logits, mask, 4u * g, S, in_h, in_w, H, W};
    k_sd_masks<<<dim3(div_up((uint64_t)H * W, kT), M), kT, 0, reinterpret_cast<hipStream_t>(stream)>>>(a);
    return check_launch("sam_masks");
}
