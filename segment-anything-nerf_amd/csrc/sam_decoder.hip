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
//
// samnerf_sam_decoder_batch is the same 44 launches for B prompt sets: the
// kernels' batched forms (template parameter BC / BATCH; the single call keeps
// its own instantiations) run the image side on B N rows and the token side on
// B T rows, what does not depend on the prompt once a call, every sum in the
// single call's order, so a set's bits are those of its single call.  The mask
// generator's steps follow: k_sd_masks_select (the postprocess as a gather),
// k_sd_mask_stats (a candidate's areas, box and filters, the logits in
// registers), k_sd_nms_rank / k_sd_nms_greedy (box NMS on the device).
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

// The batched call's tokens: rows [B][T], the points and labels read from the
// device.  A whole-number coordinate gives k_sd_tokens' bits ((float)x is it);
// a label is read as label != 0.
__global__ void __launch_bounds__(kT) k_sd_tokens_batch(const float* __restrict__ pack, size_t G, size_t pt0,
                                                        size_t pt1, size_t nap, size_t iou, size_t mtok,
                                                        const float* __restrict__ points,
                                                        const int32_t* __restrict__ labels, float* __restrict__ tok,
                                                        float* __restrict__ q, uint32_t P, uint32_t S) {
    const uint32_t T = P + 6u, b = blockIdx.x / T, row = blockIdx.x - b * T, c = threadIdx.x;
    float v;
    if (row == 0u) {
        v = pack[iou + c];
    } else if (row < 5u) {
        v = pack[mtok + (size_t)(row - 1u) * kC + c];
    } else if (row < 5u + P) {
        const size_t p = (size_t)b * P + (row - 5u);
        const float Sf = (float)S;
        v = pos_code(pack + G, (points[2u * p] + 0.5f) / Sf, (points[2u * p + 1u] + 0.5f) / Sf, c) +
            pack[(labels[p] != 0 ? pt1 : pt0) + c];
    } else {
        v = pack[nap + c];
    }
    tok[(size_t)blockIdx.x * kC + c] = v;
    q[(size_t)blockIdx.x * kC + c] = v;
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
    uint32_t a2_mod, r_mod;   // the batched call's broadcasts: row r reads A2 / R at r % mod (0: at r)
};
struct LinJobs {
    LinJob j[kMaxJobs];
};

// TM rows x 64 columns a workgroup, K in steps of 32 through LDS with the next
// step's loads in flight over the FMAs; a thread holds TM / 16 rows x 4 columns.
// Every output is one chain of FMAs over k = 0 .. K - 1.  BC: the batched call's
// form, in which A2 and R may be one set's rows read by every set (a2_mod,
// r_mod); the sums are the same chains.
template <int TM, bool BC = false>
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
                        uint32_t r2 = r;
                        if constexpr (BC) r2 = j.a2_mod ? r % j.a2_mod : r;
                        const float4 u = *reinterpret_cast<const float4*>(j.A2 + (size_t)r2 * j.lda + k);
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
            uint32_t rr = row;
            if constexpr (BC) rr = j.r_mod ? row % j.r_mod : row;
            const float4 u = *reinterpret_cast<const float4*>(j.R + (size_t)rr * j.O + col);
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
//
// BATCH: blockIdx.x also counts the prompt sets, div_up(T, QB) workgroups
// each; set b's queries are rows b T .. of Q, out and (per slice) part, its
// keys start at b * kv_stride floats of K and V (0: every set reads the same).
template <int DH, int QB, int U, bool BATCH = false>
__global__ void __launch_bounds__(kT) k_sd_attn_tok(const float* __restrict__ Q, const float* __restrict__ K,
                                                    const float* __restrict__ V, float* __restrict__ out,
                                                    float* __restrict__ part, uint32_t T, uint32_t Nk,
                                                    uint32_t sets = 1, size_t kv_stride = 0) {
    constexpr uint32_t inner = kHeads * DH;
    __shared__ float sh[4][QB][DH + 2];
    uint32_t bx = blockIdx.x, Ttot = T;
    if constexpr (BATCH) {
        const uint32_t per_set = (T + QB - 1) / QB, b = bx / per_set;
        bx -= b * per_set;
        Q += (size_t)b * T * inner;
        K += (size_t)b * kv_stride;
        V += (size_t)b * kv_stride;
        out += (size_t)b * T * inner;
        part += (size_t)b * T * kHeads * (DH + 2);
        Ttot = sets * T;
    }
    const uint32_t h = blockIdx.y, q0 = bx * QB, t = threadIdx.x;
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
            float* p = part + (((size_t)blockIdx.z * Ttot + q0 + qi) * kHeads + h) * (DH + 2);
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
// BATCH: blockIdx.z is the prompt set; its keys are rows b T .., its outputs
// rows b N .., its queries start at b * q_stride floats (0: the same for all).
template <bool BATCH = false>
__global__ void __launch_bounds__(kT) k_sd_attn_img(const float* __restrict__ Q, const float* __restrict__ K,
                                                    const float* __restrict__ V, float* __restrict__ out, uint32_t N,
                                                    uint32_t T, size_t q_stride = 0) {
    constexpr uint32_t DH = 16, inner = 128;
    __shared__ float4 Ks[kMaxTok * 4], Vs[kMaxTok * 4];
    if constexpr (BATCH) {
        const uint32_t b = blockIdx.z;
        Q += (size_t)b * q_stride;
        K += (size_t)b * T * inner;
        V += (size_t)b * T * inner;
        out += (size_t)b * N * inner;
    }
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
// BATCH: blockIdx.y is the prompt set: u1 [B][N][4][64], hyp [4][B][32] (the
// batched linears write a mask's products of every set together), low
// [B][4][4g][4g].
template <bool BATCH = false>
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
    if constexpr (BATCH) {
        const uint32_t b = blockIdx.y, B = gridDim.y;
        u1 += (size_t)b * g * g * kC;
        low += (size_t)b * 64u * g * g;
        if (t < 32u) H4[t] = reinterpret_cast<const float4*>(hyp)[((t >> 3) * B + b) * 8u + (t & 7u)];
    } else {
        if (t < 32u) H4[t] = reinterpret_cast<const float4*>(hyp)[t];
    }
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
// p is the mask's [L][L] image.  The one expression of k_sd_masks,
// k_sd_masks_select and k_sd_mask_stats (the build contracts nothing, so the
// three give the same bits).
__device__ __forceinline__ float mask_logit(const float* __restrict__ p, uint32_t L, uint32_t S, uint32_t ih,
                                            uint32_t iw, uint32_t H, uint32_t W, uint32_t Y, uint32_t X) {
    uint32_t sy[2], sx[2];
    float wy[2], wx[2];
    bilinear_tap(ih, H, Y, sy[0], sy[1], wy[1]);
    bilinear_tap(iw, W, X, sx[0], sx[1], wx[1]);
    wy[0] = 1.0f - wy[1];
    wx[0] = 1.0f - wx[1];
    uint32_t y0[2], y1[2], x0[2], x1[2];
    float ly[2], lx[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        bilinear_tap(L, S, sy[k], y0[k], y1[k], ly[k]);
        bilinear_tap(L, S, sx[k], x0[k], x1[k], lx[k]);
    }
    float v[2][2];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const float mx = 1.0f - lx[c], my = 1.0f - ly[r];
            v[r][c] = my * (mx * p[y0[r] * L + x0[c]] + lx[c] * p[y0[r] * L + x1[c]]) +
                      ly[r] * (mx * p[y1[r] * L + x0[c]] + lx[c] * p[y1[r] * L + x1[c]]);
        }
    return wy[0] * (wx[0] * v[0][0] + wx[1] * v[0][1]) + wy[1] * (wx[0] * v[1][0] + wx[1] * v[1][1]);
}

__global__ void __launch_bounds__(kT) k_sd_masks(MaskArgs a) {
    const uint32_t i = blockIdx.x * kT + threadIdx.x;
    if (i >= a.H * a.W) return;
    const uint32_t Y = i / a.W, X = i - Y * a.W;
    const float out = mask_logit(a.low + (size_t)blockIdx.y * a.L * a.L, a.L, a.S, a.ih, a.iw, a.H, a.W, Y, X);
    const size_t at = (size_t)blockIdx.y * a.H * a.W + i;
    if (a.logits) a.logits[at] = out;
    if (a.mask) a.mask[at] = out > 0.0f ? 1 : 0;
}

// The gather form: output slot blockIdx.y is mask index[slot] (null: slot) of a
// table of n; slots at and past *count (null: all `cap` slots are live) are
// left as they are, and so is a slot whose index is outside the table.
struct SelectArgs {
    MaskArgs m;
    const int32_t* index;
    const int32_t* count;
    uint32_t n;
    float thr;            // mask = logit > thr
};

__global__ void __launch_bounds__(kT) k_sd_masks_select(SelectArgs a) {
    const uint32_t i = blockIdx.x * kT + threadIdx.x, slot = blockIdx.y;
    if (i >= a.m.H * a.m.W) return;
    if (a.count && (int32_t)slot >= *a.count) return;
    const uint32_t src = a.index ? (uint32_t)a.index[slot] : slot;
    if (src >= a.n) return;
    const uint32_t Y = i / a.m.W, X = i - Y * a.m.W;
    const float out = mask_logit(a.m.low + (size_t)src * a.m.L * a.m.L, a.m.L, a.m.S, a.m.ih, a.m.iw, a.m.H, a.m.W, Y, X);
    const size_t at = (size_t)slot * a.m.H * a.m.W + i;
    if (a.m.logits) a.m.logits[at] = out;
    if (a.m.mask) a.m.mask[at] = out > a.thr ? 1 : 0;
}

// ------------------------------------------------------ generator: stats --

// A candidate's record, SAMNERF_SAM_REC_WORDS 32-bit words (samnerf_hip.h).
enum { kRecInter, kRecUnion, kRecArea, kRecX0, kRecY0, kRecX1, kRecY1, kRecStab, kRecPass, kRecIou, kRecWords };
static_assert(kRecWords == SAMNERF_SAM_REC_WORDS, "record layout");

struct StatsArgs {
    MaskArgs m;
    const float* iou;
    int32_t* rec;
    float iou_thresh, thr, off, stab_thresh;
};

// A workgroup a candidate.  One failing the IoU test costs a zeroed record;
// the others walk the view's pixels, thread t pixels t, t + 256, ..., with
// the logit of k_sd_masks in registers only, and reduce three counts and a
// box: integers, so the order of the reduction does not show.
__global__ void __launch_bounds__(kT) k_sd_mask_stats(StatsArgs a) {
    __shared__ int32_t sh[4][7];
    const uint32_t c = blockIdx.x, t = threadIdx.x;
    int32_t* rec = a.rec + (size_t)c * kRecWords;
    const float iou = a.iou[c];
    if (!(iou > a.iou_thresh)) {                          // a NaN score fails
        if (t < (uint32_t)kRecWords) rec[t] = 0;
        return;
    }
    const float* p = a.m.low + (size_t)c * a.m.L * a.m.L;
    const float hi = a.thr + a.off, lo = a.thr - a.off;
    const uint32_t n = a.m.H * a.m.W;
    int32_t inter = 0, uni = 0, area = 0, x0 = INT32_MAX, y0 = INT32_MAX, x1 = -1, y1 = -1;
    for (uint32_t i = t; i < n; i += kT) {
        const uint32_t Y = i / a.m.W, X = i - Y * a.m.W;
        const float v = mask_logit(p, a.m.L, a.m.S, a.m.ih, a.m.iw, a.m.H, a.m.W, Y, X);
        inter += v > hi ? 1 : 0;
        uni += v > lo ? 1 : 0;
        if (v > a.thr) {
            ++area;
            x0 = min(x0, (int32_t)X);
            y0 = min(y0, (int32_t)Y);
            x1 = max(x1, (int32_t)X);
            y1 = max(y1, (int32_t)Y);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        inter += __shfl_xor(inter, o, 64);
        uni += __shfl_xor(uni, o, 64);
        area += __shfl_xor(area, o, 64);
        x0 = min(x0, __shfl_xor(x0, o, 64));
        y0 = min(y0, __shfl_xor(y0, o, 64));
        x1 = max(x1, __shfl_xor(x1, o, 64));
        y1 = max(y1, __shfl_xor(y1, o, 64));
    }
    if ((t & 63u) == 0u) {
        int32_t* w = sh[t >> 6];
        w[0] = inter; w[1] = uni; w[2] = area; w[3] = x0; w[4] = y0; w[5] = x1; w[6] = y1;
    }
    __syncthreads();
    if (t != 0u) return;
    for (int w = 1; w < 4; ++w) {
        inter += sh[w][0];
        uni += sh[w][1];
        area += sh[w][2];
        x0 = min(x0, sh[w][3]);
        y0 = min(y0, sh[w][4]);
        x1 = max(x1, sh[w][5]);
        y1 = max(y1, sh[w][6]);
    }
    if (area == 0) x0 = y0 = x1 = y1 = 0;
    const float stab = (float)inter / (float)uni;        // 0 / 0 is NaN and fails
    rec[kRecInter] = inter;
    rec[kRecUnion] = uni;
    rec[kRecArea] = area;
    rec[kRecX0] = x0;
    rec[kRecY0] = y0;
    rec[kRecX1] = x1;
    rec[kRecY1] = y1;
    rec[kRecStab] = __float_as_int(stab);
    rec[kRecPass] = stab >= a.stab_thresh ? 1 : 0;
    rec[kRecIou] = __float_as_int(iou);
}

// -------------------------------------------------------- generator: NMS --

// The place of every passing candidate in the order of descending score,
// ties to the lower index: the number of passing candidates before it,
// counted against tiles of 256 through LDS.  keep[place] = candidate.
__global__ void __launch_bounds__(kT) k_sd_nms_rank(const int32_t* __restrict__ rec, uint32_t n,
                                                    int32_t* __restrict__ keep) {
    __shared__ float s_iou[kT];
    __shared__ int32_t s_pass[kT];
    const uint32_t t = threadIdx.x, i = blockIdx.x * kT + t;
    const bool live = i < n && rec[(size_t)i * kRecWords + kRecPass] != 0;
    const float mine = live ? __int_as_float(rec[(size_t)i * kRecWords + kRecIou]) : 0.0f;
    uint32_t before = 0;
    for (uint32_t j0 = 0; j0 < n; j0 += kT) {
        __syncthreads();
        const uint32_t j = j0 + t;
        s_pass[t] = j < n ? rec[(size_t)j * kRecWords + kRecPass] : 0;
        s_iou[t] = j < n ? __int_as_float(rec[(size_t)j * kRecWords + kRecIou]) : 0.0f;
        __syncthreads();
        if (live) {
            const uint32_t m = n - j0 < kT ? n - j0 : kT;
            for (uint32_t k = 0; k < m; ++k) {
                const float o = s_iou[k];
                before += s_pass[k] && (o > mine || (o == mine && j0 + k < i)) ? 1u : 0u;
            }
        }
    }
    if (live) keep[before] = (int32_t)i;
}

// torchvision's box IoU of two records' boxes, as floats.
__device__ __forceinline__ float box_iou(const int32_t* __restrict__ a, const int32_t* __restrict__ b) {
    const float ax0 = (float)a[kRecX0], ay0 = (float)a[kRecY0], ax1 = (float)a[kRecX1], ay1 = (float)a[kRecY1];
    const float bx0 = (float)b[kRecX0], by0 = (float)b[kRecY0], bx1 = (float)b[kRecX1], by1 = (float)b[kRecY1];
    const float w = fmaxf(0.0f, fminf(ax1, bx1) - fmaxf(ax0, bx0));
    const float h = fmaxf(0.0f, fminf(ay1, by1) - fmaxf(ay0, by0));
    const float inter = w * h, aa = (ax1 - ax0) * (ay1 - ay0), ab = (bx1 - bx0) * (by1 - by0);
    return inter / (aa + ab - inter);
}

constexpr uint32_t kNmsMax = 3u * 64u * 64u;

// The greedy pass, one workgroup: keep[0 .. m) holds the passing candidates
// in order; candidate i of them is kept unless a kept one before it has
// suppressed it, and a kept one marks every later one it overlaps by more
// than the threshold (a NaN IoU marks nothing).  The kept indices are packed
// to the front of keep in that order, the rest of its n entries set to -1.
__global__ void __launch_bounds__(kT) k_sd_nms_greedy(const int32_t* __restrict__ rec, uint32_t n, float thresh,
                                                      int32_t* keep, int32_t* __restrict__ count) {
    __shared__ uint8_t gone[kNmsMax];
    __shared__ int32_t s_m[4];
    const uint32_t t = threadIdx.x;
    int32_t mine = 0;
    for (uint32_t i = t; i < n; i += kT) {
        mine += rec[(size_t)i * kRecWords + kRecPass] != 0 ? 1 : 0;
        gone[i] = 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o, 64);
    if ((t & 63u) == 0u) s_m[t >> 6] = mine;
    __syncthreads();
    const uint32_t m = (uint32_t)(s_m[0] + s_m[1] + s_m[2] + s_m[3]);
    // a NaN score has no place in the order and may leave an entry unwritten: such an entry is nobody
    for (uint32_t i = t; i < m; i += kT)
        if ((uint32_t)keep[i] >= n) gone[i] = 1;
    __syncthreads();
    uint32_t kept = 0;
    for (uint32_t i = 0; i < m; ++i) {
        if (gone[i]) continue;                            // settled by the barrier of the sweep that set it
        const int32_t ci = keep[i];
        const int32_t* bi = rec + (size_t)ci * kRecWords;
        for (uint32_t j = i + 1u + t; j < m; j += kT)
            if (!gone[j] && box_iou(bi, rec + (size_t)keep[j] * kRecWords) > thresh) gone[j] = 1;
        __syncthreads();                                  // the marks, and the reads of keep[j > i], are done
        if (t == 0u) keep[kept] = ci;                     // kept <= i: no later sweep reads this entry
        ++kept;
    }
    __syncthreads();
    for (uint32_t i = kept + t; i < n; i += kT) keep[i] = -1;
    if (t == 0u) *count = (int32_t)kept;
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
    // the batched call's: the same chains, A2 / R possibly one set's rows for all (a2_mod, r_mod)
    void lin_b(const LinJob* jobs, uint32_t n) {
        if (rc) return;
        LinJobs J{};
        uint32_t maxM = 0, maxO = 0;
        for (uint32_t i = 0; i < n; ++i) {
            J.j[i] = jobs[i];
            maxM = jobs[i].M > maxM ? jobs[i].M : maxM;
            maxO = jobs[i].O > maxO ? jobs[i].O : maxO;
        }
        if (maxM > kMaxTok)
            k_sd_lin<32, true><<<dim3(div_up(maxO, 64), div_up(maxM, 32), n), kT, 0, s>>>(J);
        else
            k_sd_lin<16, true><<<dim3(div_up(maxO, 64), div_up(maxM, 16), n), kT, 0, s>>>(J);
        done("sam_decoder_batch lin");
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
                k_sd_attn_img<false><<<dim3(div_up(N, kT), kHeads), kT, 0, s>>>(W.iq, W.tk, W.tv, W.ia, N, T);
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
            k_sd_up<false><<<div_up(N, 16), kT, 0, s>>>(W.u1, pk + l.uplnw, pk + l.uplnb, pk + l.up1w, pk + l.up1b, W.hyp,
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

// ------------------------------------------------------------- the batch --

namespace {

constexpr uint32_t kMaxSets = 256;

// The batched call's workspace: token-side rows [B T], image-side rows [B N];
// what does not depend on the prompt (kim0 and layer 0's ik0, iv0, iq0) once.
struct WorkB {
    float *tok, *q, *x1, *tq, *tk, *tv, *ta, *ap, *hid, *part, *kim0, *ik0, *iv0, *iq0, *kim, *kx, *ik, *iv, *iq, *ia,
        *h1, *h2, *hyp;
    size_t bytes;
};

WorkB carve_batch(void* ws, uint32_t g, uint32_t B) {
    WorkB w{};
    Carver c(ws);
    const size_t N = (size_t)g * g, BN = (size_t)B * N, tokens = (size_t)B * kMaxTok * kC;
    w.tok = c.take(tokens);
    w.q = c.take(tokens);
    w.x1 = c.take(tokens);
    w.tq = c.take(tokens);
    w.tk = c.take(tokens);
    w.tv = c.take(tokens);
    w.ta = c.take(tokens);
    w.ap = c.take((size_t)kKeySlices * B * kMaxTok * kHeads * 18);
    w.hid = c.take((size_t)B * kMaxTok * kHid);
    w.part = c.take(kSplit * tokens);
    w.kim0 = c.take(N * kC);
    w.ik0 = c.take(N * 128);
    w.iv0 = c.take(N * 128);
    w.iq0 = c.take(N * 128);
    w.kim = c.take(BN * kC);
    w.kx = c.take(BN * kC);                    // and u1, once the last norm has read it
    w.ik = c.take(BN * 128);
    w.iv = c.take(BN * 128);
    w.iq = c.take(BN * 128);
    w.ia = c.take(BN * 128);
    w.h1 = c.take((size_t)5 * B * kC);
    w.h2 = c.take((size_t)5 * B * kC);
    w.hyp = c.take((size_t)4 * B * 32);
    w.bytes = c.bytes();
    return w;
}

bool sets_ok(uint32_t B) { return B >= 1 && B <= kMaxSets; }

}  // namespace

extern "C" size_t samnerf_sam_decoder_batch_workspace_size(uint32_t g, uint32_t B) {
    return grid_ok(g) && sets_ok(B) ? carve_batch(nullptr, g, B).bytes : 0;
}

extern "C" int samnerf_sam_decoder_batch(const void* pack, size_t pack_bytes, uint32_t g, const float* features,
                                         uint32_t h, uint32_t w, const float* points, const int32_t* labels,
                                         uint32_t B, uint32_t P, float* low_res, float* iou, void* ws,
                                         size_t ws_bytes, samnerf_stream_t stream) {
    if (!grid_ok(g)) return fail(SAMNERF_EINVAL, "sam_decoder_batch: g must be a multiple of 8 in [8, 64]");
    if (!sets_ok(B)) return fail(SAMNERF_EINVAL, "sam_decoder_batch: B must lie in [1, 256]");
    if (P < 1 || P > kMaxP) return fail(SAMNERF_EINVAL, "sam_decoder_batch: P must lie in [1, 58]");
    if (!pack || !features || !points || !labels || !low_res || !iou)
        return fail(SAMNERF_EINVAL, "sam_decoder_batch: null pack / features / points / labels / low_res / iou");
    if (!ws) return fail(SAMNERF_EINVAL, "sam_decoder_batch: null workspace");
    if ((h == 0) != (w == 0) || h > 1024 || w > 1024)
        return fail(SAMNERF_EINVAL,
                    "sam_decoder_batch: h and w are both 0 (features [g*g][256]) or both in [1, 1024]");
    if (!aligned16(pack) || !aligned16(ws) || !aligned16(iou))
        return fail(SAMNERF_EINVAL, "sam_decoder_batch: pack, iou and workspace must be 16-byte aligned");
    const Layout l = make_layout(g);
    if (pack_bytes < l.pack_count * sizeof(float))
        return fail(SAMNERF_EINVAL, "sam_decoder_batch: pack of %zu bytes, %zu expected for g = %u", pack_bytes,
                    l.pack_count * sizeof(float), g);
    const WorkB W = carve_batch(ws, g, B);
    if (ws_bytes < W.bytes)
        return fail(SAMNERF_EWORKSPACE, "sam_decoder_batch: workspace of %zu bytes, %zu needed", ws_bytes, W.bytes);
    const float* pk = static_cast<const float*>(pack);
    const uint32_t N = g * g, T = P + 6u, BT = B * T, BN = B * N;
    Launcher run{reinterpret_cast<hipStream_t>(stream), pk};
    hipStream_t s = run.s;

    SrcArgs sa{features, pk + l.nomask, W.kim0, g, h, w, 0, 0};
    if (h) {
        const double r = w > h ? (double)g / w : (double)g / h;
        sa.vh = (uint32_t)(int)(h * r);
        sa.vw = (uint32_t)(int)(w * r);
        if (sa.vh < 1 || sa.vw < 1 || sa.vh > g || sa.vw > g)
            return fail(SAMNERF_EINVAL, "sam_decoder_batch: a %u x %u map resizes to %u x %u", h, w, sa.vh, sa.vw);
    }
    k_sd_src<<<div_up(N, 4), kT, 0, s>>>(sa);
    run.done("sam_decoder_batch src");
    k_sd_tokens_batch<<<BT, kT, 0, s>>>(pk, l.G, l.pt[0], l.pt[1], l.nap, l.iou, l.mtok, points, labels, W.tok, W.q, P,
                                        16u * g);
    run.done("sam_decoder_batch tokens");

    const float* ipe = pk + l.ipe;
    const size_t tokens = (size_t)BT * kC;
    // a job whose A2 (image_pe) or R is one set's N rows, read by every set
    auto wide = [&](LinJob j, uint32_t a2_mod, uint32_t r_mod) {
        j.a2_mod = a2_mod;
        j.r_mod = r_mod;
        return j;
    };
    // token -> image attention of `a`; first: the image tokens are still the call's, one k / v for every set
    auto token_to_image = [&](const Attn& a, size_t nw, size_t nb, bool first) {
        const LinJob j[3] = {
            run.job(W.q, W.tok, a.q, nullptr, W.tq, BT),
            first ? run.job(W.kim0, ipe, a.k, nullptr, W.ik0, N)
                  : wide(run.job(W.kim, ipe, a.k, nullptr, W.ik, BN), N, 0),
            first ? run.job(W.kim0, nullptr, a.v, nullptr, W.iv0, N) : run.job(W.kim, nullptr, a.v, nullptr, W.iv, BN)};
        run.lin_b(j, 3);
        if (!run.rc) {
            k_sd_attn_tok<16, 2, 4, true><<<dim3(B * div_up(T, 2), kHeads, kKeySlices), kT, 0, s>>>(
                W.tq, first ? W.ik0 : W.ik, first ? W.iv0 : W.iv, W.ta, W.ap, T, N, B, first ? 0 : (size_t)N * 128);
            run.done("sam_decoder_batch token->image attention");
        }
        if (!run.rc) {
            k_sd_attn_merge<<<BT, 128, 0, s>>>(W.ap, W.ta, BT, kKeySlices);
            run.done("sam_decoder_batch attention merge");
        }
        const LinJob o = run.job(W.ta, nullptr, a.o, W.q, W.x1, BT);
        run.lin_b(&o, 1);
        run.ln(W.x1, 1, 0, nw, nb, W.q, BT);
    };
    for (int li = 0; li < 2; ++li) {
        const Layer& L = l.L[li];
        const float* qpe = li ? W.tok : nullptr;
        {
            const LinJob j[3] = {run.job(W.q, qpe, L.self.q, nullptr, W.tq, BT),
                                 run.job(W.q, qpe, L.self.k, nullptr, W.tk, BT),
                                 run.job(W.q, nullptr, L.self.v, nullptr, W.tv, BT)};
            run.lin_b(j, 3);
            if (!run.rc) {
                k_sd_attn_tok<32, 1, 1, true><<<dim3(BT, kHeads), kT, 0, s>>>(W.tq, W.tk, W.tv, W.ta, nullptr, T, T, B,
                                                                              (size_t)T * kC);
                run.done("sam_decoder_batch self attention");
            }
            const LinJob o = run.job(W.ta, nullptr, L.self.o, li ? W.q : nullptr, W.x1, BT);
            run.lin_b(&o, 1);
            run.ln(W.x1, 1, 0, L.nw[0], L.nb[0], W.q, BT);
        }
        token_to_image(L.t2i, L.nw[1], L.nb[1], li == 0);
        {
            const LinJob up = run.job(W.q, nullptr, L.lin1, nullptr, W.hid, BT, true);
            run.lin_b(&up, 1);
            LinJob j[kSplit];
            for (uint32_t k = 0; k < kSplit; ++k) {
                const uint32_t k0 = k * (kHid / kSplit);
                j[k] = {W.hid + k0, nullptr, pk + L.lin2.w + (size_t)k0 * kC, k ? nullptr : pk + L.lin2.b,
                        k ? nullptr : W.q, W.part + k * tokens, BT, kHid / kSplit, kC, kHid, 0u};
            }
            run.lin_b(j, kSplit);
            run.ln(W.part, kSplit, tokens, L.nw[2], L.nb[2], W.q, BT);
        }
        {
            const bool first = li == 0;
            const LinJob j[3] = {first ? run.job(W.kim0, ipe, L.i2t.q, nullptr, W.iq0, N)
                                       : wide(run.job(W.kim, ipe, L.i2t.q, nullptr, W.iq, BN), N, 0),
                                 run.job(W.q, W.tok, L.i2t.k, nullptr, W.tk, BT),
                                 run.job(W.q, nullptr, L.i2t.v, nullptr, W.tv, BT)};
            run.lin_b(j, 3);
            if (!run.rc) {
                k_sd_attn_img<true><<<dim3(div_up(N, kT), kHeads, B), kT, 0, s>>>(
                    first ? W.iq0 : W.iq, W.tk, W.tv, W.ia, N, T, first ? 0 : (size_t)N * 128);
                run.done("sam_decoder_batch image->token attention");
            }
            const LinJob o = first ? wide(run.job(W.ia, nullptr, L.i2t.o, W.kim0, W.kx, BN), 0, N)
                                   : run.job(W.ia, nullptr, L.i2t.o, W.kim, W.kx, BN);
            run.lin_b(&o, 1);
            run.ln(W.kx, 1, 0, L.nw[3], L.nb[3], W.kim, BN);
        }
    }
    token_to_image(l.fin, l.nfw, l.nfb, false);
    // the hypernetwork MLPs and the IoU head: job i takes token row (i < 4 ? 1 + i : 0) of every set
    {
        LinJob j[5];
        for (uint32_t i = 0; i < 5; ++i) {
            j[i] = run.job(W.q + (size_t)(i < 4 ? 1 + i : 0) * kC, nullptr, i < 4 ? l.hyp[i][0] : l.iouh[0], nullptr,
                           W.h1 + (size_t)i * B * kC, B, true);
            j[i].lda = T * kC;
        }
        run.lin_b(j, 5);
        for (uint32_t i = 0; i < 5; ++i)
            j[i] = run.job(W.h1 + (size_t)i * B * kC, nullptr, i < 4 ? l.hyp[i][1] : l.iouh[1], nullptr,
                           W.h2 + (size_t)i * B * kC, B, true);
        run.lin_b(j, 5);
        for (uint32_t i = 0; i < 5; ++i)
            j[i] = run.job(W.h2 + (size_t)i * B * kC, nullptr, i < 4 ? l.hyp[i][2] : l.iouh[2], nullptr,
                           i < 4 ? W.hyp + (size_t)i * B * 32 : iou, B);
        run.lin_b(j, 5);
    }
    {
        float* u1 = W.kx;
        const LinJob up = run.job(W.kim, nullptr, l.up0, nullptr, u1, BN);
        run.lin_b(&up, 1);
        if (!run.rc) {
            k_sd_up<true><<<dim3(div_up(N, 16), B), kT, 0, s>>>(u1, pk + l.uplnw, pk + l.uplnb, pk + l.up1w,
                                                                pk + l.up1b, W.hyp, low_res, g);
            run.done("sam_decoder_batch upscale");
        }
    }
    if (!run.rc) g_launches.store(run.count);
    return run.rc;
}

// ---------------------------------------------------------- the generator --

namespace {

const char* view_bad(uint32_t g, uint32_t in_h, uint32_t in_w, uint32_t H, uint32_t W) {
    if (!grid_ok(g)) return "g must be a multiple of 8 in [8, 64]";
    if (in_h < 1 || in_w < 1 || in_h > 16u * g || in_w > 16u * g) return "input_size must lie in [1, 16 g]";
    if (H < 1 || W < 1 || H > 8192 || W > 8192) return "H and W must lie in [1, 8192]";
    return nullptr;
}

}  // namespace

extern "C" int samnerf_sam_masks_select(const float* low_res, uint32_t n, const int32_t* index, uint32_t count,
                                        const int32_t* count_dev, uint32_t g, uint32_t in_h, uint32_t in_w, uint32_t H,
                                        uint32_t W, float mask_threshold, float* logits, uint8_t* mask,
                                        samnerf_stream_t stream) {
    if (const char* why = view_bad(g, in_h, in_w, H, W)) return fail(SAMNERF_EINVAL, "sam_masks_select: %s", why);
    if (!low_res || (!logits && !mask)) return fail(SAMNERF_EINVAL, "sam_masks_select: null low_res, or no output");
    if (n < 1 || n > kNmsMax) return fail(SAMNERF_EINVAL, "sam_masks_select: n must lie in [1, %u]", kNmsMax);
    if (count > kNmsMax || (!index && count > n))
        return fail(SAMNERF_EINVAL, "sam_masks_select: a count of %u over a table of %u", count, n);
    if (count == 0) return SAMNERF_OK;
    SelectArgs a{{low_res, logits, mask, 4u * g, 16u * g, in_h, in_w, H, W}, index, count_dev, n, mask_threshold};
    k_sd_masks_select<<<dim3(div_up((uint64_t)H * W, kT), count), kT, 0, reinterpret_cast<hipStream_t>(stream)>>>(a);
    return check_launch("sam_masks_select");
}

extern "C" int samnerf_sam_mask_stats(const float* low_res, const float* iou, uint32_t n, uint32_t g, uint32_t in_h,
                                      uint32_t in_w, uint32_t H, uint32_t W, float pred_iou_thresh,
                                      float mask_threshold, float stability_score_offset,
                                      float stability_score_thresh, int32_t* records, samnerf_stream_t stream) {
    if (const char* why = view_bad(g, in_h, in_w, H, W)) return fail(SAMNERF_EINVAL, "sam_mask_stats: %s", why);
    if (n > kNmsMax) return fail(SAMNERF_EINVAL, "sam_mask_stats: n must not exceed %u", kNmsMax);
    if (n == 0) return SAMNERF_OK;
    if (!low_res || !iou || !records) return fail(SAMNERF_EINVAL, "sam_mask_stats: null low_res / iou / records");
    StatsArgs a{{low_res, nullptr, nullptr, 4u * g, 16u * g, in_h, in_w, H, W}, iou, records, pred_iou_thresh,
                mask_threshold, stability_score_offset, stability_score_thresh};
    k_sd_mask_stats<<<n, kT, 0, reinterpret_cast<hipStream_t>(stream)>>>(a);
    return check_launch("sam_mask_stats");
}

extern "C" int samnerf_sam_nms(const int32_t* records, uint32_t n, float box_nms_thresh, int32_t* keep,
                               int32_t* count, samnerf_stream_t stream) {
    if (n > kNmsMax) return fail(SAMNERF_EINVAL, "sam_nms: n must not exceed %u", kNmsMax);
    if (n == 0) return SAMNERF_OK;
    if (!records || !keep || !count) return fail(SAMNERF_EINVAL, "sam_nms: null records / keep / count");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    k_sd_nms_rank<<<div_up(n, kT), kT, 0, s>>>(records, n, keep);
    if (int rc = check_launch("sam_nms rank")) return rc;
    k_sd_nms_greedy<<<1, kT, 0, s>>>(records, n, box_nms_thresh, keep, count);
    return check_launch("sam_nms greedy");
}
