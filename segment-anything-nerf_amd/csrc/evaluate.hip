// evaluate.hip -- one evaluated view on the device: what Trainer.eval_step
// (nerf/utils.py:1122-1241) and the meters of evaluate_one_epoch (PSNRMeter,
// SSIMMeter, MeanIoUMeter, utils.py:329-512, :1945-2000) compute after the
// render.  The reference copies prediction and truth to the host, takes
// np.mean there, runs torchmetrics' SSIM as a handful of torch ops, loops over
// the classes in Python and synchronises on loss.item(); here the raw sums and
// counts go into one stats record in device memory (include/samnerf_hip.h) and
// the host reads the records once per epoch.
//
// Sums follow mask_loss.hip's rule: every floating sum is a fixed-order sum.
// A thread adds its own values in double in index order, the workgroup adds its
// threads in a fixed tree (block_reduce.h block_sum_ordered; min and max through
// its order-free forms), the partial goes to the workspace, and one thread of
// k_eval_finish adds the at most 1024 partials in index order.  No float
// atomics; the histograms and counts use integer atomics (LDS, then global),
// which commute.
//
//   k_eval_rgb     per pixel: the RGBA composite, (p - t)^2, min / max, the three
//                  uint8 buffers
//   k_eval_mask    per pixel: probabilities and argmax (instance_row.h's row, with
//                  its second tree for K > 32), NLL, the three histograms
//   k_eval_sam     64 x 64 (pixel, channel) tiles: (p - g)^2 with the [256, h*w]
//                  truth transposed through LDS, both read in place
//   k_eval_finish  the partials into the record (stage 0: all but SSIM)
//   k_eval_ssim    32 x 16 output tiles: the separable 11-tap window over LDS;
//                  c1, c2 from the record's min / max, so it runs after stage 0
//   k_eval_confusion  the histograms from ready-made id maps
//
// The SSIM tile: 32 x 16 outputs need 42 x 26 inputs of p and t (8.5 KiB) and
// the horizontal pass leaves 26 x 32 values of five moments (16.3 KiB): 24.8
// KiB a workgroup, six workgroups in a CU's 160 KiB.  A 512 x 512 view has
// 16 x 32 x 3 = 1536 tiles for 768 workgroups of two tiles; each thread
// evaluates two outputs per tile.
#include <cmath>
#include <cstring>

#include "block_reduce.h"
#include "instance_row.h"
#include "quantise.h"
#include "samnerf_common.h"

using namespace samnerf;

namespace {

constexpr uint32_t kT = 256;
constexpr uint32_t kWaves = kT / 64;
constexpr uint32_t kMaxParts = 1024;          // workgroups of every reducing kernel
constexpr uint32_t kMaxEvalK = SAMNERF_EVAL_MAX_K;   // two trees of instance_row.h's row
static_assert(kMaxEvalK == 2 * kTreeLanes, "k_eval_mask's row has two trees");
constexpr uint32_t kTaps = 11, kHalo = kTaps - 1;
constexpr uint32_t kTW = 32, kTH = 16, kIW = kTW + kHalo, kIH = kTH + kHalo;
constexpr uint32_t kFeat = 256, kFT = 64;     // SAM channels; the transposing tile's side

struct RgbPart { double sq; float pmin, pmax, tmin, tmax; };
// the workspace: [kMaxParts] of each
struct Workspace {
    RgbPart rgb[kMaxParts];
    double nll[kMaxParts], ssim[kMaxParts], feat[kMaxParts];
};

struct Params {
    uint32_t H, W, n, C, K, Kp, n_inst, n_classes, hw;
    uint32_t n_rgb, n_mask, n_ssim, n_feat;   // workgroups (= partials) of each part
    float bg, lo, hi;                         // the NLL's clamp
    float g[kTaps];
    const float* pred;
    const float* truth;
    const float* logits;
    const int64_t* labels;
    const float* pf;
    const float* gf;
    uint8_t* pred_u8;
    uint8_t* truth_u8;
    uint8_t* error_u8;
    float* truth_out;
    float* probs;
    int64_t* ids;
    samnerf_eval_stats* stats;
    uint32_t* hist;                           // [3][n_classes] behind the record
    Workspace* ws;
};

// min and max of the predictions and of the truth: slots 0 .. 3 of the order-free reductions
struct MinMax {
    __device__ __forceinline__ float operator()(uint32_t j, float a, float b) const {
        return (j & 1u) ? fmaxf(a, b) : fminf(a, b);
    }
};

// utils.py:1141-1145, channel ch of pixel g
__device__ __forceinline__ float truth_of(const float* g, uint32_t C, uint32_t ch, float bg) {
    if (C == 3) return g[ch];
    const float a = g[3];
    return g[ch] * a + bg * (1.0f - a);
}

__global__ void __launch_bounds__(kT) k_eval_rgb(Params P) {
    __shared__ double shd[kWaves];
    __shared__ float shf[4 * kWaves];
    double acc = 0.0;
    float pmn = INFINITY, pmx = -INFINITY, tmn = INFINITY, tmx = -INFINITY;
    for (uint32_t i = blockIdx.x * kT + threadIdx.x; i < P.n; i += gridDim.x * kT) {
        const float* p = P.pred + (size_t)i * 3;
        const float* g = P.truth + (size_t)i * P.C;
        uint8_t p8[3], t8[3];
#pragma unroll
        for (uint32_t ch = 0; ch < 3; ++ch) {
            const float pv = p[ch], tv = truth_of(g, P.C, ch, P.bg);
            const float d = pv - tv;
            acc += (double)(d * d);
            pmn = fminf(pmn, pv); pmx = fmaxf(pmx, pv);
            tmn = fminf(tmn, tv); tmx = fmaxf(tmx, tv);
            p8[ch] = to_u8(pv); t8[ch] = to_u8(tv);
            if (P.truth_out) P.truth_out[(size_t)i * 3 + ch] = tv;
            if (P.pred_u8) P.pred_u8[(size_t)i * 3 + ch] = p8[ch];
            if (P.truth_u8) P.truth_u8[(size_t)i * 3 + ch] = t8[ch];
        }
        if (P.error_u8) {
            const float e0 = fabsf((float)t8[0] - (float)p8[0]), e1 = fabsf((float)t8[1] - (float)p8[1]),
                        e2 = fabsf((float)t8[2] - (float)p8[2]);
            P.error_u8[i] = (uint8_t)(int)(((e0 + e1) + e2) / 3.0f);
        }
    }
    float mm[4] = {pmn, pmx, tmn, tmx};
    wave_all(mm, MinMax{});
    waves_put(mm, shf);
    const double sq = block_sum_ordered(acc, shd);    // its barriers order shf as well
    if (threadIdx.x == 0) {
        float r[4] = {shf[0], shf[1], shf[2], shf[3]};
        waves_fold(r, shf, kWaves, MinMax{});
        P.ws->rgb[blockIdx.x] = RgbPart{sq, r[0], r[1], r[2], r[3]};
    }
}

// One pixel's ids into the LDS histograms; bad: ids that index nothing
__device__ __forceinline__ void hist_add(uint32_t* hist, uint32_t nc, int64_t pred, int64_t truth, uint32_t* bad) {
    if (pred >= 0 && pred < (int64_t)nc) atomicAdd(&hist[nc + (uint32_t)pred], 1u);
    else atomicAdd(bad, 1u);
    if (truth >= (int64_t)nc) atomicAdd(bad, 1u);
    else if (truth >= 0) {
        atomicAdd(&hist[2 * nc + (uint32_t)truth], 1u);
        if (truth == pred) atomicAdd(&hist[(uint32_t)truth], 1u);
    }
}

// hist[0 .. 3 nc) and the two counters behind it, into the record
__device__ __forceinline__ void hist_flush(const Params& P, const uint32_t* hist) {
    const uint32_t nc = P.n_classes;
    for (uint32_t b = threadIdx.x; b < 3 * nc; b += blockDim.x)
        if (hist[b]) atomicAdd(&P.hist[b], hist[b]);
    if (threadIdx.x == 0) {
        if (hist[3 * nc]) atomicAdd((unsigned long long*)&P.stats->overflow, (unsigned long long)hist[3 * nc]);
        if (hist[3 * nc + 1]) atomicAdd((unsigned long long*)&P.stats->n_labeled, (unsigned long long)hist[3 * nc + 1]);
    }
}

// blockDim.x pixels a chunk: 256, or 128 at K > 32 (the rows must fit LDS)
__global__ void __launch_bounds__(kT) k_eval_mask(Params P) {
    extern __shared__ float sm[];
    __shared__ double shd[kWaves];
    const uint32_t T = blockDim.x, t = threadIdx.x, K = P.K, Kp = P.Kp, nc = P.n_classes;
    float* sz = sm;                                            // [T][Kp]
    uint32_t* hist = reinterpret_cast<uint32_t*>(sm + T * Kp); // [3 nc] + bad + labeled
    for (uint32_t b = t; b < 3 * nc + 2; b += T) hist[b] = 0u;
    double acc = 0.0;
    const uint32_t chunks = (P.n + T - 1) / T;
    for (uint32_t chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x) {
        const uint32_t base = chunk * T, cnt = min(T, P.n - base), i = base + t;
        __syncthreads();
        rows_to_tile(sz, P.logits, (size_t)base * K, cnt, K, Kp, T);
        __syncthreads();
        if (t < cnt) {
            float* z = sz + t * Kp;
            const uint32_t arg = instance_row<2>(z, K, P.n_inst).arg;
            if (P.ids) P.ids[i] = (int64_t)arg;
            const int64_t label = P.labels[i];
            hist_add(hist, nc, (int64_t)arg, label, &hist[3 * nc]);
            if (label != -1) {
                if (label >= 0 && label < (int64_t)K) {
                    const float p = fminf(fmaxf(z[label], P.lo), P.hi);
                    acc += (double)(-logf(p));
                    atomicAdd(&hist[3 * nc + 1], 1u);
                } else {
                    atomicAdd(&hist[3 * nc], 1u);
                }
            }
        }
        __syncthreads();
        if (P.probs) tile_to_rows(P.probs, (size_t)base * K, sz, cnt, K, Kp, T);
    }
    __syncthreads();
    hist_flush(P, hist);
    const double s = block_sum_ordered(acc, shd);
    if (t == 0) P.ws->nll[blockIdx.x] = s;
}

__global__ void __launch_bounds__(kT) k_eval_confusion(Params P, const int64_t* pred, const int64_t* truth) {
    extern __shared__ float sm[];
    uint32_t* hist = reinterpret_cast<uint32_t*>(sm);
    const uint32_t nc = P.n_classes;
    for (uint32_t b = threadIdx.x; b < 3 * nc + 2; b += kT) hist[b] = 0u;
    __syncthreads();
    for (uint32_t i = blockIdx.x * kT + threadIdx.x; i < P.n; i += gridDim.x * kT)
        hist_add(hist, nc, pred[i], truth[i], &hist[3 * nc]);
    __syncthreads();
    hist_flush(P, hist);
}

// tile (pixel block pb, channel block cb): 64 pixels x 64 channels
__global__ void __launch_bounds__(kT) k_eval_sam(Params P) {
    __shared__ float sg[kFT][kFT + 1];        // [channel][pixel]
    __shared__ double shd[kWaves];
    const uint32_t t = threadIdx.x, lane = t & 63u, row4 = t >> 6;
    const uint32_t pblocks = (P.hw + kFT - 1) / kFT, tiles = pblocks * (kFeat / kFT);
    double acc = 0.0;
    for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const uint32_t pb = tile / (kFeat / kFT), cb = tile - pb * (kFeat / kFT);
        const uint32_t i0 = pb * kFT, c0 = cb * kFT, cnt = min(kFT, P.hw - i0);
        __syncthreads();
        for (uint32_t c = row4; c < kFT; c += kWaves)          // lane = pixel: contiguous in gt
            if (lane < cnt) sg[c][lane] = P.gf[(size_t)(c0 + c) * P.hw + i0 + lane];
        __syncthreads();
        for (uint32_t r = row4; r < cnt; r += kWaves) {        // lane = channel: contiguous in pred
            const float d = P.pf[(size_t)(i0 + r) * kFeat + c0 + lane] - sg[lane][r];
            acc += (double)(d * d);
        }
    }
    const double s = block_sum_ordered(acc, shd);
    if (t == 0) P.ws->feat[blockIdx.x] = s;
}

__global__ void __launch_bounds__(kT) k_eval_ssim(Params P) {
    __shared__ float sp[kIH * kIW], st[kIH * kIW];
    __shared__ float sh[5][kIH * kTW];
    __shared__ double shd[kWaves];
    const uint32_t t = threadIdx.x;
    const samnerf_eval_stats* S = P.stats;
    const float L = fmaxf(S->pred_max - S->pred_min, S->truth_max - S->truth_min);
    const float k1 = 0.01f * L, k2 = 0.03f * L;
    const float c1 = k1 * k1, c2 = k2 * k2;
    const uint32_t OW = P.W - kHalo, OH = P.H - kHalo;
    const uint32_t tx_n = (OW + kTW - 1) / kTW, ty_n = (OH + kTH - 1) / kTH, tiles = tx_n * ty_n * 3;
    double acc = 0.0;
    for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const uint32_t tt = tile / 3, ch = tile - tt * 3, ty = tt / tx_n, tx = tt - ty * tx_n;
        const uint32_t x0 = tx * kTW, y0 = ty * kTH;           // output (y, x) reads rows y .. y + 10
        const uint32_t iw = min(kIW, P.W - x0), ih = min(kIH, P.H - y0);
        __syncthreads();
        for (uint32_t e = t; e < kIH * kIW; e += kT) {
            const uint32_t r = e / kIW, c = e - r * kIW;
            float pv = 0.0f, tv = 0.0f;
            if (r < ih && c < iw) {
                const size_t px = (size_t)(y0 + r) * P.W + x0 + c;
                pv = P.pred[px * 3 + ch];
                tv = truth_of(P.truth + px * P.C, P.C, ch, P.bg);
            }
            sp[e] = pv; st[e] = tv;
        }
        __syncthreads();
        for (uint32_t e = t; e < kIH * kTW; e += kT) {
            const uint32_t r = e / kTW, c = e - r * kTW;
            float m[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (uint32_t k = 0; k < kTaps; ++k) {
                const float pv = sp[r * kIW + c + k], tv = st[r * kIW + c + k], g = P.g[k];
                m[0] = __builtin_fmaf(g, pv, m[0]);
                m[1] = __builtin_fmaf(g, tv, m[1]);
                m[2] = __builtin_fmaf(g, pv * pv, m[2]);
                m[3] = __builtin_fmaf(g, tv * tv, m[3]);
                m[4] = __builtin_fmaf(g, pv * tv, m[4]);
            }
#pragma unroll
            for (uint32_t q = 0; q < 5; ++q) sh[q][e] = m[q];
        }
        __syncthreads();
        for (uint32_t e = t; e < kTH * kTW; e += kT) {
            const uint32_t r = e / kTW, c = e - r * kTW;
            if (y0 + r >= OH || x0 + c >= OW) continue;
            float m[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (uint32_t k = 0; k < kTaps; ++k) {
                const float g = P.g[k];
#pragma unroll
                for (uint32_t q = 0; q < 5; ++q) m[q] = __builtin_fmaf(g, sh[q][(r + k) * kTW + c], m[q]);
            }
            const float mp2 = m[0] * m[0], mt2 = m[1] * m[1], mpt = m[0] * m[1];
            const float sp2 = m[2] - mp2, st2 = m[3] - mt2, spt = m[4] - mpt;
            const float upper = 2.0f * spt + c2, lower = (sp2 + st2) + c2;
            const float v = ((2.0f * mpt + c1) * upper) / (((mp2 + mt2) + c1) * lower);
            acc += (double)v;
        }
    }
    const double s = block_sum_ordered(acc, shd);
    if (t == 0) P.ws->ssim[blockIdx.x] = s;
}

// The partials of one sum stand in LDS (every thread loads its share at once) and one
// thread adds them in index order; the three sums of stage 0 go to three waves.
// stage 0: every sum but SSIM's, min / max and the counts; stage 1: SSIM
__global__ void __launch_bounds__(kT) k_eval_finish(Params P, int stage) {
    __shared__ double sh[3][kMaxParts];
    __shared__ float shf[4 * kWaves];
    samnerf_eval_stats* S = P.stats;
    const uint32_t t = threadIdx.x;
    if (stage == 1) {
        for (uint32_t b = t; b < P.n_ssim; b += kT) sh[0][b] = P.ws->ssim[b];
        __syncthreads();
        if (t == 0) {
            double a = 0.0;
#pragma unroll 16
            for (uint32_t b = 0; b < P.n_ssim; ++b) a += sh[0][b];
            S->ssim_sum = a;
            S->n_ssim = (uint64_t)(P.H - kHalo) * (P.W - kHalo) * 3;
        }
        return;
    }
    float pmn = INFINITY, pmx = -INFINITY, tmn = INFINITY, tmx = -INFINITY;
    for (uint32_t b = t; b < P.n_rgb; b += kT) {
        const RgbPart& o = P.ws->rgb[b];
        sh[0][b] = o.sq;
        pmn = fminf(pmn, o.pmin); pmx = fmaxf(pmx, o.pmax);
        tmn = fminf(tmn, o.tmin); tmx = fmaxf(tmx, o.tmax);
    }
    for (uint32_t b = t; b < P.n_mask; b += kT) sh[1][b] = P.ws->nll[b];
    for (uint32_t b = t; b < P.n_feat; b += kT) sh[2][b] = P.ws->feat[b];
    float mm[4] = {pmn, pmx, tmn, tmx};
    wave_all(mm, MinMax{});
    waves_put(mm, shf);
    __syncthreads();
    if (t == 0 && P.n_rgb) {
        double a = 0.0;
#pragma unroll 16
        for (uint32_t b = 0; b < P.n_rgb; ++b) a += sh[0][b];
        waves_fold(mm, shf, kWaves, MinMax{});         // thread 0 holds wave 0's
        S->sq_sum = a;
        S->n_elem = (uint64_t)P.n * 3;
        S->pred_min = mm[0]; S->pred_max = mm[1]; S->truth_min = mm[2]; S->truth_max = mm[3];
    }
    if (t == 64 && P.n_mask) {
        double a = 0.0;
#pragma unroll 16
        for (uint32_t b = 0; b < P.n_mask; ++b) a += sh[1][b];
        S->nll_sum = a;
    }
    if (t == 128 && P.n_feat) {
        double a = 0.0;
#pragma unroll 16
        for (uint32_t b = 0; b < P.n_feat; ++b) a += sh[2][b];
        S->feat_sq_sum = a;
        S->n_feat = (uint64_t)P.hw * kFeat;
    }
}

// workgroups for `work` chunks: at most kMaxParts, each with the same number of chunks but the last
uint32_t parts_for(uint32_t work) { return div_up(work, div_up(work, kMaxParts)); }

const char* validate(const samnerf_eval_args* a) {
    if (!a) return "null args";
    if (!a->stats || ((uintptr_t)a->stats & 7u)) return "stats must be a non-null, 8-byte aligned record";
    const bool rgb = a->C != 0, mask = a->K != 0, sam = a->h != 0 || a->w != 0;
    if (!rgb && !mask && !sam) return "no part asked for (C, K and h x w are all 0)";
    if (rgb || mask) {
        if (a->H == 0 || a->W == 0) return "H and W must be at least 1";
        if ((uint64_t)a->H * a->W * (a->K > 4 ? a->K : 4) > 0x7fffffffull) return "H * W * max(K, 4) must stay below 2^31";
    }
    if (rgb) {
        if (a->C != 3 && a->C != 4) return "C (the truth's channels) must be 3 or 4";
        if (!a->pred_rgb || !a->truth) return "the RGB part needs pred_rgb and truth";
    } else if (a->pred_u8 || a->truth_u8 || a->error_u8 || a->truth_out) {
        return "the uint8 buffers and truth_out need the RGB part";
    }
    if (a->ssim) {
        if (!rgb) return "SSIM needs the RGB part";
        if (a->H < kTaps || a->W < kTaps) return "SSIM needs H, W >= 11: one whole window";
    }
    if (mask) {
        if (a->K > kMaxEvalK) return "K (n_inst + redundant_instance) must lie in [1, 64]";
        if (a->n_inst < 1 || a->n_inst > a->K) return "n_inst must lie in [1, K]";
        if (a->n_classes < 1 || a->n_classes > SAMNERF_EVAL_MAX_CLASSES) return "n_classes must lie in [1, 1024]";
        if (!a->logits || !a->labels) return "the mask part needs logits and labels";
    } else if (a->probs || a->ids) {
        return "probs and ids need the mask part";
    }
    if (sam) {
        if (a->h == 0 || a->w == 0) return "h and w must both be at least 1";
        if ((uint64_t)a->h * a->w * kFeat > 0x7fffffffull) return "h * w * 256 must stay below 2^31";
        if (!a->pred_feat || !a->gt_feat) return "the SAM part needs pred_feat and gt_feat";
    }
    return nullptr;
}

}  // namespace

extern "C" int samnerf_eval_workspace_size(const samnerf_eval_args* args, size_t* bytes) {
    if (!bytes) return fail(SAMNERF_EINVAL, "eval_workspace_size: null bytes");
    *bytes = 0;
    if (const char* why = validate(args)) return fail(SAMNERF_EINVAL, "eval_workspace_size: %s", why);
    *bytes = sizeof(Workspace);
    return 0;
}

extern "C" int samnerf_eval_frame(const samnerf_eval_args* args, samnerf_stream_t stream) {
    if (const char* why = validate(args)) return fail(SAMNERF_EINVAL, "eval_frame: %s", why);
    const samnerf_eval_args& a = *args;
    if (!a.workspace || ((uintptr_t)a.workspace & 7u) || a.workspace_bytes < sizeof(Workspace))
        return fail(SAMNERF_EWORKSPACE, "eval_frame: workspace of %zu bytes, %zu needed (8-byte aligned)",
                    a.workspace ? a.workspace_bytes : (size_t)0, sizeof(Workspace));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const uint32_t nc = a.K ? a.n_classes : 0;
    Params P{};
    P.H = a.H; P.W = a.W; P.n = a.H * a.W; P.C = a.C; P.K = a.K; P.Kp = a.K | 1u; P.n_inst = a.n_inst;
    P.n_classes = nc; P.hw = a.h * a.w;
    P.bg = a.bg_color; P.lo = (float)a.epsilon; P.hi = (float)(1.0 - a.epsilon);
    // torchmetrics' _gaussian(11, 1.5) as fp32 bits: exp(-((i - 5) / 1.5)^2 / 2) / sum evaluated in
    // double and rounded once.  (An fp32 evaluation differs in the last bits from one expf to the
    // next; evaluate.py's mirror and the tests' oracle read the same table.)
    static const uint32_t kWindowBits[6] = {981912246u, 1006173953u, 1024685452u, 1038088319u, 1046093344u,
                                            1049113264u};
    for (uint32_t i = 0; i < kTaps; ++i) {
        const uint32_t b = kWindowBits[i < 6 ? i : 10 - i];
        memcpy(&P.g[i], &b, 4);
    }
    P.pred = a.pred_rgb; P.truth = a.truth; P.logits = a.logits; P.labels = a.labels;
    P.pf = a.pred_feat; P.gf = a.gt_feat;
    P.pred_u8 = a.pred_u8; P.truth_u8 = a.truth_u8; P.error_u8 = a.error_u8; P.truth_out = a.truth_out;
    P.probs = a.probs; P.ids = a.ids;
    P.stats = static_cast<samnerf_eval_stats*>(a.stats);
    P.hist = reinterpret_cast<uint32_t*>(P.stats + 1);
    P.ws = static_cast<Workspace*>(a.workspace);
    if (hipMemsetAsync(a.stats, 0, SAMNERF_EVAL_STATS_BYTES(nc), s) != hipSuccess)
        return fail(SAMNERF_ELAUNCH, "eval_frame: clearing the record failed");
    int rc;
    if (a.C) {
        P.n_rgb = parts_for(div_up(P.n, kT));
        k_eval_rgb<<<P.n_rgb, kT, 0, s>>>(P);
        if ((rc = check_launch("eval rgb"))) return rc;
    }
    if (a.K) {
        const uint32_t T = a.K > kTreeLanes ? kT / 2 : kT;
        P.n_mask = parts_for(div_up(P.n, T));
        const size_t lds = ((size_t)T * P.Kp + 3 * nc + 2) * 4;          // <= 46 KiB
        k_eval_mask<<<P.n_mask, T, lds, s>>>(P);
        if ((rc = check_launch("eval mask"))) return rc;
    }
    if (P.hw) {
        P.n_feat = parts_for(div_up(P.hw, kFT) * (kFeat / kFT));
        k_eval_sam<<<P.n_feat, kT, 0, s>>>(P);
        if ((rc = check_launch("eval sam"))) return rc;
    }
    if (a.ssim) {
        const uint32_t tiles = div_up(a.W - kHalo, kTW) * div_up(a.H - kHalo, kTH) * 3;
        P.n_ssim = parts_for(tiles);
    }
    k_eval_finish<<<1, kT, 0, s>>>(P, 0);
    if ((rc = check_launch("eval finish"))) return rc;
    if (a.ssim) {
        k_eval_ssim<<<P.n_ssim, kT, 0, s>>>(P);
        if ((rc = check_launch("eval ssim"))) return rc;
        k_eval_finish<<<1, kT, 0, s>>>(P, 1);
        if ((rc = check_launch("eval ssim finish"))) return rc;
    }
    return 0;
}

extern "C" int samnerf_eval_confusion(const int64_t* pred_ids, const int64_t* truth_ids, uint32_t n,
                                      uint32_t n_classes, void* stats, samnerf_stream_t stream) {
    if (!stats || ((uintptr_t)stats & 7u)) return fail(SAMNERF_EINVAL, "eval_confusion: stats must be a non-null, 8-byte aligned record");
    if (n_classes < 1 || n_classes > SAMNERF_EVAL_MAX_CLASSES)
        return fail(SAMNERF_EINVAL, "eval_confusion: n_classes must lie in [1, 1024]");
    if (n && (!pred_ids || !truth_ids)) return fail(SAMNERF_EINVAL, "eval_confusion: null id map");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (hipMemsetAsync(stats, 0, SAMNERF_EVAL_STATS_BYTES(n_classes), s) != hipSuccess)
        return fail(SAMNERF_ELAUNCH, "eval_confusion: clearing the record failed");
    if (!n) return 0;
    Params P{};
    P.n = n; P.n_classes = n_classes;
    P.stats = static_cast<samnerf_eval_stats*>(stats);
    P.hist = reinterpret_cast<uint32_t*>(P.stats + 1);
    k_eval_confusion<<<parts_for(div_up(n, kT)), kT, ((size_t)3 * n_classes + 2) * 4, s>>>(P, pred_ids, truth_ids);
    return check_launch("eval confusion");
}
