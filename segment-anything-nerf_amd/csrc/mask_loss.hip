// mask_loss.hip -- the loss of Trainer.train_step's --with_mask branch
// (nerf/utils.py:959-1067) and its gradient to the logits: the NLL with its
// incoherent-region re-weighting, the error-map EMA, the label regularisation
// (utils.py:843-870) and the RGB-similarity term of mixed sampling
// (utils.py:761-841).  The reference runs them as some twenty small ATen
// launches and two host read-backs around the render; here they are a handful
// of launches on the caller's stream with no read-back.
//
// Everything is fp32 in the reference's op order per element.  Every sum runs
// in an order fixed by the sizes alone: a ray's K values as a fixed tree
// (instance_row.h: the softmax and, with the same tree_sum32, its backward) or
// in index order, a per-ray or per-patch partial stored to the workspace, and
// one 256-thread workgroup (k_ml_reduce) that adds the partials strided by 256
// and then as a tree (block_reduce.h block_sum_tree).  No float atomics: the
// same inputs give the same bits.
//
//   k_ml_rows    per ray: softmax p -> workspace, argmax, and for a global ray
//                its NLL, the clamped q of its label and its error-map value
//                (the old map value is read here, before anything writes)
//   k_ml_em      the EMA's scatter with "the last ray in ray order wins": zero
//                the touched cells, atomicMax of ray + 1 on them as uint32,
//                note the winners, the winners write
//   k_ml_lr      per ray: its right / lower neighbour's weighted squared
//                differences inside its P x P patch
//   k_ml_rgb     one workgroup per local patch, p and rgb of the patch in LDS
//   k_ml_reduce  all the sums, the five loss terms, the gradient's scalars
//   k_ml_grad    per ray: d total / d p from the three terms, then through
//                the softmax
//
// An out-of-range label, sample or cell is never used as an index (see the
// header): flagged per ray / counted per patch, summed into loss_terms[4].
#include <cmath>

#include "block_reduce.h"
#include "instance_row.h"
#include "samnerf_common.h"

using namespace samnerf;

namespace {

constexpr uint32_t kT = 256;                 // threads of every workgroup here
constexpr uint32_t kWaves = kT / 64;
constexpr uint32_t kMaxQK = 8192, kMaxQ = 1024, kMaxS = 256;

enum : uint32_t {
    F_LABELLED = 1u,      // label != -1
    F_BAD_LABEL = 2u,     // global ray, label outside [0, K)
    F_BAD_CELL = 4u,      // global ray, cell outside the map
    F_EMA = 8u,           // global ray that updates the error map
};

// the workspace, in 4-byte words
struct Layout {
    size_t p, gp_rgb, nll, q, err, old, win, flags, lr, rgb_part, rgb_bad, scal, words;
};

enum { SC_CN = 0, SC_GX, SC_GY, SC_RGB, SC_COUNT = 8 };

Layout layout(const samnerf_mask_loss_args& a) {
    Layout l{};
    size_t w = 0;
    auto take = [&](size_t n) { const size_t at = w; w += (n + 3) & ~(size_t)3; return at; };
    l.p = take((size_t)a.N * a.K);
    l.gp_rgb = take(a.rgb_weight > 0 ? (size_t)a.L * a.Q * a.K : 0);
    l.nll = take(a.n);
    l.q = take(a.n);
    l.err = take(a.n);
    l.old = take(a.n);
    l.win = take(a.n);
    l.flags = take(a.N);
    l.lr = take(a.label_reg_weight > 0 ? (size_t)4 * a.N : 0);
    l.rgb_part = take(a.L);
    l.rgb_bad = take(a.L);
    l.scal = take(SC_COUNT);
    l.words = w;
    return l;
}

struct Params {
    uint32_t N, K, n, L, Q, S, P;
    int redundant, logistics, reweight, ema, lr_on, rgb_on;
    float eps, one_m_eps, u, wl, wr, thr, a;
    uint64_t map_cells;
    const float* z;
    const int64_t* labels;
    const float* incoherent;
    float* map;
    const int64_t* cells;
    const float* depth;
    const float* image;
    const int64_t* samples;
    float* p;
    float* gp_rgb;
    float* nll;
    float* q;
    float* err;
    float* old;
    uint32_t* win;
    uint32_t* flags;
    float* lr;
    float* rgb_part;
    uint32_t* rgb_bad;
    float* scal;
    float* terms;
    float* grad;
    int64_t* ids;
};

__global__ void __launch_bounds__(kT) k_ml_rows(Params P) {
    const uint32_t i = blockIdx.x * kT + threadIdx.x;
    if (i >= P.N) return;
    const uint32_t K = P.K;
    const float* z = P.z + (size_t)i * K;
    float* p = P.p + (size_t)i * K;
    const RowNorm nrm = row_norm<1>(z, K);
    const int64_t g = P.labels[i];
    const bool label_ok = g >= 0 && g < (int64_t)K;
    float pg = 0.0f, sq = 0.0f;
    RowBest b;
    for (uint32_t k = 0; k < K; ++k) {
        const float v = row_prob(z, k, nrm);
        p[k] = v;
        b.take(k, v);
        if (label_ok && k == (uint32_t)g) pg = v;
        sq += v * v;
    }
    P.ids[i] = (int64_t)b.arg;
    uint32_t f = g != -1 ? F_LABELLED : 0u;
    if (i < P.n) {
        float nll = 0.0f, q = 0.0f;
        if (!label_ok) {
            f |= F_BAD_LABEL;
        } else {
            const float c = fminf(fmaxf(pg, P.eps), P.one_m_eps);
            nll = -logf(c);
            q = (pg >= P.eps && pg <= P.one_m_eps) ? c : 0.0f;     // 0: the clamp binds, no gradient
            if (P.ema) {
                const int64_t cell = P.cells[i];
                if (cell < 0 || (uint64_t)cell >= P.map_cells) {
                    f |= F_BAD_CELL;
                } else {
                    // cos(p, onehot) = p_g / |p|; |p| >= K^-1/2 on the simplex
                    const float cs = pg / fmaxf(sqrtf(sq), 1e-8f);
                    P.err[i] = expf(-P.a * cs - P.eps);
                    P.old[i] = P.map[cell];
                    f |= F_EMA;
                }
            }
        }
        P.nll[i] = nll;
        P.q[i] = q;
    }
    P.flags[i] = f;
}

// step 0: zero the touched cells; 1: the largest ray + 1 per cell; 2: note the
// winners; 3: the winners write.  Each step is its own launch: the next one
// reads what every thread of this one wrote.
__global__ void __launch_bounds__(kT) k_ml_em(Params P, int step) {
    const uint32_t i = blockIdx.x * kT + threadIdx.x;
    if (i >= P.n || !(P.flags[i] & F_EMA)) return;
    const int64_t cell = P.cells[i];                   // validated by k_ml_rows (F_EMA)
    uint32_t* word = reinterpret_cast<uint32_t*>(P.map) + cell;
    if (step == 0) *word = 0u;
    else if (step == 1) atomicMax(word, i + 1u);
    else if (step == 2) P.win[i] = (*word == i + 1u) ? 1u : 0u;
    else if (P.win[i]) P.map[cell] = 0.1f * P.old[i] + 0.9f * P.err[i];
}

__global__ void __launch_bounds__(kT) k_ml_lr(Params P) {
    const uint32_t i = blockIdx.x * kT + threadIdx.x;
    if (i >= P.N) return;
    const uint32_t K = P.K, S = P.P;
    const uint32_t in = i % (S * S), x = in % S, y = in / S;
    const float* p = P.p + (size_t)i * K;
    float ax = 0.0f, wx = 0.0f, ay = 0.0f, wy = 0.0f;
    if (x + 1 < S) {                                   // i + 1 is inside the patch, so inside N
        const float dd = P.depth[i + 1] - P.depth[i];
        wx = expf(-(dd * dd));
        for (uint32_t k = 0; k < K; ++k) {
            const float d = p[K + k] - p[k];
            ax += d * d * wx;
        }
    }
    if (y + 1 < S) {
        const float dd = P.depth[i + S] - P.depth[i];
        wy = expf(-(dd * dd));
        const float* pd = p + (size_t)S * K;
        for (uint32_t k = 0; k < K; ++k) {
            const float d = pd[k] - p[k];
            ay += d * d * wy;
        }
    }
    float* o = P.lr + (size_t)4 * i;
    o[0] = ax; o[1] = wx; o[2] = ay; o[3] = wy;
}

// One pixel r against one sample: whether their colours are similar, the
// cosine c of p_r with the sample's mask and e = exp(-a c - epsilon).
struct Pair { bool sim; float c, e; };

__device__ __forceinline__ Pair rgb_pair(const Params& P, const float* sp, const float* srgb, const float* snrm,
                                         uint32_t r, uint32_t j, uint32_t arg) {
    const float dx = srgb[3 * r] - srgb[3 * j], dy = srgb[3 * r + 1] - srgb[3 * j + 1],
                dz = srgb[3 * r + 2] - srgb[3 * j + 2];
    Pair o;
    o.sim = sqrtf(dx * dx + dy * dy + dz * dz) < P.thr;
    float dot, nm;
    if (P.logistics) {
        dot = 0.0f;
        for (uint32_t k = 0; k < P.K; ++k) dot += sp[r * P.K + k] * sp[j * P.K + k];
        nm = fmaxf(snrm[j], 1e-8f);
    } else {
        dot = sp[r * P.K + arg];
        nm = 1.0f;
    }
    o.c = dot / (fmaxf(snrm[r], 1e-8f) * nm);
    o.e = expf(-P.a * o.c - P.eps);
    return o;
}

__global__ void __launch_bounds__(kT) k_ml_rgb(Params P) {
    extern __shared__ float sm[];
    const uint32_t K = P.K, Q = P.Q, S = P.S, l = blockIdx.x, t = threadIdx.x;
    float* sp = sm;                                     // [Q][K]  the patch's softmax
    float* srgb = sp + Q * K;                           // [Q][3]
    float* snrm = srgb + Q * 3;                         // [Q]     |p_r|
    float* swp = snrm + Q;                              // [S][kWaves] per-wave sums of a sample
    int* ssamp = reinterpret_cast<int*>(swp + S * kWaves);   // [S] the sample's pixel, -1 = invalid
    int* sarg = ssamp + S;                              // [S] argmax of its p
    int* scnt = sarg + S;                               // [S] similar pixels
    const size_t row0 = (size_t)P.n + (size_t)l * Q;
    for (uint32_t e = t; e < Q * K; e += kT) sp[e] = P.p[row0 * K + e];
    for (uint32_t e = t; e < Q * 3; e += kT) srgb[e] = P.image[row0 * 3 + e];
    for (uint32_t s = t; s < S; s += kT) {
        const int64_t j = P.samples[(size_t)l * S + s];
        ssamp[s] = (j >= 0 && j < (int64_t)Q) ? (int)j : -1;
    }
    __syncthreads();
    for (uint32_t r = t; r < Q; r += kT) {
        float sq = 0.0f;
        for (uint32_t k = 0; k < K; ++k) sq += sp[r * K + k] * sp[r * K + k];
        snrm[r] = sqrtf(sq);
    }
    for (uint32_t s = t; s < S; s += kT) {
        const int j = ssamp[s];
        RowBest b;
        int cnt = 0;
        if (j >= 0) {
            for (uint32_t k = 0; k < K; ++k) b.take(k, sp[j * K + k]);
            for (uint32_t r = 0; r < Q; ++r) {          // an integer count: any order
                const float dx = srgb[3 * r] - srgb[3 * j], dy = srgb[3 * r + 1] - srgb[3 * j + 1],
                            dz = srgb[3 * r + 2] - srgb[3 * j + 2];
                cnt += sqrtf(dx * dx + dy * dy + dz * dz) < P.thr ? 1 : 0;
            }
        }
        sarg[s] = (int)b.arg;
        scnt[s] = cnt;
    }
    __syncthreads();
    // the loss: per sample the sum over the patch's pixels (a thread's pixels
    // in order, the wave's lanes as a tree, the waves in order below)
    for (uint32_t s = 0; s < S; ++s) {
        const int j = ssamp[s];
        float v = 0.0f;
        if (j >= 0) {
            for (uint32_t r = t; r < Q; r += kT) {
                const Pair pr = rgb_pair(P, sp, srgb, snrm, r, (uint32_t)j, (uint32_t)sarg[s]);
                if (P.redundant) {
                    // binary_cross_entropy(e, 1 - sim), torch's clamp of the logs at -100
                    const float le = fmaxf(logf(pr.e), -100.0f), l1 = fmaxf(log1pf(-pr.e), -100.0f);
                    v += pr.sim ? -l1 : -le;
                } else {
                    v += pr.sim ? pr.e : 0.0f;
                }
            }
        }
        waves_put(wave_sum_down(v), swp + s * kWaves);
    }
    __syncthreads();
    if (t == 0) {
        float tot = 0.0f;
        uint32_t bad = 0;
        for (uint32_t s = 0; s < S; ++s) {
            if (ssamp[s] < 0) { ++bad; continue; }
            const float v = sum_waves4(swp + s * kWaves);
            tot += P.redundant ? v : v / (float)scnt[s];     // scnt >= 1: a sample is similar to itself
        }
        P.rgb_part[l] = tot;
        P.rgb_bad[l] = bad;
    }
    // the gradient to p_r, per pixel over the samples in order.  With
    // c = p_r . m / (|p_r| |m|):  dc/dp_r = m / (|p_r| |m|) - c p_r / |p_r|^2.
    for (uint32_t r = t; r < Q; r += kT) {
        float* g = P.gp_rgb + ((size_t)l * Q + r) * K;       // this thread's row alone
        for (uint32_t k = 0; k < K; ++k) g[k] = 0.0f;
        const float nr = fmaxf(snrm[r], 1e-8f);
        float back = 0.0f;                                    // sum of gc * c
        for (uint32_t s = 0; s < S; ++s) {
            const int j = ssamp[s];
            if (j < 0) continue;
            const Pair pr = rgb_pair(P, sp, srgb, snrm, r, (uint32_t)j, (uint32_t)sarg[s]);
            float ge;
            if (P.redundant) {
                const float y = pr.sim ? 0.0f : 1.0f;
                ge = (pr.e - y) / fmaxf((1.0f - pr.e) * pr.e, 1e-12f);
            } else {
                if (!pr.sim) continue;
                ge = 1.0f / (float)scnt[s];
            }
            const float gc = ge * (-P.a * pr.e);
            back += gc * pr.c;
            if (P.logistics) {
                const float inv = gc / (nr * fmaxf(snrm[j], 1e-8f));
                for (uint32_t k = 0; k < K; ++k) g[k] += inv * sp[(uint32_t)j * K + k];
            } else {
                g[sarg[s]] += gc / nr;
            }
        }
        const float b = back / (nr * nr);
        for (uint32_t k = 0; k < K; ++k) g[k] -= b * sp[r * K + k];
    }
}

__global__ void __launch_bounds__(kT) k_ml_reduce(Params P) {
    __shared__ float sh[kWaves];
    const uint32_t t = threadIdx.x;
    float nll = 0.0f, w = 0.0f, labelled = 0.0f, bad = 0.0f;
    for (uint32_t i = t; i < P.n; i += kT) nll += P.nll[i];
    for (uint32_t i = t; i < P.N; i += kT) {
        const uint32_t f = P.flags[i];
        labelled += (f & F_LABELLED) ? 1.0f : 0.0f;    // counts below 2^24: exact in float
        bad += ((f & F_BAD_LABEL) ? 1.0f : 0.0f) + ((f & F_BAD_CELL) ? 1.0f : 0.0f);
        if (P.reweight) {
            const float m = P.incoherent[i];
            w += 1.0f - m + P.u * m;
        }
    }
    nll = block_sum_tree(nll, sh);
    w = block_sum_tree(w, sh);
    labelled = block_sum_tree(labelled, sh);
    bad = block_sum_tree(bad, sh);
    float ax = 0.0f, wx = 0.0f, ay = 0.0f, wy = 0.0f;
    if (P.lr_on) {
        for (uint32_t i = t; i < P.N; i += kT) {
            const float* o = P.lr + (size_t)4 * i;
            ax += o[0]; wx += o[1]; ay += o[2]; wy += o[3];
        }
        ax = block_sum_tree(ax, sh);
        wx = block_sum_tree(wx, sh);
        ay = block_sum_tree(ay, sh);
        wy = block_sum_tree(wy, sh);
    }
    if (t != 0) return;
    const bool any = labelled > 0.0f;
    // a label that nothing gathers with is no error: with no labelled ray the
    // reference skips the gather, and only the error map would index with it
    if (!any && !P.ema) bad = 0.0f;
    float cn = 0.0f, t_nll = 0.0f;
    if (any) {
        t_nll = nll / (float)P.n;
        cn = 1.0f / (float)P.n;
        if (P.reweight) {
            // mean(w) * mean(nll) and mean(w) / n from the two float sums, each
            // rounded once (formed in float the three roundings cost up to 2 ulp
            // of the loss, more than the sums themselves)
            const double wbar = (double)w / (double)P.N;
            t_nll = (float)(wbar * ((double)nll / (double)P.n));
            cn = (float)(wbar / (double)P.n);
        }
    }
    float t_lr = 0.0f, gx = 0.0f, gy = 0.0f;
    if (P.lr_on) {
        // the reference sums the weights expanded over the K instances
        const float sx = (float)P.K * wx, sy = (float)P.K * wy;
        t_lr = ax / sx + ay / sy;
        gx = P.wl / sx;
        gy = P.wl / sy;
    }
    float t_rgb = 0.0f, grgb = 0.0f;
    if (P.rgb_on) {
        float tot = 0.0f;
        for (uint32_t l = 0; l < P.L; ++l) {
            tot += P.rgb_part[l];
            bad += (float)P.rgb_bad[l];
        }
        const float count = (float)P.L * (float)P.S * (P.redundant ? (float)P.Q : 1.0f);
        t_rgb = tot / count;
        grgb = P.wr / count;
    }
    float total = t_nll;
    if (P.lr_on) total = total + t_lr * P.wl;
    if (P.rgb_on) total = total + t_rgb * P.wr;
    P.terms[0] = t_nll;
    P.terms[1] = t_lr;
    P.terms[2] = t_rgb;
    P.terms[3] = total;
    P.terms[4] = bad;
    P.scal[SC_CN] = cn;
    P.scal[SC_GX] = gx;
    P.scal[SC_GY] = gy;
    P.scal[SC_RGB] = grgb;
}

// d total / d p[i][k] of the label regularisation: 2 d w / sum(w) for each of
// the (up to four) differences the pixel is part of
struct LrTaps { float wl, wr, wu, wd; };

__global__ void __launch_bounds__(kT) k_ml_grad(Params P) {
    const uint32_t i = blockIdx.x * kT + threadIdx.x;
    if (i >= P.N) return;
    const uint32_t K = P.K;
    const float* p = P.p + (size_t)i * K;
    float* out = P.grad + (size_t)i * K;
    // NLL: -(1 / q_g) / n on the label's p, where the clamp does not bind
    int gl = -1;
    float g_nll = 0.0f;
    if (i < P.n) {
        const float q = P.q[i];
        if (q > 0.0f) {
            gl = (int)P.labels[i];                      // in [0, K): q > 0 only for a valid label
            g_nll = -P.scal[SC_CN] / q;
        }
    }
    LrTaps w{0.0f, 0.0f, 0.0f, 0.0f};
    const uint32_t S = P.P;
    if (P.lr_on) {
        const uint32_t in = i % (S * S), x = in % S, y = in / S;
        const float d0 = P.depth[i], gx = 2.0f * P.scal[SC_GX], gy = 2.0f * P.scal[SC_GY];
        if (x > 0) { const float dd = d0 - P.depth[i - 1]; w.wl = gx * expf(-(dd * dd)); }
        if (x + 1 < S) { const float dd = P.depth[i + 1] - d0; w.wr = gx * expf(-(dd * dd)); }
        if (y > 0) { const float dd = d0 - P.depth[i - S]; w.wu = gy * expf(-(dd * dd)); }
        if (y + 1 < S) { const float dd = P.depth[i + S] - d0; w.wd = gy * expf(-(dd * dd)); }
    }
    const float* grow = (P.rgb_on && i >= P.n) ? P.gp_rgb + (size_t)(i - P.n) * K : nullptr;
    const float grgb = P.scal[SC_RGB];
    auto dp = [&](uint32_t k) -> float {
        float g = ((int)k == gl) ? g_nll : 0.0f;
        if (P.lr_on) {
            const float c = p[k];
            if (w.wl != 0.0f) g += w.wl * (c - p[(ptrdiff_t)k - (ptrdiff_t)K]);
            if (w.wr != 0.0f) g -= w.wr * (p[K + k] - c);
            if (w.wu != 0.0f) g += w.wu * (c - p[(ptrdiff_t)k - (ptrdiff_t)S * K]);
            if (w.wd != 0.0f) g -= w.wd * (p[(size_t)S * K + k] - c);
        }
        if (grow) g += grgb * grow[k];
        return g;
    };
    // through the softmax, in ATen's form: dz_k = fma(-p_k, sum_j g_j p_j, g_k p_k)
    float t[kMaxK], gp[kMaxK];
#pragma unroll
    for (uint32_t k = 0; k < kMaxK; ++k) t[k] = gp[k] = k < K ? dp(k) * p[k] : 0.0f;
    const float dot = tree_sum32(t);
#pragma unroll
    for (uint32_t k = 0; k < kMaxK; ++k)
        if (k < K) out[k] = __builtin_fmaf(-p[k], dot, gp[k]);
}

const char* validate(const samnerf_mask_loss_args* a) {
    if (!a) return "null args";
    if (a->K < 2 || a->K > kMaxK) return "K (n_inst + redundant_instance) must lie in [2, 32]";
    if (a->N == 0 || a->n == 0 || a->n > a->N) return "need 1 <= n <= N";
    if ((uint64_t)a->N * a->K > 0x7fffffffull) return "N * K must stay below 2^31";
    if (!a->labels) return "null labels";
    if (!(a->epsilon >= 0.0 && a->epsilon < 0.5)) return "epsilon must lie in [0, 0.5)";
    if (a->incoherent_weight < 1.0f && !a->incoherent) return "incoherent_weight < 1 needs the incoherent masks";
    if (a->error_map && (!a->error_cells || a->map_cells == 0 || a->map_cells > 0xffffffffull))
        return "error_map needs error_cells and 1 <= map_cells < 2^32";
    if (a->label_reg_weight > 0.0f) {
        if (a->P < 2) return "label regularisation needs P >= 2 (the reference divides 0 by 0 at P = 1)";
        if ((uint64_t)a->P * a->P > a->N || a->N % (a->P * a->P) != 0) return "N must be whole P x P patches";
        if (!a->depth) return "label regularisation needs depth";
    }
    if (a->rgb_weight > 0.0f) {
        if (a->L == 0 || a->Q == 0 || a->S == 0) return "the RGB-similarity term needs L, Q, S >= 1";
        if ((uint64_t)a->n + (uint64_t)a->L * a->Q != a->N) return "N must equal n + L * Q";
        if (a->Q > kMaxQ || a->Q * a->K > kMaxQK) return "a local patch must fit LDS: Q <= 1024, Q * K <= 8192";
        if (a->S > a->Q || a->S > kMaxS) return "S must not exceed min(Q, 256)";
        if (!a->image || !a->sample_index) return "the RGB-similarity term needs image and sample_index";
    }
    return nullptr;
}

}  // namespace

extern "C" size_t samnerf_mask_loss_workspace_size(const samnerf_mask_loss_args* args) {
    if (validate(args)) return 0;
    return layout(*args).words * 4;
}

extern "C" int samnerf_mask_loss(const samnerf_mask_loss_args* args, const float* logits, float* loss_terms,
                                 float* grad_logits, int64_t* pred_ids, void* ws, size_t ws_bytes,
                                 samnerf_stream_t stream) {
    if (const char* why = validate(args)) return fail(SAMNERF_EINVAL, "mask_loss: %s", why);
    if (!logits || !loss_terms || !grad_logits || !pred_ids)
        return fail(SAMNERF_EINVAL, "mask_loss: null logits / loss_terms / grad_logits / pred_ids");
    const samnerf_mask_loss_args& a = *args;
    const Layout l = layout(a);
    if (!ws || ws_bytes < l.words * 4)
        return fail(SAMNERF_EWORKSPACE, "mask_loss: workspace of %zu bytes, %zu needed", ws ? ws_bytes : (size_t)0,
                    l.words * 4);
    float* w = static_cast<float*>(ws);
    Params P{};
    P.N = a.N; P.K = a.K; P.n = a.n; P.L = a.L; P.Q = a.Q; P.S = a.S; P.P = a.P;
    P.redundant = a.redundant != 0;
    P.logistics = a.use_pred_logistics != 0;
    P.reweight = a.incoherent_weight < 1.0f;
    P.ema = a.error_map != nullptr;
    P.lr_on = a.label_reg_weight > 0.0f;
    P.rgb_on = a.rgb_weight > 0.0f;
    P.eps = (float)a.epsilon;
    P.one_m_eps = (float)(1.0 - a.epsilon);
    P.u = a.incoherent_weight; P.wl = a.label_reg_weight; P.wr = a.rgb_weight;
    P.thr = a.rgb_threshold; P.a = a.rgb_exp_weight;
    P.map_cells = a.map_cells;
    P.z = logits; P.labels = a.labels; P.incoherent = a.incoherent; P.map = a.error_map;
    P.cells = a.error_cells; P.depth = a.depth; P.image = a.image; P.samples = a.sample_index;
    P.p = w + l.p; P.gp_rgb = w + l.gp_rgb; P.nll = w + l.nll; P.q = w + l.q; P.err = w + l.err;
    P.old = w + l.old;
    P.win = reinterpret_cast<uint32_t*>(w + l.win);
    P.flags = reinterpret_cast<uint32_t*>(w + l.flags);
    P.lr = w + l.lr; P.rgb_part = w + l.rgb_part;
    P.rgb_bad = reinterpret_cast<uint32_t*>(w + l.rgb_bad);
    P.scal = w + l.scal;
    P.terms = loss_terms; P.grad = grad_logits; P.ids = pred_ids;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const uint32_t rows = div_up(a.N, kT), grows = div_up(a.n, kT);
    int rc;
    k_ml_rows<<<rows, kT, 0, s>>>(P);
    if ((rc = check_launch("mask_loss rows"))) return rc;
    if (P.ema) {
        for (int step = 0; step < 4; ++step) {
            k_ml_em<<<grows, kT, 0, s>>>(P, step);
            if ((rc = check_launch("mask_loss error map"))) return rc;
        }
    }
    if (P.lr_on) {
        k_ml_lr<<<rows, kT, 0, s>>>(P);
        if ((rc = check_launch("mask_loss label regularisation"))) return rc;
    }
    if (P.rgb_on) {
        const size_t lds = ((size_t)a.Q * a.K + (size_t)a.Q * 4 + (size_t)a.S * (kWaves + 3)) * 4;   // <= 56 KiB
        k_ml_rgb<<<a.L, kT, lds, s>>>(P);
        if ((rc = check_launch("mask_loss rgb similarity"))) return rc;
    }
    k_ml_reduce<<<1, kT, 0, s>>>(P);
    if ((rc = check_launch("mask_loss reduce"))) return rc;
    k_ml_grad<<<rows, kT, 0, s>>>(P);
    return check_launch("mask_loss grad");
}
