// prop_stages.hip -- the two proposal stages of the fused render (the map of
// the pipeline is in raymarch.hip): k_snf, k_prop_sigma, k_prop_pdf and their
// one host path (run_proposal_stages), which the render and the RGB training
// step share.
#include <cmath>
#include <cstdlib>

#include "philox.h"
#include "raymarch_device.h"
#include "render_args.h"
#include "samnerf_common.h"

using namespace samnerf;

namespace {

// MLP layer y = W x (torch layout W[out][in]), fma chain in input order.
template <int OUT, int IN, bool RELU>
__device__ __forceinline__ void dense(const float* __restrict__ W, const float* x, float* y) {
#pragma unroll
    for (int o = 0; o < OUT; ++o) {
        float a = 0.0f;
#pragma unroll
        for (int i = 0; i < IN; ++i) a = __builtin_fmaf(W[o * IN + i], x[i], a);
        y[o] = RELU ? fmaxf(a, 0.0f) : a;
    }
}

// The same layer with two output units per v_pk_fma_f32 (each lane of it is
// the scalar fma chain of dense(), so the bits are unchanged).
template <int OUT, int IN, bool RELU>
__device__ __forceinline__ void dense_pk(const float* __restrict__ W, const float* x, float* y) {
    static_assert(OUT % 2 == 0, "output pairs");
#pragma unroll
    for (int o = 0; o < OUT; o += 2) {
        f2v a = {0.0f, 0.0f};
#pragma unroll
        for (int i = 0; i < IN; ++i)
            a = __builtin_elementwise_fma(f2v{W[o * IN + i], W[(o + 1) * IN + i]}, f2v{x[i], x[i]}, a);
        y[o] = RELU ? fmaxf(a.x, 0.0f) : a.x;
        y[o + 1] = RELU ? fmaxf(a.y, 0.0f) : a.y;
    }
}

// Levels are issued in groups of GROUP (8 corner loads each) separated by a
// scheduling barrier, bounding the loads in flight (and their VGPRs) per lane.
template <int L, int C, bool REF, int GROUP = 4>
__device__ __forceinline__ void grid_features(const GridDesc<16>& g, float ux, float uy, float uz,
                                              float* feat) {
#pragma unroll
    for (int l = 0; l < L; ++l) {
        if constexpr (REF) lookup_level3_ref<C>(g.emb, g.lv[l], ux, uy, uz, feat + l * C);
        else lookup_level3<C>(g.emb, g.lv[l], ux, uy, uz, feat + l * C);
        if ((l + 1) % GROUP == 0 && l + 1 < L) __builtin_amdgcn_sched_barrier(0);
    }
}

struct PropArgs {
    const float* rays_o;
    const float* rays_d;
    const float* cnf;
    uint32_t N, n_cnf;
    RayTiles tiles;        // slot -> ray (rays_o / rays_d / cnf are in ray order)
    float aabb[6];
    float min_near;
    GridScale gs;
    GridDesc<16> grid;
    const float* W0;       // [16, 10]
    const float* W1;       // [1, 16]
    Lin bins0;             // stage 0: linspace(0, 1, T+1)
    Lin u;                 // sample_pdf positions for the next stage
    // perturb=True (samnerf_model.perturb, ray order): the stage-0 bins [N][T+1]
    // and sample_pdf's u [N][TN] as the reference computes them from
    // torch.rand_like; null: linspace (bins0 / u above)
    const float* pbins0;
    const float* pu;
    const float* bins_in;  // [T+1][N] (stages > 0)
    float* snf;            // [2][N] spacing(near), spacing(far)
    // [N][2] slot-ordered ray records {o.xyz, spacing(near)}, {d.xyz,
    // spacing(far)} (k_snf; null: not written).  The proposal sigma kernels
    // read a sample's ray in two coalesced 16-B loads from its slot, instead of
    // mapping slot -> ray (RayTiles) and gathering rays_o / rays_d / snf in
    // four loads of 64-bit addresses: the proposal stages are bound by vector
    // issue and the vector-memory address path.
    float4* rec;
    float* wtmp;           // [T][N]: ds per sample
    float* bins_out;       // [TN][N]
    int32_t* inds_out;     // [TN][N] searchsorted indices, or null (parity taps only)
    float* w_out;          // [T][N] composited weights, or null (parity taps only)
    uint32_t pdf_seq;      // diagnostic build, SAMNERF_PDF_SEQ=1: every ray on the sequential phase A
    // perturb=True drawn in the kernels (samnerf_model.perturb_device, philox.h):
    // read by the seeded kernel forms only (PHX), which take neither array above
    PerturbKey phx;
    // from samnerf_set_background: 1 under 'last_sample' (the last sample's
    // delta * sigma is +inf, renderer.py:314), 0 under the transparent modes (it
    // composites like any other); wave-uniform, read once before the
    // compositing loops
    uint32_t last_inf;
};

// Bin i of a stage's input for slot r (ray `ray`): stage 0 linspace(0, 1, T+1)
// or its perturbed copy (renderer.py:264-271), later stages the previous
// stage's resampled bins (slot-major workspace).  PHX: the seeded form, stage
// 0's perturbed bin i of the ray from one generator call.
template <int T, bool FIRST, bool PHX = false>
__device__ __forceinline__ float stage_bin(const PropArgs& a, int i, uint32_t r, uint32_t ray) {
    if constexpr (FIRST && PHX) return perturb_bin0(a.bins0(i), perturb_word(a.phx, 0u, ray, (uint32_t)i), T);
    else if constexpr (FIRST) return a.pbins0 ? a.pbins0[(size_t)ray * (T + 1) + i] : a.bins0(i);
    else return a.bins_in[(size_t)i * a.N + r];
}

// A ray's values of one stage read in (mostly) ascending order: the quad last
// drawn is kept, so a walk over the values costs one generator call per four.
struct QuadCache {
    uint32_t q = 0xFFFFFFFFu;
    Philox4 v;
};
__device__ __forceinline__ uint32_t cached_word(QuadCache& c, const PerturbKey& key, uint32_t stage,
                                                uint32_t ray, uint32_t i) {
    if ((i >> 2) != c.q) {
        c.q = i >> 2;
        c.v = perturb_quad(key, stage, ray, c.q);
    }
    return philox_word(c.v, i & 3u);
}

// Proposal stage, part 1: one thread per (ray, sample).  A wave is 64
// neighbouring rays at one sample index (their corner gathers share cache
// lines) and a block is 4 consecutive sample indices of those rays.  XCD x
// (blocks b with b % 8 == x) owns a contiguous band of ray groups, all T/4
// sample groups of each, so they share its L2.  Writes ds_k =
// (real_bin_{k+1} - real_bin_k) * trunc_exp(density) (renderer.py:282-300)
// to wtmp[k][r]; the serial part of compositing is in k_prop_pdf.
template <int T>
constexpr uint32_t prop_sigma_blocks(uint32_t N) {
    return xcd_blocks((N + 63u) / 64u) * (T / 4);
}

//
// LOOK = kLookPacked / kLookRef: direct corner gathers (lookup_level3 /
// lookup_level3_ref).  A form with wave_box.h's de-duplicated gathers (each
// level's box staged once per wave in LDS) gave the same bits and measured
// 0.88 vs 0.83 ms (retired forms).
//
// KD / KH (round 5): the proposal grid's level classes as compile-time
// masks (bit l: level l dense / hashed; the reference's proposal grids,
// network.py:96-104 at the default sizes, are DDDHH and DDHHH), with a
// power-of-two grid scale.  The run-time form (KD = KH = 0) takes each
// level's dense / hashed branch on a uniform flag, and the branches split the
// levels into separate blocks: each level's loads were issued and waited for
// before the next level's (5 memory round trips per sample).  With the
// classes known the 5 levels' 28 loads issue together, then the weighted
// corner sums (gather_issue_c2 / gather_finish_c2, the k_final lookups: the
// same rows, weights and FMA order as lookup_level3, so the same bits).
template <uint32_t KD, uint32_t KH>
__device__ __forceinline__ void prop_lookup_lay(const PropArgs& a, float x, float y, float z, float* feat);

#ifndef SAMNERF_PROP_WAVES
#define SAMNERF_PROP_WAVES 0
#endif
// PHX: the seeded form (samnerf_model.perturb_device), stage 0's bins drawn
// here.  A compile-time switch, last and defaulted: the instantiations of
// perturb=False and of the array form keep their device code.
template <int T, bool FIRST, int LOOK, uint32_t KD = 0, uint32_t KH = 0, bool PHX = false>
__global__ void __launch_bounds__(256)
#if SAMNERF_PROP_WAVES
__attribute__((amdgpu_waves_per_eu(SAMNERF_PROP_WAVES, SAMNERF_PROP_WAVES)))
#endif
k_prop_sigma(PropArgs a) {
    static_assert(T % 4 == 0, "T must be a multiple of 4");
    static_assert(FIRST || !PHX, "only stage 0's bins are drawn");
    constexpr uint32_t Q = T / 4;
    const uint32_t b = blockIdx.x, i = b >> 3;
    const uint32_t q = i % Q, g = (b & 7u) * xcd_per((a.N + 63u) / 64u) + i / Q;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t r0 = g * 64u + lane, k = q * 4u + (threadIdx.x >> 6);
    if (g * 64u >= a.N) return;                     // whole wave past the end
    if (r0 >= a.N) return;
    const uint32_t r = r0;                                // slot
    const uint32_t N = a.N;
    // the LAY forms read k_snf's slot-ordered ray record (the ray id is then
    // needed only for perturb's per-ray bins); the others map slot -> ray
    constexpr bool REC = (KD | KH) == 0x1Fu && LOOK == kLookPacked;
    float o[3], d[3], sn, sf;
    if constexpr (REC) {
        const char* rbase = reinterpret_cast<const char*>(a.rec);     // 32-bit offsets: saddr loads
        const float4 ra = *reinterpret_cast<const float4*>(rbase + r * 32u),
                     rb = *reinterpret_cast<const float4*>(rbase + r * 32u + 16u);
        o[0] = ra.x, o[1] = ra.y, o[2] = ra.z, sn = ra.w;
        d[0] = rb.x, d[1] = rb.y, d[2] = rb.z, sf = rb.w;
    } else {
        const uint32_t ray = a.tiles(r);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            o[c] = a.rays_o[(size_t)ray * 3 + c];
            d[c] = a.rays_d[(size_t)ray * 3 + c];
        }
        sn = a.snf[r], sf = a.snf[N + r];                   // k_snf (stage 0) / stage 0 (stage 1)
    }
    float b0, b1;
    if constexpr (PHX) {
        // the wave's sample index is uniform: bins k and k + 1 are words k & 3
        // and (k & 3) + 1 of one quad of the ray -- one generator call -- except
        // in the block's last wave, whose bin k + 1 is word 0 of the next quad
        const uint32_t ku = __builtin_amdgcn_readfirstlane(k), w = ku & 3u, ray = a.tiles(r);
        const Philox4 qa = perturb_quad(a.phx, 0u, ray, ku >> 2);
        uint32_t w1;
        if (w == 3u) w1 = perturb_quad(a.phx, 0u, ray, (ku >> 2) + 1u).v[0];
        else w1 = philox_word(qa, w + 1u);
        b0 = perturb_bin0(a.bins0((int)ku), philox_word(qa, w), T);
        b1 = perturb_bin0(a.bins0((int)ku + 1), w1, T);
    } else {
        // the ray id: only perturb's per-ray bins need it (FIRST)
        const uint32_t pray = (FIRST && a.pbins0) ? a.tiles(r) : 0u;
        b0 = stage_bin<T, FIRST>(a, (int)k, r, pray), b1 = stage_bin<T, FIRST>(a, (int)k + 1, r, pray);
    }
    const float rb_prev = real_bin(sn, sf, b0), rb_next = real_bin(sn, sf, b1);
    const float t = (rb_next + rb_prev) / 2.0f;
    float x = o[0] + d[0] * t, y = o[1] + d[1] * t, z = o[2] + d[2] * t;
    contract3(x, y, z);
    float feat[10];
    if constexpr ((KD | KH) == 0x1Fu && LOOK == kLookPacked) {
        prop_lookup_lay<KD, KH>(a, x, y, z, feat);
    } else {
        grid_features<5, 2, LOOK == kLookRef>(a.grid, a.gs(x), a.gs(y), a.gs(z), feat);
    }
    float h[16], sv;
    if constexpr (LOOK == kLookRef) dense<16, 10, true>(a.W0, feat, h);
    else dense_pk<16, 10, true>(a.W0, feat, h);
    dense<1, 16, false>(a.W1, h, &sv);
    // the only store, after the weight reads: an earlier store could alias
    // W0/W1 and would demote the uniform weight reads to per-lane vector loads
    a.wtmp[(size_t)k * N + r] = (rb_next - rb_prev) * expf(sv);          // trunc_exp forward
}

// Stage 0 ray setup, one thread per ray: near/far from the AABB slab test
// (renderer.py:122-139, 229-236) and their spacing (renderer.py:250-253).
__global__ void __launch_bounds__(256) k_snf(PropArgs a) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;  // slot
    if (r >= a.N) return;
    const uint32_t ray = a.tiles(r);
    float o[3], d[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        o[c] = a.rays_o[(size_t)ray * 3 + c];
        d[c] = a.rays_d[(size_t)ray * 3 + c];
    }
    float near, far;
    near_far_aabb(o, d, a.aabb, a.min_near, near, far);
    if (a.cnf) {  // renderer.py:234-236
        const uint32_t q = a.n_cnf == 1 ? 0u : ray;
        const float cn = a.cnf[q * 2], cf = a.cnf[q * 2 + 1];
        near = (isnan(near) || isnan(cn)) ? NAN : fmaxf(near, cn);
        far = (isnan(far) || isnan(cf)) ? NAN : fminf(far, cf);
    }
    const float sn = spacing(near), sf = spacing(far);
    a.snf[r] = sn;
    a.snf[a.N + r] = sf;
    if (a.rec) {
        a.rec[2 * (size_t)r] = make_float4(o[0], o[1], o[2], sn);
        a.rec[2 * (size_t)r + 1] = make_float4(d[0], d[1], d[2], sf);
    }
}

// Proposal stage, part 2 (renderer.py:84-119 and 300-307), 64 rays per block.
// Phase A, one thread per ray, in the reference's sequential order: composite
// weights with the double cumulative sum, the torch-ordered pdf normaliser,
// and cdf[i] = min(float(double cumsum of (w + 0.01) / sum), 1), written in
// place over the ray's LDS row.  Phase B, 4 threads per ray: each takes a
// contiguous quarter of the TN outputs, finds its first searchsorted(right)
// position by binary search, and merge-walks its quarter -- the same cdf
// values and the same interpolation as one walk over the whole ray, so the
// indices and bins are identical, with a quarter of the dependent steps.
template <int T, int TN, bool FIRST, bool PHX>
__device__ __forceinline__ void prop_pdf_phases(const PropArgs& a, float* sw, uint32_t r0, uint32_t nr);
#ifndef SAMNERF_PDF_SPLIT
#define SAMNERF_PDF_SPLIT 1                  // phase A split over the block's 4 waves (below)
#endif
#ifndef SAMNERF_PDF_SPLIT_MIN
#define SAMNERF_PDF_SPLIT_MIN 128            // from this many samples per ray
#endif

// PHX: the seeded form (as k_prop_sigma's): sample_pdf's u, and stage 0's bins
// where FIRST, drawn here.
template <int T, int TN, bool FIRST, bool PHX = false>
__global__ void __launch_bounds__(256)
// T = 128: 4 waves per SIMD, the 4 blocks per CU the ds rows' LDS allows
// (the split phase A otherwise takes 146 VGPRs, 3 waves)
__attribute__((amdgpu_waves_per_eu(T >= 128 ? 4 : 1, T >= 128 ? 4 : 8)))
k_prop_pdf(PropArgs a) {
    constexpr int SW = T + 1;                 // T + 1 cdf entries per row (odd stride)
    __shared__ float sw[64 * SW];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, part = tid >> 6;
    const uint32_t r0 = xcd_chunk(blockIdx.x, (a.N + 63u) / 64u) * 64u, N = a.N;
    if (r0 >= N) return;
    const uint32_t nr = min(64u, N - r0);
    float* row = sw + lane * SW;
    // All four waves stage the ds rows (sample-major wtmp, coalesced across
    // the wave): T/4 independent loads per thread in flight at once, instead
    // of one thread per ray loading its whole row in dependent batches.
    // (Staging the input bins of stage > 0 as well doubles the LDS of
    // k_prop_pdf<64> and halves its occupancy: measured slower.  32 rays per
    // block -- twice the resident phase-A waves -- measured no faster: 0.593
    // -> 0.611 ms prop0 at a full view, 0.103 -> 0.101 ms at 32K rays.)
    if (lane < nr) {
        constexpr int TQ = T / 4;
        float v[TQ];
#pragma unroll
        for (int k = 0; k < TQ; ++k) v[k] = a.wtmp[(size_t)(part * TQ + k) * N + r0 + lane];
#pragma unroll
        for (int k = 0; k < TQ; ++k) row[part * TQ + k] = v[k];
    }
    __syncthreads();
    prop_pdf_phases<T, TN, FIRST, PHX>(a, sw, r0, nr);
}

// Exact-sum window of a run of float terms (phase A's double cumulative
// sums): the exponent fields of its non-zero terms and whether any term is
// subnormal, infinite or NaN.  When every term is normal or zero and the
// exponents of the largest and smallest non-zero term differ by at most 22,
// every partial sum of up to 128 of them is a multiple of the smallest
// term's ulp below 2^(e_max + 8), i.e. exactly representable in double
// (53 bits): then each partial sum is the exact real sum, whatever order it
// was formed in, and a prefix taken as (sum of the earlier quarters) + (this
// quarter's terms in order) is bit for bit the sequential prefix.
struct SumWindow {
    uint32_t emin = 0xFFu, emax = 0u, bad = 0u;
    __device__ __forceinline__ void add(float v) {
        const uint32_t e = (__float_as_uint(v) >> 23) & 0xFFu;
        const bool nz = (__float_as_uint(v) & 0x7FFFFFFFu) != 0u;
        bad |= (nz && (e == 0u || e == 0xFFu)) ? 1u : 0u;
        emin = nz ? min(emin, e) : emin;
        emax = nz ? max(emax, e) : emax;
    }
    __device__ __forceinline__ uint32_t pack() const { return bad << 16 | emax << 8 | emin; }
};
__device__ __forceinline__ bool sum_window_exact(const uint32_t* w4) {
    uint32_t emin = 0xFFu, emax = 0u, bad = 0u;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        emin = min(emin, w4[p] & 0xFFu);
        emax = max(emax, (w4[p] >> 8) & 0xFFu);
        bad |= w4[p] >> 16;
    }
    return bad == 0u && (emax < emin || emax - emin <= 22u);
}

// Phases A and B of the proposal pdf over 64 rays whose ds rows sit in LDS
// (row stride T + 1); every thread of the block calls it after a barrier.
//
// Phase A (SAMNERF_PDF_SPLIT, round 6): the four waves of the block take a
// quarter of each ray's samples.  The reference's two serial chains -- the
// double cumulative sum of ds behind the transmittance, and the double
// cumulative sum of the pdf behind the cdf -- are prefix sums: each wave sums
// its quarter in order, the quarter sums meet in LDS, and each wave runs its
// quarter from the sum of the quarters before it.  That is the sequential
// result bit for bit when the ray's terms pass the exact-sum window
// (SumWindow), checked per ray at run time; a ray that does not (ds spanning
// more than 2^22, or non-finite) takes the whole sequential chain in wave 0
// as before.  The pdf terms (w + 0.01) / sum with w in [0, 1] always pass.
// One serial chain of 128 steps per ray, one wave per SIMD at the LDS-bound
// occupancy, was the latency that bounded k_prop_pdf.
template <int T, int TN, bool FIRST, bool PHX>
__device__ __forceinline__ void prop_pdf_phases(const PropArgs& a, float* sw, uint32_t r0, uint32_t nr) {
    constexpr int SW = T + 1;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, part = tid >> 6, N = a.N;
    float* row = sw + lane * SW;
    // stage 0 only: at T = 64 the split's barriers and registers cost more
    // than the 64-step chains it shortens (prop1 0.304-0.308 against
    // 0.299-0.303 ms sequential; prop0 0.552-0.560 against 0.580-0.588)
    constexpr bool kSplit = SAMNERF_PDF_SPLIT && T >= SAMNERF_PDF_SPLIT_MIN;
    if constexpr (kSplit) {
    constexpr int Q = T / 4;
    __shared__ double qsum[4][64];            // per quarter and ray: the quarter's double sum
    __shared__ uint32_t qwin[4][64];          // and its SumWindow
    const bool rl = lane < nr;
    const int k0 = (int)part * Q;
    const int k_inf = a.last_inf ? T - 1 : -1;            // the sample whose ds is +inf (uniform)
    // A1: ds quarter sums.  The last sample's ds is never part of the window
    // or of a quarter sum, in either background mode: 'last_sample' replaces
    // it by +inf, the transparent modes composite it as it is, and in both it
    // only enters the sample's own alpha -- the running sum is read before
    // each sample (composite_step), so the sum after the last one is never
    // read and the exact-sum argument covers the same T - 1 terms
    {
        SumWindow win;
        double q = 0.0;
        if (rl) {
#pragma unroll 8
            for (int k = k0; k < k0 + Q; ++k) {
                if (k == T - 1) break;
                const float ds = row[k];
                win.add(ds);
                q += (double)ds;
            }
        }
        qsum[part][lane] = q;
        qwin[part][lane] = win.pack();
    }
    __syncthreads();
    // A2: composite.  Exact rays: each wave its quarter from the earlier
    // quarters' sum; the others: wave 0 the whole ray, in order.
    if (rl) {
        const uint32_t w4[4] = {qwin[0][lane], qwin[1][lane], qwin[2][lane], qwin[3][lane]};
        if (!a.pdf_seq && sum_window_exact(w4)) {
            double cum = 0.0;
            for (int p = 0; p < (int)part; ++p) cum += qsum[p][lane];
#pragma unroll 8
            for (int k = k0; k < k0 + Q; ++k) row[k] = composite_step(row[k], cum, k == k_inf);
        } else if (part == 0) {
            double cum = 0.0;
#pragma unroll 8
            for (int k = 0; k < T; ++k) row[k] = composite_step(row[k], cum, k == k_inf);
        }
    }
    __syncthreads();
    // A3: the weights out (taps) and the torch-ordered normaliser (each wave
    // for itself, over all T weights), then -- after a barrier, so no wave
    // still reads weights -- each wave replaces its quarter's weights by their
    // pdf (w + 0.01) / sum in place and forms the quarter's double sum
    float wsum = 0.0f;
    if (rl) {
        if (a.w_out)
            for (int k = k0; k < k0 + Q; ++k) a.w_out[(size_t)k * N + r0 + lane] = row[k];
        wsum = torch_row_sum(T, [&](int i) { return row[i] + 0.01f; });
    }
    __syncthreads();
    float pfirst = 0.0f;                      // this quarter's first pdf (A4 reads it from here)
    {
        SumWindow win;
        double q = 0.0;
        if (rl) {
#pragma unroll 8
            for (int k = k0; k < k0 + Q; ++k) {
                const float pdf = (row[k] + 0.01f) / wsum;
                row[k] = pdf;
                win.add(pdf);
                q += (double)pdf;
            }
            pfirst = row[k0];
        }
        qsum[part][lane] = q;
        qwin[part][lane] = win.pack();
    }
    __syncthreads();
    // A4: cdf[i + 1] = min(float(double cumsum of pdf), 1) in place: wave p
    // writes entries k0 + 1 .. k0 + Q, of which only k0 + Q is a pdf another
    // wave reads -- the next wave's first, which it holds in pfirst
    if (rl) {
        const uint32_t w4[4] = {qwin[0][lane], qwin[1][lane], qwin[2][lane], qwin[3][lane]};
        if (!a.pdf_seq && sum_window_exact(w4)) {
            double c = 0.0;
            for (int p = 0; p < (int)part; ++p) c += qsum[p][lane];
            if (part == 0) row[0] = 0.0f;
            float pnext = pfirst;
#pragma unroll 8
            for (int i = 0; i < Q; ++i) {
                const float pi = pnext;
                if (i + 1 < Q) pnext = row[k0 + i + 1];
                c += (double)pi;
                row[k0 + i + 1] = fminf((float)c, 1.0f);
            }
        } else if (part == 0) {
            // not exact (a NaN pdf): wave 0 the whole chain in order, the
            // other waves write nothing of this ray (every pdf is in LDS:
            // no wave wrote a cdf entry of it)
            double c = 0.0;
            float pnext = row[0];
            row[0] = 0.0f;
            for (int i = 0; i < T; ++i) {
                const float pi = pnext;
                if (i + 1 < T) pnext = row[i + 1];
                c += (double)pi;
                row[i + 1] = fminf((float)c, 1.0f);
            }
        }
    }
    } else {
    if (part == 0 && lane < nr) {
        // unrolled by 8: the LDS reads run ahead of the double-precision
        // chains (a full unroll takes 248 VGPRs and halves occupancy)
        double cum = 0.0;
        const int k_inf = a.last_inf ? T - 1 : -1;
#pragma unroll 8
        for (int k = 0; k < T; ++k) row[k] = composite_step(row[k], cum, k == k_inf);
        if (a.w_out)
            for (int k = 0; k < T; ++k) a.w_out[(size_t)k * N + r0 + lane] = row[k];
        const float wsum = torch_row_sum(T, [&](int i) { return row[i] + 0.01f; });
        double c = 0.0;
        float wnext = row[0];
        row[0] = 0.0f;
#pragma unroll 8
        for (int i = 0; i < T; ++i) {
            const float wi = wnext;
            if (i + 1 < T) wnext = row[i + 1];
            const float pdf = (wi + 0.01f) / wsum;
            c += (double)pdf;
            row[i + 1] = fminf((float)c, 1.0f);
        }
    }
    }
    __syncthreads();
    if (lane >= nr) return;
    const uint32_t r = r0 + lane, ray = a.tiles(r);
    auto bin = [&](int i) -> float { return stage_bin<T, FIRST>(a, i, r, ray); };
    // u_j: linspace, or the perturbed positions (nondecreasing up to rounding:
    // u_j < (j+1)/TN <= u_{j+1} before it, hence the backward step below)
    const float* pu = (!PHX && a.pu) ? a.pu + (size_t)ray * TN : nullptr;
    const bool perturbed = PHX || pu;
    // seeded: the lane walks u_j and (stage 0) the bins around its cdf position
    // in order, so each keeps the quad it last drew (QuadCache): a call per four
    // u_j, and per quad of bins the walk enters (below and above share theirs
    // three times in four)
    QuadCache cu, cb, ca;
    auto uj = [&](int j) -> float {
        if constexpr (PHX) return perturb_u(a.u(j), cached_word(cu, a.phx, FIRST ? 1u : 2u, ray, (uint32_t)j), TN);
        else return pu ? pu[j] : a.u(j);
    };
    constexpr int QN = TN / 4;
    const int j0 = (int)part * QN, j1 = part == 3 ? TN : j0 + QN;
    // first index with cdf > u_j0 (cdf is nondecreasing, cdf[0] = 0 <= u)
    const float u0 = uj(j0);
    int lo = 1, hi = T + 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (row[mid] <= u0) lo = mid + 1;
        else hi = mid;
    }
    int i = lo;
    for (int j = j0; j < j1; ++j) {
        const float u = uj(j);
        if (perturbed)
            while (i > 1 && row[i - 1] > u) --i;
        while (i <= T && row[i] <= u) ++i;
        const int below = i - 1, above = i <= T ? i : T;
        const float g0 = row[below], g1 = row[above];
        float b0, b1;
        if constexpr (FIRST && PHX) {
            const uint32_t wb = cached_word(cb, a.phx, 0u, ray, (uint32_t)below);
            const uint32_t wa = ((uint32_t)above >> 2) == cb.q ? philox_word(cb.v, (uint32_t)above & 3u)
                                                               : cached_word(ca, a.phx, 0u, ray, (uint32_t)above);
            b0 = perturb_bin0(a.bins0(below), wb, T);
            b1 = perturb_bin0(a.bins0(above), wa, T);
        } else {
            b0 = bin(below), b1 = bin(above);
        }
        float t = nan_to_num((u - g0) / (g1 - g0));
        t = fminf(fmaxf(t, 0.0f), 1.0f);
        a.bins_out[(size_t)j * N + r] = b0 + t * (b1 - b0);
        if (a.inds_out) a.inds_out[(size_t)j * N + r] = i;    // torch.searchsorted(cdf, u, right=True)
    }
}

// k_prop_sigma's lookup with compile-time level classes (KD / KH): the 5
// levels' loads issued together, then the packed corner sums.
// Uniform cells (round 5): a dense level whose cell is the same for all the
// wave's lanes (the coarse proposal levels: 64 neighbouring rays at one
// sample) reads its 4 corner pairs once through the scalar cache instead of
// 4 vector gathers -- the proposal stages are bound by the vector-memory
// address path.  Same rows, weights and FMA order (same bits).  The form
// without it (all 5 levels by vector gathers; a build switch through round 6)
// measured slower: prop0 0.605 -> 0.582, prop1 0.33 -> 0.297 ms,
// profiles/r5h_prop_forms_ab.txt.
// PROP_TWO (round 5, late; removed in round 6): a dense level whose lanes sit
// in two cells read both cells' corner pairs through the scalar cache and
// took each lane's by v_cndmask -- bit-identical but slower (prop0 0.575 ->
// 0.62 ms, profiles/r5two_prop_two_cell_ab.txt): the second cell's scalar
// loads add latency the vector path hides.

// Round 6, the same rows, weights and FMA order (same
// bits), fewer VALU cycles per sample:
//  * hashed levels: the table base of the level (emb + 8 off) is a uniform
//    SGPR pair, and the per-axis hash terms are kept pre-shifted and
//    pre-masked in bytes -- X8 = 8 x, Y8 = (y P1 8) & M8, Z8 = (z P2 8) & M8
//    with M8 = 8 (size - 1), since AND distributes over XOR and the shift
//    commutes with both -- so a corner's byte offset 8 ((x ^ y P1 ^ z P2) &
//    (size - 1)) is ONE v_xor_b32 (2.2 cycles per wave64 instruction,
//    profiles/r5v_valu_rate.json) where v_bitop3 + v_add_lshl_u32 took 6.6
//    (the host admits the form only with res <= size, so X8 needs no mask);
//  * uniform dense levels: the corner sums read the scalar-loaded rows as
//    SGPR operands of the packed FMAs in their own branch.  The round-5 form
//    joined them with the vector path's rows before one shared sum, and the
//    join copied 16 SGPRs to VGPRs per level (v_mov_b32 at 4.1 cycles; the
//    compiler also merged the fourth corner pair into a vector load).
template <uint32_t KD, uint32_t KH>
__device__ __forceinline__ void prop_lookup_lay(const PropArgs& a, float x, float y, float z, float* feat) {
    const float ux = (x + a.gs.bound) * a.gs.inv_b2, uy = (y + a.gs.bound) * a.gs.inv_b2,
                uz = (z + a.gs.bound) * a.gs.inv_b2;
    const char* base = reinterpret_cast<const char*>(a.grid.emb);
    const uint64_t live = __builtin_amdgcn_read_exec();
    float fx[5], fy[5], fz[5];
    uint32_t row[5][8];
    bool uni[5];
#pragma unroll
    for (int l = 0; l < 5; ++l) {
        uni[l] = false;
        if ((KD >> l) & 1u) {
            const LevelDesc& d = a.grid.lv[l];
            uint32_t cx, cy, cz;
            locate_axis(ux, d, cx, fx[l]);
            locate_axis(uy, d, cy, fy[l]);
            locate_axis(uz, d, cz, fz[l]);
            const uint32_t top = d.res - 1u;
            const uint32_t ny = min(cy + 1u, top), nz = min(cz + 1u, top);
            // one cell for every live lane (wave-uniform: a ballot)
            const uint32_t c0 = __builtin_amdgcn_readfirstlane(cx), c1 = __builtin_amdgcn_readfirstlane(cy),
                           c2 = __builtin_amdgcn_readfirstlane(cz);
            const bool same0 = cx == c0 && cy == c1 && cz == c2;
            uni[l] = __builtin_amdgcn_ballot_w64(same0) == live;
            const bool edge = cx == top;                   // gather_issue_c2's top-cell pair
            fx[l] = edge ? 1.0f : fx[l];
            const uint32_t bx = d.off + (edge ? cx - 1u : cx);
            const uint32_t r2 = d.res * d.res;
            const uint32_t Y[2] = {(uint32_t)__umul24(cy, d.res), (uint32_t)__umul24(ny, d.res)};
            const uint32_t Z[2] = {(uint32_t)__umul24(cz, r2), (uint32_t)__umul24(nz, r2)};
#pragma unroll
            for (int p = 0; p < 4; ++p) row[l][p] = (bx + Y[p & 1] + Z[p >> 1]) << 3;
        }
    }
    // Dense levels first: the non-uniform ones' vector loads, then each
    // uniform level's rows by scalar loads and its sum straight from the SGPRs
    // (summed where the vector rows are, the compiler merged the two into one
    // sum of phi'd VGPRs: 8 v_mov_b64 per level), then the vector sums; then
    // the hashed levels' loads and sums.  (The hashed loads issued with the
    // dense ones -- one memory round trip, but 122-126 VGPRs, 4 waves per SIMD
    // instead of 6 -- measured slower, prop0 0.565 -> 0.58-0.59 ms,
    // profiles/r6b_prop_forms_ab.txt; a build switch through round 6.)
    f4a8 vd[5][4];
    float2 vh[5][8];
    auto issue_hashed = [&]() {
#pragma unroll
        for (int l = 0; l < 5; ++l) {
            if (!((KD >> l) & 1u)) {
                const LevelDesc& d = a.grid.lv[l];
                uint32_t cx, cy, cz;
                locate_axis(ux, d, cx, fx[l]);
                locate_axis(uy, d, cy, fy[l]);
                locate_axis(uz, d, cz, fz[l]);
                const uint32_t top = d.res - 1u;
                const uint32_t ny = min(cy + 1u, top), nz = min(cz + 1u, top);
                const uint32_t m8 = (d.size - 1u) << 3;
                const uint32_t X[2] = {cx << 3, (uint32_t)min(cx + 1u, top) << 3};
                const uint32_t Y[2] = {(cy * (kPrime1 << 3)) & m8, (ny * (kPrime1 << 3)) & m8};
                const uint32_t Z[2] = {(cz * (kPrime2 << 3)) & m8, (nz * (kPrime2 << 3)) & m8};
#pragma unroll
                for (int c = 0; c < 8; ++c) row[l][c] = X[c & 1] ^ Y[(c >> 1) & 1] ^ Z[c >> 2];
                const char* lb = base + (size_t)d.off * 8u;                // uniform: SGPR base
#pragma unroll
                for (int c = 0; c < 8; ++c) vh[l][c] = *reinterpret_cast<const float2*>(lb + row[l][c]);
            }
        }
    };
#pragma unroll
    for (int l = 0; l < 5; ++l) {
        if (((KD >> l) & 1u) && !uni[l]) {
#pragma unroll
            for (int p = 0; p < 4; ++p) vd[l][p] = *reinterpret_cast<const f4a8*>(base + row[l][p]);
        }
    }
    // corner pair p of a dense level holds corners 2p (x) and 2p + 1 (x + 1)
    auto dense_sum = [&](int l, const f4a8* v) {
        f2v w[4];
        corner_weights_pk(fx[l], fy[l], fz[l], w);
        f2v acc = {0.0f, 0.0f};
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const float w0 = corner_w(w, 2 * p), w1 = corner_w(w, 2 * p + 1);
            acc = __builtin_elementwise_fma(f2v{w0, w0}, f2v{v[p].x, v[p].y}, acc);
            acc = __builtin_elementwise_fma(f2v{w1, w1}, f2v{v[p].z, v[p].w}, acc);
        }
        return acc;
    };
    f2v fl[5];                 // per level (an array of 10 floats updated in branches became one
                               // phi'd aggregate: v_mov chains at every join)
#pragma unroll
    for (int l = 0; l < 5; ++l) {
        if (((KD >> l) & 1u) && uni[l]) {
            // the scalar cache: wave-uniform rows, through a constant-address-
            // space pointer (the compiler may not turn them into vector loads)
            f4a8 sd[4];
#pragma unroll
            for (int p = 0; p < 4; ++p)
                sd[p] = *(const __attribute__((address_space(4))) f4a8*)(
                    base + (uint32_t)__builtin_amdgcn_readfirstlane(row[l][p]));
            fl[l] = dense_sum(l, sd);
        }
    }
#pragma unroll
    for (int l = 0; l < 5; ++l)
        if (((KD >> l) & 1u) && !uni[l]) fl[l] = dense_sum(l, vd[l]);
    issue_hashed();
#pragma unroll
    for (int l = 0; l < 5; ++l) {
        if (!((KD >> l) & 1u)) {
            f2v w[4];
            corner_weights_pk(fx[l], fy[l], fz[l], w);
            f2v acc = {0.0f, 0.0f};
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const float wt = corner_w(w, c);
                acc = __builtin_elementwise_fma(f2v{wt, wt}, f2v{vh[l][c].x, vh[l][c].y}, acc);
            }
            fl[l] = acc;
        }
    }
#pragma unroll
    for (int l = 0; l < 5; ++l) {
        feat[2 * l] = fl[l].x;
        feat[2 * l + 1] = fl[l].y;
    }
}

// Proposal gather form: direct by default (packed / auto), the box form for
// SAMNERF_LOOKUP = box / box4.  The box form trades the kernel's 40 corner
// gathers for ~200 VALU instructions of range reduction, box staging and LDS
// addressing per sample; the direct form is only slightly TA-bound (704 TA
// vs 575 VALU cycles per wave) so the box form is slower, 0.88 vs 0.83 ms.
// Returns the compiled level classes launched (KD | KH << 8), 0 for a run-time
// form (samnerf_last_forms).
template <int T, bool FIRST, bool PHX>
uint32_t launch_prop_sigma(int look, uint32_t N, hipStream_t s, const PropArgs& pa) {
    const uint32_t nb = prop_sigma_blocks<T>(N);
    // the reference's proposal grids with a power-of-two grid scale: the
    // compile-time level classes (SAMNERF_PROP_LAY=0, diagnostic build: the
    // run-time form, for the bit-identity test)
    uint32_t kd = 0, kh = 0;
    for (int l = 0; l < 5; ++l) {
        kd |= (pa.grid.lv[l].flags & kHashed) ? 0u : 1u << l;
        kh |= (pa.grid.lv[l].flags & kHashed) ? 1u << l : 0u;
    }
    const char* pl = diag_env("SAMNERF_PROP_LAY");
    // the LAY forms' byte-offset hash terms need res <= size on hashed levels
    bool small_res = true;
    for (int l = 0; l < 5; ++l)
        if ((pa.grid.lv[l].flags & kHashed) && pa.grid.lv[l].res > pa.grid.lv[l].size) small_res = false;
    const bool lay = (look == kLookPacked || look == kLookAuto) && pa.gs.inv_b2 != 0.0f &&
                     !(pl && atoi(pl) == 0) && small_res && pa.rec;
    if (lay && kd == 0x07u && kh == 0x18u) {
        k_prop_sigma<T, FIRST, kLookPacked, 0x07u, 0x18u, PHX><<<nb, 256, 0, s>>>(pa);
        return kd | kh << 8;
    }
    if (lay && kd == 0x03u && kh == 0x1Cu) {
        k_prop_sigma<T, FIRST, kLookPacked, 0x03u, 0x1Cu, PHX><<<nb, 256, 0, s>>>(pa);
        return kd | kh << 8;
    }
    if (look == kLookRef) k_prop_sigma<T, FIRST, kLookRef, 0u, 0u, PHX><<<nb, 256, 0, s>>>(pa);
    else k_prop_sigma<T, FIRST, kLookPacked, 0u, 0u, PHX><<<nb, 256, 0, s>>>(pa);
    return 0u;
}

// One proposal stage: ds per sample, then the pdf.  (One kernel for both, ds
// kept in LDS, gave the same bits 1.9x slower: prop0 1.10 vs 0.59 ms per view,
// DESIGN.md 5.)
// PHX: the seeded kernel forms (only stage 0's sigma kernel reads positions).
template <int T, int TN, bool FIRST, bool PHX>
void run_stage(const PropArgs& pa, int look, hipStream_t s, uint32_t& form) {
    form = launch_prop_sigma<T, FIRST, FIRST && PHX>(look, pa.N, s, pa);
    k_prop_pdf<T, TN, FIRST, PHX><<<xcd_blocks(div_up(pa.N, 64)), 256, 0, s>>>(pa);
}

void set_stage(PropArgs& pa, const samnerf_model* m, int i, const ProposalRun::Stage& st) {
    pa.grid = st.grid;
    pa.W0 = m->prop_mlp[i][0];
    pa.W1 = m->prop_mlp[i][1];
    pa.pu = m->perturb[i + 1];
    pa.bins_out = st.bins_out;
    pa.wtmp = st.ds;
    pa.inds_out = st.inds_out;
    pa.w_out = st.w_out;
}

}  // namespace

namespace samnerf {

void run_proposal_stages(const samnerf_model* m, uint32_t N, const ProposalRun& r, hipStream_t s,
                         uint32_t forms[2]) {
    PropArgs pa{};
    pa.rays_o = r.rays_o;
    pa.rays_d = r.rays_d;
    pa.cnf = r.cnf;
    pa.N = N;
    const char* ps = diag_env("SAMNERF_PDF_SEQ");
    pa.pdf_seq = ps && atoi(ps) != 0 ? 1u : 0u;
    pa.tiles = r.tiles;
    pa.n_cnf = r.n_cnf;
    for (int i = 0; i < 6; ++i) pa.aabb[i] = m->aabb[i];
    pa.min_near = m->min_near;
    pa.gs = make_grid_scale(m->grid_bound);
    pa.snf = r.snf;
    pa.rec = r.rec;
    pa.last_inf = current_background().background == 0 ? 1u : 0u;

    // stage 0: 128 uniform samples -> 65 bins (renderer.py:263-267, :274-275)
    set_stage(pa, m, 0, r.st[0]);
    pa.bins0 = make_lin(0.0f, 1.0f, 129);
    pa.u = make_lin((float)(0.5 / 65), (float)(1.0 - 0.5 / 65), 65);
    pa.pbins0 = m->perturb[0];
    if (r.mark) r.mark(0, s);
    // perturb_device: the seeded kernel forms (check_perturb: no arrays then)
    const bool phx = m->perturb_device != 0;
    pa.phx = make_perturb_key(m->perturb_seed, m->perturb_offset);
    k_snf<<<div_up(N, 256), 256, 0, s>>>(pa);
    if (phx) run_stage<128, 65, true, true>(pa, r.look, s, forms[0]);
    else run_stage<128, 65, true, false>(pa, r.look, s, forms[0]);

    // stage 1: 64 samples -> 33 bins
    set_stage(pa, m, 1, r.st[1]);
    pa.u = make_lin((float)(0.5 / 33), (float)(1.0 - 0.5 / 33), 33);
    pa.bins_in = r.st[0].bins_out;
    if (r.mark) r.mark(1, s);
    if (phx) run_stage<64, 33, false, true>(pa, r.look, s, forms[1]);
    else run_stage<64, 33, false, false>(pa, r.look, s, forms[1]);
}

// The proposal stages of a training render (rgb_train.hip): the same kernels
// as samnerf_render_forward's stages 0 and 1, ray order (no tiling), writing
// every intermediate the RGB backward reads to the caller's buffers.
int proposal_forward(const samnerf_model* m, const TrainGeometry& g, const float* rays_o,
                     const float* rays_d, uint32_t N, const float* cnf, uint32_t n_cnf,
                     const ProposalOut& o, hipStream_t s) {
    ProposalRun r{};
    r.rays_o = rays_o;
    r.rays_d = rays_d;
    r.cnf = cnf;
    r.n_cnf = n_cnf;
    r.tiles = RayTiles{0u, 0u, 32u};
    r.look = kLookPacked;                  // whatever SAMNERF_LOOKUP says
    r.snf = o.snf;
    r.rec = o.rec;
    r.st[0] = {g.prop[0], o.bins1, o.ds0, nullptr, o.w0};
    r.st[1] = {g.prop[1], o.bins2, o.ds1, nullptr, o.w1};
    uint32_t forms[2];
    run_proposal_stages(m, N, r, s, forms);
    return check_launch("proposal_forward");
}

}  // namespace samnerf
