// raymarch.hip -- the NeRF ray-march inner loop (nerf/renderer.py:221-390 +
// nerf/network.py:221-259) as fused gfx950 kernels: the render entry points
// and render_impl, which runs the stages, the workspace they share (carve),
// and the stand-alone step kernels used by the parity tests.
//
// Fused pipeline for N rays (all intermediates stay in one workspace; nothing
// of shape [N, T, C] is ever materialised, unlike the reference's ~350 ATen
// ops per chunk), and the file that holds each stage:
//   prop_stages.hip (run_proposal_stages)
//   k_prop_sigma<128>       one thread per (ray, sample): near/far + uniform
//                           bins + prop0 grid/MLP -> ds = delta * sigma
//   k_prop_pdf<128, 65>     per ray: compositing (double cumsum) + torch-
//                           ordered normaliser + cdf (one thread), inverse-CDF
//                           (four threads, quarter merge walks) -> 65 bins
//   k_prop_sigma/pdf<64,33> the same for prop1 -> 33 bins
//   final_stage.hip (run_final; the corner gathers in gather_c2.h)
//   k_final<32>             final samples: hash grid L16C2 + sigma/geo MLP +
//                           SH(4) + compositing + view MLP -> image, depth,
//                           weights_sum, head-input row; keeps (u_k, w_k)
//   sgrid.hip (launch_sgrid; also the s_grid backward)
//   k_sgrid<32>             s_grid L16C8 gather, weighted by w_k -> f_sam
//   sam_head.hip (sam_head_forward, heads.h)
//   sam_head                SkipConnMLP(163->256 x5) + LayerNorm on MFMA
// render_args.h holds what these files share.
// Rays are independent and every ray does the same work (fixed 128/64/32
// samples), so no compaction or load balancing is needed; the
// proposal gathers run one thread per sample (enough waves to hide gather
// latency even at the 32K rays of one rank of an 8-GPU view).
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "heads.h"
#include "raymarch_device.h"
#include "render_args.h"
#include "samnerf_common.h"

using namespace samnerf;

namespace {

// The shader clock over a stretch of the stream (samnerf_clock_stamp, the
// bench's timed views): workgroup b stamps its XCC id, s_memtime (one tick
// per shader cycle, MI355X_MICROARCH.md) and s_memrealtime (100 MHz).  The
// read-only counter instructions only (scalar reads; the stores are vector).
__global__ void __launch_bounds__(64) k_clock_stamp(unsigned long long* out) {
    const unsigned long long t = __builtin_amdgcn_s_memtime();
    const unsigned long long rt = __builtin_amdgcn_s_memrealtime();
    // XCC_ID: hwreg 20, bits [3:0] (gfx940+)
    const unsigned xcc = __builtin_amdgcn_s_getreg((20u) | (0u << 6) | ((4u - 1u) << 11));
    if (threadIdx.x == 0) {
        out[3 * blockIdx.x + 0] = xcc;
        out[3 * blockIdx.x + 1] = t;
        out[3 * blockIdx.x + 2] = rt;
    }
}

// ------------------------------------------------------- step kernels ----

__global__ void __launch_bounds__(256)
k_get_rays(float r00, float r01, float r02, float r10, float r11, float r12, float r20, float r21,
           float r22, float tx, float ty, float tz, float fx, float fy, float cx, float cy,
           uint32_t W, uint32_t row0, uint32_t n, float* __restrict__ rays_o,
           float* __restrict__ rays_d) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const uint32_t p = row0 * W + t;
    const float i = (float)(p % W) + 0.5f;   // linspace(0, W-1, W) holds exact integers
    const float j = (float)(p / W) + 0.5f;
    const float xs = (i - cx) / fx;
    const float ys = -((j - cy) / fy);
    const float zs = -1.0f;
    // directions @ R^T  (utils.py:255-256)
    // outputs hold only this band: local ray index t
    rays_d[(size_t)t * 3 + 0] = __builtin_fmaf(zs, r02, __builtin_fmaf(ys, r01, xs * r00));
    rays_d[(size_t)t * 3 + 1] = __builtin_fmaf(zs, r12, __builtin_fmaf(ys, r11, xs * r10));
    rays_d[(size_t)t * 3 + 2] = __builtin_fmaf(zs, r22, __builtin_fmaf(ys, r21, xs * r20));
    rays_o[(size_t)t * 3 + 0] = tx;
    rays_o[(size_t)t * 3 + 1] = ty;
    rays_o[(size_t)t * 3 + 2] = tz;
}

struct Aabb {
    float v[6];
};

__global__ void __launch_bounds__(256)
k_near_far(const float* __restrict__ o, const float* __restrict__ d, uint32_t N, Aabb box,
           float min_near, float* __restrict__ nears, float* __restrict__ fars) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= N) return;
    float oo[3] = {o[r * 3], o[r * 3 + 1], o[r * 3 + 2]};
    float dd[3] = {d[r * 3], d[r * 3 + 1], d[r * 3 + 2]};
    float n, f;
    near_far_aabb(oo, dd, box.v, min_near, n, f);
    nears[r] = n;
    fars[r] = f;
}

__global__ void __launch_bounds__(256)
k_contract(const float* __restrict__ x, float* __restrict__ z, uint32_t N) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= N) return;
    float a = x[r * 3], b = x[r * 3 + 1], c = x[r * 3 + 2];
    contract3(a, b, c);
    z[r * 3] = a;
    z[r * 3 + 1] = b;
    z[r * 3 + 2] = c;
}

__global__ void __launch_bounds__(256)
k_sample_pdf(const float* __restrict__ bins, const float* __restrict__ weights, uint32_t N,
             uint32_t T0, uint32_t T, Lin u, float* __restrict__ out, int32_t* __restrict__ inds) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= N) return;
    const float* w = weights + (size_t)r * T0;
    const float* b = bins + (size_t)r * (T0 + 1);
    const float wsum = torch_row_sum((int)T0, [&](int i) { return w[i] + 0.01f; });
    sample_pdf_walk(
        (int)T0, (int)T, u, wsum, [&](int i) { return w[i]; },
        [&](int i) { return b[i]; },
        [&](int j, float v, int ind) {
            out[(size_t)r * T + j] = v;
            if (inds) inds[(size_t)r * T + j] = ind;
        });
}

__global__ void __launch_bounds__(256)
k_composite(const float* __restrict__ rb, const float* __restrict__ sig, uint32_t N, uint32_t T,
            float* __restrict__ w) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= N) return;
    double cum = 0.0;
    for (uint32_t k = 0; k < T; ++k) {
        const float ds = (rb[(size_t)r * (T + 1) + k + 1] - rb[(size_t)r * (T + 1) + k]) *
                         sig[(size_t)r * T + k];
        w[(size_t)r * T + k] = composite_step(ds, cum, k == T - 1);
    }
}

}  // namespace


// ------------------------------------------------------------------ host --

namespace {


thread_local hipEvent_t g_stage_events[8];
thread_local uint32_t g_n_stage_events = 0;
thread_local samnerf_taps g_taps = {};
thread_local uint32_t g_taps_n = 0;
thread_local bool g_taps_on = false;
// the compiled forms the last render of this thread launched
// (samnerf_last_forms): [0] / [1] the proposal stages' level classes (KD |
// KH << 8, 0 for the run-time form), [2] k_final's layout (final_layout)
thread_local uint32_t g_last_forms[4] = {};

void mark_stage(uint32_t i, hipStream_t s) {
    if (i < g_n_stage_events && g_stage_events[i]) (void)hipEventRecord(g_stage_events[i], s);
}

// Parity taps: the final samples' weights and positions, which the render
// keeps in its workspace, copied out after the stages that read them.
int copy_final_taps(const samnerf_taps& tp, const Workspace& w, uint32_t N, hipStream_t s) {
    const size_t n = N;
    if (tp.w2 && hipMemcpyAsync(tp.w2, w.w_f, 32 * n * sizeof(float), hipMemcpyDeviceToDevice, s) != hipSuccess)
        return fail(SAMNERF_ELAUNCH, "render: copying the w2 tap failed");
    if (tp.u2 && hipMemcpyAsync(tp.u2, w.u_f, 96 * n * sizeof(float), hipMemcpyDeviceToDevice, s) != hipSuccess)
        return fail(SAMNERF_ELAUNCH, "render: copying the u2 tap failed");
    return SAMNERF_OK;
}

}  // namespace

namespace samnerf {

// Gather variants, for A/B measurement and the bit-identity tests:
// SAMNERF_LOOKUP = packed (default) | ref | box (k_sgrid only; the proposal
// stages use packed).  Read per call (getenv is cheap next to a launch).
int lookup_mode() {
    const char* v = diag_env("SAMNERF_LOOKUP");
    if (!v || !*v) return kLookAuto;
    if (!strcmp(v, "ref")) return kLookRef;
    if (!strcmp(v, "box")) return kLookBox4;
    if (!strcmp(v, "box4")) return kLookBox4;
    return kLookPacked;
}

// The per-render packing launches (grid_mlp fragments, the SAM head's weight
// stream) run unless the caller vouches that the workspace already holds this
// model's packed weights (samnerf_model::reuse_packed); the diagnostic build,
// whose kernel forms switch with the environment, always packs.
bool pack_weights(const samnerf_model* m) {
#ifdef SAMNERF_DIAG_VARIANTS
    return true;
#else
    return m->reuse_packed == 0;
#endif
}

// k_sgrid_box4 packs cell indices and extents into 10 bits
bool box4_ok(const GridDesc<16>& g) {
    for (int l = 0; l < 16; ++l)
        if (g.lv[l].res > 1023u) return false;
    return true;
}

Workspace carve(const samnerf_model* m, uint32_t N, void* base) {
    Workspace w;
    Carver c(base);
    const size_t n = N;
    // the packed weights first: their offsets do not depend on N, so a
    // render of another ray count on the same workspace finds them where
    // the packing render left them (samnerf_model::reuse_packed)
    w.gpack = c.take<uint4>((size_t)2 * kFSlots * 64 * 4);
    w.gexp = c.take<int>(4);
    w.packed = c.take(m->with_sam ? sam_head_packed_floats() : 0);
    w.snf = c.take(2 * n);
    w.rec = c.take<float4>(8 * n);
    w.bins1 = c.take((m->num_steps[1] + 1) * n);
    w.bins2 = c.take((m->num_steps[2] + 1) * n);
    w.wtmp = c.take((size_t)std::max(m->num_steps[0], m->num_steps[1]) * n);
    w.u_f = c.take(3 * (size_t)m->num_steps[2] * n);
    w.w_f = c.take((size_t)m->num_steps[2] * n);
    w.rows = c.take((size_t)kRow * n);
    const bool mdef = m->with_mask && m->mask_kind == 0, madapt = m->with_mask && m->mask_kind > 0;
    w.geo_f = c.take(mdef ? (size_t)16 * m->num_steps[2] * n : 0);
    w.mpacked = c.take(mdef ? mask_head_packed_floats() : 0);
    w.aeff = c.take(madapt ? (size_t)32 * kAeff : 0);
    w.mlog = c.take(madapt ? (size_t)m->mask_out * n : 0);
    w.xsum = c.take(madapt && m->with_mask == 2 ? (size_t)kAeff * n : 0);   // training renders only
    w.bytes = c.bytes();
    return w;
}

int make_grid_desc(const samnerf_grid& g, uint32_t C, uint32_t L, GridDesc<16>& d,
                   const char* name) {
    if (!g.embeddings || !g.offsets_host)
        return fail(SAMNERF_EINVAL, "render: %s has null embeddings/offsets", name);
    if (g.level_dim != C || g.num_levels != L)
        return fail(SAMNERF_EINVAL, "render: %s must be L%u C%u (got L%u C%u)", name, L, C,
                    g.num_levels, g.level_dim);
    const ResTable rt = make_res_table(L, g.S, g.base_resolution);
    d.emb = g.embeddings;
    for (uint32_t l = 0; l < 16; ++l) {
        if (l < L) {
            const uint32_t off = (uint32_t)g.offsets_host[l];
            const uint32_t size = (uint32_t)(g.offsets_host[l + 1] - g.offsets_host[l]);
            d.lv[l] = make_level(off, size, rt.res[l], 0u);
            const bool hashed = d.lv[l].flags & kHashed;
            if (!hashed && (uint64_t)rt.res[l] * rt.res[l] * rt.res[l] > size)
                return fail(SAMNERF_EINVAL, "render: %s level %u is neither dense nor hashed", name, l);
            if (hashed && (size & (size - 1u)))
                return fail(SAMNERF_EINVAL, "render: %s level %u hashes into a non power-of-two table",
                            name, l);
            if ((uint64_t)(off + size) * C * sizeof(float) > (1ull << 32))
                return fail(SAMNERF_EINVAL, "render: %s exceeds 4 GiB (32-bit gather offsets)", name);
        } else {
            d.lv[l] = LevelDesc{0, 1, 1, 0, 1.0f, 0.0f};
        }
    }
    return SAMNERF_OK;
}

int train_geometry(const samnerf_model* m, TrainGeometry& g) {
    int rc;
    GridDesc<16> d;
    if ((rc = make_grid_desc(m->grid, 2, 16, d, "grid"))) return rc;
    g.grid = d;
    for (int p = 0; p < 2; ++p) {
        if ((rc = make_grid_desc(m->prop[p], 2, 5, d, p ? "prop_encoders.1" : "prop_encoders.0")))
            return rc;
        g.prop[p] = d;
    }
    const GridScale gs = make_grid_scale(m->grid_bound);
    g.bound = gs.bound;
    g.b2 = gs.b2;
    g.inv_b2 = gs.inv_b2;
    return SAMNERF_OK;
}

}  // namespace samnerf

extern "C" {

int samnerf_get_rays(const float* pose, float fx, float fy, float cx, float cy, uint32_t H,
                     uint32_t W, uint32_t row0, uint32_t rows, float* rays_o, float* rays_d,
                     samnerf_stream_t stream) {
    if (!pose || !rays_o || !rays_d) return fail(SAMNERF_EINVAL, "get_rays: null pointer");
    if (row0 + rows > H) return fail(SAMNERF_EINVAL, "get_rays: rows out of range");
    const uint32_t n = rows * W;
    if (n == 0) return SAMNERF_OK;
    k_get_rays<<<div_up(n, 256), 256, 0, reinterpret_cast<hipStream_t>(stream)>>>(
        pose[0], pose[1], pose[2], pose[4], pose[5], pose[6], pose[8], pose[9], pose[10], pose[3],
        pose[7], pose[11], fx, fy, cx, cy, W, row0, n, rays_o, rays_d);
    return check_launch("get_rays");
}

int samnerf_near_far(const float* rays_o, const float* rays_d, uint32_t N, const float* aabb,
                     float min_near, float* nears, float* fars, samnerf_stream_t stream) {
    if (!rays_o || !rays_d || !aabb || !nears || !fars)
        return fail(SAMNERF_EINVAL, "near_far: null pointer");
    if (N == 0) return SAMNERF_OK;
    Aabb box;
    for (int i = 0; i < 6; ++i) box.v[i] = aabb[i];
    k_near_far<<<div_up(N, 256), 256, 0, reinterpret_cast<hipStream_t>(stream)>>>(
        rays_o, rays_d, N, box, min_near, nears, fars);
    return check_launch("near_far");
}

int samnerf_contract(const float* x, float* z, uint32_t N, samnerf_stream_t stream) {
    if (!x || !z) return fail(SAMNERF_EINVAL, "contract: null pointer");
    if (N == 0) return SAMNERF_OK;
    k_contract<<<div_up(N, 256), 256, 0, reinterpret_cast<hipStream_t>(stream)>>>(x, z, N);
    return check_launch("contract");
}

int samnerf_sample_pdf(const float* bins, const float* weights, uint32_t N, uint32_t T0,
                       uint32_t T, float* out, int32_t* inds, samnerf_stream_t stream) {
    if (!bins || !weights || !out) return fail(SAMNERF_EINVAL, "sample_pdf: null pointer");
    if (T0 == 0 || T == 0) return fail(SAMNERF_EINVAL, "sample_pdf: empty bins");
    if (N == 0) return SAMNERF_OK;
    // renderer.py:97: u = linspace(0.5 / T, 1 - 0.5 / T, T), bounds from Python doubles
    const Lin u = make_lin((float)(0.5 / T), (float)(1.0 - 0.5 / T), T);
    k_sample_pdf<<<div_up(N, 256), 256, 0, reinterpret_cast<hipStream_t>(stream)>>>(
        bins, weights, N, T0, T, u, out, inds);
    return check_launch("sample_pdf");
}

int samnerf_composite_weights(const float* real_bins, const float* sigmas, uint32_t N, uint32_t T,
                              float* weights, samnerf_stream_t stream) {
    if (!real_bins || !sigmas || !weights) return fail(SAMNERF_EINVAL, "composite: null pointer");
    if (N == 0 || T == 0) return SAMNERF_OK;
    k_composite<<<div_up(N, 256), 256, 0, reinterpret_cast<hipStream_t>(stream)>>>(
        real_bins, sigmas, N, T, weights);
    return check_launch("composite_weights");
}

size_t samnerf_render_workspace_size(const samnerf_model* model, uint32_t N) {
    if (!model) return 0;
    return carve(model, N, nullptr).bytes;
}

}  // extern "C"

namespace {

// Where the per-ray outputs go: separate arrays (samnerf_render_forward) or
// the rows of one gather tile (samnerf_render_forward_tile).
struct OutLayout {
    float* image;
    float* depth;
    float* wsum;
    float* samvit;
    uint32_t img_ld, scal_ld, sv_ld;
};

int render_impl(const samnerf_model* m, const float* rays_o, const float* rays_d, uint32_t N,
                const float* cam_near_far, uint32_t n_cnf, float bg_color, const OutLayout& ol,
                float* feature_rows, void* workspace, size_t workspace_bytes, samnerf_stream_t stream) {
    float* const image = ol.image;
    float* const depth = ol.depth;
    float* const weights_sum = ol.wsum;
    float* const samvit = ol.samvit;
    if (m->num_steps[0] != 128 || m->num_steps[1] != 64 || m->num_steps[2] != 32)
        return fail(SAMNERF_EINVAL, "render: fused path is built for num_steps = [128, 64, 32]");
    // with_sam and samvit == NULL: the caller does not want the features
    // (renderer.py computes them and drops them when return_feats == 0), so the
    // s_grid composite runs only if feature_rows are requested and the head not
    // at all
    if (cam_near_far && n_cnf != 1 && n_cnf != N)
        return fail(SAMNERF_EINVAL, "render: cam_near_far must have 1 or N rows");
    if (int prc = check_perturb(m, "render")) return prc;
    if (int brc = check_background(N, "render")) return brc;
    Workspace w = carve(m, N, workspace);
    if (!workspace || workspace_bytes < w.bytes)
        return fail(SAMNERF_EWORKSPACE, "render: workspace needs %zu bytes, got %zu", w.bytes,
                    workspace_bytes);
    for (int i = 0; i < 3; ++i)
        if (!m->grid_mlp[i] || !m->view_mlp[i]) return fail(SAMNERF_EINVAL, "render: null MLP weight");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    float* rows = feature_rows ? feature_rows : w.rows;

    GridDesc<16> gp0, gp1, gg, gs;
    int rc;
    if ((rc = make_grid_desc(m->prop[0], 2, 5, gp0, "prop_encoders.0"))) return rc;
    if ((rc = make_grid_desc(m->prop[1], 2, 5, gp1, "prop_encoders.1"))) return rc;
    if ((rc = make_grid_desc(m->grid, 2, 16, gg, "grid"))) return rc;
    if (m->with_sam && (rc = make_grid_desc(m->s_grid, 8, 16, gs, "s_grid"))) return rc;

    // (parity taps: the tapped intermediates stay in slot order, the caller
    // maps slots to rays -- fused.py ray_of_slots -- so the taps see the
    // product's tiled launch)
    const RayTiles tiles = make_ray_tiles(N, m->view_width);
    // parity taps (samnerf_set_taps): the stages write their intermediates to
    // the caller's buffers instead of the workspace; the kernels are the same
    if (g_taps_on && g_taps_n != N)
        return fail(SAMNERF_EINVAL, "render: taps were set for %u rays, the call renders %u", g_taps_n, N);
    const samnerf_taps tp = g_taps_on ? g_taps : samnerf_taps{};
    float* const bins1 = tp.bins1 ? tp.bins1 : w.bins1;
    float* const bins2 = tp.bins2 ? tp.bins2 : w.bins2;
    const int look = lookup_mode();

    // stages 0 and 1: 128 samples -> 65 bins -> 64 samples -> 33 bins
    ProposalRun pr{};
    pr.rays_o = rays_o;
    pr.rays_d = rays_d;
    pr.cnf = cam_near_far;
    pr.n_cnf = n_cnf;
    pr.tiles = tiles;
    pr.look = look;
    pr.mark = mark_stage;
    pr.snf = w.snf;
    pr.rec = w.rec;
    pr.st[0] = {gp0, bins1, tp.ds0 ? tp.ds0 : w.wtmp, tp.inds1, tp.w0};
    pr.st[1] = {gp1, bins2, tp.ds1 ? tp.ds1 : w.wtmp, tp.inds2, tp.w1};
    uint32_t forms[3] = {g_last_forms[0], g_last_forms[1], g_last_forms[2]};
    run_proposal_stages(m, N, pr, s, forms);
    g_last_forms[0] = forms[0];
    g_last_forms[1] = forms[1];

    // stage 2: 32 samples through the full network
    if (!(m->t_thresh >= 0.0f && m->t_thresh < 1.0f))
        return fail(SAMNERF_EINVAL, "render_forward: t_thresh %g outside [0, 1)", (double)m->t_thresh);
    if (tp.row_stride == 0 && (tp.rows2 || tp.srows))
        return fail(SAMNERF_EINVAL, "render: taps rows2 / srows need row_stride > 0");
    const bool sam_rows = m->with_sam && (samvit || feature_rows);
    FinalRun fr{};
    fr.rays_o = rays_o;
    fr.rays_d = rays_d;
    fr.tiles = tiles;
    fr.grid = gg;
    fr.bins_in = bins2;
    fr.bg = bg_color;
    fr.bg_rgb = current_background().bg_rgb;
    fr.n_bg = current_background().n_bg;
    fr.image = image;
    fr.depth = depth;
    fr.wsum = weights_sum;
    fr.img_ld = ol.img_ld;
    fr.scal_ld = ol.scal_ld;
    fr.rows = sam_rows || feature_rows ? rows : nullptr;
    fr.sam_rows = sam_rows;
    fr.sigma_tap = tp.sigma2;
    fr.rows_tap = tp.rows2;
    fr.tap_stride = tp.row_stride ? tp.row_stride : 1u;
    fr.mark = mark_stage;
    if ((rc = run_final(m, N, fr, w, s, forms[2]))) return rc;
    g_last_forms[2] = forms[2];

    if (sam_rows) {
        mark_stage(3, s);
        launch_sgrid(N, tiles, gs, w.u_f, w.w_f, rows, tp.srows, fr.tap_stride, look, s);
        if ((rc = check_launch("render"))) return rc;
        mark_stage(4, s);
        if (samvit) rc = sam_head_forward(m, rows, N, samvit, w.packed, s, ol.sv_ld, pack_weights(m));
        mark_stage(5, s);
        if (rc == SAMNERF_OK) rc = copy_final_taps(tp, w, N, s);
        return rc;
    }
    mark_stage(3, s);
    mark_stage(4, s);
    mark_stage(5, s);
    if ((rc = check_launch("render"))) return rc;
    return copy_final_taps(tp, w, N, s);
}

}  // namespace

extern "C" {

int samnerf_render_forward(const samnerf_model* m, const float* rays_o, const float* rays_d,
                           uint32_t N, const float* cam_near_far, uint32_t n_cnf, float bg_color,
                           float* image, float* depth, float* weights_sum, float* samvit,
                           float* feature_rows, void* workspace, size_t workspace_bytes,
                           samnerf_stream_t stream) {
    // N = 0 is a no-op whatever the buffers (an empty torch tensor has a null
    // data pointer)
    if (!m) return fail(SAMNERF_EINVAL, "render: null pointer");
    if (N == 0) return SAMNERF_OK;
    if (!rays_o || !rays_d || !image || !depth || !weights_sum)
        return fail(SAMNERF_EINVAL, "render: null pointer");
    const OutLayout ol{image, depth, weights_sum, samvit, 3u, 1u, 256u};
    return render_impl(m, rays_o, rays_d, N, cam_near_far, n_cnf, bg_color, ol, feature_rows, workspace,
                       workspace_bytes, stream);
}

int samnerf_render_forward_tile(const samnerf_model* m, const float* rays_o, const float* rays_d,
                                uint32_t N, const float* cam_near_far, uint32_t n_cnf, float bg_color,
                                float* tile, uint32_t ld, int feats, float* feature_rows, void* workspace,
                                size_t workspace_bytes, samnerf_stream_t stream) {
    if (!m) return fail(SAMNERF_EINVAL, "render_tile: null pointer");
    if (N == 0) return SAMNERF_OK;
    if (!rays_o || !rays_d || !tile) return fail(SAMNERF_EINVAL, "render_tile: null pointer");
    const bool sv = feats && m->with_sam;
    if (ld < (sv ? 261u : 5u))
        return fail(SAMNERF_EINVAL, "render_tile: row of %u floats cannot hold the outputs (needs %u)", ld,
                    sv ? 261u : 5u);
    const OutLayout ol{tile, tile + 3, tile + 4, sv ? tile + 5 : nullptr, ld, ld, ld};
    return render_impl(m, rays_o, rays_d, N, cam_near_far, n_cnf, bg_color, ol, feature_rows, workspace,
                       workspace_bytes, stream);
}

int samnerf_set_stage_events(void* const* events, uint32_t n) {
    if (n > 8) return fail(SAMNERF_EINVAL, "set_stage_events: at most 8 events");
    g_n_stage_events = events ? n : 0u;
    for (uint32_t i = 0; i < g_n_stage_events; ++i)
        g_stage_events[i] = reinterpret_cast<hipEvent_t>(events[i]);
    return SAMNERF_OK;
}

int samnerf_last_forms(uint32_t* out, uint32_t n) {
    for (uint32_t i = 0; out && i < n && i < 4; ++i) out[i] = g_last_forms[i];
    return 4;
}

int samnerf_clock_stamp(uint64_t* out, samnerf_stream_t stream) {
    if (!out) return fail(SAMNERF_EINVAL, "clock_stamp: null pointer");
    k_clock_stamp<<<256, 64, 0, reinterpret_cast<hipStream_t>(stream)>>>(
        reinterpret_cast<unsigned long long*>(out));
    return check_launch("clock_stamp");
}

int samnerf_set_taps(const samnerf_taps* taps, uint32_t N) {
    g_taps_on = taps != nullptr;
    g_taps = taps ? *taps : samnerf_taps{};
    g_taps_n = taps ? N : 0u;
    return SAMNERF_OK;
}

int samnerf_mask_forward(const samnerf_model* m, uint32_t N, float* logits, const void* workspace,
                         size_t workspace_bytes, samnerf_stream_t stream) {
    if (!m) return fail(SAMNERF_EINVAL, "mask_forward: null model");
    if (!m->with_mask) return fail(SAMNERF_EINVAL, "mask_forward: model has no mask head (with_mask = 0)");
    if (N == 0) return SAMNERF_OK;
    if (!logits || !workspace) return fail(SAMNERF_EINVAL, "mask_forward: null pointer");
    if (m->mask_out < 1 || m->mask_out > 32)
        return fail(SAMNERF_EINVAL, "mask_forward: mask_out %u outside 1..32", m->mask_out);
    if (m->num_steps[2] != 32) return fail(SAMNERF_EINVAL, "mask_forward: fused path is built for 32 final samples");
    Workspace w = carve(m, N, const_cast<void*>(workspace));
    if (workspace_bytes < w.bytes)
        return fail(SAMNERF_EWORKSPACE, "mask_forward: workspace needs %zu bytes, got %zu", w.bytes,
                    workspace_bytes);
    if (m->mask_kind != 0) {                            // adaptive: k_final wrote them
        if (hipMemcpyAsync(logits, w.mlog, sizeof(float) * m->mask_out * (size_t)N, hipMemcpyDeviceToDevice,
                           reinterpret_cast<hipStream_t>(stream)) != hipSuccess)
            return fail(SAMNERF_ELAUNCH, "mask_forward: copy failed");
        return SAMNERF_OK;
    }
    for (int i = 0; i < 3; ++i)
        if (!m->mask_w[i]) return fail(SAMNERF_EINVAL, "mask_forward: null mask_mlp weight");
    GridDesc<16> gm;
    int rc = make_grid_desc(m->m_grid, 8, 16, gm, "m_grid");
    if (rc) return rc;
    const RayTiles tiles = make_ray_tiles(N, m->view_width);
    return mask_head_forward(m, gm, w.u_f, w.w_f, w.geo_f, N, logits, tiles, w.mpacked,
                             reinterpret_cast<hipStream_t>(stream));
}

size_t samnerf_mask_train_workspace_size(uint32_t N) { return mask_train_workspace_bytes(N); }

size_t samnerf_mask_train_workspace_size_model(const samnerf_model* m, uint32_t N) {
    if (!m || !m->with_mask || m->mask_kind < 0 || m->mask_kind > 2) return mask_train_workspace_bytes(N);
    return mask_train_workspace_bytes(m->mask_kind, N);
}

// the render workspace's final samples of a 'default' mask model, checked
static int mask_train_inputs(const samnerf_model* m, uint32_t N, const void* render_ws, size_t render_bytes,
                             Workspace& w, GridDesc<16>& gm, const char* what) {
    if (!m) return fail(SAMNERF_EINVAL, "%s: null model", what);
    if (!m->with_mask || m->mask_kind < 0 || m->mask_kind > 2)
        return fail(SAMNERF_EINVAL, "%s: model has no fused mask head (with_mask = 1, mask_kind 0-2)", what);
    if (m->mask_out < 1 || m->mask_out > 32)
        return fail(SAMNERF_EINVAL, "%s: mask_out %u outside 1..32", what, m->mask_out);
    if (m->num_steps[2] != 32) return fail(SAMNERF_EINVAL, "%s: fused path is built for 32 final samples", what);
    if (!render_ws) return fail(SAMNERF_EINVAL, "%s: null render workspace", what);
    w = carve(m, N, const_cast<void*>(render_ws));
    if (render_bytes < w.bytes)
        return fail(SAMNERF_EWORKSPACE, "%s: render workspace needs %zu bytes, got %zu", what, w.bytes,
                    render_bytes);
    if (m->mask_kind != 0 && m->with_mask != 2)
        return fail(SAMNERF_EINVAL, "%s: the adaptive heads train on a render with with_mask = 2 (it keeps "
                    "the per-ray input sums)", what);
    return m->mask_kind == 0 ? make_grid_desc(m->m_grid, 8, 16, gm, "m_grid") : SAMNERF_OK;
}

int samnerf_mask_train_forward(const samnerf_model* m, uint32_t N, float* logits, const void* render_ws,
                               size_t render_bytes, void* workspace, size_t workspace_bytes,
                               samnerf_stream_t stream) {
    Workspace w;
    GridDesc<16> gm;
    int rc = mask_train_inputs(m, N, render_ws, render_bytes, w, gm, "mask_train_forward");
    if (rc) return rc;
    if (N == 0) return SAMNERF_OK;
    if (!logits || !workspace) return fail(SAMNERF_EINVAL, "mask_train_forward: null pointer");
    if (m->mask_kind != 0)                               // adaptive: the chain on the per-ray sums
        return adaptive_train_forward(m, w.xsum, N, logits, workspace, workspace_bytes,
                                      reinterpret_cast<hipStream_t>(stream));
    const RayTiles tiles = make_ray_tiles(N, m->view_width);
    return mask_train_forward(m, gm, w.u_f, w.w_f, w.geo_f, N, tiles, logits, workspace, workspace_bytes,
                              reinterpret_cast<hipStream_t>(stream));
}

int samnerf_mask_train_backward(const samnerf_model* m, uint32_t N, const float* grad_logits,
                                float* const* grad_mask_w, float* grad_m_grid, const void* render_ws,
                                size_t render_bytes, void* workspace, size_t workspace_bytes,
                                samnerf_stream_t stream) {
    Workspace w;
    GridDesc<16> gm;
    int rc = mask_train_inputs(m, N, render_ws, render_bytes, w, gm, "mask_train_backward");
    if (rc) return rc;
    if (N == 0) return SAMNERF_OK;
    if (!grad_logits || !grad_mask_w || !workspace)
        return fail(SAMNERF_EINVAL, "mask_train_backward: null pointer");
    if (m->mask_kind != 0)                               // adaptive: no grid gradient (all inputs detached)
        return adaptive_train_backward(m, w.xsum, N, grad_logits, grad_mask_w, workspace, workspace_bytes,
                                       reinterpret_cast<hipStream_t>(stream));
    if (!grad_m_grid) return fail(SAMNERF_EINVAL, "mask_train_backward: null m_grid gradient");
    for (int i = 0; i < 3; ++i)
        if (!grad_mask_w[i]) return fail(SAMNERF_EINVAL, "mask_train_backward: null gradient");
    const RayTiles tiles = make_ray_tiles(N, m->view_width);
    return mask_train_backward(m, gm, w.u_f, w.w_f, w.geo_f, N, tiles, grad_logits, grad_mask_w, grad_m_grid,
                               workspace, workspace_bytes, reinterpret_cast<hipStream_t>(stream));
}

}  // extern "C"
