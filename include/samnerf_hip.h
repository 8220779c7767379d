/*
 * samnerf_hip.h -- C ABI of the MI355X (gfx950) NeRF ray-march library
 * (libsamnerf_hip.so).  Plain pointers and sizes only; no torch types.
 *
 * All pointers are DEVICE pointers unless a parameter says "host".  Every
 * function is asynchronous on `stream` (a hipStream_t; NULL = the legacy
 * default stream, which is what the reference's <<<>>> launches use,
 * gridencoder.cu:386), never synchronises the host, never allocates, and
 * returns 0 on success or a negative SAMNERF_E* code; the message is then
 * available from samnerf_last_error() (thread-local).
 *
 * Drop-in encoder entry points -- one per pybind function of the reference:
 *   gridencoder/src/gridencoder.h:12-16 (bound at gridencoder/src/bindings.cpp:6-9)
 *   shencoder/src/shencoder.h:9-10      (bound at shencoder/src/bindings.cpp:6-7)
 *   freqencoder/src/freqencoder.h:7,10  (bound at freqencoder/src/bindings.cpp:6-7)
 * Argument order and meaning follow those signatures; tensors become raw
 * float / int32 pointers (fp32 only: the reference's fp16 dispatch is dead on
 * this path because main.py:222 forces fp16 off).
 *
 * Fused entry points -- the ray-march inner loop of nerf/renderer.py:221-390
 * + nerf/network.py:221-259 (NeRFRenderer.run), which the reference runs as
 * ~350 unfused ATen ops per chunk around the encoder kernels.
 */
#ifndef SAMNERF_HIP_H
#define SAMNERF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* samnerf_stream_t; /* == hipStream_t */

enum {
    SAMNERF_OK = 0,
    SAMNERF_EINVAL = -1,   /* bad argument (shape / enum / null pointer) */
    SAMNERF_ELAUNCH = -2,  /* kernel launch failed */
    SAMNERF_EWORKSPACE = -3 /* workspace too small */
};

/* Library identity / diagnostics (host only, no GPU needed). */
const char* samnerf_version(void);
const char* samnerf_last_error(void);
/* 1 in the diagnostic build (libsamnerf_hip_diag.so: the kernels' A/B variant
 * switches read from SAMNERF_* environment variables, for the bit-identity
 * tests), 0 in the product library (one path per configuration). */
int samnerf_diag_variants(void);

/* ------------------------------------------------------------ gridencoder --
 * Replaces grid_encode_forward (gridencoder.h:12, gridencoder.cu:467-490).
 * inputs [B,D] in [0,1]; embeddings [rows,C]; offsets [L+1] int32;
 * outputs [L,B,C] (level-major, as grid.py:49 allocates it); dy_dx
 * [B, L*D*C] or NULL.  gridtype 0 hash / 1 tiled; interp 0 linear /
 * 1 smoothstep.  Levels >= max_level are not written (caller zero-fills,
 * grid.py:52).  C in {1,2,4,8,16,32}, D in {2,3,4,5}. */
int samnerf_grid_encode_forward(const float* inputs, const float* embeddings,
                                const int32_t* offsets, float* outputs,
                                uint32_t B, uint32_t D, uint32_t C, uint32_t L,
                                uint32_t max_level, float S, uint32_t H,
                                float* dy_dx, uint32_t gridtype, int align_corners,
                                uint32_t interp, samnerf_stream_t stream);

/* Replaces grid_encode_backward (gridencoder.h:13, gridencoder.cu:492-522).
 * grad [L,B,C]; grad_embeddings [rows,C] accumulated into (caller zeroes,
 * grid.py:83); dy_dx / grad_inputs both NULL or both set ([B,D], written). */
int samnerf_grid_encode_backward(const float* grad, const float* inputs,
                                 const float* embeddings, const int32_t* offsets,
                                 float* grad_embeddings, uint32_t B, uint32_t D,
                                 uint32_t C, uint32_t L, uint32_t max_level, float S,
                                 uint32_t H, const float* dy_dx, float* grad_inputs,
                                 uint32_t gridtype, int align_corners, uint32_t interp,
                                 samnerf_stream_t stream);

/* Replaces grad_total_variation (gridencoder.h:15, gridencoder.cu:662-668). */
int samnerf_grad_total_variation(const float* inputs, const float* embeddings, float* grad,
                                 const int32_t* offsets, float weight, uint32_t B,
                                 uint32_t D, uint32_t C, uint32_t L, float S, uint32_t H,
                                 uint32_t gridtype, int align_corners,
                                 samnerf_stream_t stream);

/* Replaces grad_weight_decay (gridencoder.h:16, gridencoder.cu:705-713).
 * B = rows of the embeddings table. */
int samnerf_grad_weight_decay(const float* embeddings, float* grad, const int32_t* offsets,
                              float weight, uint32_t B, uint32_t C, uint32_t L,
                              samnerf_stream_t stream);

/* -------------------------------------------------------------- shencoder --
 * Replaces sh_encode_forward (shencoder.h:9, shencoder.cu:400-417).
 * inputs [B,D=3] unit vectors; outputs [B,C*C] (C = degree 1..8);
 * dy_dx [B,D,C*C] or NULL. */
int samnerf_sh_encode_forward(const float* inputs, float* outputs, uint32_t B, uint32_t D,
                              uint32_t C, float* dy_dx, samnerf_stream_t stream);

/* Replaces sh_encode_backward (shencoder.h:10, shencoder.cu:419-438).
 * grad_inputs [B,D] is accumulated into (caller zeroes, sphere_harmonics.py:50). */
int samnerf_sh_encode_backward(const float* grad, const float* inputs, uint32_t B, uint32_t D,
                               uint32_t C, const float* dy_dx, float* grad_inputs,
                               samnerf_stream_t stream);

/* ------------------------------------------------------------ freqencoder --
 * Replaces freq_encode_forward (freqencoder.h:7, freqencoder.cu:97-110):
 * outputs [B, C], C = D + 2*D*deg. */
int samnerf_freq_encode_forward(const float* inputs, uint32_t B, uint32_t D, uint32_t deg,
                                uint32_t C, float* outputs, samnerf_stream_t stream);

/* Replaces freq_encode_backward (freqencoder.h:10, freqencoder.cu:113-129). */
int samnerf_freq_encode_backward(const float* grad, const float* outputs, uint32_t B,
                                 uint32_t D, uint32_t deg, uint32_t C, float* grad_inputs,
                                 samnerf_stream_t stream);

/* ------------------------------------------------------ ray-march pieces --
 * Stand-alone kernels of the individual steps, used by the parity tests and
 * by hosts that keep their own loop.  Each cites the reference op sequence it
 * reproduces. */

/* get_rays, full-image branch (nerf/utils.py:145-279, N = -1):
 * pose_host = row-major 4x4 cam2world (host), intrinsics (fx, fy, cx, cy);
 * rays_o, rays_d [rows*W, 3]: the rays of pixel rows [row0, row0 + rows). */
int samnerf_get_rays(const float* pose_host, float fx, float fy, float cx, float cy,
                     uint32_t H, uint32_t W, uint32_t row0, uint32_t rows,
                     float* rays_o, float* rays_d, samnerf_stream_t stream);

/* near_far_from_aabb (nerf/renderer.py:122-139); aabb_host = 6 floats. */
int samnerf_near_far(const float* rays_o, const float* rays_d, uint32_t N,
                     const float* aabb_host, float min_near, float* nears, float* fars,
                     samnerf_stream_t stream);

/* contract (nerf/renderer.py:60-69): x, z [N,3]. */
int samnerf_contract(const float* x, float* z, uint32_t N, samnerf_stream_t stream);

/* sample_pdf (nerf/renderer.py:84-119, perturb = False): bins [N,T0+1],
 * weights [N,T0] -> out [N,T]; inds [N,T] int32 (searchsorted result, may be
 * NULL). */
int samnerf_sample_pdf(const float* bins, const float* weights, uint32_t N, uint32_t T0,
                       uint32_t T, float* out, int32_t* inds, samnerf_stream_t stream);

/* sigmas -> weights (nerf/renderer.py:310-326, background 'last_sample'):
 * real_bins [N,T+1], sigmas [N,T] -> weights [N,T]. */
int samnerf_composite_weights(const float* real_bins, const float* sigmas, uint32_t N,
                              uint32_t T, float* weights, samnerf_stream_t stream);

/* Host helper: torch.linspace(start, end, steps) in float32 exactly as torch
 * computes it on the CPU (the sample positions of renderer.py:97, :265). */
void samnerf_linspace_host(float start, float end, uint32_t steps, float* out_host);

/* The seeded perturbed positions (samnerf_model.perturb_device's contract, stated
 * there), host only, no GPU needed: the positions of `stage` (0, 1, 2) of ray
 * `ray` for (seed, offset) -> out_host[num_steps[stage] + 1].  Returns
 * SAMNERF_EINVAL for a null pointer, stage > 2 or a num_steps entry outside
 * 1..65535. */
int samnerf_perturb_host(uint64_t seed, uint64_t offset, const uint32_t* num_steps, uint32_t stage,
                         uint32_t ray, float* out_host);

/* The same positions on the device, for N rays: bins0 [N][num_steps[0] + 1], u1
 * [N][num_steps[1] + 1], u2 [N][num_steps[2] + 1], ray order -- the layout of
 * samnerf_model.perturb, so a render fed these arrays equals the render with
 * perturb_device = 1 and the same (seed, offset) bit for bit (to log or replay a
 * step's draws).  Any of the three pointers may be NULL (not written);
 * num_steps is a host pointer. */
int samnerf_perturb_fill(uint64_t seed, uint64_t offset, uint32_t N, const uint32_t* num_steps,
                         float* bins0, float* u1, float* u2, samnerf_stream_t stream);

/* ------------------------------------------------------------ fused path --
 * One hash grid of the model (GridEncoder, gridencoder/grid.py:102-146). */
typedef struct {
    const float* embeddings;      /* device [rows, level_dim] */
    const int32_t* offsets_host;  /* HOST [num_levels + 1] (grid.py:124-135) */
    uint32_t num_levels;
    uint32_t level_dim;
    float S;                      /* log2(per_level_scale), grid.py:38 */
    uint32_t base_resolution;     /* H */
} samnerf_grid;

/* NeRFNetwork(opt) weights (nerf/network.py:94-219), torch layout [out, in],
 * plus the forced options of main.py:222-226. */
typedef struct {
    samnerf_grid grid;            /* network.py:102  L16 C2  */
    samnerf_grid s_grid;          /* network.py:111  L16 C8  (with_sam) */
    samnerf_grid prop[2];         /* network.py:211, :216  L5 C2 */
    const float* grid_mlp[3];     /* [64,32] [64,64] [16,64] */
    const float* view_mlp[3];     /* [32,31] [32,32] [3,32]  */
    const float* prop_mlp[2][2];  /* [16,10] [1,16] each */
    const float* sam_w[5];        /* [256,163] [256,256] [256,419] [256,256] [256,256] */
    const float* sam_b[5];        /* [256] each */
    const float* ln_w;            /* LayerNorm(256) weight / bias */
    const float* ln_b;
    int with_sam;
    float aabb[6];                /* aabb_infer (renderer.py:163-167) */
    float grid_bound;             /* 2 under contract (renderer.py:152-153) */
    float min_near;               /* main.py:69 */
    uint32_t num_steps[3];        /* (128, 64, 32), main.py:79-80 */
    int head_mode;                /* precision of the GEMMs -- grid_mlp (per sample), the SAM
                                     head and the mask head: 0 = f16x3, each fp32 product as
                                     three fp16 MFMA products on power-of-two scaled operands
                                     with fp32 accumulate (fp32-equivalent, default); 1 = exact
                                     fp32 MFMA (v_mfma_f32_32x32x2_f32) */
    float t_thresh;               /* N1, a flagged NON-PARITY mode: 0 = off (the
                                     reference's semantics, default); t in (0, 1): a wave of 32
                                     rays stops marching the final stage once every ray's
                                     transmittance is below t -- the dropped samples' weights
                                     (their sum <= t per ray) become 0, so weights_sum, depth,
                                     colour and features change by at most t x their range */
    uint32_t view_width;          /* layout hint of the ray batch, not a weight: the rays are a
                                     row-major image this many pixels wide (0 = unknown).  When W
                                     is a multiple of 8 and N of 4 W, the kernels group rays into
                                     8 x 4 pixel tiles (compact wave footprints, better gather
                                     locality); outputs stay in ray order and are bit-identical.
                                     samnerf_sgrid_backward must see the value of the forward. */
    /* --with_mask instance heads (network.py:125-203, renderer.py:392-452), rendered by
     * samnerf_mask_forward after a samnerf_render_forward with with_mask = 1 (0: no mask
     * outputs, nothing extra computed).  mask_kind 0 = 'default': m_grid L16 C8 and
     * SkipConnMLP(143 -> 256 -> 256 -> mask_out, bias=False, leaky_relu), mask_w[0..2]
     * = [256,143] [256,256] [mask_out,256]; 1 = 'adaptive' / 'density': six bias-free
     * Linears on the grid_mlp intermediates, mask_w[0..5] = [96,32] [96,160] [96,160]
     * [96,112] [96,96] [mask_out,96]; 2 = 'adaptive' / 'rgb' (needs sum_after_mlp):
     * eight, also on the view_mlp intermediates, mask_w[0..7] = [96,32] [96,160]
     * [96,160] [96,112] [96,128] [96,128] [96,96] [mask_out,96].
     * with_mask = 2: a training render -- the adaptive heads' render also keeps
     * each ray's weighted input sums (240 floats per ray) in the workspace for
     * samnerf_mask_train_forward / _backward, which need with_mask = 2 on those
     * heads; inference renders (1) neither store nor allocate them. */
    int with_mask;
    int mask_kind;
    samnerf_grid m_grid;          /* mask_kind 0 */
    const float* mask_w[8];
    uint32_t mask_out;            /* n_inst (+ redundant_instance for 'default'), 1..32 */
    int sum_after_mlp;            /* --sum_after_mlp (renderer.py:339-342): image =
                                     sigmoid(sum_k w_k view_mlp(colour_k)); RGB / mask models only
                                     (with SAM features the reference crashes) */
    /* perturb=True (renderer.py:266-271 and sample_pdf's :100-101): the perturbed
     * sample positions as the reference computes them from torch.rand_like, ray order:
     * perturb[0] = the stage-0 bins clamp(linspace(0, 1, T0+1) + (rand - 0.5) / T0, 0, 1)
     * [N][num_steps[0]+1]; perturb[1], perturb[2] = sample_pdf's u = linspace(0.5/T,
     * 1-0.5/T, T) + (rand - 0.5) / T of stages 1 and 2, [N][T] with T = num_steps[s]+1.
     * Set per call; all NULL = perturb=False (the default), all three or none.
     * (perturb_device below: the same positions drawn inside the kernels from a
     * seed instead.) */
    const float* perturb[3];
    /* 1: the render workspace already holds this model's packed MLP weights
     * (the f16x3 grid_mlp fragments and the SAM head's weight stream) from an
     * earlier samnerf_render_forward(_tile) on the same workspace with the same
     * weights and head_mode, so the packing launches (k_pack_grid_mlp,
     * k_head_wmax, k_pack_h16: ~25 us per call) are skipped; 0 (default):
     * pack.  The caller vouches for it (fused.py: the weights' data pointers
     * and torch version counters); the diagnostic library always packs. */
    int reuse_packed;
    /* perturb=True with the positions drawn inside the kernels (appended: the
     * fields above keep their offsets).  perturb_device != 0: every perturbed
     * position is a pure function of (perturb_seed, perturb_offset, stage, ray,
     * index) -- no position array is allocated, written or read, and the render
     * does not depend on view_width.  Statistically the reference's sampling
     * (uniform jitter of one bin width), NOT torch's generator stream: perturb[]
     * above keeps that contract.  The contract of this mode, exact to the bit:
     *   generator  Philox4x32-10 (multipliers 0xD2511F53 / 0xCD9E8D57, Weyl
     *              constants 0x9E3779B9 / 0xBB67AE85, ten rounds)
     *   key        (seed & 0xffffffff, seed >> 32)
     *   counter    value i of stage s of ray `ray` (ray order): c0 = (i >> 2) |
     *              s << 16, c1 = ray, c2 = offset & 0xffffffff, c3 = offset >> 32;
     *              the value uses output word i & 3
     *   stages     s = 0: the num_steps[0] + 1 stage-0 bins; s = 1, 2: sample_pdf's
     *              u of that stage, T = num_steps[s] + 1 values
     *   uniform    r = (word >> 8) * 2^-24, in [0, 1)
     *   positions  fp32, one rounding per op, no fma contraction, true division:
     *              stage 0 clamp(linspace(0, 1, T0 + 1)[i] + (r - 0.5f) / (float)T0,
     *              0, 1); stages 1, 2 linspace(0.5 / T, 1 - 0.5 / T, T)[j] + (r -
     *              0.5f) / (float)T, the linspaces as samnerf_linspace_host
     * (renderer.py:266-271 and :97-101 with r for torch.rand_like).  A call
     * should use a fresh perturb_offset (a step or chunk counter) per seed.
     * perturb_device != 0 with any perturb[i] set is SAMNERF_EINVAL.
     * samnerf_rgb_train_backward must see the forward's seed and offset. */
    int perturb_device;
    uint64_t perturb_seed;
    uint64_t perturb_offset;
} samnerf_model;

/* The reference's --background modes and bg_color shapes, for the NEXT calls of
 * this thread (like samnerf_set_taps; samnerf_model keeps its layout -- its last
 * fields stay the perturb_* ones).
 * background: 0 = 'last_sample' (the default: the last sample's delta * sigma is
 * +inf in every compositing, renderer.py:314, so weights_sum is 1); 1 =
 * transparent ('white' and 'random': that line is skipped, the last sample
 * composites like any other and weights_sum <= 1).
 * bg_rgb: device pointer, [n_bg,3] floats in ray order; NULL = the scalar bg_color
 * argument (samnerf_rgb_train_opts.bg_color for samnerf_rgb_train_step, which
 * bg_rgb overrides).  n_bg = 1: one colour for every ray (the GUI's [3] colour);
 * n_bg = N: a colour per ray (training under --background random,
 * utils.py:892-896).  No gradient is produced for the colour.
 * samnerf_set_background(NULL) restores the defaults (0, NULL, 0); it only stores
 * the values.  They are validated beside the other arguments of every call that
 * reads them -- samnerf_render_forward, _forward_tile, samnerf_rgb_train_step,
 * _forward and _backward: background not in {0, 1}, bg_rgb != NULL with n_bg not
 * in {1, N}, or bg_rgb == NULL with n_bg != 0 is SAMNERF_EINVAL, the message naming
 * the field.  The setting stays until it is set again: set it before a call and
 * restore the defaults after it.  samnerf_rgb_train_backward must run under the
 * forward's setting (the bg_rgb buffer still holding the forward's values). */
typedef struct {
    int background;
    const float* bg_rgb;
    uint32_t n_bg;
} samnerf_background;
int samnerf_set_background(const samnerf_background* bg);

/* Bytes of device workspace samnerf_render_forward needs for N rays. */
size_t samnerf_render_workspace_size(const samnerf_model* model, uint32_t N);

/* The whole ray-march inner loop for N rays (NeRFRenderer.run in eval mode:
 * perturb = False unless model->perturb or model->perturb_device is set, background 'last_sample' or transparent by samnerf_set_background, sum_after_mlp = False,
 * sam_use_view_direction = True): near/far, 3 proposal rounds with
 * inverse-CDF resampling, hash-grid + SH encoding, sigma / colour MLPs,
 * compositing, view MLP, and (with_sam) the s_grid feature composite plus the
 * SkipConnMLP + LayerNorm head.
 *   rays_o, rays_d [N,3]; cam_near_far [N,2] or [1,2] (n_cnf rows) or NULL;
 *   bg_color: scalar background (renderer.py:239-240, default 1), used when
 *   no bg_rgb is set (samnerf_set_background); bg_rgb [n_bg,3]: one RGB colour (n_bg = 1) or
 *   one per ray (n_bg = N), mixed in as (1 - weights_sum) * colour
 *   (renderer.py:356) -- also in the image columns of feature_rows;
 *   image [N,3], depth [N], weights_sum [N]; samvit [N,256] (with_sam; NULL
 *   = features not wanted: the s_grid composite and the head are skipped --
 *   renderer.py computes and drops them when return_feats == 0);
 *   feature_rows [N,164] optional: the per-ray head input
 *   cat(f_sam, f_image, image, depth) (+1 pad), kept for training.
 * Outputs are written, never accumulated.  N = 0 returns SAMNERF_OK without
 * touching any buffer (they may be NULL). */
int samnerf_render_forward(const samnerf_model* model, const float* rays_o,
                           const float* rays_d, uint32_t N, const float* cam_near_far,
                           uint32_t n_cnf, float bg_color, float* image, float* depth,
                           float* weights_sum, float* samvit, float* feature_rows,
                           void* workspace, size_t workspace_bytes, samnerf_stream_t stream);

/* The same render writing every per-ray output into one row-major tile
 * [N, ld] instead of separate arrays: columns 0-2 image, 3 depth, 4
 * weights_sum, 5-260 samvit (feats != 0 and with_sam; ld >= 261, else ld >= 5,
 * the feature columns untouched).  This is the all-gather record of a
 * ray-sharded view (samnerf_amd/dist.py, BASELINE config 4): a rank renders
 * its band straight into its slice of the gather buffer, so no pack copy
 * precedes the collective.  Replaces the reference's per-chunk torch.cat of
 * the outputs (renderer.py:205-217) for that path; bit-identical values. */
int samnerf_render_forward_tile(const samnerf_model* model, const float* rays_o,
                                const float* rays_d, uint32_t N, const float* cam_near_far,
                                uint32_t n_cnf, float bg_color, float* tile, uint32_t ld,
                                int feats, float* feature_rows, void* workspace,
                                size_t workspace_bytes, samnerf_stream_t stream);

/* The SAM head alone (samvit_mlp = SkipConnMLP(163, 256 x 5) + LayerNorm(256),
 * nerf/network.py:36-75, :120-123) on given head-input rows [N,164] (the
 * feature_rows layout of samnerf_render_forward: cat(f_sam, f_image, image,
 * depth) + 1 pad column) -> samvit [N,256], at model->head_mode's precision
 * (0 = f16x3, the default; 1 = exact fp32 MFMA).  The render runs the same
 * kernels on its own rows; this entry point serves callers that hold rows
 * (the reference's samvit_mlp call on a feature batch, renderer.py:384-388). */
size_t samnerf_sam_head_workspace_size(void);
int samnerf_sam_head_forward(const samnerf_model* model, const float* rows, uint32_t N,
                             float* samvit, void* workspace, size_t workspace_bytes,
                             samnerf_stream_t stream);

/* instance_mask_logits [N, mask_out] (renderer.py:392-395, :451-452):
 * sum_k w_k * mask_mlp(cat(m_grid(x_k), geo_feat_k)) over the final samples, the
 * weights and positions those of the samnerf_render_forward call that last used
 * `workspace` (same model, N and view_width; it stores each sample's geo_feat
 * when model->with_mask).  Precision follows head_mode (bf16x3 / exact fp32 MFMA).
 * Replaces the reference's per-chunk torch ops of that branch. */
int samnerf_mask_forward(const samnerf_model* model, uint32_t N, float* instance_mask_logits,
                         const void* workspace, size_t workspace_bytes, samnerf_stream_t stream);

/* The --with_mask training step's instance head (nerf/utils.py:941-977 under
 * renderer.py:392-395, :451-452; 'default' head, network.py:125-133), exact fp32
 * on MFMA.  forward: instance_mask_logits [N, mask_out] from the final samples
 * (positions, weights, geo_feat) that the samnerf_render_forward call with
 * with_mask = 1 left in `render_ws`, saving the head's activations in
 * `workspace` (samnerf_mask_train_workspace_size(N) bytes); backward: given
 * d loss / d logits [N, mask_out], writes the gradients of mask_w[0..2]
 * ([256,143] [256,256] [mask_out,256], overwritten) and scatters into
 * grad_m_grid (the m_grid embedding gradient, accumulated into: the
 * reference encoder's backward).  weights and geo_feat carry no gradient
 * (.detach() in the reference), the sample positions none (no parameter).
 * Replaces the reference's per-chunk torch ops and autograd of that branch.
 * 'adaptive' heads (mask_kind 1 'density', network.py:167-180, the reference's
 * scripts/train_mask.sh:16,20,21 configuration; 2 'rgb' with sum_after_mlp,
 * network.py:148-160): the render leaves each ray's weighted sums of the
 * head's (detached) inputs in `render_ws`; forward runs the bias-free Linear
 * chain on them (the head is linear: the logits of the per-sample chain and
 * weighted sum, to rounding), backward writes the gradients of every
 * mask_w[i] ([96,32] .. [mask_out,96], overwritten, fixed-order sums) -- the
 * only tensors the reference's loss reaches; grad_m_grid is unused (may be
 * NULL).  Workspace (same size function): 2 x 7 x 96 floats per ray. */
/* The 'default' head's workspace keeps its fp32 activations of all 32 samples of every
 * ray for the backward -- input (144), both hidden layers and their
 * gradients (4 x 256) and the logits and their gradient (2 x 32): about 157 KB
 * per ray, 0.64 GB at the reference's 4,096-ray batch (and the render's own
 * workspace stays alive until the backward).  Batches of 65,536 rays need
 * ~10 GB. */
size_t samnerf_mask_train_workspace_size(uint32_t N);
/* The workspace the given mask model needs (what samnerf_mask_train_workspace_size(N)
 * returns is the maximum over the head kinds): the 'default' head's
 * activation carve above, or 2 x 7 x 96 floats per ray for the adaptive heads
 * (mask_kind 1 / 2) -- ~5.4 KB per ray instead of ~157 KB. */
size_t samnerf_mask_train_workspace_size_model(const samnerf_model* model, uint32_t N);
int samnerf_mask_train_forward(const samnerf_model* model, uint32_t N, float* instance_mask_logits,
                               const void* render_ws, size_t render_ws_bytes, void* workspace,
                               size_t workspace_bytes, samnerf_stream_t stream);
int samnerf_mask_train_backward(const samnerf_model* model, uint32_t N, const float* grad_logits,
                                float* const* grad_mask_w, float* grad_m_grid, const void* render_ws,
                                size_t render_ws_bytes, void* workspace, size_t workspace_bytes,
                                samnerf_stream_t stream);

/* Backward of the s_grid feature composite for the SAM-distillation step
 * (nerf/utils.py:1098-1106 training branch): given the per-ray gradient of
 * f_sam [N,128] (the first 128 columns of d(loss)/d(feature_rows)), scatter
 * sum_k w_k * trilinear(corner) * g into grad_embeddings [rows, 8] of s_grid
 * (accumulated into).  Uses the sample weights/positions the last
 * samnerf_render_forward call left in `workspace` for the same rays. */
int samnerf_sgrid_backward(const samnerf_model* model, const float* grad_fsam, uint32_t N,
                           float* grad_embeddings, const void* workspace,
                           size_t workspace_bytes, samnerf_stream_t stream);

/* Deterministic form of samnerf_sgrid_backward (an optional mode
 * whose gradients repeat bit for bit run to run).  The reference scatters
 * with unordered fp32 atomics (gridencoder.cu:334-347), as the default form
 * does, so two identical steps differ in the last bits.  Here every
 * contribution is added to a 64-bit fixed-point accumulator instead (integer
 * atomics are associative: the totals do not depend on the order the waves
 * reach a row in), at the scale 2^(61 - ceil(log2 N) - e) with max |grad_fsam|
 * < 2^e, so no total can overflow (the final samples' weights sum to at most
 * 1 per ray); then the totals are added to grad_embeddings as fp32.  Each
 * contribution is an fp32 value (its products and the wave's 8-ray merge
 * round as in the default form) rounded to the quantum 2^(e + ceil(log2 N)
 * - 61) <= 2 max|g| 2^-(61 - ceil(log2 N)): a total of n contributions is
 * within n / 2 quanta plus 11 fp32 roundings of sum |contribution| of the
 * exact sum -- no term grows with n in fp32, which the default form's n
 * atomic adds have (tests/sgrid_ref.py bound_scatter_det, checked per row).
 * accum: accum_bytes >= samnerf_sgrid_accum_size(model) bytes of device
 * memory (else SAMNERF_EWORKSPACE), all zero on the first call (hipMemset)
 * and left zero by every call; one accumulator per stream (calls on one
 * stream run in order; concurrent calls must not share one).  A grad_fsam
 * holding a NaN or an Inf has no fixed-point scale: such a call adds with
 * the fp32 atomics, so the NaN / Inf reaches grad_embeddings as in the
 * reference (bits repeat for finite gradients only). */
size_t samnerf_sgrid_accum_size(const samnerf_model* model);
int samnerf_sgrid_backward_det(const samnerf_model* model, const float* grad_fsam, uint32_t N,
                               float* grad_embeddings, int64_t* accum, size_t accum_bytes,
                               const void* workspace, size_t workspace_bytes,
                               samnerf_stream_t stream);

/* ------------------------------------------------------------- training --
 * One Adam step (torch.optim.Adam semantics, amsgrad off, maximize off) over
 * every tensor of the table in one launch: param -= lr / (1 - beta1^step) *
 * m / (sqrt(v) / sqrt(1 - beta2^step) + eps) after m, v absorb grad (+
 * weight_decay * param).  The optimiser of the distillation step
 * (nerf/utils.py:1831, Adam(lr 1e-2, eps 1e-15) of main.py:296).  Tensors
 * with a NULL grad are skipped (torch skips parameters without .grad); step
 * counts from 1 and is the same for every tensor of the call.  The scalars
 * are doubles (Python floats): derived ones (1 - beta, bias corrections) are
 * formed in double and rounded to float once, as torch does. */
typedef struct {
    float* param;
    const float* grad;
    float* exp_avg;
    float* exp_avg_sq;
    uint64_t n;                   /* elements */
} samnerf_adam_tensor;
int samnerf_adam_step(const samnerf_adam_tensor* tensors_host, uint32_t n_tensors, double lr,
                      double beta1, double beta2, double eps, double weight_decay, uint32_t step,
                      samnerf_stream_t stream);

/* The SAM head of the distillation step with its backward (nerf/network.py:
 * 36-75, :120-123 under nerf/utils.py:1098-1106), exact fp32 on MFMA.
 * forward: rows [N,164] (the head input rows of samnerf_render_forward's
 * feature_rows) -> samvit [N,256]; saves the activations in `workspace`
 * (samnerf_head_train_workspace_size(N) bytes), which the backward of the
 * same rows reads.  backward: grad_samvit [N,256] -> grad_rows [N,164]
 * (every column written, column 163 -- depth's padding -- as 0), and
 * OVERWRITES grad_w[5] ([256,163], [256,256], [256,419], [256,256],
 * [256,256]), grad_b[5] ([256] each), grad_ln_w, grad_ln_b ([256]); no
 * buffer needs zeroing by the caller.  The weights are the model's sam_w /
 * sam_b / ln_w / ln_b. */
size_t samnerf_head_train_workspace_size(uint32_t N);
int samnerf_head_train_forward(const samnerf_model* model, const float* rows, uint32_t N,
                               float* samvit, void* workspace, size_t workspace_bytes,
                               samnerf_stream_t stream);
int samnerf_head_train_backward(const samnerf_model* model, const float* rows,
                                const float* grad_samvit, uint32_t N, float* grad_rows,
                                float* const* grad_w, float* const* grad_b, float* grad_ln_w,
                                float* grad_ln_b, void* workspace, size_t workspace_bytes,
                                samnerf_stream_t stream);

/* One RGB training step (Trainer.train_step's RGB branch, nerf/utils.py:897-937,
 * over NeRFRenderer.run in train mode, nerf/renderer.py:221-362): the render of
 * N rays (perturbed when model->perturb or perturb_device is set, as the reference trains), the loss
 * MSE(image, gt) + lambda_proposal * proposal_loss (renderer.py:30-57, when
 * update_proposal) + lambda_distort * distort_loss (renderer.py:17-27, the
 * eff_distloss form) + lambda_entropy * entropy(weights_sum) (utils.py:926-929),
 * and its gradient w.r.t. every trained tensor -- what loss.backward() leaves in
 * .grad.  RGB models only (no SAM / mask head, sum_after_mlp off).  fp32.
 *   gt_rgb [N,3] (already composited on the background); image [N,3], depth [N],
 *   weights_sum [N] the render's outputs; loss [5] (device): mse, proposal,
 *   distortion, entropy (the unweighted means) and the total.
 *   Gradients are OVERWRITTEN (zero-filled first); with update_proposal == 0 (or
 *   lambda_proposal == 0) the proposal gradients are not touched and may be NULL
 *   (the reference computes no gradient for them then).
 * Replaces the ~350-op forward and the autograd backward of the torch path. */
typedef struct {
    float lambda_proposal;        /* main.py:106, default 1 */
    float lambda_distort;         /* main.py:108, default 0.02 */
    float lambda_entropy;         /* main.py:100, default 0 */
    int update_proposal;          /* utils.py:912-913 */
    float bg_color;               /* scalar background (1 for 'last_sample'); a set bg_rgb overrides it */
} samnerf_rgb_train_opts;
typedef struct {
    float* grid;                  /* grid.embeddings [rows,2] */
    float* grid_mlp[3];           /* [64,32] [64,64] [16,64] */
    float* view_mlp[3];           /* [32,31] [32,32] [3,32] */
    float* prop[2];               /* prop_encoders.{0,1}.embeddings */
    float* prop_mlp[2][2];        /* [16,10] [1,16] each */
} samnerf_rgb_grads;
/* Workspace for N rays of this model: the saved activations plus 8 per-XCD
 * copies of the leading grid levels' gradient rows (those within 600 K rows), so
 * it depends on the model's table offsets as well as on N. */
size_t samnerf_rgb_train_workspace_size(const samnerf_model* model, uint32_t N);
/* The same step as an autograd pair -- NeRFRenderer.run in train mode under
 * grad (renderer.py:221-362), differentiable outputs image, depth, weights_sum and
 * the render's own losses (proposal_loss when with_proposal, distort_loss), the
 * Trainer's criterion left to the caller:
 *   forward: weights [N,32] (or NULL) = the final samples' weights, results['weights']
 *     of renderer.py:350; losses [2] (device) = (proposal_loss,
 *     distort_loss), unweighted; keeps
 *     what the backward reads in `workspace` (same model, rays, N, perturb arrays
 *     or perturb seed and offset);
 *   backward: grad_image [N,3], grad_weights_sum [N] / grad_depth [N] / grad_weights
 *     [N,32] (NULL = 0), grad_losses [2] (device; NULL = 0, required with
 *     with_proposal) -> the
 *     gradients, OVERWRITTEN as in samnerf_rgb_train_step. */
int samnerf_rgb_train_forward(const samnerf_model* model, const float* rays_o, const float* rays_d,
                              uint32_t N, const float* cam_near_far, uint32_t n_cnf, float bg_color,
                              int with_proposal, float* image, float* depth, float* weights_sum,
                              float* weights, float* losses, void* workspace, size_t workspace_bytes,
                              samnerf_stream_t stream);
int samnerf_rgb_train_backward(const samnerf_model* model, const float* rays_o, const float* rays_d,
                               uint32_t N, float bg_color, int with_proposal, const float* grad_image,
                               const float* grad_weights_sum, const float* grad_depth,
                               const float* grad_weights, const float* grad_losses,
                               const samnerf_rgb_grads* grads, void* workspace, size_t workspace_bytes,
                               samnerf_stream_t stream);
int samnerf_rgb_train_step(const samnerf_model* model, const float* rays_o, const float* rays_d,
                           uint32_t N, const float* cam_near_far, uint32_t n_cnf, const float* gt_rgb,
                           const samnerf_rgb_train_opts* opts, float* image, float* depth,
                           float* weights_sum, float* loss, const samnerf_rgb_grads* grads,
                           void* workspace, size_t workspace_bytes, samnerf_stream_t stream);

/* Transport record of the per-ray outputs for the all-gather of a
 * ray-sharded view (samnerf_amd/dist.py; no reference counterpart: the
 * reference renders on one GPU, nerf/renderer.py:185-219).  One record of
 * samnerf_tile_words() 32-bit words per ray: image[3], depth, weights_sum
 * (fp32, exact), a power-of-two scale s and samvit[256] as int16 q = rint(v/s)
 * (|v - q s| <= 2^-14 of the ray's max |samvit|; NaN / inf rays decode to NaN).
 * samvit must be 16-B aligned, tile 8-B aligned; N = 0 is a no-op. */
uint32_t samnerf_tile_words(void);
int samnerf_tile_encode(const float* image, const float* depth, const float* weights_sum,
                        const float* samvit, uint32_t N, void* tile, samnerf_stream_t stream);
int samnerf_tile_decode(const void* tile, uint32_t N, float* image, float* depth,
                        float* weights_sum, float* samvit, samnerf_stream_t stream);

/* Parity taps (tests only; no reference counterpart -- they expose what
 * nerf/renderer.py:261-326 and network.py:221-259 compute between its ops).
 * While set, every samnerf_render_forward call of this thread over exactly N
 * rays writes the stages' intermediates to these device buffers as well (the
 * same kernels run, with one predicated store per tapped value; outputs are
 * unchanged; rays are not regrouped into pixel tiles), sample-major:
 *   ds0 [128][N], ds1 [64][N]   optical depth delta * sigma of each proposal
 *                               sample (renderer.py:310-311)
 *   w0 [128][N], w1 [64][N]     their composited weights (renderer.py:312-326),
 *                               the input of sample_pdf
 *   bins1 [65][N], bins2 [33][N]  the resampled bins of sample_pdf
 *                               (renderer.py:274-275)
 *   inds1 [65][N], inds2 [33][N]  its torch.searchsorted(cdf, u, right=True)
 *                               indices (renderer.py:105), int32
 *   sigma2 [32][N]              the final stage's sigma = trunc_exp(density)
 *                               of every sample (network.py:227, k_final)
 *   w2 [32][N]                  the final stage's composited weights
 *                               (renderer.py:312-326)
 *   u2 [32][3][N]               the final samples' grid-space positions
 *                               (contract(xyz) + bound) / (2 bound), grid.py:156
 *   rows2, srows [ceil(N / row_stride)][32][16][8]  uint32, for the rays
 *                               r % row_stride == 0: the level-relative corner
 *                               row each trilinear weight multiplies, per final
 *                               sample, level and corner (bit 0 x, 1 y, 2 z, as
 *                               gridencoder.cu:61-79): rows2 those of k_final's
 *                               grid gathers, srows those of the s_grid
 *                               composite (k_sgrid_box4, N >= 32768 only;
 *                               samples whose weight is 0 on all 64 rays of a
 *                               wave are skipped and left unwritten)
 * Any pointer may be NULL.  taps = NULL clears them; a render over another
 * ray count fails with SAMNERF_EINVAL while they are set.  Thread-local. */
typedef struct {
    float* ds0;
    float* ds1;
    float* w0;
    float* w1;
    float* bins1;
    float* bins2;
    int32_t* inds1;
    int32_t* inds2;
    float* sigma2;
    float* w2;
    float* u2;
    uint32_t row_stride;
    uint32_t* rows2;
    uint32_t* srows;
} samnerf_taps;
int samnerf_set_taps(const samnerf_taps* taps, uint32_t N);

/* Measurement hook (bench.py): when set, samnerf_render_forward records
 * events[i] (hipEvent_t) on its stream before stage i (0 prop0, 1 prop1,
 * 2 final, 3 s_grid, 4 SAM head) and events[5] after the last one.  n = 0 or
 * events = NULL disables it.  Thread-local; costs one hipEventRecord per stage. */
int samnerf_set_stage_events(void* const* events, uint32_t n);

/* Test hook: the compiled kernel forms the last samnerf_render_forward(_tile)
 * of this thread launched, so the tests can tell which specialisation ran.
 * out[0] / out[1]: the proposal stages' level classes (dense-level mask |
 * hashed-level mask << 8) when k_prop_sigma ran with them as compile-time
 * constants, 0 for the run-time form; out[2]: k_final's layout (1 = the
 * reference grid's compile-time slot layout, 0 = run-time); out[3] reserved.
 * Writes min(n, 4) entries, returns 4.  Thread-local, no GPU work. */
int samnerf_last_forms(uint32_t* out, uint32_t n);

/* Measurement hook (bench.py): one stamp of the shader clock on `stream`,
 * from 256 single-wave workgroups (every XCD): out[3 * b + 0] = XCC id,
 * out[3 * b + 1] = s_memtime (shader-clock ticks), out[3 * b + 2] =
 * s_memrealtime (100 MHz) of workgroup b; out holds 768 uint64.  Two stamps
 * around the timed views give the clock they ran at per XCD:
 * d(memtime) / d(memrealtime) x 100 MHz.  Costs one ~5-us launch. */
int samnerf_clock_stamp(uint64_t* out, samnerf_stream_t stream);

/* ------------------------------------------------------------- mask loss --
 * The loss of Trainer.train_step's --with_mask branch (nerf/utils.py:959-1067)
 * and its gradient to the logits, in fp32 and in fixed-order sums (no float
 * atomics; the same inputs give the same bits whatever ran before).
 * logits [N,K], K = n_inst + redundant_instance in [2, 32]; the first n rays are
 * the global rays (opt.num_rays), the rest L local patches of Q pixels.
 *   NLL (always): mean over the global rays of -log clamp(softmax(z))[label],
 *     0 if no ray of all N is labelled (label != -1); with incoherent_weight
 *     u < 1 times the mean over all N rays of 1 - m + u * m (the reference's
 *     [n,1] x [N] broadcast, utils.py:979).
 *   error map (error_map != NULL): map[c_i] <- 0.1 map[c_i] + 0.9 exp(-a cos(p_i,
 *     onehot(label_i)) - epsilon) for the global rays, every old value read
 *     before any is written, the last ray in ray order winning a shared cell
 *     (utils.py:981-1017).  error_cells [n] are flat cells of the map.
 *   label regularisation (label_reg_weight > 0, utils.py:843-870): over all N
 *     rays as P x P patches of the softmax and depth; P >= 2, N % (P * P) == 0.
 *   RGB similarity (rgb_weight > 0, utils.py:761-841 under :1034-1059): per
 *     local patch, S samples sample_index [L,S] against its Q pixels of image
 *     [N,3]; redundant != 0: the binary-cross-entropy form; use_pred_logistics:
 *     the sample's softmax instead of its arg-max one-hot.  N == n + L * Q,
 *     Q * K <= 8192, Q <= 1024, S <= min(Q, 256).
 * The caller applies the reference's step condition (utils.py:1033) by leaving
 * rgb_weight 0.  A label outside [0,K) among the global rays, a sample outside
 * [0,Q) or a cell outside [0,map_cells) is never used as an index: that ray or
 * sample contributes nothing and is counted in loss_terms[4]. */
typedef struct {
    uint32_t N, K, n;
    uint32_t L, Q, S;              /* RGB similarity; 0 when off */
    uint32_t P;                    /* label regularisation patch side */
    int32_t redundant;
    int32_t use_pred_logistics;
    float incoherent_weight;       /* u; >= 1: no re-weighting */
    float label_reg_weight;
    float rgb_weight;
    float rgb_threshold;
    float rgb_exp_weight;          /* a (also the error map's) */
    double epsilon;                /* the clamp is [epsilon, 1 - epsilon], each rounded to float */
    uint64_t map_cells;
    const int64_t* labels;         /* [N], -1 = unlabelled */
    const float* incoherent;       /* [N]; read when incoherent_weight < 1 */
    float* error_map;              /* [map_cells], updated in place; NULL = off */
    const int64_t* error_cells;    /* [n] */
    const float* depth;            /* [N]; read when label_reg_weight > 0 */
    const float* image;            /* [N,3]; read when rgb_weight > 0 */
    const int64_t* sample_index;   /* [L,S]; read when rgb_weight > 0 */
} samnerf_mask_loss_args;

/* Bytes of workspace samnerf_mask_loss needs for these sizes (0 for invalid ones). */
size_t samnerf_mask_loss_workspace_size(const samnerf_mask_loss_args* args);

/* loss_terms [5]: NLL, label regularisation, RGB similarity (each unweighted),
 * their weighted total (utils.py:1026-1059) and the count of invalid inputs;
 * grad_logits [N,K] = d total / d logits (written, not accumulated); pred_ids
 * [N] int64 = argmax of the softmax, the first index winning ties.
 * SAMNERF_EINVAL: a null pointer, K outside [2, 32] or inconsistent sizes;
 * SAMNERF_EWORKSPACE: ws NULL or ws_bytes too small. */
int samnerf_mask_loss(const samnerf_mask_loss_args* args, const float* logits, float* loss_terms,
                      float* grad_logits, int64_t* pred_ids, void* ws, size_t ws_bytes,
                      samnerf_stream_t stream);

/* --------------------------------------------------------- batch sampler --
 * A training step's input: the N > 0 branches of the reference's get_rays
 * (nerf/utils.py:174-242) choose the pixels, and its collate
 * (nerf/colmap_provider.py:1084-1175) gathers the ground truth at them.  All
 * pointers are device pointers unless named _host.
 *
 * The tables of a dataset; any but poses / intrinsics may be NULL. */
typedef struct {
    const float* poses;            /* [n_img,4,4] cam2world */
    const float* intrinsics;       /* [n_intr,4] fx, fy, cx, cy; n_intr = n_img or 1 */
    uint32_t n_img, n_intr;
    uint32_t H, W;                 /* of images and masks; H also scales the map reads */
    const void* images;            /* [n_img,H,W,C] uint8, or float32 when images_float */
    uint32_t C;                    /* 1..4 */
    int32_t images_float;
    const int64_t* masks;          /* [n_img,H,W] instance labels */
    const void* incoherent_masks;  /* [n_img, incoherent_size^2], 1-byte (bool / uint8) or float32 cells */
    uint32_t incoherent_bytes;     /* 1 or 4 */
    uint32_t incoherent_size;
    const float* error_map;        /* [n_img, error_size^2] */
    uint32_t error_size;
    const float* cam_near_far;     /* [n_img,2] */
} samnerf_batch_source;

/* What the gather writes for n rays; a NULL output, or one whose table is
 * NULL, is not written. */
typedef struct {
    float* rays_o;                 /* [n,3] */
    float* rays_d;                 /* [n,3] */
    int64_t* i;                    /* [n] column */
    int64_t* j;                    /* [n] row */
    int64_t* inds_coarse;          /* [n] */
    float* images;                 /* [n,C] = pixel / 255 */
    int64_t* masks;                /* [n] */
    void* incoherent_masks;        /* [n], the table's cell type */
    float* error_maps;             /* [n] */
    float* cam_near_far;           /* [n,2] */
} samnerf_batch_out;

/* k_batch_gather, one launch: ray t is pixel pixels[t] = row * W + col of image
 * index[n_index == 1 ? 0 : t] (n_index = 1 or n), in an H x W ray image (the
 * tables' size, or the fixed-fov size of colmap_provider.py:1009-1015, which
 * must not exceed it).
 *   rays_o, rays_d  utils.py:247-259 in its op order: ((col + 0.5) - cx) / fx,
 *                   -((row + 0.5) - cy) / fy, -1, times R^T (a product and two
 *                   fmas per component), true divisions; pose and intrinsics
 *                   read per ray
 *   inds_coarse     utils.py:269-275 with incoherent_mask_size = coarse_size:
 *                   (long)(row * (float)(coarse_size / H)) * coarse_size +
 *                   (long)(col * (float)(coarse_size / W)), products in
 *                   float32; coarse_size = 0: not written
 *   images          colmap_provider.py:1086, (float)pixel / 255, a true division
 *   incoherent_masks, error_maps   colmap_provider.py:1116-1158: the cell
 *                   (long)(row * s) * S + (long)(col * s), s = (float)(S / H)
 *                   for rows AND columns as the reference has it; a cell past
 *                   the map (W > H) is not read and its output not written
 * A ray whose image or pixel is out of range writes nothing.
 * SAMNERF_EINVAL: a null pointer, n_index not 1 or n, H x W beyond the tables. */
int samnerf_batch_gather(const samnerf_batch_source* src, const int64_t* index, uint32_t n_index,
                         const int64_t* pixels, uint32_t n, uint32_t H, uint32_t W, uint32_t coarse_size,
                         const samnerf_batch_out* out, samnerf_stream_t stream);

/* The pixel choice.  Every mode takes its raw draws either from arrays (seeded
 * = 0: the reference's torch stream, or samnerf_batch_draw_fill's replay) or
 * from Philox4x32-10 under (seed, offset) (seeded = 1).  Statistically the
 * reference's sampling, NOT torch's generator stream.  The seeded contract,
 * exact to the bit (generator and key as samnerf_model.perturb_device's):
 *   counters   the perturb stages use c0 >> 16 = 0, 1, 2; these use 3..7, so a
 *              (seed, offset) shared with a render reuses none of its words.
 *              Item t (a ray, a patch or a map row, below): c0 = 3 << 16, c1 =
 *              t; cell c of map row b: c0 = (4 << 16) + (c >> 2), c1 = b, the
 *              cell's word is output word c & 3 (c < 2^20).  c2, c3 = offset.
 *   integer    in [0, R): (uint64(word) * R) >> 32; its bias is at most R / 2^32
 *   item t     word 0 -> first integer, word 1 -> second integer, words 2, 3 ->
 *              uniforms r = (word >> 8) * 2^-24 in [0, 1) (torch.rand's range)
 *   key        of a cell of weight w: w / e, e = -log(u), u = ((word >> 8) +
 *              0.5) * 2^-24, never 0 or 1 (for word >> 8 >= 2^23, where fp32 no
 *              longer holds u, e = -log1p(-(1 - u)) with 1 - u exact); a
 *              weight that is not positive and finite has key 0, one that is a
 *              key of at least the smallest subnormal.  fp32, the device's logf
 *              and log1pf: keys exist only on the device (the fill below).
 * Modes (n = rays for R and E, patches for P, map rows for C):
 *   SAMNERF_BATCH_UNIFORM (R)  utils.py:234-236 with colmap_provider.py:975 /
 *       :978.  Item = ray: index = integer(n_img), pixel = integer(H * W).
 *       Arrays: int0 = images, int1 = pixels [n].
 *   SAMNERF_BATCH_PATCHES (P)  utils.py:196-219.  Item = patch: corner row =
 *       integer(H - p), col = integer(W - p); pixels [n * p * p], patch after
 *       patch, pixel k of a patch at (row + k / p, col + k % p).  Arrays: int0 =
 *       corner rows, int1 = corner cols [n].
 *   SAMNERF_BATCH_CENTRED (C)  utils.py:180-194, :206-219; the local draws of
 *       mixed sampling, colmap_provider.py:1049-1070.  Map row b is the M x M
 *       weights of image rows[b]; rows = NULL (seeded only): item = map row,
 *       image = integer(n_img).  The centre is the cell of largest key, the
 *       lower cell winning a tie: for one draw, exactly proportional to the
 *       weights.  corner = (long)clamp(c / M * (float)(H / M) - p / 2, 0, H - p
 *       - 1) in float32 (likewise the column); pixels and index [n * p * p],
 *       cells [n] (the centres, may be NULL).  Arrays: keys [n, M * M].  M <=
 *       1024, 1 <= p < min(H, W).
 *   SAMNERF_BATCH_ERROR (E)  utils.py:222-233.  The n cells of largest key of
 *       the map of image rows[0] -- weighted sampling without replacement, the
 *       exponential-key scheme torch.multinomial uses -- ties to the lower
 *       cell, written in ascending cell order to cells [n]; pixel of slot k =
 *       min((long)(cell_row * sx + r0 * sx), H - 1) * W + likewise the column,
 *       sx = (float)(H / M), item = slot k.  M = 128 only (the reference
 *       divides by a literal 128), n <= 16384.  Arrays: keys [M * M] (16-byte
 *       aligned), u0, u1 [n].
 * Precondition of C and E: the row holds at least n (C: one) positive finite
 * weights.  Otherwise cells of weight 0 are chosen, lowest first; nothing is
 * read or written out of bounds. */
enum {
    SAMNERF_BATCH_UNIFORM = 0,
    SAMNERF_BATCH_PATCHES = 1,
    SAMNERF_BATCH_CENTRED = 2,
    SAMNERF_BATCH_ERROR = 3
};

typedef struct {
    int32_t mode;
    int32_t seeded;
    uint64_t seed, offset;
    uint32_t n_img, H, W;
    uint32_t n;
    uint32_t patch;                /* P, C */
    uint32_t M;                    /* C, E */
    const void* weights;           /* C, E seeded: [n_img, M * M] */
    uint32_t weight_bytes;         /* 4: float32; 1: bool / uint8 */
    const int64_t* rows;           /* C: [n] or NULL; E: [1] */
    const int64_t* int0;           /* the array form's draws, per mode above */
    const int64_t* int1;
    const float* keys;
    const float* u0;
    const float* u1;
    int64_t* index;                /* R: [n]; C: [n * p * p] or NULL */
    int64_t* pixels;
    int64_t* cells;                /* C: [n] or NULL; E: [n] */
} samnerf_batch_draw_args;

int samnerf_batch_draw(const samnerf_batch_draw_args* args, samnerf_stream_t stream);

/* The raw draws of a (seed, offset) as arrays, to log or replay a step:
 * samnerf_batch_draw with seeded = 0 fed these equals seeded = 1 bit for bit.
 * int0, int1 [items]: the two integers of every item under range0, range1; u0,
 * u1 [items]: its uniforms; keys [B, cells]: the keys of map rows 0..B-1 over
 * weights [n_img, cells], row b being image rows[b] or, rows = NULL, the first
 * integer of item b under n_img.  Any output may be NULL. */
int samnerf_batch_draw_fill(uint64_t seed, uint64_t offset, uint32_t items, uint32_t range0, uint32_t range1,
                            int64_t* int0, int64_t* int1, float* u0, float* u1, const void* weights,
                            uint32_t weight_bytes, uint32_t n_img, const int64_t* rows, uint32_t B,
                            uint32_t cells, float* keys, samnerf_stream_t stream);

/* Host only, no GPU needed: the integers (ints_host[2], under range0 and
 * range1) and uniforms (uniforms_host[2]) of item `item`.  They use no libm, so
 * host and device agree exactly. */
int samnerf_batch_draw_host(uint64_t seed, uint64_t offset, uint32_t item, uint32_t range0, uint32_t range1,
                            int64_t* ints_host, float* uniforms_host);

/* ----------------------------------------------------- frame presentation --
 * From a render's outputs to the GUI's display buffer: what Trainer.test_step
 * (nerf/utils.py:1263-1306, :1396-1399), Trainer.test_gui (:1698-1702) and
 * NeRFGUI.prepare_buffer / test_step (nerf/gui.py:134-140, :171-177) do after
 * the render, in fp32 with every product and sum rounded on its own, in the
 * reference's op order.  No model: it works on any render's outputs.  In order:
 *   1. logits [rH*rW, K] (K = n_inst + redundant_instance in [1, 32]; K = 0: no
 *      mask view): the instance row.  n_inst > 1 the softmax over the K columns
 *      (max, expf(z - max), the sum as a 32-lane tree, expf(z - max) / sum),
 *      n_inst == 1 the sigmoid 1 / (1 + expf(-z)); then the largest probability
 *      and its index, the first index winning ties.  samnerf_mask_loss,
 *      samnerf_eval_frame and samnerf_incoherent_ids run this same row (one
 *      device function, csrc/instance_row.h), so their probabilities and ids
 *      agree bit for bit;
 *   2. the colour.  render id = instance_id if 0 <= instance_id < n_inst, else -1.
 *      HEATMAP: color_map[id] * p[id], or color_map[argmax] * max at id -1;
 *      COMPOSITION: image * 0.7f + c * 0.3f with c = color_map[argmax], or c = image
 *      where an id is set and argmax != id (image * 0.7f + image * 0.3f, which is
 *      not image); MASK: color_map[argmax] at id -1, else color_map[id] where
 *      argmax == id and 0 elsewhere.  K = 0: the rendered image;
 *   3. sam_mask [rH*rW] bytes: frame * 0.7f + o * 0.3f with o = (1, 0, 0) where the
 *      byte is set and o = frame elsewhere (overlay_mask blends every pixel);
 *   4. points [n_points, 2] int32 (x, y), n_points <= 64: rows [y - 2, y + 2) and
 *      columns [x - 2, x + 2) become (0, 1, 0) under Python's slice rules, as the
 *      reference's indexing applies them: an end past the image is clipped, a
 *      negative start wraps round to the far edge, so a click within 2 pixels of
 *      the top or left edge selects an empty range and draws nothing;
 *   5. nearest resize of frame and depth from rH x rW to H x W, ATen's rule:
 *      src = min(floor(dst * (float)in / out), in - 1), the scale in fp32;
 *   6. the buffer [H*W, 3].  SAMNERF_PRESENT_IMAGE: the frame.  _DEPTH:
 *      (d - min) / (max - min + 1e-6f) on all three channels, min and max over
 *      the resized depth; a NaN anywhere makes every value NaN (numpy's min /
 *      max).  spp == 0: written; else (buffer * spp + new) / (spp + 1), spp as
 *      fp32;
 *   7. the side outputs, each optional: probs [rH*rW, K], ids [rH*rW] (the argmax),
 *      depth_out [H*W] (the resized depth).
 * The same inputs give the same bits: no float atomics, min and max are
 * order-free. */
enum { SAMNERF_PRESENT_HEATMAP = 0, SAMNERF_PRESENT_COMPOSITION = 1, SAMNERF_PRESENT_MASK = 2 };
enum { SAMNERF_PRESENT_IMAGE = 0, SAMNERF_PRESENT_DEPTH = 1 };
#define SAMNERF_PRESENT_MAX_POINTS 64

typedef struct {
    uint32_t rH, rW;               /* the render's size */
    uint32_t H, W;                 /* the buffer's size */
    uint32_t K, n_inst;            /* K = 0: no logits */
    uint32_t n_colors;             /* rows of color_map; >= K */
    uint32_t n_points;
    uint32_t spp;                  /* frames already in the buffer */
    int32_t mask_type;             /* SAMNERF_PRESENT_HEATMAP / _COMPOSITION / _MASK */
    int32_t instance_id;           /* opt.render_mask_instance_id */
    int32_t mode;                  /* SAMNERF_PRESENT_IMAGE / _DEPTH */
    const float* image;            /* [rH*rW,3]; read at K = 0 and by COMPOSITION */
    const float* depth;            /* [rH*rW]; read by _DEPTH and for depth_out */
    const float* logits;           /* [rH*rW,K] */
    const float* color_map;        /* [n_colors,3] */
    const uint8_t* sam_mask;       /* [rH*rW], NULL = off */
    const int32_t* points;         /* [n_points,2] */
    float* buffer;                 /* [H*W,3]; read as well when spp > 0 */
    float* probs;                  /* [rH*rW,K] or NULL */
    int64_t* ids;                  /* [rH*rW] or NULL */
    float* depth_out;              /* [H*W] or NULL */
} samnerf_present_args;

/* Bytes of workspace samnerf_present_frame needs (0 for invalid arguments, and
 * for an image buffer at the render's own size, which takes one pass). */
size_t samnerf_present_workspace_size(const samnerf_present_args* args);

/* SAMNERF_EINVAL: a null pointer the mode needs, K outside [0, 32], n_inst
 * outside [1, K], a color_map shorter than K rows (an argmax may reach past
 * n_inst: redundant instances have colours too) or than the render id,
 * n_points > 64, an unknown mask_type or mode, a size of 0 or of 2^31 values or
 * more; SAMNERF_EWORKSPACE: workspace NULL or too small where one is needed. */
int samnerf_present_frame(const samnerf_present_args* args, void* workspace, size_t workspace_bytes,
                          samnerf_stream_t stream);

/* ------------------------------------------------------------- evaluation --
 * What Trainer.eval_step (nerf/utils.py:1122-1241) and the meters of
 * evaluate_one_epoch (PSNRMeter, SSIMMeter, MeanIoUMeter, utils.py:329-512,
 * :1945-2000) compute from one evaluated view, as raw sums and counts in one
 * stats record in device memory.  Nothing is copied to the host and nothing
 * synchronises; the finished scalars (loss, PSNR, SSIM, mIoU) are the host's,
 * in float64, from one copy of the records.  A record is a samnerf_eval_stats
 * followed by three histograms of n_classes uint32 each (inter, npred,
 * ntruth): SAMNERF_EVAL_STATS_BYTES(n_classes) bytes, 8-byte aligned.  Every
 * call writes the whole record.  Each part is optional:
 *   RGB (C = 3 or 4): truth [H*W,C]; at C = 4 the composite t = rgb * a +
 *     bg_color * (1 - a), every product and sum rounded to fp32.  sq_sum = the
 *     sum over H*W*3 of the fp32 (p - t)^2, n_elem = H*W*3, min and max of the
 *     prediction and of t (a NaN is skipped).  pred_u8 / truth_u8 [H*W,3]:
 *     (uint8)(v * 255.0f), truncated (v in [0, 1]); error_u8 [H*W]: the fp32
 *     ((|t0 - p0| + |t1 - p1|) + |t2 - p2|) / 3 of those bytes, truncated;
 *     truth_out [H*W,3]: t.
 *   SSIM (ssim != 0, needs the RGB part and H, W >= 11): the 11-tap Gaussian
 *     window of sigma 1.5, g[i] = exp(-((i - 5) / 1.5)^2 / 2) / sum as fp32 values
 *     (a table: the double evaluation rounded once), applied as a row pass and
 *     a column pass of fp32 FMAs, over
 *     the (H - 10) * (W - 10) * 3 windows wholly inside the image (what
 *     torchmetrics' reflection padding and crop leave); c1 = (0.01f * L)^2,
 *     c2 = (0.03f * L)^2, L = max(pred_max - pred_min, truth_max - truth_min)
 *     read from the record; ssim_sum = the sum of ((2 E[p] E[t] + c1)(2 s_pt +
 *     c2)) / ((E[p]^2 + E[t]^2 + c1)(s_p + s_t + c2)), n_ssim the count.
 *   mask (K in [1, 64], n_inst in [1, K]): logits [H*W,K], labels [H*W] int64
 *     with -1 = unlabeled.  Probabilities and argmax: the instance row of
 *     samnerf_present_frame (step 1), with a second tree for columns 32.. added
 *     to the first where K > 32.  nll_sum = the sum over labeled
 *     pixels of -logf(min(max(p[label], (float)epsilon), (float)(1 - epsilon))),
 *     n_labeled their count.  inter[i] = #(argmax == i and label == i),
 *     npred[i] = #(argmax == i), ntruth[i] = #(label == i) for i < n_classes
 *     (<= 1024); a negative label matches no class.  overflow counts labels
 *     outside [-1, K) and ids or labels >= n_classes: none is used as an index.
 *     probs [H*W,K] and ids [H*W] are optional outputs.
 *   SAM (h, w > 0): pred_feat [h*w,256] in the render's layout and gt_feat
 *     [256,h*w], both read in place: feat_sq_sum = the sum of the fp32
 *     (p - g)^2, n_feat = h*w*256.
 * Every floating sum is in a fixed order: double partials per workgroup in the
 * workspace, added in index order by one thread.  The histograms use integer
 * atomics.  The same inputs give the same bits. */
typedef struct {
    double sq_sum;      uint64_t n_elem;
    double nll_sum;     uint64_t n_labeled;
    double ssim_sum;    uint64_t n_ssim;
    double feat_sq_sum; uint64_t n_feat;
    float pred_min, pred_max, truth_min, truth_max;
    uint64_t overflow;
    uint64_t reserved[5];
} samnerf_eval_stats;              /* 128 bytes; uint32 hist[3][n_classes] follows */
#define SAMNERF_EVAL_STATS_BYTES(n_classes) (128u + (((size_t)(n_classes) * 12u + 7u) & ~(size_t)7u))
#define SAMNERF_EVAL_MAX_CLASSES 1024
#define SAMNERF_EVAL_MAX_K 64

typedef struct {
    uint32_t H, W;                 /* the view; H*W pixels of the RGB and mask parts */
    uint32_t C;                    /* channels of truth: 3 or 4; 0 = no RGB part */
    uint32_t ssim;                 /* nonzero: the SSIM sum as well */
    uint32_t K, n_inst;            /* K = 0: no mask part */
    uint32_t n_classes;            /* bins of each histogram */
    uint32_t h, w;                 /* the feature map; 0 = no SAM part */
    float bg_color;
    double epsilon;                /* opt.epsilon */
    const float* pred_rgb;         /* [H*W,3] */
    const float* truth;            /* [H*W,C] */
    const float* logits;           /* [H*W,K] */
    const int64_t* labels;         /* [H*W] */
    const float* pred_feat;        /* [h*w,256] */
    const float* gt_feat;          /* [256,h*w] */
    uint8_t* pred_u8;              /* [H*W,3] or NULL */
    uint8_t* truth_u8;             /* [H*W,3] or NULL */
    uint8_t* error_u8;             /* [H*W] or NULL */
    float* truth_out;              /* [H*W,3] or NULL */
    float* probs;                  /* [H*W,K] or NULL */
    int64_t* ids;                  /* [H*W] or NULL */
    void* stats;                   /* the record: SAMNERF_EVAL_STATS_BYTES(n_classes) */
    void* workspace;
    size_t workspace_bytes;
} samnerf_eval_args;

/* *bytes: the workspace one call needs (the partial sums). */
int samnerf_eval_workspace_size(const samnerf_eval_args* args, size_t* bytes);

/* SAMNERF_EINVAL: no part asked for, a null pointer a part needs, C outside
 * {0, 3, 4}, ssim without the RGB part or with H or W below 11, K above 64,
 * n_inst outside [1, K], n_classes outside [1, 1024] with a mask part, a size of
 * 2^31 values or more, stats not 8-byte aligned; SAMNERF_EWORKSPACE. */
int samnerf_eval_frame(const samnerf_eval_args* args, samnerf_stream_t stream);

/* The three histograms and the overflow count alone, from ready-made id maps
 * (MeanIoUMeter.update): pred_ids, truth_ids [n] int64, stats a record as
 * above, written whole. */
int samnerf_eval_confusion(const int64_t* pred_ids, const int64_t* truth_ids, uint32_t n, uint32_t n_classes,
                           void* stats, samnerf_stream_t stream);

/* ------------------------------------------------------ incoherent masks --
 * The incoherent-region table of --with_mask training ([n_img, cells] bool: the
 * sampler's local patches are drawn from it and the loss weights its rays by
 * it).  The reference builds it from the ground-truth masks at load
 * (colmap_provider.py:798-801) and, under --use_dynamic_incoherent, from the
 * mask head's own renders (Trainer.update_incoherent_mask, nerf/utils.py:1757-
 * 1780).  Two entry points, no model, no workspace, nothing on the host:
 *
 * samnerf_incoherent_ids: render_mask (utils.py:1716-1737) and the argmax of
 * update_incoherent_mask, per ray.  logits [N, K], K = n_inst +
 * redundant_instance in [1, 32].  n_inst > 1: the softmax of the instance row
 * (samnerf_present_frame, step 1),
 * pred = [p[0] + .. + p[K-2] by the same tree, p[K-1]], and the id is
 * argmax(pred): 1 where pred[1] > pred[0], else 0 -- a tie gives 0, and so does
 * a NaN or infinite logit (every probability is then NaN).  n_inst == 1 (K ==
 * 1): the id is 0 (an argmax over one column) and pred = [sigmoid(z)].
 * ids [N] bytes; pred_mask [N, 2] ([N, 1] at n_inst == 1) fp32, optional.
 *
 * samnerf_incoherent_masks: get_incoherent_mask (utils.py:283-298) for n views
 * in one launch.  masks [n, H, W]: int64 (the dataset's [n,H,W,1]) or the bytes
 * of samnerf_incoherent_ids; values in [0, 2^14).  In fp32: bilinear down to
 * (H / sfact, W / sfact), bilinear back up, |mask - recovered|, bilinear down
 * again, cells >= 0.01f set to 1, and with keep_size nearest up to (H, W); the
 * resizes are ATen's with align_corners = false: source index
 * max(scale * (dst + 0.5) - 0.5, 0), upper neighbour clamped at the border;
 * nearest min(floor(dst * scale), in - 1).  uncertain: that float map; table:
 * 1 byte per cell, uncertain != 0 (the reference's .to(torch.bool): a residue
 * below 0.01 that is not zero is True).  Both [n, H * W] with keep_size, else
 * [n, (H / sfact) * (W / sfact)]; either may be NULL, not both.
 * H and W must be divisible by sfact, a power of two: every product and sum is
 * then exact in fp32, and the result equals the reference's on any device bit
 * for bit.  At other sizes the reference's bool is the rounding residue of
 * ATen's own kernels, which no other kernel reproduces: SAMNERF_EINVAL.  A
 * workgroup takes SAMNERF_INCOHERENT_TILE^2 coarse cells of one view. */
enum { SAMNERF_INCOHERENT_INT64 = 0, SAMNERF_INCOHERENT_UINT8 = 1 };
#define SAMNERF_INCOHERENT_TILE 16

typedef struct {
    uint32_t N, K, n_inst;
    const float* logits;           /* [N,K] */
    uint8_t* ids;                  /* [N] */
    float* pred_mask;              /* [N,2], [N,1] at n_inst == 1, or NULL */
} samnerf_incoherent_ids_args;

/* SAMNERF_EINVAL: null args, logits or ids, K outside [1, 32], n_inst outside
 * [1, K], n_inst == 1 with K > 1.  N == 0 is a successful no-op. */
int samnerf_incoherent_ids(const samnerf_incoherent_ids_args* args, samnerf_stream_t stream);

typedef struct {
    uint32_t n, H, W;              /* views and their size */
    uint32_t sfact;                /* a power of two dividing H and W */
    int32_t keep_size;             /* nonzero: outputs at H x W */
    int32_t input_type;            /* SAMNERF_INCOHERENT_INT64 / _UINT8 */
    const void* masks;             /* [n,H,W] */
    uint8_t* table;                /* [n, cells] or NULL */
    float* uncertain;              /* [n, cells] or NULL */
} samnerf_incoherent_masks_args;

/* SAMNERF_EINVAL: null args or masks, table and uncertain both NULL, sfact not
 * a power of two, H or W not divisible by sfact, H / sfact or W / sfact == 0,
 * H * W of 2^31 or more, an unknown input_type.  n == 0 is a successful no-op. */
int samnerf_incoherent_masks(const samnerf_incoherent_masks_args* args, samnerf_stream_t stream);

/* ---------------------------------------------------- distillation loss --
 * The loss of Trainer.train_step's SAM-feature branch (nerf/utils.py:1094-1108):
 * the rendered features pred [h*w][256] (ray-major, the render's samvit, 256
 * wide as everywhere in this library) resized to the teacher's map gt
 * [256][Hg][Wg], and their mean squared error.  Every size lies in [1, 1024].
 *
 * The resize is F.interpolate(mode='bilinear') with align_corners=False and no
 * antialiasing.  The taps of destination cell d of an axis of n_in source and
 * n_out destination cells are formed in fp32, in one place that the kernels
 * and samnerf_bilinear_taps_host share:
 *     scale = (float)n_in / n_out
 *     src   = max(scale * (d + 0.5f) - 0.5f, 0)
 *     i0 = (int)src,  i1 = i0 + (i0 < n_in - 1),  l1 = src - i0,  l0 = 1 - l1
 * and a cell is  l0y * (l0x * v00 + l1x * v01) + l1y * (l0x * v10 + l1x * v11).
 * These taps are this library's definition: ATen's own weights differ from
 * them in the last bit at some size pairs, so results are compared with a
 * float64 evaluation within a tolerance, never with torch for equality.
 *
 * loss = the mean over the 256 * Hg * Wg cells of (resized - gt)^2;
 * grad_pred = grad_loss * d loss / d pred (resized carries no gradient).
 * Nothing is copied to the host and nothing synchronises: the calls can be
 * captured in a graph.  The forward leaves the per-axis taps, each source
 * cell's run of destination cells and the scaled differences [Hg*Wg][256] in
 * ws; the backward reads only ws and grad_loss, so it follows a forward with
 * the same sizes and the same ws.
 *
 * Repeatable to the bit: no float atomics.  The loss is workgroup partials
 * added in a fixed order; the backward is a gather in which every source cell
 * adds its destination cells' differences row by row, column by column.  A
 * source cell that no destination cell touches (6 of 16 columns at 16 -> 5)
 * gets exactly 0.0f.  Non-finite inputs reach the loss as NaN or Inf; no
 * cell-by-cell promise is made for them.
 *
 * SAMNERF_EINVAL: a size outside [1, 1024], a null pointer other than resized,
 * pred / grad_pred / ws not 16-byte aligned; SAMNERF_EWORKSPACE: ws_bytes
 * below the workspace size. */

/* Bytes of workspace for these sizes (0 for invalid ones). */
size_t samnerf_feat_loss_workspace_size(uint32_t h, uint32_t w, uint32_t Hg, uint32_t Wg);

/* resized [256][Hg][Wg] or NULL; loss: 1 device float. */
int samnerf_feat_loss_forward(const float* pred, uint32_t h, uint32_t w, const float* gt, uint32_t Hg,
                              uint32_t Wg, float* resized, float* loss, void* ws, size_t ws_bytes,
                              samnerf_stream_t stream);

/* grad_loss: 1 device float; grad_pred [h*w][256] is overwritten. */
int samnerf_feat_loss_backward(const float* grad_loss, uint32_t h, uint32_t w, uint32_t Hg, uint32_t Wg,
                               float* grad_pred, void* ws, size_t ws_bytes, samnerf_stream_t stream);

/* The taps of one axis on the host (no GPU): i0, i1, l1 [n_out].
 * SAMNERF_EINVAL: a size outside [1, 1024] or a null pointer. */
int samnerf_bilinear_taps_host(uint32_t n_in, uint32_t n_out, uint32_t* i0, uint32_t* i1, float* l1);

/* -------------------------------------------------------- teacher image --
 * The SAM teacher's input from a render in device memory: what the reference
 * does on the host between the full-resolution render and image_encoder
 * (nerf/utils.py:1083-1085, :1203-1208; SamPredictor.set_image):
 *     (pred_rgb.cpu().numpy() * 255).astype(uint8)
 *     ResizeLongestSide(target).apply_image     PIL's 8-bit bilinear resize
 *     Sam.preprocess                             (x - mean) / std, zero padding
 * The bits are the contract: out_u8 equals PIL's Image.resize(BILINEAR) of the
 * quantised render byte for byte, out_input equals the torch ops on it.
 *
 * Size (samnerf_teacher_image_shape, in double): scale = target / max(H, W),
 * oh = (int)(H * scale + 0.5), ow = (int)(W * scale + 0.5).
 *
 * Quantise: u8 = (uint8)(int)(v * 255.0f), the fp32 product truncated, for v
 * in [0, 1]; outside that range the result is the casts' and is not defined
 * here.
 *
 * Resize: a horizontal pass and then a vertical pass, the intermediate image
 * rounded to uint8 between them.  For an axis of `in` source and `out`
 * destination cells, all in double:
 *     scale = in / out,  fs = max(scale, 1),  support = fs,  ss = 1 / fs
 *     center = (xx + 0.5) * scale
 *     xmin = max(0, (int)(center - support + 0.5))
 *     n    = min(in, (int)(center + support + 0.5)) - xmin
 *     w[x] = 1 - a where a = |(x + xmin - center + 0.5) * ss| < 1, else 0
 *     w[x] /= sum of w (when it is not 0);  k[x] = (int)(0.5 + w[x] * 4194304)
 * and a pass writes clamp(((1 << 21) + sum k[x] * pixel[xmin + x]) >> 22, 0,
 * 255), in int32, which cannot overflow.  The tables are built by a kernel
 * from these expressions (truncating casts), not on the host.
 *
 * Input tensor: per channel c, ((float)u8 - mean[c]) / std[c] -- one fp32
 * subtraction and one correctly rounded fp32 division -- written CHW into
 * out_input [3][S][S]; every cell right of or below the image is +0.0f.
 *
 * samnerf_teacher_image only enqueues three launches on `stream`: no
 * allocation, no copy to the host, no synchronisation; it can be captured in
 * a graph.  No float atomics: the same inputs give the same bits.
 *
 * rgb: fp32 [H][W][3] on the device.  mean, std: three HOST floats each, NULL
 * for SAM's registered buffers (123.675, 116.28, 103.53) and (58.395, 57.12,
 * 57.375).  out_u8: uint8 [oh][ow][3] or NULL (what apply_image returns);
 * out_input: fp32 [3][S][S] or NULL (what Sam.preprocess returns).  workspace:
 * samnerf_teacher_image_workspace_size(H, W, oh, ow) bytes, 256-byte aligned.
 *
 * SAMNERF_EINVAL, before anything is launched or any pointer read: H, W, oh,
 * ow (and S with out_input) outside [1, 8192]; a null rgb; out_u8 and
 * out_input both NULL; S < max(oh, ow) with out_input; workspace NULL or
 * workspace_bytes too small. */

/* oh, ow for a longest side of `target`.  SAMNERF_EINVAL: H, W or target
 * outside [1, 8192], a null pointer.  Host only. */
int samnerf_teacher_image_shape(uint32_t H, uint32_t W, uint32_t target, uint32_t* oh, uint32_t* ow);

/* Bytes of workspace for these sizes (0 for invalid ones).  Host only. */
size_t samnerf_teacher_image_workspace_size(uint32_t H, uint32_t W, uint32_t oh, uint32_t ow);

int samnerf_teacher_image(const float* rgb, uint32_t H, uint32_t W, uint32_t oh, uint32_t ow, uint32_t S,
                          const float* mean, const float* std, uint8_t* out_u8, float* out_input,
                          void* workspace, size_t workspace_bytes, samnerf_stream_t stream);

/* ---------------------------------------------------------- SAM decoder --
 * SAM's prompt encoder and mask decoder for point prompts, and the
 * postprocess of its masks: what SamPredictor.predict_torch runs between the
 * image embedding and the masks when the prompt is points (no box, no mask
 * input, one prompt set), with plain SAM's weights (no HQ token).  Written
 * from the model's published description and tested against this project's
 * own float64 restatement with synthetic weights; it has not been compared
 * with an installed segment_anything or a real checkpoint.
 *
 * Sizes: C = 256 channels, 8 heads; g x g image tokens (g a multiple of 8 in
 * [8, 64]; SAM's is 64), N = g*g; the input frame is S = 16 g; low-res masks
 * are 4g x 4g.  P points in [1, 58], T = P + 6 tokens.
 *
 *   pe(c), c = (x, y) in [0,1]^2:  v = (2c - 1) @ G * 2 pi, cat(sin v, cos v)
 *   image_pe[y*g + x] = pe(((x + .5) / g, (y + .5) / g))
 *   point token = pe(((x + .5) / S, (y + .5) / S)) + point_embeddings[label];
 *   one padding token = not_a_point_embed;
 *   tokens = cat(iou_token, mask_tokens[4], points[P], pad), also query_pe
 *   src = features + no_mask_embed
 *   Attention(q, k, v; inner): 8 heads of inner / 8, softmax(q k^T /
 *   sqrt(inner / 8)) v, out_proj; inner = 256 for the token self-attention
 *   and 128 for every cross-attention
 *   block l in {0, 1} (LayerNorm eps 1e-5, MLP lin2(relu(lin1 256 -> 2048))):
 *     q = norm1(l == 0 ? self(q, q, q) : q + self(q + pe, q + pe, q))
 *     q = norm2(q + t2i(q + query_pe, k + image_pe, k))
 *     q = norm3(q + mlp(q))
 *     k = norm4(k + i2t(k + image_pe, q + query_pe, q))
 *   q = norm_final(q + final_t2i(q + query_pe, k + image_pe, k))
 *   upscaled = gelu(convT2(gelu(LayerNorm2d(convT1(k as [256][g][g])))))
 *     (2 x 2 stride-2 transposed convolutions 256 -> 64 -> 32, LayerNorm2d
 *     over the channels of a pixel with eps 1e-6, the erf GELU)
 *   hyper_i = MLP_i(q[1 + i]) (256 -> 256 -> 256 -> 32, ReLU between)
 *   low_res[i] = hyper_i . upscaled;  iou = MLP(q[0]) (256 -> 256 -> 256 -> 4)
 *
 * Every product is an exact fp32 FMA accumulated in fp32; sin, cos, exp and
 * erf are the accurate library functions.  No float atomics and every sum in a
 * fixed order: the same inputs give the same bits.  Nothing is copied to the
 * host and nothing synchronises; the points travel as kernel arguments.
 *
 * raw: the checkpoint's tensors as fp32, concatenated in this order, each in
 * its state-dict shape (samnerf_sam_decoder_raw_count floats in all):
 *   prompt_encoder: pe_layer.positional_encoding_gaussian_matrix [2][128],
 *     point_embeddings.0, .1, not_a_point_embed, no_mask_embed [256] each;
 *   mask_decoder: iou_token [256], mask_tokens [4][256];
 *   transformer.layers.0, then .1: self_attn, cross_attn_token_to_image,
 *     cross_attn_image_to_token (each q_proj, k_proj, v_proj, out_proj as
 *     weight then bias), norm1 .. norm4 (weight, bias), mlp.lin1, mlp.lin2
 *     (weight, bias);
 *   transformer.final_attn_token_to_image (as above), norm_final_attn;
 *   output_upscaling.0 (weight [256][64][2][2], bias), .1 (weight, bias),
 *     .3 (weight [64][32][2][2], bias);
 *   output_hypernetworks_mlps.0 .. 3, each layers.0 .. 2 (weight, bias);
 *   iou_prediction_head.layers.0 .. 2 (weight, bias).
 * samnerf_sam_decoder_pack turns them into the kernels' order (linear weights
 * as [in][out], the transposed convolutions pixel-major) and adds the image_pe
 * table of g; once per checkpoint and g.
 *
 * SAMNERF_EINVAL, before anything is launched: g not a multiple of 8 in
 * [8, 64]; P outside [1, 58]; a label other than 0 or 1; a null pointer (the
 * workspace included); pack, iou or workspace not 16-byte aligned; a pack
 * smaller than samnerf_sam_decoder_pack_size(g); h, w not both 0 or both in
 * [1, 1024].  SAMNERF_EWORKSPACE: workspace_bytes (or pack_bytes, when
 * packing) too small. */

/* Floats of `raw`.  Host only. */
size_t samnerf_sam_decoder_raw_count(void);

/* Bytes of the pack for g (0 for an invalid g).  Host only. */
size_t samnerf_sam_decoder_pack_size(uint32_t g);

int samnerf_sam_decoder_pack(const float* raw, size_t raw_count, uint32_t g, void* pack, size_t pack_bytes,
                             samnerf_stream_t stream);

/* Bytes of workspace for g (0 for an invalid g).  Host only. */
size_t samnerf_sam_decoder_workspace_size(uint32_t g);

/* features: h = w = 0: the image tokens [g*g][256], token-major (zero where
 * the view is padded); otherwise a rendered map [h][w][256], which the first
 * kernel resizes to a long side of g (vh = (int)(h * r), vw = (int)(w * r),
 * r = g / max(h, w) in double; the taps of the distillation loss above) and
 * pads with zeros.  points: P HOST (x, y) pairs in the S frame; labels: P HOST
 * values 0 or 1.  low_res [4][4g][4g] and iou [4] on the device: mask 0 is
 * multimask_output=False's, masks 1 .. 3 multimask_output=True's. */
int samnerf_sam_decoder(const void* pack, size_t pack_bytes, uint32_t g, const float* features, uint32_t h,
                        uint32_t w, const int32_t* points, const int32_t* labels, uint32_t P, float* low_res,
                        float* iou, void* workspace, size_t workspace_bytes, samnerf_stream_t stream);

/* Kernel launches of the last successful samnerf_sam_decoder call. */
int samnerf_sam_decoder_launches(void);

/* Sam.postprocess_masks in one launch: low_res [M][4g][4g] (M in [1, 4])
 * resized to S x S (bilinear, align_corners=False), cropped to (in_h, in_w),
 * resized to (H, W): 16 taps per output pixel with the taps above, the S x S
 * image never written.  logits fp32 [M][H][W] and / or mask uint8 [M][H][W]
 * (logit > 0); one of them may be NULL.  SAMNERF_EINVAL: g as above, M outside
 * [1, 4], in_h or in_w outside [1, S], H or W outside [1, 8192], a null
 * low_res, both outputs NULL. */
int samnerf_sam_masks(const float* low_res, uint32_t M, uint32_t g, uint32_t in_h, uint32_t in_w, uint32_t H,
                      uint32_t W, float* logits, uint8_t* mask, samnerf_stream_t stream);

/* ------------------------------------------- SAM decoder: prompt batches --
 * B prompt sets of P points each over one image embedding: what SAM's
 * automatic mask generator runs per chunk of its point grid.  The kernels of
 * the single call with a batch axis: image-side linears on B N rows (image_pe
 * and the weights read by every set), token-side kernels on B T rows, the
 * attentions, the norm and the upscale with the set in the grid.  What does
 * not depend on the prompt runs once a call: the source tokens, layer 0's
 * token->image k / v projections and layer 0's image->token q projection (the
 * image tokens first change at the end of layer 0).  Every accumulation order
 * is the single call's, so set b of a batch has the bits of a single call on
 * points[b]; for whole-number coordinates those of the int32 entry.  The
 * launch count depends on no argument (samnerf_sam_decoder_launches).
 *
 * points [B][P][2] fp32 (x, y) in the S frame and labels [B][P] int32, both
 * ON THE DEVICE; a label is read as label != 0.  features, h, w as above.
 * low_res [B][4][4g][4g], iou [B][4].  SAMNERF_EINVAL before any launch: g as
 * above, B outside [1, 256], P outside [1, 58], a null pointer, pack / iou /
 * workspace not 16-byte aligned, a short pack, h / w as above.
 * SAMNERF_EWORKSPACE: a workspace smaller than
 * samnerf_sam_decoder_batch_workspace_size(g, B) (0 for a bad g or B). */
size_t samnerf_sam_decoder_batch_workspace_size(uint32_t g, uint32_t B);

int samnerf_sam_decoder_batch(const void* pack, size_t pack_bytes, uint32_t g, const float* features, uint32_t h,
                              uint32_t w, const float* points, const int32_t* labels, uint32_t B, uint32_t P,
                              float* low_res, float* iou, void* workspace, size_t workspace_bytes,
                              samnerf_stream_t stream);

/* The gather form of samnerf_sam_masks: output slot s is mask index[s] (index
 * NULL: s) of the table low_res [n][4g][4g], n in [1, 12288].  `count` slots
 * are launched; with count_dev (a device int32) only slots below *count_dev
 * are written and the others keep what they held, as does a slot whose index
 * lies outside the table.  logits / mask [count][H][W], the expression of
 * samnerf_sam_masks bit for bit; mask = logit > mask_threshold (SAM's is 0).  count = 0 succeeds with no launch. */
int samnerf_sam_masks_select(const float* low_res, uint32_t n, const int32_t* index, uint32_t count,
                             const int32_t* count_dev, uint32_t g, uint32_t in_h, uint32_t in_w, uint32_t H,
                             uint32_t W, float mask_threshold, float* logits, uint8_t* mask,
                             samnerf_stream_t stream);

/* One record of SAMNERF_SAM_REC_WORDS 32-bit words per mask candidate:
 *   0 inter  = #(logit > mask_threshold + stability_score_offset)
 *   1 union  = #(logit > mask_threshold - stability_score_offset)
 *   2 area   = #(logit > mask_threshold)
 *   3..6 x0, y0, x1, y1 of (logit > mask_threshold): min / max column and row,
 *        the max inclusive (batched_mask_to_box); 0, 0, 0, 0 for an empty mask
 *   7 stability = (float)inter / (float)union, its fp32 bits
 *   8 pass   = (iou > pred_iou_thresh) && (stability >= stability_score_thresh)
 *   9 iou, its fp32 bits
 * over the (H, W) view, the logit being samnerf_sam_masks' expression kept in
 * registers.  A candidate failing the IoU test is not walked: its record is
 * all zero.  NaN compares false.  Integer sums and min / max, no atomics.
 * n in [0, 12288]; n = 0 succeeds with no launch. */
#define SAMNERF_SAM_REC_WORDS 10

int samnerf_sam_mask_stats(const float* low_res, const float* iou, uint32_t n, uint32_t g, uint32_t in_h,
                           uint32_t in_w, uint32_t H, uint32_t W, float pred_iou_thresh, float mask_threshold,
                           float stability_score_offset, float stability_score_thresh, int32_t* records,
                           samnerf_stream_t stream);

/* Greedy box NMS over the passing records, on the device: descending iou,
 * ties to the lower index; a later box is suppressed when
 * inter / (a_i + a_j - inter) > box_nms_thresh in fp32, inter =
 * max(0, min(x1) - max(x0)) * max(0, min(y1) - max(y0)), a = (x1 - x0)(y1 - y0)
 * on the boxes as floats (torchvision's nms); 0 / 0 suppresses nothing.
 * keep [n] int32: the kept indices in that order, then -1; *count their
 * number.  n in [0, 12288]; n = 0 succeeds with no launch and writes nothing. */
int samnerf_sam_nms(const int32_t* records, uint32_t n, float box_nms_thresh, int32_t* keep, int32_t* count,
                    samnerf_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* SAMNERF_HIP_H */
