"""Plain numpy float64 reference of the s_grid stage: the forward composite
(k_sgrid / k_sgrid_box4) and the distillation step's gradient scatter
(k_sgrid_backward, fp32-atomic and 64-bit fixed-point forms), with the error
bounds of their fp32 evaluation.  numpy only, no GPU.

Built on tests/grid_ref.py: the s_grid is a D = 3 hash grid (gridtype 0,
align_corners off, linear interpolation), and the kernels' locate_axis /
dense_or_hash_row are the definition grid_ref.locate / grid_ref.corner_rows
reproduce exactly (fp32 position and fraction, `min(cell + 1, res - 1)`
corner, dense stride sum or prime XOR).  Everything else is float64.

Inputs are ray-major, as FusedRenderer.render(taps=True) returns them --
u2 [N, 32, 3] sample positions, w2 [N, 32] sample weights: copies of the
very arrays both kernels read, N1's dropped samples (w = 0, u = 0.5)
included -- plus the s_grid's GridSpec and, for the scatter, g [N, >= 128],
the gradient of the head-input rows whose first 128 columns are f_sam's.

The bounds are counted from the kernels' operations, in units of
U = 2^-24 (fp32 round-to-nearest: |fl(x) - x| <= U |x|), first order in U as
grid_ref's; they are not measured on the kernels.
"""
import numpy as np

import grid_ref
from grid_ref import U
from oracle.encoders import grid_level_resolutions

T = 32          # final-stage samples per ray
C = 8           # s_grid channels per level
F = 128         # f_sam columns of a head-input row


def geometry(spec):
    """GridSpec -> (offsets int64 [L + 1], indexing resolution per level)."""
    return (np.asarray(spec.offsets(), np.int64),
            grid_level_resolutions(spec.num_levels, spec.S, spec.base_resolution))


def level_kinds(spec):
    """Per level 'dense' or 'hashed' (the dense stride sum fits the table)."""
    offsets, res = geometry(spec)
    return ["hashed" if grid_ref.strides_used(r, int(offsets[l + 1] - offsets[l]), 3)[1] else "dense"
            for l, r in enumerate(res)]


def _samples(u2, w2):
    u2 = np.asarray(u2)
    w2 = np.asarray(w2)
    N = w2.shape[0]
    assert u2.dtype == np.float32 and w2.dtype == np.float32
    assert u2.shape == (N, T, 3) and w2.shape == (N, T)
    # the kernels clamp, grid_ref zeroes a point outside [0, 1]: the two only
    # agree on positions inside, which is all the render ever hands over
    if not (np.isfinite(u2).all() and (u2 >= 0).all() and (u2 <= 1).all()):
        raise ValueError("sgrid_ref: sample positions outside [0, 1]")
    if not np.isfinite(w2).all():
        raise ValueError("sgrid_ref: non-finite sample weights")
    return u2.reshape(N * T, 3), w2.reshape(N * T).astype(np.float64), N


def composite(u2, w2, emb, spec):
    """f_sam [N, 128] float64, column level * 8 + ch = sum_k w_k *
    interp_level(u_k)[ch]; abs_ww = sum_k |w_k| sum_c |w_c e| (the magnitude
    the bound is relative to); abs_1 = sum over the samples with w_k != 0 of
    sum_c |e| (zero where nothing can contribute: the output must be +0.0)."""
    x, w, N = _samples(u2, w2)
    offsets, res = geometry(spec)
    L = len(res)
    assert L * C == F and emb.shape == (int(offsets[-1]), C)
    val, abs_w, abs_1, _ = grid_ref.forward(x, emb, offsets, res)          # [L, N*T, C]

    def per_ray(a, wk):
        a = (a * wk[None, :, None]).reshape(L, N, T, C).sum(axis=2)         # [L, N, C]
        return np.ascontiguousarray(a.transpose(1, 0, 2)).reshape(N, F)

    return per_ray(val, w), per_ray(abs_w, np.abs(w)), per_ray(abs_1, (w != 0).astype(np.float64))


def scatter(u2, w2, g, spec):
    """Gradient of the embeddings for the row gradient g [N, >= 128] (only the
    first 128 columns are read) -> val [rows, 8] float64, abs_w = sum |w_k
    w_c g|, abs_1 = sum |w_k g| and count [rows] = the (sample, corner)
    contributions a row receives.  grid_ref.backward_embeddings over the
    N * 32 samples as points with grad = w_k * g formed in float64; samples
    with w_k == 0 are left out (of count too): they add exactly nothing."""
    x, w, N = _samples(u2, w2)
    offsets, res = geometry(spec)
    L = len(res)
    g64 = np.asarray(g)[:, :F].astype(np.float64)
    assert g64.shape == (N, F) and np.isfinite(g64).all()
    keep = w != 0
    ray = np.repeat(np.arange(N), T)[keep]
    grad = (w[keep, None] * g64[ray]).reshape(-1, L, C).transpose(1, 0, 2)   # [L, B, C]
    return grid_ref.backward_embeddings(grad, x[keep], int(offsets[-1]), offsets, res)


# ----------------------------------------------------------------- bounds --

# Composite (k_sgrid, every form: same operations in the same order).  One
# output is sum over 32 samples of w_k * f_k, f_k = sum over 8 corners of
# w_c e.  A term w_k w_c e passes through
#   8 + 3 + 1  the interpolation, as grid_ref.bound_forward(3, 0, ..): the
#              8-corner FMA chain, the weight's products and its 1 - f
#              (1 - f is exact for cell >= 1, where f is a multiple of 2^-23:
#              the count only bites in the first cell of an axis);
#   8          the product w_k * f_k (a packed multiply, -ffp-contract=off: no
#              FMA) and its quarter's chain acc = acc + w f over 8 samples,
#              whose first add, to +0, is exact: 1 + 7;
#   3          ((q0 + q1) + q2) + q3 of the four quarters.
# Every rounding is relative to a partial sum bounded by abs_ww.
COMPOSITE_COEFF = (8 + 3 + 1) + 8 + 3

# |fl(x) - x| <= U |x| holds for results in fp32's normal range only.  Below
# 2^-126 a result is rounded to a multiple of 2^-149, or flushed to zero (the
# memory-side float atomics may), so every operation also carries an absolute
# error of up to TINY -- nothing next to U |x| until the weights themselves
# underflow, which N1's nearly closed rays reach: their transmittance falls
# through 1e-30 before the wave exits, and w_k times a corner weight times g
# leaves the normal range.  The floor is counted per operation and scaled by
# the largest factor an error is still multiplied with (every weight is <= 1:
# max |e| in the composite, max |g| in the scatter); it applies where the
# relative magnitude is non-zero (all-zero products are exact).
TINY = 2.0 ** -126


def bound_composite(abs_ww, emax):
    # per sample: two weight products per corner (times |e|), the 8 FMAs, the
    # w f product and one add: <= 16 emax + 10; 32 samples and 3 quarter adds
    return U * COMPOSITE_COEFF * abs_ww + (abs_ww > 0) * (1024 * TINY * max(1.0, float(emax)))


# Atomic scatter (k_sgrid_backward<T, false>).  One contribution is
# ((wx * wy) * wz) * (w_k * g): up to three 1 - f, two weight products, the
# w_k * g product and the product of the two = 7 roundings, i.e.
# grid_ref.bound_grad_embeddings' D + m = 3 + 1 plus the w * g product and
# the extra weight product (+ 2) plus the first of count adds.  The count
# contributions of a row are then added -- by the wave's butterfly and by
# the fp32 atomics, in any order -- with count - 1 roundings, each relative
# to a partial sum bounded by abs_w: (count + 6) U abs_w.  Underflow floor:
# 7 operations and one add per contribution, an error in a weight product
# still multiplied by |w_k g| <= max |g|.
def _scatter_floor(abs_w, count, gmax):
    return (abs_w > 0) * (8 * count[:, None] * TINY * max(1.0, float(gmax)))


def bound_scatter_atomic(abs_w, count, gmax):
    return U * (count[:, None] + 3 + 1 + 2) * abs_w + _scatter_floor(abs_w, count, gmax)


def det_shift(N, gmax):
    """log2 of the fixed-point scale of samnerf_sgrid_backward_det: 61 -
    ceil(log2 N) - e with max |g[:, :128]| in [2^(e-1), 2^e)."""
    log2n = 0
    while (1 << log2n) < N:
        log2n += 1
    _, e = np.frexp(np.float32(gmax))
    return 61 - log2n - int(e)


# Deterministic scatter (k_sgrid_backward<T, true> + k_sgrid_det_finish).  The
# atomic bound's count * U term is absent: the adds are integer.
#   7                     one contribution formed in fp32, as above;
#   3                     the 3-level fp32 butterfly merge of the wave's 8
#                         rays, which stays in this mode (a value passes
#                         through at most 3 adds before it is quantised);
#   1                     the one rounding of the total to fp32
#                         ((float)((double)v * 2^-shift): the int64 -> double
#                         conversion's 2^-53 is second order);
#   count * 2^-(shift+1)  each added value is rounded to an integer multiple
#                         of 2^-shift (__double2ll_rn of an exact product), at
#                         most one per contribution.
# (The underflow floor of the fp32 contributions is far below the quantum
# 2^-shift at any gradient scale; it is added for the derivation's sake.)
def bound_scatter_det(abs_w, count, N, gmax):
    if gmax == 0:
        return np.zeros_like(abs_w)
    return (U * (7 + 3 + 1) * abs_w + count[:, None] * 2.0 ** -(det_shift(N, gmax) + 1)
            + _scatter_floor(abs_w, count, gmax))


# Accumulation into a prefilled gradient P.  The deterministic form adds its
# fp32 total to P once: one more rounding, U |P + val|.  The fp32-atomic form
# adds every (merged) contribution to the table entry itself, so each of its
# up to count atomics rounds a partial sum that contains P: count U |P|, not
# one U |P + val| (the fp32 emulation of test_sgrid_ref_cpu.py exceeds the
# latter at rows with a handful of contributions, whatever the kernel does).
def bound_prefill_det(p_plus_val):
    return U * np.abs(p_plus_val)


def bound_prefill_atomic(prefill, count):
    return U * count[:, None] * np.abs(np.asarray(prefill, np.float64))


# ------------------------------------------------- shared case parameters --

S_GRID_LOG2 = (11, 14, 16)
N_SWEEP = (1, 7, 8, 9, 33, 37, 64, 65)
# (name, N, view_width): the ray sets of test_gpu_sgrid_scatter.py, which the
# CPU module runs with synthetic samples
RAY_SETS = [(f"first{n}", n, 0) for n in N_SWEEP] + [
    ("dup64", 64, 0), ("tiles16x12", 192, 16), ("tiles8x4", 32, 8), ("early100", 100, 0),
    ("edge37", 37, 0)]


def dup64_sources():
    """Source ray of each of the 64 rays of the duplicated-ray set: a wave of
    k_sgrid_backward is 8 neighbouring rays (x 8 channels) whose equal corner
    rows merge over a butterfly at ray distances 1, 2, 4."""
    src = np.arange(64)
    src[8:16] = 8                        # wave 1: all equal -- the full merge
    src[17] = 16                         # wave 2: a pair at distance 1,
    src[22] = 20                         #         one at distance 2
    src[28] = 24                         # wave 3: one at distance 4
    src[35] = 32                         # wave 4: rays 0 and 3 equal: never compared, both issue
    src[41] = src[43] = 40               # wave 5: 0, 1, 3 equal: 3 meets the merged (dead) 1 at distance 2
    src[50] = src[51] = 48               # wave 6: 0, 2, 3 equal: 3 dies into 2, then 2 into 0
    src[61] = src[62] = src[63] = 57     # wave 7: 1, 5, 6, 7 equal
    return src


def slot_rays(N, view_width):
    """The kernels' slot -> ray map (8 x 4 pixel tiles of a view of this
    width; the identity without one), as samnerf_amd.fused.ray_of_slots."""
    s = np.arange(N)
    W = int(view_width)
    if W < 8 or W % 8 or N % (4 * W):
        return s
    tile, inn = s >> 5, s & 31
    trow, tcol = tile // (W // 8), tile % (W // 8)
    return (trow * 4 + (inn >> 3)) * W + tcol * 8 + (inn & 7)
