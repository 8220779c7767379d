"""Plain numpy float64 reference of the drop-in grid encoder, any D.

Independent of oracle/encoders_oracle.c: nothing here calls it.  The only
import from oracle/ is `grid_level_resolutions` (the per-level indexing
resolution, pinned by test_grid_resolution_table_matches_survey).

What is reproduced exactly is the operation's *definition* -- the steps that
decide which cell a point is in and which table rows it reads:

  position, fp32   align_corners off: p = fma(x, res, -0.5) (x * res - 0.5 in
                   float64, rounded once), clamped to [0, res - 1],
                   cell = floor(p);
                   align_corners on:  p = fp32(x * (res - 1)),
                   cell = min(floor(p), res - 2);
                   frac = fp32(p - cell);
  +1 corner        min(cell + 1, res - 1);
  row              dense stride sum while stride <= size; hash tables whose
                   stride overran use the prime XOR instead; uint32 wrap,
                   then % size;
  outside          a point with a coordinate < 0 or > 1 contributes nothing
                   and gets zeros.

Everything else -- smoothstep f*f*(3 - 2f), its derivative 6f(1 - f), corner
weights, all sums -- is float64.  Each function returns the value together
with the magnitudes its error bound needs (see the bound_* functions).

The second half of the file builds the grid configurations and point sets the
CPU and GPU test modules share.
"""
import functools
import itertools

import numpy as np

from oracle.encoders import grid_level_resolutions

PRIMES = (1, 2654435761, 805459861, 3674653429, 2097192037, 1434869437, 2165219737)
_M = 0xFFFFFFFF
U = 2.0 ** -24                      # fp32 unit roundoff
NO_ROW = 0xFFFFFFFF                 # corner-row entry of an outside point
MODES = list(itertools.product((0, 1), (False, True), (0, 1)))   # (gridtype, align, interp)


# ------------------------------------------------------------- definition --

def strides_used(res, size, D):
    """Number of axes the dense stride sum consumes before stride > size, and
    whether the stride overran the table."""
    stride, d = 1, 0
    while d < D and stride <= size:
        stride = (stride * res) & _M
        d += 1
    return d, stride > size


def corner_rows(cell, res, size, gridtype):
    """cell [..., D] non-negative ints -> row [...] in [0, size)."""
    cell = np.asarray(cell, np.int64)
    D = cell.shape[-1]
    stride = 1
    row = np.zeros(cell.shape[:-1], np.int64)
    for d in range(D):
        if stride > size:
            break
        row = (row + cell[..., d] * stride) & _M
        stride = (stride * res) & _M
    if gridtype == 0 and stride > size:
        row = np.zeros(cell.shape[:-1], np.int64)
        for d in range(D):
            row ^= (cell[..., d] * PRIMES[d]) & _M
    return row % size


def inside_mask(x):
    x = np.asarray(x)
    return ~((x < 0) | (x > 1)).any(axis=1)


def locate(x, res, align, exact=False):
    """-> cell [B, D] int64, frac [B, D] float64 (pre-smoothstep).  Outside
    points are located as if at 0 (callers mask them).  `exact` keeps the
    position in float64 (finite-difference checks only)."""
    ins = inside_mask(x)
    x64 = np.where(ins[:, None], np.asarray(x, np.float64), 0.0)
    rnd = (lambda a: a) if exact else (lambda a: a.astype(np.float32).astype(np.float64))
    if align:
        p = rnd(x64 * (res - 1))
        cell = np.minimum(np.floor(p), res - 2)
    else:
        p = np.clip(rnd(x64 * res - 0.5), 0.0, float(res - 1))
        cell = np.floor(p)
    frac = rnd(p - cell)
    return cell.astype(np.int64), frac


def _interp(frac, interp):
    """-> (interpolation weight of the +1 side, d weight / d frac), float64."""
    if interp == 1:
        return frac * frac * (3.0 - 2.0 * frac), 6.0 * frac * (1.0 - frac)
    return frac, np.ones_like(frac)


def _levels(offsets, res):
    offsets = np.asarray(offsets, np.int64)
    return [(int(offsets[l]), int(offsets[l + 1] - offsets[l]), int(res[l])) for l in range(len(res))]


def _corner(c, dims, cell, f, res):
    """Corner bit pattern c over axes `dims`: weight product [B] and the
    corner's cell (other axes left as in `cell`)."""
    w = np.ones(cell.shape[0])
    cc = cell.copy()
    for k, d in enumerate(dims):
        if (c >> k) & 1:
            w = w * f[:, d]
            cc[:, d] = np.minimum(cell[:, d] + 1, res - 1)
        else:
            w = w * (1.0 - f[:, d])
    return w, cc


# -------------------------------------------------------------- functions --

def forward(x, emb, offsets, res, gridtype=0, align=False, interp=0, max_level=None, exact=False):
    """-> value [L, B, C], abs_w = sum |w e|, abs_1 = sum |e| (both [L, B, C])
    and the corner rows [L, B, 2^D] uint32 (NO_ROW for outside points).
    Levels >= max_level stay zero."""
    B, D = x.shape
    L, C = len(res), emb.shape[1]
    max_level = L if max_level is None else min(max_level, L)
    e64 = np.asarray(emb, np.float64)
    ins = inside_mask(x)
    val = np.zeros((L, B, C))
    abs_w = np.zeros((L, B, C))
    abs_1 = np.zeros((L, B, C))
    rows = np.full((L, B, 1 << D), NO_ROW, np.uint32)
    for l, (off, size, r) in enumerate(_levels(offsets, res)[:max_level]):
        cell, frac = locate(x, r, align, exact)
        f, _ = _interp(frac, interp)
        table = e64[off:off + size]
        for c in range(1 << D):
            w, cc = _corner(c, range(D), cell, f, r)
            row = corner_rows(cc, r, size, gridtype)
            e = table[row]
            val[l] += w[:, None] * e
            abs_w[l] += np.abs(w[:, None] * e)
            abs_1[l] += np.abs(e)
            rows[l, :, c] = row
        for a in (val, abs_w, abs_1):
            a[l, ~ins] = 0.0
        rows[l, ~ins] = NO_ROW
    return val, abs_w, abs_1, rows


def dy_dx(x, emb, offsets, res, gridtype=0, align=False, interp=0, max_level=None, exact=False):
    """-> value [B, L, D, C]; abs_w = sum |t| over the terms
    t = span * w * (e_hi - e_lo) * dfrac; abs_1 = the same sum with w = 1."""
    B, D = x.shape
    L, C = len(res), emb.shape[1]
    max_level = L if max_level is None else min(max_level, L)
    e64 = np.asarray(emb, np.float64)
    ins = inside_mask(x)
    val = np.zeros((B, L, D, C))
    abs_w = np.zeros((B, L, D, C))
    abs_1 = np.zeros((B, L, D, C))
    for l, (off, size, r) in enumerate(_levels(offsets, res)[:max_level]):
        cell, frac = locate(x, r, align, exact)
        f, df = _interp(frac, interp)
        table = e64[off:off + size]
        span = float(r - 1 if align else r)
        for gd in range(D):
            others = [d for d in range(D) if d != gd]
            for c in range(1 << (D - 1)):
                w, cc = _corner(c, others, cell, f, r)
                lo = corner_rows(cc, r, size, gridtype)
                cc[:, gd] = np.minimum(cell[:, gd] + 1, r - 1)
                hi = corner_rows(cc, r, size, gridtype)
                t1 = span * (table[hi] - table[lo]) * df[:, gd, None]
                val[:, l, gd] += w[:, None] * t1
                abs_w[:, l, gd] += np.abs(w[:, None] * t1)
                abs_1[:, l, gd] += np.abs(t1)
        for a in (val, abs_w, abs_1):
            a[~ins, l] = 0.0
    return val, abs_w, abs_1


def backward_embeddings(grad, x, n_rows, offsets, res, gridtype=0, align=False, interp=0,
                        max_level=None, exact=False):
    """grad [L, B, C] -> value [rows, C]; per element abs_w = sum |w g| and
    abs_1 = sum |g|; per row the count of (point, corner) contributions."""
    B, D = x.shape
    L, C = len(res), grad.shape[2]
    max_level = L if max_level is None else min(max_level, L)
    g64 = np.asarray(grad, np.float64)
    ins = inside_mask(x)
    val = np.zeros((n_rows, C))
    abs_w = np.zeros((n_rows, C))
    abs_1 = np.zeros((n_rows, C))
    count = np.zeros(n_rows, np.int64)
    for l, (off, size, r) in enumerate(_levels(offsets, res)[:max_level]):
        cell, frac = locate(x, r, align, exact)
        f, _ = _interp(frac, interp)
        g = g64[l][ins]
        for c in range(1 << D):
            w, cc = _corner(c, range(D), cell, f, r)
            row = off + corner_rows(cc, r, size, gridtype)[ins]
            wg = w[ins, None] * g
            np.add.at(val, row, wg)
            np.add.at(abs_w, row, np.abs(wg))
            np.add.at(abs_1, row, np.abs(g))
            np.add.at(count, row, 1)
    return val, abs_w, abs_1, count


def backward_inputs(grad, dy):
    """grad [L, B, C], dy [B, L, D, C] -> value [B, D] and sum |g * dy|."""
    g = np.asarray(grad, np.float64).transpose(1, 0, 2)[:, :, None, :]      # [B, L, 1, C]
    t = g * np.asarray(dy, np.float64)
    return t.sum(axis=(1, 3)), np.abs(t).sum(axis=(1, 3))


def total_variation(x, emb, offsets, res, weight, gridtype=0, align=False):
    """TV gradient at the cells of `x`, all levels -> value [rows, C],
    abs_c = sum |contribution|, abs_v = sum (w * rsqrt * sum |v|), count per
    row.  The `cell < res` upper test is the reference's (always true: the
    +1 neighbour of the last cell wraps through % size)."""
    B, D = x.shape
    C = emb.shape[1]
    e64 = np.asarray(emb, np.float64)
    ins = inside_mask(x)
    w = float(np.float32(weight)) / (2 * D)
    eps = float(np.float32(1e-9))
    val = np.zeros(e64.shape)
    abs_c = np.zeros(e64.shape)
    abs_v = np.zeros(e64.shape)
    count = np.zeros(e64.shape[0], np.int64)
    for off, size, r in _levels(offsets, res):
        cell, _ = locate(x, r, align)
        table = e64[off:off + size]
        here = corner_rows(cell, r, size, gridtype)
        e0 = table[here]
        s = np.zeros((B, C))
        sa = np.zeros((B, C))
        sq = np.zeros((B, C))
        for d in range(D):
            for step, ok in ((1, cell[:, d] < r), (-1, cell[:, d] > 0)):
                c2 = cell.copy()
                c2[:, d] = np.maximum(cell[:, d] + step, 0)
                v = (e0 - table[corner_rows(c2, r, size, gridtype)]) * ok[:, None]
                s += v
                sa += np.abs(v)
                sq += v * v
        rs = 1.0 / np.sqrt(sq + eps)
        row = off + here[ins]
        np.add.at(val, row, (w * s * rs)[ins])
        np.add.at(abs_c, row, np.abs(w * s * rs)[ins])
        np.add.at(abs_v, row, (abs(w) * sa * rs)[ins])
        np.add.at(count, row, 1)
    return val, abs_c, abs_v, count


def weight_decay(emb, offsets, weight):
    """2 * weight * e / rows_in_level."""
    offsets = np.asarray(offsets, np.int64)
    sizes = np.repeat(np.diff(offsets), np.diff(offsets)).astype(np.float64)
    return 2.0 * float(np.float32(weight)) * np.asarray(emb, np.float64) / sizes[:, None]


# ----------------------------------------------------------------- bounds --
# Absolute-error bounds of an fp32 evaluation (any summation order) around the
# float64 value, u = 2^-24.  s = 1 for smoothstep: its weights are formed in
# fp32 as f*f*(3 - 2f) and 1 - that, so they carry an *absolute* error of a few
# u each (D of them per corner), which no |w e|-relative term covers; hence
# the abs_1 term.  m counts the roundings of one weight factor (1 for 1 - f,
# 3 more multiplies/fma for smoothstep).

def _sm(interp):
    return (1, 3) if interp == 1 else (0, 1)


def bound_forward(D, interp, abs_w, abs_1):
    # 2^D fmas of the sum + D products and m roundings per weight, relative to
    # sum |w e|; 4u absolute per smoothstep factor, D factors, times sum |e|
    s, m = _sm(interp)
    return U * (((1 << D) + D + m) * abs_w + 4 * D * s * abs_1)


def bound_grad_embeddings(D, interp, abs_w, abs_1, count):
    # as the forward, with count[row] additions (atomics / butterfly, any order)
    s, m = _sm(interp)
    return U * ((count[:, None] + D + m) * abs_w + 4 * D * s * abs_1)


def bound_dy_dx(D, interp, abs_w, abs_1):
    # 2^(D-1) fmas + (D - 1) weight products + span, difference, dfrac (<= 6
    # roundings); absolute smoothstep error on the D - 1 weight factors
    s, _ = _sm(interp)
    return U * (((1 << (D - 1)) + D + 6) * abs_w + 4 * (D - 1) * s * abs_1)


def bound_grad_inputs(L, C, abs_gdy):
    # one fma chain of L*C terms (+ the final store): (L*C + 1) u sum |g dy|
    return (L * C + 1) * U * abs_gdy


def bound_tv(D, abs_c, abs_v, count):
    # per contribution: difference, up to 2D additions, the square sum feeding
    # rsqrtf (<= 2 ulp), w = weight / 2D and two products: (3D + 7) u relative
    # to w * rsqrt * sum |v|; then count[row] atomic additions
    return U * ((3 * D + 7) * abs_v + count[:, None] * abs_c)


def worst_ratio(got, ref, bound, zero_key, prefill=None):
    """max |got - ref| / bound over the elements with a non-zero bound, after
    asserting that every element whose `zero_key` magnitude is zero holds
    exactly +0.0 (or the prefill) bit for bit.  No element is excluded."""
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == ref.shape == bound.shape
    expect = np.zeros_like(got) if prefill is None else np.asarray(prefill, np.float32)
    z = np.broadcast_to(zero_key == 0, got.shape)
    assert np.array_equal(got[z].view(np.uint32), expect[z].view(np.uint32)), \
        "an element nothing contributes to is not +0.0 / the prefill"
    err = np.abs(got.astype(np.float64) - ref)
    # a zero bound (every weight exactly zero, linear interpolation on a cell
    # face) asks for the exact value
    tight = ~z & (bound == 0)
    assert (err[tight] == 0).all(), "an element with a zero error bound is not exact"
    rest = ~z & ~tight
    return float((err[rest] / bound[rest]).max()) if rest.any() else 0.0


# ------------------------------------------------------ shared test cases --

LOG2_CAP = 10
CONFIGS = {2: (16, 1.5, 6), 3: (4, 1.6, 6), 4: (2, 1.7, 6), 5: (2, 1.5, 5)}   # D: (H, scale, L)
CHANNELS = (1, 2, 4, 8, 16, 32)
B_POINTS = 700


def grid_offsets(D, H, per_level_scale, L, log2_cap=LOG2_CAP):
    """Table layout of GridEncoder(input_dim=D, ...): ceil(H * scale^l) per
    axis, capped at 2^log2_cap rows, rounded up to a multiple of 8."""
    sizes = []
    for lvl in range(L):
        r = int(np.ceil(H * per_level_scale ** lvl))
        sizes.append(int(np.ceil(min(2 ** log2_cap, r ** D) / 8) * 8))
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)


class Case:
    """One grid configuration: geometry + the 700 test points."""

    def __init__(self, D):
        self.D = D
        self.H, self.scale, self.L = CONFIGS[D]
        self.S = float(np.log2(self.scale))
        self.offsets = grid_offsets(D, self.H, self.scale, self.L)
        self.res = grid_level_resolutions(self.L, self.S, self.H)
        self.rows = int(self.offsets[-1])
        self.x = make_points(D, self.res)

    def level_kinds(self):
        """Per level: (axes consumed by the stride sum, overran)."""
        return [strides_used(r, size, self.D) for _, size, r in _levels(self.offsets, self.res)]

    def emb(self, C, lo=-1.0, hi=1.0):
        return np.random.default_rng(100 * self.D + C).uniform(lo, hi, (self.rows, C)).astype(np.float32)

    def grad(self, C, B=None):
        B = self.x.shape[0] if B is None else B
        return np.random.default_rng(7 * self.D + C).standard_normal((self.L, B, C)).astype(np.float32)


def make_points(D, res, B=B_POINTS, seed=0):
    """[uniform | 20 in [-0.02, 1.02]^D | 0, 1, -0.0, nextafter(1, 0) |
    32 on the cell faces (k + 0.5) / res of a middle level | 128 inside one
    finest-level cell | 64 identical]: the last two make many lanes of a wave
    hit the same rows."""
    rng = np.random.default_rng(1000 * D + seed)
    n_uni = B - (20 + 4 + 32 + 128 + 64)
    uni = rng.uniform(0, 1, (n_uni, D))
    oob = rng.uniform(-0.02, 1.02, (20, D))
    oob[0, 0], oob[1, D - 1] = -0.01, 1.01               # certainly outside
    special = np.stack([np.zeros(D), np.ones(D), np.full(D, -0.0),
                        np.full(D, np.nextafter(np.float32(1), np.float32(0)))])
    rm = res[len(res) // 2]
    faces = (rng.integers(0, rm, (32, D)) + 0.5) / rm
    rf = res[-1]
    k = rng.integers(1, rf - 1, (1, D))
    cluster = (k + 0.5 + rng.uniform(0.02, 0.98, (128, D))) / rf     # non-align cell k
    same = np.repeat(rng.uniform(0.1, 0.9, (1, D)), 64, axis=0)
    x = np.concatenate([uni, oob, special, faces, cluster, same]).astype(np.float32)
    assert x.shape == (B, D)
    return x


def tail_points(case, B):
    """B points for the partial-last-wave shapes: clustered points (shared
    rows), outside points and uniform ones."""
    x = case.x
    n_uni = x.shape[0] - (20 + 4 + 32 + 128 + 64)
    cluster, oob = x[n_uni + 56:n_uni + 184], x[n_uni:n_uni + 20]
    return np.ascontiguousarray(
        np.concatenate([cluster[:max(1, B // 2)], oob[:2], x[:n_uni]])[:B])


@functools.lru_cache(maxsize=None)
def case(D):
    return Case(D)
