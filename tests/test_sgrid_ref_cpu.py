"""The float64 s_grid reference (tests/sgrid_ref.py) checked on its own, no GPU.

  * composite and scatter are each other's transpose (float64, 1e-12);
  * a numpy fp32 emulation of the kernels' arithmetic -- the same 1 - f
    weights, ((wx * wy) * wz) * (w * g), the 8-ray butterfly merge, the adds
    in a random order; the FMA chain, quarter chains and quarter adds of the
    forward -- sits under the derived bounds at every ray set and table size
    the GPU module (test_gpu_sgrid_scatter.py) runs, with synthetic samples:
    the bounds are sound for inputs of that kind before any kernel is asked;
  * rows nothing reaches and zero-weight samples are handled as zeros.
"""
import numpy as np
import pytest

import grid_ref
import sgrid_ref
from oracle import synth

T, C, F = sgrid_ref.T, sgrid_ref.C, sgrid_ref.F


def _spec(log2):
    return synth.ModelSpec(with_sam=True, grid_log2=12, prop_log2=10, s_grid_log2=log2).s_grid


def _emb(spec, seed=0):
    rows = int(spec.offsets()[-1])
    return np.random.default_rng(seed).uniform(-0.5, 0.5, (rows, C)).astype(np.float32)


def synth_samples(name, N, seed=0):
    """Rays of one camera through the unit cube: neighbouring rays share
    cells at the coarse levels.  Rays 8..15 are identical (N >= 16), one ray
    has 12 zero-weight samples parked at u = 0.5 (as N1 leaves them), the
    dup64 set repeats rays as on the GPU, the early100 set lets the weights
    fall through fp32's range and drops the tail samples of whole 8-ray
    groups, the edge37 set sits against the upper faces of the cube."""
    rng = np.random.default_rng(1000 * N + seed)
    o = rng.uniform(0.35, 0.65, 3)
    d = rng.standard_normal(3)
    d /= np.linalg.norm(d)
    dirs = d + 0.01 * rng.standard_normal((N, 3))
    t = np.sort(rng.uniform(0.0, 0.3, (N, T)), axis=1)
    u2 = np.clip(o + t[:, :, None] * dirs[:, None, :], 0.0, 1.0).astype(np.float32)
    w2 = rng.uniform(0, 1, (N, T)) ** 4
    w2 = (w2 / w2.sum(axis=1, keepdims=True) * rng.uniform(0.5, 1.0, (N, 1))).astype(np.float32)
    if N >= 16:
        u2[8:16], w2[8:16] = u2[8], w2[8]
    if name == "dup64":
        src = sgrid_ref.dup64_sources()
        u2, w2 = u2[src], w2[src]
    if name == "edge37":                       # the last cell of every level: the clamped + 1 corner
        u2 = (1.0 - (1.0 - u2) * 0.03).astype(np.float32)
    if name == "early100":
        # nearly closed rays: the transmittance falls by 1e-2..1e-4 a sample,
        # through fp32's normal range, until the group is dropped
        fall = np.cumprod(rng.uniform(1e-4, 1e-2, (N, T)), axis=1)
        w2 = (w2 * 32 * fall).astype(np.float32)
        w2[:, 0] = 0.5
        for g0 in range(0, N, 8):
            keep = int(rng.integers(12, T))
            u2[g0:g0 + 8, keep:], w2[g0:g0 + 8, keep:] = 0.5, 0.0
    z = N // 2
    u2[z, T - 12:], w2[z, T - 12:] = 0.5, 0.0
    g = rng.standard_normal((N, 164)).astype(np.float32)
    return np.ascontiguousarray(u2), np.ascontiguousarray(w2), g


# ------------------------------------------------------- fp32 emulations --

def _f32_weights(frac):
    f = frac.astype(np.float32)
    return f, np.float32(1.0) - f


def _corners(x, r, size):
    """Per corner: (level-relative row [B], fp32 weight (wx * wy) * wz [B])."""
    cell, frac = grid_ref.locate(x, r, False)
    f, omf = _f32_weights(frac)
    for c in range(8):
        cc = cell.copy()
        w = []
        for d in range(3):
            if (c >> d) & 1:
                cc[:, d] = np.minimum(cell[:, d] + 1, r - 1)
                w.append(f[:, d])
            else:
                w.append(omf[:, d])
        yield grid_ref.corner_rows(cc, r, size, 0), (w[0] * w[1]) * w[2]


def emulate_composite(u2, w2, emb, spec):
    offsets, res = sgrid_ref.geometry(spec)
    N = w2.shape[0]
    x = u2.reshape(-1, 3)
    out = np.zeros((N, F), np.float32)
    for l, r in enumerate(res):
        off, size = int(offsets[l]), int(offsets[l + 1] - offsets[l])
        acc = np.zeros((N * T, C), np.float32)
        for row, w in _corners(x, r, size):             # fma(w, e, acc): one rounding
            e = emb[off + row].astype(np.float64)
            acc = (w.astype(np.float64)[:, None] * e + acc.astype(np.float64)).astype(np.float32)
        p = w2[:, :, None] * acc.reshape(N, T, C)       # fp32 product
        q = np.zeros((4, N, C), np.float32)
        for k in range(T):
            q[k // 8] = q[k // 8] + p[:, k]
        out[:, l * C:(l + 1) * C] = ((q[0] + q[1]) + q[2]) + q[3]
    return out


def emulate_scatter(u2, w2, g, spec, view_width, det, rng, prefill=None):
    """k_sgrid_backward in numpy fp32: contributions, the butterfly merge of
    each 8-slot wave, then fp32 adds in a random order (det=False) or int64
    fixed-point adds and one final rounding (det=True)."""
    offsets, res = sgrid_ref.geometry(spec)
    N = w2.shape[0]
    n_rows = int(offsets[-1])
    order = sgrid_ref.slot_rays(N, view_width)
    G = -(-N // 8)
    slot = np.full(G * 8, order[-1])
    slot[:N] = order
    live = (np.arange(G * 8) < N).reshape(G, 8)
    x = u2[slot].reshape(-1, 3)
    idx = np.arange(8)
    ent_rows, ent_vals = [], []
    for l, r in enumerate(res):
        off, size = int(offsets[l]), int(offsets[l + 1] - offsets[l])
        wg = (w2[slot][:, :, None] * g[slot][:, None, l * C:(l + 1) * C]).reshape(G, 8, T, C)
        for row, w in _corners(x, r, size):
            row = row.reshape(G, 8, T)
            val = w.reshape(G, 8, T, 1) * wg
            alive = np.broadcast_to(live[:, :, None], row.shape).copy()
            for sd in (1, 2, 4):
                p = idx ^ sd
                m = alive & alive[:, p] & (row == row[:, p])
                lower = ((idx & sd) == 0)[None, :, None]
                val = np.where((m & lower)[..., None], val + val[:, p], val)
                alive &= ~(m & ~lower)
            ent_rows.append(off + row[alive])
            ent_vals.append(val[alive])
    rows = np.concatenate(ent_rows)
    vals = np.concatenate(ent_vals)
    out = np.zeros((n_rows, C), np.float32) if prefill is None else prefill.copy()
    if det:
        gmax = np.abs(g[:, :F]).max()
        if gmax == 0:
            return out
        shift = sgrid_ref.det_shift(N, gmax)
        acc = np.zeros((n_rows, C), np.int64)
        np.add.at(acc, rows, np.rint(np.ldexp(vals.astype(np.float64), shift)).astype(np.int64))
        nz = acc != 0
        out[nz] = out[nz] + np.ldexp(acc[nz].astype(np.float64), -shift).astype(np.float32)
        return out
    perm = rng.permutation(rows.shape[0])
    perm = perm[np.argsort(rows[perm], kind="stable")]
    rows, vals = rows[perm], vals[perm]
    first = np.r_[0, np.flatnonzero(np.diff(rows)) + 1]
    rank = np.arange(rows.shape[0]) - np.repeat(first, np.diff(np.r_[first, rows.shape[0]]))
    for k in range(int(rank.max()) + 1):
        s = rank == k
        out[rows[s]] = out[rows[s]] + vals[s]
    return out


# ------------------------------------------------------------------ tests --

def test_table_layouts_are_the_ones_the_cases_name():
    kinds = {log2: sgrid_ref.level_kinds(_spec(log2)) for log2 in sgrid_ref.S_GRID_LOG2}
    assert kinds[11] == ["hashed"] * 16
    assert kinds[14] == ["dense"] * 2 + ["hashed"] * 14
    assert kinds[16] == ["dense"] * 4 + ["hashed"] * 12
    offs, res = sgrid_ref.geometry(_spec(14))
    assert res[:5] == [16, 21, 26, 32, 41] and res[-1] == 512
    assert int(offs[2] - offs[1]) == 9264                  # 21^3 rounded up to 8: no power of two


@pytest.mark.parametrize("log2", sgrid_ref.S_GRID_LOG2)
def test_composite_and_scatter_are_adjoint(log2):
    spec = _spec(log2)
    u2, w2, g = synth_samples("first37", 37)
    rng = np.random.default_rng(5)
    E = rng.standard_normal((int(spec.offsets()[-1]), C)).astype(np.float32)
    f_sam = sgrid_ref.composite(u2, w2, E, spec)[0]
    val = sgrid_ref.scatter(u2, w2, g, spec)[0]
    lhs = float((g[:, :F].astype(np.float64) * f_sam).sum())
    rhs = float((E.astype(np.float64) * val).sum())
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), abs(rhs)), (lhs, rhs)


def test_zero_handling():
    spec = _spec(14)
    u2, w2, g = synth_samples("early100", 100)
    assert (w2 == 0).sum() > 12
    val, abs_w, abs_1, count = sgrid_ref.scatter(u2, w2, g, spec)
    assert count.sum() == int((w2 != 0).sum()) * 8 * 16       # zero-weight samples are not counted
    untouched = count == 0
    assert untouched.any() and not abs_1[untouched].any() and not val[untouched].any()
    assert (abs_1[~untouched] > 0).all()
    # a ray of zero weights gets an exactly-zero f_sam with a zero key
    w0 = w2.copy()
    w0[3] = 0.0
    f_sam, abs_ww, key = sgrid_ref.composite(u2, w0, _emb(spec), spec)
    assert not f_sam[3].any() and not abs_ww[3].any() and not key[3].any()
    assert (key[4] > 0).all()
    # an all-zero gradient has no fixed-point scale and a zero bound
    assert not sgrid_ref.bound_scatter_det(abs_w, count, 100, 0.0).any()


def test_det_shift_follows_exponent_and_ray_count():
    assert sgrid_ref.det_shift(1, 1.0) == 61 - 0 - 1          # 1.0 in [2^0, 2^1)
    assert sgrid_ref.det_shift(64, 0.75) == 61 - 6 - 0
    assert sgrid_ref.det_shift(65, 0.75) == 61 - 7 - 0
    assert sgrid_ref.det_shift(37, 4.5) == 61 - 6 - 3


@pytest.mark.parametrize("log2", sgrid_ref.S_GRID_LOG2)
@pytest.mark.parametrize("name,N,vw", sgrid_ref.RAY_SETS, ids=[r[0] for r in sgrid_ref.RAY_SETS])
def test_fp32_emulation_sits_under_the_bounds(name, N, vw, log2):
    spec = _spec(log2)
    emb = _emb(spec)
    u2, w2, g = synth_samples(name, N)
    rng = np.random.default_rng(N + log2)
    f_sam, abs_ww, key = sgrid_ref.composite(u2, w2, emb, spec)
    r_fwd = grid_ref.worst_ratio(emulate_composite(u2, w2, emb, spec), f_sam,
                                 sgrid_ref.bound_composite(abs_ww, np.abs(emb).max()), key)
    val, abs_w, abs_1, count = sgrid_ref.scatter(u2, w2, g, spec)
    gmax = np.abs(g[:, :F]).max()
    b_at = sgrid_ref.bound_scatter_atomic(abs_w, count, gmax)
    b_det = sgrid_ref.bound_scatter_det(abs_w, count, N, gmax)
    r_at = grid_ref.worst_ratio(emulate_scatter(u2, w2, g, spec, vw, False, rng), val, b_at, abs_1)
    r_det = grid_ref.worst_ratio(emulate_scatter(u2, w2, g, spec, vw, True, rng), val, b_det, abs_1)
    # onto a prefill: untouched elements keep it bit for bit (worst_ratio)
    P = rng.standard_normal(val.shape).astype(np.float32)
    tot = P.astype(np.float64) + val
    r_pat = grid_ref.worst_ratio(emulate_scatter(u2, w2, g, spec, vw, False, rng, P), tot,
                                 b_at + sgrid_ref.bound_prefill_atomic(P, count), abs_1, prefill=P)
    r_pdet = grid_ref.worst_ratio(emulate_scatter(u2, w2, g, spec, vw, True, rng, P), tot,
                                  b_det + sgrid_ref.bound_prefill_det(tot), abs_1, prefill=P)
    print(f"emulation {name} N={N} L2={log2}: forward {r_fwd:.3f} atomic {r_at:.3f} det {r_det:.3f} "
          f"prefill atomic {r_pat:.3f} det {r_pdet:.3f}")
    assert max(r_fwd, r_at, r_det, r_pat, r_pdet) <= 1.0
