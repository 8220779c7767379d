"""Pin tests/grid_ref.py (float64 numpy reference of the grid encoder, any D),
then pin the C oracle against it over every compiled form.  CPU only.

1. The reference against things that are neither it nor the oracle:
   F.grid_sample on dense levels (2-D and 3-D), hand-computed hash / tiled
   rows, adjointness in float64, dy_dx against central differences.
2. oracle/encoders_oracle.c against the reference for D = 2..5, every C, all
   8 (gridtype, align_corners, interpolation) modes, within the derived fp32
   bounds of grid_ref.bound_*; its corner rows must be equal exactly.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import grid_ref as gr
from oracle import encoders as enc

DIMS = (2, 3, 4, 5)


# ------------------------------------------------ reference: known answers --

@pytest.mark.parametrize("D", [2, 3])
def test_reference_dense_levels_equal_grid_sample(D):
    """Dense levels, linear, align_corners off == F.grid_sample(bilinear,
    border, align_corners=False) in float64, up to the fp32 position step."""
    H, L, C = (9, 3, 3) if D == 2 else (5, 3, 2)
    scale = 1.5
    offsets = gr.grid_offsets(D, H, scale, L, log2_cap=20)
    res = enc.grid_level_resolutions(L, float(np.log2(scale)), H)
    rng = np.random.default_rng(D)
    emb = rng.uniform(-1, 1, (int(offsets[-1]), C)).astype(np.float32)
    x = rng.uniform(0, 1, (500, D)).astype(np.float32)
    x[:4] = [[0] * D, [1] * D, [0.5] * D, [1e-7, 0.999999, 0.25][:D]]
    val = gr.forward(x, emb, offsets, res)[0]
    for l in range(L):
        r, size = res[l], int(offsets[l + 1] - offsets[l])
        assert gr.strides_used(r, size, D) == (D, False), "test needs dense levels"
        vol = torch.from_numpy(emb[offsets[l]:offsets[l] + r ** D].astype(np.float64))
        vol = vol.view(*([r] * D), C).permute(D, *range(D))[None]        # [1, C, (z,) y, x]
        g = torch.from_numpy(2 * x.astype(np.float64) - 1).view(1, *([1] * (D - 1)), -1, D)
        ref = F.grid_sample(vol, g, mode="bilinear", padding_mode="border", align_corners=False)
        ref = ref.reshape(C, -1).T.numpy()
        # position rounded to fp32 (2^-24 * res cells) times the largest slope (2 per axis)
        np.testing.assert_allclose(val[l], ref, rtol=0, atol=2 * D * r * 2.0 ** -23)


def _literal_cells(D):
    """Hand-written cells and their rows: (res, size, gridtype, cell, row)."""
    P = gr.PRIMES
    M = 0xFFFFFFFF
    if D == 2:
        return [
            # hash, stride overran (37^2 > 1024): xor of cell * prime
            (37, 1024, 0, (5, 9), (5 ^ ((9 * 2654435761) & M)) % 1024),
            (37, 1024, 0, (36, 36), (36 ^ ((36 * 2654435761) & M)) % 1024),
            # tiled, same level: 5 + 9*37 = 338; 36 + 36*37 = 1368 -> 1368 % 1024 = 344
            (37, 1024, 1, (5, 9), 338),
            (37, 1024, 1, (36, 36), 344),
            # hash table on a dense level indexes densely: 3 + 7*16 = 115
            (16, 256, 0, (3, 7), 115),
        ]
    if D == 4:
        return [
            (10, 1024, 0, (1, 2, 3, 4),
             (1 ^ ((2 * P[1]) & M) ^ ((3 * P[2]) & M) ^ ((4 * P[3]) & M)) % 1024),
            (10, 1024, 0, (9, 0, 9, 5),
             (9 ^ 0 ^ ((9 * P[2]) & M) ^ ((5 * P[3]) & M)) % 1024),
            # tiled: strides 1, 10, 100, 1000 all <= 1024: 1 + 20 + 300 + 4000 = 4321 % 1024 = 225
            (10, 1024, 1, (1, 2, 3, 4), 225),
            # tiled, res 40: strides 1, 40 then 1600 > 1024 stops before axis 2:
            # 7 + 11*40 = 447, axes 2 and 3 ignored
            (40, 1024, 1, (7, 11, 39, 39), 447),
            (40, 1024, 1, (39, 39, 0, 1), (39 + 39 * 40) % 1024),
        ]
    if D == 5:
        return [
            (6, 1024, 0, (1, 2, 3, 4, 5),
             (1 ^ ((2 * P[1]) & M) ^ ((3 * P[2]) & M) ^ ((4 * P[3]) & M) ^ ((5 * P[4]) & M)) % 1024),
            (6, 1024, 0, (5, 5, 5, 5, 5),
             (5 ^ ((5 * P[1]) & M) ^ ((5 * P[2]) & M) ^ ((5 * P[3]) & M) ^ ((5 * P[4]) & M)) % 1024),
            # tiled, res 6: strides 1, 6, 36, 216 then 1296 > 1024 stops before
            # the last axis: 1 + 12 + 108 + 864 = 985
            (6, 1024, 1, (1, 2, 3, 4, 5), 985),
            # 5 + 30 + 180 + 1080 = 1295 % 1024 = 271
            (6, 1024, 1, (5, 5, 5, 5, 0), 271),
        ]
    raise AssertionError(D)


@pytest.mark.parametrize("D", [2, 4, 5])
def test_reference_rows_literal(D):
    for res, size, gridtype, cell, row in _literal_cells(D):
        assert int(gr.corner_rows(np.array([cell]), res, size, gridtype)[0]) == row, (res, cell)
    # the prime table itself, from the instant-ngp paper's coherent hash
    assert gr.PRIMES[:5] == (1, 2654435761, 805459861, 3674653429, 2097192037)


def test_reference_forward_reads_literal_rows():
    """forward() at a cell centre reads exactly the 2^D literal rows: D = 4,
    tiled, res 40 (the stride stops after two axes)."""
    D, res, size = 4, 40, 1024
    offsets = np.array([0, size], np.int32)
    x = ((np.array([[7, 11, 38, 2]]) + 0.75) / res).astype(np.float32)      # cell (7, 11, 38, 2)
    rows = gr.forward(x, np.zeros((size, 1), np.float32), offsets, [res], gridtype=1)[3]
    want = [(7 + (c & 1)) + (11 + ((c >> 1) & 1)) * 40 for c in range(16)]
    assert rows[0, 0].tolist() == want


@pytest.mark.parametrize("D", DIMS)
def test_reference_backward_is_adjoint_in_float64(D):
    """<backward(g), emb> == <g, forward(emb)>, every mode, to 1e-12."""
    cs = gr.case(D)
    C = 2
    emb, g = cs.emb(C), cs.grad(C)
    for gridtype, align, interp in gr.MODES:
        val = gr.forward(cs.x, emb, cs.offsets, cs.res, gridtype, align, interp)[0]
        gemb, _, _, count = gr.backward_embeddings(g, cs.x, cs.rows, cs.offsets, cs.res, gridtype,
                                                   align, interp)
        lhs = float((g.astype(np.float64) * val).sum())
        rhs = float((gemb * emb.astype(np.float64)).sum())
        assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), abs(rhs)), (gridtype, align, interp)
        inside = int(gr.inside_mask(cs.x).sum())
        assert int(count.sum()) == inside * cs.L * (1 << D)


@pytest.mark.parametrize("D", DIMS)
def test_reference_dy_dx_matches_central_differences(D):
    """dy_dx against central differences of the float64-position forward, on
    points at least 0.05 of a cell away from every cell face (and from the
    clamped border half-cells) at every level."""
    cs = gr.case(D)
    C = 2
    emb = cs.emb(C)
    rng = np.random.default_rng(D)
    h = 1e-7
    for gridtype, align, interp in gr.MODES:
        x = rng.uniform(0, 1, (40000, D))
        keep = np.ones(len(x), bool)
        for r in cs.res:
            p = x * (r - 1) if align else x * r - 0.5
            fr = p - np.floor(p)
            keep &= ((fr > 0.05) & (fr < 0.95) & (p > 0.05) & (p < r - 1.05)).all(1)
        x = x[keep][:64]
        assert len(x) >= 16
        dy, _, abs_1 = gr.dy_dx(x, emb, cs.offsets, cs.res, gridtype, align, interp, exact=True)
        for ax in range(D):
            xp, xm = x.copy(), x.copy()
            xp[:, ax] += h
            xm[:, ax] -= h
            fp = gr.forward(xp, emb, cs.offsets, cs.res, gridtype, align, interp, exact=True)[0]
            fm = gr.forward(xm, emb, cs.offsets, cs.res, gridtype, align, interp, exact=True)[0]
            num = ((fp - fm) / (2 * h)).transpose(1, 0, 2)                    # [B, L, C]
            # cancellation in fp - fm: ~2^-52 * |f| / h ~ 1e-8; curvature h^2 res^3 negligible
            err = np.abs(dy[:, :, ax] - num)
            assert (err <= 1e-6 * (1 + abs_1[:, :, ax])).all(), (gridtype, align, interp, err.max())


def test_reference_weight_decay_and_input_backward_closed_forms():
    offsets = np.array([0, 8, 24], np.int32)
    emb = np.arange(48, dtype=np.float32).reshape(24, 2)
    wd = gr.weight_decay(emb, offsets, 0.5)
    assert wd[3, 1] == 2 * 0.5 * 7 / 8 and wd[10, 0] == 2 * 0.5 * 20 / 16
    g = np.ones((2, 3, 2), np.float32)
    dy = np.arange(3 * 2 * 2 * 2, dtype=np.float32).reshape(3, 2, 2, 2)
    val, ab = gr.backward_inputs(g, dy)
    assert np.array_equal(val, dy.astype(np.float64).sum(axis=(1, 3))) and np.array_equal(val, ab)


def test_case_geometry():
    """From the offsets: every D has dense and hashed levels, and D >= 3 has
    a level with res^(D-1) > size (res^2 > size at D = 3), where the tiled
    stride sum stops before the last axis."""
    for D in DIMS:
        cs = gr.case(D)
        kinds = cs.level_kinds()
        sizes = np.diff(cs.offsets)
        assert sum(1 for k in kinds if not k[1]) >= 2, (D, kinds)
        assert sum(1 for k in kinds if k[1]) >= 3, (D, kinds)
        assert (sizes <= 2 ** gr.LOG2_CAP).all()
        if D >= 3:
            assert any(r ** (D - 1) > s for r, s in zip(cs.res, sizes)), (D, cs.res, sizes)
            assert any(used < D for used, _ in kinds)
        assert cs.x.shape == (gr.B_POINTS, D) and not gr.inside_mask(cs.x).all()


# -------------------------------------------------- oracle vs the reference --

_WORST = {}


@pytest.fixture
def worst(request):
    """Per-test worst error / bound per quantity, printed after the test."""
    w = {}
    yield w
    if w:
        print(f"\n{request.node.name}: worst error / bound",
              {k: round(v, 3) for k, v in sorted(w.items())})
    for k, v in w.items():
        _WORST[k] = max(_WORST.get(k, 0.0), v)


@pytest.fixture(scope="module", autouse=True)
def _worst_over_the_module():
    yield
    print("\nworst oracle error / bound:", {k: round(v, 3) for k, v in sorted(_WORST.items())})


def _note(worst, key, ratio):
    worst[key] = max(worst.get(key, 0.0), ratio)
    return ratio


@pytest.mark.parametrize("C", gr.CHANNELS)
@pytest.mark.parametrize("D", DIMS)
def test_oracle_matches_reference_every_form(oracle_lib, worst, D, C):
    cs = gr.case(D)
    emb, g = cs.emb(C), cs.grad(C)
    x, offs, L = cs.x, cs.offsets, cs.L
    for gridtype, align, interp in gr.MODES:
        mode = (gridtype, align, interp)
        kw = dict(gridtype=gridtype, align_corners=align, interp=interp)
        out, dy, rows = enc.grid_encode_forward(x, emb, offs, L, cs.S, cs.H, calc_dy_dx=True,
                                                return_rows=True, **kw)
        val, abs_w, abs_1, ref_rows = gr.forward(x, emb, offs, cs.res, *mode)
        # corner rows: integers, equal exactly
        assert np.array_equal(rows, ref_rows), mode
        # forward: u * ((2^D + D + m) abs_w + 4 D s abs_1)  (grid_ref.bound_forward)
        r = _note(worst, "forward", gr.worst_ratio(out, val, gr.bound_forward(D, interp, abs_w, abs_1),
                                                   abs_1))
        assert r <= 1.0, ("forward", mode, r)
        # dy_dx: u * ((2^(D-1) + D + 6) abs_w + 4 (D-1) s abs_1)  (grid_ref.bound_dy_dx)
        dval, dabs_w, dabs_1 = gr.dy_dx(x, emb, offs, cs.res, *mode)
        r = _note(worst, "dy_dx", gr.worst_ratio(dy.reshape(dval.shape), dval,
                                                 gr.bound_dy_dx(D, interp, dabs_w, dabs_1), dabs_1))
        assert r <= 1.0, ("dy_dx", mode, r)
        # grad_embeddings: u * ((count + D + m) abs_w + 4 D s abs_1), per element
        dy32 = dval.astype(np.float32)
        gemb, gin = enc.grid_encode_backward(g, x, emb, offs, L, cs.S, cs.H,
                                             dy_dx=dy32.reshape(len(x), -1), **kw)
        bval, babs_w, babs_1, count = gr.backward_embeddings(g, x, cs.rows, offs, cs.res, *mode)
        r = _note(worst, "grad_embeddings", gr.worst_ratio(
            gemb, bval, gr.bound_grad_embeddings(D, interp, babs_w, babs_1, count), babs_1))
        assert r <= 1.0, ("grad_embeddings", mode, r)
        # grad_inputs from the reference's dy_dx in fp32: (L C + 1) u sum |g dy|
        ival, iabs = gr.backward_inputs(g, dy32)
        r = _note(worst, "grad_inputs", gr.worst_ratio(gin, ival, gr.bound_grad_inputs(L, C, iabs), iabs))
        assert r <= 1.0, ("grad_inputs", mode, r)
        if interp == 0:
            # TV: u * ((3 D + 7) abs_v + count abs_c), per element
            tv = enc.grad_total_variation(x, emb, np.zeros_like(emb), offs, 0.37, L, cs.S, cs.H,
                                          gridtype=gridtype, align_corners=align)
            tval, abs_c, abs_v, tcount = gr.total_variation(x, emb, offs, cs.res, 0.37, gridtype, align)
            r = _note(worst, "tv", gr.worst_ratio(tv, tval, gr.bound_tv(D, abs_c, abs_v, tcount), abs_v))
            assert r <= 1.0, ("tv", mode, r)
    wd = enc.grad_weight_decay(emb, np.zeros_like(emb), offs, 0.1, L)
    np.testing.assert_allclose(wd, gr.weight_decay(emb, offs, 0.1), rtol=2.0 ** -22, atol=0)


@pytest.mark.parametrize("D", DIMS)
def test_oracle_max_level_and_rows(oracle_lib, D):
    """A level cap leaves the higher levels of the oracle's outputs at zero and
    out of the backward; rows match at every cap."""
    cs = gr.case(D)
    C = 2
    emb, g = cs.emb(C), cs.grad(C)
    for ml in (0, 1, cs.L - 1):
        out, rows = enc.grid_encode_forward(cs.x, emb, cs.offsets, cs.L, cs.S, cs.H, max_level=ml,
                                            return_rows=True, gridtype=1, align_corners=True, interp=1)
        val, abs_w, abs_1, ref_rows = gr.forward(cs.x, emb, cs.offsets, cs.res, 1, True, 1, max_level=ml)
        assert np.array_equal(rows[:ml], ref_rows[:ml]) and not out[ml:].any()
        assert gr.worst_ratio(out, val, gr.bound_forward(D, 1, abs_w, abs_1), abs_1) <= 1.0
        gemb = enc.grid_encode_backward(g, cs.x, emb, cs.offsets, cs.L, cs.S, cs.H, max_level=ml,
                                        gridtype=1, align_corners=True, interp=1)
        assert not gemb[cs.offsets[ml]:].any()
