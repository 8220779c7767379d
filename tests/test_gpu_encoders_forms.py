"""Every compiled form of the drop-in encoders on the MI355X against the
float64 reference (tests/grid_ref.py) and the C oracle.

Grid: all 24 (D, C) instantiations of k_grid_forward, k_grid_backward,
k_input_backward and k_grad_tv, each over the 8 (gridtype, align_corners,
interpolation) modes, at the points of grid_ref.make_points (faces, corners of
the unit cube, outside points, many points in one cell).  Error bounds are the
derived ones of grid_ref.bound_* (u = 2^-24; they hold for any summation order,
so float atomics and the butterfly merge are covered); no element is masked,
and an element nothing contributes to must be +0.0 / its prefill bit for bit.
SH and frequency encoder edges follow.
"""
import numpy as np
import pytest
import torch

import grid_ref as gr
from oracle import encoders as enc

pytestmark = pytest.mark.gpu

DIMS = (2, 3, 4, 5)
SENTINEL = -12345.678
TV_WEIGHT = 0.37


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
    print("\nworst kernel error / bound:", {k: round(v, 3) for k, v in sorted(_WORST.items())})


def _note(worst, key, ratio):
    worst[key] = max(worst.get(key, 0.0), ratio)
    return ratio


class Dev:
    """Device copies of one case's tensors + thin calls into _gridencoder."""

    def __init__(self, cs, x, emb, cuda):
        self.cs, self.cuda = cs, cuda
        self.B, self.D, self.C = x.shape[0], cs.D, emb.shape[1]
        self.x = torch.from_numpy(x).to(cuda)
        self.emb = torch.from_numpy(emb).to(cuda)
        self.offs = torch.from_numpy(cs.offsets).to(cuda)

    def forward(self, mode, max_level=None, dy=True, fill=0.0):
        import _gridencoder
        cs = self.cs
        out = torch.full((cs.L, self.B, self.C), fill, device=self.cuda)
        dyt = torch.full((self.B, cs.L * self.D * self.C), fill, device=self.cuda) if dy else None
        _gridencoder.grid_encode_forward(self.x, self.emb, self.offs, out, self.B, self.D, self.C,
                                         cs.L, cs.L if max_level is None else max_level, cs.S,
                                         cs.H, dyt, mode[0], mode[1], mode[2])
        return out.cpu().numpy(), (dyt.cpu().numpy().reshape(self.B, cs.L, self.D, self.C)
                                   if dy else None)

    def backward(self, mode, g, dy=None, max_level=None, gemb0=None, gin_fill=0.0):
        import _gridencoder
        cs = self.cs
        ge = (torch.zeros(self.emb.shape, device=self.cuda) if gemb0 is None
              else torch.from_numpy(gemb0).to(self.cuda))
        gi = torch.full((self.B, self.D), gin_fill, device=self.cuda) if dy is not None else None
        dyt = torch.from_numpy(dy.reshape(self.B, -1)).to(self.cuda) if dy is not None else None
        _gridencoder.grid_encode_backward(torch.from_numpy(g).to(self.cuda), self.x, self.emb,
                                          self.offs, ge, self.B, self.D, self.C, cs.L,
                                          cs.L if max_level is None else max_level, cs.S, cs.H,
                                          dyt, gi, mode[0], mode[1], mode[2])
        return ge.cpu().numpy(), (gi.cpu().numpy() if gi is not None else None)

    def tv(self, gridtype, align, grad0=None, weight=TV_WEIGHT):
        import _gridencoder
        cs = self.cs
        gt = (torch.zeros(self.emb.shape, device=self.cuda) if grad0 is None
              else torch.from_numpy(grad0).to(self.cuda))
        _gridencoder.grad_total_variation(self.x, self.emb, gt, self.offs, weight, self.B, self.D,
                                          self.C, cs.L, cs.S, cs.H, gridtype, align)
        return gt.cpu().numpy()

    def wd(self, grad0=None, weight=0.1):
        import _gridencoder
        gt = (torch.zeros(self.emb.shape, device=self.cuda) if grad0 is None
              else torch.from_numpy(grad0).to(self.cuda))
        _gridencoder.grad_weight_decay(self.emb, gt, self.offs, weight, self.emb.shape[0], self.C,
                                       self.cs.L)
        return gt.cpu().numpy()


def test_case_geometry_from_offsets():
    """The configurations reach a dense level, a hashed level and, for
    D >= 3, a level whose tiled stride sum stops before the last axis
    (res^(D-1) > size; res^2 > size at D = 3)."""
    for D in DIMS:
        cs = gr.case(D)
        sizes = np.diff(cs.offsets)
        assert sum(r ** D <= s for r, s in zip(cs.res, sizes)) >= 2
        assert sum(r ** D > s for r, s in zip(cs.res, sizes)) >= 3
        if D >= 3:
            assert any(r ** (D - 1) > s for r, s in zip(cs.res, sizes))


# ------------------------------------------------------------ full matrix --

@pytest.mark.parametrize("C", gr.CHANNELS)
@pytest.mark.parametrize("D", DIMS)
def test_grid_every_form(hip_lib, oracle_lib, cuda, worst, D, C):
    cs = gr.case(D)
    emb, g, x = cs.emb(C), cs.grad(C), cs.x
    dev = Dev(cs, x, emb, cuda)
    outside = ~gr.inside_mask(x)
    assert outside.sum() >= 2
    for mode in gr.MODES:
        gridtype, align, interp = mode
        out, dy = dev.forward(mode, fill=SENTINEL)
        # forward: bit-equal to the C oracle ...
        ref32 = enc.grid_encode_forward(x, emb, cs.offsets, cs.L, cs.S, cs.H, gridtype=gridtype,
                                        align_corners=align, interp=interp)
        assert np.array_equal(out.view(np.uint32), ref32.view(np.uint32)), mode
        # ... and within u * ((2^D + D + m) abs_w + 4 D s abs_1) of the reference
        # (2^D fmas, D + m roundings per weight; smoothstep weights are absolute)
        val, abs_w, abs_1, _ = gr.forward(x, emb, cs.offsets, cs.res, *mode)
        r = _note(worst, "forward", gr.worst_ratio(out, val, gr.bound_forward(D, interp, abs_w, abs_1),
                                                   abs_1))
        assert r <= 1.0, ("forward", mode, r)
        # dy_dx: u * ((2^(D-1) + D + 6) abs_w + 4 (D-1) s abs_1); outside rows +0.0
        dval, dabs_w, dabs_1 = gr.dy_dx(x, emb, cs.offsets, cs.res, *mode)
        r = _note(worst, "dy_dx", gr.worst_ratio(dy, dval, gr.bound_dy_dx(D, interp, dabs_w, dabs_1),
                                                 dabs_1))
        assert r <= 1.0, ("dy_dx", mode, r)
        assert not dy[outside].view(np.uint32).any() and not out[:, outside].view(np.uint32).any()
        # grad_embeddings, per element: u * ((count[row] + D + m) abs_w + 4 D s abs_1)
        # (count additions in any order: atomics + butterfly)
        dy32 = dval.astype(np.float32)
        gemb, gin = dev.backward(mode, g, dy=dy32, gin_fill=SENTINEL)
        bval, babs_w, babs_1, count = gr.backward_embeddings(g, x, cs.rows, cs.offsets, cs.res, *mode)
        r = _note(worst, "grad_embeddings", gr.worst_ratio(
            gemb, bval, gr.bound_grad_embeddings(D, interp, babs_w, babs_1, count), babs_1))
        assert r <= 1.0, ("grad_embeddings", mode, r)
        # grad_inputs from the reference's dy_dx rounded to fp32, overwriting the
        # sentinel: one fma chain of L*C terms, (L C + 1) u sum |g dy|
        ival, iabs = gr.backward_inputs(g, dy32)
        r = _note(worst, "grad_inputs", gr.worst_ratio(gin, ival, gr.bound_grad_inputs(cs.L, C, iabs),
                                                       iabs))
        assert r <= 1.0, ("grad_inputs", mode, r)
        if interp == 0:
            # TV, per element: u * ((3 D + 7) abs_v + count[row] abs_c)  (rsqrtf <= 2 ulp)
            tv = dev.tv(gridtype, align)
            tval, abs_c, abs_v, tcount = gr.total_variation(x, emb, cs.offsets, cs.res, TV_WEIGHT,
                                                            gridtype, align)
            r = _note(worst, "tv", gr.worst_ratio(tv, tval, gr.bound_tv(D, abs_c, abs_v, tcount), abs_v))
            assert r <= 1.0, ("tv", mode, r)
    # weight decay: (2 w) * e / size, three roundings
    np.testing.assert_allclose(dev.wd(), gr.weight_decay(emb, cs.offsets, 0.1), rtol=2.0 ** -22, atol=0)


@pytest.mark.parametrize("C,B", [(1, 65), (2, 33), (32, 3), (1, 1)])
@pytest.mark.parametrize("D", DIMS)
def test_grid_backward_partial_last_wave(hip_lib, cuda, worst, D, C, B):
    """B * C is no multiple of 64: the last wave's tail lanes stay alive for
    the shuffles on the point B - 1 and must add nothing."""
    cs = gr.case(D)
    x = gr.tail_points(cs, B)
    emb, g = cs.emb(C), cs.grad(C, B)
    dev = Dev(cs, x, emb, cuda)
    for mode in gr.MODES:
        gemb, _ = dev.backward(mode, g)
        bval, babs_w, babs_1, count = gr.backward_embeddings(g, x, cs.rows, cs.offsets, cs.res, *mode)
        # per element: u * ((count[row] + D + m) abs_w + 4 D s abs_1)
        r = _note(worst, "grad_embeddings_tail", gr.worst_ratio(
            gemb, bval, gr.bound_grad_embeddings(D, mode[2], babs_w, babs_1, count), babs_1))
        assert r <= 1.0, (mode, r)


# -------------------------------------------------------------- max_level --

@pytest.mark.parametrize("D,C", [(2, 2), (3, 8), (4, 1), (5, 4)])
def test_grid_max_level_leaves_higher_levels_untouched(hip_lib, oracle_lib, cuda, worst, D, C):
    cs = gr.case(D)
    emb, g, x = cs.emb(C), cs.grad(C), cs.x
    dev = Dev(cs, x, emb, cuda)
    sent = np.float32(SENTINEL).view(np.uint32)
    prefill = np.random.default_rng(D).standard_normal(emb.shape).astype(np.float32)
    for ml in (0, 1, cs.L - 1, cs.L):
        for mode in ((0, False, 0), (1, True, 1)):
            out, dy = dev.forward(mode, max_level=ml, fill=SENTINEL)
            assert (out[ml:].view(np.uint32) == sent).all() and (dy[:, ml:].view(np.uint32) == sent).all()
            ref32 = enc.grid_encode_forward(x, emb, cs.offsets, cs.L, cs.S, cs.H, max_level=ml,
                                            gridtype=mode[0], align_corners=mode[1], interp=mode[2])
            assert np.array_equal(out[:ml].view(np.uint32), ref32[:ml].view(np.uint32))
            dval, dabs_w, dabs_1 = gr.dy_dx(x, emb, cs.offsets, cs.res, *mode, max_level=ml)
            # u * ((2^(D-1) + D + 6) abs_w + 4 (D-1) s abs_1) on the levels below the cap
            assert _note(worst, "dy_dx", gr.worst_ratio(
                np.ascontiguousarray(dy[:, :ml]), dval[:, :ml],
                gr.bound_dy_dx(D, mode[2], dabs_w, dabs_1)[:, :ml], dabs_1[:, :ml])) <= 1.0
            gemb, _ = dev.backward(mode, g, max_level=ml, gemb0=prefill)
            first = int(cs.offsets[ml])
            assert np.array_equal(gemb[first:].view(np.uint32), prefill[first:].view(np.uint32))
            assert ml == 0 or not np.array_equal(gemb[:first], prefill[:first])


# ---------------------------------------------------- accumulate contracts --

@pytest.mark.parametrize("D,C", [(2, 16), (3, 1), (4, 32), (5, 2)])
def test_grid_gradients_accumulate_into_prefill(hip_lib, cuda, worst, D, C):
    """grad_embeddings and the TV / weight-decay `grad` are added to what the
    buffer holds.  Each of the count[row] additions now rounds a running sum
    that includes the prefill, so the bound gains (count + 1) u |prefill|."""
    cs = gr.case(D)
    emb, g, x = cs.emb(C), cs.grad(C), cs.x
    dev = Dev(cs, x, emb, cuda)
    prefill = np.random.default_rng(50 + D).standard_normal(emb.shape).astype(np.float32)
    p64 = prefill.astype(np.float64)
    for mode in ((0, True, 1), (1, False, 0)):
        gemb, _ = dev.backward(mode, g, gemb0=prefill)
        bval, babs_w, babs_1, count = gr.backward_embeddings(g, x, cs.rows, cs.offsets, cs.res, *mode)
        bound = gr.bound_grad_embeddings(D, mode[2], babs_w, babs_1, count) \
            + gr.U * (count[:, None] + 1) * np.abs(p64)
        assert _note(worst, "grad_embeddings_prefilled",
                     gr.worst_ratio(gemb, p64 + bval, bound, babs_1, prefill=prefill)) <= 1.0, mode
        tv = dev.tv(mode[0], mode[1], grad0=prefill)
        tval, abs_c, abs_v, tcount = gr.total_variation(x, emb, cs.offsets, cs.res, TV_WEIGHT,
                                                        mode[0], mode[1])
        bound = gr.bound_tv(D, abs_c, abs_v, tcount) + gr.U * (tcount[:, None] + 1) * np.abs(p64)
        assert _note(worst, "tv_prefilled",
                     gr.worst_ratio(tv, p64 + tval, bound, abs_v, prefill=prefill)) <= 1.0, mode
    # weight decay: the term to rtol 2^-22, then one rounded addition
    wref = gr.weight_decay(emb, cs.offsets, 0.1)
    err = np.abs(dev.wd(grad0=prefill).astype(np.float64) - (p64 + wref))
    assert (err <= 2.0 ** -22 * np.abs(wref) + gr.U * np.abs(p64 + wref)).all()


# --------------------------------------------------------- argument checks --

def test_grid_zero_points_is_a_no_op(hip_lib, cuda):
    import _gridencoder
    cs = gr.case(3)
    C = 2
    dev = Dev(cs, cs.x[:8], cs.emb(C), cuda)
    mk = lambda *shape: torch.full(shape, SENTINEL, device=cuda)
    out, dy, ge, gi, gt = mk(cs.L, 8, C), mk(8, cs.L * 3 * C), mk(cs.rows, C), mk(8, 3), mk(cs.rows, C)
    g = mk(cs.L, 8, C)
    _gridencoder.grid_encode_forward(dev.x, dev.emb, dev.offs, out, 0, 3, C, cs.L, cs.L, cs.S, cs.H,
                                     dy, 0, False, 0)
    _gridencoder.grid_encode_backward(g, dev.x, dev.emb, dev.offs, ge, 0, 3, C, cs.L, cs.L, cs.S,
                                      cs.H, dy, gi, 0, False, 0)
    _gridencoder.grad_total_variation(dev.x, dev.emb, gt, dev.offs, 1.0, 0, 3, C, cs.L, cs.S, cs.H,
                                      0, False)
    torch.cuda.synchronize()
    for t in (out, dy, ge, gi, gt):
        assert bool((t == SENTINEL).all())


@pytest.mark.parametrize("D,C,msg", [(1, 2, "D must be 2, 3, 4 or 5"), (6, 2, "D must be 2, 3, 4 or 5"),
                                     (3, 3, "C must be 1, 2, 4, 8, 16 or 32"),
                                     (3, 64, "C must be 1, 2, 4, 8, 16 or 32")])
def test_grid_rejects_uncompiled_forms(hip_lib, cuda, D, C, msg):
    import _gridencoder
    z = lambda *shape: torch.zeros(shape, device=cuda)
    offs = torch.tensor([0, 8, 16], dtype=torch.int32, device=cuda)
    x, emb, out, dy, gi = z(4, D), z(16, C), z(2, 4, C), z(4, 2 * D * C), z(4, D)
    with pytest.raises(RuntimeError, match=msg):
        _gridencoder.grid_encode_forward(x, emb, offs, out, 4, D, C, 2, 2, 1.0, 2, dy, 0, False, 0)
    with pytest.raises(RuntimeError, match=msg):
        _gridencoder.grid_encode_backward(out, x, emb, offs, z(16, C), 4, D, C, 2, 2, 1.0, 2, dy, gi,
                                          0, False, 0)
    with pytest.raises(RuntimeError, match=msg):
        _gridencoder.grad_total_variation(x, emb, z(16, C), offs, 1.0, 4, D, C, 2, 1.0, 2, 0, False)


# ------------------------------------------------------------ module level --

@pytest.mark.parametrize("D,C", [(2, 2), (3, 4)])
def test_grid_encoder_module_tiled_smoothstep_align(hip_lib, cuda, worst, D, C):
    """GridEncoder(tiled, smoothstep, align_corners) under autograd with
    bound = 2, max_level = 2 and inputs that require grad."""
    from gridencoder import GridEncoder
    H, scale, L = gr.CONFIGS[D]
    ge = GridEncoder(input_dim=D, num_levels=L, level_dim=C, per_level_scale=scale, base_resolution=H,
                     log2_hashmap_size=gr.LOG2_CAP, gridtype="tiled", interpolation="smoothstep",
                     align_corners=True).to(cuda)
    cs = gr.case(D)
    assert np.array_equal(ge.offsets_host, cs.offsets)
    emb = cs.emb(C)
    with torch.no_grad():
        ge.embeddings.copy_(torch.from_numpy(emb))
    bound, ml, mode = 2, 2, (1, True, 1)
    xin = (torch.from_numpy(cs.x).to(cuda) * (2 * bound) - bound).requires_grad_()
    y = ge(xin, bound=bound, max_level=ml)
    B = cs.x.shape[0]
    assert y.shape == (B, L * C)
    x01 = ((xin.detach() + bound) / (2 * bound)).cpu().numpy()      # what the kernel was given
    val, abs_w, abs_1, _ = gr.forward(x01, emb, cs.offsets, cs.res, *mode, max_level=ml)
    got = np.ascontiguousarray(y.detach().cpu().numpy().reshape(B, L, C).transpose(1, 0, 2))
    assert not got[ml:].view(np.uint32).any()
    # u * ((2^D + D + m) abs_w + 4 D s abs_1)
    assert _note(worst, "module_forward",
                 gr.worst_ratio(got, val, gr.bound_forward(D, 1, abs_w, abs_1), abs_1)) <= 1.0
    w = torch.from_numpy(np.random.default_rng(D).standard_normal((B, L * C)).astype(np.float32)).to(cuda)
    (y * w).sum().backward()
    g = np.ascontiguousarray(w.cpu().numpy().reshape(B, L, C).transpose(1, 0, 2))
    bval, babs_w, babs_1, count = gr.backward_embeddings(g, x01, cs.rows, cs.offsets, cs.res, *mode,
                                                         max_level=ml)
    # u * ((count[row] + D + m) abs_w + 4 D s abs_1)
    assert _note(worst, "module_grad_embeddings", gr.worst_ratio(
        ge.embeddings.grad.cpu().numpy(), bval,
        gr.bound_grad_embeddings(D, 1, babs_w, babs_1, count), babs_1)) <= 1.0
    # inputs.grad = (sum g dy_dx) / (2 bound): the kernel contracts its own fp32
    # dy_dx, so the dy_dx bound enters weighted by |g|, plus the fma chain
    dval, dabs_w, dabs_1 = gr.dy_dx(x01, emb, cs.offsets, cs.res, *mode, max_level=ml)
    ival, iabs = gr.backward_inputs(g, dval)
    dyb = gr.bound_dy_dx(D, 1, dabs_w, dabs_1)
    ibound = gr.bound_grad_inputs(L, C, iabs) + \
        (np.abs(g.astype(np.float64)).transpose(1, 0, 2)[:, :, None, :] * dyb).sum(axis=(1, 3)) * (1 + gr.U)
    assert _note(worst, "module_grad_inputs", gr.worst_ratio(
        xin.grad.cpu().numpy(), ival / (2 * bound), ibound / (2 * bound),
        dabs_1.sum(axis=(1, 3)))) <= 1.0


# ---------------------------------------------------------------- SH edges --

def _sh_dirs(B, seed):
    rng = np.random.default_rng(seed)
    d = rng.standard_normal((max(B, 8), 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    edge = np.array([[1e-7, 0, 1], [0, -1e-7, -1], [1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0],
                     [0, 0, 1], [0, 0, -1]], np.float64)
    return np.ascontiguousarray(np.concatenate([edge, d])[:B].astype(np.float32))


@pytest.mark.parametrize("B", [1, 255, 257])
@pytest.mark.parametrize("degree", [1, 2, 3, 4, 5, 6, 7, 8])
def test_sh_forward_without_dy_dx_and_accumulating_backward(hip_lib, oracle_lib, cuda, degree, B):
    import _shencoder
    C2 = degree * degree
    d = _sh_dirs(B, degree)
    ref, rdy = enc.sh_encode_forward(d, degree, calc_dy_dx=True)
    di = torch.from_numpy(d).to(cuda)
    out = torch.full((B, C2), SENTINEL, device=cuda)
    _shencoder.sh_encode_forward(di, out, B, 3, degree, None)               # the no-dy_dx branch
    np.testing.assert_allclose(out.cpu().numpy(), ref, rtol=1e-6, atol=1e-6)
    # backward accumulates: prefill + sum g dy.  Kernel and oracle each round an
    # fma chain of C2 terms started from the prefill: (C2 + 1) u (|p| + sum |g dy|) each
    rng = np.random.default_rng(100 + degree)
    g = rng.standard_normal((B, C2)).astype(np.float32)
    prefill = rng.standard_normal((B, 3)).astype(np.float32)
    gi = torch.from_numpy(prefill).to(cuda)
    _shencoder.sh_encode_backward(torch.from_numpy(g).to(cuda), di, B, 3, degree,
                                  torch.from_numpy(rdy).to(cuda), gi)
    want = prefill.astype(np.float64) + enc.sh_encode_backward(g, d, degree, rdy)
    mag = np.abs(prefill) + np.abs(g[:, None, :].astype(np.float64) * rdy.reshape(B, 3, C2)).sum(2)
    assert (np.abs(gi.cpu().numpy() - want) <= 2 * (C2 + 1) * gr.U * mag).all()


def test_sh_rejects_bad_shapes(hip_lib, cuda):
    import _shencoder
    z = lambda *shape: torch.zeros(shape, device=cuda)
    for D in (2, 4):
        with pytest.raises(RuntimeError, match="input dim == 3"):
            _shencoder.sh_encode_forward(z(4, D), z(4, 16), 4, D, 4, None)
        with pytest.raises(RuntimeError, match="input dim == 3"):
            _shencoder.sh_encode_backward(z(4, 16), z(4, D), 4, D, 4, z(4, D * 16), z(4, D))
    for C in (0, 9):
        with pytest.raises(RuntimeError, match=r"degree in \[1, 8\]"):
            _shencoder.sh_encode_forward(z(4, 3), z(4, 81), 4, 3, C, None)
        with pytest.raises(RuntimeError, match=r"degree in \[1, 8\]"):
            _shencoder.sh_encode_backward(z(4, 81), z(4, 3), 4, 3, C, z(4, 3 * 81), z(4, 3))


# -------------------------------------------------------------- freq edges --

@pytest.mark.parametrize("B", [1, 1000])
@pytest.mark.parametrize("D,deg", [(1, 1), (2, 10), (4, 3), (3, 0)])
def test_freq_shapes(hip_lib, cuda, D, deg, B):
    import _freqencoder
    C = D + 2 * D * deg
    rng = np.random.default_rng(10 * D + deg)
    x = rng.uniform(-4, 4, (B, D)).astype(np.float32)
    xi = torch.from_numpy(x).to(cuda)
    out = torch.full((B, C), SENTINEL, device=cuda)
    _freqencoder.freq_encode_forward(xi, B, D, deg, C, out)
    y = out.cpu().numpy()
    # identity columns: copies
    assert np.array_equal(y[:, :D].view(np.uint32), x.view(np.uint32))
    # sin / cos columns: inside the reference's __sinf envelope (2^-21.41 +
    # |arg| 2^-22, see test_freq_forward_within_reference_fast_math_envelope)
    # around float64 sin of the fp32 argument
    for k in range(deg):
        for j, phase in enumerate((0.0, np.pi / 2)):
            a = (np.ldexp(x, k).astype(np.float32) + np.float32(phase)).astype(np.float64)
            col = y[:, D + (2 * k + j) * D:D + (2 * k + j + 1) * D].astype(np.float64)
            assert (np.abs(col - np.sin(a)) <= 2.0 ** -21.41 + np.abs(a) * 2.0 ** -22).all(), (k, j)
    # backward: g_x + sum_f 2^f (g_sin o_cos - g_cos o_sin) on the kernel's own
    # fp32 outputs; 2 deg + 1 roundings: (2 deg + 1) 2^-23 sum |term|
    g = rng.standard_normal((B, C)).astype(np.float32)
    gi = torch.full((B, D), SENTINEL, device=cuda)
    _freqencoder.freq_encode_backward(torch.from_numpy(g).to(cuda), out, B, D, deg, C, gi)
    g64, y64 = g.astype(np.float64), y.astype(np.float64)
    want, mag = g64[:, :D].copy(), np.abs(g64[:, :D])
    for f in range(deg):
        s, c = D + 2 * f * D, D + 2 * f * D + D
        t1 = 2.0 ** f * g64[:, s:s + D] * y64[:, c:c + D]
        t2 = 2.0 ** f * g64[:, c:c + D] * y64[:, s:s + D]
        want += t1 - t2
        mag += np.abs(t1) + np.abs(t2)
    assert (np.abs(gi.cpu().numpy() - want) <= (2 * deg + 1) * 2.0 ** -23 * mag).all()


def test_freq_rejects_wrong_output_width(hip_lib, cuda):
    import _freqencoder
    z = lambda *shape: torch.zeros(shape, device=cuda)
    with pytest.raises(RuntimeError, match="C != D"):
        _freqencoder.freq_encode_forward(z(4, 2), 4, 2, 3, 13, z(4, 14))
    with pytest.raises(RuntimeError, match="C != D"):
        _freqencoder.freq_encode_backward(z(4, 14), z(4, 14), 4, 2, 3, 15, z(4, 2))
