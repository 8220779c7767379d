"""The s_grid composite (k_sgrid, k_sgrid_box4) and its gradient scatter
(k_sgrid_backward, fp32-atomic and 64-bit fixed-point forms) against the
float64 reference of tests/sgrid_ref.py, element by element.

One render per case with taps: u2 / w2 are device copies of the workspace
arrays both kernels read, so the reference sees the very samples the kernels
do (N1's dropped samples included) and the comparison is exact up to the fp32
evaluation, whose bounds sgrid_ref derives from the kernels' operation counts.
Every assertion goes through grid_ref.worst_ratio: no element is excluded, and
elements nothing reaches must hold +0.0 / the prefill bit for bit.

Tables (s_grid_log2): 11 -- all 16 levels hashed into 2048 rows, hundreds of
contributions per row; 14 -- levels 0-1 dense, one in a 9264-row table; 16 --
levels 0-3 dense.  Ray sets (sgrid_ref.RAY_SETS): the first N rays of a view
for N around the wave (8 rays) and block (32 rays) sizes of the scatter and
the 64-ray blocks of the composite; 64 rays with duplicates that drive the
scatter's butterfly merge through every lane distance and its non-transitive
patterns; two tiled views (slot order differs from ray order); the opaque
sphere under N1's early exit (dropped samples); cameras far out on the +x, +y
and +z axes, whose heavy samples sit in the last cell of the dense levels
(the position clamp and the `min(cell + 1, res - 1)` corner).

Each case prints `sgrid_ratio ...` lines (pytest -s): how much of the derived
bound the kernel uses; profiles/sgrid_scatter_ratios.txt keeps one run's.
"""
import ctypes

import numpy as np
import pytest
import torch

import grid_ref
import sgrid_ref
from grid_ref import U
from helpers import make_net
from oracle import synth

pytestmark = pytest.mark.gpu

F = sgrid_ref.F
CASES = [(name, N, vw, log2) for log2 in sgrid_ref.S_GRID_LOG2 for name, N, vw in sgrid_ref.RAY_SETS
         if name != "early100" or log2 == 14]
IDS = [f"{name}-L{log2}" for name, _, _, log2 in CASES]
# the checks that need no sweep: a partial wave over a non-power-of-two dense
# table, the merge patterns under the heaviest collisions, a tiled view
FEW = [c for c in CASES if (c[0], c[3]) in (("first37", 14), ("dup64", 11), ("tiles16x12", 16))]
FEW_IDS = [f"{c[0]}-L{c[3]}" for c in FEW]

_nets, _cases = {}, {}


def _net(cuda, log2, surface):
    key = (log2, surface)
    if key not in _nets:
        if surface:          # the opaque sphere of test_gpu_n1.py: its dense density levels need the full tables
            spec = synth.ModelSpec(with_sam=True, s_grid_log2=log2)
            params = synth.make_surface_params(spec, seed=3, amp=1.5)
        else:
            spec = synth.ModelSpec(with_sam=True, grid_log2=12, prop_log2=10, s_grid_log2=log2)
            params = synth.make_params(spec, seed=11, emb_scale=0.5, ln_jitter=0.1)
        _nets[key] = (spec, make_net(spec, params, cuda))
    return _nets[key]


def _rays(cuda, name, N):
    from samnerf_amd import ops
    if name == "tiles16x12":
        W, H, rot = 16, 12, 7
    elif name == "tiles8x4":
        W, H, rot = 8, 4, 8
    elif name == "early100":
        W, H, rot = 10, 10, 6
    else:
        W, H, rot = 16, 16, 3
    if name == "edge37":
        # 40 units out on one axis the contracted coordinate is 2 - 1/40: u =
        # 0.994, the last cell of every level up to res 80 on that axis
        parts = []
        for axis, n in enumerate((13, 12, 12)):
            center = [0.0, 0.0, 0.0]
            center[axis] = -40.0
            pose, intr = synth.gui_camera(4, 4, rot=synth.random_rotation(20 + axis), center=center)
            ro, rd = ops.get_rays(pose, intr, 4, 4, device=cuda)
            parts.append((ro[:n], rd[:n]))
        return (torch.cat([p[0] for p in parts]).contiguous(), torch.cat([p[1] for p in parts]).contiguous())
    pose, intr = synth.gui_camera(W, H, rot=synth.random_rotation(rot))
    ro, rd = ops.get_rays(pose, intr, H, W, device=cuda)
    if name == "dup64":
        src = torch.from_numpy(sgrid_ref.dup64_sources()).to(cuda)
        ro, rd = ro[src], rd[src]
    assert ro.shape[0] >= N
    return ro[:N].contiguous(), rd[:N].contiguous()


class Case:
    """One render with taps, its gradient, and the float64 references (each
    computed once, shared by the tests, never modified)."""

    def __init__(self, cuda, name, N, vw, log2):
        from samnerf_amd.fused import FusedRenderer, ROW
        self.name, self.N, self.vw, self.log2 = name, N, vw, log2
        early = name == "early100"
        self.model_spec, self.net = _net(cuda, log2, early)
        self.spec = self.model_spec.s_grid
        self.ro, self.rd = _rays(cuda, name, N)
        self.fr = FusedRenderer(self.net, t_thresh=1e-3 if early else None)
        self.rows = torch.empty(N, ROW, device=cuda)
        out = self.fr.render(self.ro, self.rd, rows=self.rows, taps=True, keep_workspace=True,
                             own_workspace=True, feats=False, view_width=vw)
        self.ws = out["_workspace"]
        self.u2 = out["u2"].cpu().numpy()
        self.w2 = out["w2"].cpu().numpy()
        self.g = torch.randn(N, ROW, device=cuda, generator=torch.Generator(device=cuda).manual_seed(100 + N))
        self.emb = self.net.s_grid.embeddings.detach()
        self._fwd = self._bwd = None
        # the precondition of the fixed point's overflow margin
        # (sgrid_det_shift: weights summing to <= 1 per ray)
        w64 = self.w2.astype(np.float64)
        assert np.isfinite(self.w2).all() and (self.w2 >= 0).all()
        assert (w64.sum(axis=1) <= 1 + 32 * U).all(), w64.sum(axis=1).max()

    def tag(self):
        return f"set={self.name} N={self.N} L2={self.log2} view_width={self.vw}"

    def forward_ref(self):
        if self._fwd is None:
            self._fwd = sgrid_ref.composite(self.u2, self.w2, self.emb.cpu().numpy(), self.spec)
        return self._fwd

    def scatter_ref(self):
        if self._bwd is None:
            self._bwd = sgrid_ref.scatter(self.u2, self.w2, self.g.cpu().numpy(), self.spec)
        return self._bwd

    def top_cell_samples(self, min_w=0.0, level=None, axis=None):
        """Samples of weight above min_w in the last cell of an axis (any, or
        `axis`) at a level (any, or `level`): where the + 1 corner is clamped
        to res - 1."""
        _, res = sgrid_ref.geometry(self.spec)
        x = self.u2.reshape(-1, 3)[self.w2.reshape(-1) > min_w]
        axes = slice(None) if axis is None else [axis]
        return sum(int((grid_ref.locate(x, r, False)[0][:, axes] == r - 1).any(axis=1).sum())
                   for l, r in enumerate(res) if level is None or l == level)

    def gmax(self, g=None):
        return float((self.g if g is None else g)[:, :F].abs().max())

    def run(self, det, g=None, prefill=None):
        """fr.sgrid_backward into zeros or a copy of `prefill` -> numpy."""
        self.fr.deterministic = det
        ge = torch.zeros_like(self.emb) if prefill is None else prefill.clone()
        self.fr.sgrid_backward(self.g if g is None else g, self.ws, ge)
        torch.cuda.synchronize()
        return ge.cpu().numpy()

    def accumulator_is_zero(self):
        (acc,) = self.fr._accum.values()                 # one stream: one accumulator
        return not bool(acc[:self.emb.numel() * 8].any())


@pytest.fixture(params=CASES, ids=IDS)
def case(request, hip_lib, cuda):
    return _get(cuda, request.param)


@pytest.fixture(params=FEW, ids=FEW_IDS)
def few(request, hip_lib, cuda):
    return _get(cuda, request.param)


def _get(cuda, key):
    if key not in _cases:
        _cases[key] = Case(cuda, *key)
    return _cases[key]


def test_forward_composite(case):
    f_sam, abs_ww, key = case.forward_ref()
    got = case.rows[:, :F].cpu().numpy()
    bound = sgrid_ref.bound_composite(abs_ww, float(case.emb.abs().max()))
    ratio = grid_ref.worst_ratio(np.ascontiguousarray(got), f_sam, bound, key)
    print(f"sgrid_ratio {case.tag()} form=forward ratio={ratio:.4f}")
    assert ratio <= 1.0


def test_forward_forms_bit_identical(case, monkeypatch, diag):
    """k_sgrid<kLookPacked> (what a small render launches), k_sgrid<kLookRef>
    and k_sgrid_box4 on the diagnostic build: the product render's bits at
    every N, small and ragged ones included."""
    from samnerf_amd.fused import ROW
    for mode in ("packed", "ref", "box4"):
        monkeypatch.setenv("SAMNERF_LOOKUP", mode)
        rows = torch.empty(case.N, ROW, device=case.rows.device)
        out = case.fr.render(case.ro, case.rd, rows=rows, taps=1, feats=False, view_width=case.vw)
        if mode == "box4":           # the form ran: only k_sgrid_box4 writes the corner-row taps
            assert bool((out["srows"] != -1).any())
        assert torch.equal(rows, case.rows), (mode, (rows - case.rows).abs().max().item())


def test_scatter_atomic(case):
    val, abs_w, abs_1, count = case.scatter_ref()
    ratio = grid_ref.worst_ratio(case.run(False), val, sgrid_ref.bound_scatter_atomic(abs_w, count, case.gmax()),
                                 abs_1)
    print(f"sgrid_ratio {case.tag()} form=atomic ratio={ratio:.4f} max_count={int(count.max())} "
          f"top_cell_samples={case.top_cell_samples()}")
    assert ratio <= 1.0


def test_scatter_deterministic(case):
    val, abs_w, abs_1, count = case.scatter_ref()
    bound = sgrid_ref.bound_scatter_det(abs_w, count, case.N, case.gmax())
    outs = []
    for _ in range(3):
        outs.append(case.run(True))
        assert case.accumulator_is_zero()
    ratio = grid_ref.worst_ratio(outs[0], val, bound, abs_1)
    print(f"sgrid_ratio {case.tag()} form=deterministic ratio={ratio:.4f} "
          f"shift={sgrid_ref.det_shift(case.N, case.gmax())}")
    assert ratio <= 1.0
    for o in outs[1:]:
        assert np.array_equal(o.view(np.uint32), outs[0].view(np.uint32))


def test_early_exit_case_is_not_vacuous(hip_lib, cuda):
    c = _get(cuda, ("early100", 100, 0, 14))
    dropped = (c.w2 == 0) & (c.u2 == 0.5).all(axis=2)
    assert dropped.any()
    groups = dropped[:96].reshape(12, 8, -1).all(axis=1)      # a scatter wave: 8 rays at one sample
    assert groups.any()
    assert (c.w2 > 0).any(axis=1).all()
    print("early100: dropped samples", int(dropped.sum()), "smallest positive weight", c.w2[c.w2 > 0].min())


def test_edge_case_is_not_vacuous(hip_lib, cuda):
    """Samples that carry weight sit in the last cell of each axis at every
    dense level of the 2^16 table: the position clamp to res - 1 acts there
    (cell = res - 1 only with frac = 0, so the clamped + 1 corner's weight is
    exactly zero: the corner clamp guards the address, the value cannot see
    it -- the reference and count carry those zero contributions)."""
    c = _get(cuda, ("edge37", 37, 0, 16))
    hits = [[c.top_cell_samples(1e-3, level, axis) for axis in range(3)] for level in range(4)]
    print("edge37: samples of weight > 1e-3 in the last cell, per dense level and axis", hits)
    assert min(min(h) for h in hits) > 0


def test_accumulation_into_a_prefill(case):
    """Both forms add to what grad_embeddings holds: untouched elements keep
    the prefill bit for bit (worst_ratio), touched ones are P + val within the
    form's bound plus the roundings against P (sgrid_ref.bound_prefill_*)."""
    val, abs_w, abs_1, count = case.scatter_ref()
    P = torch.randn(case.emb.shape, device=case.emb.device,
                    generator=torch.Generator(device=case.emb.device).manual_seed(9))
    Pn = P.cpu().numpy()
    tot = Pn.astype(np.float64) + val
    b_at = (sgrid_ref.bound_scatter_atomic(abs_w, count, case.gmax())
            + sgrid_ref.bound_prefill_atomic(Pn, count))
    b_det = (sgrid_ref.bound_scatter_det(abs_w, count, case.N, case.gmax())
             + sgrid_ref.bound_prefill_det(tot))
    r_at = grid_ref.worst_ratio(case.run(False, prefill=P), tot, b_at, abs_1, prefill=Pn)
    r_det = grid_ref.worst_ratio(case.run(True, prefill=P), tot, b_det, abs_1, prefill=Pn)
    print(f"sgrid_ratio {case.tag()} form=prefill atomic={r_at:.4f} deterministic={r_det:.4f}")
    assert r_at <= 1.0 and r_det <= 1.0
    assert case.accumulator_is_zero()


def test_only_the_first_128_gradient_columns_count(few):
    """NaN in columns 128..163 of the row gradient (f_image, image, depth: not
    the s_grid's) changes nothing.  The deterministic form must stay on its
    fixed-point path: same bits as with zeros there, repeating, under its
    bound.  The fp32-atomic form's bits depend on the order the atomics land
    in, so two of its runs are only bit-equal where a row receives at most two
    contributions (a + b commutes); everywhere it must stay finite and under
    its bound."""
    val, abs_w, abs_1, count = few.scatter_ref()
    g0, gn = few.g.clone(), few.g.clone()
    g0[:, F:] = 0.0
    gn[:, F:] = float("nan")
    d0, dn, dn2 = few.run(True, g=g0), few.run(True, g=gn), few.run(True, g=gn)
    assert few.accumulator_is_zero()
    assert np.array_equal(d0.view(np.uint32), dn.view(np.uint32))
    assert np.array_equal(dn.view(np.uint32), dn2.view(np.uint32))
    assert grid_ref.worst_ratio(dn, val, sgrid_ref.bound_scatter_det(abs_w, count, few.N, few.gmax()),
                                abs_1) <= 1.0
    a0, an = few.run(False, g=g0), few.run(False, g=gn)
    assert np.isfinite(an).all()
    assert grid_ref.worst_ratio(an, val, sgrid_ref.bound_scatter_atomic(abs_w, count, few.gmax()), abs_1) <= 1.0
    le2 = count <= 2
    assert np.array_equal(a0[le2].view(np.uint32), an[le2].view(np.uint32))


@pytest.mark.parametrize("k", [40, -40])
def test_fixed_point_scale_invariance(few, k):
    """The shift follows the gradient's exponent, so det(g 2^k) holds the same
    integer totals as det(g): the results differ by exactly 2^k."""
    base = few.run(True)
    nz = base != 0
    assert (np.abs(base[nz].astype(np.float64)) * 2.0 ** min(k, 0) >= 2.0 ** -126).all()   # no subnormal result
    scaled = few.run(True, g=few.g * 2.0 ** k)
    assert few.accumulator_is_zero()
    want = (base.astype(np.float64) * 2.0 ** k).astype(np.float32)
    assert np.array_equal(scaled.view(np.uint32), want.view(np.uint32))


def test_zero_gradient_leaves_the_prefill(few):
    P = torch.randn(few.emb.shape, device=few.emb.device,
                    generator=torch.Generator(device=few.emb.device).manual_seed(3))
    for det in (True, False):
        got = few.run(det, g=torch.zeros_like(few.g), prefill=P)
        assert np.array_equal(got.view(np.uint32), P.cpu().numpy().view(np.uint32)), det
    assert few.accumulator_is_zero()


def test_c_abi_refuses_before_any_launch(hip_lib, cuda):
    """N = 0 is a successful no-op, a workspace one byte short is
    SAMNERF_EWORKSPACE and a model without the SAM branch SAMNERF_EINVAL, for
    both entry points; grad_embeddings is untouched by all of them."""
    from samnerf_amd._lib import lib
    from samnerf_amd.fused import FusedRenderer
    OK, EINVAL, EWORKSPACE = 0, -1, -3
    c = _get(cuda, ("first37", 37, 0, 14))
    ws, need, m, _ = c.ws                                # the render's struct, its view_width
    size = lib().samnerf_sgrid_accum_size(ctypes.byref(m))
    acc = torch.zeros(size, dtype=torch.uint8, device=cuda)
    ge = torch.zeros_like(c.emb)
    p = lambda t: ctypes.c_void_p(t.data_ptr())

    def atomic(model, n, ws_bytes):
        return lib().samnerf_sgrid_backward(ctypes.byref(model), p(c.g), n, p(ge), p(ws), ws_bytes, None)

    def det(model, n, ws_bytes):
        return lib().samnerf_sgrid_backward_det(ctypes.byref(model), p(c.g), n, p(ge), p(acc), acc.numel(),
                                                p(ws), ws_bytes, None)

    spec = synth.ModelSpec(with_sam=False, grid_log2=12, prop_log2=10)
    plain = FusedRenderer(make_net(spec, synth.make_params(spec, seed=1, emb_scale=0.5), cuda)).model()
    for call in (atomic, det):
        assert call(m, 0, need) == OK
        assert call(m, c.N, need - 1) == EWORKSPACE
        assert b"workspace too small" in lib().samnerf_last_error()
        assert call(plain, c.N, need) == EINVAL
        assert b"no s_grid" in lib().samnerf_last_error()
    torch.cuda.synchronize()
    assert not bool(ge.any()) and not bool(acc.any())
