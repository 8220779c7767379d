"""The mask-head training kernels (csrc/mask_head_train.hip) away from the
comfortable corner of tests/test_gpu_mask_train.py (ray counts that are
multiples of 32, a 2^12 m_grid, fresh zeroed buffers):

  1. pad rows: the saved activations are [units][Rp], Rp = 32 N rounded up to
     1,024 rows; k_mt_fwd / k_mt_fwd16 / k_mt_bwd must write zeros for rows
     R .. Rp, which k_mt_dw loads unconditionally;
  2. workgroups (16 sample-major rows) that straddle a sample index (N % 16
     != 0), in the gather, the run-merging scatter (mt_scatter) and the
     adaptive kernels' 16-ray workgroups / 32-ray LDS tiles;
  3. m_grid tables with several dense levels, with dense levels that scatter
     directly (not through the per-XCD copies) and a k_mt_rep_sum length other
     than 4 x 4096 x 8;
  5. the distance to a float64 twin of the step (oracle_backend.float64_twin);
  6. the C ABI's contract: grad_mask_w overwritten, grad_m_grid accumulated
     into, nothing read from the workspace before it is written;
  7. ray tiles (samnerf_model.view_width) in k_mt_logits / k_mt_bwd.
(4, the last layer's partly filled second output tile, is K = 17 in
test_gpu_mask_train.py.)  Every comparison evaluates the twin at the HIP
path's own bins, as there.

float64 twin, measured on the MI355X (test_fused_mask_step_vs_float64_twin's
RATIO lines: relative error of a gradient against the float64 twin, HIP /
fp32 CPU twin, N = 100, K = 5; the bound is err_hip <= max(M err_cpu, 1e-5)):
                        head_mode 0 (f16x3)          head_mode 1 (fp32)
  m_grid.embeddings     6.366e-07 / 5.732e-07 = 1.111   6.371e-07 -> 1.112
  mask_mlp.0.net.0      6.560e-07 / 6.072e-07 = 1.080   6.576e-07 -> 1.083
  mask_mlp.0.net.1      4.152e-07 / 4.427e-07 = 0.938   4.282e-07 -> 0.967
  mask_mlp.0.net.2      3.322e-07 / 6.483e-07 = 0.512   3.380e-07 -> 0.521
  adaptive density, six weights: 0.764 .. 1.133; loss within 9e-8 of the
  float64 loss in every case.
The f16x3 forward is no farther from the float64 twin than the exact one (no
ratio near the 4 that would be a finding): M = 2 x 1.111 for head_mode 0,
M = 2 for the exact-fp32 paths (test_gpu_rgb_train.py's convention).

What the pad-row tests can and cannot see (mutants of the kernels, run by
hand): a forward launched over the live rows' workgroups alone (pad rows
never written) passes every test whose workspace comes from torch.empty and
fails test_c_abi_backward_contract_with_poisoned_workspace (NaN in dW); the
`r < R ? .. : 0` selects on the forward's stores are not what keeps the pad
rows zero -- a dead row's gathered input is zero, the layers have no bias and
scale_exp_of_max(0) is 2^125, finite, so the layers give exact zeros with or
without them.  A k_mt_rep_sum length fixed at 4 x 4,096 x 8 and swapped dense
strides in corner_row_of fail test_fused_mask_step_reference_size_m_grid
(m_grid gradient off by 0.47 and 0.71 relative at 2^15).
"""
import ctypes

import pytest
import torch

from mask_train_fixtures import (assert_not_vacuous, float64_twin_errors, level_slices, ragged_batch,
                                 twin_step)
from oracle import synth
from test_gpu_mask_train import GRAD_TOL, _adaptive_nets, _grad_errors, _mask_nets

pytestmark = pytest.mark.gpu

DEFAULT_KEYS = {"m_grid.embeddings", "mask_mlp.0.net.0.weight", "mask_mlp.0.net.1.weight",
                "mask_mlp.0.net.2.weight"}

# head_mode 0 (k_mt_fwd16) against the float64 twin: err_hip / err_cpu_fp32 per
# tensor as printed by test_fused_mask_step_vs_float64_twin on the MI355X, and
# M = twice the worst of them (tests/test_gpu_eval.py's margin for such a bound)
F64_RATIOS = {"m_grid.embeddings": 1.111, "mask_mlp.0.net.0.weight": 1.080, "mask_mlp.0.net.1.weight": 0.938,
              "mask_mlp.0.net.2.weight": 0.512}
F64_M_F16X3 = 2.0 * max(F64_RATIOS.values())


def _bins(net, ro, rd, cnf=None):
    from samnerf_amd.fused import FusedRenderer
    out = FusedRenderer(net).render(ro, rd, cam_near_far=cnf, taps=True)
    return [out["bins1"].contiguous().cpu(), out["bins2"].contiguous().cpu()]


def _hip_step(gpu, cuda, ro, rd, gt, cnf):
    from samnerf_amd.train import mask_train_step
    gpu.zero_grad(set_to_none=True)
    _, loss = mask_train_step(gpu, ro.to(cuda), rd.to(cuda), gt.to(cuda), cam_near_far=cnf.to(cuda))
    loss.backward()
    return float(loss.detach())


def _check_against_twin(gpu, cpu, loss, loss_c, keys, tag):
    loss_c = float(loss_c.detach())
    assert abs(loss - loss_c) <= 1e-5 * abs(loss_c) + 1e-7, (loss, loss_c)
    errs = _grad_errors(gpu, cpu)
    print(tag, "relative gradient errors:", {k: f"{v:.1e}" for k, v in errs.items()})
    assert set(errs) == keys, errs
    bad = {k: v for k, v in errs.items() if v > GRAD_TOL}
    assert not bad, bad


@pytest.mark.parametrize("n_rays,head_mode", [(1, 1), (33, 1), (37, 1), (37, 0), (100, 1), (100, 0)])
def test_fused_mask_step_ragged_batches(hip_lib, cuda, n_rays, head_mode):
    """Paths 1 and 2, 'default' head, K = 5, per-ray cam_near_far: N = 1 (2 live
    workgroups, 62 of pad rows alone), 33 (Rp = 2,048: the second k_mt_dw chunk
    holds 32 live rows), 37 and 100 (workgroups straddle sample indices; one
    or more full chunks and a part one), k_mt_fwd (head_mode 1) and k_mt_fwd16
    (0): loss and the four gradients against the fp32 CPU twin.  The twin's
    gradients are non-zero and no label's probability is clamped."""
    gpu, cpu = _mask_nets(cuda, 5, head_mode=head_mode)
    ro, rd, gt, cnf = ragged_batch(n_rays, 5)
    bins = _bins(gpu, ro.to(cuda), rd.to(cuda), cnf.to(cuda))
    loss = _hip_step(gpu, cuda, ro, rd, gt, cnf)
    loss_c, probs = twin_step(cpu, ro, rd, gt, cnf, bins)
    assert_not_vacuous(cpu, probs)
    _check_against_twin(gpu, cpu, loss, loss_c, DEFAULT_KEYS, f"N={n_rays} head_mode={head_mode}")


@pytest.mark.parametrize("adaptive_type,n_inst", [("density", 5), ("rgb", 3)])
@pytest.mark.parametrize("n_rays", [1, 37, 100])
def test_fused_adaptive_mask_step_ragged_batches(hip_lib, cuda, adaptive_type, n_inst, n_rays):
    """Path 2, adaptive heads: k_adt_fwd / k_adt_bwd with a part-filled 16-ray
    workgroup and k_adt_dw with a part-filled 32-ray LDS tile (N = 1, 37, 100),
    per-ray cam_near_far: test_fused_adaptive_mask_step_matches_cpu_twin's
    assertions; at N = 37 two identical steps also give the same bits
    (k_adt_dw sums in a fixed order)."""
    gpu, cpu = _adaptive_nets(cuda, adaptive_type, n_inst)
    ro, rd, gt, cnf = ragged_batch(n_rays, n_inst, rot=6)
    bins = _bins(gpu, ro.to(cuda), rd.to(cuda), cnf.to(cuda))
    loss = _hip_step(gpu, cuda, ro, rd, gt, cnf)
    loss_c, probs = twin_step(cpu, ro, rd, gt, cnf, bins)
    assert_not_vacuous(cpu, probs)
    n_layers = 6 if adaptive_type == "density" else 8
    _check_against_twin(gpu, cpu, loss, loss_c, {f"mask_mlp.{i}.weight" for i in range(n_layers)},
                        f"{adaptive_type} N={n_rays}")
    if n_rays == 37:
        first = {k: p.grad.clone() for k, p in gpu.named_parameters() if p.grad is not None}
        assert _hip_step(gpu, cuda, ro, rd, gt, cnf) == loss
        for k, p in gpu.named_parameters():
            if p.grad is not None:
                assert torch.equal(first[k], p.grad), k


@pytest.mark.parametrize("m_grid_log2,n_rays,head_mode", [(15, 100, 1), (15, 100, 0), (19, 256, 1)])
def test_fused_mask_step_reference_size_m_grid(hip_lib, cuda, m_grid_log2, n_rays, head_mode):
    """Path 3: the training gather (lookup_level3<8>) and scatter
    (corner_row_of<8>, k_mt_rep_sum) on m_grid tables larger than the other
    tests' 2^12 (there level 0 alone is dense, 16^3 rows, and all four
    replicated levels are 4,096 rows): 2^15, and the product's default 2^19
    (nerf/network.py:114), against the fp32 CPU twin -- the step's tolerances
    and, so that a wrong row on one coarse level cannot hide in the norm of
    the whole table, the m_grid gradient level by level.

    The test reads the model's own offsets and asserts what it relies on.  They
    are not those a (res + 1)^3 lattice would give: this encoder indexes a
    dense level with strides 1, res, res^2 (gridencoder.cu:62-78) and sizes it
    min(2^log2, res^3) rounded up to 8 rows (grid.py:124-135), so a level is
    dense where res^3 <= its rows and the offsets are 0, 4096, 13360, 30936,
    63704, ...: offsets[4] <= 65536 at every table size, and the backward
    replicates levels 0-3 (rep_levels = 4) always -- a split at three levels
    cannot be reached with the product's m_grid (L16, base 16, 512).  What
    these sizes do reach: at 2^15 dense levels 0-3 with resolutions that are
    no power of two (21, 26), hashed levels 4-15, and copies of 63,704 rows
    folded by k_mt_rep_sum; at 2^19 also dense levels (4-6) that scatter
    straight into the gradient."""
    gpu, cpu = _mask_nets(cuda, 5, head_mode=head_mode, m_grid_log2=m_grid_log2)
    levels = level_slices(cpu.m_grid)
    offs = [a for _, a, _, _, _ in levels]
    dense = [lvl for lvl, _, _, _, d in levels if d]
    hashed = [lvl for lvl, _, _, _, d in levels if not d]
    assert len(dense) >= 4 and any(levels[lvl][3] & (levels[lvl][3] - 1) for lvl in dense), dense
    assert hashed and all((levels[lvl][2] - levels[lvl][1]) == 2 ** m_grid_log2 for lvl in hashed), hashed
    rep_levels = 0                           # mask_train_backward's split (kRepRows = 65536)
    while rep_levels < 4 and offs[rep_levels + 1] <= 65536:
        rep_levels += 1
    assert rep_levels == 4 and offs[4] == 63704 != 4 * 4096, offs[:5]
    if m_grid_log2 == 19:
        assert [lvl for lvl in dense if lvl >= rep_levels] == [4, 5, 6], dense
    ro, rd, gt, cnf = ragged_batch(n_rays, 5)
    bins = _bins(gpu, ro.to(cuda), rd.to(cuda), cnf.to(cuda))
    loss = _hip_step(gpu, cuda, ro, rd, gt, cnf)
    loss_c, probs = twin_step(cpu, ro, rd, gt, cnf, bins)
    assert_not_vacuous(cpu, probs)
    a, b = gpu.m_grid.embeddings.grad.cpu(), cpu.m_grid.embeddings.grad
    empty, per_level = [], {}
    for lvl, r0, r1, _, _ in levels:
        ref = float(b[r0:r1].norm())
        if ref == 0.0:
            empty.append(lvl)
            continue
        per_level[lvl] = float((a[r0:r1] - b[r0:r1]).norm()) / ref
    print("m_grid gradient, relative error per level:", {k: f"{v:.1e}" for k, v in per_level.items()})
    assert len(empty) <= 2, empty
    bad = {k: v for k, v in per_level.items() if v > GRAD_TOL}
    assert not bad, bad
    _check_against_twin(gpu, cpu, loss, loss_c, DEFAULT_KEYS, f"m_grid 2^{m_grid_log2} head_mode={head_mode}")


@pytest.mark.parametrize("head,head_mode", [("default", 1), ("default", 0), ("density", 1)])
def test_fused_mask_step_vs_float64_twin(hip_lib, cuda, head, head_mode):
    """Path 5: each gradient of the HIP mask step is as close to a float64 twin
    of the step as the fp32 CPU twin is -- within M x, or 1e-5 relative -- and
    the loss within 2e-6, at N = 100 rays, K = 5, the HIP path's bins: the
    'default' head on k_mt_fwd (head_mode 1, M = 2) and on the f16x3
    k_mt_fwd16 (head_mode 0, M = F64_M_F16X3 from the measured ratios), and
    the adaptive density head (k_adt_*, M = 2)."""
    gpu, cpu = (_mask_nets(cuda, 5, head_mode=head_mode) if head == "default"
                else _adaptive_nets(cuda, "density", 5))
    ro, rd, gt, cnf = ragged_batch(100, 5)
    bins = _bins(gpu, ro.to(cuda), rd.to(cuda), cnf.to(cuda))
    loss = _hip_step(gpu, cuda, ro, rd, gt, cnf)
    errs, loss64, _ = float64_twin_errors({"hip": gpu}, cpu, ro, rd, gt, cnf, bins)
    assert errs["hip"] and set(errs["hip"]) == set(errs["cpu_fp32"])
    for k in errs["hip"]:
        print(f"RATIO {head} head_mode={head_mode} {k} {errs['hip'][k]:.3e} / {errs['cpu_fp32'][k]:.3e} = "
              f"{errs['hip'][k] / errs['cpu_fp32'][k]:.3f}")
    print(f"loss {loss!r} float64 {loss64!r} relative {abs(loss - loss64) / abs(loss64):.2e}")
    assert abs(loss - loss64) <= 2e-6 * abs(loss64)
    M = F64_M_F16X3 if (head == "default" and head_mode == 0) else 2.0
    bad = {k: (v, errs["cpu_fp32"][k]) for k, v in errs["hip"].items()
           if v > max(M * errs["cpu_fp32"][k], 1e-5)}
    assert not bad, bad


# ------------------------------------------------------------ the C ABI itself
def _c_abi_step(fr, ro, rd, g_logits, fill, pattern=None, view_width=0):
    """_FusedMaskTrain.forward / backward through the C ABI with the caller's
    buffers: the training workspace filled with `fill` bytes, logits and the
    weight gradients prefilled with NaN, grad_m_grid with `pattern`.  Returns
    (logits, weight gradients, grad_m_grid or None)."""
    from samnerf_amd.fused import _ptr, _stream, check, lib
    N, dev = ro.shape[0], ro.device
    out = fr.render(ro, rd, keep_workspace=True, feats=False, own_workspace=True, mask=True,
                    mask_logits=False, view_width=view_width)
    ws, need, m, vw = out.pop("_workspace")
    assert vw == view_width and (int(m.with_mask), int(m.view_width)) == (2, vw)   # the render's struct
    tneed = lib().samnerf_mask_train_workspace_size_model(ctypes.byref(m), N)
    tws = torch.full((tneed,), fill, dtype=torch.uint8, device=dev)
    logits = torch.full((N, int(m.mask_out)), float("nan"), device=dev)
    check(lib().samnerf_mask_train_forward(ctypes.byref(m), N, _ptr(logits), _ptr(ws), need, _ptr(tws), tneed,
                                           _stream(ro)), "mask_train_forward")
    net = fr.net
    if int(m.mask_kind) == 0:
        weights = [net.mask_mlp[0].net[i].weight for i in range(3)]
        g_emb = pattern.clone()
    else:
        weights = [layer.weight for layer in net.mask_mlp]
        g_emb = None
    gw = [torch.full(tuple(w.shape), float("nan"), device=dev) for w in weights]
    arr = (ctypes.c_void_p * 8)(*[t.data_ptr() for t in gw])
    check(lib().samnerf_mask_train_backward(ctypes.byref(m), N, _ptr(g_logits), arr, _ptr(g_emb), _ptr(ws), need,
                                            _ptr(tws), tneed, _stream(ro)), "mask_train_backward")
    torch.cuda.synchronize(dev)
    return logits, gw, g_emb


def _autograd_route(fr, ro, rd, g_logits):
    """The same gradients through render_mask_train + backward: (logits,
    weight gradients, m_grid gradient or None)."""
    from samnerf_amd.fused import render_mask_train
    net = fr.net
    net.zero_grad(set_to_none=True)
    with torch.enable_grad():
        logits = render_mask_train(fr, ro, rd)["instance_mask_logits"]
    logits.backward(g_logits)
    grads = {k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None}
    g_emb = grads.pop("m_grid.embeddings", None)
    return logits.detach(), list(grads.values()), g_emb


def _rel(a, b):
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _pattern(net, cuda):
    """A known non-zero content of grad_m_grid: (1 .. 5) x 2^-18 per element,
    small against the gradient's elements so that (pattern + g) - pattern
    keeps g to 1e-7."""
    n = net.m_grid.embeddings.numel()
    return ((torch.arange(n, device=cuda) % 5 + 1).float() * 2.0 ** -18).view_as(net.m_grid.embeddings)


@pytest.mark.parametrize("head,head_mode", [("default", 1), ("default", 0), ("density", 1)])
def test_c_abi_backward_contract_with_poisoned_workspace(hip_lib, cuda, head, head_mode):
    """Paths 1 and 6 at N = 37 (R = 1,184 live rows of Rp = 2,048): the training
    workspace starts as 0xFF bytes (every float a NaN), so a pad row that
    k_mt_fwd / k_mt_fwd16 / k_mt_bwd left unwritten reaches k_mt_dw as NaN;
    grad_mask_w starts as NaN (include/samnerf_hip.h: overwritten) and
    grad_m_grid as a known pattern (accumulated into).  Logits and weight
    gradients are finite and equal those of a zero-filled workspace (logits
    bit for bit; weight gradients to 1e-6, float atomics -- bit for bit on the
    adaptive head's fixed-order sums) and the autograd route's; grad_m_grid
    minus the pattern is the autograd route's m_grid gradient, and rows that
    gradient leaves at zero keep the pattern's bits."""
    from samnerf_amd.fused import FusedRenderer
    gpu, _ = (_mask_nets(cuda, 5, head_mode=head_mode) if head == "default"
              else _adaptive_nets(cuda, "density", 5))
    ro, rd, _, _ = ragged_batch(37, 5)
    ro, rd = ro.to(cuda), rd.to(cuda)
    g = torch.randn(37, 5, generator=torch.Generator().manual_seed(8)).to(cuda)
    fr = FusedRenderer(gpu)
    pattern = _pattern(gpu, cuda) if head == "default" else None
    lg_p, gw_p, ge_p = _c_abi_step(fr, ro, rd, g, 0xFF, pattern)
    lg_z, gw_z, ge_z = _c_abi_step(fr, ro, rd, g, 0x00, pattern)
    lg_a, gw_a, ge_a = _autograd_route(fr, ro, rd, g)
    assert torch.isfinite(lg_p).all() and all(torch.isfinite(t).all() for t in gw_p)
    assert torch.equal(lg_p, lg_z) and torch.equal(lg_p, lg_a)
    assert len(gw_p) == len(gw_a) == (3 if head == "default" else 6)
    for i, (p, z, a) in enumerate(zip(gw_p, gw_z, gw_a)):
        assert float(a.norm()) > 0, i
        if head == "default":
            assert _rel(p, z) <= 1e-6, (i, _rel(p, z))
        else:
            assert torch.equal(p, z), i
        assert _rel(p, a) <= 1e-6, (i, _rel(p, a))
    if head == "default":
        assert float(ge_a.norm()) > 0 and torch.isfinite(ge_p).all()
        assert _rel(ge_p - pattern, ge_a) <= 1e-5, _rel(ge_p - pattern, ge_a)
        assert _rel(ge_z - pattern, ge_a) <= 1e-5
        untouched = (ge_a == 0).all(-1)
        assert bool(untouched.any()) and torch.equal(ge_p[untouched], pattern[untouched])


@pytest.mark.parametrize("head_mode", [1, 0])
def test_c_abi_mask_training_with_ray_tiles(hip_lib, cuda, head_mode):
    """Path 7: a 16 x 8 view rendered with view_width = 16 (four 8 x 4 ray
    tiles: the workspace's samples are in slot order) and the two training
    calls with that view_width -- k_mt_logits writes and k_mt_bwd reads ray
    tiles(slot): logits bit for bit those of view_width = 0 in ray order,
    gradients within 1e-5 (test_gpu_train.py::test_distillation_step_with_ray_tiles's
    bound)."""
    from oracle import renderer as orc
    from samnerf_amd.fused import FusedRenderer, ray_of_slots
    gpu, _ = _mask_nets(cuda, 5, head_mode=head_mode)
    pose, intr = synth.gui_camera(16, 8, rot=synth.random_rotation(3))
    ro, rd = orc.get_rays(pose, intr, 8, 16)
    ro, rd = ro.to(cuda).contiguous(), rd.to(cuda).contiguous()
    assert not torch.equal(ray_of_slots(128, 16), torch.arange(128))
    g = torch.randn(128, 5, generator=torch.Generator().manual_seed(9)).to(cuda)
    fr = FusedRenderer(gpu)
    pattern = torch.zeros_like(gpu.m_grid.embeddings)
    lg_t, gw_t, ge_t = _c_abi_step(fr, ro, rd, g, 0xFF, pattern, view_width=16)
    lg_0, gw_0, ge_0 = _c_abi_step(fr, ro, rd, g, 0xFF, pattern, view_width=0)
    assert torch.isfinite(lg_t).all() and torch.equal(lg_t, lg_0)
    for i, (t, z) in enumerate(zip(gw_t + [ge_t], gw_0 + [ge_0])):
        assert float(z.norm()) > 0 and _rel(t, z) <= 1e-5, (i, _rel(t, z))
