"""perturb=True drawn inside the kernels (samnerf_model.perturb_device,
fused.PhiloxPerturb) on the GPU.

The fill kernel (samnerf_perturb_fill) against the numpy restatement of the
contract (tests/philox_ref.py) bit for bit; then everything else stands on it:
a seeded render equals the render fed the filled arrays bit for bit -- plain,
ray-tiled (slot != ray), with a mask head, through NeRFRenderer's
perturb_rng = "philox", in the RGB training forward and backward, and in the
diagnostic library's one-kernel proposal form.
"""
import numpy as np
import pytest
import torch

import philox_ref
from helpers import make_net
from oracle import synth
from test_gpu_rgb_train import GRAD_TOL

pytestmark = pytest.mark.gpu

STEPS = (128, 64, 32)
SEED = 0xF00DFACE87654321            # high bits set
OUTS = ("image", "depth", "weights_sum", "samvit")
TAPS = ("bins1", "inds1", "bins2", "inds2", "w0", "w1")


def _sam_net(cuda, seed=22):
    spec = synth.ModelSpec(with_sam=True, grid_log2=14, s_grid_log2=14, prop_log2=12)
    return make_net(spec, synth.make_params(spec, seed=seed, emb_scale=0.5, ln_jitter=0.1), cuda)


def _view(W, H, cuda, rot=4):
    from samnerf_amd import ops
    pose, intr = synth.gui_camera(W, H, rot=synth.random_rotation(rot))
    return ops.get_rays(pose, intr, H, W, device=cuda)


def _same(a, b, keys, what):
    for k in keys:
        assert torch.equal(a[k], b[k]), (what, k, (a[k].float() - b[k].float()).abs().max().item())


@pytest.mark.parametrize("offset", [0, 2 ** 32 + 5])
def test_fill_kernel_equals_the_contract(hip_lib, cuda, offset):
    """N = 67: a ragged last wave, a ray count that is no multiple of 4."""
    from samnerf_amd.fused import perturb_fill
    N = 67
    want = philox_ref.all_positions(SEED, offset, STEPS, N)
    got = perturb_fill(SEED, offset, N, STEPS, cuda)
    for s in range(3):
        g = got[s].cpu().numpy()
        assert g.shape == want[s].shape and g.dtype == np.float32
        assert np.array_equal(g.view(np.uint32), want[s].view(np.uint32)), s
    # one output pointer NULL: the others are written as before, nothing else is
    for skip in range(3):
        part = perturb_fill(SEED, offset, N, STEPS, cuda, want=tuple(i != skip for i in range(3)))
        assert part[skip] is None
        for s in range(3):
            if s != skip:
                assert torch.equal(part[s], got[s])


@pytest.mark.parametrize("head_mode", [0, 1])
@pytest.mark.parametrize("shape", ["n67", "tiled_64x8"])
def test_seeded_render_equals_array_render(hip_lib, cuda, shape, head_mode):
    """PhiloxPerturb(seed, offset) against the arrays of perturb_fill(seed,
    offset): every output and the proposal stages' taps, bit for bit.  The 64 x
    8 view with view_width = 64 runs 8 x 4 pixel tiles (slot != ray): the
    kernels must draw by ray id."""
    from samnerf_amd.fused import FusedRenderer, PhiloxPerturb, perturb_fill
    net = _sam_net(cuda)
    ro, rd = _view(64, 8, cuda)
    vw = 64
    if shape == "n67":
        ro, rd, vw = ro[:67].contiguous(), rd[:67].contiguous(), 0
    N, offset = ro.shape[0], 3
    fr = FusedRenderer(net, head_mode=head_mode)
    arrays = perturb_fill(SEED, offset, N, STEPS, cuda)
    for taps in (False, True):
        seeded = fr.render(ro, rd, perturb=PhiloxPerturb(SEED, offset), view_width=vw, taps=taps)
        filled = fr.render(ro, rd, perturb=arrays, view_width=vw, taps=taps)
        _same(seeded, filled, OUTS + (TAPS if taps else ()), (shape, head_mode, taps))
    if vw:
        # and independent of the tiling, as every other output is
        flat = fr.render(ro, rd, perturb=PhiloxPerturb(SEED, offset), view_width=0)
        _same(seeded, flat, OUTS, "tiled vs untiled")


def test_seeded_render_with_mask_head(hip_lib, cuda):
    from samnerf_amd.fused import FusedRenderer, PhiloxPerturb, perturb_fill
    spec = synth.ModelSpec(with_sam=False, with_mask=True, mask_type="default", n_inst=3, redundant_instance=2,
                           grid_log2=14, prop_log2=12, m_grid_log2=14)
    net = make_net(spec, synth.make_params(spec, seed=12, emb_scale=0.5), cuda)
    ro, rd = _view(64, 8, cuda, rot=8)
    fr = FusedRenderer(net)
    seeded = fr.render(ro, rd, mask=True, perturb=PhiloxPerturb(SEED, 9), view_width=64)
    filled = fr.render(ro, rd, mask=True, perturb=perturb_fill(SEED, 9, ro.shape[0], STEPS, cuda), view_width=64)
    _same(seeded, filled, ("image", "depth", "weights_sum", "instance_mask_logits"), "mask")
    assert seeded["instance_mask_logits"].shape == (512, 5)


def test_seeded_render_repeats_and_acts(hip_lib, cuda):
    from samnerf_amd.fused import FusedRenderer, PhiloxPerturb
    net = _sam_net(cuda)
    ro, rd = _view(64, 8, cuda)
    fr = FusedRenderer(net)
    a = fr.render(ro, rd, perturb=PhiloxPerturb(SEED, 1))
    b = fr.render(ro, rd, perturb=PhiloxPerturb(SEED, 1))
    _same(a, b, OUTS, "repeat")
    other = fr.render(ro, rd, perturb=PhiloxPerturb(SEED, 2))
    assert not torch.equal(a["image"], other["image"])
    seed2 = fr.render(ro, rd, perturb=PhiloxPerturb(SEED ^ 1 << 63, 1))
    assert not torch.equal(a["image"], seed2["image"])
    plain = fr.render(ro, rd)
    assert (plain["image"] - a["image"]).abs().max().item() > 1e-4        # the draw did act
    # a seeded call leaves nothing behind in the shared model struct
    again = fr.render(ro, rd)
    _same(plain, again, OUTS, "unperturbed after seeded")


def test_seeded_render_rejects_arrays_with_seed(hip_lib, cuda):
    """The C check end to end: perturb_device with arrays set is an error."""
    import ctypes
    from samnerf_amd import _lib
    from samnerf_amd.fused import FusedRenderer, perturb_fill
    from samnerf_amd.ops import _ptr, _stream
    net = _sam_net(cuda)
    ro, rd = _view(8, 8, cuda)
    fr = FusedRenderer(net)
    fr.render(ro, rd)                                   # sizes the workspace
    arrays = perturb_fill(SEED, 0, 64, STEPS, cuda)
    m = fr.call_model(perturb=arrays)                   # this call's own struct
    m.perturb_device = 1
    ws, need = fr.workspace(m, 64, ro.device)
    out = [torch.empty(64, 3, device=cuda), torch.empty(64, device=cuda), torch.empty(64, device=cuda)]
    rc = _lib.lib().samnerf_render_forward(ctypes.byref(m), _ptr(ro), _ptr(rd), 64, None, 0, 1.0, _ptr(out[0]),
                                           _ptr(out[1]), _ptr(out[2]), None, None, _ptr(ws), need, _stream(ro))
    assert rc == -1 and "perturb_device" in _lib.last_error()


def test_renderer_philox_rng_draws_per_dispatched_call(hip_lib, cuda):
    """perturb_rng = "philox": a staged render of 4,096 rays in chunks of 1,024
    equals the four chunks rendered with offsets k .. k + 3."""
    from samnerf_amd.fused import FusedRenderer, PhiloxPerturb
    net = _sam_net(cuda)
    assert net.perturb_rng == "torch"
    ro, rd = _view(64, 64, cuda)
    net.opt.max_ray_batch = 1024
    net.perturb_rng, net.perturb_seed = "philox", SEED
    with torch.no_grad():
        net.render(ro[:64], rd[:64], perturb=True)                # the counter is per renderer, not per view
        k = net._perturb_calls
        assert k == 1
        got = net.render(ro, rd, staged=True, perturb=True, return_feats=1)
        assert net._perturb_calls == k + 4
        fr = FusedRenderer(net)
        for i, h in enumerate(range(0, 4096, 1024)):
            part = fr.render(ro[h:h + 1024], rd[h:h + 1024], perturb=PhiloxPerturb(SEED, k + i))
            for key in OUTS:
                assert torch.equal(got[key][h:h + 1024].reshape(part[key].shape), part[key]), (i, key)
        again = net.render(ro, rd, staged=True, perturb=True, return_feats=1)     # offsets k + 4 ..
        assert not torch.equal(again["image"], got["image"])
        # perturb=False dispatches draw nothing, whatever the mode
        plain = net.render(ro, rd, staged=True, return_feats=1)
        net.perturb_rng = "torch"
        ref = net.render(ro, rd, staged=True, return_feats=1)
    _same(plain, ref, OUTS, "unperturbed")


def _rgb_net(cuda):
    spec = synth.ModelSpec(with_sam=False, grid_log2=12, s_grid_log2=10, prop_log2=10)
    return make_net(spec, synth.make_params(spec, seed=12, emb_scale=0.5), cuda).train()


def _train_render(net, ro, rd, perturb):
    """One training render and the backward of a loss that reaches every
    output; returns the detached outputs and the gradients by name."""
    from samnerf_amd.fused import FusedRenderer, render_rgb_train
    net.zero_grad(set_to_none=True)
    out = render_rgb_train(FusedRenderer(net, head_mode=1), ro, rd, perturb=perturb)
    g = torch.Generator().manual_seed(3)
    wi = torch.rand(ro.shape[0], 3, generator=g).to(ro.device)
    ww = torch.rand(ro.shape[0], 32, generator=g).to(ro.device)
    loss = (out["image"] * wi).mean() + 0.1 * out["depth"].mean() + 0.2 * out["weights_sum"].mean() \
        + (out["weights"] * ww).mean() + out["proposal_loss"] + 0.02 * out["distort_loss"]
    loss.backward()
    grads = {k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None}
    return {k: v.detach().clone() for k, v in out.items() if torch.is_tensor(v)}, grads


def test_rgb_training_seeded_equals_arrays(hip_lib, cuda):
    """256 rays: the forward's outputs and both losses bit for bit; the backward
    recomputes the forward's bins from (seed, offset), so every gradient agrees
    within tests/test_gpu_rgb_train.py's per-tensor tolerance (the scatter's
    unordered fp32 atomics do not repeat to the bit)."""
    from samnerf_amd.fused import PhiloxPerturb, perturb_fill
    net = _rgb_net(cuda)
    ro, rd = _view(16, 16, cuda, rot=3)
    out_s, g_s = _train_render(net, ro, rd, PhiloxPerturb(SEED, 11))
    out_a, g_a = _train_render(net, ro, rd, perturb_fill(SEED, 11, 256, STEPS, cuda))
    _same(out_s, out_a, ("image", "depth", "weights_sum", "weights", "proposal_loss", "distort_loss"), "rgb train")
    assert set(g_s) == set(g_a) and any("prop_encoders" in k for k in g_s) and any("prop_mlp" in k for k in g_s)
    worst = {k: float((g_s[k] - g_a[k]).norm() / g_a[k].norm().clamp_min(1e-12)) for k in g_a}
    print("seeded vs arrays, relative gradient differences:", {k: f"{v:.1e}" for k, v in worst.items()})
    bad = {k: v for k, v in worst.items() if v > GRAD_TOL}
    assert not bad, bad
    # the draw reaches the training render: another offset, another image
    out_o, _ = _train_render(net, ro, rd, PhiloxPerturb(SEED, 12))
    assert not torch.equal(out_o["image"], out_s["image"])


def test_rgb_train_step_seeded_equals_arrays(hip_lib, cuda):
    """samnerf_rgb_train_step (one C call): image and the five loss terms."""
    from samnerf_amd.fused import PhiloxPerturb, perturb_fill
    from samnerf_amd.train import rgb_train_step_fused
    net = _rgb_net(cuda)
    ro, rd = _view(16, 16, cuda, rot=3)
    gt = torch.rand(256, 3, generator=torch.Generator().manual_seed(5)).to(cuda)
    res = []
    for pert in (PhiloxPerturb(SEED, 4), perturb_fill(SEED, 4, 256, STEPS, cuda)):
        net.zero_grad(set_to_none=True)
        img, loss, out = rgb_train_step_fused(net, ro, rd, gt, global_step=1, perturb=pert)
        res.append((img.clone(), loss.clone(), {k: out[k].clone() for k in ("mse", "proposal_loss", "distort_loss")},
                    {k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None}))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    for k in res[0][2]:
        assert torch.equal(res[0][2][k], res[1][2][k]), k
    for k, g in res[1][3].items():
        assert float((res[0][3][k] - g).norm() / g.norm().clamp_min(1e-12)) <= GRAD_TOL, k
