"""The distillation loss on the MI355X (csrc/feat_loss.hip): resized, loss and
grad_pred against the float64 CPU twin of the reference's op sequence
(nerf/utils.py:1101-1106), exact zeros for untouched source cells, bit
repeatability, graph capture, and the fused distillation step end to end.

Tolerance of every comparison with the twin: the larger of the fp32 CPU
reference's own largest error against it on the same tensor and 1e-5 of the
tensor's largest magnitude (the project's figure for fp32 against a float64
twin).  The kernels' taps are the library's own fp32 formula, which ATen's
weights match to the last bit or the one before: nothing here is compared with
torch for equality."""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import make_net
from oracle import synth

pytestmark = pytest.mark.gpu

SHAPES = [((64, 64), (64, 64)),      # identity, the product case
          ((49, 66), (64, 64)),      # up on one axis, down on the other: a 738 x 994 image
          ((5, 7), (16, 12)),        # upscale above 2x: long gather ranges
          ((16, 12), (5, 7)),        # downscale above 2x: 72 of 192 source cells untouched
          ((1, 1), (3, 3)),          # a single source cell
          ((3, 1), (2, 5)),          # a single source column
          ((6, 9), (8, 8))]          # the end-to-end shape
IDS = [f"{a[0]}x{a[1]}-{b[0]}x{b[1]}" for a, b in SHAPES]


def _sequence(rows, h, w, gt):
    pred = rows.reshape(1, h, w, 256).permute(0, 3, 1, 2).contiguous()
    pred = F.interpolate(pred, gt.shape[2:], mode="bilinear")
    return pred, F.mse_loss(pred, gt, reduction="none").mean()


@functools.lru_cache(maxsize=None)
def case(src, dst):
    """Seeded inputs of one shape, the float64 twin's results and the
    tolerances from the fp32 CPU reference; computed once, never modified."""
    (h, w), (Hg, Wg) = src, dst
    g = torch.Generator().manual_seed(1000 * h + 10 * w + Hg)
    rows = torch.randn(h * w, 256, generator=g)
    gt = torch.randn(1, 256, Hg, Wg, generator=g)
    out = {}
    for name, dt in (("f64", torch.float64), ("f32", torch.float32)):
        x = rows.to(dt).clone().requires_grad_(True)
        pred, loss = _sequence(x, h, w, gt.to(dt))
        loss.backward()
        out[name] = {"resized": pred.detach(), "loss": loss.detach(), "grad": x.grad}
    tol = {}
    for k, ref in out["f64"].items():
        own = (out["f32"][k].double() - ref).abs().max().item()
        tol[k] = max(own, 1e-5 * ref.abs().max().item())
    return rows, gt, out["f64"], tol


def check(name, got, ref, tol):
    err = (got.detach().double().cpu().reshape(ref.shape) - ref).abs().max().item()
    print(f"{name}: max error {err:.3e}, tolerance {tol:.3e}, largest magnitude {ref.abs().max().item():.3e}")
    assert err <= tol, (name, err, tol)


def run(rows, h, w, gt, resized=True, upstream=None):
    from samnerf_amd.feat_loss import feat_loss
    x = rows.detach().clone().requires_grad_(True)
    loss, pred = feat_loss(x, h, w, gt, resized=resized)
    if upstream is None:
        loss.backward()
    else:
        loss.backward(torch.tensor(upstream, device=rows.device))
    return loss.detach(), pred, x.grad


@pytest.mark.parametrize("src,dst", SHAPES, ids=IDS)
def test_matches_the_float64_twin_and_repeats(hip_lib, cuda, src, dst):
    rows, gt, ref, tol = case(src, dst)
    rows, gt = rows.to(cuda), gt.to(cuda)
    loss, pred, grad = run(rows, *src, gt)
    assert loss.dim() == 0 and pred.shape == gt.shape and not pred.requires_grad
    check("resized", pred, ref["resized"], tol["resized"])
    check("loss", loss, ref["loss"], tol["loss"])
    check("grad_pred", grad, ref["grad"], tol["grad"])
    # the same call again: the same bits
    loss2, pred2, grad2 = run(rows, *src, gt)
    assert torch.equal(loss, loss2) and torch.equal(pred, pred2) and torch.equal(grad, grad2)
    # without the resized output: the same loss and gradient bits
    loss3, none, grad3 = run(rows, *src, gt, resized=False)
    assert none is None and torch.equal(loss, loss3) and torch.equal(grad, grad3)
    # half the upstream gradient: exactly half of every value
    _, _, half = run(rows, *src, gt, upstream=0.5)
    assert torch.equal(half, grad * 0.5)


def _raw(L, rows, h, w, gt, grad_loss, grad_pred, resized=None):
    """The two C calls on the current stream, on buffers the caller owns."""
    from samnerf_amd._lib import check as ok
    from samnerf_amd.ops import _ptr, _stream
    Hg, Wg = gt.shape[2:]
    need = L.samnerf_feat_loss_workspace_size(h, w, Hg, Wg)
    ws = torch.empty(need, dtype=torch.uint8, device=rows.device)
    loss = torch.empty((), device=rows.device)

    def go():
        ok(L.samnerf_feat_loss_forward(_ptr(rows), h, w, _ptr(gt), Hg, Wg, _ptr(resized), _ptr(loss), _ptr(ws),
                                       need, _stream(rows)), "forward")
        ok(L.samnerf_feat_loss_backward(_ptr(grad_loss), h, w, Hg, Wg, _ptr(grad_pred), _ptr(ws), need,
                                        _stream(rows)), "backward")
    return go, loss, ws


def test_untouched_source_cells_get_exact_zeros(hip_lib, cuda):
    """(16,12) -> (5,7): the five destination rows touch ten of the sixteen
    source rows, the seven columns all twelve source columns; the other
    6 x 12 = 72 cells of a NaN-filled grad_pred come back as 0.0."""
    src, dst = (16, 12), (5, 7)
    rows, gt, ref, tol = case(src, dst)
    rows, gt = rows.to(cuda), gt.to(cuda)

    def touched_cells(n_in, n_out):
        i0 = (ctypes.c_uint32 * n_out)()
        i1 = (ctypes.c_uint32 * n_out)()
        l1 = (ctypes.c_float * n_out)()
        assert hip_lib.samnerf_bilinear_taps_host(n_in, n_out, i0, i1, l1) == 0
        t = np.zeros(n_in, bool)
        t[list(i0)] = t[list(i1)] = True
        return t

    touched = torch.from_numpy(np.outer(touched_cells(16, 5), touched_cells(12, 7)).reshape(-1))
    assert int((~touched).sum()) == 72
    grad = torch.full((16 * 12, 256), float("nan"), device=cuda)
    go, _, _ = _raw(hip_lib, rows, 16, 12, gt, torch.ones((), device=cuda), grad)
    go()
    grad = grad.cpu()
    assert torch.equal(grad[~touched], torch.zeros(72, 256))
    assert not torch.isnan(grad).any()
    assert torch.equal(ref["grad"][~touched], torch.zeros(72, 256, dtype=torch.float64))
    check("grad_pred", grad, ref["grad"], tol["grad"])


def test_graph_capture_replays_to_the_same_bits(hip_lib, cuda):
    """Forward + backward captured once; the replay on other input values
    equals the eager calls on them: no host synchronisation, and no table
    made on the host from the first inputs."""
    src, dst = (49, 66), (64, 64)
    rows, gt, _, _ = case(src, dst)
    rows, gt = rows.to(cuda), gt.to(cuda)
    other = torch.randn(rows.shape, generator=torch.Generator().manual_seed(5)).to(cuda)
    gl = torch.full((), 0.75, device=cuda)
    want = {}
    for name, x in (("first", rows), ("other", other)):
        grad = torch.empty_like(rows)
        res = torch.empty_like(gt)
        go, loss, _ = _raw(hip_lib, x, *src, gt, gl, grad, res)
        go()
        want[name] = (loss.clone(), res, grad)
    x = rows.clone()
    grad = torch.empty_like(rows)
    res = torch.empty_like(gt)
    go, loss, ws = _raw(hip_lib, x, *src, gt, gl, grad, res)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        go()                                              # warm up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        go()
    for name, values in (("first", rows), ("other", other), ("first", rows)):
        x.copy_(values)
        for t in (grad, res, loss):
            t.fill_(float("nan"))
        ws.zero_()
        graph.replay()
        torch.cuda.synchronize()
        wl, wr, wg = want[name]
        assert torch.equal(loss, wl) and torch.equal(res, wr) and torch.equal(grad, wg), name


@pytest.fixture(scope="module")
def small_view(cuda):
    from samnerf_amd import ops
    spec = synth.ModelSpec(with_sam=True, grid_log2=12, s_grid_log2=11, prop_log2=10)
    params = synth.make_params(spec, seed=21, emb_scale=0.5, ln_jitter=0.1)
    pose, intr = synth.gui_camera(9, 6, rot=synth.random_rotation(4))
    ro, rd = ops.get_rays(pose, intr, 6, 9, device=cuda)
    gt = torch.randn(1, 256, 8, 8, generator=torch.Generator().manual_seed(2)).to(cuda)

    def net():
        n = make_net(spec, params, cuda)
        n.train()
        for k, p in n.named_parameters():                  # main.py:255-262
            p.requires_grad = k.startswith("s_grid") or k.startswith("samvit_mlp")
        return n
    return net, ro, rd, gt


def _grads(net):
    return {k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None}


def test_fused_step_repeats_and_matches_the_torch_loss(hip_lib, cuda, small_view):
    """sam_train_step_fused on a 6 x 9 view against an 8 x 8 target, where the
    torch loss adds the resize's gradient with float atomics: two runs give
    the same bits in all thirteen trained tensors, and those gradients are
    the torch-loss step's within 1e-5 of each tensor's largest magnitude."""
    from samnerf_amd.fused import FusedRenderer
    from samnerf_amd.train import sam_train_step, sam_train_step_fused
    make, ro, rd, gt = small_view
    net = make()
    fr = FusedRenderer(net, deterministic=True)
    runs = []
    for _ in range(2):
        net.zero_grad(set_to_none=True)
        pred, loss = sam_train_step_fused(fr, ro, rd, 6, 9, gt)
        loss.backward()
        runs.append((loss.detach().clone(), pred.clone(), _grads(net)))
    assert len(runs[0][2]) == 13
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    for k in runs[0][2]:
        assert torch.equal(runs[0][2][k], runs[1][2][k]), k
    net.zero_grad(set_to_none=True)
    pred_t, loss_t = sam_train_step(fr, ro, rd, 6, 9, gt)
    loss_t.backward()
    ref = _grads(net)
    check("loss", runs[0][0], loss_t.detach().double().cpu(), 1e-5 * abs(loss_t.item()))
    check("pred", runs[0][1], pred_t.detach().double().cpu(), 1e-5 * pred_t.abs().max().item())
    for k, g in runs[0][2].items():
        check(k, g, ref[k].double().cpu(), 1e-5 * ref[k].abs().max().item())


def test_fused_steps_reduce_the_loss(hip_lib, cuda, small_view):
    from samnerf_amd.fused import FusedRenderer
    from samnerf_amd.optim import FusedAdam
    from samnerf_amd.train import sam_train_step_fused
    make, ro, rd, gt = small_view
    net = make()
    fr = FusedRenderer(net, deterministic=True)
    opt = FusedAdam([p for p in net.parameters() if p.requires_grad], lr=1e-2, eps=1e-15)
    losses = []
    for _ in range(5):
        opt.zero_grad()
        _, loss = sam_train_step_fused(fr, ro, rd, 6, 9, gt, resized=False)
        loss.backward()
        opt.step()
        losses.append(loss.item())
    print("losses", losses)
    assert losses[-1] < losses[0], losses
