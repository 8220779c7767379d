"""The loss of Trainer.train_step's SAM-distillation branch
(nerf/utils.py:1094-1108) as one call: the rendered feature rows [h*w, 256]
resized to the teacher's [1, 256, Hg, Wg] map (bilinear, align_corners=False)
and their mean squared error.

`feat_loss` takes the render's ray-major `samvit` as it is.  For a contiguous
fp32 CUDA tensor it is samnerf_feat_loss_forward / _backward
(csrc/feat_loss.hip): three launches forward and one backward, no copy between
the two layouts, no float atomics -- the step repeats bit for bit at every
size, not only where the resize is the identity -- and the upstream gradient
goes to the kernel as a device pointer.  For any other tensor it is the
reference's own op sequence (`torch_feat_loss`), which is what a CPU model
runs and what the tests compare the kernels with.

The kernels' taps are the library's own fp32 definition (include/samnerf_hip.h);
ATen's weights differ from them in the last bit at some size pairs, so the two
paths agree to rounding, not to the bit.
"""
import torch
import torch.nn.functional as F

from .ops import _ptr, _stream

FEAT = 256
MAX_SIDE = 1024


def _check_shapes(pred, h, w, gt_samvit):
    h, w = int(h), int(w)
    if pred.dim() != 2 or tuple(pred.shape) != (h * w, FEAT):
        raise ValueError(f"feat_loss: pred must be [h * w, {FEAT}] = [{h * w}, {FEAT}], not {tuple(pred.shape)}")
    if gt_samvit.dim() != 4 or gt_samvit.shape[0] != 1 or gt_samvit.shape[1] != FEAT:
        raise ValueError(f"feat_loss: gt_samvit must be [1, {FEAT}, Hg, Wg], not {tuple(gt_samvit.shape)}")
    Hg, Wg = int(gt_samvit.shape[2]), int(gt_samvit.shape[3])
    if not all(1 <= n <= MAX_SIDE for n in (h, w, Hg, Wg)):
        raise ValueError(f"feat_loss: sizes {h} x {w} -> {Hg} x {Wg} must lie in [1, {MAX_SIDE}]")
    return h, w, Hg, Wg


def torch_feat_loss(pred, h, w, gt_samvit, resized=True):
    """utils.py:1101-1106 in the reference's own ops (any device, any float
    dtype): the rows as an NCHW map, F.interpolate to the teacher's size, the
    mean of the squared differences.  Returns (loss, pred_samvit | None)."""
    h, w, _, _ = _check_shapes(pred, h, w, gt_samvit)
    p = pred.reshape(1, h, w, FEAT).permute(0, 3, 1, 2).contiguous()
    p = F.interpolate(p, gt_samvit.shape[2:], mode="bilinear")
    loss = F.mse_loss(p, gt_samvit, reduction="none").mean()
    return loss, (p if resized else None)


class _HipFeatLoss(torch.autograd.Function):
    """samnerf_feat_loss_forward, and samnerf_feat_loss_backward on the
    workspace it left."""

    @staticmethod
    def forward(ctx, pred, h, w, gt, want_resized):
        from ._lib import check, lib
        dev = pred.device
        Hg, Wg = gt.shape[2], gt.shape[3]
        need = lib().samnerf_feat_loss_workspace_size(h, w, Hg, Wg)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        loss = torch.empty((), device=dev)
        out = torch.empty(1, FEAT, Hg, Wg, device=dev) if want_resized else None
        check(lib().samnerf_feat_loss_forward(_ptr(pred), h, w, _ptr(gt), Hg, Wg, _ptr(out), _ptr(loss),
                                              _ptr(ws), need, _stream(pred)), "feat_loss_forward")
        ctx.save_for_backward(ws)
        ctx.sizes = (h, w, Hg, Wg, need)
        if out is not None:
            ctx.mark_non_differentiable(out)
        return loss, out

    @staticmethod
    def backward(ctx, g_loss, g_resized):
        from ._lib import check, lib
        ws, = ctx.saved_tensors
        h, w, Hg, Wg, need = ctx.sizes
        g = g_loss.detach().to(device=ws.device, dtype=torch.float32).reshape(1).contiguous()   # stays on the device
        grad = torch.empty(h * w, FEAT, device=ws.device)
        check(lib().samnerf_feat_loss_backward(_ptr(g), h, w, Hg, Wg, _ptr(grad), _ptr(ws), need,
                                               _stream(ws)), "feat_loss_backward")
        return grad, None, None, None, None


def feat_loss(pred, h, w, gt_samvit, resized=True):
    """The distillation loss of one step.  pred [h * w, 256]: the render's
    samvit, ray-major (may require grad); gt_samvit [1, 256, Hg, Wg]: the
    teacher's map; every size in [1, 1024].  Returns (loss, pred_samvit):
    loss is a 0-d tensor that carries the gradient to pred, pred_samvit the
    resized prediction [1, 256, Hg, Wg] without gradient (None with
    resized=False, which also saves its store)."""
    h, w, Hg, Wg = _check_shapes(pred, h, w, gt_samvit)
    if pred.is_cuda and pred.dtype == torch.float32 and pred.is_contiguous():
        gt = gt_samvit.detach().to(device=pred.device, dtype=torch.float32).contiguous()
        return _HipFeatLoss.apply(pred, h, w, gt, bool(resized))
    return torch_feat_loss(pred, h, w, gt_samvit, resized=resized)
