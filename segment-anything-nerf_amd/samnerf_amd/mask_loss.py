"""The loss of Trainer.train_step's --with_mask branch (nerf/utils.py:959-1067)
as one call: the negative log-likelihood of the global rays with its
incoherent-region re-weighting, the error-map EMA, the label regularisation
(utils.py:843-870) and the RGB-similarity term of mixed sampling
(utils.py:761-841).

`mask_loss` takes the logits [N, K] of one step: the first `n` rays are the
global rays (opt.num_rays), the rest `L` local patches of `Q` pixels
(opt.num_local_sample, opt.local_sample_patch_size ** 2).  For a contiguous
fp32 CUDA tensor it is samnerf_mask_loss (csrc/mask_loss.hip): one C call
forms the loss and d loss / d logits, fixed-order sums, repeatable to the bit;
the backward scales the saved gradient.  For any other tensor it is the
reference's own torch op sequence (`torch_mask_loss`), which is what a CPU
model runs and what the tests compare the kernels with.

The reference's quirks are kept: the re-weighting multiplies the [n, 1] loss
by the [N] weight vector (a [n, N] broadcast: mean(w) * mean(nll)); the label
regularisation sees the softmax before its clamp (utils.py:964, :1030); the
non-mixed RGB-similarity call (utils.py:1062) lacks an argument and raises.
"""
import ctypes

import torch
import torch.nn.functional as F

from .ops import _o, _ptr, _stream

TERMS = ("nll", "label_regularization", "rgb_similarity", "total", "invalid")


def rgb_similarity_active(opt, global_step):
    """utils.py:1033."""
    return _o(opt, "rgb_similarity_loss_weight", 0) > 0 and global_step > _o(opt, "rgb_similarity_iter", -1)


def coarse_cells(inds, H, W, size):
    """utils.py:269-275: the cell of the size x size error / incoherent map
    under each flat pixel index of an H x W image."""
    row, col = inds // W, inds % W
    cell_row = (row * (size / H)).long()
    cell_col = (col * (size / W)).long()
    return (cell_row * size + cell_col).long()


def draw_similarity_samples(incoherent, num_sample, generator=None):
    """utils.py:779-790: `num_sample` pixels of each local patch, drawn without
    replacement among those whose incoherence is below 0.2 (all of them where
    a patch has none).  incoherent [L, Q] or [L, Q, C] (channel 0 is read);
    returns int64 [L, num_sample]."""
    if incoherent.dim() == 3:
        incoherent = incoherent[..., 0]
    eligible = ((1. - incoherent.to(torch.float32)) > 0.8).to(torch.float32)
    eligible[eligible.sum(-1) == 0] = 1.0
    return torch.multinomial(eligible, num_samples=num_sample, replacement=False, generator=generator)


def _check_config(opt, N, n, K, global_step, depth, image, sample_index, incoherent, error_map,
                  error_cells):
    """The host-side errors shared by both paths; returns (L, Q, S, P, rgb_on, lr_on)."""
    if not 2 <= K <= 32:
        raise ValueError(f"mask_loss: K = {K} instances (n_inst + redundant_instance) must lie in [2, 32]")
    if not 1 <= n <= N:
        raise ValueError(f"mask_loss: n = {n} global rays of N = {N}")
    lr_on = _o(opt, "label_regularization_weight", 0) > 0
    P = int(_o(opt, "patch_size", 1))
    if lr_on:
        if P < 2:
            raise ValueError("mask_loss: label regularisation needs patch_size >= 2 "
                             "(the reference divides 0 by 0 at patch_size 1)")
        if N % (P * P) != 0:
            raise ValueError(f"mask_loss: N = {N} rays are not whole {P} x {P} patches")
        if depth is None:
            raise ValueError("mask_loss: label regularisation needs depth")
    rgb_on = rgb_similarity_active(opt, global_step)
    L = Q = S = 0
    if rgb_on:
        if not _o(opt, "mixed_sampling", False):
            raise TypeError("mask_loss: the RGB-similarity term without mixed_sampling is the "
                            "reference's utils.py:1062, which calls rgb_similarity_loss() without its "
                            "required 'incoherent' argument and raises; use --mixed_sampling")
        L = int(opt.num_local_sample)
        Q = int(opt.local_sample_patch_size) ** 2
        if N - n != L * Q:
            raise ValueError(f"mask_loss: {N - n} local rays are not {L} patches of {Q} pixels")
        if image is None or sample_index is None:
            raise ValueError("mask_loss: the RGB-similarity term needs image and sample_index")
        S = int(sample_index.shape[-1])
        if tuple(sample_index.shape) != (L, S) or not 1 <= S <= Q:
            raise ValueError(f"mask_loss: sample_index must be [{L}, S] with 1 <= S <= {Q}")
    if _o(opt, "incoherent_uncertainty_weight", 1) < 1 and incoherent is None:
        raise ValueError("mask_loss: incoherent_uncertainty_weight < 1 needs the incoherent masks")
    if (error_map is None) != (error_cells is None):
        raise ValueError("mask_loss: error_map and error_cells come together")
    return L, Q, S, P, rgb_on, lr_on


def torch_rgb_similarity(opt, rgb, probs, sample_index):
    """utils.py:793-841 with the drawn sample_index handed in.  rgb [L, Q, 3],
    probs [L, Q, K] (the softmax), sample_index [L, S]."""
    rows = torch.arange(rgb.shape[0], dtype=torch.int64).to(rgb.device)[:, None]
    rgb_s = rgb[rows, sample_index].unsqueeze(2)                        # [L, S, 1, 3]
    mask_s = probs[rows, sample_index].unsqueeze(2).detach()            # [L, S, 1, K]
    if not _o(opt, "rgb_similarity_use_pred_logistics", False):
        top = torch.argmax(mask_s, -1)
        mask_s = torch.zeros_like(mask_s).scatter_(-1, top[..., None], 1)
    similar = torch.norm(rgb.unsqueeze(1) - rgb_s, dim=-1) < opt.rgb_similarity_threshold     # [L, S, Q]
    cos = F.cosine_similarity(probs.unsqueeze(1), mask_s, dim=-1)
    e = torch.exp(- opt.rgb_similarity_exp_weight * cos - opt.epsilon)
    if _o(opt, "redundant_instance", 0) > 0:
        target = (1. - similar.to(torch.int)).to(e.dtype)
        return F.binary_cross_entropy(e, target, reduction='mean')
    return ((similar * e).sum(-1) / similar.sum(-1)).mean()


def torch_label_regularization(P, depth, probs):
    """utils.py:843-870.  depth [N], probs [N, K] (the softmax), N whole P x P patches."""
    q = probs.view(-1, P, P, probs.shape[-1]).permute(0, 3, 1, 2).contiguous()      # [B, K, P, P]
    dx = q[:, :, :, 1:] - q[:, :, :, :-1]
    dy = q[:, :, 1:, :] - q[:, :, :-1, :]
    d = depth.view(-1, P, P)
    ddx = d[:, :, 1:] - d[:, :, :-1]
    ddy = d[:, 1:, :] - d[:, :-1, :]
    wx = torch.exp(-(ddx * ddx)).unsqueeze(1).expand_as(dx)
    wy = torch.exp(-(ddy * ddy)).unsqueeze(1).expand_as(dy)
    return torch.sum(dx * dx * wx) / torch.sum(wx) + torch.sum(dy * dy * wy) / torch.sum(wy)


def torch_mask_loss(logits, labels, n, opt, *, incoherent=None, error_map=None, error_cells=None,
                    depth=None, image=None, sample_index=None, global_step=0):
    """utils.py:959-1067 in the reference's own ops (any device, any float
    dtype).  error_map is updated in place at the flat cells error_cells [n].
    Returns (loss, terms, pred_ids); terms maps TERMS to 0-d tensors."""
    N, K = logits.shape
    L, Q, S, P, rgb_on, lr_on = _check_config(opt, N, n, K, global_step, depth, image, sample_index,
                                              incoherent, error_map, error_cells)
    gt = labels.reshape(-1)
    probs = torch.softmax(logits, dim=-1)
    clamped = torch.clamp(probs.view(-1, K), min=opt.epsilon, max=1 - opt.epsilon)
    if (gt != -1).sum() > 0:                     # any ray labelled: the global rays' NLL
        loss = -torch.log(torch.gather(clamped[:n], -1, gt[:n, None]))
    else:
        loss = torch.tensor(0).to(clamped.dtype).to(logits.device)
    u = _o(opt, "incoherent_uncertainty_weight", 1)
    if u < 1:
        loss = (1 - incoherent + u * incoherent) * loss          # [n, 1] x [N]: the reference's broadcast
    if error_map is not None:
        with torch.no_grad():
            onehot = torch.zeros_like(clamped[:n]).scatter_(-1, gt[:n, None], 1)
            cos = F.cosine_similarity(probs[:n], onehot, dim=-1)
            error = torch.exp(- opt.rgb_similarity_exp_weight * cos - opt.epsilon)
            flat = error_map.view(-1)
            cells = error_cells.reshape(-1)
            flat.scatter_(0, cells, 0.1 * flat.gather(0, cells) + 0.9 * error.to(flat.dtype))
    nll = loss.mean()
    loss = nll
    zero = torch.zeros((), dtype=logits.dtype, device=logits.device)
    lr = rgb = zero
    if lr_on:
        lr = torch_label_regularization(P, depth.detach(), probs)
        loss = loss + lr * opt.label_regularization_weight
    if rgb_on:
        rgb = torch_rgb_similarity(opt, image[n:].detach().view(L, Q, -1), probs[n:].view(L, Q, -1), sample_index)
        loss = loss + rgb * opt.rgb_similarity_loss_weight
    terms = {"nll": nll.detach(), "label_regularization": lr.detach(), "rgb_similarity": rgb.detach(),
             "total": loss.detach(), "invalid": zero}
    return loss, terms, probs.argmax(dim=-1)


class _HipMaskLoss(torch.autograd.Function):
    """samnerf_mask_loss: the forward forms the loss and its gradient, the
    backward scales that gradient by the upstream scalar."""

    @staticmethod
    def forward(ctx, logits, args, keep):
        from ._lib import check, lib
        N, K = logits.shape
        dev = logits.device
        need = lib().samnerf_mask_loss_workspace_size(ctypes.byref(args))
        ws = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
        terms = torch.empty(5, device=dev)
        grad = torch.empty(N, K, device=dev)
        ids = torch.empty(N, dtype=torch.int64, device=dev)
        check(lib().samnerf_mask_loss(ctypes.byref(args), _ptr(logits), _ptr(terms), _ptr(grad), _ptr(ids),
                                      _ptr(ws), need, _stream(logits)), "mask_loss")
        ctx.save_for_backward(grad)
        ctx.mark_non_differentiable(terms, ids)
        return terms[3].clone(), terms, ids

    @staticmethod
    def backward(ctx, g_loss, g_terms, g_ids):
        grad, = ctx.saved_tensors
        return grad * g_loss, None, None


def _hip_mask_loss(logits, labels, n, opt, incoherent, error_map, error_cells, depth, image,
                   sample_index, global_step, check_inputs):
    from ._lib import SamnerfMaskLossArgs
    N, K = logits.shape
    dev = logits.device
    L, Q, S, P, rgb_on, lr_on = _check_config(opt, N, n, K, global_step, depth, image, sample_index,
                                              incoherent, error_map, error_cells)
    keep = []

    def dev_tensor(t, dtype, numel, what):
        if t is None:
            return None
        t = t.detach().to(device=dev, dtype=dtype).reshape(-1).contiguous()
        if t.numel() != numel:
            raise ValueError(f"mask_loss: {what} holds {t.numel()} values, not {numel}")
        keep.append(t)
        return t

    a = SamnerfMaskLossArgs()
    a.N, a.K, a.n = N, K, n
    a.epsilon = float(opt.epsilon)
    a.rgb_exp_weight = float(_o(opt, "rgb_similarity_exp_weight", 10.0))
    a.incoherent_weight = float(_o(opt, "incoherent_uncertainty_weight", 1.0))
    a.labels = dev_tensor(labels, torch.int64, N, "labels").data_ptr()
    if a.incoherent_weight < 1:
        a.incoherent = dev_tensor(incoherent, torch.float32, N, "incoherent").data_ptr()
    if error_map is not None:
        if not (error_map.is_cuda and error_map.dtype == torch.float32 and error_map.is_contiguous()):
            raise ValueError("mask_loss: error_map must be a contiguous fp32 CUDA tensor (updated in place)")
        a.error_map = error_map.data_ptr()
        a.map_cells = error_map.numel()
        a.error_cells = dev_tensor(error_cells, torch.int64, n, "error_cells").data_ptr()
    if lr_on:
        a.P = P
        a.label_reg_weight = float(opt.label_regularization_weight)
        a.depth = dev_tensor(depth, torch.float32, N, "depth").data_ptr()
    if rgb_on:
        a.L, a.Q, a.S = L, Q, S
        a.rgb_weight = float(opt.rgb_similarity_loss_weight)
        a.rgb_threshold = float(opt.rgb_similarity_threshold)
        a.redundant = int(_o(opt, "redundant_instance", 0) > 0)
        a.use_pred_logistics = int(bool(_o(opt, "rgb_similarity_use_pred_logistics", False)))
        a.image = dev_tensor(image, torch.float32, N * 3, "image").data_ptr()
        a.sample_index = dev_tensor(sample_index, torch.int64, L * S, "sample_index").data_ptr()
    loss, terms, ids = _HipMaskLoss.apply(logits, a, keep)
    if check_inputs:
        bad = int(terms[4])                      # the one read-back of the step
        if bad:
            raise RuntimeError(f"mask_loss: {bad} invalid inputs (a label outside [0, {K}) among the "
                               f"{n} global rays, a sample_index outside the patch or an error cell "
                               "outside the map); they were left out of the loss")
    return loss, dict(zip(TERMS, terms.unbind(0))), ids


def mask_loss(logits, labels, n, opt, *, incoherent=None, error_map=None, error_cells=None, depth=None,
              image=None, sample_index=None, global_step=0, check_inputs=True):
    """The --with_mask loss of one training step.  logits [N, K]; labels int64
    [N] (-1 = unlabelled); n: the global rays (opt.num_rays); opt: the
    reference's options (epsilon, incoherent_uncertainty_weight,
    label_regularization_weight + patch_size, rgb_similarity_* + mixed_sampling
    + num_local_sample + local_sample_patch_size, redundant_instance).
    incoherent [N] (the re-weighting), error_map + error_cells [n] (the EMA,
    in place; flat cells index * M + inds_coarse), depth [N] (label
    regularisation), image [N, 3] + sample_index [L, S] (RGB similarity, see
    draw_similarity_samples).  Returns (loss, terms, pred_ids): loss carries
    the gradient to logits, terms maps TERMS to detached 0-d tensors.

    On the HIP path an out-of-range label, sample or cell is never used as an
    index: it is left out and counted in terms['invalid'], and check_inputs
    (one host read-back) raises on a non-zero count."""
    if logits.dim() != 2:
        raise ValueError("mask_loss: logits must be [N, K]")
    n = int(n)
    if logits.is_cuda and logits.dtype == torch.float32 and logits.is_contiguous():
        return _hip_mask_loss(logits, labels, n, opt, incoherent, error_map, error_cells, depth, image,
                              sample_index, global_step, check_inputs)
    return torch_mask_loss(logits, labels, n, opt, incoherent=incoherent, error_map=error_map,
                           error_cells=error_cells, depth=depth, image=image,
                           sample_index=sample_index, global_step=global_step)
