"""Evaluation on the device: Trainer.eval_step and the meters it feeds.

What the reference does with one evaluated view after the render
(nerf/utils.py:1122-1241, :329-512, :1945-2000), as one call:
  * the RGBA composite of the ground truth, the MSE loss and PSNRMeter's
    -10 log10(mean squared error);
  * SSIMMeter's torchmetrics structural_similarity_index_measure at its
    defaults (11 x 11 Gaussian window, sigma 1.5, data range from the images);
  * the uint8 prediction, truth and error images evaluate_one_epoch saves;
  * --with_mask: softmax or sigmoid, the clamped NLL over labeled pixels, the
    argmax ids and MeanIoUMeter's per-class intersections and unions;
  * --with_sam: the feature MSE against gt_samvit.

`eval_frame` is samnerf_eval_frame (csrc/evaluate.hip) for CUDA tensors: raw
sums and counts into one stats record in device memory, nothing copied to the
host, no synchronisation.  `read_stats` derives the finished scalars in
float64 on the host from a copy of the records.  `torch_eval_frame` is the
reference's own op sequence restated op for op -- torch on the tensors' device,
then the meters' host numpy -- which is what CPU tensors get and what the tests
compare the kernels with; on float64 inputs it is the float64 evaluation.
`eval_step` is Trainer.eval_step on a model of this package, `Evaluator` a
table of records for an epoch, and PSNRMeter / SSIMMeter / MeanIoUMeter keep
the reference's interface.

The SSIM is written from torchmetrics' documented defaults; torchmetrics is not
a dependency.  Its reflection padding by 5 and crop by 5 leave exactly the
windows wholly inside the image, so only those are evaluated.  LPIPS, the PNG /
.npy writing and the use_point SAM-decoder branch are not covered.
"""
import ctypes
import os

import numpy as np
import torch
import torch.nn.functional as F

from .ops import _o, _stream, torch_mask_probs

HEADER_BYTES = 128
MAX_CLASSES = 1024
MAX_K = 64
DEFAULT_CLASSES = 256
FEAT = 256
_HEADER = np.dtype([("sq_sum", "<f8"), ("n_elem", "<u8"), ("nll_sum", "<f8"), ("n_labeled", "<u8"),
                    ("ssim_sum", "<f8"), ("n_ssim", "<u8"), ("feat_sq_sum", "<f8"), ("n_feat", "<u8"),
                    ("pred_min", "<f4"), ("pred_max", "<f4"), ("truth_min", "<f4"), ("truth_max", "<f4"),
                    ("overflow", "<u8"), ("reserved", "<u8", (5,))])
assert _HEADER.itemsize == HEADER_BYTES


def stats_bytes(n_classes):
    """SAMNERF_EVAL_STATS_BYTES (include/samnerf_hip.h)."""
    return HEADER_BYTES + ((int(n_classes) * 12 + 7) & ~7)


# ------------------------------------------------------------- torch mirror --

def gaussian_window(dtype=torch.float32, device=None):
    """torchmetrics' _gaussian(11, 1.5): g[i] = exp(-((i - 5) / 1.5)^2 / 2) / sum as float32
    values -- the float64 evaluation rounded once, which is also the kernel's table -- handed out
    in `dtype`.  (torchmetrics evaluates the line in the images' dtype; in float32 the last bits
    then depend on the exp at hand: numpy's and torch's float32 evaluations on the CPU differ
    from each other and from this one, by up to 5 ulps.)"""
    dist = torch.arange((1 - 11) / 2, (1 + 11) / 2, step=1, dtype=torch.float64)
    gauss = torch.exp(-torch.pow(dist / 1.5, 2) / 2)
    return (gauss / gauss.sum()).to(torch.float32).to(device=device, dtype=dtype)


def torch_ssim(preds, truths):
    """structural_similarity_index_measure(preds, truths) at its defaults, for
    [B, 3, H, W] images, in their dtype: the valid windows only (module docstring)."""
    if preds.shape[-2] < 11 or preds.shape[-1] < 11:
        raise ValueError("ssim: H and W must be at least 11 (one whole window)")
    C = preds.shape[1]
    data_range = max(preds.max() - preds.min(), truths.max() - truths.min())
    c1 = pow(0.01 * data_range, 2)
    c2 = pow(0.03 * data_range, 2)
    g = gaussian_window(preds.dtype, preds.device)
    kernel = torch.matmul(g[:, None], g[None, :]).expand(C, 1, 11, 11)
    inputs = torch.cat((preds, truths, preds * preds, truths * truths, preds * truths))
    outputs = F.conv2d(inputs, kernel, groups=C)
    mu_p, mu_t, e_pp, e_tt, e_pt = outputs.split(preds.shape[0])
    mu_pred_sq, mu_target_sq, mu_pred_target = mu_p.pow(2), mu_t.pow(2), mu_p * mu_t
    sigma_pred_sq = e_pp - mu_pred_sq
    sigma_target_sq = e_tt - mu_target_sq
    sigma_pred_target = e_pt - mu_pred_target
    upper = 2 * sigma_pred_target + c2
    lower = sigma_pred_sq + sigma_target_sq + c2
    full = ((2 * mu_pred_target + c1) * upper) / ((mu_pred_sq + mu_target_sq + c1) * lower)
    return full.reshape(full.shape[0], -1).mean(-1).mean()


def _np(x):
    return x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


def numpy_psnr(preds, truths):
    """PSNRMeter.update's value (utils.py:352)."""
    return -10 * np.log10(np.mean((_np(preds) - _np(truths)) ** 2))


def numpy_iou_terms(preds, truths, n_classes=None):
    """MeanIoUMeter.update (utils.py:484-496): per class the intersection and the
    union counts, and the mean IoU over the classes with a union (float64)."""
    preds, truths = _np(preds).astype(np.int64), _np(truths).astype(np.int64)
    num_classes = max(preds.max() + 1, truths.max() + 1) if n_classes is None else n_classes
    inter, union, ious = [], [], []
    for i in range(num_classes):
        intersection = np.logical_and(preds == i, truths == i).sum()
        u = np.logical_or(preds == i, truths == i).sum()
        inter.append(intersection)
        union.append(u)
        if u > 0:
            ious.append(intersection / u)
    return np.asarray(inter, np.int64), np.asarray(union, np.int64), np.mean(ious)


def miou_from_hist(inter, npred, ntruth):
    """The same float64 mean from the three histograms, in class order."""
    inter, union = np.asarray(inter, np.int64), np.asarray(npred, np.int64) + np.asarray(ntruth, np.int64) - inter
    ious = [inter[i] / union[i] for i in range(len(union)) if union[i] > 0]
    return np.mean(ious)


def _check_parts(pred_rgb, truth, logits, labels, n_inst, pred_feat, gt_feat):
    if pred_rgb is None and logits is None and pred_feat is None:
        raise ValueError("eval_frame: nothing to evaluate (pred_rgb, logits and pred_feat are all None)")
    if (pred_rgb is None) != (truth is None):
        raise ValueError("eval_frame: pred_rgb and truth come together")
    if (logits is None) != (labels is None):
        raise ValueError("eval_frame: logits and labels come together")
    if (pred_feat is None) != (gt_feat is None):
        raise ValueError("eval_frame: pred_feat and gt_feat come together")
    if pred_rgb is not None:
        if truth.dim() != 3 or truth.shape[-1] not in (3, 4):
            raise ValueError("eval_frame: truth must be [H, W, 3] or [H, W, 4]")
        if pred_rgb.numel() != truth.shape[0] * truth.shape[1] * 3:
            raise ValueError(f"eval_frame: pred_rgb of {tuple(pred_rgb.shape)} against truth {tuple(truth.shape)}")
    if logits is not None:
        K = int(logits.shape[-1])
        if n_inst is None or not 1 <= int(n_inst) <= K:
            raise ValueError(f"eval_frame: logits need n_inst in [1, K = {K}]")
        if logits.numel() != labels.numel() * K:
            raise ValueError(f"eval_frame: logits of {tuple(logits.shape)} against {labels.numel()} labels")
    if pred_feat is not None:
        if gt_feat.dim() != 4 or gt_feat.shape[0] != 1 or gt_feat.shape[1] != FEAT:
            raise ValueError("eval_frame: gt_feat must be [1, 256, h, w]")
        if pred_feat.numel() != gt_feat.numel():
            raise ValueError("eval_frame: pred_feat and gt_feat differ in size; resize with torch ops first")


def torch_eval_frame(pred_rgb=None, truth=None, *, bg_color=1, ssim=True, buffers=False, logits=None,
                     labels=None, n_inst=None, epsilon=1e-6, n_classes=None, pred_feat=None, gt_feat=None):
    """eval_frame in the reference's own ops, on any device and in the inputs'
    float dtype.  Returns a dict of what the view's parts give:
      RGB   'truth' [H, W, 3] (the composite), 'mse' (the loss, a 0-d tensor),
            'psnr' (numpy, as PSNRMeter returns it), 'ssim' (0-d tensor, with
            ssim=True), 'pred_min' .. 'truth_max', and with buffers=True the
            'pred_u8', 'truth_u8' [H, W, 3] and 'error_u8' [H, W] numpy arrays;
      mask  'probs' [H, W, K], 'ids' [H, W], 'nll' (the loss, 0-d tensor),
            'n_labeled', 'inter', 'npred', 'ntruth' (int64 numpy [n_classes];
            n_classes None: the meter's own max + 1), 'miou' (float64);
      SAM   'feat_mse' (0-d tensor)."""
    _check_parts(pred_rgb, truth, logits, labels, n_inst, pred_feat, gt_feat)
    out = {}
    if pred_rgb is not None:
        H, W, C = truth.shape
        pred = pred_rgb.reshape(H, W, 3)
        images = truth
        if C == 4:                                             # utils.py:1141-1145
            gt_rgb = images[..., :3] * images[..., 3:] + bg_color * (1 - images[..., 3:])
        else:
            gt_rgb = images
        out["truth"] = gt_rgb
        out["mse"] = F.mse_loss(pred, gt_rgb, reduction="none").mean()
        out["psnr"] = numpy_psnr(pred, gt_rgb)
        for k, v in (("pred_min", pred.min()), ("pred_max", pred.max()), ("truth_min", gt_rgb.min()),
                     ("truth_max", gt_rgb.max())):
            out[k] = v
        if ssim:                                               # SSIMMeter.prepare_inputs, update
            p4, t4 = (x.unsqueeze(0).permute(0, 3, 1, 2).contiguous() for x in (pred, gt_rgb))
            out["ssim"] = torch_ssim(p4, t4)
        if buffers:                                            # utils.py:1984-1999
            p8 = (_np(pred) * 255).astype(np.uint8)
            t8 = (_np(gt_rgb) * 255).astype(np.uint8)
            out["pred_u8"], out["truth_u8"] = p8, t8
            out["error_u8"] = np.abs(t8.astype(np.float32) - p8.astype(np.float32)).mean(-1).astype(np.uint8)
    if logits is not None:
        K = int(logits.shape[-1])
        gt_mask = labels.to(torch.long)
        shape = tuple(gt_mask.shape) if gt_mask.dim() >= 2 else (gt_mask.numel(),)
        gt_flat = gt_mask.reshape(-1)
        labeled = gt_flat != -1
        inst_mask = logits.reshape(*shape, K)
        pred_mask = torch_mask_probs(inst_mask, n_inst)
        flat = torch.clamp(pred_mask.reshape(-1, K), min=epsilon, max=1 - epsilon)
        if labeled.sum() > 0:
            loss = -torch.log(torch.gather(flat[labeled], -1, gt_flat[labeled][..., None]))
        else:
            loss = torch.tensor(0).to(flat.dtype).to(flat.device)
        out["probs"], out["nll"], out["n_labeled"] = pred_mask, loss.mean(), int(labeled.sum())
        ids = pred_mask.argmax(-1)                             # utils.py:1953
        out["ids"] = ids
        inter, union, miou = numpy_iou_terms(ids, gt_mask, n_classes)
        pi, ti = _np(ids).reshape(-1), _np(gt_flat)
        nc = len(inter)
        out["inter"] = inter
        out["npred"] = np.bincount(pi[(pi >= 0) & (pi < nc)], minlength=nc).astype(np.int64)
        out["ntruth"] = np.bincount(ti[(ti >= 0) & (ti < nc)], minlength=nc).astype(np.int64)
        assert np.array_equal(out["npred"] + out["ntruth"] - inter, union)
        out["miou"] = miou
    if pred_feat is not None:
        h, w = gt_feat.shape[2:]
        pred_samvit = pred_feat.reshape(1, h, w, FEAT).permute(0, 3, 1, 2).contiguous()
        pred_samvit = F.interpolate(pred_samvit, gt_feat.shape[2:], mode="bilinear")
        out["feat_mse"] = F.mse_loss(pred_samvit, gt_feat, reduction="none").mean()
    return out


# ------------------------------------------------------------------ kernels --

def read_stats(stats, n_classes=0):
    """The finished values of stats records, on the host in float64: stats a
    uint8 tensor or array [..., stats_bytes(n_classes)] (one copy when it is on
    the device).  Returns a list of dicts (one dict for a single record) with
    'mse', 'psnr', 'ssim', 'nll', 'miou', 'feat_mse' (None where the part was
    not evaluated), the raw sums and counts, min / max and the histograms.
    Raises where a record counted ids or labels it could not index."""
    raw = np.ascontiguousarray(_np(stats)).view(np.uint8)
    nb = stats_bytes(n_classes)
    single = raw.ndim == 1
    raw = raw.reshape(-1, raw.shape[-1])
    if raw.shape[1] < nb:
        raise ValueError(f"read_stats: records of {raw.shape[1]} bytes, {nb} needed for {n_classes} classes")
    res = []
    for r in raw:
        h = r[:HEADER_BYTES].view(_HEADER)[0]
        if int(h["overflow"]):
            raise RuntimeError(f"eval_frame: {int(h['overflow'])} ids or labels outside the classes "
                               f"(labels must lie in [-1, K), ids and labels below n_classes = {n_classes})")
        d = {k: (float(h[k]) if _HEADER[k].kind == "f" else int(h[k])) for k in _HEADER.names if k != "reserved"}
        for k in ("pred_min", "pred_max", "truth_min", "truth_max"):
            d[k] = np.float32(h[k])
        d["mse"] = d["sq_sum"] / d["n_elem"] if d["n_elem"] else None
        d["psnr"] = -10 * np.log10(np.float64(d["mse"])) if d["n_elem"] else None
        d["ssim"] = d["ssim_sum"] / d["n_ssim"] if d["n_ssim"] else None
        d["feat_mse"] = d["feat_sq_sum"] / d["n_feat"] if d["n_feat"] else None
        d["nll"] = d["miou"] = None
        if n_classes:
            hist = r[HEADER_BYTES:HEADER_BYTES + 12 * n_classes].view("<u4").reshape(3, n_classes).astype(np.int64)
            d["inter"], d["npred"], d["ntruth"] = hist
            if hist[1].sum() or hist[2].sum():
                d["nll"] = d["nll_sum"] / d["n_labeled"] if d["n_labeled"] else 0.0
                d["miou"] = miou_from_hist(*hist)
        res.append(d)
    return res[0] if single else res


def _hip_eval_frame(pred_rgb, truth, bg_color, ssim, buffers, logits, labels, n_inst, epsilon, n_classes,
                    pred_feat, gt_feat, stats, return_extra):
    from ._lib import SamnerfEvalArgs, check, lib
    ref = pred_rgb if pred_rgb is not None else (logits if logits is not None else pred_feat)
    dev = ref.device
    keep = []

    def dev_tensor(t, dtype):
        t = t.detach().to(device=dev, dtype=dtype).contiguous()
        keep.append(t)
        return t.data_ptr()

    a = SamnerfEvalArgs()
    a.bg_color, a.epsilon = float(bg_color), float(epsilon)
    out = {}
    if pred_rgb is not None:
        H, W, C = (int(v) for v in truth.shape)
        a.H, a.W, a.C, a.ssim = H, W, C, int(bool(ssim))
        a.pred_rgb, a.truth = dev_tensor(pred_rgb, torch.float32), dev_tensor(truth, torch.float32)
        if ssim and (H < 11 or W < 11):
            raise ValueError("eval_frame: SSIM needs H and W of at least 11 (one whole window)")
        if return_extra:
            out["truth"] = truth if C == 3 else torch.empty(H, W, 3, device=dev)
            if C == 4:
                a.truth_out = out["truth"].data_ptr()
        if buffers:
            out["pred_u8"] = torch.empty(H, W, 3, dtype=torch.uint8, device=dev)
            out["truth_u8"] = torch.empty(H, W, 3, dtype=torch.uint8, device=dev)
            out["error_u8"] = torch.empty(H, W, dtype=torch.uint8, device=dev)
            a.pred_u8, a.truth_u8, a.error_u8 = (out[k].data_ptr() for k in ("pred_u8", "truth_u8", "error_u8"))
    nc = 0
    if logits is not None:
        K = int(logits.shape[-1])
        if K > MAX_K:
            raise ValueError(f"eval_frame: K = {K} instances, at most {MAX_K}")
        nc = int(n_classes) if n_classes is not None else K
        if not 1 <= nc <= MAX_CLASSES:
            raise ValueError(f"eval_frame: n_classes = {nc} outside [1, {MAX_CLASSES}]")
        shape = tuple(labels.shape) if labels.dim() >= 2 else (labels.numel(),)
        n = labels.numel()
        if pred_rgb is not None and n != a.H * a.W:
            raise ValueError("eval_frame: the mask part and the RGB part differ in size")
        if pred_rgb is None:
            a.H, a.W = (int(shape[0]), int(n // shape[0])) if len(shape) >= 2 else (1, n)
        a.K, a.n_inst, a.n_classes = K, int(n_inst), nc
        a.logits, a.labels = dev_tensor(logits, torch.float32), dev_tensor(labels, torch.int64)
        if return_extra:
            out["probs"] = torch.empty(*shape, K, device=dev)
            out["ids"] = torch.empty(*shape, dtype=torch.int64, device=dev)
            a.probs, a.ids = out["probs"].data_ptr(), out["ids"].data_ptr()
    if pred_feat is not None:
        a.h, a.w = int(gt_feat.shape[2]), int(gt_feat.shape[3])
        a.pred_feat, a.gt_feat = dev_tensor(pred_feat, torch.float32), dev_tensor(gt_feat, torch.float32)
    nb = stats_bytes(nc)
    if stats is None:
        stats = torch.empty(nb, dtype=torch.uint8, device=dev)
    elif not (stats.is_cuda and stats.dtype == torch.uint8 and stats.is_contiguous() and stats.numel() >= nb
              and stats.data_ptr() % 8 == 0):
        raise ValueError(f"eval_frame: stats must be a contiguous, 8-byte aligned uint8 CUDA tensor of {nb} bytes")
    a.stats = stats.data_ptr()
    need = ctypes.c_size_t(0)
    check(lib().samnerf_eval_workspace_size(ctypes.byref(a), ctypes.byref(need)), "eval_frame")
    ws = torch.empty(need.value // 8, dtype=torch.float64, device=dev)
    a.workspace, a.workspace_bytes = ws.data_ptr(), need.value
    check(lib().samnerf_eval_frame(ctypes.byref(a), _stream(stats)), "eval_frame")
    out["stats"] = stats
    return out


def eval_frame(pred_rgb=None, truth=None, *, bg_color=1, ssim=True, buffers=False, logits=None, labels=None,
               n_inst=None, epsilon=1e-6, n_classes=None, pred_feat=None, gt_feat=None, stats=None,
               return_extra=True):
    """One evaluated view.

    RGB part: pred_rgb [H*W, 3] or [H, W, 3] and truth [H, W, 3 or 4] (RGBA is
    composited over bg_color); ssim adds the SSIM sum (H, W >= 11); buffers adds
    the uint8 prediction, truth and error images.  Mask part: logits [..., K]
    with n_inst (K = n_inst + redundant_instance <= 64) and labels [...] int64
    (-1 = unlabeled), epsilon (opt.epsilon), n_classes bins (default K; <= 1024).
    SAM part: pred_feat [h*w, 256] in the render's layout and gt_feat
    [1, 256, h, w] of the same size.

    CUDA tensors go to the HIP kernels: the result is {'stats': the record (a
    uint8 device tensor, `stats` itself where given: one row of an Evaluator's
    table), and with return_extra 'truth', 'probs', 'ids', with buffers
    'pred_u8', 'truth_u8', 'error_u8'}, all on the device and none read back;
    read_stats(result['stats'], n_classes) finishes the scalars.  Anything else
    goes to torch_eval_frame."""
    _check_parts(pred_rgb, truth, logits, labels, n_inst, pred_feat, gt_feat)
    ref = pred_rgb if pred_rgb is not None else (logits if logits is not None else pred_feat)
    if ref.is_cuda:
        return _hip_eval_frame(pred_rgb, truth, bg_color, ssim, buffers, logits, labels, n_inst, epsilon,
                               n_classes, pred_feat, gt_feat, stats, return_extra)
    return torch_eval_frame(pred_rgb, truth, bg_color=bg_color, ssim=ssim, buffers=buffers, logits=logits,
                            labels=labels, n_inst=n_inst, epsilon=epsilon, n_classes=n_classes,
                            pred_feat=pred_feat, gt_feat=gt_feat)


def eval_confusion(pred_ids, truth_ids, n_classes=DEFAULT_CLASSES, stats=None):
    """samnerf_eval_confusion: the three histograms of two CUDA id maps into a
    stats record (returned; nothing is read back)."""
    from ._lib import check, lib
    dev = pred_ids.device
    p = pred_ids.detach().to(device=dev, dtype=torch.int64).reshape(-1).contiguous()
    t = truth_ids.detach().to(device=dev, dtype=torch.int64).reshape(-1).contiguous()
    if p.numel() != t.numel():
        raise ValueError("eval_confusion: the id maps differ in size")
    if stats is None:
        stats = torch.empty(stats_bytes(n_classes), dtype=torch.uint8, device=dev)
    check(lib().samnerf_eval_confusion(p.data_ptr(), t.data_ptr(), p.numel(), int(n_classes), stats.data_ptr(),
                                       _stream(stats)), "eval_confusion")
    return stats


# ------------------------------------------------------------------ eval_step --

def _field(stats, name, dtype):
    off = _HEADER.fields[name][1]
    return stats[off:off + 8].view(dtype)[0]


def _device_mean(stats, total, count):
    """total / count of a device record as a float32 0-d tensor, 0 at count 0; no read-back."""
    s, n = _field(stats, total, torch.float64), _field(stats, count, torch.int64)
    return torch.where(n > 0, s / n.clamp(min=1).to(torch.float64), torch.zeros_like(s)).to(torch.float32)


def eval_step(model, data, opt, criterion=None, stats=None, sam_features=None, predictor=None):
    """Trainer.eval_step (utils.py:1122-1241) on a model of this package:
    returns (pred_rgb, pred_depth, pred_extra, truth, loss) as the reference
    does -- the RGB branch (None, gt_rgb, MSE), --with_mask (pred_mask [H, W, K],
    gt_mask, the NLL; 0 under data['use_default_intrinsics']) and --with_sam
    without use_point (pred_samvit [1, 256, h, w], pred_rgb, the feature MSE;
    sam_features(image_uint8) -> gt_samvit [1, 256, h', w'] stands for the SAM
    predictor; with predictor= instead, an object with SamPredictor's interface,
    gt_samvit comes from teacher.set_image_from_render and the render never
    leaves the device).  criterion: None or an MSELoss (the reference's) goes to the
    kernels; anything else is applied with torch ops.  stats: the record to
    fill (a row of an Evaluator's table).  On CUDA the loss is a device tensor
    derived from the record without a read-back."""
    H, W = int(data["H"]), int(data["W"])
    cnf = data["cam_near_far"] if "cam_near_far" in data else None
    with_mask, with_sam = bool(_o(opt, "with_mask", False)), bool(_o(opt, "with_sam", False))
    outputs = model.render(data["rays_o"], data["rays_d"], staged=True, index=data.get("index"), bg_color=1,
                           perturb=False, cam_near_far=cnf, return_feats=0, return_mask=with_mask)
    pred_rgb = outputs["image"].reshape(H, W, 3)
    pred_depth = outputs["depth"].reshape(H, W)
    cuda = pred_rgb.is_cuda
    plain_mse = criterion is None or (isinstance(criterion, torch.nn.MSELoss) and criterion.reduction == "none")
    if not with_sam and not with_mask:
        images = data["images"]
        if images.dim() == 4:
            images = images.reshape(H, W, -1)
        r = eval_frame(pred_rgb, images, bg_color=1, ssim=min(H, W) >= 11, stats=stats)
        gt_rgb = r["truth"]
        if not plain_mse:
            loss = criterion(pred_rgb, gt_rgb).mean()
        else:
            loss = _device_mean(r["stats"], "sq_sum", "n_elem") if cuda else r["mse"]
        return pred_rgb, pred_depth, None, gt_rgb, loss
    if with_mask:
        n_inst, red = int(opt.n_inst), int(_o(opt, "redundant_instance", 0))
        if red > 0:
            # utils.py:1170: view(-1, n_inst) of [H, W, n_inst + redundant] raises where H W K is no
            # multiple of n_inst (recorded: tests/golden/eval.npz), and has K / n_inst rows a pixel
            # otherwise, which the boolean index by `labeled` [H * W] rejects
            raise RuntimeError(f"eval_step: redundant_instance = {red} > 0: the reference's view(-1, n_inst) no "
                               "longer has one row per pixel and eval_step raises")
        gt_mask = data["masks"].to(torch.long)
        logits = outputs["instance_mask_logits"].reshape(H, W, n_inst)
        labels = gt_mask.reshape(H, W)
        r = eval_frame(logits=logits, labels=labels, n_inst=n_inst, epsilon=float(opt.epsilon), stats=stats,
                       n_classes=_o(opt, "eval_classes", None))
        pred_mask = r["probs"]
        if data.get("use_default_intrinsics", False):
            return pred_rgb, pred_depth, pred_mask, gt_mask, torch.tensor(0.)
        loss = _device_mean(r["stats"], "nll_sum", "n_labeled") if cuda else r["nll"]
        w = float(_o(opt, "label_regularization_weight", 0))
        if w > 0:
            from .mask_loss import mask_loss, torch_label_regularization
            depth = outputs["depth"].detach().reshape(-1)
            if cuda and 2 <= n_inst <= 32:
                _, terms, _ = mask_loss(logits.reshape(-1, n_inst).contiguous(), torch.zeros_like(labels).reshape(-1),
                                        H * W, opt, depth=depth, check_inputs=False)
                reg = terms["label_regularization"]
            else:
                reg = torch_label_regularization(int(opt.patch_size), depth, pred_mask.reshape(-1, n_inst))
            loss = loss + reg * w
        return pred_rgb, pred_depth, pred_mask, gt_mask, loss
    if _o(opt, "use_point", False):
        raise NotImplementedError("eval_step: the use_point branch runs the SAM decoder (sam_bridge); not covered")
    if predictor is not None:
        from .teacher import set_image_from_render
        gt_samvit = set_image_from_render(predictor, pred_rgb.detach())
    elif sam_features is None:
        raise ValueError("eval_step: --with_sam needs sam_features(image_uint8) -> gt_samvit [1, 256, h, w], "
                         "or predictor=")
    else:
        image = (pred_rgb.detach().cpu().numpy() * 255).astype(np.uint8)
        gt_samvit = sam_features(image)
    h, w = int(data["h"]), int(data["w"])
    out2 = model.render(data["rays_o_lr"], data["rays_d_lr"], staged=False, index=data.get("index"), bg_color=1,
                        perturb=False, cam_near_far=cnf, return_feats=1, H=h, W=w)
    feat = out2["samvit"].reshape(h * w, FEAT)
    pred_samvit = feat.reshape(1, h, w, FEAT).permute(0, 3, 1, 2)
    if tuple(gt_samvit.shape[2:]) == (h, w) and plain_mse:
        # F.interpolate(..., mode='bilinear') to the prediction's own size is the identity
        r = eval_frame(pred_feat=feat, gt_feat=gt_samvit, stats=stats)
        loss = _device_mean(r["stats"], "feat_sq_sum", "n_feat") if cuda else r["feat_mse"]
        return pred_rgb, pred_depth, pred_samvit.contiguous(), pred_rgb, loss
    pred_samvit = F.interpolate(pred_samvit.contiguous(), gt_samvit.shape[2:], mode="bilinear")
    crit = criterion if criterion is not None else torch.nn.MSELoss(reduction="none")
    return pred_rgb, pred_depth, pred_samvit, pred_rgb, crit(pred_samvit, gt_samvit).mean()


# ------------------------------------------------------------------- epochs --

class Evaluator:
    """The stats table of one evaluation epoch: n_views records in device
    memory.  update(i, ...) fills record i (eval_frame's arguments; no host
    synchronisation); results() makes the one copy and returns
    {'views': [per-view dicts of read_stats], 'loss', 'psnr', 'ssim', 'miou':
    float64 means over the views that have the value}."""

    def __init__(self, n_views, n_classes=0, device="cuda"):
        self.n_views, self.n_classes = int(n_views), int(n_classes)
        self.table = torch.zeros(self.n_views, stats_bytes(self.n_classes), dtype=torch.uint8, device=device)

    def update(self, i, *args, **kw):
        if self.n_classes:
            kw.setdefault("n_classes", self.n_classes)
        return eval_frame(*args, stats=self.table[i], **kw)

    def results(self):
        views = read_stats(self.table, self.n_classes)
        out = {"views": views}
        for v in views:
            v["loss"] = v["mse"] if v["mse"] is not None else (v["nll"] if v["nll"] is not None else v["feat_mse"])
        for k in ("loss", "psnr", "ssim", "miou"):
            vals = [v[k] for v in views if v[k] is not None]
            out[k] = float(np.mean(np.asarray(vals, np.float64))) if vals else None
        return out


class _Meter:
    name_ = ""

    def __init__(self):
        self.clear()

    def clear(self):
        self.V = 0
        self.N = 0
        self._records = []

    def _value(self, d):
        raise NotImplementedError

    def _n_classes(self):
        return 0

    def measure(self):
        if self._records:                                       # the first host read
            recs, self._records = torch.stack(self._records), []
            for d in read_stats(recs, self._n_classes()):
                self.V += self._value(d)
                self.N += 1
        return self.V / self.N if self.N > 0 else 0

    def write(self, writer, global_step, prefix=""):
        writer.add_scalar(os.path.join(prefix, self.name_), self.measure(), global_step)

    def report(self):
        return f"{self.name_} = {self.measure():.6f}"


def _hwc(x):
    return x.reshape(-1, *x.shape[-2:]) if x.dim() != 3 else x


class _Pending:
    """A view's PSNR still in its device record: float() or format() reads it.
    evaluate_one_epoch puts update()'s value into the error image's file name
    (utils.py:1979); a caller that does not look never waits."""

    def __init__(self, record):
        self.record = record

    def __float__(self):
        return float(read_stats(self.record)["psnr"])

    def __format__(self, spec):
        return format(float(self), spec)


class PSNRMeter(_Meter):
    """utils.py:329-370.  CUDA tensors accumulate on the device; measure() reads."""
    name_ = "PSNR"

    def update(self, preds, truths):
        if torch.is_tensor(preds) and preds.is_cuda:
            t = _hwc(truths)
            self._records.append(eval_frame(preds, t, ssim=False, return_extra=False)["stats"])
            return _Pending(self._records[-1])
        psnr = numpy_psnr(preds, truths)
        self.V += psnr
        self.N += 1
        return psnr

    def _value(self, d):
        return d["psnr"]


class SSIMMeter(_Meter):
    """utils.py:421-463."""
    name_ = "SSIM"

    def __init__(self, device=None):
        super().__init__()
        self.device = device

    def update(self, preds, truths):
        if preds.is_cuda:
            self._records.append(eval_frame(preds, _hwc(truths), ssim=True, return_extra=False)["stats"])
            return
        p4, t4 = ((x.unsqueeze(0) if len(x.shape) == 3 else x).permute(0, 3, 1, 2).contiguous()
                  for x in (preds, truths))
        self.V += torch_ssim(p4, t4)
        self.N += 1

    def _value(self, d):
        return d["ssim"]


class MeanIoUMeter(_Meter):
    """utils.py:466-512.  On the device the classes are n_classes bins (the
    reference takes max + 1 of each pair of maps; an empty class adds nothing
    to the mean, so any n_classes above the largest id gives its value, and a
    larger id makes measure() raise)."""
    name_ = "mIoU"

    def __init__(self, n_classes=DEFAULT_CLASSES):
        super().__init__()
        self.n_classes = int(n_classes)

    def _n_classes(self):
        return self.n_classes

    def update(self, preds, truths):
        if torch.is_tensor(preds) and preds.is_cuda:
            self._records.append(eval_confusion(preds, truths.to(preds.device), self.n_classes))
            return
        self.V += numpy_iou_terms(preds, truths)[2]
        self.N += 1

    def _value(self, d):
        return miou_from_hist(d["inter"], d["npred"], d["ntruth"])

    def name(self):
        return "mIoU"
