"""Frame presentation: from a render's outputs to the GUI's display buffer.

What the reference does after the render, as one call:
  * the mask views of Trainer.test_step (nerf/utils.py:1263-1306): softmax or
    sigmoid of the logits, max and argmax, and one of the --render_mask_type
    displays (overlay_mask_heatmap / _composition / _only, utils.py:55-94) with
    --render_mask_instance_id and the 100-colour map of utils.py:606-610;
  * the SAM decoder's mask blended over the frame and the click squares
    (overlay_mask, overlay_point, utils.py:46-52, :97-105, :1396-1399);
  * test_gui's nearest resize back to the window size (utils.py:1698-1702);
  * NeRFGUI.prepare_buffer and the running mean over spp frames
    (nerf/gui.py:134-140, :171-177).

`present_frame` is samnerf_present_frame (csrc/present.hip) for CUDA tensors:
one launch for an image buffer at the render's size, two for a resized one or
a depth buffer, nothing on the host.  `torch_present_frame` is the reference's
own op sequence restated op for op -- torch for the test_step / test_gui part,
numpy on the host for prepare_buffer and the spp mean -- which is what a CPU
tensor gets and what the tests compare the kernels with.  `test_step` and
`render_frame` are Trainer.test_step and Trainer.test_gui + prepare_buffer on
a model of this package.

The reference's quirks are kept: overlay_mask_composition with a render id
shows image * 0.7 + image * 0.3 (not image) off the instance; overlay_mask
blends every pixel, not only the masked ones; overlay_point's slices follow
Python's rules, so a click within 2 pixels of the top or left edge draws
nothing (the negative start wraps round).  One thing is mended: with a render
id overlay_mask_only indexes its [H, W, 3] image with the flattened [H * W]
mask and raises; here the mask keeps its [H, W] shape, which is what the two
lines say.
"""
import ctypes

import numpy as np
import torch
import torch.nn.functional as F

from .ops import _o, _ptr, _stream, torch_mask_probs

MASK_TYPES = ("heatmap", "composition", "mask")
MODES = ("image", "depth")
MAX_POINTS = 64
_color_map = None


def default_color_map(device=None):
    """The reference's colour table (utils.py:606-610), float32 [100, 3]:
    gist_ncar resampled to 100 entries, read at (7 i + 5) % 100.  Built on
    first use with matplotlib (plt.cm.get_cmap is gone from matplotlib 3.9;
    matplotlib.colormaps[...].resampled is its successor); pass color_map=
    explicitly where matplotlib is not installed."""
    global _color_map
    if _color_map is None:
        try:
            import matplotlib
        except ImportError as e:
            raise RuntimeError("default_color_map: the reference's colour table is matplotlib's gist_ncar; "
                               "matplotlib is not installed, so pass color_map= (float32 [n, 3]) explicitly") from e
        cmap = matplotlib.colormaps["gist_ncar"].resampled(100)
        table = np.multiply([cmap((i * 7 + 5) % 100)[:3] for i in range(100)], 1)
        _color_map = torch.from_numpy(table).to(torch.float)
    return _color_map if device is None else _color_map.to(device)


# ------------------------------------------------------------- torch mirror --
# utils.py:46-105, restated

def overlay_mask(image, mask, alpha=0.7, color=(1, 0, 0)):
    over_image = image.clone()
    over_image[mask] = torch.tensor(list(color), device=image.device, dtype=image.dtype)
    return image * alpha + over_image * (1 - alpha)


def overlay_mask_only(instance_id, color_map=None, render_id=-1):
    H, W = instance_id.shape
    instance_id = instance_id.reshape(H * W)
    if render_id == -1:
        return color_map[instance_id].reshape(H, W, -1)
    mask = instance_id == render_id
    color_mask = torch.zeros([H, W, 3], device=instance_id.device)
    color_mask[mask.reshape(H, W)] = color_map[render_id]
    return color_mask


def overlay_mask_composition(image, instance_id, color_map=None, render_id=-1, alpha=0.7):
    H, W = instance_id.shape
    color_mask = color_map[instance_id.reshape(H * W)].reshape(H, W, -1)
    if render_id != -1:
        mask = instance_id != render_id
        color_mask[mask] = image[mask]
    return image * alpha + color_mask * (1 - alpha)


def overlay_mask_heatmap(mask, instance_id, color_map=None):
    if isinstance(instance_id, int):
        instance_id = (torch.ones_like(mask) * instance_id).to(color_map.device).to(torch.long)
    H, W = instance_id.shape
    color_mask = color_map[instance_id.reshape(H * W)].reshape(H, W, -1)
    return color_mask * mask[..., None]


def overlay_point(image, points, radius=2, color=(0, 1, 0)):
    mask = torch.zeros_like(image[:, :, 0]).bool()
    for point in points:
        x, y = int(point[0]), int(point[1])
        mask[y - radius:y + radius, x - radius:x + radius] = True
    image[mask] = torch.tensor(list(color), device=image.device, dtype=image.dtype)
    return image


def _shapes(image, depth, logits, n_inst):
    ref = depth if depth is not None else image
    if ref is None or ref.dim() < 2:
        raise ValueError("present_frame: image [rH, rW, 3] or depth [rH, rW] gives the render's size")
    rH, rW = int(ref.shape[0]), int(ref.shape[1])
    K = 0
    if logits is not None:
        K = int(logits.shape[-1])
        if logits.numel() != rH * rW * K:
            raise ValueError(f"present_frame: logits of {tuple(logits.shape)} on a {rH} x {rW} render")
        if n_inst is None:
            raise ValueError("present_frame: logits need n_inst (opt.n_inst; K = n_inst + redundant_instance)")
        if not 1 <= int(n_inst) <= K:
            raise ValueError(f"present_frame: n_inst = {n_inst} outside [1, K = {K}]")
    return rH, rW, K


def _check_modes(mask_type, mode):
    if mask_type not in MASK_TYPES:
        raise ValueError(f"present_frame: mask_type {mask_type!r}, one of {MASK_TYPES}")
    if mode not in MODES:
        raise ValueError(f"present_frame: mode {mode!r}, one of {MODES}")


def torch_present_frame(image, depth, H, W, *, logits=None, n_inst=None, mask_type="heatmap", instance_id=0,
                        color_map=None, sam_mask=None, points=None, mode="image", buffer=None, spp=0,
                        return_extra=False):
    """present_frame in the reference's own ops, on any device: torch for
    utils.py:1263-1306, :1396-1399 and :1698-1702 on the tensors' device, then
    numpy on the host for gui.py:134-140 and :176, as the reference does.
    Returns the buffer [H, W, 3] on the inputs' device (a new tensor; `buffer`
    is not written)."""
    _check_modes(mask_type, mode)
    rH, rW, K = _shapes(image, depth, logits, n_inst)
    pred_rgb, pred_depth, pred_mask, ids = image, depth, None, None
    if logits is not None:
        if color_map is None:
            color_map = default_color_map(logits.device)
        inst_mask = logits.reshape(rH, rW, K)
        pred_mask = torch_mask_probs(inst_mask, n_inst)
        ids = pred_mask.argmax(-1)
        in_range = instance_id >= 0 and instance_id < n_inst
        if mask_type == "heatmap":
            if in_range:
                instance_mask, instance = pred_mask[..., instance_id], int(instance_id)
            else:
                instance_mask, _ = torch.max(pred_mask, -1)
                instance = pred_mask.argmax(-1)
            pred_rgb = overlay_mask_heatmap(instance_mask, instance, color_map=color_map)
        elif mask_type == "composition":
            pred_rgb = overlay_mask_composition(pred_rgb, pred_mask.argmax(-1), color_map=color_map,
                                                render_id=instance_id if in_range else -1)
        else:
            pred_rgb = overlay_mask_only(pred_mask.argmax(-1), color_map=color_map,
                                         render_id=instance_id if in_range else -1)
    if sam_mask is not None:
        pred_rgb = overlay_mask(pred_rgb, sam_mask.reshape(rH, rW).bool())
    if points is not None and len(points):
        pts = points.detach().cpu().numpy() if torch.is_tensor(points) else np.asarray(points)
        pred_rgb = overlay_point(pred_rgb.clone(), pts)
    preds, preds_depth = pred_rgb, pred_depth
    if (rH, rW) != (H, W):
        if preds is not None:
            preds = F.interpolate(preds.unsqueeze(0).permute(0, 3, 1, 2), size=(H, W),
                                  mode="nearest").permute(0, 2, 3, 1).squeeze(0).contiguous()
        if preds_depth is not None:
            preds_depth = F.interpolate(preds_depth.unsqueeze(0).unsqueeze(1), size=(H, W),
                                        mode="nearest").squeeze(0).squeeze(0)
    if mode == "image":
        new = preds.detach().cpu().numpy().astype(np.float32)
    else:
        d = preds_depth.detach().cpu().numpy().astype(np.float32)
        d = (d - d.min()) / (d.max() - d.min() + 1e-6)
        new = np.expand_dims(d, -1).repeat(3, -1)
    if spp:
        spp = int(spp)
        new = (buffer.detach().cpu().numpy().reshape(H, W, 3) * spp + new) / (spp + 1)
    dev = (image if image is not None else depth).device
    out = torch.from_numpy(np.ascontiguousarray(new)).to(dev)
    if return_extra:
        return out, {"probs": pred_mask, "ids": ids, "depth": preds_depth}
    return out


# ------------------------------------------------------------------ kernels --

def _hip_present_frame(image, depth, H, W, logits, n_inst, mask_type, instance_id, color_map, sam_mask, points,
                       mode, buffer, spp, return_extra):
    from ._lib import SamnerfPresentArgs, check, lib
    rH, rW, K = _shapes(image, depth, logits, n_inst)
    dev = (image if image is not None else depth).device
    keep = []

    def dev_tensor(t, dtype, numel, what):
        if t is None:
            return None
        t = torch.as_tensor(t).detach().to(device=dev, dtype=dtype).reshape(-1).contiguous()
        if numel is not None and t.numel() != numel:
            raise ValueError(f"present_frame: {what} holds {t.numel()} values, not {numel}")
        keep.append(t)
        return t.data_ptr()

    a = SamnerfPresentArgs()
    a.rH, a.rW, a.H, a.W, a.K = rH, rW, int(H), int(W), K
    a.mask_type, a.mode = MASK_TYPES.index(mask_type), MODES.index(mode)
    a.instance_id = max(min(int(instance_id), 2 ** 31 - 1), -1)
    a.spp = int(spp)
    a.image = dev_tensor(image, torch.float32, rH * rW * 3, "image")
    a.depth = dev_tensor(depth, torch.float32, rH * rW, "depth")
    extra = {"probs": None, "ids": None, "depth": None}
    if logits is not None:
        if color_map is None:
            color_map = default_color_map(dev)
        a.n_inst = int(n_inst)
        a.n_colors = int(color_map.shape[0])
        a.logits = dev_tensor(logits, torch.float32, rH * rW * K, "logits")
        a.color_map = dev_tensor(color_map, torch.float32, a.n_colors * 3, "color_map")
        if return_extra:
            extra["probs"] = torch.empty(rH, rW, K, device=dev)
            extra["ids"] = torch.empty(rH, rW, dtype=torch.int64, device=dev)
            a.probs, a.ids = extra["probs"].data_ptr(), extra["ids"].data_ptr()
    if sam_mask is not None:
        a.sam_mask = dev_tensor(torch.as_tensor(sam_mask) != 0, torch.uint8, rH * rW, "sam_mask")
    if points is not None and len(points):
        pts = torch.as_tensor(np.asarray(points.detach().cpu()) if torch.is_tensor(points) else np.asarray(points))
        if pts.dim() != 2 or pts.shape[1] != 2:
            raise ValueError("present_frame: points must be [P, 2] as (x, y)")
        a.n_points = int(pts.shape[0])
        a.points = dev_tensor(pts, torch.int32, None, "points")
    if return_extra and depth is not None:
        extra["depth"] = torch.empty(int(H), int(W), device=dev)
        a.depth_out = extra["depth"].data_ptr()
    if buffer is None:
        if spp:
            raise ValueError("present_frame: spp > 0 blends into buffer, which is missing")
        buffer = torch.empty(int(H), int(W), 3, device=dev)
    elif not (buffer.is_cuda and buffer.dtype == torch.float32 and buffer.is_contiguous()
              and buffer.numel() == int(H) * int(W) * 3):
        raise ValueError("present_frame: buffer must be a contiguous fp32 CUDA tensor [H, W, 3] (written in place)")
    a.buffer = buffer.data_ptr()
    need = lib().samnerf_present_workspace_size(ctypes.byref(a))
    ws = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
    check(lib().samnerf_present_frame(ctypes.byref(a), _ptr(ws), need, _stream(buffer)), "present_frame")
    out = buffer.view(int(H), int(W), 3)
    return (out, extra) if return_extra else out


def present_frame(image, depth, H, W, *, logits=None, n_inst=None, mask_type="heatmap", instance_id=0,
                  color_map=None, sam_mask=None, points=None, mode="image", buffer=None, spp=0,
                  return_extra=False):
    """The display buffer [H, W, 3] of one rendered frame.

    image [rH, rW, 3], depth [rH, rW]: the render's outputs (either may be None
    where the view does not read it).  logits [rH, rW, K] with n_inst
    (K = n_inst + redundant_instance <= 32): the mask view `mask_type`
    ('heatmap', 'composition', 'mask') of instance `instance_id`
    (opt.render_mask_instance_id; outside [0, n_inst): every instance by its
    argmax) in the colours of color_map [n >= K, 3] (default_color_map()).
    sam_mask [rH, rW]: the decoder's mask, blended in red; points [P <= 64, 2]
    (x, y): the click squares.  mode 'image' shows the frame, 'depth' the depth
    normalised by its min and max.  spp = 0 writes the buffer (a new one unless
    `buffer` is given); spp > 0 updates `buffer` in place to the mean over
    spp + 1 frames.  return_extra adds {'probs' [rH, rW, K], 'ids' [rH, rW],
    'depth' [H, W]}.

    CUDA tensors go to the HIP kernels, anything else to torch_present_frame."""
    _check_modes(mask_type, mode)
    ref = image if image is not None else depth
    if ref is not None and ref.is_cuda:
        return _hip_present_frame(image, depth, H, W, logits, n_inst, mask_type, instance_id, color_map,
                                  sam_mask, points, mode, buffer, spp, return_extra)
    return torch_present_frame(image, depth, H, W, logits=logits, n_inst=n_inst, mask_type=mask_type,
                               instance_id=instance_id, color_map=color_map, sam_mask=sam_mask, points=points,
                               mode=mode, buffer=buffer, spp=spp, return_extra=return_extra)


# ------------------------------------------------------- test_step, test_gui --

def _mask_kwargs(opt, outputs, color_map):
    if not _o(opt, "with_mask", False):
        return {}
    return dict(logits=outputs["instance_mask_logits"], n_inst=int(opt.n_inst),
                mask_type=_o(opt, "render_mask_type", "heatmap"),
                instance_id=int(_o(opt, "render_mask_instance_id", -1)), color_map=color_map)


def test_step(model, data, opt, bg_color=None, perturb=False, color_map=None, sam=None):
    """Trainer.test_step (utils.py:1243-1407) for RGB and --with_mask models:
    render data['rays_o'], data['rays_d'] as a data['H'] x data['W'] frame and
    present it at that size.  sam: (mask [H, W], points [P, 2]) of a decoder run
    on this view, overlaid as utils.py:1396-1399 (the decoder itself:
    sam_bridge).  Returns (pred_rgb [H, W, 3], pred_depth [H, W]), and pred_mask
    [H, W, K] as well under opt.return_extra with opt.with_mask."""
    if _o(opt, "with_sam", False):
        raise NotImplementedError("present.test_step: a --with_sam model's feature render and decoder are "
                                  "sam_bridge.render_and_predict's (pass present=)")
    H, W = int(data["H"]), int(data["W"])
    cnf = data["cam_near_far"] if "cam_near_far" in data else None
    with_mask = bool(_o(opt, "with_mask", False))
    outputs = model.render(data["rays_o"], data["rays_d"], staged=True, bg_color=bg_color, perturb=perturb,
                           cam_near_far=cnf, return_feats=False, return_mask=with_mask)
    pred_rgb = outputs["image"].reshape(H, W, 3)
    pred_depth = outputs["depth"].reshape(H, W)
    kw = _mask_kwargs(opt, outputs, color_map)
    if sam is not None:
        kw.update(sam_mask=sam[0], points=sam[1])
    frame, extra = present_frame(pred_rgb, pred_depth, H, W, return_extra=True, **kw)
    if _o(opt, "return_extra", False) and with_mask:
        return frame, pred_depth, extra["probs"]
    return frame, pred_depth


def render_frame(model, opt, pose, intrinsics, W, H, bg_color=None, spp=1, downscale=1, mode="image",
                 buffer=None, color_map=None, sam=None):
    """Trainer.test_gui (utils.py:1647-1712) and NeRFGUI.prepare_buffer with the
    spp mean (gui.py:134-140, :171-177): render the view at
    int(H * downscale) x int(W * downscale) and present it at H x W.  As in the
    GUI, spp is the perturbation's switch (off at 1) and the count of frames
    already in `buffer`; buffer=None starts a new one (need_update).  Returns
    the device buffer [H, W, 3]; the one host copy into the GUI's texture is the
    caller's."""
    from . import ops
    rH, rW = int(H * downscale), int(W * downscale)
    intr = np.asarray(intrinsics, np.float32) * downscale
    dev = next(model.parameters()).device
    ro, rd = ops.get_rays(pose, intr, rH, rW, device=dev)
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            outputs = model.render(ro, rd, staged=True, bg_color=bg_color, perturb=False if spp == 1 else spp,
                                   return_feats=False, return_mask=bool(_o(opt, "with_mask", False)))
    finally:
        model.train(was_training)
    kw = _mask_kwargs(opt, outputs, color_map)
    if sam is not None:
        kw.update(sam_mask=sam[0], points=sam[1])
    return present_frame(outputs["image"].reshape(rH, rW, 3), outputs["depth"].reshape(rH, rW), H, W, mode=mode,
                         buffer=buffer, spp=int(spp) if buffer is not None else 0, **kw)
