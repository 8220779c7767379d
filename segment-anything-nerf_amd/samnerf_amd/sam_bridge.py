"""Hand-off of rendered SAM features to a SAM mask decoder.

`Trainer.sam_predict` (nerf/utils.py:1409-1475) feeds the 256-d feature map
rendered by the NeRF (here: the fused HIP path's `samvit`, already in device
memory) to segment-anything's `SamPredictor` in place of the ViT image
embedding: resize to a 64-long side, zero-pad to 64 x 64, set the
predictor's image state, scale the click to the 1024-long input frame, and
decode one mask.  The decoder itself is a third-party model absent from this
image (segment_anything_hq, requirements.txt:25); `sam_predict` drives any
object with SamPredictor's interface (reset_image, original_size, input_size,
features, is_image_set, interm_features, predict_torch), so a ROCm build of
SAM plugs in unchanged.  Nothing leaves the device: the features stay the
render's tensor, resized and padded on the GPU.

`sam_predict_device` is the same hand-off to the project's own decoder
(sam_decoder.SamDecoder: SAM's prompt encoder and mask decoder for point
prompts as HIP kernels), which also serves `sam_predict` through
sam_decoder.DevicePredictor.
"""
import numpy as np
import torch
import torch.nn.functional as F


def input_size_for(H, W):
    """The predictor's input frame (utils.py:1415-1416): longest side 1024."""
    r = 1024 / W if W > H else 1024 / H
    return (int(H * r), int(W * r)), r


def prepare_sam_features(features):
    """features [1,256,h,w] (or a rendered samvit [h,w,256]) -> [1,256,64,64]:
    bilinear resize of the longest side to 64 (align_corners=False), then
    zero padding right / bottom (utils.py:1426-1431)."""
    if features.dim() == 3:
        features = features.permute(2, 0, 1).unsqueeze(0)
    h, w = features.shape[2:]
    r = 64 / w if w > h else 64 / h
    features = F.interpolate(features, (int(h * r), int(w * r)), mode="bilinear",
                             align_corners=False)
    return F.pad(features, (0, 64 - features.shape[3], 0, 64 - features.shape[2]),
                 mode="constant", value=0)


def click_coords(H, W, point_coords=None, rng=None):
    """Point prompt in the 1024 frame (utils.py:1435-1446): the given pixel
    clicks scaled by the resize ratio, or one random point away from the 20%
    border (np.random, as the reference, unless `rng` is given)."""
    input_size, r = input_size_for(H, W)
    if point_coords is None:
        rng = np.random if rng is None else rng
        bh, bw = int(input_size[0] * 0.2), int(input_size[1] * 0.2)
        # the reference draws x from the height range and y from the width range
        return np.array([[rng.randint(0 + bh, input_size[1] - bh),
                          rng.randint(0 + bw, input_size[0] - bw)]]), r
    return (np.asarray(point_coords).astype(np.float32) * r).astype(np.int32), r


def sam_predict(predictor, H, W, features, point_coords=None, mask_input=None, device=None,
                rng=None):
    """Trainer.sam_predict with rendered features (image=None branch).
    Returns (masks[0] [H, W], original_point_coords [N, 2], low_res_masks[0])."""
    device = device if device is not None else features.device
    input_size, r = input_size_for(H, W)
    predictor.reset_image()
    predictor.original_size = (H, W)
    predictor.input_size = input_size
    predictor.features = prepare_sam_features(features)
    predictor.is_image_set = True
    pts, _ = click_coords(H, W, point_coords, rng)
    mask_t = None
    if mask_input is not None:
        mask_t = torch.as_tensor(mask_input, dtype=torch.float, device=device)[None, :, :, :]
    labels = np.ones_like(pts[:, 0])
    coords_t = torch.as_tensor(pts, dtype=torch.float, device=device)[None, :, :]
    labels_t = torch.as_tensor(labels, dtype=torch.int, device=device)[None, :]
    predictor.interm_features = None
    masks, _iou, low_res = predictor.predict_torch(coords_t, labels_t, mask_input=mask_t,
                                                   multimask_output=False)
    original = (pts / r).astype(np.int32)
    return masks[0], original, low_res[0]


def sam_predict_device(decoder, H, W, samvit_hwc, point_coords=None, rng=None):
    """sam_predict on a sam_decoder.SamDecoder with the rendered map as it is:
    samvit_hwc [h, w, 256] (the render's samvit viewed as rows of the h x w
    view) goes to the decoder's first kernel, which resizes its long side to
    the token grid and pads it -- no F.interpolate, no permute, and no host
    copy but the click coordinates.  Same return as sam_predict."""
    S = decoder.S
    r = S / W if W > H else S / H
    input_size = (int(H * r), int(W * r))
    if point_coords is None:
        if S != 1024:
            raise ValueError("sam_predict_device: a random click is drawn in the 1024 frame (g = 64)")
        pts, _ = click_coords(H, W, None, rng)
    else:
        pts = (np.asarray(point_coords).astype(np.float32) * r).astype(np.int32)
    low_res, _iou = decoder.decode(samvit_hwc.contiguous(), pts)
    masks = decoder.masks(low_res[:1], input_size, (H, W))
    return masks, (pts / r).astype(np.int32), low_res[:1]


def segment_everything(decoder_or_generator, H, W, samvit_hwc, **kw):
    """SAM's automatic mask generator on a rendered view (debug.py's
    Auto_Generator with `feature=`, batch_generate_mask.py's per-view masks):
    samvit_hwc [h, w, 256] goes to the decoder as it is, like
    sam_predict_device.  A sam_decoder.SamDecoder is wrapped in a
    sam_generator.DeviceMaskGenerator built from the generator's keywords
    (points_per_side, pred_iou_thresh, ...); `multimask_output` and
    `as_tensors` go to generate()."""
    from .sam_generator import DeviceMaskGenerator
    call = {k: kw.pop(k) for k in ("multimask_output", "as_tensors") if k in kw}
    gen = decoder_or_generator
    if not isinstance(gen, DeviceMaskGenerator):
        gen = DeviceMaskGenerator(gen, **kw)
    elif kw:
        raise TypeError(f"segment_everything: {sorted(kw)} belong to the generator's constructor")
    return gen.generate(samvit_hwc.contiguous(), H, W, **call)


class PromptMemory:
    """The remembered 3D prompt points of Trainer.test_step (utils.py:1318-1384),
    which make a click follow its object across views: a click is lifted to 3D
    by the rendered depth; a new point is added, or takes out the remembered
    points within `dist_thresh` of it; the remembered points are projected into
    each view and kept where they are on screen and not occluded.  Plain torch
    ops on a handful of points, on the tensors' device."""
    dist_thresh = 0.01
    depth_thresh = 0.05

    def __init__(self):
        self.point_3d = None

    def update(self, point_coords, rays_o, rays_d, depth):
        """utils.py:1318-1345.  point_coords [P, 2] (x, y) integer pixels of the
        H x W view; rays_o, rays_d [H*W, 3]; depth [H, W]."""
        H, W = depth.shape
        pc = torch.as_tensor(np.asarray(point_coords), dtype=torch.long, device=depth.device)
        rays_o, rays_d = rays_o.view(H, W, 3), rays_d.view(H, W, 3)
        point_depth = depth[pc[:, 1], pc[:, 0]]
        point_3d = rays_o[pc[:, 1], pc[:, 0]] + rays_d[pc[:, 1], pc[:, 0]] * point_depth.unsqueeze(-1)
        if self.point_3d is None:
            self.point_3d = point_3d
            return
        dist = (self.point_3d - point_3d).norm(dim=-1)
        if dist.min() > self.dist_thresh:
            self.point_3d = torch.cat([self.point_3d, point_3d], dim=0)
        else:
            keep_mask = dist > self.dist_thresh
            self.point_3d = self.point_3d[keep_mask] if keep_mask.any() else None

    def camera_points(self, pose):
        """The remembered points in the camera frame of `pose` [4, 4]: [N, 4]."""
        point_3d = torch.cat([self.point_3d, torch.ones_like(self.point_3d[:, :1])], axis=-1)
        w2c = torch.inverse(torch.as_tensor(pose, dtype=point_3d.dtype, device=point_3d.device).view(4, 4))
        return point_3d @ w2c.T

    def project(self, pose, intrinsics, depth):
        """utils.py:1349-1384: the remembered points as integer pixels (x, y) of
        the view (pose [4, 4], intrinsics (fx, fy, cx, cy), its rendered depth
        [H, W]), int64 numpy [M, 2], or None where none is on screen and
        unoccluded."""
        if self.point_3d is None:
            return None
        H, W = depth.shape
        point_3d_cam = self.camera_points(pose)
        fx, fy, cx, cy = [torch.as_tensor(intrinsics, dtype=point_3d_cam.dtype, device=point_3d_cam.device)
                          .reshape(4)[i] for i in range(4)]
        coords = torch.stack([
            W - (fx * point_3d_cam[:, 0] / point_3d_cam[:, 2] + cx),
            fy * point_3d_cam[:, 1] / point_3d_cam[:, 2] + cy,
        ], dim=-1).long()
        screen_mask = (coords[:, 0] >= 0) & (coords[:, 0] < W) & (coords[:, 1] >= 0) & (coords[:, 1] < H)
        if not screen_mask.any():
            return None
        coords = coords[screen_mask]
        point_depth = - point_3d_cam[screen_mask, 2]
        observed_depth = depth[coords[:, 1], coords[:, 0]]
        unoccluded_mask = (point_depth - observed_depth).abs() <= self.depth_thresh
        if not unoccluded_mask.any():
            return None
        return coords[unoccluded_mask].detach().cpu().numpy()


def render_and_predict(renderer, predictor, rays_o_lr, rays_d_lr, h, w, H, W, point_coords=None,
                       memory=None, present=None, **kw):
    """The interactive loop of the GUI (nerf/gui.py:143-161, utils.py:1647-1712)
    on the fused path: render the h x w feature rays, hand the feature map to
    the decoder without a host copy.

    present: the H x W view to show the result on, a dict with 'image'
    [H, W, 3] and 'depth' [H, W] and, for `memory` (a PromptMemory), 'rays_o',
    'rays_d' [H*W, 3], 'pose' [4, 4], 'intrinsics' [4]; other keys go to
    present.present_frame (mode, buffer, spp, ...).  With memory the click
    updates the remembered points and the decoder is prompted with their
    projection into this view (utils.py:1318-1394), or not run where none is
    visible.  Returns (prediction or None, out, frame): the frame with the
    decoder's mask and the click squares over it (utils.py:1396-1399).  Without
    memory and present the result is (prediction, out), as before."""
    out = renderer.render(rays_o_lr, rays_d_lr)
    feats = out["samvit"].view(h, w, 256)
    if memory is None and present is None:
        return sam_predict(predictor, H, W, feats, point_coords=point_coords, **kw), out
    from .present import present_frame
    view = dict(present or {})
    geometry = {k: view.pop(k, None) for k in ("rays_o", "rays_d", "pose", "intrinsics")}
    image, depth = view.pop("image", None), view.pop("depth", None)
    if memory is not None:
        if depth is None or any(v is None for v in geometry.values()):
            raise ValueError("render_and_predict: memory= needs present= with depth, rays_o, rays_d, pose, intrinsics")
        if point_coords is not None:
            memory.update(point_coords, geometry["rays_o"], geometry["rays_d"], depth)
        point_coords = memory.project(geometry["pose"], geometry["intrinsics"], depth)
    pred = None
    if point_coords is not None:
        pred = sam_predict(predictor, H, W, feats, point_coords=point_coords, **kw)
    if present is None:
        return pred, out, None
    if pred is not None:
        view.update(sam_mask=pred[0][0], points=pred[1])      # masks [N, H, W]: the first, as utils.py:1396
    return pred, out, present_frame(image, depth, H, W, **view)
