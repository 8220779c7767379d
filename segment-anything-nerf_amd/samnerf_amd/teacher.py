"""The SAM teacher's side of the distillation step, from a render that is
already on the device: everything between the full-resolution render and
`image_encoder(...)`, and the feature cache around it.

The reference (nerf/utils.py:1083-1087, :1205-1208) copies the render to the
host, quantises it with numpy and calls `SamPredictor.set_image`, whose own
preprocessing is a PIL bilinear resize of the uint8 image on the host, an
upload, and only then the normalise and pad on the GPU.  `teacher_image` is
that sequence as three launches (samnerf_teacher_image,
csrc/teacher_image.hip), bit for bit: the same uint8 image PIL returns, the
same fp32 planes `Sam.preprocess` returns.  `set_image_from_render` is
`SamPredictor.set_image` on top of it, `FeatureCache` / `use_cache_now` the
reference's Cache and its policy (utils.py:515-531, :875-878); the step that
ties them together is `train.sam_distill_step`.

The ViT and its weights stay out: `set_image_from_render` drives any object
with SamPredictor's interface (reset_image, original_size, input_size,
features, is_image_set, model.image_encoder), the stance of
`sam_bridge.sam_predict`.  `torch_teacher_image` is the reference's own
sequence spelled out (host round trip, PIL, torch ops): the mirror the tests
compare the kernels with, and the timing baseline.
"""
import ctypes
import random

import numpy as np
import torch
import torch.nn.functional as F

from .ops import _ptr, _stream

PIXEL_MEAN = (123.675, 116.28, 103.53)        # Sam's registered buffers
PIXEL_STD = (58.395, 57.12, 57.375)
MAX_SIDE = 8192

_workspaces = {}


def preprocess_shape(H, W, target=1024):
    """ResizeLongestSide.get_preprocess_shape: (oh, ow) with the longest side
    at `target` (Python floats: the C doubles of samnerf_teacher_image_shape)."""
    scale = target * 1.0 / max(H, W)
    return int(H * scale + 0.5), int(W * scale + 0.5)


def _sizes(pred_rgb, target, size):
    if pred_rgb.dim() != 3 or pred_rgb.shape[2] != 3:
        raise ValueError(f"teacher_image: pred_rgb must be [H, W, 3], not {tuple(pred_rgb.shape)}")
    H, W = int(pred_rgb.shape[0]), int(pred_rgb.shape[1])
    oh, ow = preprocess_shape(H, W, int(target))
    S = int(target) if size is None else int(size)
    if not all(1 <= n <= MAX_SIDE for n in (H, W, oh, ow, S)):
        raise ValueError(f"teacher_image: sizes {H} x {W} -> {oh} x {ow} in {S} x {S} must lie in [1, {MAX_SIDE}]")
    if S < max(oh, ow):
        raise ValueError(f"teacher_image: size = {S} is below the resized image's {oh} x {ow}")
    return H, W, oh, ow, S


def _want(want):
    want = (want,) if isinstance(want, str) else tuple(want)
    if not want or any(k not in ("u8", "input") for k in want):
        raise ValueError(f"teacher_image: want = {want!r}: 'u8' and / or 'input'")
    return want


def torch_teacher_image(pred_rgb, target=1024, size=None, pixel_mean=PIXEL_MEAN, pixel_std=PIXEL_STD,
                        want=("u8", "input")):
    """The reference's sequence on any tensor: `.cpu().numpy() * 255 ->
    astype(uint8)` (utils.py:1083-1084), ResizeLongestSide.apply_image (PIL's
    bilinear resize), the upload to pred_rgb's device, and Sam.preprocess in
    torch ops.  Same result dict as teacher_image."""
    try:
        from PIL import Image
    except ImportError as e:
        raise RuntimeError("torch_teacher_image: the reference's resize is PIL's (Image.resize, BILINEAR) and PIL "
                           "is not installed; the HIP path (teacher_image on a CUDA tensor) does not need it") from e
    want = _want(want)
    H, W, oh, ow, S = _sizes(pred_rgb, target, size)
    dev = pred_rgb.device
    image = (pred_rgb.detach().cpu().numpy() * 255).astype(np.uint8)
    resized = np.array(Image.fromarray(image).resize((ow, oh), Image.BILINEAR))
    u8 = torch.as_tensor(resized, device=dev)
    out = {"input_size": (oh, ow)}
    if "u8" in want:
        out["u8"] = u8
    if "input" in want:
        x = u8.permute(2, 0, 1).contiguous()[None, :, :, :]
        mean = torch.tensor(pixel_mean, dtype=torch.float32, device=dev).view(-1, 1, 1)
        std = torch.tensor(pixel_std, dtype=torch.float32, device=dev).view(-1, 1, 1)
        x = (x - mean) / std
        out["input"] = F.pad(x, (0, S - ow, 0, S - oh))
    return out


def teacher_image(pred_rgb, target=1024, size=None, pixel_mean=PIXEL_MEAN, pixel_std=PIXEL_STD,
                  want=("u8", "input")):
    """pred_rgb [H, W, 3] in [0, 1] -> {'u8': uint8 [oh, ow, 3] (what
    ResizeLongestSide.apply_image returns, for a predictor whose
    set_torch_image runs its own preprocess), 'input': fp32 [1, 3, S, S] (what
    Sam.preprocess returns, for image_encoder), 'input_size': (oh, ow)}, the
    tensors on pred_rgb's device.  target: the longest side after the resize;
    size: S, the padded plane's side (default: target).  pixel_mean /
    pixel_std: three Python floats each.  want: which of the two to produce.

    A contiguous fp32 CUDA tensor goes to the kernels on torch's current
    stream, with nothing read back; anything else runs torch_teacher_image."""
    if not (pred_rgb.is_cuda and pred_rgb.dtype == torch.float32 and pred_rgb.is_contiguous()):
        return torch_teacher_image(pred_rgb, target, size, pixel_mean, pixel_std, want)
    from ._lib import check, lib
    want = _want(want)
    H, W, oh, ow, S = _sizes(pred_rgb, target, size)
    dev = pred_rgb.device
    stream = _stream(pred_rgb)
    need = lib().samnerf_teacher_image_workspace_size(H, W, oh, ow)
    key = (dev, stream.value, H, W, oh, ow)
    ws = _workspaces.get(key)
    if ws is None:
        if len(_workspaces) >= 16:                 # a handful of view sizes in practice
            _workspaces.clear()
        ws = _workspaces[key] = torch.empty(need, dtype=torch.uint8, device=dev)
    u8 = torch.empty(oh, ow, 3, dtype=torch.uint8, device=dev) if "u8" in want else None
    inp = torch.empty(1, 3, S, S, dtype=torch.float32, device=dev) if "input" in want else None
    mean = (ctypes.c_float * 3)(*[float(v) for v in pixel_mean])
    std = (ctypes.c_float * 3)(*[float(v) for v in pixel_std])
    check(lib().samnerf_teacher_image(_ptr(pred_rgb.detach()), H, W, oh, ow, S, mean, std, _ptr(u8), _ptr(inp),
                                      _ptr(ws), need, stream), "teacher_image")
    out = {"input_size": (oh, ow)}
    if u8 is not None:
        out["u8"] = u8
    if inp is not None:
        out["input"] = inp
    return out


def _pixel_stats(predictor):
    """(mean, std) of a predictor as Python floats: its model's pixel_mean /
    pixel_std buffers where it has them, read once and kept on it (they live
    on the device, and a read per step would be a host synchronisation per
    step), SAM's values otherwise."""
    kept = getattr(predictor, "_samnerf_pixel_stats", None)
    if kept is not None:
        return kept
    model = getattr(predictor, "model", None)
    mean, std = getattr(model, "pixel_mean", None), getattr(model, "pixel_std", None)
    mean = PIXEL_MEAN if mean is None else tuple(torch.as_tensor(mean).reshape(-1).tolist())
    std = PIXEL_STD if std is None else tuple(torch.as_tensor(std).reshape(-1).tolist())
    try:
        predictor._samnerf_pixel_stats = (mean, std)
    except AttributeError:
        pass
    return mean, std


def set_image_from_render(predictor, pred_rgb):
    """SamPredictor.set_image for a render [H, W, 3] in [0, 1] that is already
    on the device: the image state is set as set_torch_image sets it and the
    encoder runs on teacher_image's input tensor.  Returns predictor.features.
    An encoder that returns a tuple (HQ-SAM) also sets interm_features."""
    mean, std = _pixel_stats(predictor)
    t = teacher_image(pred_rgb, pixel_mean=mean, pixel_std=std, want=("input",))
    predictor.reset_image()
    predictor.original_size = (int(pred_rgb.shape[0]), int(pred_rgb.shape[1]))
    predictor.input_size = tuple(t["input_size"])
    out = predictor.model.image_encoder(t["input"])
    if isinstance(out, tuple):
        predictor.features, predictor.interm_features = out
    else:
        predictor.features = out
    predictor.is_image_set = True
    return predictor.features


class FeatureCache:
    """The reference's Cache (utils.py:515-531): a ring of `size` training
    batches with their teacher features; get() draws one with Python's random."""

    def __init__(self, size=100):
        self.size = size
        self.data = {}
        self.key = 0

    def full(self):
        return len(self.data) == self.size

    def insert(self, x):
        self.data[self.key] = x
        self.key = (self.key + 1) % self.size

    def get(self, key=None):
        if key is None:
            key = random.randint(0, len(self.data) - 1)
        return self.data[key]


def use_cache_now(opt, cache, global_step):
    """utils.py:875-878: a cached batch stands in for the loader's once the
    cache is full, except on every cache_interval-th step."""
    return bool(opt.with_sam and opt.cache_size > 0 and cache is not None and cache.full()
                and global_step % opt.cache_interval != 0)
