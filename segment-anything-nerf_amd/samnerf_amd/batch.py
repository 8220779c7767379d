"""A training step's input: the reference's ray selection and collate.

`TrainBatchSampler(source, opt).sample(global_step, index)` returns the dict the
reference's dataset collate returns for the training branches without SAM
(nerf/colmap_provider.py:935-1204, `training and not with_sam`), which is what
`rgb_train_step_fused` and `mask_train_step_full` consume.  It restates

  * the host decisions of colmap_provider.py:966-1044 and :1047-1070 -- when
    random_image_batch switches on, random_sample, which map feeds which mode,
    the patch size only under with_mask, the fixed-fov intrinsics of with_mask
    without default intrinsics;
  * the N > 0 branches of get_rays (nerf/utils.py:174-242), by mode:
      R  uniform pixels over random images (utils.py:234-236),
      P  random patches (utils.py:196-219),
      C  a patch centred on a draw from the error map or the incoherent mask
         (utils.py:180-194; the local draws of mixed sampling),
      E  error-map-weighted pixels without replacement (utils.py:222-233);
  * the gathers of colmap_provider.py:1084-1175 and the mixed-sampling
    concatenation with the reference's asymmetries: local rays are appended to
    rays_o, rays_d, masks, incoherent_masks, error_maps, cam_near_far and
    poses, and NOT to images or inds_coarse.

Two sources of randomness.  rng="torch" draws with torch's generator in the
reference's call order: with the same torch.manual_seed a CPU BatchSource
reproduces the reference's collate.  The pixel choice is then a few torch ops
and the gather is k_batch_gather (csrc/batch_sampler.hip) on a CUDA source,
torch ops (`torch_gather`, the twin the kernel is tested against) on a CPU one.
rng=PhiloxBatch(seed, offset) lets the kernels draw: statistically the
reference's sampling, not its stream; the contract is in include/samnerf_hip.h.
A seeded step is a pure function of (seed, offset, global_step) and the maps.

Mode P: the reference adds its [num_patch, 2] corners to [1, p*p, 2] offsets
(utils.py:215; the line that expands each patch is commented out above it),
which only broadcasts when num_patch is 1 or p*p, and for p*p gives pixel k of
patch k rather than whole patches.  The sampler returns whole patches, the
evident intent; the two agree at num_patch = 1.

Out of scope: use_multi_res resizing (colmap_provider.py:940-962), the SAM
pose-augmentation branch (its rays are full-image: ops.get_rays), img_names
and file loading.
"""
import ctypes
import dataclasses

import numpy as np
import torch

from . import _lib
from ._lib import check, lib
from .ops import _o, _ptr, _stream

MODE_R, MODE_P, MODE_C, MODE_E = 0, 1, 2, 3


@dataclasses.dataclass(frozen=True)
class PhiloxBatch:
    """The pixel choice drawn inside the kernels (samnerf_batch_draw, seeded):
    every draw is a pure function of (seed, offset, item) under Philox4x32-10
    -- the contract is in include/samnerf_hip.h; its counters are disjoint
    from PhiloxPerturb's, so one (seed, offset) may serve both.  Statistically
    the reference's sampling, not torch's generator stream (rng="torch" keeps
    that).  Step `global_step` of a sampler uses the offsets offset + 2 *
    global_step (global rays) and that plus one (local patches)."""
    seed: int
    offset: int = 0

    def __post_init__(self):
        for name in ("seed", "offset"):
            v = getattr(self, name)
            if not (isinstance(v, int) and 0 <= v < 1 << 63):
                raise ValueError(f"PhiloxBatch: {name} must be an integer in [0, 2^63)")


class BatchSource:
    """The device-resident tables of a dataset (the reference's ColmapDataset
    fields of the same names): poses [n_img,4,4], intrinsics [n_img,4] (or
    [1,4]), and optionally images [n_img,H,W,C] uint8 (or float32, C = 3 or 4),
    masks [n_img,H,W,1] int64, incoherent_masks and gt_incoherent_masks
    [n_img, size * size] bool / uint8 / float32, error_map [n_img, M * M]
    float32 -- the live tensor, the same object handed to mask_train_step_full,
    which updates it in place -- and cam_near_far [n_img,2]."""

    def __init__(self, poses, intrinsics, H, W, images=None, masks=None, incoherent_masks=None,
                 gt_incoherent_masks=None, error_map=None, cam_near_far=None, incoherent_mask_size=None):
        self.poses = poses.to(torch.float32).contiguous()
        self.intrinsics = intrinsics.to(torch.float32).contiguous()
        self.H, self.W = int(H), int(W)
        self.device = self.poses.device
        n = self.n_img = self.poses.shape[0]
        if self.poses.shape[1:] != (4, 4) or self.intrinsics.dim() != 2 or self.intrinsics.shape[1] != 4 \
                or self.intrinsics.shape[0] not in (1, n):
            raise ValueError("BatchSource: poses [n_img,4,4] and intrinsics [n_img or 1, 4]")
        self.incoherent_mask_size = int(self.H if incoherent_mask_size is None else incoherent_mask_size)
        if images is not None:
            if images.dtype not in (torch.uint8, torch.float32) or images.shape[:3] != (n, self.H, self.W) \
                    or images.dim() != 4 or not 1 <= images.shape[3] <= 4:
                raise ValueError("BatchSource: images must be [n_img,H,W,C] uint8 or float32, C <= 4")
        if masks is not None:
            if masks.dtype != torch.int64 or tuple(masks.shape) not in ((n, self.H, self.W), (n, self.H, self.W, 1)):
                raise ValueError("BatchSource: masks must be int64 [n_img,H,W,1]")
        for name, t in (("incoherent_masks", incoherent_masks), ("gt_incoherent_masks", gt_incoherent_masks)):
            if t is not None and (t.dtype not in (torch.bool, torch.uint8, torch.float32) or t.dim() != 2
                                  or t.shape[0] != n):
                raise ValueError(f"BatchSource: {name} must be [n_img, cells] bool, uint8 or float32")
        if incoherent_masks is not None and incoherent_masks.shape[1] != self.incoherent_mask_size ** 2:
            raise ValueError("BatchSource: incoherent_masks must hold incoherent_mask_size ** 2 cells per image")
        if error_map is not None:
            m = int(round(error_map.shape[-1] ** 0.5))
            if error_map.dtype != torch.float32 or error_map.dim() != 2 or error_map.shape[0] != n \
                    or m * m != error_map.shape[1] or not error_map.is_contiguous():
                raise ValueError("BatchSource: error_map must be contiguous float32 [n_img, M * M]")
        if cam_near_far is not None and (cam_near_far.dtype != torch.float32 or tuple(cam_near_far.shape) != (n, 2)):
            raise ValueError("BatchSource: cam_near_far must be float32 [n_img,2]")
        self.images = None if images is None else images.contiguous()
        self.masks = None if masks is None else masks.contiguous()
        self.incoherent_masks = None if incoherent_masks is None else incoherent_masks.contiguous()
        self.gt_incoherent_masks = None if gt_incoherent_masks is None else gt_incoherent_masks.contiguous()
        self.error_map = error_map                       # never copied: the trainer's tensor
        self.cam_near_far = None if cam_near_far is None else cam_near_far.contiguous()
        for name in ("intrinsics", "images", "masks", "incoherent_masks", "gt_incoherent_masks", "error_map",
                     "cam_near_far"):
            t = getattr(self, name)
            if t is not None and t.device != self.device:
                raise ValueError(f"BatchSource: {name} is on {t.device}, poses on {self.device}")

    @property
    def error_map_size(self):
        return None if self.error_map is None else int(round(self.error_map.shape[-1] ** 0.5))

    def c_struct(self, intrinsics=None, with_cam_near_far=True):
        """samnerf_batch_source over these tensors (which the caller keeps alive)."""
        intr = self.intrinsics if intrinsics is None else intrinsics
        s = _lib.SamnerfBatchSource()
        s.poses, s.intrinsics = _ptr(self.poses), _ptr(intr)
        s.n_img, s.n_intr, s.H, s.W = self.n_img, intr.shape[0], self.H, self.W
        if self.images is not None:
            s.images, s.C, s.images_float = _ptr(self.images), self.images.shape[3], int(self.images.dtype == torch.float32)
        s.masks = _ptr(self.masks)
        if self.incoherent_masks is not None:
            s.incoherent_masks, s.incoherent_bytes = _ptr(self.incoherent_masks), self.incoherent_masks.element_size()
            s.incoherent_size = self.incoherent_mask_size
        if self.error_map is not None:
            s.error_map, s.error_size = _ptr(self.error_map), self.error_map_size
        if with_cam_near_far:
            s.cam_near_far = _ptr(self.cam_near_far)
        return s


# ----------------------------------------------------------- the torch twin --

def torch_select(mode, H, W, n, patch=1, weights=None, size=None, device="cpu", generator=None):
    """The pixel choice of get_rays' N > 0 branches in the reference's torch ops
    and call order.  weights: the [B, size * size] rows of modes C and E.
    Returns (pixels [rays], cells): cells is mode E's inds_coarse [1, n], mode
    C's centres [B, 1], else None.  Mode R draws only the pixels (the images
    are the collate's draw)."""
    g = generator
    if mode == MODE_R:
        return torch.randint(0, H * W, size=[n], device=device, generator=g), None
    if mode == MODE_E:
        if size != 128:
            raise ValueError(f"mode E takes a 128 x 128 map only (utils.py:226 divides by a literal 128), not {size}")
        cells = torch.multinomial(weights.to(torch.float32), n, replacement=False, generator=g)
        B = weights.shape[0]
        cx, cy = cells // 128, cells % 128
        sx, sy = H / size, W / size
        x = (cx * sx + torch.rand(B, n, device=device, generator=g) * sx).long().clamp(max=H - 1)
        y = (cy * sy + torch.rand(B, n, device=device, generator=g) * sy).long().clamp(max=W - 1)
        return (x * W + y)[0], cells
    cells = None
    if mode == MODE_C:
        cells = torch.multinomial(weights.to(torch.float32), 1, generator=g)
        cx, cy = cells // size, cells % size
        sx, sy = H / size, W / size
        x0 = torch.clamp(cx * sx - patch // 2, min=0, max=H - patch - 1).long()
        y0 = torch.clamp(cy * sy - patch // 2, min=0, max=W - patch - 1).long()
    else:
        x0 = torch.randint(0, H - patch, size=[n], device=device, generator=g)[:, None]
        y0 = torch.randint(0, W - patch, size=[n], device=device, generator=g)[:, None]
    return expand_patches(x0, y0, patch, W), cells


def expand_patches(x0, y0, patch, W):
    """utils.py:206-219: corners [B, 1] -> the flat pixels of their patches."""
    k = torch.arange(patch * patch, device=x0.device)
    return ((x0 + (k // patch)[None]) * W + y0 + (k % patch)[None]).reshape(-1)


def torch_gather(src, index, pixels, H, W, intrinsics=None, coarse_size=None):
    """What get_rays (utils.py:238-275) and the collate's gathers
    (colmap_provider.py:1084-1162) produce for rays `pixels` of images `index`
    ([1] or one per ray), op for op.  The twin of k_batch_gather."""
    dev = pixels.device
    index = torch.as_tensor(index, device=dev).reshape(-1)
    poses = src.poses[index]
    intr = src.intrinsics[index if src.intrinsics.shape[0] > 1 else torch.zeros_like(index)] \
        if intrinsics is None else intrinsics
    fx, fy, cx, cy = intr[:, 0], intr[:, 1], intr[:, 2], intr[:, 3]
    row, col = pixels // W, pixels % W
    i, j = col.to(torch.float32) + 0.5, row.to(torch.float32) + 0.5
    out = {"i": i.long(), "j": j.long()}
    zs = -torch.ones_like(i)
    xs = (i - cx) / fx
    ys = -(j - cy) / fy
    directions = torch.stack((xs, ys, zs), dim=-1)
    out["rays_d"] = (directions.unsqueeze(1) @ poses[:, :3, :3].transpose(-1, -2)).squeeze(1)
    out["rays_o"] = poses[:, :3, 3].expand_as(out["rays_d"])
    if coarse_size:
        out["inds_coarse"] = ((row * (coarse_size / H)).long() * coarse_size + (col * (coarse_size / W)).long()).long()
    rj, ri = out["j"], out["i"]
    if src.images is not None:
        out["images"] = (src.images[index, rj, ri].float() / 255).view(-1, src.images.shape[-1])
    if src.masks is not None:
        out["masks"] = src.masks[index, rj, ri].view(-1, 1)
    if src.incoherent_masks is not None:
        S = src.incoherent_mask_size
        s = S / src.H
        out["incoherent_masks"] = src.incoherent_masks[index, (rj * s).long() * S + (ri * s).long()].view(-1)
    if src.error_map is not None:
        S = src.error_map_size
        s = S / src.H
        out["error_maps"] = src.error_map[index, (rj * s).long() * S + (ri * s).long()].view(-1)
    if src.cam_near_far is not None:
        out["cam_near_far"] = src.cam_near_far[index]
    return out


# ------------------------------------------------------------- the kernels --

def hip_gather(src, index, pixels, H, W, intrinsics=None, coarse_size=None, want=None):
    """k_batch_gather: torch_gather's dict for a CUDA source, one launch.
    cam_near_far comes per ray, [n, 2].  want: the keys to produce (default:
    every one whose table the source holds)."""
    dev = src.device
    if dev.type != "cuda":
        raise RuntimeError("hip_gather needs a CUDA BatchSource (torch_gather is the CPU twin)")
    index = torch.as_tensor(index, device=dev, dtype=torch.int64).reshape(-1).contiguous()
    pixels = pixels.to(torch.int64).contiguous()
    n = pixels.shape[0]
    if intrinsics is not None:
        intrinsics = intrinsics.to(device=dev, dtype=torch.float32).contiguous()
    s = src.c_struct(intrinsics)
    shapes = {"rays_o": ((n, 3), torch.float32), "rays_d": ((n, 3), torch.float32), "i": ((n,), torch.int64),
              "j": ((n,), torch.int64)}
    if coarse_size:
        shapes["inds_coarse"] = ((n,), torch.int64)
    if src.images is not None:
        shapes["images"] = ((n, src.images.shape[3]), torch.float32)
    if src.masks is not None:
        shapes["masks"] = ((n, 1), torch.int64)
    if src.incoherent_masks is not None:
        shapes["incoherent_masks"] = ((n,), src.incoherent_masks.dtype)
    if src.error_map is not None:
        shapes["error_maps"] = ((n,), torch.float32)
    if src.cam_near_far is not None:
        shapes["cam_near_far"] = ((n, 2), torch.float32)
    if want is not None:
        shapes = {k: v for k, v in shapes.items() if k in want}
    out = {k: torch.empty(shape, dtype=dt, device=dev) for k, (shape, dt) in shapes.items()}
    o = _lib.SamnerfBatchOut()
    for k, t in out.items():
        setattr(o, k, _ptr(t))
    check(lib().samnerf_batch_gather(ctypes.byref(s), _ptr(index), index.shape[0], _ptr(pixels), n, H, W,
                                     int(coarse_size or 0), ctypes.byref(o), _stream(dev)), "samnerf_batch_gather")
    return out


def check_weights(weights, n, what):
    """The precondition of the weighted draws: every row holds at least n
    weights that are positive and finite (one read-back)."""
    w = weights.to(torch.float32)
    ok = ((w > 0) & torch.isfinite(w)).sum(-1)
    if bool((ok < n).any()):
        raise ValueError(f"{what}: a map row holds {int(ok.min())} positive finite weights, the draw needs {n}")


def hip_draw(mode, n_img, H, W, n, *, device, patch=1, M=0, weights=None, rows=None, philox=None, offset=0,
             int0=None, int1=None, keys=None, u0=None, u1=None):
    """samnerf_batch_draw.  philox = PhiloxBatch: the seeded form at `offset`
    (added to philox.offset); else the array form over int0 / int1 (R, P), keys
    (C, E) and u0 / u1 (E).  weights: the [n_img, M * M] table, rows: the
    images of the map rows.  Returns {index, pixels, cells} (those the mode
    writes)."""
    a = _lib.SamnerfBatchDrawArgs()
    a.mode, a.seeded = mode, int(philox is not None)
    if philox is not None:
        a.seed, a.offset = philox.seed, philox.offset + offset
    a.n_img, a.H, a.W, a.n, a.patch, a.M = n_img, H, W, n, patch, M
    if mode == MODE_E and M != 128:
        raise ValueError(f"mode E takes a 128 x 128 map only (utils.py:226 divides by a literal 128), not {M}")
    if weights is not None:
        if not weights.is_contiguous() or weights.dtype not in (torch.float32, torch.bool, torch.uint8):
            raise ValueError("hip_draw: weights must be contiguous float32, bool or uint8")
        a.weights, a.weight_bytes = _ptr(weights), weights.element_size()
    if rows is not None:
        rows = torch.as_tensor(rows, device=device, dtype=torch.int64).reshape(-1).contiguous()
    a.rows = _ptr(rows)
    for name, t, dt in (("int0", int0, torch.int64), ("int1", int1, torch.int64), ("keys", keys, torch.float32),
                        ("u0", u0, torch.float32), ("u1", u1, torch.float32)):
        if t is not None:
            if t.dtype != dt or not t.is_contiguous() or t.device.type != "cuda":
                raise ValueError(f"hip_draw: {name} must be a contiguous CUDA {dt} tensor")
            setattr(a, name, _ptr(t))
    rays = n * patch * patch if mode in (MODE_P, MODE_C) else n
    out = {"pixels": torch.empty(rays, dtype=torch.int64, device=device)}
    if mode in (MODE_R, MODE_C):
        out["index"] = torch.empty(rays, dtype=torch.int64, device=device)
    if mode in (MODE_C, MODE_E):
        out["cells"] = torch.empty(n, dtype=torch.int64, device=device)
    for k, t in out.items():
        setattr(a, k, _ptr(t))
    check(lib().samnerf_batch_draw(ctypes.byref(a), _stream(device)), "samnerf_batch_draw")
    return out


def batch_draw_fill(philox, items, range0, range1, device, weights=None, rows=None, B=0, offset=0):
    """samnerf_batch_draw_fill: the raw draws of (philox.seed, philox.offset +
    offset) as tensors -- int0, int1, u0, u1 [items] and, with weights
    [n_img, cells], keys [B, cells] -- which feed hip_draw's array form."""
    out = {"int0": torch.empty(items, dtype=torch.int64, device=device),
           "int1": torch.empty(items, dtype=torch.int64, device=device),
           "u0": torch.empty(items, dtype=torch.float32, device=device),
           "u1": torch.empty(items, dtype=torch.float32, device=device)}
    n_img = cells = wb = 0
    if weights is not None:
        n_img, cells, wb = weights.shape[0], weights.shape[1], weights.element_size()
        out["keys"] = torch.empty(B, cells, dtype=torch.float32, device=device)
    if rows is not None:
        rows = torch.as_tensor(rows, device=device, dtype=torch.int64).reshape(-1).contiguous()
    check(lib().samnerf_batch_draw_fill(philox.seed, philox.offset + offset, items, range0, range1, _ptr(out["int0"]),
                                        _ptr(out["int1"]), _ptr(out["u0"]), _ptr(out["u1"]), _ptr(weights), wb,
                                        n_img, _ptr(rows), B, cells, _ptr(out.get("keys")), _stream(device)),
          "samnerf_batch_draw_fill")
    return out


def batch_draw_host(seed, offset, item, range0, range1):
    """samnerf_batch_draw_host: ((int0, int1), (u0, u1)) of one item, no GPU."""
    ints = (ctypes.c_int64 * 2)()
    us = (ctypes.c_float * 2)()
    check(lib().samnerf_batch_draw_host(seed, offset, item, range0, range1, ints, us), "samnerf_batch_draw_host")
    return (int(ints[0]), int(ints[1])), (float(us[0]), float(us[1]))


# -------------------------------------------------------------- the sampler --

def fixed_fov_intrinsics(res, device):
    """colmap_provider.py:1011-1015."""
    focal = res / (2 * np.tan(0.5 * 60 * np.pi / 180))
    return torch.from_numpy(np.array([focal, focal, res / 2, res / 2], dtype=np.float32)).unsqueeze(0).to(device)


class TrainBatchSampler:
    """The reference's training collate without SAM over a BatchSource; see
    the module docstring.  opt: the reference's options (num_rays, with_mask,
    patch_size, error_map, error_map_size, mixed_sampling, num_local_sample,
    local_sample_patch_size, rgb_similarity_iter, random_image_batch,
    enable_cam_near_far, online_resolution).  rng: "torch" or a PhiloxBatch
    (CUDA source only).  use_default_intrinsics: the dataset's flag
    (colmap_provider.py:1009-1015).  check_inputs: verify the weighted draws'
    precondition each step (one read-back), as mask_train_step_full does.

    use_kernels: which path a CUDA source takes for the gather under
    rng="torch" (default True; False is the torch twin on the GPU)."""

    def __init__(self, source, opt, rng="torch", use_default_intrinsics=True, check_inputs=True, use_kernels=True,
                 generator=None):
        if rng != "torch" and not isinstance(rng, PhiloxBatch):
            raise ValueError('TrainBatchSampler: rng is "torch" or a PhiloxBatch')
        if _o(opt, "with_sam", False):
            raise ValueError("TrainBatchSampler: the SAM stage renders full images (ops.get_rays)")
        if _o(opt, "use_multi_res", False):
            raise ValueError("TrainBatchSampler: use_multi_res resizing is out of scope")
        if isinstance(rng, PhiloxBatch) and source.device.type != "cuda":
            raise RuntimeError("TrainBatchSampler: PhiloxBatch draws inside the HIP kernels; there is no CPU "
                               "fallback (rng='torch' runs anywhere)")
        self.source, self.opt, self.rng = source, opt, rng
        self.use_default_intrinsics = use_default_intrinsics
        self.check_inputs = check_inputs
        self.generator = generator
        self.hip = source.device.type == "cuda" and (use_kernels or isinstance(rng, PhiloxBatch))
        self.random_image_batch = bool(_o(opt, "random_image_batch", False))
        # the last step's choice, to log or replay it: index, pixels and, under
        # mixed sampling, local_index, local_pixels
        self.last_draw = {}

    # the gather of one group of rays
    def _gather(self, index, pixels, H, W, intrinsics, coarse):
        if self.hip:
            return hip_gather(self.source, index, pixels, H, W, intrinsics, coarse)
        return torch_gather(self.source, index, pixels, H, W, intrinsics, coarse)

    def sample(self, global_step, index):
        src, opt, dev = self.source, self.opt, self.source.device
        seeded = isinstance(self.rng, PhiloxBatch)
        g = self.generator
        iter_ = _o(opt, "rgb_similarity_iter", -1)
        with_mask = bool(_o(opt, "with_mask", False))
        use_error = bool(_o(opt, "error_map", False))
        # colmap_provider.py:966-979
        if global_step > iter_ or global_step / src.n_img > 3:
            self.random_image_batch = True
        n = int(opt.num_rays)
        random_sample = False
        if self.random_image_batch and (not with_mask or global_step <= iter_ or iter_ < 0
                                        or _o(opt, "patch_size", 1) <= 1):
            random_sample = True
        philox_off = 2 * int(global_step)
        if random_sample:
            # seeded: mode R draws the images with the pixels, below
            index = None if seeded else torch.randint(0, src.n_img, size=(n,), device=dev, generator=g)
        elif torch.is_tensor(index):
            index = index.to(dev).reshape(-1)
        else:
            index = [int(v) for v in np.atleast_1d(index)]
        if not random_sample and len(index) != 1:
            raise ValueError("TrainBatchSampler: the dataloader hands one image index per step")
        # colmap_provider.py:983-1015
        H, W = src.H, src.W
        fixed = None
        if with_mask and not self.use_default_intrinsics:
            H = W = int(opt.online_resolution)
            fixed = fixed_fov_intrinsics(H, dev)
        # colmap_provider.py:1024-1044: which map, which mode
        patch = int(_o(opt, "patch_size", 1)) if with_mask else 1
        if use_error:
            table, size = src.error_map, int(opt.error_map_size)
            if table is not None and size != src.error_map_size:
                raise ValueError("TrainBatchSampler: opt.error_map_size is not the error map's side")
        else:
            table = src.gt_incoherent_masks if (not random_sample and _o(opt, "patch_size", 1) > 1) else None
            size = src.H
        if random_sample:
            mode = MODE_R
        elif patch > 1:
            mode = MODE_C if table is not None else MODE_P
        else:
            mode = MODE_E
            if table is None:
                raise ValueError("TrainBatchSampler: patch_size 1 without random sampling draws from a map "
                                 "(utils.py:223) and the source holds none")
        if mode in (MODE_C, MODE_E) and table.shape[1] != size * size:
            raise ValueError(f"TrainBatchSampler: the map holds {table.shape[1]} cells, not {size} x {size}")
        if mode == MODE_E and size != 128:
            raise ValueError(f"mode E takes a 128 x 128 map only (utils.py:226 divides by a literal 128), not {size}")
        cells = None
        if mode in (MODE_C, MODE_E) and self.check_inputs:
            check_weights(table[index], n if mode == MODE_E else 1, "TrainBatchSampler")
        if seeded:
            count = n // (patch * patch) if mode == MODE_P else (1 if mode == MODE_C else n)
            d = hip_draw(mode, src.n_img, H, W, count, device=dev, patch=patch, M=size if mode >= MODE_C else 0,
                         weights=table if mode >= MODE_C else None, rows=index if mode >= MODE_C else None,
                         philox=self.rng, offset=philox_off)
            pixels = d["pixels"]
            if mode == MODE_R:
                index = d["index"]
            if mode == MODE_E:
                cells = d["cells"][None]
        else:
            count = n // (patch * patch) if mode == MODE_P else n
            pixels, c = torch_select(mode, H, W, count, patch, None if mode < MODE_C else table[index], size, dev, g)
            if mode == MODE_E:
                cells = c
        rays = self._gather(index, pixels, H, W, fixed, None if mode == MODE_E else size)
        self.last_draw = {"index": index, "pixels": pixels}
        if cells is not None:
            rays["inds_coarse"] = cells
        # colmap_provider.py:1047-1070: the local patches of mixed sampling
        local = None
        if _o(opt, "mixed_sampling", False) and global_step > iter_:
            L, lp = int(opt.num_local_sample), int(opt.local_sample_patch_size)
            if lp < 2:
                raise ValueError("TrainBatchSampler: local_sample_patch_size must be at least 2 (at 1 the "
                                 "reference draws one ray for num_local_sample poses)")
            if fixed is None and random_sample:
                raise ValueError("TrainBatchSampler: the reference hands the global rays' per-ray intrinsics to the "
                                 "local patches (colmap_provider.py:1060), which does not broadcast; mixed sampling "
                                 "over a random image batch needs the fixed-fov intrinsics "
                                 "(use_default_intrinsics=False)")
            if use_error:
                ltable, lsize = src.error_map, int(opt.error_map_size)
            else:
                ltable, lsize = src.incoherent_masks, src.H
            if ltable is None:
                raise ValueError("TrainBatchSampler: mixed sampling draws its patches from a map "
                                 "(utils.py:182) and the source holds none")
            if ltable.shape[1] != lsize * lsize:
                raise ValueError(f"TrainBatchSampler: the map holds {ltable.shape[1]} cells, not {lsize} x {lsize}")
            if seeded:
                if self.check_inputs:
                    check_weights(ltable, 1, "TrainBatchSampler")      # any image may be drawn
                d = hip_draw(MODE_C, src.n_img, H, W, L, device=dev, patch=lp, M=lsize, weights=ltable,
                             philox=self.rng, offset=philox_off + 1)
                lindex, lpixels = d["index"], d["pixels"]
            else:
                lidx = torch.randint(0, src.n_img, size=(L,), device=dev, generator=g)
                lindex = lidx[..., None].expand(-1, lp * lp).reshape(-1)
                if self.check_inputs:
                    check_weights(ltable[lidx], 1, "TrainBatchSampler")
                lpixels, _ = torch_select(MODE_C, H, W, 1, lp, ltable[lidx], lsize, dev, g)
            # the global rays' intrinsics: the fixed-fov row, or the one image's
            lintr = fixed if fixed is not None else src.intrinsics[index if src.intrinsics.shape[0] > 1 else [0]]
            local = self._gather(lindex, lpixels, H, W, lintr, None)
            self.last_draw.update(local_index=lindex, local_pixels=lpixels)
            local["poses"] = src.poses[lindex]
        # colmap_provider.py:1019, :1084-1181
        res = {"H": H, "W": W, "use_default_intrinsics": self.use_default_intrinsics, "img_names": None}
        single = not random_sample

        def joined(key):
            return rays[key] if local is None else torch.cat([rays[key], local[key]], 0)
        if src.images is not None:
            res["images"] = rays["images"]
        if src.masks is not None:
            res["masks"] = joined("masks")
        if src.incoherent_masks is not None:
            res["incoherent_masks"] = joined("incoherent_masks")
        if src.error_map is not None:
            res["error_maps"] = joined("error_maps")
        if _o(opt, "enable_cam_near_far", False) and src.cam_near_far is not None:
            cnf = rays["cam_near_far"][:1] if (single and self.hip) else rays["cam_near_far"]
            res["cam_near_far"] = cnf if local is None else torch.cat([cnf, local["cam_near_far"]], 0)
        idx_t = torch.as_tensor(index, device=dev).reshape(-1)
        res["poses"] = src.poses[idx_t]
        res["intrinsics"] = fixed if fixed is not None else \
            src.intrinsics[idx_t if src.intrinsics.shape[0] > 1 else torch.zeros_like(idx_t)]
        res["rays_o"], res["rays_d"] = rays["rays_o"], rays["rays_d"]
        res["index"] = index
        if use_error:
            res["inds_coarse"] = rays["inds_coarse"]
        if local is not None:
            res["poses"] = torch.cat([res["poses"], local["poses"]], 0)
            res["rays_o"] = torch.cat([res["rays_o"], local["rays_o"]], 0)
            res["rays_d"] = torch.cat([res["rays_d"], local["rays_d"]], 0)
        res["i"], res["j"] = rays["i"], rays["j"]
        return res
