"""Incoherent-region masks: the [n_img, cells] bool table the training sampler
draws its local patches from and the mask loss weights its rays by.

The reference builds it in two places:
  * at load, from the ground-truth masks (colmap_provider.py:798-801):
    `gt_incoherent_masks`;
  * under --use_dynamic_incoherent, every incoherent_update_iter steps from the
    mask head's own renders of every training view at incoherent_mask_size^2
    (Trainer.update_incoherent_mask, nerf/utils.py:1757-1780, with render_mask,
    :1716-1737, and collate_mask, colmap_provider.py:907-932):
    `update_incoherent_mask`, switched by `due`.
Both run get_incoherent_mask (utils.py:283-298) and turn its float map into a
bool with .to(torch.bool): any non-zero cell is True, a residue below the 0.01
threshold included.

CUDA tensors go to csrc/incoherent.hip: `render_mask_ids` is
samnerf_incoherent_ids (softmax, [sum of the first K - 1, last], argmax as one
byte per ray) and `get_incoherent_mask` / `incoherent_table` are
samnerf_incoherent_masks (the whole chain for every view in one launch).
`torch_get_incoherent_mask` and `torch_render_mask_ids` are the reference's own
op sequences; they are what a CPU tensor gets and what the tests compare the
kernels with.

Sizes that sfact does not divide stay on the torch ops, on any device: there
the reference's bool is set by the rounding residue of ATen's resize kernels
(values such as 1.2e-8 become True), not by the mask, and no other kernel
reproduces it.  At divisible sizes every product and sum of the chain is exact
in fp32 (integer ids below 2^14), so the kernel equals the reference bit for
bit.  `last_path` names the path the last get_incoherent_mask /
incoherent_table call took: "hip" or "torch".

Kept as the reference has it: with n_inst == 1 render_mask returns the sigmoid
of one column, whose argmax is always 0, so the dynamic table is all False.
"""
import ctypes

import torch
import torch.nn.functional as F

from . import _lib
from ._lib import check, lib
from .ops import _o, _stream, torch_mask_probs

last_path = None
# update_incoherent_mask renders as many views per render call as fit this
# many rays -- a 512 x 512 view's worth, 16 views at incoherent_mask_size 128 --
# in one unstaged call: one view of 128 x 128 is a single chunk of the default
# max_ray_batch and leaves most of the GPU idle.  The table does not depend on it.
RAYS_PER_CALL = 1 << 18
_INT_TYPES = (torch.bool, torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64)


# ------------------------------------------------------------- torch mirror --

def torch_get_incoherent_mask(input_masks, sfact=2, keep_size=True):
    """utils.py:283-298, restated: input_masks [n, 1, h, w] -> the float map
    mask_uncertain [n, 1, h, w] ([n, 1, h // sfact, w // sfact] without
    keep_size)."""
    mask = input_masks.float()
    w = input_masks.shape[-1]
    h = input_masks.shape[-2]
    mask_small = F.interpolate(mask, (h // sfact, w // sfact), mode='bilinear')
    mask_recover = F.interpolate(mask_small, (h, w), mode='bilinear')
    mask_residue = (mask - mask_recover).abs()
    mask_uncertain = F.interpolate(mask_residue, (h // sfact, w // sfact), mode='bilinear')
    mask_uncertain[mask_uncertain >= 0.01] = 1.
    if keep_size:
        mask_uncertain = F.interpolate(mask_uncertain, (h, w), mode='nearest')
    return mask_uncertain


def torch_render_mask_ids(logits, n_inst, return_pred=False):
    """render_mask's lines after the render (utils.py:1732-1737) and
    update_incoherent_mask's argmax (:1767) on logits [..., K]: the ids [...]
    as uint8 (the argmax's int64 holds 0 and 1 only), and pred_mask [..., 2]
    ([..., K] at n_inst == 1) with return_pred."""
    pred_mask = torch_mask_probs(logits, n_inst)
    if n_inst > 1:
        pred_mask = torch.stack([pred_mask[..., :-1].sum(-1), pred_mask[..., -1]], -1)
    ids = pred_mask.argmax(-1).to(torch.uint8)
    return (ids, pred_mask) if return_pred else ids


# ------------------------------------------------------------------ kernels --

def _divisible(h, w, sfact):
    sfact = int(sfact)
    return sfact >= 1 and sfact & (sfact - 1) == 0 and h // sfact > 0 and w // sfact > 0 \
        and h % sfact == 0 and w % sfact == 0


def _hip_masks(masks, n, H, W, sfact, keep_size, want_table, want_map, table=None):
    """samnerf_incoherent_masks over contiguous int64 or uint8 masks [n, H, W]."""
    dev = masks.device
    cells = H * W if keep_size else (H // sfact) * (W // sfact)
    a = _lib.SamnerfIncoherentMasksArgs()
    a.n, a.H, a.W, a.sfact, a.keep_size = n, H, W, int(sfact), int(bool(keep_size))
    a.input_type = 0 if masks.dtype == torch.int64 else 1
    a.masks = masks.data_ptr()
    if want_table and table is None:
        table = torch.empty(n, cells, dtype=torch.bool, device=dev)
    fmap = torch.empty(n, cells, dtype=torch.float32, device=dev) if want_map else None
    a.table = None if table is None else table.data_ptr()
    a.uncertain = None if fmap is None else fmap.data_ptr()
    check(lib().samnerf_incoherent_masks(ctypes.byref(a), _stream(dev)), "samnerf_incoherent_masks")
    return table, fmap


def _kernel_input(masks):
    """The masks as the kernel reads them, or None where it does not: integer
    ids as int64 or uint8 [n, H, W] on a GPU."""
    if not masks.is_cuda or masks.dtype not in _INT_TYPES:
        return None
    if masks.dtype not in (torch.int64, torch.uint8):
        masks = masks.to(torch.uint8 if masks.dtype == torch.bool else torch.int64)
    return masks.contiguous()


def get_incoherent_mask(input_masks, sfact=2, keep_size=True):
    """The reference's get_incoherent_mask: input_masks [n, 1, h, w] (integer
    ids below 2^14) -> the float map mask_uncertain [n, 1, h, w], or
    [n, 1, h // sfact, w // sfact] without keep_size.  Integer ids on a GPU at a
    size sfact (a power of two) divides run on the kernel; everything else is
    torch_get_incoherent_mask (see the module docstring); `last_path` says
    which."""
    global last_path
    if input_masks.dim() != 4 or input_masks.shape[1] != 1:
        raise ValueError("get_incoherent_mask: input_masks must be [n, 1, h, w]")
    n, _, h, w = input_masks.shape
    m = _kernel_input(input_masks) if _divisible(h, w, sfact) else None
    if m is None:
        last_path = "torch"
        return torch_get_incoherent_mask(input_masks, sfact, keep_size)
    last_path = "hip"
    _, fmap = _hip_masks(m, n, h, w, sfact, keep_size, False, True)
    return fmap.view(n, 1, h, w) if keep_size else fmap.view(n, 1, h // sfact, w // sfact)


def incoherent_table(masks, sfact=2, out=None):
    """get_incoherent_mask(...).to(torch.bool) of masks [n, H, W, 1] (or
    [n, H, W]) as the [n, H * W] bool table of BatchSource; out: a bool
    [n, H * W] tensor to write instead of a new one."""
    global last_path
    if masks.dim() == 4 and masks.shape[3] == 1:
        masks = masks[..., 0]
    if masks.dim() != 3:
        raise ValueError("incoherent_table: masks must be [n, H, W, 1] or [n, H, W]")
    n, H, W = masks.shape
    if out is not None and (out.dtype != torch.bool or tuple(out.shape) != (n, H * W) or not out.is_contiguous()
                            or out.device != masks.device):
        raise ValueError("incoherent_table: out must be a contiguous bool [n, H * W] tensor on the masks' device")
    m = _kernel_input(masks) if _divisible(H, W, sfact) else None
    if m is None:
        last_path = "torch"
        table = torch_get_incoherent_mask(masks[:, None], sfact).to(torch.bool).view(n, H * W)
        if out is None:
            return table
        out.copy_(table)
        return out
    last_path = "hip"
    table, _ = _hip_masks(m, n, H, W, sfact, True, True, False, table=out)
    return table


def gt_incoherent_masks(masks, opt=None):
    """colmap_provider.py:798-803: the [n, H * W] bool table of the dataset's
    masks [n, H, W, 1] at sfact 2, or None where opt (given) asks for neither
    the similarity loss nor the uncertainty weight."""
    if opt is not None and not (_o(opt, "rgb_similarity_loss_weight", 0) > 0
                                or _o(opt, "incoherent_uncertainty_weight", 1) < 1):
        return None
    return incoherent_table(masks, sfact=2)


def render_mask_ids(logits, n_inst, return_pred=False, out=None):
    """render_mask's pred_mask and its argmax for logits [..., K]: the ids [...]
    as uint8 and, with return_pred, pred_mask [..., 2] ([..., 1] at n_inst ==
    1).  CUDA logits run on samnerf_incoherent_ids, others on
    torch_render_mask_ids.  out: a contiguous uint8 tensor of as many elements
    to write the ids into (a slice of update_incoherent_mask's stack)."""
    if not logits.is_cuda:
        res = torch_render_mask_ids(logits, n_inst, return_pred)
        if out is not None:
            out.view(-1).copy_((res[0] if return_pred else res).reshape(-1))
        return res
    K = int(logits.shape[-1])
    shape = tuple(logits.shape[:-1])
    z = logits.detach().to(torch.float32).contiguous()
    N = z.numel() // max(K, 1)
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=z.device)
    elif out.dtype != torch.uint8 or not out.is_contiguous() or out.numel() != N or out.device != z.device:
        raise ValueError("render_mask_ids: out must be a contiguous uint8 tensor of one element per ray")
    pred = torch.empty(*shape, 2 if n_inst > 1 else 1, device=z.device) if return_pred else None
    a = _lib.SamnerfIncoherentIdsArgs()
    a.N, a.K, a.n_inst = N, K, int(n_inst)
    a.logits, a.ids = z.data_ptr(), out.data_ptr()
    a.pred_mask = None if pred is None else pred.data_ptr()
    check(lib().samnerf_incoherent_ids(ctypes.byref(a), _stream(z.device)), "samnerf_incoherent_ids")
    return (out, pred) if return_pred else out


# ----------------------------------------------------- the dynamic update --

def due(global_step, opt):
    """The condition of utils.py:1820: every incoherent_update_iter steps once
    global_step has reached rgb_similarity_iter (only under
    use_dynamic_incoherent, which is what leaves the table to this update)."""
    if not _o(opt, "use_dynamic_incoherent", False):
        return False
    return global_step % opt.incoherent_update_iter == 0 and global_step >= opt.rgb_similarity_iter


def default_views_per_launch(S):
    """The views of S x S rays that make one render call of RAYS_PER_CALL rays (at least one)."""
    return max(1, RAYS_PER_CALL // (int(S) * int(S)))


def mask_view_rays(source, first, count, S, opt):
    """collate_mask (colmap_provider.py:907-932) for views [first, first +
    count): the rays of their S x S images under the fixed-fov intrinsics, view
    after view, and the per-ray cam_near_far (or None).  One k_batch_gather
    launch from the source's device-resident poses."""
    from .batch import fixed_fov_intrinsics, hip_gather
    dev = source.device
    index = torch.arange(first, first + count, device=dev).repeat_interleave(S * S)
    pixels = torch.arange(S * S, device=dev).repeat(count)
    want = ["rays_o", "rays_d"]
    with_cnf = bool(_o(opt, "enable_cam_near_far", False)) and source.cam_near_far is not None
    if with_cnf:
        want.append("cam_near_far")
    rays = hip_gather(source, index, pixels, S, S, fixed_fov_intrinsics(S, dev), None, want=want)
    return rays["rays_o"], rays["rays_d"], rays.get("cam_near_far")


def update_incoherent_mask(renderer, source, opt, views_per_launch=None):
    """Trainer.update_incoherent_mask on a BatchSource: render every training
    view at S x S (S = source.incoherent_mask_size, the reference's
    int(H / incoherent_downsample_scale)) through the mask head, turn the
    logits into ids, run get_incoherent_mask(sfact=2) over the [n, S, S] stack
    in one launch and write the bool table into source.incoherent_masks
    [n_img, S * S] -- allocated on first use, the same storage afterwards, so
    the sampler's next call reads the new cells.  Nothing is copied to the host
    and nothing synchronises.  The model's train / eval mode is restored.

    views_per_launch: views rendered per render call (default
    default_views_per_launch(S): RAYS_PER_CALL rays); the rays carry their
    view's cam_near_far, and the table is bit for bit the one of a view per
    call.  A call of up to RAYS_PER_CALL rays is one unstaged render; a larger
    one is staged in chunks of opt.max_ray_batch, as the reference's."""
    if source.device.type != "cuda":
        raise RuntimeError("update_incoherent_mask needs a CUDA BatchSource: the render and the kernels run there")
    S, n = int(source.incoherent_mask_size), source.n_img
    if S < 2 or S % 2:
        raise ValueError(f"update_incoherent_mask: incoherent_mask_size {S} must be even: at an odd size the "
                         "reference's table is the rounding residue of its resize kernels")
    n_inst = int(opt.n_inst)
    K = n_inst + int(_o(opt, "redundant_instance", 0))
    if n_inst == 1 and K != 1:
        raise NotImplementedError("update_incoherent_mask: n_inst == 1 with redundant columns")
    per = int(views_per_launch or default_views_per_launch(S))
    if per < 1:
        raise ValueError("update_incoherent_mask: views_per_launch must be at least 1")
    dev = source.device
    ids = torch.empty(n, S, S, dtype=torch.uint8, device=dev)
    was_training = renderer.training
    renderer.eval()
    try:
        with torch.no_grad():
            for first in range(0, n, per):
                count = min(per, n - first)
                ro, rd, cnf = mask_view_rays(source, first, count, S, opt)
                outputs = renderer.render(ro, rd, staged=count * S * S > RAYS_PER_CALL, bg_color=1, perturb=False,
                                          cam_near_far=cnf, return_feats=0,
                                          return_mask=_o(opt, "with_mask", False))
                logits = outputs["instance_mask_logits"].reshape(count * S * S, K)
                render_mask_ids(logits, n_inst, out=ids[first:first + count])
    finally:
        renderer.train(was_training)
    table = source.incoherent_masks
    if table is None or table.dtype != torch.bool or tuple(table.shape) != (n, S * S) or not table.is_contiguous() \
            or table.device != dev:
        table = torch.empty(n, S * S, dtype=torch.bool, device=dev)
    _hip_masks(ids, n, S, S, 2, True, True, False, table=table)
    source.incoherent_masks = table
    source.incoherent_mask_size = S
    return table
