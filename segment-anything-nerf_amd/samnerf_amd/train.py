"""Training steps of the reference's Trainer on this package's kernels.

`rgb_train_step` is Trainer.train_step's RGB branch (nerf/utils.py:897-937):
render with perturbed sampling through the reference's op sequence with the
HIP drop-in encoders (forward and backward kernels: grid, SH), MSE + the
proposal (mip-NeRF 360 inter-level) and distortion losses, optional entropy
regulariser, and the adaptive ray-count update.  `sam_train_step` is its
SAM-distillation branch (utils.py:1072-1106) on the fused forward and the HIP
s_grid scatter (BASELINE config 5).  Optimisation (Adam over
NeRFNetwork.get_params-style groups, main.py:296) is the caller's.
"""
import torch
import torch.nn.functional as F


def update_proposal_now(global_step, with_sam=False):
    """utils.py:912-913: proposal nets train every step for the first 3000,
    then every 5th."""
    return (not with_sam) and (global_step <= 3000 or global_step % 5 == 0)


def rgb_train_step(model, rays_o, rays_d, gt_rgb, global_step, bg_color=None,
                   cam_near_far=None, perturb=True):
    """Returns (pred_rgb, loss, outputs).  gt_rgb [N,3] (or [N,4] with alpha,
    composited on bg as utils.py:903-906).  Updates model.opt.num_rays like
    the reference when adaptive_num_rays is on."""
    opt = model.opt
    if bg_color is None:
        bg_color = 1
    if gt_rgb.shape[-1] == 4:
        gt_rgb = gt_rgb[..., :3] * gt_rgb[..., 3:] + bg_color * (1 - gt_rgb[..., 3:])
    update_proposal = update_proposal_now(global_step, opt.with_sam)
    outputs = model.render(rays_o, rays_d, staged=False, bg_color=bg_color, perturb=perturb,
                           cam_near_far=cam_near_far, update_proposal=update_proposal,
                           return_feats=0)
    pred_rgb = outputs["image"]
    loss = F.mse_loss(pred_rgb, gt_rgb, reduction="none").mean()
    if "proposal_loss" in outputs and opt.lambda_proposal > 0:
        loss = loss + opt.lambda_proposal * outputs["proposal_loss"]
    if "distort_loss" in outputs and opt.lambda_distort > 0:
        loss = loss + opt.lambda_distort * outputs["distort_loss"]
    if opt.lambda_entropy > 0:
        w = outputs["weights_sum"].clamp(1e-5, 1 - 1e-5)
        entropy = -w * torch.log2(w) - (1 - w) * torch.log2(1 - w)
        loss = loss + opt.lambda_entropy * entropy.mean()
    if opt.adaptive_num_rays and "num_points" in outputs:
        opt.num_rays = int(round((opt.num_points / outputs["num_points"]) * opt.num_rays))
    return pred_rgb, loss, outputs


def rgb_train_step_fused(model, rays_o, rays_d, gt_rgb, global_step, bg_color=None,
                         cam_near_far=None, perturb=True):
    """rgb_train_step on the HIP training kernels (samnerf_rgb_train_step,
    csrc/rgb_train.hip): one C call renders the rays (the reference's perturbed
    sampling, drawn with torch's generator in its order, or inside the kernels
    for perturb=PhiloxPerturb(seed, offset)), forms the loss of
    utils.py:917-931 and writes every trained tensor's gradient into .grad --
    what loss.backward() leaves there (the proposal tensors' .grad is None on
    the steps the reference does not update them, utils.py:912-913).  Returns
    (pred_rgb, loss, outputs) like rgb_train_step; loss is a detached 0-d
    tensor, outputs holds image / depth / weights_sum / num_points and the
    unweighted loss terms.  Gradients accumulate into an existing .grad as
    loss.backward() does (proposal tensors: not touched on the steps they do
    not train)."""
    import ctypes

    from ._lib import SamnerfRgbTrainOpts, check, lib
    from .fused import (FusedRenderer, background_rows, call_scope, resolve_perturb, rgb_grads_struct,
                        rgb_train_params)
    from .ops import _ptr, _stream

    opt = model.opt
    if bg_color is None:
        bg_color = 1
    if torch.is_tensor(bg_color) and bg_color.device != gt_rgb.device:
        bg_color = bg_color.to(gt_rgb.device)
    if gt_rgb.shape[-1] == 4:
        gt_rgb = gt_rgb[..., :3] * gt_rgb[..., 3:] + bg_color * (1 - gt_rgb[..., 3:])
    update_proposal = update_proposal_now(global_step, opt.with_sam)
    rays_o = rays_o.contiguous().float()
    rays_d = rays_d.contiguous().float()
    gt = gt_rgb.reshape(-1, 3).contiguous().float()
    N = rays_o.shape[0]
    dev = rays_o.device
    # a scalar, one colour or a colour per ray (samnerf_background.bg_rgb overrides
    # the options' scalar); no gradient flows to it
    bg_scalar, bg_rows = background_rows(bg_color, N, dev)
    fr = getattr(model, "_fused_train", None)
    if fr is None or fr.net is not model:
        fr = model._fused_train = FusedRenderer(model, head_mode=1)
    m = fr.call_model(perturb=resolve_perturb(perturb, N, fr.model().num_steps, dev))
    o = SamnerfRgbTrainOpts()
    o.lambda_proposal = float(getattr(opt, "lambda_proposal", 0.0))
    o.lambda_distort = float(getattr(opt, "lambda_distort", 0.0))
    o.lambda_entropy = float(getattr(opt, "lambda_entropy", 0.0))
    o.update_proposal = int(bool(update_proposal))
    o.bg_color = float(bg_scalar)
    with_prop = bool(update_proposal) and o.lambda_proposal > 0
    every = rgb_train_params(model, True)
    main, prop = every[:7], every[7:]
    trained = main + (prop if with_prop else [])
    # the kernels OVERWRITE their gradient buffers: they write into fresh
    # buffers, which become .grad where it is None and are added into an
    # existing .grad otherwise (loss.backward()'s accumulation)
    for p in trained:
        if p.grad is not None and (p.grad.dtype != torch.float32 or p.grad.device != p.device
                                   or p.grad.shape != p.shape):
            raise RuntimeError("rgb_train_step_fused: existing .grad must be float32, on the "
                               "parameter's device and of its shape")
    scratch = [torch.empty_like(p, memory_format=torch.contiguous_format) for p in trained]
    g = rgb_grads_struct(scratch, with_prop)
    need = lib().samnerf_rgb_train_workspace_size(ctypes.byref(m), N)
    ws = fr._scratch("rgb_train", dev, need)
    cnf, n_cnf = None, 0
    if cam_near_far is not None:
        cnf = cam_near_far.contiguous().float()
        n_cnf = cnf.shape[0]
    image = torch.empty(N, 3, device=dev)
    depth = torch.empty(N, device=dev)
    wsum = torch.empty(N, device=dev)
    loss = torch.empty(5, device=dev)
    with call_scope(model, bg_rows):
        check(lib().samnerf_rgb_train_step(
            ctypes.byref(m), _ptr(rays_o), _ptr(rays_d), N, _ptr(cnf), n_cnf, _ptr(gt),
            ctypes.byref(o), _ptr(image), _ptr(depth), _ptr(wsum), _ptr(loss), ctypes.byref(g),
            _ptr(ws), need, _stream(rays_o)), "rgb_train_step")
    for p, t in zip(trained, scratch):
        if p.grad is None:
            p.grad = t
        else:
            p.grad.add_(t)
    outputs = {"image": image, "depth": depth, "weights_sum": wsum, "num_points": N * int(m.num_steps[2]),
               "mse": loss[0], "proposal_loss": loss[1], "distort_loss": loss[2], "entropy": loss[3]}
    if opt.adaptive_num_rays:
        opt.num_rays = int(round((opt.num_points / outputs["num_points"]) * opt.num_rays))
    return image, loss[4], outputs


def sam_train_step(renderer, rays_o_lr, rays_d_lr, h, w, gt_samvit, cam_near_far=None):
    """utils.py:1091-1106 on the fused path: 64x64 feature rays, bilinear
    resize to the target, MSE.  Returns (pred [1,256,h',w'], loss)."""
    from .fused import render_sam_train
    out = render_sam_train(renderer, rays_o_lr, rays_d_lr, cam_near_far=cam_near_far)
    pred = out["samvit"].reshape(1, h, w, 256).permute(0, 3, 1, 2).contiguous()
    pred = F.interpolate(pred, gt_samvit.shape[2:], mode="bilinear")
    return pred, F.mse_loss(pred, gt_samvit, reduction="none").mean()


def sam_train_step_fused(renderer, rays_o_lr, rays_d_lr, h, w, gt_samvit, cam_near_far=None, view_width=0,
                         resized=True):
    """sam_train_step with the loss on the device as well: render_sam_train
    plus samnerf_amd.feat_loss (csrc/feat_loss.hip) on the render's ray-major
    rows -- no NCHW copy, no float atomics in the resize's gradient, so with
    FusedRenderer(deterministic=True) the step repeats bit for bit at every
    view size, not only where h x w is the teacher's.  Returns (pred
    [1,256,h',w'] without gradient, or None with resized=False; loss)."""
    from .feat_loss import feat_loss
    from .fused import render_sam_train
    out = render_sam_train(renderer, rays_o_lr, rays_d_lr, cam_near_far=cam_near_far, view_width=view_width)
    loss, pred = feat_loss(out["samvit"], h, w, gt_samvit, resized=resized)
    return pred, loss


def sam_distill_step(model, renderer, data, opt, global_step, predictor, cache=None, perturb=True):
    """Trainer.train_step's --with_sam branch whole (utils.py:872-889,
    1072-1108), with the reference's `data` keys: rays_o, rays_d [H*W, 3], H, W
    (the full-resolution view), rays_o_lr, rays_d_lr, h, w (the feature view)
    and, optionally, index and cam_near_far.

    cache: a teacher.FeatureCache (the Trainer's self.cache) or None.  Once it
    is full, every step but each opt.cache_interval-th takes a cached batch
    with its teacher features (teacher.use_cache_now).  On a miss the
    full-resolution view is rendered under no_grad (staged, perturbed, the
    proposal nets frozen), teacher.set_image_from_render hands it to the
    predictor's image encoder on the device, and the batch goes into the cache
    with its gt_samvit.  Then sam_train_step_fused on the feature rays.
    Returns (pred_samvit, gt_samvit, loss); nothing in the step reads device
    memory on the host."""
    from .teacher import set_image_from_render, use_cache_now
    use_cache = use_cache_now(opt, cache, global_step)
    if use_cache:
        data = cache.get()
    cam_near_far = data["cam_near_far"] if "cam_near_far" in data else None
    if use_cache:
        gt_samvit = data["gt_samvit"]
    else:
        with torch.no_grad():
            rays_o, rays_d = data["rays_o"], data["rays_d"]
            H, W = int(data["H"]), int(data["W"])
            N = rays_o.shape[0]
            bg_color = torch.rand(N, 3, device=rays_o.device) if getattr(opt, "background", None) == "random" else 1
            outputs = model.render(rays_o, rays_d, staged=True, index=data.get("index"), bg_color=bg_color,
                                   perturb=perturb, cam_near_far=cam_near_far, update_proposal=False,
                                   return_feats=0)
            pred_rgb = outputs["image"].reshape(H, W, 3)
            gt_samvit = set_image_from_render(predictor, pred_rgb)
            if opt.cache_size > 0 and cache is not None:
                data["gt_samvit"] = gt_samvit
                cache.insert(data)
    pred_samvit, loss = sam_train_step_fused(renderer, data["rays_o_lr"], data["rays_d_lr"], int(data["h"]),
                                             int(data["w"]), gt_samvit, cam_near_far=cam_near_far)
    return pred_samvit, gt_samvit, loss


def mask_train_step(model, rays_o, rays_d, gt_mask, num_rays=None, cam_near_far=None):
    """Trainer.train_step's --with_mask branch (nerf/utils.py:941-977, 1026):
    render the instance logits (perturb off, proposal nets frozen, white
    background), softmax over instances, clamp to [epsilon, 1 - epsilon], and
    the mean negative log-likelihood of the labels of the first `num_rays`
    rays (the global rays of mixed sampling; no loss if no pixel is labelled,
    label -1 = unlabelled; like the reference, a -1 among the rays that enter
    the gather is an error -- raised here before it can become a device-side
    assert).  The error-map EMA, incoherent-region
    re-weighting, label regularisation and RGB-similarity terms
    (utils.py:978-1065) are options of the data pipeline and are not
    reproduced.  gt_mask: int64 [N] (or [B, N]).  Returns (pred_ids, loss)."""
    opt = model.opt
    gt = gt_mask.reshape(-1).long()
    n = gt.shape[0] if num_rays is None else num_rays
    outputs = model.render(rays_o, rays_d, staged=False, bg_color=1, perturb=False,
                           cam_near_far=cam_near_far, update_proposal=False, return_feats=0,
                           return_mask=1)
    inst = torch.softmax(outputs["instance_mask_logits"], dim=-1)
    pred = inst.view(-1, opt.n_inst)
    pred = torch.clamp(pred, min=opt.epsilon, max=1 - opt.epsilon)
    labeled = gt != -1
    if labeled.sum() > 0:
        if bool((gt[:n] < 0).any()):
            raise RuntimeError("mask_train_step: label -1 inside the gathered rays "
                               "(utils.py:973 gathers with it: index out of bounds)")
        loss = -torch.log(torch.gather(pred[:n], -1, gt[:n, None]))
    else:
        loss = torch.zeros((), dtype=pred.dtype, device=pred.device)
    return pred.argmax(dim=-1), loss.mean()


def mask_train_step_full(model, data, global_step, error_map=None, check_inputs=True):
    """The whole --with_mask branch of Trainer.train_step (nerf/utils.py:941-1070)
    with the reference's `data` keys: rays_o, rays_d, masks [B, N] and, where
    the options ask for them, incoherent_masks (the re-weighting; the sampling
    weights of the RGB-similarity draw without --error_map), error_maps (those
    weights with --error_map), inds_coarse + index (the error map's cells) and
    cam_near_far.  error_map: the Trainer's [images, M * M] tensor
    (self.error_map), updated in place, or None.  The first opt.num_rays rays
    are the global rays, the rest opt.num_local_sample patches of
    opt.local_sample_patch_size ** 2 pixels (--mixed_sampling).

    The render is mask_train_step's; the loss is samnerf_amd.mask_loss: on a
    CUDA model one C call (csrc/mask_loss.hip) for the loss and its gradient
    to the logits, on a CPU model the reference's torch ops.  The only host
    work per step is the RGB-similarity draw (torch.multinomial, as
    utils.py:779-790) and, under check_inputs, one read-back of the count of
    invalid inputs.  Returns (pred_ids, gt_mask, loss) like the reference."""
    from .mask_loss import draw_similarity_samples, mask_loss, rgb_similarity_active
    opt = model.opt
    rays_o, rays_d = data["rays_o"], data["rays_d"]
    gt_mask = data["masks"].to(torch.long)
    cam_near_far = data["cam_near_far"] if "cam_near_far" in data else None
    outputs = model.render(rays_o, rays_d, staged=False, bg_color=1, perturb=False,
                           cam_near_far=cam_near_far, update_proposal=False, return_feats=0,
                           return_mask=1)
    logits = outputs["instance_mask_logits"]
    logits = logits.reshape(-1, logits.shape[-1])
    N = logits.shape[0]
    n = min(int(opt.num_rays), N)
    kw = {}
    if getattr(opt, "incoherent_uncertainty_weight", 1) < 1:
        kw["incoherent"] = data["incoherent_masks"].reshape(-1)
    if error_map is not None:
        index = torch.as_tensor(data["index"], device=logits.device).reshape(-1, 1)
        cells = index * error_map.shape[-1] + data["inds_coarse"].reshape(index.shape[0], -1)
        kw["error_map"], kw["error_cells"] = error_map, cells.reshape(-1)[:n]
    if getattr(opt, "label_regularization_weight", 0) > 0:
        kw["depth"] = outputs["depth"].detach().reshape(-1)
    if rgb_similarity_active(opt, global_step) and getattr(opt, "mixed_sampling", False):
        L, Q = int(opt.num_local_sample), int(opt.local_sample_patch_size) ** 2
        src = data["error_maps"] if getattr(opt, "error_map", False) else data["incoherent_masks"]
        kw["image"] = outputs["image"].detach().reshape(-1, 3)
        kw["sample_index"] = draw_similarity_samples(src.reshape(-1)[n:].view(L, Q),
                                                     int(opt.rgb_similarity_num_sample))
    loss, _, pred_ids = mask_loss(logits, gt_mask.reshape(-1), n, opt, global_step=global_step,
                                  check_inputs=check_inputs, **kw)
    return pred_ids, gt_mask, loss
