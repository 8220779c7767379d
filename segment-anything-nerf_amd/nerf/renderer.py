"""NeRFRenderer on gfx950 -- interface of nerf/renderer.py:142-464.

`run()` keeps the reference's keyword interface (bg_color, perturb,
cam_near_far, update_proposal, return_feats, return_mask, H, W) and by default
executes the whole ray-march loop as the fused HIP pipeline
(samnerf_amd.fused, raymarch.hip).  `run_torch()` is the reference's own
unfused op sequence on the GPU with the drop-in encoders -- the
"reference-equivalent" single-GPU baseline of BASELINE.md and the path for
options the fused kernels do not cover (training-mode bookkeeping and
autograd).  Perturbed sampling runs fused: the perturbed positions are drawn
with torch's generator in the reference's order (fused.perturbed_positions),
or -- perturb_rng = "philox", opt-in -- inside the kernels from a seed and a
per-call counter (fused.PhiloxPerturb: statistically the same sampling, not
torch's stream; no position arrays).
Staged rendering chunks rays like renderer.py:185-219 but,
unlike the reference, also works with return_feats (flat [N,256] rows are
reshaped once at the end, fixing the SURVEY.md 0.3 crash).
"""
import math

import torch
import torch.nn as nn


def near_far_from_aabb(rays_o, rays_d, aabb, min_near=0.05):
    """renderer.py:122-139 on torch tensors."""
    tmin = (aabb[:3] - rays_o) / (rays_d + 1e-15)
    tmax = (aabb[3:] - rays_o) / (rays_d + 1e-15)
    near = torch.where(tmin < tmax, tmin, tmax).amax(dim=-1, keepdim=True)
    far = torch.where(tmin > tmax, tmin, tmax).amin(dim=-1, keepdim=True)
    miss = far < near
    near[miss] = 1e9
    far[miss] = 1e9
    return torch.clamp(near, min=min_near), far


def contract(x):
    """renderer.py:60-69: L-inf contraction of R^3 into [-2, 2]^3."""
    shape, C = x.shape[:-1], x.shape[-1]
    x = x.view(-1, C)
    mag, idx = x.abs().max(1, keepdim=True)
    scale = 1 / mag.repeat(1, C)
    scale.scatter_(1, idx, (2 - 1 / mag) / mag)
    return torch.where(mag < 1, x, x * scale).view(*shape, C)


def sample_pdf(bins, weights, T, perturb=False):
    """renderer.py:84-119: inverse-CDF resampling of T positions."""
    N, T0 = weights.shape
    weights = weights + 0.01
    pdf = weights / torch.sum(weights, -1, keepdim=True)
    cdf = torch.cumsum(pdf, -1).clamp(max=1)
    cdf = torch.cat([torch.zeros_like(cdf[..., :1]), cdf], -1)
    u = torch.linspace(0.5 / T, 1 - 0.5 / T, steps=T).to(weights.device).expand(N, T)
    if perturb:
        u = u + (torch.rand_like(u) - 0.5) / T
    u = u.contiguous()
    inds = torch.searchsorted(cdf, u, right=True)
    below = torch.clamp(inds - 1, 0, T0)
    above = torch.clamp(inds, 0, T0)
    c0, c1 = torch.gather(cdf, -1, below), torch.gather(cdf, -1, above)
    b0, b1 = torch.gather(bins, -1, below), torch.gather(bins, -1, above)
    t = torch.clamp(torch.nan_to_num((u - c0) / (c1 - c0)), 0, 1)
    return b0 + t * (b1 - b0)


def eff_distloss(w, m, interval):
    """Distortion loss sum_ij w_i w_j |m_i - m_j| + 1/3 sum_i w_i^2 s_i, mean over
    rays, in its O(T) cumulative-sum form.  Restates the third-party
    `torch_efficient_distloss.eff_distloss` the reference calls
    (renderer.py:14, 25; requirements.txt:22, un-pinned, absent here): parity
    unpinned, tests/test_losses.py checks it against the double sum."""
    loss_uni = (1 / 3) * (interval * w.pow(2)).sum(dim=-1).mean()
    wm = w * m
    w_cumsum = w.cumsum(dim=-1)
    wm_cumsum = wm.cumsum(dim=-1)
    loss_bi_0 = wm[..., 1:] * w_cumsum[..., :-1]
    loss_bi_1 = w[..., 1:] * wm_cumsum[..., :-1]
    loss_bi = 2 * (loss_bi_0 - loss_bi_1).sum(dim=-1).mean()
    return loss_bi + loss_uni


def distort_loss(bins, weights):
    """renderer.py:17-27: bins [N, T+1], weights [N, T]."""
    intervals = bins[..., 1:] - bins[..., :-1]
    mid_points = bins[..., :-1] + intervals / 2
    return eff_distloss(weights, mid_points, intervals)


def proposal_loss(all_bins, all_weights):
    """renderer.py:30-57 (mip-NeRF 360 inter-level loss): the final stage's
    (detached) weights must be bounded by each proposal stage's."""
    def loss_interlevel(t0, w0, t1, w1):
        cw1 = torch.cat([torch.zeros_like(w1[..., :1]), torch.cumsum(w1, dim=-1)], dim=-1)
        inds_lo = (torch.searchsorted(t1[..., :-1].contiguous(), t0[..., :-1].contiguous(),
                                      right=True) - 1).clamp(0, w1.shape[-1] - 1)
        inds_hi = torch.searchsorted(t1[..., 1:].contiguous(), t0[..., 1:].contiguous(),
                                     right=True).clamp(0, w1.shape[-1] - 1)
        cw1_lo = torch.take_along_dim(cw1[..., :-1], inds_lo, dim=-1)
        cw1_hi = torch.take_along_dim(cw1[..., 1:], inds_hi, dim=-1)
        w = cw1_hi - cw1_lo
        return (w0 - w).clamp(min=0) ** 2 / (w0 + 1e-8)

    bins_ref = all_bins[-1].detach()
    weights_ref = all_weights[-1].detach()
    loss = 0
    for bins, weights in zip(all_bins[:-1], all_weights[:-1]):
        loss += loss_interlevel(bins_ref, weights_ref, bins, weights).mean()
    return loss


def _spacing(x):
    return torch.where(x < 1, x / 2, 1 - 1 / (2 * x))


def _spacing_inv(x):
    return torch.where(x < 0.5, 2 * x, 1 / (2 - 2 * x))


class NeRFRenderer(nn.Module):
    def __init__(self, opt):
        super().__init__()
        self.opt = opt
        self.real_bound = opt.bound
        self.bound = 2 if opt.contract else opt.bound
        self.cascade = 1 + math.ceil(math.log2(self.bound))
        self.min_near = opt.min_near
        self.density_thresh = getattr(opt, "density_thresh", 10)
        box = torch.FloatTensor([-self.real_bound] * 3 + [self.real_bound] * 3)
        self.register_buffer("aabb_train", box)
        self.register_buffer("aabb_infer", box.clone())
        self.fused = True          # fused HIP pipeline for eligible calls
        self._fused = None
        # fused path: GEMM precision (0 = f16x3, fp32-equivalent; 1 = exact fp32
        # MFMA) and the flagged non-parity early exit N1 (0 = off, the
        # reference's semantics); read by samnerf_amd.fused.FusedRenderer
        self.head_mode = 0
        self.t_thresh = 0.0
        # perturb=True on the fused paths: "torch" (default) draws the positions
        # with torch's generator as the reference does; "philox" has the kernels
        # draw them from PhiloxPerturb(perturb_seed, k), k counting this
        # renderer's dispatched fused calls (staged chunks and successive training
        # steps draw differently).  run_torch always draws with torch.
        self.perturb_rng = "torch"
        self.perturb_seed = 0
        self._perturb_calls = 0

    def forward(self, x, d, **kwargs):
        raise NotImplementedError()

    def density(self, x, **kwargs):
        raise NotImplementedError()

    def update_aabb(self, aabb):
        if not torch.is_tensor(aabb):
            aabb = torch.from_numpy(aabb).float()
        self.aabb_train = aabb.clamp(-self.real_bound, self.real_bound).to(self.aabb_train.device)
        self.aabb_infer = self.aabb_train.clone()

    # ------------------------------------------------------------ render --
    def render(self, rays_o, rays_d, staged=False, cam_near_far=None, **kwargs):
        if not staged:
            return self.run(rays_o, rays_d, cam_near_far=cam_near_far, **kwargs)
        N = rays_o.shape[0]
        H, W = kwargs.pop("H", None), kwargs.pop("W", None)
        bg = kwargs.pop("bg_color", None)
        per_ray_bg = torch.is_tensor(bg) and bg.dim() == 2 and bg.shape[0] == N and N != 1
        results = {}
        step = self.opt.max_ray_batch
        for head in range(0, N, step):
            tail = min(head + step, N)
            cnf = cam_near_far
            if cnf is not None and cnf.shape[0] != 1:
                cnf = cnf[head:tail]
            # a per-ray background [N,3] / [N,1] is sliced with the rays; a
            # scalar or one [3] / [1,3] colour goes to every chunk
            bgk = bg[head:tail] if per_ray_bg else bg
            # chunks of whole image rows keep the ray-tiling hint (W only: the
            # chunk's samvit stays flat)
            wk = W if (W is not None and step % W == 0) else None
            part = self.run(rays_o[head:tail], rays_d[head:tail], cam_near_far=cnf, W=wk, bg_color=bgk,
                            **kwargs)
            for k, v in part.items():
                if v is None:
                    continue
                if torch.is_tensor(v):
                    v = v.reshape(tail - head, *v.shape[1:]) if k != "samvit" else v.reshape(tail - head, -1)
                    if k not in results:
                        results[k] = torch.empty(N, *v.shape[1:], device=rays_o.device)
                    results[k][head:tail] = v
                else:
                    results[k] = v
        if "samvit" in results and H is not None and kwargs.get("return_feats", 0):
            results["samvit"] = results["samvit"].view(H, W, -1)
        return results

    @staticmethod
    def _fused_bg_ok(bg_color, N):
        """A background the fused kernels take: a number, a 1-element tensor,
        one [3] / [1,3] colour or anything that broadcasts against [N,3] --
        without gradient (none is produced for the colour)."""
        if not torch.is_tensor(bg_color):
            return True
        if bg_color.requires_grad and torch.is_grad_enabled():
            return False
        from samnerf_amd.fused import bg_layout
        try:
            bg_layout(bg_color.detach(), N)
        except ValueError:
            return False
        return True

    def _fused_ok(self, rays_o, perturb, return_mask, kwargs, bg_color=None):
        if return_mask:
            from samnerf_amd.fused import mask_kind
            if mask_kind(self) is None:
                return False                 # the other mask heads: unfused path
        # training mode only for no-grad renders without the train-mode extras
        # (renderer.py:348-356 adds them only without SAM and masks): the SAM
        # distillation's teacher render, utils.py:1078-1079
        train_ok = not self.training or (not torch.is_grad_enabled() and (
            self.opt.with_sam or getattr(self.opt, "with_mask", False)))
        return (self.fused and rays_o.is_cuda and train_ok
                and self._fused_bg_ok(bg_color, rays_o.shape[0])
                # sum_after_mlp: RGB (+ mask) models on the fused path; with SAM
                # the reference's branch crashes and run_torch raises
                and not (getattr(self.opt, "sum_after_mlp", False) and self.opt.with_sam)
                and list(self.opt.num_steps) == [128, 64, 32]
                and (not self.opt.with_sam or self.opt.sam_use_view_direction))

    def _fused_train_ok(self, rays_o, bg_color, return_feats, return_mask):
        """Train mode under grad for an RGB model (renderer.py:348-356's case):
        the HIP training kernels (samnerf_amd.fused.render_rgb_train)."""
        o = self.opt
        return (self.fused and rays_o.is_cuda and self.training and torch.is_grad_enabled()
                and not o.with_sam and not getattr(o, "with_mask", False)
                and not getattr(o, "sum_after_mlp", False) and not return_feats and not return_mask
                and list(o.num_steps) == [128, 64, 32]
                and self._fused_bg_ok(bg_color, rays_o.shape[0]))

    def _fused_mask_train_ok(self, rays_o, bg_color, perturb, return_feats, return_mask):
        """Train mode under grad with return_mask=1 for a fused mask head --
        'default', 'adaptive' / 'density' (the reference's scripts/train_mask.sh)
        or 'adaptive' / 'rgb' with sum_after_mlp (the --with_mask step,
        utils.py:946-948): the HIP mask-head training kernels
        (samnerf_amd.fused.render_mask_train)."""
        o = self.opt
        if not (return_mask and not return_feats and getattr(o, "with_mask", False)):
            return False
        from samnerf_amd.fused import mask_kind
        return (mask_kind(self) is not None and self.fused and rays_o.is_cuda
                and self.training and torch.is_grad_enabled() and not perturb
                and not (getattr(o, "sum_after_mlp", False) and o.with_sam)
                and list(o.num_steps) == [128, 64, 32]
                and (not o.with_sam or o.sam_use_view_direction)
                and (not torch.is_tensor(bg_color) or (bg_color.numel() == 1 and not bg_color.requires_grad)))

    def _fused_perturb(self, perturb):
        """What a dispatched fused call gets as perturb=: the caller's value, or
        under perturb_rng = "philox" the seeded source of this call for a plain
        perturb=True.  Every dispatched call advances the counter."""
        if self.perturb_rng not in ("torch", "philox"):
            raise ValueError(f"perturb_rng {self.perturb_rng!r}: 'torch' or 'philox'")
        k = self._perturb_calls
        self._perturb_calls = k + 1
        if self.perturb_rng == "philox" and perturb and not isinstance(perturb, (tuple, list)):
            from samnerf_amd.fused import PhiloxPerturb
            if not isinstance(perturb, PhiloxPerturb):
                return PhiloxPerturb(int(self.perturb_seed), k)
        return perturb

    def run(self, rays_o, rays_d, bg_color=None, perturb=False, cam_near_far=None,
            update_proposal=True, return_feats=0, return_mask=0, H=None, W=None, **kwargs):
        if self._fused_mask_train_ok(rays_o, bg_color, perturb, return_feats, return_mask):
            from samnerf_amd.fused import FusedRenderer, render_mask_train
            if self._fused is None or self._fused.net is not self:
                self._fused = FusedRenderer(self)
            return render_mask_train(self._fused, rays_o, rays_d, cam_near_far, bg_color)
        if self._fused_train_ok(rays_o, bg_color, return_feats, return_mask):
            from samnerf_amd.fused import FusedRenderer, render_rgb_train
            if self._fused is None or self._fused.net is not self:
                self._fused = FusedRenderer(self)
            return render_rgb_train(self._fused, rays_o, rays_d, cam_near_far, bg_color,
                                    self._fused_perturb(perturb), update_proposal)
        if self._fused_ok(rays_o, perturb, return_mask, kwargs, bg_color):
            from samnerf_amd.fused import FusedRenderer
            if self._fused is None or self._fused.net is not self:
                self._fused = FusedRenderer(self)
            n = rays_o.shape[0]
            vw = W if (W is not None and n % W == 0) else 0      # a whole number of image rows
            out = self._fused.render(rays_o, rays_d, cam_near_far, bg_color,
                                     feats=return_feats > 0, view_width=vw, mask=return_mask > 0,
                                     perturb=self._fused_perturb(perturb))
            samvit = out.pop("samvit", None)
            if return_feats > 0 and samvit is not None:
                out["samvit"] = samvit.view(H, W, -1) if H is not None else samvit
            return out
        return self.run_torch(rays_o, rays_d, bg_color=bg_color, perturb=perturb,
                              cam_near_far=cam_near_far, update_proposal=update_proposal,
                              return_feats=return_feats, return_mask=return_mask, H=H, W=W)

    def run_torch(self, rays_o, rays_d, bg_color=None, perturb=False, cam_near_far=None,
                  update_proposal=True, return_feats=0, return_mask=0, H=None, W=None, **kwargs):
        """The reference's unfused op sequence (renderer.py:221-464) with the
        HIP drop-in encoders: ~350 small kernels per call.  Covers what the
        fused kernels do not: training-mode extras and autograd, the
        'lightweight_mask' / adaptive 'sam' heads, sum_after_mlp with SAM."""
        opt = self.opt
        with_mask = getattr(opt, "with_mask", False)
        mask_type = getattr(opt, "mask_mlp_type", "default")
        sum_after = getattr(opt, "sum_after_mlp", False)
        save_ir = with_mask and mask_type == "adaptive"
        rays_o = rays_o.contiguous()
        rays_d = rays_d.contiguous()
        N = rays_o.shape[0]
        dev = rays_o.device
        nears, fars = near_far_from_aabb(rays_o, rays_d,
                                         self.aabb_train if self.training else self.aabb_infer,
                                         self.min_near)
        if cam_near_far is not None:
            nears = torch.maximum(nears, cam_near_far[:, [0]])
            fars = torch.minimum(fars, cam_near_far[:, [1]])
        if bg_color is None:
            bg_color = 1
        results = {}
        s_n, s_f = _spacing(nears), _spacing(fars)
        bins = weights = None
        all_bins, all_weights = [], []
        for it, T in enumerate(opt.num_steps):
            if it == 0:
                bins = torch.linspace(0, 1, T + 1, device=dev).unsqueeze(0).expand(N, -1)
                if perturb:
                    bins = (bins + (torch.rand_like(bins) - 0.5) / T).clamp(0, 1)
            else:
                bins = sample_pdf(bins, weights, T + 1, perturb).detach()
            real_bins = _spacing_inv(s_n * (1 - bins) + s_f * bins)
            rays_t = (real_bins[..., 1:] + real_bins[..., :-1]) / 2
            xyzs = rays_o.unsqueeze(1) + rays_d.unsqueeze(1) * rays_t.unsqueeze(2)
            if opt.contract:
                xyzs = contract(xyzs)
            if it != len(opt.num_steps) - 1:
                with torch.set_grad_enabled(update_proposal):
                    sigmas = self.density(xyzs, proposal=it)["sigma"]
            else:
                dirs = rays_d.view(-1, 1, 3).expand_as(xyzs)
                dirs = dirs / torch.norm(dirs, dim=-1, keepdim=True)
                outputs = self(xyzs, dirs, save_intermedian_results=save_ir)
                sigmas, colors = outputs["sigma"], outputs["color"]
                if opt.with_sam:
                    features = self.s_grid(xyzs, bound=self.bound)
                if return_mask > 0 and mask_type in ("default", "lightweight_mask"):
                    masks = self.m_grid(xyzs, bound=self.bound)
            ds = (real_bins[..., 1:] - real_bins[..., :-1]) * sigmas
            if opt.background == "last_sample":
                ds = torch.cat([ds[..., :-1], torch.full_like(ds[..., -1:], torch.inf)], dim=-1)
            alphas = 1 - torch.exp(-ds)
            trans = torch.cumsum(ds[..., :-1], dim=-1)
            trans = torch.exp(-torch.cat([torch.zeros_like(trans[..., :1]), trans], dim=-1))
            weights = alphas * trans
            weights.nan_to_num_(0)
            if self.training:
                all_bins.append(bins)
                all_weights.append(weights)
        weights_sum = weights.sum(-1)
        depth = (weights * rays_t).sum(-1)
        f_image = (weights.unsqueeze(-1) * colors).sum(-2)
        if sum_after:                                        # renderer.py:339-342
            f_colors = self.view_mlp(colors, save_intermedian_results=save_ir)
            image = torch.sigmoid((weights.unsqueeze(-1) * f_colors).sum(-2))
        else:
            image = torch.sigmoid(self.view_mlp(f_image, save_intermedian_results=save_ir))
        if self.training and not with_mask and not opt.with_sam:       # renderer.py:348-356
            results["num_points"] = xyzs.shape[0] * xyzs.shape[1]
            results["weights"] = weights
            if getattr(opt, "lambda_proposal", 0) > 0 and update_proposal:
                results["proposal_loss"] = proposal_loss(all_bins, all_weights)
            if getattr(opt, "lambda_distort", 0) > 0:
                results["distort_loss"] = distort_loss(bins, weights)
        image = image + (1 - weights_sum).unsqueeze(-1) * bg_color
        results.update(weights_sum=weights_sum, depth=depth, image=image)
        if opt.with_sam:
            if sum_after:
                raise NotImplementedError("with_sam + sum_after_mlp: the reference's branch crashes "
                                          "(renderer.py:371-372, SURVEY.md 0.2)")
            f_sam = (weights.unsqueeze(-1) * features).sum(-2)
            f = torch.cat([f_sam, f_image, image, depth.unsqueeze(-1)], dim=-1)
            samvit = self.samvit_mlp(f)
            if return_feats > 0:
                results["samvit"] = samvit.view(H, W, -1) if H is not None else samvit
        if return_mask > 0:                                  # renderer.py:392-454
            point_masks = self.mask_logits(masks if mask_type in ("default", "lightweight_mask")
                                           else None, outputs, colors)
            results["instance_mask_logits"] = (weights.detach().unsqueeze(-1) * point_masks).sum(-2)
        return results
