#!/usr/bin/env python3
"""For information: what the --with_mask loss costs as torch ops and as
samnerf_mask_loss, at scripts/train_mask.sh's shape: 6,000 global rays + 16
local 16 x 16 patches (10,096 rays), K = 5, the error map on, the RGB-similarity
term on with 20 samples per patch, the adaptive 'density' head with
--sum_after_mlp.

  loss   the loss and d loss / d logits on given logits: (a) the reference's
         torch op sequence (utils.py:961-1065, samnerf_amd.mask_loss's torch
         path) on the GPU + backward, (b) samnerf_mask_loss with its one
         read-back (check_inputs), (c) without it.  The multinomial draw is the
         host's on every path and is not timed here (the steps below draw).
  step   render + loss + backward to the head's weights: mask_train_step_full
         (HIP loss) against the same render with the torch ops around it (what a
         user of the parent commit pastes around its step).
  plain  every optional term off: mask_train_step_full against mask_train_step
         (the parent's step), twice each per round: the second copy of each
         gives the round's own spread.

Per variant and round: HIP events around `reps` calls and the shader clock of
those calls (two samnerf_clock_stamp launches); the variants alternate within
a round.  One JSON line per (variant, round), then a summary line.
usage (GPU box): python tools/mask_loss_time.py [rounds] [reps]"""
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "segment-anything-nerf_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402

N_GLOBAL, L, SIDE, S, K, M = 6000, 16, 16, 20, 5, 128


def main():
    from nerf.network import NeRFNetwork, default_opt
    from samnerf_amd import _lib, ops, synth
    from samnerf_amd.mask_loss import draw_similarity_samples, mask_loss, torch_mask_loss
    from samnerf_amd.train import mask_train_step, mask_train_step_full
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 4
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 30
    dev = torch.device("cuda", 0)
    cur = torch.cuda.current_stream()
    Q = SIDE * SIDE
    N = N_GLOBAL + L * Q
    spec = synth.ModelSpec(with_sam=False, with_mask=True, mask_type="adaptive", adaptive_type="density",
                           n_inst=K, sum_after_mlp=True)
    params = synth.make_params(spec, seed=5, emb_scale=0.5)
    net = NeRFNetwork(default_opt(with_sam=False, with_mask=True, mask_mlp_type="adaptive",
                                  adaptive_mlp_type="density", n_inst=K, sum_after_mlp=True))
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in params.items()})
    net = net.to(dev).train()
    for k, p in net.named_parameters():
        p.requires_grad = k.startswith("mask_mlp")
    opt = net.opt
    opt.num_rays, opt.adaptive_num_rays = N_GLOBAL, False
    script = dict(mixed_sampling=True, num_local_sample=L, local_sample_patch_size=SIDE,
                  rgb_similarity_loss_weight=5.0, rgb_similarity_threshold=0.15, rgb_similarity_num_sample=S,
                  rgb_similarity_iter=-1, rgb_similarity_exp_weight=10.0, error_map=True,
                  incoherent_uncertainty_weight=1.0, label_regularization_weight=0.0, patch_size=1)

    def configure(on):
        for k, v in script.items():
            setattr(opt, k, v)
        if not on:
            opt.rgb_similarity_loss_weight, opt.error_map = 0.0, False

    g = torch.Generator().manual_seed(6)
    pose, intr = synth.gui_camera(512, 512)
    ro, rd = ops.get_rays(pose, intr, 512, 512, device=dev)
    inds = torch.randint(0, 512 * 512, (N,), generator=g).to(dev)
    inc = torch.rand(N, generator=g).to(dev)
    data = {"rays_o": ro[inds].contiguous(), "rays_d": rd[inds].contiguous(),
            "masks": torch.randint(0, K, (1, N), generator=g).to(dev), "incoherent_masks": (inc > 0.5).float(),
            "error_maps": inc * 0.5, "index": [1],
            "inds_coarse": torch.randint(0, M * M, (1, N_GLOBAL), generator=g).to(dev)}
    emap = torch.rand(2, M * M, generator=g).to(dev)
    configure(True)
    draw = draw_similarity_samples(data["error_maps"][N_GLOBAL:].view(L, Q), S)
    with torch.no_grad():
        out = net.render(data["rays_o"], data["rays_d"], staged=False, bg_color=1, perturb=False,
                         update_proposal=False, return_feats=0, return_mask=1)
    logits0 = out["instance_mask_logits"].detach().reshape(N, K).contiguous()
    image = out["image"].detach()
    labels = data["masks"].reshape(-1)
    cells = (M * M + data["inds_coarse"]).reshape(-1)
    kw = dict(error_map=emap, error_cells=cells, image=image, sample_index=draw, global_step=1)

    def loss_only(which):
        z = logits0.clone().requires_grad_(True)
        if which == "torch":
            loss = torch_mask_loss(z, labels, N_GLOBAL, opt, **kw)[0]
        else:
            loss = mask_loss(z, labels, N_GLOBAL, opt, check_inputs=which == "hip_checked", **kw)[0]
        loss.backward()

    def render_torch_glue():
        """The parent's render with the reference's torch ops around it."""
        o = net.render(data["rays_o"], data["rays_d"], staged=False, bg_color=1, perturb=False,
                       update_proposal=False, return_feats=0, return_mask=1)
        drawn = draw_similarity_samples(data["error_maps"][N_GLOBAL:].view(L, Q), S)
        return torch_mask_loss(o["instance_mask_logits"].reshape(N, K), labels, N_GLOBAL, opt,
                               **dict(kw, image=o["image"].detach(), sample_index=drawn))[0]

    def step(which):
        net.zero_grad(set_to_none=True)
        if which == "full":
            loss = mask_train_step_full(net, data, 1, error_map=emap)[2]
        elif which == "torch_glue":
            loss = render_torch_glue()
        elif which == "plain_full":
            loss = mask_train_step_full(net, data, 1)[2]
        else:
            loss = mask_train_step(net, data["rays_o"], data["rays_d"], data["masks"], num_rays=N_GLOBAL)[1]
        loss.backward()

    def stamp(buf):
        _lib.lib().samnerf_clock_stamp(ctypes.c_void_p(buf.data_ptr()), ctypes.c_void_p(cur.cuda_stream))

    def timed(fn, n):
        stamps = torch.zeros(2, 768, dtype=torch.int64, device=dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        stamp(stamps[0])
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        stamp(stamps[1])
        torch.cuda.synchronize()
        clock = bench.timed_clock(stamps.cpu().numpy())
        return e0.elapsed_time(e1) / n, clock["ghz"] if clock else None

    groups = [
        ("loss", True, [("torch", lambda: loss_only("torch")), ("hip_checked", lambda: loss_only("hip_checked")),
                        ("hip", lambda: loss_only("hip"))]),
        ("step", True, [("torch_glue", lambda: step("torch_glue")), ("full", lambda: step("full"))]),
        ("plain", False, [("mask_train_step", lambda: step("plain")), ("full", lambda: step("plain_full")),
                          ("mask_train_step_2", lambda: step("plain")), ("full_2", lambda: step("plain_full"))]),
    ]
    ms = {}
    for what, on, variants in groups:
        configure(on)
        for _, fn in variants:
            for _ in range(3):
                fn()
        for rnd in range(1, rounds + 1):
            for name, fn in variants:
                t, ghz = timed(fn, reps)
                ms.setdefault((what, name), []).append(t)
                print(json.dumps({"what": what, "variant": name, "round": rnd, "ms_per_call": round(t, 4),
                                  "clock_ghz": None if ghz is None else round(ghz, 4)}), flush=True)
    mean = {f"{w}/{n}": round(statistics.mean(v), 4) for (w, n), v in ms.items()}
    spread = max(abs(mean["plain/mask_train_step"] - mean["plain/mask_train_step_2"]),
                 abs(mean["plain/full"] - mean["plain/full_2"]))
    new = (mean["plain/full"] + mean["plain/full_2"]) / 2
    old = (mean["plain/mask_train_step"] + mean["plain/mask_train_step_2"]) / 2
    print(json.dumps({"what": "summary", "rays": N, "rounds": rounds, "reps": reps, "mean_ms": mean,
                      "plain_new_minus_parent_ms": round(new - old, 4), "plain_spread_ms": round(spread, 4)}))


if __name__ == "__main__":
    main()
