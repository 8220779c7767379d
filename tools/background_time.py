#!/usr/bin/env python3
"""For information: what the transparent background modes cost on the fused
path and what the unfused path they used to fall back to costs.  Times, on
the parity-weight scene with --background white / random,
  * the 512 x 512 view with a [3] background colour (NeRFRenderer.render,
    staged=False, return_feats=1) through the fused kernels and through
    run_torch, and the same view under 'last_sample' on the fused kernels;
  * one 4,096-ray RGB training step with a per-ray background
    (rgb_train_step_fused against rgb_train_step on run_torch + autograd).
Wall time per call between two synchronisations, the median of `reps` calls
after `warm`.  Prints one JSON line.
usage (GPU box): python tools/background_time.py [reps] [warm]"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "segment-anything-nerf_amd"))

import torch  # noqa: E402

import bench  # noqa: E402


def median_ms(fn, reps, warm):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(ts), 4)


def main():
    from samnerf_amd import ops, synth
    from samnerf_amd.train import rgb_train_step, rgb_train_step_fused
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    warm = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    dev = torch.device("cuda", 0)
    H = W = 512
    pose, intr = synth.gui_camera(W, H)
    ro, rd = ops.get_rays(pose, intr, H, W, device=dev)
    colour = torch.tensor([0.2, 0.5, 0.9], device=dev)
    out = {"what": "median wall ms per call between synchronisations", "reps": reps, "warm": warm}
    net, _, _ = bench.build_net(True, dev, emb_scale=0.5)

    def view(fused, background):
        net.opt.background, net.fused = background, fused
        with torch.no_grad():
            return net.render(ro, rd, staged=False, bg_color=colour, return_feats=1, H=H, W=W)
    out["view_512_white_fused_ms"] = median_ms(lambda: view(True, "white"), reps, warm)
    out["view_512_last_sample_fused_ms"] = median_ms(lambda: view(True, "last_sample"), reps, warm)
    out["view_512_white_run_torch_ms"] = median_ms(lambda: view(False, "white"), max(reps // 3, 2), 1)
    out["view_512_weights_sum_mean_white"] = float(view(True, "white")["weights_sum"].mean())
    del net
    torch.cuda.empty_cache()

    rgb, _, _ = bench.build_net(False, dev, emb_scale=0.5)
    rgb.train()
    rgb.opt.background = "random"
    g = torch.Generator().manual_seed(1)
    idx = torch.randperm(H * W, generator=g)[:4096].to(dev)
    so, sd = ro[idx].contiguous(), rd[idx].contiguous()
    gt = torch.rand(4096, 4, generator=g).to(dev)
    bg = torch.rand(4096, 3, generator=g).to(dev)

    def fused_step():
        rgb.zero_grad(set_to_none=True)
        rgb_train_step_fused(rgb, so, sd, gt, global_step=1, bg_color=bg)

    def torch_step():
        rgb.zero_grad(set_to_none=True)
        rgb.fused = False
        try:
            rgb_train_step(rgb, so, sd, gt, global_step=1, bg_color=bg)[1].backward()
        finally:
            rgb.fused = True
    out["rgb_step_4096_random_fused_ms"] = median_ms(fused_step, reps, warm)
    out["rgb_step_4096_random_run_torch_ms"] = median_ms(torch_step, max(reps // 3, 2), 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
