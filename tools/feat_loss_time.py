#!/usr/bin/env python3
"""What the distillation step costs with the loss as torch ops and with
samnerf_amd.feat_loss (GPU box).

The step is bench.py's config 5: the fused forward of the feature rays with
grad, the loss against a N(0,1) [1,256,64,64] target (seed 1), backward (HIP
s_grid scatter + HIP head), FusedAdam(lr 1e-2, eps 1e-15) with the RGB
parameters frozen.  Two view sizes: 64 x 64 (4,096 rays; the resize is the
identity) and 49 x 66 (3,234 rays; what a 738 x 994 image gives, resized to
64 x 64).  Paths:

  torch_a, torch_b   train.sam_train_step: permute + F.interpolate + mse_loss
                     and their autograd backward -- the yardstick, timed twice
                     so that its own run-to-run spread is known
  feat_loss          train.sam_train_step_fused: csrc/feat_loss.hip

Every path trains its own copy of the same net, so no path sees another's
updates.  Paths are timed in interleaved rounds in rotating order, so clock and
thermal drift hit every path.  Per path and round: HIP events on the current
stream around `--steps` steps after a warm-up, and the host clock around the
same steps ending in a device synchronise.

Prints one JSON line per measurement and a summary per shape; --out appends
them to a file (profiles/feat_loss_time.jsonl).
usage: python tools/feat_loss_time.py [--rounds 5] [--steps 200] [--deterministic] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "segment-anything-nerf_amd"))

ORDER = ("torch_a", "feat_loss", "torch_b")


def make_step(dev, h, w, fused, deterministic):
    from nerf.network import NeRFNetwork, default_opt
    from samnerf_amd import ops, synth
    from samnerf_amd.fused import FusedRenderer
    from samnerf_amd.optim import FusedAdam
    from samnerf_amd.train import sam_train_step, sam_train_step_fused
    spec = synth.ModelSpec(with_sam=True)
    params = synth.make_params(spec, seed=0, emb_scale=1e-4, ln_jitter=0.0)      # bench.py build_net
    net = NeRFNetwork(default_opt(with_sam=True))
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in params.items()})
    net = net.to(dev).train()
    for k, p in net.named_parameters():
        p.requires_grad = k.startswith("s_grid") or k.startswith("samvit_mlp")
    opt = FusedAdam([p for p in net.parameters() if p.requires_grad], lr=1e-2, eps=1e-15)
    renderer = FusedRenderer(net, deterministic=deterministic)
    pose, intr = synth.gui_camera(w, h)
    ro, rd = ops.get_rays(pose, intr, h, w, device=dev)
    gt = torch.randn(1, 256, 64, 64, generator=torch.Generator(device="cpu").manual_seed(1)).to(dev)
    last = {}

    def step():
        # both render in ray order (view_width 0, all sam_train_step offers):
        # the paths differ in the loss alone
        _, loss = (sam_train_step_fused if fused else sam_train_step)(renderer, ro, rd, h, w, gt)
        loss.backward()
        opt.step()
        opt.zero_grad(set_to_none=True)
        last["loss"] = loss
    return step, last


def shape(dev, h, w, rounds, steps, deterministic, emit):
    tags = dict(view=[h, w], rays=h * w, target=[64, 64], deterministic=deterministic)
    fns, lasts = {}, {}
    for path in ORDER:
        fns[path], lasts[path] = make_step(dev, h, w, path == "feat_loss", deterministic)
    first = {}
    for path, f in fns.items():                           # warm-up: code objects, allocator, Adam state
        f()
        first[path] = float(lasts[path]["loss"].detach())
        for _ in range(9):
            f()
    torch.cuda.synchronize()
    per = {p: [] for p in ORDER}
    for r in range(rounds):
        for k in range(len(ORDER)):
            path = ORDER[(k + r) % len(ORDER)]
            f = fns[path]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            for _ in range(steps):
                f()
            e1.record()
            torch.cuda.synchronize()
            wall = (time.perf_counter() - t0) / steps * 1e3
            ev = e0.elapsed_time(e1) / steps
            per[path].append(ev)
            emit(dict(kind="round", path=path, round=r, steps=steps, event_ms=ev, wall_ms=wall, **tags))
    mean = {p: float(np.mean(v)) for p, v in per.items()}
    spread = max(abs(mean["torch_a"] - mean["torch_b"]),
                 float(np.max(np.abs(np.array(per["torch_a"]) - np.array(per["torch_b"])))))
    torch_ms = 0.5 * (mean["torch_a"] + mean["torch_b"])
    emit(dict(kind="summary", event_ms_mean=mean, torch_ms=torch_ms, aa_spread_ms=spread,
              feat_loss_round_spread_ms=float(np.max(per["feat_loss"]) - np.min(per["feat_loss"])),
              feat_loss_over_torch=mean["feat_loss"] / torch_ms,
              not_slower_beyond_spread=bool(mean["feat_loss"] - torch_ms <= spread),
              first_step_loss=first, **tags))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--deterministic", action="store_true", help="FusedRenderer(deterministic=True)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("feat_loss_time: needs the GPU; a CPU run measures nothing")
    dev = torch.device("cuda:0")
    out = open(a.out, "a") if a.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()
    for h, w in ((64, 64), (49, 66)):
        shape(dev, h, w, a.rounds, a.steps, a.deterministic, emit)


if __name__ == "__main__":
    main()
