#!/usr/bin/env python3
"""What evaluating one rendered view costs, by path (GPU box).

samnerf_amd.evaluate.eval_frame -- the HIP kernels, the result left in a device
stats record -- against torch_eval_frame, the reference's own op sequence on
the same GPU with its host copies, numpy passes and per-class Python loop, per
512 x 512 view on synthetic render outputs:

  rgb       loss + PSNR + SSIM + the three uint8 images (RGBA truth)
  mask_k5   loss + argmax + mIoU at K = 5
  mask_k33  the same at K = 33

Paths: hip; twin_a and twin_b, the mirror timed twice so that its own
run-to-run spread is known.  Rounds are interleaved in rotating order, so clock
and thermal drift hit every path.  Per path and round: the host clock around
`--steps` views ending in a device synchronise, and HIP events around the same
views.  The kernel path's one copy of the stats table per epoch is timed apart
(`read_ms`: 100 records).

Prints one JSON line per measurement and a summary per workload; --out appends
them to a file (profiles/eval_time.jsonl).
usage: python tools/eval_time.py [--rounds 5] [--steps 50] [--out FILE]
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

H = W = 512
PATHS = ("hip", "twin_a", "twin_b")


def workloads(dev):
    g = torch.Generator().manual_seed(5)
    out = {"rgb": ((torch.rand(H * W, 3, generator=g).to(dev), torch.rand(H, W, 4, generator=g).to(dev)),
                   dict(buffers=True))}
    for K in (5, 33):
        out[f"mask_k{K}"] = ((), dict(logits=(2 * torch.randn(H, W, K, generator=g)).to(dev),
                                      labels=torch.randint(-1, K, (H, W), generator=g).to(dev), n_inst=K,
                                      epsilon=1e-6, n_classes=K))
    return out


def main():
    from samnerf_amd.evaluate import Evaluator, eval_frame, read_stats, torch_eval_frame
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU; there is nothing to time without one"
    dev = torch.device("cuda", 0)
    lines = []

    def emit(rec):
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    for name, (args, kw) in workloads(dev).items():
        nc = kw.get("n_classes", 0)
        table = Evaluator(1, n_classes=nc, device=dev)
        fns = {"hip": lambda: eval_frame(*args, stats=table.table[0], **kw),
               "twin_a": lambda: torch_eval_frame(*args, **kw)}
        fns["twin_b"] = fns["twin_a"]
        for f in fns.values():                              # warm-up: code objects, allocator
            for _ in range(5):
                f()
        torch.cuda.synchronize()
        # the two paths agree on what they compute, before either is timed
        got, want = read_stats(table.table[0], nc), fns["twin_a"]()
        if name == "rgb":
            check = dict(mse=(got["mse"], float(want["mse"])), ssim=(got["ssim"], float(want["ssim"])))
        else:
            check = dict(nll=(got["nll"], float(want["nll"])), miou=(float(got["miou"]), float(want["miou"])))
        per = {p: [] for p in PATHS}
        for r in range(a.rounds):
            for k in range(len(PATHS)):
                path = PATHS[(k + r) % len(PATHS)]
                f = fns[path]
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                e0.record()
                for _ in range(a.steps):
                    f()
                e1.record()
                torch.cuda.synchronize()
                wall = (time.perf_counter() - t0) / a.steps * 1e3
                per[path].append(wall)
                emit(dict(kind="round", workload=name, path=path, round=r, steps=a.steps, wall_ms=wall,
                          event_ms=e0.elapsed_time(e1) / a.steps))
        med = {p: float(np.median(v)) for p, v in per.items()}
        spread = max(abs(med["twin_a"] - med["twin_b"]),
                     float(np.max(np.abs(np.array(per["twin_a"]) - np.array(per["twin_b"])))))
        twin = 0.5 * (med["twin_a"] + med["twin_b"])
        emit(dict(kind="summary", workload=name, view=[H, W], wall_ms_median=med, twin_spread_ms=spread,
                  hip_faster=bool(twin - med["hip"] > spread), twin_over_hip=twin / med["hip"],
                  saved_ms_per_view=twin - med["hip"], agree=check))
    big = Evaluator(100, n_classes=33, device=dev)
    torch.cuda.synchronize()
    reads = []
    for _ in range(5):
        t0 = time.perf_counter()
        big.results()
        reads.append((time.perf_counter() - t0) * 1e3)
    emit(dict(kind="read", records=100, n_classes=33, read_ms=float(np.median(reads))))
    if a.out:
        with open(a.out, "a") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
