#!/usr/bin/env python3
"""What presenting one rendered frame costs, by path (GPU box).

samnerf_amd.present.present_frame -- the HIP kernels -- against
torch_present_frame, the reference's own op sequence on the same GPU (torch
ops, the two host copies, numpy for the buffer), per 512 x 512 display buffer
on synthetic render outputs (K = 5 instances):

  heatmap, composition, mask   the three --render_mask_type views, every
                               instance by its argmax, rendered at 512 x 512
  rgb_sam_click                the RGB frame under a SAM mask and one click
  depth                        the depth buffer (min / max normalisation)
  downscaled                   the composition view rendered at 256 x 256
                               (downscale = 0.5) and presented at 512 x 512

Paths: hip; twin_a and twin_b, the mirror timed twice so that its own
run-to-run spread is known.  Rounds are interleaved in rotating order, so clock
and thermal drift hit every path.  Per path and round: the host clock around
`--steps` frames ending in a device synchronise (a GUI waits for the enqueue as
much as for the kernels), HIP events around the same frames, and the shader
clock of the stretch from two samnerf_clock_stamp launches.  The kernel path's
result stays on the device; the one copy into the GUI's texture is not part of
either path's time.

Prints one JSON line per measurement and a summary per workload; --out appends
them to a file (profiles/present_time.jsonl).
usage: python tools/present_time.py [--rounds 5] [--steps 100] [--out FILE]
"""
import argparse
import ctypes
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
K = 5
PATHS = ("hip", "twin_a", "twin_b")


def workloads(dev):
    g = torch.Generator().manual_seed(5)

    def frame(h, w):
        return dict(image=torch.rand(h, w, 3, generator=g).to(dev), depth=(0.3 + 2 * torch.rand(h, w, generator=g)).to(dev),
                    logits=(2 * torch.randn(h, w, K, generator=g)).to(dev))
    full, half = frame(H, W), frame(H // 2, W // 2)
    cm = torch.rand(100, 3, generator=g).to(dev)
    sam = (torch.rand(H, W, generator=g) < 0.3).to(dev)

    def view(f, mask_type):
        return (f["image"], f["depth"]), dict(logits=f["logits"], n_inst=K, mask_type=mask_type, instance_id=-1,
                                              color_map=cm)
    out = {t: view(full, t) for t in ("heatmap", "composition", "mask")}
    out["rgb_sam_click"] = ((full["image"], full["depth"]), dict(sam_mask=sam, points=np.array([[300, 200]], np.int32)))
    out["depth"] = ((full["image"], full["depth"]), dict(mode="depth"))
    out["downscaled"] = view(half, "composition")
    return out


def main():
    import bench
    from samnerf_amd import _lib
    from samnerf_amd.present import present_frame, torch_present_frame
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU; there is nothing to time without one"
    dev = torch.device("cuda", 0)
    cur = torch.cuda.current_stream(dev)
    lines = []

    def emit(rec):
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    def stamp(buf):
        _lib.lib().samnerf_clock_stamp(ctypes.c_void_p(buf.data_ptr()), ctypes.c_void_p(cur.cuda_stream))

    for name, ((image, depth), kw) in workloads(dev).items():
        buf = torch.empty(H, W, 3, device=dev)
        fns = {"hip": lambda: present_frame(image, depth, H, W, buffer=buf, **kw),
               "twin_a": lambda: torch_present_frame(image, depth, H, W, **kw)}
        fns["twin_b"] = fns["twin_a"]
        for f in fns.values():                              # warm-up: code objects, allocator
            for _ in range(10):
                f()
        torch.cuda.synchronize()
        per = {p: [] for p in PATHS}
        for r in range(a.rounds):
            for k in range(len(PATHS)):
                path = PATHS[(k + r) % len(PATHS)]
                f = fns[path]
                stamps = torch.zeros(2, 768, dtype=torch.int64, device=dev)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                stamp(stamps[0])
                t0 = time.perf_counter()
                e0.record()
                for _ in range(a.steps):
                    f()
                e1.record()
                stamp(stamps[1])
                torch.cuda.synchronize()
                wall = (time.perf_counter() - t0) / a.steps * 1e3
                clock = bench.timed_clock(stamps.cpu().numpy())
                per[path].append(wall)
                emit(dict(kind="round", workload=name, path=path, round=r, steps=a.steps, wall_ms=wall,
                          event_ms=e0.elapsed_time(e1) / a.steps, ghz=clock["ghz"] if clock else None))
        mean = {p: float(np.mean(v)) for p, v in per.items()}
        spread = max(abs(mean["twin_a"] - mean["twin_b"]),
                     float(np.max(np.abs(np.array(per["twin_a"]) - np.array(per["twin_b"])))))
        twin = 0.5 * (mean["twin_a"] + mean["twin_b"])
        emit(dict(kind="summary", workload=name, render=list(depth.shape), buffer=[H, W], wall_ms_mean=mean,
                  twin_spread_ms=spread, hip_faster=bool(twin - mean["hip"] > spread), twin_over_hip=twin / mean["hip"],
                  saved_ms_per_frame=twin - mean["hip"]))
    if a.out:
        with open(a.out, "a") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
