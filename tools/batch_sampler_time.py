#!/usr/bin/env python3
"""What one training batch costs to choose and gather, by path (GPU box).

TrainBatchSampler.sample at the reference's defaults -- 4,096 rays, 512 x 512
images, a 128 x 128 error map, 100 synthetic uint8 images -- for each mode:

  rgb_random    mode R: the RGB stage's random image batch
  mask_mixed    mode R + two 16 x 16 local patches (mode C): the mask stage
                with --error_map --mixed_sampling past rgb_similarity_iter
  error_pixels  mode E: error-map-weighted pixels without replacement
  centred       mode C: one 64 x 64 patch centred on an error-map draw
  patch         mode P: one random 64 x 64 patch

and each path on the same GPU:

  seeded        rng=PhiloxBatch: the kernels draw and gather
  hip           rng="torch": torch draws, k_batch_gather gathers
  twin_a/_b     rng="torch", use_kernels=False: the torch twin, timed twice so
                that its own run-to-run spread is known

Rounds are interleaved in rotating order, so clock and thermal drift hit every
path.  Per path and round: the host clock around `--steps` steps ending in a
device synchronise (the sampler is launch-bound: what a training loop waits
for is the enqueue as much as the kernels), HIP events around the same steps,
and the shader clock of the stretch from two samnerf_clock_stamp launches.
check_inputs is off on every path (it is one read-back per step on all of
them).  Then, once per mode and path, the device kernels of one step counted
by torch.profiler.

A mode's HIP path counts as faster only where the twin's mean exceeds it by
more than the spread between twin_a and twin_b.

Prints one JSON line per measurement and a summary per mode; --out appends
them to a file (profiles/batch_sampler_time.jsonl).
usage: python tools/batch_sampler_time.py [--rounds 5] [--steps 200] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "segment-anything-nerf_amd"))

N_IMG, H, W, M = 100, 512, 512, 128
BASE = dict(num_rays=4096, with_sam=False, with_mask=True, use_multi_res=False, rgb_similarity_iter=10,
            random_image_batch=False, patch_size=1, error_map=True, error_map_size=M, mixed_sampling=False,
            num_local_sample=2, local_sample_patch_size=16, enable_cam_near_far=True, online_resolution=H)
MODES = {
    "rgb_random": (dict(with_mask=False, error_map=False, random_image_batch=True), 1, True),
    "mask_mixed": (dict(mixed_sampling=True), 11, False),
    "error_pixels": (dict(), 1, True),
    "centred": (dict(patch_size=64), 1, True),
    "patch": (dict(patch_size=64, error_map=False), 1, True),
}
PATHS = ("seeded", "hip", "twin_a", "twin_b")


def make_source(dev, with_mask, with_incoherent):
    from samnerf_amd import synth
    from samnerf_amd.batch import BatchSource
    g = torch.Generator().manual_seed(3)
    poses = torch.stack([torch.from_numpy(synth.gui_camera(W, H, rot=synth.random_rotation(k))[0])
                         for k in range(N_IMG)])
    intr = torch.from_numpy(synth.gui_camera(W, H)[1])[None].repeat(N_IMG, 1)
    kw = dict(images=torch.randint(0, 256, (N_IMG, H, W, 3), generator=g, dtype=torch.uint8).to(dev),
              cam_near_far=torch.tensor([[0.05, 2.0]]).repeat(N_IMG, 1).to(dev))
    if with_mask:
        kw["masks"] = torch.randint(0, 8, (N_IMG, H, W, 1), generator=g).to(dev)
        kw["error_map"] = (0.05 + torch.rand(N_IMG, M * M, generator=g)).to(dev)
        if with_incoherent:
            inc = (torch.rand(N_IMG, H * W, generator=g) > 0.5).to(dev)
            kw["incoherent_masks"] = kw["gt_incoherent_masks"] = inc
    return BatchSource(poses.to(dev), intr.to(dev), H, W, **kw)


def main():
    import bench
    from samnerf_amd import _lib
    from samnerf_amd.batch import PhiloxBatch, TrainBatchSampler
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=200)
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

    sources = {(m, i): make_source(dev, m, i) for m, i in ((False, False), (True, True), (True, False))}
    torch.manual_seed(1)
    for mode, (over, step, default_intr) in MODES.items():
        opt = dict(BASE, **over)
        # mode P is what the collate takes when the dataset has no incoherent masks
        src = sources[(opt["with_mask"], opt["with_mask"] and mode != "patch")]
        samplers = {}
        for path in PATHS:
            samplers[path] = TrainBatchSampler(
                src, types.SimpleNamespace(**opt), rng=PhiloxBatch(9, 0) if path == "seeded" else "torch",
                use_default_intrinsics=default_intr, check_inputs=False, use_kernels=not path.startswith("twin"))
        for s in samplers.values():                         # warm-up: code objects, allocator
            for _ in range(10):
                out = s.sample(step, [3])
        torch.cuda.synchronize()
        rays = int(out["rays_o"].shape[0])
        per = {p: [] for p in PATHS}
        for r in range(a.rounds):
            for k in range(len(PATHS)):
                path = PATHS[(k + r) % len(PATHS)]
                s = samplers[path]
                stamps = torch.zeros(2, 768, dtype=torch.int64, device=dev)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                stamp(stamps[0])
                t0 = time.perf_counter()
                e0.record()
                for _ in range(a.steps):
                    s.sample(step, [3])
                e1.record()
                stamp(stamps[1])
                torch.cuda.synchronize()
                wall = (time.perf_counter() - t0) / a.steps * 1e3
                clock = bench.timed_clock(stamps.cpu().numpy())
                per[path].append(wall)
                emit(dict(kind="round", mode=mode, path=path, round=r, rays=rays, steps=a.steps, wall_ms=wall,
                          event_ms=e0.elapsed_time(e1) / a.steps, ghz=clock["ghz"] if clock else None))
        kernels = {}
        for path in PATHS[:3]:
            try:
                from torch.profiler import ProfilerActivity, profile
                with profile(activities=[ProfilerActivity.CUDA]) as prof:
                    samplers[path].sample(step, [3])
                    torch.cuda.synchronize()
                kernels[path] = sum(e.count for e in prof.key_averages() if e.device_type.name != "CPU")
            except Exception as e:                           # the count is a note, the times are the result
                kernels[path] = f"not counted: {type(e).__name__}"
        mean = {p: float(np.mean(v)) for p, v in per.items()}
        spread = abs(mean["twin_a"] - mean["twin_b"])
        round_spread = float(np.max(np.abs(np.array(per["twin_a"]) - np.array(per["twin_b"]))))
        twin = 0.5 * (mean["twin_a"] + mean["twin_b"])
        emit(dict(kind="summary", mode=mode, rays=rays, wall_ms_mean=mean, twin_spread_ms=spread,
                  twin_round_spread_ms=round_spread, device_kernels=kernels,
                  seeded_faster=bool(twin - mean["seeded"] > max(spread, round_spread)),
                  hip_faster=bool(twin - mean["hip"] > max(spread, round_spread)),
                  twin_over_seeded=twin / mean["seeded"], twin_over_hip=twin / mean["hip"]))
    if a.out:
        with open(a.out, "a") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
