#!/usr/bin/env python3
"""What a click costs between the rendered feature map and the mask (GPU
box): g = 64, a 64 x 64 rendered map, a 512 x 512 view, 1 click and 8 clicks.

  device   sam_bridge.sam_predict_device on a sam_decoder.SamDecoder: the map
           as rendered to csrc/sam_decoder.hip (44 launches) and the
           postprocess (1 launch)
  twin     sam_bridge.sam_predict on tests/sam_decoder_ref.TwinPredictor in
           float32 on the same GPU: the same model as torch ops, which is what
           a third-party torch SAM decoder would run -- timed twice (twin_a,
           twin_b) so that its own run-to-run spread is known.  The baseline is
           this sequence on the same box, never the code under test.

Weights are synthetic (sam_decoder_ref.synthetic_state_dict): times do not
depend on their values.  The paths alternate in rotating order in one process
after a warm-up; per path and round, HIP events on the current stream around
enough calls to fill at least `--fill` seconds (sized from a trial), and the
host clock around the same calls ending in a device synchronise.  Both paths'
low-res masks are compared (relative error) before anything is timed.

Prints one JSON line per measurement and a summary per click count; --out
appends them to a file (profiles/sam_decoder_time.jsonl).
usage: python tools/sam_decoder_time.py [--rounds 5] [--fill 0.5] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "segment-anything-nerf_amd"), ROOT):
    sys.path.insert(0, p)

G, H, W = 64, 512, 512


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--fill", type=float, default=0.5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("sam_decoder_time: needs the GPU; a CPU run measures nothing")
    import sam_decoder_ref as ref
    from samnerf_amd import lib
    from samnerf_amd.sam_bridge import sam_predict, sam_predict_device
    from samnerf_amd.sam_decoder import SamDecoder
    dev = torch.device("cuda:0")
    out = open(a.out, "a") if a.out else None
    tags = dict(g=G, view=[H, W], map=[G, G], weights="synthetic", gpu=torch.cuda.get_device_name(dev),
                baseline="the float32 torch twin on the same GPU")

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    sd = ref.synthetic_state_dict(ref.WEIGHT_SEED)
    dec = SamDecoder.from_state_dict(sd, g=G, device=dev)
    twin = ref.TwinPredictor(sd, g=G, dtype=torch.float32, device=dev)
    feats = torch.randn(G, G, 256, generator=torch.Generator().manual_seed(0)).to(dev)
    rng = np.random.RandomState(0)
    for clicks in (1, 8):
        pts = np.stack([rng.randint(0, W, clicks), rng.randint(0, H, clicks)], -1)
        paths = {"device": lambda: sam_predict_device(dec, H, W, feats, point_coords=pts),
                 "twin_a": lambda: sam_predict(twin, H, W, feats, point_coords=pts)}
        paths["twin_b"] = paths["twin_a"]
        order = ["twin_a", "device", "twin_b"]
        got, want = paths["device"](), paths["twin_a"]()
        torch.cuda.synchronize()
        launches = lib().samnerf_sam_decoder_launches() + 1
        err = (got[2] - want[2]).abs().max().item() / want[2].abs().max().item()
        emit(dict(kind="check", clicks=clicks, low_res_rel_diff=err, masks_equal=bool(torch.equal(got[0], want[0])),
                  device_launches_per_call=launches, **tags))
        if not err < 1e-4:
            sys.exit("sam_decoder_time: the two paths differ; nothing timed")
        calls = {}
        for p in order:                                    # warm-up, and the size of a window from a trial
            for _ in range(10):
                paths[p]()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(20):
                paths[p]()
            torch.cuda.synchronize()
            calls[p] = max(20, int(np.ceil(a.fill / ((time.perf_counter() - t0) / 20))))
        per_ev, per_wall = {p: [] for p in order}, {p: [] for p in order}
        for r in range(a.rounds):
            for k in range(len(order)):
                p = order[(k + r) % len(order)]
                f, n = paths[p], calls[p]
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                e0.record()
                for _ in range(n):
                    f()
                e1.record()
                torch.cuda.synchronize()
                wall, ev = (time.perf_counter() - t0) / n * 1e3, e0.elapsed_time(e1) / n
                per_ev[p].append(ev)
                per_wall[p].append(wall)
                emit(dict(kind="round", clicks=clicks, path=p, round=r, calls=n, event_ms=ev, wall_ms=wall, **tags))
        ta, tb = np.array(per_ev["twin_a"]), np.array(per_ev["twin_b"])
        twin_ms, dev_ms = 0.5 * float(ta.mean() + tb.mean()), float(np.mean(per_ev["device"]))
        emit(dict(kind="summary", clicks=clicks, device_launches_per_call=launches,
                  event_ms_mean={p: float(np.mean(v)) for p, v in per_ev.items()},
                  wall_ms_mean={p: float(np.mean(v)) for p, v in per_wall.items()},
                  device_ms=dev_ms, twin_ms=twin_ms, twin_over_device=twin_ms / dev_ms,
                  device_round_spread_ms=float(np.max(per_ev["device"]) - np.min(per_ev["device"])),
                  twin_aa_spread_ms=max(abs(float(ta.mean() - tb.mean())), float(np.max(np.abs(ta - tb)))),
                  what="event_ms: HIP events around the calls of a round; the host enqueues both paths", **tags))


if __name__ == "__main__":
    main()
