#!/usr/bin/env python3
"""What perturb=True costs, by where the draws come from (GPU box).

The 512^2 headline view (BASELINE config 3: SAM model, reference table sizes,
view_width 512, one stream) in three modes on one box, rounds interleaved so
clock and thermal drift hit all three:

  unperturbed   perturb=False
  torch         perturb=True, the reference's draws: torch.rand_like and the
                position tensors (fused.perturbed_positions) inside the timed
                region, the render fed the arrays -- what bench.py's
                perturbed_render line times
  seeded        perturb=PhiloxPerturb(seed, k): the kernels draw, no arrays

Per mode and round: HIP events around `--views` views, the shader clock of
those views from two samnerf_clock_stamp launches (bench.timed_clock), then the
stage times -- prop0, prop1 and the three after them (samnerf_set_stage_events)
-- over `--stage-views` more views; the summary says which stage carries what a
mode adds.  The same for one RGB training step of 4,096 rays
(rgb_train_step_fused: forward, loss, backward; no optimiser) with torch draws
and seeded.

--ab-lib PATH: another build of the library (the parent commit's): the
unperturbed view's prop0 / prop1 stage times of this build against that one,
interleaved in rotating order, and that one against itself (a second handle
of a copy of the file) for the run-to-run spread: this build passes where its
mean difference lies inside the range of the round-by-round A/A differences.

Prints one JSON line per measurement and a summary line; --out appends them
to a file (profiles/).
usage: python tools/perturb_time.py [--rounds 5] [--views 20] [--ab-lib LIB] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "segment-anything-nerf_amd"))

SEED = 0x5EED0123456789AB


class Lib:
    """While active, every call goes through the given library handle (as
    _lib.diag_library does for the diagnostic build)."""

    def __init__(self, handle):
        self.handle = handle

    def __enter__(self):
        from samnerf_amd import _lib
        self.prev = _lib.lib()
        _lib._lib = self.handle

    def __exit__(self, *exc):
        from samnerf_amd import _lib
        _lib._lib = self.prev


def main():
    import bench
    from samnerf_amd import _lib, ops, synth
    from samnerf_amd.fused import FusedRenderer, PhiloxPerturb
    from samnerf_amd.train import rgb_train_step_fused
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--views", type=int, default=20)
    ap.add_argument("--stage-views", type=int, default=5)
    ap.add_argument("--train-steps", type=int, default=20)
    ap.add_argument("--ab-lib", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    lines = []

    def emit(rec):
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    net, _, _ = bench.build_net(True, dev)
    pose, intr = synth.gui_camera(512, 512)
    ro, rd = ops.get_rays(pose, intr, 512, 512, device=dev)
    cur = torch.cuda.current_stream(dev)
    counter = [0]

    def source(mode):
        if mode == "seeded":
            counter[0] += 1
            return PhiloxPerturb(SEED, counter[0])
        return mode == "torch"

    def stamp(buf):
        _lib.lib().samnerf_clock_stamp(ctypes.c_void_p(buf.data_ptr()), ctypes.c_void_p(cur.cuda_stream))

    def timed_views(fr, mode, n):
        """ms per view over n views (HIP events) and their shader clock."""
        stamps = torch.zeros(2, 768, dtype=torch.int64, device=dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        stamp(stamps[0])
        e0.record()
        for _ in range(n):
            fr.render(ro, rd, view_width=512, perturb=source(mode))
        e1.record()
        stamp(stamps[1])
        torch.cuda.synchronize()
        clock = bench.timed_clock(stamps.cpu().numpy())
        return e0.elapsed_time(e1) / n, clock["ghz"] if clock else None

    def stage_views(fr, mode, n):
        """Mean stage ms (prop0, prop1, final, s_grid, head) over n views."""
        sets = []
        for _ in range(n):
            evs = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
            for e in evs:
                e.record()
            sets.append((evs, (ctypes.c_void_p * 6)(*[e.cuda_event for e in evs])))
        torch.cuda.synchronize()
        try:
            for _, raw in sets:
                _lib.lib().samnerf_set_stage_events(raw, 6)
                fr.render(ro, rd, view_width=512, perturb=source(mode))
            torch.cuda.synchronize()
        finally:
            _lib.lib().samnerf_set_stage_events(None, 0)
        return {st: float(np.mean([evs[j].elapsed_time(evs[j + 1]) for evs, _ in sets]))
                for j, st in enumerate(("prop0", "prop1", "final", "s_grid", "head"))}

    # ---- the view in three modes
    modes = ("unperturbed", "torch", "seeded")
    fr = FusedRenderer(net)
    for m in modes:
        for _ in range(3):
            fr.render(ro, rd, view_width=512, perturb=source(m))
    stages = ("prop0", "prop1", "final", "s_grid", "head")
    per = {m: {k: [] for k in ("ms", "ghz") + stages} for m in modes}
    for rnd in range(a.rounds):
        for m in modes:
            ms, ghz = timed_views(fr, m, a.views)
            st = stage_views(fr, m, a.stage_views)
            per[m]["ms"].append(ms)
            per[m]["ghz"].append(ghz)
            for k in stages:
                per[m][k].append(st[k])
            emit({"what": "view", "mode": m, "round": rnd, "ms_per_view": round(ms, 4), "clock_ghz": ghz,
                  "stage_ms": {k: round(v, 4) for k, v in st.items()}})
    mean = {m: {k: float(np.mean([v for v in vs if v is not None])) for k, vs in d.items()} for m, d in per.items()}
    base = mean["unperturbed"]["ms"]
    emit({"what": "view summary", "views_per_round": a.views, "rounds": a.rounds,
          "mean": {m: {k: round(v, 4) for k, v in d.items()} for m, d in mean.items()},
          "ratio_to_unperturbed": {m: round(mean[m]["ms"] / base, 4) for m in modes},
          # what the mode adds to the unperturbed view, by stage; "outside_the_stages": the
          # rest of the view time (the torch draws and position tensors precede prop0)
          "extra_ms_by_stage": {m: {**{k: round(mean[m][k] - mean["unperturbed"][k], 4) for k in stages},
                                    "outside_the_stages": round(
                                        (mean[m]["ms"] - base)
                                        - sum(mean[m][k] - mean["unperturbed"][k] for k in stages), 4)}
                                for m in modes[1:]}})

    # ---- one RGB training step of 4,096 rays, torch draws and seeded
    tnet, _, _ = bench.build_net(False, dev, seed=3, emb_scale=0.5)
    tnet.train()
    tnet.opt.adaptive_num_rays = False
    inds = torch.randint(0, 512 * 512, (4096,), generator=torch.Generator().manual_seed(4)).to(dev)
    tro, trd = ro[inds].contiguous(), rd[inds].contiguous()
    gt = torch.rand(4096, 3, generator=torch.Generator().manual_seed(4)).to(dev)

    def train_steps(mode, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for i in range(n):
            for p in tnet.parameters():
                p.grad = None
            rgb_train_step_fused(tnet, tro, trd, gt, global_step=1 + i, perturb=source(mode) or True)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n

    tper = {m: [] for m in modes[1:]}
    for m in tper:
        train_steps(m, 3)
    for rnd in range(a.rounds):
        for m in tper:
            ms = train_steps(m, a.train_steps)
            tper[m].append(ms)
            emit({"what": "rgb train step, 4096 rays", "mode": m, "round": rnd, "ms_per_step": round(ms, 4)})
    emit({"what": "rgb train step summary", "rays": 4096, "steps_per_round": a.train_steps,
          "mean_ms": {m: round(float(np.mean(v)), 4) for m, v in tper.items()},
          "note": "forward + loss + backward (samnerf_rgb_train_step), gradients dropped each step, no optimiser"})

    # ---- the unperturbed proposal stages of this build against another build
    if a.ab_lib:
        path = os.path.abspath(a.ab_lib)
        libs = {"this": _lib.lib(), "other": _lib._load(path, lenient=True)}
        # a second handle of the same file for the A/A (a copy: one path loads once)
        import shutil
        import tempfile
        twin = os.path.join(tempfile.mkdtemp(), "twin_" + os.path.basename(path))
        shutil.copy(path, twin)
        libs["other_again"] = _lib._load(twin, lenient=True)
        frs = {k: FusedRenderer(net) for k in libs}
        ab = {k: {"prop0": [], "prop1": [], "ms": []} for k in libs}
        for k in libs:
            with Lib(libs[k]):
                for _ in range(3):
                    frs[k].render(ro, rd, view_width=512)
        names = list(libs)
        for rnd in range(a.rounds):
            for k in names[rnd % 3:] + names[:rnd % 3]:          # rotate: no build always runs first
                with Lib(libs[k]):
                    ms, ghz = timed_views(frs[k], "unperturbed", a.views)
                    st = stage_views(frs[k], "unperturbed", a.stage_views)
                ab[k]["ms"].append(ms)
                ab[k]["prop0"].append(st["prop0"])
                ab[k]["prop1"].append(st["prop1"])
                emit({"what": "unperturbed view A/B", "lib": k, "round": rnd, "ms_per_view": round(ms, 4),
                      "clock_ghz": ghz, "prop0_ms": round(st["prop0"], 4), "prop1_ms": round(st["prop1"], 4)})
        mu = {k: {s: float(np.mean(v)) for s, v in d.items()} for k, d in ab.items()}
        keys = ("prop0", "prop1", "ms")
        # the run-to-run spread: the other build against itself, round by round (two
        # handles of one file differ by nothing but when they ran) -- the range of
        # those differences; this build passes where its mean difference from the
        # other build lies inside that range
        aa = {s: np.array(ab["other_again"][s]) - np.array(ab["other"][s]) for s in keys}
        emit({"what": "unperturbed view A/B summary", "other": a.ab_lib, "rounds": a.rounds,
              "mean": {k: {s: round(v, 4) for s, v in d.items()} for k, d in mu.items()},
              "this_minus_other": {s: round(mu["this"][s] - mu["other"][s], 4) for s in keys},
              "other_minus_itself_mean": {s: round(float(aa[s].mean()), 4) for s in keys},
              "other_minus_itself_range": {s: [round(float(aa[s].min()), 4), round(float(aa[s].max()), 4)]
                                           for s in keys},
              "within_spread": {s: bool(aa[s].min() <= mu["this"][s] - mu["other"][s] <= aa[s].max())
                                for s in keys}})

    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
