#!/usr/bin/env python3
"""What the SAM teacher's input costs between the render and image_encoder
(GPU box): a 512 x 512 render -> the 1024-long input, both outputs.

  device      samnerf_amd.teacher.teacher_image on the render where it is:
              three launches (csrc/teacher_image.hip)
  reference   teacher.torch_teacher_image, the reference's own sequence
              (nerf/utils.py:1083-1085 + SamPredictor.set_image): the copy to
              the host with its synchronise, numpy's quantisation, PIL's
              bilinear resize, the upload, the torch normalise and pad --
              timed twice (reference_a, reference_b) so that its own
              run-to-run spread is known.  The baseline is this sequence on the
              same box, never the code under test.  Without PIL on the box only
              the device path is timed, and every record says so.

Then the same pair inside a cache-miss distillation step
(train.sam_distill_step without a cache, bench.py's config-5 net and
optimiser): the perturbed 512 x 512 teacher render under no_grad, the teacher
image by either path, an image encoder that returns a fixed [1, 256, 64, 64]
map without looking at its input, the 64 x 64 feature step with backward and
FusedAdam (step_device, step_reference_a / _b).  The ViT that a real predictor
runs at that point is not run and not measured, so the step's time here is a
lower bound of a real miss step and the saved share an upper bound.

Paths are timed in interleaved rounds in rotating order after a warm-up.  Per
path and round: HIP events on the current stream around `--calls` calls (a
hundredth of them for the reference, `--steps` steps for the step), and the
host clock around the same calls ending in a device synchronise; for the
reference, whose calls block on the host, the host clock is the figure.  The
shader clock over each timed window (two samnerf_clock_stamp launches around
it) goes into the record.  The two paths' results are compared bit for bit
before anything is timed.

Prints one JSON line per measurement and a summary; --out appends them to a
file (profiles/teacher_time.jsonl).
usage: python tools/teacher_time.py [--rounds 5] [--calls 5000] [--steps 40] [--out FILE]
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
TARGET = 1024


def window_clock(stamps):
    """GHz from two samnerf_clock_stamp records (256 x (XCC id, s_memtime,
    s_memrealtime at 100 MHz)): per XCD the medians' differences, then the mean."""
    a, b = stamps[0].reshape(256, 3), stamps[1].reshape(256, 3)
    per = []
    for x in sorted(set(a[:, 0].tolist()) & set(b[:, 0].tolist())):
        ta, tb = a[a[:, 0] == x], b[b[:, 0] == x]
        dr = float(np.median(tb[:, 2]) - np.median(ta[:, 2]))
        if dr > 0:
            per.append(float(np.median(tb[:, 1]) - np.median(ta[:, 1])) / dr * 0.1)
    return float(np.mean(per)) if per else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=5000)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("teacher_time: needs the GPU; a CPU run measures nothing")
    from samnerf_amd import teacher
    dev = torch.device("cuda:0")
    try:
        import PIL
        pil = PIL.__version__
    except ImportError:
        pil = None
    out = open(a.out, "a") if a.out else None
    tags = dict(render=[H, W], target=TARGET, outputs=["u8", "input"], pil=pil,
                gpu=torch.cuda.get_device_name(dev),
                vit="not run, not measured")
    if pil is None:
        tags["note"] = "PIL is not installed on this box: the reference sequence cannot run, device time alone"

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    rgb = torch.rand(H, W, 3, generator=torch.Generator().manual_seed(0)).to(dev)
    paths = {"device": lambda: teacher.teacher_image(rgb, target=TARGET)}
    order = ["device"]
    if pil is not None:
        paths["reference_a"] = paths["reference_b"] = lambda: teacher.torch_teacher_image(rgb, target=TARGET)
        order = ["reference_a", "device", "reference_b"]
        got, want = paths["device"](), paths["reference_a"]()
        equal = bool(torch.equal(got["u8"], want["u8"]) and torch.equal(got["input"], want["input"]))
        emit(dict(kind="check", device_equals_reference_bit_for_bit=equal, **tags))
        if not equal:
            sys.exit("teacher_time: the device path and the reference sequence differ; nothing timed")
    stamps = torch.zeros(2, 768, dtype=torch.int64, device=dev)
    per_ev, per_wall = timed(paths, order, lambda p: a.calls if p == "device" else max(a.calls // 100, 5),
                             a.rounds, stamps, emit, tags)
    summarise("summary", "device", per_ev, per_wall, pil is not None, emit, tags)
    step_paths, step_order = make_steps(dev, teacher, pil is not None)
    per_ev, per_wall = timed(step_paths, step_order, lambda p: a.steps, a.rounds, stamps, emit, tags)
    summarise("step_summary", "step_device", per_ev, per_wall, pil is not None, emit, tags)


def make_steps(dev, teacher, with_reference):
    """A cache-miss distillation step per teacher-image path, each on its own
    copy of bench.py's config-5 net."""
    import types

    from nerf.network import NeRFNetwork, default_opt
    from samnerf_amd import ops, synth
    from samnerf_amd.fused import FusedRenderer
    from samnerf_amd.optim import FusedAdam
    from samnerf_amd.train import sam_distill_step
    spec = synth.ModelSpec(with_sam=True)
    params = synth.make_params(spec, seed=0, emb_scale=1e-4, ln_jitter=0.0)      # bench.py build_net
    pose, intr = synth.gui_camera(W, H)
    ro, rd = ops.get_rays(pose, intr, H, W, device=dev)
    pose, intr = synth.gui_camera(64, 64)
    ro_lr, rd_lr = ops.get_rays(pose, intr, 64, 64, device=dev)
    gt = torch.randn(1, 256, 64, 64, generator=torch.Generator(device="cpu").manual_seed(1)).to(dev)
    predictor = types.SimpleNamespace(reset_image=lambda: None,
                                      model=types.SimpleNamespace(image_encoder=lambda x: gt))
    opt = types.SimpleNamespace(with_sam=True, cache_size=0, cache_interval=4, background="white")
    device_path, reference_path = teacher.teacher_image, teacher.torch_teacher_image

    def make(image_path):
        net = NeRFNetwork(default_opt(with_sam=True))
        net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in params.items()})
        net = net.to(dev).train()
        for k, p in net.named_parameters():
            p.requires_grad = k.startswith("s_grid") or k.startswith("samvit_mlp")
        adam = FusedAdam([p for p in net.parameters() if p.requires_grad], lr=1e-2, eps=1e-15)
        renderer = FusedRenderer(net)

        def step():
            teacher.teacher_image = image_path           # set_image_from_render looks it up per call
            try:
                data = {"rays_o": ro, "rays_d": rd, "H": H, "W": W, "rays_o_lr": ro_lr, "rays_d_lr": rd_lr,
                        "h": 64, "w": 64}
                _, _, loss = sam_distill_step(net, renderer, data, opt, 1, predictor)
            finally:
                teacher.teacher_image = device_path
            loss.backward()
            adam.step()
            adam.zero_grad(set_to_none=True)
        return step
    paths = {"step_device": make(device_path)}
    order = ["step_device"]
    if with_reference:
        paths["step_reference_a"], paths["step_reference_b"] = make(reference_path), make(reference_path)
        order = ["step_reference_a", "step_device", "step_reference_b"]
    return paths, order


def summarise(kind, device, per_ev, per_wall, with_reference, emit, tags):
    summary = dict(kind=kind, event_ms_mean={p: float(np.mean(v)) for p, v in per_ev.items()},
                   wall_ms_mean={p: float(np.mean(v)) for p, v in per_wall.items()},
                   device_round_spread_ms=float(np.max(per_wall[device]) - np.min(per_wall[device])), **tags)
    if with_reference:
        a, b = [np.array(v) for k, v in sorted(per_wall.items()) if k != device]
        ref_ms = 0.5 * float(a.mean() + b.mean())
        dev_ms = float(np.mean(per_wall[device]))
        summary.update(reference_ms=ref_ms, device_ms=dev_ms, saved_ms=ref_ms - dev_ms,
                       aa_spread_ms=max(abs(float(a.mean() - b.mean())), float(np.max(np.abs(a - b)))),
                       device_over_reference=dev_ms / ref_ms, saved_share_of_reference=(ref_ms - dev_ms) / ref_ms,
                       what="wall_ms: host clock around the calls, ending in a device synchronise")
    emit(summary)


def timed(paths, order, calls_of, rounds, stamps, emit, tags):
    """Interleaved rounds in rotating order after a warm-up: ({path: [event ms]}, {path: [wall ms]})."""
    dev = stamps.device
    from samnerf_amd import lib
    for p in order:                                        # warm-up: code objects, allocator, PIL's tables
        for _ in range(10):
            paths[p]()
    torch.cuda.synchronize()
    per_ev, per_wall = {p: [] for p in order}, {p: [] for p in order}
    for r in range(rounds):
        for k in range(len(order)):
            p = order[(k + r) % len(order)]
            f = paths[p]
            calls = calls_of(p)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            cur = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            lib().samnerf_clock_stamp(ctypes.c_void_p(stamps[0].data_ptr()), cur)
            e0.record()
            for _ in range(calls):
                f()
            e1.record()
            lib().samnerf_clock_stamp(ctypes.c_void_p(stamps[1].data_ptr()), cur)
            torch.cuda.synchronize()
            wall = (time.perf_counter() - t0) / calls * 1e3
            ev = e0.elapsed_time(e1) / calls
            per_ev[p].append(ev)
            per_wall[p].append(wall)
            emit(dict(kind="round", path=p, round=r, calls=calls, event_ms=ev, wall_ms=wall,
                      shader_clock_ghz=window_clock(stamps.cpu().numpy()), **tags))
    return per_ev, per_wall


if __name__ == "__main__":
    main()
