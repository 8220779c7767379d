#!/usr/bin/env python3
"""What the incoherent-mask table costs, by path (GPU box).

chain   from the rendered logits of n = 64 views (K = 2) to the [n, S * S] bool
        table, at S = 128 and S = 512: samnerf_incoherent_ids +
        samnerf_incoherent_masks (two launches) against the mirror, the
        reference's op sequence on the same GPU (softmax, sum, stack, argmax,
        four F.interpolate calls, the residue, the threshold, .to(bool)).
update  samnerf_amd.incoherent.update_incoherent_mask for 64 views at S = 128
        on the full-size mask model: views_per_launch = 1, the default, and
        per-view renders with the mirror's post-processing; `render` is the ray
        generation and the renders alone, the share of the update that is not
        the table's.

Paths are timed in interleaved rounds in rotating order, so clock and thermal
drift hit every path; the mirror is timed twice (twin_a, twin_b) so that its own
run-to-run spread is known.  Per path and round: HIP events on the current
stream around `--steps` calls after a warm-up, and the host clock around the
same calls ending in a device synchronise.

Prints one JSON line per measurement and a summary per workload; --out appends
them to a file (profiles/incoherent_time.jsonl).
usage: python tools/incoherent_time.py [--rounds 5] [--steps 200] [--update-steps 3] [--out FILE]
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

N_VIEWS = 64


def timed_rounds(fns, order, rounds, steps, emit, **tags):
    """{path: [event ms per call, one per round]}"""
    for f in fns.values():                                # warm-up: code objects, allocator
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    per = {p: [] for p in order}
    for r in range(rounds):
        for k in range(len(order)):
            path = order[(k + r) % len(order)]
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
    return per


def chain(dev, S, rounds, steps, emit):
    from samnerf_amd import incoherent as inc
    g = torch.Generator().manual_seed(S)
    # smooth logits: blobs of each id with edges, as a mask head renders them
    base = torch.nn.functional.interpolate(torch.randn(N_VIEWS, 2, S // 16, S // 16, generator=g), (S, S),
                                           mode="bilinear")
    logits = (4 * base).permute(0, 2, 3, 1).contiguous().to(dev)               # [n, S, S, 2]
    table = torch.empty(N_VIEWS, S * S, dtype=torch.bool, device=dev)
    ids = torch.empty(N_VIEWS, S, S, dtype=torch.uint8, device=dev)

    def hip():
        inc.render_mask_ids(logits, 2, out=ids)
        inc.incoherent_table(ids, sfact=2, out=table)
        return table

    def twin():
        i = inc.torch_render_mask_ids(logits, 2)
        return inc.torch_get_incoherent_mask(i[:, None], sfact=2).to(torch.bool).view(N_VIEWS, S * S)
    same_ids = bool((inc.render_mask_ids(logits, 2) == inc.torch_render_mask_ids(logits, 2)).all())
    same_table = bool((inc.incoherent_table(ids, sfact=2)
                       == inc.torch_get_incoherent_mask(ids[:, None], sfact=2).to(torch.bool).view(N_VIEWS, -1)).all())
    fns = {"hip": hip, "twin_a": twin, "twin_b": twin}
    per = timed_rounds(fns, ("hip", "twin_a", "twin_b"), rounds, steps, emit, workload="chain", S=S, views=N_VIEWS)
    mean = {p: float(np.mean(v)) for p, v in per.items()}
    spread = max(abs(mean["twin_a"] - mean["twin_b"]),
                 float(np.max(np.abs(np.array(per["twin_a"]) - np.array(per["twin_b"])))))
    twin_ms = 0.5 * (mean["twin_a"] + mean["twin_b"])
    emit(dict(kind="summary", workload="chain", S=S, views=N_VIEWS, event_ms_mean=mean, twin_spread_ms=spread,
              hip_spread_ms=float(np.max(per["hip"]) - np.min(per["hip"])),
              hip_faster=bool(twin_ms - mean["hip"] > spread), twin_over_hip=twin_ms / mean["hip"],
              true_share=float(table.float().mean()), ids_equal_mirror=same_ids,
              table_equal_mirror_on_same_ids=same_table))


def update(dev, S, rounds, steps, emit):
    from nerf.network import NeRFNetwork, default_opt
    from oracle import synth
    from samnerf_amd import incoherent as inc
    from samnerf_amd.batch import BatchSource
    spec = synth.ModelSpec(with_sam=False, with_mask=True, mask_type="default", n_inst=2)
    params = synth.make_params(spec, seed=19, emb_scale=0.5)
    opt = default_opt(with_sam=False, with_mask=True, mask_mlp_type="default", n_inst=2)
    net = NeRFNetwork(opt)
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in params.items()})
    net = net.to(dev).train()
    poses = np.stack([synth.gui_camera(S, S, rot=synth.random_rotation(r))[0] for r in range(N_VIEWS)])
    intr = np.asarray(synth.gui_camera(S, S, rot=synth.random_rotation(0))[1], np.float32).reshape(1, 4)
    cnf = torch.tensor([[0.2, 6.0]], device=dev).repeat(N_VIEWS, 1)
    src = BatchSource(torch.from_numpy(poses.astype(np.float32)).to(dev), torch.from_numpy(intr).to(dev), 4 * S, 4 * S,
                      cam_near_far=cnf, incoherent_mask_size=S)
    opt.enable_cam_near_far = True
    K = 2

    def renders(per, sink=None):
        net.eval()
        with torch.no_grad():
            for first in range(0, N_VIEWS, per):
                count = min(per, N_VIEWS - first)
                ro, rd, c = inc.mask_view_rays(src, first, count, S, opt)
                out = net.render(ro, rd, staged=count * S * S > inc.RAYS_PER_CALL, bg_color=1, perturb=False,
                                 cam_near_far=c, return_feats=0, return_mask=True)
                if sink is not None:
                    sink(first, count, out["instance_mask_logits"])
        net.train()

    def mirror_update():
        masks = []
        renders(1, lambda first, count, z: masks.append(inc.torch_render_mask_ids(z.reshape(S, S, K), 2)))
        ids = torch.stack(masks, 0)[:, None]
        return inc.torch_get_incoherent_mask(ids, sfact=2).to(torch.bool).view(N_VIEWS, S * S)

    default = inc.default_views_per_launch(S)
    fns = {"hip_1": lambda: inc.update_incoherent_mask(net, src, opt, views_per_launch=1),
           f"hip_{default}": lambda: inc.update_incoherent_mask(net, src, opt, views_per_launch=default),
           "mirror_1": mirror_update,
           "render_1": lambda: renders(1), f"render_{default}": lambda: renders(default)}
    a = inc.update_incoherent_mask(net, src, opt, views_per_launch=1).clone()
    b = inc.update_incoherent_mask(net, src, opt, views_per_launch=default)
    same = bool((a == b).all())
    per = timed_rounds(fns, tuple(fns), rounds, steps, emit, workload="update", S=S, views=N_VIEWS)
    mean = {p: float(np.mean(v)) for p, v in per.items()}
    spread = {p: float(np.max(v) - np.min(v)) for p, v in per.items()}
    emit(dict(kind="summary", workload="update", S=S, views=N_VIEWS, rays=N_VIEWS * S * S, event_ms_mean=mean,
              round_spread_ms=spread, ms_per_view={p: v / N_VIEWS for p, v in mean.items()},
              render_share={"hip_1": mean["render_1"] / mean["hip_1"],
                            f"hip_{default}": mean[f"render_{default}"] / mean[f"hip_{default}"]},
              same_table_1_and_default=same, true_share=float(b.float().mean())))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--update-steps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU; there is nothing to time without one"
    dev = torch.device("cuda", 0)
    lines = []

    def emit(rec):
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    for S in (128, 512):
        chain(dev, S, a.rounds, a.steps, emit)
    update(dev, 128, a.rounds, a.update_steps, emit)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
