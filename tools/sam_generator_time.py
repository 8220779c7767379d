#!/usr/bin/env python3
"""What "segment everything" costs on a rendered feature map (GPU box): g = 64,
a 64 x 64 rendered map, a 512 x 512 view, 32 x 32 points, three masks a point.

  loop     what the single-click entry points allow: SamDecoder.decode and
           masks (logits) per point, the filters as torch ops per point, one
           torch box-IoU matrix and a host greedy pass for the NMS
  twin     the float32 torch twin (tests/sam_decoder_ref.Twin) per point on the
           same GPU with the same torch filters and NMS: what a third-party
           torch SAM would run -- timed twice (twin_a, twin_b) for its spread
  c16 .. c128  sam_generator.DeviceMaskGenerator at points_per_batch 16, 32, 64
           and 128, the list of records read back (its one host read)

Synthetic weights give noise-like logits on which SAM's default thresholds
pass nothing, so the thresholds are set from a first pass: pred_iou_thresh
and stability_score_thresh at the medians (half of the candidates walk the
pixels, half of those reach the NMS), mask_threshold at twice the standard
deviation of low_res (boxes that differ), the offset a quarter of it.

The paths alternate in rotating order in one process after a warm-up; per path
and round, HIP events on the current stream around one run.  The kept
candidates of every path are compared with the generator's before anything is
timed.  One more pass of the generator's steps with an event between them
gives the stage split.  Prints one JSON line per measurement; --out appends
them to a file (profiles/sam_generator_time.jsonl).
usage: python tools/sam_generator_time.py [--rounds 3] [--out FILE]
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

G, H, W, SIDE = 64, 512, 512, 32
CHUNKS = (16, 32, 64, 128)


def torch_filters(logits, iou, th):
    """The generator's filters of one point's masks as torch ops: (keep mask, boxes, stability)."""
    thr, off = th["mask_threshold"], th["stability_score_offset"]
    ok = iou > th["pred_iou_thresh"]
    inter = (logits > thr + off).flatten(1).sum(1)
    union = (logits > thr - off).flatten(1).sum(1)
    stab = inter.float() / union.float()
    ok = ok & (stab >= th["stability_score_thresh"])
    m = logits > thr
    rows, cols = m.any(2), m.any(1)
    ar_h, ar_w = torch.arange(m.shape[1], device=m.device), torch.arange(m.shape[2], device=m.device)
    big = 1 << 20
    y0 = torch.where(rows, ar_h, big).min(1).values
    y1 = torch.where(rows, ar_h, -1).max(1).values
    x0 = torch.where(cols, ar_w, big).min(1).values
    x1 = torch.where(cols, ar_w, -1).max(1).values
    box = torch.stack([x0, y0, x1, y1], 1)
    box = torch.where(m.flatten(1).any(1)[:, None], box, torch.zeros_like(box))
    return ok, box, stab


def torch_nms(box, score, ok, thresh):
    """Greedy box NMS: the IoU matrix on the device, the greedy pass on the host."""
    idx = torch.nonzero(ok)[:, 0]
    if idx.numel() == 0:
        return []
    order = idx[torch.sort(score[idx], descending=True, stable=True).indices]
    b = box[order].float()
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    w = (torch.minimum(b[:, None, 2], b[None, :, 2]) - torch.maximum(b[:, None, 0], b[None, :, 0])).clamp(min=0)
    h = (torch.minimum(b[:, None, 3], b[None, :, 3]) - torch.maximum(b[:, None, 1], b[None, :, 1])).clamp(min=0)
    inter = w * h
    over = (inter / (area[:, None] + area[None, :] - inter) > thresh).cpu().numpy()
    order = order.cpu().numpy()
    gone, keep = np.zeros(len(order), bool), []
    for i in range(len(order)):
        if gone[i]:
            continue
        keep.append(int(order[i]))
        gone[i + 1:] |= over[i, i + 1:]
    return keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("sam_generator_time: needs the GPU; a CPU run measures nothing")
    import sam_decoder_ref as ref
    from samnerf_amd import lib
    from samnerf_amd.sam_decoder import REC_WORDS, SamDecoder
    from samnerf_amd.sam_generator import DeviceMaskGenerator
    dev = torch.device("cuda:0")
    out = open(a.out, "a") if a.out else None
    tags = dict(g=G, view=[H, W], map=[G, G], points=[SIDE, SIDE], masks_per_point=3, weights="synthetic",
                gpu=torch.cuda.get_device_name(dev))

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    sd = ref.synthetic_state_dict(ref.WEIGHT_SEED)
    dec = SamDecoder.from_state_dict(sd, g=G, device=dev)
    twin = ref.Twin(sd, torch.float32, dev)
    fmap = torch.randn(G, G, 256, generator=torch.Generator().manual_seed(0)).to(dev)
    tokens = fmap.view(G * G, 256)
    size = (1024, 1024)

    # the thresholds, from a first pass that refuses nothing
    probe = DeviceMaskGenerator(dec, points_per_side=SIDE, points_per_batch=64, pred_iou_thresh=-1e30,
                                stability_score_thresh=-1.0, max_masks=1)
    pts_view, pts_in = probe.points_for(H, W)
    assert (pts_in == np.round(pts_in)).all()              # 32 i + 16: whole pixels, so the int32 entry takes them
    pts_whole = pts_in.astype(np.int32)
    low0, iou0 = dec.decode_batch(tokens, torch.as_tensor(pts_in[:64].astype(np.float32)).view(64, 1, 2))
    th = dict(mask_threshold=2.0 * float(low0[:, 1:].std()))
    th["stability_score_offset"] = 0.25 * th["mask_threshold"]
    th["pred_iou_thresh"], th["stability_score_thresh"], th["box_nms_thresh"] = -1e30, -1.0, 0.7
    n = 3 * SIDE * SIDE
    low = torch.empty(n, 4 * G, 4 * G, device=dev)
    iou = torch.empty(n, device=dev)
    pts_dev = torch.as_tensor(pts_in.astype(np.float32)).to(dev).view(-1, 1, 2)
    for p0 in range(0, SIDE * SIDE, 64):
        lo, io = dec.decode_batch(tokens, pts_dev[p0:p0 + 64])
        low[3 * p0:3 * (p0 + 64)] = lo[:, 1:].reshape(-1, 4 * G, 4 * G)
        iou[3 * p0:3 * (p0 + 64)] = io[:, 1:].reshape(-1)
    rec = dec.mask_stats(low, iou, size, (H, W), -1e30, -1.0, th["stability_score_offset"], th["mask_threshold"])
    stab = rec[:, 7].view(torch.float32)
    th["pred_iou_thresh"] = float(iou.median())
    live = iou > th["pred_iou_thresh"]
    th["stability_score_thresh"] = float(stab[live & ~stab.isnan()].median())
    del low, iou, rec
    emit(dict(kind="thresholds", **th, **tags))

    def device_path(chunk):
        gen = DeviceMaskGenerator(dec, points_per_side=SIDE, points_per_batch=chunk, max_masks=1024, **th)
        return lambda: [x["candidate"] for x in gen.generate(tokens, H, W)]

    def loop_path(decode):
        def run():
            oks, boxes, scores = [], [], []
            for k in range(SIDE * SIDE):
                logits, io = decode(k)
                ok, box, _ = torch_filters(logits, io, th)
                oks.append(ok), boxes.append(box), scores.append(io)
            return torch_nms(torch.cat(boxes), torch.cat(scores), torch.cat(oks), th["box_nms_thresh"])
        return run

    def decode_device(k):
        lo, io = dec.decode(tokens, pts_whole[k:k + 1])
        return dec.masks(lo[1:], size, (H, W), logits=True), io[1:]

    ones = np.ones(1, np.int32)

    def decode_twin(k):
        lo, io = twin.decode(tokens, pts_dev[k, 0][None], ones, G)
        return ref.postprocess(lo[1:], G, size, (H, W)), io[1:]

    paths = {"loop": loop_path(decode_device), "twin_a": loop_path(decode_twin)}
    paths["twin_b"] = paths["twin_a"]
    for c in CHUNKS:
        paths[f"c{c}"] = device_path(c)
    order = ["loop", "twin_a"] + [f"c{c}" for c in CHUNKS] + ["twin_b"]

    want = paths["c64"]()
    for p in ("c16", "c128", "loop", "twin_a"):
        got = paths[p]()
        emit(dict(kind="check", path=p, kept=len(got), kept_c64=len(want), same_as_c64=got == want, **tags))
    torch.cuda.synchronize()

    per = {p: [] for p in order}
    for r in range(a.rounds):
        for k in range(len(order)):
            p = order[(k + r) % len(order)]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            paths[p]()
            e1.record()
            torch.cuda.synchronize()
            wall, ev = (time.perf_counter() - t0) * 1e3, e0.elapsed_time(e1)
            per[p].append(ev)
            emit(dict(kind="round", path=p, round=r, event_ms=ev, wall_ms=wall, **tags))
    ta, tb = np.array(per["twin_a"]), np.array(per["twin_b"])
    loop = np.array(per["loop"])
    emit(dict(kind="summary", event_ms_mean={p: float(np.mean(v)) for p, v in per.items()},
              event_ms_min={p: float(np.min(v)) for p, v in per.items()},
              event_ms_max={p: float(np.max(v)) for p, v in per.items()},
              twin_aa_spread_ms=float(np.max(np.abs(ta - tb))),
              device_faster_than_loop_every_round={f"c{c}": bool((np.array(per[f"c{c}"]) < loop).all())
                                                   for c in CHUNKS},
              launches_per_decode=lib().samnerf_sam_decoder_launches(), **tags))

    # the stage split of one pass at the default chunk
    chunk = 64
    ws = lib().samnerf_sam_decoder_batch_workspace_size(G, chunk)
    low = torch.empty(n, 4 * G, 4 * G, device=dev)
    iou = torch.empty(n, device=dev)
    rec = torch.empty(n, REC_WORDS, dtype=torch.int32, device=dev)
    marks = {k: 0.0 for k in ("decoder", "copy", "stats", "nms", "select")}

    def timed(key, f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = f()
        e1.record()
        torch.cuda.synchronize()
        marks[key] += e0.elapsed_time(e1)
        return r

    def put(c0, c1, lo, io):
        low[c0:c1] = lo[:, 1:].reshape(-1, 4 * G, 4 * G)
        iou[c0:c1] = io[:, 1:].reshape(-1)
    for p0 in range(0, SIDE * SIDE, chunk):
        lo, io = timed("decoder", lambda: dec.decode_batch(tokens, pts_dev[p0:p0 + chunk]))
        c0, c1 = 3 * p0, 3 * (p0 + chunk)
        timed("copy", lambda: put(c0, c1, lo, io))
        timed("stats", lambda: dec.mask_stats(low[c0:c1], iou[c0:c1], size, (H, W), th["pred_iou_thresh"],
                                              th["stability_score_thresh"], th["stability_score_offset"],
                                              th["mask_threshold"], out=rec[c0:c1]))
    keep, count = timed("nms", lambda: dec.nms(rec, th["box_nms_thresh"]))
    timed("select", lambda: dec.masks_select(low, size, (H, W), index=keep, count=count, cap=1024,
                                             mask_threshold=th["mask_threshold"]))
    emit(dict(kind="stages", chunk=chunk, event_ms=marks, kept=int(count.item()),
              passing=int((rec[:, 8] != 0).sum().item()), walked=int((rec[:, 9] != 0).sum().item()),
              workspace_bytes=ws, retained_low_res_bytes=low.numel() * 4, **tags))


if __name__ == "__main__":
    main()
