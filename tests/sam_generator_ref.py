"""The twin of sam_generator.DeviceMaskGenerator in torch over
sam_decoder_ref.Twin and postprocess, the dtype a parameter: the point grid,
a decode per point, the predicted-IoU filter, the stability score, the boxes,
a plain-Python greedy box NMS and the records.  float64 is the reference of
the tests, float32 their yardstick.

Synthetic weights give noise-like logits: SAM's default thresholds decide
nothing on them (every box is the whole view, every stability score far from
0.95).  choose_thresholds() therefore takes the generator's five thresholds
from the float64 twin's own values, each at the midpoint of the widest gap
near the median, so that every filter has something to pass and something to
refuse and every decision has a margin."""
import functools

import numpy as np
import torch

import sam_decoder_ref as ref

# name, g, points per side, view H x W, points per batch, feature seed, and the quantile of the passing
# candidates' logits that is the case's mask_threshold (multimask, single).  The seeds and quantiles are those
# at which test_sam_generator_cpu.py::test_the_cases_are_decided holds, found by trying seeds 0, 1, 2, ...
CASES = [
    ("g8_4x4", 8, 4, (33, 65), 5, 2, (0.98, 0.98)),
    ("g16_6x6", 16, 6, (48, 64), 8, 13, (0.995, 0.98)),
]
CASE_NAMES = [c[0] for c in CASES]
EPS = 1e-4                   # the `decided` rule of sam_decoder_ref: |logit - cut| > EPS max|low_res|


def case(name):
    return CASES[CASE_NAMES.index(name)]


def point_grid(n):
    """(i + 0.5) / n, rows of y, x fastest: [n*n, 2] (x, y) in float64."""
    ax = (np.arange(n, dtype=np.float64) + 0.5) / n
    return np.stack([np.tile(ax, n), np.repeat(ax, n)], -1)


@functools.lru_cache(maxsize=None)
def case_inputs(name):
    """dict(g, H, W, input_size, features [g*g, 256] float64, points_view, points_in [n, 2] float64)."""
    _, g, side, (H, W), chunk, seed, _ = case(name)
    gen = torch.Generator().manual_seed(seed)
    input_size, _ = ref.input_size_for(H, W, g)
    f = torch.randn(g, g, ref.C, generator=gen, dtype=torch.float64)
    rr = g / W if W > H else g / H
    f[int(H * rr):] = 0
    f[:, int(W * rr):] = 0
    pv = point_grid(side) * np.array([[W, H]], dtype=np.float64)
    pin = pv * np.array([[input_size[1] / W, input_size[0] / H]])
    return dict(g=g, H=H, W=W, input_size=input_size, features=f.view(g * g, ref.C), points_view=pv, points_in=pin,
                chunk=chunk, side=side)


@functools.lru_cache(maxsize=None)
def decoded(name, dtype=torch.float64):
    """Every point of the grid decoded alone, the points as the device gets
    them (float32 of the float64 product): (low_res [n, 4, L, L], iou [n, 4],
    logits [n, 4, H, W]) in `dtype`.  Computed once, do not modify."""
    x = case_inputs(name)
    t = ref.Twin(ref.state_dict(), dtype)
    feats = x["features"].to(dtype)
    pts = torch.from_numpy(x["points_in"].astype(np.float32))
    lows, ious = [], []
    for p in pts:
        low, iou = t.decode(feats, p[None], np.ones(1, np.int32), x["g"])
        lows.append(low)
        ious.append(iou)
    low, iou = torch.stack(lows), torch.stack(ious)
    L = low.shape[-1]
    logits = ref.postprocess(low.view(-1, L, L), x["g"], x["input_size"], (x["H"], x["W"]))
    return low, iou, logits.view(len(pts), 4, x["H"], x["W"])


def candidates(name, multimask, dtype=torch.float64):
    """(low_res [n, L, L], iou [n], logits [n, H, W]), candidate = point * M + mask."""
    low, iou, logits = decoded(name, dtype)
    sel = slice(1, 4) if multimask else slice(0, 1)
    return low[:, sel].flatten(0, 1), iou[:, sel].flatten(0, 1), logits[:, sel].flatten(0, 1)


def boxes_of(mask):
    """batched_mask_to_box: [n, H, W] bool -> [n, 4] int64 x0, y0, x1, y1 (max inclusive), zeros when empty."""
    out = torch.zeros(mask.shape[0], 4, dtype=torch.int64)
    for i, m in enumerate(mask):
        ys, xs = torch.nonzero(m, as_tuple=True)
        if len(ys):
            out[i] = torch.tensor([xs.min(), ys.min(), xs.max(), ys.max()])
    return out


def box_iou(a, b, dtype=np.float32):
    """torchvision's: boxes as floats, a = (x1 - x0)(y1 - y0); 0 / 0 is NaN."""
    a, b = np.asarray(a, dtype=dtype), np.asarray(b, dtype=dtype)
    w = max(dtype(0), min(a[2], b[2]) - max(a[0], b[0]))
    h = max(dtype(0), min(a[3], b[3]) - max(a[1], b[1]))
    inter = dtype(w * h)
    with np.errstate(invalid="ignore", divide="ignore"):
        return dtype(inter) / dtype(dtype((a[2] - a[0]) * (a[3] - a[1])) + dtype((b[2] - b[0]) * (b[3] - b[1])) - inter)


def greedy_nms(boxes, scores, passing, thresh, dtype=np.float32, trace=None):
    """The kept indices in order: descending score, ties to the lower index;
    a kept box suppresses a later one whose IoU with it exceeds thresh (NaN
    suppresses nothing).  trace, a list, receives every IoU compared."""
    order = sorted((i for i in range(len(scores)) if passing[i]), key=lambda i: (-float(scores[i]), i))
    gone, keep = set(), []
    for a, i in enumerate(order):
        if i in gone:
            continue
        keep.append(i)
        for j in order[a + 1:]:
            if j in gone:
                continue
            v = box_iou(boxes[i], boxes[j], dtype)
            if trace is not None:
                trace.append(float(v))
            if v > thresh:
                gone.add(j)
    return keep


def stats(logits, iou, th):
    """The records of n candidates from their logits [n, H, W] in the logits'
    dtype: dict of inter, union, area (int64), box [n, 4], stability, pass_iou,
    pass (bool); a candidate failing the IoU test has zeros."""
    thr, off = th["mask_threshold"], th["stability_score_offset"]
    pass_iou = iou > th["pred_iou_thresh"]
    inter = (logits > thr + off).flatten(1).sum(1)
    union = (logits > thr - off).flatten(1).sum(1)
    mask = logits > thr
    stab = inter.to(logits.dtype) / union.to(logits.dtype)
    ok = pass_iou & (stab >= th["stability_score_thresh"])
    z = ~pass_iou
    box = boxes_of(mask)
    box[z] = 0
    return dict(inter=inter.masked_fill(z, 0), union=union.masked_fill(z, 0),
                area=mask.flatten(1).sum(1).masked_fill(z, 0), box=box, stability=stab.masked_fill(z, 0),
                pass_iou=pass_iou, passing=ok, mask=mask)


def undecided(logits, low, th):
    """Per candidate, the pixels whose float64 logit lies within EPS max|low_res| of each cut: [n, 3] (+off, -off, 0)."""
    thr, off = th["mask_threshold"], th["stability_score_offset"]
    eps = EPS * low.abs().max()
    return torch.stack([((logits - c).abs() <= eps).flatten(1).sum(1) for c in (thr + off, thr - off, thr)], 1)


def widest_gap(values, lo=0.25, hi=0.75):
    """The midpoint of the widest gap between neighbours of the sorted values
    such that the fraction above it lies in [lo, hi]; (cut, gap)."""
    v = np.sort(np.asarray(values, dtype=np.float64))
    n, best = len(v), None
    for k in range(1, n):                                   # the cut between v[k - 1] and v[k]: n - k above
        if lo <= (n - k) / n <= hi and v[k] > v[k - 1] and (best is None or v[k] - v[k - 1] > best[1]):
            best = (0.5 * (v[k] + v[k - 1]), v[k] - v[k - 1])
    assert best is not None, "no gap with the wanted fraction above it"
    return best


@functools.lru_cache(maxsize=None)
def choose_thresholds(name, multimask):
    """The five thresholds from the float64 twin's values: pred_iou_thresh at
    the widest gap of the scores around their median; mask_threshold a high
    quantile (CASES) of the passing candidates' logits (sparse masks, so that the
    boxes differ), stability_score_offset a quarter of it; stability_score_thresh
    at the widest gap of the stability scores of those passing the IoU test;
    box_nms_thresh at the widest gap of the pairwise box IoUs for which the
    greedy NMS removes at least one candidate and keeps at least three."""
    low, iou, logits = candidates(name, multimask)
    th = {"pred_iou_thresh": float(widest_gap(iou.numpy())[0])}
    passing = iou > th["pred_iou_thresh"]
    th["mask_threshold"] = float(torch.quantile(logits[passing].flatten(), case(name)[6][0 if multimask else 1]))
    th["stability_score_offset"] = 0.25 * th["mask_threshold"]
    th["stability_score_thresh"] = 0.0
    s = stats(logits, iou, th)
    th["stability_score_thresh"] = float(widest_gap(s["stability"][passing].numpy())[0])
    s = stats(logits, iou, th)
    idx = [i for i in range(len(iou)) if s["passing"][i]]
    pair = sorted({float(box_iou(s["box"][i], s["box"][j], np.float64)) for a, i in enumerate(idx)
                   for j in idx[a + 1:] if not np.isnan(box_iou(s["box"][i], s["box"][j], np.float64))})
    best = None
    for a, b in zip(pair[:-1], pair[1:]):
        cut = 0.5 * (a + b)
        keep = greedy_nms(s["box"], iou, s["passing"], cut, np.float64)
        if 3 <= len(keep) < len(idx) and (best is None or b - a > best[1]):
            best = (cut, b - a)
    assert best is not None, "no NMS threshold removes one candidate and keeps three"
    th["box_nms_thresh"] = float(best[0])
    return th


def generate(name, multimask, dtype=torch.float64, th=None):
    """The twin generator: dict(keep, stats, trace, low, iou, logits) with the thresholds of choose_thresholds."""
    th = th or choose_thresholds(name, multimask)
    low, iou, logits = candidates(name, multimask, dtype)
    s = stats(logits, iou, th)
    trace = []
    npd = np.float64 if dtype == torch.float64 else np.float32
    keep = greedy_nms(s["box"], iou, s["passing"], th["box_nms_thresh"], npd, trace)
    return dict(keep=keep, stats=s, trace=trace, low=low, iou=iou, logits=logits, th=th)


def margins(name, multimask):
    """What the decided-cases test asserts, from both twins.
    iou: |iou - thresh| and the float32 twin's error, per candidate.
    stability, per candidate passing the IoU test: the decision is the sign of
    d = inter - t union, counted in pixels.  A pixel within EPS max|low_res| of
    the upper cut can move inter, and so d, by 1; one near the lower cut moves
    union by 1 and d by t.  stab_margin = |d|, stab_error = (undecided at the
    upper cut) + t (undecided at the lower cut).
    nms: |IoU - thresh| of every comparison of the float64 run, and the
    largest float32 error of a compared IoU."""
    a, b = generate(name, multimask), generate(name, multimask, torch.float32)
    th, s = a["th"], a["stats"]
    und = undecided(a["logits"], a["low"], th)
    t = th["stability_score_thresh"]
    live = s["pass_iou"]
    d = (s["inter"].double() - t * s["union"].double()).abs()
    nms_err = max([abs(x - y) for x, y in zip(a["trace"], b["trace"]) if x == x] or [0.0]) \
        if len(a["trace"]) == len(b["trace"]) else float("inf")
    return dict(iou_margin=(a["iou"] - th["pred_iou_thresh"]).abs(), iou_err=(b["iou"].double() - a["iou"]).abs(),
                stab_margin=d[live], stab_error=(und[:, 0].double() + t * und[:, 1].double())[live], undecided=und,
                nms_margin=[abs(v - th["box_nms_thresh"]) for v in a["trace"] if v == v], nms_err=nms_err,
                same=(a["keep"] == b["keep"] and torch.equal(a["stats"]["pass_iou"], b["stats"]["pass_iou"])
                      and torch.equal(a["stats"]["passing"], b["stats"]["passing"])
                      and torch.equal(a["stats"]["box"], b["stats"]["box"])),
                f64=a, f32=b)
