"""tests/golden/eval.npz (tools/make_eval_golden.py): the reference's own
evaluation, recorded; and the float64 SSIM oracle, which has no recording
(torchmetrics is not installed where the file is made).  Loaded once and
shared; arrays are handed out as fresh tensors."""
import functools
import json

import numpy as np
import torch

import golden_file

_G = golden_file.loader("eval.npz")
GOLDEN, _file, arr, t, has, same = _G.path, _G._file, _G.arr, _G.t, _G.has, _G.same
EPSILON = 0.000001


def rgb_cases():
    """[(index, H, W, C)]"""
    return [(i, *c) for i, c in enumerate(json.loads(str(_file()["rgb/cases"])))]


def mask_cases():
    """[(index, H, W, K, n_inst, labels kind)]"""
    return [(i, *c) for i, c in enumerate(json.loads(str(_file()["mask/cases"])))]


@functools.lru_cache(maxsize=None)
def ssim64(ci):
    """The definition of the issue, evaluated in float64 with numpy on RGB case
    ci's prediction and composited truth: the float32 window weights
    g[i] = exp(-((i - 5) / 1.5)^2 / 2) / sum, the 2-D window their outer product,
    the five windowed means over the windows wholly inside the image,
    L = max(max p - min p, max t - min t), c1 = (0.01 L)^2, c2 = (0.03 L)^2, the
    mean of ((2 E[p] E[t] + c1)(2 s_pt + c2)) / ((E[p]^2 + E[t]^2 + c1)(s_p + s_t + c2))."""
    return ssim64_of(arr(f"rgb/{ci}/pred"), arr(f"rgb/{ci}/gt32"))


def window32():
    """The float32 window: the float64 evaluation of the formula, rounded once.
    (A float32 evaluation depends on the exp at hand in its last bits.)"""
    d = (np.arange(11, dtype=np.float64) - 5) / 1.5
    g = np.exp(-(d * d) / 2)
    return (g / g.sum()).astype(np.float32)


def ssim64_of(p, tr):
    p, tr = np.asarray(p, np.float64), np.asarray(tr, np.float64)
    g = window32().astype(np.float64)
    win = np.outer(g, g)

    def mean(x):                                   # [H, W, 3] -> [H - 10, W - 10, 3]
        v = np.lib.stride_tricks.sliding_window_view(x, (11, 11), axis=(0, 1))    # [H-10, W-10, 3, 11, 11]
        return (v * win).sum((-1, -2))
    L = max(p.max() - p.min(), tr.max() - tr.min())
    c1, c2 = (0.01 * L) ** 2, (0.03 * L) ** 2
    mp, mt = mean(p), mean(tr)
    sp, st, spt = mean(p * p) - mp * mp, mean(tr * tr) - mt * mt, mean(p * tr) - mp * mt
    v = ((2 * mp * mt + c1) * (2 * spt + c2)) / ((mp * mp + mt * mt + c1) * (sp + st + c2))
    return float(v.mean())
