"""The teacher image in numpy: what csrc/teacher_image.hip computes, restated
from include/samnerf_hip.h so that the GPU tests need no PIL.

  preprocess_shape   ResizeLongestSide.get_preprocess_shape
  quantise           (v * 255).astype(uint8) of an fp32 render in [0, 1]
  coefficients       one axis of PIL's 8-bit bilinear resize: per output index
                     the first tap and the 22-bit integer weights
  resize_u8          the horizontal and then the vertical pass, the
                     intermediate image rounded to uint8 between them
  normalise_pad      Sam.preprocess: (u8 - mean) / std as CHW in an S x S plane,
                     zeros right of and below the image
  teacher_image      the four together

tests/test_teacher_cpu.py holds it against PIL.Image.resize itself, bit for
bit, and against PIL's recorded outputs (tests/golden/teacher.npz).
"""
import math

import numpy as np

PIXEL_MEAN = (123.675, 116.28, 103.53)
PIXEL_STD = (58.395, 57.12, 57.375)
PRECISION_BITS = 22

# the shapes (h, w) -> (oh, ow) at which the restatement was held against PIL
PIL_SHAPES = [((5, 7), (16, 23)), ((64, 64), (128, 128)), ((37, 53), (715, 1024)), ((100, 75), (64, 48)),
              ((33, 65), (17, 1024)), ((9, 9), (9, 20)), ((300, 200), (1024, 683)), ((1200, 900), (1024, 768)),
              ((7, 5), (3, 2))]


def preprocess_shape(H, W, target=1024):
    scale = target * 1.0 / max(H, W)
    return int(H * scale + 0.5), int(W * scale + 0.5)


def quantise(rgb):
    rgb = np.asarray(rgb, np.float32)
    return (rgb * np.float32(255.0)).astype(np.int32).astype(np.uint8)


def taps_per_index(n_in, n_out):
    """The row length of an axis's coefficient table: 2 ceil(support) + 1."""
    return int(math.ceil(max(n_in / n_out, 1.0))) * 2 + 1


def coefficients(n_in, n_out):
    """[(xmin, [k ...])] per output index; Python floats are C doubles and
    int() truncates as the C cast does."""
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = fs
    ss = 1.0 / fs
    out = []
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(0, int(center - support + 0.5))
        n = min(n_in, int(center + support + 0.5)) - xmin
        w = []
        ww = 0.0
        for x in range(n):
            a = abs((x + xmin - center + 0.5) * ss)
            v = 1.0 - a if a < 1.0 else 0.0
            w.append(v)
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        out.append((xmin, [int(0.5 + v * float(1 << PRECISION_BITS)) for v in w]))
    return out


def _pass(img, n_out):
    """One pass along axis 0 of a uint8 array [n_in, ...]."""
    res = np.empty((n_out,) + img.shape[1:], np.uint8)
    src = img.astype(np.int64)
    for xx, (xmin, k) in enumerate(coefficients(img.shape[0], n_out)):
        acc = np.full(img.shape[1:], 1 << (PRECISION_BITS - 1), np.int64)
        for t, kv in enumerate(k):
            acc += kv * src[xmin + t]
        assert acc.max() < 2 ** 31                                   # the kernel's int32 holds it
        res[xx] = np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)
    return res


def resize_u8(img, oh, ow):
    """img uint8 [h, w, 3] -> [oh, ow, 3]."""
    img = np.ascontiguousarray(img, np.uint8)
    tmp = _pass(img.transpose(1, 0, 2), ow).transpose(1, 0, 2)       # horizontal
    return np.ascontiguousarray(_pass(tmp, oh))                       # vertical


def normalise_pad(u8, S, mean=PIXEL_MEAN, std=PIXEL_STD):
    oh, ow = u8.shape[:2]
    out = np.zeros((3, S, S), np.float32)
    m, s = np.asarray(mean, np.float32), np.asarray(std, np.float32)
    out[:, :oh, :ow] = ((u8.astype(np.float32) - m) / s).transpose(2, 0, 1)
    return out


def teacher_image(rgb, oh, ow, S, mean=PIXEL_MEAN, std=PIXEL_STD):
    """rgb fp32 [H, W, 3] in [0, 1] -> (u8 [oh, ow, 3], input [3, S, S])."""
    u8 = resize_u8(quantise(rgb), oh, ow)
    return u8, normalise_pad(u8, S, mean, std)


def edge_values():
    """Every k / 255 with its two fp32 neighbours, inside [0, 1]: where the
    truncating quantisation changes its result."""
    k = (np.arange(256, dtype=np.float32) / np.float32(255.0)).astype(np.float32)
    v = np.concatenate([np.nextafter(k, np.float32(-1)), k, np.nextafter(k, np.float32(2))])
    return np.clip(v, 0.0, 1.0).astype(np.float32)
