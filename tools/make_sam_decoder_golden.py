#!/usr/bin/env python3
"""tests/golden/sam_decoder.npz: the float64 twin's low_res and iou of the
g = 8 cases of tests/sam_decoder_ref.py, which pin the twin against drift.
usage: python tools/make_sam_decoder_golden.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "segment-anything-nerf_amd"), ROOT):
    sys.path.insert(0, p)

import sam_decoder_ref as ref  # noqa: E402

out = {}
for name in ref.GOLDEN_CASES:
    low, iou, _ = ref.twin_outputs(name)
    out[name + ".low_res"], out[name + ".iou"] = low.numpy(), iou.numpy()
path = os.path.join(ROOT, "tests", "golden", "sam_decoder.npz")
np.savez_compressed(path, **out)
print(path, os.path.getsize(path), "bytes")
