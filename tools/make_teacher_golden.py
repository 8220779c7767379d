#!/usr/bin/env python3
"""Generate tests/golden/teacher.npz: PIL's own Image.resize(..., BILINEAR) of
two seeded random uint8 RGB images, (5, 7) -> (16, 23) and (100, 75) ->
(64, 48), so that the teacher-image tests have PIL's bytes where PIL is not
installed.  Only data goes into the file; the PIL version is recorded with it.

usage: python tools/make_teacher_golden.py
"""
import os

import numpy as np
import PIL
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "..", "tests", "golden", "teacher.npz")
CASES = [((5, 7), (16, 23)), ((100, 75), (64, 48))]


def main():
    rng = np.random.default_rng(20261021)
    rec = {"pil_version": np.array(PIL.__version__)}
    for i, ((h, w), (oh, ow)) in enumerate(CASES):
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        rec[f"in{i}"] = img
        rec[f"out{i}"] = np.asarray(Image.fromarray(img).resize((ow, oh), Image.BILINEAR))
        assert rec[f"out{i}"].shape == (oh, ow, 3)
    np.savez_compressed(OUT, **rec)
    print(f"wrote {os.path.normpath(OUT)}: {os.path.getsize(OUT)} bytes, PIL {PIL.__version__}")


if __name__ == "__main__":
    main()
