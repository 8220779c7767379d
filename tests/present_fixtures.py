"""tests/golden/present.npz (tools/make_present_golden.py): the reference's own
frame presentation, recorded.  Loaded once and shared; the arrays are handed
out as fresh tensors, so no test changes what another reads."""
import json

import golden_file

_G = golden_file.loader("present.npz")
GOLDEN, _file, arr, t, has, same = _G.path, _G._file, _G.arr, _G.t, _G.has, _G.same
MASK_TYPES = ("heatmap", "composition", "mask")
CLICKS = ("interior", "left", "top", "right", "bottom", "corner", "all")
SIZES = [(5, 7), (33, 65)]
BUFFERS = [("image", "plain"), ("depth", "plain"), ("depth", "constant"), ("depth", "nan")]


def mask_cases():
    """[(index, rH, rW, K, n_inst)]"""
    return [(i, *c) for i, c in enumerate(json.loads(str(_file()["mask/cases"])))]


def resize_cases():
    return [tuple(c) for c in json.loads(str(_file()["resize/cases"]))]


def instance_ids(K, n_inst):
    """The generator's: -1, an id in range, one >= n_inst."""
    return (-1, min(1, n_inst - 1), n_inst)


def mask_views():
    """Every (case, mask_type, instance_id) of the file, as pytest ids."""
    return [(ci, mt, iid) for ci, _, _, K, n in mask_cases() for mt in MASK_TYPES for iid in instance_ids(K, n)]


def image_of(rH, rW):
    return t(f"image/{rH}x{rW}")
