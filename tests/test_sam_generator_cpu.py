"""The batched SAM decoder and the mask generator without a GPU: the C ABI's
refusals, the workspace size, the export table, the generator's refusals, the
point grid, and the conditions the end-to-end GPU cases must meet (every
filter and every NMS comparison decided, with a margin)."""
import ctypes
import re

import numpy as np
import pytest
import torch

import sam_generator_ref as gref

NEW = ["samnerf_sam_decoder_batch", "samnerf_sam_decoder_batch_workspace_size", "samnerf_sam_masks_select",
       "samnerf_sam_mask_stats", "samnerf_sam_nms"]


def test_header_export_table_and_ctypes_agree(hip_lib):
    import os

    from conftest import REPO
    from samnerf_amd import EXPORTED
    text = open(os.path.join(REPO, "include", "samnerf_hip.h")).read()
    for name in NEW:
        assert re.search(r"^(?:int|size_t)\s+" + name + r"\s*\(", text, re.M), name
        assert name in EXPORTED and hasattr(hip_lib, name)
    assert "#define SAMNERF_SAM_REC_WORDS 10" in text
    from samnerf_amd.sam_decoder import REC_WORDS
    from samnerf_amd.sam_generator import REC_FIELDS
    assert REC_WORDS == 10 == len(REC_FIELDS)


def test_batch_workspace_size(hip_lib):
    size = hip_lib.samnerf_sam_decoder_batch_workspace_size
    for g in (0, 4, 12, 72):
        assert size(g, 1) == 0
    for B in (0, 257, 1 << 20):
        assert size(8, B) == 0
    for g in (8, 16, 64):
        sizes = [size(g, B) for B in (1, 2, 3, 64, 255, 256)]
        assert all(a < b for a, b in zip(sizes, sizes[1:])) and sizes[0] > 0
        assert all(s % 256 == 0 for s in sizes)
    # the single call's size function stays what it was: its own carve
    assert hip_lib.samnerf_sam_decoder_workspace_size(8) > 0


def test_decoder_batch_refusals(hip_lib):
    L = hip_lib
    p = ctypes.c_void_p(4096)            # never dereferenced: validation fails first

    def call(g=8, B=2, P=1, ws=p, ws_bytes=None, pack_bytes=None, feats=p, pts=p, lab=p, low=p, iou=p, pack=p,
             h=0, w=0):
        ws_bytes = L.samnerf_sam_decoder_batch_workspace_size(g, B) if ws_bytes is None else ws_bytes
        pack_bytes = L.samnerf_sam_decoder_pack_size(g) if pack_bytes is None else pack_bytes
        return L.samnerf_sam_decoder_batch(pack, pack_bytes, g, feats, h, w, pts, lab, B, P, low, iou, ws, ws_bytes,
                                           None)
    for g in (0, 4, 12, 72):
        assert call(g=g, ws_bytes=1 << 40, pack_bytes=1 << 30) == -1 and b"multiple of 8" in L.samnerf_last_error()
    for B in (0, 257):
        assert call(B=B, ws_bytes=1 << 40) == -1 and b"B must lie in [1, 256]" in L.samnerf_last_error()
    for P in (0, 59):
        assert call(P=P) == -1 and b"P must lie in [1, 58]" in L.samnerf_last_error()
    for null in ("feats", "pts", "lab", "low", "iou", "pack"):
        assert call(**{null: None}) == -1 and b"null" in L.samnerf_last_error()
    assert call(ws=None) == -1 and b"null workspace" in L.samnerf_last_error()
    need = L.samnerf_sam_decoder_batch_workspace_size(8, 2)
    assert call(ws_bytes=need - 1) == -3 and b"workspace" in L.samnerf_last_error()
    assert call(B=3, ws_bytes=need) == -3
    assert call(ws=ctypes.c_void_p(4096 + 4)) == -1 and b"16-byte aligned" in L.samnerf_last_error()
    assert call(iou=ctypes.c_void_p(4096 + 8)) == -1 and b"16-byte aligned" in L.samnerf_last_error()
    assert call(pack_bytes=L.samnerf_sam_decoder_pack_size(8) - 1) == -1 and b"pack" in L.samnerf_last_error()
    assert call(h=5, w=0) == -1 and call(h=1025, w=4) == -1


def test_generator_kernel_refusals(hip_lib):
    L = hip_lib
    p = ctypes.c_void_p(4096)
    sel, stats, nms = L.samnerf_sam_masks_select, L.samnerf_sam_mask_stats, L.samnerf_sam_nms
    for g in (0, 12, 72):
        assert sel(p, 4, p, 4, None, g, 8, 8, 8, 8, 0.0, p, None, None) == -1
        assert stats(p, p, 4, g, 8, 8, 8, 8, 0.5, 0.0, 1.0, 0.9, p, None) == -1
    for ih, iw, H, W in ((0, 8, 8, 8), (8, 129, 8, 8), (8, 8, 0, 8), (8, 8, 8, 8193)):
        assert sel(p, 4, p, 4, None, 8, ih, iw, H, W, 0.0, p, None, None) == -1
        assert stats(p, p, 4, 8, ih, iw, H, W, 0.5, 0.0, 1.0, 0.9, p, None) == -1
    assert sel(None, 4, p, 4, None, 8, 8, 8, 8, 8, 0.0, p, None, None) == -1
    assert sel(p, 4, p, 4, None, 8, 8, 8, 8, 8, 0.0, None, None, None) == -1 and b"no output" in L.samnerf_last_error()
    assert sel(p, 0, p, 4, None, 8, 8, 8, 8, 8, 0.0, p, None, None) == -1
    assert sel(p, 4, None, 5, None, 8, 8, 8, 8, 8, 0.0, p, None, None) == -1       # identity past the table
    assert sel(p, 12289, p, 4, None, 8, 8, 8, 8, 8, 0.0, p, None, None) == -1
    assert sel(p, 4, p, 0, None, 8, 8, 8, 8, 8, 0.0, p, None, None) == 0           # nothing to do: no launch
    # n = 0 succeeds with no launch, whatever the pointers; n past 3 * 64^2 is refused
    assert stats(None, None, 0, 8, 8, 8, 8, 8, 0.5, 0.0, 1.0, 0.9, None, None) == 0
    assert nms(None, 0, 0.7, None, None, None) == 0
    assert stats(p, p, 12289, 8, 8, 8, 8, 8, 0.5, 0.0, 1.0, 0.9, p, None) == -1
    assert nms(p, 12289, 0.7, p, p, None) == -1
    for null in range(3):
        a = [p, p, p]
        a[null] = None
        assert stats(a[0], a[1], 4, 8, 8, 8, 8, 8, 0.5, 0.0, 1.0, 0.9, a[2], None) == -1
        assert nms(a[0], 4, 0.7, a[1], a[2], None) == -1 and b"null" in L.samnerf_last_error()


def test_generator_refusals_name_themselves():
    from samnerf_amd.sam_generator import DeviceMaskGenerator

    class Dec:
        g, S, device = 8, 128, torch.device("cpu")
    with pytest.raises(NotImplementedError, match="crop_n_layers"):
        DeviceMaskGenerator(Dec(), crop_n_layers=1)
    with pytest.raises(NotImplementedError, match="min_mask_region_area"):
        DeviceMaskGenerator(Dec(), min_mask_region_area=100)
    for mode in ("uncompressed_rle", "coco_rle"):
        with pytest.raises(NotImplementedError, match="RLE"):
            DeviceMaskGenerator(Dec(), output_mode=mode)
    with pytest.raises(ValueError, match="points_per_batch"):
        DeviceMaskGenerator(Dec(), points_per_batch=257)
    gen = DeviceMaskGenerator(Dec())
    assert gen.points_per_side == 32 and gen.pred_iou_thresh == 0.88 and gen.stability_score_thresh == 0.95
    assert gen.stability_score_offset == 1.0 and gen.box_nms_thresh == 0.7 and gen.max_masks == 256


@pytest.mark.parametrize("n", [1, 4, 32])
def test_point_grid_is_the_definition(n):
    from samnerf_amd.sam_generator import build_point_grid
    grid = build_point_grid(n)
    assert grid.shape == (n * n, 2) and grid.dtype == np.float64
    for k in sorted({0, min(1, n * n - 1), min(n, n * n - 1), n * n - 1}):
        y, x = divmod(k, n)
        assert abs(grid[k, 0] - (x + 0.5) / n) < 1e-15 and abs(grid[k, 1] - (y + 0.5) / n) < 1e-15
    assert np.abs(grid - gref.point_grid(n)).max() < 1e-15


def test_points_are_scaled_into_the_input_frame():
    from samnerf_amd.sam_generator import DeviceMaskGenerator

    class Dec:
        g, S, device = 8, 128, torch.device("cpu")
    x = gref.case_inputs("g8_4x4")
    view, inp = DeviceMaskGenerator(Dec(), points_per_side=4).points_for(x["H"], x["W"])
    assert np.abs(view - x["points_view"]).max() < 1e-12 and np.abs(inp - x["points_in"]).max() < 1e-12
    assert x["input_size"] == (64, 128) and abs(inp[5, 0] - (1.5 / 4) * 128) < 1e-9
    assert abs(inp[5, 1] - (1.5 / 4) * 33 * (64 / 33)) < 1e-9


@pytest.mark.parametrize("multimask", [True, False])
@pytest.mark.parametrize("name", gref.CASE_NAMES)
def test_the_cases_are_decided(name, multimask):
    """The end-to-end GPU cases compare decisions, so every decision must have
    a margin: the float64 and float32 twins decide alike at every filter and
    every NMS comparison, and every margin is at least ten times the float32
    twin's own error in that quantity (sam_generator_ref.margins)."""
    m = gref.margins(name, multimask)
    a, s = m["f64"], m["f64"]["stats"]
    assert m["same"], "the float32 twin takes another decision somewhere"
    assert len(a["trace"]) == len(m["f32"]["trace"])
    assert bool((m["iou_margin"] >= 10 * m["iou_err"]).all())
    assert bool((m["stab_margin"] >= 10 * m["stab_error"]).all()) and bool((m["stab_margin"] > 0).all())
    assert min(m["nms_margin"]) >= max(10 * m["nms_err"], 1e-5)
    n, n_iou, n_pass = len(a["iou"]), int(s["pass_iou"].sum()), int(s["passing"].sum())
    assert 0.25 <= n_iou / n <= 0.75, (n_iou, n)
    assert 0.25 <= n_pass / n_iou <= 0.75, (n_pass, n_iou)
    assert 3 <= len(a["keep"]) < n_pass, (a["keep"], n_pass)
    # what the GPU test allows in area and bbox: the undecided pixels of the mask's own cut are few
    assert int(m["undecided"][:, 2].max()) <= 8
