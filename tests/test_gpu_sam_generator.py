"""The mask generator's kernels and DeviceMaskGenerator on the GPU.  The stats
are integer counts and min / max over the device's own logits, the NMS is
decided comparisons: both are compared exactly.  The end-to-end cases are
those test_sam_generator_cpu.py shows to be decided, against the float64 twin
(sam_generator_ref)."""
import functools

import numpy as np
import pytest
import torch

import sam_decoder_ref as ref
import sam_generator_ref as gref

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def decoder(g):
    from samnerf_amd.sam_decoder import SamDecoder
    return SamDecoder.from_state_dict(ref.state_dict(), g=g, device="cuda:0")


@functools.lru_cache(maxsize=None)
def table(g, n):
    """n candidates (low_res [n, 4g, 4g], iou [n]) from the device's own decoder."""
    gen = torch.Generator().manual_seed(40 + g + n)
    dec, B = decoder(g), (n + 2) // 3
    feats = torch.randn(g * g, 256, generator=gen).to("cuda:0")
    pts = (torch.rand(B, 1, 2, generator=gen) * (16 * g - 1)).to("cuda:0")
    low, iou = dec.decode_batch(feats, pts)
    return low[:, 1:].reshape(-1, 4 * g, 4 * g)[:n].contiguous(), iou[:, 1:].reshape(-1)[:n].contiguous()


def f32(x):
    return float(np.float32(x))


def fields(rec):
    """The int32 records [n, 10] as a dict of host tensors."""
    r = rec.cpu()
    return dict(inter=r[:, 0], union=r[:, 1], area=r[:, 2], box=r[:, 3:7], stability=r[:, 7].view(torch.float32),
                passing=r[:, 8], iou=r[:, 9].view(torch.float32))


@pytest.mark.parametrize("g,H,W,n", [(8, 20, 15, 1), (8, 33, 65, 3), (8, 33, 65, 48), (16, 64, 64, 3), (16, 64, 64, 48)])
def test_stats_are_exact_against_the_devices_own_logits(hip_lib, cuda, g, H, W, n):
    dec = decoder(g)
    low, iou = table(g, n)
    low, iou = low.clone(), iou.clone()
    if n >= 3:                                   # an all-positive and an all-negative mask, both past the IoU test
        low[0] = low[0].abs() + 3.0
        low[1] = -low[1].abs() - 3.0
        iou[:2] = iou.max() + 1.0
    size, _ = ref.input_size_for(H, W, g)
    thr, off = f32(0.3), f32(0.7)
    iou_t = f32(iou.median().item() - 1e-3) if n > 1 else f32(iou.item() - 1.0)
    logits = dec.masks_select(low, size, (H, W), logits=True)
    assert logits.shape == (n, H, W)
    hi, lo = f32(np.float32(thr) + np.float32(off)), f32(np.float32(thr) - np.float32(off))
    inter, union = (logits > hi).flatten(1).sum(1), (logits > lo).flatten(1).sum(1)
    mask = logits > thr
    stab = inter.float() / union.float()
    stab_t = f32(stab[~stab.isnan()].median().item())
    got = fields(dec.mask_stats(low, iou, size, (H, W), iou_t, stab_t, off, thr))
    live = (iou > iou_t).cpu()
    assert live.any() and (n == 1 or not live.all())
    box = gref.boxes_of(mask.cpu())
    if n >= 3:
        assert mask[0].all() and not mask[1].any()
        assert box[0].tolist() == [0, 0, W - 1, H - 1] and box[1].tolist() == [0, 0, 0, 0]
    for key, want in (("inter", inter), ("union", union), ("area", mask.flatten(1).sum(1)), ("box", box)):
        want = want.cpu().to(torch.int32)
        want[~live] = 0
        assert torch.equal(got[key], want), key
    want_stab = torch.where(live, stab.cpu(), torch.zeros(n))
    assert torch.equal(got["stability"].isnan(), want_stab.isnan())           # a NaN's payload is nobody's promise
    assert torch.equal(got["stability"].nan_to_num(2.0).view(torch.int32), want_stab.nan_to_num(2.0).view(torch.int32))
    assert torch.equal(got["passing"].bool(), live & (stab.cpu() >= stab_t))
    assert torch.equal(got["iou"].view(torch.int32), torch.where(live, iou.cpu(), torch.zeros(n)).view(torch.int32))
    if n >= 3:
        assert got["passing"][0] == (1.0 >= stab_t) and got["passing"][1] == 0        # 0 / 0 is NaN and fails


@pytest.mark.parametrize("g,H,W", [(8, 33, 65), (16, 48, 64)])
def test_masks_select_is_sam_masks_on_the_gathered_rows(hip_lib, cuda, g, H, W):
    dec = decoder(g)
    low, _ = table(g, 48)
    size, _ = ref.input_size_for(H, W, g)
    index = torch.tensor([47, 0, 13, 13, 5, 30, 2], dtype=torch.int32, device=cuda)
    want_l = torch.cat([dec.masks(low[index[a:a + 4].long()], size, (H, W), logits=True) for a in (0, 4)])
    want_m = torch.cat([dec.masks(low[index[a:a + 4].long()], size, (H, W)) for a in (0, 4)])
    assert torch.equal(dec.masks_select(low, size, (H, W), index=index, logits=True).view(torch.int32),
                       want_l.view(torch.int32))
    assert torch.equal(dec.masks_select(low, size, (H, W), index=index), want_m)
    assert torch.equal(dec.masks_select(low[:4], size, (H, W)), dec.masks(low[:4], size, (H, W)))
    # a device-side count below the capacity: rows at and past it keep their fill
    count = torch.tensor([3], dtype=torch.int32, device=cuda)
    out_l = torch.full((7, H, W), float("nan"), device=cuda)
    out_m = torch.full((7, H, W), 77, dtype=torch.uint8, device=cuda)
    dec.masks_select(low, size, (H, W), index=index, count=count, logits=True, out=out_l)
    dec.masks_select(low, size, (H, W), index=index, count=count, out=out_m)
    assert torch.equal(out_l[:3].view(torch.int32), want_l[:3].view(torch.int32)) and bool(out_l[3:].isnan().all())
    assert torch.equal(out_m[:3].bool(), want_m[:3]) and bool((out_m[3:] == 77).all())
    # an index outside the table writes nothing
    bad = torch.tensor([1, 48, -1], dtype=torch.int32, device=cuda)
    out_m.fill_(77)
    dec.masks_select(low, size, (H, W), index=bad, out=out_m[:3])
    assert torch.equal(out_m[0].bool(), dec.masks(low[1:2], size, (H, W))[0]) and bool((out_m[1:] == 77).all())


# ---------------------------------------------------------------------- NMS --

def built(n, kind, seed):
    """Records of n boxes and scores on a grid coarse enough that no pair's IoU is near a threshold by accident."""
    rng = np.random.RandomState(seed)
    rec = np.zeros((n, 10), np.int32)
    x0, y0 = rng.randint(0, 40, n), rng.randint(0, 40, n)
    w, h = rng.randint(1, 30, n), rng.randint(1, 30, n)
    score = rng.rand(n).astype(np.float32)
    passing = (rng.rand(n) < 0.8).astype(np.int32)
    if kind == "ties":
        score = (rng.randint(0, 4, n) / 4).astype(np.float32)
    elif kind == "zero_area":
        w[::3] = 0
        h[1::5] = 0
    elif kind == "identical":
        x0[:], y0[:], w[:], h[:] = 3, 4, 10, 12
        x0[n // 2:] = 30
    elif kind == "all_fail":
        passing[:] = 0
    rec[:, 3], rec[:, 4], rec[:, 5], rec[:, 6] = x0, y0, x0 + w, y0 + h
    rec[:, 8] = passing
    rec[:, 9] = score.view(np.int32)
    return rec, score, passing


NMS_CASES = [(n, "plain") for n in (1, 2, 64, 65, 257, 1000)] + \
    [(65, "ties"), (257, "zero_area"), (64, "identical"), (65, "all_fail"), (1000, "ties")]


@pytest.mark.parametrize("n,kind", NMS_CASES)
def test_nms_is_the_python_greedy_rule(hip_lib, cuda, n, kind):
    rec, score, passing = built(n, kind, 7 * n + len(kind))
    thresh = f32(0.37)
    boxes = rec[:, 3:7]
    trace = []
    want = gref.greedy_nms(boxes, score, passing, thresh, trace=trace)
    # the precondition: no IoU the rule compares lies within 1e-5 of the threshold
    assert all(v != v or abs(v - thresh) > 1e-5 for v in trace)
    dec = decoder(8)
    keep = torch.full((n,), 12345, dtype=torch.int32, device=cuda)
    count = torch.full((1,), -7, dtype=torch.int32, device=cuda)
    dec.nms(torch.from_numpy(rec).to(cuda), thresh, out=(keep, count))
    assert count.item() == len(want)
    assert keep[:len(want)].tolist() == want
    assert bool((keep[len(want):] == -1).all())
    if kind == "all_fail":
        assert count.item() == 0
    elif kind == "identical":
        assert len(want) == 2
    elif n >= 64 and kind == "plain":
        assert 1 < len(want) < int(passing.sum())


# --------------------------------------------------------------- end to end --

def generator(name, multimask, **kw):
    from samnerf_amd.sam_generator import DeviceMaskGenerator
    x, th = gref.case_inputs(name), gref.choose_thresholds(name, multimask)
    args = dict(points_per_side=x["side"], points_per_batch=x["chunk"], pred_iou_thresh=th["pred_iou_thresh"],
                stability_score_thresh=th["stability_score_thresh"],
                stability_score_offset=th["stability_score_offset"], box_nms_thresh=th["box_nms_thresh"],
                mask_threshold=th["mask_threshold"])
    args.update(kw)
    return DeviceMaskGenerator(decoder(x["g"]), **args), x["features"].float().to("cuda:0").contiguous(), x


@pytest.mark.parametrize("multimask", [True, False])
@pytest.mark.parametrize("name", gref.CASE_NAMES)
def test_generate_against_the_float64_twin(hip_lib, cuda, name, multimask):
    gen, feats, x = generator(name, multimask)
    H, W = x["H"], x["W"]
    anns = gen.generate(feats, H, W, multimask_output=multimask)
    twin, yard = gref.generate(name, multimask), gref.generate(name, multimask, torch.float32)
    s, th = twin["stats"], twin["th"]
    assert [a["candidate"] for a in anns] == twin["keep"] and gen.truncated is False
    und_all = gref.undecided(twin["logits"], twin["low"], th)
    und = und_all[:, 2]
    M = 3 if multimask else 1
    bar = ref.rel_err(yard["iou"], twin["iou"])
    eps = gref.EPS * twin["low"].abs().max()
    for a in anns:
        c = a["candidate"]
        slack = int(und[c])
        assert abs(a["area"] - int(s["area"][c])) <= slack
        x0, y0, x1, y1 = s["box"][c].tolist()
        assert all(abs(p - q) <= slack for p, q in zip(a["bbox"], [x0, y0, x1 - x0, y1 - y0]))
        assert a["crop_box"] == [0, 0, W, H]
        assert np.allclose(a["point_coords"][0], x["points_view"][c // M], rtol=0, atol=1e-9)
        err = abs(a["predicted_iou"] - float(twin["iou"][c])) / float(twin["iou"].abs().max())
        print(f"sam_generator {name} candidate {c}: iou error {err:.3e}, float32 twin {bar:.3e}")
        assert err <= 4 * bar or err <= 1e-5
        near = int(und_all[c, :2].sum())                     # pixels that may move inter or union by one
        assert abs(a["stability_score"] - float(s["stability"][c])) <= near / max(1, int(s["union"][c]) - near) + 1e-6
        decided = (twin["logits"][c] - th["mask_threshold"]).abs() > eps
        assert decided.double().mean().item() >= 0.99
        seg = a["segmentation"]
        assert seg.dtype == torch.bool and seg.shape == (H, W)
        assert bool(((seg.cpu() == s["mask"][c]) | ~decided).all())
        assert a["area"] == int(seg.sum())


def test_generate_repeats_truncates_and_stays_on_the_device(hip_lib, cuda):
    name, multimask = gref.CASE_NAMES[0], True
    gen, feats, x = generator(name, multimask)
    H, W = x["H"], x["W"]
    a = gen.generate(feats, H, W, as_tensors=True)
    torch.empty(1 << 20, device=cuda).normal_()
    b = gen.generate(feats, H, W, as_tensors=True)
    for k in ("masks", "records", "keep", "count"):
        assert a[k].is_cuda and torch.equal(a[k], b[k]), k
    n_keep = int(a["count"].item())
    assert n_keep == len(gref.generate(name, multimask)["keep"]) >= 3
    assert a["masks"].shape == (min(256, 48), H, W) and not a["masks"][n_keep:].any()
    # the same through the rendered-map entry of the bridge, and a view of the table as a map
    from samnerf_amd.sam_bridge import segment_everything
    full = gen.generate(feats, H, W)
    small, _, _ = generator(name, multimask, max_masks=2)
    cut = small.generate(feats, H, W)
    assert small.truncated is True and gen.truncated is False and len(cut) == 2
    for p, q in zip(cut, full[:2]):
        assert p["candidate"] == q["candidate"] and p["bbox"] == q["bbox"] and p["area"] == q["area"]
        assert torch.equal(p["segmentation"], q["segmentation"])
    again = segment_everything(gen, H, W, feats)
    assert [p["candidate"] for p in again] == [p["candidate"] for p in full]


def test_as_tensors_makes_no_host_copy(hip_lib, cuda):
    """With as_tensors=True nothing is read back and nothing synchronises:
    torch's sync debug mode turns any blocking copy or .item() into an error."""
    name, multimask = gref.CASE_NAMES[0], False
    gen, feats, x = generator(name, multimask)
    gen.generate(feats, x["H"], x["W"], multimask_output=False, as_tensors=True)      # the grid's upload, once
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = gen.generate(feats, x["H"], x["W"], multimask_output=False, as_tensors=True)
        with pytest.raises(RuntimeError):
            out["count"].item()                                                       # the mode does catch a read
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert all(out[k].is_cuda for k in ("masks", "records", "keep", "count"))
    assert out["count"].item() == len(gref.generate(name, multimask)["keep"])
