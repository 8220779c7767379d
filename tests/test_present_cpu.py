"""Frame presentation without a GPU: the torch mirror
(samnerf_amd.present.torch_present_frame) against the reference's recorded
results (tests/golden/present.npz) bit for bit, the C ABI's argument checks,
and the geometry of sam_bridge.PromptMemory."""
import ctypes

import numpy as np
import pytest
import torch

import present_fixtures as fx


def _mirror(*a, **k):
    from samnerf_amd.present import torch_present_frame
    return torch_present_frame(*a, **k)


# ------------------------------------------------------------ the mirror --

def test_default_color_map_is_the_references_table():
    from samnerf_amd.present import default_color_map
    cm = default_color_map()
    assert cm.dtype == torch.float32 and fx.same(cm, fx.t("color_map"))


@pytest.mark.parametrize("ci,mask_type,iid", fx.mask_views())
def test_mask_views_equal_the_recordings(ci, mask_type, iid):
    _, rH, rW, K, n_inst = fx.mask_cases()[ci]
    frame, extra = _mirror(fx.image_of(rH, rW), None, rH, rW, logits=fx.t(f"mask/{ci}/logits"), n_inst=n_inst,
                           mask_type=mask_type, instance_id=iid, color_map=fx.t("color_map"), return_extra=True)
    assert fx.same(extra["probs"], fx.t(f"mask/{ci}/probs32"))
    assert fx.same(extra["ids"], fx.t(f"mask/{ci}/ids"))
    assert fx.same(frame, fx.t(f"mask/{ci}/{mask_type}/{iid}/frame32"))


def test_the_golden_has_exact_ties_off_column_zero():
    """The first-index rule is only tested where ties exist, at varied columns."""
    for ci, _, _, K, n_inst in fx.mask_cases():
        if K == 1:
            continue
        p = fx.t(f"mask/{ci}/probs64").view(-1, K)
        top, idx = torch.topk(p, 2, dim=-1)
        tie = top[:, 0] == top[:, 1]
        assert bool(((top[:, 0] - top[:, 1] >= 1e-3) | tie).all())
        assert tie.float().mean() >= 0.05
        ids = fx.t(f"mask/{ci}/ids").view(-1)[tie]
        first = (p == p.max(-1, keepdim=True).values).int().argmax(-1)      # the first of two or more equal columns
        assert fx.same(ids, first[tie]) and (K == 2 or len(set(ids.tolist())) > 1)


@pytest.mark.parametrize("rH,rW", fx.SIZES)
def test_sam_overlay_and_clicks_equal_the_recordings(rH, rW):
    image, sam = fx.image_of(rH, rW), fx.t(f"sam/{rH}x{rW}/mask")
    assert fx.same(_mirror(image, None, rH, rW, sam_mask=sam), fx.t(f"sam/{rH}x{rW}/frame32"))
    drawn = 0
    for c in fx.CLICKS:
        pts = fx.arr(f"points/{rH}x{rW}/{c}/points")
        want = fx.t(f"points/{rH}x{rW}/{c}/frame32")
        assert fx.same(_mirror(image, None, rH, rW, points=pts), want), c
        drawn += int(not fx.same(want, image))
        if c in ("left", "top"):            # the negative start wraps: nothing is drawn
            assert fx.same(want, image)
    assert drawn == 5
    both = _mirror(image, None, rH, rW, sam_mask=sam, points=fx.arr(f"points/{rH}x{rW}/all/points"))
    assert fx.same(both, fx.t(f"sam_points/{rH}x{rW}/frame32"))


@pytest.mark.parametrize("rH,rW,H,W", fx.resize_cases())
def test_nearest_resize_equals_the_recordings(rH, rW, H, W):
    image, depth = fx.image_of(rH, rW), fx.t(f"depth/{rH}x{rW}")
    frame, extra = _mirror(image, depth, H, W, return_extra=True)
    assert fx.same(frame, fx.t(f"resize/{rH}x{rW}_{H}x{W}/image"))
    assert fx.same(extra["depth"], fx.t(f"resize/{rH}x{rW}_{H}x{W}/depth"))


@pytest.mark.parametrize("mode,dname", fx.BUFFERS)
def test_buffer_modes_and_the_spp_mean_equal_the_recordings(mode, dname):
    H, W = 33, 65
    image, depth = fx.image_of(H, W), fx.t(f"buffer/depth_{dname}/depth")
    buf = _mirror(image, depth, H, W, mode=mode)
    want = fx.t(f"buffer/{mode}_{dname}/spp0")
    assert fx.same(buf, want)
    if dname == "nan":
        assert torch.isnan(want).all()
    if dname == "constant":
        assert not want.any()
    if dname != "plain":
        return
    nxt_image, nxt_depth = fx.t("buffer/next_image"), fx.t("buffer/next_depth")
    for spp in (1, 5):
        buf = _mirror(nxt_image, nxt_depth, H, W, mode=mode, buffer=buf, spp=spp)
        assert fx.same(buf, fx.t(f"buffer/{mode}_{dname}/spp{spp}")), spp


def test_present_frame_on_cpu_tensors_is_the_mirror():
    from samnerf_amd.present import present_frame
    _, rH, rW, K, n_inst = fx.mask_cases()[3]
    kw = dict(logits=fx.t("mask/3/logits"), n_inst=n_inst, mask_type="composition", instance_id=1,
              color_map=fx.t("color_map"))
    assert fx.same(present_frame(fx.image_of(rH, rW), None, 13, 19, **kw),
                   _mirror(fx.image_of(rH, rW), None, 13, 19, **kw))
    with pytest.raises(ValueError, match="mask_type"):
        present_frame(fx.image_of(rH, rW), None, rH, rW, mask_type="heat")


# ------------------------------------------------------------ the C ABI --

def _args(**kw):
    from samnerf_amd._lib import SamnerfPresentArgs
    a = SamnerfPresentArgs()
    fake = 0x1000                      # never dereferenced: every call below fails its checks first
    a.rH, a.rW, a.H, a.W, a.K, a.n_inst, a.n_colors = 5, 7, 5, 7, 3, 3, 100
    a.image = a.depth = a.logits = a.color_map = a.buffer = fake
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("kw,why", [
    (dict(K=33, n_inst=33), "K"),
    (dict(n_inst=0), "n_inst"),
    (dict(n_inst=4), "n_inst"),
    (dict(n_colors=2), "color_map"),
    (dict(n_points=65, points=0x1000), "64 points"),
    (dict(n_points=1), "null points"),
    (dict(buffer=None), "null buffer"),
    (dict(logits=None), "logits"),
    (dict(color_map=None), "color_map"),
    (dict(mask_type=3), "mask_type"),
    (dict(mode=2), "mode"),
    (dict(mask_type=1, image=None), "image"),
    (dict(K=0, image=None), "image"),
    (dict(K=0, probs=0x1000), "need logits"),
    (dict(mode=1, depth=None), "depth"),
    (dict(depth=None, depth_out=0x1000), "depth"),
    (dict(H=0), "at least 1"),
    (dict(rH=1 << 16, rW=1 << 16), "2\\^31"),
])
def test_argument_checks(hip_lib, kw, why):
    from samnerf_amd._lib import last_error
    a = _args(**kw)
    assert hip_lib.samnerf_present_workspace_size(ctypes.byref(a)) == 0
    rc = hip_lib.samnerf_present_frame(ctypes.byref(a), None, 0, None)
    assert rc == -1                    # SAMNERF_EINVAL
    import re
    assert re.search(why, last_error()), last_error()
    assert hip_lib.samnerf_present_frame(None, None, 0, None) == -1


def test_workspace_sizes_and_the_workspace_check(hip_lib):
    from samnerf_amd._lib import last_error
    assert hip_lib.samnerf_present_workspace_size(ctypes.byref(_args())) == 0          # one pass
    a = _args(H=13, W=19)
    assert hip_lib.samnerf_present_workspace_size(ctypes.byref(a)) == 5 * 7 * 3 * 4
    assert hip_lib.samnerf_present_frame(ctypes.byref(a), None, 0, None) == -3         # SAMNERF_EWORKSPACE
    assert "420 needed" in last_error()
    assert hip_lib.samnerf_present_frame(ctypes.byref(a), 0x1000, 419, None) == -3
    d = _args(mode=1)
    assert hip_lib.samnerf_present_workspace_size(ctypes.byref(d)) == 256 * 3 * 4
    assert hip_lib.samnerf_present_frame(ctypes.byref(d), None, 0, None) == -3
    # an instance id past n_inst means "every instance", whatever its size
    assert hip_lib.samnerf_present_workspace_size(ctypes.byref(_args(H=13, W=19, instance_id=1000))) == 420


# ------------------------------------------------------- PromptMemory --

def _view(W=16, H=12, seed=3, dtype=torch.float32):
    """gui_camera's pose and the reference's full-image rays (utils.py:247-259,
    pixel centres) on the CPU."""
    from samnerf_amd import synth
    pose, intr = synth.gui_camera(W, H, rot=synth.random_rotation(seed))
    fx_, fy_, cx, cy = [float(v) for v in intr]
    j, i = torch.meshgrid(torch.arange(H, dtype=dtype) + 0.5, torch.arange(W, dtype=dtype) + 0.5, indexing="ij")
    d = torch.stack(((i - cx) / fx_, -(j - cy) / fy_, -torch.ones_like(i)), -1).reshape(-1, 3)
    p = torch.from_numpy(pose).to(dtype)
    return pose, intr, p[:3, 3].expand(H * W, 3).contiguous(), (d @ p[:3, :3].T).contiguous()


PIXELS = [[5, 3], [10, 7], [2, 9]]


def test_remembered_points_project_back_to_their_pixels():
    from samnerf_amd.sam_bridge import PromptMemory
    W, H = 16, 12
    pose, intr, ro, rd = _view(W, H)
    depth = torch.full((H, W), 0.8)
    mem = PromptMemory()
    for p in PIXELS:
        mem.update(np.array([p]), ro, rd, depth)
    assert mem.point_3d.shape == (3, 3)
    # the float64 projection stays clear of an integer, so .long() cannot hang on a rounding
    m64 = PromptMemory()
    pose64, _, ro64, rd64 = _view(W, H, dtype=torch.float64)
    for p in PIXELS:
        m64.update(np.array([p]), ro64, rd64, depth.double())
    cam = m64.camera_points(pose64.astype(np.float64))
    u = W - (float(intr[0]) * cam[:, 0] / cam[:, 2] + float(intr[2]))
    v = float(intr[1]) * cam[:, 1] / cam[:, 2] + float(intr[3])
    for c in (u, v):
        assert float((c - c.round()).abs().min()) >= 1e-3
    got = mem.project(pose, intr, depth)
    assert got.dtype == np.int64 and np.array_equal(got, np.array(PIXELS))


def test_occlusion_and_screen_tests():
    from samnerf_amd.sam_bridge import PromptMemory
    W, H = 16, 12
    pose, intr, ro, rd = _view(W, H)
    depth = torch.full((H, W), 0.8)
    mem = PromptMemory()
    for p in PIXELS:
        mem.update(np.array([p]), ro, rd, depth)
    assert mem.project(pose, intr, depth + 0.06) is None
    assert np.array_equal(mem.project(pose, intr, depth + 0.04), np.array(PIXELS))
    hidden = depth.clone()
    hidden[7, 10] += 0.06                                # one of the three behind a surface
    assert np.array_equal(mem.project(pose, intr, hidden), np.array([PIXELS[0], PIXELS[2]]))
    # a view of 8 x 6 with the same intrinsics: only the points inside its frame remain
    small = mem.project(pose, intr, torch.full((6, 8), 0.8))
    assert small is None or all(0 <= x < 8 and 0 <= y < 6 for x, y in small)
    assert PromptMemory().project(pose, intr, depth) is None


class _Decoder:
    """SamPredictor's interface; the mask is the left half of the view."""

    def reset_image(self):
        pass

    def predict_torch(self, coords, labels, mask_input=None, multimask_output=True):
        self.coords = coords
        H, W = self.original_size
        mask = (torch.arange(W) < W // 2).expand(1, 1, H, W)
        return mask, torch.ones(1, 1), torch.zeros(1, 1, 4, 4)


class _Renderer:
    def render(self, ro, rd):
        return {"samvit": torch.zeros(ro.shape[0], 256)}


def test_render_and_predict_with_memory_and_present():
    """A click is remembered, found again in the next frame without a click,
    dropped when a surface hides it; the frame carries the mask and the square."""
    from samnerf_amd.sam_bridge import PromptMemory, render_and_predict
    W, H = 16, 12
    pose, intr, ro, rd = _view(W, H)
    image = torch.rand(H, W, 3, generator=torch.Generator().manual_seed(1))
    depth = torch.full((H, W), 0.8)
    lr = (torch.zeros(12, 3), torch.zeros(12, 3), 3, 4, H, W)
    dec, mem = _Decoder(), PromptMemory()
    view = dict(image=image, depth=depth, rays_o=ro, rays_d=rd, pose=pose, intrinsics=intr)
    left = (torch.arange(W) < W // 2).expand(H, W)
    want = _mirror(image, depth, H, W, sam_mask=left, points=np.array([[5, 3]], np.int32))
    for click in (np.array([[5, 3]]), None):
        pred, out, frame = render_and_predict(_Renderer(), dec, *lr, point_coords=click, memory=mem, present=view)
        assert np.array_equal(pred[1], [[5, 3]]) and dec.coords.tolist() == [[[320.0, 192.0]]]
        assert fx.same(frame, want) and not fx.same(frame, image)
    pred, out, frame = render_and_predict(_Renderer(), dec, *lr, memory=mem, present=dict(view, depth=depth + 0.06))
    assert pred is None and fx.same(frame, image) and "samvit" in out
    # present alone: the click as given, in a depth buffer too; neither: the result as before
    pred, out, frame = render_and_predict(_Renderer(), dec, *lr, point_coords=np.array([[9, 6]]),
                                          present=dict(image=image, depth=depth, mode="depth"))
    assert np.array_equal(pred[1], [[9, 6]]) and not frame.any()
    res = render_and_predict(_Renderer(), dec, *lr, point_coords=np.array([[9, 6]]))
    assert len(res) == 2 and np.array_equal(res[0][1], [[9, 6]])
    with pytest.raises(ValueError, match="memory= needs"):
        render_and_predict(_Renderer(), dec, *lr, memory=mem, present=dict(image=image, depth=depth))


def test_add_and_remove_rule():
    """A click 0.02 from every remembered point adds one; a click within 0.005
    of a remembered point takes that point out (utils.py:1331-1345)."""
    from samnerf_amd.sam_bridge import PromptMemory

    def click(mem, p):
        mem.update(np.array([[0, 0]]), torch.tensor([p]), torch.zeros(1, 3), torch.ones(1, 1))
    mem = PromptMemory()
    click(mem, [0.1, 0.2, 0.3])
    click(mem, [0.1, 0.2, 0.32])                         # 0.02 away: added
    assert mem.point_3d.shape == (2, 3)
    click(mem, [0.1, 0.2, 0.305])                        # 0.005 from the first, 0.015 from the second
    assert torch.equal(mem.point_3d, torch.tensor([[0.1, 0.2, 0.32]]))
    click(mem, [0.1, 0.205, 0.32])                       # the last one goes: nothing is remembered
    assert mem.point_3d is None
