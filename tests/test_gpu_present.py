"""samnerf_present_frame (csrc/present.hip) through samnerf_amd.present.

Bit for bit against the reference's recordings (tests/golden/present.npz)
wherever no exp is involved -- the argmax ids, the mask and composition
views, the SAM overlay, the click squares, the nearest resize, the depth
buffer and the spp mean -- and against the torch mirror run on the same GPU in
every mode (the kernels sum the softmax as ATen's GPU softmax does).

Tolerance where an exp is involved and the recording is the CPU's.  d_ref is
the distance between the reference's float32 recording and its float64
evaluation of the same inputs.  The kernels are another float32 evaluation of
the same formula (another expf, the sum in another fixed order), so their
distance from the float64 evaluation is bounded by M_REF * d_ref + one float32
ulp of the quantity's largest magnitude (the ulp covers a d_ref of 0), as in
tests/test_gpu_mask_loss.py.
"""
import numpy as np
import pytest
import torch

import present_fixtures as fx

pytestmark = pytest.mark.gpu

# Twice the worst ratio (error - ulp) / d_ref measured on the MI355X over the
# six K > 1 cases of the file (each prints its own as "RATIO ..."):
#   probabilities  0.52  (33 x 65, K = 5; 0.48 at 17 x 17, K = 32)
#   heatmap frame  0.50  (33 x 65, K = 5, every instance by its argmax)
# The kernels' error is at or below the reference's own everywhere: err and
# d_ref are both 1.2e-7 or less, and the ratio only counts what exceeds one ulp.
M_REF = 1.04
# Twice the largest distance, in float32 ulps, between the kernel's sigmoid
# (n_inst == 1) and torch.sigmoid on the same device.  Measured on the MI355X
# at K = 1 and K = 3, logits out to +-30: 0 ulps, so the bound is equality.
SIGMOID_ULPS = 0


def _ulp(x):
    return float(np.spacing(np.float32(x.abs().max().item())))


def _dist(a, b):
    return float((a.double() - b.double()).abs().max())


def _to(dev, v):
    return v.to(dev) if torch.is_tensor(v) else v


def _hip(cuda, image, depth, H, W, **kw):
    from samnerf_amd.present import present_frame
    out = present_frame(_to(cuda, image), _to(cuda, depth), H, W, **{k: _to(cuda, v) for k, v in kw.items()})
    if isinstance(out, tuple):
        return out[0].cpu(), {k: (v.cpu() if v is not None else None) for k, v in out[1].items()}
    return out.cpu()


def _mirror(dev, image, depth, H, W, **kw):
    from samnerf_amd.present import torch_present_frame
    out = torch_present_frame(_to(dev, image), _to(dev, depth), H, W, **{k: _to(dev, v) for k, v in kw.items()})
    if isinstance(out, tuple):
        return out[0].cpu(), {k: (v.cpu() if v is not None else None) for k, v in out[1].items()}
    return out.cpu()


def _case(ci):
    _, rH, rW, K, n_inst = fx.mask_cases()[ci]
    return rH, rW, K, n_inst, fx.image_of(rH, rW), dict(logits=fx.t(f"mask/{ci}/logits"), n_inst=n_inst,
                                                       color_map=fx.t("color_map"))


@pytest.mark.parametrize("ci", range(7))
def test_ids_mask_and_composition_views_equal_the_recordings(hip_lib, cuda, ci):
    rH, rW, K, n_inst, image, kw = _case(ci)
    for mask_type in ("mask", "composition"):
        for iid in fx.instance_ids(K, n_inst):
            frame, extra = _hip(cuda, image, None, rH, rW, mask_type=mask_type, instance_id=iid, return_extra=True,
                                **kw)
            assert fx.same(extra["ids"], fx.t(f"mask/{ci}/ids")), (mask_type, iid)
            assert fx.same(frame, fx.t(f"mask/{ci}/{mask_type}/{iid}/frame32")), (mask_type, iid)


@pytest.mark.parametrize("ci", range(1, 7))
def test_probabilities_and_heatmap_within_the_references_own_error(hip_lib, cuda, ci):
    rH, rW, K, n_inst, image, kw = _case(ci)
    bad = []
    for iid in fx.instance_ids(K, n_inst):
        frame, extra = _hip(cuda, image, None, rH, rW, mask_type="heatmap", instance_id=iid, return_extra=True, **kw)
        assert fx.same(extra["ids"], fx.t(f"mask/{ci}/ids"))
        for name, got, r32, r64 in (("probs", extra["probs"], fx.t(f"mask/{ci}/probs32"), fx.t(f"mask/{ci}/probs64")),
                                    ("heatmap", frame, fx.t(f"mask/{ci}/heatmap/{iid}/frame32"),
                                     fx.t(f"mask/{ci}/heatmap/{iid}/frame64"))):
            d_ref, ulp, err = _dist(r32, r64), _ulp(r64), _dist(got, r64)
            ratio = max(err - ulp, 0.0) / d_ref if d_ref > 0 else (0.0 if err <= ulp else float("inf"))
            print(f"RATIO case {ci} {rH}x{rW} K={K} id={iid} {name}: err={err:.3e} d_ref={d_ref:.3e} "
                  f"ulp={ulp:.3e} ratio={ratio:.2f}")
            if not err <= M_REF * d_ref + ulp:
                bad.append((name, iid, err, d_ref, ulp))
    assert not bad, bad


def _ulps_apart(a, b):
    """Distance in float32 ulps (both finite, same sign: probabilities)."""
    ia, ib = a.contiguous().view(torch.int32).long(), b.contiguous().view(torch.int32).long()
    return int((ia - ib).abs().max())


def test_sigmoid_against_the_devices_own(hip_lib, cuda):
    """n_inst == 1: K = 1 from the file, and K = 3 (one instance, two redundant columns)."""
    rH, rW, K, n_inst, image, kw = _case(0)
    worst = 0
    for z in (kw["logits"], fx.t("mask/2/logits"), torch.linspace(-30, 30, 35 * 3).view(5, 7, 3)):
        frame, extra = _hip(cuda, image, None, rH, rW, mask_type="heatmap", instance_id=-1, return_extra=True,
                            logits=z, n_inst=1, color_map=kw["color_map"])
        want = torch.sigmoid(z.to(cuda)).cpu()
        u = _ulps_apart(extra["probs"], want)
        print(f"SIGMOID K={z.shape[-1]}: {u} ulps from torch.sigmoid on the device")
        worst = max(worst, u)
        # the rest follows from the kernel's own probabilities without an exp: exact
        assert fx.same(extra["ids"], extra["probs"].argmax(-1))
        assert fx.same(frame, kw["color_map"][extra["ids"]] * extra["probs"].max(-1).values[..., None])
    assert worst <= SIGMOID_ULPS


@pytest.mark.parametrize("ci", range(1, 7))
def test_every_mode_equals_the_mirror_on_the_same_gpu(hip_lib, cuda, ci):
    """K > 1: present_frame and the reference's op sequence on the same device, bit for bit."""
    rH, rW, K, n_inst, image, kw = _case(ci)
    depth = 0.3 + torch.rand(rH, rW, generator=torch.Generator().manual_seed(ci))
    sam = torch.rand(rH, rW, generator=torch.Generator().manual_seed(50 + ci)) < 0.4
    pts = np.array([[rW // 2, rH // 2], [rW - 1, rH - 1], [1, 1]], np.int32)
    for mask_type in fx.MASK_TYPES:
        for iid in fx.instance_ids(K, n_inst):
            a = _hip(cuda, image, depth, rH, rW, mask_type=mask_type, instance_id=iid, return_extra=True, **kw)
            b = _mirror(cuda, image, depth, rH, rW, mask_type=mask_type, instance_id=iid, return_extra=True, **kw)
            assert fx.same(a[0], b[0]), (mask_type, iid)
            for k in ("probs", "ids", "depth"):
                assert fx.same(a[1][k], b[1][k]), (mask_type, iid, k)
        # overlays, the resize and the spp mean on top of the view; then the depth buffer
        full = dict(kw, mask_type=mask_type, instance_id=1, sam_mask=sam, points=pts)
        prev = torch.rand(2 * rH + 3, 3 * rW - 2, 3, generator=torch.Generator().manual_seed(9))
        for mode in ("image", "depth"):
            a = _hip(cuda, image, depth, 2 * rH + 3, 3 * rW - 2, mode=mode, buffer=prev.clone(), spp=3, **full)
            b = _mirror(cuda, image, depth, 2 * rH + 3, 3 * rW - 2, mode=mode, buffer=prev.clone(), spp=3, **full)
            assert fx.same(a, b), (mask_type, mode)


@pytest.mark.parametrize("rH,rW", fx.SIZES)
def test_sam_overlay_and_clicks_equal_the_recordings(hip_lib, cuda, rH, rW):
    image, sam = fx.image_of(rH, rW), fx.t(f"sam/{rH}x{rW}/mask")
    assert fx.same(_hip(cuda, image, None, rH, rW, sam_mask=sam), fx.t(f"sam/{rH}x{rW}/frame32"))
    for c in fx.CLICKS:
        got = _hip(cuda, image, None, rH, rW, points=fx.arr(f"points/{rH}x{rW}/{c}/points"))
        assert fx.same(got, fx.t(f"points/{rH}x{rW}/{c}/frame32")), c
    both = _hip(cuda, image, None, rH, rW, sam_mask=sam, points=fx.arr(f"points/{rH}x{rW}/all/points"))
    assert fx.same(both, fx.t(f"sam_points/{rH}x{rW}/frame32"))


@pytest.mark.parametrize("rH,rW,H,W", fx.resize_cases())
def test_nearest_resize_equals_the_recordings(hip_lib, cuda, rH, rW, H, W):
    frame, extra = _hip(cuda, fx.image_of(rH, rW), fx.t(f"depth/{rH}x{rW}"), H, W, return_extra=True)
    assert fx.same(frame, fx.t(f"resize/{rH}x{rW}_{H}x{W}/image"))
    assert fx.same(extra["depth"], fx.t(f"resize/{rH}x{rW}_{H}x{W}/depth"))


@pytest.mark.parametrize("mode,dname", fx.BUFFERS)
def test_buffer_modes_and_the_spp_mean_equal_the_recordings(hip_lib, cuda, mode, dname):
    from samnerf_amd.present import present_frame
    H, W = 33, 65
    image, depth = fx.image_of(H, W).to(cuda), fx.t(f"buffer/depth_{dname}/depth").to(cuda)
    buf = present_frame(image, depth, H, W, mode=mode)
    assert fx.same(buf, fx.t(f"buffer/{mode}_{dname}/spp0"))
    if dname != "plain":
        return
    nxt_image, nxt_depth = fx.t("buffer/next_image").to(cuda), fx.t("buffer/next_depth").to(cuda)
    for spp in (1, 5):
        out = present_frame(nxt_image, nxt_depth, H, W, mode=mode, buffer=buf, spp=spp)
        assert out.data_ptr() == buf.data_ptr()                       # updated in place
        assert fx.same(buf, fx.t(f"buffer/{mode}_{dname}/spp{spp}")), spp


def test_two_calls_give_the_same_bits(hip_lib, cuda):
    rH, rW, K, n_inst, image, kw = _case(5)
    depth = fx.t("depth/33x65")
    a = _hip(cuda, image, depth, 50, 97, mode="depth", mask_type="heatmap", instance_id=-1, return_extra=True, **kw)
    torch.empty(1 << 20, device=cuda).normal_()
    b = _hip(cuda, image, depth, 50, 97, mode="depth", mask_type="heatmap", instance_id=-1, return_extra=True, **kw)
    assert fx.same(a[0], b[0]) and all(fx.same(a[1][k], b[1][k]) for k in a[1])


# ------------------------------------------------------------- end to end --

def _mask_net(cuda):
    from helpers import make_net
    from oracle import synth
    spec = synth.ModelSpec(with_sam=False, with_mask=True, mask_type="default", n_inst=5, redundant_instance=0,
                           grid_log2=12, prop_log2=10, m_grid_log2=12)
    net = make_net(spec, synth.make_params(spec, seed=21, emb_scale=0.5), cuda).eval()
    net.opt.render_mask_type, net.opt.render_mask_instance_id, net.opt.return_extra = "composition", 2, True
    return net


def _keep_outputs(net, monkeypatch):
    seen, render = [], net.render

    def keeping(*a, **k):
        out = render(*a, **k)
        seen.append({key: v.clone() for key, v in out.items() if torch.is_tensor(v)})
        return out
    monkeypatch.setattr(net, "render", keeping)
    return seen


def test_test_step_equals_the_mirror_on_the_same_render(hip_lib, cuda, monkeypatch):
    from oracle import synth
    from samnerf_amd import ops
    from samnerf_amd.present import test_step as present_test_step
    net = _mask_net(cuda)
    seen = _keep_outputs(net, monkeypatch)
    H = W = 16
    pose, intr = synth.gui_camera(W, H, rot=synth.random_rotation(4))
    ro, rd = ops.get_rays(pose, intr, H, W, device=cuda)
    cm = fx.t("color_map").to(cuda)
    with torch.no_grad():
        rgb, depth, pred_mask = present_test_step(net, {"rays_o": ro, "rays_d": rd, "H": H, "W": W}, net.opt,
                                                  color_map=cm)
    out, = seen
    want, extra = _mirror(cuda, out["image"].view(H, W, 3), out["depth"].view(H, W), H, W,
                          logits=out["instance_mask_logits"], n_inst=5, mask_type="composition", instance_id=2,
                          color_map=cm, return_extra=True)
    assert rgb.shape == (H, W, 3) and fx.same(rgb, want) and fx.same(pred_mask, extra["probs"])
    assert fx.same(depth, out["depth"].view(H, W))
    assert len(set(extra["ids"].view(-1).tolist())) > 1, "a one-colour frame shows little"


def test_render_frame_downscaled_depth_buffer_equals_the_mirror(hip_lib, cuda, monkeypatch):
    from oracle import synth
    from samnerf_amd.present import render_frame
    net = _mask_net(cuda)
    seen = _keep_outputs(net, monkeypatch)
    H = W = 32
    pose, intr = synth.gui_camera(W, H, rot=synth.random_rotation(4))
    cm = fx.t("color_map").to(cuda)
    buf = render_frame(net, net.opt, pose, intr, W, H, downscale=0.5, mode="depth", color_map=cm)
    out, = seen
    assert out["depth"].numel() == 16 * 16 and buf.shape == (H, W, 3) and buf.is_cuda
    want = _mirror(cuda, out["image"].view(16, 16, 3), out["depth"].view(16, 16), H, W, mode="depth")
    assert fx.same(buf, want)
    # the next frame of the same view joins the mean in place
    again = render_frame(net, net.opt, pose, intr, W, H, downscale=0.5, mode="image", buffer=buf, spp=1,
                         color_map=cm)
    assert again.data_ptr() == buf.data_ptr() and len(seen) == 2
    o2 = seen[1]
    want2 = _mirror(cuda, o2["image"].view(16, 16, 3), o2["depth"].view(16, 16), H, W, mode="image", buffer=want,
                    spp=1, logits=o2["instance_mask_logits"], n_inst=5, mask_type="composition", instance_id=2,
                    color_map=cm)
    assert fx.same(buf, want2)
