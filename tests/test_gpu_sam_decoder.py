"""csrc/sam_decoder.hip on the GPU against the float64 twin
(tests/sam_decoder_ref.py) with synthetic weights: every token count at which
the padding changes (T = 7, 16, 17, 32, 33, 64), one, four and sixty-four
64-key tiles, both label kinds, zero-padded views, the [h, w, 256] entry.

The bound of an output: error = max |got - float64| / max |float64|; the
yardstick is the float32 twin's error on the same case, computed here.  The
device passes at 4 x the yardstick (it sums in another order and its erf, exp
and sin differ from ATen's by a few ulp) or, failing that, at 1e-5, the
README's floor for the training heads."""
import functools

import numpy as np
import pytest
import torch

import sam_decoder_ref as ref

pytestmark = pytest.mark.gpu
CASE_NAMES = [c[0] for c in ref.CASES]


@functools.lru_cache(maxsize=None)
def decoder(g):
    from samnerf_amd.sam_decoder import SamDecoder
    return SamDecoder.from_state_dict(ref.state_dict(), g=g, device="cuda:0")


def device_inputs(name, cuda):
    x = ref.case_inputs(name)
    feats = (x["features"] if "features" in x else x["map"]).float().to(cuda).contiguous()
    return x, feats


def run_case(name, cuda):
    x, feats = device_inputs(name, cuda)
    dec = decoder(x["g"])
    low, iou = dec.decode(feats, x["points"], x["labels"])
    logits = dec.masks(low, x["input_size"], (x["H"], x["W"]), logits=True)
    mask = dec.masks(low, x["input_size"], (x["H"], x["W"]))
    return low, iou, logits, mask


def agree_where_decided(mask, logits64, low64):
    """Rule 2: equal at every pixel whose float64 logit exceeds 1e-4 max|low_res|."""
    keep = logits64.abs() > 1e-4 * low64.abs().max()
    assert keep.double().mean().item() >= 0.99
    return bool(((mask.cpu() == (logits64 > 0)) | ~keep).all())


@pytest.mark.parametrize("name", CASE_NAMES)
def test_outputs_within_the_float32_twins_error(hip_lib, cuda, name):
    got = run_case(name, cuda)
    want = ref.twin_outputs(name)
    yard = ref.twin_outputs(name, torch.float32)
    ok = True
    for what, g, w, y in zip(("low_res", "iou", "logits"), got, want, yard):
        err, bar = ref.rel_err(g, w), ref.rel_err(y, w)
        print(f"sam_decoder_case {name:14s} {what:8s} device {err:.3e}  float32 twin {bar:.3e}  "
              f"ratio {err / bar if bar else float('inf'):.2f}")
        ok = ok and (err <= 4 * bar or err <= 1e-5)
    assert ok
    assert got[3].dtype == torch.bool and got[3].shape == want[2].shape
    assert agree_where_decided(got[3], want[2], want[0])
    assert torch.equal(got[3], got[2] > 0)


@pytest.mark.parametrize("name", ["g8_p58", "g16_p11", "g16_map24x32", "g64_p3"])
def test_two_calls_give_the_same_bits(hip_lib, cuda, name):
    a = run_case(name, cuda)
    torch.empty(1 << 20, device=cuda).normal_()
    b = run_case(name, cuda)
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.uint8) if x.dtype == torch.bool else x.view(torch.int32),
                           y.view(torch.uint8) if y.dtype == torch.bool else y.view(torch.int32))


@pytest.mark.parametrize("name", ["g8_p1", "g16_p58", "g16_map24x32"])
def test_outputs_are_written_whole_and_nothing_beside_them(hip_lib, cuda, name):
    x, feats = device_inputs(name, cuda)
    dec, g, H, W = decoder(x["g"]), x["g"], x["H"], x["W"]
    guard = 64

    def guarded(n, dtype, fill):
        buf = torch.full((guard + n + guard,), fill, dtype=dtype, device=cuda)
        return buf, buf[guard:guard + n]

    def untouched(buf, n, fill):
        edge = torch.cat([buf[:guard], buf[guard + n:]])
        return bool(edge.isnan().all()) if fill != fill else bool((edge == fill).all())
    nan = float("nan")
    n_low = 4 * 16 * g * g
    lb, low = guarded(n_low, torch.float32, nan)
    ib, iou = guarded(4, torch.float32, nan)
    dec.decode(feats, x["points"], x["labels"], out=(low.view(4, 4 * g, 4 * g), iou))
    assert untouched(lb, n_low, nan) and untouched(ib, 4, nan)
    assert not low.isnan().any() and not iou.isnan().any()
    want = run_case(name, cuda)
    assert torch.equal(low.view(4, 4 * g, 4 * g), want[0]) and torch.equal(iou, want[1])
    gb, logits = guarded(4 * H * W, torch.float32, nan)
    mb, mask = guarded(4 * H * W, torch.uint8, 77)
    dec.masks(want[0], x["input_size"], (H, W), logits=True, out=logits.view(4, H, W))
    dec.masks(want[0], x["input_size"], (H, W), out=mask.view(4, H, W))
    assert untouched(gb, 4 * H * W, nan) and untouched(mb, 4 * H * W, 77)
    assert not logits.isnan().any() and bool((mask <= 1).all())
    assert torch.equal(logits.view(4, H, W), want[2]) and torch.equal(mask.view(4, H, W).bool(), want[3])


def test_multimask_selection_and_the_predictor_interface(hip_lib, cuda):
    from samnerf_amd.sam_decoder import DevicePredictor
    name = "g8_p10"
    x, feats = device_inputs(name, cuda)
    low, iou, logits, mask = run_case(name, cuda)
    pred = DevicePredictor(decoder(8))
    pred.features = feats.view(8, 8, 256).permute(2, 0, 1)[None]
    pred.original_size, pred.input_size, pred.is_image_set = (x["H"], x["W"]), x["input_size"], True
    c = torch.as_tensor(x["points"], dtype=torch.float, device=cuda)[None]
    l = torch.as_tensor(x["labels"], dtype=torch.int, device=cuda)[None]
    m1, i1, l1 = pred.predict_torch(c, l, multimask_output=False)
    m3, i3, l3 = pred.predict_torch(c, l, multimask_output=True, return_logits=True)
    assert m1.shape == (1, 1, x["H"], x["W"]) and m1.dtype == torch.bool and i1.shape == (1, 1)
    assert l3.shape == (1, 3, 32, 32) and m3.dtype == torch.float32
    assert torch.equal(m1[0], mask[:1]) and torch.equal(l1[0], low[:1]) and torch.equal(i1[0], iou[:1])
    assert torch.equal(m3[0], logits[1:]) and torch.equal(l3[0], low[1:]) and torch.equal(i3[0], iou[1:])


# ------------------------------------------------------------- end to end --

def test_render_click_mask_and_frame_against_the_twin(hip_lib, cuda):
    """A rendered feature view through every way in -- sam_predict on a
    DevicePredictor, sam_predict_device on the map as rendered,
    render_and_predict with a PromptMemory and a presented frame -- against
    TwinPredictor (float64) on the same features."""
    from helpers import make_net
    from oracle import synth
    from samnerf_amd import ops
    from samnerf_amd.fused import FusedRenderer
    from samnerf_amd.present import present_frame
    from samnerf_amd.sam_bridge import PromptMemory, render_and_predict, sam_predict, sam_predict_device
    from samnerf_amd.sam_decoder import DevicePredictor
    from test_present_cpu import _view
    spec = synth.ModelSpec(with_sam=True, grid_log2=12, s_grid_log2=11, prop_log2=10)
    net = make_net(spec, synth.make_params(spec, seed=4, emb_scale=0.5, ln_jitter=0.1), cuda)
    W, H, w, h = 16, 12, 16, 12
    pose, intr, ro, rd = _view(W, H)
    pose_lr, intr_lr = synth.gui_camera(w, h, rot=synth.random_rotation(3))
    ro_lr, rd_lr = ops.get_rays(pose_lr, intr_lr, h, w, device=cuda)
    renderer = FusedRenderer(net)
    feats = renderer.render(ro_lr, rd_lr)["samvit"].view(h, w, 256)
    dec = decoder(64)
    click = np.array([[5, 3]])               # with these weights the twin's mask of this click has both values

    twin = ref.TwinPredictor(ref.state_dict(), g=64)
    t_masks, t_orig, t_low = sam_predict(twin, H, W, feats.double().cpu(), point_coords=click)
    logits64, low64 = twin.last_logits, twin.last_low_res
    assert t_masks.shape == (1, H, W) and 0 < t_masks.sum() < H * W, "a one-valued mask shows little"

    bar = ref.rel_err(sam_predict(ref.TwinPredictor(ref.state_dict(), g=64, dtype=torch.float32), H, W, feats.cpu(),
                                  point_coords=click)[2], t_low)
    a = sam_predict(DevicePredictor(dec), H, W, feats, point_coords=click)
    b = sam_predict_device(dec, H, W, feats, point_coords=click)
    for way, (masks, orig, low) in (("predictor", a), ("map", b)):
        assert masks.shape == (1, H, W) and masks.dtype == torch.bool and low.shape == (1, 256, 256)
        assert np.array_equal(orig, t_orig)
        assert agree_where_decided(masks, logits64, low64)
        err = ref.rel_err(low, t_low)
        print(f"sam_decoder_case {'render_' + way:14s} low_res  device {err:.3e}  float32 twin {bar:.3e}  "
              f"ratio {err / bar:.2f}")
        assert err <= 4 * bar or err <= 1e-5

    image = torch.rand(H, W, 3, generator=torch.Generator().manual_seed(1)).to(cuda)
    depth = torch.full((H, W), 0.8, device=cuda)
    view = dict(image=image, depth=depth, rays_o=ro.to(cuda), rays_d=rd.to(cuda), pose=pose, intrinsics=intr)
    pred, out, frame = render_and_predict(renderer, DevicePredictor(dec), ro_lr, rd_lr, h, w, H, W,
                                          point_coords=click[:1], memory=PromptMemory(), present=view)
    twin2 = ref.TwinPredictor(ref.state_dict(), g=64)
    t_pred, _, t_frame = render_and_predict(renderer, twin2, ro_lr, rd_lr, h, w, H, W, point_coords=click[:1],
                                            memory=PromptMemory(), present=dict(view))
    assert pred is not None and t_pred is not None and np.array_equal(pred[1], t_pred[1])
    assert np.array_equal(pred[1], click[:1])
    assert agree_where_decided(pred[0], twin2.last_logits, twin2.last_low_res)
    same = (pred[0][0] == t_pred[0][0].to(cuda))
    want = present_frame(image, depth, H, W, sam_mask=t_pred[0][0].to(cuda), points=t_pred[1])
    assert frame.shape == (H, W, 3) and torch.equal(frame[same], want[same])
    assert same.double().mean().item() >= 0.99 and not torch.equal(frame, image)
