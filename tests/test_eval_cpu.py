"""Evaluation without a GPU: the torch mirror (samnerf_amd.evaluate), eval_step
and the three meters on CPU inputs against the reference's recorded results
(tests/golden/eval.npz) bit for bit; the SSIM mirror against the float64
oracle of tests/eval_fixtures.py and two known answers; the C ABI's new entry
points and their argument checks."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

import eval_fixtures as fx
from conftest import REPO


def _ev():
    from samnerf_amd import evaluate
    return evaluate


class _StubModel:
    """model.render returns the seeded outputs (the generator's stub)."""

    def __init__(self, *outputs):
        self.outputs, self.calls = list(outputs), []

    def render(self, *a, **k):
        self.calls.append(k)
        return self.outputs[len(self.calls) - 1]


def _opt(**kw):
    base = dict(with_sam=False, with_mask=False, n_inst=1, redundant_instance=0, epsilon=fx.EPSILON,
                label_regularization_weight=0, use_point=False)
    base.update(kw)
    return types.SimpleNamespace(**base)


def _data(H, W, **kw):
    return dict(rays_o=None, rays_d=None, index=None, H=H, W=W, use_default_intrinsics=False, **kw)


# ------------------------------------------------------------ the RGB part --

@pytest.mark.parametrize("ci,H,W,C", fx.rgb_cases())
def test_rgb_mirror_eval_step_and_psnr_meter_equal_the_recordings(ci, H, W, C):
    ev = _ev()
    pred, truth = fx.t(f"rgb/{ci}/pred"), fx.t(f"rgb/{ci}/truth")
    r = ev.torch_eval_frame(pred, truth, buffers=True)
    assert fx.same(r["truth"], fx.t(f"rgb/{ci}/gt32")) and fx.same(r["mse"], fx.t(f"rgb/{ci}/loss32"))
    assert isinstance(r["psnr"], np.float32) and fx.same(r["psnr"], fx.arr(f"rgb/{ci}/psnr32"))
    assert fx.same(np.array([r[k] for k in ("pred_min", "pred_max", "truth_min", "truth_max")], np.float32),
                   fx.arr(f"rgb/{ci}/minmax"))
    for k in ("pred_u8", "truth_u8", "error_u8"):
        assert fx.same(r[k], fx.arr(f"rgb/{ci}/{k}")), k
    # the float64 evaluation is the mirror on float64 inputs
    r64 = ev.torch_eval_frame(pred.double(), truth.double(), ssim=False)
    assert fx.same(r64["mse"], fx.t(f"rgb/{ci}/loss64")) and fx.same(r64["psnr"], fx.arr(f"rgb/{ci}/psnr64"))
    # eval_step: the five values
    model = _StubModel({"image": pred.reshape(-1, 3), "depth": torch.arange(H * W).float()})
    p, d, extra, gt, loss = ev.eval_step(model, _data(H, W, images=truth), _opt())
    assert model.calls[0]["bg_color"] == 1 and model.calls[0]["perturb"] is False and not model.calls[0]["return_mask"]
    assert extra is None and fx.same(p, pred) and d.shape == (H, W)
    assert fx.same(gt, fx.t(f"rgb/{ci}/gt32")) and fx.same(loss, fx.t(f"rgb/{ci}/loss32"))
    meter = ev.PSNRMeter()
    v = meter.update(p, gt)
    assert fx.same(v, fx.arr(f"rgb/{ci}/psnr32")) and meter.measure() == v and meter.N == 1
    assert meter.report() == f"PSNR = {v:.6f}"
    meter.clear()
    assert meter.measure() == 0


@pytest.mark.parametrize("ci,H,W,C", fx.rgb_cases())
def test_ssim_mirror_in_float64_equals_the_oracle(ci, H, W, C):
    ev = _ev()
    pred, gt = fx.t(f"rgb/{ci}/pred").double(), fx.t(f"rgb/{ci}/gt32").double()
    got = float(ev.torch_eval_frame(pred, gt)["ssim"])
    want = fx.ssim64(ci)
    # two float64 evaluations in different summation orders: 121-term dot products of values
    # below 1, then a cancellation E[p^2] - E[p]^2 of terms below 1 divided by a variance of
    # about 0.08 (uniform colours): 1e-12 is four orders above that and six below the float32 error
    assert abs(got - want) <= 1e-12, (got, want)
    got32 = float(ev.torch_eval_frame(pred.float(), gt.float())["ssim"])
    assert abs(got32 - want) < 1e-5
    meter = ev.SSIMMeter()
    meter.update(pred.float(), gt.float())
    assert float(meter.measure()) == got32 and meter.report().startswith("SSIM = ")


def test_ssim_known_answers():
    ev = _ev()
    img = fx.t("rgb/2/pred")
    assert float(ev.torch_eval_frame(img, img.clone())["ssim"]) == 1.0
    want, tol32, tol64 = constant_pair_answer()
    p, q = constant_pair()
    assert abs(float(ev.torch_eval_frame(p.double(), q.double())["ssim"]) - want) <= tol64
    assert abs(float(ev.torch_eval_frame(p, q)["ssim"]) - want) <= tol32


def constant_pair(H=13, W=17):
    """Two images constant per channel: (1, 0, 1/2) and (0, 1, 1/4).  Two wholly
    constant images have a data range of 0, so c1 = c2 = 0 and the variance
    factor is 0 / 0; with the channels apart the range is 1 and every window is
    still constant."""
    p, q = torch.empty(H, W, 3), torch.empty(H, W, 3)
    for ch, (a, b) in enumerate(((1.0, 0.0), (0.0, 1.0), (0.5, 0.25))):
        p[..., ch], q[..., ch] = a, b
    return p, q


def constant_pair_answer():
    """(2ab + c1) / (a^2 + b^2 + c1), the mean over the three channels, and how
    far a float32 / float64 evaluation may be from it.  The windowed mean of a
    constant a is a S, S the sum of the 121 products of float32 weights: the
    weights' own rounding leaves |S - 1| <= 24 * 2^-24, and summing in precision u
    adds 124 u.  The variance terms are then at most a^2 (2 |S - 1| + 2 u)
    instead of 0, against c2 = 9e-4, so the variance factor is within
    3 * 2 (24 * 2^-24 + 125 u) / 9e-4 of 1 (a <= 1, three terms), and the luminance
    factor moves by less than that; u = 2^-24 or 2^-53."""
    c1 = 0.01 ** 2
    want = float(np.mean([(2 * a * b + c1) / (a * a + b * b + c1) for a, b in ((1, 0), (0, 1), (0.5, 0.25))]))
    tol = [2 * 3 * 2 * (24 * 2.0 ** -24 + 125 * u) / 9e-4 for u in (2.0 ** -24, 2.0 ** -53)]
    return want, tol[0], tol[1]


def test_the_window_is_one_table():
    want = fx.window32()
    assert fx.same(_ev().gaussian_window().numpy(), want)
    src = open(os.path.join(REPO, "segment-anything-nerf_amd", "csrc", "evaluate.hip")).read()
    bits = [int(b) for b in re.search(r"kWindowBits\[6\] = \{([^}]*)\}", src).group(1).replace("u", "").split(",")]
    assert bits == want.view(np.uint32)[:6].tolist() and fx.same(want, want[::-1].copy())
    assert abs(float(want.astype(np.float64).sum()) - 1) < 24 * 2.0 ** -24


def test_ssim_needs_one_whole_window():
    with pytest.raises(ValueError, match="at least 11"):
        _ev().torch_eval_frame(torch.zeros(10, 12, 3), torch.zeros(10, 12, 3))


# ----------------------------------------------------------- the mask part --

@pytest.mark.parametrize("ci,H,W,K,n_inst,kind", fx.mask_cases())
def test_mask_mirror_eval_step_and_miou_meter_equal_the_recordings(ci, H, W, K, n_inst, kind):
    ev = _ev()
    z, labels = fx.t(f"mask/{ci}/logits"), fx.t(f"mask/{ci}/labels")
    r = ev.torch_eval_frame(logits=z, labels=labels, n_inst=n_inst, epsilon=fx.EPSILON, n_classes=K)
    assert fx.same(r["nll"], fx.t(f"mask/{ci}/loss32")) and fx.same(r["ids"], fx.t(f"mask/{ci}/ids"))
    for k in ("inter", "npred", "ntruth"):
        assert fx.same(r[k], fx.arr(f"mask/{ci}/{k}")), k
    assert r["n_labeled"] == int(fx.arr(f"mask/{ci}/n_labeled"))
    assert isinstance(r["miou"], np.float64) and fx.same(r["miou"], fx.arr(f"mask/{ci}/miou"))
    assert fx.same(ev.miou_from_hist(r["inter"], r["npred"], r["ntruth"]), fx.arr(f"mask/{ci}/miou"))
    if fx.has(f"mask/{ci}/probs32"):
        assert fx.same(r["probs"], fx.t(f"mask/{ci}/probs32"))
    r64 = ev.torch_eval_frame(logits=z.double(), labels=labels, n_inst=n_inst, epsilon=fx.EPSILON)
    assert fx.same(r64["nll"], fx.t(f"mask/{ci}/loss64"))
    if kind == "none":
        assert float(r["nll"]) == 0.0 and r["n_labeled"] == 0
    # eval_step
    outputs = {"image": torch.zeros(H * W, 3), "depth": torch.zeros(H * W), "instance_mask_logits": z.reshape(-1, K)}
    opt = _opt(with_mask=True, n_inst=n_inst)
    model = _StubModel(outputs)
    p, d, pred_mask, gt_mask, loss = ev.eval_step(model, _data(H, W, masks=labels.clone()), opt)
    assert model.calls[0]["return_mask"] and pred_mask.shape == (H, W, K) and fx.same(gt_mask, labels)
    assert fx.same(loss, fx.t(f"mask/{ci}/loss32")) and fx.same(pred_mask.argmax(-1), fx.t(f"mask/{ci}/ids"))
    zero = ev.eval_step(_StubModel(outputs), dict(_data(H, W, masks=labels.clone()), use_default_intrinsics=True), opt)[4]
    assert float(zero) == 0.0
    meter = ev.MeanIoUMeter()
    meter.update(pred_mask.argmax(-1), gt_mask)
    assert fx.same(meter.measure(), fx.arr(f"mask/{ci}/miou")) and meter.name() == "mIoU"


def test_miou_meter_with_a_truth_class_above_every_prediction():
    ev = _ev()
    meter = ev.MeanIoUMeter()
    meter.update(fx.t("meter/pred"), fx.t("meter/truth"))
    assert fx.same(meter.measure(), fx.arr("meter/miou"))
    meter.update(fx.arr("meter/pred"), fx.arr("meter/truth"))              # numpy arrays, as the reference takes
    assert fx.same(meter.measure(), fx.arr("meter/miou")) and meter.N == 2


def test_eval_step_raises_where_the_reference_does():
    ev = _ev()
    assert str(fx.arr("redundant_raises")) == "RuntimeError"
    z, labels = fx.t("mask/2/logits"), fx.t("mask/2/labels").clamp(max=2)
    outputs = {"image": torch.zeros(121, 3), "depth": torch.zeros(121), "instance_mask_logits": z.reshape(-1, 5)}
    with pytest.raises(RuntimeError, match="redundant_instance"):
        ev.eval_step(_StubModel(outputs), _data(11, 11, masks=labels), _opt(with_mask=True, n_inst=3, redundant_instance=2))
    with pytest.raises(NotImplementedError, match="use_point"):
        ev.eval_step(_StubModel({"image": torch.zeros(121, 3), "depth": torch.zeros(121)}), _data(11, 11),
                     _opt(with_sam=True, use_point=True))


def test_eval_step_label_regularization_is_mask_loss_own_term():
    ev = _ev()
    from samnerf_amd.mask_loss import torch_label_regularization
    H, W, K = 12, 19, 5                           # 228 pixels: 57 patches of 2 x 2
    z, labels = fx.t("mask/4/logits"), fx.t("mask/6/labels")[:H, :W].contiguous()
    depth = 0.5 + torch.rand(H * W, generator=torch.Generator().manual_seed(3))
    outputs = {"image": torch.zeros(H * W, 3), "depth": depth, "instance_mask_logits": z.reshape(-1, K)}
    base = ev.eval_step(_StubModel(outputs), _data(H, W, masks=labels), _opt(with_mask=True, n_inst=K))
    got = ev.eval_step(_StubModel(outputs), _data(H, W, masks=labels),
                       _opt(with_mask=True, n_inst=K, label_regularization_weight=0.25, patch_size=2))
    want = base[4] + torch_label_regularization(2, depth, base[2].reshape(-1, K)) * 0.25
    assert fx.same(got[4], want) and float(got[4]) != float(base[4])


# ------------------------------------------------------------ the SAM part --

def test_sam_branch_equals_the_recording():
    ev = _ev()
    image, feat, gt = fx.t("sam/image"), fx.t("sam/pred"), fx.t("sam/gt")
    H, W, h, w = 11, 11, 5, 7
    r = ev.torch_eval_frame(pred_feat=feat, gt_feat=gt)
    assert fx.same(r["feat_mse"], fx.t("sam/loss32"))
    assert fx.same(ev.torch_eval_frame(pred_feat=feat.double(), gt_feat=gt.double())["feat_mse"], fx.t("sam/loss64"))
    seen = []

    def features(img):
        seen.append(img)
        return gt
    model = _StubModel({"image": image.reshape(-1, 3), "depth": torch.zeros(H * W)}, {"samvit": feat})
    p, d, pred_samvit, truth, loss = ev.eval_step(model, _data(H, W, h=h, w=w, rays_o_lr=None, rays_d_lr=None),
                                                  _opt(with_sam=True), sam_features=features)
    assert truth is p and fx.same(loss, fx.t("sam/loss32"))
    assert seen[0].dtype == np.uint8 and seen[0].shape == (H, W, 3)
    assert model.calls[1]["return_feats"] == 1 and model.calls[1]["H"] == h and model.calls[1]["W"] == w
    assert fx.same(pred_samvit, feat.reshape(1, h, w, 256).permute(0, 3, 1, 2))


# ------------------------------------------------------------------ the ABI --

def test_the_abi_declares_the_entry_points_with_the_headers_signatures(hip_lib):
    from samnerf_amd import _lib
    text = open(os.path.join(REPO, "include", "samnerf_hip.h")).read()
    for name, n_args in (("samnerf_eval_workspace_size", 2), ("samnerf_eval_frame", 2), ("samnerf_eval_confusion", 6)):
        m = re.search(r"^int " + name + r"\(([^;]*)\);", text, re.M)
        assert m, name
        assert len(m.group(1).split(",")) == n_args == len(_lib._SIGS[name][0]), name
        assert _lib._SIGS[name][1] is ctypes.c_int and hasattr(hip_lib, name)
    # the struct: every field of the header, in order
    body = re.search(r"typedef struct \{([^}]*)\} samnerf_eval_args;", text).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [f.strip().split()[-1].lstrip("*") for d in body.split(";") if d.strip()
              for f in d.split(",")]
    assert fields == [f[0] for f in _lib.SamnerfEvalArgs._fields_]
    stats = re.search(r"typedef struct \{([^}]*)\} samnerf_eval_stats;", text).group(1)
    assert "reserved[5]" in stats and _ev().stats_bytes(0) == 128 and _ev().stats_bytes(5) == 192


def test_argument_errors_come_back_as_codes(hip_lib):
    from samnerf_amd._lib import SamnerfEvalArgs
    L, p = hip_lib, 64                             # never dereferenced: validation fails first
    need = ctypes.c_size_t(7)

    def rc(**kw):
        a = SamnerfEvalArgs()
        a.stats = p
        for k, v in kw.items():
            setattr(a, k, v)
        return L.samnerf_eval_workspace_size(ctypes.byref(a), ctypes.byref(need)), L.samnerf_eval_frame(ctypes.byref(a), None)
    assert rc() == (-1, -1) and b"no part" in L.samnerf_last_error() and need.value == 0
    assert rc(H=10, W=11, C=3, ssim=1, pred_rgb=p, truth=p) == (-1, -1) and b">= 11" in L.samnerf_last_error()
    assert rc(H=11, W=11, C=5, pred_rgb=p, truth=p) == (-1, -1)
    assert rc(H=11, W=11, K=65, n_inst=2, n_classes=65, logits=p, labels=p) == (-1, -1)
    assert rc(H=11, W=11, K=5, n_inst=6, n_classes=5, logits=p, labels=p) == (-1, -1)
    assert rc(H=11, W=11, K=5, n_inst=5, n_classes=1025, logits=p, labels=p) == (-1, -1)
    assert rc(H=11, W=11, K=5, n_inst=5, n_classes=5, logits=p) == (-1, -1)
    assert rc(h=4, w=0, pred_feat=p, gt_feat=p) == (-1, -1)
    assert rc(H=11, W=11, C=3, pred_rgb=p, truth=p, stats=p + 4) == (-1, -1) and b"aligned" in L.samnerf_last_error()
    # valid arguments: the size is known without a GPU, and a missing workspace is its own code
    assert rc(H=11, W=11, C=3, ssim=1, pred_rgb=p, truth=p) == (0, -3) and need.value > 0
    assert L.samnerf_eval_confusion(p, p, 4, 0, p, None) == -1
    assert L.samnerf_eval_confusion(None, p, 4, 5, p, None) == -1 and b"null id map" in L.samnerf_last_error()


def test_read_stats_finishes_a_record_in_float64():
    ev = _ev()
    rec = np.zeros(ev.stats_bytes(3), np.uint8)
    h = rec[:128].view(ev._HEADER)[0]
    h["sq_sum"], h["n_elem"], h["nll_sum"], h["n_labeled"] = 0.5, 50, 3.0, 4
    rec[128:128 + 36].view("<u4")[:] = [2, 0, 1, 4, 0, 2, 3, 0, 3]       # inter, npred, ntruth
    d = ev.read_stats(rec, 3)
    assert d["mse"] == 0.01 and d["psnr"] == 20.0 and d["nll"] == 0.75 and d["ssim"] is None
    assert d["miou"] == np.mean([2 / 5, 1 / 4])                          # class 1 has no union
    h["overflow"] = 2
    with pytest.raises(RuntimeError, match="outside the classes"):
        ev.read_stats(rec, 3)
