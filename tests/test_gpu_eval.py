"""samnerf_eval_frame / samnerf_eval_confusion (csrc/evaluate.hip) through
samnerf_amd.evaluate.

Bit for bit against the reference's recordings (tests/golden/eval.npz)
wherever no floating sum is involved: the composited truth, min / max, the three
uint8 images, the argmax ids, the three histograms, the labeled count and the
mIoU (float64, from Evaluator.results()).

Floating sums -- squared error (loss, PSNR), NLL, SSIM, feature MSE -- by the
convention of tests/test_gpu_present.py and tests/test_gpu_mask_loss.py.  d_ref
is the distance between the reference's float32 recording and the float64
evaluation of the same inputs (for SSIM: between the float32 F.conv2d mirror on
the CPU and the float64 oracle of tests/eval_fixtures.py).  The kernels are
another float32 evaluation whose sums run in double, so their distance from the
float64 evaluation is bounded by M * d_ref + one float32 ulp of the quantity.

Shapes: 11 x 11 (one SSIM window, one workgroup), 12 x 19 (a ragged tile and a
ragged last wave), 45 x 70 (the SSIM tile is 32 x 16 outputs: 2 x 3 tiles a
channel; 13 workgroups of 256 pixels); K = 1 (n_inst = 1), 2, 5 and 33 (K > 32
takes 128-pixel chunks and a second tree sum); RGB and RGBA truth.
"""
import types

import numpy as np
import pytest
import torch

import eval_fixtures as fx

pytestmark = pytest.mark.gpu

# Twice the worst ratio (error - ulp) / d_ref measured on the MI355X over the
# cases of this file (each prints its own as "RATIO ..."):
#   SSIM           0.48  (12 x 19, RGBA truth; 0.29 through eval_step at 16 x 16,
#                         0.19 or less elsewhere)
#   probabilities  0.43  (12 x 19, K = 5; 0.26 or less elsewhere)
#   squared error, PSNR, NLL, feature MSE   0.00: within one ulp of the float64
#                         evaluation in every case (the sums run in double)
# No ratio is above 1: the kernels are nearer the float64 evaluation than the
# reference's own float32 result is.
M_REF = 0.96


def _ev():
    from samnerf_amd import evaluate
    return evaluate


def _bound(name, got, r32, r64, bad):
    got, r32, r64 = float(got), float(r32), float(r64)
    d_ref, ulp, err = abs(r32 - r64), float(np.spacing(np.float32(abs(r64)))), abs(got - r64)
    ratio = max(err - ulp, 0.0) / d_ref if d_ref > 0 else (0.0 if err <= ulp else float("inf"))
    print(f"RATIO {name}: got={got!r} err={err:.3e} d_ref={d_ref:.3e} ulp={ulp:.3e} ratio={ratio:.3f}")
    if not err <= M_REF * d_ref + ulp:
        bad.append((name, err, d_ref, ulp))


@pytest.mark.parametrize("ci,H,W,C", fx.rgb_cases())
def test_rgb_part_against_the_recordings(hip_lib, cuda, ci, H, W, C):
    ev = _ev()
    pred, truth = fx.t(f"rgb/{ci}/pred"), fx.t(f"rgb/{ci}/truth")
    table = ev.Evaluator(2, device=cuda)
    r = table.update(1, pred.to(cuda).reshape(-1, 3), truth.to(cuda), buffers=True)
    res = table.results()
    d = res["views"][1]
    assert fx.same(r["truth"], fx.t(f"rgb/{ci}/gt32"))
    for k in ("pred_u8", "truth_u8", "error_u8"):
        assert fx.same(r[k], fx.arr(f"rgb/{ci}/{k}")), k
    assert fx.same(np.array([d[k] for k in ("pred_min", "pred_max", "truth_min", "truth_max")], np.float32),
                   fx.arr(f"rgb/{ci}/minmax"))
    assert d["n_elem"] == H * W * 3 and d["n_ssim"] == (H - 10) * (W - 10) * 3 and d["n_labeled"] == 0
    assert res["views"][0]["mse"] is None                  # the other slot was not touched
    bad = []
    _bound(f"rgb {ci} {H}x{W}x{C} mse", d["mse"], fx.arr(f"rgb/{ci}/loss32"), fx.arr(f"rgb/{ci}/loss64"), bad)
    _bound(f"rgb {ci} {H}x{W}x{C} psnr", d["psnr"], fx.arr(f"rgb/{ci}/psnr32"), fx.arr(f"rgb/{ci}/psnr64"), bad)
    ssim32 = ev.torch_eval_frame(pred, truth)["ssim"]
    _bound(f"rgb {ci} {H}x{W}x{C} ssim", d["ssim"], ssim32, fx.ssim64(ci), bad)
    assert not bad, bad
    assert res["psnr"] == d["psnr"] and res["ssim"] == d["ssim"] and res["loss"] == d["mse"]


@pytest.mark.parametrize("ci,H,W,K,n_inst,kind", fx.mask_cases())
def test_mask_part_against_the_recordings(hip_lib, cuda, ci, H, W, K, n_inst, kind):
    ev = _ev()
    z, labels = fx.t(f"mask/{ci}/logits"), fx.t(f"mask/{ci}/labels")
    table = ev.Evaluator(1, n_classes=K, device=cuda)
    r = table.update(0, logits=z.to(cuda), labels=labels.to(cuda), n_inst=n_inst, epsilon=fx.EPSILON)
    res = table.results()
    d = res["views"][0]
    assert fx.same(r["ids"], fx.t(f"mask/{ci}/ids")) and r["probs"].shape == (H, W, K)
    for k in ("inter", "npred", "ntruth"):
        assert fx.same(d[k], fx.arr(f"mask/{ci}/{k}")), k
    assert d["n_labeled"] == int(fx.arr(f"mask/{ci}/n_labeled")) and d["overflow"] == 0
    assert isinstance(d["miou"], np.float64) and fx.same(d["miou"], fx.arr(f"mask/{ci}/miou"))
    assert res["miou"] == float(d["miou"])
    if kind == "none":
        assert d["nll"] == 0.0 and d["nll_sum"] == 0.0
    bad = []
    _bound(f"mask {ci} {H}x{W} K={K} nll", d["nll"], fx.arr(f"mask/{ci}/loss32"), fx.arr(f"mask/{ci}/loss64"), bad)
    if fx.has(f"mask/{ci}/probs64"):
        p32, p64 = fx.t(f"mask/{ci}/probs32").double(), fx.t(f"mask/{ci}/probs64")
        got = r["probs"].cpu().double()
        d_ref, err = float((p32 - p64).abs().max()), float((got - p64).abs().max())
        ulp = float(np.spacing(np.float32(p64.max().item())))
        print(f"RATIO mask {ci} probs: err={err:.3e} d_ref={d_ref:.3e} ulp={ulp:.3e} "
              f"ratio={max(err - ulp, 0.0) / d_ref if d_ref else 0.0:.3f}")
        if not err <= M_REF * d_ref + ulp:
            bad.append(("probs", err, d_ref, ulp))
    assert not bad, bad


def _whole_view(ev, cuda, table, slot):
    """Every part in one call at 45 x 70: RGBA truth with SSIM and buffers, K = 5, the 5 x 7 features."""
    return table.update(slot, fx.t("rgb/5/pred").to(cuda), fx.t("rgb/5/truth").to(cuda), buffers=True,
                        logits=fx.t("mask/6/logits").to(cuda), labels=fx.t("mask/6/labels").to(cuda), n_inst=5,
                        epsilon=fx.EPSILON, pred_feat=fx.t("sam/pred").to(cuda), gt_feat=fx.t("sam/gt").to(cuda))


def test_two_calls_give_the_same_record_and_the_parts_do_not_disturb_each_other(hip_lib, cuda):
    ev = _ev()
    table = ev.Evaluator(3, n_classes=5, device=cuda)
    a = _whole_view(ev, cuda, table, 0)
    torch.empty(1 << 20, device=cuda).normal_()
    b = _whole_view(ev, cuda, table, 2)
    raw = table.table.cpu()
    assert torch.equal(raw[0], raw[2]) and not raw[1].any()
    for k in ("truth", "probs", "ids", "pred_u8", "truth_u8", "error_u8"):
        assert fx.same(a[k], b[k]), k
    # the same sums as each part gives alone
    alone = ev.Evaluator(3, n_classes=5, device=cuda)
    alone.update(0, fx.t("rgb/5/pred").to(cuda), fx.t("rgb/5/truth").to(cuda))
    alone.update(1, logits=fx.t("mask/6/logits").to(cuda), labels=fx.t("mask/6/labels").to(cuda), n_inst=5,
                 epsilon=fx.EPSILON)
    alone.update(2, pred_feat=fx.t("sam/pred").to(cuda), gt_feat=fx.t("sam/gt").to(cuda))
    whole, parts = table.results()["views"][0], alone.results()["views"]
    assert (whole["sq_sum"], whole["ssim_sum"]) == (parts[0]["sq_sum"], parts[0]["ssim_sum"])
    assert whole["nll_sum"] == parts[1]["nll_sum"] and fx.same(whole["inter"], parts[1]["inter"])
    assert whole["feat_sq_sum"] == parts[2]["feat_sq_sum"] and whole["n_feat"] == 35 * 256


def test_feature_mse_against_the_recording(hip_lib, cuda):
    ev = _ev()
    r = ev.eval_frame(pred_feat=fx.t("sam/pred").to(cuda), gt_feat=fx.t("sam/gt").to(cuda))
    d = ev.read_stats(r["stats"])
    bad = []
    _bound("sam 5x7 feat_mse", d["feat_mse"], fx.arr("sam/loss32"), fx.arr("sam/loss64"), bad)
    assert not bad, bad


def test_meters_on_cuda_tensors_give_the_evaluators_numbers(hip_lib, cuda):
    ev = _ev()
    table = ev.Evaluator(4, n_classes=ev.DEFAULT_CLASSES, device=cuda)
    psnr, ssim, miou = ev.PSNRMeter(), ev.SSIMMeter(), ev.MeanIoUMeter()
    for slot, (ci, mi) in enumerate(((1, 2), (5, 6))):
        pred, gt = fx.t(f"rgb/{ci}/pred").to(cuda), fx.t(f"rgb/{ci}/gt32").to(cuda)
        table.update(slot, pred, gt)
        pending = psnr.update(pred, gt)
        ssim.update(pred, gt)
        z, labels = fx.t(f"mask/{mi}/logits").to(cuda), fx.t(f"mask/{mi}/labels").to(cuda)
        r = table.update(2 + slot, logits=z, labels=labels, n_inst=5, epsilon=fx.EPSILON)
        miou.update(r["probs"].argmax(-1), labels)             # utils.py:1953-1954
    res = table.results()
    assert psnr.N == 0 and psnr._records                       # nothing read yet
    assert psnr.measure() == np.mean([v["psnr"] for v in res["views"][:2]]) and psnr.N == 2
    assert ssim.measure() == np.mean([v["ssim"] for v in res["views"][:2]])
    assert miou.measure() == np.mean([v["miou"] for v in res["views"][2:]])
    assert miou.measure() == np.mean([fx.arr("mask/2/miou"), fx.arr("mask/6/miou")])
    assert psnr.report() == f"PSNR = {psnr.measure():.6f}"
    # update()'s value formats as the reference's does (the error image's file name, utils.py:1979)
    assert f"{pending:.2f}" == f"{res['views'][1]['psnr']:.2f}" and float(pending) == res["views"][1]["psnr"]
    # a truth class above every predicted id and above K
    alone = ev.MeanIoUMeter()
    alone.update(fx.t("meter/pred").to(cuda), fx.t("meter/truth").to(cuda))
    assert fx.same(np.float64(alone.measure()), fx.arr("meter/miou"))
    # ids past the bins are counted, never used as an index, and measure() raises
    small = ev.MeanIoUMeter(n_classes=6)
    small.update(fx.t("meter/pred").to(cuda), fx.t("meter/truth").to(cuda))
    with pytest.raises(RuntimeError, match="outside the classes"):
        small.measure()


# ------------------------------------------------------------- end to end --

def _net(cuda):
    from helpers import make_net
    from oracle import synth
    spec = synth.ModelSpec(with_sam=False, with_mask=True, mask_type="default", n_inst=5, redundant_instance=0,
                           grid_log2=12, prop_log2=10, m_grid_log2=12)
    return make_net(spec, synth.make_params(spec, seed=21, emb_scale=0.5), cuda).eval()


def _keep_outputs(net, monkeypatch):
    seen, render = [], net.render

    def keeping(*a, **k):
        out = render(*a, **k)
        seen.append({key: v.clone() for key, v in out.items() if torch.is_tensor(v)})
        return out
    monkeypatch.setattr(net, "render", keeping)
    return seen


@pytest.mark.parametrize("branch", ["rgb", "mask"])
def test_eval_step_equals_the_mirror_on_the_same_render(hip_lib, cuda, monkeypatch, branch):
    from oracle import synth
    from samnerf_amd import ops
    ev = _ev()
    net = _net(cuda)
    seen = _keep_outputs(net, monkeypatch)
    H = W = 16
    pose, intr = synth.gui_camera(W, H, rot=synth.random_rotation(4))
    ro, rd = ops.get_rays(pose, intr, H, W, device=cuda)
    g = torch.Generator().manual_seed(8)
    images = torch.randint(0, 256, (H, W, 4), generator=g).float() / 255
    masks = torch.randint(-1, 5, (H, W), generator=g)
    opt = types.SimpleNamespace(with_mask=branch == "mask", with_sam=False, n_inst=5, redundant_instance=0,
                                epsilon=fx.EPSILON, label_regularization_weight=0)
    data = {"rays_o": ro, "rays_d": rd, "H": H, "W": W, "images": images.to(cuda), "masks": masks.to(cuda),
            "use_default_intrinsics": False}
    table = ev.Evaluator(1, n_classes=5 if branch == "mask" else 0, device=cuda)
    with torch.no_grad():
        p, d, extra, truth, loss = ev.eval_step(net, data, opt, stats=table.table[0])
    out, = seen
    assert fx.same(p, out["image"].view(H, W, 3)) and fx.same(d, out["depth"].view(H, W)) and loss.is_cuda
    rec = table.results()["views"][0]
    bad = []
    if branch == "rgb":
        img = out["image"].cpu().view(H, W, 3)
        m32, m64 = ev.torch_eval_frame(img, images), ev.torch_eval_frame(img.double(), images.double())
        assert extra is None and fx.same(truth, m32["truth"])
        _bound("eval_step rgb loss", loss, m32["mse"], m64["mse"], bad)
        _bound("eval_step rgb psnr", rec["psnr"], m32["psnr"], m64["psnr"], bad)
        _bound("eval_step rgb ssim", rec["ssim"], m32["ssim"], fx.ssim64_of(img.numpy(), m32["truth"].numpy()), bad)
        assert float(loss) == float(np.float32(rec["mse"]))
    else:
        z = out["instance_mask_logits"].cpu()
        kw = dict(labels=masks, n_inst=5, epsilon=fx.EPSILON, n_classes=5)
        m32, m64 = ev.torch_eval_frame(logits=z, **kw), ev.torch_eval_frame(logits=z.double(), **kw)
        assert fx.same(truth, masks) and extra.shape == (H, W, 5)
        # an argmax can differ from the CPU's only where the float64 probabilities nearly tie
        top = torch.topk(m64["probs"].view(-1, 5), 2, dim=-1).values
        clear = ((top[:, 0] - top[:, 1]) > 1e-5).view(H, W)
        ids = extra.argmax(-1).cpu()
        assert fx.same(ids[clear], m32["ids"][clear]) and bool(clear.float().mean() > 0.9)
        if bool(clear.all()):
            for k in ("inter", "npred", "ntruth"):
                assert fx.same(rec[k], m32[k]), k
            assert fx.same(rec["miou"], m32["miou"])
        assert rec["n_labeled"] == m32["n_labeled"]
        _bound("eval_step mask nll", loss, m32["nll"], m64["nll"], bad)
        zero = ev.eval_step(net, dict(data, use_default_intrinsics=True), opt)[4]
        assert float(zero) == 0.0
    assert not bad, bad


def test_second_tree_degenerates_to_the_first(hip_lib, cuda):
    """K = 64 with columns 32 .. 63 at -inf against K = 32 on the first 32
    columns: expf(-inf) == 0 and sum + 0 == sum, so the two-tree row gives the
    one-tree row's bits.  11 x 29 = 319 rows: two full 128-row chunks and a
    ragged 63 at K = 64, one full 256-row chunk and 63 at K = 32.  (Nothing
    about nll_sum: its partials are partitioned differently at 128 and 256.)"""
    ev = _ev()
    H, W = 11, 29
    z32 = 2 * torch.randn(H, W, 32, generator=torch.Generator().manual_seed(64))
    z64 = torch.cat([z32, torch.full((H, W, 32), float("-inf"))], -1)
    labels = (torch.arange(H * W, dtype=torch.int64) % 32).view(H, W).to(cuda)
    a = ev.eval_frame(logits=z32.to(cuda), labels=labels, n_inst=32)
    b = ev.eval_frame(logits=z64.to(cuda), labels=labels, n_inst=64)
    assert b["probs"].shape == (H, W, 64)
    assert fx.same(b["probs"][..., :32].contiguous(), a["probs"]) and fx.same(b["ids"], a["ids"])
    assert not b["probs"][..., 32:].any()
    assert len(set(a["ids"].view(-1).tolist())) > 1
