#!/usr/bin/env python3
"""Generate tests/golden/eval.npz from the REFERENCE's own evaluation: what
Trainer.eval_step and the meters of evaluate_one_epoch compute from a
render's outputs.

Runs only where the reference tree exists (tools/make_golden.py's
install_reference), never in a test.  Recorded, on seeded inputs:

  * per RGB case (size, RGB or RGBA truth): Trainer.eval_step called unbound on
    a stub whose model.render returns the seeded image -- its gt_rgb and loss --
    the reference's PSNRMeter on them, min and max, and the three uint8 images
    of evaluate_one_epoch (utils.py:1984-1999, three numpy lines that cannot be
    called apart from the epoch loop and are restated here);
  * per mask case (size, K, n_inst, labels): eval_step's pred_mask and loss,
    the argmax of utils.py:1953, the reference's MeanIoUMeter on ids and
    labels, and the three per-class counts the mean is made of;
  * MeanIoUMeter alone on id maps with a truth class above every predicted id;
  * the --with_sam branch on a stub predictor (feature loss);
  * that redundant_instance > 0 makes eval_step raise.

Every float32 result has a float64 evaluation of the same inputs beside it (the
same reference code on float64 tensors).  SSIM has no recording: torchmetrics
is not installed; its oracle is tests/eval_fixtures.py.

The logits are make_present_golden's: multiples of 1/8, the top two float64
probabilities of every pixel at least 1e-3 apart or exactly tied with tied
logits, at least 5 % ties, or the file is not written.  Images are multiples of
1/255.  Only data goes into the file.

usage: PYTHONDONTWRITEBYTECODE=1 python tools/make_eval_golden.py
"""
import json
import os
import sys
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_present_golden as mpg  # noqa: E402  (make_logits, check_logits, rand_image)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import make_golden  # noqa: E402

# one SSIM window and one workgroup; a ragged tile and a ragged last wave; several
# 32 x 16 SSIM tiles both ways (2 x 3) and 13 workgroups of 256 pixels
SIZES = [(11, 11), (12, 19), (45, 70)]
RGB_CASES = [(H, W, C) for H, W in SIZES for C in (3, 4)]
# (H, W, K, n_inst, labels): 'some' = about 10 % unlabeled, 'none' = every label
# -1, 'absent' = one class in neither map.  K = 33 takes the 128-pixel chunks.
MASK_CASES = [(11, 11, 1, 1, "some"), (11, 11, 2, 2, "some"), (11, 11, 5, 5, "some"), (11, 11, 33, 33, "some"),
              (12, 19, 5, 5, "none"), (12, 19, 33, 33, "absent"), (45, 70, 5, 5, "some"), (45, 70, 2, 2, "some")]
PROBS_LIMIT = 4000           # values of pred_mask recorded only for the small cases
EPSILON = 0.000001           # main.py's default
ABSENT = 7


def stub(opt, outputs, features=None, second=None):
    calls = []

    def render(*a, **k):
        calls.append(k)
        return outputs if len(calls) == 1 else second
    st = types.SimpleNamespace(model=types.SimpleNamespace(render=render), opt=opt, device="cpu",
                               criterion=torch.nn.MSELoss(reduction="none"))
    if features is not None:
        st.sam_predictor = types.SimpleNamespace(set_image=lambda image: None, features=features)
    return st


def make_opt(**kw):
    base = dict(with_sam=False, with_mask=False, n_inst=1, redundant_instance=0, epsilon=EPSILON,
                label_regularization_weight=0, use_point=False, fp16=False)
    base.update(kw)
    return types.SimpleNamespace(**base)


def data_of(H, W, **kw):
    d = dict(rays_o=None, rays_d=None, index=None, H=H, W=W, use_default_intrinsics=False)
    d.update(kw)
    return d


def main():
    _, _, utils = make_golden.install_reference()
    eval_step = utils.Trainer.eval_step
    out = {}
    g = torch.Generator().manual_seed(31)

    # ---- the RGB branch, PSNRMeter, the saved images
    for ci, (H, W, C) in enumerate(RGB_CASES):
        pred = mpg.rand_image(g, H, W)
        truth = torch.randint(0, 256, (H, W, C), generator=g).float() / 255
        name = f"rgb/{ci}"
        out[f"{name}/pred"], out[f"{name}/truth"] = pred.numpy(), truth.numpy()
        res = {}
        for tag, dt in (("32", torch.float32), ("64", torch.float64)):
            outputs = {"image": pred.to(dt).reshape(-1, 3), "depth": torch.zeros(H * W, dtype=dt)}
            p, d, extra, gt, loss = eval_step(stub(make_opt(), outputs), data_of(H, W, images=truth.to(dt)))
            assert extra is None and p.dtype == dt and gt.dtype == dt
            meter = utils.PSNRMeter()
            psnr = meter.update(p, gt)
            assert meter.N == 1 and meter.measure() == psnr
            res[tag] = (p, gt, loss, psnr)
            out[f"{name}/loss{tag}"], out[f"{name}/psnr{tag}"] = loss.numpy(), np.asarray(psnr)
        p, gt = res["32"][0], res["32"][1]
        assert res["32"][3].dtype == np.float32 and res["64"][3].dtype == np.float64
        out[f"{name}/gt32"] = gt.numpy()
        out[f"{name}/minmax"] = np.array([p.min(), p.max(), gt.min(), gt.max()], np.float32)
        # utils.py:1984-1999
        pred8 = p.detach().cpu().numpy()
        pred8 = (pred8 * 255).astype(np.uint8)
        truth8 = gt.detach().cpu().numpy()
        truth8 = (truth8 * 255).astype(np.uint8)
        error = np.abs(truth8.astype(np.float32) - pred8.astype(np.float32)).mean(-1).astype(np.uint8)
        out[f"{name}/pred_u8"], out[f"{name}/truth_u8"], out[f"{name}/error_u8"] = pred8, truth8, error
        print(name, (H, W, C), float(res["32"][2]), float(res["32"][3]))
    out["rgb/cases"] = np.array(json.dumps(RGB_CASES))

    # ---- the --with_mask branch, the argmax, MeanIoUMeter
    for ci, (H, W, K, n_inst, kind) in enumerate(MASK_CASES):
        z = mpg.make_logits(g, H, W, K)
        labels = torch.randint(0, K, (H, W), generator=g)
        if kind == "absent":
            z[..., ABSENT] = -20.0
            labels[labels == ABSENT] = ABSENT + 1
        ties, pairs = mpg.check_logits(z, n_inst)
        if K > 1:
            assert ties >= 0.05 and len(pairs) >= min(3, K * (K - 1) // 2), (ties, pairs)
        if kind == "none":
            labels[:] = -1
        else:
            labels[torch.rand(H, W, generator=g) < 0.1] = -1
        name = f"mask/{ci}"
        out[f"{name}/logits"], out[f"{name}/labels"] = z.numpy(), labels.numpy()
        opt = make_opt(with_mask=True, n_inst=n_inst)
        res = {}
        for tag, dt in (("32", torch.float32), ("64", torch.float64)):
            outputs = {"image": torch.zeros(H * W, 3, dtype=dt), "depth": torch.zeros(H * W, dtype=dt),
                       "instance_mask_logits": z.to(dt).reshape(-1, K)}
            _, _, pred_mask, gt_mask, loss = eval_step(stub(opt, outputs), data_of(H, W, masks=labels.clone()))
            assert pred_mask.shape == (H, W, K) and pred_mask.dtype == dt and torch.equal(gt_mask, labels)
            res[tag] = (pred_mask, loss)
            out[f"{name}/loss{tag}"] = loss.numpy()
            if H * W * K <= PROBS_LIMIT:
                out[f"{name}/probs{tag}"] = pred_mask.numpy()
        ids = res["32"][0].argmax(-1)                          # utils.py:1953
        assert torch.equal(ids, res["64"][0].argmax(-1))
        meter = utils.MeanIoUMeter()
        meter.update(ids, labels)
        miou = meter.measure()
        assert meter.N == 1 and isinstance(miou, np.float64)
        pi, ti = ids.numpy().reshape(-1), labels.numpy().reshape(-1)
        out[f"{name}/ids"], out[f"{name}/miou"] = ids.numpy(), np.asarray(miou)
        out[f"{name}/npred"] = np.bincount(pi, minlength=K).astype(np.int64)
        out[f"{name}/ntruth"] = np.bincount(ti[ti >= 0], minlength=K).astype(np.int64)
        out[f"{name}/inter"] = np.bincount(pi[pi == ti], minlength=K).astype(np.int64)
        out[f"{name}/n_labeled"] = np.asarray(int((ti != -1).sum()))
        if kind == "absent":
            assert out[f"{name}/npred"][ABSENT] == 0 and out[f"{name}/ntruth"][ABSENT] == 0
        # use_default_intrinsics: utils.py:1187-1188
        outputs = {"image": torch.zeros(H * W, 3), "depth": torch.zeros(H * W), "instance_mask_logits": z.reshape(-1, K)}
        zero = eval_step(stub(opt, outputs), data_of(H, W, masks=labels.clone(), use_default_intrinsics=True))[4]
        assert float(zero) == 0.0
        print(name, (H, W, K, n_inst, kind), f"ties {ties:.3f}", float(res["32"][1]), float(miou))
    out["mask/cases"] = np.array(json.dumps(MASK_CASES))

    # ---- redundant_instance > 0: view(-1, n_inst) loses the pixel rows
    H, W, K = 11, 11, 5
    outputs = {"image": torch.zeros(H * W, 3), "depth": torch.zeros(H * W),
               "instance_mask_logits": torch.from_numpy(out["mask/2/logits"]).reshape(-1, K)}
    try:
        eval_step(stub(make_opt(with_mask=True, n_inst=3, redundant_instance=2), outputs),
                  data_of(H, W, masks=torch.from_numpy(out["mask/2/labels"]).clamp(max=2)))
        raised = ""
    except Exception as e:  # noqa: BLE001
        raised = type(e).__name__
    out["redundant_raises"] = np.array(raised)
    print("redundant_instance > 0 raises:", raised or "nothing")

    # ---- MeanIoUMeter alone: a truth class above every predicted id
    pred_ids = torch.from_numpy(out["mask/6/ids"])
    truth_ids = torch.randint(-1, 8, pred_ids.shape, generator=g)
    assert int(truth_ids.max()) == 7 and int(pred_ids.max()) == 4
    meter = utils.MeanIoUMeter()
    meter.update(pred_ids, truth_ids)
    out["meter/pred"], out["meter/truth"], out["meter/miou"] = pred_ids.numpy(), truth_ids.numpy(), np.asarray(meter.measure())

    # ---- the --with_sam branch without use_point
    H, W, h, w = 11, 11, 5, 7
    image = mpg.rand_image(g, H, W)
    feat = torch.round(torch.randn(h * w, 256, generator=g) * 16) / 16
    gt = torch.round(torch.randn(1, 256, h, w, generator=g) * 16) / 16
    out["sam/image"], out["sam/pred"], out["sam/gt"] = image.numpy(), feat.numpy(), gt.numpy()
    for tag, dt in (("32", torch.float32), ("64", torch.float64)):
        first = {"image": image.to(dt).reshape(-1, 3), "depth": torch.zeros(H * W, dtype=dt)}
        st = stub(make_opt(with_sam=True), first, features=gt.to(dt), second={"samvit": feat.to(dt)})
        p, d, pred_samvit, truth, loss = eval_step(st, data_of(H, W, h=h, w=w, rays_o_lr=None, rays_d_lr=None))
        assert truth is p and torch.equal(pred_samvit, feat.to(dt).reshape(1, h, w, 256).permute(0, 3, 1, 2))
        out[f"sam/loss{tag}"] = loss.numpy()

    path = os.path.join(make_golden.GOLDEN, "eval.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print("wrote", path, size, "bytes")
    assert size < (1 << 20), "over the size limit for a committed file"


if __name__ == "__main__":
    main()
