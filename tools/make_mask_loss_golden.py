#!/usr/bin/env python3
"""Generate tests/golden/mask_loss.npz from the REFERENCE's own mask loss.

Runs only where the reference tree exists (tools/make_golden.py's
install_reference), never in a test.  The reference's Trainer.train_step,
rgb_similarity_loss and label_regularization (nerf/utils.py:761-870,
:941-1070) are bound to a stub object whose model.render returns canned
tensors, so what is recorded is the loss side of the --with_mask branch alone:
per case the inputs, the sample_index its torch.multinomial drew, the loss,
d loss / d logits by autograd and the updated error map -- in float32 and from
a float64 run of the same code on the same inputs and the same draw.

Cases: scripts/train_mask.sh's configuration past rgb_similarity_iter (Q = 16
and Q = 256 / S = 20), the error map off, incoherent_uncertainty_weight 0.5,
label regularisation with patch_size 4, redundant_instance 2 (the BCE form;
opt.n_inst is the total there, as Trainer.train_step's view needs) and
rgb_similarity_use_pred_logistics.  Also utils.py:269-275's inds_coarse of a
small image (through the reference's get_rays).

usage: PYTHONDONTWRITEBYTECODE=1 python tools/make_mask_loss_golden.py
"""
import json
import os
import sys
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import make_golden  # noqa: E402

SCRIPT = dict(epsilon=1e-6, rgb_similarity_loss_weight=5.0, rgb_similarity_threshold=0.15,
              incoherent_uncertainty_weight=1.0, redundant_instance=0, rgb_similarity_num_sample=5,
              label_regularization_weight=0.0, rgb_similarity_iter=600000, num_local_sample=3,
              local_sample_patch_size=4, mixed_sampling=True, error_map=True, error_map_size=8,
              rgb_similarity_exp_weight=10.0, rgb_similarity_use_pred_logistics=False, patch_size=1,
              n_inst=5, num_rays=96, with_sam=False, with_mask=True, background="white", cache_size=0)

CASES = {
    "script": dict(global_step=600001),
    "script_q256": dict(global_step=600001, num_local_sample=2, local_sample_patch_size=16,
                        rgb_similarity_num_sample=20),
    "no_error_map": dict(global_step=600001, error_map=False),
    "incoherent_half": dict(global_step=10, incoherent_uncertainty_weight=0.5),
    "label_reg": dict(global_step=10, label_regularization_weight=0.1, patch_size=4),
    "redundant": dict(global_step=600001, redundant_instance=2),
    "pred_logistics": dict(global_step=600001, rgb_similarity_use_pred_logistics=True),
}


def make_inputs(cfg, seed):
    g = torch.Generator().manual_seed(seed)
    n, L, Q, K = cfg["num_rays"], cfg["num_local_sample"], cfg["local_sample_patch_size"] ** 2, cfg["n_inst"]
    S, M = cfg["rgb_similarity_num_sample"], cfg["error_map_size"]
    N = n + L * Q
    x = {"logits": 2.0 * torch.randn(N, K, generator=g)}
    labels = torch.randint(0, K, (N,), generator=g)
    labels[n:][torch.rand(N - n, generator=g) < 0.3] = -1          # unlabelled: local rays only
    x["labels"] = labels
    palette = torch.rand(4, 3, generator=g)
    x["image"] = (palette[torch.randint(0, 4, (N,), generator=g)] + 0.03 * torch.randn(N, 3, generator=g)).clamp(0, 1)
    x["depth"] = 2.0 + torch.rand(N, generator=g)
    # incoherence in [0, 1]: the first S pixels of a patch are always eligible
    # (below 0.2), so the multinomial has S positive weights; the last patch
    # has none (the reference resets such a row to ones)
    inc = torch.rand(N, generator=g)
    loc = inc[n:].view(L, Q)
    loc[:, :S] *= 0.19
    loc[-1] = 0.5 + 0.5 * loc[-1]
    x["incoherent"] = (inc > 0.5).float()
    x["error_maps"] = inc
    x["error_map"] = torch.rand(2, M * M, generator=g)
    x["inds_coarse"] = torch.randint(0, M * M, (1, n), generator=g)  # n > cells / 2: duplicates
    return x


def run_reference(utils, cfg, x, dtype, seed, sample_index=None):
    """One Trainer.train_step on a stub; returns loss, grad, map, ids, draw."""
    # float64: the inputs are cast; the one op that mixes in a float32 tensor
    # of its own making is the BCE form's target (1. - int tensor), which
    # binary_cross_entropy refuses beside a float64 input: cast there
    real_bce = utils.F.binary_cross_entropy
    if dtype == torch.float64:
        utils.F.binary_cross_entropy = lambda inp, tgt, **kw: real_bce(inp, tgt.to(inp.dtype), **kw)
    try:
        def f(t):
            return t.to(dtype).clone()
        logits = f(x["logits"]).requires_grad_(True)
        outputs = {"instance_mask_logits": logits, "image": f(x["image"]), "depth": f(x["depth"])}
        st = types.SimpleNamespace()
        st.opt = types.SimpleNamespace(**{k: v for k, v in cfg.items() if k != "global_step"})
        st.device = torch.device("cpu")
        st.global_step = cfg["global_step"]
        st.error_map = f(x["error_map"]) if cfg["error_map"] else None
        st.model = types.SimpleNamespace(render=lambda *a, **k: outputs)
        st.rgb_similarity_loss = types.MethodType(utils.Trainer.rgb_similarity_loss, st)
        st.label_regularization = types.MethodType(utils.Trainer.label_regularization, st)
        N = logits.shape[0]
        data = {"rays_o": torch.zeros(N, 3), "rays_d": torch.zeros(N, 3), "index": [1], "H": 8, "W": 8,
                "masks": x["labels"][None].clone(), "incoherent_masks": f(x["incoherent"]),
                "error_maps": f(x["error_maps"]), "inds_coarse": x["inds_coarse"].clone()}
        drawn = []
        real = torch.multinomial

        def multinomial(w, **kw):
            drawn.append(real(w, **kw) if sample_index is None else sample_index.clone())
            return drawn[-1]
        torch.multinomial = multinomial
        torch.manual_seed(seed)
        try:
            pred, _, loss = utils.Trainer.train_step(st, data)
        finally:
            torch.multinomial = real
        loss.backward()
        grad = logits.grad if logits.grad is not None else torch.zeros_like(logits)
        emap = st.error_map.detach() if st.error_map is not None else torch.zeros(0, dtype=dtype)
        return loss.detach(), grad, emap, pred, (drawn[0] if drawn else torch.zeros(0, 0, dtype=torch.long))
    finally:
        utils.F.binary_cross_entropy = real_bce


def main():
    _, _, utils = make_golden.install_reference()
    out = {"cases": np.array(json.dumps(list(CASES)))}
    for ci, (name, over) in enumerate(CASES.items()):
        cfg = dict(SCRIPT, **over)
        seed = 100 + ci
        x = make_inputs(cfg, seed)
        loss32, grad32, map32, ids, draw = run_reference(utils, cfg, x, torch.float32, seed)
        loss64, grad64, map64, _, _ = run_reference(utils, cfg, x, torch.float64, seed,
                                                    sample_index=draw if draw.numel() else None)
        out[f"{name}/config"] = np.array(json.dumps(dict(cfg, seed=seed)))
        for k, v in x.items():
            out[f"{name}/{k}"] = v.numpy()
        for k, v in dict(sample_index=draw, pred_ids=ids, loss32=loss32, grad32=grad32, map32=map32,
                         loss64=loss64, grad64=grad64, map64=map64).items():
            out[f"{name}/{k}"] = v.numpy()
        print(f"{name}: N={x['logits'].shape[0]} loss32={float(loss32):.8f} "
              f"d(32,64)={abs(float(loss32) - float(loss64)):.2e} "
              f"grad d={float((grad32.double() - grad64).abs().max()):.2e} draw={tuple(draw.shape)}")
    # utils.py:269-275 through the reference's get_rays (all pixels, N = -1)
    H, W, size = 6, 10, 4
    res = utils.get_rays(torch.eye(4)[None], np.array([10.0, 10.0, W / 2, H / 2]), H, W, N=-1,
                         incoherent_mask_size=size)
    out["coarse/hws"] = np.array([H, W, size])
    out["coarse/inds_coarse"] = res["inds_coarse"].numpy()
    path = os.path.join(make_golden.GOLDEN, "mask_loss.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
