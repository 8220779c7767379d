"""tests/golden/mask_loss.npz (tools/make_mask_loss_golden.py: the reference's
own Trainer.train_step on canned renders, float32 and float64) for the CPU and
GPU tests of samnerf_amd.mask_loss, loaded once."""
import json
import types

import torch

import golden_file

golden = golden_file.loader("mask_loss.npz")._file


def case_names():
    return json.loads(str(golden()["cases"]))


def make_opt(**kw):
    """The reference's defaults (main.py:116-175) of the options the loss reads."""
    o = dict(epsilon=1e-6, incoherent_uncertainty_weight=1.0, label_regularization_weight=0.0,
             patch_size=1, rgb_similarity_loss_weight=0.0, rgb_similarity_threshold=0.3,
             rgb_similarity_exp_weight=10.0, rgb_similarity_num_sample=1, rgb_similarity_iter=-1,
             rgb_similarity_use_pred_logistics=False, redundant_instance=0, mixed_sampling=False,
             local_sample_patch_size=16, num_local_sample=2, error_map=False, error_map_size=128,
             n_inst=2, num_rays=4096)
    o.update(kw)
    return types.SimpleNamespace(**o)


def load_case(name, dtype=torch.float32, device="cpu"):
    """(opt, n, kwargs of mask_loss with fresh tensors, golden outputs)."""
    g = golden()
    cfg = json.loads(str(g[f"{name}/config"]))

    def t(key, dt=None):
        x = torch.from_numpy(g[f"{name}/{key}"])
        return x.to(device=device, dtype=dt if dt is not None else x.dtype).clone()
    opt = make_opt(**{k: v for k, v in cfg.items() if k not in ("global_step", "seed")})
    n = cfg["num_rays"]
    M = cfg["error_map_size"]
    kw = dict(global_step=cfg["global_step"], depth=t("depth", dtype), image=t("image", dtype),
              incoherent=t("incoherent", dtype))
    if cfg["error_map"]:
        kw["error_map"] = t("error_map", dtype)
        kw["error_cells"] = (1 * M * M + t("inds_coarse")).reshape(-1)      # data['index'] = [1]
    if g[f"{name}/sample_index"].size:
        kw["sample_index"] = t("sample_index")
    want = {k: torch.from_numpy(g[f"{name}/{k}"]) for k in
            ("loss32", "grad32", "map32", "loss64", "grad64", "map64", "pred_ids")}
    return opt, n, t("logits", dtype), t("labels"), kw, want, cfg


def local_incoherence(name):
    """What rgb_similarity_loss receives as `incoherent` (utils.py:1046-1056)."""
    g = golden()
    cfg = json.loads(str(g[f"{name}/config"]))
    src = g[f"{name}/error_maps"] if cfg["error_map"] else g[f"{name}/incoherent"]
    n, L, Q = cfg["num_rays"], cfg["num_local_sample"], cfg["local_sample_patch_size"] ** 2
    return torch.from_numpy(src)[n:].view(L, Q, -1), cfg
