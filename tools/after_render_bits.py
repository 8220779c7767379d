#!/usr/bin/env python3
"""Fingerprints of the outputs of the entry points that run after a render
(mask_loss, present, evaluate, incoherent, batch_sampler .hip) for one library
build (SAMNERF_LIB, or the in-tree product), as sha256 prefixes of the raw
bytes on fixed-seed inputs made here.  Two builds whose lines match are
bit-identical on these workloads; tools/lib_bits.py does the same for the
render and training side.  usage (GPU box): [SAMNERF_LIB=...] python tools/after_render_bits.py"""
import hashlib
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "segment-anything-nerf_amd"))

import torch  # noqa: E402


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()[:16]


def mask_loss_bits(dev, out):
    from samnerf_amd.mask_loss import mask_loss
    base = dict(epsilon=1e-6, incoherent_uncertainty_weight=0.5, label_regularization_weight=0.0, patch_size=1,
                rgb_similarity_loss_weight=0.0, rgb_similarity_threshold=0.15, rgb_similarity_exp_weight=10.0,
                rgb_similarity_num_sample=20, rgb_similarity_iter=-1, rgb_similarity_use_pred_logistics=False,
                redundant_instance=0, mixed_sampling=False, local_sample_patch_size=16, num_local_sample=3,
                error_map=True, error_map_size=128, n_inst=5)
    K, M, n, L, Q, S = 5, 1500, 1280, 3, 256, 20
    for tag, local in (("global", False), ("local", True)):
        N = n + L * Q if local else 2049
        g = torch.Generator().manual_seed(11 + local)
        z = (2.0 * torch.randn(N, K, generator=g)).to(dev).requires_grad_(True)
        labels = torch.randint(0, K, (N,), generator=g)
        pal = torch.rand(4, 3, generator=g)
        image = (pal[torch.randint(0, 4, (N,), generator=g)] + 0.03 * torch.randn(N, 3, generator=g)).clamp(0, 1)
        kw = dict(incoherent=(torch.rand(N, generator=g) > 0.5).float().to(dev),
                  error_map=torch.rand(2, M, generator=g).to(dev))
        opt = dict(base, num_rays=N)
        rays = N
        if local:
            labels[n:][torch.rand(N - n, generator=g) < 0.3] = -1
            opt.update(num_rays=n, mixed_sampling=True, rgb_similarity_loss_weight=5.0,
                       label_regularization_weight=0.1, patch_size=16)
            kw.update(image=image.to(dev), depth=(2.0 + torch.rand(N, generator=g)).to(dev), global_step=1,
                      sample_index=torch.stack([torch.randperm(Q, generator=g)[:S] for _ in range(L)]).to(dev))
            rays = n
        kw["error_cells"] = (M + torch.randint(0, M, (rays,), generator=g)).to(dev)
        loss, terms, ids = mask_loss(z, labels.to(dev), rays, types.SimpleNamespace(**opt), **kw)
        loss.backward()
        out[f"mask_loss_{tag}"] = {"terms": {k: float(v).hex() for k, v in terms.items()}, "grad": sha(z.grad),
                                   "ids": sha(ids), "error_map": sha(kw["error_map"])}


def present_bits(dev, out):
    from samnerf_amd.present import present_frame
    g = torch.Generator().manual_seed(21)
    rH, rW, K = 33, 65, 5
    image, depth = torch.rand(rH, rW, 3, generator=g).to(dev), (1 + torch.rand(rH, rW, generator=g)).to(dev)
    kw = dict(logits=(2 * torch.randn(rH, rW, K, generator=g)).to(dev), n_inst=K,
              color_map=torch.rand(K, 3, generator=g).to(dev), return_extra=True)
    for mt in ("heatmap", "composition", "mask"):
        frame, extra = present_frame(image, depth, rH, rW, mask_type=mt, instance_id=1, **kw)
        out[f"present_{mt}"] = {"frame": sha(frame), "probs": sha(extra["probs"]), "ids": sha(extra["ids"])}
    frame, extra = present_frame(image, depth, 50, 97, mode="depth", mask_type="heatmap", instance_id=-1, **kw)
    out["present_depth"] = {"frame": sha(frame), "depth": sha(extra["depth"])}


def eval_bits(dev, out):
    from samnerf_amd.evaluate import eval_frame
    g = torch.Generator().manual_seed(31)
    H, W = 45, 70
    pred, truth = torch.rand(H * W, 3, generator=g).to(dev), torch.rand(H, W, 4, generator=g).to(dev)
    for K in (5, 33):
        z = (2 * torch.randn(H, W, K, generator=g)).to(dev)
        labels = torch.randint(-1, K, (H, W), generator=g).to(dev)
        r = eval_frame(pred, truth, buffers=True, logits=z, labels=labels, n_inst=K)
        out[f"eval_K{K}"] = {k: sha(r[k]) for k in ("stats", "probs", "ids", "pred_u8", "truth_u8", "error_u8")}


def incoherent_bits(dev, out):
    from samnerf_amd import incoherent
    g = torch.Generator().manual_seed(41)
    ids, pred = incoherent.render_mask_ids((2 * torch.randn(3000, 5, generator=g)).to(dev), 5, return_pred=True)
    masks = torch.randint(0, 4, (3, 1, 8, 12), generator=g).repeat_interleave(8, 2).repeat_interleave(8, 3).to(dev)
    out["incoherent"] = {"ids": sha(ids), "pred": sha(pred),
                         "map": sha(incoherent.get_incoherent_mask(masks, sfact=4)),
                         "table": sha(incoherent.incoherent_table(masks[:, 0], sfact=4))}
    if incoherent.last_path != "hip":
        raise RuntimeError(f"the incoherent masks ran on {incoherent.last_path!r}, not on the kernel")


def batch_bits(dev, out):
    from samnerf_amd import batch
    g = torch.Generator().manual_seed(51)
    M = 128
    weights = torch.rand(3, M * M, generator=g).to(dev)
    r = batch.hip_draw(batch.MODE_C, 3, 64, 96, 7, device=dev, patch=4, M=M, weights=weights,
                       philox=batch.PhiloxBatch(1234, 9))
    out["batch_draw_centred"] = {k: sha(v) for k, v in sorted(r.items()) if v is not None}


def main():
    dev = torch.device("cuda", 0)
    out = {}
    for part in (mask_loss_bits, present_bits, eval_bits, incoherent_bits, batch_bits):
        part(dev, out)
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
