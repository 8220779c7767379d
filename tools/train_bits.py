#!/usr/bin/env python3
"""Fingerprints of the training heads' deterministic outputs for one library
build (SAMNERF_LIB, or the in-tree product), as sha256 prefixes of the raw
bytes on fixed-seed inputs made here: the SAM head's forward and backward
(sam_head_train.hip), the 'default' mask head's training logits in both head
modes and the adaptive 'density' head's logits and weight gradients
(mask_head_train.hip), and the four workspace sizes.  The 'default' mask
head's dW and m_grid gradients go through float atomics and are not here.
Two builds whose lines match are bit-identical on these workloads;
tools/lib_bits.py and tools/after_render_bits.py do the same for the render
and for what runs after it.
usage (GPU box): [SAMNERF_LIB=...] python tools/train_bits.py"""
import ctypes
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "segment-anything-nerf_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

SIZES_N = (1, 37, 4096, 65536)


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()[:16]


def make_net(dev, seed, **spec_kw):
    """A small-table synth model (the heads do not depend on the table sizes)."""
    from nerf.network import NeRFNetwork, default_opt
    from samnerf_amd import synth
    spec = synth.ModelSpec(grid_log2=12, s_grid_log2=11, prop_log2=10, m_grid_log2=12, **spec_kw)
    params = synth.make_params(spec, seed=seed, emb_scale=0.5, ln_jitter=0.3)
    opt = default_opt(with_sam=spec.with_sam, grid_log2=12, s_grid_log2=11, prop_log2=10, m_grid_log2=12,
                      with_mask=spec.with_mask, mask_mlp_type=spec.mask_type, adaptive_mlp_type=spec.adaptive_type,
                      n_inst=spec.n_inst, sum_after_mlp=spec.sum_after_mlp)
    net = NeRFNetwork(opt)
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in params.items()})
    return net.to(dev).train()


def rays(dev, n):
    from samnerf_amd import ops, synth
    pose, intr = synth.gui_camera(16, 16, rot=synth.random_rotation(4))
    ro, rd = ops.get_rays(pose, intr, 16, 16, device=dev)
    return ro[:n].contiguous(), rd[:n].contiguous()


def sam_head_bits(dev, out, sizes):
    from samnerf_amd._lib import lib
    from samnerf_amd.fused import FusedRenderer, _head_params, _SamHeadTrain
    net = make_net(dev, 15, with_sam=True)
    fr = FusedRenderer(net)
    params = _head_params(net)
    names = [f"w{i}" for i in range(5)] + [f"b{i}" for i in range(5)] + ["ln_w", "ln_b"]
    for n in (37, 1000, 4096):
        g = torch.Generator().manual_seed(100 + n)
        rows = (torch.randn(n, 164, generator=g) * torch.rand(1, 164, generator=g) * 3).to(dev)
        rows[:, 163] = 0.0
        G = torch.randn(n, 256, generator=g).to(dev)
        r = rows.clone().requires_grad_(True)
        samvit = _SamHeadTrain.apply(r, fr, *params)
        samvit.backward(G)
        out[f"sam_head_N{n}"] = dict({"samvit": sha(samvit), "grad_rows": sha(r.grad)},
                                     **{k: sha(p.grad) for k, p in zip(names, params)})
        for p in params:
            p.grad = None
    sizes["head_train"] = [int(lib().samnerf_head_train_workspace_size(n)) for n in SIZES_N]
    m = fr.call_model()
    sizes["render_sam"] = [int(lib().samnerf_render_workspace_size(ctypes.byref(m), n)) for n in SIZES_N]


def mask_bits(dev, out, sizes):
    from samnerf_amd._lib import lib
    from samnerf_amd.fused import FusedRenderer, render_mask_train
    net = make_net(dev, 21, with_sam=False, with_mask=True, mask_type="default", n_inst=5)
    for p in net.parameters():
        p.requires_grad = False
    for head_mode in (1, 0):
        net.head_mode = head_mode
        for n in (37, 100):
            ro, rd = rays(dev, n)
            logits = render_mask_train(FusedRenderer(net), ro, rd)["instance_mask_logits"]
            out[f"mask_logits_h{head_mode}_N{n}"] = sha(logits)
    m = FusedRenderer(net).call_model(with_mask=2)
    sizes["mask_train"] = [int(lib().samnerf_mask_train_workspace_size(n)) for n in SIZES_N]
    sizes["render_mask"] = [int(lib().samnerf_render_workspace_size(ctypes.byref(m), n)) for n in SIZES_N]


def adaptive_bits(dev, out, sizes):
    from samnerf_amd._lib import lib
    from samnerf_amd.fused import FusedRenderer, render_mask_train
    net = make_net(dev, 22, with_sam=False, with_mask=True, mask_type="adaptive", adaptive_type="density", n_inst=5,
                   sum_after_mlp=True)
    net.head_mode = 1
    for k, p in net.named_parameters():
        p.requires_grad = k.startswith("mask_mlp")
    ro, rd = rays(dev, 37)
    with torch.enable_grad():
        logits = render_mask_train(FusedRenderer(net), ro, rd)["instance_mask_logits"]
    logits.backward(torch.randn(37, 5, generator=torch.Generator().manual_seed(9)).to(dev))
    out["adaptive_density_N37"] = dict({"logits": sha(logits)},
                                       **{f"w{i}": sha(layer.weight.grad) for i, layer in enumerate(net.mask_mlp)})
    m = FusedRenderer(net).call_model(with_mask=2)
    sizes["render_adaptive_train"] = [int(lib().samnerf_render_workspace_size(ctypes.byref(m), n)) for n in SIZES_N]


def rgb_sizes(dev, sizes):
    from samnerf_amd._lib import lib
    from samnerf_amd.fused import FusedRenderer
    m = FusedRenderer(make_net(dev, 12, with_sam=False)).call_model()
    sizes["rgb_train"] = [int(lib().samnerf_rgb_train_workspace_size(ctypes.byref(m), n)) for n in SIZES_N]
    sizes["render_rgb"] = [int(lib().samnerf_render_workspace_size(ctypes.byref(m), n)) for n in SIZES_N]


def main():
    dev = torch.device("cuda", 0)
    out, sizes = {}, {}
    sam_head_bits(dev, out, sizes)
    mask_bits(dev, out, sizes)
    adaptive_bits(dev, out, sizes)
    rgb_sizes(dev, sizes)
    out["workspace_bytes"] = {"N": list(SIZES_N), **sizes}
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
