"""The --background white / random fixtures (tests/golden/render_bg_*.npz,
train_bg_random_rgb.npz, written by tools/make_golden_background.py from the
reference's own NeRFNetwork.run): their inputs, and the CPU mirror on them.

A fixture stores the camera (pose, intrinsics, H, W) and the clamp (near, first
far, last far) instead of the rays and the [N,2] cam_near_far: inputs() rebuilds
both exactly (the generator asserts it), which keeps the SAM fixture below the
size of render_small_sam.npz."""
import numpy as np
import torch

from helpers import fixture_params, make_net, spec_from_fixture
from oracle import renderer as orc

NAMES = ["render_bg_white_rgb", "render_bg_white_sam", "render_bg_white_mask", "train_bg_random_rgb"]
OUT_KEYS = ("image", "depth", "weights_sum", "samvit", "instance_mask_logits", "weights", "proposal_loss",
            "distort_loss")


def near_far(n, near=0.05, far0=0.5, far1=4.0):
    """Per-ray cam_near_far [n,2]: with the synthetic parameters an unclamped
    view is almost opaque (weights_sum > 0.998 under 'white'), which could not
    tell the background modes apart; far planes from 0.5 to 4 spread
    weights_sum over 0.25 .. 0.96."""
    return torch.stack([torch.full((n,), float(near)), torch.linspace(float(far0), float(far1), n)],
                       dim=1).contiguous()


def inputs(fx):
    """(rays_o [N,3], rays_d [N,3], cam_near_far [N,2], bg_color or None) of a
    fixture, CPU tensors."""
    H, W = int(fx["H"]), int(fx["W"])
    ro, rd = orc.get_rays(np.asarray(fx["pose"]), np.asarray(fx["intrinsics"]), H, W)
    near, far0, far1 = [float(v) for v in fx["near_far"]]
    bg = torch.from_numpy(np.asarray(fx["bg_color"])) if "bg_color" in fx else None
    return ro, rd, near_far(H * W, near, far0, far1), bg


def fixture_net(fx, device):
    """The mirror network of a fixture: its parameters, background mode and
    train / eval state."""
    spec = spec_from_fixture(fx)
    net = make_net(spec, fixture_params(fx, spec), device)
    net.opt.background = str(fx["background"])
    net.train(bool(int(fx["train"])))
    return net


def run_kwargs(fx):
    kw = dict(return_feats=int("samvit" in fx), return_mask=int("instance_mask_logits" in fx))
    if kw["return_feats"]:
        kw.update(H=int(fx["H"]), W=int(fx["W"]))
    return kw


def run_mirror(fx):
    """This repository's CPU mirror on a fixture's inputs: run_torch with the
    oracle encoders (the pairing tests/test_mask_cpu.py holds to bit equality)."""
    from oracle_backend import oracle_encoders
    net = fixture_net(fx, "cpu")
    ro, rd, cnf, bg = inputs(fx)
    with oracle_encoders(), torch.no_grad():
        return net.run_torch(ro, rd, bg_color=bg, perturb=False, cam_near_far=cnf, **run_kwargs(fx))
