#!/usr/bin/env python3
"""Generate the --background white / random fixtures under tests/golden/ from
the REFERENCE's own NeRFNetwork.run (nerf/renderer.py:221-464), with the stubs
and stand-in encoders of tools/make_golden.py (nothing of the reference is
copied; it runs only where the reference tree exists):

  render_bg_white_rgb.npz   eval, background 'white', RGB model, 16 x 16 rays,
                            bg_color a [3] tensor (0.2, 0.5, 0.9)
  render_bg_white_sam.npz   the same with SAM features (return_feats=1), bg_color None
  render_bg_white_mask.npz  the 'default' mask head, return_mask=1
  train_bg_random_rgb.npz   net.train(), background 'random', a per-ray bg_color
                            [256,3] from a seeded generator, perturb=False:
                            image, depth, weights_sum, weights, proposal_loss,
                            distort_loss

Every fixture clamps the rays with a per-ray cam_near_far [N,2], near 0.05 and
far linspace(0.5, 4.0, N): with the synthetic parameters an unclamped view is
almost opaque (weights_sum 0.998-0.999 under 'white'), which could not tell the
background modes apart.  Before anything is written the generator asserts
min(weights_sum) < 0.3, max(weights_sum) > 0.9 and that at least half the rays
have 0.3 < weights_sum < 0.9.

distort_loss: the reference's distort_loss (renderer.py:17-27) calls the third-
party torch_efficient_distloss.eff_distloss, absent here (make_golden_losses.py);
the stub module is given this repository's restatement of that function
(nerf/renderer.py eff_distloss, pinned by tests/test_losses.py against the
defining double sum), so the stored value is the reference's own intervals and
mid points through the restated third-party sum.

The reference run and the mirror check are two processes, because both trees
name their package `nerf`: this process runs the reference and writes the
candidates to a temporary directory; a child (--verify DIR) runs this
repository's CPU mirror -- run_torch with the oracle encoders, the pairing
tests/test_mask_cpu.py holds to bit equality -- on each and requires every
output to agree bit for bit; only then are the files moved to tests/golden/.

usage: PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_background.py
"""
import argparse
import importlib.util
import os
import shutil
import subprocess
import sys
import tempfile

sys.dont_write_bytecode = True
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

GOLDEN = os.path.join(REPO, "tests", "golden")
SMALL = dict(grid_log2=12, s_grid_log2=10, prop_log2=10)
H = W = 16


from background_fixtures import NAMES, OUT_KEYS, inputs, near_far, run_mirror  # noqa: E402

NEAR, FAR0, FAR1 = 0.05, 0.5, 4.0


def check_spread(name, ws):
    ws = np.asarray(ws).reshape(-1)
    mid = float(((ws > 0.3) & (ws < 0.9)).mean())
    print(f"  {name}: weights_sum min {ws.min():.4f} max {ws.max():.4f}, {mid:.2f} of the rays in (0.3, 0.9)")
    assert ws.min() < 0.3 and ws.max() > 0.9 and mid >= 0.5, "the view does not separate the background modes"


def cases():
    """name -> (ModelSpec keywords, seed, rot_seed, background, train, run keywords)"""
    g = torch.Generator().manual_seed(21)
    return {
        "render_bg_white_rgb": (dict(with_sam=False, **SMALL), 12, 3, "white", False,
                                dict(bg_color=torch.tensor([0.2, 0.5, 0.9]))),
        "render_bg_white_sam": (dict(with_sam=True, **SMALL), 12, 4, "white", False,
                                dict(bg_color=None, return_feats=1, H=H, W=W)),
        "render_bg_white_mask": (dict(with_sam=False, with_mask=True, mask_type="default", sum_after_mlp=True,
                                      m_grid_log2=10, **SMALL), 12, 6, "white", False,
                                 dict(bg_color=None, return_mask=1)),
        "train_bg_random_rgb": (dict(with_sam=False, **SMALL), 12, 5, "random", True,
                                dict(bg_color=torch.rand(H * W, 3, generator=g), perturb=False)),
    }


def reference_outputs(tmp):
    import make_golden as mg
    from oracle import encoders as enc
    from oracle import renderer as orc
    from oracle import synth
    enc.build()
    network, renderer, _ = mg.install_reference()
    # the absent third-party sum behind the reference's distort_loss: this
    # repository's restatement, loaded by file (its package is named `nerf` too)
    spec_ = importlib.util.spec_from_file_location(
        "samnerf_mirror_renderer", os.path.join(REPO, "segment-anything-nerf_amd", "nerf", "renderer.py"))
    mirror = importlib.util.module_from_spec(spec_)
    spec_.loader.exec_module(mirror)
    renderer.eff_distloss = mirror.eff_distloss
    for name, (kw, seed, rot_seed, background, train, run_kw) in cases().items():
        spec = synth.ModelSpec(**kw)
        mg.TABLE_LOG2.clear()
        mg.TABLE_LOG2[(16, 2, int(2048 * spec.grid_bound))] = spec.grid_log2
        mg.TABLE_LOG2[(16, 8, 512)] = spec.m_grid_log2 if spec.with_mask else spec.s_grid_log2
        mg.TABLE_LOG2[(5, 2, 128)] = spec.prop_log2
        mg.TABLE_LOG2[(5, 2, 256)] = spec.prop_log2
        params = synth.make_params(spec, seed=seed, emb_scale=0.5, ln_jitter=0.1)
        opt = mg.make_opt(spec)
        opt.background = background
        model = network.NeRFNetwork(opt)
        model.load_state_dict({k: torch.from_numpy(np.asarray(params[k])) for k in model.state_dict()},
                              strict=True)
        model.train(train)
        pose, intr = synth.gui_camera(W, H, rot=synth.random_rotation(rot_seed))
        rays_o, rays_d = orc.get_rays(pose, intr, H, W)
        cnf = near_far(H * W, NEAR, FAR0, FAR1)
        with torch.no_grad():
            ref = model.run(rays_o, rays_d, cam_near_far=cnf, **run_kw)
        check_spread(name, ref["weights_sum"].detach().numpy())
        out = dict(
            spec=np.array([spec.with_sam, spec.grid_log2, spec.s_grid_log2, spec.prop_log2], np.int64),
            mask_spec=np.array([spec.with_mask, spec.n_inst, spec.redundant_instance, spec.m_grid_log2,
                                spec.sum_after_mlp], np.int64),
            mask_types=np.array([spec.mask_type, spec.adaptive_type]),
            seed=np.int64(seed), emb_scale=np.float64(0.5), ln_jitter=np.float64(0.1),
            background=np.array(background), train=np.int64(train),
            H=np.int64(H), W=np.int64(W), pose=pose, intrinsics=intr,
            near_far=np.array([NEAR, FAR0, FAR1], np.float32))
        # (the rays and the [N,2] clamp are rebuilt from these by
        # tests/background_fixtures.py inputs(), bit for bit: with them stored
        # the SAM fixture would exceed render_small_sam.npz)
        ro2, rd2, cnf2, _ = inputs({**out, **({"bg_color": run_kw["bg_color"].numpy()}
                                              if run_kw.get("bg_color") is not None else {})})
        assert torch.equal(ro2, rays_o) and torch.equal(rd2, rays_d) and torch.equal(cnf2, cnf)
        if run_kw.get("bg_color") is not None:
            out["bg_color"] = run_kw["bg_color"].numpy()
        for k in OUT_KEYS:
            if k in ref and torch.is_tensor(ref[k]):
                v = ref[k].detach()          # (update_proposal re-enables grad inside no_grad)
                out[k] = v.reshape(H * W, -1).numpy() if k == "samvit" else v.numpy()
        if train:
            assert "weights" in out and "proposal_loss" in out and "distort_loss" in out, sorted(out)
        np.savez_compressed(os.path.join(tmp, name + ".npz"), **out)
        size = os.path.getsize(os.path.join(tmp, name + ".npz"))
        limit = os.path.getsize(os.path.join(GOLDEN, "render_small_sam.npz"))
        print(f"  {name}: {size} bytes (limit {limit})")
        assert size < limit, name


def verify(tmp):
    from oracle import encoders as enc
    enc.build()
    for name in NAMES:
        fx = np.load(os.path.join(tmp, name + ".npz"))
        out = run_mirror(fx)
        for k in OUT_KEYS:
            if k in fx:
                a = out[k].detach().reshape(fx[k].shape).numpy()
                d = float(np.abs(a.astype(np.float64) - fx[k]).max())
                print(f"  {name}: {k:22s} max|ref-mirror| = {d:.3e}")
                assert np.array_equal(a, fx[k]), f"the CPU mirror diverges from the reference on {name}/{k}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--verify", metavar="DIR", help="(child) check the candidates in DIR against the CPU mirror")
    args = ap.parse_args()
    if args.verify:
        verify(args.verify)
        return
    with tempfile.TemporaryDirectory() as tmp:
        reference_outputs(tmp)
        env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
        subprocess.run([sys.executable, os.path.abspath(__file__), "--verify", tmp], check=True, env=env)
        for name in NAMES:
            shutil.move(os.path.join(tmp, name + ".npz"), os.path.join(GOLDEN, name + ".npz"))
            print("  wrote", os.path.join("tests", "golden", name + ".npz"))


if __name__ == "__main__":
    main()
