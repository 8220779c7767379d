#!/usr/bin/env python3
"""Generate tests/golden/batch_sampler.npz from the REFERENCE's own ray
selection and collate.

Runs only where the reference tree exists (tools/make_golden.py's
install_reference), never in a test.  Recorded, each at a fixed
torch.manual_seed:

  * the tables of a small synthetic dataset (3 images of 120 x 120, a
    128 x 128 error map), low-entropy so that the file stays small;
  * per mode of get_rays' N > 0 branches (nerf/utils.py:174-242) the arguments
    and every output of the reference's get_rays: R (uniform, also on a
    96 x 120 image), P (one random patch), C (a patch centred on an error-map
    draw, one row and three rows) and E (error-map pixels without
    replacement);
  * the result dict of the reference's ColmapDataset.collate
    (nerf/colmap_provider.py:935-1204) bound to a stub dataset over those
    tables: the RGB stage's random batch, the mask stage with --error_map
    --mixed_sampling past rgb_similarity_iter, the mask stage's error-map
    pixels before it, and a patch centred on the ground-truth incoherent mask.

Only data goes into the file.

usage: PYTHONDONTWRITEBYTECODE=1 python tools/make_batch_sampler_golden.py
"""
import importlib
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

N_IMG, H, W, M = 3, 120, 120, 128

OPT = dict(num_rays=65, with_sam=False, with_mask=False, use_multi_res=False, rgb_similarity_iter=10,
           random_image_batch=False, patch_size=1, error_map=False, error_map_size=M, mixed_sampling=False,
           num_local_sample=3, local_sample_patch_size=4, enable_cam_near_far=True, online_resolution=H)

COLLATE = {
    "rgb_random": dict(opt=dict(random_image_batch=True), global_step=1, index=[1], default_intrinsics=True),
    "mask_mixed": dict(opt=dict(with_mask=True, error_map=True, mixed_sampling=True), global_step=11, index=[2],
                       default_intrinsics=False),
    "mask_error_pixels": dict(opt=dict(with_mask=True, error_map=True), global_step=1, index=[2],
                              default_intrinsics=True),
    "mask_incoherent_patch": dict(opt=dict(with_mask=True, patch_size=4), global_step=1, index=[0],
                                  default_intrinsics=True),
}


def rotation(g):
    q, r = torch.linalg.qr(torch.randn(3, 3, generator=g, dtype=torch.float64))
    q = q * torch.sign(torch.diagonal(r))
    if torch.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def make_tables(seed):
    g = torch.Generator().manual_seed(seed)
    poses = torch.eye(4, dtype=torch.float64).repeat(N_IMG, 1, 1)
    for k in range(N_IMG):
        poses[k, :3, :3] = rotation(g)
        poses[k, :3, 3] = torch.randn(3, generator=g, dtype=torch.float64)
    intr = torch.tensor([[130.0 + 7 * k, 128.0 - 5 * k, W / 2 + 0.25 * k, H / 2 - 0.5 * k] for k in range(N_IMG)])
    img, row, col, ch = np.ix_(np.arange(N_IMG), np.arange(H), np.arange(W), np.arange(4))
    images = ((row * 7 + col * 13 + img * 31 + ch * 5 + (row // 9) * (col // 11)) % 256).astype(np.uint8)
    masks = ((row // 17 + col // 23 + img) % 5 - (row % 29 == 0)).astype(np.int64)[..., :1]
    inc = ((row // 8 + col // 8 + img) % 3 == 0)[..., 0].reshape(N_IMG, H * W)
    emap = torch.randint(1, 17, (N_IMG, M * M), generator=g).float() / 16
    emap[1, ::3] = 0.0
    cnf = torch.tensor([[0.1 + 0.05 * k, 4.0 + k] for k in range(N_IMG)])
    return dict(poses=poses.float(), intrinsics=intr, images=torch.from_numpy(images), masks=torch.from_numpy(masks),
                gt_incoherent_masks=torch.from_numpy(inc), error_map=emap, cam_near_far=cnf)


def record(out, name, res):
    keys = []
    for k, v in res.items():
        if torch.is_tensor(v):
            out[f"{name}/{k}"] = v.detach().cpu().numpy()
        elif isinstance(v, (list, int, bool, np.integer)):
            out[f"{name}/{k}"] = np.asarray(v)
        else:
            continue
        keys.append(k)
    out[f"{name}/keys"] = np.array(json.dumps(keys))


def import_provider():
    for n in ("tqdm", "scipy", "scipy.spatial", "scipy.spatial.transform", "pyquaternion"):
        try:
            importlib.import_module(n)
        except ImportError:
            make_golden._stub(n)
    return importlib.import_module("nerf.colmap_provider")


def main():
    _, _, utils = make_golden.install_reference()
    provider = import_provider()
    assert os.path.realpath(provider.__file__).startswith(make_golden.REF + "/")
    t = make_tables(7)
    out = {f"tables/{k}": v.numpy() for k, v in t.items()}
    out["tables/hwm"] = np.array([H, W, M])

    # ---- get_rays, mode by mode
    def rays(name, seed, idx, h, w, n, **kw):
        torch.manual_seed(seed)
        if idx is None:
            idx = torch.randint(0, N_IMG, size=(n,))
        idx = torch.as_tensor(idx)
        res = utils.get_rays(t["poses"][idx], t["intrinsics"][idx], h, w, n, **kw)
        res["index"] = idx
        record(out, f"rays/{name}", res)
        out[f"rays/{name}/args"] = np.array(json.dumps(dict(
            seed=seed, H=h, W=w, N=n, **{k: v for k, v in kw.items() if not torch.is_tensor(v)})))
        print(name, {k: tuple(v.shape) for k, v in res.items() if torch.is_tensor(v)})

    rays("R", 21, None, H, W, 65, random_sample=True, incoherent_mask_size=M)
    rays("R_rect", 22, None, 96, W, 65, random_sample=True, incoherent_mask_size=M)
    rays("P", 23, [1], H, W, 16, patch_size=4, incoherent_mask_size=M)
    rays("C", 24, [1], H, W, 1, patch_size=4, incoherent_mask=t["error_map"][[1]],
         include_incoherent_region=True, incoherent_mask_size=M)
    rows = torch.tensor([2, 0, 2])
    rays("C3", 25, rows[:, None].expand(-1, 16).reshape(-1), H, W, 1, patch_size=4,
         incoherent_mask=t["error_map"][rows], include_incoherent_region=True, incoherent_mask_size=M)
    out["rays/C3/rows"] = rows.numpy()
    rays("E", 26, [2], H, W, 65, patch_size=1, incoherent_mask=t["error_map"][[2]], incoherent_mask_size=M)

    # ---- the collate, on a stub dataset
    for ci, (name, case) in enumerate(COLLATE.items()):
        st = types.SimpleNamespace(**{k: v.clone() for k, v in t.items()})
        st.opt = types.SimpleNamespace(**dict(OPT, **case["opt"]))
        st.training, st.preload, st.device = True, True, torch.device("cpu")
        st.global_step, st.H, st.W = case["global_step"], H, W
        st.use_default_intrinsics = case["default_intrinsics"]
        st.incoherent_masks, st.incoherent_mask_size = st.gt_incoherent_masks, H
        st.img_names = None
        if not st.opt.with_mask:
            st.masks = st.gt_incoherent_masks = st.incoherent_masks = st.error_map = None
        seed = 40 + ci
        torch.manual_seed(seed)
        res = provider.ColmapDataset.collate(st, list(case["index"]))
        record(out, f"collate/{name}", res)
        out[f"collate/{name}/case"] = np.array(json.dumps(dict(case, seed=seed, opt=dict(OPT, **case["opt"]))))
        print(name, {k: (tuple(v.shape), str(v.dtype)) for k, v in res.items() if torch.is_tensor(v)})
    out["collate/cases"] = np.array(json.dumps(list(COLLATE)))
    path = os.path.join(make_golden.GOLDEN, "batch_sampler.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
