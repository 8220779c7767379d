"""tests/golden/batch_sampler.npz (tools/make_batch_sampler_golden.py): the
reference's get_rays and collate on a small synthetic dataset, loaded once."""
import json
import types

import torch

import golden_file

_G = golden_file.loader("batch_sampler.npz")
GOLDEN, golden = _G.path, _G._file


def tables():
    g = golden()
    return {k[len("tables/"):]: torch.from_numpy(v) for k, v in g.items() if k.startswith("tables/") and k != "tables/hwm"}


def hwm():
    return tuple(int(v) for v in golden()["tables/hwm"])


def make_source(device="cpu", with_mask=True, H=None, **over):
    """A BatchSource over the golden's tables (the reference's stub dataset:
    incoherent_masks is gt_incoherent_masks, size H)."""
    from samnerf_amd.batch import BatchSource
    t = {k: v.to(device) for k, v in tables().items()}
    h, w, _ = hwm()
    kw = dict(images=t["images"], cam_near_far=t["cam_near_far"])
    if with_mask:
        kw.update(masks=t["masks"], incoherent_masks=t["gt_incoherent_masks"],
                  gt_incoherent_masks=t["gt_incoherent_masks"], error_map=t["error_map"].clone())
    kw.update(over)
    if H is not None:                                  # a shorter image: the tables cut to H rows
        kw = {k: (v[:, :H].contiguous() if k in ("images", "masks") and v is not None else v) for k, v in kw.items()}
        kw["incoherent_masks"] = kw["gt_incoherent_masks"] = None
        h = H
    return BatchSource(t["poses"], t["intrinsics"], h, w, **kw)


def rays_case(name):
    g = golden()
    p = f"rays/{name}/"
    res = {k[len(p):]: v for k, v in g.items() if k.startswith(p) and k[len(p):] not in ("keys", "args")}
    return json.loads(str(g[p + "args"])), {k: torch.from_numpy(v) for k, v in res.items()}


def collate_cases():
    return json.loads(str(golden()["collate/cases"]))


def collate_case(name):
    g = golden()
    p = f"collate/{name}/"
    case = json.loads(str(g[p + "case"]))
    keys = json.loads(str(g[p + "keys"]))
    return case, {k: g[p + k] for k in keys}, types.SimpleNamespace(**case["opt"])
