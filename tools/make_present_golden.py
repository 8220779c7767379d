#!/usr/bin/env python3
"""Generate tests/golden/present.npz from the REFERENCE's own frame
presentation: what Trainer.test_step / test_gui and NeRFGUI do to a render's
outputs before the GUI shows them.

Runs only where the reference tree exists (tools/make_golden.py's
install_reference), never in a test.  Recorded, on seeded inputs:

  * color_map: the table of nerf/utils.py:606-610, with matplotlib's documented
    successor of the removed plt.cm.get_cmap (colormaps[...].resampled);
  * per mask case (size, K, n_inst): the softmax / sigmoid / max / argmax lines
    of test_step (a literal restatement of utils.py:1264-1306) and, per
    --render_mask_type and --render_mask_instance_id, the frame from the
    reference's overlay_mask_heatmap / overlay_mask_composition /
    overlay_mask_only; the float64 evaluation of the probabilities and of the
    heatmap frame beside the float32 one;
  * overlay_mask and overlay_point (click by click and all together);
  * test_gui's two F.interpolate calls;
  * NeRFGUI.prepare_buffer and NeRFGUI.test_step's spp update, called unbound
    on a stub (image and depth mode; a constant depth, one with a NaN).

overlay_mask_only with a render id indexes its [H, W, 3] image with the
flattened [H * W] mask and raises an IndexError in the reference; the recording
of those cases is the same two lines with the mask in its [H, W] shape, and
`mask_only_raises` records that the reference did raise.

The logits are multiples of 1/8, so that two probabilities of a pixel are
either equal because their logits are, or clearly apart: the generator checks
that the top two float64 probabilities of every pixel differ by at least 1e-3
or are exactly equal, with at least 5 % exact ties over varied column pairs,
and refuses to write the file otherwise.  No pixel is then excluded from any
comparison.

Only data goes into the file.

usage: PYTHONDONTWRITEBYTECODE=1 python tools/make_present_golden.py
"""
import importlib
import json
import os
import sys
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import matplotlib  # noqa: E402  (before install_reference, which stubs what is not imported)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import make_golden  # noqa: E402

# (rH, rW, K, n_inst): every K at the smallest size, K = 5 (two redundant
# columns) over five workgroups with a ragged last wave, K = 32 over two
MASK_CASES = [(5, 7, 1, 1), (5, 7, 2, 2), (5, 7, 3, 3), (5, 7, 5, 3), (5, 7, 32, 32), (33, 65, 5, 3),
              (17, 17, 32, 32)]
SIZES = [(5, 7), (33, 65)]
RESIZES = [(5, 7, 13, 19), (33, 65, 50, 97), (33, 65, 16, 32)]
MASK_TYPES = ("heatmap", "composition", "mask")
SPPS = (0, 1, 5)


def instance_ids(K, n_inst):
    """-1, an id in range, one >= n_inst (a redundant column where there is one)."""
    return (-1, min(1, n_inst - 1), n_inst)


def make_logits(g, rH, rW, K):
    z = torch.round(2.0 * torch.randn(rH, rW, K, generator=g) * 8) / 8
    if K > 1:
        flat = z.view(-1, K)
        rows = torch.nonzero(torch.rand(flat.shape[0], generator=g) < 0.12)[:, 0]
        for r in rows.tolist():
            a, b = torch.randperm(K, generator=g)[:2].tolist()
            flat[r, a] = flat[r, b] = flat[r].max() + 0.5
    return z


def check_logits(z, n_inst):
    """The top two float64 probabilities of every pixel: >= 1e-3 apart, or equal
    because the logits are."""
    K = z.shape[-1]
    if K == 1:
        return 0.0, set()
    p = torch.softmax(z.double(), -1) if n_inst > 1 else torch.sigmoid(z.double())
    top, idx = torch.topk(p.view(-1, K), 2, dim=-1)
    zt = torch.gather(z.view(-1, K), 1, idx)
    gap = top[:, 0] - top[:, 1]
    tie = gap == 0
    assert bool(((gap >= 1e-3) | tie).all()), "a pixel's top two probabilities are closer than 1e-3"
    assert bool((zt[tie, 0] == zt[tie, 1]).all()), "a tie that is not a tie of the logits"
    pairs = {tuple(sorted(r)) for r in idx[tie].tolist()}
    return float(tie.double().mean()), pairs


def mask_lines(utils, inst_mask, pred_rgb, n_inst, mask_type, instance_id, color_map):
    """utils.py:1267-1306 with opt.* as arguments; returns (pred_rgb, pred_mask, max, argmax, raised)."""
    raised = False
    if n_inst > 1:
        inst_mask = torch.softmax(inst_mask, dim=-1)
        pred_mask = inst_mask
    else:
        pred_mask = torch.sigmoid(inst_mask)
    if mask_type == 'heatmap':
        if instance_id >= 0 and instance_id < n_inst:
            instance_mask = pred_mask[..., instance_id]
            instance = instance_id
        else:
            instance_mask, _ = torch.max(pred_mask, -1)
            instance = pred_mask.argmax(-1)
        pred_rgb = utils.overlay_mask_heatmap(instance_mask, instance, color_map=color_map)
    elif mask_type == 'composition':
        instance = pred_mask.argmax(-1)
        render_id = instance_id if instance_id >= 0 and instance_id < n_inst else -1
        pred_rgb = utils.overlay_mask_composition(pred_rgb, instance, color_map=color_map, render_id=render_id)
    elif mask_type == 'mask':
        instance = pred_mask.argmax(-1)
        render_id = instance_id if instance_id >= 0 and instance_id < n_inst else -1
        try:
            pred_rgb = utils.overlay_mask_only(instance, color_map=color_map, render_id=render_id)
        except IndexError:
            raised = True
            pred_rgb = torch.zeros([*instance.shape, 3])
            pred_rgb[instance == render_id] = color_map[render_id]
    mx, _ = torch.max(pred_mask, -1)
    return pred_rgb, pred_mask, mx, pred_mask.argmax(-1), raised


def rand_image(g, H, W):
    """Colours of 8 bits (k / 255): copies of them compress, so the file stays small."""
    return torch.randint(0, 256, (H, W, 3), generator=g).float() / 255


def click_sets(H, W):
    """(x, y): interior, within 2 pixels of each edge, the bottom-right corner."""
    return {"interior": [[W // 2, H // 2]], "left": [[1, H // 2]], "top": [[W // 2, 1]], "right": [[W - 1, H // 2]],
            "bottom": [[W // 2, H - 1]], "corner": [[W - 1, H - 1]],
            "all": [[W // 2, H // 2], [1, H // 2], [W // 2, 1], [W - 1, H // 2], [W // 2, H - 1], [W - 1, H - 1]]}


class _Event:
    def __init__(self, *a, **k):
        pass

    def record(self):
        pass

    def elapsed_time(self, other):
        return 1.0


def gui_stub(gui, mode, outputs):
    st = types.SimpleNamespace(mode=mode, need_update=True, spp=1, opt=types.SimpleNamespace(max_spp=64),
                               need_update_user_inputs=False, W=0, H=0, bg_color=None, downscale=1,
                               dynamic_resolution=False, cam=types.SimpleNamespace(pose=None, intrinsics=None),
                               render_buffer=None)
    st.trainer = types.SimpleNamespace(test_gui=lambda *a, **k: outputs)
    st.prepare_buffer = types.MethodType(gui.NeRFGUI.prepare_buffer, st)
    return st


def main():
    _, _, utils = make_golden.install_reference()
    for n in ("scipy", "scipy.spatial", "scipy.spatial.transform"):
        try:
            importlib.import_module(n)
        except ImportError:
            make_golden._stub(n)
    gui = importlib.import_module("nerf.gui")
    assert os.path.realpath(gui.__file__).startswith(make_golden.REF + "/")
    torch.cuda.Event, torch.cuda.synchronize = _Event, lambda *a, **k: None     # NeRFGUI.test_step's timers
    out = {}

    # ---- utils.py:606-610 (plt.cm.get_cmap('gist_ncar', 100) in its present spelling)
    cmap = matplotlib.colormaps['gist_ncar'].resampled(100)
    table = np.multiply([cmap((i * 7 + 5) % 100)[:3] for i in range(100)], 1)
    color_map = torch.from_numpy(table).to(torch.float)
    out["color_map"] = color_map.numpy()

    g = torch.Generator().manual_seed(20)
    frames = {}
    for rH, rW in SIZES:
        frames[rH, rW] = (rand_image(g, rH, rW), 0.3 + 2.0 * torch.rand(rH, rW, generator=g))
        out[f"image/{rH}x{rW}"], out[f"depth/{rH}x{rW}"] = (t.numpy() for t in frames[rH, rW])
    frames[17, 17] = (rand_image(g, 17, 17), None)
    out["image/17x17"] = frames[17, 17][0].numpy()

    # ---- the mask views
    raised = []
    for ci, (rH, rW, K, n_inst) in enumerate(MASK_CASES):
        z = make_logits(g, rH, rW, K)
        ties, pairs = check_logits(z, n_inst)
        if K > 1:
            assert ties >= 0.05 and len(pairs) >= min(3, K * (K - 1) // 2), (ties, pairs)
        image = frames[rH, rW][0]
        name = f"mask/{ci}"
        out[f"{name}/logits"] = z.numpy()
        for mask_type in MASK_TYPES:
            for iid in instance_ids(K, n_inst):
                rgb, p32, mx, arg, r = mask_lines(utils, z.clone(), image.clone(), n_inst, mask_type, iid, color_map)
                out[f"{name}/{mask_type}/{iid}/frame32"] = rgb.numpy()
                if r:
                    raised.append([ci, iid])
                if mask_type == "heatmap":
                    rgb64, p64, _, arg64, _ = mask_lines(utils, z.double(), image.double(), n_inst, mask_type, iid,
                                                         color_map.double())
                    assert torch.equal(arg, arg64)
                    out[f"{name}/{mask_type}/{iid}/frame64"] = rgb64.numpy()
        out[f"{name}/probs32"], out[f"{name}/probs64"] = p32.numpy(), p64.numpy()
        out[f"{name}/max32"], out[f"{name}/ids"] = mx.numpy(), arg.numpy()
        print(name, (rH, rW, K, n_inst), f"ties {ties:.3f} at {len(pairs)} column pairs")
    out["mask/cases"] = np.array(json.dumps(MASK_CASES))
    out["mask_only_raises"] = np.array(json.dumps(raised))

    # ---- overlay_mask, overlay_point
    for rH, rW in SIZES:
        image = frames[rH, rW][0]
        sam = torch.rand(rH, rW, generator=g) < 0.4
        out[f"sam/{rH}x{rW}/mask"] = sam.numpy()
        out[f"sam/{rH}x{rW}/frame32"] = utils.overlay_mask(image.clone(), sam).numpy()
        for cname, pts in click_sets(rH, rW).items():
            pts = np.asarray(pts, np.int32)
            out[f"points/{rH}x{rW}/{cname}/points"] = pts
            out[f"points/{rH}x{rW}/{cname}/frame32"] = utils.overlay_point(image.clone(), pts).numpy()
        # the two together, as utils.py:1396-1399
        pts = np.asarray(click_sets(rH, rW)["all"], np.int32)
        out[f"sam_points/{rH}x{rW}/frame32"] = utils.overlay_point(utils.overlay_mask(image.clone(), sam), pts).numpy()

    # ---- utils.py:1698-1702
    for rH, rW, H, W in RESIZES:
        preds, preds_depth = frames[rH, rW]
        a = F.interpolate(preds.unsqueeze(0).permute(0, 3, 1, 2), size=(
            H, W), mode='nearest').permute(0, 2, 3, 1).squeeze(0).contiguous()
        b = F.interpolate(preds_depth.unsqueeze(0).unsqueeze(
            1), size=(H, W), mode='nearest').squeeze(0).squeeze(1)
        out[f"resize/{rH}x{rW}_{H}x{W}/image"] = a.numpy()
        out[f"resize/{rH}x{rW}_{H}x{W}/depth"] = b.numpy().reshape(H, W)
    out["resize/cases"] = np.array(json.dumps(RESIZES))

    # ---- NeRFGUI.prepare_buffer and the spp update of NeRFGUI.test_step
    H, W = 33, 65
    image, depth = (t.numpy() for t in frames[H, W])
    depths = {"plain": depth, "constant": np.full((H, W), 1.25, np.float32), "nan": depth.copy()}
    depths["nan"][7, 11] = np.nan
    for dname, d in depths.items():
        out[f"buffer/depth_{dname}/depth"] = d
    nxt = {"image": rand_image(g, H, W).numpy(), "depth": (0.3 + 2.0 * torch.rand(H, W, generator=g)).numpy()}
    out["buffer/next_image"], out["buffer/next_depth"] = nxt["image"], nxt["depth"]
    for mode, dname in [("image", "plain"), ("depth", "plain"), ("depth", "constant"), ("depth", "nan")]:
        outputs = {"image": image, "depth": depths[dname]}
        st = gui_stub(gui, mode, outputs)
        gui.NeRFGUI.test_step(st)                         # need_update: the buffer is written
        assert st.spp == 1 and not st.need_update
        out[f"buffer/{mode}_{dname}/spp0"] = np.asarray(st.render_buffer).reshape(H, W, 3)
        if dname != "plain":
            continue
        # each update starts from the buffer recorded before it: spp0 -> spp1 -> spp5
        for spp in SPPS[1:]:
            st.spp = spp
            st.trainer = types.SimpleNamespace(test_gui=lambda *a, **k: nxt)
            gui.NeRFGUI.test_step(st)
            assert st.spp == spp + 1 and st.render_buffer.dtype == np.float32
            out[f"buffer/{mode}_{dname}/spp{spp}"] = np.asarray(st.render_buffer).reshape(H, W, 3)

    path = os.path.join(make_golden.GOLDEN, "present.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print("wrote", path, size, "bytes")
    assert size < (1 << 20), "over the size limit for a committed file"


if __name__ == "__main__":
    main()
