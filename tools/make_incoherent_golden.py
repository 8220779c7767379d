#!/usr/bin/env python3
"""Generate tests/golden/incoherent.npz from the REFERENCE's own incoherent-mask
code: get_incoherent_mask (nerf/utils.py:283-298), imported from the reference
tree, and the lines of render_mask (:1732-1737) and update_incoherent_mask
(:1766-1776) that need no model, restated literally.

Runs only where the reference tree exists (tools/make_golden.py's
install_reference), never in a test.  Recorded, on seeded inputs:

  * per mask case (n, h, w, sfact): the masks -- blobs of integer ids whose
    edges cross the kernel's tile borders, a few one-pixel specks, and in the
    64 x 64 case one all-zero and one all-one view -- and, with keep_size both
    ways, the float map in float32 and in float64 (the same function handed a
    tensor whose .float() is .double()) and the packed .to(torch.bool) of the
    float32 one.  At sizes sfact divides the two maps are equal, which the
    generator asserts; 7 x 9 and 33 x 65 are recorded for the mirror only:
    there the two may differ (the run prints on how many cells), the bool
    following the float32 map's rounding residue;
  * per K in {1, 2, 3, 5, 32}: logits [33 * 65, K] (multiples of 1/8, stored as
    int16 eighths), pred_mask in float32 and float64, and the argmax ids;
  * one update: three views of 8 x 8 logits at K = 3 through both restated
    blocks, the [3, 64] bool table.

The generator refuses to write unless, in float64, every pixel's
|p_last - sum of the others| is at least 1e-3 or it is an exact tie of two
equal logits at K = 2, with at least 5 % of the K = 2 pixels such ties, and the
float32 ids equal the float64 ones.  No pixel is then left out of any
comparison.

Only data goes into the file.

usage: PYTHONDONTWRITEBYTECODE=1 python tools/make_incoherent_golden.py
"""
import json
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import make_golden  # noqa: E402

TILE = 16                                     # SAMNERF_INCOHERENT_TILE
# (n, h, w, sfact); the two after 4 x 6 put halos across tile borders on both axes
MASK_CASES = [(3, 2, 2, 2), (3, 4, 6, 2), (3, 2 * TILE * 2 - 2, 2 * TILE * 2 + 2, 2),
              (3, 2 * TILE * 2 + 2, 2 * TILE * 2 + 4, 2), (5, 64, 64, 2), (3, 8, 12, 4), (3, 36, 68, 4)]
ODD_CASES = [(3, 7, 9, 2), (3, 33, 65, 2)]    # the mirror only
KS = [(1, 1), (2, 2), (3, 3), (5, 3), (32, 32)]          # (K, n_inst)
ROWS = 33 * 65
UPDATE = (3, 8, 3, 3)                         # views, S, K, n_inst


class AsDouble:
    """What get_incoherent_mask needs of its input, with .float() in float64."""

    def __init__(self, t):
        self.t, self.shape = t, t.shape

    def float(self):
        return self.t.double()


def make_masks(g, n, h, w, ids=6):
    m = torch.zeros(n, h, w, dtype=torch.int64)
    yy, xx = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    for v in range(n):
        for _ in range(2 + (h * w) // 200):
            cy, cx = (torch.rand(2, generator=g) * torch.tensor([h, w])).tolist()
            r = 1 + float(torch.rand(1, generator=g)) * max(h, w) / 3
            ident = int(torch.randint(0, ids, (1,), generator=g))
            if float(torch.rand(1, generator=g)) < 0.5:
                m[v][(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = ident
            else:
                m[v][((yy - cy).abs() <= r) & ((xx - cx).abs() <= r / 2)] = ident
        for _ in range(min(4, h * w // 8)):   # one-pixel specks
            y, x = int(torch.randint(0, h, (1,), generator=g)), int(torch.randint(0, w, (1,), generator=g))
            m[v, y, x] = int(torch.randint(1, ids, (1,), generator=g))
    return m


def make_logits(g, rows, K):
    z = torch.round(2.0 * torch.randn(rows, K, generator=g) * 8) / 8
    if K == 1:
        return z
    # the last column against all the others: lift it to about even odds
    z[:, -1] += round(float(np.log(K - 1)) * 8) / 8
    if K == 2:
        tie = torch.rand(rows, generator=g) < 0.12
        z[tie, 1] = z[tie, 0]
    # a pixel too close to call moves half a logit away
    for _ in range(8):
        p = torch.softmax(z.double(), -1)
        gap = (p[:, -1] - p[:, :-1].sum(-1)).abs()
        near = (gap < 1e-3) & ~((z[:, 0] == z[:, -1]) if K == 2 else torch.zeros(rows, dtype=torch.bool))
        if not bool(near.any()):
            break
        z[near, -1] += 0.5
    return z


def check_logits(z):
    """The refusal rule of the docstring; returns the share of exact ties."""
    K = z.shape[-1]
    if K == 1:
        return 0.0
    p = torch.softmax(z.double(), -1)
    gap = (p[:, -1] - p[:, :-1].sum(-1)).abs()
    tie = (z[:, 0] == z[:, 1]) if K == 2 else torch.zeros(z.shape[0], dtype=torch.bool)
    assert bool(((gap >= 1e-3) | tie).all()), "a pixel closer than 1e-3 that is not a tie of equal logits"
    assert bool((gap[tie] == 0).all()), "equal logits whose float64 probabilities differ"
    if K == 2:
        assert float(tie.double().mean()) >= 0.05, "fewer than 5 % ties at K = 2"
    return float(tie.double().mean())


def render_mask_lines(inst_mask, n_inst):
    """utils.py:1732-1737 with opt.n_inst as an argument."""
    if n_inst > 1:
        inst_mask = torch.softmax(inst_mask, dim=-1)
        pred_mask = torch.stack([inst_mask[..., :-1].sum(-1), inst_mask[..., -1]], -1)
    else:
        pred_mask = torch.sigmoid(inst_mask)
    return pred_mask


def update_lines(utils, rendered_mask_list, incoherent_mask_size):
    """utils.py:1766-1776 without the np.save of :1772."""
    rendered_masks_softmax = torch.stack(rendered_mask_list, 0).detach()
    rendered_masks = rendered_masks_softmax.argmax(-1)[:, None, ...]
    incoherent_masks = utils.get_incoherent_mask(rendered_masks, sfact=2)
    incoherent_masks = incoherent_masks.to(torch.bool)[:, None, ...]
    incoherent_masks = incoherent_masks.view(-1, incoherent_mask_size * incoherent_mask_size)
    return rendered_masks, incoherent_masks


def main():
    _, _, utils = make_golden.install_reference()
    out = {}
    g = torch.Generator().manual_seed(31)

    for ci, (n, h, w, sfact) in enumerate(MASK_CASES + ODD_CASES):
        odd = ci >= len(MASK_CASES)
        masks = make_masks(g, n, h, w)
        if (h, w) == (64, 64):
            masks[3] = 0
            masks[4] = 1
        assert int(masks.max()) < 256                     # the uint8 form of the tests
        name = f"masks/{ci}"
        out[f"{name}/masks"] = masks.numpy().astype(np.uint8)
        for keep in (True, False):
            u32 = utils.get_incoherent_mask(masks[:, None], sfact=sfact, keep_size=keep)
            u64 = utils.get_incoherent_mask(AsDouble(masks[:, None]), sfact=sfact, keep_size=keep)
            assert u32.dtype == torch.float32 and u64.dtype == torch.float64
            assert odd or bool((u32.double() == u64).all()), (name, "the float32 and float64 chains differ")
            k = f"{name}/keep{int(keep)}"
            out[f"{k}/u32"], out[f"{k}/u64"] = u32.numpy(), u64.numpy()
            b = u32.to(torch.bool)
            out[f"{k}/bool_packed"] = np.packbits(b.numpy().reshape(-1))
            print(name, (n, h, w, sfact), f"keep_size={keep}: {float(b.float().mean()):.3f} True,",
                  f"{int(((u32 != 0) & (u32 < 0.01)).sum())} non-zero cells below 0.01,",
                  f"{int((u32.double() != u64).sum())} cells where float32 and float64 differ")
    out["masks/cases"] = np.array(json.dumps(MASK_CASES))
    out["masks/odd_cases"] = np.array(json.dumps(ODD_CASES))

    for K, n_inst in KS:
        z = make_logits(g, ROWS, K)
        ties = check_logits(z)
        z8 = torch.round(z * 8)
        assert bool((z8 / 8 == z).all()) and float(z8.abs().max()) < 2 ** 15
        p32, p64 = render_mask_lines(z.clone(), n_inst), render_mask_lines(z.double(), n_inst)
        ids = p32.argmax(-1)
        assert torch.equal(ids, p64.argmax(-1)), "the float32 and float64 ids differ"
        if K == 2:
            assert not bool(ids[z[:, 0] == z[:, 1]].any()), "a tie must give 0"
        out[f"logits/{K}/z8"] = z8.numpy().astype(np.int16)
        out[f"logits/{K}/pred32"], out[f"logits/{K}/pred64"] = p32.numpy(), p64.numpy()
        out[f"logits/{K}/ids"] = ids.numpy().astype(np.uint8)
        print(f"logits K={K} n_inst={n_inst}: ties {ties:.3f}, ids==1 {float(ids.float().mean()):.3f}")
    out["logits/cases"] = np.array(json.dumps(KS))

    views, S, K, n_inst = UPDATE
    z = make_logits(g, views * S * S, K)
    check_logits(z)
    rendered = [render_mask_lines(z[v * S * S:(v + 1) * S * S].reshape(S, S, K), n_inst) for v in range(views)]
    ids, table = update_lines(utils, rendered, S)
    assert table.dtype == torch.bool and tuple(table.shape) == (views, S * S) and bool(table.any())
    out["update/z8"] = torch.round(z * 8).numpy().astype(np.int16)
    out["update/ids"] = ids.numpy().astype(np.uint8)
    out["update/table_packed"] = np.packbits(table.numpy().reshape(-1))
    out["update/case"] = np.array(json.dumps(UPDATE))

    path = os.path.join(make_golden.GOLDEN, "incoherent.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print("wrote", path, size, "bytes")
    largest = max(os.path.getsize(os.path.join(make_golden.GOLDEN, f)) for f in os.listdir(make_golden.GOLDEN)
                  if f.endswith(".npz") and f != "incoherent.npz")
    assert size < (1 << 20) and size <= largest, "larger than the goldens already present"


if __name__ == "__main__":
    main()
