"""tests/golden/incoherent.npz (tools/make_incoherent_golden.py): the reference's
own get_incoherent_mask and its render_mask / update_incoherent_mask lines,
recorded.  Loaded once and shared; the arrays are handed out as fresh tensors,
so no test changes what another reads."""
import json

import numpy as np
import torch

import golden_file

_G = golden_file.loader("incoherent.npz")
GOLDEN, _file, arr, t, has, same = _G.path, _G._file, _G.arr, _G.t, _G.has, _G.same
TILE = 16                                     # SAMNERF_INCOHERENT_TILE


def mask_cases():
    """[(index, n, h, w, sfact)] of the sizes sfact divides."""
    return [(i, *c) for i, c in enumerate(json.loads(str(_file()["masks/cases"])))]


def odd_cases():
    """[(index, n, h, w, sfact)] of the sizes it does not: the mirror's only."""
    first = len(mask_cases())
    return [(first + i, *c) for i, c in enumerate(json.loads(str(_file()["masks/odd_cases"])))]


def masks(ci, dtype=torch.int64):
    """[n, h, w] ids."""
    return t(f"masks/{ci}/masks").to(dtype)


def cells(h, w, sfact, keep):
    return (h, w) if keep else (h // sfact, w // sfact)


def want_bool(ci, n, h, w, sfact, keep):
    """The reference's .to(torch.bool) of its float32 map, [n, cells]."""
    ch, cw = cells(h, w, sfact, keep)
    bits = np.unpackbits(arr(f"masks/{ci}/keep{int(keep)}/bool_packed"))[:n * ch * cw]
    return torch.from_numpy(bits.astype(bool)).view(n, ch * cw)


def want_map(ci, keep, double=False):
    """The reference's float map [n, 1, ch, cw], float32 or float64."""
    return t(f"masks/{ci}/keep{int(keep)}/u{64 if double else 32}")


def logit_cases():
    """[(K, n_inst)]"""
    return [tuple(c) for c in json.loads(str(_file()["logits/cases"]))]


def logits(K):
    return t(f"logits/{K}/z8").float() / 8


def update_case():
    """(views, S, K, n_inst, logits [views * S * S, K], ids [views, 1, S, S] uint8, table [views, S * S] bool)"""
    views, S, K, n_inst = json.loads(str(_file()["update/case"]))
    bits = np.unpackbits(arr("update/table_packed"))[:views * S * S]
    return views, S, K, n_inst, t("update/z8").float() / 8, t("update/ids"), \
        torch.from_numpy(bits.astype(bool)).view(views, S * S)
