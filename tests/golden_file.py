"""The loader of a tests/golden/<name>.npz, shared by the *_fixtures modules:
the file is read once, and its arrays are handed out as fresh copies, so no
test changes what another reads."""
import functools
import os
import types

import numpy as np
import torch

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def same(a, b):
    """Bit for bit, NaN equal to NaN."""
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    b = b.detach().cpu().numpy() if torch.is_tensor(b) else np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def loader(name):
    """path, _file() (cached {key: array}), arr (a copy), t (a fresh tensor), has, same."""
    path = os.path.join(GOLDEN_DIR, name)

    @functools.lru_cache(maxsize=None)
    def _file():
        with np.load(path) as z:
            return {k: z[k] for k in z.files}

    def arr(key):
        return _file()[key].copy()

    def has(key):
        return key in _file()

    def t(key):
        return torch.from_numpy(arr(key))

    return types.SimpleNamespace(path=path, _file=_file, arr=arr, has=has, t=t, same=same)
