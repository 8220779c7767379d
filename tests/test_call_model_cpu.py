"""The per-call model struct of the fused renderer, without a GPU: call_model's
copy of a base struct, resolve_perturb's normalisation, rgb_grads_struct and
the packed-weight key (samnerf_amd/fused.py)."""
import ctypes

import numpy as np
import pytest
import torch

from samnerf_amd._lib import SamnerfModel
from samnerf_amd.fused import (PhiloxPerturb, call_model, pack_key, perturbed_positions, resolve_perturb,
                               rgb_grads_struct)

STEPS = (128, 64, 32)
PER_CALL = ("view_width", "with_mask", "perturb", "reuse_packed", "perturb_device", "perturb_seed",
            "perturb_offset")


def _base():
    """A hand-built base struct: by-value fields, fake pointers, a keep list."""
    m = SamnerfModel()
    offs = np.arange(17, dtype=np.int32)
    m.keep = [offs]
    m.grid.embeddings = 0x1000
    m.grid.offsets_host = offs.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    m.grid.num_levels, m.grid.level_dim = 16, 2
    for i in range(3):
        m.grid_mlp[i] = 0x2000 + 16 * i
        m.num_steps[i] = STEPS[i]
    for i, v in enumerate((-1.0, -2.0, -3.0, 1.0, 2.0, 3.0)):
        m.aabb[i] = v
    m.with_sam, m.head_mode, m.t_thresh, m.mask_out = 1, 1, 0.25, 7
    m.sam_w[4] = 0x3000
    return m


def _outside(m):
    """The struct's bytes with the per-call fields blanked."""
    b = bytearray(bytes(m))
    for name in PER_CALL:
        f = getattr(SamnerfModel, name)
        b[f.offset:f.offset + f.size] = bytes(f.size)
    return bytes(b)


def _arrays(N=5, dtype=torch.float32):
    return tuple(torch.rand(N, T + 1).to(dtype) for T in STEPS)


def test_per_call_fields_do_not_overlap():
    """_outside blanks whole fields: the names exist and do not overlap."""
    spans = sorted((getattr(SamnerfModel, n).offset, getattr(SamnerfModel, n).size) for n in PER_CALL)
    assert all(a + s <= b for (a, s), (b, _) in zip(spans, spans[1:]))


def test_copy_keeps_the_base_and_sets_the_call_fields():
    base = _base()
    before = bytes(base)
    m = call_model(base, view_width=8, with_mask=2, reuse_packed=1)
    assert _outside(m) == _outside(base) == before          # the base's per-call fields are zero
    assert (m.view_width, m.with_mask, m.reuse_packed) == (8, 2, 1)
    assert (m.perturb_device, m.perturb_seed, m.perturb_offset) == (0, 0, 0)
    assert [m.perturb[i] for i in range(3)] == [None] * 3
    assert m.keep == base.keep and m.keep is not base.keep and m.keep[0] is base.keep[0]
    # writing to the copy leaves the base alone
    m.view_width, m.with_mask, m.reuse_packed, m.perturb_device, m.head_mode = 64, 1, 0, 1, 0
    m.aabb[0] = 9.0
    m.keep.append("x")
    assert bytes(base) == before and len(base.keep) == 1
    # the defaults: a plain copy
    d = call_model(base)
    assert bytes(d) == before
    assert call_model(base, view_width=None).view_width == 0


def test_copy_with_a_philox_source():
    base = _base()
    before = bytes(base)
    m = call_model(base, perturb=PhiloxPerturb(2 ** 64 - 1, 2 ** 32 + 5))
    assert (m.perturb_device, m.perturb_seed, m.perturb_offset) == (1, 2 ** 64 - 1, 2 ** 32 + 5)
    assert [m.perturb[i] for i in range(3)] == [None] * 3
    assert _outside(m) == before and bytes(base) == before and m.keep == base.keep


def test_copy_with_arrays():
    base = _base()
    before = bytes(base)
    arrays = _arrays()
    m = call_model(base, view_width=16, perturb=arrays)
    assert [m.perturb[i] for i in range(3)] == [t.data_ptr() for t in arrays]
    assert (m.perturb_device, m.perturb_seed, m.perturb_offset) == (0, 0, 0)
    assert m.keep[0] is base.keep[0] and all(a is b for a, b in zip(m.keep[1:], arrays)) and len(m.keep) == 4
    assert _outside(m) == before and bytes(base) == before and len(base.keep) == 1
    with pytest.raises(RuntimeError, match=r"perturb\[1\]"):
        call_model(base, perturb=(arrays[0], arrays[1].t().contiguous().t(), arrays[2]))
    with pytest.raises(RuntimeError, match=r"perturb\[0\]"):
        call_model(base, perturb=_arrays(dtype=torch.float64))


def test_resolve_perturb_off_and_seeded():
    cpu = torch.device("cpu")
    for off in (False, 0, None):
        assert resolve_perturb(off, 5, STEPS, cpu) is None
    p = PhiloxPerturb(3, 4)
    assert resolve_perturb(p, 5, STEPS, cpu) is p


@pytest.mark.parametrize("on", [True, 4])
def test_resolve_perturb_draws_the_reference_positions(on):
    cpu = torch.device("cpu")
    torch.manual_seed(11)
    want = perturbed_positions(6, STEPS, cpu)
    torch.manual_seed(11)
    got = resolve_perturb(on, 6, STEPS, cpu)
    assert isinstance(got, tuple) and len(got) == 3
    for a, b, T in zip(got, want, STEPS):
        assert a.shape == (6, T + 1) and a.dtype == torch.float32 and a.is_contiguous()
        assert torch.equal(a, b)


@pytest.mark.parametrize("box", [tuple, list])
def test_resolve_perturb_passes_arrays_through(box):
    cpu = torch.device("cpu")
    arrays = _arrays(5)
    got = resolve_perturb(box(arrays), 5, STEPS, cpu)
    assert isinstance(got, tuple) and all(a.data_ptr() == b.data_ptr() for a, b in zip(got, arrays))
    # other dtypes and strides arrive as contiguous fp32 of the same values
    odd = (arrays[0].double(), arrays[1].t().contiguous().t(), arrays[2])
    got = resolve_perturb(box(odd), 5, STEPS, cpu)
    for a, b in zip(got, arrays):
        assert a.dtype == torch.float32 and a.is_contiguous() and torch.equal(a, b)


def test_resolve_perturb_rejects_wrong_arrays():
    cpu = torch.device("cpu")
    arrays = _arrays(5)
    shapes = r"\[\(5, 129\), \(5, 65\), \(5, 33\)\]"
    bad = [arrays[:2], arrays + (arrays[2],), (), (arrays[0], arrays[2], arrays[1]),
           (arrays[0][:4], arrays[1], arrays[2]), (arrays[0], arrays[1], arrays[2][:, :32]),
           (arrays[0].reshape(-1), arrays[1], arrays[2])]
    for b in bad:
        with pytest.raises(ValueError, match=shapes):
            resolve_perturb(b, 5, STEPS, cpu)
    with pytest.raises(ValueError, match=r"\(4, 129\)"):
        resolve_perturb(arrays, 4, STEPS, cpu)              # the right arrays for another ray count


def test_rgb_grads_struct():
    tensors = [torch.zeros(3 + i) for i in range(13)]       # rgb_train_params order, 13 with the proposal nets
    ptr = [t.data_ptr() for t in tensors]
    g = rgb_grads_struct(tensors, True)
    assert g.grid == ptr[0]
    assert [g.grid_mlp[i] for i in range(3)] == ptr[1:4]
    assert [g.view_mlp[i] for i in range(3)] == ptr[4:7]
    assert [g.prop[i] for i in range(2)] == ptr[7:9]
    assert [g.prop_mlp[q][i] for q in range(2) for i in range(2)] == ptr[9:13]
    assert len(set(ptr)) == 13
    for ts in (tensors, tensors[:7]):
        g = rgb_grads_struct(ts, False)
        assert g.grid == ptr[0] and [g.grid_mlp[i] for i in range(3)] == ptr[1:4]
        assert [g.view_mlp[i] for i in range(3)] == ptr[4:7]
        assert [g.prop[i] for i in range(2)] == [None, None]
        assert [g.prop_mlp[q][i] for q in range(2) for i in range(2)] == [None] * 4


def test_pack_key_names_the_packing_library():
    lib_a, lib_b = object(), object()
    m = _base()
    ws = torch.zeros(64, dtype=torch.uint8)
    ts = [torch.zeros(4, 4) for _ in range(3)]
    assert pack_key(lib_a, ws, m, ts) == pack_key(lib_a, ws, m, ts)
    assert pack_key(lib_a, ws, m, ts) != pack_key(lib_b, ws, m, ts)
    # and what it depended on before: the buffer, head_mode, the tensors' versions
    key = pack_key(lib_a, ws, m, ts)
    assert key != pack_key(lib_a, torch.zeros(64, dtype=torch.uint8), m, ts)
    assert key != pack_key(lib_a, ws, call_model(m), ts[:2] + [torch.zeros(4, 4)])
    other = call_model(m)
    other.head_mode = 0
    assert key != pack_key(lib_a, ws, other, ts)
    ts[1].add_(1.0)
    assert key != pack_key(lib_a, ws, m, ts)
