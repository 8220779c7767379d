"""The seeded source of perturb=True (samnerf_model.perturb_device,
fused.PhiloxPerturb), without a GPU: the numpy restatement of the contract
(tests/philox_ref.py) against the published known answers of Philox4x32-10,
the library's host entry point (samnerf_perturb_host, compiled from the header
the kernels use) against that restatement bit for bit, the properties the
kernels rely on, and the argument check."""
import ctypes
import itertools

import numpy as np
import pytest

import philox_ref

STEPS = (128, 64, 32)
SEEDS = (0, 0x0123456789ABCDEF, 2 ** 64 - 1)
OFFSETS = (0, 1, 2 ** 32 + 5)
RAYS = (0, 1, 66, 2 ** 32 - 1)


@pytest.mark.parametrize("counter,key,want", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     "d16cfe09 94fdcceb 5001e420 24126ea1")])
def test_reference_generator_known_answers(counter, key, want):
    got = philox_ref.philox4x32_10(counter, key)
    assert " ".join(f"{int(v):08x}" for v in got) == want


@pytest.mark.parametrize("stage", [0, 1, 2])
def test_perturb_host_equals_the_contract_bit_for_bit(hip_lib, stage):
    from samnerf_amd.fused import perturb_host
    for seed, offset in itertools.product(SEEDS, OFFSETS):
        want = philox_ref.positions(seed, offset, STEPS, stage, RAYS)
        for i, ray in enumerate(RAYS):
            got = perturb_host(seed, offset, STEPS, stage, ray)
            assert got.dtype == np.float32 and got.shape == (STEPS[stage] + 1,)
            assert np.array_equal(got.view(np.uint32), want[i].view(np.uint32)), (seed, offset, ray)


def test_perturb_host_rejects_bad_arguments(hip_lib):
    steps = (ctypes.c_uint32 * 3)(*STEPS)
    out = (ctypes.c_float * 129)()
    L = hip_lib
    assert L.samnerf_perturb_host(1, 0, steps, 3, 0, out) == -1 and b"stage" in L.samnerf_last_error()
    assert L.samnerf_perturb_host(1, 0, None, 0, 0, out) == -1
    assert L.samnerf_perturb_host(1, 0, steps, 0, 0, None) == -1
    bad = (ctypes.c_uint32 * 3)(128, 0, 32)
    assert L.samnerf_perturb_host(1, 0, bad, 0, 0, out) == -1 and b"num_steps" in L.samnerf_last_error()
    assert L.samnerf_perturb_host(1, 0, steps, 0, 0, out) == 0


def test_positions_are_valid_sample_positions():
    """What the kernels rely on, for 256 rays: bins inside [0, 1], u inside
    [0, 1] and nondecreasing up to rounding (the bound tests/test_perturb.py
    holds torch's draws to)."""
    bins0, u1, u2 = philox_ref.all_positions(0x5EED5EED12345678, 3, STEPS, 256)
    assert bins0.shape == (256, 129) and u1.shape == (256, 65) and u2.shape == (256, 33)
    assert bins0.min() >= 0 and bins0.max() <= 1
    for u in (u1, u2):
        assert u.min() >= 0 and u.max() <= 1
        assert (u[:, 1:] - u[:, :-1]).min() > -1e-6
    # the jitter spans its bin: a draw that ignored the generator would not
    jit = (bins0[:, 1:-1] - philox_ref.lin(STEPS, 0)[None, 1:-1]) * STEPS[0]
    assert jit.min() < -0.49 and jit.max() > 0.49 and abs(float(jit.mean())) < 0.01


def test_every_counter_field_changes_the_values():
    base = dict(seed=0x0123456789ABCDEF, offset=7, stage=1, ray=66)

    def draw(**kw):
        a = {**base, **kw}
        return philox_ref.words(a["seed"], a["offset"], a["stage"], [a["ray"]], 33)[0]

    ref = draw()
    # each half of the seed and of the offset, the stage and the ray
    for change in (dict(seed=base["seed"] ^ 1), dict(seed=base["seed"] ^ 1 << 32), dict(offset=8),
                   dict(offset=7 + (1 << 32)), dict(stage=2), dict(stage=0), dict(ray=67), dict(ray=2)):
        other = draw(**change)
        assert (other != ref).mean() > 0.9, change
    # and through the library: stage 1 against stage 2 over their common length, ray against ray
    from samnerf_amd.fused import perturb_host
    a = perturb_host(base["seed"], 7, STEPS, 0, 66)
    for b in (perturb_host(base["seed"] + 1, 7, STEPS, 0, 66), perturb_host(base["seed"], 8, STEPS, 0, 66),
              perturb_host(base["seed"], 7, STEPS, 0, 67)):
        assert (a[1:-1] != b[1:-1]).mean() > 0.9


def _model(arrays, device=1):
    from samnerf_amd._lib import SamnerfModel
    m = SamnerfModel()
    for i, v in enumerate(STEPS):
        m.num_steps[i] = v
    m.perturb_device = device
    m.perturb_seed = 2 ** 64 - 1
    m.perturb_offset = 2 ** 32 + 5
    for i in arrays:
        m.perturb[i] = 64
    return m


def test_model_struct_keeps_the_new_fields_last():
    """Appended: every earlier field keeps its offset."""
    from samnerf_amd._lib import SamnerfModel
    names = [f[0] for f in SamnerfModel._fields_]
    assert names[-3:] == ["perturb_device", "perturb_seed", "perturb_offset"]
    assert names[-4] == "reuse_packed"
    m = _model(())
    assert (m.perturb_seed, m.perturb_offset) == (2 ** 64 - 1, 2 ** 32 + 5)


@pytest.mark.parametrize("arrays", [(0, 1, 2), (1,)])
def test_perturb_device_with_arrays_is_einval(hip_lib, arrays):
    """The argument check of every entry point that takes perturb arrays,
    reached before any GPU call (tests/test_capi.py's pattern: the pointers
    are never dereferenced)."""
    from samnerf_amd._lib import SamnerfRgbGrads, SamnerfRgbTrainOpts
    L = hip_lib
    p = ctypes.c_void_p(64)
    m = ctypes.byref(_model(arrays))
    N, big = 4, 1 << 40
    opts, grads = SamnerfRgbTrainOpts(), SamnerfRgbGrads()
    calls = {
        "render": lambda: L.samnerf_render_forward(m, p, p, N, None, 0, 1.0, p, p, p, None, None, p, big, None),
        "render_tile": lambda: L.samnerf_render_forward_tile(m, p, p, N, None, 0, 1.0, p, 5, 0, None, p, big, None),
        "rgb_train_forward": lambda: L.samnerf_rgb_train_forward(m, p, p, N, None, 0, 1.0, 1, p, p, p, p, p, p,
                                                                 big, None),
        "rgb_train_backward": lambda: L.samnerf_rgb_train_backward(m, p, p, N, 1.0, 1, p, None, None, None, p,
                                                                   ctypes.byref(grads), p, big, None),
        "rgb_train_step": lambda: L.samnerf_rgb_train_step(m, p, p, N, None, 0, p, ctypes.byref(opts), p, p, p, p,
                                                           ctypes.byref(grads), p, big, None),
    }
    for name, call in calls.items():
        assert call() == -1, name
        msg = L.samnerf_last_error()
        assert b"perturb" in msg, (name, msg)
        if len(arrays) == 3:
            assert b"perturb_device" in msg, (name, msg)


def test_philox_perturb_value_type():
    from samnerf_amd.fused import PhiloxPerturb
    p = PhiloxPerturb(5)
    assert (p.seed, p.offset) == (5, 0) and p == PhiloxPerturb(5, 0)
    assert not isinstance(p, (tuple, list))            # never mistaken for the three arrays
    for bad in (dict(seed=-1), dict(seed=1 << 64), dict(seed=1, offset=-1), dict(seed=1.5)):
        with pytest.raises(ValueError):
            PhiloxPerturb(**bad)
