"""--background white / random and RGB background colours, the parts that need
no GPU: the CPU mirror (run_torch on the oracle encoders) reproduces the
reference's fixtures bit for bit, the C ABI validates the per-thread background
setting (samnerf_set_background) before any GPU call, and the bg_color
normalisation of the fused paths as a pure function of shapes."""
import ctypes
import os

import numpy as np
import pytest
import torch

from background_fixtures import NAMES, OUT_KEYS, run_mirror
from conftest import GOLDEN


@pytest.mark.parametrize("name", NAMES)
def test_mirror_reproduces_reference_background_fixture(oracle_lib, name):
    """The yardstick of the GPU tests: the mirror's unfused path equals the
    reference's NeRFNetwork.run under 'white' (eval: RGB with a [3] colour,
    SAM features, the 'default' mask head) and 'random' (train mode, a colour
    per ray, with the render's losses)."""
    fx = np.load(os.path.join(GOLDEN, name + ".npz"))
    ws = fx["weights_sum"]
    # the clamp spreads the opacity, so the modes differ on these views
    assert ws.min() < 0.3 and ws.max() > 0.9 and ((ws > 0.3) & (ws < 0.9)).mean() >= 0.5
    out = run_mirror(fx)
    checked = 0
    for k in OUT_KEYS:
        if k in fx:
            a = out[k].detach().reshape(fx[k].shape).numpy()
            assert np.array_equal(a, fx[k]), (k, float(np.abs(a - fx[k]).max()))
            checked += 1
    assert checked >= 3


def _model():
    from samnerf_amd._lib import SamnerfModel
    m = SamnerfModel()
    for i, v in enumerate((128, 64, 32)):
        m.num_steps[i] = v
    return m


def _entry_points(L, m, N):
    """Every entry point that reads the background fields, with pointers that
    are never dereferenced (tests/test_capi.py's pattern): the argument checks
    run before any GPU call."""
    from samnerf_amd._lib import SamnerfRgbGrads, SamnerfRgbTrainOpts
    p = ctypes.c_void_p(64)
    mp = ctypes.byref(m)
    o, g = SamnerfRgbTrainOpts(), SamnerfRgbGrads()
    return {
        "render": lambda: L.samnerf_render_forward(mp, p, p, N, None, 0, 1.0, p, p, p, None, None, p, 1 << 40, None),
        "render_tile": lambda: L.samnerf_render_forward_tile(mp, p, p, N, None, 0, 1.0, p, 5, 0, None, p, 1 << 40,
                                                             None),
        "rgb_train_step": lambda: L.samnerf_rgb_train_step(mp, p, p, N, None, 0, p, ctypes.byref(o), p, p, p, p,
                                                           ctypes.byref(g), p, 1 << 40, None),
        "rgb_train_forward": lambda: L.samnerf_rgb_train_forward(mp, p, p, N, None, 0, 1.0, 1, p, p, p, p, p, p,
                                                                 1 << 40, None),
        "rgb_train_backward": lambda: L.samnerf_rgb_train_backward(mp, p, p, N, 1.0, 1, p, None, None, None, p,
                                                                   ctypes.byref(g), p, 1 << 40, None),
    }


def test_background_struct_mirrors_the_header():
    """samnerf_background {int background; const float* bg_rgb; uint32_t n_bg;}
    in the header's order; samnerf_model itself keeps its layout (the setting is
    per thread, like the parity taps)."""
    from samnerf_amd._lib import EXPORTED, SamnerfBackground, SamnerfModel
    assert [f[0] for f in SamnerfBackground._fields_] == ["background", "bg_rgb", "n_bg"]
    assert (SamnerfBackground.background.offset, SamnerfBackground.bg_rgb.offset, SamnerfBackground.n_bg.offset) \
        == (0, 8, 16)
    b = SamnerfBackground()
    assert (b.background, b.bg_rgb, b.n_bg) == (0, None, 0)      # the default: 'last_sample', scalar colour
    assert "samnerf_set_background" in EXPORTED
    assert [f[0] for f in SamnerfModel._fields_][-1] == "perturb_offset"


@pytest.mark.parametrize("case,field", [("background2", b"background"), ("n_bg2", b"n_bg"),
                                        ("null_rows", b"bg_rgb")])
def test_background_argument_errors(hip_lib, case, field):
    """background outside {0, 1}; bg_rgb with n_bg = 2 for N = 4 rays; n_bg = 1
    with a null bg_rgb: SAMNERF_EINVAL (-1) with a message naming the field,
    from every entry point that reads the setting, before any GPU call."""
    from samnerf_amd._lib import SamnerfBackground
    L = hip_lib
    m = _model()
    b = SamnerfBackground()
    if case == "background2":
        b.background = 2
    elif case == "n_bg2":
        b.bg_rgb, b.n_bg = 64, 2
    else:
        b.bg_rgb, b.n_bg = None, 1
    calls = _entry_points(L, m, 4)
    try:
        assert L.samnerf_set_background(ctypes.byref(b)) == 0
        for what, call in calls.items():
            assert call() == -1, what
            msg = L.samnerf_last_error()
            assert field in msg, (what, msg)
    finally:
        assert L.samnerf_set_background(None) == 0


def test_bg_layout_is_a_pure_function_of_shapes():
    """(scalar, n_bg) of every bg_color shape the reference passes: n_bg 0 =
    the scalar argument, 1 = one colour, N = a colour per ray."""
    from samnerf_amd.fused import background_rows, bg_layout
    N = 5
    assert bg_layout(None, N) == (1.0, 0)
    assert bg_layout(1, N) == (1.0, 0)
    s, n = bg_layout(torch.tensor(0.3), N)
    assert (s, n) == (float(torch.tensor(0.3)), 0)
    assert bg_layout(torch.tensor([0.25]), N) == (0.25, 0)
    assert bg_layout(torch.ones(3), N) == (None, 1)
    assert bg_layout(torch.ones(1, 3), N) == (None, 1)
    assert bg_layout(torch.ones(N, 3), N) == (None, N)
    assert bg_layout(torch.ones(N, 1), N) == (None, N)
    # three rays: [3] is still one colour (it broadcasts along the channels), [3,1] and [3,3] are per ray
    assert bg_layout(torch.ones(3), 3) == (None, 1)
    assert bg_layout(torch.ones(3, 1), 3) == (None, 3)
    assert bg_layout(torch.ones(3, 3), 3) == (None, 3)
    for bad in (torch.ones(2, 3), torch.ones(N, 2), torch.ones(N + 1, 3), torch.ones(2, N, 3)):
        with pytest.raises(ValueError, match="does not broadcast"):
            bg_layout(bad, N)
    # the rows the kernels read: contiguous float32 [n_bg, 3], broadcast along the channels
    sc, rows = background_rows(torch.tensor([[0.1], [0.2], [0.3], [0.4], [0.5]], dtype=torch.float64), N, "cpu")
    assert sc == 1.0 and rows.shape == (N, 3) and rows.dtype == torch.float32 and rows.is_contiguous()
    assert torch.equal(rows[:, 0], rows[:, 2]) and rows[3, 1] == np.float32(0.4)
    sc, rows = background_rows(torch.tensor([0.2, 0.5, 0.9]), N, "cpu")
    assert rows.shape == (1, 3) and torch.equal(rows[0], torch.tensor([0.2, 0.5, 0.9]))
    assert background_rows(0.5, N, "cpu") == (0.5, None)


def test_dispatch_conditions_accept_the_background_modes():
    """NeRFRenderer's fused conditions no longer look at opt.background; a
    colour that requires grad, or one that does not broadcast, is not a fused
    case."""
    from nerf.renderer import NeRFRenderer
    ok = NeRFRenderer._fused_bg_ok
    N = 4
    assert ok(None, N) and ok(1, N) and ok(torch.ones(3), N) and ok(torch.ones(N, 3), N) and ok(torch.ones(N, 1), N)
    assert not ok(torch.ones(2, 3), N)
    assert not ok(torch.ones(3, requires_grad=True), N)
