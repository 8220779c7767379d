"""The teacher image without a GPU: the numpy restatement (tests/teacher_ref.py)
against PIL itself and against PIL's recorded outputs, preprocess_shape, the
torch mirror, set_image_from_render on a stub predictor, the feature cache and
its policy, and the C ABI's host entry points and argument errors."""
import ctypes
import types

import numpy as np
import pytest
import torch

import teacher_fixtures as fx
import teacher_ref as ref


# ---------------------------------------------------------- the restatement --

@pytest.mark.parametrize("src,dst", ref.PIL_SHAPES)
def test_restatement_equals_pil_bit_for_bit(src, dst):
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(src[0] * 10007 + dst[1])
    img = rng.integers(0, 256, src + (3,), dtype=np.uint8)
    want = np.asarray(Image.fromarray(img).resize((dst[1], dst[0]), Image.BILINEAR))
    got = ref.resize_u8(img, *dst)
    assert got.shape == want.shape and int((got != want).sum()) == 0


@pytest.mark.parametrize("i", [0, 1])
def test_restatement_equals_the_recorded_pil_outputs(i):
    img, want = fx.golden.arr(f"in{i}"), fx.golden.arr(f"out{i}")
    assert fx.golden.same(ref.resize_u8(img, *want.shape[:2]), want)


def test_an_unchanged_axis_passes_through():
    img = np.random.default_rng(3).integers(0, 256, (9, 9, 3), dtype=np.uint8)
    assert np.array_equal(ref.resize_u8(img, 9, 9), img)
    for xx, (xmin, k) in enumerate(ref.coefficients(9, 9)):
        assert [(1 << 22) if xmin + j == xx else 0 for j in range(len(k))] == k


def test_quantise_is_numpys():
    v = np.concatenate([ref.edge_values(), np.random.default_rng(1).random(1000, dtype=np.float32)])
    assert np.array_equal(ref.quantise(v), (v * 255).astype(np.uint8))
    assert ref.quantise(np.float32(1.0)) == 255 and ref.quantise(np.float32(0.0)) == 0


# -------------------------------------------------------------------- shapes --

SHAPES = [((512, 512), (1024, 1024)), ((480, 640), (768, 1024)), ((37, 53), (715, 1024)),
          ((1200, 900), (1024, 768)), ((1, 1), (1024, 1024))]


@pytest.mark.parametrize("src,dst", SHAPES)
def test_preprocess_shape(src, dst):
    from samnerf_amd.teacher import preprocess_shape
    assert preprocess_shape(*src) == dst == ref.preprocess_shape(*src)
    assert preprocess_shape(5, 7, target=23) == (16, 23) and preprocess_shape(100, 75, 64) == (64, 48)


# ---------------------------------------------------------- the torch mirror --

@pytest.mark.parametrize("H,W,target,size", [(5, 7, 23, 32), (100, 75, 64, None), (9, 9, 20, None), (7, 5, 3, 4)])
def test_torch_teacher_image_equals_the_restatement(H, W, target, size):
    pytest.importorskip("PIL")
    from samnerf_amd.teacher import preprocess_shape, teacher_image, torch_teacher_image
    rgb = torch.rand(H, W, 3, generator=torch.Generator().manual_seed(H * W))
    edges = torch.from_numpy(ref.edge_values())
    n = min(rgb.numel(), edges.numel())
    rgb.view(-1)[:n] = edges[:n]
    oh, ow = preprocess_shape(H, W, target)
    S = size or target
    for mean, std in ((ref.PIXEL_MEAN, ref.PIXEL_STD), ((100.0, 110.5, 120.25), (50.0, 60.5, 70.125))):
        want_u8, want_in = ref.teacher_image(rgb.numpy(), oh, ow, S, mean, std)
        got = torch_teacher_image(rgb, target=target, size=size, pixel_mean=mean, pixel_std=std)
        assert got["input_size"] == (oh, ow)
        assert fx.golden.same(got["u8"], want_u8)
        assert got["input"].shape == (1, 3, S, S) and fx.golden.same(got["input"][0], want_in)
        pad = np.concatenate([got["input"][0, :, oh:, :].numpy().ravel(), got["input"][0, :, :, ow:].numpy().ravel()])
        assert not pad.any() and not np.signbit(pad).any()
    # a CPU tensor takes the mirror; want= selects
    only = teacher_image(rgb, target=target, size=size, want=("u8",))
    assert sorted(only) == ["input_size", "u8"] and fx.golden.same(only["u8"], ref.teacher_image(rgb.numpy(), oh, ow, S)[0])
    with pytest.raises(ValueError, match="below"):
        torch_teacher_image(rgb, target=target, size=max(oh, ow) - 1)
    with pytest.raises(ValueError, match="want"):
        torch_teacher_image(rgb, target=target, want=("features",))


@pytest.mark.parametrize("i,target", fx.GOLDEN_CASES)
def test_torch_teacher_image_on_the_recorded_inputs(i, target):
    pytest.importorskip("PIL")
    from samnerf_amd.teacher import torch_teacher_image
    got = torch_teacher_image(fx.render_of(fx.golden.arr(f"in{i}")), target=target)
    assert fx.golden.same(got["u8"], fx.golden.arr(f"out{i}"))


# ------------------------------------------------------- set_image_from_render --

@pytest.mark.parametrize("tuple_out", [False, True])
def test_set_image_from_render_sets_the_predictor_state_in_order(tuple_out):
    pytest.importorskip("PIL")
    from samnerf_amd.teacher import set_image_from_render
    p = fx.StubPredictor(tuple_out=tuple_out)
    rgb = torch.rand(12, 20, 3, generator=torch.Generator().manual_seed(8))
    feats = set_image_from_render(p, rgb)
    names = ["features", "interm_features"] if tuple_out else ["features"]
    assert p.log == ["reset_image()", "original_size", "input_size"] + names + ["is_image_set"]
    assert p.original_size == (12, 20) and p.input_size == (614, 1024) == ref.preprocess_shape(12, 20)
    assert p.is_image_set is True and feats is p.features and feats.shape == (1, 256, 64, 64)
    enc = p.model.image_encoder
    assert len(enc.seen) == 1 and enc.seen[0].shape == (1, 3, 1024, 1024) and enc.seen[0].dtype == torch.float32
    _, want = ref.teacher_image(rgb.numpy(), 614, 1024, 1024)
    assert fx.golden.same(enc.seen[0][0], want)
    if tuple_out:
        assert isinstance(p.interm_features, list) and p.interm_features[0].shape == (1, 3, 64, 64)
    else:
        assert p.interm_features is None


def test_set_image_from_render_takes_the_models_own_buffers():
    pytest.importorskip("PIL")
    from samnerf_amd.teacher import set_image_from_render
    p = fx.StubPredictor(with_buffers=True)
    rgb = torch.rand(6, 4, 3, generator=torch.Generator().manual_seed(9))
    set_image_from_render(p, rgb)
    _, want = ref.teacher_image(rgb.numpy(), 1024, 683, 1024, (100.0, 110.0, 120.0), (50.0, 60.0, 70.0))
    assert fx.golden.same(p.model.image_encoder.seen[0][0], want)


# ----------------------------------------------------------- cache and policy --

def test_feature_cache_is_a_ring():
    from samnerf_amd.teacher import FeatureCache
    c = FeatureCache(3)
    for i in range(3):
        assert not c.full()
        c.insert({"i": i})
    assert c.full() and [c.get(k)["i"] for k in range(3)] == [0, 1, 2]
    c.insert({"i": 3})                                   # overwrites the oldest
    assert c.full() and [c.get(k)["i"] for k in range(3)] == [3, 1, 2]
    c.insert({"i": 4})
    assert [c.get(k)["i"] for k in range(3)] == [3, 4, 2]
    import random
    random.seed(11)
    want = [random.randint(0, 2) for _ in range(8)]
    random.seed(11)
    assert [c.get()["i"] for _ in range(8)] == [[3, 4, 2][k] for k in want]


def test_use_cache_now_truth_table():
    from samnerf_amd.teacher import FeatureCache, use_cache_now
    full, part = FeatureCache(2), FeatureCache(2)
    full.insert(1), full.insert(2), part.insert(1)
    for with_sam in (True, False):
        for cache_size in (0, 2):
            for cache, is_full in ((full, True), (part, False), (None, False)):
                for step in range(0, 9):
                    opt = types.SimpleNamespace(with_sam=with_sam, cache_size=cache_size, cache_interval=4)
                    want = with_sam and cache_size > 0 and is_full and step % 4 != 0
                    assert use_cache_now(opt, cache, step) is want, (with_sam, cache_size, is_full, step)


# ------------------------------------------------------------------- the ABI --

def test_shape_and_workspace_size(hip_lib):
    L = hip_lib
    oh, ow = ctypes.c_uint32(), ctypes.c_uint32()
    for src, dst in SHAPES + [((5, 7), (16, 23))]:
        target = 1024 if src != (5, 7) else 23
        assert L.samnerf_teacher_image_shape(src[0], src[1], target, ctypes.byref(oh), ctypes.byref(ow)) == 0
        assert (oh.value, ow.value) == dst
    assert L.samnerf_teacher_image_shape(0, 4, 1024, ctypes.byref(oh), ctypes.byref(ow)) == -1
    assert L.samnerf_teacher_image_shape(4, 8193, 1024, ctypes.byref(oh), ctypes.byref(ow)) == -1
    assert L.samnerf_teacher_image_shape(4, 4, 0, ctypes.byref(oh), ctypes.byref(ow)) == -1
    assert L.samnerf_teacher_image_shape(4, 4, 1024, None, ctypes.byref(ow)) == -1

    def size(H, W, oh, ow):
        up = lambda n: (n + 255) & ~255                                     # noqa: E731
        kx, ky = ref.taps_per_index(W, ow), ref.taps_per_index(H, oh)
        return up(8 * ow) + up(8 * oh) + up(4 * ow * kx) + up(4 * oh * ky) + up((H * ow * 3 + 3) // 4 * 4)
    for H, W, oh_, ow_ in [(512, 512, 1024, 1024), (5, 7, 16, 23), (100, 75, 64, 48), (7, 5, 3, 2), (8192, 1, 1, 8192)]:
        assert L.samnerf_teacher_image_workspace_size(H, W, oh_, ow_) == size(H, W, oh_, ow_)
    assert ref.taps_per_index(512, 1024) == 3 and ref.taps_per_index(100, 64) == 5 and ref.taps_per_index(7, 3) == 7
    for bad in [(0, 4, 4, 4), (4, 0, 4, 4), (4, 4, 0, 4), (4, 4, 4, 0), (8193, 4, 4, 4), (4, 4, 4, 8193)]:
        assert L.samnerf_teacher_image_workspace_size(*bad) == 0


def test_argument_errors_return_before_any_pointer_is_read(hip_lib):
    L = hip_lib
    p = ctypes.c_void_p(64)          # never dereferenced: validation fails first
    need = L.samnerf_teacher_image_workspace_size(5, 7, 16, 23)
    assert need > 0

    def call(rgb=p, H=5, W=7, oh=16, ow=23, S=32, u8=p, inp=p, ws=p, n=need):
        return L.samnerf_teacher_image(rgb, H, W, oh, ow, S, None, None, u8, inp, ws, n, None)
    assert call(rgb=None) == -1 and b"null rgb" in L.samnerf_last_error()
    assert call(u8=None, inp=None) == -1 and b"both null" in L.samnerf_last_error()
    assert call(S=22) == -1 and b"S = 22" in L.samnerf_last_error()
    assert call(S=8193) == -1
    assert call(S=0) == -1
    for k in ("H", "W", "oh", "ow"):
        assert call(**{k: 0}) == -1 and b"[1, 8192]" in L.samnerf_last_error()
        assert call(**{k: 8193}) == -1
    assert call(n=need - 1) == -1 and b"workspace" in L.samnerf_last_error()
    assert call(ws=None) == -1 and b"workspace" in L.samnerf_last_error()
    # S is not looked at without out_input, but the other checks still hold
    assert call(S=0, inp=None, n=need - 1) == -1 and b"workspace" in L.samnerf_last_error()
