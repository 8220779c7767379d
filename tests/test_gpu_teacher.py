"""The teacher image on the device (csrc/teacher_image.hip, samnerf_amd.teacher)
against the numpy restatement of the header's arithmetic (tests/teacher_ref.py,
itself held against PIL in tests/test_teacher_cpu.py): every byte of the uint8
image and every bit of the input planes, the padding, output selection,
repeatability, and the steps built on it -- set_image_from_render,
train.sam_distill_step, evaluate.eval_step(predictor=...)."""
import functools
import types

import numpy as np
import pytest
import torch

import teacher_fixtures as fx
import teacher_ref as ref
from helpers import make_net
from oracle import synth

pytestmark = pytest.mark.gpu

# (H, W) -> (oh, ow) in an S x S plane
SIZES = [((5, 7), (16, 23), 23), ((9, 9), (9, 20), 20), ((16, 16), (16, 16), 16), ((100, 75), (64, 48), 64),
         ((7, 5), (3, 2), 3), ((33, 65), (17, 1024), 1024)]
KINDS = ["uniform", "ends", "edges"]


@functools.lru_cache(maxsize=None)
def case(src, dst, S, kind, mean=ref.PIXEL_MEAN, std=ref.PIXEL_STD):
    """(rgb fp32 [H, W, 3], u8, input) as read-only numpy arrays, computed once."""
    H, W = src
    rng = np.random.default_rng(H * 1009 + W * 17 + dst[1] + KINDS.index(kind))
    n = H * W * 3
    if kind == "uniform":
        rgb = rng.random(n, dtype=np.float32)
    elif kind == "ends":
        rgb = rng.integers(0, 2, n).astype(np.float32)
    else:
        rgb = rng.permutation(np.resize(ref.edge_values(), max(n, 768)))[:n]
    rgb = np.ascontiguousarray(rgb.reshape(H, W, 3), np.float32)
    assert rgb.min() >= 0.0 and rgb.max() <= 1.0
    u8, inp = ref.teacher_image(rgb, dst[0], dst[1], S, mean, std)
    for a in (rgb, u8, inp):
        a.setflags(write=False)
    return rgb, u8, inp


def raw(L, rgb, dst, S, u8, inp, mean=None, std=None):
    """One samnerf_teacher_image call on torch's current stream."""
    import ctypes

    from samnerf_amd.ops import _ptr, _stream
    H, W = rgb.shape[:2]
    need = L.samnerf_teacher_image_workspace_size(H, W, dst[0], dst[1])
    ws = torch.empty(need, dtype=torch.uint8, device=rgb.device)
    m = None if mean is None else (ctypes.c_float * 3)(*mean)
    s = None if std is None else (ctypes.c_float * 3)(*std)
    rc = L.samnerf_teacher_image(_ptr(rgb), H, W, dst[0], dst[1], S, m, s, _ptr(u8), _ptr(inp), _ptr(ws), need,
                                 _stream(rgb))
    assert rc == 0, L.samnerf_last_error()


def buffers(dst, S, cuda):
    return (torch.full((dst[0], dst[1], 3), 77, dtype=torch.uint8, device=cuda),
            torch.full((3, S, S), float("nan"), device=cuda))


def same(got, want):
    return fx.golden.same(got, want)


# ----------------------------------------------------------------- the bits --

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("src,dst,S", SIZES)
def test_u8_and_input_equal_the_restatement(hip_lib, cuda, src, dst, S, kind):
    rgb, want_u8, want_in = case(src, dst, S, kind)
    u8, inp = buffers(dst, S, cuda)
    raw(hip_lib, torch.from_numpy(rgb.copy()).to(cuda), dst, S, u8, inp)
    diff = int((u8.cpu().numpy() != want_u8).sum())
    print(f"{src} -> {dst} {kind}: {diff} differing bytes of {want_u8.size}")
    assert same(u8, want_u8)
    assert same(inp, want_in)                       # NaN-prefilled: every cell was written


def test_sams_plane_size_once(hip_lib, cuda):
    """(64, 48) -> (1024, 768) into S = 1024: more than one block on both axes,
    a pad strip 256 wide."""
    src, dst, S = (64, 48), (1024, 768), 1024
    rgb, want_u8, want_in = case(src, dst, S, "uniform")
    u8, inp = buffers(dst, S, cuda)
    raw(hip_lib, torch.from_numpy(rgb.copy()).to(cuda), dst, S, u8, inp)
    assert same(u8, want_u8) and same(inp, want_in)
    assert ref.preprocess_shape(*src) == dst


def test_other_mean_and_std(hip_lib, cuda):
    mean, std = (100.0, 110.5, 120.25), (50.0, 60.5, 70.125)
    src, dst, S = (5, 7), (16, 23), 23
    rgb, want_u8, want_in = case(src, dst, S, "uniform", mean, std)
    u8, inp = buffers(dst, S, cuda)
    raw(hip_lib, torch.from_numpy(rgb.copy()).to(cuda), dst, S, u8, inp, mean, std)
    assert same(u8, want_u8) and same(inp, want_in)


# ------------------------------------------------------------------ padding --

def test_padding_is_positive_zero_on_both_axes(hip_lib, cuda):
    src, dst, S = (5, 7), (16, 23), 32
    rgb, want_u8, want_in = case(src, dst, S, "uniform")
    u8, inp = buffers(dst, S, cuda)
    raw(hip_lib, torch.from_numpy(rgb.copy()).to(cuda), dst, S, u8, inp)
    got = inp.cpu().numpy()
    assert not np.isnan(got).any()
    below, right = got[:, dst[0]:, :], got[:, :, dst[1]:]
    assert below.size and right.size
    for pad in (below, right):
        assert (pad.view(np.uint32) == 0).all()     # +0.0: no bit set
    assert same(inp, want_in) and same(u8, want_u8)


# --------------------------------------------------------- output selection --

def test_an_output_that_is_not_asked_for_is_not_touched(hip_lib, cuda):
    src, dst, S = (100, 75), (64, 48), 64
    rgb, want_u8, want_in = case(src, dst, S, "uniform")
    x = torch.from_numpy(rgb.copy()).to(cuda)
    u8, inp = buffers(dst, S, cuda)
    raw(hip_lib, x, dst, S, u8, None)
    assert same(u8, want_u8) and bool(torch.isnan(inp).all())
    u8.fill_(77)
    raw(hip_lib, x, dst, S, None, inp)
    assert same(inp, want_in) and bool((u8 == 77).all())


# ------------------------------------------------------------ repeatability --

def test_two_calls_and_another_stream_give_the_same_bits(hip_lib, cuda):
    src, dst, S = (33, 65), (17, 1024), 1024
    rgb, want_u8, want_in = case(src, dst, S, "uniform")
    x = torch.from_numpy(rgb.copy()).to(cuda)
    runs = []
    for _ in range(2):
        u8, inp = buffers(dst, S, cuda)
        raw(hip_lib, x, dst, S, u8, inp)
        runs.append((u8, inp))
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=cuda)
    with torch.cuda.stream(side):
        u8, inp = buffers(dst, S, cuda)
        raw(hip_lib, x, dst, S, u8, inp)
    side.synchronize()
    runs.append((u8, inp))
    for u8, inp in runs:
        assert same(u8, want_u8) and same(inp, want_in)


# ------------------------------------------------------------ the module --

@pytest.mark.parametrize("i,target", fx.GOLDEN_CASES)
def test_teacher_image_equals_the_mirror_of_its_cpu_copy(hip_lib, cuda, i, target):
    """On a CUDA render the kernels, on its CPU copy PIL: the same dict.  Where
    PIL is absent, PIL's recorded bytes for the same input stand in."""
    from samnerf_amd import teacher
    rgb = fx.render_of(fx.golden.arr(f"in{i}"))
    got = teacher.teacher_image(rgb.to(cuda), target=target, size=target + 3)
    want_u8 = fx.golden.arr(f"out{i}")
    assert got["u8"].is_cuda and got["input"].is_cuda and got["input"].shape == (1, 3, target + 3, target + 3)
    assert got["input_size"] == want_u8.shape[:2]
    assert same(got["u8"], want_u8)
    assert same(got["input"][0], ref.normalise_pad(want_u8, target + 3))
    try:
        import PIL  # noqa: F401
    except ImportError:
        return
    mirror = teacher.torch_teacher_image(rgb, target=target, size=target + 3)
    assert mirror["input_size"] == got["input_size"]
    assert same(got["u8"], mirror["u8"]) and same(got["input"], mirror["input"])
    only = teacher.teacher_image(rgb.to(cuda), target=target, want="input")
    assert sorted(only) == ["input", "input_size"]


def test_set_image_from_render_on_the_device(hip_lib, cuda):
    from samnerf_amd.teacher import set_image_from_render
    p = fx.StubPredictor(tuple_out=True)
    rgb = torch.rand(12, 20, 3, generator=torch.Generator().manual_seed(8))
    feats = set_image_from_render(p, rgb.to(cuda))
    assert p.log == ["reset_image()", "original_size", "input_size", "features", "interm_features", "is_image_set"]
    assert p.original_size == (12, 20) and p.input_size == (614, 1024) and p.is_image_set is True
    seen = p.model.image_encoder.seen
    assert len(seen) == 1 and seen[0].is_cuda and seen[0].shape == (1, 3, 1024, 1024)
    assert same(seen[0][0], ref.teacher_image(rgb.numpy(), 614, 1024, 1024)[1])
    assert feats is p.features and feats.is_cuda and feats.shape == (1, 256, 64, 64)


# ------------------------------------------------------------------ the steps --

@pytest.fixture(scope="module")
def scene(cuda):
    """The small synthetic SAM scene of the training tests: a 16 x 16 full view
    and an 8 x 8 feature view of it."""
    from samnerf_amd import ops
    spec = synth.ModelSpec(with_sam=True, grid_log2=12, s_grid_log2=11, prop_log2=10)
    params = synth.make_params(spec, seed=21, emb_scale=0.5, ln_jitter=0.1)
    rot = synth.random_rotation(4)
    pose, intr = synth.gui_camera(16, 16, rot=rot)
    ro, rd = ops.get_rays(pose, intr, 16, 16, device=cuda)
    pose_lr, intr_lr = synth.gui_camera(8, 8, rot=rot)
    ro_lr, rd_lr = ops.get_rays(pose_lr, intr_lr, 8, 8, device=cuda)

    def data():
        return {"rays_o": ro, "rays_d": rd, "H": 16, "W": 16, "rays_o_lr": ro_lr, "rays_d_lr": rd_lr, "h": 8, "w": 8,
                "index": [0]}

    def net(train=True):
        n = make_net(spec, params, cuda)
        if train:
            n.train()
            for k, p in n.named_parameters():                  # main.py:255-262
                p.requires_grad = k.startswith("s_grid") or k.startswith("samvit_mlp")
        return n
    return net, data


def _count_renders(net, monkeypatch):
    calls = []
    render = net.render

    def counted(*a, **kw):
        out = render(*a, **kw)
        calls.append((kw, out))
        return out
    monkeypatch.setattr(net, "render", counted)
    return calls


def _grads(net):
    return {k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None}


def test_sam_distill_step_miss_then_hit(hip_lib, cuda, scene, monkeypatch):
    from samnerf_amd.fused import FusedRenderer
    from samnerf_amd.teacher import FeatureCache
    from samnerf_amd.train import sam_distill_step, sam_train_step_fused
    make, data = scene
    net = make()
    fr = FusedRenderer(net, deterministic=True)
    calls = _count_renders(net, monkeypatch)
    opt = types.SimpleNamespace(with_sam=True, cache_size=1, cache_interval=4, background="white")
    cache, p = FeatureCache(1), fx.StubPredictor()
    d = data()
    # step 1: the cache is empty -- a miss
    net.zero_grad(set_to_none=True)
    pred, gt, loss = sam_distill_step(net, fr, d, opt, 1, p, cache=cache)
    loss.backward()
    miss = (loss.detach().clone(), pred.clone(), _grads(net))
    assert len(calls) == 1 and calls[0][0]["staged"] and calls[0][0]["perturb"] and not calls[0][0]["update_proposal"]
    assert cache.full() and cache.get(0) is d and d["gt_samvit"] is gt and gt is p.features
    assert gt.is_cuda and gt.shape == (1, 256, 64, 64) and not gt.requires_grad
    image = calls[0][1]["image"].reshape(16, 16, 3).cpu().numpy()
    seen = p.model.image_encoder.seen
    assert len(seen) == 1 and same(seen[0][0], ref.teacher_image(image, 1024, 1024, 1024)[1])
    assert p.original_size == (16, 16) and p.input_size == (1024, 1024)
    assert pred.shape == (1, 256, 64, 64) and len(miss[2]) == 13
    # the same step by hand
    net.zero_grad(set_to_none=True)
    pred_h, loss_h = sam_train_step_fused(fr, d["rays_o_lr"], d["rays_d_lr"], 8, 8, gt)
    loss_h.backward()
    hand = _grads(net)
    assert torch.equal(miss[0], loss_h.detach()) and torch.equal(miss[1], pred_h)
    for k in hand:
        assert torch.equal(miss[2][k], hand[k]), k
    # step 2: the cache is full and 2 % 4 != 0 -- a hit: no full-resolution render, no encoder call
    del calls[:]
    pred2, gt2, loss2 = sam_distill_step(net, fr, data(), opt, 2, p, cache=cache)
    assert not calls and len(seen) == 1 and gt2 is gt and torch.equal(loss2.detach(), miss[0])
    # step 4: every cache_interval-th step renders again and overwrites the ring's slot
    d4 = data()
    _, gt4, _ = sam_distill_step(net, fr, d4, opt, 4, p, cache=cache)
    assert len(calls) == 1 and len(seen) == 2 and cache.get(0) is d4 and d4["gt_samvit"] is gt4
    # without a cache every step is a miss and nothing is kept
    d5 = data()
    sam_distill_step(net, fr, d5, types.SimpleNamespace(with_sam=True, cache_size=0, cache_interval=4), 5, p)
    assert len(calls) == 2 and "gt_samvit" not in d5


def test_sam_distill_step_does_not_synchronise(hip_lib, cuda, scene):
    """A miss step and a hit step, with their backward, under torch's sync
    debug mode set to raise on a synchronising call it knows of (a read-back, a
    pageable copy, nonzero, item): none happens.  The teacher render draws its
    sample positions in the kernels (perturb_rng = 'philox'); with torch's
    generator the render uploads two small linspaces from the host, as the
    reference does, which is a synchronising copy but no read of device memory."""
    from samnerf_amd.fused import FusedRenderer
    from samnerf_amd.teacher import FeatureCache
    from samnerf_amd.train import sam_distill_step
    make, data = scene
    net = make()
    net.perturb_rng = "philox"
    fr = FusedRenderer(net, deterministic=True)
    opt = types.SimpleNamespace(with_sam=True, cache_size=1, cache_interval=4, background="white")
    p = fx.StubPredictor()
    sam_distill_step(net, fr, data(), opt, 1, p, cache=FeatureCache(1))[2].backward()      # warm-up: first-call set-up
    cache = FeatureCache(1)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for step in (1, 2):
            sam_distill_step(net, fr, data(), opt, step, p, cache=cache)[2].backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert cache.full() and len(p.model.image_encoder.seen) == 2       # the warm-up's and step 1's; step 2 hit


def test_eval_step_with_a_predictor(hip_lib, cuda, scene):
    from samnerf_amd.evaluate import eval_step
    make, data = scene
    net = make(train=False)
    opt = types.SimpleNamespace(with_sam=True, with_mask=False, use_point=False)
    p = fx.StubPredictor()
    with torch.no_grad():
        rgb, depth, pred, truth, loss = eval_step(net, data(), opt, predictor=p)
        seen = p.model.image_encoder.seen
        assert len(seen) == 1 and seen[0].is_cuda
        assert same(seen[0][0], ref.teacher_image(rgb.cpu().numpy(), 1024, 1024, 1024)[1])
        assert truth is rgb and pred.shape == (1, 256, 64, 64) and p.original_size == (16, 16)
        # the callback path, fed the same features: the same loss; and it is what it was
        images = []

        def features(image):
            images.append(image)
            return p.features
        rgb_c, _, pred_c, _, loss_c = eval_step(net, data(), opt, sam_features=features)
        assert len(seen) == 1 and len(images) == 1
        assert isinstance(images[0], np.ndarray) and images[0].dtype == np.uint8 and images[0].shape == (16, 16, 3)
        assert np.array_equal(images[0], ref.quantise(rgb_c.cpu().numpy()))
        assert torch.equal(rgb_c, rgb) and torch.equal(pred_c, pred) and torch.equal(loss_c, loss)
        with pytest.raises(ValueError, match="sam_features"):
            eval_step(net, data(), opt)
