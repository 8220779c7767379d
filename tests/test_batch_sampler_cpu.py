"""The batch sampler without a GPU (samnerf_amd.batch): its torch path against
the reference's own get_rays and collate (tests/golden/batch_sampler.npz,
tools/make_batch_sampler_golden.py) -- exactly, every key -- and the host side
of the seeded draws (samnerf_batch_draw_host) against tests/philox_ref.py."""
import numpy as np
import pytest
import torch

import philox_ref
from batch_sampler_fixtures import collate_case, collate_cases, hwm, make_source, rays_case, tables

MODES = {"R": 0, "R_rect": 0, "P": 1, "C": 2, "C3": 2, "E": 3}


def _same(tag, got, want):
    want = torch.as_tensor(want)
    assert tuple(got.shape) == tuple(want.shape), (tag, got.shape, want.shape)
    assert got.dtype == want.dtype, (tag, got.dtype, want.dtype)
    assert torch.equal(got, want), (tag, (got != want).sum())


@pytest.mark.parametrize("name", list(MODES))
def test_twin_reproduces_the_reference_get_rays(name):
    """torch_select + torch_gather at the golden's seed: i, j, inds_coarse,
    rays_o and rays_d are the reference's, exactly."""
    from samnerf_amd import batch
    args, want = rays_case(name)
    t = tables()
    H, W, M = args["H"], args["W"], args["incoherent_mask_size"]
    src = make_source(with_mask=False, H=H if H != hwm()[0] else None, images=None)
    mode, n = MODES[name], args["N"]
    torch.manual_seed(args["seed"])
    index = want["index"]
    if mode == 0:
        assert torch.equal(torch.randint(0, 3, size=(n,)), index)     # the collate's draw comes first
    weights = None
    if mode >= 2:
        rows = torch.from_numpy(np.asarray(rays_case("C3")[1]["rows"])) if name == "C3" else index
        weights = t["error_map"][rows]
    count = n // 16 if mode == 1 else n
    pixels, cells = batch.torch_select(mode, H, W, count, args.get("patch_size", 1), weights, M)
    got = batch.torch_gather(src, index, pixels, H, W, coarse_size=None if mode == 3 else M)
    if mode == 3:
        got["inds_coarse"] = cells
    for k in ("i", "j", "inds_coarse", "rays_o", "rays_d"):
        _same(f"{name}/{k}", got[k], want[k])


@pytest.mark.parametrize("name", collate_cases())
def test_sampler_reproduces_the_reference_collate(name):
    """TrainBatchSampler(rng='torch') on a CPU source at the golden's seed:
    every tensor the reference's collate returned, key by key -- shapes,
    dtypes, values, and which keys the local rays were appended to."""
    from samnerf_amd.batch import TrainBatchSampler
    case, want, opt = collate_case(name)
    src = make_source(with_mask=opt.with_mask)
    sampler = TrainBatchSampler(src, opt, rng="torch", use_default_intrinsics=case["default_intrinsics"])
    torch.manual_seed(case["seed"])
    got = sampler.sample(case["global_step"], case["index"])
    for k, w in want.items():
        if k in ("H", "W", "use_default_intrinsics"):
            assert got[k] == w, k
        elif k == "index" and not torch.is_tensor(got[k]):
            assert list(got[k]) == list(w)
        else:
            _same(f"{name}/{k}", got[k], w)
    if name == "mask_mixed":
        n, local = opt.num_rays, opt.num_local_sample * opt.local_sample_patch_size ** 2
        for k in ("rays_o", "rays_d", "masks", "incoherent_masks", "error_maps", "cam_near_far", "poses"):
            assert got[k].shape[0] == n + local, k
        for k in ("images", "inds_coarse", "i", "j"):
            assert got[k].shape[0] == n, k


def test_random_image_batch_switches_on_and_stays():
    """colmap_provider.py:966-967: past rgb_similarity_iter, or after three
    epochs; the reference sets the option and never clears it."""
    from samnerf_amd.batch import TrainBatchSampler
    _, _, opt = collate_case("rgb_random")
    opt.random_image_batch = False
    opt.patch_size = 1
    src = make_source(with_mask=False)
    s = TrainBatchSampler(src, opt)
    opt.with_mask = False
    with pytest.raises(ValueError, match="draws from a map"):
        s.sample(1, [0])                                   # not yet random: mode E, and no map
    assert s.sample(10, [0])["rays_o"].shape == (65, 3)    # 10 / 3 images > 3 epochs
    assert s.random_image_batch and torch.is_tensor(s.sample(1, [0])["index"])


def _words(seed, offset, item):
    ctr = np.array([3 << 16, item, offset & philox_ref.MASK, offset >> 32], np.uint64)
    return [int(w) for w in philox_ref.philox4x32_10(ctr, [seed & philox_ref.MASK, seed >> 32])]


@pytest.mark.parametrize("seed,offset,item", [(0, 0, 0), (5, 7, 3), ((1 << 63) - 1, (1 << 40) + 9, 4095),
                                              (0x0123456789ABCDEF, 1 << 33, 0xFFFFFFFF)])
def test_draw_host_known_answers(hip_lib, seed, offset, item):
    """The word-for-value contract of include/samnerf_hip.h against the numpy
    generator: integers (uint64(word) * R) >> 32 of words 0 and 1, uniforms
    (word >> 8) * 2^-24 of words 2 and 3."""
    from samnerf_amd.batch import batch_draw_host
    w = _words(seed, offset, item)
    for r0, r1 in ((3, 14400), (1, 2), (1 << 31, 0xFFFFFFFF)):
        ints, us = batch_draw_host(seed, offset, item, r0, r1)
        assert ints == ((w[0] * r0) >> 32, (w[1] * r1) >> 32)
        assert us == ((w[2] >> 8) * 2.0 ** -24, (w[3] >> 8) * 2.0 ** -24)


def test_draw_host_ranges(hip_lib):
    from samnerf_amd.batch import batch_draw_host
    seen = set()
    for item in range(512):
        (a, b), (u, v) = batch_draw_host(11, 2, item, 1, 2)
        (c, _), _ = batch_draw_host(11, 2, item, 1 << 31, 1)
        assert a == 0 and b in (0, 1) and 0 <= c < 1 << 31 and 0.0 <= u < 1.0 and 0.0 <= v < 1.0
        seen.add(b)
    assert seen == {0, 1}


def test_draw_streams_share_no_counter_with_the_perturb_stages():
    """Perturb counters have c0 >> 16 in {0, 1, 2} (at most 65536 values per
    stage and ray: quad < 2^14); the items use 3 and the keys 4..7 (cell < 2^20:
    quad < 2^18).  The same (seed, offset, ray) therefore gives other words."""
    perturb_c0 = {(q | s << 16) >> 16 for s in range(3) for q in (0, (1 << 14) - 1)}
    batch_c0 = {(3 << 16) >> 16} | {((4 << 16) + q) >> 16 for q in (0, (1 << 16) - 1, 1 << 16, (1 << 18) - 1)}
    assert perturb_c0 == {0, 1, 2} and batch_c0 == {3, 4, 5, 7} and not perturb_c0 & batch_c0
    for s in range(3):
        assert _words(9, 1, 5) != [int(v) for v in philox_ref.words(9, 1, s, [5], 4)[0]]


def test_wrapper_errors(hip_lib):
    from samnerf_amd import batch
    _, _, opt = collate_case("mask_error_pixels")
    src = make_source()
    # mode E on a map that is not 128 x 128
    small = make_source(error_map=torch.ones(3, 64 * 64))
    opt.error_map_size = 64
    with pytest.raises(ValueError, match="128 x 128 map only"):
        batch.TrainBatchSampler(small, opt).sample(1, [0])
    with pytest.raises(ValueError, match="128 x 128 map only"):
        batch.torch_select(batch.MODE_E, 120, 120, 4, 1, torch.ones(1, 64 * 64), 64)
    with pytest.raises(ValueError, match="128 x 128 map only"):
        batch.hip_draw(batch.MODE_E, 3, 120, 120, 4, device="cpu", M=64)
    # a row with fewer positive weights than the draw needs
    opt.error_map_size = 128
    src.error_map[2, 64:] = 0.0
    src.error_map[2, 5] = float("inf")
    with pytest.raises(ValueError, match="63 positive finite weights, the draw needs 65"):
        batch.TrainBatchSampler(src, opt, check_inputs=True).sample(1, [2])
    # the seeded source has no CPU fallback
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        batch.TrainBatchSampler(src, opt, rng=batch.PhiloxBatch(1))
    with pytest.raises(ValueError):
        batch.PhiloxBatch(-1)
