"""The batch sampler's kernels (csrc/batch_sampler.hip) on the GPU: the gather
against its torch twin and the reference's golden, the seeded draws against
their replay from samnerf_batch_draw_fill's arrays, the weighted draw against a
stable sort of its own keys and against the distribution it claims, and the
loop error map -> sampling -> render -> loss -> error map on the device."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from batch_sampler_fixtures import hwm, make_source, rays_case, tables

pytestmark = pytest.mark.gpu

RAYS_D_TOL = 2e-6          # absolute; samnerf_get_rays' bar for rotated poses (the twin's matmul sums in another order)
SEED = 0x5EED5EED5EED


@functools.lru_cache(maxsize=None)
def _sources(C, H=None):
    over = {}
    if C == 3:
        over["images"] = tables()["images"][..., :3].contiguous()
    cpu = make_source("cpu", H=H, **over)
    gpu = make_source("cuda", H=H, **{k: v.cuda() for k, v in over.items()})
    return cpu, gpu


def _rays(n, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    index = torch.randint(0, 3, (n,), generator=g)
    pixels = torch.randint(0, H * W, (n,), generator=g)
    if n >= 4:                       # the corners of the image
        pixels[:4] = torch.tensor([0, W - 1, (H - 1) * W, H * W - 1])
    return index, pixels


def _compare(got, want):
    assert set(got) == set(want)
    for k, w in want.items():
        g = got[k].cpu()
        if k == "cam_near_far":
            w = w.expand(g.shape[0], 2)
        assert g.shape == w.shape and g.dtype == w.dtype, k
        if k == "rays_d":
            err = float((g - w).abs().max())
            print(f"rays_d max abs error {err:.3e}")
            assert err <= RAYS_D_TOL
        else:
            assert torch.equal(g, w), k


@pytest.mark.parametrize("C", [3, 4])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4096])
def test_gather_matches_the_twin(hip_lib, cuda, n, C):
    """k_batch_gather on the twin's indices: H = W = 120 under a 128 x 128 map,
    so 128 / 120 is no binary fraction; rotated poses that differ per ray."""
    from samnerf_amd import batch
    cpu, gpu = _sources(C)
    H, W, M = hwm()
    index, pixels = _rays(n, H, W, 100 + n)
    want = batch.torch_gather(cpu, index, pixels, H, W, coarse_size=M)
    got = batch.hip_gather(gpu, index.cuda(), pixels.cuda(), H, W, coarse_size=M)
    _compare(got, want)
    # one image for all rays, and one row of intrinsics
    fixed = batch.fixed_fov_intrinsics(H, "cpu")
    want = batch.torch_gather(cpu, [2], pixels, H, W, intrinsics=fixed, coarse_size=M)
    got = batch.hip_gather(gpu, [2], pixels.cuda(), H, W, intrinsics=fixed, coarse_size=M)
    _compare(got, want)


def test_gather_on_a_96_x_120_image(hip_lib, cuda):
    from samnerf_amd import batch
    cpu, gpu = _sources(4, H=96)
    index, pixels = _rays(65, 96, 120, 7)
    want = batch.torch_gather(cpu, index, pixels, 96, 120, coarse_size=128)
    got = batch.hip_gather(gpu, index.cuda(), pixels.cuda(), 96, 120, coarse_size=128)
    _compare(got, want)


@pytest.mark.parametrize("name", ["R", "R_rect", "C3", "E"])
def test_gather_matches_the_reference(hip_lib, cuda, name):
    """The reference's own get_rays at its own pixels: integers exact, rays_o
    exact, rays_d within the bar."""
    from samnerf_amd import batch
    args, want = rays_case(name)
    H, W, M = args["H"], args["W"], args["incoherent_mask_size"]
    _, gpu = _sources(4, H=H if H != hwm()[0] else None)
    pixels = (want["j"] * W + want["i"]).cuda()
    got = batch.hip_gather(gpu, want["index"].cuda(), pixels, H, W, coarse_size=M,
                           want=("rays_o", "rays_d", "i", "j", "inds_coarse"))
    for k in ("i", "j", "rays_o") + (("inds_coarse",) if name != "E" else ()):
        assert torch.equal(got[k].cpu(), want[k]), k
    err = float((got["rays_d"].cpu() - want["rays_d"]).abs().max())
    print(f"{name}: rays_d max abs error against the reference {err:.3e}")
    assert err <= RAYS_D_TOL


def test_null_tables_leave_their_outputs_untouched(hip_lib, cuda):
    """A source without masks, maps, images and cam_near_far, handed output
    buffers for them: every byte keeps its canary; the rest is written."""
    from samnerf_amd import _lib, batch
    t = tables()
    src = batch.BatchSource(t["poses"].cuda(), t["intrinsics"].cuda(), 120, 120)
    n = 65
    index, pixels = _rays(n, 120, 120, 3)
    index, pixels = index.cuda(), pixels.cuda()
    shapes = {"rays_o": (n, 3), "rays_d": (n, 3), "i": (n,), "j": (n,), "inds_coarse": (n,), "images": (n, 4),
              "masks": (n,), "incoherent_masks": (n,), "error_maps": (n,), "cam_near_far": (n, 2)}
    bufs = {k: torch.full((int(np.prod(s)) * 8,), 0xA5, dtype=torch.uint8, device=cuda) for k, s in shapes.items()}
    o = _lib.SamnerfBatchOut()
    for k, b in bufs.items():
        setattr(o, k, ctypes.c_void_p(b.data_ptr()))
    s = src.c_struct()
    stream = ctypes.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)
    rc = hip_lib.samnerf_batch_gather(ctypes.byref(s), ctypes.c_void_p(index.data_ptr()), n,
                                      ctypes.c_void_p(pixels.data_ptr()), n, 120, 120, 0, ctypes.byref(o), stream)
    assert rc == 0, hip_lib.samnerf_last_error()
    torch.cuda.synchronize()
    for k in ("images", "masks", "incoherent_masks", "error_maps", "cam_near_far", "inds_coarse"):
        assert bool((bufs[k] == 0xA5).all()), k                 # inds_coarse: coarse_size = 0
    assert torch.equal(bufs["i"].view(torch.int64)[:n].cpu(), pixels.cpu() % 120)
    assert torch.equal(bufs["j"].view(torch.int64)[:n].cpu(), pixels.cpu() // 120)
    assert bool((bufs["rays_o"][n * 12:] == 0xA5).all()) and bool((bufs["i"][n * 8:] == 0xA5).all())
    # out-of-range rays write nothing
    bad_index = index.clone()
    bad_index[0], pixels[1] = 3, 120 * 120
    bufs["i"].fill_(0xA5)
    rc = hip_lib.samnerf_batch_gather(ctypes.byref(s), ctypes.c_void_p(bad_index.data_ptr()), n,
                                      ctypes.c_void_p(pixels.data_ptr()), n, 120, 120, 0, ctypes.byref(o), stream)
    assert rc == 0
    torch.cuda.synchronize()
    assert bool((bufs["i"][:16] == 0xA5).all()) and not bool((bufs["i"][16:24] == 0xA5).all())


# ------------------------------------------------------- array form = seeded

def _eq(a, b):
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_seeded_uniform_and_patches_equal_their_replay(hip_lib, cuda):
    from samnerf_amd import batch
    ph = batch.PhiloxBatch(SEED, 5)
    H, W, n = 96, 120, 4096
    seeded = batch.hip_draw(batch.MODE_R, 3, H, W, n, device=cuda, philox=ph, offset=2)
    f = batch.batch_draw_fill(ph, n, 3, H * W, cuda, offset=2)
    _eq(seeded, batch.hip_draw(batch.MODE_R, 3, H, W, n, device=cuda, int0=f["int0"], int1=f["int1"]))
    assert int(seeded["index"].min()) == 0 and int(seeded["index"].max()) == 2
    assert 0 <= int(seeded["pixels"].min()) and int(seeded["pixels"].max()) < H * W
    for item in (0, 1, 63, 64, 4095):
        (a, b), (u, v) = batch.batch_draw_host(SEED, 7, item, 3, H * W)
        assert (a, b) == (int(seeded["index"][item]), int(seeded["pixels"][item]))
        assert (u, v) == (float(f["u0"][item]), float(f["u1"][item]))
    other = batch.hip_draw(batch.MODE_R, 3, H, W, n, device=cuda, philox=ph, offset=3)
    assert not torch.equal(other["pixels"], seeded["pixels"])
    # mode P: 5 patches of 4 x 4
    p, k = 4, 5
    seeded = batch.hip_draw(batch.MODE_P, 3, H, W, k, device=cuda, patch=p, philox=ph)
    f = batch.batch_draw_fill(ph, k, H - p, W - p, cuda)
    _eq(seeded, batch.hip_draw(batch.MODE_P, 3, H, W, k, device=cuda, patch=p, int0=f["int0"], int1=f["int1"]))
    want = batch.expand_patches(f["int0"][:, None], f["int1"][:, None], p, W)
    assert torch.equal(seeded["pixels"], want)
    assert int(f["int0"].max()) < H - p and int(f["int1"].max()) < W - p


def test_seeded_weighted_draws_equal_their_replay(hip_lib, cuda):
    from samnerf_amd import batch
    ph = batch.PhiloxBatch(SEED, 9)
    H, W, M = hwm()
    emap = tables()["error_map"].cuda()
    # mode C, three rows whose images are drawn too
    seeded = batch.hip_draw(batch.MODE_C, 3, H, W, 3, device=cuda, patch=4, M=M, weights=emap, philox=ph)
    f = batch.batch_draw_fill(ph, 3, 3, 1, cuda, weights=emap, B=3)
    again = batch.hip_draw(batch.MODE_C, 3, H, W, 3, device=cuda, patch=4, M=M, rows=f["int0"], keys=f["keys"])
    _eq(seeded, again)
    assert torch.equal(seeded["index"].view(3, 16)[:, 0], f["int0"])
    for b in range(3):
        assert batch.batch_draw_host(SEED, 9, b, 3, 1)[0][0] == int(f["int0"][b])
    # the twin's corner arithmetic on the kernel's centres
    c = seeded["cells"][:, None]
    x0 = torch.clamp((c // M) * (H / M) - 2, min=0, max=H - 5).long()
    y0 = torch.clamp((c % M) * (W / M) - 2, min=0, max=W - 5).long()
    assert torch.equal(seeded["pixels"], batch.expand_patches(x0, y0, 4, W))
    # mode E
    n = 65
    seeded = batch.hip_draw(batch.MODE_E, 3, H, W, n, device=cuda, M=M, weights=emap, rows=[2], philox=ph)
    f = batch.batch_draw_fill(ph, n, 1, 1, cuda, weights=emap, rows=[2], B=1)
    again = batch.hip_draw(batch.MODE_E, 3, H, W, n, device=cuda, M=M, rows=[2], keys=f["keys"], u0=f["u0"],
                           u1=f["u1"])
    _eq(seeded, again)
    # the twin's pixel arithmetic on the kernel's cells and uniforms (utils.py:226-230)
    cells = seeded["cells"]
    x = ((cells // 128) * (H / M) + f["u0"] * (H / M)).long().clamp(max=H - 1)
    y = ((cells % 128) * (W / M) + f["u1"] * (W / M)).long().clamp(max=W - 1)
    assert torch.equal(seeded["pixels"], x * W + y)
    (_, _), (u, v) = batch.batch_draw_host(SEED, 9, 64, 1, 1)
    assert (u, v) == (float(f["u0"][64]), float(f["u1"][64]))


# ------------------------------------------------ weighted draw: correctness

def _expected(keys, n):
    order = torch.sort(keys, descending=True, stable=True).indices[:n]
    return torch.sort(order).values


def _weights(case, n, cells=16384):
    g = torch.Generator().manual_seed(17)
    if case == "random":
        return torch.rand(cells, generator=g) + 1e-3
    if case == "ones":
        return torch.ones(cells)
    w = torch.zeros(cells)
    if case == "exactly_n":
        w[torch.randperm(cells, generator=g)[:n]] = torch.rand(n, generator=g) + 0.5
    else:                                                     # half zeros
        keep = torch.randperm(cells, generator=g)[:cells // 2]
        w[keep] = torch.rand(cells // 2, generator=g) + 0.5
    return w


@pytest.mark.parametrize("n", [1, 65, 4095, 4096])
@pytest.mark.parametrize("case", ["random", "ones", "exactly_n", "half_zeros"])
def test_error_map_draw_is_the_top_n_of_its_keys(hip_lib, cuda, case, n):
    from samnerf_amd import batch
    ph = batch.PhiloxBatch(SEED + n, 1)
    w = _weights(case, n)
    table = torch.stack([torch.ones(16384), w]).cuda()
    got = batch.hip_draw(batch.MODE_E, 2, 120, 120, n, device=cuda, M=128, weights=table, rows=[1], philox=ph)
    keys = batch.batch_draw_fill(ph, 1, 1, 1, cuda, weights=table, rows=[1], B=1)["keys"][0]
    assert torch.equal(got["cells"], _expected(keys, n))
    assert bool((keys[table[1] == 0] == 0).all()) and bool((keys[table[1] > 0] > 0).all())
    if case == "ones":
        assert keys.unique().numel() < 16384, "no tie among the keys: the tie rule is not exercised"
    if case == "exactly_n":
        assert torch.equal(got["cells"], torch.nonzero(table[1] > 0).view(-1))
    if case == "half_zeros":
        assert bool((table[1][got["cells"]] > 0).all())
    assert 0 <= int(got["pixels"].min()) and int(got["pixels"].max()) < 120 * 120


def test_error_map_draw_breaks_ties_towards_the_lower_cell(hip_lib, cuda):
    """Keys handed in with heavy ties (eight distinct values): the stable
    sort's choice, whatever the histogram digits look like."""
    from samnerf_amd import batch
    g = torch.Generator().manual_seed(5)
    keys = (torch.randint(0, 8, (16384,), generator=g).float() * 0.37).cuda()
    for n in (1, 100, 5000, 16384):
        u = torch.zeros(n, device=cuda)
        got = batch.hip_draw(batch.MODE_E, 1, 120, 120, n, device=cuda, M=128, rows=[0], keys=keys, u0=u, u1=u)
        assert torch.equal(got["cells"], _expected(keys, n)), n


@pytest.mark.parametrize("B,M", [(1, 128), (3, 128), (3, 7), (1, 1024)])
def test_centred_draw_is_the_arg_max_of_its_keys(hip_lib, cuda, B, M):
    """n = 1 per row; M = 1024 is far beyond what LDS could stage and spans the
    key stages 4..7; M = 7 has a ragged last quad."""
    from samnerf_amd import batch
    ph = batch.PhiloxBatch(SEED, 40 + M)
    g = torch.Generator().manual_seed(M)
    table = (torch.rand(3, M * M, generator=g) * (torch.rand(3, M * M, generator=g) > 0.5)).cuda()
    if M == 128:
        table[1] = 1.0                                       # ties
    rows = [1, 0, 2][:B]
    got = batch.hip_draw(batch.MODE_C, 3, 600, 520, B, device=cuda, patch=16, M=M, weights=table, rows=rows,
                         philox=ph)
    keys = batch.batch_draw_fill(ph, 1, 1, 1, cuda, weights=table, rows=rows, B=B)["keys"]
    want = torch.stack([_expected(keys[b], 1)[0] for b in range(B)])
    assert torch.equal(got["cells"], want)
    assert bool((table[rows][torch.arange(B), got["cells"]] > 0).all())
    assert int(got["pixels"].max()) < 600 * 520 and int(got["pixels"].min()) >= 0


# ----------------------------------------------- weighted draw: distribution

CHI2_BOUND = 110.84        # chi2.ppf(1 - 1e-4, 61)


def _pearson(counts, w):
    pos = w > 0
    expected = counts.sum() * w[pos] / w[pos].sum()
    return float(((counts[pos] - expected) ** 2 / expected).sum())


def test_centred_draw_follows_the_weights(hip_lib, cuda):
    """8192 single draws over 62 positive cells of weights 1 and 3: Pearson's
    statistic under the 1e-4 quantile of chi2(61), the zeroed cells never
    drawn; torch.multinomial passes the same assertion (the bound's check)."""
    from samnerf_amd import batch
    M, B = 8, 8192
    w = torch.ones(M * M, dtype=torch.float64)
    w[1::2] = 3.0
    w[[10, 37]] = 0.0
    table = w.float()[None].cuda().contiguous()
    got = batch.hip_draw(batch.MODE_C, 1, 120, 120, B, device=cuda, patch=2, M=M, weights=table,
                         rows=torch.zeros(B, dtype=torch.int64), philox=batch.PhiloxBatch(2024))
    counts = torch.bincount(got["cells"].cpu(), minlength=M * M).double()
    stat = _pearson(counts, w)
    torch.manual_seed(2024)
    ref = torch.bincount(torch.multinomial(w.float().expand(B, -1), 1).view(-1), minlength=M * M).double()
    ref_stat = _pearson(ref, w)
    print(f"Pearson statistic: kernel {stat:.2f}, torch.multinomial {ref_stat:.2f}, bound {CHI2_BOUND}")
    assert counts[10] == 0 and counts[37] == 0 and counts.sum() == B
    assert stat < CHI2_BOUND
    assert ref[10] == 0 and ref[37] == 0 and ref_stat < CHI2_BOUND


# ------------------------------------------------------------- loop closure

def _loop(cuda, steps=3):
    from test_gpu_mask_loss import _full_opts, _nets

    from samnerf_amd import batch, synth
    from samnerf_amd.train import mask_train_step_full
    torch.manual_seed(5)                     # mask_train_step_full's RGB-similarity draw is torch's
    gpu, _ = _nets(cuda, "adaptive")
    opt = gpu.opt
    n, M, S = 1024, 16, 64
    _full_opts(opt, n)
    opt.with_mask, opt.error_map_size, opt.online_resolution = True, M, S
    opt.random_image_batch, opt.enable_cam_near_far = False, False
    g = torch.Generator().manual_seed(31)
    poses = torch.stack([torch.from_numpy(synth.gui_camera(S, S, rot=synth.random_rotation(k))[0]) for k in (4, 5, 6)])
    intr = torch.from_numpy(synth.gui_camera(S, S)[1])[None].repeat(3, 1)
    src = batch.BatchSource(
        poses.to(cuda), intr.to(cuda), S, S,
        images=torch.randint(0, 256, (3, S, S, 3), generator=g, dtype=torch.uint8).to(cuda),
        masks=torch.randint(0, 5, (3, S, S, 1), generator=g).to(cuda),
        incoherent_masks=(torch.rand(3, S * S, generator=g) > 0.5).float().to(cuda),
        error_map=(0.05 + 0.3 * torch.rand(3, M * M, generator=g)).to(cuda))
    sampler = batch.TrainBatchSampler(src, opt, rng=batch.PhiloxBatch(77, 1000), use_default_intrinsics=False)
    log = []
    for step in range(1, steps + 1):
        before = src.error_map.clone()
        data = sampler.sample(step, [0])
        draw = dict(sampler.last_draw)
        pred, _, loss = mask_train_step_full(gpu, data, step, error_map=src.error_map)
        log.append(dict(before=before, after=src.error_map.clone(), data=data, draw=draw, pred=pred,
                        loss=loss.detach()))
    return src, opt, log


def test_error_map_loop_stays_on_the_device_and_repeats(hip_lib, cuda):
    from samnerf_amd import batch
    src, opt, log = _loop(cuda)
    M2 = opt.error_map_size ** 2
    for k, s in enumerate(log):
        d = s["data"]
        assert d["rays_o"].shape == (1024 + 512, 3) and d["inds_coarse"].shape == (1024,)
        assert d["masks"].shape == (1536, 1) and d["images"].shape == (1024, 3)
        # the map changes only at the global rays' cells
        touched = torch.zeros(3 * M2, dtype=torch.bool, device=cuda)
        touched[d["index"] * M2 + d["inds_coarse"]] = True
        changed = (s["after"] != s["before"]).view(-1)
        assert bool(changed.any()) and not bool((changed & ~touched).any()), k
        if k:
            assert torch.equal(s["before"], log[k - 1]["after"])
        # the local patches are the draw over the map as the previous step left it
        replay = batch.hip_draw(batch.MODE_C, 3, 64, 64, 2, device=cuda, patch=16, M=opt.error_map_size,
                                weights=s["before"].contiguous(), philox=batch.PhiloxBatch(77, 1000),
                                offset=2 * (k + 1) + 1)
        assert torch.equal(replay["pixels"], s["draw"]["local_pixels"])
        assert torch.equal(replay["index"], s["draw"]["local_index"])
    _, _, again = _loop(cuda)
    for a, b in zip(log, again):
        assert torch.equal(a["after"], b["after"]) and torch.equal(a["pred"], b["pred"])
        assert torch.equal(a["loss"], b["loss"])
        for k, v in a["data"].items():
            if torch.is_tensor(v):
                assert torch.equal(v, b["data"][k]), k


# ------------------------------------------------- the sampler's two GPU paths

@pytest.mark.parametrize("name", ["rgb_random", "mask_mixed", "mask_error_pixels", "mask_incoherent_patch"])
def test_sampler_kernel_path_equals_the_twin_on_the_gpu(hip_lib, cuda, name):
    """rng='torch' on a CUDA source: the same torch draws feed k_batch_gather
    and the torch twin; every key agrees (rays_d within the bar).  images:
    torch's GPU kernel divides by the scalar 255 as a product with fl(1 / 255)
    (two roundings: within 2 ulp of the true quotient, values below 1), where
    the kernel and torch on the CPU divide; test_gather_matches_the_twin holds
    the kernel to the CPU's bits."""
    from batch_sampler_fixtures import collate_case

    from samnerf_amd.batch import TrainBatchSampler
    case, want, opt = collate_case(name)
    _, gpu = _sources(4)
    src = gpu if opt.with_mask else make_source("cuda", with_mask=False)
    outs = []
    for use_kernels in (True, False):
        s = TrainBatchSampler(src, opt, use_default_intrinsics=case["default_intrinsics"], use_kernels=use_kernels)
        torch.manual_seed(case["seed"])
        outs.append(s.sample(case["global_step"], case["index"]))
    hip, twin = outs
    assert set(hip) == set(twin) and set(want) <= set(hip)
    for k, w in twin.items():
        if not torch.is_tensor(w):
            assert hip[k] == w, k
            continue
        assert hip[k].shape == w.shape and hip[k].dtype == w.dtype, k
        assert k not in want or tuple(w.shape) == tuple(want[k].shape), k      # the reference's shapes
        if k == "rays_d":
            assert float((hip[k] - w).abs().max()) <= RAYS_D_TOL
        elif k == "images":
            assert float((hip[k] - w).abs().max()) <= 2 * 2.0 ** -24
        else:
            assert torch.equal(hip[k], w), k


def test_byte_and_float_tables_agree(hip_lib, cuda):
    """The 1-byte forms of the tables (bool weights of the incoherent-mask
    draw, uint8 images) against the float32 forms of the same values."""
    from samnerf_amd import batch
    ph = batch.PhiloxBatch(SEED, 70)
    t = tables()
    H, W, _ = hwm()
    inc = t["gt_incoherent_masks"].cuda()
    draws = [batch.hip_draw(batch.MODE_C, 3, H, W, 3, device=cuda, patch=4, M=H, weights=w, rows=[0, 2, 1], philox=ph)
             for w in (inc, inc.float(), inc.to(torch.uint8))]
    _eq(draws[0], draws[1])
    _eq(draws[0], draws[2])
    assert bool(inc[torch.tensor([0, 2, 1], device=cuda), draws[0]["cells"]].all())
    _, gpu = _sources(4)
    as_float = make_source("cuda", images=t["images"].float().cuda(),
                           incoherent_masks=t["gt_incoherent_masks"].float().cuda())
    index, pixels = _rays(65, H, W, 9)
    a = batch.hip_gather(gpu, index.cuda(), pixels.cuda(), H, W, coarse_size=128)
    b = batch.hip_gather(as_float, index.cuda(), pixels.cuda(), H, W, coarse_size=128)
    for k in a:
        assert torch.equal(a[k].float(), b[k].float()), k
