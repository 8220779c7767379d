"""csrc/incoherent.hip through samnerf_amd.incoherent, on the GPU.

samnerf_incoherent_masks against the reference's recordings
(tests/golden/incoherent.npz) bit for bit, the bool and the float map: at
sizes sfact divides every product and sum of the chain is exact in fp32
(tests/test_incoherent_cpu.py checks the recordings' float32 and float64 maps
are the same numbers), so there is no tolerance.  The shapes put tile borders
(SAMNERF_INCOHERENT_TILE = 16 coarse cells) and their halos on both axes.

samnerf_incoherent_ids: the ids equal the recording exactly -- the generator
guarantees every pixel's |p_last - sum of the others| >= 1e-3 in float64, or an
exact tie of equal logits -- and pred_mask follows the distance rule of
tests/test_gpu_present.py: d_ref is the distance between the reference's
float32 recording and its float64 evaluation; the kernel is another float32
evaluation of the same formula, so its distance from the float64 evaluation is
bounded by M_REF * d_ref + one float32 ulp of the largest magnitude.

update_incoherent_mask: the table equals the two kernels applied by hand to
per-view renders of the same rays, whatever views_per_launch is.
"""
import copy

import numpy as np
import pytest
import torch

import incoherent_fixtures as fx

pytestmark = pytest.mark.gpu

M_REF = 1.04                                  # tests/test_gpu_present.py's, for its probabilities


# ------------------------------------------------- samnerf_incoherent_masks --

@pytest.mark.parametrize("ci,n,h,w,sfact", fx.mask_cases())
@pytest.mark.parametrize("dtype", [torch.int64, torch.uint8])
@pytest.mark.parametrize("keep", [True, False])
def test_masks_kernel_equals_the_recordings_bit_for_bit(hip_lib, cuda, ci, n, h, w, sfact, dtype, keep):
    from samnerf_amd import incoherent as inc
    m = fx.masks(ci, dtype).to(cuda)
    want_b, want_u = fx.want_bool(ci, n, h, w, sfact, keep), fx.want_map(ci, keep)
    for views in (1, n):                      # one view, and all of them in one launch
        table, fmap = inc._hip_masks(m[:views].contiguous(), views, h, w, sfact, keep, True, True)
        assert table.dtype == torch.bool and fx.same(table, want_b[:views])
        assert fx.same(fmap.view(views, 1, *fx.cells(h, w, sfact, keep)), want_u[:views])
    # the public names
    u = inc.get_incoherent_mask(m[:, None], sfact=sfact, keep_size=keep)
    assert inc.last_path == "hip" and u.is_cuda and fx.same(u, want_u)
    if keep:
        src = m[..., None] if dtype == torch.int64 else m
        assert fx.same(inc.incoherent_table(src, sfact=sfact), want_b) and inc.last_path == "hip"
        if sfact == 2 and dtype == torch.int64:
            assert fx.same(inc.gt_incoherent_masks(src), want_b)


def test_table_alone_and_map_alone(hip_lib, cuda):
    from samnerf_amd import incoherent as inc
    ci, n, h, w, sfact = fx.mask_cases()[3]
    m = fx.masks(ci).to(cuda)
    table, none = inc._hip_masks(m, n, h, w, sfact, True, True, False)
    assert none is None and fx.same(table, fx.want_bool(ci, n, h, w, sfact, True))
    none, fmap = inc._hip_masks(m, n, h, w, sfact, True, False, True)
    assert none is None and fx.same(fmap.view(n, 1, h, w), fx.want_map(ci, True))


@pytest.mark.parametrize("ci,n,h,w,sfact", fx.odd_cases())
def test_an_odd_size_takes_the_mirror_and_says_so(hip_lib, cuda, ci, n, h, w, sfact):
    from samnerf_amd import incoherent as inc
    m = fx.masks(ci).to(cuda)
    got = inc.get_incoherent_mask(m[:, None], sfact=sfact)
    assert inc.last_path == "torch" and got.is_cuda
    assert fx.same(got, inc.torch_get_incoherent_mask(m[:, None], sfact=sfact))
    table = inc.incoherent_table(m, sfact=sfact)
    assert inc.last_path == "torch" and fx.same(table, got.to(torch.bool).view(n, h * w))
    with pytest.raises(RuntimeError, match="divisible by sfact"):
        inc._hip_masks(m, n, h, w, sfact, True, True, False)


# --------------------------------------------------- samnerf_incoherent_ids --

def _ulp(x):
    return float(np.spacing(np.float32(x.abs().max().item())))


def _dist(a, b):
    return float((a.double() - b.double()).abs().max())


@pytest.mark.parametrize("K,n_inst", fx.logit_cases())
@pytest.mark.parametrize("N", [35, 33 * 65])
def test_ids_equal_the_recording_and_pred_mask_is_within_the_references_error(hip_lib, cuda, K, n_inst, N):
    from samnerf_amd import incoherent as inc
    z = fx.logits(K)[:N]
    ids, pred = inc.render_mask_ids(z.to(cuda), n_inst, return_pred=True)
    assert ids.dtype == torch.uint8 and fx.same(ids, fx.t(f"logits/{K}/ids")[:N])
    assert fx.same(inc.render_mask_ids(z.to(cuda), n_inst), ids)               # without pred_mask
    r32, r64 = fx.t(f"logits/{K}/pred32")[:N], fx.t(f"logits/{K}/pred64")[:N]
    assert pred.shape == r32.shape
    d_ref, ulp, err = _dist(r32, r64), _ulp(r64), _dist(pred.cpu(), r64)
    print(f"PRED K={K} N={N}: err={err:.3e} d_ref={d_ref:.3e} ulp={ulp:.3e}")
    assert err <= M_REF * d_ref + ulp, (err, d_ref, ulp)


def test_ids_of_ties_nans_and_infinities(hip_lib, cuda):
    from samnerf_amd import incoherent as inc
    bad = torch.tensor([[0.0, float("nan")], [float("nan"), 5.0], [0.0, float("inf")], [0.0, 5.0], [2.5, 2.5],
                        [5.0, 0.0]])
    assert inc.render_mask_ids(bad.to(cuda), 2).tolist() == [0, 0, 0, 1, 0, 0]
    assert inc.render_mask_ids(bad.to(cuda), 2).tolist() == inc.torch_render_mask_ids(bad, 2).tolist()
    # shaped logits keep their shape; the ids go where `out` says
    z = fx.logits(3)[:2 * 5 * 7].view(2, 5, 7, 3).to(cuda)
    out = torch.full((3, 5, 7), 9, dtype=torch.uint8, device=cuda)
    ids = inc.render_mask_ids(z, 3, out=out[1:])
    assert ids.shape == (2, 5, 7) and fx.same(out[1:].view(-1), fx.t("logits/3/ids")[:70]) and bool((out[0] == 9).all())


# --------------------------------------------------- update_incoherent_mask --

def _mask_net(cuda, n_inst, seed=19):
    """The smallest 'default' mask-head model of the mask-training tests.  Seeds 19 and 6 render both ids in
    every view at S = 8 and 12 (most synthetic seeds render one id everywhere, whose table is all False)."""
    from helpers import make_net
    from oracle import synth
    spec = synth.ModelSpec(with_sam=False, with_mask=True, mask_type="default", n_inst=n_inst, grid_log2=12,
                           prop_log2=10, m_grid_log2=12)
    return make_net(spec, synth.make_params(spec, seed=seed, emb_scale=0.5), cuda)


def _source(cuda, S, with_cnf, H=16):
    from oracle import synth
    from samnerf_amd.batch import BatchSource
    poses = np.stack([synth.gui_camera(H, H, rot=synth.random_rotation(r))[0] for r in (4, 5, 6)])
    intr = np.asarray(synth.gui_camera(H, H, rot=synth.random_rotation(4))[1], np.float32).reshape(1, 4)
    cnf = torch.tensor([[0.3, 1.5], [0.25, 2.5], [0.4, 3.0]], device=cuda) if with_cnf else None
    return BatchSource(torch.from_numpy(poses.astype(np.float32)).to(cuda), torch.from_numpy(intr).to(cuda), H, H,
                       cam_near_far=cnf, incoherent_mask_size=S)


def _opt(net, with_cnf):
    opt = copy.copy(net.opt)
    opt.enable_cam_near_far = with_cnf
    return opt


def _by_hand(net, source, opt, S):
    """One view per render call with collate_mask's [1, 2] cam_near_far, then the two kernels."""
    from samnerf_amd import incoherent as inc
    K = opt.n_inst + opt.redundant_instance
    ids = []
    with torch.no_grad():
        for v in range(source.n_img):
            ro, rd, _ = inc.mask_view_rays(source, v, 1, S, opt)
            cnf = source.cam_near_far[[v]] if opt.enable_cam_near_far else None
            out = net.render(ro, rd, staged=True, bg_color=1, perturb=False, cam_near_far=cnf, return_feats=0,
                             return_mask=True)
            ids.append(inc.render_mask_ids(out["instance_mask_logits"].reshape(S, S, K), opt.n_inst))
    ids = torch.stack(ids, 0)
    return ids, inc.incoherent_table(ids, sfact=2)


def test_mask_view_rays_are_collate_masks(hip_lib, cuda):
    """The fixed-fov full image of each pose, view after view."""
    from samnerf_amd import incoherent as inc, ops
    from samnerf_amd.batch import fixed_fov_intrinsics
    S = 12
    source = _source(cuda, S, True)
    opt = _opt(_mask_net(cuda, 2), True)
    ro, rd, cnf = inc.mask_view_rays(source, 1, 2, S, opt)
    intr = fixed_fov_intrinsics(S, "cpu")[0].numpy()
    for k, v in enumerate((1, 2)):
        wo, wd = ops.get_rays(source.poses[v].cpu().numpy(), intr, S, S, device=cuda)
        sl = slice(k * S * S, (k + 1) * S * S)
        assert torch.allclose(ro[sl], wo, atol=1e-6) and torch.allclose(rd[sl], wd, atol=1e-6)
        assert bool((cnf[sl] == source.cam_near_far[v]).all())
    opt.enable_cam_near_far = False
    assert inc.mask_view_rays(source, 0, 1, S, opt)[2] is None


@pytest.mark.parametrize("S", [8, 12])
@pytest.mark.parametrize("with_cnf", [False, True])
def test_update_equals_the_kernels_by_hand_for_any_views_per_launch(hip_lib, cuda, S, with_cnf):
    from samnerf_amd import incoherent as inc
    net = _mask_net(cuda, 2).train()
    source, opt = _source(cuda, S, with_cnf), _opt(net, with_cnf)
    ids, want = _by_hand(net.eval(), source, opt, S)
    net.train()
    print(f"UPDATE S={S} cnf={with_cnf}: ids==1 {float(ids.float().mean()):.3f}, "
          f"table True {float(want.float().mean()):.3f}")
    assert want.shape == (3, S * S) and want.dtype == torch.bool
    assert bool(want.any()) and not bool(want.all()), "a one-valued table shows little"
    assert source.incoherent_masks is None
    ptr = None
    for per in (1, 2, 3, None):
        table = inc.update_incoherent_mask(net, source, opt, views_per_launch=per)
        assert net.training                               # the mode is restored
        assert table is source.incoherent_masks and source.incoherent_mask_size == S
        assert fx.same(table, want), per
        assert ptr is None or table.data_ptr() == ptr     # a later call writes the same storage
        ptr = table.data_ptr()
    net.eval()
    inc.update_incoherent_mask(net, source, opt)
    assert not net.training and source.incoherent_masks.data_ptr() == ptr


def test_the_sampler_reads_the_replaced_table(hip_lib, cuda):
    import types

    from samnerf_amd import incoherent as inc
    from samnerf_amd.batch import TrainBatchSampler
    S, H = 8, 16
    net_a, net_b = _mask_net(cuda, 2, seed=19), _mask_net(cuda, 2, seed=6)
    source = _source(cuda, S, False, H=H)
    sampler = TrainBatchSampler(source, types.SimpleNamespace(num_rays=512), rng="torch")
    assert "incoherent_masks" not in sampler.sample(1, [0])

    def cells_of(table):
        batch = sampler.sample(1, [0])
        d = sampler.last_draw
        row, col = d["pixels"] // H, d["pixels"] % H
        cell = (row * (S / H)).long() * S + (col * (S / H)).long()
        return batch["incoherent_masks"], table[d["index"], cell]

    first = inc.update_incoherent_mask(net_a, source, _opt(net_a, False)).clone()
    got, want = cells_of(first)
    assert got.dtype == torch.bool and fx.same(got, want)
    second = inc.update_incoherent_mask(net_b, source, _opt(net_b, False))
    assert second is source.incoherent_masks and not torch.equal(first, second), "the two models draw one table"
    got, want = cells_of(second)
    assert fx.same(got, want) and bool(got.any()) and not bool(got.all())


def test_one_instance_gives_an_all_false_table(hip_lib, cuda):
    from samnerf_amd import incoherent as inc
    net = _mask_net(cuda, 1)
    source = _source(cuda, 8, False)
    table = inc.update_incoherent_mask(net, source, _opt(net, False))
    assert table.shape == (3, 64) and not bool(table.any())
