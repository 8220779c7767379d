"""samnerf_amd.mask_loss on the CPU: its torch path is the reference's op
sequence (nerf/utils.py:761-870, :959-1067), so on the golden's inputs
(tests/golden/mask_loss.npz, the reference's own Trainer.train_step) it gives
the recorded float32 loss, gradient and error map exactly, and its float64 run
the float64 ones."""
import pytest
import torch

from mask_loss_fixtures import case_names, golden, load_case, local_incoherence, make_opt


def _run(name, dtype):
    from samnerf_amd.mask_loss import mask_loss
    opt, n, logits, labels, kw, want, cfg = load_case(name, dtype)
    logits.requires_grad_(True)
    loss, terms, ids = mask_loss(logits, labels, n, opt, **kw)
    loss.backward()
    return loss.detach(), logits.grad, kw.get("error_map"), ids, want, terms


@pytest.mark.parametrize("name", case_names())
def test_torch_path_equals_the_reference_float32(name):
    loss, grad, emap, ids, want, terms = _run(name, torch.float32)
    assert torch.equal(loss, want["loss32"]), (float(loss), float(want["loss32"]))
    assert torch.equal(grad, want["grad32"])
    if emap is not None:
        assert torch.equal(emap, want["map32"])
        assert not torch.equal(emap, torch.from_numpy(golden()[f"{name}/error_map"]))
    assert torch.equal(ids, want["pred_ids"])
    assert torch.equal(terms["total"], loss)


@pytest.mark.parametrize("name", case_names())
def test_torch_path_equals_the_reference_float64(name):
    loss, grad, emap, ids, want, _ = _run(name, torch.float64)
    assert loss.dtype == torch.float64
    assert torch.equal(loss, want["loss64"]), (float(loss), float(want["loss64"]))
    assert torch.equal(grad, want["grad64"])
    if emap is not None:
        assert torch.equal(emap, want["map64"])


def test_no_labelled_ray_gives_zero_loss_and_gradient():
    from samnerf_amd.mask_loss import mask_loss
    logits = torch.randn(40, 3, generator=torch.Generator().manual_seed(1), requires_grad=True)
    labels = torch.full((40,), -1, dtype=torch.long)
    loss, terms, ids = mask_loss(logits, labels, 24, make_opt(n_inst=3))
    assert float(loss) == 0.0
    # the reference's loss is then a constant (utils.py:975): no graph at all
    if loss.requires_grad:
        (g,) = torch.autograd.grad(loss, logits, allow_unused=True)
        assert g is None or not g.any()
    assert torch.equal(ids, logits.argmax(-1))


def test_non_mixed_rgb_similarity_raises_like_the_reference():
    """utils.py:1062 calls rgb_similarity_loss without `incoherent`: TypeError."""
    from samnerf_amd.mask_loss import mask_loss
    logits = torch.zeros(16, 2)
    labels = torch.zeros(16, dtype=torch.long)
    opt = make_opt(rgb_similarity_loss_weight=5.0, mixed_sampling=False)
    with pytest.raises(TypeError, match="mixed_sampling"):
        mask_loss(logits, labels, 16, opt, image=torch.zeros(16, 3), global_step=0)
    # before rgb_similarity_iter the term is off and the same call is fine
    opt.rgb_similarity_iter = 10
    mask_loss(logits, labels, 16, opt, global_step=10)


def test_host_errors():
    from samnerf_amd.mask_loss import mask_loss
    labels = torch.zeros(18, dtype=torch.long)
    with pytest.raises(ValueError, match=r"\[2, 32\]"):
        mask_loss(torch.zeros(18, 33), labels, 18, make_opt())
    with pytest.raises(ValueError, match="patch_size >= 2"):
        mask_loss(torch.zeros(18, 2), labels, 18, make_opt(label_regularization_weight=0.1),
                  depth=torch.zeros(18))
    with pytest.raises(ValueError, match="whole 4 x 4 patches"):
        mask_loss(torch.zeros(18, 2), labels, 18, make_opt(label_regularization_weight=0.1, patch_size=4),
                  depth=torch.zeros(18))


def test_coarse_cells_equals_the_reference():
    from samnerf_amd.mask_loss import coarse_cells
    g = golden()
    H, W, size = (int(v) for v in g["coarse/hws"])
    got = coarse_cells(torch.arange(H * W), H, W, size)
    assert torch.equal(got, torch.from_numpy(g["coarse/inds_coarse"]))
    assert got.dtype == torch.int64 and int(got.max()) < size * size


@pytest.mark.parametrize("name", ["script", "script_q256", "no_error_map"])
def test_draw_similarity_samples_equals_the_recorded_draw(name):
    """The reference seeds nothing itself: the golden tool seeds torch's global
    generator with the case's seed right before the step, whose only draw is
    this multinomial."""
    from samnerf_amd.mask_loss import draw_similarity_samples
    inc, cfg = local_incoherence(name)
    torch.manual_seed(cfg["seed"])
    got = draw_similarity_samples(inc, cfg["rgb_similarity_num_sample"])
    assert torch.equal(got, torch.from_numpy(golden()[f"{name}/sample_index"]))
    # only eligible pixels are drawn, except in the patch that has none
    elig = (1. - inc[..., 0].float()) > 0.8
    assert elig[:-1].gather(1, got[:-1]).all() and not elig[-1].any()


def test_c_abi_argument_errors(hip_lib):
    import ctypes

    from samnerf_amd._lib import SamnerfMaskLossArgs
    p = ctypes.c_void_p(64)              # never dereferenced: validation fails first
    a = SamnerfMaskLossArgs()
    a.N, a.K, a.n, a.incoherent_weight, a.epsilon, a.labels = 8, 33, 8, 1.0, 1e-6, 64
    assert hip_lib.samnerf_mask_loss(ctypes.byref(a), p, p, p, p, p, 1 << 20, None) == -1
    assert b"[2, 32]" in hip_lib.samnerf_last_error()
    assert hip_lib.samnerf_mask_loss_workspace_size(ctypes.byref(a)) == 0
    a.K = 4
    need = hip_lib.samnerf_mask_loss_workspace_size(ctypes.byref(a))
    assert need > 8 * 4 * 4
    assert hip_lib.samnerf_mask_loss(ctypes.byref(a), None, p, p, p, p, need, None) == -1
    assert hip_lib.samnerf_mask_loss(ctypes.byref(a), p, p, p, p, p, need - 1, None) == -3
    a.n = 9
    assert hip_lib.samnerf_mask_loss(ctypes.byref(a), p, p, p, p, p, need, None) == -1
    a.n, a.rgb_weight, a.L, a.Q, a.S, a.image, a.sample_index = 4, 1.0, 1, 3, 1, 64, 64
    assert hip_lib.samnerf_mask_loss(ctypes.byref(a), p, p, p, p, p, need, None) == -1
    assert b"n + L * Q" in hip_lib.samnerf_last_error()
