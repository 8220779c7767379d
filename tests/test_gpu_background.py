"""--background white / random and RGB background colours on the fused HIP
paths (render, RGB training, distillation and mask steps).

Every view here is clamped by a per-ray cam_near_far (background_fixtures.
near_far): with the synthetic parameters an unclamped ray is almost opaque and
could not tell the modes apart; with far planes from 0.5 to 4 weights_sum
spreads over 0.25 .. 0.96.  Bounds are those of the tests of the 'last_sample'
paths (test_gpu_render / _fullview / _rgb_train / _train / _mask_train / _n1).
"""
import contextlib
import copy
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from background_fixtures import fixture_net, inputs, near_far, run_kwargs
from conftest import GOLDEN
from helpers import make_net, max_abs
from oracle import renderer as orc
from oracle import synth
from test_gpu_render import TOL, _check_outputs
from test_gpu_rgb_train import GRAD_TOL, _compare_grads, _rays

pytestmark = pytest.mark.gpu


def _no_run_torch(monkeypatch, net):
    def boom(*a, **k):
        raise AssertionError("run_torch called: the fused path did not take this call")
    monkeypatch.setattr(type(net), "run_torch", boom)


def _rgb_net(device, background, seed=12, train=False, fused=True, with_sam=False):
    spec = synth.ModelSpec(with_sam=with_sam, grid_log2=12, s_grid_log2=10, prop_log2=10)
    params = synth.make_params(spec, seed=seed, emb_scale=0.5, ln_jitter=0.1)
    net = make_net(spec, params, device)
    net.opt.background = background
    net.fused = fused
    return net.train(train)


# ---------------------------------------------------------------- goldens --

@pytest.mark.parametrize("head_mode", [0, 1])
@pytest.mark.parametrize("name", ["render_bg_white_rgb", "render_bg_white_sam", "render_bg_white_mask"])
def test_fused_render_matches_reference_background_golden(hip_lib, cuda, monkeypatch, name, head_mode):
    """The reference's own 'white' renders (a [3] colour, SAM features, the
    'default' mask head) through net.render on the fused kernels."""
    fx = np.load(os.path.join(GOLDEN, name + ".npz"))
    net = fixture_net(fx, cuda)
    net.head_mode = head_mode
    _no_run_torch(monkeypatch, net)
    ro, rd, cnf, bg = inputs(fx)                          # bg stays on the CPU: the render moves it
    out = net.render(ro.to(cuda), rd.to(cuda), staged=False, cam_near_far=cnf.to(cuda), bg_color=bg,
                     **run_kwargs(fx))
    ref = {k: torch.from_numpy(fx[k]) for k in ("image", "depth", "weights_sum", "samvit") if k in fx}
    errs = _check_outputs(out, ref)
    if "instance_mask_logits" in fx:
        errs["instance_mask_logits"] = max_abs(out["instance_mask_logits"], fx["instance_mask_logits"])
        assert errs["instance_mask_logits"] < TOL, errs
    print(name, head_mode, errs)


# ------------------------------------------------- weights: exact relations --

@pytest.fixture(scope="module")
def tapped(hip_lib, cuda):
    """32 x 32 clamped rays rendered once per mode with the parity taps."""
    from samnerf_amd.fused import FusedRenderer
    ro, rd = _rays(32, 4, cuda)
    cnf = near_far(1024).to(cuda)
    out = {}
    for mode in ("last_sample", "white"):
        o = FusedRenderer(_rgb_net(cuda, mode)).render(ro, rd, cam_near_far=cnf, taps=True)
        out[mode] = {k: v.cpu().contiguous() for k, v in o.items()}
    return out


def test_modes_differ_only_in_the_last_sample(tapped):
    a, b = tapped["last_sample"], tapped["white"]
    # stage 0 has the same bins in both modes, so the same ds; only the last weight differs
    assert torch.equal(a["ds0"], b["ds0"])
    assert torch.equal(a["w0"][:, :127], b["w0"][:, :127])
    assert not torch.equal(a["w0"][:, 127], b["w0"][:, 127])
    assert torch.equal(a["weights_sum"], torch.ones_like(a["weights_sum"])) or \
        (a["weights_sum"] - 1).abs().max().item() < 1e-6
    ws = b["weights_sum"]
    assert ws.min() < 0.3 and ws.max() > 0.9 and ((ws > 0.3) & (ws < 0.9)).float().mean() >= 0.5


@pytest.mark.parametrize("mode", ["last_sample", "white"])
def test_composited_weights_match_oracle_in_each_mode(tapped, mode):
    o = tapped[mode]
    for st in (0, 1):
        ref = orc.composite_from_ds(o[f"ds{st}"], last_sample=mode == "last_sample")
        err = (o[f"w{st}"] - ref).abs().max().item()
        print(f"{mode} stage {st}: weights max |err| {err:.2e}")
        assert err < 1e-6, (mode, st, err)


@pytest.mark.parametrize("mode", ["last_sample", "white"])
@pytest.mark.parametrize("stage", [0, 1])
def test_prop_indices_bit_exact_in_each_mode(tapped, mode, stage):
    o = tapped[mode]
    if stage == 0:
        bins = torch.linspace(0, 1, 129).unsqueeze(0).expand(1024, -1)
        w, T, gb, gi = o["w0"], 65, o["bins1"], o["inds1"]
    else:
        bins, w, T, gb, gi = o["bins1"], o["w1"], 33, o["bins2"], o["inds2"]
    ref_b, ref_i = orc.sample_pdf(bins, w, T, return_inds=True)
    mism = (gi.long() != ref_i).sum().item()
    assert mism == 0, f"{mode} stage {stage}: {mism} of {ref_i.numel()} indices differ"
    assert torch.equal(gb, ref_b)


# --------------------------------------------- background colour: relations --

@pytest.fixture(scope="module")
def coloured(hip_lib, cuda):
    net = _rgb_net(cuda, "white")
    net.opt.max_ray_batch = 256
    ro, rd = _rays(32, 4, cuda)
    cnf = near_far(1024).to(cuda)
    g = torch.Generator().manual_seed(5)
    c3 = torch.tensor([0.2, 0.5, 0.9])
    per_ray = torch.rand(1024, 3, generator=g)

    def render(bg, **kw):
        with torch.no_grad():
            o = net.render(ro, rd, staged=kw.pop("staged", False), cam_near_far=cnf, bg_color=bg, **kw)
        return {k: v.cpu() for k, v in o.items()}
    return {"net": net, "ro": ro, "rd": rd, "cnf": cnf, "c3": c3, "per_ray": per_ray, "render": render,
            "zero": render(0.0)}


@pytest.mark.parametrize("shape", ["colour", "per_ray"])
def test_background_colour_is_mixed_in_per_channel(coloured, monkeypatch, shape):
    """image_c = image_0 + (1 - weights_sum) * c to two fp32 roundings of
    values below 2 (the product, the sum), depth and weights_sum untouched."""
    _no_run_torch(monkeypatch, coloured["net"])
    c = coloured["c3"] if shape == "colour" else coloured["per_ray"]
    zero, out = coloured["zero"], coloured["render"](c.to(coloured["ro"].device) if shape == "per_ray" else c)
    assert torch.equal(out["depth"], zero["depth"]) and torch.equal(out["weights_sum"], zero["weights_sum"])
    want = zero["image"].double() + (1 - zero["weights_sum"].double()).unsqueeze(-1) * c.double()
    err = (out["image"].double() - want).abs().max().item()
    print(shape, "max |image_c - image_0 - (1 - ws) c| =", err)
    assert err <= 2.0 ** -22, err
    # the colour matters on these rays
    assert (out["image"] - zero["image"]).abs().max().item() > 0.3


def test_scalar_and_grey_colour_agree(coloured):
    a = coloured["render"](0.7)
    b = coloured["render"](torch.tensor([0.7, 0.7, 0.7]))
    c = coloured["render"](torch.tensor([[0.7]]))
    assert torch.equal(a["image"], b["image"]) and torch.equal(a["image"], c["image"])


def test_per_ray_background_follows_the_ray_under_tiling(coloured, cuda):
    """view_width = 32: the kernels run 8 x 4 pixel tiles per wave (slot !=
    ray); the colour is read by ray."""
    from samnerf_amd.fused import FusedRenderer
    fr = FusedRenderer(coloured["net"])
    bg = coloured["per_ray"].to(cuda)
    flat = fr.render(coloured["ro"], coloured["rd"], coloured["cnf"], bg)
    tiled = fr.render(coloured["ro"], coloured["rd"], coloured["cnf"], bg, view_width=32)
    for k in ("image", "depth", "weights_sum"):
        assert torch.equal(flat[k], tiled[k]), k
    assert torch.equal(flat["image"].cpu(), coloured["render"](bg)["image"])


@pytest.mark.parametrize("shape", ["colour", "per_ray"])
def test_staged_render_slices_a_per_ray_background(coloured, monkeypatch, shape):
    _no_run_torch(monkeypatch, coloured["net"])
    bg = coloured["c3"] if shape == "colour" else coloured["per_ray"].to(coloured["ro"].device)
    whole, staged = coloured["render"](bg), coloured["render"](bg, staged=True)      # 4 chunks of 256
    for k in ("image", "depth", "weights_sum"):
        assert torch.equal(whole[k], staged[k]), k


def test_per_ray_background_with_out_tile_raises(coloured, cuda):
    from samnerf_amd.fused import FusedRenderer
    fr = FusedRenderer(coloured["net"])
    tile = torch.empty(1024, 5, device=cuda)
    with pytest.raises(NotImplementedError, match="per-ray background"):
        fr.render(coloured["ro"], coloured["rd"], coloured["cnf"], coloured["per_ray"].to(cuda), out_tile=tile)
    one = fr.render(coloured["ro"], coloured["rd"], coloured["cnf"], coloured["c3"], out_tile=tile)
    assert torch.equal(one["image"].cpu(), coloured["render"](coloured["c3"])["image"])


def test_gui_frame_call_with_a_cpu_colour(hip_lib, cuda, monkeypatch):
    """The reference GUI's frame call (gui.py:80, 304 -> test_step): a [3]
    colour created on the CPU, a 'last_sample' SAM model, staged."""
    net = _rgb_net(cuda, "last_sample", with_sam=True)
    _no_run_torch(monkeypatch, net)
    ro, rd = _rays(16, 3, cuda)
    with torch.no_grad():
        a = net.render(ro, rd, staged=True, bg_color=torch.ones(3), perturb=False, return_feats=False)
        b = net.render(ro, rd, staged=True, bg_color=1, perturb=False, return_feats=False)
    for k in ("image", "depth", "weights_sum"):
        assert torch.equal(a[k], b[k]), k


# ------------------------------------------------------------ RGB training --

def _train_pair(cuda, background, seed=12, twin="cpu", lambda_entropy=1e-3):
    gpu = _rgb_net(cuda, background, seed, train=True)
    other = _rgb_net(cuda if twin == "cuda" else "cpu", background, seed, train=True, fused=False)
    for n in (gpu, other):
        n.opt.lambda_entropy = lambda_entropy
    return gpu, other


def _batch(n, seed):
    """n clamped rays, a per-ray background and an RGBA target (CPU)."""
    ro, rd = _rays(16, 6)
    g = torch.Generator().manual_seed(seed)
    return (ro[:n].contiguous(), rd[:n].contiguous(), near_far(n), torch.rand(n, 3, generator=g),
            torch.rand(n, 4, generator=g))


def _bins(net, ro, rd, cnf, pert=None):
    from samnerf_amd.fused import FusedRenderer
    out = FusedRenderer(net).render(ro, rd, cam_near_far=cnf, taps=True, perturb=pert or False)
    return [out["bins1"].contiguous(), out["bins2"].contiguous()]


def _rel(a, b):
    a, b = (float(torch.as_tensor(x).detach()) for x in (a, b))
    return abs(a - b) / max(abs(b), 1e-12)


def test_fused_rgb_step_random_background_matches_cpu_twin(hip_lib, cuda):
    """samnerf_rgb_train_step under --background random: a colour per ray, an
    RGBA target composited on it, the entropy term live -- image, the loss
    terms and all 11 gradients against autograd of the reference's op sequence
    on the CPU, and each gradient as close to the float64 twin as the fp32 CPU
    twin is (2x, or 1e-5)."""
    from oracle_backend import float64_twin, injected_bins, oracle_encoders
    from samnerf_amd.train import rgb_train_step, rgb_train_step_fused
    gpu, cpu = _train_pair(cuda, "random")
    ro, rd, cnf, bg, gt = _batch(256, 2)
    d = [t.to(cuda) for t in (ro, rd, cnf, bg, gt)]
    bins = [b.cpu() for b in _bins(gpu, d[0], d[1], d[2])]
    img, loss, out = rgb_train_step_fused(gpu, d[0], d[1], d[4], global_step=1, bg_color=d[3],
                                          cam_near_far=d[2], perturb=False)
    n64 = copy.deepcopy(cpu).double()
    rec = []
    with oracle_encoders(record=rec), injected_bins(bins):
        img_c, loss_c, out_c = rgb_train_step(cpu, ro, rd, gt, global_step=1, bg_color=bg, cam_near_far=cnf,
                                              perturb=False)
        loss_c.backward()
    ws = out["weights_sum"].cpu()
    assert ws.min() < 0.3 and ws.max() > 0.9
    assert (img.cpu() - img_c.detach()).abs().max().item() < 1e-5
    assert (ws - out_c["weights_sum"].detach()).abs().max().item() < 1e-5
    wc = out_c["weights_sum"].detach().clamp(1e-5, 1 - 1e-5)
    ent_c = (-wc * torch.log2(wc) - (1 - wc) * torch.log2(1 - wc)).mean()
    terms = {"proposal_loss": (out["proposal_loss"], out_c["proposal_loss"]),
             "distort_loss": (out["distort_loss"], out_c["distort_loss"]),
             "entropy": (out["entropy"], ent_c), "loss": (loss, loss_c)}
    rel = {k: _rel(a, b) for k, (a, b) in terms.items()}
    print("loss terms (hip, cpu, relative):", {k: (float(torch.as_tensor(a).detach()), float(torch.as_tensor(b).detach()), rel[k])
           for k, (a, b) in terms.items()})
    assert max(rel.values()) <= 1e-4, rel
    _compare_grads(gpu, cpu)
    # the term is live: weights_sum is identically 1 under 'last_sample'
    ls = _rgb_net(cuda, "last_sample", train=True)
    ls.opt.lambda_entropy = 1e-3
    _, _, out_ls = rgb_train_step_fused(ls, d[0], d[1], d[4], global_step=1, bg_color=d[3], cam_near_far=d[2],
                                        perturb=False)
    e, e_ls = float(out["entropy"]), float(out_ls["entropy"])
    print("entropy: random", e, "last_sample", e_ls)
    assert e > 0 and abs(e - e_ls) > 1e-3 * abs(e_ls)
    # float64 twin at the fp32 run's sample positions
    with float64_twin(grid_inputs=rec), injected_bins(bins):
        _, loss64, _ = rgb_train_step(n64, ro.double(), rd.double(), gt.double(), global_step=1,
                                      bg_color=bg.double(), cam_near_far=cnf.double(), perturb=False)
        loss64.backward()
    bad = {}
    for (k, pg), (_, pc), (_, p64) in zip(gpu.named_parameters(), cpu.named_parameters(), n64.named_parameters()):
        if p64.grad is None:
            continue
        den = p64.grad.norm().clamp_min(1e-300)
        eh = ((pg.grad.cpu().double() - p64.grad).norm() / den).item()
        ec = ((pc.grad.double() - p64.grad).norm() / den).item()
        print(f"  vs float64  {k:32s} hip {eh:.2e} | cpu fp32 {ec:.2e}")
        if eh > max(2.0 * ec, 1e-5):
            bad[k] = (eh, ec)
    assert not bad, bad


def test_train_mode_render_random_background_autograd(hip_lib, cuda, monkeypatch):
    """net.render in train mode under grad with a per-ray background, then
    loss.backward(): the HIP training kernels through the autograd Function,
    against the torch path at the same bins."""
    from oracle_backend import injected_bins
    a, b = _train_pair(cuda, "random", seed=31, twin="cuda")
    ro, rd, cnf, bg, _ = (t.to(cuda) for t in _batch(256, 4))
    bins = _bins(a, ro, rd, cnf)
    outs = []
    for n in (a, b):
        with injected_bins(bins) if n is b else contextlib.nullcontext(), monkeypatch.context() as mp:
            if n is a:
                _no_run_torch(mp, n)
            o = n.render(ro, rd, staged=False, bg_color=bg, perturb=False, update_proposal=True,
                         return_feats=0, cam_near_far=cnf)
        loss = (o["image"] * torch.linspace(0.5, 1.5, 3, device=cuda)).mean() + 0.3 * o["depth"].mean() \
            + 2.0 * o["weights_sum"].mean() + o["proposal_loss"] + 0.02 * o["distort_loss"]
        loss.backward()
        outs.append((float(loss.detach()), o))
    assert (outs[0][1]["image"] - outs[1][1]["image"]).abs().max().item() < 1e-5
    assert abs(outs[0][0] - outs[1][0]) <= 1e-5 * abs(outs[1][0])
    _compare_grads(a, b)


def test_rgb_step_random_background_seeded_perturb(hip_lib, cuda):
    """PhiloxPerturb under a transparent background: the seeded step equals the
    step on the arrays the seed fills (image and loss terms bit for bit)."""
    from samnerf_amd.fused import PhiloxPerturb, perturb_fill
    from samnerf_amd.train import rgb_train_step_fused
    ro, rd, cnf, bg, gt = (t.to(cuda) for t in _batch(256, 6))
    res = []
    for pert in (PhiloxPerturb(77, 3), perturb_fill(77, 3, 256, [128, 64, 32], cuda)):
        net = _rgb_net(cuda, "random", train=True)
        img, loss, out = rgb_train_step_fused(net, ro, rd, gt, global_step=1, bg_color=bg, cam_near_far=cnf,
                                              perturb=pert)
        res.append((img, loss, out, net))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    for k in ("weights_sum", "depth", "proposal_loss", "distort_loss", "entropy"):
        assert torch.equal(res[0][2][k], res[1][2][k]), k
    ws = res[0][2]["weights_sum"]
    assert ws.min().item() < 0.35 and ws.max().item() > 0.9
    for (k, pa), (_, pb) in zip(res[0][3].named_parameters(), res[1][3].named_parameters()):
        assert torch.isfinite(pa.grad).all(), k
        assert float((pa.grad - pb.grad).norm() / pb.grad.norm().clamp_min(1e-30)) < 1e-5, k


def test_train_forward_matches_reference_random_golden(hip_lib, cuda, monkeypatch):
    """train_bg_random_rgb.npz (the reference's train-mode run under
    'random'): the fused training forward within 1e-5; the per-sample weights
    only where the HIP proposal kernels resample the reference's very bins."""
    from background_fixtures import run_mirror
    from oracle_backend import recorded_bins
    fx = np.load(os.path.join(GOLDEN, "train_bg_random_rgb.npz"))
    net = fixture_net(fx, cuda)
    ro, rd, cnf, bg = (t.to(cuda) for t in inputs(fx))
    with torch.enable_grad(), monkeypatch.context() as mp:
        _no_run_torch(mp, net)
        out = net.render(ro, rd, staged=False, cam_near_far=cnf, bg_color=bg, perturb=False)
    assert out["image"].requires_grad
    got = {k: v.detach().cpu() for k, v in out.items() if torch.is_tensor(v)}
    errs = {k: max_abs(got[k], fx[k]) for k in ("image", "weights_sum")}
    d_ref = torch.from_numpy(fx["depth"])
    errs["depth_rel"] = ((got["depth"] - d_ref).abs() / d_ref.abs().clamp(min=1.0)).max().item()
    for k in ("proposal_loss", "distort_loss"):
        errs[k + "_rel"] = _rel(got[k], float(fx[k]))
    ref_bins = []
    with recorded_bins(ref_bins):
        run_mirror(fx)                                       # bit-equal to the reference (test_background_cpu)
    mine = _bins(net, ro, rd, cnf)
    same = all(torch.equal(a.cpu(), b) for a, b in zip(mine, ref_bins))
    if same:
        errs["weights"] = max_abs(got["weights"], fx["weights"])
    print("train golden:", errs, "bins identical:", same)
    assert max(errs[k] for k in ("image", "weights_sum", "depth_rel")) < 1e-5, errs
    assert errs.get("weights", 0.0) < 1e-5, errs
    assert max(errs["proposal_loss_rel"], errs["distort_loss_rel"]) <= 1e-4, errs


# ------------------------------------------- distillation and mask steps --

def test_distillation_step_white_background_matches_cpu_twin(hip_lib, cuda):
    """One SAM distillation step (fused forward, HIP s_grid scatter, HIP head)
    under 'white': loss and the 13 gradients within 1e-4 of the CPU twin at
    the same bins (test_gpu_train's bound)."""
    from oracle_backend import injected_bins, oracle_encoders
    from samnerf_amd.fused import FusedRenderer
    from samnerf_amd.train import sam_train_step
    nets = {"gpu": _rgb_net(cuda, "white", seed=7, train=True, with_sam=True),
            "cpu": _rgb_net("cpu", "white", seed=7, train=True, with_sam=True, fused=False)}
    for net in nets.values():
        for k, p in net.named_parameters():
            p.requires_grad = k.startswith("s_grid") or k.startswith("samvit_mlp")
    ro, rd = _rays(16, 10)
    cnf = near_far(256)
    gt = torch.randn(1, 256, 16, 16, generator=torch.Generator().manual_seed(1))
    _, lg = sam_train_step(FusedRenderer(nets["gpu"]), ro.to(cuda), rd.to(cuda), 16, 16, gt.to(cuda),
                           cam_near_far=cnf.to(cuda))
    lg.backward()
    bins = [b.cpu() for b in _bins(nets["gpu"], ro.to(cuda), rd.to(cuda), cnf.to(cuda))]
    with oracle_encoders(), injected_bins(bins):
        out = nets["cpu"].run_torch(ro, rd, return_feats=1, cam_near_far=cnf)
        assert out["weights_sum"].min() < 0.3
        pred = out["samvit"].reshape(1, 16, 16, 256).permute(0, 3, 1, 2).contiguous()
        lc = F.mse_loss(F.interpolate(pred, gt.shape[2:], mode="bilinear"), gt, reduction="none").mean()
        lc.backward()
    assert _rel(lg, lc) <= 1e-4, (float(lg), float(lc))
    errs = {}
    for (k, pg), (_, pc) in zip(nets["gpu"].named_parameters(), nets["cpu"].named_parameters()):
        if not pc.requires_grad:
            assert pg.grad is None, k
            continue
        errs[k] = float((pg.grad.cpu() - pc.grad).norm() / pc.grad.norm().clamp_min(1e-12))
    print("distillation gradient relative errors", errs)
    assert len(errs) == 13 and max(errs.values()) < 1e-4, errs


def test_mask_step_white_background_matches_cpu_twin(hip_lib, cuda, monkeypatch):
    """One --with_mask step of the 'default' head under 'white': loss within
    1e-5, gradients of m_grid and mask_mlp within 1e-4 (test_gpu_mask_train)."""
    from oracle_backend import injected_bins, oracle_encoders
    from samnerf_amd.train import mask_train_step
    from test_gpu_mask_train import GRAD_TOL as MASK_TOL
    from test_gpu_mask_train import _grad_errors, _mask_nets
    gpu, cpu = _mask_nets(cuda, n_inst=5, head_mode=1)
    for n in (gpu, cpu):
        n.opt.background = "white"
    ro, rd = _rays(16, 4)
    cnf = near_far(256)
    gt = torch.randint(0, 5, (256,), generator=torch.Generator().manual_seed(3))
    bins = [b.cpu() for b in _bins(gpu, ro.to(cuda), rd.to(cuda), cnf.to(cuda))]
    with monkeypatch.context() as mp:
        _no_run_torch(mp, gpu)
        _, loss = mask_train_step(gpu, ro.to(cuda), rd.to(cuda), gt.to(cuda), cam_near_far=cnf.to(cuda))
    loss.backward()
    with oracle_encoders(), injected_bins(bins):
        _, loss_c = mask_train_step(cpu, ro, rd, gt, cam_near_far=cnf)
        loss_c.backward()
    assert _rel(loss, loss_c) <= 1e-5 + 1e-7 / abs(float(loss_c.detach())), (float(loss), float(loss_c))
    errs = _grad_errors(gpu, cpu)
    print("mask gradient relative errors:", {k: f"{v:.1e}" for k, v in errs.items()})
    assert set(errs) == {"m_grid.embeddings", "mask_mlp.0.net.0.weight", "mask_mlp.0.net.1.weight",
                         "mask_mlp.0.net.2.weight"}, errs
    assert max(errs.values()) <= MASK_TOL, errs


# --------------------------------------------------------------------- N1 --

def test_early_exit_bound_holds_in_transparent_mode(hip_lib, cuda):
    """t_thresh = 1e-3 under 'white' on the opaque-sphere scene: the dropped
    samples' weights sum to at most the remaining transmittance <= t (no last
    sample absorbs the rest), so weights_sum falls by at most t, depth by at
    most t x far, the image stays within test_gpu_n1's bound."""
    from samnerf_amd import synth as psynth
    from samnerf_amd.fused import FusedRenderer
    t = 1e-3
    spec = psynth.ModelSpec(with_sam=False)                 # the sphere lives in the dense levels of full-size tables
    net = make_net(spec, psynth.make_surface_params(spec, seed=3, amp=1.5), cuda)
    net.opt.background = "white"
    ro, rd = _rays(48, 6, cuda)
    bg = torch.tensor([0.1, 0.6, 0.3])
    full = {k: v.cpu() for k, v in FusedRenderer(net, t_thresh=0.0).render(ro, rd, bg_color=bg).items()}
    out = {k: v.cpu() for k, v in FusedRenderer(net, t_thresh=t).render(ro, rd, bg_color=bg).items()}
    _, far = orc.near_far_from_aabb(ro.cpu(), rd.cpu(), torch.tensor([-128.0] * 3 + [128.0] * 3), 0.2)
    errs = {"changed_rays": (out["weights_sum"] != full["weights_sum"]).float().mean().item(),
            "wsum_drop": (full["weights_sum"] - out["weights_sum"]).max().item(),
            "wsum_rise": (out["weights_sum"] - full["weights_sum"]).max().item(),
            "image": max_abs(out["image"], full["image"]),
            "depth_over_far": ((out["depth"] - full["depth"]).abs() / far.reshape(-1)).max().item()}
    print("N1 transparent", t, errs)
    assert errs["changed_rays"] > 0.1, errs
    assert errs["wsum_drop"] <= t * 1.001 + 1e-6 and errs["wsum_rise"] <= 1e-6, errs
    assert errs["image"] <= t + 1e-3, errs
    assert errs["depth_over_far"] <= t * 1.001 + 1e-6, errs


# ---------------------------------------------------------- ragged counts --

@pytest.mark.parametrize("n", [1, 37, 100])
def test_ragged_counts_transparent_per_ray_background(hip_lib, cuda, n):
    """Ray counts that fill no wave, part of one and part of two: the render
    equals the same rays of a larger batch bit for bit; the training step's
    gradients are finite and within GRAD_TOL of the torch path."""
    from oracle_backend import injected_bins
    from samnerf_amd.fused import FusedRenderer
    from samnerf_amd.train import rgb_train_step, rgb_train_step_fused
    ro, rd, cnf, bg, gt = (t.to(cuda) for t in _batch(256, 8))
    fr = FusedRenderer(_rgb_net(cuda, "white"))
    big = fr.render(ro, rd, cnf, bg)
    part = fr.render(ro[:n].contiguous(), rd[:n].contiguous(), cnf[:n].contiguous(), bg[:n].contiguous())
    for k in ("image", "depth", "weights_sum"):
        assert torch.equal(part[k], big[k][:n]), k
    a, b = _train_pair(cuda, "random", seed=17, twin="cuda")
    s = [t[:n].contiguous() for t in (ro, rd, cnf, bg, gt)]
    bins = _bins(a, s[0], s[1], s[2])
    img, loss, _ = rgb_train_step_fused(a, s[0], s[1], s[4], global_step=1, bg_color=s[3], cam_near_far=s[2],
                                        perturb=False)
    with injected_bins(bins):
        img_t, loss_t, _ = rgb_train_step(b, s[0], s[1], s[4], global_step=1, bg_color=s[3], cam_near_far=s[2],
                                          perturb=False)
        loss_t.backward()
    assert all(torch.isfinite(p.grad).all() for p in a.parameters() if p.grad is not None)
    assert (img - img_t.detach()).abs().max().item() < 1e-5
    assert _rel(loss, loss_t) <= 1e-4 + 1e-7 / abs(float(loss_t.detach()))
    _compare_grads(a, b)
