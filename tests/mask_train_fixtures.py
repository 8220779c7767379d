"""Shared inputs and references of the mask-head training tests
(tests/test_gpu_mask_train_shapes.py on the GPU, tests/test_mask_cpu.py
without one): ragged ray batches with a per-ray cam_near_far, the float64
twin of mask_train_step, and the m_grid level slices."""
import contextlib
import copy

import torch

from oracle import synth


def ragged_batch(n_rays, n_inst, rot=4, seed=None):
    """The first n_rays rays of a 16 x 16 camera, a per-ray cam_near_far drawn as
    test_gpu_rgb_train.py::test_fused_rgb_step_ragged_batches draws it, and
    labels in [0, n_inst); all on the CPU."""
    from oracle import renderer as orc
    pose, intr = synth.gui_camera(16, 16, rot=synth.random_rotation(rot))
    ro, rd = orc.get_rays(pose, intr, 16, 16)
    ro, rd = ro[:n_rays].contiguous(), rd[:n_rays].contiguous()
    g = torch.Generator().manual_seed(n_rays if seed is None else seed)
    gt = torch.randint(0, n_inst, (n_rays,), generator=g)
    cnf = torch.stack([torch.full((n_rays,), 0.3), 0.8 + 2 * torch.rand(n_rays, generator=g)], -1)
    return ro, rd, gt, cnf


def twin_step(cpu, ro, rd, gt, cnf=None, bins=None, record=None):
    """mask_train_step of the fp32 CPU twin (the reference's op sequence with
    autograd and the C oracle's encoders), at the given bins, with backward.
    Returns (loss, the clamped probability of each ray's label)."""
    from oracle_backend import injected_bins, oracle_encoders
    from samnerf_amd.train import mask_train_step
    seen = []
    render = cpu.render

    def keep(*a, **k):
        out = render(*a, **k)
        seen.append(out["instance_mask_logits"].detach())
        return out
    cpu.render = keep
    try:
        with oracle_encoders(record=record), injected_bins(bins) if bins else contextlib.nullcontext():
            _, loss = mask_train_step(cpu, ro, rd, gt, cam_near_far=cnf)
            loss.backward()
    finally:
        del cpu.render
    probs = torch.softmax(seen[0].double(), -1).view(-1, cpu.opt.n_inst)
    return loss, probs.gather(-1, gt.view(-1, 1))[:, 0]


def assert_not_vacuous(cpu, label_probs):
    """Every reference gradient is non-zero and no label's probability is
    clamped (utils.py:962: a clamped row has zero gradient, and a comparison of
    zeros passes whatever the kernels do)."""
    eps = float(cpu.opt.epsilon)
    assert bool(((label_probs > eps) & (label_probs < 1 - eps)).all()), label_probs
    norms = {k: float(p.grad.norm()) for k, p in cpu.named_parameters() if p.grad is not None}
    assert norms and all(v > 0 for v in norms.values()), norms


def float64_twin_errors(nets_fp32, cpu, ro, rd, gt, cnf=None, bins=None):
    """Relative gradient errors of each fp32 network (its .grad filled by the
    caller) and of the fp32 CPU twin against a float64 twin of mask_train_step
    (oracle_backend.float64_twin: the reference's op sequence in float64 at the
    fp32 twin's own recorded sample positions), both twins at `bins`; the
    mask-step form of test_gpu_rgb_train.py::_float64_twin_errors.  Returns
    (errors[name][tensor], float64 loss, fp32 twin loss)."""
    from oracle_backend import float64_twin, injected_bins
    from samnerf_amd.train import mask_train_step
    n64 = copy.deepcopy(cpu).double()
    rec = []
    loss_c, _ = twin_step(cpu, ro, rd, gt, cnf, bins, record=rec)
    assert rec, "no encoder call recorded"
    with float64_twin(grid_inputs=rec), injected_bins(bins) if bins else contextlib.nullcontext():
        _, loss64 = mask_train_step(n64, ro.double(), rd.double(), gt,
                                    cam_near_far=None if cnf is None else cnf.double())
        loss64.backward()
    errs = {}
    for name, net in list(nets_fp32.items()) + [("cpu_fp32", cpu)]:
        e = {}
        for (k, a), (_, b) in zip(net.named_parameters(), n64.named_parameters()):
            if b.grad is None:
                assert a.grad is None, k
                continue
            e[k] = ((a.grad.detach().cpu().double() - b.grad).norm() / b.grad.norm().clamp_min(1e-300)).item()
        errs[name] = e
    return errs, float(loss64.detach()), float(loss_c.detach())


def level_slices(grid):
    """[(level, first row, end row, resolution, dense)] of a GridEncoder from
    its own `offsets` buffer; dense: res^3 <= the level's rows, the reference's
    rule (gridencoder.cu:62-78: strides 1, res, res^2 while the running stride
    fits the table, a hash once it outgrows it)."""
    import numpy as np

    from oracle import encoders as enc
    offs = [int(v) for v in grid.offsets.cpu().tolist()]
    L = len(offs) - 1
    res = enc.grid_level_resolutions(L, float(np.log2(grid.per_level_scale)), int(grid.base_resolution))
    return [(lvl, offs[lvl], offs[lvl + 1], int(res[lvl]), int(res[lvl]) ** 3 <= offs[lvl + 1] - offs[lvl])
            for lvl in range(L)]
