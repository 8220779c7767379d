"""The RGB training step's kernels (csrc/rgb_train.hip, through the train-mode
render's autograd Function) against the float64 twin of tests/rgb_train_ref.py:
one output at a time, and each gradient one table level / one MLP weight at a
time, in max norm.

Per case one pair of CPU twins at the HIP path's own bins and draws (cached),
per probe one fresh forward + backward on the kernels.  A probe is a loss on a
single output with a seeded cotangent, so the backward of depth, weights_sum,
weights and of the distortion term is compared at full weight (the training
loss gives the latter 2 %).  Every unit must be within twice the fp32 CPU
twin's own distance to float64 (or 1e-5): the criterion of
test_fused_rgb_step_vs_float64_twin, here per unit instead of per tensor norm,
so that a wrong row or level is not averaged over the table.  Rows and units
whose float64 gradient is exactly zero must be +0.0 bit for bit.

Cases (rgb_train_ref.CASES; tests/test_rgb_train_ref_cpu.py asserts what each
is there for without a GPU):
  fog1, fog37, fog100   a lone ray (1 of 4 waves of k_rt_prop_ray_w's block, 1
             of 8 half-waves of k_rt_composite_h's), ragged last waves; grid
             2^16: levels 0-2 dense, 11 levels through the per-XCD copies
             (k_rt_rep_sum) and 5 scattered directly
  white37    transparent background, a colour per ray, clamped far planes:
             weights_sum 0.25 .. 0.96, the only family where the weights_sum
             probe means something
  pert37, philox37   perturbed sampling from arrays and from a Philox seed
             (the PHX kernel forms recompute the stage-0 bins in the backward)
  prop18     proposal tables with 4 replicated levels and 1 direct one
  short37    0.02-long segments: whole rays inside one coarse cell, runs of
             equal rows as long as the wave and across waves (scatter_level_c2)
  edge37     samples in the last cell of the dense levels (corner clamp)
  surface16  an opaque sphere at the default table sizes: fp32 weights that
             are exactly zero, units the density does not reach

Under 'last_sample' weights_sum is identically 1 and its exact gradient zero:
both fp32 paths produce rounding noise there (float64 ~1e-16), so that probe
is not compared; the kernels' result must be below 1e-5 of the image probe's
gradient per unit instead.

Each test prints `rgbrow_ratio ...` for its worst unit (pytest -s);
profiles/rgb_train_rows_ratios.txt keeps one run's lines.
"""
import numpy as np
import pytest
import torch

import rgb_train_ref as R

pytestmark = pytest.mark.gpu

CASE_PROBES = [(c.name, p) for c in R.CASES.values() for p in c.probes]
LAST_SAMPLE = [c.name for c in R.CASES.values() if c.background == "last_sample" and not c.surface]

# (probe, unit kind) -> factor on the 2x criterion: the largest ratio measured
# over the cases (profiles/rgb_train_rows_ratios.txt) x 1.5.  Only the proposal
# loss has entries.  Its gradient is -2 x / (w0 + 1e-8) per final interval with
# x = w0 - (cw[hi + 1] - cw[lo]), a difference of nearly equal numbers: x
# carries the absolute error of the cumulative weights cw, ~2^-24 cw, which is
# 1e-5 .. 1e-3 of x on either fp32 path (the twin's own distance to float64 in
# these units is 5e-6 .. 6e-4, against 3e-6 for the other probes).
# k_rt_prop_ray_w forms cw from per-lane chunk sums and a 64-lane
# Hillis-Steele scan, the twin with torch.cumsum's sequential fp32 sum: two
# roundings of the same prefix sums, neither nearer to float64 by
# construction, and a unit's max-norm error is set by the few intervals where
# x is small.  So the ratio of the two errors scatters around 1 (measured 0.1
# .. 3.3 over the cases) instead of staying below 2; the same holds for the
# loss value itself (FORWARD_ALLOW).
ALLOW = {("prop", "prop_encoders.0.embeddings"): 1.8696 * 1.5,
         ("prop", "prop_encoders.1.embeddings"): 1.9336 * 1.5,
         ("prop", "prop_mlp.0.net.0.weight"): 1.6012 * 1.5,
         ("prop", "prop_mlp.0.net.1.weight"): 3.3175 * 1.5,
         ("prop", "prop_mlp.1.net.1.weight"): 1.4238 * 1.5}
FORWARD_ALLOW = {"proposal_loss": 4.1667 * 1.5}


def _allow(probe):
    return lambda unit: ALLOW.get((probe, unit.split("[")[0]), 1.0)


def _report(r, case, probe):
    print(r.line(case, probe))
    for v in r.violations:
        print(f"rgbrow_violation case={case} probe={probe} kind={v[0]!r} unit={v[1]} row={v[2]} {v[3]}")
    for u in sorted(r.per_unit, key=lambda u: -u[3])[1:]:
        if u[3] > 0.5:
            print(f"rgbrow_unit case={case} probe={probe} unit={u[0]} row={u[4]} hip={u[1]:.3e} cpu={u[2]:.3e} "
                  f"ratio={u[3]:.4f}")


@pytest.mark.parametrize("name,probe", CASE_PROBES, ids=[f"{c}-{p}" for c, p in CASE_PROBES])
def test_backward_unit_by_unit(hip_lib, cuda, name, probe):
    """Every unit of one probe's gradients within the criterion (ratio <= 1)
    and the exact-zero rules.  The proposal probe's units carry the allowance
    explained at ALLOW (a cancelling x = w0 - w whose cumulative sums the
    kernel and the twin round differently); no other probe has one."""
    case = R.get_case(name, cuda)
    t = case.twins()
    r = R.compare(case.hip_grads(probe), t["g32"][probe], t["g64"][probe], case.model, _allow(probe))
    _report(r, name, probe)
    assert not r.violations, r.violations
    assert r.ratio <= 1.0, r.worst


@pytest.mark.parametrize("name", list(R.CASES))
def test_forward_output_by_output(hip_lib, cuda, name):
    """image, depth (relative to the ray's far plane), weights_sum, weights and
    the two loss scalars (relative), each in max norm: within twice the fp32
    twin's distance to float64, or 1e-6."""
    case = R.get_case(name, cuda)
    t = case.twins()
    rows = R.compare_forward(case.hip_forward(), t["fwd32"], t["fwd64"], case.far())
    for k, eh, ec, ratio in rows:
        print(f"rgbrow_forward case={name} output={k} hip={eh:.3e} cpu={ec:.3e} ratio={ratio:.4f}")
    assert all(np.isfinite(v).all() for v in case.hip_forward().values())
    assert all(ratio <= FORWARD_ALLOW.get(k, 1.0) for k, _, _, ratio in rows), rows


@pytest.mark.parametrize("name", LAST_SAMPLE)
def test_weights_sum_probe_is_noise_under_last_sample(hip_lib, cuda, name):
    case = R.get_case(name, cuda)
    noise, image = case.hip_grads("wsum"), case.hip_grads("image")
    worst = ("-", 0.0)
    for unit, k, rows in R.units(case.names, case.model):
        if image[k] is None:
            assert noise[k] is None, k
            continue
        a, b = (x[k] if rows is None else x[k][rows] for x in (noise, image))
        assert np.isfinite(a).all()
        ratio = float(np.abs(a).max() / np.abs(b).max()) if np.abs(b).max() > 0 else float(np.abs(a).max() > 0)
        worst = max(worst, (unit, ratio), key=lambda u: u[1])
        assert ratio < 1e-5, (unit, ratio)
    print(f"rgbrow_noise case={name} unit={worst[0]} wsum_over_image={worst[1]:.3e}")


def _sum64(parts):
    out = {}
    for k in parts[0]:
        have = [p[k].astype(np.float64) for p in parts if p[k] is not None]
        out[k] = sum(have) if have else None
    return out


def test_upstream_gradients_add_up(hip_lib, cuda):
    """fog37, one backward with all six upstream gradients set (g_img, g_ws,
    g_depth, g_w, g_loss together) against the six single-probe backwards:
    per unit, the joint gradient is within the criterion of float64 (the sum
    of the twins' probes; the weights_sum probe's exact gradient is zero), and
    it differs from the sum of the kernels' own six by no more than that
    bound -- they do not disturb each other."""
    case = R.get_case("fog37", cuda)
    t = case.twins()
    out = case.hip_render()
    joint = case.hip_backward(sum(case.probe_loss(out, p) for p in R.PROBES))
    singles = _sum64([case.hip_grads(p) for p in R.PROBES])
    f64 = _sum64([t["g64"][p] for p in case.spec.probes])
    c32 = {k: None if v is None else v.astype(np.float32)
           for k, v in _sum64([t["g32"][p] for p in case.spec.probes]).items()}
    r = R.compare(joint, c32, f64, case.model, _allow("prop"))   # the proposal tensors: that probe alone
    _report(r, "fog37", "all6")
    assert r.ok, (r.violations, r.worst)
    by_unit = {u[0]: u for u in r.per_unit}
    worst = ("-", 0.0)
    for unit, k, rows in R.units(case.names, case.model):
        a, b, ref = (x[k] if rows is None else x[k][rows] for x in (joint, singles, f64))
        ratio = float(np.abs(a.astype(np.float64) - b).max() / np.abs(ref).max()) / \
            max(2 * by_unit[unit][2] if unit in by_unit else 0.0, 1e-5)
        worst = max(worst, (unit, ratio), key=lambda u: u[1])
    print(f"rgbrow_linearity case=fog37 unit={worst[0]} ratio={worst[1]:.4f}")
    assert worst[1] <= 1.0, worst


def test_second_backward_on_one_forward(hip_lib, cuda):
    """rt_backward only reads what the forward left in the workspace (the
    per-stage d(ds) included: k_rt_prop_bwd scales it by g_loss on the fly) and
    overwrites its own scratch and the gradients, and _FusedRGBTrain keeps
    the workspace in ctx.state: a second backward under retain_graph=True is
    supported.  It gives the MLP gradients (fixed-order slab sums) bit for bit
    and the table gradients (float atomics) to rounding, as a fresh forward +
    backward does."""
    case = R.get_case("fog37", cuda)
    net = case.hip_net()

    def loss_of(out):
        return case.probe_loss(out, "image") + case.probe_loss(out, "weights") + \
            case.probe_loss(out, "prop") + case.probe_loss(out, "dist")

    def grads(loss, **kw):
        net.zero_grad(set_to_none=True)
        loss.backward(**kw)
        torch.cuda.synchronize()
        return {k: p.grad.detach().cpu().numpy().copy() for k, p in net.named_parameters() if p.grad is not None}

    loss = loss_of(case.hip_render())
    first = grads(loss, retain_graph=True)
    # scribble over freed blocks: a backward that relied on anything but the
    # workspace and its inputs would see it
    junk = [torch.full((1 << 20,), float("nan"), device=cuda) for _ in range(4)]
    del junk
    second = grads(loss)
    fresh = grads(loss_of(case.hip_render()))
    assert set(first) == set(second) == set(fresh) and len(first) == 13
    for k in first:
        for other in (second, fresh):
            if "mlp" in k:
                assert np.array_equal(first[k].view(np.uint32), other[k].view(np.uint32)), k
        for unit, _, rows in R.units([k], case.model):
            a, b, c = (x[k] if rows is None else x[k][rows] for x in (first, second, fresh))
            scale = float(np.abs(a).max())
            assert scale > 0 and np.abs(a - b).max() <= 1e-5 * scale and np.abs(a - c).max() <= 1e-5 * scale, unit
