"""tests/rgb_train_ref.py without a GPU: every case of
tests/test_gpu_rgb_train_rows.py meets the conditions it is there for
(computed from the two CPU twins alone, at their own bins), the fp32 twin
passes compare() against float64 in the kernels' place, and compare() names
the level and row of three planted errors -- one row off by 1e-3, one corner's
contribution added to the neighbouring row, a value in a row nothing reaches.
"""
import numpy as np
import pytest
import torch

import grid_ref
import rgb_train_ref as R


@pytest.fixture(params=list(R.CASES))
def case(request, oracle_lib):
    return R.get_case(request.param)


def _self_compare(case, probe):
    t = case.twins()
    return R.compare(t["g32"][probe], t["g32"][probe], t["g64"][probe], case.model)


def test_case_conditions(case):
    """What each case is there for (see CASES and the GPU module's docstring),
    and for every case: rows nothing reaches on every hashed level that has
    more rows than the batch has corners, and an fp32 twin within 1e-2 of
    float64 in every unit of every probe (a unit beyond that is
    ill-conditioned at this input: change the input, do not exclude it)."""
    t, name = case.twins(), case.spec.name
    S = 32 * case.n
    for probe in case.spec.probes:
        r = _self_compare(case, probe)
        assert r.cpu_worst() < 1e-2, (probe, max(r.per_unit, key=lambda u: u[2]))
        assert np.isfinite([u[2] for u in r.per_unit]).all()
    zeros = R.zero_rows_per_level(case, "image", R.GRID_NAMES[0])
    for l, (rows, res, hashed) in enumerate(R.level_kinds(case, R.GRID_NAMES[0])):
        if hashed and rows > 8 * S:
            assert zeros[l] > 0, l
    if name.startswith("fog"):
        k = case.replicated_levels(R.GRID_NAMES[0])
        assert 0 < k < 16, k
        assert abs(t["fwd64"]["weights_sum"] - 1).max() < 1e-12          # 'last_sample'
    if name == "prop18":
        for p in (1, 2):
            assert 0 < case.replicated_levels(R.GRID_NAMES[p]) < 5
    else:
        assert all(case.replicated_levels(R.GRID_NAMES[p]) == 5 for p in (1, 2))
    if name == "short37":
        assert R.rays_in_one_cell(case, stage=1, level=0) >= 1
    if name == "edge37":
        assert R.last_cell_samples(case, 1e-3) >= 100
    if name == "white37":
        assert t["fwd64"]["weights_sum"].min() < 0.5
    if name == "surface16":
        # float64 never underflows here, so only each ray's last sample
        # (delta * sigma = +inf: no gradient) has an exactly zero contribution
        # there; the saturation shows in fp32, where weights behind the
        # surface are exactly 0 (expf underflow): the kernels' isfinite / zero
        # paths.  And the hashed levels, which the sphere's routing keeps out
        # of the density, are whole units with an identically zero gradient.
        assert int((t["dfeat64"]["weights"] == 0).all(axis=1).sum()) >= case.n
        assert int((t["fwd32"]["weights"] == 0).sum()) > 0
        r = _self_compare(case, "weights")
        assert r.checked < 22
    if case.spec.perturb:
        b0 = case.draws[0].numpy()
        lin = np.linspace(0, 1, 129, dtype=np.float32)
        assert (b0 != lin).any() and (np.abs(b0 - lin) <= 0.5 / 128 + 1e-6).all()
        # the twins marched at exactly these stage-0 bins: the recorded stage-0
        # positions are a function of them alone
        assert t["rec"][0].shape == (case.n * 128, 3)


def test_fp32_twin_passes_in_the_kernels_place(case):
    for probe in case.spec.probes:
        r = _self_compare(case, probe)
        assert r.ok, (probe, r.violations, r.worst)
        assert r.ratio <= 0.5 + 1e-12                      # err / max(2 err, 1e-5)
    rows = R.compare_forward(t := case.twins()["fwd32"], t, case.twins()["fwd64"], case.far())
    assert all(ratio <= 0.5 + 1e-12 for _, _, _, ratio in rows), rows


@pytest.fixture
def fog37(oracle_lib):
    return R.get_case("fog37")


def _planted(case, probe="image"):
    t = case.twins()
    g = {k: (None if v is None else v.copy()) for k, v in t["g32"][probe].items()}
    return t, g, t["g64"][probe]


def test_compare_names_a_scaled_row(fog37):
    t, g, g64 = _planted(fog37)
    offs = fog37.tables()[R.GRID_NAMES[0]][1]
    lvl = 7
    row = int(np.argmax(np.abs(g64[R.GRID_NAMES[0]][offs[lvl]:offs[lvl + 1]]).max(axis=1)))
    g[R.GRID_NAMES[0]][offs[lvl] + row] *= np.float32(1.001)
    r = R.compare(g, t["g32"]["image"], g64, fog37.model)
    assert not r.ok and not r.violations
    assert r.worst[0] == f"{R.GRID_NAMES[0]}[L{lvl}]" and r.worst[4] == row, r.worst
    assert 1.001e-3 / 1e-5 >= r.ratio > 1.0


def test_compare_names_a_corner_added_to_the_next_row(fog37):
    """The heaviest corner of the sample with the largest feature gradient at
    hashed level 5, added one row further on: the float64 contribution is the
    corner weight times the float64 feature gradient (dfeat64)."""
    t, g, g64 = _planted(fog37)
    name, lvl = R.GRID_NAMES[0], 5
    _, offs, res = fog37.tables()[name]
    size = int(offs[lvl + 1] - offs[lvl])
    df = t["dfeat64"]["image"][:, 2 * lvl:2 * lvl + 2]
    s = int(np.argmax(np.abs(df).max(axis=1)))
    x = t["rec"][2].numpy()[s:s + 1]
    cell, frac = grid_ref.locate(x, int(res[lvl]), False)
    best = max(range(8), key=lambda c: np.prod([frac[0, d] if (c >> d) & 1 else 1 - frac[0, d] for d in range(3)]))
    w = np.prod([frac[0, d] if (best >> d) & 1 else 1 - frac[0, d] for d in range(3)])
    corner = np.minimum(cell[0] + [(best >> d) & 1 for d in range(3)], int(res[lvl]) - 1)
    row = int(grid_ref.corner_rows(corner[None], int(res[lvl]), size, 0)[0])
    assert row + 1 < size
    contrib = (w * df[s]).astype(np.float32)
    assert np.abs(contrib).max() > 1e-2 * np.abs(g64[name][offs[lvl]:offs[lvl + 1]]).max()
    g[name][offs[lvl] + row] -= contrib
    g[name][offs[lvl] + row + 1] += contrib
    r = R.compare(g, t["g32"]["image"], g64, fog37.model)
    assert not r.ok
    named = [(r.worst[0], r.worst[4])] + [(v[1], v[2]) for v in r.violations]
    assert all(u == f"{name}[L{lvl}]" and rw in (row, row + 1) for u, rw in named), named
    assert r.ratio > 1.0


def test_compare_names_a_value_in_an_unreached_row(fog37):
    t, g, g64 = _planted(fog37)
    name, lvl = R.GRID_NAMES[0], 12
    offs = fog37.tables()[name][1]
    dead = np.flatnonzero((g64[name][offs[lvl]:offs[lvl + 1]] == 0).all(axis=1))
    row = int(dead[len(dead) // 2])
    for value in (np.float32(1e-12), np.float32(-0.0)):
        h = dict(g)
        h[name] = g[name].copy()
        h[name][offs[lvl] + row, 1] = value
        r = R.compare(h, t["g32"]["image"], g64, fog37.model)
        assert not r.ok
        assert [(v[1], v[2]) for v in r.violations] == [(f"{name}[L{lvl}]", row)], r.violations


def test_compare_wants_zero_where_the_loss_does_not_reach(fog37):
    """The image probe does not reach the proposal networks (their gradient is
    None on the twins): None or all +0.0 passes, anything else is named."""
    t, g, g64 = _planted(fog37)
    name = R.GRID_NAMES[1]
    assert g64[name] is None
    g[name] = np.zeros((int(fog37.tables()[name][1][-1]), 2), np.float32)
    assert R.compare(g, t["g32"]["image"], g64, fog37.model).ok
    g[name][5000, 0] = 1e-20
    r = R.compare(g, t["g32"]["image"], g64, fog37.model)
    offs = fog37.tables()[name][1]
    lvl = int(np.searchsorted(offs, 5000, side="right") - 1)
    assert [(v[1], v[2]) for v in r.violations] == [(f"{name}[L{lvl}]", 5000 - int(offs[lvl]))]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_injected_draws_give_the_stage0_bins_bit_for_bit(dtype):
    """The mirror's stage-0 expression under injected_draws returns the queued
    bins themselves, sample_pdf's u the queued u to rounding; a draw left in
    the queue is an error."""
    import nerf.renderer as rr
    from samnerf_amd.fused import perturbed_positions
    torch.manual_seed(3)
    b0, u1, u2 = perturbed_positions(5, [128, 64, 32], "cpu")
    with R.injected_draws((b0, u1, u2)):
        bins = rr.torch.linspace(0, 1, 129, dtype=dtype).unsqueeze(0).expand(5, -1)
        got = (bins + (rr.torch.rand_like(bins) - 0.5) / 128).clamp(0, 1)
        assert type(got) is torch.Tensor and got.dtype == dtype and torch.equal(got, b0.to(dtype))
        for want in (u1, u2):
            T = want.shape[1]
            u = torch.linspace(0.5 / T, 1 - 0.5 / T, steps=T, dtype=dtype).expand(5, T)
            assert ((u + (rr.torch.rand_like(u) - 0.5) / T) - want.to(dtype)).abs().max() < 1e-6
    assert rr.torch is torch
    with pytest.raises(AssertionError, match="not used"):
        with R.injected_draws((b0, u1, u2)):
            pass
    assert rr.torch is torch
