"""bench.py's roofline object (the bench contract's `roofline`): on the
committed PMC rates (profiles/pmc_rates.json) and a synthetic set of stage
times, the dominant stage carries bound / achieved / peak / unit / frac /
traffic with frac = achieved / peak, and every stage entry has a bound.
Host logic only: no GPU.  Below it, bench.py's --dump-outputs writer (host)
and one plain run of the command line on the GPU."""
import os
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def test_roofline_fields_and_ratio():
    import bench
    rates = bench.pmc_rates()
    if not rates:
        pytest.skip("no committed PMC rates")
    stage_avg = {"prop0": 0.556, "prop1": 0.293, "final": 0.705, "s_grid": 0.628, "sam_head": 0.514}
    roof, stages = bench.rooflines(stage_avg, 512 * 512, 0, rates, timed_clock={"ghz": 2.2})
    assert roof["kernel"] == "final"
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in roof and roof[k] is not None, k
    assert roof["frac"] == pytest.approx(roof["achieved"] / roof["peak"])
    assert 0.0 < roof["frac"] < 1.5
    assert roof["timed_clock_ghz"] == 2.2
    assert set(stages) == set(stage_avg)
    for st, e in stages.items():
        assert "bound" in e and e["frac"] > 0, st


def test_dump_outputs_writes_float32_and_samples_large_outputs(tmp_path):
    """--dump-outputs: every floating output of the view as <name>.npy in
    float32; one above DUMP_MAX_BYTES as the same sorted sample of its rows on
    every call; non-tensor and integer entries are not outputs."""
    import numpy as np
    import torch
    import bench
    n = 2 * bench.DUMP_MAX_BYTES // (4 * 256) + 3             # samvit just over twice the cap
    g = torch.Generator().manual_seed(0)
    out = {"image": torch.rand(n, 3, generator=g), "depth": torch.rand(n, generator=g).double(),
           "samvit": torch.rand(n, 256, generator=g), "_workspace": (1, 2), "tap_rays": torch.arange(4)}
    bench.dump_outputs(out, str(tmp_path / "a"))
    bench.dump_outputs(out, str(tmp_path / "b"))
    assert sorted(os.listdir(tmp_path / "a")) == ["depth.npy", "image.npy", "samvit.npy"]
    got = {k: np.load(tmp_path / "a" / f"{k}.npy") for k in ("image", "depth", "samvit")}
    assert all(a.dtype == np.float32 for a in got.values())
    assert np.array_equal(got["image"], out["image"].numpy())
    assert np.array_equal(got["depth"], out["depth"].float().numpy())
    rows = bench.DUMP_MAX_BYTES // (4 * 256)
    assert got["samvit"].shape == (rows, 256) and got["samvit"].nbytes <= bench.DUMP_MAX_BYTES
    keep = np.sort(np.random.default_rng(0).choice(n, rows, replace=False))
    assert np.array_equal(got["samvit"], out["samvit"].numpy()[keep])
    assert np.array_equal(got["samvit"], np.load(tmp_path / "b" / "samvit.npy"))


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_the_last_view(tmp_path):
    """A plain `bench.py --gpus 1 --steps N --warmup W` (a small view) prints
    one result line with the headline fields and none of --full's, really
    times N steps, and --dump-outputs leaves the view's outputs."""
    import json
    import subprocess
    import numpy as np
    d = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "3",
                        "--warmup", "1", "--H", "64", "--W", "64", "--dump-outputs", str(d)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    rec = json.loads(lines[0])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in rec, k
    assert rec["steps"] == 3 and rec["full"] is False
    assert rec["value"] == pytest.approx(64 * 64 / (rec["ms_per_step"] * 1e-3))
    for k in ("roofline", "stage_ms", "reference_equivalent_gpu", "parity_vs_ref", "cfg2_rgb", "rgb_train"):
        assert k not in rec, k
    assert rec["cpu_baseline"] is None
    shapes = {"image": (4096, 3), "depth": (4096,), "weights_sum": (4096,), "samvit": (4096, 256)}
    assert sorted(os.listdir(d)) == sorted(k + ".npy" for k in shapes)
    for k, sh in shapes.items():
        a = np.load(d / (k + ".npy"))
        assert a.dtype == np.float32 and a.shape == sh and np.isfinite(a).all(), k
