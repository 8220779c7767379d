"""Float64 reference of the RGB training step (csrc/rgb_train.hip), output by
output and level by level.

Three evaluations of the train-mode render (NeRFRenderer.run under grad) per
case, at the same sample positions:
  hip    the kernels, through net.render with fused = True (_FusedRGBTrain);
  cpu32  the reference's op sequence in fp32 on the CPU with the C oracle's
         encoders (oracle_backend.oracle_encoders);
  f64    the same op sequence in float64 at the fp32 run's recorded positions
         (oracle_backend.float64_twin): the "exact" value.
Both twins resample at the HIP path's bins where those are given
(oracle_backend.injected_bins, read through the render's parity taps) and draw
the perturbed positions the kernels drew (injected_draws below).

A probe is a loss on exactly one output -- (image c).sum(), (depth c).sum(),
(weights_sum c).sum(), (weights c).sum() with seeded cotangents c, the
proposal loss, the distortion loss -- so an error in one upstream gradient's
path is not scaled down by a loss weight before it is compared.  compare()
takes one probe's gradients apart into units: a level of a hash table or a
whole MLP weight, each in max norm against its own float64 scale, with the
project's criterion (test_fused_rgb_step_vs_float64_twin: within twice the
fp32 twin's own distance to float64, or 1e-5) applied per unit, and reports
the unit and row that is worst.  Rows (and whole units) whose float64
gradient is exactly zero must hold +0.0 bit for bit.

Nothing here needs a GPU except Case.hip_* (tests/test_gpu_rgb_train_rows.py);
tests/test_rgb_train_ref_cpu.py checks the cases' preconditions and that the
comparison notices planted errors.
"""
import contextlib
import copy
import dataclasses

import numpy as np
import torch

import grid_ref
from helpers import make_net
from oracle import renderer as orc
from oracle import synth
from oracle.encoders import grid_level_resolutions

REP_ROWS = 600000            # rgb_train.hip kRepRows: leading levels ending at or below it scatter into replicas
NUM_STEPS = (128, 64, 32)
PROBES = ("image", "depth", "wsum", "weights", "prop", "dist")
GRID_NAMES = ("grid.embeddings", "prop_encoders.0.embeddings", "prop_encoders.1.embeddings")


@dataclasses.dataclass(frozen=True)
class CaseSpec:
    name: str
    n: int
    grid_log2: int = 16
    prop_log2: int = 10
    background: str = "last_sample"
    perturb: str = ""                  # "", "arrays" (the three arrays of perturbed_positions) or "philox"
    rays: str = "view"                 # first n of a 10 x 10 view | "edge" (test_gpu_sgrid_scatter's edge37)
    clamp: str = ""                    # "", "white" (background_fixtures.near_far) or "short"
    surface: bool = False
    probes: tuple = ("image", "depth", "weights", "prop", "dist")
    rot: int = 6                       # the view's rotation seed
    draw_seed: int = 77                # perturb = "arrays": torch's seed for perturbed_positions


CASES = {c.name: c for c in [
    CaseSpec("fog1", 1), CaseSpec("fog37", 37), CaseSpec("fog100", 100),
    CaseSpec("white37", 37, background="white", clamp="white", probes=PROBES),
    CaseSpec("pert37", 37, perturb="arrays", draw_seed=78), CaseSpec("philox37", 37, perturb="philox"),
    CaseSpec("prop18", 37, prop_log2=18),
    CaseSpec("short37", 37, clamp="short", rot=1),
    CaseSpec("edge37", 37, rays="edge"),
    CaseSpec("surface16", 16, grid_log2=19, prop_log2=17, surface=True,
             probes=("image", "weights", "prop", "dist")),
]}
PHILOX = (20240607, 3)                 # philox37's (seed, offset)


# ------------------------------------------------------------- the draws --

class _Stage0Draw(torch.Tensor):
    """What torch.rand_like returns for the stage-0 bins under injected_draws.
    run_torch forms (bins + (rand - 0.5) / T).clamp(0, 1): every operation on
    the draw gives another draw and the closing clamp gives the injected bins,
    so the twin continues with exactly the array the kernels read (no r can
    reproduce a given fp32 result of that expression bit for bit)."""

    @classmethod
    def __torch_function__(cls, func, types, args=(), kwargs=None):
        src = next(a for a in args if isinstance(a, _Stage0Draw))
        if getattr(func, "__name__", "") == "clamp":
            return src.payload
        return _stage0_draw(src.payload)


def _stage0_draw(payload):
    t = torch.Tensor._make_subclass(_Stage0Draw, torch.empty(0))
    t.payload = payload
    return t


class _TorchWithDraws:
    """The torch module as nerf.renderer sees it under injected_draws: rand_like
    hands out the queued draws, everything else is torch's."""

    def __init__(self, queue):
        self._queue = queue

    def __getattr__(self, name):
        return getattr(torch, name)

    def rand_like(self, like):
        want = self._queue.pop(0).to(dtype=like.dtype, device=like.device)
        assert want.shape == like.shape, (want.shape, like.shape)
        if not self._queue_was_stage0:
            self._queue_was_stage0 = True
            return _stage0_draw(want.contiguous())
        # sample_pdf: u + (r - 0.5) / T with u = `like`; its result is replaced
        # by the injected bins, which must only agree with it to 1e-5
        return (want - like) * like.shape[-1] + 0.5

    _queue_was_stage0 = False


@contextlib.contextmanager
def injected_draws(draws):
    """The mirror renderer's perturb=True draws replaced, in call order, by
    (bins0 [N,129], u1 [N,65], u2 [N,33]) -- perturbed_positions' arrays, or
    what samnerf_perturb_fill gives for a PhiloxPerturb: the stage-0 bins
    become bins0 exactly, sample_pdf's u become u1 / u2 to rounding (its
    output is what oracle_backend.injected_bins replaces).  The mirror's own
    torch.rand_like would draw other numbers under a float64 default dtype."""
    import nerf.renderer as rr
    queue = [d.detach().cpu() for d in draws]
    old = rr.torch
    rr.torch = _TorchWithDraws(queue)
    try:
        yield
        assert not queue, f"{len(queue)} injected draws not used"
    finally:
        rr.torch = old


def philox_draws(seed, offset, n, device=None):
    """The three arrays of PhiloxPerturb(seed, offset) over n rays (CPU fp32):
    samnerf_perturb_fill on a device, samnerf_perturb_host (the same header,
    no GPU) without one."""
    from samnerf_amd import fused
    if device is not None:
        return tuple(t.cpu() for t in fused.perturb_fill(seed, offset, n, NUM_STEPS, device))
    return tuple(torch.from_numpy(np.stack([fused.perturb_host(seed, offset, NUM_STEPS, st, r) for r in range(n)]))
                 for st in range(3))


# -------------------------------------------------------------- the cases --

def _view_rays(n, rot):
    pose, intr = synth.gui_camera(10, 10, rot=synth.random_rotation(rot))
    ro, rd = orc.get_rays(pose, intr, 10, 10)
    return ro[:n].contiguous(), rd[:n].contiguous()


def _edge_rays():
    """test_gpu_sgrid_scatter._rays("edge37"): cameras 40 units out on the +x,
    +y, +z axes (contracted coordinate 2 - 1/40, u = 0.994)."""
    parts = []
    for axis, n in enumerate((13, 12, 12)):
        center = [0.0, 0.0, 0.0]
        center[axis] = -40.0
        pose, intr = synth.gui_camera(4, 4, rot=synth.random_rotation(20 + axis), center=center)
        ro, rd = orc.get_rays(pose, intr, 4, 4)
        parts.append((ro[:n], rd[:n]))
    return torch.cat([p[0] for p in parts]).contiguous(), torch.cat([p[1] for p in parts]).contiguous()


def _as_np(t):
    return None if t is None else t.detach().cpu().numpy()


class Case:
    """One case: its inputs (CPU fp32), seeded cotangents, and -- computed
    once, shared by the tests, never modified -- the twins' forward outputs
    and per-probe gradients.  device: where the HIP path runs (None: twins
    only, at their own bins)."""

    def __init__(self, spec, device=None):
        from background_fixtures import near_far
        self.spec, self.n, self.device = spec, spec.n, device
        n = spec.n
        self.model = synth.ModelSpec(with_sam=False, grid_log2=spec.grid_log2, s_grid_log2=10,
                                     prop_log2=spec.prop_log2)
        if spec.surface:
            self.params = synth.make_surface_params(self.model, seed=3, amp=1.5)
        else:
            self.params = synth.make_params(self.model, seed=12, emb_scale=0.5)
        self.ro, self.rd = _edge_rays() if spec.rays == "edge" else _view_rays(n, spec.rot)
        assert self.ro.shape[0] == n
        g = torch.Generator().manual_seed(1000 + n)
        # drawn here, as float32, outside float64_twin: inside it the default
        # dtype is float64 and the same seed gives other numbers
        self.cot = {"image": torch.randn(n, 3, generator=g, dtype=torch.float32),
                    "depth": torch.randn(n, generator=g, dtype=torch.float32),
                    "wsum": torch.randn(n, generator=g, dtype=torch.float32),
                    "weights": torch.randn(n, 32, generator=g, dtype=torch.float32)}
        self.bg = torch.rand(n, 3, generator=g, dtype=torch.float32) if spec.background != "last_sample" else None
        self.cnf = None
        if spec.clamp == "white":
            self.cnf = near_far(n)
        elif spec.clamp == "short":      # 0.02-long segments: a whole ray inside one coarse cell
            near = torch.linspace(0.3, 2.0, n)
            self.cnf = torch.stack([near, near + 0.02], dim=1).contiguous()
        self.draws = self.philox = None
        if spec.perturb == "arrays":
            from samnerf_amd.fused import perturbed_positions
            torch.manual_seed(spec.draw_seed)
            self.draws = tuple(t.float() for t in perturbed_positions(n, list(NUM_STEPS), "cpu"))
        elif spec.perturb == "philox":
            from samnerf_amd.fused import PhiloxPerturb
            self.philox = PhiloxPerturb(*PHILOX)
            self.draws = philox_draws(*PHILOX, n, device)
        self.names = None
        self._hip_net = self._twins = self._hip_fwd = None
        self._hip_grads = {}

    # ---- the three evaluations
    def net(self, device):
        net = make_net(self.model, self.params, device).train()
        net.opt.background = self.spec.background
        return net

    def _render(self, net, double=False, perturb=None):
        c = (lambda t: None if t is None else t.to(next(net.parameters()).device,
                                                    torch.float64 if double else torch.float32))
        if perturb is None:
            perturb = self.draws is not None
        return net.render(c(self.ro), c(self.rd), staged=False, bg_color=c(self.bg), perturb=perturb,
                          cam_near_far=c(self.cnf), update_proposal=True, return_feats=0)

    def probe_loss(self, out, probe, double=False):
        if probe == "prop":
            return out["proposal_loss"]
        if probe == "dist":
            return out["distort_loss"]
        key = {"image": "image", "depth": "depth", "wsum": "weights_sum", "weights": "weights"}[probe]
        c = self.cot[probe].to(out[key].device, torch.float64 if double else torch.float32)
        return (out[key] * c).sum()

    def _trained(self, net):
        ps = [(k, p) for k, p in net.named_parameters() if p.requires_grad]
        names = [k for k, _ in ps]
        assert self.names in (None, names)
        self.names = names
        return [p for _, p in ps]

    def far(self):
        """Each ray's far plane (what depth is compared relative to)."""
        from nerf.renderer import near_far_from_aabb
        net = self.net("cpu")
        _, fars = near_far_from_aabb(self.ro, self.rd, net.aabb_train, net.min_near)
        fars = fars.reshape(-1)
        return (fars if self.cnf is None else torch.minimum(fars, self.cnf[:, 1])).double().numpy()

    def hip_bins(self):
        """The HIP proposal kernels' resampled bins [N,65], [N,33] for this
        case, through the render's parity taps (the training forward runs the
        same kernels, proposal_forward)."""
        from samnerf_amd.fused import FusedRenderer
        net, d = self.hip_net(), self.device
        pert = self.philox or (tuple(t.to(d) for t in self.draws) if self.draws else False)
        out = FusedRenderer(net).render(self.ro.to(d), self.rd.to(d),
                                        cam_near_far=None if self.cnf is None else self.cnf.to(d), taps=True,
                                        perturb=pert)
        return [out["bins1"].cpu().contiguous(), out["bins2"].cpu().contiguous()]

    def twins(self):
        """-> dict: fwd32 / fwd64 (numpy outputs), g32 / g64 (probe -> name ->
        numpy gradient or None), rec (the recorded encoder inputs: stage 0,
        stage 1, final), dfeat64 (probe -> float64 gradient w.r.t. the final
        grid's features [32 N, 32])."""
        if self._twins is not None:
            return self._twins
        from oracle_backend import float64_twin, injected_bins, oracle_encoders, recorded_bins
        import gridencoder.grid as gg
        cpu = self.net("cpu")
        n64 = copy.deepcopy(cpu).double()
        draws = (lambda: injected_draws(self.draws)) if self.draws is not None else contextlib.nullcontext
        bins = self.hip_bins() if self.device is not None else None
        rec, own = [], []
        res = {"rec": rec}
        with oracle_encoders(record=rec), draws(), \
                (injected_bins(bins) if bins is not None else recorded_bins(own)):
            out = self._render(cpu)
            ps = self._trained(cpu)
            res["fwd32"] = self._forward_np(out)
            res["g32"] = {p: self._grads(self.probe_loss(out, p), ps) for p in self.spec.probes}
        bins = bins if bins is not None else own
        res["bins"] = bins
        feats = []
        with float64_twin(grid_inputs=rec), draws(), injected_bins(bins):
            inner = gg.grid_encode

            def keep(*a, **k):
                f = inner(*a, **k)
                feats.append(f)
                return f
            gg.grid_encode = keep            # float64_twin restores the module's own on exit
            out = self._render(n64, double=True)
            ps = self._trained(n64)
            res["fwd64"] = self._forward_np(out)
            res["g64"], res["dfeat64"] = {}, {}
            for p in self.spec.probes:
                g = self._grads(self.probe_loss(out, p, double=True), ps + [feats[-1]])
                res["dfeat64"][p] = g.pop("_extra0")
                res["g64"][p] = g
        self._twins = res
        return res

    def _forward_np(self, out):
        return {k: out[k].detach().cpu().double().numpy()
                for k in ("image", "depth", "weights_sum", "weights", "proposal_loss", "distort_loss")}

    def _grads(self, loss, tensors):
        gs = torch.autograd.grad(loss, tensors, retain_graph=True, allow_unused=True)
        out = {k: _as_np(g) for k, g in zip(self.names, gs)}
        for i, g in enumerate(gs[len(self.names):]):
            out[f"_extra{i}"] = _as_np(g)
        return out

    # ---- the kernels
    def hip_net(self):
        if self._hip_net is None:
            self._hip_net = self.net(self.device)
            self._hip_net.fused = True
        return self._hip_net

    def hip_render(self):
        """A fresh train-mode forward on the kernels (the autograd Function)."""
        net = self.hip_net()
        pert = self.philox or (tuple(t.to(self.device) for t in self.draws) if self.draws else False)
        with torch.enable_grad():
            out = self._render(net, perturb=pert)
        assert out["image"].requires_grad and out["image"].grad_fn is not None
        return out

    def hip_forward(self):
        if self._hip_fwd is None:
            self._hip_fwd = self._forward_np(self.hip_render())
        return self._hip_fwd

    def hip_backward(self, loss):
        """loss.backward() into cleared .grad -> name -> numpy gradient or None."""
        net = self.hip_net()
        self._trained(net)
        net.zero_grad(set_to_none=True)
        loss.backward()
        torch.cuda.synchronize()
        return {k: _as_np(p.grad) for k, p in net.named_parameters() if k in self.names}

    def hip_grads(self, probe):
        if probe not in self._hip_grads:
            self._hip_grads[probe] = self.hip_backward(self.probe_loss(self.hip_render(), probe))
        return self._hip_grads[probe]

    # ---- geometry of the tables
    def tables(self):
        """name -> (GridSpec, offsets, resolutions)."""
        specs = dict(zip(GRID_NAMES, [self.model.grid] + self.model.prop))
        return {k: (g, g.offsets(), grid_level_resolutions(g.num_levels, g.S, g.base_resolution))
                for k, g in specs.items()}

    def replicated_levels(self, name):
        """How many leading levels of a table scatter into the per-XCD copies
        (rgb_train.hip rep_span): those that end at or below kRepRows."""
        _, offs, _ = self.tables()[name]
        k = 0
        while k < len(offs) - 1 and offs[k + 1] <= REP_ROWS:
            k += 1
        return k


_cases = {}


def get_case(name, device=None):
    key = (name, str(device))
    if key not in _cases:
        _cases[key] = Case(CASES[name], device)
    return _cases[key]


# --------------------------------------------------------- the comparison --

def units(names, model):
    """[(unit name, parameter name, row slice or None)]: one unit per level of
    a hash table, one per MLP weight."""
    specs = dict(zip(GRID_NAMES, [model.grid] + model.prop))
    out = []
    for k in names:
        if k in specs:
            offs = specs[k].offsets()
            out += [(f"{k}[L{l}]", k, slice(int(offs[l]), int(offs[l + 1]))) for l in range(len(offs) - 1)]
        else:
            out.append((k, k, None))
    return out


@dataclasses.dataclass
class Result:
    per_unit: list                 # (unit, err_hip, err_cpu, ratio, worst row)
    violations: list               # (kind, unit, row, detail): exact-zero rules broken
    zero_rows: int                 # grid rows whose float64 gradient is exactly zero
    checked: int                   # units with a non-zero float64 gradient

    @property
    def worst(self):
        return max(self.per_unit, key=lambda u: u[3]) if self.per_unit else ("-", 0.0, 0.0, 0.0, -1)

    @property
    def ratio(self):
        return self.worst[3]

    @property
    def ok(self):
        return not self.violations and self.ratio <= 1.0

    def line(self, case, probe):
        u, eh, ec, r, row = self.worst
        return (f"rgbrow_ratio case={case} probe={probe} unit={u} row={row} hip={eh:.3e} cpu={ec:.3e} "
                f"ratio={r:.4f} zero_rows={self.zero_rows}")

    def cpu_worst(self):
        return max((u[2] for u in self.per_unit), default=0.0)


def _is_pos_zero(x):
    return x.view(np.uint32) == 0


def compare(hip, cpu32, f64, model, allow=None):
    """One probe's gradients, name -> array or None (a tensor the loss does not
    reach), unit by unit in float64.  err(x) = max |x - f64| / max |f64| over
    the unit; ratio = err(hip) / (a max(2 err(cpu32), 1e-5)) with a = 1, or
    allow(unit name) where a test documents why a unit needs more.  A unit
    whose float64 gradient is identically zero, and every table row whose
    float64 gradient is zero in both channels, must be +0.0 on the hip side
    bit for bit; no element is excluded from either check."""
    per_unit, violations, zero_rows, checked = [], [], 0, 0
    for unit, name, rows in units(list(f64), model):
        ref = f64[name]
        got = hip.get(name)
        if ref is None:
            if got is not None:
                if rows is not None:
                    got = got[rows]
                bad = ~_is_pos_zero(got).reshape(len(got), -1).all(axis=1)
                if bad.any():
                    violations.append(("tensor the loss does not reach not +0.0", unit, int(np.argmax(bad)), ""))
            continue
        assert got is not None, f"{name}: no gradient from the kernels"
        assert got.dtype == np.float32 and got.shape == ref.shape and ref.dtype == np.float64
        twin = cpu32[name]
        if rows is not None:
            ref, got, twin = ref[rows], got[rows], twin[rows]
        ref2, got2 = ref.reshape(len(ref), -1), got.reshape(len(got), -1)
        scale = np.abs(ref2).max()
        if rows is not None or scale == 0:
            dead = (ref2 == 0).all(axis=1)
            if rows is not None:
                zero_rows += int(dead.sum())
            bad = dead & ~_is_pos_zero(got2).all(axis=1)
            if bad.any():
                r = int(np.argmax(bad))
                violations.append(("row with a zero float64 gradient not +0.0", unit, r,
                                   f"{int(bad.sum())} such rows; this one holds {got2[r].tolist()}, the fp32 twin "
                                   f"{twin.reshape(ref2.shape)[r].tolist()}, unit scale {scale:.3e}"))
        if scale == 0:
            continue
        checked += 1
        e_hip = np.abs(got2.astype(np.float64) - ref2)
        if not np.isfinite(e_hip).all():
            violations.append(("non-finite gradient", unit, int(np.argmax(~np.isfinite(e_hip).all(axis=1))), ""))
            continue
        eh = e_hip.max() / scale
        ec = np.abs(twin.astype(np.float64).reshape(ref2.shape) - ref2).max() / scale
        a = 1.0 if allow is None else float(allow(unit))
        per_unit.append((unit, float(eh), float(ec), float(eh / (a * max(2.0 * ec, 1e-5))),
                         int(np.argmax(e_hip.max(axis=1)))))
    return Result(per_unit, violations, zero_rows, checked)


def compare_forward(hip, cpu32, f64, far):
    """The six outputs, each in max norm over its elements: image, weights_sum
    and weights absolute, depth relative to its ray's far plane, the two loss
    scalars relative.  -> [(output, err_hip, err_cpu, ratio)], ratio =
    err(hip) / max(2 err(cpu32), 1e-6)."""
    out = []
    for k in ("image", "depth", "weights_sum", "weights", "proposal_loss", "distort_loss"):
        ref = f64[k]
        den = far if k == "depth" else (np.abs(ref) if k.endswith("_loss") and ref != 0 else 1.0)
        eh = float((np.abs(hip[k] - ref) / den).max())
        ec = float((np.abs(cpu32[k] - ref) / den).max())
        out.append((k, eh, ec, eh / max(2.0 * ec, 1e-6)))
    return out


# ------------------------------------------ what a case must be, to count --

def final_samples(case):
    """The final stage's sample positions [32 N, 3] (fp32, as recorded) and the
    float64 weights [32 N]."""
    t = case.twins()
    return t["rec"][2].numpy(), t["fwd64"]["weights"].reshape(-1)


def level_kinds(case, name):
    """Per level of a table: (rows, resolution, hashed)."""
    _, offs, res = case.tables()[name]
    return [(int(offs[l + 1] - offs[l]), int(res[l]), int(res[l]) ** 3 > int(offs[l + 1] - offs[l]))
            for l in range(len(res))]


def zero_rows_per_level(case, probe, name):
    g = case.twins()["g64"][probe][name]
    _, offs, _ = case.tables()[name]
    return [int((g[offs[l]:offs[l + 1]] == 0).all(axis=1).sum()) for l in range(len(offs) - 1)]


def rays_in_one_cell(case, stage=1, level=0):
    """Rays whose consecutive samples of a proposal stage all lie in one cell
    of a level of that stage's table (so all eight corner rows coincide)."""
    x = case.twins()["rec"][stage].numpy()
    _, _, res = case.tables()[GRID_NAMES[1 + stage]]
    cell, _ = grid_ref.locate(x, int(res[level]), False)
    cell = cell.reshape(case.n, -1, 3)
    return int((cell == cell[:, :1]).all(axis=(1, 2)).sum())


def last_cell_samples(case, min_w=1e-3):
    """Final samples of weight above min_w in the last cell of an axis at a
    dense level of the final grid (where min(cell + 1, res - 1) clamps)."""
    x, w = final_samples(case)
    x = x[w > min_w]
    hit = np.zeros(len(x), bool)
    for rows, res, hashed in level_kinds(case, GRID_NAMES[0]):
        if not hashed:
            hit |= (grid_ref.locate(x, res, False)[0] == res - 1).any(axis=1)
    return int(hit.sum())
