"""What the shared exact-fp32 training core (csrc/mlp_train.h: dense16, the
dW row loop, the packs) must guarantee to both training heads, as bitwise
self-consistency at the smallest shapes where it can go wrong.  No reference
arithmetic is involved, so no tolerance: a row's outputs depend on that row
alone (whatever workgroup, lane and wave it lands in), and rows that carry no
gradient add nothing to a parameter gradient."""

import pytest
import torch

from helpers import make_net
from oracle import synth

pytestmark = pytest.mark.gpu


def _sam_head(cuda):
    from samnerf_amd.fused import FusedRenderer, _head_params
    spec = synth.ModelSpec(with_sam=True, grid_log2=12, s_grid_log2=11, prop_log2=10)
    net = make_net(spec, synth.make_params(spec, seed=15, emb_scale=0.5, ln_jitter=0.3), cuda)
    return FusedRenderer(net), _head_params(net)


def _sam_inputs(cuda, n, seed=5):
    g = torch.Generator().manual_seed(seed)
    rows = (torch.randn(n, 164, generator=g) * torch.rand(1, 164, generator=g) * 3).to(cuda)
    rows[:, 163] = 0.0
    return rows, torch.randn(n, 256, generator=g).to(cuda)


def _sam_step(fr, params, rows, G):
    """samvit, grad_rows and the 12 parameter gradients of one forward + backward."""
    from samnerf_amd.fused import _SamHeadTrain
    r = rows.clone().requires_grad_(True)
    samvit = _SamHeadTrain.apply(r, fr, *params)
    samvit.backward(G)
    grads = [p.grad.clone() for p in params]
    for p in params:
        p.grad = None
    return samvit.detach(), r.grad, grads


def test_sam_head_rows_are_independent(hip_lib, cuda):
    """N = 37: three workgroups, the last with 5 live rows.  The same rows and
    output gradients in reversed order put every row into another workgroup,
    lane and (through the clamped, dropped tiles) beside other pad rows:
    samvit and grad_rows, un-reversed, are the first run's bits."""
    fr, params = _sam_head(cuda)
    rows, G = _sam_inputs(cuda, 37)
    samvit, grows, _ = _sam_step(fr, params, rows, G)
    samvit_r, grows_r, _ = _sam_step(fr, params, rows.flip(0).contiguous(), G.flip(0).contiguous())
    assert torch.isfinite(samvit).all() and float(grows.abs().max()) > 0
    assert torch.equal(samvit_r.flip(0), samvit)
    assert torch.equal(grows_r.flip(0), grows)


@pytest.mark.parametrize("n,n_pad", [(37, 64), (300, 320)])
def test_sam_head_padding_adds_nothing_to_dw(hip_lib, cuda, n, n_pad):
    """Rows n .. n_pad - 1 are copies of row 0 with grad_samvit = 0: they reach
    the dW tiles, the bias sums and the LN partials as zeros, in the same 256-ray
    chunks as the run without them (37 / 64: one chunk; 300 / 320: parts = 2
    and a ragged second chunk), so all 12 parameter gradients and the live
    rows' grad_rows keep their bits."""
    fr, params = _sam_head(cuda)
    rows, G = _sam_inputs(cuda, n)
    _, grows, grads = _sam_step(fr, params, rows, G)
    rows_p = torch.cat([rows, rows[:1].expand(n_pad - n, -1)]).contiguous()
    G_p = torch.cat([G, torch.zeros(n_pad - n, 256, device=cuda)]).contiguous()
    _, grows_p, grads_p = _sam_step(fr, params, rows_p, G_p)
    assert len(grads) == 12
    for i, (a, b) in enumerate(zip(grads, grads_p)):
        assert float(a.abs().max()) > 0 and torch.equal(a, b), i
    assert torch.equal(grows_p[:n], grows)


def test_mask_head_exact_forward_rows_are_independent(hip_lib, cuda):
    """head_mode 1 through the C ABI: the logits of the first 37 rays of an
    N = 48 call are those of an N = 37 call on the same rays.  Rows are
    sample-major (k * N + slot), so the two calls group the samples into
    16-row workgroups differently."""
    from samnerf_amd.fused import FusedRenderer
    from test_gpu_mask_train import _mask_nets
    from test_gpu_mask_train_shapes import _c_abi_step
    from mask_train_fixtures import ragged_batch
    gpu, _ = _mask_nets(cuda, 5, head_mode=1)
    ro, rd, _, _ = ragged_batch(48, 5)
    ro, rd = ro.to(cuda), rd.to(cuda)
    g = torch.randn(48, 5, generator=torch.Generator().manual_seed(9)).to(cuda)
    fr = FusedRenderer(gpu)
    pattern = torch.zeros_like(gpu.m_grid.embeddings)
    lg48, _, _ = _c_abi_step(fr, ro, rd, g, 0xFF, pattern)
    lg37, _, _ = _c_abi_step(fr, ro[:37].contiguous(), rd[:37].contiguous(), g[:37].contiguous(), 0xFF, pattern)
    assert torch.isfinite(lg48).all() and float(lg37.abs().max()) > 0
    assert torch.equal(lg48[:37], lg37)
