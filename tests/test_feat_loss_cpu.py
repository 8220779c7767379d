"""The distillation loss (csrc/feat_loss.hip, samnerf_amd/feat_loss.py) without
a GPU: the per-axis bilinear taps on the host against a float64 evaluation of
the same formula, the C ABI's argument errors, and the torch mirror against
the reference's op sequence (nerf/utils.py:1101-1106)."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

PAIRS = [(64, 64), (49, 64), (66, 64), (5, 16), (7, 12), (16, 5), (12, 7), (1, 3), (3, 1), (3, 2), (37, 100),
         (100, 37)]


def host_taps(L, n_in, n_out):
    i0 = (ctypes.c_uint32 * n_out)()
    i1 = (ctypes.c_uint32 * n_out)()
    l1 = (ctypes.c_float * n_out)()
    assert L.samnerf_bilinear_taps_host(n_in, n_out, i0, i1, l1) == 0, L.samnerf_last_error()
    return np.array(i0, np.int64), np.array(i1, np.int64), np.array(l1, np.float32)


def taps_matrix64(n_in, n_out):
    """The header's formula in float64 as the [n_out, n_in] resize matrix."""
    d = np.arange(n_out, dtype=np.float64)
    src = np.maximum(n_in / n_out * (d + 0.5) - 0.5, 0.0)
    i0 = np.floor(src).astype(np.int64)
    i1 = i0 + (i0 < n_in - 1)
    l1 = src - i0
    m = np.zeros((n_out, n_in))
    np.add.at(m, (np.arange(n_out), i0), 1.0 - l1)
    np.add.at(m, (np.arange(n_out), i1), l1)
    return m


@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_host_taps_match_the_float64_formula(hip_lib, n_in, n_out):
    """Each entry within n_in * 2^-22: a few ulps of src (src < n_in), which
    also covers i0 landing on the other side of an integer src, where almost
    no weight moves.  Rows sum to 1 within 2^-23; taps stay inside the axis."""
    i0, i1, l1 = host_taps(hip_lib, n_in, n_out)
    assert np.all(i0 <= i1) and np.all(i1 <= n_in - 1) and np.all(i0 >= 0)
    assert np.all(i1 - i0 == (i0 < n_in - 1))
    l0 = np.float32(1.0) - l1                              # fp32, as the kernels form it
    m = np.zeros((n_out, n_in))
    rows = np.arange(n_out)
    np.add.at(m, (rows, i0), l0.astype(np.float64))
    np.add.at(m, (rows, i1), l1.astype(np.float64))
    err = np.abs(m - taps_matrix64(n_in, n_out)).max()
    print(f"taps {n_in} -> {n_out}: max entry error {err:.3e} (bound {n_in * 2.0 ** -22:.3e})")
    assert err <= n_in * 2.0 ** -22
    assert np.abs(m.sum(1) - 1.0).max() <= 2.0 ** -23


def test_identity_taps_are_exact(hip_lib):
    """(h, w) == (Hg, Wg): l1 = 0 and i0 = d for every cell."""
    i0, i1, l1 = host_taps(hip_lib, 64, 64)
    assert np.array_equal(i0, np.arange(64)) and not l1.any()


def test_argument_errors_return_codes_and_messages(hip_lib):
    L = hip_lib
    p = ctypes.c_void_p(64)      # never dereferenced: validation fails first
    big = 1 << 40

    def fwd(pred=p, h=4, w=4, gt=p, Hg=4, Wg=4, resized=p, loss=p, ws=p, nbytes=big):
        return L.samnerf_feat_loss_forward(pred, h, w, gt, Hg, Wg, resized, loss, ws, nbytes, None)

    def bwd(gl=p, h=4, w=4, Hg=4, Wg=4, gp=p, ws=p, nbytes=big):
        return L.samnerf_feat_loss_backward(gl, h, w, Hg, Wg, gp, ws, nbytes, None)

    for bad in (0, 1025):
        for k in ("h", "w", "Hg", "Wg"):
            assert fwd(**{k: bad}) == -1 and b"[1, 1024]" in L.samnerf_last_error(), (k, bad)
            assert bwd(**{k: bad}) == -1 and b"[1, 1024]" in L.samnerf_last_error(), (k, bad)
            assert L.samnerf_feat_loss_workspace_size(*[bad if j == k else 4 for j in ("h", "w", "Hg", "Wg")]) == 0
    for k in ("pred", "gt", "loss", "ws"):
        assert fwd(**{k: None}) == -1 and b"null" in L.samnerf_last_error(), k
    for k in ("gl", "gp", "ws"):
        assert bwd(**{k: None}) == -1 and b"null" in L.samnerf_last_error(), k
    assert fwd(nbytes=1) == -3 and b"workspace" in L.samnerf_last_error()
    assert bwd(nbytes=1) == -3 and b"workspace" in L.samnerf_last_error()
    # the vector loads' alignment is an argument error too, not a fault
    assert fwd(pred=ctypes.c_void_p(68)) == -1 and b"aligned" in L.samnerf_last_error()
    # the workspace holds at least the scaled differences [Hg*Wg][256]
    assert L.samnerf_feat_loss_workspace_size(49, 66, 64, 64) >= 64 * 64 * 256 * 4
    assert L.samnerf_feat_loss_workspace_size(1, 1, 1, 1) > 0
    i0 = (ctypes.c_uint32 * 4)()
    l1 = (ctypes.c_float * 4)()
    assert L.samnerf_bilinear_taps_host(0, 4, i0, i0, l1) == -1
    assert L.samnerf_bilinear_taps_host(4, 1025, i0, i0, l1) == -1
    assert L.samnerf_bilinear_taps_host(4, 4, None, i0, l1) == -1 and b"null" in L.samnerf_last_error()


@pytest.mark.parametrize("h,w,Hg,Wg", [(6, 9, 8, 8), (8, 8, 8, 8), (5, 7, 3, 2)])
def test_torch_mirror_is_the_reference_op_sequence(h, w, Hg, Wg):
    from samnerf_amd.feat_loss import feat_loss, torch_feat_loss
    g = torch.Generator().manual_seed(3)
    rows = torch.randn(h * w, 256, generator=g)
    gt = torch.randn(1, 256, Hg, Wg, generator=g)

    def reference(x):
        pred = x.reshape(1, h, w, 256).permute(0, 3, 1, 2).contiguous()
        pred = F.interpolate(pred, gt.shape[2:], mode="bilinear")
        return F.mse_loss(pred, gt, reduction="none").mean(), pred

    a = rows.clone().requires_grad_(True)
    want, want_pred = reference(a)
    want.backward()
    for fn in (torch_feat_loss, feat_loss):            # a CPU tensor takes the torch path
        b = rows.clone().requires_grad_(True)
        loss, pred = fn(b, h, w, gt)
        loss.backward()
        assert torch.equal(loss, want) and torch.equal(pred, want_pred) and torch.equal(b.grad, a.grad)
        loss2, none = fn(rows, h, w, gt, resized=False)
        assert none is None and torch.equal(loss2, want)


def test_shape_errors():
    from samnerf_amd.feat_loss import feat_loss
    gt = torch.zeros(1, 256, 4, 4)
    with pytest.raises(ValueError, match=r"\[h \* w, 256\]"):
        feat_loss(torch.zeros(15, 256), 4, 4, gt)
    with pytest.raises(ValueError, match="gt_samvit"):
        feat_loss(torch.zeros(16, 256), 4, 4, gt[0])
    with pytest.raises(ValueError, match="1024"):
        feat_loss(torch.zeros(1025, 256), 1025, 1, gt)
