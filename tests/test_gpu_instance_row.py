"""One instance row, four entry points (csrc/instance_row.h): present_frame,
eval_frame, render_mask_ids and mask_loss turn the same logits into the same
probabilities and the same argmax, bit for bit.

300 rows (one full 256-row chunk and a ragged 44) of 2 * randn logits with a
few rows overwritten: all columns equal, an exact two-way tie for the maximum,
one +inf, one NaN (the last two give NaN probabilities in every kernel, and NaN
counts as equal to NaN).  mask_loss's ids are compared on the finite rows, with
present's and evaluate's K-way ids (and with render_mask_ids' two-way ids where
K == 2 makes them the same thing)."""
import pytest
import torch

import mask_loss_fixtures as mlfx
import present_fixtures as pfx
from golden_file import same

pytestmark = pytest.mark.gpu

H, W = 12, 25
ALL_EQUAL, TIE, TIE_RAGGED, INF, NAN = 3, 70, 260, 150, 299


def _logits(K):
    z = 2 * torch.randn(H * W, K, generator=torch.Generator().manual_seed(100 + K))
    z[ALL_EQUAL] = 0.75
    for row in (TIE, TIE_RAGGED):
        z[row, 0] = z[row, K - 1] = z[row].max() + 1
    if K > 1:
        z[INF, 1] = float("inf")
    else:
        z[INF, 0] = float("inf")
    z[NAN, 0] = float("nan")
    return z.view(H, W, K)


def _present(cuda, z, n_inst):
    from samnerf_amd.present import present_frame
    _, extra = present_frame(torch.zeros(H, W, 3, device=cuda), None, H, W, logits=z.to(cuda), n_inst=n_inst,
                             mask_type="mask", instance_id=-1, color_map=pfx.t("color_map").to(cuda),
                             return_extra=True)
    return extra["probs"].cpu(), extra["ids"].cpu()


def _evaluate(cuda, z, n_inst):
    from samnerf_amd.evaluate import eval_frame
    labels = torch.arange(H * W, dtype=torch.int64).view(H, W) % z.shape[-1]
    r = eval_frame(logits=z.to(cuda), labels=labels.to(cuda), n_inst=n_inst)
    return r["probs"].cpu(), r["ids"].cpu()


def _incoherent(cuda, z, n_inst):
    from samnerf_amd.incoherent import render_mask_ids
    ids, pred = render_mask_ids(z.to(cuda), n_inst, return_pred=True)
    return ids.cpu(), pred.cpu()


@pytest.mark.parametrize("K", [2, 5, 32])
def test_one_row_four_entry_points(hip_lib, cuda, K):
    from samnerf_amd.mask_loss import mask_loss
    z = _logits(K)
    probs, ids = _present(cuda, z, K)
    eprobs, eids = _evaluate(cuda, z, K)
    assert probs.shape == (H, W, K) and same(probs, eprobs) and same(ids, eids)
    assert torch.isnan(probs.view(-1, K)[[INF, NAN]]).all() and not torch.isnan(probs.view(-1, K)[ALL_EQUAL]).any()
    assert ids.view(-1)[ALL_EQUAL] == 0 and ids.view(-1)[TIE] == 0 and ids.view(-1)[TIE_RAGGED] == 0

    iids, pred = _incoherent(cuda, z, K)
    assert same(pred[..., 1], probs[..., K - 1])
    assert same(iids, pred.argmax(-1).to(torch.uint8))

    N = H * W
    labels = (torch.arange(N, dtype=torch.int64) % K).to(cuda)
    opt = mlfx.make_opt(n_inst=K, num_rays=N)
    _, _, lids = mask_loss(z.view(N, K).to(cuda), labels, N, opt)
    finite = torch.isfinite(z.view(N, K)).all(-1)
    assert int(finite.sum()) == N - 2
    assert same(lids.cpu().view(-1)[finite], ids.view(-1)[finite])
    if K == 2:
        assert same(lids.cpu().view(-1)[finite].to(torch.uint8), iids.view(-1)[finite])


def test_one_sigmoid_three_entry_points(hip_lib, cuda):
    z = _logits(1)
    probs, ids = _present(cuda, z, 1)
    eprobs, eids = _evaluate(cuda, z, 1)
    assert probs.shape == (H, W, 1) and same(probs, eprobs) and same(ids, eids)
    iids, pred = _incoherent(cuda, z, 1)
    assert same(pred, probs) and not iids.any()
