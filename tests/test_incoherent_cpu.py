"""samnerf_amd.incoherent without a GPU: the torch mirror against every
recording of tests/golden/incoherent.npz (the reference's own
get_incoherent_mask and its render_mask / update_incoherent_mask lines), the
update's step condition, and the argument errors of the C ABI."""
import ctypes
import types

import pytest
import torch

import incoherent_fixtures as fx


@pytest.mark.parametrize("ci,n,h,w,sfact", fx.mask_cases() + fx.odd_cases())
@pytest.mark.parametrize("keep", [True, False])
def test_mirror_equals_the_recorded_map_and_bool(ci, n, h, w, sfact, keep):
    from samnerf_amd import incoherent as inc
    m = fx.masks(ci)
    got = inc.torch_get_incoherent_mask(m[:, None], sfact=sfact, keep_size=keep)
    assert fx.same(got, fx.want_map(ci, keep))
    assert fx.same(got.to(torch.bool).view(n, -1), fx.want_bool(ci, n, h, w, sfact, keep))
    # a CPU tensor takes the mirror, through the public names too
    assert fx.same(inc.get_incoherent_mask(m[:, None], sfact=sfact, keep_size=keep), got)
    assert inc.last_path == "torch"
    if keep:
        assert fx.same(inc.incoherent_table(m[..., None], sfact=sfact), fx.want_bool(ci, n, h, w, sfact, True))
        assert fx.same(inc.incoherent_table(m.to(torch.uint8), sfact=sfact), fx.want_bool(ci, n, h, w, sfact, True))


@pytest.mark.parametrize("ci,n,h,w,sfact", fx.mask_cases())
def test_divisible_sizes_are_exact_in_float32(ci, n, h, w, sfact):
    """What lets a kernel equal the recording bit for bit: at these sizes the
    reference's float32 and float64 maps are the same numbers."""
    for keep in (True, False):
        assert torch.equal(fx.want_map(ci, keep).double(), fx.want_map(ci, keep, double=True))


def test_residues_below_the_threshold_are_true():
    """.to(torch.bool) keeps what the 0.01 threshold did not lift to 1."""
    ci, n, h, w, sfact = fx.mask_cases()[4]
    u = fx.want_map(ci, True)
    low = (u != 0) & (u < 0.01)
    assert bool(low.any()) and bool(fx.want_bool(ci, n, h, w, sfact, True).view_as(u)[low].all())
    # the all-zero and the all-one view have no incoherent cell
    assert not bool(fx.want_bool(ci, n, h, w, sfact, True)[3:].any())


def test_gt_incoherent_masks_follows_the_providers_condition():
    from samnerf_amd import incoherent as inc
    ci, n, h, w, sfact = fx.mask_cases()[1]
    m = fx.masks(ci)[..., None]
    want = fx.want_bool(ci, n, h, w, 2, True)
    assert fx.same(inc.gt_incoherent_masks(m), want)
    on = types.SimpleNamespace(rgb_similarity_loss_weight=0.5, incoherent_uncertainty_weight=1)
    on2 = types.SimpleNamespace(rgb_similarity_loss_weight=0, incoherent_uncertainty_weight=0.5)
    off = types.SimpleNamespace(rgb_similarity_loss_weight=0, incoherent_uncertainty_weight=1)
    assert fx.same(inc.gt_incoherent_masks(m, on), want) and fx.same(inc.gt_incoherent_masks(m, on2), want)
    assert inc.gt_incoherent_masks(m, off) is None


@pytest.mark.parametrize("K,n_inst", fx.logit_cases())
def test_render_mask_ids_mirror_equals_the_recording(K, n_inst):
    from samnerf_amd import incoherent as inc
    z = fx.logits(K)
    ids, pred = inc.torch_render_mask_ids(z, n_inst, return_pred=True)
    assert fx.same(ids, fx.t(f"logits/{K}/ids")) and fx.same(pred, fx.t(f"logits/{K}/pred32"))
    ids2, pred2 = inc.render_mask_ids(z, n_inst, return_pred=True)          # CPU logits: the mirror
    assert fx.same(ids2, ids) and fx.same(pred2, pred)
    if K == 1:
        assert not bool(ids.any())
    else:
        assert 0.1 < float(ids.float().mean()) < 0.9


def test_a_tie_and_a_nan_give_zero():
    from samnerf_amd import incoherent as inc
    z = fx.logits(2)
    tie = z[:, 0] == z[:, 1]
    assert float(tie.float().mean()) >= 0.05
    assert not bool(fx.t("logits/2/ids")[tie].any())
    bad = torch.tensor([[0.0, float("nan")], [float("nan"), 5.0], [0.0, float("inf")], [0.0, 5.0]])
    assert inc.torch_render_mask_ids(bad, 2).tolist() == [0, 0, 0, 1]


def test_update_lines_mirror_equals_the_recording():
    """render_mask_ids -> incoherent_table is update_incoherent_mask after the renders."""
    from samnerf_amd import incoherent as inc
    views, S, K, n_inst, z, ids, table = fx.update_case()
    got_ids = inc.render_mask_ids(z.view(views, S, S, K), n_inst)
    assert fx.same(got_ids[:, None], ids)
    assert fx.same(inc.incoherent_table(got_ids, sfact=2), table)


def test_due_gives_the_expected_steps():
    from samnerf_amd.incoherent import due
    opt = types.SimpleNamespace(use_dynamic_incoherent=True, incoherent_update_iter=50, rgb_similarity_iter=120)
    assert [s for s in range(1, 301) if due(s, opt)] == [150, 200, 250, 300]
    opt.rgb_similarity_iter = 100
    assert [s for s in range(1, 201) if due(s, opt)] == [100, 150, 200]
    opt.use_dynamic_incoherent = False
    assert not any(due(s, opt) for s in range(1, 201))


def test_c_abi_rejects_bad_sizes_and_null_pointers(hip_lib):
    from samnerf_amd import _lib
    L = hip_lib
    p = 64                                    # never dereferenced: validation fails first

    def masks(**kw):
        a = _lib.SamnerfIncoherentMasksArgs()
        a.n, a.H, a.W, a.sfact, a.keep_size, a.input_type, a.masks, a.table = 1, 8, 8, 2, 1, 0, p, p
        for k, v in kw.items():
            setattr(a, k, v)
        rc = L.samnerf_incoherent_masks(ctypes.byref(a), None)
        return rc, L.samnerf_last_error()

    for kw, text in ((dict(H=7), b"divisible by sfact"), (dict(W=9), b"divisible by sfact"),
                     (dict(H=33, W=65), b"divisible by sfact"), (dict(sfact=3, H=9, W=9), b"power of two"),
                     (dict(sfact=0), b"power of two"), (dict(sfact=16), b"H / sfact"),
                     (dict(H=0), b"at least 1"), (dict(masks=None), b"null masks"),
                     (dict(table=None), b"nothing to write"), (dict(input_type=2), b"input_type"),
                     (dict(H=1 << 16, W=1 << 16), b"2^31")):
        rc, msg = masks(**kw)
        assert rc == -1 and msg.startswith(b"incoherent_masks: ") and text in msg, (kw, rc, msg)
    assert L.samnerf_incoherent_masks(None, None) == -1 and b"null args" in L.samnerf_last_error()
    assert masks(n=0, masks=None, table=None)[0] == 0        # no view: a successful no-op, no launch

    def ids(**kw):
        a = _lib.SamnerfIncoherentIdsArgs()
        a.N, a.K, a.n_inst, a.logits, a.ids = 4, 3, 3, p, p
        for k, v in kw.items():
            setattr(a, k, v)
        rc = L.samnerf_incoherent_ids(ctypes.byref(a), None)
        return rc, L.samnerf_last_error()

    for kw, text in ((dict(K=0), b"[1, 32]"), (dict(K=33, n_inst=33), b"[1, 32]"), (dict(n_inst=0), b"[1, K]"),
                     (dict(n_inst=4), b"[1, K]"), (dict(n_inst=1), b"n_inst == 1 takes K == 1"),
                     (dict(logits=None), b"null logits"), (dict(ids=None), b"null ids")):
        rc, msg = ids(**kw)
        assert rc == -1 and msg.startswith(b"incoherent_ids: ") and text in msg, (kw, rc, msg)
    assert L.samnerf_incoherent_ids(None, None) == -1 and b"null args" in L.samnerf_last_error()
    assert ids(N=0, logits=None, ids=None)[0] == 0
