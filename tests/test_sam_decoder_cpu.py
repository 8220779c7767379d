"""The SAM decoder without a GPU: the state-dict loader, the C ABI's refusals,
the float64 twin against its golden file, the tile-partial attention algebra
of the kernels, and the conditions the GPU tests' cases must meet."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import sam_decoder_ref as ref
from conftest import GOLDEN

CASE_NAMES = [c[0] for c in ref.CASES]


# ------------------------------------------------------------------ loader --

def test_loader_accepts_prefixes_and_ignores_other_keys():
    from samnerf_amd.sam_decoder import flatten_state_dict, state_dict_spec
    sd = ref.synthetic_state_dict(3, extra=True)
    flat = flatten_state_dict(sd)
    assert flat.dtype == torch.float32 and flat.numel() == sum(math.prod(s) for _, s in state_dict_spec())
    assert torch.equal(flat, flatten_state_dict({"module." + k: v for k, v in sd.items()}))
    assert torch.equal(flat, flatten_state_dict(ref.synthetic_state_dict(3)))
    first = sd["prompt_encoder.pe_layer.positional_encoding_gaussian_matrix"].float().reshape(-1)
    assert torch.equal(flat[:256], first)
    last = sd["mask_decoder.iou_prediction_head.layers.2.bias"].float()
    assert torch.equal(flat[-4:], last)


def test_loader_names_a_missing_key_and_a_wrong_shape():
    from samnerf_amd.sam_decoder import flatten_state_dict
    sd = dict(ref.synthetic_state_dict(3))
    gone = "mask_decoder.transformer.layers.1.norm3.bias"
    bad = "mask_decoder.output_upscaling.3.weight"
    del sd[gone]
    sd[bad] = sd[bad][:, :16]
    with pytest.raises(ValueError) as e:
        flatten_state_dict(sd)
    assert gone in str(e.value) and bad in str(e.value) and "(64, 16, 2, 2)" in str(e.value)


def test_loader_refuses_the_hq_token():
    from samnerf_amd.sam_decoder import flatten_state_dict
    sd = dict(ref.synthetic_state_dict(3))
    sd["mask_decoder.hf_token.weight"] = torch.zeros(1, 256)
    with pytest.raises(NotImplementedError, match="HQ token"):
        flatten_state_dict(sd)


def test_raw_count_matches_the_spec(hip_lib):
    from samnerf_amd.sam_decoder import state_dict_spec
    assert hip_lib.samnerf_sam_decoder_raw_count() == sum(math.prod(s) for _, s in state_dict_spec())
    # the pack: the raw tensors, two biases tiled four times, and image_pe [g*g][256]
    for g in (8, 64):
        assert hip_lib.samnerf_sam_decoder_pack_size(g) == \
            4 * (hip_lib.samnerf_sam_decoder_raw_count() + 3 * (64 + 32) + g * g * 256)


# ---------------------------------------------------------------- refusals --

def test_c_abi_refusals(hip_lib):
    L = hip_lib
    p = ctypes.c_void_p(4096)            # never dereferenced: validation fails first
    pts = (ctypes.c_int32 * 118)()
    ok = (ctypes.c_int32 * 59)(*([1] * 59))
    i32 = ctypes.POINTER(ctypes.c_int32)
    pt, lb = ctypes.cast(pts, i32), ctypes.cast(ok, i32)

    def call(g=8, P=1, labels=lb, ws=p, ws_bytes=None, pack_bytes=None):
        ws_bytes = L.samnerf_sam_decoder_workspace_size(g) if ws_bytes is None else ws_bytes
        pack_bytes = L.samnerf_sam_decoder_pack_size(g) if pack_bytes is None else pack_bytes
        return L.samnerf_sam_decoder(p, pack_bytes, g, p, 0, 0, pt, labels, P, p, p, ws, ws_bytes, None)

    for g in (0, 4, 12, 72, 128):
        assert L.samnerf_sam_decoder_pack_size(g) == 0 and L.samnerf_sam_decoder_workspace_size(g) == 0
        assert call(g=g, ws_bytes=1 << 30, pack_bytes=1 << 30) == -1 and b"multiple of 8" in L.samnerf_last_error()
        assert L.samnerf_sam_decoder_pack(p, L.samnerf_sam_decoder_raw_count(), g, p, 1 << 30, None) == -1
        assert L.samnerf_sam_masks(p, 1, g, 8, 8, 8, 8, p, None, None) == -1
    for g in range(8, 65, 8):
        assert L.samnerf_sam_decoder_pack_size(g) > 0 and L.samnerf_sam_decoder_workspace_size(g) > 0
    for P in (0, 59, 1000):
        assert call(P=P) == -1 and b"P must lie in [1, 58]" in L.samnerf_last_error()
    for bad in (2, -1):
        labels = (ctypes.c_int32 * 3)(1, 0, bad)
        assert call(P=3, labels=ctypes.cast(labels, i32)) == -1 and b"labels must be 0 or 1" in L.samnerf_last_error()
    assert call(ws=None) == -1 and b"null workspace" in L.samnerf_last_error()
    assert call(ws_bytes=L.samnerf_sam_decoder_workspace_size(8) - 1) == -3 and b"workspace" in L.samnerf_last_error()
    assert call(pack_bytes=L.samnerf_sam_decoder_pack_size(8) - 1) == -1 and b"pack" in L.samnerf_last_error()
    assert call(g=16, ws_bytes=L.samnerf_sam_decoder_workspace_size(8)) == -3
    assert L.samnerf_sam_decoder(p, 1 << 30, 8, p, 5, 0, pt, lb, 1, p, p, p, 1 << 30, None) == -1
    # the pack and the postprocess
    n = L.samnerf_sam_decoder_raw_count()
    assert L.samnerf_sam_decoder_pack(p, n - 1, 8, p, 1 << 30, None) == -1 and b"expected" in L.samnerf_last_error()
    assert L.samnerf_sam_decoder_pack(p, n, 8, p, 16, None) == -3
    assert L.samnerf_sam_decoder_pack(None, n, 8, p, 1 << 30, None) == -1
    for M, ih, iw, H, W in ((0, 8, 8, 8, 8), (5, 8, 8, 8, 8), (1, 0, 8, 8, 8), (1, 8, 129, 8, 8), (1, 8, 8, 0, 8),
                            (1, 8, 8, 8, 8193)):
        assert L.samnerf_sam_masks(p, M, 8, ih, iw, H, W, p, None, None) == -1
    assert L.samnerf_sam_masks(p, 1, 8, 8, 8, 8, 8, None, None, None) == -1
    assert L.samnerf_sam_masks(None, 1, 8, 8, 8, 8, 8, p, None, None) == -1


def test_out_of_scope_prompts_are_named():
    from samnerf_amd.sam_decoder import DevicePredictor

    class Dec:
        g, S, device = 8, 128, torch.device("cpu")
    pred = DevicePredictor(Dec())
    pred.features = torch.zeros(1, 256, 8, 8)
    pred.original_size, pred.input_size, pred.is_image_set = (8, 8), (128, 128), True
    c, l = torch.zeros(1, 1, 2), torch.ones(1, 1, dtype=torch.int)
    with pytest.raises(NotImplementedError, match="mask_input"):
        pred.predict_torch(c, l, mask_input=torch.zeros(1, 1, 32, 32))
    with pytest.raises(NotImplementedError, match="box"):
        pred.predict_torch(c, l, boxes=torch.zeros(1, 4))
    with pytest.raises(NotImplementedError, match="B > 1"):
        pred.predict_torch(torch.zeros(2, 1, 2), torch.ones(2, 1, dtype=torch.int))
    pred.interm_features = [torch.zeros(1)]
    with pytest.raises(NotImplementedError, match="HQ token"):
        pred.predict_torch(c, l)
    with pytest.raises(NotImplementedError, match="ViT"):
        pred.set_image(np.zeros((8, 8, 3), np.uint8))
    with pytest.raises(ValueError, match=r"\[1, 256, 8, 8\]"):
        pred.features = torch.zeros(1, 256, 64, 64)


# -------------------------------------------------------------------- twin --

def test_twin_matches_its_golden_file():
    gold = np.load(os.path.join(GOLDEN, "sam_decoder.npz"))
    assert sorted(gold.files) == sorted(n + s for n in ref.GOLDEN_CASES for s in (".low_res", ".iou"))
    for name in ref.GOLDEN_CASES:
        low, iou, _ = ref.twin_outputs(name)
        assert low.dtype == torch.float64
        # float64 on another BLAS sums in another order: 1e-12 of the scale, a million times below fp32's error
        assert ref.rel_err(low, torch.from_numpy(gold[name + ".low_res"])) < 1e-12
        assert ref.rel_err(iou, torch.from_numpy(gold[name + ".iou"])) < 1e-12


def test_tile_partials_merged_in_order_are_the_softmax():
    """The kernels' attention: every thread (here: every 64-key tile) keeps
    (max, sum of exp, weighted values) and the partials are merged in a fixed
    order with the flash-attention combination; a partial without a key has
    max -inf and weight 0.  In float64 that is the softmax to rounding."""
    t = ref.Twin(ref.state_dict())
    g = torch.Generator().manual_seed(5)
    for T, N, dh in ((7, 64, 16), (17, 256, 16), (64, 200, 32)):
        q, k, v = (torch.randn(8, n, dh, generator=g, dtype=torch.float64) for n in (T, N, N))
        s = q @ k.transpose(1, 2) / math.sqrt(dh)
        want = torch.softmax(s, -1) @ v
        m = torch.full((8, T), -math.inf, dtype=torch.float64)
        l = torch.zeros(8, T, dtype=torch.float64)
        acc = torch.zeros(8, T, dh, dtype=torch.float64)
        for lo in list(range(0, N, 64)) + [N]:             # the last tile is empty
            st = s[:, :, lo:lo + 64]
            mo = st.max(-1).values if st.shape[-1] else torch.full((8, T), -math.inf, dtype=torch.float64)
            p = torch.exp(st - mo[..., None])
            lo_, ao = p.sum(-1), p @ v[:, lo:lo + 64]
            mn = torch.maximum(m, mo)
            c1 = torch.where(m == -math.inf, torch.zeros_like(m), torch.exp(m - mn))
            c2 = torch.where(mo == -math.inf, torch.zeros_like(m), torch.exp(mo - mn))
            l, acc, m = l * c1 + lo_ * c2, acc * c1[..., None] + ao * c2[..., None], mn
        assert (acc / l[..., None] - want).abs().max() < 1e-14
    # and the twin's own attention is that softmax over its projections
    x = torch.randn(9, 256, generator=g, dtype=torch.float64)
    n = "mask_decoder.transformer.layers.0.self_attn"
    qp, kp, vp = (t.lin(f"{n}.{p}_proj", x).view(9, 8, 32).transpose(0, 1) for p in "qkv")
    o = (torch.softmax(qp @ kp.transpose(1, 2) / math.sqrt(32), -1) @ vp).transpose(0, 1).reshape(9, 256)
    assert torch.equal(t.attention(n, x, x, x), t.lin(n + ".out_proj", o))


@pytest.mark.parametrize("name", CASE_NAMES)
def test_fixture_conditions(name):
    """What the GPU tests lean on, for every case: the pixels left out of the
    mask comparison (|float64 logit| <= 1e-4 max|low_res|) are at most 1 % of
    the view, the float32 twin flips no pixel at all, and its error -- the
    GPU tests' yardstick -- is fp32 rounding carried through nine norms and
    seven softmaxes (1e-6 to 1e-5 of the scale on these cases), far from the
    1e-2 and more of a wrong term."""
    low, iou, logits = ref.twin_outputs(name)
    low32, iou32, logits32 = ref.twin_outputs(name, torch.float32)
    assert 1.0 < low.abs().max() < 50.0
    left_out = 1.0 - ref.decided(name).double().mean().item()
    assert left_out <= 0.01, left_out
    assert torch.equal(logits32 > 0, logits > 0)
    for got, want in ((low32, low), (iou32, iou), (logits32, logits)):
        assert ref.rel_err(got, want) < 1e-4
