"""SamDecoder.decode_batch on the GPU.  Every linear output of the decoder is
one FMA chain over k and every attention sum has a fixed order, so the batch
axis cannot change a bit: set b of a batch must equal the single call on
points[b] exactly (compared as int32 views).  Fractional coordinates, which the
int32 entry cannot take, go against the float64 twin under
test_gpu_sam_decoder.py's rule."""
import functools

import numpy as np
import pytest
import torch

import sam_decoder_ref as ref

pytestmark = pytest.mark.gpu

# g, P, B, mixed labels, the [h, w, 256] map entry
SHAPES = [
    (8, 1, 5, False, None),
    (8, 10, 3, True, None),
    (8, 11, 3, False, (7, 5)),
    (8, 58, 2, False, None),
    (16, 26, 2, False, None),
    (16, 27, 2, True, (24, 32)),
    (64, 1, 2, False, None),
    (8, 3, 1, True, None),          # B = 1
    (8, 2, 7, True, None),          # odd, ragged against any tile
]


@functools.lru_cache(maxsize=None)
def decoder(g):
    from samnerf_amd.sam_decoder import SamDecoder
    return SamDecoder.from_state_dict(ref.state_dict(), g=g, device="cuda:0")


def inputs(g, P, B, mixed, hw, seed=0, fractional=False):
    gen = torch.Generator().manual_seed(1000 + 97 * g + 11 * P + B + seed)
    S = 16 * g
    feats = torch.randn(*(hw or (g * g,)), 256, generator=gen)
    if fractional:
        pts = torch.rand(B, P, 2, generator=gen) * (S - 1)
    else:
        pts = torch.randint(0, S, (B, P, 2), generator=gen).float()
    labels = torch.randint(0, 2, (B, P), generator=gen, dtype=torch.int32) if mixed else \
        torch.ones(B, P, dtype=torch.int32)
    return feats, pts, labels


def bits(x):
    return x.contiguous().view(torch.int32)


@pytest.mark.parametrize("g,P,B,mixed,hw", SHAPES)
def test_every_set_has_the_bits_of_its_single_call(hip_lib, cuda, g, P, B, mixed, hw):
    dec = decoder(g)
    feats, pts, labels = inputs(g, P, B, mixed, hw)
    feats = feats.to(cuda)
    low, iou = dec.decode_batch(feats, pts.to(cuda), labels.to(cuda))
    assert low.shape == (B, 4, 4 * g, 4 * g) and iou.shape == (B, 4)
    assert not low.isnan().any() and not iou.isnan().any()
    for b in range(B):
        l1, i1 = dec.decode(feats, pts[b].numpy().astype(np.int32), labels[b].numpy())
        assert torch.equal(bits(low[b]), bits(l1)), f"low_res of set {b}"
        assert torch.equal(bits(iou[b]), bits(i1)), f"iou of set {b}"
    if B > 1:
        assert not torch.equal(low[0], low[1]), "the sets must differ for the comparison to show anything"


def test_identical_sets_give_identical_rows_and_the_launch_count_is_the_single_calls(hip_lib, cuda):
    dec = decoder(8)
    feats, pts, labels = inputs(8, 4, 3, True, None)
    pts[2], labels[2] = pts[0], labels[0]
    feats = feats.to(cuda)
    dec.decode(feats, pts[0].numpy().astype(np.int32), labels[0].numpy())
    single = hip_lib.samnerf_sam_decoder_launches()
    low, iou = dec.decode_batch(feats, pts.to(cuda), labels.to(cuda))
    assert hip_lib.samnerf_sam_decoder_launches() == single == 44
    assert torch.equal(bits(low[0]), bits(low[2])) and torch.equal(bits(iou[0]), bits(iou[2]))
    assert not torch.equal(low[0], low[1])
    dec.decode_batch(feats, pts[:1].repeat(7, 1, 1).to(cuda), labels[:1].repeat(7, 1).to(cuda))
    assert hip_lib.samnerf_sam_decoder_launches() == single


def test_a_label_is_read_as_nonzero(hip_lib, cuda):
    """A label other than 0 or 1 on the device is the caller's error; the
    kernel reads it as label != 0 and indexes nothing with it.  Host labels
    are checked by the wrapper."""
    dec = decoder(8)
    feats, pts, labels = inputs(8, 3, 2, True, None)
    feats, pts = feats.to(cuda), pts.to(cuda)
    labels[0] = torch.tensor([1, 0, 1])
    odd = labels.clone()
    odd[0] = torch.tensor([7, 0, -2 ** 31])
    a = dec.decode_batch(feats, pts, labels.to(cuda))
    b = dec.decode_batch(feats, pts, odd.to(cuda))
    assert torch.equal(bits(a[0]), bits(b[0])) and torch.equal(bits(a[1]), bits(b[1]))
    with pytest.raises(ValueError, match="labels must be 0 or 1"):
        dec.decode_batch(feats, pts, odd.numpy())


@pytest.mark.parametrize("g,P,B", [(8, 5, 4), (16, 12, 2)])
def test_fractional_coordinates_against_the_float64_twin(hip_lib, cuda, g, P, B):
    dec = decoder(g)
    feats, pts, labels = inputs(g, P, B, True, None, seed=5, fractional=True)
    assert (pts != pts.round()).all()
    low, iou = dec.decode_batch(feats.to(cuda), pts.to(cuda), labels.to(cuda))
    t64, t32 = ref.Twin(ref.state_dict()), ref.Twin(ref.state_dict(), torch.float32)
    ok = True
    for b in range(B):
        want = t64.decode(feats.double(), pts[b], labels[b], g)
        yard = t32.decode(feats, pts[b], labels[b], g)
        for what, got, w, y in zip(("low_res", "iou"), (low[b], iou[b]), want, yard):
            err, bar = ref.rel_err(got, w), ref.rel_err(y, w)
            print(f"sam_decoder_batch g{g} set {b} {what:8s} device {err:.3e}  float32 twin {bar:.3e}  "
                  f"ratio {err / bar if bar else float('inf'):.2f}")
            ok = ok and (err <= 4 * bar or err <= 1e-5)
    assert ok


@pytest.mark.parametrize("g,P,B,hw", [(8, 11, 3, None), (16, 5, 2, (24, 32))])
def test_repeatable_whole_and_nothing_beside_the_buffers(hip_lib, cuda, g, P, B, hw):
    """Two calls give the same bits; a workspace and outputs filled with NaN
    give the bits of zero-filled ones; the guard bands around low_res, iou and
    the workspace keep their NaN and none is left in the outputs."""
    dec = decoder(g)
    feats, pts, labels = inputs(g, P, B, True, hw)
    feats, pts, labels = feats.to(cuda), pts.to(cuda), labels.to(cuda)
    need = hip_lib.samnerf_sam_decoder_batch_workspace_size(g, B)
    guard = 256                                              # bytes and floats: the carve's alignment

    def run(fill):
        n_low, nan = B * 64 * g * g, float("nan")
        lb = torch.full((guard + n_low + guard,), nan, device=cuda)
        ib = torch.full((guard + 4 * B + guard,), nan, device=cuda)
        wb = torch.full((guard + need // 4 + guard,), nan, device=cuda)
        low, iou, ws = lb[guard:guard + n_low], ib[guard:guard + 4 * B], wb[guard:guard + need // 4]
        low.fill_(fill), iou.fill_(fill), ws.fill_(fill)
        dec.decode_batch(feats, pts, labels, out=(low.view(B, 4, 4 * g, 4 * g), iou.view(B, 4)),
                         workspace=ws.view(torch.uint8))
        for buf, n in ((lb, n_low), (ib, 4 * B), (wb, need // 4)):
            assert bool(torch.cat([buf[:guard], buf[guard + n:]]).isnan().all())
        assert not low.isnan().any() and not iou.isnan().any()
        return low.clone(), iou.clone()
    a = run(0.0)
    torch.empty(1 << 20, device=cuda).normal_()
    b = run(0.0)
    c = run(float("nan"))
    want = dec.decode_batch(feats, pts, labels)
    for x in (b, c, want):
        assert torch.equal(bits(a[0]), bits(x[0].reshape(-1))) and torch.equal(bits(a[1]), bits(x[1].reshape(-1)))


def test_predict_points_batch_shapes_and_selection(hip_lib, cuda):
    from samnerf_amd.sam_decoder import DevicePredictor
    g, H, W = 8, 15, 20
    dec = decoder(g)
    feats, pts, labels = inputs(g, 2, 3, True, None)
    feats = feats.to(cuda)
    input_size, _ = ref.input_size_for(H, W, g)
    pred = DevicePredictor(dec)
    pred.features = feats.view(g, g, 256).permute(2, 0, 1)[None]
    pred.original_size, pred.input_size, pred.is_image_set = (H, W), input_size, True
    low, iou = dec.decode_batch(feats, pts.to(cuda), labels.to(cuda))
    m3, i3, l3 = pred.predict_points_batch(pts.to(cuda), labels.to(cuda), multimask_output=True, return_logits=True)
    m1, i1, l1 = pred.predict_points_batch(pts.to(cuda), labels.to(cuda), multimask_output=False)
    assert m3.shape == (3, 3, H, W) and m3.dtype == torch.float32 and i3.shape == (3, 3) and l3.shape == (3, 3, 32, 32)
    assert m1.shape == (3, 1, H, W) and m1.dtype == torch.bool and i1.shape == (3, 1) and l1.shape == (3, 1, 32, 32)
    assert torch.equal(l3, low[:, 1:]) and torch.equal(i3, iou[:, 1:])
    assert torch.equal(l1, low[:, :1]) and torch.equal(i1, iou[:, :1])
    for b in range(3):
        assert torch.equal(m3[b], dec.masks(low[b, 1:], input_size, (H, W), logits=True))
        assert torch.equal(m1[b], dec.masks(low[b, :1], input_size, (H, W)))
    with pytest.raises(NotImplementedError, match="B > 1"):
        pred.predict_torch(pts.to(cuda), labels.to(cuda))
