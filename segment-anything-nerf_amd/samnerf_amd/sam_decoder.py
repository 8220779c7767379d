"""SAM's prompt encoder and mask decoder for point prompts on the device
(csrc/sam_decoder.hip, include/samnerf_hip.h "SAM decoder").

`SamDecoder.from_state_dict` takes a SAM checkpoint's state dict (plain SAM:
`prompt_encoder.*` and `mask_decoder.*`; the ViT's `image_encoder.*` and the
mask-input `mask_downscaling.*` keys are ignored) and packs it once.
`decode` turns image tokens and clicks into the four low-res masks and IoU
scores in 44 launches; `masks` is Sam.postprocess_masks in one.
`decode_batch` takes B prompt sets of P points each (device tensors, B up to
256) in the same 44 launches, every set with the bits of its own `decode`;
`masks_select`, `mask_stats` and `nms` are the automatic mask generator's
steps on the device (sam_generator.DeviceMaskGenerator puts them together).
`DevicePredictor` gives them SamPredictor's interface, so
`sam_bridge.sam_predict` / `render_and_predict` drive it unchanged.

The model is written from its published description and tested against the
project's own float64 restatement (tests/sam_decoder_ref.py) with synthetic
weights.  It has not been compared with an installed segment_anything or a
real checkpoint.

Not built, each raising NotImplementedError: a mask input, box prompts,
prompt sets of different sizes in one call, the HQ token (`interm_features`),
and the ViT image encoder.  `DevicePredictor.predict_torch` keeps SamPredictor's
one-set form; `predict_points_batch` is the batched one.
"""
import ctypes

import numpy as np
import torch

from .ops import _ptr, _stream

C = 256
MAX_POINTS = 58
MAX_SETS = 256
MAX_CANDIDATES = 3 * 64 * 64
REC_WORDS = 10        # SAMNERF_SAM_REC_WORDS: inter, union, area, x0, y0, x1, y1, stability, pass, iou


def _attention(prefix, inner):
    keys = []
    for p, (o, i) in (("q_proj", (inner, C)), ("k_proj", (inner, C)), ("v_proj", (inner, C)),
                      ("out_proj", (C, inner))):
        keys += [(f"{prefix}.{p}.weight", (o, i)), (f"{prefix}.{p}.bias", (o,))]
    return keys


def _linear(prefix, i, o):
    return [(f"{prefix}.weight", (o, i)), (f"{prefix}.bias", (o,))]


def _norm(prefix, n=C):
    return [(f"{prefix}.weight", (n,)), (f"{prefix}.bias", (n,))]


def state_dict_spec():
    """The (key, shape) pairs the decoder reads, in samnerf_sam_decoder_pack's
    raw order (include/samnerf_hip.h)."""
    pe, md = "prompt_encoder", "mask_decoder"
    keys = [(f"{pe}.pe_layer.positional_encoding_gaussian_matrix", (2, 128)),
            (f"{pe}.point_embeddings.0.weight", (1, C)), (f"{pe}.point_embeddings.1.weight", (1, C)),
            (f"{pe}.not_a_point_embed.weight", (1, C)), (f"{pe}.no_mask_embed.weight", (1, C)),
            (f"{md}.iou_token.weight", (1, C)), (f"{md}.mask_tokens.weight", (4, C))]
    for l in range(2):
        t = f"{md}.transformer.layers.{l}"
        keys += _attention(f"{t}.self_attn", C) + _attention(f"{t}.cross_attn_token_to_image", C // 2)
        keys += _attention(f"{t}.cross_attn_image_to_token", C // 2)
        for n in range(1, 5):
            keys += _norm(f"{t}.norm{n}")
        keys += _linear(f"{t}.mlp.lin1", C, 2048) + _linear(f"{t}.mlp.lin2", 2048, C)
    keys += _attention(f"{md}.transformer.final_attn_token_to_image", C // 2)
    keys += _norm(f"{md}.transformer.norm_final_attn")
    up = f"{md}.output_upscaling"
    keys += [(f"{up}.0.weight", (C, 64, 2, 2)), (f"{up}.0.bias", (64,))] + _norm(f"{up}.1", 64)
    keys += [(f"{up}.3.weight", (64, 32, 2, 2)), (f"{up}.3.bias", (32,))]
    for i in range(4):
        h = f"{md}.output_hypernetworks_mlps.{i}.layers"
        keys += _linear(f"{h}.0", C, C) + _linear(f"{h}.1", C, C) + _linear(f"{h}.2", C, 32)
    h = f"{md}.iou_prediction_head.layers"
    keys += _linear(f"{h}.0", C, C) + _linear(f"{h}.1", C, C) + _linear(f"{h}.2", C, 4)
    return keys


def flatten_state_dict(sd):
    """The decoder's tensors of `sd` as one fp32 CPU vector in the raw order.
    Keys may carry a `module.` prefix; `image_encoder.*`, `mask_downscaling.*`
    and anything else the decoder does not read is ignored.  A missing or
    mis-shaped tensor is a ValueError that names it."""
    sd = {(k[len("module."):] if k.startswith("module.") else k): v for k, v in sd.items()}
    if any("hf_token" in k or "hf_mlp" in k for k in sd):
        raise NotImplementedError("SamDecoder: the HQ token (SAM-HQ's hf_token / hf_mlp) is not built; plain SAM only")
    missing, wrong, parts = [], [], []
    for key, shape in state_dict_spec():
        if key not in sd:
            missing.append(key)
            continue
        t = torch.as_tensor(sd[key])
        if tuple(t.shape) != shape:
            wrong.append(f"{key}: {tuple(t.shape)}, expected {shape}")
            continue
        parts.append(t.detach().to(device="cpu", dtype=torch.float32).reshape(-1))
    if missing or wrong:
        raise ValueError("SamDecoder.from_state_dict: " +
                         "; ".join((["missing " + ", ".join(missing)] if missing else []) +
                                   (["wrong shape " + ", ".join(wrong)] if wrong else [])))
    return torch.cat(parts)


class SamDecoder:
    """The packed decoder of one checkpoint for a g x g token grid."""

    def __init__(self, raw, g=64, device="cuda"):
        from ._lib import check, lib
        L = lib()
        self.g, self.S, self.device = int(g), 16 * int(g), torch.device(device)
        need = L.samnerf_sam_decoder_pack_size(self.g)
        if need == 0:
            raise ValueError(f"SamDecoder: g = {g} must be a multiple of 8 in [8, 64]")
        if raw.numel() != L.samnerf_sam_decoder_raw_count():
            raise ValueError(f"SamDecoder: {raw.numel()} weights, {L.samnerf_sam_decoder_raw_count()} expected")
        raw = raw.to(self.device)
        self.pack = torch.empty(need, dtype=torch.uint8, device=self.device)
        check(L.samnerf_sam_decoder_pack(_ptr(raw), raw.numel(), self.g, _ptr(self.pack), need,
                                         _stream(self.device)), "sam_decoder_pack")
        torch.cuda.current_stream(self.device).synchronize()      # raw may go once the kernels have read it
        self.ws_bytes = L.samnerf_sam_decoder_workspace_size(self.g)
        self.ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device=self.device)

    @classmethod
    def from_state_dict(cls, sd, g=64, device="cuda"):
        return cls(flatten_state_dict(sd), g=g, device=device)

    def decode(self, features, points, labels=None, out=None):
        """features: the image tokens [g*g, 256] (token-major, zero where the
        view is padded) or a rendered map [h, w, 256], fp32 on the device;
        points [P, 2] integer (x, y) in the S = 16 g frame (host), labels [P]
        of 0 / 1 (default all 1).  Returns (low_res [4, 4g, 4g], iou [4]);
        `out` = (low_res, iou) writes into given tensors."""
        from ._lib import check, lib
        g = self.g
        if not (features.is_cuda and features.dtype == torch.float32 and features.is_contiguous()):
            raise ValueError("SamDecoder.decode: features must be a contiguous fp32 tensor on the device")
        if features.dim() == 2 and tuple(features.shape) == (g * g, C):
            h = w = 0
        elif features.dim() == 3 and features.shape[2] == C:
            h, w = int(features.shape[0]), int(features.shape[1])
        else:
            raise ValueError(f"SamDecoder.decode: features must be [{g * g}, {C}] or [h, w, {C}], "
                             f"not {tuple(features.shape)}")
        pts = np.ascontiguousarray(np.asarray(points).reshape(-1, 2).astype(np.int32))
        lab = np.ones(len(pts), np.int32) if labels is None else \
            np.ascontiguousarray(np.asarray(labels).reshape(-1).astype(np.int32))
        if len(lab) != len(pts):
            raise ValueError(f"SamDecoder.decode: {len(pts)} points and {len(lab)} labels")
        low, iou = out if out is not None else (torch.empty(4, 4 * g, 4 * g, device=self.device),
                                                torch.empty(4, device=self.device))
        i32p = ctypes.POINTER(ctypes.c_int32)
        check(lib().samnerf_sam_decoder(_ptr(self.pack), self.pack.numel(), g, _ptr(features), h, w,
                                        pts.ctypes.data_as(i32p), lab.ctypes.data_as(i32p), len(pts), _ptr(low),
                                        _ptr(iou), _ptr(self.ws), self.ws_bytes, _stream(self.device)),
              "sam_decoder")
        return low, iou

    def _features_hw(self, features, who):
        g = self.g
        if not (features.is_cuda and features.dtype == torch.float32 and features.is_contiguous()):
            raise ValueError(f"SamDecoder.{who}: features must be a contiguous fp32 tensor on the device")
        if features.dim() == 2 and tuple(features.shape) == (g * g, C):
            return 0, 0
        if features.dim() == 3 and features.shape[2] == C:
            return int(features.shape[0]), int(features.shape[1])
        raise ValueError(f"SamDecoder.{who}: features must be [{g * g}, {C}] or [h, w, {C}], "
                         f"not {tuple(features.shape)}")

    def _batch_workspace(self, B):
        from ._lib import lib
        need = lib().samnerf_sam_decoder_batch_workspace_size(self.g, B)
        if need == 0:
            raise ValueError(f"SamDecoder.decode_batch: B = {B} must lie in [1, {MAX_SETS}]")
        ws = getattr(self, "_ws_batch", None)
        if ws is None or ws.numel() < need:
            self._ws_batch = ws = None                         # the old one goes before the new one comes
            self._ws_batch = ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        return ws, need

    def decode_batch(self, features, points, labels=None, out=None, workspace=None):
        """B prompt sets over one image: features as in `decode`; points
        [B, P, 2] (x, y) in the S frame, fractional or whole, and labels [B, P]
        (default all 1), as device tensors (used as they are: no host copy) or
        host arrays (labels then checked to be 0 / 1).  Returns (low_res
        [B, 4, 4g, 4g], iou [B, 4]); set b has the bits of decode(points[b]).
        `out` = (low_res, iou) and `workspace` (a uint8 device tensor of
        samnerf_sam_decoder_batch_workspace_size bytes) may be given."""
        from ._lib import check, lib
        g = self.g
        h, w = self._features_hw(features, "decode_batch")
        if not torch.is_tensor(points):
            points = torch.as_tensor(np.asarray(points, dtype=np.float32))
        if points.dim() != 3 or points.shape[2] != 2:
            raise ValueError(f"SamDecoder.decode_batch: points must be [B, P, 2], not {tuple(points.shape)}")
        B, P = int(points.shape[0]), int(points.shape[1])
        if not 1 <= P <= MAX_POINTS:
            raise ValueError(f"SamDecoder.decode_batch: P = {P} must lie in [1, {MAX_POINTS}]")
        points = points.to(device=self.device, dtype=torch.float32).contiguous()
        if labels is None:
            labels = torch.ones(B, P, dtype=torch.int32, device=self.device)
        else:
            if not (torch.is_tensor(labels) and labels.is_cuda):
                host = np.asarray(labels.cpu() if torch.is_tensor(labels) else labels)
                if not np.isin(host, (0, 1)).all():
                    raise ValueError("SamDecoder.decode_batch: labels must be 0 or 1")
                labels = torch.as_tensor(host.astype(np.int32))
            labels = labels.to(device=self.device, dtype=torch.int32).contiguous()
        if tuple(labels.shape) != (B, P):
            raise ValueError(f"SamDecoder.decode_batch: labels must be [{B}, {P}], not {tuple(labels.shape)}")
        if workspace is None:
            workspace, need = self._batch_workspace(B)
        else:
            need = workspace.numel()
        low, iou = out if out is not None else (torch.empty(B, 4, 4 * g, 4 * g, device=self.device),
                                                torch.empty(B, 4, device=self.device))
        check(lib().samnerf_sam_decoder_batch(_ptr(self.pack), self.pack.numel(), g, _ptr(features), h, w,
                                              _ptr(points), _ptr(labels), B, P, _ptr(low), _ptr(iou),
                                              _ptr(workspace), need, _stream(self.device)), "sam_decoder_batch")
        return low, iou

    def masks_select(self, low_res, input_size, original_size, index=None, count=None, cap=None, logits=False,
                     out=None, mask_threshold=0.0):
        """`masks` as a gather: slot s of the output is mask index[s] (a device
        int32 tensor; None: s) of the table low_res [n, 4g, 4g].  `cap` slots
        (default: len(index), or n) are launched; `count`, a device int32, keeps
        the slots at and past it as they were.  mask = logit > mask_threshold."""
        from ._lib import check, lib
        low_res = low_res.contiguous()
        n, (H, W) = int(low_res.shape[0]), (int(original_size[0]), int(original_size[1]))
        if cap is None:
            cap = n if index is None else int(index.numel())
        if out is None:
            out = torch.zeros(cap, H, W, device=low_res.device, dtype=torch.float32 if logits else torch.uint8)
        check(lib().samnerf_sam_masks_select(_ptr(low_res), n, None if index is None else _ptr(index), cap,
                                             None if count is None else _ptr(count), self.g, int(input_size[0]),
                                             int(input_size[1]), H, W, float(mask_threshold),
                                             _ptr(out) if logits else None, None if logits else _ptr(out),
                                             _stream(low_res)), "sam_masks_select")
        return out if logits else out.view(torch.bool)

    def mask_stats(self, low_res, iou, input_size, original_size, pred_iou_thresh, stability_score_thresh,
                   stability_score_offset=1.0, mask_threshold=0.0, out=None):
        """The generator's filters of n candidates (low_res [n, 4g, 4g], iou
        [n]) over the (H, W) view: int32 records [n, REC_WORDS] (the stability
        and iou words hold fp32 bits), include/samnerf_hip.h."""
        from ._lib import check, lib
        low_res, iou = low_res.contiguous(), iou.contiguous()
        n = int(low_res.shape[0])
        if out is None:
            out = torch.empty(n, REC_WORDS, dtype=torch.int32, device=low_res.device)
        check(lib().samnerf_sam_mask_stats(_ptr(low_res), _ptr(iou), n, self.g, int(input_size[0]),
                                           int(input_size[1]), int(original_size[0]), int(original_size[1]),
                                           float(pred_iou_thresh), float(mask_threshold),
                                           float(stability_score_offset), float(stability_score_thresh), _ptr(out),
                                           _stream(low_res)), "sam_mask_stats")
        return out

    def nms(self, records, box_nms_thresh, out=None):
        """Greedy box NMS of the passing records on the device: (keep [n] int32,
        the kept candidate indices in order and then -1; count [1] int32)."""
        from ._lib import check, lib
        n = int(records.shape[0])
        keep, count = out if out is not None else (torch.full((n,), -1, dtype=torch.int32, device=records.device),
                                                   torch.zeros(1, dtype=torch.int32, device=records.device))
        check(lib().samnerf_sam_nms(_ptr(records), n, float(box_nms_thresh), _ptr(keep), _ptr(count),
                                    _stream(records)), "sam_nms")
        return keep, count

    def masks(self, low_res, input_size, original_size, logits=False, out=None):
        """Sam.postprocess_masks and the threshold: low_res [M, 4g, 4g] ->
        bool masks [M, H, W] (logits=False) or their fp32 logits."""
        from ._lib import check, lib
        low_res = low_res.contiguous()
        M, (H, W) = int(low_res.shape[0]), (int(original_size[0]), int(original_size[1]))
        if out is None:
            out = torch.empty(M, H, W, device=low_res.device, dtype=torch.float32 if logits else torch.uint8)
        check(lib().samnerf_sam_masks(_ptr(low_res), M, self.g, int(input_size[0]), int(input_size[1]), H, W,
                                      _ptr(out) if logits else None, None if logits else _ptr(out),
                                      _stream(low_res)), "sam_masks")
        return out if logits else out.view(torch.bool)


class DevicePredictor:
    """SamPredictor's interface, as sam_bridge.sam_predict drives it, over a
    SamDecoder: reset_image, original_size, input_size, features
    ([1, 256, g, g], as the ViT leaves them), is_image_set, interm_features,
    predict_torch."""

    def __init__(self, decoder):
        self.decoder = decoder
        self.model = None                   # no ViT: set_image has nothing to run
        self.reset_image()

    def reset_image(self):
        self.is_image_set = False
        self._tokens = None
        self._features = None
        self.original_size = None
        self.input_size = None
        self.interm_features = None

    def set_image(self, *a, **k):
        raise NotImplementedError("DevicePredictor: the ViT image encoder is not built; set `features` "
                                  "from a render (sam_bridge.sam_predict)")

    set_torch_image = set_image

    @property
    def features(self):
        return self._features

    @features.setter
    def features(self, f):
        g = self.decoder.g
        if f is None:
            self._features = self._tokens = None
            return
        if tuple(f.shape) != (1, C, g, g):
            raise ValueError(f"DevicePredictor.features must be [1, {C}, {g}, {g}], not {tuple(f.shape)}")
        self._features = f
        self._tokens = f[0].to(device=self.decoder.device, dtype=torch.float32).permute(1, 2, 0) \
            .reshape(g * g, C).contiguous()

    def predict_torch(self, point_coords, point_labels, boxes=None, mask_input=None, multimask_output=True,
                      return_logits=False, hq_token_only=False):
        """SamPredictor.predict_torch for one prompt set (B = 1) of whole-pixel
        points.  More than one set is refused here, as it always was;
        `predict_points_batch` takes B sets."""
        if not self.is_image_set or self._tokens is None:
            raise RuntimeError("DevicePredictor: an image's features must be set before a prediction")
        if mask_input is not None:
            raise NotImplementedError("DevicePredictor: mask_input (the dense prompt's mask_downscaling) is not built")
        if boxes is not None:
            raise NotImplementedError("DevicePredictor: box prompts are not built")
        if self.interm_features is not None or hq_token_only:
            raise NotImplementedError("DevicePredictor: the HQ token (interm_features) is not built; plain SAM only")
        if point_coords is None or point_labels is None:
            raise NotImplementedError("DevicePredictor: a prediction needs point prompts")
        if point_coords.dim() != 3 or point_coords.shape[0] != 1:
            raise NotImplementedError("DevicePredictor: batches of prompt sets (B > 1, the automatic mask "
                                      "generator's use) are not built")
        pts = point_coords[0].detach().cpu().numpy()
        if (pts != np.round(pts)).any():
            raise NotImplementedError("DevicePredictor: point coordinates must be whole pixels of the input frame")
        low, iou = self.decoder.decode(self._tokens, pts.astype(np.int32), point_labels[0].detach().cpu().numpy())
        sel = slice(1, 4) if multimask_output else slice(0, 1)
        low, iou = low[sel], iou[sel]
        masks = self.decoder.masks(low, self.input_size, self.original_size, logits=return_logits)
        return masks[None], iou[None], low[None]

    def predict_points_batch(self, point_coords, point_labels, multimask_output=True, return_logits=False):
        """predict_torch for B prompt sets of P points each: point_coords
        [B, P, 2] in the input frame (fractional allowed), point_labels [B, P];
        tensors on the device stay there.  Returns (masks [B, M, H, W] bool or
        logits, iou [B, M], low_res [B, M, 4g, 4g]), M = 3 (masks 1 .. 3) with
        multimask_output and 1 (mask 0) without."""
        if not self.is_image_set or self._tokens is None:
            raise RuntimeError("DevicePredictor: an image's features must be set before a prediction")
        if self.interm_features is not None:
            raise NotImplementedError("DevicePredictor: the HQ token (interm_features) is not built; plain SAM only")
        dec = self.decoder
        low, iou = dec.decode_batch(self._tokens, point_coords, point_labels)
        sel = slice(1, 4) if multimask_output else slice(0, 1)
        low, iou = low[:, sel].contiguous(), iou[:, sel].contiguous()
        B, M, L = low.shape[0], low.shape[1], low.shape[2]
        H, W = int(self.original_size[0]), int(self.original_size[1])
        masks = dec.masks_select(low.view(B * M, L, L), self.input_size, (H, W), logits=return_logits)
        return masks.view(B, M, H, W), iou, low
