"""The twin of csrc/sam_decoder.hip in torch: SAM's prompt encoder, mask
decoder and postprocess for point prompts, restated from the model's published
description (include/samnerf_hip.h has the equations) with the dtype as a
parameter.  float64 is the reference of the tests, float32 their yardstick.
It is the project's own text: no segment_anything is installed, and the twin
has not been compared with one.

synthetic_state_dict(seed): SAM's keys and shapes with linear and transposed-
convolution weights randn / sqrt(fan_in), biases 0.1 randn, LayerNorm weights
1 + 0.1 randn, embeddings and the gaussian matrix randn.  At this scale the
float64 logits have a maximum of about 5 and a standard deviation of about 1.
"""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

C = 256
PE, MD = "prompt_encoder", "mask_decoder"


def synthetic_state_dict(seed, extra=False):
    """float64 tensors under SAM's keys; extra=True adds keys a loader must ignore."""
    from samnerf_amd.sam_decoder import state_dict_spec
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for key, shape in state_dict_spec():
        r = torch.randn(*shape, generator=g, dtype=torch.float64)
        leaf = key.rsplit(".", 1)[1]
        norm = ".norm" in key or key.startswith(f"{MD}.output_upscaling.1.")
        if key.startswith(PE) or key.endswith("_token.weight") or key.endswith("_tokens.weight"):
            sd[key] = r
        elif norm:
            sd[key] = 1 + 0.1 * r if leaf == "weight" else 0.1 * r
        elif leaf == "bias":
            sd[key] = 0.1 * r
        elif len(shape) == 4:                     # ConvTranspose2d k2 s2: an output pixel sums over `in`
            sd[key] = r / math.sqrt(shape[0])
        else:
            sd[key] = r / math.sqrt(shape[1])
    if extra:
        sd["image_encoder.pos_embed"] = torch.zeros(1, 4, 4, 8)
        sd[f"{PE}.mask_downscaling.0.weight"] = torch.zeros(4, 1, 2, 2)
    return sd


class Twin:
    def __init__(self, sd, dtype=torch.float64, device="cpu"):
        self.dtype, self.device = dtype, torch.device(device)
        self.w = {k: torch.as_tensor(v).to(device=self.device, dtype=dtype) for k, v in sd.items()}

    def lin(self, n, x):
        return x @ self.w[n + ".weight"].T + self.w[n + ".bias"]

    def norm(self, n, x):
        return F.layer_norm(x, (x.shape[-1],), self.w[n + ".weight"], self.w[n + ".bias"], 1e-5)

    def attention(self, n, q, k, v, heads=8):
        q, k, v = self.lin(n + ".q_proj", q), self.lin(n + ".k_proj", k), self.lin(n + ".v_proj", v)

        def split(x):
            return x.view(x.shape[0], heads, -1).transpose(0, 1)
        q, k, v = split(q), split(k), split(v)
        a = torch.softmax(q @ k.transpose(1, 2) / math.sqrt(q.shape[-1]), -1)
        return self.lin(n + ".out_proj", (a @ v).transpose(0, 1).reshape(q.shape[1], -1))

    def pe(self, c):
        """c [..., 2] in [0, 1], ordered (x, y)."""
        v = (2 * c - 1) @ self.w[f"{PE}.pe_layer.positional_encoding_gaussian_matrix"] * (2 * math.pi)
        return torch.cat([v.sin(), v.cos()], -1)

    def image_pe(self, g):
        ax = (torch.arange(g, dtype=self.dtype, device=self.device) + 0.5) / g
        yy, xx = torch.meshgrid(ax, ax, indexing="ij")
        return self.pe(torch.stack([xx, yy], -1).view(-1, 2))

    def tokens(self, points, labels, S):
        def tensor(v):                                     # a tensor stays where it is: no host round trip
            return v if torch.is_tensor(v) else torch.as_tensor(np.asarray(v))
        p = tensor(points).to(device=self.device, dtype=self.dtype).view(-1, 2) + 0.5
        lb = tensor(labels).to(self.device).view(-1)
        e = self.pe(p / S)
        e = e + torch.where((lb == 1)[:, None], self.w[f"{PE}.point_embeddings.1.weight"],
                            self.w[f"{PE}.point_embeddings.0.weight"])
        return torch.cat([self.w[f"{MD}.iou_token.weight"], self.w[f"{MD}.mask_tokens.weight"], e,
                          self.w[f"{PE}.not_a_point_embed.weight"]], 0)

    def decode(self, features, points, labels, g):
        """features [g*g, 256] token-major -> (low_res [4, 4g, 4g], iou [4])."""
        tr = f"{MD}.transformer"
        tok = self.tokens(points, labels, 16 * g)
        ipe = self.image_pe(g)
        q, k = tok, features.to(device=self.device, dtype=self.dtype) + self.w[f"{PE}.no_mask_embed.weight"]
        for l in range(2):
            n = f"{tr}.layers.{l}"
            if l == 0:
                q = self.attention(n + ".self_attn", q, q, q)
            else:
                qq = q + tok
                q = q + self.attention(n + ".self_attn", qq, qq, q)
            q = self.norm(n + ".norm1", q)
            q = self.norm(n + ".norm2", q + self.attention(n + ".cross_attn_token_to_image", q + tok, k + ipe, k))
            q = self.norm(n + ".norm3", q + self.lin(n + ".mlp.lin2", F.relu(self.lin(n + ".mlp.lin1", q))))
            k = self.norm(n + ".norm4", k + self.attention(n + ".cross_attn_image_to_token", k + ipe, q + tok, q))
        q = self.norm(tr + ".norm_final_attn",
                      q + self.attention(tr + ".final_attn_token_to_image", q + tok, k + ipe, k))
        up = f"{MD}.output_upscaling"
        x = k.T.reshape(1, C, g, g)
        x = F.conv_transpose2d(x, self.w[up + ".0.weight"], self.w[up + ".0.bias"], stride=2)
        u = x.mean(1, keepdim=True)
        s = (x - u).pow(2).mean(1, keepdim=True)
        x = (x - u) / torch.sqrt(s + 1e-6)
        x = self.w[up + ".1.weight"][:, None, None] * x + self.w[up + ".1.bias"][:, None, None]
        x = F.gelu(x)
        x = F.gelu(F.conv_transpose2d(x, self.w[up + ".3.weight"], self.w[up + ".3.bias"], stride=2))

        def mlp(n, t):
            return self.lin(n + ".2", F.relu(self.lin(n + ".1", F.relu(self.lin(n + ".0", t)))))
        hyper = torch.stack([mlp(f"{MD}.output_hypernetworks_mlps.{i}.layers", q[1 + i]) for i in range(4)])
        low = (hyper @ x.view(32, -1)).view(4, 4 * g, 4 * g)
        return low, mlp(f"{MD}.iou_prediction_head.layers", q[0])


def postprocess(low, g, input_size, original_size):
    """Sam.postprocess_masks: low [M, 4g, 4g] -> logits [M, H, W]."""
    S = 16 * g
    m = F.interpolate(low[None], (S, S), mode="bilinear", align_corners=False)
    m = m[..., :input_size[0], :input_size[1]]
    return F.interpolate(m, tuple(original_size), mode="bilinear", align_corners=False)[0]


def input_size_for(H, W, g):
    r = 16 * g / W if W > H else 16 * g / H
    return (int(H * r), int(W * r)), r


def resize_pad(map_hwc, g):
    """sam_bridge.prepare_sam_features for a g-long side, to token-major rows [g*g, 256]."""
    h, w = map_hwc.shape[:2]
    r = g / w if w > h else g / h
    f = F.interpolate(map_hwc.permute(2, 0, 1)[None], (int(h * r), int(w * r)), mode="bilinear", align_corners=False)
    f = F.pad(f, (0, g - f.shape[3], 0, g - f.shape[2]))
    return f[0].permute(1, 2, 0).reshape(g * g, C)


class TwinPredictor:
    """SamPredictor's interface (what sam_bridge.sam_predict drives) over the twin."""

    def __init__(self, sd, g=64, dtype=torch.float64, device="cpu"):
        self.twin, self.g = Twin(sd, dtype, device), g
        self.reset_image()

    def reset_image(self):
        self.is_image_set, self.features = False, None
        self.original_size = self.input_size = self.interm_features = None

    def predict_torch(self, point_coords, point_labels, boxes=None, mask_input=None, multimask_output=True,
                      return_logits=False):
        assert self.is_image_set and boxes is None and mask_input is None and self.interm_features is None
        g = self.g
        feats = self.features[0].permute(1, 2, 0).reshape(g * g, C)
        low, iou = self.twin.decode(feats, point_coords[0], point_labels[0], g)
        sel = slice(1, 4) if multimask_output else slice(0, 1)
        low, iou = low[sel], iou[sel]
        logits = postprocess(low, g, self.input_size, self.original_size)
        self.last_logits, self.last_low_res = logits, low
        dev = self.features.device                         # the caller's device, as a predictor's outputs are
        return (logits if return_logits else logits > 0)[None].to(dev), iou[None].to(dev), low[None].to(dev)


# name, g, P, mixed labels, view H x W, and for the [h, w, 256] entry the map's h x w
CASES = [
    ("g8_p1", 8, 1, False, (20, 15), None),
    ("g8_p10", 8, 10, True, (15, 20), None),
    ("g8_p11", 8, 11, False, (33, 65), None),
    ("g8_p26", 8, 26, True, (64, 64), None),
    ("g8_p27", 8, 27, False, (20, 15), None),
    ("g8_p58", 8, 58, True, (15, 20), None),
    ("g8_map7x5", 8, 2, True, (28, 20), (7, 5)),
    ("g16_p2", 16, 2, True, (33, 65), None),
    ("g16_p11", 16, 11, True, (20, 15), None),
    ("g16_p58", 16, 58, False, (64, 64), None),
    ("g16_map24x32", 16, 3, False, (48, 64), (24, 32)),
    ("g64_p3", 64, 3, True, (100, 75), None),
]
GOLDEN_CASES = [c[0] for c in CASES if c[1] == 8]
WEIGHT_SEED = 7


@functools.lru_cache(maxsize=None)
def state_dict():
    return synthetic_state_dict(WEIGHT_SEED)


@functools.lru_cache(maxsize=None)
def case_inputs(name):
    """float64 CPU inputs of a case: dict(g, features | map, points, labels, H, W, input_size)."""
    i = [c[0] for c in CASES].index(name)
    _, g, P, mixed, (H, W), hw = CASES[i]
    gen = torch.Generator().manual_seed(100 + i)
    input_size, r = input_size_for(H, W, g)
    out = dict(g=g, H=H, W=W, input_size=input_size)
    if hw is None:
        f = torch.randn(g, g, C, generator=gen, dtype=torch.float64)
        rr = g / W if W > H else g / H
        vh, vw = int(H * rr), int(W * rr)                 # the valid region, zero padding right / below
        f[vh:] = 0
        f[:, vw:] = 0
        out["features"] = f.view(g * g, C)
    else:
        out["map"] = torch.randn(hw[0], hw[1], C, generator=gen, dtype=torch.float64)
    out["points"] = torch.stack([torch.randint(0, input_size[1], (P,), generator=gen),
                                 torch.randint(0, input_size[0], (P,), generator=gen)], -1).numpy().astype(np.int32)
    out["labels"] = (torch.randint(0, 2, (P,), generator=gen) if mixed else torch.ones(P, dtype=torch.long)) \
        .numpy().astype(np.int32)
    return out


@functools.lru_cache(maxsize=None)
def twin_outputs(name, dtype=torch.float64):
    """(low_res, iou, logits) of the twin in `dtype` on the CPU; computed once, do not modify."""
    x = case_inputs(name)
    t = Twin(state_dict(), dtype)
    feats = x["features"].to(dtype) if "features" in x else resize_pad(x["map"].to(dtype), x["g"])
    low, iou = t.decode(feats, x["points"], x["labels"], x["g"])
    return low, iou, postprocess(low, x["g"], x["input_size"], (x["H"], x["W"]))


def rel_err(got, want):
    return (got.double().cpu() - want).abs().max().item() / want.abs().max().item()


def decided(name):
    """The pixels of a case whose float64 logit is far enough from 0 to be the
    mask's business: |logit| > 1e-4 max|low_res|."""
    low, _, logits = twin_outputs(name)
    return logits.abs() > 1e-4 * low.abs().max()
