"""Stand-ins for segment-anything's SamPredictor in the teacher tests: the
fields and calls samnerf_amd.teacher.set_image_from_render drives, with every
assignment logged in order, and an image encoder that is a fixed function of
its input."""
import types

import torch
import torch.nn.functional as F

from golden_file import loader

golden = loader("teacher.npz")
GOLDEN_CASES = [(0, 23), (1, 64)]           # (index, target): (5,7)->(16,23) and (100,75)->(64,48)


def render_of(u8):
    """An fp32 render whose quantisation is the uint8 image: the middle of each byte's interval."""
    return ((torch.as_tensor(u8).to(torch.float32) + 0.5) / 255.0).contiguous()


class StubEncoder:
    """Average-pool the [1, 3, S, S] input to 64 x 64, then a fixed 3 -> 256
    matrix: [1, 256, 64, 64].  tuple_out: return (features, [interm]) as
    HQ-SAM's encoder does."""
    def __init__(self, tuple_out=False):
        self.tuple_out = tuple_out
        self.seen = []
        g = torch.Generator().manual_seed(5)
        self.matrix = torch.randn(256, 3, generator=g)

    def __call__(self, x):
        self.seen.append(x)
        if self.matrix.device != x.device:
            self.matrix = self.matrix.to(x.device)       # once: later calls copy nothing from the host
        pooled = F.adaptive_avg_pool2d(x, 64)
        feats = torch.einsum("oc,bchw->bohw", self.matrix, pooled).contiguous()
        return (feats, [pooled]) if self.tuple_out else feats


class StubPredictor:
    """SamPredictor's image state.  log: the names in the order they were set."""

    def __init__(self, tuple_out=False, with_buffers=False):
        object.__setattr__(self, "log", [])
        self.model = types.SimpleNamespace(image_encoder=StubEncoder(tuple_out))
        if with_buffers:
            self.model.pixel_mean = torch.tensor([100.0, 110.0, 120.0]).view(-1, 1, 1)
            self.model.pixel_std = torch.tensor([50.0, 60.0, 70.0]).view(-1, 1, 1)
        self.log.clear()

    def __setattr__(self, name, value):
        if not name.startswith("_"):
            self.log.append(name)
        object.__setattr__(self, name, value)

    def reset_image(self):
        self.log.append("reset_image()")
        for k in ("is_image_set", "features", "interm_features", "original_size", "input_size"):
            object.__setattr__(self, k, None)
        object.__setattr__(self, "is_image_set", False)
