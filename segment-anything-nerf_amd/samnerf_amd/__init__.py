"""MI355X-native NeRF ray-march hot path (gfx950 HIP kernels behind a C ABI).

  ops       tensor-level wrappers of the C ABI (encoders + step kernels)
  fused     FusedRenderer: NeRFRenderer.run as five fused kernel launches
  dist      ray sharding over ranks + RCCL all-gather of output tiles
  batch     TrainBatchSampler: a training step's ray choice and collate gathers
  incoherent  the incoherent-region tables: from the GT masks, and the dynamic update
  feat_loss   the distillation loss: bilinear resize to the teacher's map + MSE
  teacher     the SAM teacher's input from a render on the device, set_image, the feature cache
"""
from ._lib import EXPORTED, LIB_PATH, SamnerfUnavailable, lib  # noqa: F401
