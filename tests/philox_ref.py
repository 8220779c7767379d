"""numpy restatement of the seeded perturb contract (include/samnerf_hip.h,
samnerf_model.perturb_device): Philox4x32-10 and the perturbed positions.  The
reference of tests/test_perturb_philox.py and tests/test_gpu_perturb_philox.py;
it shares no code with csrc/philox.h."""
import numpy as np
import torch

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF                     # for Python integers
U32 = np.uint64(MASK)                 # for uint64 arrays


def philox4x32_10(counter, key):
    """counter [..., 4], key [..., 2] (anything that broadcasts to uint32) ->
    the four output words [..., 4] uint32."""
    c = [v & U32 for v in np.moveaxis(np.asarray(counter, np.uint64), -1, 0)]
    k = [v & U32 for v in np.moveaxis(np.asarray(key, np.uint64), -1, 0)]
    c = list(np.broadcast_arrays(*c, *k)[:4])
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]                  # < 2^64: no overflow
        s32 = np.uint64(32)
        c = [(p1 >> s32) ^ c[1] ^ k[0], p1 & U32, (p0 >> s32) ^ c[3] ^ k[1], p0 & U32]
        k = [(k[0] + np.uint64(W0)) & U32, (k[1] + np.uint64(W1)) & U32]
    return np.stack(c, -1).astype(np.uint32)


def words(seed, offset, stage, rays, n):
    """The raw words of values 0..n-1 of `stage` for each ray: [len(rays), n] uint32."""
    rays = np.asarray(rays, np.uint64).reshape(-1, 1)
    quads = np.arange((n + 3) // 4, dtype=np.uint64).reshape(1, -1)
    ctr = np.stack(np.broadcast_arrays(quads | np.uint64(stage << 16), rays, np.uint64(offset & MASK),
                                       np.uint64(offset >> 32)), -1)
    out = philox4x32_10(ctr, [seed & MASK, seed >> 32])            # [rays, quads, 4]
    return out.reshape(len(rays), -1)[:, :n]


def lin(num_steps, stage):
    """The unperturbed positions torch computes on the CPU (renderer.py:265, :97)."""
    n = int(num_steps[stage]) + 1
    if stage == 0:
        return torch.linspace(0, 1, n).numpy()
    return torch.linspace(0.5 / n, 1 - 0.5 / n, steps=n).numpy()


def positions(seed, offset, num_steps, stage, rays):
    """float32 [len(rays), num_steps[stage] + 1]: every op rounded to fp32."""
    n = int(num_steps[stage]) + 1
    r = (words(seed, offset, stage, rays, n) >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    assert r.dtype == np.float32
    base = lin(num_steps, stage).astype(np.float32)[None, :]
    if stage == 0:
        v = base + (r - np.float32(0.5)) / np.float32(n - 1)
        v = np.clip(v, np.float32(0), np.float32(1))
    else:
        v = base + (r - np.float32(0.5)) / np.float32(n)
    assert v.dtype == np.float32
    return v


def all_positions(seed, offset, num_steps, N):
    """(bins0, u1, u2) of rays 0..N-1, the layout of samnerf_perturb_fill."""
    return tuple(positions(seed, offset, num_steps, s, np.arange(N)) for s in range(3))
