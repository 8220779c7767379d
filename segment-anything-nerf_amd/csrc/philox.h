// philox.h -- the seeded source of perturb=True (samnerf_model.perturb_device):
// Philox4x32-10 and the two perturbed-position expressions, host and device.
// Every consumer -- the proposal kernels (prop_stages.hip), the training
// backward (rgb_train.hip), the fill kernel and the host entry point
// (perturb.hip) -- calls these; nothing restates the arithmetic.
//
// The contract (include/samnerf_hip.h): value i of stage s of ray `ray` is
// output word i & 3 of Philox4x32-10 under the key (seed lo, seed hi) at the
// counter ((i >> 2) | s << 16, ray, offset lo, offset hi); r = (word >> 8) *
// 2^-24; the position is the reference's expression (renderer.py:266-271,
// :97-101) with r in place of torch.rand_like, in fp32, one rounding per op
// (the library is built with -ffp-contract=off), the division a true division.
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SAMNERF_HD __host__ __device__ __forceinline__
#else
#define SAMNERF_HD inline
#endif

namespace samnerf {

struct Philox4 {
    uint32_t v[4];
};

// Key and the call's half of the counter, from (seed, offset)
struct PerturbKey {
    uint32_t k0, k1, c2, c3;
};

SAMNERF_HD PerturbKey make_perturb_key(uint64_t seed, uint64_t offset) {
    PerturbKey k;
    k.k0 = (uint32_t)(seed & 0xffffffffull);
    k.k1 = (uint32_t)(seed >> 32);
    k.c2 = (uint32_t)(offset & 0xffffffffull);
    k.c3 = (uint32_t)(offset >> 32);
    return k;
}

// Philox4x32-10 (Salmon et al., SC'11): ten rounds of two 32 x 32 -> 64
// multiplications, the key bumped by the Weyl constants between rounds.
SAMNERF_HD Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                 uint32_t k1) {
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    Philox4 r;
    r.v[0] = c0, r.v[1] = c1, r.v[2] = c2, r.v[3] = c3;
    return r;
}

// The four words that hold values 4 quad .. 4 quad + 3 of (stage, ray)
SAMNERF_HD Philox4 perturb_quad(const PerturbKey& k, uint32_t stage, uint32_t ray, uint32_t quad) {
    return philox4x32_10(quad | stage << 16, ray, k.c2, k.c3, k.k0, k.k1);
}

// Word w (0..3) of a quad by selects: a run-time index into the struct would
// put it in scratch memory on the device
SAMNERF_HD uint32_t philox_word(const Philox4& q, uint32_t w) {
    const uint32_t lo = (w & 1u) ? q.v[1] : q.v[0], hi = (w & 1u) ? q.v[3] : q.v[2];
    return (w & 2u) ? hi : lo;
}

// Value i of (stage, ray): one generator call
SAMNERF_HD uint32_t perturb_word(const PerturbKey& k, uint32_t stage, uint32_t ray, uint32_t i) {
    return philox_word(perturb_quad(k, stage, ray, i >> 2), i & 3u);
}

SAMNERF_HD float philox_uniform(uint32_t word) { return (float)(word >> 8) * 0x1p-24f; }

// Stage 0: clamp(lin0[i] + (r - 0.5) / T0, 0, 1), lin0 = linspace(0, 1, T0 + 1)
SAMNERF_HD float perturb_bin0(float lin, uint32_t word, uint32_t T0) {
    const float v = lin + (philox_uniform(word) - 0.5f) / (float)T0;
    return fminf(fmaxf(v, 0.0f), 1.0f);
}

// Stages 1 and 2: linu[j] + (r - 0.5) / T, linu = linspace(0.5 / T, 1 - 0.5 / T, T)
SAMNERF_HD float perturb_u(float lin, uint32_t word, uint32_t T) {
    return lin + (philox_uniform(word) - 0.5f) / (float)T;
}

}  // namespace samnerf
