// softmax_sum.h -- the one summation order of every softmax over the instance
// columns (mask_loss.hip, present.hip, evaluate.hip).
#pragma once

#include <stdint.h>

#include <hip/hip_runtime.h>

namespace samnerf {

constexpr uint32_t kTreeLanes = 32;

// The sum of t[0..32) as the tree of a 32-lane butterfly: t[i] += t[i + off] for
// off = 16, 8, 4, 2, 1.  With the entries past K zero this is the order of
// ATen's softmax kernels on the GPU (one lane per instance, next_pow2(K)
// lanes, xor-shuffles), so the step's softmax and its backward give the bits
// the torch ops of mask_train_step give.  Static indices: t stays in VGPRs.
__device__ __forceinline__ float tree_sum32(float (&t)[kTreeLanes]) {
#pragma unroll
    for (uint32_t off = kTreeLanes / 2; off > 0; off >>= 1) {
#pragma unroll
        for (uint32_t i = 0; i < off; ++i) t[i] += t[i + off];
    }
    return t[0];
}

}  // namespace samnerf
