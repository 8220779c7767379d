// instance_row.h -- the one instance-probability row of everything that reads a
// render's instance_mask_logits (mask_loss.hip, present.hip, evaluate.hip,
// incoherent.hip): a ray's K logits to its K probabilities, the argmax of
// those, and the move of a workgroup's rows through LDS.
//
// n_inst > 1 is a softmax: mx = max of the logits starting from z[0],
// expf(z[k] - mx) summed as 32-lane trees (tree_sum32), and expf(z[k] - mx)
// evaluated again for the division by the sum; n_inst == 1 is the sigmoid
// 1 / (1 + expf(-z[k])) of each column.  The argmax starts from best = -1 and
// takes a column only where it is strictly greater: the first index wins a tie
// and a NaN is never taken.  Every kernel's bits are these expressions in this
// order; include/samnerf_hip.h (samnerf_present_frame, step 1) promises them.
#pragma once

#include <stdint.h>

#include <hip/hip_runtime.h>

namespace samnerf {

constexpr uint32_t kTreeLanes = 32;
constexpr uint32_t kMaxK = kTreeLanes;        // the columns of a one-tree row

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

// The softmax's two scalars of a row z[0..K), K <= 32 * Trees (global memory
// or LDS).  The tree of columns 32 .. 63 is added to the first one's sum, and only
// where K > 32: a K <= 32 row gives the same bits at Trees = 1 and 2.
struct RowNorm { float mx, sum; };

template <uint32_t Trees>
__device__ __forceinline__ RowNorm row_norm(const float* z, uint32_t K) {
    static_assert(Trees == 1 || Trees == 2, "one tree, or two for K up to 64");
    RowNorm n;
    n.mx = z[0];
    for (uint32_t k = 1; k < K; ++k) n.mx = fmaxf(n.mx, z[k]);
    float t[kTreeLanes];
#pragma unroll
    for (uint32_t k = 0; k < kTreeLanes; ++k) t[k] = k < K ? expf(z[k] - n.mx) : 0.0f;
    n.sum = tree_sum32(t);
    if (Trees == 2 && K > kTreeLanes) {
#pragma unroll
        for (uint32_t k = 0; k < kTreeLanes; ++k) t[k] = kTreeLanes + k < K ? expf(z[kTreeLanes + k] - n.mx) : 0.0f;
        n.sum += tree_sum32(t);
    }
    return n;
}

// column k of the softmax of z
__device__ __forceinline__ float row_prob(const float* z, uint32_t k, RowNorm n) { return expf(z[k] - n.mx) / n.sum; }

__device__ __forceinline__ float row_sigmoid(float z) { return 1.0f / (1.0f + expf(-z)); }

// the argmax in the making: take() the columns in index order
struct RowBest {
    float best = -1.0f;
    uint32_t arg = 0;
    __device__ __forceinline__ void take(uint32_t k, float v) {
        if (v > best) { best = v; arg = k; }           // the first index wins ties
    }
};

// The whole row in place, z[0..K) from logits to probabilities, and its argmax;
// each(k, p_k) sees every column on the argmax's pass.
template <uint32_t Trees, typename Each>
__device__ __forceinline__ RowBest instance_row(float* z, uint32_t K, uint32_t n_inst, Each each) {
    if (n_inst > 1) {
        const RowNorm n = row_norm<Trees>(z, K);
        for (uint32_t k = 0; k < K; ++k) z[k] = row_prob(z, k, n);
    } else {
        for (uint32_t k = 0; k < K; ++k) z[k] = row_sigmoid(z[k]);
    }
    RowBest b;
    for (uint32_t k = 0; k < K; ++k) {
        const float v = z[k];
        b.take(k, v);
        each(k, v);
    }
    return b;
}

template <uint32_t Trees>
__device__ __forceinline__ RowBest instance_row(float* z, uint32_t K, uint32_t n_inst) {
    return instance_row<Trees>(z, K, n_inst, [](uint32_t, float) {});
}

// A workgroup's cnt rows of K floats between memory (row-major, the first of
// them at rows[first]) and the LDS tile [cnt][Kp], Kp = K | 1: lane = dword in
// memory, and the odd row length lets each thread walk its own row without a
// bank conflict.  All T threads of the workgroup call; the caller's barriers
// stand between these and the threads' work on their rows.
__device__ __forceinline__ void rows_to_tile(float* tile, const float* rows, size_t first, uint32_t cnt, uint32_t K,
                                             uint32_t Kp, uint32_t T) {
    for (uint32_t e = threadIdx.x; e < cnt * K; e += T) {
        const uint32_t row = e / K;
        tile[row * Kp + (e - row * K)] = rows[first + e];
    }
}

__device__ __forceinline__ void tile_to_rows(float* rows, size_t first, const float* tile, uint32_t cnt, uint32_t K,
                                             uint32_t Kp, uint32_t T) {
    for (uint32_t e = threadIdx.x; e < cnt * K; e += T) {
        const uint32_t row = e / K;
        rows[first + e] = tile[row * Kp + (e - row * K)];
    }
}

}  // namespace samnerf
