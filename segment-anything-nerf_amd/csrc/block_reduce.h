// block_reduce.h -- the workgroup reductions of the kernels that run after a
// render (mask_loss, present, evaluate, batch_sampler .hip).  A workgroup is
// whole 64-lane waves: lane 0 of wave w leaves the wave's value in an LDS slot
// sh[w], and after a barrier the slots are combined.  Two floating sums whose
// orders are part of their results' bits -- block_sum_tree (float, mask_loss)
// and block_sum_ordered (double, evaluate) -- and the order-free ones (min,
// max, any as a max, an integer arg-max) from wave_all / waves_put /
// waves_fold with the caller's combiner.  rgb_train.hip's wave_sum is none of
// these: a DPP reduction in another order with a wave-uniform result.
#pragma once

#include <stdint.h>

#include <hip/hip_runtime.h>

namespace samnerf {

// v over the wave, lane l adding lane l + 32, 16, .. 1: the sum is in lane 0
__device__ __forceinline__ float wave_sum_down(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

// four waves' sums in the tree's order
__device__ __forceinline__ float sum_waves4(const float* w) { return (w[0] + w[1]) + (w[2] + w[3]); }

// The sum of v over a 256-thread workgroup, in every thread.  The first barrier
// lets the last call's readers finish: calls may follow each other on one sh[4].
__device__ __forceinline__ float block_sum_tree(float v, float* sh) {
    v = wave_sum_down(v);
    __syncthreads();                                   // sh may still be read from the last call
    if ((threadIdx.x & 63u) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return sum_waves4(sh);
}

// op over the wave's 64 lanes as an xor butterfly: every lane gets the result
template <typename T, typename Op>
__device__ __forceinline__ T wave_all(T v, Op op) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = op(v, __shfl_xor(v, o, 64));
    return v;
}

// N order-free values a thread at once: op(j, a, b) combines slot j
template <uint32_t N, typename Op>
__device__ __forceinline__ void wave_all(float (&v)[N], Op op) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (uint32_t j = 0; j < N; ++j) v[j] = op(j, v[j], __shfl_xor(v[j], o, 64));
    }
}

// lane 0 of each wave: the wave's value(s) into sh[wave] / sh[N wave + j].  No
// barrier here: one must stand between this and the reads of sh.
template <typename T>
__device__ __forceinline__ void waves_put(T v, T* sh) {
    if ((threadIdx.x & 63u) == 0) sh[threadIdx.x >> 6] = v;
}

template <uint32_t N>
__device__ __forceinline__ void waves_put(const float (&v)[N], float* sh) {
    if ((threadIdx.x & 63u) == 0) {
        float* o = sh + N * (threadIdx.x >> 6);
#pragma unroll
        for (uint32_t j = 0; j < N; ++j) o[j] = v[j];
    }
}

// the slots of `waves` waves combined in index order
template <typename T, typename Op>
__device__ __forceinline__ T waves_fold(const T* sh, uint32_t waves, Op op) {
    T a = sh[0];
    for (uint32_t w = 1; w < waves; ++w) a = op(a, sh[w]);
    return a;
}

// waves 1 .. of the N-slot form into v, which holds wave 0's values on entry: a
// thread of wave 0 after wave_all, or sh[0..N) read back
template <uint32_t N, typename Op>
__device__ __forceinline__ void waves_fold(float (&v)[N], const float* sh, uint32_t waves, Op op) {
    for (uint32_t w = 1; w < waves; ++w) {
#pragma unroll
        for (uint32_t j = 0; j < N; ++j) v[j] = op(j, v[j], sh[N * w + j]);
    }
}

// The sum of v over the workgroup (blockDim.x / 64 waves): the waves' xor
// butterflies, then the waves in index order; valid in thread 0.  Barriers
// after the waves' stores and after the reads of sh: sh may be reused at once,
// and what the threads stored to LDS before the call is visible after it
// (k_eval_rgb's min / max slots rely on that).
__device__ __forceinline__ double block_sum_ordered(double v, double* sh) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63u) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    double a = sh[0];
    for (uint32_t w = 1; w < (blockDim.x >> 6); ++w) a += sh[w];
    __syncthreads();
    return a;
}

}  // namespace samnerf
