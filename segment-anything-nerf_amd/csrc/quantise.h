// quantise.h -- a rendered channel as a byte, shared by the kernels that hand
// images to 8-bit consumers (evaluate.hip's dumps, teacher_image.hip's SAM
// input): numpy's (v * 255).astype(np.uint8) of an fp32 value in [0, 1] --
// the fp32 product, truncated.  Outside [0, 1] the result is the casts' and
// is not compared with numpy.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace samnerf {

__device__ __forceinline__ uint8_t to_u8(float v) { return (uint8_t)(int)(v * 255.0f); }

}  // namespace samnerf
