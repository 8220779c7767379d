// heads.h -- the SAM and mask heads' host entry points as the fused render
// (raymarch.hip) calls them: defined in sam_head.hip, mask_head.hip and
// mask_head_train.hip, which include this header too, so the compiler checks
// each definition against the one declaration.
#pragma once

#include "samnerf_common.h"

namespace samnerf {

int sam_head_forward(const samnerf_model* m, const float* rows, uint32_t N, float* samvit,
                     float* packed, hipStream_t s, uint32_t ld = 256u, bool pack = true);
size_t sam_head_packed_floats();
int mask_head_forward(const samnerf_model* m, const GridDesc<16>& grid, const float* u_f, const float* w_f,
                      const float* geo_f, uint32_t N, float* out, RayTiles tiles, float* packed,
                      hipStream_t s);
size_t mask_head_packed_floats();
size_t mask_train_workspace_bytes(uint32_t N);
size_t mask_train_workspace_bytes(int mask_kind, uint32_t N);
int mask_train_forward(const samnerf_model* m, const GridDesc<16>& grid, const float* u_f, const float* w_f,
                       const float* geo_f, uint32_t N, RayTiles tiles, float* logits, void* ws,
                       size_t ws_bytes, hipStream_t s);
int mask_train_backward(const samnerf_model* m, const GridDesc<16>& grid, const float* u_f, const float* w_f,
                        const float* geo_f, uint32_t N, RayTiles tiles, const float* grad_logits,
                        float* const* grad_w, float* grad_m_grid, void* ws, size_t ws_bytes, hipStream_t s);
int adaptive_train_forward(const samnerf_model* m, const float* X, uint32_t N, float* logits, void* ws,
                           size_t ws_bytes, hipStream_t s);
int adaptive_train_backward(const samnerf_model* m, const float* X, uint32_t N, const float* grad_logits,
                            float* const* grad_w, void* ws, size_t ws_bytes, hipStream_t s);

}  // namespace samnerf
