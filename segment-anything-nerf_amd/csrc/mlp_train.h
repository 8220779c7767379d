// mlp_train.h -- the exact-fp32 MLP training core of the two training heads
// (sam_head_train.hip, mask_head_train.hip): one scheme, 16 rows per
// workgroup, every product an fp32 MFMA (an fma chain in k order,
// cdna_hip_programming.md "FP32-input MFMA"), the weights read from an
// L2-resident pack in fragment order.
//   pack_pair    one element of a layer's two packs (forward, transposed);
//   dense16      out[16 NT x 16] = A in[4 S x 16] for a workgroup's 16 rows:
//                every forward layer (wf pack) and every dX layer (wb pack);
//   dw_item / dw_mma / dw_rows / dw_row
//                dW = G^T X over the rows, one 32 x 32 output tile per wave on
//                v_mfma_f32_32x32x2_f32.
// What is layer-specific (bias, leaky_relu and its backward, the skip rows,
// where a finished dW tile goes) is a functor at the call site.
//
// mfma_chain: acc[m] += sum over KS k-steps s of A_m(s) B(s) on
// v_mfma_f32_16x16x4_f32: the A fragment of tile m at step s is Ap[m][s * 64],
// B(s) = bl[s * 64] (LDS).  The A loads of the next U steps are issued before
// the MFMAs of the current U (register double buffer), so a wave waits for L2
// once per chain instead of once per step: the first version, one load then
// its MFMA, left the SAM head's backward at ~380 us of L2 latency for 4,096
// rays.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace samnerf {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ f32x4 mfma16(float a, float b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

template <int MT, int U>
__device__ __forceinline__ void chain_load(float (&buf)[U][MT], const float* const (&Ap)[MT], int g) {
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
        for (int m = 0; m < MT; ++m) buf[u][m] = Ap[m][(g * U + u) * 64];
    // keep the whole group's loads ahead of the MFMAs that follow (the
    // scheduler otherwise sinks them between the MFMAs and reuses registers,
    // leaving ~2 steps of loads in flight)
    __builtin_amdgcn_sched_barrier(0);
}

template <int MT, int U>
__device__ __forceinline__ void chain_mfma(f32x4 (&acc)[MT], const float (&buf)[U][MT], const float* bl, int g) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const float b = bl[(g * U + u) * 64];
#pragma unroll
        for (int m = 0; m < MT; ++m) acc[m] = mfma16(buf[u][m], b, acc[m]);
    }
}

// Two register buffers in ping-pong, no copies between them (a rotating
// cur = nxt copy made the compiler wait for the fresh loads right after
// issuing them).  Past the last group the load repeats it (unused).
template <int MT, int KS, int U>
__device__ __forceinline__ void mfma_chain(f32x4 (&acc)[MT], const float* const (&Ap)[MT], const float* bl) {
    static_assert(KS % U == 0, "k-steps must split into groups of U");
    constexpr int G = KS / U;
    float b0[U][MT], b1[U][MT];
    chain_load<MT, U>(b0, Ap, 0);
#pragma unroll 1
    for (int g = 0; g < G; g += 2) {
        chain_load<MT, U>(b1, Ap, min(g + 1, G - 1));
        chain_mfma<MT, U>(acc, b0, bl, g);
        if (g + 1 < G) {
            chain_load<MT, U>(b0, Ap, min(g + 2, G - 1));
            chain_mfma<MT, U>(acc, b1, bl, g + 1);
        }
    }
}

// leaky_relu(0.01) and torch's in-place backward of it, from the result h:
// grad * (h > 0 ? 1 : slope)
__device__ __forceinline__ float leaky(float x) { return x >= 0.0f ? x : x * 0.01f; }
__device__ __forceinline__ float leaky_grad(float h, float d) { return h > 0.0f ? d : d * 0.01f; }

// The two packs of a layer W [out][in] with padded dims Kp (fan-in) and Op
// (fan-out), Kp * Op floats each:
//   wf[tile t < Op/16][step s < Kp/4][lane]: A of out = W x (16x16x4):
//     A[i = lane & 15][k = lane >> 4] = W[16t + i][4s + k]
//   wb[tile t < Kp/16][step s < Op/4][lane]: A of dx = W^T g:
//     A[i][k] = W[4s + k][16t + i]
// Element o of both, from weight(row, col), which returns 0 outside the
// logical shape.
template <typename Weight>
__device__ __forceinline__ void pack_pair(int Kp, int Op, uint32_t o, Weight weight, float& f, float& b) {
    const uint32_t lane = o & 63u, i = lane & 15u, k = lane >> 4, ts = o >> 6;
    {
        const uint32_t S = (uint32_t)Kp / 4u, t = ts / S, s = ts % S;
        f = weight((int)(16u * t + i), (int)(4u * s + k));
    }
    {
        const uint32_t S = (uint32_t)Op / 4u, t = ts / S, s = ts % S;
        b = weight((int)(4u * s + k), (int)(16u * t + i));
    }
}

// One dense layer over a workgroup's 16 rows: out[16 NT x ROWS] = A in[4 S x
// ROWS], A_layer the layer's pack (tile t at t * S * 64), in[(4s + k) * ROWS +
// j] in LDS.  Wave w of 4 takes the output tiles t = w, w + 4, .. (ADJACENT:
// MT w, MT w + 1, .., a wave's units and weights contiguous); tiles past NT
// repeat the last one and are dropped (the chain stays branch-free), a wave
// with no tile at all returns.  store(unit, j, value) once per live
// accumulator element; each is its own k-ordered fma chain, whatever the
// tile order.
template <int S, int NT, int ROWS = 16, bool ADJACENT = false, typename Store>
__device__ __forceinline__ void dense16(const float* __restrict__ A_layer, const float* in, int w, int lane,
                                        Store store) {
    static_assert(ROWS == 16, "the chain steps B by 64 floats: 4 k of 16 rows");
    constexpr int MT = (NT + 3) / 4;
    if (NT < 4 && w >= NT) return;
    const int j = lane & 15, k = lane >> 4;
    f32x4 acc[MT];
    const float* Ap[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        acc[m] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
        Ap[m] = A_layer + (size_t)min(ADJACENT ? MT * w + m : w + 4 * m, NT - 1) * S * 64 + lane;
    }
    mfma_chain<MT, S, 4>(acc, Ap, in + k * ROWS + j);
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        const int t = ADJACENT ? MT * w + m : w + 4 * m;
        if (t >= NT) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) store(16 * t + 4 * k + r, j, acc[m][r]);
    }
}

// dW_l[u][c] = sum over the rows r of G_l[u][r] X_l[c][r] in 32 x 32 output
// tiles: layer l has tiles_u[l] x tiles_k[l] of them, numbered layer by layer,
// k fastest.
template <int NL>
struct DwTiles {
    int tiles_u[NL], tiles_k[NL];
    __host__ __device__ constexpr int before(int l) const {      // tiles before layer l
        int b = 0;
        for (int i = 0; i < l; ++i) b += tiles_u[i] * tiles_k[i];
        return b;
    }
    __host__ __device__ constexpr int total() const { return before(NL); }
};
struct DwItem {
    int l, ut, kt;        // layer, 32-wide output-unit tile, 32-wide input tile
};
template <int NL>
__device__ __forceinline__ DwItem dw_item(const DwTiles<NL>& T, int tile) {
    int l = 0;
    while (l < NL - 1 && tile >= T.before(l + 1)) ++l;
    const int lt = tile - T.before(l);
    return DwItem{l, lt / T.tiles_k[l], lt % T.tiles_k[l]};
}

// acc (one tile, lane = (column i = lane & 31, half h = lane >> 5)) += the
// products of 8 rows.  The sum runs over rows, so the rows of an MFMA's k pair
// can be any two: half h of group m takes rows 8m + 4h .. +3 over four MFMAs,
// one 16-B load per operand (g, x: the lane's four G / X values).
__device__ __forceinline__ void dw_mma(f32x16& acc, const float4& g, const float4& x) {
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(g.x, x.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(g.y, x.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(g.z, x.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(g.w, x.w, acc, 0, 0, 0);
}

// The groups of ROWS rows in order, kDwU at a time through two register
// buffers in ping-pong (mfma_chain's scheme): a group's loads (g(m) / x(m))
// are in flight while the previous group's MFMAs run, where one load pair
// then its four MFMAs waited for L2 on every trip.  Past the last group the
// load repeats it (unused): anything that sums over the rows beside the MFMAs
// must sit where a group is consumed, not in a loader.  For long row runs
// (k_mt_dw: 1,024); k_ht_dw's one or two 256-row chunks per wave were faster
// without it.
constexpr int kDwU = 2;

template <int ROWS, typename LoadG, typename LoadX>
__device__ __forceinline__ void dw_rows(f32x16& acc, LoadG g, LoadX x) {
    static_assert(ROWS % (8 * kDwU) == 0, "rows go in groups of 8 x kDwU: others would be dropped silently");
    constexpr int G = ROWS / 8 / kDwU;
    auto load = [&](float4 (&ga)[kDwU], float4 (&xb)[kDwU], int grp) {
#pragma unroll
        for (int u = 0; u < kDwU; ++u) {
            ga[u] = g(grp * kDwU + u);
            xb[u] = x(grp * kDwU + u);
        }
        __builtin_amdgcn_sched_barrier(0);
    };
    auto mma = [&](const float4 (&ga)[kDwU], const float4 (&xb)[kDwU]) {
#pragma unroll
        for (int u = 0; u < kDwU; ++u) dw_mma(acc, ga[u], xb[u]);
    };
    float4 g0[kDwU], x0[kDwU], g1[kDwU], x1[kDwU];
    load(g0, x0, 0);
#pragma unroll 1
    for (int grp = 0; grp < G; grp += 2) {
        load(g1, x1, min(grp + 1, G - 1));
        mma(g0, x0);
        if (grp + 1 < G) {
            load(g0, x0, min(grp + 2, G - 1));
            mma(g1, x1);
        }
    }
}

// accumulator register q of lane half h holds row dw_row(q, h) of the tile
// (column lane & 31)
__device__ __forceinline__ int dw_row(int q, int h) { return (q & 3) + 8 * (q >> 2) + 4 * h; }

}  // namespace samnerf
