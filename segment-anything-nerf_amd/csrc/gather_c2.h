// gather_c2.h -- the C = 2 corner gathers of NL level slots in two halves
// (issue the loads, then the weighted sums): k_final's hash-grid lookup
// (final_stage.hip).
#pragma once

#include "samnerf_common.h"

using namespace samnerf;

namespace {

// Trilinear lookup of both channels of NL L16C2 levels whose descriptors
// differ between the half-waves (lane-varying; no divergent branch): the row
// of corner (x, y, z) is x + y*res + z*res^2 (dense) or (x ^ y*P1 ^ z*P2) &
// (size-1) (hashed), built from per-axis terms.  All 8*NL corner loads are
// issued before the first is consumed (one memory round trip per call; the
// compiler otherwise waits for each level before issuing the next).
// GatherC2: the gathered corner rows of NL levels (both channels) and their
// fractions, what gather_issue_c2 hands to gather_finish_c2, so a caller can
// put other work (k_final: the sample's position stores) between the two.
template <int NL>
struct GatherC2 {
    float2 e[NL][8];
    float fx[NL], fy[NL], fz[NL];
};

// Wave-uniform classes of the NL level slots of one call: bit l of `dense`
// = the level of slot l is dense in both half-waves, of `hashed` = hashed in
// both.  Such a slot skips the per-lane dense/hash selects, and a dense one
// fetches its x-adjacent corner pairs with one 16-B load each (the rows
// (x, y, z) and (x + 1, y, z) are adjacent).  Mixed slots keep the
// lane-varying form.
struct SlotKinds {
    uint32_t dense, hashed;
};

// Hashed slots of a LAY 1 k-block (k_final, round 6): the table base of each
// slot's half-wave-0 level (uniform), this lane's half-wave bit (0, or the
// byte distance to the next level) and the byte mask.  A corner's byte offset
// from the slot base is then X8 ^ Y8 ^ Z8 with the per-axis terms pre-shifted
// by 3 and pre-masked (AND distributes over XOR) and the half-wave bit folded
// into X8 (it sits above every masked bit): one v_xor_b32 per corner where
// v_bitop3 + v_add_lshl_u32 took 6.6 cycles (profiles/r5v_valu_rate.json).
// Same rows as the reference's (x ^ y P1 ^ z P2) & (S - 1) at offset off.
struct HashSlots {
    const char* base[4];
    uint32_t hx, m8;
};

// tap (parity taps only, samnerf_taps.rows2; null otherwise): the level-
// relative row each corner weight multiplies, tap[l * tap_ls + c] for slot l
// and corner c (bit 0 x, 1 y, 2 z, as gridencoder.cu:61-79 / the oracle's
// corner order) -- the rows the loads below read.  A dense pair's top cell
// reads (top - 1, top) with weights (0, 1), recorded as such.
template <int NL>
__device__ __forceinline__ void gather_issue_c2(const float2* __restrict__ emb, const LevelDesc* d,
                                                float ux, float uy, float uz, GatherC2<NL>& g,
                                                SlotKinds kinds = SlotKinds{0u, 0u},
                                                uint32_t* tap = nullptr, int tap_ls = 8,
                                                const HashSlots* hs = nullptr) {
    // byte offsets of every corner (dense-pair slots: of the 4 pairs) first,
    // then all loads, so they are in flight together
    uint32_t row[NL][8];
#pragma unroll
    for (int l = 0; l < NL; ++l) {
        uint32_t cx, cy, cz;
        locate_axis(ux, d[l], cx, g.fx[l]);
        locate_axis(uy, d[l], cy, g.fy[l]);
        locate_axis(uz, d[l], cz, g.fz[l]);
        const uint32_t top = d[l].res - 1u;
        const uint32_t ny = min(cy + 1u, top), nz = min(cz + 1u, top);
        if ((kinds.dense >> l) & 1u) {
            // pair (cx, cx + 1); in the top cell (cx = top, so fx = 0) the pair
            // (top - 1, top) is loaded and the x weights swapped (fx := 1):
            // corner 0 then adds 0 * row(top - 1), an exact no-op (the running
            // sum is never -0), and corner 1 adds row(top) with corner 0's
            // original weight (1 * wy) * wz -- the same bits as the reference
            const bool edge = cx == top;
            g.fx[l] = edge ? 1.0f : g.fx[l];
            const uint32_t bx = d[l].off + (edge ? cx - 1u : cx);
            const uint32_t r2 = d[l].res * d[l].res;
            const uint32_t Y[2] = {(uint32_t)__umul24(cy, d[l].res), (uint32_t)__umul24(ny, d[l].res)};
            const uint32_t Z[2] = {(uint32_t)__umul24(cz, r2), (uint32_t)__umul24(nz, r2)};
#pragma unroll
            for (int p = 0; p < 4; ++p) row[l][p] = (bx + Y[p & 1] + Z[p >> 1]) << 3;
        } else if (((kinds.hashed >> l) & 1u) && hs) {
            // byte offsets from the slot base hs->base[l] (HashSlots)
            const uint32_t m8 = hs->m8;
            const uint32_t X[2] = {(cx << 3) | hs->hx, ((uint32_t)min(cx + 1u, top) << 3) | hs->hx};
            const uint32_t Y[2] = {(cy * (kPrime1 << 3)) & m8, (ny * (kPrime1 << 3)) & m8};
            const uint32_t Z[2] = {(cz * (kPrime2 << 3)) & m8, (nz * (kPrime2 << 3)) & m8};
#pragma unroll
            for (int c = 0; c < 8; ++c) row[l][c] = X[c & 1] ^ Y[(c >> 1) & 1] ^ Z[c >> 2];
        } else if ((kinds.hashed >> l) & 1u) {
            const uint32_t mask = d[l].size - 1u;
            const uint32_t X[2] = {cx, min(cx + 1u, top)};
            const uint32_t Y[2] = {cy * kPrime1, ny * kPrime1};
            const uint32_t Z[2] = {cz * kPrime2, nz * kPrime2};
#pragma unroll
            for (int c = 0; c < 8; ++c)
                row[l][c] = (d[l].off + ((X[c & 1] ^ Y[(c >> 1) & 1] ^ Z[c >> 2]) & mask)) << 3;
        } else {
            const bool hashed = d[l].flags & kHashed;
            const uint32_t my = hashed ? kPrime1 : d[l].res, mz = hashed ? kPrime2 : d[l].res * d[l].res;
            // per-lane choice between the hashed and the dense row as a bitwise
            // blend on an opaque all-ones / zero mask: written as a select the
            // compiler turned each of the 8 corners into a divergent
            // exec-masked branch pair
            uint32_t hsel = hashed ? 0xffffffffu : 0u;
            asm volatile("" : "+v"(hsel));
            const uint32_t hmask = hsel & (d[l].size - 1u), dmask = ~hsel;
            const uint32_t X[2] = {cx, min(cx + 1u, top)};
            const uint32_t Y[2] = {cy * my, ny * my};
            const uint32_t Z[2] = {cz * mz, nz * mz};
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const uint32_t xs = X[c & 1], ys = Y[(c >> 1) & 1], zs = Z[c >> 2];
                row[l][c] = (d[l].off + (((xs ^ ys ^ zs) & hmask) | ((xs + ys + zs) & dmask))) << 3;
            }
        }
    }
    if (tap) {
#pragma unroll
        for (int l = 0; l < NL; ++l) {
            if ((kinds.dense >> l) & 1u) {
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    const uint32_t r0 = (row[l][p] >> 3) - d[l].off;
                    tap[l * tap_ls + 2 * p] = r0;
                    tap[l * tap_ls + 2 * p + 1] = r0 + 1u;
                }
            } else if (((kinds.hashed >> l) & 1u) && hs) {
#pragma unroll
                for (int c = 0; c < 8; ++c) tap[l * tap_ls + c] = (row[l][c] & hs->m8) >> 3;
            } else {
#pragma unroll
                for (int c = 0; c < 8; ++c) tap[l * tap_ls + c] = (row[l][c] >> 3) - d[l].off;
            }
        }
    }
    // 32-bit byte offsets from the uniform table base (saddr loads)
    const char* base = reinterpret_cast<const char*>(emb);
#pragma unroll
    for (int l = 0; l < NL; ++l) {
        if ((kinds.dense >> l) & 1u) {
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const f4a8 v = *reinterpret_cast<const f4a8*>(base + row[l][p]);
                g.e[l][2 * p] = make_float2(v.x, v.y);
                g.e[l][2 * p + 1] = make_float2(v.z, v.w);
            }
        } else {
            const char* lb = (((kinds.hashed >> l) & 1u) && hs) ? hs->base[l] : base;
#pragma unroll
            for (int c = 0; c < 8; ++c) g.e[l][c] = *reinterpret_cast<const float2*>(lb + row[l][c]);
        }
    }
}

// Weighted corner sums with the reference's weights (wx * wy) * wz.  PK: both
// channels on one v_pk_fma_f32 per corner (each lane the scalar fma: same
// bits).  The forms schedule differently: PK measured faster in k_final's
// S = 1 form (1.04 -> 1.00 ms per view), scalar in its prefetching S = 2 form
// (0.26 vs 0.29 ms at 32K rays).
template <int NL, bool PK = false>
__device__ __forceinline__ void gather_finish_c2(const GatherC2<NL>& g, float* f) {
#pragma unroll
    for (int l = 0; l < NL; ++l) {
        if constexpr (PK) {
            f2v wc[4];
            corner_weights_pk(g.fx[l], g.fy[l], g.fz[l], wc);
            f2v acc = {0.0f, 0.0f};
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const float w = corner_w(wc, c);
                acc = __builtin_elementwise_fma(f2v{w, w}, f2v{g.e[l][c].x, g.e[l][c].y}, acc);
            }
            f[2 * l] = acc.x;
            f[2 * l + 1] = acc.y;
        } else {
            f2v wc[4];
            corner_weights_pk(g.fx[l], g.fy[l], g.fz[l], wc);
            float f0 = 0.0f, f1 = 0.0f;
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const float w = corner_w(wc, c);
                f0 = __builtin_fmaf(w, g.e[l][c].x, f0);
                f1 = __builtin_fmaf(w, g.e[l][c].y, f1);
            }
            f[2 * l] = f0;
            f[2 * l + 1] = f1;
        }
    }
}

}  // namespace
