// perturb.hip -- the seeded perturbed positions outside the render (philox.h
// holds the generator and the position expressions): the host entry point
// samnerf_perturb_host and the fill kernel samnerf_perturb_fill, which writes
// the arrays of samnerf_model.perturb that the seeded render never forms.
#include "philox.h"
#include "render_args.h"
#include "samnerf_common.h"

using namespace samnerf;

namespace {

struct FillArgs {
    PerturbKey key;
    uint32_t N;
    uint32_t n[3];         // values per ray of each stage
    uint32_t q[3];         // quads per ray of each stage
    Lin lin[3];            // the unperturbed positions
    float* out[3];         // [N][n[s]], or null
};

// One thread per (ray, quad): one generator call, up to four stores.
__global__ void __launch_bounds__(256) k_perturb_fill(FillArgs a) {
    const uint32_t qs = a.q[0] + a.q[1] + a.q[2];
    const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (t >= (uint64_t)a.N * qs) return;
    const uint32_t ray = (uint32_t)(t / qs);
    uint32_t quad = (uint32_t)(t % qs), s = 0;
    if (quad >= a.q[0]) quad -= a.q[0], s = 1;
    if (s == 1 && quad >= a.q[1]) quad -= a.q[1], s = 2;
    const uint32_t n = s == 0 ? a.n[0] : s == 1 ? a.n[1] : a.n[2];
    float* out = s == 0 ? a.out[0] : s == 1 ? a.out[1] : a.out[2];
    if (!out) return;
    Lin lin = a.lin[0];
    if (s == 1) lin = a.lin[1];
    if (s == 2) lin = a.lin[2];
    const Philox4 w = perturb_quad(a.key, s, ray, quad);
#pragma unroll
    for (uint32_t e = 0; e < 4; ++e) {
        const uint32_t i = quad * 4u + e;
        if (i >= n) break;
        const float l = lin((int)i);
        out[(size_t)ray * n + i] = s == 0 ? perturb_bin0(l, w.v[e], n - 1u) : perturb_u(l, w.v[e], n);
    }
}

bool steps_ok(const uint32_t* num_steps) {
    for (int s = 0; s < 3; ++s)
        if (num_steps[s] < 1u || num_steps[s] > 65535u) return false;
    return true;
}

// start and end of a stage's unperturbed positions (renderer.py:265, :97: the
// bounds of u are Python doubles rounded to float)
void stage_range(uint32_t stage, uint32_t n, float& start, float& end) {
    start = stage == 0 ? 0.0f : (float)(0.5 / n);
    end = stage == 0 ? 1.0f : (float)(1.0 - 0.5 / n);
}

}  // namespace

extern "C" {

int samnerf_perturb_host(uint64_t seed, uint64_t offset, const uint32_t* num_steps, uint32_t stage,
                         uint32_t ray, float* out) {
    if (!num_steps || !out) return fail(SAMNERF_EINVAL, "perturb_host: null pointer");
    if (stage > 2) return fail(SAMNERF_EINVAL, "perturb_host: stage %u outside 0..2", stage);
    if (!steps_ok(num_steps)) return fail(SAMNERF_EINVAL, "perturb_host: num_steps outside 1..65535");
    const uint32_t n = num_steps[stage] + 1u;
    float start, end;
    stage_range(stage, n, start, end);
    samnerf_linspace_host(start, end, n, out);
    const PerturbKey key = make_perturb_key(seed, offset);
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t w = perturb_word(key, stage, ray, i);
        out[i] = stage == 0 ? perturb_bin0(out[i], w, n - 1u) : perturb_u(out[i], w, n);
    }
    return SAMNERF_OK;
}

int samnerf_perturb_fill(uint64_t seed, uint64_t offset, uint32_t N, const uint32_t* num_steps, float* bins0,
                         float* u1, float* u2, samnerf_stream_t stream) {
    if (!num_steps) return fail(SAMNERF_EINVAL, "perturb_fill: null pointer");
    if (!steps_ok(num_steps)) return fail(SAMNERF_EINVAL, "perturb_fill: num_steps outside 1..65535");
    if (N == 0 || (!bins0 && !u1 && !u2)) return SAMNERF_OK;
    FillArgs a{};
    a.key = make_perturb_key(seed, offset);
    a.N = N;
    a.out[0] = bins0, a.out[1] = u1, a.out[2] = u2;
    uint32_t qs = 0;
    for (uint32_t s = 0; s < 3; ++s) {
        a.n[s] = num_steps[s] + 1u;
        a.q[s] = (a.n[s] + 3u) / 4u;
        qs += a.q[s];
        float start, end;
        stage_range(s, a.n[s], start, end);
        a.lin[s] = make_lin(start, end, a.n[s]);
    }
    const uint64_t blocks = ((uint64_t)N * qs + 255u) / 256u;
    if (blocks > 0x7fffffffull) return fail(SAMNERF_EINVAL, "perturb_fill: too many rays");
    k_perturb_fill<<<(uint32_t)blocks, 256, 0, reinterpret_cast<hipStream_t>(stream)>>>(a);
    return check_launch("perturb_fill");
}

}  // extern "C"
