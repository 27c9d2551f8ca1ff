// Keyed sampler noise (`sample_seed`): the raw normals of one `_draw`, a function of (seed, sample id, run, draw, atom)
// alone - so a molecule gets the same noise whatever its row, its batch's size and padded width, or its rank.
//
// Counter-based Philox4x32-10 (Salmon, Moraes, Dror, Shaw, SC'11), key = (seed lo32, seed hi32),
// counter = (sample_id, draw, atom, (run << 8) | block), block 0..2.  Each block's 4 words give 4 normals by Box-Muller on
// (w0,w1) and (w2,w3):  u1 = ((w_even >> 8) + 1) 2^-24,  u2 = (w_odd >> 8) 2^-24,  r = sqrt(-2 ln u1),
// z_even = r cos(2 pi u2),  z_odd = r sin(2 pi u2).  Normal q = 4*block + j is channel q: 0..2 = x, 3..10 = h, 11 unused.
// The full statement is in include/mlconfgen_hip.h and DESIGN.md section 6; ml_conformer_generator_amd/seeding.py holds
// the host Philox (molecule sizes).
//
// One lane per (molecule, padded atom, block): no cross-lane work, so every lane runs the same instructions on its own
// counter and the value of a slot cannot depend on where the molecule sits in the plan.  Padded slots get exact zeros.
#include "mcg_common.h"
#include "mcg_api_internal.h"
#include "mcg_philox.h"

namespace {

using mcg_philox::philox4x32_10;
constexpr int kNoiseThreads = 256;

__device__ __forceinline__ void box_muller(uint32_t w_even, uint32_t w_odd, float& z_even, float& z_odd) {
    const float u1 = (float)((w_even >> 8) + 1u) * 0x1p-24f;     // (0, 1]: exact, 24 bits
    const float u2 = (float)(w_odd >> 8) * 0x1p-24f;             // [0, 1)
    const float r = sqrtf(-2.0f * logf(u1));
    float s, c;
    sincosf(6.28318530717958647692f * u2, &s, &c);
    z_even = r * c;
    z_odd = r * s;
}

__global__ __launch_bounds__(kNoiseThreads) void k_noise_keyed(const int64_t* __restrict__ sample_ids,
                                                                const int* __restrict__ n_nodes, int B, int N,
                                                                uint32_t k0, uint32_t k1, uint32_t run, uint32_t draw,
                                                                float* __restrict__ rx, float* __restrict__ rh) {
    const int t = blockIdx.x * kNoiseThreads + threadIdx.x;
    if (t >= B * N * 3) return;
    const int b = t / (N * 3), rem = t - b * (N * 3), i = rem / 3, blk = rem - i * 3;
    float z[4] = {0.f, 0.f, 0.f, 0.f};
    if (i < n_nodes[b]) {
        const uint4 w = philox4x32_10(make_uint4((uint32_t)sample_ids[b], draw, (uint32_t)i, (run << 8) | (uint32_t)blk),
                                      k0, k1);
        box_muller(w.x, w.y, z[0], z[1]);
        box_muller(w.z, w.w, z[2], z[3]);
    }
    float* xo = rx + ((size_t)b * N + i) * 3;
    float* ho = rh + ((size_t)b * N + i) * 8;
    if (blk == 0) {                       // channels 0..3: x0 x1 x2 h0
        xo[0] = z[0]; xo[1] = z[1]; xo[2] = z[2]; ho[0] = z[3];
    } else if (blk == 1) {                // channels 4..7: h1..h4
        ho[1] = z[0]; ho[2] = z[1]; ho[3] = z[2]; ho[4] = z[3];
    } else {                              // channels 8..10: h5..h7 (the 12th normal is discarded)
        ho[5] = z[0]; ho[6] = z[1]; ho[7] = z[2];
    }
}

}  // namespace

extern "C" int mcg_sampler_noise_keyed(const mcg_plan* pl, uint64_t seed, const int64_t* sample_ids_dev, uint32_t run,
                                       uint32_t draw, float* randn_x, float* randn_h, void* stream) {
    if (!pl || !sample_ids_dev || !randn_x || !randn_h) {
        mcg_set_error("mcg_sampler_noise_keyed: null plan, sample ids or output");
        return MCG_ERR_ARG;
    }
    if (run >= (1u << 24)) {
        mcg_set_error("mcg_sampler_noise_keyed: run %u does not fit 24 bits", run);
        return MCG_ERR_ARG;
    }
    const int B = mcg_plan_B(pl), N = mcg_plan_N(pl);
    const long long lanes = (long long)B * N * 3;       // plans are capped at 1e6 atoms: far below INT_MAX
    if (lanes <= 0) return MCG_OK;
    hipLaunchKernelGGL(k_noise_keyed, dim3((unsigned)((lanes + kNoiseThreads - 1) / kNoiseThreads)), dim3(kNoiseThreads),
                       0, (hipStream_t)stream, sample_ids_dev, mcg_plan_n_nodes(pl), B, N, (uint32_t)(seed & 0xffffffffu),
                       (uint32_t)(seed >> 32), run, draw, randn_x, randn_h);
    MCG_HIP(hipGetLastError());
    mcg_plan_mark_done(pl, stream);
    return MCG_OK;
}
