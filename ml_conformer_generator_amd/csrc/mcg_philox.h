// Counter-based Philox4x32-10 (Salmon, Moraes, Dror, Shaw, SC'11) on the device, shared by the keyed sampler noise
// (mcg_noise.hip) and the keyed pose starts (mcg_pose_search.hip): one text, so both streams are the generator that
// ml_conformer_generator_amd/seeding.py restates on the host.  Integer work only.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mcg_philox {

constexpr uint32_t kPhiloxM0 = 0xD2511F53u, kPhiloxM1 = 0xCD9E8D57u;
constexpr uint32_t kPhiloxW0 = 0x9E3779B9u, kPhiloxW1 = 0xBB67AE85u;

__device__ __forceinline__ uint4 philox4x32_10(uint4 c, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        if (r) { k0 += kPhiloxW0; k1 += kPhiloxW1; }
        const uint32_t hi0 = __umulhi(kPhiloxM0, c.x), lo0 = kPhiloxM0 * c.x;
        const uint32_t hi1 = __umulhi(kPhiloxM1, c.z), lo1 = kPhiloxM1 * c.z;
        c = make_uint4(hi1 ^ c.y ^ k0, lo1, hi0 ^ c.w ^ k1, lo0);
    }
    return c;
}

}  // namespace mcg_philox
