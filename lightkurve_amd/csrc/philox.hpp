// philox.hpp — the counter-based normal generator shared by overfit.hip (noise light curves of the over-fitting metric) and
// fillgaps.hip (flux of inserted cadences): Philox4x32-10 (Salmon et al. 2011) and Box-Muller on 53-bit uniforms built from
// the four output words.  Any counter gets the same number whatever the launch shape; tests/overfit_cases.normals restates it.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

namespace lk {

// ------------------------------------------------------------------------------------------------ Philox4x32-10
struct Philox4 {
    uint32_t x[4];
};

__host__ __device__ inline Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return Philox4{{c0, c1, c2, c3}};
}

// two standard normals from one Philox call: u1 in (0, 1], u2 in [0, 1), both exact multiples of 2^-53
__device__ __forceinline__ void philox_normal_pair(const Philox4 &p, double &a, double &b) {
    const uint64_t w1 = (((uint64_t)(p.x[0] >> 5)) << 26) + (p.x[1] >> 6) + 1u;
    const uint64_t w2 = (((uint64_t)(p.x[2] >> 5)) << 26) + (p.x[3] >> 6);
    const double u1 = (double)w1 * 0x1p-53, u2 = (double)w2 * 0x1p-53;
    const double r = sqrt(-2.0 * log(u1));
    const double ang = 6.283185307179586 * u2;
    double s, c;
    sincos(ang, &s, &c);
    a = r * c;
    b = r * s;
}

}  // namespace lk
