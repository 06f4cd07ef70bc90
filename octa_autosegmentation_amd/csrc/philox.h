// philox.h -- Philox-4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel Random Numbers: As Easy as 1, 2, 3", SC 2011), a counter-based generator
// in plain C++: 128 bits of counter and 64 bits of key in, four 32-bit words out, no state. A kernel that numbers its draws by WHAT they are for
// (sample, pixel, purpose) instead of by which thread makes them gets the same numbers under every launch geometry, and the same numbers again
// for the same key. Host code may include this header too (the functions are host + device).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define OCTA_PHILOX_FN __host__ __device__ __forceinline__
#else
#define OCTA_PHILOX_FN inline
#endif

namespace octa {

struct Philox4 {
    uint32_t v[4];
};

OCTA_PHILOX_FN Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
    constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u;      // the round multipliers
    constexpr uint32_t W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;      // the Weyl increments of the key (golden ratio, sqrt 3 - 1)
    for (int r = 0; r < 10; r++) {
        const uint64_t p0 = (uint64_t)M0 * c0, p1 = (uint64_t)M1 * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += W0;
        k1 += W1;
    }
    return Philox4{{c0, c1, c2, c3}};
}

// 32 random bits -> float in (0, 1]: (r + 0.5) 2^-32, rounded to float (the largest r round to 1.0; 0 is never returned, so log() is finite)
OCTA_PHILOX_FN float philox_unit(uint32_t r) { return ((float)r + 0.5f) * 2.3283064365386963e-10f; }

}  // namespace octa
