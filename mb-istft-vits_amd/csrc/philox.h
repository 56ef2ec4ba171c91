// The seeded noise generator, shared by the fill kernel (rng.hip) and the host entry mbv_randn_host.
// Philox4x32-10; key (seed & 0xffffffff, seed >> 32); counter (t >> 2, c, purpose, row).  The four output words give
// the normals of frames 4 (t >> 2) + 0 .. 3 of channel c: element (c, t) is lane t & 3 of block t >> 2, always.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mbv {

struct Philox4 { uint32_t w[4]; };

__host__ __device__ inline Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                                 uint32_t k1) {
  constexpr uint32_t kM0 = 0xD2511F53u, kM1 = 0xCD9E8D57u, kW0 = 0x9E3779B9u, kW1 = 0xBB67AE85u;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)kM0 * c0, p1 = (uint64_t)kM1 * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
    k0 += kW0; k1 += kW1;
  }
  return Philox4{{c0, c1, c2, c3}};
}

// the two uniforms of a word pair: u1 in (0, 1], u2 in [0, 1), both exact in fp32
__host__ __device__ inline float philox_u1(uint32_t wa) { return (float)((wa >> 8) + 1u) * 0x1p-24f; }
__host__ __device__ inline float philox_u2(uint32_t wb) { return (float)(wb >> 8) * 0x1p-24f; }

}  // namespace mbv
