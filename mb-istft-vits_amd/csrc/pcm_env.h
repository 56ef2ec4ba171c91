// The gain envelope of the wire step as device code: shared by the wire kernels (resample.hip) and the time-warp
// kernel (warp.hip), which both multiply a model-rate sample where they read it.
#pragma once
#include "kernels.h"

namespace mbv {

// The gain envelope (kernels.h) at model-rate sample j >= 0 of its row: G[f] + w (G[f + 1] - G[f]) with
// f = j / hop and w = (float)(j - f hop) * inv_hop, every operation rounded to fp32 on its own (no fma: the NumPy
// restatement computes the same bits).  j < frames * hop (checked on the host), so f + 1 <= frames: inside the table.
// The toolchain's __fmul_rn / __fadd_rn are inline functions over the plain operators, compiled contractable: hipcc
// fuses them into an fma like any others.  The pragma is what keeps the product and the sum apart; it covers the
// operators written in this function (also after inlining), not those inside a function it calls
__device__ __forceinline__ float env_at(const PcmEnv& e, int64_t j) {
#pragma clang fp contract(off)
  int64_t f;
  int r;
  if (j < 0x80000000LL) {                                 // the common case: one 32-bit division
    const unsigned q = (unsigned)j / (unsigned)e.hop;
    f = q;
    r = (int)((unsigned)j - q * (unsigned)e.hop);
  } else {
    f = j / e.hop;
    r = (int)(j - f * e.hop);
  }
  const float g0 = e.gain[f], g1 = e.gain[f + 1];
  const float w = (float)r * e.inv_hop;
  const float d = g1 - g0;
  const float wd = w * d;
  return g0 + wd;
}

// the sample a shaped row stages: rounded once, before anything else reads it; a row without an envelope keeps v
__device__ __forceinline__ float env_mul(float v, const PcmEnv& e, int64_t j) {
#pragma clang fp contract(off)
  return e.gain ? v * env_at(e, j) : v;
}

}  // namespace mbv
