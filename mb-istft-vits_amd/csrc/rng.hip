// Seeded device noise: standard normals as a pure function of (seed, purpose, row, channel, frame).
// One launch fills every block of a table; the consumers keep reading plain noise buffers.
#include "kernels.h"
#include "philox.h"

#include <cmath>

namespace mbv {

namespace {

// Box-Muller on one word pair: (even lane, odd lane) = r (cos, sin)(2 pi u2), r = sqrt(-2 ln u1).  Accurate libm
// calls only (no intrinsics): the values are part of the contract.
__device__ inline void normal_pair(uint32_t wa, uint32_t wb, float* even, float* odd) {
  const float r = sqrtf(-2.f * logf(philox_u1(wa)));
  float sn, cs;
  sincospif(2.f * philox_u2(wb), &sn, &cs);
  *even = r * cs;
  *odd = r * sn;
}

// the host's sincospi: x in [0, 2) on a 2^-23 grid, reduced exactly to |r| <= 1/4 around a multiple of 1/2
inline void host_sincospi(float x, float* sn, float* cs) {
  const float q = rintf(2.f * x);
  const float r = x - 0.5f * q;                                  // exact
  const float a = (float)((double)r * 3.14159265358979323846);
  const float s0 = sinf(a), c0 = cosf(a);
  switch ((int)q & 3) {
    case 0: *sn = s0; *cs = c0; break;
    case 1: *sn = c0; *cs = -s0; break;
    case 2: *sn = -s0; *cs = -c0; break;
    default: *sn = -c0; *cs = s0; break;
  }
}

inline void host_normal_pair(uint32_t wa, uint32_t wb, float* even, float* odd) {
  const float r = sqrtf(-2.f * logf(philox_u1(wa)));
  float sn, cs;
  host_sincospi(2.f * philox_u2(wb), &sn, &cs);
  *even = r * cs;
  *odd = r * sn;
}

// One thread = one Philox call = the (up to) four frames of one Philox block of one channel of one table row.
// Work items of a row run frame-fastest, so a wavefront stores 64 consecutive quads: 1 KiB, contiguous.
__global__ __launch_bounds__(256) void randn_blocks_kernel(const RandnRow* __restrict__ rows, int n, int64_t total) {
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (gid >= total) return;
  int lo = 0, hi = n - 1;                   // the row that holds gid: the last with begin <= gid (begins increase)
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (rows[mid].begin <= gid) lo = mid; else hi = mid - 1;
  }
  const RandnRow k = rows[lo];
  const int64_t local = gid - k.begin;
  const int64_t c = local / k.quads;
  const int64_t blk = (int64_t)(k.first >> 2) + (local - c * k.quads);
  const Philox4 p = philox4x32_10((uint32_t)blk, (uint32_t)c, k.purpose, k.row, k.seed_lo, k.seed_hi);
  float v[4];
  normal_pair(p.w[0], p.w[1], &v[0], &v[1]);
  normal_pair(p.w[2], p.w[3], &v[2], &v[3]);
  const int64_t t0 = 4 * blk, end = (int64_t)k.first + k.count;
  float* base = k.dst + c * k.stride;
  const int64_t off = t0 - k.first;         // negative only for lanes below `first`, which are not stored
  if (t0 >= k.first && t0 + 4 <= end && ((uintptr_t)(base + off) & 15) == 0) {
    *reinterpret_cast<float4*>(base + off) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (t0 + j >= k.first && t0 + j < end) base[off + j] = v[j];
  }
}

}  // namespace

void launch_randn_blocks(const RandnRow* rows, int n, int64_t total, hipStream_t s) {
  const unsigned grid = (unsigned)((total + 255) / 256);
  hipLaunchKernelGGL(randn_blocks_kernel, dim3(grid), dim3(256), 0, s, rows, n, total);
}

void randn_host(uint64_t seed, uint32_t purpose, uint32_t row, uint32_t c, int64_t first, int64_t count, float* dst) {
  const int64_t end = first + count;
  for (int64_t blk = first >> 2; 4 * blk < end; ++blk) {
    const Philox4 p = philox4x32_10((uint32_t)blk, c, purpose, row, (uint32_t)seed, (uint32_t)(seed >> 32));
    float v[4];
    host_normal_pair(p.w[0], p.w[1], &v[0], &v[1]);
    host_normal_pair(p.w[2], p.w[3], &v[2], &v[3]);
    for (int j = 0; j < 4; ++j) {
      const int64_t t = 4 * blk + j;
      if (t >= first && t < end) dst[t - first] = v[j];
    }
  }
}

}  // namespace mbv
