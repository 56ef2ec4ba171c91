// G.711 companding of 16-bit linear PCM, host and device: bitwise CPython 3.10's audioop.lin2ulaw / lin2alaw /
// ulaw2lin / alaw2lin at width 2, i.e. the arithmetic of Sun's g711.c.
//   mu-law  works on s >> 2 (14 bits): magnitude clipped to 8159, bias 33, 8 segments of 16 steps, all bits inverted
//   A-law   works on s >> 3 (13 bits): a negative s takes -(s >> 3) - 1, 8 segments, even bits inverted (0x55)
// The segment is the position of the magnitude's leading bit (count-leading-zeros instead of g711.c's table search).
// Integer arithmetic only: no table, so the same text serves the wire kernels' epilogue, the live-input staging and
// the host.  DESIGN §7.15; pinned exhaustively by tests/test_g711.py (host restatement) and tests/test_gpu_g711.py.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define MBV_G711_FN __host__ __device__ __forceinline__
#else
#define MBV_G711_FN inline
#endif

namespace mbv {

// the codec of a wire launch (MBV_G711_ULAW / MBV_G711_ALAW of the header); 0 = 16-bit linear, no codec
constexpr int kLawNone = 0;
constexpr int kLawUlaw = 1;
constexpr int kLawAlaw = 2;

MBV_G711_FN int g711_clz(unsigned v) {       // v > 0
#if defined(__HIP_DEVICE_COMPILE__)
  return __clz((int)v);
#else
  return __builtin_clz(v);
#endif
}

MBV_G711_FN uint8_t g711_ulaw_encode(int16_t s) {
  int v = (int)s >> 2;
  int mask = 0xFF;
  if (v < 0) { v = -v; mask = 0x7F; }
  if (v > 8159) v = 8159;
  v += 33;                                   // 33 <= v <= 8192: the leading bit is bit 5 .. 13
  const int seg = 26 - g711_clz((unsigned)v);
  if (seg >= 8) return (uint8_t)(0x7F ^ mask);
  return (uint8_t)(((seg << 4) | ((v >> (seg + 1)) & 0xF)) ^ mask);
}

MBV_G711_FN uint8_t g711_alaw_encode(int16_t s) {
  int v = (int)s >> 3;
  int mask = 0xD5;
  if (v < 0) { v = -v - 1; mask = 0x55; }    // 0 <= v <= 4095
  const int seg = v < 32 ? 0 : 27 - g711_clz((unsigned)v);
  return (uint8_t)(((seg << 4) | ((v >> (seg < 2 ? 1 : seg)) & 0xF)) ^ mask);
}

MBV_G711_FN int16_t g711_ulaw_decode(uint8_t b) {
  const int u = ~b & 0xFF;
  const int t = (((u & 0xF) << 3) + 0x84) << ((u & 0x70) >> 4);
  return (int16_t)((u & 0x80) ? 0x84 - t : t - 0x84);
}

MBV_G711_FN int16_t g711_alaw_decode(uint8_t b) {
  const int a = b ^ 0x55;
  const int seg = (a & 0x70) >> 4;
  int t = (a & 0xF) << 4;
  if (seg == 0) t += 8;
  else t = (t + 0x108) << (seg - 1);
  return (int16_t)((a & 0x80) ? t : -t);
}

template <int LAW>
MBV_G711_FN uint8_t g711_encode(int16_t s) {
  static_assert(LAW == kLawUlaw || LAW == kLawAlaw, "mu-law or A-law");
  return LAW == kLawUlaw ? g711_ulaw_encode(s) : g711_alaw_encode(s);
}

template <int LAW>
MBV_G711_FN int16_t g711_decode(uint8_t b) {
  static_assert(LAW == kLawUlaw || LAW == kLawAlaw, "mu-law or A-law");
  return LAW == kLawUlaw ? g711_ulaw_decode(b) : g711_alaw_decode(b);
}

}  // namespace mbv
