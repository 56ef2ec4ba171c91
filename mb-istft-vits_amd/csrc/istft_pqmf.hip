// Fused waveform tail: subband_conv_post output -> 22.05 kHz waveform in ONE
// launch (HBM-bound: 4608 B read + 1024 B written per z-frame).
//
//   spec  = exp(x[:, :, :9]) ; phase = pi * sin(x[:, :, 9:])          models.py:368-369
//   y_mb  = istft(spec * e^{j phase}, n_fft 16, hop 4, hann, center)   stft.py:197-202
//   o     = conv1d(pad31(zero_stuff4(y_mb) * 4), h_syn)                pqmf.py:115-116
//           (MS: h_syn = weight-normed multistream_conv_post)         models.py:463-465
//
// One workgroup owns TM sub-band samples per band (4*TM output samples) of
// one utterance and runs three phases separated by barriers:
//   A  one lane per (band, frame): 18 coalesced loads down the frame axis,
//      exp / sin / sincos, 16-point real inverse DFT (even/odd-bin split),
//      hann window -> LDS  fr[band][n][frame]
//   B  one lane per sub-band time index (all 4 bands): overlap-add of the 4
//      frames that cover it, divide by the edge-aware sum of squared windows
//      (what torch.istft does), zero outside the signal.
//      Fixed PQMF bank: the four band samples are immediately rotated into the
//      8 cosine-modulation phases U_q = sum_k cos(theta_k(q)) y_k  (the bank is
//      h_k[j] = 2 p[j] cos(theta_k(j)) with theta_k(j+8) = theta_k(j) + (2k+1)pi,
//      so cos(theta_k(j)) = (-1)^(j/8) cos(theta_k(j mod 8))) -> LDS Us[q][.]
//      Trainable bank (MS): the band samples go to LDS ys[band][.] as they are.
//   C  one lane per sub-band sample m: the 4 polyphase outputs o[4m..4m+3];
//      fixed bank: 16 prototype taps each (63 FMA per lane instead of 252),
//      trainable bank: <= 16 taps x 4 bands each.  The zero-stuffed x4
//      upsampling never materialises; one 16-byte store per lane.
// Frames / samples in the halos are recomputed, not exchanged; consecutive
// tiles are mapped to the same XCD so halo rows hit in its L2.
#include "kernels.h"

namespace mbv {

namespace {

constexpr float kPi = 3.14159265358979323846f;

// cos(2*pi*j/16), sin(2*pi*j/16)
__device__ constexpr float COS16[16] = {
    1.0f, 0.92387953251128674f, 0.70710678118654752f, 0.38268343236508977f,
    0.0f, -0.38268343236508977f, -0.70710678118654752f, -0.92387953251128674f,
    -1.0f, -0.92387953251128674f, -0.70710678118654752f, -0.38268343236508977f,
    0.0f, 0.38268343236508977f, 0.70710678118654752f, 0.92387953251128674f};
__device__ constexpr float SIN16[16] = {
    0.0f, 0.38268343236508977f, 0.70710678118654752f, 0.92387953251128674f,
    1.0f, 0.92387953251128674f, 0.70710678118654752f, 0.38268343236508977f,
    0.0f, -0.38268343236508977f, -0.70710678118654752f, -0.92387953251128674f,
    -1.0f, -0.92387953251128674f, -0.70710678118654752f, -0.38268343236508977f};
// periodic hann(16): 0.5 - 0.5 cos(2 pi n / 16)
__device__ constexpr float HANN16[16] = {
    0.0f, 0.03806023374435663f, 0.14644660940672624f, 0.30865828381745514f,
    0.5f, 0.69134171618254486f, 0.85355339059327376f, 0.96193976625564337f,
    1.0f, 0.96193976625564337f, 0.85355339059327376f, 0.69134171618254486f,
    0.5f, 0.30865828381745514f, 0.14644660940672624f, 0.03806023374435663f};
// squared window, for per-lane (runtime-indexed) envelope sums at the signal edges
__device__ const float WSQ16[16] = {
    0.0f, 0.0014485813926750633f, 0.021446609406726238f, 0.095269936169136614f,
    0.25f, 0.47795336853422657f, 0.72855339059327373f, 0.92532811390396186f,
    1.0f, 0.92532811390396186f, 0.72855339059327373f, 0.47795336853422657f,
    0.25f, 0.095269936169136614f, 0.021446609406726238f, 0.0014485813926750633f};

// Fixed PQMF bank (pqmf.py:15-75: taps 62, cutoff 0.15, Kaiser beta 9), factorised:
//   4 h_k[j] = PQMF_G[j] * PQMF_C[k][j mod 8],  PQMF_C[k][q] = cos((2k+1)(pi/8)(q - 30.5) - (-1)^k pi/4),
//   PQMF_G[j] = 8 p[j] (-1)^(j/8).  Generated in float64 by scripts/gen_pqmf_tables.py, rounded to fp32.
__device__ constexpr float PQMF_C[32] = {
    9.807852507e-01f, 9.807852507e-01f, 8.314695954e-01f, 5.555702448e-01f,
    1.950903237e-01f, -1.950903237e-01f, -5.555702448e-01f, -8.314695954e-01f,
    -8.314695954e-01f, -8.314695954e-01f, 1.950903237e-01f, 9.807852507e-01f,
    5.555702448e-01f, -5.555702448e-01f, -9.807852507e-01f, -1.950903237e-01f,
    -5.555702448e-01f, -5.555702448e-01f, 9.807852507e-01f, -1.950903237e-01f,
    -8.314695954e-01f, 8.314695954e-01f, 1.950903237e-01f, -9.807852507e-01f,
    1.950903237e-01f, 1.950903237e-01f, -5.555702448e-01f, 8.314695954e-01f,
    -9.807852507e-01f, 9.807852507e-01f, -8.314695954e-01f, 5.555702448e-01f,
};
__device__ constexpr float PQMF_G[64] = {
    6.692762690e-05f, 2.144142782e-04f, 4.045689129e-04f, 4.907859839e-04f,
    2.202252799e-04f, -6.902719615e-04f, -2.394147683e-03f, -4.707115702e-03f,
    6.936517078e-03f, 7.863246836e-03f, 5.977601744e-03f, -6.432701142e-18f,
    -1.040009875e-02f, -2.390390635e-02f, -3.716831654e-02f, -4.507908970e-02f,
    4.180690646e-02f, 2.259947546e-02f, -1.405207906e-02f, -6.448587775e-02f,
    -1.188977659e-01f, -1.619237214e-01f, -1.750242710e-01f, -1.404098570e-01f,
    4.571796954e-02f, -1.117221490e-01f, -3.222790956e-01f, -5.640172958e-01f,
    -8.056510091e-01f, -1.012026548e+00f, -1.150984049e+00f, -1.200000048e+00f,
    1.150984049e+00f, 1.012026548e+00f, 8.056510091e-01f, 5.640172958e-01f,
    3.222790956e-01f, 1.117221490e-01f, -4.571796954e-02f, -1.404098570e-01f,
    1.750242710e-01f, 1.619237214e-01f, 1.188977659e-01f, 6.448587775e-02f,
    1.405207906e-02f, -2.259947546e-02f, -4.180690646e-02f, -4.507908970e-02f,
    3.716831654e-02f, 2.390390635e-02f, 1.040009875e-02f, 6.432701142e-18f,
    -5.977601744e-03f, -7.863246836e-03f, -6.936517078e-03f, -4.707115702e-03f,
    2.394147683e-03f, 6.902719615e-04f, -2.202252799e-04f, -4.907859839e-04f,
    -4.045689129e-04f, -2.144142782e-04f, -6.692762690e-05f, 0.000000000e+00f,
};

// PRE: the producing conv already scaled the log-magnitude rows by log2(e) and the phase rows by
// 1/(2 pi) (folded into subband_conv_post's packed weights), so exp2 / sin-in-turns apply directly.
template <bool FAST, bool PRE>
__device__ __forceinline__ void polar(float xm, float xp, float& mag, float& ph, float& re,
                                      float& im, bool need_im) {
  if constexpr (FAST) {
    // hardware transcendentals: v_exp_f32 (2^x), v_sin_f32 / v_cos_f32 (argument in turns, valid
    // for |turns| <= 256, i.e. |x| <= 1608 rad).  pi*sin(x) in turns is 0.5*sin(x): no multiply
    // by pi on the path to cos/sin.
    mag = __builtin_amdgcn_exp2f(PRE ? xm : xm * 1.44269504088896341f);
    const float s = __builtin_amdgcn_sinf(PRE ? xp : xp * 0.15915494309189535f);
    ph = kPi * s;
    re = mag * __builtin_amdgcn_cosf(0.5f * s);
    im = need_im ? mag * __builtin_amdgcn_sinf(0.5f * s) : 0.f;
  } else {
    if constexpr (PRE) { xm *= 0.69314718055994531f; xp *= 6.28318530717958648f; }
    mag = expf(xm);
    ph = kPi * sinf(xp);
    float sn, cs;
    sincosf(ph, &sn, &cs);
    re = mag * cs;
    im = mag * sn;
  }
}

// (magnitude, phase [rad]) given directly: the `istft_finalize` entry of the chunked-decode flow
template <bool FAST>
__device__ __forceinline__ void polar_in(float mag, float ph, float& re, float& im, bool need_im) {
  if constexpr (FAST) {
    const float t = ph * 0.15915494309189535f;          // radians -> turns
    re = mag * __builtin_amdgcn_cosf(t);
    im = need_im ? mag * __builtin_amdgcn_sinf(t) : 0.f;
  } else {
    float sn, cs;
    sincosf(ph, &sn, &cs);
    re = mag * cs;
    im = mag * sn;
  }
}

// 16-point real inverse DFT of a one-sided spectrum (Im of DC / Nyquist ignored, as c2r
// does), times hann(16)/16.  Packed real-IFFT: with A_k = X_k + conj(X_{8-k}),
// D_k = X_k - conj(X_{8-k}), Z_k = A_k + j W^k D_k (W = e^{j 2 pi/16}, k < 8) one has
// x[2n] + j x[2n+1] = (1/16) sum_k Z_k e^{j 2 pi k n / 8}; Z_{8-k} = conj(A_k - j W^k D_k).
// The 8-point complex inverse transform is two radix-4 butterflies + one radix-2 stage:
// ~110 flops instead of the 16 x 16 matrix form.
struct cpx { float r, i; };
__device__ __forceinline__ cpx cadd(cpx a, cpx b) { return {a.r + b.r, a.i + b.i}; }
__device__ __forceinline__ cpx csub(cpx a, cpx b) { return {a.r - b.r, a.i - b.i}; }
__device__ __forceinline__ void idft4(cpx y0, cpx y1, cpx y2, cpx y3, cpx o[4]) {
  const cpx t0 = cadd(y0, y2), t1 = csub(y0, y2), t2 = cadd(y1, y3), t3 = csub(y1, y3);
  o[0] = cadd(t0, t2);
  o[2] = csub(t0, t2);
  o[1] = {t1.r - t3.i, t1.i + t3.r};      // t1 + j t3
  o[3] = {t1.r + t3.i, t1.i - t3.r};      // t1 - j t3
}
__device__ __forceinline__ void irfft16_hann(const float* re, const float* im, float* out) {
  cpx Z[8];
  Z[0] = {re[0] + re[8], re[0] - re[8]};
  Z[4] = {2.f * re[4], -2.f * im[4]};
#pragma unroll
  for (int k = 1; k < 4; ++k) {
    const float Ar = re[k] + re[8 - k], Ai = im[k] - im[8 - k];
    const float Dr = re[k] - re[8 - k], Di = im[k] + im[8 - k];
    const float Br = -SIN16[k] * Dr - COS16[k] * Di;
    const float Bi = COS16[k] * Dr - SIN16[k] * Di;
    Z[k] = {Ar + Br, Ai + Bi};
    Z[8 - k] = {Ar - Br, Bi - Ai};
  }
  cpx E[4], O[4];
  idft4(Z[0], Z[2], Z[4], Z[6], E);
  idft4(Z[1], Z[3], Z[5], Z[7], O);
  constexpr float r = 0.70710678118654752f;
  const cpx T0 = O[0];
  const cpx T1 = {(O[1].r - O[1].i) * r, (O[1].r + O[1].i) * r};
  const cpx T2 = {-O[2].i, O[2].r};
  const cpx T3 = {(-O[3].r - O[3].i) * r, (O[3].r - O[3].i) * r};
  const cpx T[4] = {T0, T1, T2, T3};
#pragma unroll
  for (int n = 0; n < 4; ++n) {
    const cpx a = cadd(E[n], T[n]), b = csub(E[n], T[n]);
    out[2 * n] = a.r * (HANN16[2 * n] * (1.f / 16.f));
    out[2 * n + 1] = a.i * (HANN16[2 * n + 1] * (1.f / 16.f));
    out[2 * n + 8] = b.r * (HANN16[2 * n + 8] * (1.f / 16.f));
    out[2 * n + 9] = b.i * (HANN16[2 * n + 9] * (1.f / 16.f));
  }
}

}  // namespace

// `taps` (device, 256 floats, only read by the trainable-bank variant):
//   t[band][p][i] = 4 h[band][3 - p + 4 i]   (x4 up-sampling gain folded in; 0 where the tap is > 62)
// RANGED (launch_istft_pqmf_range): the grid holds only the tiles that cover sub-band samples [rg.keep_lo,
// rg.keep_hi) of every row, phase C stores only those (at a.o + b rg.o_row_stride + 4 (m - keep_lo)), and nothing
// else is written.  (rg is the last argument, so that the one-shot instantiations keep their code.)
// RANGED with rg.row_lens (the row-exact ragged decode, mbv_decode_ragged): row b is an utterance of row_lens[b]
// z-frames inside a launch laid out for a.Tp — its frame count, envelope edges and the synthesis filter's zero
// padding are those of its stand-alone launch (F_b = 16 len_b + 1, M_b = 64 len_b), only the strides are a.Tp's;
// tiles at and past M_b do nothing, and row b is stored at row rg.row_map[b] of o.
// (the kernel's text is in istft_tail.inc, together with istft_single_kernel's: both exist a second time with
// per-row ranges and destinations, the pooled streaming decode's tails)
#define MBV_ISTFT_POOL 0
#include "istft_tail.inc"
#undef MBV_ISTFT_POOL
#define MBV_ISTFT_POOL 1
#include "istft_tail.inc"
#undef MBV_ISTFT_POOL

// 480 sub-band samples x 512 threads (4 workgroups / CU).  Measured and rejected (r02): (a) non-temporal stores for
// spec / phase / o_mb — 91 vs 84 us for the all-outputs launch; (b) a persistent grid with the next tile's 18
// inputs prefetched into registers: needs 80 registers per lane = 3 instead of 4 workgroups per CU,
// and loses more to the lower occupancy than the prefetch gains (35.9 / 39.3 vs 32.2 us);
// (c) 16-byte accesses through in-register 4 x 4 transposes across lane quads (DPP): x_post loads
// 36.6 vs 31.6 us, spec / phase stores 84.8 vs 80.0 us in the same run (an apparent 84 -> 75 us gain
// was box-to-box variation).  All three are in the history of this file (r02).  What the launch is
// bound by: bytes in flight per CU at full occupancy (4 x 512 threads, 18 loads per lane) against
// the latency of the level that serves them — 0.81 of the HBM peak from the Infinity Cache, 0.63
// from HBM itself (bench.py roofline.past_cache), 0.61-0.65 with all outputs written.
void launch_istft_pqmf(const IstftArgs& a, hipStream_t s) {
  constexpr int TM = 480, NT = 512;
  const int M = 64 * a.Tp;
  const int tiles_per_utt = (M + TM - 1) / TM;
  const int total = tiles_per_utt * a.B;
  const dim3 grid(total), block(NT);
#define MBV_ISTFT_LAUNCH(FIXED, FAST, PRE, POLAR) \
  hipLaunchKernelGGL((istft_pqmf_kernel<TM, NT, FIXED, FAST, PRE, POLAR>), grid, block, 0, s, a, a.filt, tiles_per_utt, total, IstftRange{})
  if (a.polar_in) {          // (spec, phase) input: a.spec / a.phase are read, not written
    const int v = (a.fixed_bank ? 2 : 0) | (a.exact_math ? 0 : 1);
    switch (v) {
      case 0: MBV_ISTFT_LAUNCH(false, false, false, true); break;
      case 1: MBV_ISTFT_LAUNCH(false, true, false, true); break;
      case 2: MBV_ISTFT_LAUNCH(true, false, false, true); break;
      default: MBV_ISTFT_LAUNCH(true, true, false, true); break;
    }
    return;
  }
  const int variant = (a.fixed_bank ? 4 : 0) | (a.exact_math ? 0 : 2) | (a.prescaled ? 1 : 0);
  switch (variant) {
    case 0: MBV_ISTFT_LAUNCH(false, false, false, false); break;
    case 1: MBV_ISTFT_LAUNCH(false, false, true, false); break;
    case 2: MBV_ISTFT_LAUNCH(false, true, false, false); break;
    case 3: MBV_ISTFT_LAUNCH(false, true, true, false); break;
    case 4: MBV_ISTFT_LAUNCH(true, false, false, false); break;
    case 5: MBV_ISTFT_LAUNCH(true, false, true, false); break;
    case 6: MBV_ISTFT_LAUNCH(true, true, false, false); break;
    default: MBV_ISTFT_LAUNCH(true, true, true, false); break;
  }
#undef MBV_ISTFT_LAUNCH
}

// The streaming decode's tail (mbv_decode_range): x_post of a z-window, only the chunk's samples stored.  Every
// kept sample is computed by the same operations as in the one-shot launch (a tile's position changes no sample's
// arithmetic), so it is bitwise the one-shot sample whenever x_post is.
void launch_istft_pqmf_range(const IstftArgs& a, const IstftRange& r, hipStream_t s) {
  constexpr int TM = 480, NT = 512;
  const int tiles_per_utt = (r.keep_hi + TM - 1) / TM - r.keep_lo / TM;
  const int total = tiles_per_utt * a.B;
  const dim3 grid(total), block(NT);
  const int v = (a.fixed_bank ? 2 : 0) | (a.exact_math ? 0 : 1);      // (x_post is always prescaled here)
  switch (v) {
    case 0: hipLaunchKernelGGL((istft_pqmf_kernel<TM, NT, false, false, true, false, true>), grid, block, 0, s, a, a.filt, tiles_per_utt, total, r); break;
    case 1: hipLaunchKernelGGL((istft_pqmf_kernel<TM, NT, false, true, true, false, true>), grid, block, 0, s, a, a.filt, tiles_per_utt, total, r); break;
    case 2: hipLaunchKernelGGL((istft_pqmf_kernel<TM, NT, true, false, true, false, true>), grid, block, 0, s, a, a.filt, tiles_per_utt, total, r); break;
    default: hipLaunchKernelGGL((istft_pqmf_kernel<TM, NT, true, true, true, false, true>), grid, block, 0, s, a, a.filt, tiles_per_utt, total, r); break;
  }
}

// The pooled streaming decode's tail (mbv_decode_chunks): the same operations per kept sample once more, with the
// range and the destination of every row read from its table entry.  A range of n units touches at most
// (n - 1) / TM + 2 tiles, wherever it starts.
void launch_istft_pqmf_pool(const IstftArgs& a, const PoolRow* rows, int max_keep, hipStream_t s) {
  constexpr int TM = 480, NT = 512;
  const int tiles_per_utt = (max_keep - 1) / TM + 2;
  const int total = tiles_per_utt * a.B;
  const dim3 grid(total), block(NT);
  const int v = (a.fixed_bank ? 2 : 0) | (a.exact_math ? 0 : 1);
  switch (v) {
    case 0: hipLaunchKernelGGL((istft_pqmf_pool_kernel<TM, NT, false, false>), grid, block, 0, s, a, a.filt, tiles_per_utt, total, rows); break;
    case 1: hipLaunchKernelGGL((istft_pqmf_pool_kernel<TM, NT, false, true>), grid, block, 0, s, a, a.filt, tiles_per_utt, total, rows); break;
    case 2: hipLaunchKernelGGL((istft_pqmf_pool_kernel<TM, NT, true, false>), grid, block, 0, s, a, a.filt, tiles_per_utt, total, rows); break;
    default: hipLaunchKernelGGL((istft_pqmf_pool_kernel<TM, NT, true, true>), grid, block, 0, s, a, a.filt, tiles_per_utt, total, rows); break;
  }
}

// ============================================================================
// Single-band tail of iSTFT_Generator (models.py:296-300): exp / pi*sin, TorchSTFT.inverse
// (n_fft 16, hop 4), no filter bank.  Phase A: one lane per frame (255 frames per workgroup);
// phase B: one lane per quad of output samples (252 quads): overlap-add of the 4 covering
// frames, edge-aware envelope, one 16-byte store.
// ============================================================================
// RANGED (launch_istft_single_range): only the tiles that cover quads [rg.keep_lo, rg.keep_hi), only those stored,
// at a.o + b rg.o_row_stride + 4 (q - keep_lo)
void launch_istft_single(const IstftSbArgs& a, hipStream_t s) {
  const int tiles = (a.F - 1 + 251) / 252;
  const dim3 grid(tiles * a.B), block(256);
  if (a.polar_in) {
    if (a.exact_math) hipLaunchKernelGGL((istft_single_kernel<false, false, true>), grid, block, 0, s, a, tiles, IstftRange{});
    else hipLaunchKernelGGL((istft_single_kernel<true, false, true>), grid, block, 0, s, a, tiles, IstftRange{});
    return;
  }
  const int variant = (a.exact_math ? 0 : 2) | (a.prescaled ? 1 : 0);
  switch (variant) {
    case 0: hipLaunchKernelGGL((istft_single_kernel<false, false, false>), grid, block, 0, s, a, tiles, IstftRange{}); break;
    case 1: hipLaunchKernelGGL((istft_single_kernel<false, true, false>), grid, block, 0, s, a, tiles, IstftRange{}); break;
    case 2: hipLaunchKernelGGL((istft_single_kernel<true, false, false>), grid, block, 0, s, a, tiles, IstftRange{}); break;
    default: hipLaunchKernelGGL((istft_single_kernel<true, true, false>), grid, block, 0, s, a, tiles, IstftRange{}); break;
  }
}

void launch_istft_single_range(const IstftSbArgs& a, const IstftRange& r, hipStream_t s) {
  const int tiles = (r.keep_hi + 251) / 252 - r.keep_lo / 252;
  const dim3 grid(tiles * a.B), block(256);
  if (a.exact_math) hipLaunchKernelGGL((istft_single_kernel<false, true, false, true>), grid, block, 0, s, a, tiles, r);
  else hipLaunchKernelGGL((istft_single_kernel<true, true, false, true>), grid, block, 0, s, a, tiles, r);
}

void launch_istft_single_pool(const IstftSbArgs& a, const PoolRow* rows, int max_keep, hipStream_t s) {
  const int tiles = (max_keep - 1) / 252 + 2;
  const dim3 grid(tiles * a.B), block(256);
  if (a.exact_math) hipLaunchKernelGGL((istft_single_pool_kernel<false>), grid, block, 0, s, a, tiles, rows);
  else hipLaunchKernelGGL((istft_single_pool_kernel<true>), grid, block, 0, s, a, tiles, rows);
}

}  // namespace mbv
