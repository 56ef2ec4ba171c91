// Linear spectrogram of waveform rows: |STFT| with the semantics of spectrogram_torch(y, n_fft, sr, hop, win,
// center=False) (mel_processing.py:51-70): (n_fft - hop) / 2 zeros on each side, periodic Hann window of
// length win centred in n_fft as torch.stft centres it, onesided, abs() with no epsilon.  Every row is
// transformed as if alone (zeros at and past its valid length) and padded with zero frames as the
// collate function pads a ragged batch (data_utils.py:125-147).
//
// The real FFT of n_fft points is a complex FFT of N = n_fft / 2 points (z[m] = x[2m] + i x[2m+1]) followed
// by the split post-pass X[k] = E[k] + W^k O[k], k = 0 .. N.  The complex FFT is a Stockham auto-sort FFT
// of radix-8 passes (one or two radix-4 passes when log2 N is not a multiple of 3): a team of N / 8 lanes
// owns one frame, every lane holds 8 points in registers per pass, and the passes exchange through LDS.
// Twiddles and the window come from fp32 tables built in float64 on the host (capi.hip caches them).
#include "kernels.h"

#include <cmath>

namespace mbv {

namespace {

constexpr int kThreads = 256;

__device__ __forceinline__ float2 cmul(float2 a, float2 b) {
  return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}
__device__ __forceinline__ float2 cadd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 csub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ float2 mul_mi(float2 a) { return make_float2(a.y, -a.x); }   // a * (-i)

// forward DFT of R points in place (e^{-2 pi i jk / R})
template <int R> __device__ __forceinline__ void dft(float2* a);
template <> __device__ __forceinline__ void dft<4>(float2* a) {
  const float2 s0 = cadd(a[0], a[2]), d0 = csub(a[0], a[2]);
  const float2 s1 = cadd(a[1], a[3]), d1 = mul_mi(csub(a[1], a[3]));
  a[0] = cadd(s0, s1);
  a[2] = csub(s0, s1);
  a[1] = cadd(d0, d1);
  a[3] = csub(d0, d1);
}
template <> __device__ __forceinline__ void dft<8>(float2* a) {
  const float r = 0.70710678118654752f;   // 1 / sqrt(2)
  float2 e[4] = {a[0], a[2], a[4], a[6]}, o[4] = {a[1], a[3], a[5], a[7]};
  dft<4>(e);
  dft<4>(o);
  // o[k] *= e^{-2 pi i k / 8}
  o[1] = make_float2(r * (o[1].x + o[1].y), r * (o[1].y - o[1].x));
  o[2] = mul_mi(o[2]);
  o[3] = make_float2(r * (o[3].y - o[3].x), -r * (o[3].x + o[3].y));
  for (int k = 0; k < 4; ++k) {
    a[k] = cadd(e[k], o[k]);
    a[k + 4] = csub(e[k], o[k]);
  }
}

// One Stockham pass of radix R over the team's N points (Ns = product of the radices before it).  Each lane
// does 8 / R butterflies: reads a[r] = buf[j + r N / R], twiddles by W_{Ns R}^{r (j mod Ns)}, transforms and
// writes to ((j / Ns) Ns R + j mod Ns) + r Ns.  tw[m] = e^{-2 pi i m / (2N)}, so W_{Ns R}^q = tw[2 q N / (Ns R)].
// FIRST: the pass reads the windowed frame from the staged input instead of buf.
template <int LOGN, int R, bool FIRST>
__device__ __forceinline__ void stockham_pass(float2* buf, int Ns, int t, const float2* __restrict__ tw,
                                              const float* __restrict__ xs, const float* __restrict__ win) {
  constexpr int N = 1 << LOGN, T = N / 8, Q = 8 / R;
  float2 a[Q][R];
  for (int q = 0; q < Q; ++q) {
    const int j = t + q * T;
    const int k = j & (Ns - 1);
    for (int r = 0; r < R; ++r) {
      const int m = j + r * (N / R);
      if (FIRST) {
        a[q][r] = make_float2(win[2 * m] * xs[2 * m], win[2 * m + 1] * xs[2 * m + 1]);
      } else {
        a[q][r] = buf[m];
        if (r) a[q][r] = cmul(a[q][r], tw[2 * ((r * k) * (N / (Ns * R)))]);
      }
    }
    dft<R>(a[q]);
  }
  __syncthreads();                         // every lane has read before any lane overwrites
  for (int q = 0; q < Q; ++q) {
    const int j = t + q * T;
    const int k = j & (Ns - 1);
    const int o = (j - k) * R + k;
    for (int r = 0; r < R; ++r) buf[o + r * Ns] = a[q][r];
  }
  __syncthreads();
}

// ---------------------------------------------------------------------------------------------------
// One workgroup = FB consecutive frames [f0, f0 + FB) of row b.  The input span of those frames
// ((FB - 1) hop + n_fft samples, padding included) is staged in LDS once, zero outside [0, valid).
// G = 256 / (N / 8) frames are transformed at a time, one per team; the magnitudes go to an LDS tile
// [N + 1][FB + 1] that is then stored bin by bin as runs of FB consecutive frames.
// ROWS (pooled voice conversion, kernels.h): row b's samples, their count and their dtype come from rows[b] (x, valid,
// in_stride and scale are not used: the table travels in global memory, the LDS layout is the scalar kernel's), and
// the destination row has KC = cpad >= N + 1 channels, those from N + 1 on written as zeros.  rows[b].first > 0: the row
// is the frame window [first, first + frames) of its recording (live conversion); frame f reads from (first + f) hop - pad.
// ---------------------------------------------------------------------------------------------------
template <int LOGN, typename In, bool ROWS>
__global__ void __launch_bounds__(kThreads)
spectrogram_kernel(const In* __restrict__ x, const int64_t* __restrict__ valid, int64_t in_stride, float scale,
                   int hop, int pad, const float2* __restrict__ tw, const float* __restrict__ win, int FB,
                   float* __restrict__ spec, int64_t F, int64_t* __restrict__ spec_lengths,
                   const ConvertRow* __restrict__ rows, int cpad) {
  constexpr int N = 1 << LOGN, NFFT = 2 * N, T = N / 8, G = kThreads / T;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float2* work = reinterpret_cast<float2*>(smem);                 // [G][N]
  float* tile = smem + 2 * G * N;                                 // [N + 1][FB + 1]
  const int FBp = FB + 1;
  float* xs = tile + (N + 1) * FBp;                               // [(FB - 1) hop + n_fft]

  const int b = blockIdx.y;
  const int KC = ROWS ? cpad : N + 1;                             // channels of a destination row
  int64_t v = in_stride;
  const void* xr = nullptr;
  bool pcm = false;
  int64_t first = 0;                                              // ROWS: the row is a frame window starting here
  int rframes = 0;
  if (ROWS) {
    const ConvertRow r = rows[b];
    v = r.samples < 0 ? 0 : r.samples;
    xr = r.wave;
    pcm = r.dtype == 1;
    scale = pcm ? 1.f / 32768.f : 1.f;
    first = r.first;
    rframes = r.frames;
  } else if (valid) {
    v = valid[b];
    v = v < 0 ? 0 : (v > in_stride ? in_stride : v);
  }
  const int64_t padded = v + 2 * (int64_t)pad;
  int64_t nfr = padded < NFFT ? 0 : 1 + (padded - NFFT) / hop;
  if (ROWS) {                       // the window's own frames (a whole recording: first = 0 and frames = nfr already)
    nfr -= first;
    if (nfr > rframes) nfr = rframes;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0 && spec_lengths) spec_lengths[b] = nfr;
  const int64_t f0 = (int64_t)blockIdx.x * FB;
  if (f0 >= F) return;
  const int nf = (int)(F - f0 < FB ? F - f0 : FB);               // frames of this block inside the output
  float* out = spec + (int64_t)b * KC * F + f0;
  const int lg_fb = __ffs(FB) - 1;                                // FB is a power of two

  if (f0 >= nfr) {                                                // past the row's length: zeros only
    for (int e = threadIdx.x; e < KC * FB; e += kThreads) {
      const int k = e >> lg_fb, fl = e & (FB - 1);
      if (fl < nf) out[(int64_t)k * F + fl] = 0.f;
    }
    return;
  }

  // stage padded samples [f0 hop, f0 hop + S) = x[f0 hop - pad + i]
  const int S = (FB - 1) * hop + NFFT;
  const int64_t j0 = (first + f0) * hop - pad;
  const In* xb = x + (int64_t)b * in_stride;
  for (int i0 = 0; i0 < S; i0 += 8 * kThreads) {     // 8 loads in flight per lane before their LDS writes
    float r[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int i = i0 + u * kThreads + threadIdx.x;
      const int64_t j = j0 + i;
      if (ROWS)
        r[u] = (i < S && j >= 0 && j < v) ? (pcm ? (float)((const short*)xr)[j] : ((const float*)xr)[j]) * scale : 0.f;
      else
        r[u] = (i < S && j >= 0 && j < v) ? (float)xb[j] * scale : 0.f;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int i = i0 + u * kThreads + threadIdx.x;
      if (i < S) xs[i] = r[u];
    }
  }
  __syncthreads();

  const int team = threadIdx.x / T, t = threadIdx.x - team * T;
  float2* buf = work + team * N;
  for (int g = 0; g < FB; g += G) {
    const int fl = g + team;
    const float* xf = xs + fl * hop;
    // passes: radix 8 throughout, two radix-4 for LOGN = 1 (mod 3), one radix-4 for LOGN = 2 (mod 3)
    constexpr int P8 = LOGN % 3 == 1 ? LOGN / 3 - 1 : LOGN / 3;
    constexpr int P4 = LOGN % 3 == 1 ? 2 : LOGN % 3 == 2 ? 1 : 0;
    int Ns = 1;
    stockham_pass<LOGN, 8, true>(buf, Ns, t, tw, xf, win);
    Ns *= 8;
#pragma unroll
    for (int p = 1; p < P8; ++p) { stockham_pass<LOGN, 8, false>(buf, Ns, t, tw, xf, win); Ns *= 8; }
#pragma unroll
    for (int p = 0; p < P4; ++p) { stockham_pass<LOGN, 4, false>(buf, Ns, t, tw, xf, win); Ns *= 4; }
    // split post-pass: X[k] = E[k] + W_{2N}^k O[k],  E = (Z[k] + conj Z[N-k]) / 2,  O = (Z[k] - conj Z[N-k]) / 2i
    const bool live = f0 + fl < nfr;
    for (int k = t; k <= N; k += T) {
      const float2 zk = buf[k & (N - 1)];
      const float2 zn = buf[(N - k) & (N - 1)];
      const float er = 0.5f * (zk.x + zn.x), ei = 0.5f * (zk.y - zn.y);
      const float orr = 0.5f * (zk.y + zn.y), oi = -0.5f * (zk.x - zn.x);
      const float2 w = tw[k];
      const float re = er + (w.x * orr - w.y * oi);
      const float im = ei + (w.x * oi + w.y * orr);
      tile[k * FBp + fl] = live ? sqrtf(re * re + im * im) : 0.f;
    }
    __syncthreads();                     // buf is rewritten by the next group's first pass
  }

  for (int e = threadIdx.x; e < KC * FB; e += kThreads) {
    const int k = e >> lg_fb, fl = e & (FB - 1);
    if (fl < nf) out[(int64_t)k * F + fl] = (!ROWS || k <= N) ? tile[k * FBp + fl] : 0.f;
  }
}

template <int LOGN>
void launch_logn(const void* x, int dtype, const int64_t* valid, int B, int64_t in_stride, int hop, int pad,
                 const float2* tw, const float* win, int FB, float* spec, int64_t F, int64_t* spec_lengths,
                 hipStream_t s) {
  const int64_t nbx = F > 0 ? (F + FB - 1) / FB : 1;
  const size_t lds = spectrogram_lds_bytes(1 << (LOGN + 1), hop, FB);
  const dim3 grid((unsigned)nbx, (unsigned)B), block(kThreads);
  static const bool attr = [] {                   // dynamic LDS past 64 KiB must be allowed per kernel
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&spectrogram_kernel<LOGN, short, false>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)kSpectrogramMaxLds);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&spectrogram_kernel<LOGN, float, false>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)kSpectrogramMaxLds);
    return true;
  }();
  (void)attr;
  if (dtype == 1)
    hipLaunchKernelGGL((spectrogram_kernel<LOGN, short, false>), grid, block, lds, s, (const short*)x, valid, in_stride,
                       1.f / 32768.f, hop, pad, tw, win, FB, spec, F, spec_lengths, nullptr, 0);
  else
    hipLaunchKernelGGL((spectrogram_kernel<LOGN, float, false>), grid, block, lds, s, (const float*)x, valid, in_stride,
                       1.f, hop, pad, tw, win, FB, spec, F, spec_lengths, nullptr, 0);
}

template <int LOGN>
void launch_rows_logn(const ConvertRow* rows, int B, int hop, int pad, const float2* tw, const float* win, int FB,
                      float* dst, int cpad, int64_t F, hipStream_t s) {
  const int64_t nbx = F > 0 ? (F + FB - 1) / FB : 1;
  const size_t lds = spectrogram_lds_bytes(1 << (LOGN + 1), hop, FB);
  const dim3 grid((unsigned)nbx, (unsigned)B), block(kThreads);
  static const bool attr = [] {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&spectrogram_kernel<LOGN, float, true>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)kSpectrogramMaxLds);
    return true;
  }();
  (void)attr;
  hipLaunchKernelGGL((spectrogram_kernel<LOGN, float, true>), grid, block, lds, s, (const float*)nullptr, nullptr,
                     (int64_t)0, 1.f, hop, pad, tw, win, FB, dst, F, nullptr, rows, cpad);
}

}  // namespace

int64_t spectrogram_frames(int64_t n, int n_fft, int hop) {
  const int64_t padded = n + 2 * (int64_t)((n_fft - hop) / 2);
  return padded < n_fft ? 0 : 1 + (padded - n_fft) / hop;
}

size_t spectrogram_lds_bytes(int n_fft, int hop, int FB) {
  const int N = n_fft / 2, G = kThreads / (N / 8);
  return sizeof(float) * ((size_t)2 * G * N + (size_t)(N + 1) * (FB + 1) + (size_t)(FB - 1) * hop + n_fft);
}

int spectrogram_block_frames(int n_fft, int hop) {
  const int G = kThreads / (n_fft / 16);
  int FB = n_fft <= 1024 ? 32 : 32768 / n_fft;                      // 128-B runs per bin where the tile fits
  while (FB > G && spectrogram_lds_bytes(n_fft, hop, FB) > kSpectrogramMaxLds) FB /= 2;
  return FB;
}

void spectrogram_tables(int n_fft, int win, std::vector<float>* tw, std::vector<float>* window) {
  // tw: e^{-2 pi i m / n_fft}, m < n_fft, as (re, im) pairs; window: periodic Hann of length win, centred
  tw->assign(2 * (size_t)n_fft, 0.f);
  for (int m = 0; m < n_fft; ++m) {
    const double a = 2.0 * M_PI * (double)m / (double)n_fft;
    (*tw)[2 * m] = (float)std::cos(a);
    (*tw)[2 * m + 1] = (float)-std::sin(a);
  }
  window->assign(n_fft, 0.f);
  const int left = (n_fft - win) / 2;
  for (int j = 0; j < win; ++j) (*window)[left + j] = (float)(0.5 - 0.5 * std::cos(2.0 * M_PI * (double)j / (double)win));
}

void launch_spectrogram(const void* x, int dtype, const int64_t* valid, int B, int64_t in_stride, int n_fft, int hop,
                        const float* tw, const float* win, float* spec, int64_t F, int64_t* spec_lengths,
                        hipStream_t s) {
  const int pad = (n_fft - hop) / 2;
  const int FB = spectrogram_block_frames(n_fft, hop);
  const float2* t2 = reinterpret_cast<const float2*>(tw);
  switch (n_fft) {
    case 256: launch_logn<7>(x, dtype, valid, B, in_stride, hop, pad, t2, win, FB, spec, F, spec_lengths, s); break;
    case 512: launch_logn<8>(x, dtype, valid, B, in_stride, hop, pad, t2, win, FB, spec, F, spec_lengths, s); break;
    case 1024: launch_logn<9>(x, dtype, valid, B, in_stride, hop, pad, t2, win, FB, spec, F, spec_lengths, s); break;
    case 2048: launch_logn<10>(x, dtype, valid, B, in_stride, hop, pad, t2, win, FB, spec, F, spec_lengths, s); break;
    default: launch_logn<11>(x, dtype, valid, B, in_stride, hop, pad, t2, win, FB, spec, F, spec_lengths, s); break;
  }
}

void launch_spectrogram_rows(const ConvertRow* rows, int B, int n_fft, int hop, const float* tw, const float* win,
                             float* dst, int cpad, int64_t F, hipStream_t s) {
  const int pad = (n_fft - hop) / 2;
  const int FB = spectrogram_block_frames(n_fft, hop);
  const float2* t2 = reinterpret_cast<const float2*>(tw);
  switch (n_fft) {
    case 256: launch_rows_logn<7>(rows, B, hop, pad, t2, win, FB, dst, cpad, F, s); break;
    case 512: launch_rows_logn<8>(rows, B, hop, pad, t2, win, FB, dst, cpad, F, s); break;
    case 1024: launch_rows_logn<9>(rows, B, hop, pad, t2, win, FB, dst, cpad, F, s); break;
    case 2048: launch_rows_logn<10>(rows, B, hop, pad, t2, win, FB, dst, cpad, F, s); break;
    default: launch_rows_logn<11>(rows, B, hop, pad, t2, win, FB, dst, cpad, F, s); break;
  }
}

}  // namespace mbv
