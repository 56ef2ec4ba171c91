// ITU-R BS.1770 integrated loudness on the device: K-weighting, 100 ms segment energies, 400 ms
// blocks, two gates.  The filter recurrence is serial in the sample index, so the kernel is parallel over segments:
// every segment's zero-state end state r_k in parallel, the chain s_{k+1} = M s_k + r_k in segment order, then every
// energy e_k in parallel from its true start state.  All of it in fp64: the kernel waits on a dependent chain, not on
// arithmetic.  Inside a segment the arithmetic is a fixed function of the samples and the start state, and the chain is
// a fixed function of (s_k, r_k), so no value depends on how the segments were cut into launches.
#include "kernels.h"

#include <cmath>

namespace mbv {

namespace {

constexpr int kLoudnessThreads = 256;      // segments in flight per workgroup, and the tile of the gate pass

// one sample through the cascade; s = shelf (s1, s2), high-pass (s1, s2).  Explicit fma: the rounding is the contract
__device__ inline double kw_step(const LoudnessParams& p, double x, double* s) {
  const double* c = p.coef;
  const double y1 = fma(c[0], x, s[0]);
  s[0] = fma(-c[3], y1, fma(c[1], x, s[1]));
  s[1] = fma(-c[4], y1, c[2] * x);
  const double y2 = fma(c[5], y1, s[2]);
  s[2] = fma(-c[8], y2, fma(c[6], y1, s[3]));
  s[3] = fma(-c[9], y2, c[7] * y1);
  return y2;
}

// H samples from state s (updated); -> the sum of y^2 in sample order.  A lane walks its own segment, so its loads
// share no cache line with its neighbours' and a wave has few of them in flight: the next kLoudnessBatch samples are
// loaded while the current ones go through the chain (measured on 16 rows of 30 s: 822 us with a load per step, 448 us
// so; the values are the same, only the loads move).
constexpr int kLoudnessBatch = 16;
__device__ inline double kw_segment(const LoudnessParams& p, const float* __restrict__ x, int H, double* s) {
  double e = 0.0;
  float cur[kLoudnessBatch], nxt[kLoudnessBatch];
  const int whole = H / kLoudnessBatch * kLoudnessBatch;
  if (whole > 0) {
#pragma unroll
    for (int j = 0; j < kLoudnessBatch; ++j) cur[j] = x[j];
  }
  for (int i = 0; i < whole; i += kLoudnessBatch) {
    const bool more = i + kLoudnessBatch < whole;
    if (more) {
#pragma unroll
      for (int j = 0; j < kLoudnessBatch; ++j) nxt[j] = x[i + kLoudnessBatch + j];
    }
#pragma unroll
    for (int j = 0; j < kLoudnessBatch; ++j) {
      const double y = kw_step(p, (double)cur[j], s);
      e = fma(y, y, e);
    }
    if (more) {
#pragma unroll
      for (int j = 0; j < kLoudnessBatch; ++j) cur[j] = nxt[j];
    }
  }
  for (int i = whole; i < H; ++i) {
    const double y = kw_step(p, (double)x[i], s);
    e = fma(y, y, e);
  }
  return e;
}

__global__ __launch_bounds__(kLoudnessThreads) void loudness_kernel(const LoudnessRow* __restrict__ rows,
                                                                    const LoudnessParams p) {
  __shared__ double sh_s[kLoudnessThreads][4];     // r_k of the tile, then s_k of the tile
  __shared__ double sh_cur[4];                     // the chain's state at the tile's first segment
  __shared__ double sh_e[kLoudnessThreads + 3];    // the gate pass's tile of energies
  const LoudnessRow k = rows[blockIdx.x];
  const int tid = threadIdx.x;
  const int H = p.H;
  int64_t v = k.avail;
  if (k.valid) {
    const int64_t q = *k.valid;
    v = q < 0 ? 0 : (q < v ? q : v);
  }
  const int64_t vseg = v / H;
  const int64_t ks = k.k0 < vseg ? k.k0 : vseg, ke = k.k1 < vseg ? k.k1 : vseg;
  if (tid < 4) sh_cur[tid] = k.k0 == 0 ? 0.0 : k.state[tid];
  __syncthreads();
  for (int64_t base = ks; base < ke; base += kLoudnessThreads) {
    const int64_t seg = base + tid;
    const bool active = seg < ke;
    const float* x = k.x + seg * H;                // (not read unless active: seg * H + H <= vseg * H <= avail)
    if (active) {
      double s[4] = {0.0, 0.0, 0.0, 0.0};
      kw_segment(p, x, H, s);
      for (int i = 0; i < 4; ++i) sh_s[tid][i] = s[i];
    }
    __syncthreads();
    if (tid == 0) {
      const int cnt = (int)(ke - base < kLoudnessThreads ? ke - base : kLoudnessThreads);
      double s[4] = {sh_cur[0], sh_cur[1], sh_cur[2], sh_cur[3]};
      for (int j = 0; j < cnt; ++j) {
        double nx[4];
        for (int i = 0; i < 4; ++i) {
          const double r = sh_s[j][i];
          nx[i] = fma(p.M[4 * i], s[0], fma(p.M[4 * i + 1], s[1], fma(p.M[4 * i + 2], s[2], fma(p.M[4 * i + 3], s[3], r))));
          sh_s[j][i] = s[i];
        }
        for (int i = 0; i < 4; ++i) s[i] = nx[i];
      }
      for (int i = 0; i < 4; ++i) sh_cur[i] = s[i];
    }
    __syncthreads();
    if (active) {
      double s[4] = {sh_s[tid][0], sh_s[tid][1], sh_s[tid][2], sh_s[tid][3]};
      k.energy[seg] = kw_segment(p, x, H, s);
    }
    __syncthreads();
  }
  // segments of the range at or past the row's valid length are absent: their energy is 0
  for (int64_t seg = (ke > k.k0 ? ke : k.k0) + tid; seg < k.k1; seg += kLoudnessThreads) k.energy[seg] = 0.0;
  if (tid < 4) k.state[tid] = sh_cur[tid];
  __syncthreads();                                 // this launch's energies are visible to the gate pass

  // blocks j = segments j .. j + 3 over everything measured so far, [0, ke); both sums in index order
  const int64_t nb = ke >= 4 ? ke - 3 : 0;
  const double norm = 4.0 * (double)H;
  double rel = -1.0, sum = 0.0;
  int64_t cnt = 0;
  for (int pass = 0; pass < 2; ++pass) {
    sum = 0.0;
    cnt = 0;
    for (int64_t base = 0; base < nb; base += kLoudnessThreads) {
      const int tile = (int)(nb - base < kLoudnessThreads ? nb - base : kLoudnessThreads);
      for (int i = tid; i < tile + 3; i += kLoudnessThreads) sh_e[i] = k.energy[base + i];   // base + i < nb + 3 = ke
      __syncthreads();
      if (tid == 0)
        for (int j = 0; j < tile; ++j) {
          const double z = (((sh_e[j] + sh_e[j + 1]) + sh_e[j + 2]) + sh_e[j + 3]) / norm;
          if (z > p.z_abs && z > rel) {
            sum += z;
            ++cnt;
          }
        }
      __syncthreads();
    }
    // the relative gate: 10 LU below the loudness of the absolute-gated blocks, i.e. a tenth of their mean square
    if (pass == 0) rel = cnt > 0 ? 0.1 * (sum / (double)cnt) : HUGE_VAL;
  }
  if (tid == 0) *k.L = cnt > 0 ? (float)(-0.691 + 10.0 * log10(sum / (double)cnt)) : -HUGE_VALF;
}

}  // namespace

void kweighting_host(int rate, LoudnessParams* p) {
  const double pi = 3.14159265358979323846, fs = (double)rate;
  {  // the shelf (BS.1770's first stage), re-derived for fs by the bilinear transform
    const double f0 = 1681.974450955533, G = 3.999843853973347, Q = 0.7071752369554196;
    const double K = std::tan(pi * f0 / fs), Vh = std::pow(10.0, G / 20.0), Vb = std::pow(Vh, 0.4996667741545416);
    const double a0 = 1.0 + K / Q + K * K;
    p->coef[0] = (Vh + Vb * K / Q + K * K) / a0;
    p->coef[1] = 2.0 * (K * K - Vh) / a0;
    p->coef[2] = (Vh - Vb * K / Q + K * K) / a0;
    p->coef[3] = 2.0 * (K * K - 1.0) / a0;
    p->coef[4] = (1.0 - K / Q + K * K) / a0;
  }
  {  // the high-pass (second stage); its numerator is not normalised, as in the standard's table
    const double f0 = 38.13547087602444, Q = 0.5003270373238773;
    const double K = std::tan(pi * f0 / fs), a0 = 1.0 + K / Q + K * K;
    p->coef[5] = 1.0;
    p->coef[6] = -2.0;
    p->coef[7] = 1.0;
    p->coef[8] = 2.0 * (K * K - 1.0) / a0;
    p->coef[9] = (1.0 - K / Q + K * K) / a0;
  }
  p->H = (rate + 5) / 10;
  p->pad_ = 0;
  p->z_abs = std::pow(10.0, (-70.0 + 0.691) / 10.0);
  // one zero-input step of the state (kw_step with x = 0), then its H-th power, accumulated in long double
  const double* c = p->coef;
  const long double A[4][4] = {{-c[3], 1, 0, 0},
                               {-c[4], 0, 0, 0},
                               {(long double)c[6] - (long double)c[8] * c[5], 0, -c[8], 1},
                               {(long double)c[7] - (long double)c[9] * c[5], 0, -c[9], 0}};
  long double P[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
  for (int step = 0; step < p->H; ++step) {
    long double N[4][4];
    for (int i = 0; i < 4; ++i)
      for (int j = 0; j < 4; ++j) N[i][j] = A[i][0] * P[0][j] + A[i][1] * P[1][j] + A[i][2] * P[2][j] + A[i][3] * P[3][j];
    for (int i = 0; i < 4; ++i)
      for (int j = 0; j < 4; ++j) P[i][j] = N[i][j];
  }
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) p->M[4 * i + j] = (double)P[i][j];
}

void launch_loudness(const LoudnessRow* rows, int n, const LoudnessParams& p, hipStream_t s) {
  hipLaunchKernelGGL(loudness_kernel, dim3((unsigned)n), dim3(kLoudnessThreads), 0, s, rows, p);
}

}  // namespace mbv
