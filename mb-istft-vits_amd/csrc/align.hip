// Forced alignment (SynthesizerTrn.forward, models.py:659-680): the negative cross-entropy matrix of a recording
// against its text, Monotonic Alignment Search over it (monotonic_align/core.pyx:7-32), and the cumulated
// durations that length regulation reads.
#include "kernels.h"

namespace mbv {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

// ---------------------------------------------------------------------------
// neg_cent (models.py:670-675):
//   value[b, y, x] = sum_d ( -1/2 log 2pi - logs[d, x] - 1/2 m[d, x]^2 s[d, x] )       (terms 1 and 4: per column)
//                  + sum_d ( -1/2 z[d, y]^2 ) s[d, x] + sum_d z[d, y] ( m[d, x] s[d, x] )   (terms 2 and 3)
// with s = e^{-2 logs}.  Terms 2 and 3 are one contraction of depth 2 I: A[y, :] = [-1/2 z^2 | z],
// Bm[:, x] = [s | m s], both built on the way into LDS and multiplied by the exact-fp32 matrix instruction
// (v_mfma_f32_32x32x2_f32: one fused multiply-add per step, k in order).  The column constant is summed by the
// threads that stage Bm (four partial sums per column, each in channel order) and added last.
// One workgroup of 256 threads = four waves = a 64 (y) x 64 (x) tile, one 32 x 32 block per wave; channels
// come in chunks of kNcD.  Only cells y < t_y[b], x < t_x[b] are stored, nothing at or beyond them is read.
// ---------------------------------------------------------------------------
constexpr int kNcTile = 64;
constexpr int kNcD = 16;                 // channels per LDS chunk (2 kNcD contraction steps)
constexpr float kHalfLog2Pi = 0.918938533204672741780329736406f;

__global__ __launch_bounds__(256) void neg_cent_kernel(const float* __restrict__ z_p, const float* __restrict__ m_p,
                                                       const float* __restrict__ logs_p, int64_t p_bstride,
                                                       const int* __restrict__ t_ys, const int* __restrict__ t_xs,
                                                       float* __restrict__ value, int I, int Tt, int Ts) {
  __shared__ float As[2 * kNcD][kNcTile + 1];
  __shared__ float Bs[2 * kNcD][kNcTile + 1];
  __shared__ float Cs[4][kNcTile];
  const int b = blockIdx.z;
  const int ty = min(t_ys[b], Tt), tx = min(t_xs[b], Ts);
  const int y0 = blockIdx.y * kNcTile, x0 = blockIdx.x * kNcTile;
  if (y0 >= ty || x0 >= tx) return;                      // (uniform over the workgroup)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = tid & 63, dq = tid >> 6;               // staging: column / frame `col`, channels dq, dq + 4, ...
  const float* zb = z_p + (int64_t)b * I * Tt;
  const float* mb = m_p + (int64_t)b * p_bstride;
  const float* lb = logs_p + (int64_t)b * p_bstride;
  const bool yin = y0 + col < ty, xin = x0 + col < tx;
  const int wy = (wave >> 1) * 32, wx = (wave & 1) * 32;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  float cpart = 0.f;
  for (int d0 = 0; d0 < I; d0 += kNcD) {
#pragma unroll
    for (int q = 0; q < kNcD / 4; ++q) {
      const int dl = dq + 4 * q, d = d0 + dl;
      float zv = 0.f, s = 0.f, ms = 0.f;
      if (d < I) {
        if (yin) zv = zb[(int64_t)d * Tt + y0 + col];
        if (xin) {
          const float lg = lb[(int64_t)d * Ts + x0 + col], mv = mb[(int64_t)d * Ts + x0 + col];
          s = expf(-2.f * lg);
          ms = mv * s;
          cpart += (-kHalfLog2Pi - lg) - 0.5f * mv * ms;
        }
      }
      As[dl][col] = -0.5f * zv * zv;
      As[kNcD + dl][col] = zv;
      Bs[dl][col] = s;
      Bs[kNcD + dl][col] = ms;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 2 * kNcD; k += 2) {
      const int kk = k + (lane >> 5);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[kk][wy + (lane & 31)], Bs[kk][wx + (lane & 31)], acc, 0, 0, 0);
    }
    __syncthreads();
  }
  Cs[dq][col] = cpart;
  __syncthreads();
  const int x = x0 + wx + (lane & 31);
  if (x < tx) {
    const int cx = wx + (lane & 31);
    const float cc = (Cs[0][cx] + Cs[1][cx]) + (Cs[2][cx] + Cs[3][cx]);
    float* vb = value + (int64_t)b * Tt * Ts;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int y = y0 + wy + 8 * (r >> 2) + 4 * (lane >> 5) + (r & 3);   // accumulator layout of the 32 x 32 block
      if (y < ty) vb[(int64_t)y * Ts + x] = acc[r] + cc;
    }
  }
}

// ---------------------------------------------------------------------------
// Monotonic Alignment Search: maximum_path_each of monotonic_align/core.pyx:7-32, cell for cell.
// One wavefront per utterance.  Lane l owns columns l, l + 64, ...; the cumulated previous row stays in registers
// and the left neighbour comes from the lane below (lane 63 of group j - 1 feeds lane 0 of group j), so a row step
// needs no barrier.  Rows of `value` are loaded kMasAhead steps ahead.  Per cell only the bit
// "value[y-1, x] < value[y-1, x-1]" (the backtrack's test, strict) is kept: one ballot per 64 columns per row, in
// LDS, or in `bits_g` when T_t * NJ * 8 bytes do not fit.  Lane 0 backtracks over the bits and leaves the column of
// every row in the first word of the row's bits; the durations are its run lengths.
//   status[b]: 0 ok; 1 t_x > t_y (no monotone path: core.pyx reads outside its arrays there);
//              2 t_x < 1 or t_y < 1; 3 a length outside the tensors.  Refused rows: w = 0, path = 0.
// ---------------------------------------------------------------------------
constexpr int kMasAhead = 4;
constexpr float kMaxNegVal = -1e9f;

template <int NJ, bool BITS_LDS>
__global__ __launch_bounds__(64) void max_path_kernel(const float* __restrict__ value, const int* __restrict__ t_ys,
                                                      const int* __restrict__ t_xs, int* __restrict__ w_out,
                                                      int* __restrict__ path, int* __restrict__ status,
                                                      unsigned long long* __restrict__ bits_g, int Tt, int Ts) {
  extern __shared__ unsigned long long bits_l[];
  const int b = blockIdx.x, lane = threadIdx.x;
  const int ty = t_ys[b], tx = t_xs[b];
  int st = 0;
  if (tx > Ts || ty > Tt) st = 3;
  else if (tx < 1 || ty < 1) st = 2;
  else if (tx > ty) st = 1;
  if (status && lane == 0) status[b] = st;
  int* wb = w_out + (int64_t)b * Ts;
  int* pb = path ? path + (int64_t)b * Tt * Ts : nullptr;
  if (st) {
    for (int x = lane; x < Ts; x += 64) wb[x] = 0;
    if (pb)
      for (int64_t i = lane; i < (int64_t)Tt * Ts; i += 64) pb[i] = 0;
    return;
  }
  unsigned long long* bits = BITS_LDS ? bits_l : bits_g + (int64_t)b * Tt * NJ;
  const float* vb = value + (int64_t)b * Tt * Ts;

  float ahead[kMasAhead][NJ];
#pragma unroll
  for (int p = 0; p < kMasAhead; ++p)
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int x = lane + 64 * j;
      ahead[p][j] = (p < ty && x < tx) ? vb[(int64_t)p * Ts + x] : 0.f;
    }
  float prev[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) prev[j] = 0.f;

  for (int yb = 0; yb < ty; yb += kMasAhead) {
#pragma unroll
    for (int p = 0; p < kMasAhead; ++p) {
      const int y = yb + p;
      if (y < ty) {                                       // (uniform)
        float cur[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
          cur[j] = ahead[p][j];
          const int x = lane + 64 * j, yn = y + kMasAhead;
          if (yn < ty && x < tx) ahead[p][j] = vb[(int64_t)yn * Ts + x];
        }
        const int lo = max(0, tx + y - ty), hi = min(tx, y + 1);
        float carry = 0.f;                                // prev[63 + 64 (j - 1)]
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
          const int x = lane + 64 * j;
          float left = __shfl_up(prev[j], 1);
          if (lane == 0) left = carry;
          carry = __shfl(prev[j], 63);
          const unsigned long long bal = __ballot(prev[j] < left);
          if (lane == 0) bits[(int64_t)y * NJ + j] = bal;
          const float v_cur = x == y ? kMaxNegVal : prev[j];
          const float v_prev = x == 0 ? (y == 0 ? 0.f : kMaxNegVal) : left;
          if (x >= lo && x < hi) prev[j] = cur[j] + (v_cur > v_prev ? v_cur : v_prev);   // max(v_prev, v_cur) as C's macro
        }
      }
    }
  }
  if (!BITS_LDS) __threadfence();
  __syncthreads();
  // backtrack (core.pyx:34-37)
  for (int x = tx + lane; x < Ts; x += 64) wb[x] = 0;
  if (lane == 0) {
    int index = tx - 1, run = 0;
    for (int y = ty - 1; y >= 0; --y) {
      bool leftmove = false;
      if (index != 0) {
        if (index == y) leftmove = true;
        else leftmove = (bits[(int64_t)y * NJ + (index >> 6)] >> (index & 63)) & 1ull;
      }
      bits[(int64_t)y * NJ] = (unsigned long long)index;
      ++run;
      if (leftmove) { wb[index] = run; run = 0; --index; }
    }
    wb[index] = run;
  }
  if (!pb) return;
  if (!BITS_LDS) __threadfence();
  __syncthreads();
  for (int y = 0; y < Tt; ++y) {
    const int index = y < ty ? (int)bits[(int64_t)y * NJ] : -1;
    for (int x = lane; x < Ts; x += 64) pb[(int64_t)y * Ts + x] = x == index ? 1 : 0;
  }
}

// ---------------------------------------------------------------------------
// Given integer durations -> what length regulation reads (models.py:717-719): w_ceil = w * x_mask,
// cum = inclusive cumsum, y_len = max(sum, 1).  The range rules and the marker are those of durations_kernel
// (ops.hip): a token of >= 2^20 frames, an utterance beyond 2^30, and here also a negative or non-integer entry,
// count 0 frames and flag the utterance: y_len = 1, y_lengths = -1.
//   dtype 0: int32, 1: int64, 2: float32
// ---------------------------------------------------------------------------
// ROWS (pooled admission, kernels.h): row b reads its own tensor rows[b].dur [t_text] of rows[b].dur_dtype; a row
// without one is left alone, predicted durations and all
template <bool ROWS>
__global__ __launch_bounds__(256) void set_durations_kernel(const void* w, int dtype, const AdmitEncRow* rows, const int* lens,
                                                            float* w_ceil, int* cum, int* ylen32, int64_t* ylen64,
                                                            const int* bad, int T) {
  __shared__ int scan[256];
  __shared__ int carry_s, over_s;
  const int b = blockIdx.x, tid = threadIdx.x;
  int len = lens[b];
  if (ROWS) {
    w = rows[b].dur;
    dtype = rows[b].dur_dtype;
    if (!w) return;                                // uniform over the workgroup
    if (len > rows[b].t_text) len = rows[b].t_text;    // never read past the row's own tensor
  }
  if (tid == 0) { carry_s = 0; over_s = 0; }
  __syncthreads();
  for (int t0 = 0; t0 < T; t0 += 256) {
    const int t = t0 + tid;
    int d = 0;
    if (t < T) {
      float wc = 0.f;
      bool ok = true;
      if (t < len) {
        const int64_t i = ROWS ? (int64_t)t : (int64_t)b * T + t;
        if (dtype == 0) {
          const int v = ((const int*)w)[i];
          ok = v >= 0 && v < (1 << 20);
          wc = (float)v;
        } else if (dtype == 1) {
          const long long v = ((const long long*)w)[i];
          ok = v >= 0 && v < (1 << 20);
          wc = (float)v;
        } else {
          wc = ((const float*)w)[i];
          ok = wc >= 0.f && wc < 1048576.f && wc == floorf(wc);
        }
      }
      if (w_ceil) w_ceil[(int64_t)b * T + t] = wc;
      if (ok) d = (int)wc;
      else over_s = 1;
    }
    scan[tid] = d;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
      int v = tid >= off ? scan[tid - off] : 0;
      __syncthreads();
      scan[tid] += v;
      __syncthreads();
    }
    const int carry = carry_s;
    if (t < T) cum[(int64_t)b * T + t] = carry + scan[tid];
    __syncthreads();
    if (tid == 255) {
      int c = carry + scan[255];
      if (c > (1 << 30)) { over_s = 1; c = 1 << 30; }
      carry_s = c;
    }
    __syncthreads();
  }
  if (tid == 0) {
    const int total = (carry_s < 1 || over_s) ? 1 : carry_s;
    ylen32[b] = total;
    if (ylen64) ylen64[b] = ((bad && bad[b]) || over_s) ? -1 : total;
  }
}

__global__ void align_status_kernel(const int* bad_x, const int* bad_y, const int* mas, int* status, float* w_f,
                                    const int* w_i, int B, int T) {
  // status: bit 0 an id / length / sid outside its table or tensor, bit 1 t_x > t_y, bit 2 an empty row
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < B && status) {
    const int s = mas[i];
    status[i] = ((bad_x[i] || bad_y[i] || s == 3) ? 1 : 0) | (s == 1 ? 2 : 0) | (s == 2 ? 4 : 0);
  }
  if (w_f && i < (int64_t)B * T) w_f[i] = (float)w_i[i];
}

template <int NJ>
void max_path_launch(const float* value, const int* t_ys, const int* t_xs, int* w, int* path, int* status,
                     unsigned long long* bits_g, int B, int Tt, int Ts, hipStream_t s) {
  const size_t lds = max_path_lds_bytes(Tt, Ts);
  if (lds)
    hipLaunchKernelGGL((max_path_kernel<NJ, true>), dim3(B), dim3(64), lds, s, value, t_ys, t_xs, w, path, status,
                       nullptr, Tt, Ts);
  else
    hipLaunchKernelGGL((max_path_kernel<NJ, false>), dim3(B), dim3(64), 0, s, value, t_ys, t_xs, w, path, status,
                       bits_g, Tt, Ts);
}

}  // namespace

void launch_neg_cent(const float* z_p, const float* m_p, const float* logs_p, int64_t p_bstride, const int* t_ys,
                     const int* t_xs, float* value, int B, int I, int Tt, int Ts, hipStream_t s) {
  dim3 grid((Ts + kNcTile - 1) / kNcTile, (Tt + kNcTile - 1) / kNcTile, B);
  hipLaunchKernelGGL(neg_cent_kernel, grid, dim3(256), 0, s, z_p, m_p, logs_p, p_bstride, t_ys, t_xs, value, I, Tt, Ts);
}

bool max_path_supported(int Ts) { return Ts >= 1 && Ts <= kMaxPathMaxTs; }

static int max_path_nj(int Ts) {
  int nj = 1;
  while (nj * 64 < Ts) nj *= 2;
  return nj;
}

size_t max_path_lds_bytes(int Tt, int Ts) {
  const size_t n = (size_t)Tt * max_path_nj(Ts) * 8;
  return n <= kMaxPathLdsBytes ? n : 0;
}

size_t max_path_scratch_bytes(int B, int Tt, int Ts) {
  return max_path_lds_bytes(Tt, Ts) ? 0 : (size_t)B * Tt * max_path_nj(Ts) * 8;
}

void launch_max_path(const float* value, const int* t_ys, const int* t_xs, int* w, int* path, int* status,
                     void* bits_scratch, int B, int Tt, int Ts, hipStream_t s) {
  unsigned long long* bg = (unsigned long long*)bits_scratch;
  switch (max_path_nj(Ts)) {
    case 1: max_path_launch<1>(value, t_ys, t_xs, w, path, status, bg, B, Tt, Ts, s); break;
    case 2: max_path_launch<2>(value, t_ys, t_xs, w, path, status, bg, B, Tt, Ts, s); break;
    case 4: max_path_launch<4>(value, t_ys, t_xs, w, path, status, bg, B, Tt, Ts, s); break;
    case 8: max_path_launch<8>(value, t_ys, t_xs, w, path, status, bg, B, Tt, Ts, s); break;
    default: max_path_launch<16>(value, t_ys, t_xs, w, path, status, bg, B, Tt, Ts, s); break;
  }
}

void launch_set_durations(const void* w, int dtype, const int* lens, float* w_ceil, int* cum, int* ylen32,
                          int64_t* ylen64, const int* bad, int B, int T, hipStream_t s) {
  hipLaunchKernelGGL(set_durations_kernel<false>, dim3(B), dim3(256), 0, s, w, dtype, nullptr, lens, w_ceil, cum, ylen32, ylen64, bad, T);
}

void launch_set_durations_rows(const AdmitEncRow* rows, const int* lens, float* w_ceil, int* cum, int* ylen32,
                               int64_t* ylen64, const int* bad, int B, int T, hipStream_t s) {
  hipLaunchKernelGGL(set_durations_kernel<true>, dim3(B), dim3(256), 0, s, nullptr, 0, rows, lens, w_ceil, cum, ylen32, ylen64, bad, T);
}

void launch_align_status(const int* bad_x, const int* bad_y, const int* mas, int* status, float* w_f, const int* w_i,
                         int B, int T, hipStream_t s) {
  const int64_t n = (int64_t)B * T;
  hipLaunchKernelGGL(align_status_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, bad_x, bad_y, mas, status,
                     w_f, w_i, B, T);
}

}  // namespace mbv
