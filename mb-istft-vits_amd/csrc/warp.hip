// Per-token pitch by varispeed: the time-warp kernel between the decoded model-rate row and the wire
// kernels.  It is resampy's interpolator (tests/resample_ref.py::resample_loop) with the quantities that loop holds
// once per call held once per OUTPUT: output t of a row sits at the float64 model time tau(t) that the row's rate
// table R and its prefix sum U give (kernels.h), the ratio there is 1 / R[f], and the window is read from the one
// table of the filter with the index step of that ratio.  A polyphase bank cannot serve it: the phase set changes with
// the frame.  The arithmetic is restated in float64 NumPy by tests/warp_ref.py; parity is with that module.
//
// Everything here is a pure function of the output index, so a row does not depend on how it is cut into ranges or
// which other rows share its launch, and the streamed, the pooled and the one-shot warp are the same bits.
#include "kernels.h"
#include "pcm_env.h"

#include <cmath>

namespace mbv {

namespace {
constexpr int kWarpNb = 512;   // table entries per zero crossing: 2^precision of both resampy filters
}

int64_t warp_plan(int hop, int64_t F, const float* R, double* U, int64_t* n_out) {
  for (int64_t f = 0; f < F; ++f)
    if (!(R[f] >= kPitchMin && R[f] <= kPitchMax)) return f;   // a NaN fails both comparisons
  double u = 0.0;
  U[0] = 0.0;
  for (int64_t f = 0; f < F; ++f) {
    u += (double)hop / (double)R[f];
    U[f + 1] = u;
  }
  *n_out = (int64_t)std::floor(u);
  return -1;
}

int warp_half_width(int num_zeros, int64_t F, const float* R) {
  double top = 1.0;
  for (int64_t f = 0; f < F; ++f)
    if ((double)R[f] > top) top = (double)R[f];
  return (int)std::ceil((double)num_zeros * top) + 2;
}

int64_t warp_ready(int hop, int64_t F, const float* R, const double* U, int num_zeros, int64_t in_avail) {
  if (in_avail >= F * hop) return (int64_t)std::floor(U[F]);
  const int64_t a = in_avail - warp_half_width(num_zeros, F, R);
  if (a <= 0) return 0;
  const int64_t g = a / hop;                                  // a < F hop: g < F
  const double pos = U[g] + (double)(a - g * hop) / (double)R[g];
  const int64_t count = (int64_t)std::floor(pos) - 1;
  return count > 0 ? count : 0;
}

// the frame of output t (the largest f < F with U[f] <= t; U[0] = 0 <= t) and its model time
__device__ __forceinline__ double warp_tau(const WarpRow& r, int64_t t, int* frame) {
#pragma clang fp contract(off)
  const double td = (double)t;
  int lo = 0, hi = r.F;                                       // U[lo] <= t, and frame hi starts after t or is F
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (r.U[mid] <= td) lo = mid;
    else hi = mid;
  }
  *frame = lo;
  const double base = (double)((int64_t)lo * r.hop);
  const double into = td - r.U[lo];
  const double adv = into * (double)r.R[lo];
  return base + adv;
}

// one wing of resampy's loop from the staged window: sum_i w(off + i step) xs[at + i dir], w by linear interpolation
// of the table.  Four partial sums, as resample_output keeps them
__device__ __forceinline__ float warp_wing(const float* xs, int at, int dir, int count, int off, int step, float eta,
                                           const float* __restrict__ win, const float* __restrict__ delta) {
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  int i = 0;
  for (; i + 3 < count; i += 4) {
    const int j = off + i * step;
    a0 = fmaf(fmaf(eta, delta[j], win[j]), xs[at + i * dir], a0);
    a1 = fmaf(fmaf(eta, delta[j + step], win[j + step]), xs[at + (i + 1) * dir], a1);
    a2 = fmaf(fmaf(eta, delta[j + 2 * step], win[j + 2 * step]), xs[at + (i + 2) * dir], a2);
    a3 = fmaf(fmaf(eta, delta[j + 3 * step], win[j + 3 * step]), xs[at + (i + 3) * dir], a3);
  }
  for (; i < count; ++i) {
    const int j = off + i * step;
    a0 = fmaf(fmaf(eta, delta[j], win[j]), xs[at + i * dir], a0);
  }
  return (a0 + a1) + (a2 + a3);
}

// Row blockIdx.y of the table, tile out_first + 256 blockIdx.x of its own range; the grid holds the tiles of the
// longest range and a tile past its row's end returns after the table load (uniform over the workgroup).
//   1. every thread finds the model time of the tile's first and last output and of its own: three binary searches on
//      U, no exchange.  A thread past the range takes the last output's place and stores nothing
//   2. the workgroup stages x[j0, j0 + W), j0 = floor(tau(first)) - hw, W up to floor(tau(last)) + hw + 2 - j0, through
//      the one predicated read: env_mul(x[j], env, j) for 0 <= j < min(n, in_avail), a zero anywhere else.  The row
//      beyond the decoded frontier is uninitialised memory and is never loaded
//   3. each thread runs the two tap loops from LDS.  Their counts are those of resampy's loop, cut to the staged
//      window: with hw as the host computes it nothing is cut, and whatever a table holds no index leaves the window
// One barrier; no thread leaves before it.  LDS: kWarpWindow floats.
__global__ void __launch_bounds__(kWarpTile) warp_ranges_kernel(const WarpRow* __restrict__ rows) {
  __shared__ float xs[kWarpWindow];
  const WarpRow r = rows[blockIdx.y];
  const int64_t t0 = r.out_first + (int64_t)blockIdx.x * kWarpTile;
  if (t0 >= r.out_end) return;                            // uniform over the workgroup: a shorter range than the grid's
  int64_t t_last = t0 + kWarpTile - 1;
  if (t_last > r.out_end - 1) t_last = r.out_end - 1;
  const int64_t t = t0 + threadIdx.x;
  const bool live = t <= t_last;
  int f, f_edge;
  const int64_t j0 = (int64_t)warp_tau(r, t0, &f_edge) - r.hw;
  const int64_t j_end = (int64_t)warp_tau(r, t_last, &f_edge) + r.hw + 2;
  int64_t W = j_end - j0;
  if (W > kWarpWindow) W = kWarpWindow;
  const int64_t limit = r.n < r.in_avail ? r.n : r.in_avail;
  for (int i = threadIdx.x; i < W; i += kWarpTile) {
    const int64_t j = j0 + i;
    xs[i] = (j >= 0 && j < limit) ? env_mul(r.x[j], r.env, j) : 0.f;
  }
  __syncthreads();
  if (!live) return;

  const double tau = warp_tau(r, t, &f);
  const float rate = fminf(fmaxf(r.R[f], kPitchMin), kPitchMax);   // the bounds the host has checked: step >= 256
  const double scale = rate > 1.f ? 1.0 / (double)rate : 1.0;
  const int step = (int)(scale * kWarpNb);                // truncated, as resampy's int(scale * num_table)
  const int nwin = kWarpNb * r.num_zeros + 1;
  const float* __restrict__ win = r.win;
  const float* __restrict__ delta = r.win + nwin;
  const int64_t nt = (int64_t)tau;
  const int64_t cw = nt - j0;                             // xs[c] = the sample at floor(tau)
  const bool inside = cw >= 0 && cw < W;                  // always, with the tables the host has planned
  const int c = inside ? (int)cw : 0;
  float sum = 0.f;
  {
#pragma clang fp contract(off)
    double frac = scale * (tau - (double)nt);
    double idx = frac * kWarpNb;
    int off = min(max((int)idx, 0), kWarpNb);             // 0 <= frac <= scale <= 1: never clamped
    int count = (nwin - off) / step;                      // left wing: x[nt - i]
    if (count > c + 1) count = c + 1;
    if (!inside) count = 0;
    sum = warp_wing(xs, c, -1, count, off, step, (float)(idx - off), win, delta);
    frac = scale - frac;
    idx = frac * kWarpNb;
    off = min(max((int)idx, 0), kWarpNb);
    count = (nwin - off) / step;                          // right wing: x[nt + 1 + k]
    if (count > (int)W - c - 1) count = (int)W - c - 1;
    if (!inside) count = 0;
    sum += warp_wing(xs, c + 1, 1, count, off, step, (float)(idx - off), win, delta);
  }
  // the window times scale: one factor for every tap of the output
  r.out[t] = rate > 1.f ? sum * (float)scale : sum;
}

void launch_warp_ranges(const WarpRow* rows, int n, int64_t max_count, hipStream_t s) {
  const int64_t bx = (max_count + kWarpTile - 1) / kWarpTile;
  hipLaunchKernelGGL(warp_ranges_kernel, dim3((unsigned)bx, n), dim3(kWarpTile), 0, s, rows);
}

}  // namespace mbv
