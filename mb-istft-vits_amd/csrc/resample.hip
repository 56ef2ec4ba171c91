// Band-limited resampling of waveform rows: librosa 0.9.2 `resample(res_type="kaiser_best" | "kaiser_fast")`,
// i.e. resampy's windowed-sinc interpolator followed by librosa's fix_length (tts_vits.py:199-200).
//
// resampy places output t at the float64 input time t / ratio and evaluates its interpolation table
// there.  With target / orig = L / M in lowest terms that time is t M / L: output t reads around
// n_t = floor(t M / L) with fractional phase r = (t M) mod L, so only L distinct weight vectors exist.
// The host builds them once (float64, resampy's arithmetic: table lookup with linear interpolation, the
// truncated index step int(scale * 2^precision)), rounds them to fp32 and the kernel is a plain
// polyphase FIR: out[t] = sum_k bank[r][k] * x[n_t - left + k], K taps per phase.
// One case does not follow from t M / L: at r = 0 the float64 quotient t / ratio can round to just
// below the integer n_t, and resampy then interpolates from n_t - 1 at fraction ~1.  When downsampling
// that is not the same filter (the index step is truncated), so the bank has a row L for it: phase
// fraction 1, read around n_t - 1.  The kernel evaluates t / ratio in fp64 for r = 0 to pick the row.
//
// Parity is with a restatement of resampy's algorithm (tests/resample_ref.py), not with the library:
// its filter tables are rebuilt from the documented specs here.
#include "kernels.h"
#include "g711.h"
#include "pcm_env.h"

#include <cmath>
#include <cstdio>
#include <type_traits>
#include <vector>

namespace mbv {

namespace {

struct FilterSpec { int num_zeros, precision; double beta, rolloff; };
// resampy's filter specs (kaiser_best / kaiser_fast)
const FilterSpec kSpecs[2] = {
    {64, 9, 14.769656459379492, 0.9475937167399596},
    {16, 9, 8.555504641634386, 0.85},
};

// modified Bessel function of the first kind, order 0: the power series (all terms positive, no cancellation)
double bessel_i0(double x) {
  const double q = 0.25 * x * x;
  double term = 1.0, sum = 1.0;
  for (int k = 1; k < 500; ++k) {
    term *= q / ((double)k * k);
    sum += term;
    if (term < sum * 1e-17) break;
  }
  return sum;
}

double sinc(double x) {
  if (x == 0.0) return 1.0;
  const double px = M_PI * x;
  return std::sin(px) / px;
}

int64_t gcd64(int64_t a, int64_t b) { while (b) { int64_t t = a % b; a = b; b = t; } return a; }

}  // namespace

int resample_reduce(int orig_sr, int target_sr, int* L, int* M) {
  if (orig_sr <= 0 || target_sr <= 0) return 1;
  const int64_t g = gcd64(orig_sr, target_sr);
  *L = (int)(target_sr / g);
  *M = (int)(orig_sr / g);
  return 0;
}

void resample_window(int filter, std::vector<double>* win, int* num_zeros, int* nb) {
  const FilterSpec& f = kSpecs[filter];
  const int n = (1 << f.precision) * f.num_zeros;
  const int nwin = n + 1;
  win->resize(nwin);
  const double alpha = (double)n;            // (2n + 1 - 1) / 2
  const double i0b = bessel_i0(f.beta);
  for (int i = 0; i < nwin; ++i) {
    const double u = (double)i / alpha;      // (j - alpha) / alpha for j = n + i
    const double kw = bessel_i0(f.beta * std::sqrt(1.0 - u * u)) / i0b;
    const double x = (double)i * ((double)f.num_zeros / (double)n);
    (*win)[i] = kw * (f.rolloff * sinc(f.rolloff * x));
  }
  if (num_zeros) *num_zeros = f.num_zeros;
  if (nb) *nb = 1 << f.precision;
}

const char* resample_bank(int orig_sr, int target_sr, int filter, std::vector<float>* bank, ResampleGeom* geom) {
  if (orig_sr <= 0 || target_sr <= 0) return "sample rates must be positive";
  if (filter != 0 && filter != 1) return "unknown resampling filter (0 = kaiser_best, 1 = kaiser_fast)";
  ResampleGeom g{};
  resample_reduce(orig_sr, target_sr, &g.L, &g.M);
  if (g.L > kResampleMaxPhases)
    return "rate pair needs more than 4096 polyphase phases (target / gcd(orig, target) > 4096)";
  const FilterSpec& f = kSpecs[filter];
  const int nb = 1 << f.precision;
  const int n = nb * f.num_zeros;
  const int nwin = n + 1;
  const double ratio = (double)target_sr / (double)orig_sr;
  const double scale = ratio < 1.0 ? ratio : 1.0;
  const int step = (int)(scale * nb);        // truncation as resampy's int(scale * num_table)
  if (step < 1) return "downsampling ratio too small for the filter table";
  // win = kaiser(2n + 1, beta)[n:] * rolloff * sinc(rolloff * linspace(0, num_zeros, n + 1)); the geometry alone
  // (bank == null: mbv_resample_ready, once per streamed chunk) needs only the wing counts, not the table
  std::vector<double> win, delta;
  if (bank) {
    resample_window(filter, &win, nullptr, nullptr);
    delta.resize(nwin);
    if (ratio < 1.0)
      for (auto& w : win) w *= ratio;
    for (int i = 0; i + 1 < nwin; ++i) delta[i] = win[i + 1] - win[i];
    delta[nwin - 1] = 0.0;
  }

  // one wing of resampy's loop at fractional position `frac`: count and (offset, eta) into the table
  struct Wing { int off, count; double eta; };
  auto wing = [&](double frac) {
    const double idx = frac * nb;
    Wing w;
    w.off = (int)idx;
    w.eta = idx - w.off;
    w.count = (nwin - w.off) / step;
    return w;
  };
  // row r < L: fraction r / L;  row L: fraction 1 (the r = 0 output reached from below, read around n_t - 1)
  int lmax = 0, rmax = 0;
  for (int r = 0; r <= g.L; ++r) {
    const double frac = scale * ((double)r / (double)g.L);
    const Wing a = wing(frac), b = wing(scale - frac);
    if (a.count > lmax) lmax = a.count;
    if (b.count > rmax) rmax = b.count;
  }
  g.left = lmax - 1;                         // left wing: x[n - i], i < lmax
  g.K = (g.left + 1 + rmax + 3) / 4 * 4;     // right wing: x[n + 1 + k], k < rmax; padded to whole float4 rows
  if (g.K > kResampleMaxTaps) return "rate pair needs more than 4096 taps per phase (downsampling ratio too small)";
  if (resample_lds_floats(g) > kResampleMaxLdsFloats) return "rate pair needs an input window larger than the LDS stage";
  g.ratio = ratio;
  if (bank) {
    bank->assign((size_t)(g.L + 1) * g.K, 0.f);
    std::vector<double> row(g.K);
    for (int r = 0; r <= g.L; ++r) {
      std::fill(row.begin(), row.end(), 0.0);
      const double frac = scale * ((double)r / (double)g.L);
      const Wing a = wing(frac), b = wing(scale - frac);
      for (int i = 0; i < a.count; ++i) {
        const int j = a.off + i * step;
        row[g.left - i] = win[j] + a.eta * delta[j];
      }
      for (int k = 0; k < b.count; ++k) {
        const int j = b.off + k * step;
        row[g.left + 1 + k] = win[j] + b.eta * delta[j];
      }
      for (int k = 0; k < g.K; ++k) (*bank)[(size_t)r * g.K + k] = (float)row[k];
    }
  }
  *geom = g;
  return nullptr;
}

int64_t resample_ready(const ResampleGeom& g, int64_t in_avail, int64_t in_total) {
  if (in_avail < 0) in_avail = 0;
  const int64_t all = (int64_t)std::ceil((double)in_total * g.ratio);   // fix_length of the whole row, as mbv_resample
  if (in_avail >= in_total) return all;
  // output t reads up to x[floor(t M / L) - left + K - 1]: final once floor(t M / L) < in_avail - K + left + 1
  const int64_t a = in_avail - g.K + g.left + 1;
  if (a <= 0) return 0;
  const int64_t r = (a * g.L + g.M - 1) / g.M;
  return r < all ? r : all;
}

const char* limiter_refusal(const LimiterParams& p) {
  if (!(p.ceiling > 0.f && p.ceiling <= 1.f)) return "limiter ceiling must be in (0, 1]";
  if (p.lookahead < 0 || p.lookahead > kLimiterMaxLookahead) return "limiter lookahead must be in [0, 255] output samples";
  if (p.hold < 0 || p.hold > kLimiterMaxHold) return "limiter hold must be in [0, 1024] output samples";
  return nullptr;
}

int64_t resample_ready_open(const ResampleGeom& g, int64_t in_avail) {
  // the open branch of resample_ready: floor(t M / L) - left + K - 1 < in_avail.  No total enters it.
  const int64_t a = in_avail - g.K + g.left + 1;
  if (a <= 0) return 0;
  return (a * g.L + g.M - 1) / g.M;
}

// ---------------------------------------------------------------------------------------------------
// Device code shared by every kernel below: the staged input window of a tile and the polyphase sum of one
// output.  One workgroup = up to kResampleTile consecutive outputs of one row, one output
// per thread.  The input window they read (with the K-tap halo) is staged in LDS, zero outside [0, limit):
// resampy's min(n + 1, ...) / min(n_in - n - 1, ...) edge rule, every row resampled as if it were alone.
// ---------------------------------------------------------------------------------------------------
// first staged input index of the tile that starts at output t0 (- 1: room for row L, which reads around n_t - 1)
__device__ __forceinline__ int64_t resample_window_first(int64_t t0, int L, int M, int left) {
  return (t0 * M) / L - left - 1;
}

// stage x[j0, j0 + W) of one row, W = window of outputs [t0, t_last]; indices outside [0, limit) are not
// loaded (zeros).  W <= resample_lds_floats(geom), checked on the host.
__device__ __forceinline__ void resample_stage(float* xs, const float* __restrict__ xb, int64_t j0, int64_t t_last,
                                               int L, int M, int K, int left, int64_t limit) {
  const int W = (int)((t_last * M) / L - left + K - j0);
  for (int i = threadIdx.x; i < W; i += kResampleTile) {
    const int64_t j = j0 + i;
    xs[i] = (j >= 0 && j < limit) ? xb[j] : 0.f;
  }
}

// the same window of an int16 recording: (float)s * 2^-15 is exact, bitwise pcm.float() / 32768
__device__ __forceinline__ void resample_stage(float* xs, const short* __restrict__ xb, int64_t j0, int64_t t_last,
                                               int L, int M, int K, int left, int64_t limit) {
  const int W = (int)((t_last * M) / L - left + K - j0);
  for (int i = threadIdx.x; i < W; i += kResampleTile) {
    const int64_t j = j0 + i;
    xs[i] = (j >= 0 && j < limit) ? (float)xb[j] * (1.f / 32768.f) : 0.f;
  }
}

// the same window of a G.711 recording: the byte expands to its int16 (g711.h), then as above
template <int LAW>
__device__ __forceinline__ void resample_stage(float* xs, const uint8_t* __restrict__ xb, int64_t j0, int64_t t_last,
                                               int L, int M, int K, int left, int64_t limit) {
  const int W = (int)((t_last * M) / L - left + K - j0);
  for (int i = threadIdx.x; i < W; i += kResampleTile) {
    const int64_t j = j0 + i;
    xs[i] = (j >= 0 && j < limit) ? (float)g711_decode<LAW>(xb[j]) * (1.f / 32768.f) : 0.f;
  }
}

// The segmented source of a turn row (kernels.h).  The scan over the row's few segments has a uniform
// trip count and reads the table through uniform addresses; per element it only selects an address and a ramp, and
// the ONE load behind it is predicated exactly as the plain row's is (below the frontier, inside a segment).
// `envs` (ENV = true only): envs[s] beside segs[s], the gain envelope of that segment (gain null: none)
struct TurnSrc { const TurnSeg* __restrict__ segs; int n; const PcmEnv* __restrict__ envs; };

// timeline index j: zero in a pause, beyond the timeline and at or past `limit` (nothing there is loaded).  ENV: the
// envelope of the segment first, its de-click ramp after it (the order of a timeline assembled from shaped waves)
template <bool ENV>
__device__ __forceinline__ float turn_sample(const TurnSrc& src, int64_t j, int64_t limit) {
  const float* p = nullptr;
  float g = 1.f;
  bool ramped = false;
  int es = 0;
  int64_t li = 0;
  for (int s = 0; s < src.n; ++s) {
    const TurnSeg sg = src.segs[s];
    const int64_t i = j - sg.start;
    const bool in = i >= 0 && i < sg.n;
    const int64_t fall = i - (sg.n - sg.ramp);             // >= 0: inside the falling ramp
    const bool rise = i < sg.ramp;
    const float gs = (float)(rise ? i + 1 : sg.ramp - fall) * sg.inv;
    p = in ? sg.x + i : p;
    g = in ? gs : g;
    ramped = in ? (rise || fall >= 0) : ramped;
    if constexpr (ENV) {
      es = in ? s : es;
      li = in ? i : li;
    }
  }
  if (!p || j >= limit) return 0.f;
  float v = *p;
  if constexpr (ENV) v = env_mul(v, src.envs[es], li);
  return ramped ? v * g : v;
}

// What a row of a wire launch reads from, and the ONE place where it is read: the plain row `xb` (TURN = false), shaped
// by `env` under ENV, or the timeline `src` of a turn.  Nothing at or past `limit` (and nothing in front of 0) is
// loaded: a zero stands there.  The members a <TURN, ENV> does not name above are never set and never read.
template <bool TURN, bool ENV>
struct WireSource {
  const float* __restrict__ xb;
  PcmEnv env;
  TurnSrc src;
  // the sample at index j of the row (of the timeline): what FIR = false hands on as it is
  __device__ __forceinline__ float at(int64_t j, int64_t limit) const {
    if constexpr (TURN) {
      return turn_sample<ENV>(src, j, limit);
    } else {
      if (j < 0 || j >= limit) return 0.f;
      if constexpr (ENV) return env_mul(xb[j], env, j);
      else return xb[j];
    }
  }
  // the window of the fp32 resample_stage above, from this source
  __device__ __forceinline__ void stage(float* xs, int64_t j0, int64_t t_last, const ResampleGeom& g,
                                        int64_t limit) const {
    const int W = (int)((t_last * g.M) / g.L - g.left + g.K - j0);
    for (int i = threadIdx.x; i < W; i += kResampleTile) xs[i] = at(j0 + i, limit);
  }
};

// output t from the staged window
__device__ __forceinline__ float resample_output(const float* xs, int64_t j0, int64_t t, const float* __restrict__ bank,
                                                 int L, int M, int K, int left, double ratio) {
  const int64_t q = t * M;
  int64_t nt = q / L;
  int r = (int)(q - nt * L);
  if (r == 0 && t > 0 && (double)t / ratio < (double)nt) { r = L; --nt; }   // resampy: int(t / ratio) = n_t - 1
  const float4* w4 = reinterpret_cast<const float4*>(bank + (size_t)r * K);
  const float* xw = xs + (nt - left - j0);
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  for (int k = 0; k < K / 4; ++k) {
    const float4 w = w4[k];
    a0 = fmaf(w.x, xw[4 * k + 0], a0);
    a1 = fmaf(w.y, xw[4 * k + 1], a1);
    a2 = fmaf(w.z, xw[4 * k + 2], a2);
    a3 = fmaf(w.w, xw[4 * k + 3], a3);
  }
  return (a0 + a1) + (a2 + a3);
}

// valid input samples of row b (clamped to the row) and the outputs resampy computes from them
__device__ __forceinline__ int64_t resample_row_valid(const int64_t* __restrict__ valid, int b, int64_t in_stride) {
  if (!valid) return in_stride;
  const int64_t n = valid[b];
  return n < 0 ? 0 : (n > in_stride ? in_stride : n);
}

// ---------------------------------------------------------------------------------------------------
// fp32 tile: outputs [t0, t0 + kResampleTile) below out_end of one row, from its input samples [0, n); outputs in
// [n_out, out_end) are written as zeros (librosa's fix_length pad and the row padding).  x is fp32 (dtype 0), int16
// (dtype 1) or G.711 bytes (kWaveUlaw, kWaveAlaw).  The one-shot kernel and the live-input kernel both store through
// this function.
// ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ void resample_f32_tile(float* xs, const void* x, int dtype, int64_t n, int64_t n_out,
                                                  int64_t t0, int64_t out_end, float* ob,
                                                  const float* __restrict__ bank, int L, int M, int K, int left,
                                                  double ratio) {
  const int64_t t = t0 + threadIdx.x;
  if (t0 >= n_out) {                                      // uniform over the workgroup: tail only
    if (t < out_end) ob[t] = 0.f;
    return;
  }
  const int64_t t_last = (t0 + kResampleTile - 1 < n_out - 1) ? t0 + kResampleTile - 1 : n_out - 1;
  const int64_t j0 = resample_window_first(t0, L, M, left);
  if (dtype == 1) resample_stage(xs, static_cast<const short*>(x), j0, t_last, L, M, K, left, n);
  else if (dtype == kWaveUlaw) resample_stage<kLawUlaw>(xs, static_cast<const uint8_t*>(x), j0, t_last, L, M, K, left, n);
  else if (dtype == kWaveAlaw) resample_stage<kLawAlaw>(xs, static_cast<const uint8_t*>(x), j0, t_last, L, M, K, left, n);
  else resample_stage(xs, static_cast<const float*>(x), j0, t_last, L, M, K, left, n);
  __syncthreads();
  if (t >= out_end) return;
  if (t >= n_out) { ob[t] = 0.f; return; }
  ob[t] = resample_output(xs, j0, t, bank, L, M, K, left, ratio);
}

// One-shot kernel: whole rows, the closed fp32 row with the range [0, out_stride) (dtype is a constant here: no branch)
__global__ void __launch_bounds__(kResampleTile)
resample_kernel(const float* __restrict__ x, const int64_t* __restrict__ valid, int64_t in_stride,
                const float* __restrict__ bank, int L, int M, int K, int left, double ratio,
                float* __restrict__ out, int64_t out_stride, int64_t* __restrict__ out_samples) {
  extern __shared__ float xs[];
  const int b = blockIdx.y;
  const int64_t n = resample_row_valid(valid, b, in_stride);
  int64_t n_out = (int64_t)((double)n * ratio);          // resampy: int(n_in * sample_ratio)
  if (n_out > out_stride) n_out = out_stride;
  if (blockIdx.x == 0 && threadIdx.x == 0 && out_samples) {
    int64_t keep = (int64_t)ceil((double)n * ratio);     // librosa fix_length: int(np.ceil(n * ratio))
    out_samples[b] = keep > out_stride ? out_stride : keep;
  }
  resample_f32_tile(xs, x + (int64_t)b * in_stride, 0, n, n_out, (int64_t)blockIdx.x * kResampleTile, out_stride,
                    out + (int64_t)b * out_stride, bank, L, M, K, left, ratio);
}

void launch_resample(const float* x, const int64_t* valid, int B, int64_t in_stride, const float* bank,
                     const ResampleGeom& g, float* out, int64_t out_stride, int64_t* out_samples, hipStream_t s) {
  const int64_t bx = (out_stride + kResampleTile - 1) / kResampleTile;
  const size_t lds = (size_t)resample_lds_floats(g) * sizeof(float);
  hipLaunchKernelGGL(resample_kernel, dim3((unsigned)bx, B), dim3(kResampleTile), lds, s, x, valid, in_stride,
                     bank, g.L, g.M, g.K, g.left, g.ratio, out, out_stride, out_samples);
}

// Live input (mbv_resample_ranges): the one-shot tile over the outputs [out_first, out_end) of many recordings that
// are still arriving, blockIdx.y = table row, blockIdx.x = tile out_first + 256 x of that row's own range; the grid
// holds the tiles of the longest range and a tile past its row's end returns after the table load.
//   - the caller has checked out_end against the readiness of the row, so no stored output of an open row has a tap
//     at or past n; the staging still refuses to load those indices (the raw buffer beyond the frontier is
//     uninitialised memory)
//   - an open row computes every output of its range; a closed one stores zeros in [int(n ratio), out_end)
// No atomics, no LDS beyond resample_lds_floats(g).
__global__ void __launch_bounds__(kResampleTile)
resample_ranges_kernel(const ResampleRangeRow* __restrict__ rows, const float* __restrict__ bank, int L, int M, int K,
                       int left, double ratio) {
  extern __shared__ float xs[];
  const ResampleRangeRow r = rows[blockIdx.y];
  const int64_t t0 = r.out_first + (int64_t)blockIdx.x * kResampleTile;
  if (t0 >= r.out_end) return;                            // uniform over the workgroup: a shorter range than the grid's
  int64_t n_out = r.out_end;
  if (r.closed) {
    n_out = (int64_t)((double)r.n * ratio);               // resampy: int(n_in * sample_ratio)
    if (n_out > r.out_end) n_out = r.out_end;
  }
  resample_f32_tile(xs, r.x, r.dtype, r.n, n_out, t0, r.out_end, r.out, bank, L, M, K, left, ratio);
}

void launch_resample_ranges(const ResampleRangeRow* rows, int n, int64_t max_count, const float* bank,
                            const ResampleGeom& g, hipStream_t s) {
  const int64_t bx = (max_count + kResampleTile - 1) / kResampleTile;
  const size_t lds = (size_t)resample_lds_floats(g) * sizeof(float);
  hipLaunchKernelGGL(resample_ranges_kernel, dim3((unsigned)bx, n), dim3(kResampleTile), lds, s, rows, bank, g.L, g.M,
                     g.K, g.left, g.ratio);
}

// ---------------------------------------------------------------------------------------------------
// int16 tile of the streamed wire path: outputs [out_first + 256 blockIdx.x, ..) below out_end of one row (a
// PcmPoolRow), from its input samples [0, in_avail) only, fused with the int16 epilogue of pcm16_kernel (ops.hip) and
// a running peak.  The ranged kernel and the pooled one both store through this function.
//   - the caller has checked out_end <= resample_ready(in_avail), so no stored output has a tap at or past in_avail;
//     the staging still refuses to load those indices (the row beyond the decoded frontier is uninitialised memory,
//     and a zero tap times a NaN is a NaN)
//   - the first tile writes out_samples even for an empty range; any other tile at or past out_end returns at once
//   - FIR = false: equal rates, the sample itself (a ranged pcm16 with a given peak)
//   - epilogue in the order of pcm16_kernel: (v / peak) * 0.9 where peak > 0.01, clip, * 32767, truncate
//   - running = max(running, |v|) over the row's computed outputs (t < int(n ratio); the samples between that and
//     ceil(n ratio) are zeros), by atomicMax on the bits as absmax_kernel does: one per wave
//   - each int16 goes to the row's own pcm[t] and, with a packed buffer, to packed[packed_off + t - out_first]
//   - LIM = true: the look-ahead limiter between the static gain and the clip (resample_pcm16_limited below); the
//     caller has checked out_end + lookahead <= resample_ready(in_avail) unless the row is complete.  LIM = false
//     never reads the row's `lim`
//   - LAW = kLawUlaw / kLawAlaw: the G.711 byte of that int16 is stored where the int16 would be, so
//     pcm, pcm_cap, packed and packed_off then count bytes; everything before the store is the same code.  Uniform
//     over a launch, like FIR and LIM
//   - fade (kernels.h): the value the clip takes is first scaled by the ramp of its own index t; a row
//     without one (count < 0) skips the multiply, so its bits are those of a launch that knows no fade.  FADE = false
//     (a ranged launch without a fade) compiles the test away: that instantiation is the kernel of before
//   - the input is read through a WireSource (above) and nowhere else: its stage() for the FIR, its at() for FIR = false
//   - TURN = true: the row's input is the timeline of `src` (r.x is null), read through turn_sample;
//     in_total / in_avail count timeline samples.  TURN = false never reads `src`: those instantiations are the kernels
//     of before
//   - ENV = true: a row may carry a gain envelope `env` (a turn row: one per segment, src.envs).  The
//     sample is multiplied where the source is read (WireSource::at, turn_sample); FIR, peak, static gain, limiter,
//     fade and clip see the shaped signal.  A row of such a
//     launch without one (gain null) executes no multiply.  ENV = false never reads `env`: those instantiations are the
//     kernels of before, and a launch in which no row is shaped uses them
// ---------------------------------------------------------------------------------------------------
// what a wire launch stores for the int16 q
template <int LAW>
struct WireSample {
  using type = uint8_t;
  static __device__ __forceinline__ uint8_t of(short q) { return g711_encode<LAW>(q); }
};
template <>
struct WireSample<kLawNone> {
  using type = short;
  static __device__ __forceinline__ short of(short q) { return q; }
};

// the ramp of output t: 1 in front of the fade, (count - k) inv inside it, 0 behind it (a range that overshoots)
__device__ __forceinline__ float fade_gain(const PcmFade& f, int64_t t) {
  const int64_t k = t - f.first;
  if (k < 0) return 1.f;
  return k < f.count ? (float)(f.count - k) * f.inv : 0.f;
}

// The epilogue of both tiles for output t < out_end: a live value (one the row computed) is scaled by the ramp of its
// own index, clipped and scaled to int16; then truncation, the codec, and the store to the row's pcm and to the packed
// buffer (pk null: none).  live = false with v = 0 stores the zero of [n_out, out_end).  FADE = false never reads `fade`
template <int LAW, bool FADE>
__device__ __forceinline__ void wire_store(float v, bool live, int64_t t, const PcmFade& fade,
                                           typename WireSample<LAW>::type* pcm, typename WireSample<LAW>::type* pk) {
  if (live) {
    if constexpr (FADE)
      if (fade.count >= 0) v *= fade_gain(fade, t);
    v = fminf(fmaxf(v, -1.f), 1.f);
    v = v * 32767.f;
  }
  const typename WireSample<LAW>::type q = WireSample<LAW>::of((short)(int)v);
  pcm[t] = q;
  if (pk) pk[t] = q;
}

// running = max(running, m) with m >= 0 each thread's |v| (0 where it has none): one atomic per wave at the most.
// Every thread of the workgroup calls it (the shuffle is over whole waves)
__device__ __forceinline__ void wire_peak(unsigned* running, float m) {
  if (running) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
    // m >= 0: bit order == value order.  The peak only grows, so a wave that reads a value at least its own has
    // nothing to add: most waves skip the atomic (hundreds of them on one address serialise in L2)
    if ((threadIdx.x & 63) == 0 && __float_as_uint(m) > __atomic_load_n(running, __ATOMIC_RELAXED))
      atomicMax(running, __float_as_uint(m));
  }
}

// The limited tile of outputs [t0, t_end), t_end = min(t0 + 256, out_end, n_out) > t0:
//   1. v[k], static gain included, for k in [t0 - La - H, t_end - 1 + La] (zero outside [0, n_out)) from ONE staged
//      window by the FIR of the unlimited tile (FIR = false: the sample itself), a few per thread; r[k] beside it.
//      Every k is below out_end + La, which the caller has checked against the readiness of the row
//   2. the sliding minimum over Wn = H + La + 1 values by doubling: a_s[i] = min r[i .. i + 2^s) in two LDS buffers
//      that swap, then m[j] = min(a_p[j], a_p[j + Wn - 2^p]), 2^p <= Wn < 2^(p+1).  min is exact: the bits do not
//      depend on the scheme
//   3. g[t]: La + 1 fp32 adds in ascending order from m[t - La], one division; y = v g; the epilogue of the
//      unlimited tile.  Where every m is 1.0f the sum and the quotient are exact, g = 1.0f and y is bitwise v.
//      A fade scales y, not v: the limiter sees the unfaded signal, and |y| only shrinks (the ramp is below 1)
// LDS: [input window of the row's span][v][a][b], limiter_lds_floats (kernels.h).  All loops and barriers are uniform
// over the workgroup; no thread leaves before the last barrier.
template <bool FIR, int LAW, bool FADE, bool TURN, bool ENV>
__device__ __forceinline__ void resample_pcm16_limited(float* lds, const PcmPoolRow& r, const WireSource<TURN, ENV>& in,
                                                       const PcmFade& fade, int64_t t0, int64_t n_out, int64_t limit,
                                                       typename WireSample<LAW>::type* pcm,
                                                       typename WireSample<LAW>::type* pk,
                                                       const float* __restrict__ bank, const ResampleGeom& g) {
  const int La = r.lim.lookahead, H = r.lim.hold;
  const float c = r.lim.ceiling;
  int64_t t_end = t0 + kResampleTile;
  if (t_end > r.out_end) t_end = r.out_end;
  if (t_end > n_out) t_end = n_out;
  const int cnt = (int)(t_end - t0);
  const int S = cnt + 2 * La + H;                        // v values held
  const int64_t lo = t0 - La - H;                        // output index of vs[0]
  const int span = kResampleTile + 2 * La + H;           // limiter_span: the layout does not depend on the tile
  float* vs = lds + (FIR ? (int64_t)(span - 1) * g.M / g.L + 2 + g.K : 0);
  float* a = vs + span;
  float* b = a + span;
  int64_t j0 = 0;
  if (FIR) {
    const int64_t k_lo = lo > 0 ? lo : 0;
    int64_t k_hi = lo + S - 1;
    if (k_hi > n_out - 1) k_hi = n_out - 1;
    j0 = resample_window_first(k_lo, g.L, g.M, g.left);
    in.stage(lds, j0, k_hi, g, limit);
    __syncthreads();
  }
  float p = 0.f;
  if (r.peak) p = r.peak[0];
  float top = 0.f;                                       // |v| before the gain, over this tile's own outputs
  for (int i = threadIdx.x; i < S; i += kResampleTile) {
    const int64_t k = lo + i;
    float v = 0.f;
    if (k >= 0 && k < n_out) {
      if constexpr (FIR) v = resample_output(lds, j0, k, bank, g.L, g.M, g.K, g.left, g.ratio);
      else v = in.at(k, limit);
      if (k >= t0 && k < t_end) top = fmaxf(top, fabsf(v));
      if (p > 0.01f) v = (v / p) * 0.9f;
    }
    vs[i] = v;
    const float m = fabsf(v);
    a[i] = m > c ? c / m : 1.f;
  }
  __syncthreads();
  wire_peak(r.running, top);
  const int Wn = H + La + 1;
  int w = 1;
  while (2 * w <= Wn) {
    for (int i = threadIdx.x; i < S; i += kResampleTile) b[i] = i + w < S ? fminf(a[i], a[i + w]) : a[i];
    __syncthreads();
    float* sw = a; a = b; b = sw;
    w *= 2;
  }
  const int Sm = cnt + La;                               // m[t0 - La .. t_end): b[jj] = m[t0 - La + jj]
  for (int jj = threadIdx.x; jj < Sm; jj += kResampleTile) b[jj] = fminf(a[jj], a[jj + Wn - w]);
  __syncthreads();
  const int64_t t = t0 + threadIdx.x;
  if (t >= r.out_end) return;
  float y = 0.f;
  if (t < t_end) {
    float sum = b[threadIdx.x];
    for (int i = 1; i <= La; ++i) sum += b[threadIdx.x + i];
    const float gn = sum / (float)(La + 1);
    y = vs[threadIdx.x + La + H] * gn;
  }
  wire_store<LAW, FADE>(y, t < t_end, t, fade, pcm, pk);
}

template <bool FIR, bool LIM, int LAW, bool FADE, bool TURN, bool ENV>
__device__ __forceinline__ void resample_pcm16_tile(float* xs, const PcmPoolRow& r, const WireSource<TURN, ENV>& in,
                                                    const PcmFade& fade, const float* __restrict__ bank,
                                                    const ResampleGeom& g, short* __restrict__ packed) {
  using W = typename WireSample<LAW>::type;
  W* pcm = reinterpret_cast<W*>(r.pcm);
  const int64_t t0 = r.out_first + (int64_t)blockIdx.x * kResampleTile;
  if (blockIdx.x != 0 && t0 >= r.out_end) return;         // uniform over the workgroup: a shorter range than the grid's
  const int64_t n = resample_row_valid(r.valid, 0, r.in_total);
  int64_t n_out = FIR ? (int64_t)((double)n * g.ratio) : n;
  if (n_out > r.pcm_cap) n_out = r.pcm_cap;
  if (blockIdx.x == 0 && threadIdx.x == 0 && r.out_samples) {
    int64_t keep = FIR ? (int64_t)ceil((double)n * g.ratio) : n;
    r.out_samples[0] = keep > r.pcm_cap ? r.pcm_cap : keep;
  }
  const int64_t t = t0 + threadIdx.x;
  if (t0 >= r.out_end) return;                            // the empty range (only out_samples to write)
  W* pk = (packed && r.packed_off >= 0) ? reinterpret_cast<W*>(packed) + (r.packed_off - r.out_first) : nullptr;
  if (t0 >= n_out) {                                      // uniform over the workgroup: zeros past the row's end
    if (t < r.out_end) wire_store<LAW, false>(0.f, false, t, fade, pcm, pk);
    return;
  }
  const int64_t limit = n < r.in_avail ? n : r.in_avail;
  if constexpr (LIM) {
    resample_pcm16_limited<FIR, LAW, FADE>(xs, r, in, fade, t0, n_out, limit, pcm, pk, bank, g);
    return;
  }
  int64_t j0 = 0;
  if (FIR) {
    int64_t t_last = t0 + kResampleTile - 1;
    if (t_last > n_out - 1) t_last = n_out - 1;
    if (t_last > r.out_end - 1) t_last = r.out_end - 1;
    j0 = resample_window_first(t0, g.L, g.M, g.left);
    in.stage(xs, j0, t_last, g, limit);
    __syncthreads();
  }
  float v = 0.f;
  const bool live = t < r.out_end && t < n_out;
  if (live) {
    if constexpr (FIR) v = resample_output(xs, j0, t, bank, g.L, g.M, g.K, g.left, g.ratio);
    else v = in.at(t, limit);
  }
  wire_peak(r.running, fabsf(v));
  if (t >= r.out_end) return;
  if (live && r.peak) {
    const float p = r.peak[0];
    if (p > 0.01f) v = (v / p) * 0.9f;
  }
  wire_store<LAW, FADE>(v, live, t, fade, pcm, pk);
}

// Ranged kernel (mbv_resample_pcm16_range and its forms): row blockIdx.y of [B] tensors, one range for all rows; the
// row is built in registers from the arguments.  pcm_stride counts stored samples (int16, or bytes with a codec).
// LIM = false never reads `lim`, FADE = false never reads `fade`, ENV = false never reads `env` / `env_stride` (row b's
// table starts at env.gain + b env_stride)
template <bool FIR, bool LIM, int LAW, bool FADE, bool ENV>
__global__ void __launch_bounds__(kResampleTile)
resample_pcm16_range_kernel(const float* __restrict__ x, const int64_t* __restrict__ valid, int64_t in_stride,
                            int64_t in_avail, const float* __restrict__ bank, ResampleGeom g, int64_t out_first,
                            int64_t out_end, const float* __restrict__ peak,
                            typename WireSample<LAW>::type* __restrict__ pcm, int64_t pcm_stride,
                            unsigned* __restrict__ running, int64_t* __restrict__ out_samples, LimiterParams lim,
                            PcmFade fade, PcmEnv env, int64_t env_stride) {
  extern __shared__ float xs[];
  const int b = blockIdx.y;
  const PcmPoolRow r{x + (int64_t)b * in_stride, in_stride, valid ? valid + b : nullptr, in_avail, out_first, out_end,
                     peak ? peak + b : nullptr, reinterpret_cast<short*>(pcm + (int64_t)b * pcm_stride), pcm_stride,
                     running ? running + b : nullptr, out_samples ? out_samples + b : nullptr, -1, lim, 0};
  WireSource<false, ENV> in{};
  in.xb = r.x;
  if constexpr (ENV) {
    in.env = env;
    in.env.gain += (int64_t)b * env_stride;
  }
  resample_pcm16_tile<FIR, LIM, LAW, FADE>(xs, r, in, fade, bank, g, nullptr);
}

// Pooled kernel (mbv_resample_pcm16_chunks, mbv_resample_turns and their forms): row blockIdx.y of a table, each with
// its own range (and, LIM, its own limiter); the grid holds the tiles of the longest one.  fades: null, or fades[i]
// beside rows[i].  TURN = false: envs[i] beside rows[i] (ENV; never read otherwise), `slices` / `segs` never read.
// TURN = true: the row's input is segs[first .. first + count) of slices[i], and envs[k] lies beside segs[k]
template <bool FIR, bool LIM, int LAW, bool TURN, bool ENV>
__global__ void __launch_bounds__(kResampleTile)
resample_pcm16_pool_kernel(const PcmPoolRow* __restrict__ rows, const TurnSlice* __restrict__ slices,
                           const TurnSeg* __restrict__ segs, const PcmEnv* __restrict__ envs,
                           const PcmFade* __restrict__ fades, const float* __restrict__ bank, ResampleGeom g,
                           short* __restrict__ packed) {
  extern __shared__ float xs[];
  const PcmPoolRow r = rows[blockIdx.y];
  const PcmFade fade = fades ? fades[blockIdx.y] : PcmFade{0, -1, 0.f, 0};
  WireSource<TURN, ENV> in{};
  if constexpr (TURN) {
    const TurnSlice sl = slices[blockIdx.y];
    in.src = TurnSrc{segs + sl.first, sl.count, ENV ? envs + sl.first : nullptr};
  } else {
    in.xb = r.x;
    if constexpr (ENV) in.env = envs[blockIdx.y];
  }
  resample_pcm16_tile<FIR, LIM, LAW, true>(xs, r, in, fade, bank, g, packed);
}

namespace {
// f(c) with c a std::bool_constant of `on`
template <typename F>
void with_flag(bool on, F f) {
  if (on) f(std::true_type{});
  else f(std::false_type{});
}

// f(LAW as a std::integral_constant) for the codec of a launch (the caller has refused every other value)
template <typename F>
void with_law(int law, F f) {
  if (law == kLawUlaw) f(std::integral_constant<int, kLawUlaw>{});
  else if (law == kLawAlaw) f(std::integral_constant<int, kLawAlaw>{});
  else f(std::integral_constant<int, kLawNone>{});
}

// What the two wire launchers share.  f(FIR, LIM, LAW, X, ENV as constants, grid, lds bytes, geometry) for a launch of
// `rows` rows whose longest range has max_count outputs; X is FADE for the ranged kernel and TURN for the pooled one.
// FIR = bank given, else equal rates with the geometry of the sample itself.  LDS: lim_floats (limiter_lds_floats) for
// a limited launch, else the staged window of the FIR.  The shaped instantiation runs only where an envelope is given
template <typename F>
void wire_launch(const float* bank, const ResampleGeom& g, bool limited, int64_t lim_floats, int law, bool x,
                 bool shaped, int64_t max_count, int rows, F f) {
  int64_t bx = (max_count + kResampleTile - 1) / kResampleTile;
  if (bx < 1) bx = 1;                                     // an empty range still writes out_samples
  const dim3 grid((unsigned)bx, rows);
  const size_t lds = (size_t)(limited ? lim_floats : bank ? resample_lds_floats(g) : 0) * sizeof(float);
  const ResampleGeom gk = bank ? g : ResampleGeom{1, 1, 0, 0, 1.0};
  with_flag(bank != nullptr, [&](auto fir) {
    with_flag(limited, [&](auto lim) {
      with_law(law, [&](auto lc) {
        with_flag(x, [&](auto xc) { with_flag(shaped, [&](auto ec) { f(fir, lim, lc, xc, ec, grid, lds, gk); }); });
      });
    });
  });
}
}  // namespace

void launch_resample_pcm16_range(const float* x, const int64_t* valid, int B, int64_t in_stride, int64_t in_avail,
                                 const float* bank, const ResampleGeom& g, int64_t out_first, int64_t out_count,
                                 const float* peak, void* pcm, int64_t pcm_stride, unsigned* running,
                                 int64_t* out_samples, const LimiterParams* lim, int law, const PcmFade& fade,
                                 const PcmEnv& env, int64_t env_stride, hipStream_t s) {
  const LimiterParams lp = lim ? *lim : LimiterParams{};
  wire_launch(bank, g, lim != nullptr, lim ? limiter_lds_floats(g, bank != nullptr, lp) : 0, law, fade.count >= 0,
              env.gain != nullptr, out_count, B,
              [&](auto fir, auto lc_lim, auto lc, auto fc, auto ec, dim3 grid, size_t lds, const ResampleGeom& gk) {
                constexpr int LAW = decltype(lc)::value;
                hipLaunchKernelGGL((resample_pcm16_range_kernel<decltype(fir)::value, decltype(lc_lim)::value, LAW,
                                                                decltype(fc)::value, decltype(ec)::value>),
                                   grid, dim3(kResampleTile), lds, s, x, valid, in_stride, in_avail, bank, gk, out_first,
                                   out_first + out_count, peak, static_cast<typename WireSample<LAW>::type*>(pcm),
                                   pcm_stride, running, out_samples, lp, fade, env, env_stride);
              });
}

void launch_resample_pcm16_pool(const PcmPoolLaunch& a, const float* bank, const ResampleGeom& g, hipStream_t s) {
  wire_launch(bank, g, a.limited, a.lds_floats, a.law, a.slices != nullptr, a.envs != nullptr, a.max_count, a.n,
              [&](auto fir, auto lim, auto lc, auto tc, auto ec, dim3 grid, size_t lds, const ResampleGeom& gk) {
                hipLaunchKernelGGL((resample_pcm16_pool_kernel<decltype(fir)::value, decltype(lim)::value,
                                                               decltype(lc)::value, decltype(tc)::value,
                                                               decltype(ec)::value>),
                                   grid, dim3(kResampleTile), lds, s, a.rows, a.slices, a.segs, a.envs, a.fades, bank, gk,
                                   static_cast<short*>(a.packed));   // the tile reads it as the codec's sample type
              });
}

// Stand-alone codec (mbv_g711_encode / mbv_g711_decode): one sample per thread
template <int LAW>
__global__ void __launch_bounds__(256) g711_encode_kernel(const short* __restrict__ pcm, int64_t n,
                                                          uint8_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = g711_encode<LAW>(pcm[i]);
}

template <int LAW>
__global__ void __launch_bounds__(256) g711_decode_kernel(const uint8_t* __restrict__ in, int64_t n,
                                                          short* __restrict__ pcm) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) pcm[i] = g711_decode<LAW>(in[i]);
}

void launch_g711_encode(const short* pcm, int64_t n, int law, uint8_t* out, hipStream_t s) {
  const dim3 grid((unsigned)((n + 255) / 256)), block(256);
  if (law == kLawUlaw) hipLaunchKernelGGL(g711_encode_kernel<kLawUlaw>, grid, block, 0, s, pcm, n, out);
  else hipLaunchKernelGGL(g711_encode_kernel<kLawAlaw>, grid, block, 0, s, pcm, n, out);
}

void launch_g711_decode(const uint8_t* in, int64_t n, int law, short* pcm, hipStream_t s) {
  const dim3 grid((unsigned)((n + 255) / 256)), block(256);
  if (law == kLawUlaw) hipLaunchKernelGGL(g711_decode_kernel<kLawUlaw>, grid, block, 0, s, in, n, pcm);
  else hipLaunchKernelGGL(g711_decode_kernel<kLawAlaw>, grid, block, 0, s, in, n, pcm);
}

}  // namespace mbv
