// Small memory-bound pieces of the path: embedding, channel LayerNorm,
// durations (proj + exp/ceil/cumsum), per-token prosody (scale / extra frames / fit-to-length on those durations),
// length regulation, speaker conditioning.
#include "kernels.h"

namespace mbv {

// ---------------------------------------------------------------------------
// x[b, c, t] = emb[ids[b,t]][c] * sqrt(H) * (t < len[b])       models.py:173-177
// Also narrows the int64 lengths to the int32 copy the other kernels use.
// ---------------------------------------------------------------------------
__global__ void embed_kernel(const int64_t* ids, const int64_t* lens, const float* emb, float* x,
                             int* lens32, int* bad, int B, int T, int H, int n_vocab, float scale) {
  const int b = blockIdx.z;
  const int c = blockIdx.y;
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t == 0 && c == 0) {
    const long long l = lens[b];
    lens32[b] = l < 0 ? 0 : (l > T ? T : (int)l);
    if (l < 0 || l > T) bad[b] = 1;               // x_lengths outside [0, T]
  }
  if (t >= T) return;
  const int len = (int)lens[b];
  long long id = ids[(int64_t)b * T + t];
  if (id < 0 || id >= n_vocab) {                    // nn.Embedding would raise IndexError: report it
    if (c == 0) bad[b] = 1;                         // (mbv_encode returns y_lengths = -1 for the utterance)
    id = 0;
  }
  float v = emb[id * H + c] * scale;
  x[((int64_t)b * H + c) * T + t] = t < len ? v : 0.f;
}

void launch_embed(const int64_t* ids, const int64_t* lens, const float* emb, float* x, int* lens32,
                  int* bad, int B, int T, int H, int n_vocab, hipStream_t s) {
  (void)hipMemsetAsync(bad, 0, (size_t)B * sizeof(int), s);
  dim3 grid((T + 63) / 64, H, B);
  hipLaunchKernelGGL(embed_kernel, grid, dim3(64), 0, s, ids, lens, emb, x, lens32, bad, B, T, H, n_vocab,
                     sqrtf((float)H));
}

// ---------------------------------------------------------------------------
// Split-bf16 copy of the packed conv weights (opt-in conv_bf16 mode, conv1d.hip): every 16-byte slot of
// four fp32 K-values becomes [bf16 hi x 4 | bf16 mid x 4], hi = bf16(x), mid = bf16(x - hi) — the layout
// the conv kernel also gives its input window in that mode, so an MFMA operand is two slots' halves.
// ---------------------------------------------------------------------------
typedef __bf16 bf16x4_t __attribute__((ext_vector_type(4)));
__global__ __launch_bounds__(256) void split_planes_kernel(const float4* src, float4* dst, size_t n4) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
    const float4 v = src[i];
    const float x[4] = {v.x, v.y, v.z, v.w};
    bf16x4_t hi, mid;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const __bf16 h = (__bf16)x[k];
      hi[k] = h;
      mid[k] = (__bf16)(x[k] - (float)h);
    }
    struct { bf16x4_t h, m; } o{hi, mid};
    dst[i] = __builtin_bit_cast(float4, o);
  }
}
void launch_split_planes(const float* src, float* dst, size_t n_floats, hipStream_t s) {
  const size_t n4 = n_floats / 4;
  const int grid = (int)(n4 / 256 + 1 < 2048 ? n4 / 256 + 1 : 2048);
  hipLaunchKernelGGL(split_planes_kernel, dim3(grid), dim3(256), 0, s, reinterpret_cast<const float4*>(src),
                     reinterpret_cast<float4*>(dst), n4);
}

// ---------------------------------------------------------------------------
// Channel LayerNorm (modules.py:29-32), eps 1e-5, two-pass statistics like
// F.layer_norm.  Fused: residual add (attentions.py:41,45), ReLU in front
// (models.py:129-130), mask behind (attentions.py:46).
// Block = 32 time steps x 8 channel groups; each thread keeps its <= 32
// channel values in registers, the 8 partials are reduced through LDS.
// ---------------------------------------------------------------------------
constexpr int LN_TX = 32, LN_CY = 8, LN_MAXPER = 32;   // C <= 256 (H and the dp filter width)

__global__ __launch_bounds__(256) void layernorm_kernel(const float* a, const float* r,
                                                        const float* gamma, const float* beta,
                                                        float* y, int C, int T, int pre_relu,
                                                        const int* out_lens) {
  __shared__ float red[LN_CY][LN_TX];
  const int tx = threadIdx.x & 31, cy = threadIdx.x >> 5;
  const int b = blockIdx.y;
  const int t = blockIdx.x * LN_TX + tx;
  const bool ok = t < T;
  const int64_t base = (int64_t)b * C * T + t;
  float v[LN_MAXPER];
  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < LN_MAXPER; ++i) {
    const int c = cy + i * LN_CY;
    float x = 0.f;
    if (ok && c < C) {
      x = a[base + (int64_t)c * T];
      if (r) x += r[base + (int64_t)c * T];
      if (pre_relu) x = fmaxf(x, 0.f);
    }
    v[i] = x;
    sum += x;
  }
  red[cy][tx] = sum;
  __syncthreads();
  float mean = 0.f;
#pragma unroll
  for (int k = 0; k < LN_CY; ++k) mean += red[k][tx];
  mean /= (float)C;
  __syncthreads();
  float sq = 0.f;
#pragma unroll
  for (int i = 0; i < LN_MAXPER; ++i) {
    const int c = cy + i * LN_CY;
    if (c < C) { const float d = v[i] - mean; sq += d * d; }
  }
  red[cy][tx] = sq;
  __syncthreads();
  float var = 0.f;
#pragma unroll
  for (int k = 0; k < LN_CY; ++k) var += red[k][tx];
  const float rstd = rsqrtf(var / (float)C + 1e-5f);
  const float m = (out_lens && t >= out_lens[b]) ? 0.f : 1.f;
  if (!ok) return;
#pragma unroll
  for (int i = 0; i < LN_MAXPER; ++i) {
    const int c = cy + i * LN_CY;
    if (c < C) y[base + (int64_t)c * T] = ((v[i] - mean) * rstd * gamma[c] + beta[c]) * m;
  }
}

void launch_layernorm(const float* a, const float* r, const float* gamma, const float* beta,
                      float* y, int B, int C, int T, int pre_relu, const int* out_lens,
                      hipStream_t s) {
  dim3 grid((T + LN_TX - 1) / LN_TX, B);
  hipLaunchKernelGGL(layernorm_kernel, grid, dim3(256), 0, s, a, r, gamma, beta, y, C, T, pre_relu,
                     out_lens);
}

// ---------------------------------------------------------------------------
// Durations: dp.proj (C -> 1, models.py:136-137) fused with models.py:717-719:
//   logw = (w . (h * mask) + b) * mask ; w = exp(logw) * mask * length_scale
//   w_ceil = ceil(w) ; cum = inclusive cumsum ; y_len = max(sum, 1)
// One block per utterance; T is scanned in chunks of 256.
// Supported range: every token below 2^20 frames, every utterance at most 2^30 (the int32 sums cannot wrap:
// a chunk adds < 2^28 to a carry that stops at 2^30).  A duration at or beyond that, or not a number, counts 0
// frames and flags the utterance like an invalid token id: y_len = 1, y_lengths = -1; w_ceil keeps its value.
// ---------------------------------------------------------------------------
constexpr float kMaxTokenFrames = 1048576.f;     // 2^20
constexpr int kMaxTotalFrames = 1 << 30;
// ROWS: length_scale = rows[b].length_scale (pooled admission, kernels.h); else the call's scalar
template <bool ROWS>
__global__ __launch_bounds__(256) void durations_kernel(const float* h, const float* w,
                                                        const float* bias, const int* lens,
                                                        float length_scale, const AdmitEncRow* rows, float* logw,
                                                        float* w_ceil, int* cum, int* ylen32,
                                                        int64_t* ylen64, const int* bad, int C, int T) {
  __shared__ int scan[256];
  __shared__ int carry_s, over_s;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int len = lens[b];
  if (ROWS) length_scale = rows[b].length_scale;
  if (tid == 0) { carry_s = 0; over_s = 0; }
  __syncthreads();
  for (int t0 = 0; t0 < T; t0 += 256) {
    const int t = t0 + tid;
    int d = 0;
    if (t < T) {
      float lw = 0.f, wc = 0.f;
      if (t < len) {
        if (w) {
          // four interleaved partial sums: one dependent fmaf chain over 256 channels behind 256 loads was
          // 63 us per launch, as long as a text-encoder conv
          float acc4[4] = {0.f, 0.f, 0.f, 0.f};
          const float* hp = h + (int64_t)b * C * T + t;
          int c = 0;
          for (; c + 8 <= C; c += 8) {
            float hv[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) hv[q] = hp[(int64_t)(c + q) * T];
#pragma unroll
            for (int q = 0; q < 8; ++q) acc4[q & 3] = fmaf(w[c + q], hv[q], acc4[q & 3]);
          }
          for (; c < C; ++c) acc4[c & 3] = fmaf(w[c], hp[(int64_t)c * T], acc4[c & 3]);
          lw = ((acc4[0] + acc4[1]) + (acc4[2] + acc4[3])) + bias[0];
        } else {
          lw = h[(int64_t)b * T + t];            // SDP: logw computed by the flows (sdp.hip)
        }
        wc = ceilf(expf(lw) * length_scale);
      }
      logw[(int64_t)b * T + t] = lw;
      w_ceil[(int64_t)b * T + t] = wc;
      if (wc < kMaxTokenFrames) d = (int)wc;
      else over_s = 1;                                  // too long, inf or NaN (every writer stores the same 1)
    }
    scan[tid] = d;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {          // Hillis-Steele inclusive scan
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
      if (c > kMaxTotalFrames) { over_s = 1; c = kMaxTotalFrames; }
      carry_s = c;
    }
    __syncthreads();
  }
  if (tid == 0) {
    const int total = (carry_s < 1 || over_s) ? 1 : carry_s;
    ylen32[b] = total;
    if (ylen64) ylen64[b] = ((bad && bad[b]) || over_s) ? -1 : total;     // -1: invalid token id / length / sid / duration
  }
}

void launch_durations(const float* h, const float* w, const float* b, const int* lens,
                      float length_scale, float* logw, float* w_ceil, int* cum, int* ylen32,
                      int64_t* ylen64, const int* bad, int B, int C, int T, hipStream_t s) {
  hipLaunchKernelGGL(durations_kernel<false>, dim3(B), dim3(256), 0, s, h, w, b, lens, length_scale, nullptr, logw,
                     w_ceil, cum, ylen32, ylen64, bad, C, T);
}

void launch_durations_rows(const float* h, const float* w, const float* b, const int* lens, const AdmitEncRow* rows,
                           float* logw, float* w_ceil, int* cum, int* ylen32, int64_t* ylen64, const int* bad, int B,
                           int C, int T, hipStream_t s) {
  hipLaunchKernelGGL(durations_kernel<true>, dim3(B), dim3(256), 0, s, h, w, b, lens, 0.f, rows, logw, w_ceil, cum,
                     ylen32, ylen64, bad, C, T);
}

// ---------------------------------------------------------------------------
// Per-token prosody (mbv_shape_durations / mbv_shape_durations_rows / mbv_op_shape_durations): the durations of
// durations_kernel again, from the logw it left, with a scale PER TOKEN, extra frames per token and, for rows that
// ask for it, one global factor f that makes the row fit a frame count:
//   w_t = ceilf(expf(logw_t) * fl32(s_t * f)) + extra_t         (two separate fp32 multiplications, then the ceil)
//   D(f) = sum over t < len of w_t;  f = the largest fp32 in [lo, hi] with D(f) <= frames
// D is non-decreasing in f (every step is monotone in fp32) and positive floats order like their bit patterns, so
// the search is a bisection on the bit pattern: D(hi) first, then at most 31 halvings of [bits(lo) - 1, bits(hi)],
// where bits(lo) - 1 stands for "not even lo fits" (status 1, f = lo).  During the search a token counts
// min(frames, 2^20) and the sums are 64-bit; the final pass applies the range rules of durations_kernel to the
// token's total (a negative, infinite or NaN scale and a negative extra flag the row as well) and writes w_ceil
// (fp32 totals, extras included), cum (chunked scan with carry), ylen32 and ylen64.
// One block per row.  expf(logw_t) and s_t of the first kShapeReg * 256 tokens stay in registers across the
// evaluations; a longer text recomputes the rest from memory.
// ROWS: block i works on row rows[i].row of the run with that row's own [t_text] tensors; rows without controls are
// not in the table.  Else block b is row b, scale / extra are [B, T], and `rows` (or null: no row fits) holds the
// fit parameters of row b.
// ---------------------------------------------------------------------------
constexpr int kShapeReg = 8;

__device__ __forceinline__ long long shape_block_sum(long long v, long long* red) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  __syncthreads();                                     // (red is free again: everyone read the last result)
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}

__device__ __forceinline__ long long shape_count(float e, float s, float f, int extra) {
  const float wc = ceilf(e * (s * f));
  long long d = wc < kMaxTokenFrames ? (wc > 0.f ? (long long)wc : 0) : (long long)kMaxTokenFrames;   // (NaN: 2^20)
  return d + (extra > 0 ? extra : 0);
}

template <bool ROWS>
__global__ __launch_bounds__(256) void shape_durations_kernel(const float* __restrict__ logw, const int* __restrict__ lens,
                                                              const float* scale, const int* extra, float scalar,
                                                              const ShapeRow* __restrict__ rows, float* w_ceil, int* cum,
                                                              int* ylen32, int64_t* ylen64, const int* bad,
                                                              float* fit_stage, FitOut* fit_out, int T) {
  __shared__ int scan[256];
  __shared__ long long red[4];
  __shared__ int carry_s, over_s;
  const int tid = threadIdx.x;
  int b = blockIdx.x;
  int len;
  long long frames = 0;
  float lo = 1.f, hi = 1.f;
  if (ROWS) {
    const ShapeRow r = rows[blockIdx.x];
    b = r.row;
    len = lens[b] < r.t_text ? lens[b] : r.t_text;      // never read past the row's own tensors
    scale = r.scale; extra = r.extra; scalar = r.scalar;
    frames = r.frames; lo = r.lo; hi = r.hi;
    fit_out = r.fit_out;
  } else {
    len = lens[b];
    if (scale) scale += (int64_t)b * T;
    if (extra) extra += (int64_t)b * T;
    if (rows) { frames = rows[b].frames; lo = rows[b].lo; hi = rows[b].hi; }
    if (fit_out) fit_out += b;
  }
  const float* lw = logw + (int64_t)b * T;
  float e_r[kShapeReg], s_r[kShapeReg];
  int x_r[kShapeReg];
#pragma unroll
  for (int k = 0; k < kShapeReg; ++k) {
    const int t = k * 256 + tid;
    e_r[k] = 0.f; s_r[k] = 0.f; x_r[k] = 0;
    if (t < len) {
      e_r[k] = expf(lw[t]);
      s_r[k] = scale ? scale[t] : scalar;
      x_r[k] = extra ? extra[t] : 0;
    }
  }
  float f = 1.f;
  int status = 0;
  if (frames > 0) {
    auto D = [&](float ff) {
      long long v = 0;
#pragma unroll
      for (int k = 0; k < kShapeReg; ++k)
        if (k * 256 + tid < len) v += shape_count(e_r[k], s_r[k], ff, x_r[k]);
      for (int t = kShapeReg * 256 + tid; t < len; t += 256)
        v += shape_count(expf(lw[t]), scale ? scale[t] : scalar, ff, extra ? extra[t] : 0);
      return shape_block_sum(v, red);
    };
    f = hi;
    if (D(hi) > frames) {
      unsigned a = __float_as_uint(lo) - 1u, z = __float_as_uint(hi);      // D(a) fits (a < bits(lo): by decree), D(z) does not
      while (z - a > 1u) {
        const unsigned mid = a + (z - a) / 2u;
        if (D(__uint_as_float(mid)) <= frames) a = mid; else z = mid;     // (uniform over the block)
      }
      if (a < __float_as_uint(lo)) { f = lo; status = 1; }
      else f = __uint_as_float(a);
    }
  }
  if (tid == 0) { carry_s = 0; over_s = 0; }
  __syncthreads();
  for (int t0 = 0; t0 < T; t0 += 256) {
    const int t = t0 + tid;
    int d = 0;
    if (t < T) {
      float wt = 0.f;
      if (t < len) {
        float e = 0.f, s = 0.f;
        int x = 0;
        bool reg = false;
#pragma unroll
        for (int k = 0; k < kShapeReg; ++k)
          if (t0 == k * 256) { e = e_r[k]; s = s_r[k]; x = x_r[k]; reg = true; }
        if (!reg) { e = expf(lw[t]); s = scale ? scale[t] : scalar; x = extra ? extra[t] : 0; }
        const float sf = frames > 0 ? s * f : s;
        const float wc = ceilf(e * sf);
        wt = wc + (float)x;
        // the scale itself must be a finite number >= 0, the extra >= 0, and the token's total in range
        if (s >= 0.f && s < INFINITY && x >= 0 && wc < kMaxTokenFrames && wt < kMaxTokenFrames) d = (int)wc + x;
        else over_s = 1;
      }
      w_ceil[(int64_t)b * T + t] = wt;
    }
    scan[tid] = d;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {          // Hillis-Steele inclusive scan
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
      if (c > kMaxTotalFrames) { over_s = 1; c = kMaxTotalFrames; }
      carry_s = c;
    }
    __syncthreads();
  }
  if (tid == 0) {
    const int total = (carry_s < 1 || over_s) ? 1 : carry_s;
    ylen32[b] = total;
    if (ylen64) ylen64[b] = ((bad && bad[b]) || over_s) ? -1 : total;
    if (fit_stage) { fit_stage[b] = f; fit_stage[gridDim.x + b] = (float)status; }
    if (fit_out) { fit_out->scale = f; fit_out->status = status; }
  }
}

void launch_shape_durations(const float* logw, const int* lens, const float* scale, const int* extra, float scalar,
                            const ShapeRow* fit, float* w_ceil, int* cum, int* ylen32, int64_t* ylen64, const int* bad,
                            float* fit_stage, FitOut* fit_out, int B, int T, hipStream_t s) {
  hipLaunchKernelGGL(shape_durations_kernel<false>, dim3(B), dim3(256), 0, s, logw, lens, scale, extra, scalar, fit,
                     w_ceil, cum, ylen32, ylen64, bad, fit_stage, fit_out, T);
}

void launch_shape_durations_rows(const float* logw, const int* lens, const ShapeRow* rows, int n, float* w_ceil,
                                 int* cum, int* ylen32, int64_t* ylen64, const int* bad, int T, hipStream_t s) {
  hipLaunchKernelGGL(shape_durations_kernel<true>, dim3(n), dim3(256), 0, s, logw, lens, nullptr, nullptr, 1.f, rows,
                     w_ceil, cum, ylen32, ylen64, bad, nullptr, nullptr, T);
}

// Token marks (mbv_token_marks / mbv_token_marks_rows): the EXCLUSIVE prefix sums of the durations the length regulator
// uses, as int64 next to y_lengths in the caller's read-back buffer.  `cum` is the inclusive scan the kernels above
// (or launch_set_durations) left, so this is a shifted copy: dst[0] = 0, dst[j] = cum[b, j - 1].  Row b of the grid
// writes `count` entries to dst + b stride, or, with a table, rows[b].count entries to rows[b].dst (null: none).
__global__ __launch_bounds__(256) void token_marks_kernel(const int* __restrict__ cum, int T, int64_t* dst,
                                                          int64_t stride, int count, const MarkRow* __restrict__ rows) {
  const int b = blockIdx.y;
  const int j = blockIdx.x * 256 + threadIdx.x;
  int64_t* d = rows ? rows[b].dst : dst + (int64_t)b * stride;
  const int n = rows ? rows[b].count : count;
  if (!d || j >= n || j > T) return;
  d[j] = j ? (int64_t)cum[(int64_t)b * T + j - 1] : 0;
}

void launch_token_marks(const int* cum, int B, int T, int64_t* dst, int64_t stride, int count, const MarkRow* rows,
                        hipStream_t s) {
  hipLaunchKernelGGL(token_marks_kernel, dim3((unsigned)(T / 256 + 1), B), dim3(256), 0, s, cum, T, dst, stride, count,
                     rows);
}

// Chunk seams of a bounded look-ahead (mbv_seam_rows): row = blockIdx.y of the table, sample i of its seam.
// The blend is written with __fmul_rn / __fadd_rn so that no product is contracted into the sum: a restatement in fp32
// on the host is bitwise.  Thread i reads stash[i] before it writes it, and a row's head and overhang never overlap.
__global__ __launch_bounds__(256) void seam_rows_kernel(const SeamRow* __restrict__ rows) {
  const SeamRow r = rows[blockIdx.y];
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < r.head_count) {
    const float w_p = __fmul_rn((float)(r.seam - i), r.inv), w_q = __fmul_rn((float)(i + 1), r.inv);
    r.head[i] = __fadd_rn(__fmul_rn(r.stash[i], w_p), __fmul_rn(r.head[i], w_q));
  }
  if (i < r.over_count) r.stash[i] = r.over[i];
}

void launch_seam_rows(const SeamRow* rows, int n, int max_seam, hipStream_t s) {
  hipLaunchKernelGGL(seam_rows_kernel, dim3((unsigned)((max_seam + 255) / 256), n), dim3(256), 0, s, rows);
}

// Frame gains (mbv_frame_gain / mbv_frame_gain_rows / mbv_op_frame_gain, kernels.h): out[t] = gain[j(t)], j(t) the
// token expand_kernel gives frame t (the same search over the same scan), held behind the row's kept frames; all 1.0f
// for a flagged or empty row.  One thread per entry of [0, frames]; only loads and one store, so a copy.
template <bool ROWS>
__global__ __launch_bounds__(256) void frame_gain_kernel(const int* __restrict__ cum, const int* __restrict__ ylen32,
                                                         const int64_t* __restrict__ ylen64, const float* gain,
                                                         float* out, int64_t out_stride, int frames,
                                                         const GainRow* __restrict__ rows, int T) {
  int b = blockIdx.y;
  int n_tok = T;
  if (ROWS) {
    const GainRow r = rows[blockIdx.y];
    b = r.row;
    gain = r.gain; out = r.out; frames = r.frames;
    n_tok = r.t_text < T ? r.t_text : T;                  // never read past the row's own gain tensor
  } else {
    gain += (int64_t)b * T;
    out += (int64_t)b * out_stride;
  }
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t > frames) return;
  int64_t y = ylen64 ? ylen64[b] : (int64_t)ylen32[b];
  if (y > frames) y = frames;
  float g = 1.f;
  if (y > 0 && n_tok > 0) {
    const int tt = t < y ? t : (int)y - 1;
    const int* cb = cum + (int64_t)b * T;
    int lo = 0, hi = n_tok - 1;                           // first j with cum[j] > tt
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (cb[mid] > tt) hi = mid; else lo = mid + 1;
    }
    if (cb[lo] > tt) g = gain[lo];                        // else: all-zero durations, no token holds the frame
  }
  out[t] = g;
}

void launch_frame_gain(const int* cum, const int* ylen32, const int64_t* ylen64, const float* gain, float* out,
                       int64_t out_stride, int frames, int B, int T, hipStream_t s) {
  hipLaunchKernelGGL(frame_gain_kernel<false>, dim3((unsigned)(frames / 256 + 1), B), dim3(256), 0, s, cum, ylen32,
                     ylen64, gain, out, out_stride, frames, nullptr, T);
}

void launch_frame_gain_rows(const int* cum, const int* ylen32, const GainRow* rows, int n, int max_frames, int T,
                            hipStream_t s) {
  hipLaunchKernelGGL(frame_gain_kernel<true>, dim3((unsigned)(max_frames / 256 + 1), n), dim3(256), 0, s, cum, ylen32,
                     nullptr, nullptr, nullptr, 0, 0, rows, T);
}

// ---------------------------------------------------------------------------
// Length regulation (models.py:720-729, commons.py:128-143).  The reference
// builds a one-hot path [B,1,T',T] and matmuls; it is a gather: frame t' takes
// token j = first index with cum[j] > t'.  Writes m_p, logs_p, z_p (= m_p +
// noise * exp(logs_p) * noise_scale), z (copy of z_p: the flows run in place),
// and optionally the dense attn path and y_mask.
// ---------------------------------------------------------------------------
// ROWS (pooled admission, kernels.h): row b takes noise_scale and its noise block [C, noise_stride] from rows[b];
// frames at and past noise_stride (behind the row's own T') read no noise — they are masked to 0 in z
template <bool ROWS>
__global__ __launch_bounds__(256) void expand_kernel(const float* m_t, const float* logs_t,
                                                     int64_t src_bstride, const int* cum,
                                                     const int* ylen,
                                                     const float* noise, float noise_scale, const AdmitSynRow* rows,
                                                     float* m_p, float* logs_p, float* z_p, float* z,
                                                     float* y_mask, int C, int T, int Tp) {
  const int b = blockIdx.y;
  const int tp = blockIdx.x * blockDim.x + threadIdx.x;
  if (tp >= Tp) return;
  const int yl = ylen[b];
  int64_t n_stride = Tp;
  if (ROWS) {
    const AdmitSynRow r = rows[b];
    noise_scale = r.noise_scale;
    n_stride = r.noise_stride;
    noise = (noise_scale != 0.f && tp < n_stride) ? r.noise : nullptr;
  }
  const int* cb = cum + (int64_t)b * T;
  int j = -1;
  if (tp < yl) {
    int lo = 0, hi = T - 1;                  // first j with cum[j] > tp
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (cb[mid] > tp) hi = mid; else lo = mid + 1;
    }
    j = cb[lo] > tp ? lo : -1;               // -1: all-zero durations (y_len clamped to 1)
  }
  if (y_mask && blockIdx.z == 0) y_mask[(int64_t)b * Tp + tp] = tp < yl ? 1.f : 0.f;
  const int c_lo = blockIdx.z * 16, c_hi = c_lo + 16 < C ? c_lo + 16 : C;   // 16 channels per block
  for (int c = c_lo; c < c_hi; ++c) {
    const int64_t o = ((int64_t)b * C + c) * Tp + tp;
    float m = 0.f, lg = 0.f;
    if (j >= 0) {
      m = m_t[(int64_t)b * src_bstride + (int64_t)c * T + j];
      lg = logs_t[(int64_t)b * src_bstride + (int64_t)c * T + j];
    }
    float zp = m;
    if (noise) zp = m + noise[ROWS ? (int64_t)c * n_stride + tp : o] * expf(lg) * noise_scale;
    if (m_p) m_p[o] = m;
    if (logs_p) logs_p[o] = lg;
    if (z_p) z_p[o] = zp;
    z[o] = tp < yl ? zp : 0.f;       // z enters the flows masked (the reference masks it in the first coupling that updates a half;
                                     // the fused WN layers only touch valid frames, wn_fused.hip); z_p keeps the reference's unmasked draw
  }
}

__global__ void attn_path_kernel(const int* cum, const int* ylen, float* attn, int T, int Tp) {
  // attn[b, 0, tp, t] = 1 iff cum[t-1] <= tp < cum[t] and tp < y_len
  const int b = blockIdx.z, tp = blockIdx.y;
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= T) return;
  const int* cb = cum + (int64_t)b * T;
  const int hi = cb[t], lo = t > 0 ? cb[t - 1] : 0;
  attn[((int64_t)b * Tp + tp) * T + t] = (tp < ylen[b] && tp >= lo && tp < hi) ? 1.f : 0.f;
}

void launch_expand(const float* m_t, const float* logs_t, int64_t src_bstride, const int* cum,
                   const int* ylen, const float* noise, float noise_scale, float* m_p,
                   float* logs_p, float* z_p, float* z, float* attn, float* y_mask, int B, int C,
                   int T, int Tp, hipStream_t s) {
  dim3 grid((Tp + 255) / 256, B, (C + 15) / 16);
  hipLaunchKernelGGL(expand_kernel<false>, grid, dim3(256), 0, s, m_t, logs_t, src_bstride, cum, ylen, noise,
                     noise_scale, nullptr, m_p, logs_p, z_p, z, y_mask, C, T, Tp);
  if (attn) {
    dim3 g2((T + 255) / 256, Tp, B);
    hipLaunchKernelGGL(attn_path_kernel, g2, dim3(256), 0, s, cum, ylen, attn, T, Tp);
  }
}

void launch_expand_rows(const float* m_t, const float* logs_t, int64_t src_bstride, const int* cum, const int* ylen,
                        const AdmitSynRow* rows, float* z, int B, int C, int T, int Tp, hipStream_t s) {
  dim3 grid((Tp + 255) / 256, B, (C + 15) / 16);
  hipLaunchKernelGGL(expand_kernel<true>, grid, dim3(256), 0, s, m_t, logs_t, src_bstride, cum, ylen, nullptr, 0.f,
                     rows, nullptr, nullptr, nullptr, z, nullptr, C, T, Tp);
}

// Pooled admission: what N `(z * y_mask)[:, :, :keep].contiguous()` chains of one-utterance calls do, for the rows of
// one padded run, each into its request's own tensor.
__global__ void scatter_z_rows_kernel(const float* z, const int* ylen, const AdmitSynRow* rows, int C, int Tp) {
  const int b = blockIdx.z, c = blockIdx.y;
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const AdmitSynRow r = rows[b];
  if (t >= r.keep) return;
  const int64_t zs = r.z_stride ? r.z_stride : r.keep;
  const int ts = r.src_off + t;                       // (src_off + keep <= Tp: the host checks it)
  r.z[(int64_t)c * zs + t] = z[((int64_t)b * C + c) * Tp + ts] * (ts < ylen[b] ? 1.f : 0.f);
}

void launch_scatter_z_rows(const float* z, const int* ylen, const AdmitSynRow* rows, int B, int C, int Tp, int max_keep,
                           hipStream_t s) {
  hipLaunchKernelGGL(scatter_z_rows_kernel, dim3((max_keep + 255) / 256, C, B), dim3(256), 0, s, z, ylen, rows, C, Tp);
}

// ---------------------------------------------------------------------------
// Live text (kernels.h).  Block (x, c, row): 256 token columns of channel row c of the run's stats
// [B, C2, T] (c < C2), or of its w_ceil (c == C2), into the stream's tables.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void take_tokens_rows_kernel(const float* __restrict__ stats,
                                                               const float* __restrict__ w_ceil,
                                                               const TakeRow* __restrict__ rows, int C2, int T) {
  const TakeRow r = rows[blockIdx.z];
  const int j = r.a + blockIdx.x * 256 + threadIdx.x;
  if (j >= r.b) return;
  const int c = blockIdx.y;
  if (c < C2) {
    r.stats[(int64_t)c * r.stride + j] = stats[((int64_t)r.src * C2 + c) * T + j];
    return;
  }
  const int d = *r.y_length < 0 ? -1 : (int)w_ceil[(int64_t)r.src * T + j];
  r.dur[j] = d;
  if (r.dur_copy) r.dur_copy[j - r.a] = d;
}

void launch_take_tokens_rows(const float* stats, const float* w_ceil, const TakeRow* rows, int n, int C2, int T,
                             int max_cols, hipStream_t s) {
  hipLaunchKernelGGL(take_tokens_rows_kernel, dim3((unsigned)((max_cols + 255) / 256), C2 + 1, n), dim3(256), 0, s,
                     stats, w_ceil, rows, C2, T);
}

// Block (x, row, z): frames [256 x, 256 x + 256) of the row's block, 16 channels.  Every round scans 256 durations
// (the scan of shape_durations_kernel) and the thread whose frame falls into the round takes its token from it: the
// first j with cum[j] > t, what expand_kernel's search over the whole scan gives.  All threads of a block stay in the
// loop (its barriers); the host has made sure that frame + frames lies inside z_p and the noise.
__global__ __launch_bounds__(256) void expand_ranges_kernel(const ExpandRange* __restrict__ rows, int C) {
  __shared__ int scan[256];
  __shared__ int carry_s;
  const ExpandRange r = rows[blockIdx.y];
  const int tid = threadIdx.x;
  if ((int)(blockIdx.x * 256) >= r.frames) return;          // (the whole block: no barrier is left waiting)
  const int t = blockIdx.x * 256 + tid;
  if (tid == 0) carry_s = 0;
  __syncthreads();
  int j = -1;
  for (int base = r.a; base < r.b; base += 256) {
    const int tok = base + tid;
    int d = tok < r.b ? r.dur[tok] : 0;
    scan[tid] = d > 0 ? d : 0;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {                // Hillis-Steele inclusive scan
      const int v = tid >= off ? scan[tid - off] : 0;
      __syncthreads();
      scan[tid] += v;
      __syncthreads();
    }
    const int carry = carry_s;
    if (j < 0 && t >= carry && t < carry + scan[255]) {
      int lo = 0, hi = 255;                                  // first k with carry + scan[k] > t
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (carry + scan[mid] > t) hi = mid; else lo = mid + 1;
      }
      j = base + lo;
    }
    __syncthreads();
    if (tid == 255) carry_s = carry + scan[255];
    __syncthreads();
  }
  if (j < 0 || t >= r.frames) return;
  const float noise_scale = r.noise_scale;
  const float* noise = noise_scale != 0.f ? r.noise : nullptr;
  const int64_t f = (int64_t)r.frame + t;
  const int c_lo = blockIdx.z * 16, c_hi = c_lo + 16 < C ? c_lo + 16 : C;
  for (int c = c_lo; c < c_hi; ++c) {
    const float m = r.stats[(int64_t)c * r.stride + j];
    const float lg = r.stats[(int64_t)(C + c) * r.stride + j];
    float zp = m;
    if (noise) zp = m + noise[(int64_t)c * r.noise_stride + f] * expf(lg) * noise_scale;
    r.z_p[(int64_t)c * r.z_stride + f] = zp;
  }
}

void launch_expand_ranges(const ExpandRange* rows, int n, int C, int max_frames, hipStream_t s) {
  hipLaunchKernelGGL(expand_ranges_kernel, dim3((unsigned)((max_frames + 255) / 256), n, (C + 15) / 16), dim3(256), 0, s,
                     rows, C);
}

__global__ __launch_bounds__(256) void gather_windows_kernel(const FlowRow* __restrict__ rows, float* __restrict__ z,
                                                             int C, int T) {
  const int b = blockIdx.z, c = blockIdx.y;
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= T) return;
  const FlowRow r = rows[b];
  z[((int64_t)b * C + c) * T + t] = t < r.frames ? r.z_p[(int64_t)c * r.stride + r.wa + t] : 0.f;
}

void launch_gather_windows(const FlowRow* rows, float* z, int B, int C, int T, hipStream_t s) {
  hipLaunchKernelGGL(gather_windows_kernel, dim3((unsigned)((T + 255) / 256), C, B), dim3(256), 0, s, rows, z, C, T);
}

// ---------------------------------------------------------------------------
// Speaker conditioning: 1x1 convs on g [B, gin, 1] are GEMVs
// (models.py:127 dp.cond, modules.py:152 WN cond_layer, modules.py:215 ResBlock cond).
// ---------------------------------------------------------------------------
__global__ void cond_gemv_kernel(const float* g, const float* table, const int64_t* sid,
                                 const float* W, const float* bias, float* out, int Cin, int Cout) {
  const int b = blockIdx.y;
  const int co = blockIdx.x * blockDim.x + threadIdx.x;
  if (co >= Cout) return;
  const float* gv = table ? table + sid[b] * Cin : g + (int64_t)b * Cin;
  const float* wr = W + (int64_t)co * Cin;
  float acc = 0.f;
  for (int ci = 0; ci < Cin; ++ci) acc = fmaf(wr[ci], gv[ci], acc);
  out[(int64_t)b * Cout + co] = acc + (bias ? bias[co] : 0.f);
}

void launch_cond_gemv(const float* g, const float* table, const int64_t* sid, const float* W,
                      const float* bias, float* out, int B, int Cin, int Cout, hipStream_t s) {
  dim3 grid((Cout + 127) / 128, B);
  hipLaunchKernelGGL(cond_gemv_kernel, grid, dim3(128), 0, s, g, table, sid, W, bias, out, Cin, Cout);
}

// Row r < n_rows is table[r]; row n_rows + j of a defined voice slot j < voices.slots is voices.rows[j] (the blended
// speakers, below); every other id is flagged in `bad` and reads row 0.
__global__ void gather_rows_kernel(const float* table, const int64_t* sid, float* out, int C,
                                   int n_rows, int* bad, const VoiceTable voices) {
  const int b = blockIdx.y;
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const long long r = sid[b];
  const float* src = table;
  if (r >= 0 && r < n_rows) {
    src = table + r * C;
  } else if (r >= n_rows && r - n_rows < voices.slots && voices.defined[r - n_rows]) {
    src = voices.rows + (r - n_rows) * C;
  } else if (bad && c == 0) {
    bad[b] = 1;
  }
  out[(int64_t)b * C + c] = src[c];
}

void launch_gather_rows(const float* table, const int64_t* sid, float* out, int B, int C,
                        int n_rows, int* bad, hipStream_t s, VoiceTable voices) {
  dim3 grid((C + 127) / 128, B);
  hipLaunchKernelGGL(gather_rows_kernel, grid, dim3(128), 0, s, table, sid, out, C, n_rows, bad, voices);
}

// ---------------------------------------------------------------------------
// Blended speakers: block (x, v) writes channels [128 x, 128 x + 128) of voice defs[v] to rows[defs[v].slot] and
// marks the slot defined.  A ready row is copied; a blend is the fp32 chain acc = w_0 e_0[c], then
// acc = fmaf(w_k, e_k[c], acc) for k = 1 .. count - 1 in ascending k, e_k = table[ids[k]]: a one-hot blend is
// bitwise its table row.  The host has checked slot, count and ids (capi.hip); two definitions never share a slot.
// ---------------------------------------------------------------------------
__global__ void speaker_blend_kernel(const VoiceDef* __restrict__ defs, const float* __restrict__ table,
                                     float* __restrict__ rows, int* __restrict__ defined, int C) {
  const VoiceDef& d = defs[blockIdx.y];
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  float acc;
  if (d.vector) {
    acc = d.vector[c];
  } else {
    acc = d.weights[0] * table[(int64_t)d.ids[0] * C + c];
    for (int k = 1; k < d.count; ++k) acc = fmaf(d.weights[k], table[(int64_t)d.ids[k] * C + c], acc);
  }
  rows[(int64_t)d.slot * C + c] = acc;
  if (c == 0) defined[d.slot] = 1;
}

void launch_speaker_blend(const VoiceDef* defs, int n, const float* table, float* rows, int* defined, int C,
                          hipStream_t s) {
  dim3 grid((C + 127) / 128, n);
  hipLaunchKernelGGL(speaker_blend_kernel, grid, dim3(128), 0, s, defs, table, rows, defined, C);
}

__global__ void unscale_xpost_kernel(const float* src, float* dst, int rows, int F, int64_t n) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    const int ch = (int)((i / F) % rows);
    dst[i] = src[i] * ((ch % 18) < 9 ? 0.69314718055994531f : 6.28318530717958648f);
  }
}

void launch_unscale_xpost(const float* src, float* dst, int B, int rows, int F, hipStream_t s) {
  const int64_t n = (int64_t)B * rows * F;
  int blocks = (int)((n + 255) / 256);
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(unscale_xpost_kernel, dim3(blocks), dim3(256), 0, s, src, dst, rows, F, n);
}

// ---------------------------------------------------------------------------
// Wire-format epilogue of the service wrapper (tts_vits.py:204-217): per utterance
//   peak = max |x| over the valid samples; if auto_normalize and peak > 0.01: x = x / peak * 0.9
//   x = clip(x, -1, 1); pcm = int16(x * 32767)   (truncation toward zero, as ndarray.astype)
// Same fp32 operation order as the NumPy code, so the int16 stream is bit-exact.
// ---------------------------------------------------------------------------
// valid samples of row b, clamped to the row: after infer(max_len=k) the waveform rows hold only
// spf * k samples while y_lengths still counts the untruncated frames (models.py:733-734)
__device__ __forceinline__ int64_t valid_samples(const int64_t* lens, int b, int spf, int64_t stride) {
  if (!lens) return stride;
  const int64_t n = lens[b] * (int64_t)spf;
  return n < 0 ? 0 : (n > stride ? stride : n);
}

__global__ void absmax_kernel(const float* x, const int64_t* lens, int64_t stride, int spf,
                              unsigned* peak_bits) {
  const int b = blockIdx.y;
  const int64_t n = valid_samples(lens, b, spf, stride);
  const float* xb = x + (int64_t)b * stride;
  float m = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    m = fmaxf(m, fabsf(xb[i]));
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
  if ((threadIdx.x & 63) == 0) atomicMax(&peak_bits[b], __float_as_uint(m));   // m >= 0: bit order == value order
}

__global__ void pcm16_kernel(const float* x, const int64_t* lens, int64_t stride, int spf,
                             const unsigned* peak_bits, int auto_normalize, short* out) {
  const int b = blockIdx.y;
  const int64_t n = valid_samples(lens, b, spf, stride);
  const float peak = __uint_as_float(peak_bits[b]);
  const bool norm = auto_normalize && peak > 0.01f;
  const float* xb = x + (int64_t)b * stride;
  short* ob = out + (int64_t)b * stride;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < stride; i += (int64_t)gridDim.x * blockDim.x) {
    float v = 0.f;
    if (i < n) {
      v = xb[i];
      if (norm) v = (v / peak) * 0.9f;
      v = fminf(fmaxf(v, -1.f), 1.f);
      v = v * 32767.f;
    }
    ob[i] = (short)(int)v;
  }
}

void launch_pcm16(const float* x, const int64_t* lens, int B, int64_t stride, int spf, int auto_normalize,
                  unsigned* peak_scratch, short* out, hipStream_t s) {
  (void)hipMemsetAsync(peak_scratch, 0, (size_t)B * sizeof(unsigned), s);
  int bx = (int)((stride + 255) / 256);
  if (bx > 256) bx = 256;
  hipLaunchKernelGGL(absmax_kernel, dim3(bx, B), dim3(256), 0, s, x, lens, stride, spf, peak_scratch);
  hipLaunchKernelGGL(pcm16_kernel, dim3(bx, B), dim3(256), 0, s, x, lens, stride, spf, peak_scratch,
                     auto_normalize, out);
}

// ROWS (pooled voice conversion, kernels.h): row b takes noise_scale and its noise block [I, noise_stride] from
// rows[b]; frames at and past noise_stride (behind the row's own length) read no noise — they are masked to 0
template <bool ROWS>
__global__ void posterior_sample_kernel(const float* stats, const float* noise, const int* lens,
                                        float* z, int I, int T, float noise_scale, const AdmitSynRow* rows) {
  const int b = blockIdx.z, c = blockIdx.y;
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= T) return;
  const float m = stats[((int64_t)b * 2 * I + c) * T + t];
  const float lg = stats[((int64_t)b * 2 * I + I + c) * T + t];
  const int64_t o = ((int64_t)b * I + c) * T + t;
  int64_t no = o;
  if (ROWS) {
    const AdmitSynRow r = rows[b];
    noise_scale = r.noise_scale;
    const int64_t nl = r.noise_len ? r.noise_len : r.noise_stride;
    noise = (noise_scale != 0.f && t < nl) ? r.noise : nullptr;
    no = (int64_t)c * r.noise_stride + t;
  }
  const float v = noise ? m + (noise[no] * noise_scale) * expf(lg) : m;   // (noise_scale 1: exact)
  z[o] = t < lens[b] ? v : 0.f;
}

void launch_posterior_sample(const float* stats, const float* noise, const int* lens, float* z, int B,
                             int I, int T, hipStream_t s, float noise_scale) {
  dim3 grid((T + 127) / 128, I, B);
  hipLaunchKernelGGL(posterior_sample_kernel<false>, grid, dim3(128), 0, s, stats, noise, lens, z, I, T, noise_scale,
                     nullptr);
}

void launch_posterior_sample_rows(const float* stats, const AdmitSynRow* rows, const int* lens, float* z, int B,
                                  int I, int T, hipStream_t s) {
  dim3 grid((T + 127) / 128, I, B);
  hipLaunchKernelGGL(posterior_sample_kernel<true>, grid, dim3(128), 0, s, stats, nullptr, lens, z, I, T, 0.f, rows);
}

__global__ void sequence_mask_kernel(const int* lens, float* mask, int T) {
  const int b = blockIdx.y;
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < T) mask[(int64_t)b * T + t] = t < lens[b] ? 1.f : 0.f;
}

void launch_sequence_mask(const int* lens, float* mask, int B, int T, hipStream_t s) {
  hipLaunchKernelGGL(sequence_mask_kernel, dim3((T + 255) / 256, B), dim3(256), 0, s, lens, mask, T);
}

__global__ void lens_to_i32_kernel(const int64_t* lens, int* out, int B, int T, int* bad) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const long long l = lens[b];
  out[b] = l < 0 ? 0 : (l > T ? T : (int)l);
  bad[b] = (l < 0 || l > T) ? 1 : 0;
}

void launch_lens_to_i32(const int64_t* lens, int* out, int B, int T, int* bad, hipStream_t s) {
  hipLaunchKernelGGL(lens_to_i32_kernel, dim3((B + 63) / 64), dim3(64), 0, s, lens, out, B, T, bad);
}

__global__ void fill_kernel(float* p, float v, int64_t n) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) p[i] = v;
}

// trimmed decode (ConvArgs::trim_map): per-utterance column-tile counts, their prefix sums and the tile -> utterance map
__global__ void trim_map_kernel(const int* __restrict__ lens, int B, int num, int add, int T, int BN, int* __restrict__ out) {
  __shared__ int part[256];
  const int tid = threadIdx.x;
  const int per = (B + 255) / 256;
  auto tiles_of = [&](int b) {
    long lim = (long)lens[b] * num + add;
    lim = lim < 0 ? 0 : (lim > T ? T : lim);
    return (int)((lim + BN - 1) / BN);
  };
  int s = 0;
  for (int i = 0; i < per; ++i) { const int b = tid * per + i; if (b < B) s += tiles_of(b); }
  part[tid] = s;
  __syncthreads();
  if (tid == 0) { int run = 0; for (int i = 0; i < 256; ++i) { const int v = part[i]; part[i] = run; run += v; } }
  __syncthreads();
  int run = part[tid];
  for (int i = 0; i < per; ++i) {
    const int b = tid * per + i;
    if (b < B) {
      out[b] = run;
      const int n = tiles_of(b);
      for (int k = 0; k < n; ++k) out[B + 1 + run + k] = b;
      run += n;
      if (b == B - 1) out[B] = run;
    }
  }
}
size_t launch_trim_map_ints(int B, int T, int BN) { return (size_t)B + 1 + (size_t)B * ((T + BN - 1) / BN); }
void launch_trim_map(const int* lens, int B, int num, int add, int T, int BN, int* out, hipStream_t s) {
  hipLaunchKernelGGL(trim_map_kernel, dim3(1), dim3(256), 0, s, lens, B, num, add, T, BN, out);
}

// "tail_once" (kernels.h): the trim map of a launch whose zero-input tail only the donor row computes
__global__ void tail_map_kernel(const int* __restrict__ lens, int B, const TailMapJobs jobs, unsigned long long* __restrict__ dropped) {
  __shared__ int part[256];
  __shared__ int part_b[256];
  const TailMapJob jb = jobs.job[blockIdx.x];
  const int num = jb.num, reach = jb.reach, T = jb.T, BN = jb.BN;
  int* const out = jb.out;
  const int tid = threadIdx.x;
  const int per = (B + 255) / 256;
  // donor: smallest length, lowest index on ties (a thread owns a run of rows in index order)
  int best = 0x7fffffff, best_b = 0x7fffffff;
  for (int i = 0; i < per; ++i) { const int b = tid * per + i; if (b < B && lens[b] < best) { best = lens[b]; best_b = b; } }
  part[tid] = best; part_b[tid] = best_b;
  __syncthreads();
  if (tid == 0) {
    for (int i = 1; i < 256; ++i) if (part[i] < best) { best = part[i]; best_b = part_b[i]; }
    part_b[0] = best_b;
  }
  __syncthreads();
  const int donor = part_b[0];
  __syncthreads();
  const int full = (T + BN - 1) / BN;
  if (jb.pack_gap > 0) {                // packed job (kernels.h): the block table instead of the tile map
    const int gap = jb.pack_gap;
    auto sp_of = [&](int b) { return tail_pack_sp(lens[b], num, reach, T, b == donor); };
    int s = 0;
    for (int i = 0; i < per; ++i) { const int b = tid * per + i; if (b < B) s += tail_pack_row_blocks(sp_of(b), gap); }
    part[tid] = s;
    __syncthreads();
    if (tid == 0) { int run = 0; for (int i = 0; i < 256; ++i) { const int v = part[i]; part[i] = run; run += v; } }
    __syncthreads();
    int run = part[tid];
    for (int i = 0; i < per; ++i) {
      const int b = tid * per + i;
      if (b < B) {
        const int sp = sp_of(b);
        out[kTailPackHdr + b] = sp;
        tail_pack_row(out, B, b, run, sp, gap, jb.pad_right);
        run += tail_pack_row_blocks(sp, gap);
        if (b == B - 1) {
          tail_pack_finish(out, B, T, gap, BN, donor, run);
          const long left_out = (long)B * full - out[0];         // (the gaps can cost more than short tails save)
          if (dropped && left_out > 0) atomicAdd(dropped, (unsigned long long)left_out);
        }
      }
    }
    return;
  }
  auto tiles_of = [&](int b) {
    if (b == donor) return full;
    long lim = (long)lens[b] * num + reach;
    lim = lim < 0 ? 0 : (lim > T ? T : lim);
    return (int)((lim + BN - 1) / BN);
  };
  int s = 0;
  for (int i = 0; i < per; ++i) { const int b = tid * per + i; if (b < B) s += tiles_of(b); }
  part[tid] = s;
  __syncthreads();
  if (tid == 0) { int run = 0; for (int i = 0; i < 256; ++i) { const int v = part[i]; part[i] = run; run += v; } }
  __syncthreads();
  int run = part[tid];
  for (int i = 0; i < per; ++i) {
    const int b = tid * per + i;
    if (b < B) {
      out[b] = run;
      const int n = tiles_of(b);
      for (int k = 0; k < n; ++k) out[B + 1 + run + k] = b;
      run += n;
      if (b == B - 1) {
        out[B] = run;
        out[B + 1 + (long)B * full] = donor;
        if (dropped) atomicAdd(dropped, (unsigned long long)((long)B * full - run));
      }
    }
  }
}
size_t launch_tail_map_ints(int B, int T, int BN) { return launch_trim_map_ints(B, T, BN) + 1; }
void launch_tail_maps(const int* lens, int B, const TailMapJobs& jobs, int n, unsigned long long* dropped, hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(tail_map_kernel, dim3(n), dim3(256), 0, s, lens, B, jobs, dropped);
}

// one workgroup per (row m, utterance b): the columns behind the tiles row b kept, from the donor's row m
template <bool VEC>
__global__ void tail_fill_kernel(float* __restrict__ y, int64_t y_bstride, int B, int T, int BN, const int* __restrict__ map, int packed) {
  const int m = blockIdx.x, b = blockIdx.y;
  const int full = (T + BN - 1) / BN;
  // (packed table: the columns from S_b' on — a multiple of 32, or T)
  const int donor = packed ? map[1] : map[B + 1 + (long)B * full];
  if (b == donor) return;
  const long c0 = packed ? (long)map[kTailPackHdr + b] : (long)(map[b + 1] - map[b]) * BN;
  if (c0 >= T) return;
  const float* src = y + (int64_t)donor * y_bstride + (int64_t)m * T;
  float* dst = y + (int64_t)b * y_bstride + (int64_t)m * T;
  if constexpr (VEC) {      // (c0 is a multiple of BN, BN of 4, and so is T)
    for (long c = c0 + 4 * threadIdx.x; c < T; c += 4 * blockDim.x)
      *reinterpret_cast<float4*>(dst + c) = *reinterpret_cast<const float4*>(src + c);
  } else {
    for (long c = c0 + threadIdx.x; c < T; c += blockDim.x) dst[c] = src[c];
  }
}
void launch_tail_fill(float* y, int64_t y_bstride, int B, int M, int T, int BN, const int* map, hipStream_t s, bool packed) {
  const bool vec = T % 4 == 0 && y_bstride % 4 == 0 && BN % 4 == 0 && (reinterpret_cast<uintptr_t>(y) & 15) == 0;
  if (vec) hipLaunchKernelGGL(tail_fill_kernel<true>, dim3(M, B), dim3(256), 0, s, y, y_bstride, B, T, BN, map, (int)packed);
  else hipLaunchKernelGGL(tail_fill_kernel<false>, dim3(M, B), dim3(256), 0, s, y, y_bstride, B, T, BN, map, (int)packed);
}

// row-exact ragged decode: the rows of a class and their lengths at the decoder's three rates, from host values
// carried in the kernel arguments (no copy, no synchronisation)
__global__ void ragged_rows_kernel(const RaggedRowsArg r, int n, int first, int us, int* __restrict__ out, int stride) {
  const int i = threadIdx.x;
  if (i >= n) return;
  const int len = r.len[i];
  out[first + i] = r.row[i];
  out[stride + first + i] = len;
  out[2 * stride + first + i] = us * len;
  out[3 * stride + first + i] = us * us * len;
}

void launch_ragged_rows(const RaggedRowsArg& r, int n, int first, int us, int* out, int stride, hipStream_t s) {
  hipLaunchKernelGGL(ragged_rows_kernel, dim3(1), dim3(kRaggedChunk), 0, s, r, n, first, us, out, stride);
}

__global__ void gather_frames_kernel(const float* __restrict__ src, int64_t src_bstride, int src_rstride,
                                     const int* __restrict__ rows, const int* __restrict__ lens, int C, int T,
                                     float* __restrict__ dst) {
  const int i = blockIdx.z, c = blockIdx.y;
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int len = lens ? lens[i] : T;
  if (t < T && t < len)
    dst[((int64_t)i * C + c) * T + t] = src[rows[i] * src_bstride + (int64_t)c * src_rstride + t];
}

void launch_gather_frames(const float* src, int64_t src_bstride, int src_rstride, const int* rows, const int* lens,
                          int n, int C, int T, float* dst, hipStream_t s) {
  const int nt = T >= 256 ? 256 : 64;
  hipLaunchKernelGGL(gather_frames_kernel, dim3((T + nt - 1) / nt, C, n), dim3(nt), 0, s, src, src_bstride,
                     src_rstride, rows, lens, C, T, dst);
}

// blockIdx.y < C: channel row c of window i; blockIdx.y == C (only when gin > 0): the row's speaker vector
__global__ void gather_windows_kernel(const PoolRow* __restrict__ rows, int C, int T, float* __restrict__ dst, int gin,
                                      float* __restrict__ gdst) {
  const int i = blockIdx.z, c = blockIdx.y;
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const PoolRow r = rows[i];
  if (c == C) {
    for (int k = t; k < gin; k += gridDim.x * blockDim.x) gdst[(int64_t)i * gin + k] = r.g[k];
    return;
  }
  if (t < T && t < r.len) dst[((int64_t)i * C + c) * T + t] = r.z[(int64_t)c * r.z_stride + r.wa + t];
}

void launch_gather_windows(const PoolRow* rows, int n, int C, int T, float* dst, int gin, float* gdst, hipStream_t s) {
  const int nt = T >= 256 ? 256 : 64;
  hipLaunchKernelGGL(gather_windows_kernel, dim3((T + nt - 1) / nt, C + (gin > 0 ? 1 : 0), n), dim3(nt), 0, s, rows, C, T,
                     dst, gin, gdst);
}

void launch_fill(float* p, float v, int64_t n, hipStream_t s) {
  int blocks = (int)((n + 255) / 256);
  if (blocks > 4096) blocks = 4096;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(fill_kernel, dim3(blocks), dim3(256), 0, s, p, v, n);
}

}  // namespace mbv
