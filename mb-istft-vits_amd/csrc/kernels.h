// Internal launch interface of the gfx950 kernels (host side, no torch).
// Layout everywhere: fp32 [B, C, time], time fastest.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

namespace mbv {

// ---------------------------------------------------------------- table upload
// Every device table of the pooled entries (one Row per utterance, chunk or recording) goes up the same way: the rows
// travel by value as kernel arguments, N per launch, no copy and no synchronisation.  upload_rows walks rows
// [0, n): row i = fill(i) -> dst[i], then extra(i, row) for the columns a table derives from its rows.
template <typename Row, int N>
struct RowsArg { Row row[N]; };
struct NoExtra {
  template <typename Row>
  __device__ void operator()(int, const Row&) const {}
};
template <typename Row, int N, typename Extra>
__global__ void rows_kernel(const RowsArg<Row, N> r, int n, int first, Row* __restrict__ dst, const Extra extra) {
  const int i = threadIdx.x;
  if (i >= n) return;
  dst[first + i] = r.row[i];
  extra(first + i, r.row[i]);
}
template <int N, typename Row, typename Fill, typename Extra = NoExtra>
void upload_rows(size_t n, Row* dst, hipStream_t s, Fill fill, Extra extra = Extra{}) {
  static_assert(sizeof(RowsArg<Row, N>) + 64 <= 4096, "kernel arguments stay under 4 KiB per launch");
  for (size_t f = 0; f < n; f += N) {
    RowsArg<Row, N> r{};
    const int nn = (int)(n - f < (size_t)N ? n - f : (size_t)N);
    for (int i = 0; i < nn; ++i) r.row[i] = fill(f + i);
    hipLaunchKernelGGL((rows_kernel<Row, N, Extra>), dim3(1), dim3(N), 0, s, r, nn, (int)f, dst, extra);
  }
}

// ---------------------------------------------------------------- conv1d (MFMA)
// Packed weight layout of the implicit-GEMM conv kernel (k-interleaved, see conv1d.hip):
//   Wp[K][Cin/8][ci & 1][Mpad][(ci % 8) / 2], Mpad a multiple of 128, rows >= M zero.
enum ConvEpilogue : int {
  EPI_STORE = 0,     // y = acc + bias  [relu] [*out_mask]
  EPI_RESID = 1,     // y = acc + bias + res (+chan_add)
  EPI_RESID_ACC = 2, // y = ((accum_in ? accum_in : 0) + acc + bias + res (+chan_add)) * out_scale
  EPI_GATE = 3,      // rows come in (tanh-tile, sigmoid-tile) pairs: y[c] = tanh(.)*sigmoid(.)
  EPI_RES_SKIP = 4,  // row < split: xio = (xio + v) * mask ; else skip[row-split] (+)= v
  EPI_COUPLE = 5,    // y = (y + couple_sign * (acc + bias) * mask) * mask   (sign -1: reverse flow)
  EPI_CONVT = 6,     // ConvTranspose1d(k16, stride U = 4 | 8, p (16-U)/2) as a (16/U + 1)-tap conv over its U
                     // output phases: rows come in groups of 64 = 64/U channels x (first U/2 phases | last
                     // U/2 phases); tap 0 is all-zero for the second half, the last tap for the first
                     // (their MFMAs are skipped); a lane stores y[co, U t .. U t + U - 1]
  EPI_LN = 7,        // conv1d_narrow.hip only (T <= 256, M <= 768): y = LN_c( relu?(acc + bias) * out_mask + res ) * gamma + beta
                     // [* ln_mask]: the conv that feeds a channel LayerNorm and that LayerNorm in one launch
                     // (attentions.py:40-46 conv_o / ffn -> norm(x + y); models.py:128-135 conv -> relu -> norm)
};

struct ConvArgs {
  // input
  const float* x;          // [B, Cin, Tin] (+ offsets folded into the pointer)
  int64_t x_bstride;       // elements between batches
  int Tin;                 // valid input length (positions >= Tin read as zero padding)
  int x_rstride;           // elements between channel rows of x (>= Tin)
  int Cin;
  // weights
  const float* w;          // packed, k-interleaved (above)
  const float* bias;       // [M] in packed-row order, or nullptr
  int M;                   // real output rows (packed order)
  int Mpad;
  int K;
  int dil;
  int pad_left;            // input index = t + tap*dil - pad_left
  // prologue
  float in_slope;          // leaky-relu slope on the input (1 = identity)
  const int* in_lens;      // if set: input *= (t < in_lens[b])
  const float* chan_add;   // if set: [B, Cin] added to the input before the activation
  int reflect1;            // ReflectionPad1d((1,0)) in front of the conv (models.py:364)
  // output
  float* y;                // [B, My, T]
  int64_t y_bstride;
  int T;                   // output length (row stride of y / res / accum)
  int epi;
  int relu;
  const int* out_lens;     // mask for STORE / RES_SKIP / COUPLE
  const float* res;        // RESID*: residual [B, M, T]
  int64_t res_bstride;
  const float* res_chan_add;  // RESID*: [B, M] added to the residual (ResBlock cond)
  const float* accum_in;   // RESID_ACC
  float out_scale;
  const float* gate_cond;  // GATE: [B, gate_cond_stride] conditioning, already offset to this layer
  int gate_cond_bstride;
  int gate_half;           // GATE: H (rows of the tanh half)
  float* skip;             // RES_SKIP: [B, M - split, T]
  int split;               // RES_SKIP
  int skip_accum;          // RES_SKIP: skip += v instead of skip = v
  float couple_sign;       // COUPLE: -1 reverse (x1 - m), +1 forward (x1 + m)
  int B;
  // r03, opt-in trimmed decode (mbv_set_option "trim"): only the column tiles that hold frames below a per-utterance
  // limit exist as work.  trim_map (device, launch_trim_map): [0 .. B] prefix sums of ceil(limit_b / BN), then the
  // utterance of every column tile; trim_bn = the BN it was built for (checked by the launcher).  The kernel walks
  // (column tile, row tile) pairs of that compact list; nothing else changes.  nullptr: every tile (default).
  const int* trim_map;
  int trim_bn;
  // r03 virtual-sequence tiling (launch_conv1d, EPI_CONVT): > 0 = column tiles run through the batch laid end to end,
  // utterance b at virtual column b * vs_tv (vs_tv = T + halo); set by the launcher only
  int vs_tv;
  // "tail_once", packed route (CONV_TAIL_PACK): tail_pack = 1 asks the planner for it (set by the decoder's
  // tail path and mbv_op_conv only); pack_tbl (device, launch_tail_maps with a packed job) is the block table the
  // kernel tiles over, pack_blocks the entries it holds (tail_pack_blocks)
  int tail_pack;
  const int* pack_tbl;
  int pack_blocks;
  // split-K scratch (small launches): partial accumulators + one self-resetting ticket per tile
  // (conv1d_plan decides from the sizes alone: ws_floats / n_counters are 0 whenever ws / counters are null)
  float* ws;
  size_t ws_floats;
  unsigned* counters;
  int n_counters;
  int convt_u;             // EPI_CONVT: upsampling stride (4 or 8)
  int splitk;              // 1: split-K allowed for this launch (mbv_set_option "splitk" / MBV_CONV_SPLITK)
  int prec;                // 0: exact fp32 MFMA (default); 3: opt-in split-bf16, three products (mbv_set_option "conv_bf16")
  const float* w_split;    // prec == 3: the same packed weights as [bf16 hi x 4 | bf16 mid x 4] slots (launch_split_planes)
  // EPI_LN
  const float* ln_gamma;   // [M]
  const float* ln_beta;    // [M]
  const int* ln_out_lens;  // mask behind the LayerNorm (the encoder's last layer), or nullptr
};
// Which kernel launch_conv1d runs for a ConvArgs, as data (pure host logic: no launch, no device access; pointers
// are only tested against null).  Values match MBV_ROUTE_* of include/mbistft_vits.h.
enum ConvRoute : int {
  CONV_NARROW_M = 1,        // conv1d_narrow.hip, row blocks by M (T <= 256, EPI_LN)
  CONV_NARROW_LAUNCH = 2,   // conv1d_narrow.hip, row blocks by launch size (split-K mode, few tiles)
  CONV_M64 = 3,             // 64 x 128 tiles, 256 threads (<= 64 rows)
  CONV_HALF = 4,            // 64 x 384 tiles, 256 threads (<= 64 rows, long and many)
  CONV_SMALL = 5,           // 128 x 128 tiles, 256 threads (split-K when S > 1)
  CONV_BIG = 6,             // 128 x 384 tiles, 512 threads
  CONV_SPLIT_BATCH = 7,     // the first nb_big utterances on 128 x 384 tiles, the rest on 128 x 128
  CONV_VS = 8,              // 128 x 384 tiles over the virtual sequence of the batch (stride-4 EPI_CONVT)
  CONV_TAIL_PACK = 9,       // 128 x 384 tiles over the packed column axis of a tail_once launch (ConvArgs::tail_pack)
};
struct ConvPlan {
  int route;
  int bm, bn, threads, ck;  // tile shape of the launch (of its first part for CONV_SPLIT_BATCH); 0 for the narrow kernel
  int nb_big;               // CONV_SPLIT_BATCH: utterances on the 128 x 384 shape
  int vs_tv;                // CONV_VS: virtual columns per utterance (T + halo)
  int S;                    // split-K factor (1: none)
};
// trimmed: plan for a launch with a trim map (default: a.trim_map != nullptr)
// route_T > 0: the length the rule "T <= 256 -> narrow kernel" sees instead of a.T.  The ranged decode
// (mbv_decode_range) passes the one-shot decode's length, so that a conv over a z-window runs the same chain of
// operations as the conv over the whole utterance (the narrow kernel starts its sums from the bias, the tiled
// kernels add it last).
ConvPlan conv1d_plan(const ConvArgs& a, bool trimmed, int route_T = 0);
inline ConvPlan conv1d_plan(const ConvArgs& a) { return conv1d_plan(a, a.trim_map != nullptr); }
void launch_conv1d(const ConvArgs& a, hipStream_t s, int route_T = 0);     // executes conv1d_plan(a, ., route_T)
bool conv1d_supported(int K, int dil);   // kernel sizes / dilations the MFMA kernel is built for
// conv1d_narrow.hip: the same contraction in 32-column x row-block units (launches with few columns)
bool conv1d_narrow_supported(const ConvArgs& a);
void launch_conv1d_narrow(const ConvArgs& a, bool by_launch_size, hipStream_t s);

// ---------------------------------------------------------------- fused WN layer (wn_fused.hip)
// One layer of modules.WN (k = 5, dilation 1) in one launch: gate conv + tanh*sigmoid + 1x1 res/skip +
// residual / skip update, over the 32-frame units that hold valid frames.
//   wg  gate conv packed like every conv (Wp[tap][H/8][ci & 1][Mg_pad][(ci % 8) / 2]) with the ROWS in
//       tiles of 32 = [tanh ch 16t..16t+7 | sigmoid 16t..16t+7 | tanh 16t+8..16t+15 | sigmoid 16t+8..16t+15]
//   wr  res/skip 1x1 packed with natural rows and the input channels permuted: packed channel ci
//       <- source channel 8 (ci / 8) + 4 (ci & 1) + ((ci & 7) >> 1)   (the order the gated tile leaves
//       the accumulators in)
//   bg / gcond in reference row order ([tanh rows | sigmoid rows]); br natural.
struct WnLayerArgs {
  const float* h_in;       // [B, H, T]  (read with the frame mask applied)
  float* h_out;            // [B, H, T]  != h_in; unused when last
  float* skip;             // [B, H, T]
  const int* lens;         // [B]
  const int* ustart;       // [B + 1]: launch_wn_units (prefix sums of ceil(len / 16))
  const int* hmap;         // [ustart[B] + 1]: utterance of every half-unit
  const float* wg; const float* bg;
  const float* gcond;      // [B, gcond_bstride] already offset to this layer, or nullptr
  int gcond_bstride;
  const float* wr; const float* br;
  int B, H, T;
  int Mg_pad;              // padded rows of wg
  int Mr, Mr_pad;          // rows of the res/skip conv (2H, or H for the last layer)
  int last;                // Mr == H: every row goes to skip
  int skip_accum;          // skip += (layers > 0) instead of skip =
  // r03: the coupling layer's 1x1 `post` conv (modules.py:346-350) folded into the res/skip convs: their skip rows are
  // W_post . W_rs[skip rows] (Cs = I/2 rows instead of H), so `skip` accumulates m = post(sum of skips) directly and
  // the LAST layer applies the coupling x1 = (x1 + couple_sign * m) on its valid frames instead of storing skip.
  // r03, first layer of a coupling only: the 1x1 `pre` conv (modules.py:339) folded in as well.  h = (W_pre x0 + b) mask
  // is linear in x0' = [x0 ; mask] (Cin' = I/2 + 1 channels, padded to 8 Gi), so the gate conv runs on x0' directly with
  // the composite weights W_in[tap] W_pre' (K-loop of Gi instead of H/8 groups: 13 instead of 24) and the residual rows
  // start from W_pre' x0'(t) computed as one more K-block of the res/skip GEMM (wpre: rows H, padded to >= 128 NRT).
  // h_in then is the x0 half of z: in_cb channels per utterance, the first 8 (Gi - 1) rows real, group Gi - 1 = the mask.
  int Gi;                  // input channel groups of the gate conv / the window; 0: H / 8
  int in_cb;               // channel rows per utterance of h_in; 0: H
  const float* wpre;       // W_pre' packed like every conv (Cin = 8 Gi, natural channel order), or nullptr
  int wpre_Mpad;
  int Cs;                  // channels of `skip` ([B, Cs, T]); 0: H (unfolded)
  float* x1;               // last layer only: the half of z the coupling updates, [B, x1_bstride / T ..] rows Cs; nullptr: store skip
  int64_t x1_bstride;      // elements between utterances of x1 (I * T)
  float couple_sign;       // -1 reverse (x1 - m), +1 forward (x1 + m)
};
bool wn_fused_supported(int H, int K);
bool wn_fused_fits(int B, int H, int T);      // h / skip small enough for the kernel's 32-bit offsets
// may a coupling layer's `pre` / `post` be folded into its fused WN layers (the kernel's input window / row tiles)
bool wn_prefold_fits(int H, int I);
bool wn_postfold_fits(int H, int I);
// `ustart` points at wn_units_ints(B, T) ints: [B + 1] prefix sums, then the half-unit -> utterance map
size_t wn_units_ints(int B, int T);
void launch_wn_units(const int* lens, int B, int T, int* ustart, int* hmap, hipStream_t s);
void launch_wn_layer(const WnLayerArgs& a, hipStream_t s);

// ---------------------------------------------------------------- text encoder pieces
// bad[b] is set when an utterance has a token id / length outside the valid range
void launch_embed(const int64_t* ids, const int64_t* lens, const float* emb, float* x, int* lens32,
                  int* bad, int B, int T, int H, int n_vocab, hipStream_t s);
// y = LN_c( a (+ r) [relu] ) * gamma + beta  [* mask]
void launch_split_planes(const float* src, float* dst, size_t n_floats, hipStream_t s);   // fp32 slots -> [hi x 4 | mid x 4] bf16
void launch_layernorm(const float* a, const float* r, const float* gamma, const float* beta,
                      float* y, int B, int C, int T, int pre_relu, const int* out_lens,
                      hipStream_t s);
// windowed relative-position attention, qkv [B, 3H, T] -> o [B, H, T]
void launch_rel_attention(const float* qkv, const float* emb_k, const float* emb_v,
                          const int* lens, float* o, int B, int H, int n_heads, int T,
                          hipStream_t s);

// ---------------------------------------------------------------- durations / length regulation
// logw = (w . h*mask + b) * mask ; w_ceil = ceil(exp(logw)*mask*scale) ; cum = cumsum ; ylen
void launch_durations(const float* h, const float* w, const float* b, const int* lens,
                      float length_scale, float* logw, float* w_ceil, int* cum, int* ylen32,
                      int64_t* ylen64, const int* bad, int B, int C, int T, hipStream_t s);
// (w == nullptr: h is logw itself, [B, T] — the SDP path)
// a token of >= 2^20 frames (or inf / NaN) or an utterance of > 2^30: ylen32 = 1, ylen64 = -1 (ops.hip)
// per-token prosody (ops.hip shape_durations_kernel): w_t = ceilf(expf(logw_t) * fl32(s_t * f)) + extra_t from the logw
// a durations launch left; replaces w_ceil (fp32 totals), cum, ylen32 and ylen64 (the range rules and the -1 marker
// above; a negative / infinite / NaN scale or a negative extra below the row's length flags it too).
// A table row (in the arena, upload_rows).  launch_shape_durations reads only frames / lo / hi of row b from it (null
// table: no row is fitted); launch_shape_durations_rows works on the rows the table names, one block each.
struct FitOut { float scale; int32_t status; };          // mbv_fit_result
struct ShapeRow {
  const float* scale;          // this row's scale per token [t_text], or null: `scalar` for every token
  const int* extra;            // extra frames per token [t_text], or null
  FitOut* fit_out;             // where the row's factor and status go, or null
  int64_t frames;              // fit: the frame count to stay within; 0: no fit (f = 1 is not applied at all)
  float lo, hi, scalar;
  int32_t row, t_text, pad_;
};
constexpr int kShapeChunk = 64;    // rows per upload_rows launch: 3.5 KiB of kernel arguments
void launch_shape_durations(const float* logw, const int* lens, const float* scale, const int* extra, float scalar,
                            const ShapeRow* fit, float* w_ceil, int* cum, int* ylen32, int64_t* ylen64, const int* bad,
                            float* fit_stage, FitOut* fit_out, int B, int T, hipStream_t s);
void launch_shape_durations_rows(const float* logw, const int* lens, const ShapeRow* rows, int n, float* w_ceil,
                                 int* cum, int* ylen32, int64_t* ylen64, const int* bad, int T, hipStream_t s);
// token marks: dst[b stride + j] = j ? cum[b, j - 1] : 0 for j < count (<= T + 1); with a table (in the arena,
// upload_rows) row b writes rows[b].count entries to rows[b].dst instead, none where that is null.  One launch.
struct MarkRow {
  int64_t* dst;
  int32_t count, pad_;
};
void launch_token_marks(const int* cum, int B, int T, int64_t* dst, int64_t stride, int count, const MarkRow* rows,
                        hipStream_t s);
// Frame gains (mbv_frame_gain / mbv_frame_gain_rows / mbv_op_frame_gain): the per-token gain spread over
// the z-frames by the rule of expand_kernel, as the table a PcmEnv reads.  With y = min(y_len, frames) (y_len from
// ylen64 when given, where a negative value flags the row, else from ylen32):
//   out[t] = gain[j(t)] for t < y, j(t) = the first token with cum[j] > t;   out[t] = out[y - 1] for y <= t <= frames
// and 1.0f everywhere for a flagged row, for y = 0, and where no token holds the frame.  A copy: bitwise.  Row b of the
// grid reads gain + b T and writes frames + 1 entries to out + b out_stride; with a table (in the arena, upload_rows)
// block row i works on row rows[i].row of the run with that row's own gain [t_text], out and frames.  One launch.
struct GainRow {
  const float* gain;
  float* out;
  int32_t row, t_text, frames, pad_;
};
void launch_frame_gain(const int* cum, const int* ylen32, const int64_t* ylen64, const float* gain, float* out,
                       int64_t out_stride, int frames, int B, int T, hipStream_t s);
void launch_frame_gain_rows(const int* cum, const int* ylen32, const GainRow* rows, int n, int max_frames, int T,
                            hipStream_t s);

// ---------------------------------------------------------------- StochasticDurationPredictor (sdp.hip)
// DDSConv halves (modules.py:98-111), C <= 256
void launch_dds_sep(const float* x, const int* lens, const float* w, const float* bias,
                    const float* gamma, const float* beta, float* y, int B, int C, int T, int K,
                    int dil, hipStream_t s);
void launch_dds_res(const float* a, const float* xres, const float* gamma, const float* beta,
                    float* y, int B, int C, int T, const int* out_lens, hipStream_t s);
// h = pre_w * z[:, zc] + pre_b + cond                      (ConvFlow.pre + DDSConv's x + g)
void launch_sdp_pre(const float* z, int zc, const float* pre_w, const float* pre_b, const float* cond,
                    float* h, int B, int C, int T, hipStream_t s);
// Flip + inverse rational-quadratic spline + mask, in place on z [B, 2, T]; h [B, 29, T]
void launch_sdp_spline(const float* h, float* z, const int* lens, int B, int C, int T,
                       float edge_const, hipStream_t s);
void launch_sdp_logw(const float* z, const float* m, const float* logs, const int* lens, float* logw,
                     int B, int T, hipStream_t s);
void launch_sdp_noise(const float* noise, float scale, float* z, int64_t n, hipStream_t s);
// x[b, c, t] += v[b, c]
void launch_chan_add(float* x, const float* v, int B, int C, int T, hipStream_t s);
// m_t / logs_t: [B, C, T] views with batch stride src_bstride (halves of the enc_p.proj output)
void launch_expand(const float* m_t, const float* logs_t, int64_t src_bstride, const int* cum,
                   const int* ylen, const float* noise, float noise_scale, float* m_p,
                   float* logs_p, float* z_p, float* z, float* attn, float* y_mask, int B, int C,
                   int T, int Tp, hipStream_t s);

// ---------------------------------------------------------------- pooled admission: table-reading variants
// One padded front-half run for many requests (capi.hip mbv_encode_rows / mbv_synthesize_rows): what the scalar
// launches above take as one value per call comes from a device table with one row per utterance.  Every variant
// is the scalar kernel's own body (one template), so an element's chain of operations is the scalar launch's.
struct AdmitEncRow {
  float length_scale, noise_scale_w;
  const float* noise_w;        // this row's SDP noise [2, t_text], packed; null without the SDP
  const void* dur;             // given durations [t_text] of dtype dur_dtype, or null: keep the predicted ones
  int dur_dtype, t_text;
};
struct AdmitSynRow {
  const float* noise;          // this row's prior noise [C, noise_stride]
  int64_t noise_stride;
  float noise_scale;           // 0: zp = m, the noise is not read (the scalar path's null-noise branch)
  int keep;                    // frames of z the request keeps (1 .. its y_len)
  float* z;                    // the request's own [C, keep]
  // live conversion (mbv_convert_ranges): the row is a frame window of a longer recording.  All 0: the rules above.
  int noise_len;               // frames of `noise` (already offset to the window) that may be read; 0: noise_stride
  int src_off;                 // the kept frames start at frame src_off of the run's row
  int64_t z_stride;            // row stride of `z` (already offset to the first kept frame); 0: keep
};
constexpr int kAdmitChunk = 64;   // rows per upload_rows launch
// launch_durations with length_scale = rows[b].length_scale
void launch_durations_rows(const float* h, const float* w, const float* b, const int* lens, const AdmitEncRow* rows,
                           float* logw, float* w_ceil, int* cum, int* ylen32, int64_t* ylen64, const int* bad, int B,
                           int C, int T, hipStream_t s);
// launch_sdp_noise on z [B, 2, T]: row b from its own packed [2, t_text] block, zeros behind t_text
void launch_sdp_noise_rows(const AdmitEncRow* rows, float* z, int B, int T, hipStream_t s);
// launch_set_durations for the rows that carry durations (their own [t_text] tensor); the others keep everything
void launch_set_durations_rows(const AdmitEncRow* rows, const int* lens, float* w_ceil, int* cum, int* ylen32,
                               int64_t* ylen64, const int* bad, int B, int T, hipStream_t s);
// launch_expand writing z only: row b reads noise at row stride rows[b].noise_stride (frames below it only)
void launch_expand_rows(const float* m_t, const float* logs_t, int64_t src_bstride, const int* cum, const int* ylen,
                        const AdmitSynRow* rows, float* z, int B, int C, int T, int Tp, hipStream_t s);
// rows[b].z[c, t] = z[b, c, t] * (t < ylen[b]) for t < rows[b].keep: every request's masked, truncated z in one launch
// (with src_off / z_stride: rows[b].z[c z_stride + t] = z[b, c, src_off + t] * (src_off + t < ylen[b]))
void launch_scatter_z_rows(const float* z, const int* ylen, const AdmitSynRow* rows, int B, int C, int Tp, int max_keep,
                           hipStream_t s);

// ---------------------------------------------------------------- live text (capi.hip mbv_take_tokens_rows / mbv_expand_ranges /
// mbv_flow_ranges): an utterance whose tokens are still arriving.  Tables in the arena (upload_rows).
// Token columns [a, b) of row `src` of an encode run into a stream's own token tables: stats[c, j] = the run's
// m_text / logs_text (c < 2 C), dur[j] = (int)w_ceil[src, j], or -1 where *y_length < 0 (the run flagged the row);
// dur_copy (or null) receives dur[a .. b) packed, for the tick's one read-back.  Copies only.  One launch.
struct TakeRow {
  const int64_t* y_length;
  float* stats;                // [2 C, stride]
  int* dur;                    // [stride]
  int* dur_copy;               // [b - a] or null
  int64_t stride;
  int src, a, b, pad_;
};
constexpr int kTextChunk = 48;     // rows per upload_rows launch: 48 x 80 bytes (an ExpandRange) = 3.75 KiB of kernel arguments
void launch_take_tokens_rows(const float* stats, const float* w_ceil, const TakeRow* rows, int n, int C2, int T,
                             int max_cols, hipStream_t s);
// Length regulation of a block of tokens at a running frame offset: with cum the inclusive scan of dur[a .. b) (done in
// the kernel, 256 tokens a round), frame `frame + t`, t < frames, takes token j = the first with cum[j] > t and
//   z_p[c, frame + t] = m[c, j] + noise[c, frame + t] * expf(logs[c, j]) * noise_scale      (m alone at scale 0)
// — expand_kernel's expression on expand_kernel's operands, so the element is bitwise that kernel's.  One launch.
struct ExpandRange {
  const float* stats;          // [2 C, stride]: m | logs
  const int* dur;              // [stride]
  int64_t stride;
  const float* noise;          // [C, noise_stride], or null
  int64_t noise_stride;
  float* z_p;                  // [C, z_stride]
  int64_t z_stride;
  float noise_scale;
  int a, b, frame, frames, pad_;   // frames: the sum of dur[a .. b) as the host read it; nothing behind it is written
};
void launch_expand_ranges(const ExpandRange* rows, int n, int C, int max_frames, hipStream_t s);
// z[b, c, t] = rows[b].z_p[c, wa + t] for t < frames, 0 behind: the window of a stream's z_p as one row of a padded
// flow run.  upload_rows' Extra fills the columns the flows read.
struct FlowRow {
  const float* z_p;
  int64_t stride, sid;
  int wa, frames;
};
struct FlowRowCols {
  int* lens; int64_t* sid;
  __device__ void operator()(int i, const FlowRow& k) const { lens[i] = k.frames; sid[i] = k.sid; }
};
void launch_gather_windows(const FlowRow* rows, float* z, int B, int C, int T, hipStream_t s);

// ---------------------------------------------------------------- speaker conditioning
// out[b][co] = bias[co] + sum_ci W[co][ci] * g[b][ci]   (g = table[sid[b]] if sid)
void launch_cond_gemv(const float* g, const float* table, const int64_t* sid, const float* W,
                      const float* bias, float* out, int B, int Cin, int Cout, hipStream_t s);
// Blended speakers ("voices"): a second table behind the embedding table.  Voice slot j is speaker id n_rows + j once
// defined[j] is set; both sizes are conventions, not limits of the kernels (a slot costs one row of C floats, a
// term one id and one weight in the definition).
constexpr int kVoiceSlots = 256;   // MBV_SPEAKER_SLOTS
constexpr int kBlendMax = 16;      // MBV_BLEND_MAX
struct VoiceTable {                // all zero: no second table
  const float* rows = nullptr;     // [slots][C]
  const int* defined = nullptr;    // [slots], written in stream order
  int slots = 0;
};
// A table row (upload_rows): one definition.  vector != null: that ready row [C] (count, ids, weights unused).
struct VoiceDef {
  int slot, count;
  int ids[kBlendMax];
  float weights[kBlendMax];
  const float* vector;
};
constexpr int kVoiceChunk = 24;    // rows per upload_rows launch: 24 x 144 bytes = 3.4 KiB of kernel arguments
// out[b] = table[sid[b]] for 0 <= sid[b] < n_rows, voices.rows[sid[b] - n_rows] for a defined voice; anything else
// sets bad[b] (where given) and reads row 0
void launch_gather_rows(const float* table, const int64_t* sid, float* out, int B, int C,
                        int n_rows, int* bad, hipStream_t s, VoiceTable voices = VoiceTable{});
// rows[defs[v].slot] = the blend (fp32, ascending k: w_0 e_0, then fmaf) or the ready row of definition v < n, and
// defined[defs[v].slot] = 1: ONE launch, grid (channel tiles, n).  defs is a device table (upload_rows).
void launch_speaker_blend(const VoiceDef* defs, int n, const float* table, float* rows, int* defined, int C,
                          hipStream_t s);

// ---------------------------------------------------------------- fused iSTFT + PQMF
struct IstftArgs {
  const float* x_post;   // [B, 72, F]
  const float* filt;     // 352-float device table, see istft_pqmf.hip (generic taps | c[k][q] | g[j])
  float* o;              // [B, 256 T']
  float* o_mb;           // MB: [B,4,64T'] ; MS: [B,4,256T'] zero-stuffed ; or null
  float* spec;           // [B,4,9,F] or null
  float* phase;          // [B,4,9,F] or null
  int B, Tp, multistream;
  int fixed_bank;        // 1: the PQMF design (cosine-modulated, factorised); 0: arbitrary 4x63 taps
  int exact_math;        // 1: libm expf/sinf/sincosf instead of the hardware transcendentals
  int prescaled;         // 1: x_post rows already carry log2(e) (magnitude) / 1/(2 pi) (phase)
  int polar_in;          // 1: x_post unused; spec / phase [B,4,9,F] are the INPUT (istft_finalize)
  const int* trim_lens;  // opt-in trimmed decode: [B] valid z-frames; samples at and beyond 256 * trim_lens[b] are not computed
                         // (the caller zero-fills o; o_mb / spec / phase must be null)
};
void launch_istft_pqmf(const IstftArgs& a, hipStream_t s);
// Ranged output of the waveform tails (the streaming decode, mbv_decode_range): only the tiles that cover the kept
// samples exist, only those are stored, nothing else is written (IstftArgs: o_mb / spec / phase / trim_lens null,
// x_post prescaled; IstftSbArgs: spec / phase null).  MB / MS: sub-band samples [keep_lo, keep_hi), sample 4 m + p
// of row b at o[b * o_row_stride + 4 (m - keep_lo) + p]; SB: output quads [keep_lo, keep_hi), quad q at
// o[b * o_row_stride + 4 (q - keep_lo)].  o is already offset to the chunk's first sample.  (A separate
// argument, so that the one-shot kernels keep their argument layout and code.)
// row_lens / row_map (device [B], or null): the row-exact ragged decode.  Row b is an utterance of row_lens[b]
// z-frames (<= a.Tp): its frame count, envelope edges and filter padding are those of its stand-alone launch, only
// the tensor strides are the launch's; nothing at or past 64 row_lens[b] is computed or stored; row b goes to row
// row_map[b] of o.
struct IstftRange {
  int keep_lo, keep_hi;
  int64_t o_row_stride;
  const int* row_lens;
  const int* row_map;
};
void launch_istft_pqmf_range(const IstftArgs& a, const IstftRange& r, hipStream_t s);

// Pooled ranged decode (mbv_decode_chunks): row b of a run is the z-window of ONE chunk of some utterance.  Its
// source, its window and what the tail keeps of it are its own; the table lives in the arena (upload_rows).
struct PoolRow {
  const float* z;          // the utterance's z [192, .] at row stride z_stride
  int64_t z_stride;
  const float* g;          // [gin] or null
  float* o;                // where sample 256 `first` of the utterance goes (the chunk's first sample)
  int wa, len;             // the window: z-frames [wa, wa + len) of the utterance
  int keep_lo, keep_hi;    // kept sub-band samples (MB / MS) or output quads (SB) of the window, 64 per z-frame
};
// The ranged tails with per-row ranges and destinations: row b is a window of rows[b].len z-frames inside a launch
// laid out for a.Tp (a.F) exactly as a row of the ragged decode is; tiles [keep_lo / TM, ceil(keep_hi / TM)) of
// every row do work (the grid holds span_tiles(max_keep) per row, the others return at once), and unit u in
// [keep_lo, keep_hi) is stored at rows[b].o + 4 (u - keep_lo).  max_keep >= keep_hi - keep_lo of every row.
void launch_istft_pqmf_pool(const IstftArgs& a, const PoolRow* rows, int max_keep, hipStream_t s);

// single-band iSTFT (iSTFT_Generator, models.py:296-300): x_post [B, 18, F] -> o [B, 4 (F-1)]
struct IstftSbArgs {
  const float* x_post;   // [B, 18, F]
  float* o;              // [B, 4 (F - 1)]
  float* spec;           // [B, 9, F] or null
  float* phase;          // [B, 9, F] or null
  int B, F;
  int exact_math, prescaled;
  int polar_in;          // 1: spec / phase [B,9,F] are the input
};
void launch_istft_single(const IstftSbArgs& a, hipStream_t s);
void launch_istft_single_range(const IstftSbArgs& a, const IstftRange& r, hipStream_t s);
void launch_istft_single_pool(const IstftSbArgs& a, const PoolRow* rows, int max_keep, hipStream_t s);

// x_post rows back to the reference's units (stage introspection): inverse of the pre-scaling
void launch_unscale_xpost(const float* src, float* dst, int B, int rows, int F, hipStream_t s);

// float waveform -> int16 PCM (normalise / clip / scale), tts_vits.py:204-217
void launch_pcm16(const float* x, const int64_t* lens, int B, int64_t stride, int spf, int auto_normalize,
                  unsigned* peak_scratch, short* out, hipStream_t s);

// ---------------------------------------------------------------- resampling (resample.hip)
// librosa.resample(kaiser_best | kaiser_fast) as a polyphase FIR: target / orig = L / M in lowest terms,
// output t reads x[floor(t M / L) - left + k], k < K, with the fp32 weights bank[(t M) mod L][k]; bank row L
// (fraction 1, read from floor(t M / L) - 1) serves the r = 0 outputs whose float64 time t / ratio rounds below
// the integer (resample.hip).
constexpr int kResampleTile = 256;             // outputs per workgroup (one per thread)
constexpr int kResampleMaxPhases = 4096;       // cap on L
constexpr int kResampleMaxTaps = 4096;         // cap on K
constexpr int kResampleMaxLdsFloats = 16384;   // cap on the staged input window (64 KiB)
struct ResampleGeom {
  int L, M;          // target / orig in lowest terms
  int K;             // taps per phase (a multiple of 4; trailing taps zero)
  int left;          // taps left of n_t: tap k reads x[n_t - left + k]
  double ratio;      // float(target) / orig, as resampy and librosa compute it
};
inline int64_t resample_lds_floats(const ResampleGeom& g) {
  return (int64_t)(kResampleTile - 1) * g.M / g.L + 2 + g.K;
}
int resample_reduce(int orig_sr, int target_sr, int* L, int* M);
// host: the float64 bank rounded to fp32, [L + 1][K] (bank may be null to get the geometry alone).
// Returns null on success, else the reason the pair is refused.
const char* resample_bank(int orig_sr, int target_sr, int filter, std::vector<float>* bank, ResampleGeom* geom);
void launch_resample(const float* x, const int64_t* valid, int B, int64_t in_stride, const float* bank,
                     const ResampleGeom& g, float* out, int64_t out_stride, int64_t* out_samples, hipStream_t s);
// streamed wire path: how many outputs of a row of in_total samples are final once its inputs [0, in_avail) exist
// (no tap of theirs, padded zeros included, at or past in_avail); ceil(in_total ratio) once in_avail >= in_total
int64_t resample_ready(const ResampleGeom& g, int64_t in_avail, int64_t in_total);
// launch_resample_pcm16_range (below, behind the structs it takes):
// outputs [out_first, out_first + out_count) of every row from x[.., 0 : in_avail) -> int16 (pcm16_kernel's
// epilogue with the given peaks, null = no normalisation) and the running peak; bank null = equal rates (no FIR).
// The caller guarantees out_first + out_count <= min(resample_ready(g, in_avail, in_stride), pcm_stride).
// law (g711.h; the same for both launchers below): kLawNone stores the int16 (pcm is short*), kLawUlaw / kLawAlaw
// its G.711 byte at the same index (pcm, pcm_stride, pcm_cap, packed and packed_off then address bytes); DESIGN §7.15.
// Fade-out of the wire step (the *_faded entries): with k = t - first, the fp32 value of output t that
// the clip and the quantisation take is first multiplied by
//   1 for k < 0,   (float)(count - k) * inv for 0 <= k < count,   0 for k >= count;      inv = 1.0f / (float)(count + 1)
// (after the limiter's gain where there is one).  A pure function of t: no state, no halo.  count < 0: no fade, and
// the value is not touched.  Both launchers take it: one for all rows of a ranged launch, a table beside the row
// table (null = no row fades) for a pooled one.
struct PcmFade {
  int64_t first, count;
  float inv;
  int32_t pad_;
};
constexpr PcmFade kNoFade{0, -1, 0.f, 0};
// Gain envelope of the wire step (the *_shaped entries): per-token volume.  `gain` is the frame-gain
// table G of the row, fp32 [frames + 1] (launch_frame_gain); model-rate sample j of the row, j < frames * hop, is
// multiplied WHERE THE WIRE TILE READS ITS SOURCE by
//   e(j) = G[f] + w * (G[f + 1] - G[f]),   f = j / hop,   w = (float)(j - f * hop) * inv_hop,   inv_hop = 1.0f / (float)hop
// every operation rounded to fp32 on its own (contraction switched off: no fma), and the staged sample is
// fl32(x[j] * e(j)).  A pure function of j: no state, no halo.  Everything behind the read (FIR, running peak,
// static gain, limiter, fade, clip, G.711) sees the shaped signal.  gain null: no envelope, no multiply, and the row is
// bitwise the unshaped row.  One value (with a row stride) for a ranged launch, a table beside the row table (null =
// no row is shaped) for a pooled one, a table beside the segment table for turns.  A launch without an envelope runs
// the instantiations that know none.
struct PcmEnv {
  const float* gain;           // G [frames + 1], or null
  int64_t frames;
  int32_t hop;                 // model-rate samples per frame
  float inv_hop;
};
constexpr PcmEnv kNoEnv{nullptr, 0, 0, 0.f};
// Look-ahead limiter of the wire step (mbv_resample_pcm16_range_limited / mbv_resample_pcm16_chunks_limited, DESIGN
// §7.14).  With v the sample the unlimited kernels clip (static peak gain included; zero outside the row's computed
// outputs), all in fp32:
//   r[t] = |v[t]| > c ? c / |v[t]| : 1       m[j] = min r[j - H .. j + L]
//   g[t] = (m[t-L] + ... + m[t]) / (float)(L + 1), added in ascending order from m[t-L]       y[t] = v[t] g[t]
// Stateless: a workgroup recomputes v on [t0 - L - H, t_last + L] (every r that the g of its outputs reads), so an
// int16 does not depend on where a range or a tile begins.
constexpr int kLimiterMaxLookahead = 255;
constexpr int kLimiterMaxHold = 1024;
struct LimiterParams {
  float ceiling;               // c, 0 < c <= 1
  int32_t lookahead, hold;     // L, H in output samples
};
// null, or why the parameters are refused
const char* limiter_refusal(const LimiterParams& p);
// v values a workgroup holds: its tile and the halo
inline int64_t limiter_span(const LimiterParams& p) { return kResampleTile + 2 * (int64_t)p.lookahead + p.hold; }
// LDS floats of the limited tile: the staged input window of the span (none with equal rates), v, and two buffers
// of the log-step minimum
inline int64_t limiter_lds_floats(const ResampleGeom& g, bool fir, const LimiterParams& p) {
  const int64_t S = limiter_span(p);
  return (fir ? (S - 1) * g.M / g.L + 2 + g.K : 0) + 3 * S;
}
// outputs that are final under the limiter: t + L below what the resampler has made final, everything once the row
// is complete.  ready / all: resample_ready of the frontier / of the whole row (in_avail for an open row, no `all`)
inline int64_t limiter_ready(int64_t ready, int64_t all, bool complete, int lookahead) {
  if (complete) return all;
  return ready > lookahead ? ready - lookahead : 0;
}
// lim: null, or the limiter of every row: the launch then goes through the limited tile, and the caller guarantees
// out_first + out_count <= min(limiter_ready(..), pcm_stride) and limiter_lds_floats(g, bank, *lim) <= kResampleMaxLdsFloats
void launch_resample_pcm16_range(const float* x, const int64_t* valid, int B, int64_t in_stride, int64_t in_avail,
                                 const float* bank, const ResampleGeom& g, int64_t out_first, int64_t out_count,
                                 const float* peak, void* pcm, int64_t pcm_stride, unsigned* running,
                                 int64_t* out_samples, const LimiterParams* lim, int law, const PcmFade& fade,
                                 const PcmEnv& env, int64_t env_stride, hipStream_t s);
// Pooled wire output (mbv_resample_pcm16_chunks): the ranged step of MANY rows in one launch.  A table row holds
// what launch_resample_pcm16_range takes as scalars and [B] vectors, for ONE row of one stream; the table lives in
// the arena (upload_rows).
struct PcmPoolRow {
  const float* x;              // the stream's wave row
  int64_t in_total;
  const int64_t* valid;        // one int64, or null = in_total
  int64_t in_avail, out_first, out_end;
  const float* peak;           // one float, or null = no normalisation
  short* pcm;                  // the stream's own full-length row (bytes under a G.711 launch)
  int64_t pcm_cap;             // in stored samples
  unsigned* running;           // one value, or null
  int64_t* out_samples;        // one value, or null
  int64_t packed_off;          // where out_first goes in the call's packed buffer, or -1
  LimiterParams lim;           // the row's limiter: read by a limited launch only
  int32_t pad_;
};
constexpr int kPcmPoolChunk = 32;   // rows per upload_rows launch: 32 x 112 bytes = 3.5 KiB of kernel arguments
// Turns on the wire (mbv_resample_turns): the input of a row is not one wave row but a TIMELINE of
// segments, each the waveform of one utterance, with silence between them; it is never materialised.  Timeline index j
// holds x[j - start] g(j - start) of the segment with start <= j < start + n, and 0.f anywhere else.  g is the
// de-click ramp of a segment's two ends, with i the local index, one fp32 multiply with one rounding:
//   i < ramp:       (float)(i + 1) * inv              i >= n - ramp:   (float)(ramp - (i - (n - ramp))) * inv
// (the fade's own ramp, mirrored for the rise; inv = 1.0f / (float)(ramp + 1), as mbv_pcm_fade_make computes it) and
// no multiply anywhere else; ramp <= n / 2, so the two never overlap.  A table row of the pooled kernels
// (a PcmPoolRow with x = null) reads segs[first .. first + count) of the call's segment table: the segments
// that intersect its input window, ascending.  Everything behind the staging is the code of the plain rows, so a turn
// row is bitwise the plain row of the assembled timeline.
struct TurnSeg {
  const float* x;              // the utterance's wave row
  int64_t start, n;            // its place on the timeline and its valid length
  int32_t ramp;                // de-click samples at either end (0: none)
  float inv;
};
struct TurnSlice { int32_t first, count; };
constexpr int kTurnMaxSegs = 4096;   // segments of one call (MBV_TURN_MAX_SEGS)
// One pooled launch: outputs [out_first, out_end) of every table row (n <= 65535), each what launch_resample_pcm16_range
// stores for that row alone (one tile function); also packed[packed_off + t - out_first] when packed is given.  The
// caller guarantees out_end <= min(resample_ready(g, in_avail, in_total), pcm_cap) of every row, and under `limited`
// out_end <= min(limiter_ready(..), pcm_cap).
struct PcmPoolLaunch {
  const PcmPoolRow* rows;
  bool limited;                // every row through the limited tile, each with its own `lim`
  const TurnSlice* slices;     // null: chunk rows.  Else turn rows: slices[i] beside rows[i], into
  const TurnSeg* segs;         //   the call's segment table
  const PcmEnv* envs;          // null, or envs[i] beside rows[i]; for turn rows envs[k] beside segs[k], the envelope of
                               //   that segment in its own sample index (applied before the de-click ramp)
  const PcmFade* fades;        // null, or fades[i] beside rows[i]
  int n;
  int64_t max_count;           // >= out_end - out_first of every row
  int64_t lds_floats;          // limited: >= limiter_lds_floats of every row, <= kResampleMaxLdsFloats; else not read
  void* packed;
  int law;
};
// bank null = equal rates
void launch_resample_pcm16_pool(const PcmPoolLaunch& a, const float* bank, const ResampleGeom& g, hipStream_t s);
// the stand-alone codec: n samples, law kLawUlaw or kLawAlaw (checked by the caller)
void launch_g711_encode(const short* pcm, int64_t n, int law, uint8_t* out, hipStream_t s);
void launch_g711_decode(const uint8_t* in, int64_t n, int law, short* pcm, hipStream_t s);
// Live input (mbv_resample_ranges): fp32 outputs [out_first, out_end) of MANY recordings that are still arriving,
// each from its own raw row (fp32, int16 scaled by 1 / 32768, or G.711 bytes expanded to that int16) into its own
// model-rate row, in one launch.  A table row is one recording; the table lives in the arena (upload_rows,
// kPcmPoolChunk per launch).
constexpr int kWaveUlaw = 8;   // MBV_WAVE_ULAW / MBV_WAVE_ALAW of the header: the live-input resampler alone takes them
constexpr int kWaveAlaw = 9;
struct ResampleRangeRow {
  const void* x;               // the raw recording, read in place
  int32_t dtype;               // 0 = fp32, 1 = int16, kWaveUlaw, kWaveAlaw
  int32_t closed;              // 1: n is the recording's length (outputs at or past int(n ratio) are zeros)
  int64_t n;                   // raw samples that exist: nothing at or past it is loaded
  int64_t out_first, out_end;
  float* out;                  // the recording's own model-rate row
};
// open count of resample_ready without a total: outputs no tap of which lies at or past in_avail
int64_t resample_ready_open(const ResampleGeom& g, int64_t in_avail);
// outputs [out_first, out_end) of every table row (n <= 65535), each what launch_resample stores there for the
// finished recording (one tile function).  max_count >= out_end - out_first of every row.  The caller guarantees out_end <=
// resample_ready_open(g, n) for an open row, <= ceil(n ratio) for a closed one, and the row's capacity.
void launch_resample_ranges(const ResampleRangeRow* rows, int n, int64_t max_count, const float* bank,
                            const ResampleGeom& g, hipStream_t s);

// the fp64 half window of a filter (0 = kaiser_best, 1 = kaiser_fast; checked by the caller), [nb * num_zeros + 1]:
// kaiser(2n + 1, beta)[n:] * rolloff * sinc(rolloff * linspace(0, num_zeros, n + 1)), unscaled.  resample_bank builds
// its phases from it, the time-warp kernel reads it as it is
void resample_window(int filter, std::vector<double>* win, int* num_zeros, int* nb);

// ---------------------------------------------------------------- time warp (warp.hip)
// Per-token pitch by varispeed: a resampler whose ratio changes with the output sample.  One row has F frames of hop
// model-rate samples (n = F hop), a playback rate R[f] in [kPitchMin, kPitchMax] per frame, and the output position of
// every frame start, U[0] = 0, U[f + 1] = U[f] + (double)hop / (double)R[f] in ascending order; n_out = floor(U[F]).
// Output t lies in the frame f with U[f] <= t < U[f + 1], at model time
//   tau = (double)(f hop) + ((double)t - U[f]) (double)R[f]        every operation rounded to fp64 on its own
// and is resampy's interpolator evaluated there with ratio 1 / R[f]: scale = R[f] > 1 ? 1 / R[f] : 1, index step
// int(scale nb), the window times scale, taps outside [0, min(n, in_avail)) zero.  A pure function of t: no state.
constexpr float kPitchMin = 0.5f, kPitchMax = 2.0f;
constexpr int kWarpTile = 256;                 // outputs per workgroup (one per thread)
// floats of the staged window: 255 outputs at kPitchMax apart and the half width of kaiser_best there on both sides
constexpr int kWarpWindow = 776;
// first frame whose rate is not finite or lies outside the bounds, or -1; then U [F + 1] and *n_out are written
int64_t warp_plan(int hop, int64_t F, const float* R, double* U, int64_t* n_out);
// taps at either side of floor(tau) that an output can reach, with slack: ceil(num_zeros max(1, max R)) + 2
int warp_half_width(int num_zeros, int64_t F, const float* R);
// outputs no tap of which lies at or past in_avail (the count of DESIGN §7.22); floor(U[F]) once in_avail >= F hop
int64_t warp_ready(int hop, int64_t F, const float* R, const double* U, int num_zeros, int64_t in_avail);
// A table row (in the arena, upload_rows): one stream.  `win` is the fp32 window of the row's filter, [nwin] values
// followed by their [nwin] forward differences (the last one zero), nwin = 512 num_zeros + 1
struct WarpRow {
  const float* x;              // the decoded model-rate row
  int64_t n, in_avail;         // F hop; nothing at or past min(n, in_avail) is loaded
  const double* U;             // [F + 1]
  const float* R;              // [F]
  int32_t F, hop;
  PcmEnv env;                  // or kNoEnv: the sample at j is env_mul(x[j], env, j)
  int64_t out_first, out_end;
  float* out;                  // the warped row
  const float* win;
  int32_t num_zeros, hw;       // hw = warp_half_width of the row
};
// outputs [out_first, out_end) of every table row (n <= 65535) in one launch; max_count >= out_end - out_first of every
// row.  The caller guarantees out_end <= warp_ready of the row and the row's capacity.
void launch_warp_ranges(const WarpRow* rows, int n, int64_t max_count, hipStream_t s);

// ---------------------------------------------------------------- linear spectrogram (spectrogram.hip)
// |STFT| of spectrogram_torch(center=False) per row as if alone: (n_fft - hop) / 2 zeros each side, periodic
// Hann of length win centred in n_fft, [B, n_fft / 2 + 1, F] with frames past a row's length zero.
constexpr size_t kSpectrogramMaxLds = 80 * 1024;   // two workgroups per CU
int64_t spectrogram_frames(int64_t n, int n_fft, int hop);     // 0 if n + 2 pad < n_fft
size_t spectrogram_lds_bytes(int n_fft, int hop, int FB);
int spectrogram_block_frames(int n_fft, int hop);              // FB: frames per workgroup (a power of two)
// host, float64 rounded once: tw = e^{-2 pi i m / n_fft} as (re, im), m < n_fft; window [n_fft], zeros outside
// the centred span of win
void spectrogram_tables(int n_fft, int win, std::vector<float>* tw, std::vector<float>* window);
// x: fp32 (dtype 0) or int16 scaled by 1 / 32768 (dtype 1), [B, in_stride]; n_fft a power of two in [256, 4096]
void launch_spectrogram(const void* x, int dtype, const int64_t* valid, int B, int64_t in_stride, int n_fft, int hop,
                        const float* tw, const float* win, float* spec, int64_t F, int64_t* spec_lengths,
                        hipStream_t s);

// ---------------------------------------------------------------- forced alignment (align.hip)
// value[b, y, x] = neg_cent of models.py:670-675 for y < t_ys[b], x < t_xs[b] (other cells are not written):
// z_p [B, I, Tt]; m_p / logs_p [B, I, Ts] views with batch stride p_bstride (halves of the enc_p.proj output);
// value [B, Tt, Ts], Ts fastest.  Lengths are clamped to the tensors.
void launch_neg_cent(const float* z_p, const float* m_p, const float* logs_p, int64_t p_bstride, const int* t_ys,
                     const int* t_xs, float* value, int B, int I, int Tt, int Ts, hipStream_t s);
// maximum_path_each of monotonic_align/core.pyx on value [B, Tt, Ts] (left untouched; cells outside
// [t_ys[b], t_xs[b]) are not read): w [B, Ts] int32 frames per token (0 for x >= t_x), path [B, Tt, Ts] int32 or
// null, status [B] or null (0 ok, 1 t_x > t_y, 2 an empty side, 3 a length outside the tensors; such rows get
// w = 0, path = 0).  The decision bits of an utterance live in LDS when max_path_lds_bytes(Tt, Ts) != 0, else in
// bits_scratch (max_path_scratch_bytes(B, Tt, Ts) bytes).
constexpr int kMaxPathMaxTs = 1024;            // columns (tokens) the search kernel is built for
constexpr size_t kMaxPathLdsBytes = 64 * 1024;
bool max_path_supported(int Ts);
size_t max_path_lds_bytes(int Tt, int Ts);
size_t max_path_scratch_bytes(int B, int Tt, int Ts);
void launch_max_path(const float* value, const int* t_ys, const int* t_xs, int* w, int* path, int* status,
                     void* bits_scratch, int B, int Tt, int Ts, hipStream_t s);
// given non-negative integer durations w [B, T] (dtype 0 int32, 1 int64, 2 float32), masked by lens:
// w_ceil (or null), cum, ylen32 = max(sum, 1), ylen64 (or null; -1 under the rules of launch_durations, and for a
// negative or non-integer entry)
void launch_set_durations(const void* w, int dtype, const int* lens, float* w_ceil, int* cum, int* ylen32,
                          int64_t* ylen64, const int* bad, int B, int T, hipStream_t s);
// status[b] = bit 0: bad_x | bad_y | mas == 3, bit 1: mas == 1, bit 2: mas == 2 ; w_f = float(w_i) (either may be null)
void launch_align_status(const int* bad_x, const int* bad_y, const int* mas, int* status, float* w_f, const int* w_i,
                         int B, int T, hipStream_t s);

// z = (m + noise * noise_scale * exp(logs)) * mask   (PosteriorEncoder, models.py:245); stats = [B, 2I, T]
void launch_posterior_sample(const float* stats, const float* noise, const int* lens, float* z, int B,
                             int I, int T, hipStream_t s, float noise_scale = 1.f);

// ---------------------------------------------------------------- pooled voice conversion: table-reading variants
// One padded posterior run for many audio requests (capi.hip mbv_convert_rows), in the style of pooled admission
// above: each variant is the scalar kernel's own body behind a template flag.
struct ConvertRow {
  const void* wave;            // this row's samples, in place: fp32 (dtype 0) or int16 scaled by 1 / 32768 (dtype 1)
  int64_t samples;
  int dtype, frames;           // frames = spectrogram_frames(samples): the row's length in the run
  int sid_src, sid_tgt;
  // live conversion (mbv_convert_ranges): the row is the frame window [first, first + frames) of a recording of which
  // `samples` have arrived; the host guarantees that those frames are final.  0: the whole recording.
  int first, reserved;
};
// upload_rows' Extra of a ConvertRow table: the columns the existing launches read, lens (frames) and the two sids
struct ConvertRowCols {
  int* lens; int64_t* sid_src; int64_t* sid_tgt;
  __device__ void operator()(int i, const ConvertRow& k) const { lens[i] = k.frames; sid_src[i] = k.sid_src; sid_tgt[i] = k.sid_tgt; }
};
// launch_spectrogram for row b = rows[b].wave over rows[b].samples, written into dst [B, cpad, F] (cpad >=
// n_fft / 2 + 1: enc_q's channel-padded input): EXACT zeros in channels n_fft / 2 + 1 .. cpad and in frames at and
// past the row's own count, so every element of dst is written.  rows[b].first > 0: frame f of the row is frame
// first + f of the recording (samples [(first + f) hop - pad, .. + n_fft), zeros outside [0, samples))
void launch_spectrogram_rows(const ConvertRow* rows, int B, int n_fft, int hop, const float* tw, const float* win,
                             float* dst, int cpad, int64_t F, hipStream_t s);
// launch_posterior_sample with row b's noise block [I, rows[b].noise_stride] and rows[b].noise_scale; at scale 0
// (and behind the block, or behind rows[b].noise_len where that is set) the scalar kernel's null-noise branch
void launch_posterior_sample_rows(const float* stats, const AdmitSynRow* rows, const int* lens, float* z, int B,
                                  int I, int T, hipStream_t s);
void launch_sequence_mask(const int* lens, float* mask, int B, int T, hipStream_t s);   // commons.py:121
void launch_lens_to_i32(const int64_t* lens, int* out, int B, int T, int* bad, hipStream_t s);

// misc
void launch_fill(float* p, float v, int64_t n, hipStream_t s);
// trimmed decode: column-tile map of one conv geometry; limit_b = min(T, lens[b] * num + add) output frames.
// out: (B + 1) + B * ceil(T / BN) ints (launch_trim_map_ints)
size_t launch_trim_map_ints(int B, int T, int BN);
void launch_trim_map(const int* lens, int B, int num, int add, int T, int BN, int* out, hipStream_t s);
// "tail_once" (run_decoder): the same map for launches whose zero-input tail is computed once.  The donor — the row
// with the smallest lens[b], lowest index on ties — keeps every tile; every other row keeps the tiles that hold a
// column below S_b = min(T, lens[b] * num + reach), a prefix, and the tiles wholly inside [S_b, T) are dropped.  One
// launch builds up to kTailMapJobs maps (one workgroup each).  out: launch_tail_map_ints ints = the trim map, then
// the donor's index; *dropped (device, may be null) += the column tiles dropped by each map.
//
// Packed job (pack_gap > 0; the CONV_TAIL_PACK route): instead of dropping whole BN-column tiles, every
// row contributes its columns [0, S_b') to ONE packed column axis — S_b' = S_b rounded up to 32 and clamped to T,
// the donor [0, T) — each region followed by a gap of pack_gap = the launch's halo rounded up to 32 columns, and
// the conv kernel cuts its BN-column tiles over that axis.  Every 32-column block of the axis has one owner and is
// wholly output or wholly gap.  out (tail_pack_ints ints): [0] column tiles, [1] donor, [2] blocks in use, [3] 0,
// [4 .. 4 + B) S_b', then from tail_pack_entries_at(B) one int4 per block {row, first column, read limit, 1 =
// output}.  A gap block continues its row's column numbering: the columns below the read limit S_b' + pad_right
// are the row's right halo (real memory), everything from there on reads as zero — the next row's left padding.
// Blocks behind the last gap are empty (read limit 0); the table holds a tile's worth of them behind the last tile.
constexpr int kTailMapJobs = 24;
struct TailMapJob { int num, reach, T, BN; int* out; int pack_gap, pad_right; };
struct TailMapJobs { TailMapJob job[kTailMapJobs]; };
constexpr int kTailPackHdr = 4;
__host__ __device__ inline int tail_pack_gap(int halo) { return (halo + 31) & ~31; }
__host__ __device__ inline int tail_pack_entries_at(int B) { return (kTailPackHdr + B + 3) & ~3; }
__host__ __device__ inline int tail_pack_blocks(int B, int T, int gap, int BN) {       // entries the table holds
  const long per_tile = BN / 32, n = (long)B * ((T + 31) / 32 + gap / 32);
  return (int)((n + per_tile - 1) / per_tile * per_tile + per_tile);
}
__host__ __device__ inline size_t tail_pack_ints(int B, int T, int gap, int BN) {
  return (size_t)tail_pack_entries_at(B) + 4 * (size_t)tail_pack_blocks(B, T, gap, BN);
}
__host__ __device__ inline int tail_pack_sp(long len, int num, int reach, int T, bool donor) {
  if (donor) return T;
  long s = len * num + reach;
  s = s < 0 ? 0 : (s > T ? T : s);
  s = (s + 31) & ~31L;
  return (int)(s > T ? T : s);
}
__host__ __device__ inline int tail_pack_row_blocks(int sp, int gap) { return (sp + 31) / 32 + gap / 32; }
// the entries of row b, whose region starts at block `first`
__host__ __device__ inline void tail_pack_row(int* out, int B, int b, int first, int sp, int gap, int pad_right) {
  int* e = out + tail_pack_entries_at(B) + 4 * (long)first;
  const int n_out = (sp + 31) / 32, n = n_out + gap / 32;
  for (int k = 0; k < n; ++k, e += 4) { e[0] = b; e[1] = 32 * k; e[2] = sp + pad_right; e[3] = k < n_out; }
}
// header and the empty blocks behind the last row's gap, `used` = blocks in use
__host__ __device__ inline void tail_pack_finish(int* out, int B, int T, int gap, int BN, int donor, int used) {
  const int per_tile = BN / 32, cap = tail_pack_blocks(B, T, gap, BN);
  out[0] = (used + per_tile - 1) / per_tile; out[1] = donor; out[2] = used; out[3] = 0;
  int* e = out + tail_pack_entries_at(B) + 4 * (long)used;
  for (int k = used; k < cap; ++k, e += 4) { e[0] = 0; e[1] = 0; e[2] = 0; e[3] = 0; }
}
size_t launch_tail_map_ints(int B, int T, int BN);
void launch_tail_maps(const int* lens, int B, const TailMapJobs& jobs, int n, unsigned long long* dropped, hipStream_t s);
// y[b, m, c] = y[donor, m, c] for every column c of a tile that `map` (launch_tail_maps, tiles of BN columns) dropped
// from row b; y [B, M, T] with batch stride y_bstride.  16-byte accesses when T, y_bstride and y allow them.
// packed: `map` is a packed job's table, and row b gets the donor's columns [S_b', T)
void launch_tail_fill(float* y, int64_t y_bstride, int B, int M, int T, int BN, const int* map, hipStream_t s,
                      bool packed = false);
// row-exact ragged decode: n rows of a class, given by value from the host (rows / lens hold up to kRaggedChunk
// entries per launch) -> out[0 .. 4 stride): the source row of every class row, then its length at the three
// rates of the decoder (len, us len, us^2 len), entry first + i
constexpr int kRaggedChunk = 256;
struct RaggedRowsArg { int row[kRaggedChunk]; int len[kRaggedChunk]; };
void launch_ragged_rows(const RaggedRowsArg& r, int n, int first, int us, int* out, int stride, hipStream_t s);
// dst[i, c, t] = src[rows[i], c, t] for t < lens[i] (lens null: t < T): dst [n, C, T], src rows of C x src_rstride
void launch_gather_frames(const float* src, int64_t src_bstride, int src_rstride, const int* rows, const int* lens,
                          int n, int C, int T, float* dst, hipStream_t s);
// pooled ranged decode: upload_rows' Extra of a PoolRow table (kPoolChunk rows per launch), the window length of
// row i at the three rates of the decoder at lens[k stride + i], k < 3
constexpr int kPoolChunk = 64;
struct PoolRowLens {
  int* lens; int stride, us;
  __device__ void operator()(int i, const PoolRow& k) const {
    lens[i] = k.len; lens[stride + i] = us * k.len; lens[2 * stride + i] = us * us * k.len;
  }
};
// dst[i, c, t] = rows[i].z[c z_stride + wa + t] for t < rows[i].len (nothing outside a row's window is read; dst
// [n, C, T] behind a row's length is left as it is: every reader masks at the length); gdst[i, :] = rows[i].g[0 .. gin)
void launch_gather_windows(const PoolRow* rows, int n, int C, int T, float* dst, int gin, float* gdst, hipStream_t s);
// which column-tile width launch_conv1d will use for this conv (128 or 384; 0: a kernel without trim support)
int conv1d_trim_bn(const ConvArgs& a);

// ---------------------------------------------------------------- seeded noise (rng.hip, philox.h)
// One table row = one block of mbv_randn_blocks that has frames: dst[c stride + (t - first)] for c < channels,
// t in [first, first + count).  `quads` = the Philox blocks (four frames each) that hold one of those frames,
// `begin` = the prefix sum of channels * quads over the rows before it: the launch's grid runs over that sum.
struct RandnRow {
  float* dst;
  int64_t stride, begin;
  uint32_t seed_lo, seed_hi, purpose, row;
  int32_t first, count, quads, reserved;
};
constexpr int kRandnChunk = 64;     // rows per upload_rows launch: 3.5 KiB of kernel arguments
// every row of the table (in the arena: upload_rows) in one launch; total = the work items of all rows, > 0
void launch_randn_blocks(const RandnRow* rows, int n, int64_t total, hipStream_t s);
// the same values on the host (fp32 logf / sqrtf / sinf / cosf): frames [first, first + count) of channel c
void randn_host(uint64_t seed, uint32_t purpose, uint32_t row, uint32_t c, int64_t first, int64_t count, float* dst);

// ---------------------------------------------------------------- chunk seams (ops.hip)
// A table row (in the arena, upload_rows): one stream that decoded a chunk under a bounded look-ahead with a seam of
// `seam` samples.  The chunk's first `head_count` samples q[i] become p[i] w_p(i) + q[i] w_q(i), p = the stash (what the
// previous decode gave for the same samples), w_p = (float)(seam - i) inv, w_q = (float)(i + 1) inv, each product and
// the sum rounded once (no contraction); then the first `over_count` samples behind the chunk go to the stash.  head and
// over never overlap and no two rows share a stash or a head (checked by mbv_seam_rows).
struct SeamRow {
  float* head;                 // the chunk's first sample
  const float* over;           // the first sample behind the chunk
  float* stash;                // [seam]
  int32_t head_count, over_count, seam;
  float inv;                   // 1.0f / (float)(seam + 1)
};
constexpr int kSeamChunk = 64;      // rows per upload_rows launch: 64 x 40 bytes = 2.5 KiB of kernel arguments
constexpr int kSeamMax = 1 << 20;   // samples of a seam
// every row of the table in ONE launch: grid (ceil(max_seam / 256), n), 1 <= n <= 65535
void launch_seam_rows(const SeamRow* rows, int n, int max_seam, hipStream_t s);

// ---------------------------------------------------------------- loudness (loudness.hip)
// ITU-R BS.1770 integrated loudness of mono fp32 rows, measured in 100 ms segments of H samples.  The K-weighting
// cascade runs in transposed direct form II, state (s1, s2) of the shelf then (s1, s2) of the high-pass, in fp64:
//   y = b0 x + s1;  s1 = b1 x - a1 y + s2;  s2 = b2 x - a2 y          (per stage; the shelf's y is the high-pass's x)
// coef = shelf {b0, b1, b2, a1, a2}, high-pass {b0, b1, b2, a1, a2}; M = the H-step zero-input transition of that
// state, row-major; both built by kweighting_host in float64 and carried as kernel arguments.
struct LoudnessParams {
  double coef[10];
  double M[16];
  double z_abs;                // 10^((-70 + 0.691) / 10): the absolute gate on a block's mean square
  int32_t H, pad_;
};
// rate >= 1000 (checked by the caller): H = (rate + 5) / 10 and the tables above
void kweighting_host(int rate, LoudnessParams* p);
// One table row = segments [k0, k1) of one waveform row; the table lives in the arena (upload_rows).
struct LoudnessRow {
  const float* x;              // the row's samples
  const int64_t* valid;        // one int64 (clamped to [0, avail]), or null = avail
  int64_t avail;               // samples of x that exist: nothing at or past it is read
  int64_t k0, k1;              // k1 * H <= avail; segments at or past valid / H count as absent (their energy is 0)
  double* state;               // 4 doubles: s_{k0} in (ignored, zero, when k0 == 0), s_{min(k1, valid / H)} out
  double* energy;              // e_k for k in [k0, k1); entries [0, k0) are read by the gate pass
  float* L;                    // one float: the integrated loudness over segments [0, min(k1, valid / H))
};
constexpr int kLoudnessChunk = 32;   // rows per upload_rows launch: 2 KiB of kernel arguments
// every row of the table in ONE launch (one workgroup a row); n >= 1
void launch_loudness(const LoudnessRow* rows, int n, const LoudnessParams& p, hipStream_t s);

}  // namespace mbv
