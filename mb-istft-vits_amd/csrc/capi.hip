// C-ABI (include/mbistft_vits.h) + host orchestration of the infer path.
// No torch, no exceptions across the boundary; all device work is enqueued on
// the caller's stream.  Reference call stack being replaced: SURVEY §3.1.
#include "../../include/mbistft_vits.h"
#include "kernels.h"
#include "g711.h"

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
#include <string>
#include <vector>

using namespace mbv;

namespace {

constexpr int kWindow = 4;        // attentions.py:14
constexpr int kDpFilter = 256;    // models.py:652
constexpr int kFlowLayers = 4;    // models.py:647
constexpr int kFlowK = 5;
constexpr int kNFlows = 4;
constexpr float kLrelu = 0.1f;    // modules.py:17

static_assert(kVoiceSlots == MBV_SPEAKER_SLOTS && kBlendMax == MBV_BLEND_MAX, "the header states the kernels' conventions");

thread_local std::string g_create_error;

struct HostTensor {
  std::vector<float> data;
  std::vector<int64_t> shape;
  int64_t numel() const { int64_t n = 1; for (auto s : shape) n *= s; return n; }
};

struct PConv {              // packed conv living in the weight arena (offsets in floats)
  size_t w = 0, bias = 0;
  bool has_bias = false;
  int M = 0, Mpad = 0, Cin = 0, K = 1;
};
struct PVec { size_t off = 0; int n = 0; bool present = false; };

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// A scratch buffer and the number of times it has been laid out.  Every ensure / lay_out on it bumps `claim`: the caller
// overwrites the buffer from offset 0 and the buffer may move, so whatever pointed into it (an EncRun, a StageRef) is
// dead from then on.  That is the one rule for state kept between entries: it remembers the claim it was made under.
struct Scratch { char* p = nullptr; size_t bytes = 0; uint64_t claim = 0; };

// ... what was carved out of a Scratch (home null: nothing yet) under which claim, and whether it is still there
struct Carved { Scratch* home = nullptr; uint64_t claim = 0; bool live() const { return home && home->claim == claim; } };
struct StageRef : Carved { const float* ptr = nullptr; int64_t numel = 0; };

// one encode run: its shape and the tensors it left in its scratch `home`
struct EncRun : Carved {
  int B = 0, T = 0;
  bool has_g = false;
  float *x_enc = nullptr, *stats = nullptr, *logw = nullptr, *w_ceil = nullptr, *gvec = nullptr;
  int *lens32 = nullptr, *cum = nullptr, *ylen32 = nullptr;
  int* bad32 = nullptr;         // per-utterance flags (invalid id / length / sid)
  float* fit = nullptr;         // [2, B]: the factor and the status mbv_shape_durations left (stages fit_scale / fit_status)
  std::vector<float> scales;    // the length_scale the encode took: one value, or one per row (mbv_encode_rows)
  std::vector<int> t_text;      // mbv_encode_rows: every row's own text length (its tensors end there)
  bool rows = false;            // made by mbv_encode_rows
  Scratch own;                  // the buffer of a pooled slot >= 1 (slot 0 and the plain encode live in scrA)
};

// one launch of the decoder, as integers (decoder_table)
enum { DL_PRE = 0, DL_UP = 1, DL_C1 = 2, DL_C2 = 3, DL_POST = 4, DL_TAIL = 5 };
struct DecLaunch {
  int kind, stage, j, q;
  int Cin, M, K, dil, pad_left;
  int num, add, rate;
  int epi, convt_u, reflect1;
  int res, chan_add, res_chan_add, lens;
  int tk, tp;                      // DL_UP: kernel size and padding of the ConvTranspose1d itself
  int n_fft, hop, bands, taps;     // DL_TAIL: iSTFT (center = True) and the synthesis filter (taps, pad taps / 2)
};
inline int dec_us(const mbv_config& c) { return c.decoder == MBV_DEC_SINGLEBAND ? 8 : 4; }   // upsample stride of both stages
// ConvTranspose1d(k 16, stride u, padding (16 - u) / 2) as a phase conv over its input frames (EPI_CONVT)
constexpr int kConvtK = 16;
inline int convt_taps(int u) { return kConvtK / u + 1; }
inline int convt_pad_left(int u) { return u == 4 ? 2 : 1; }

}  // namespace

struct mbv_model {
  mbv_config cfg{};
  std::string err;
  std::map<std::string, HostTensor> raw;
  std::map<std::string, std::vector<int64_t>> expected;   // key -> shape
  bool finalized = false;
  size_t arena_used = 0;           // floats of the packed arena in use (darena may be larger after a reload)
  int64_t import_n = 0;
  const float* import_src = nullptr;   // do_finalize: lay the arena out from the config alone and fill it from this device buffer (mbv_import_arena)

  // weight arena
  std::vector<float> harena;
  float* darena = nullptr;
  size_t darena_floats = 0;
  float* darena_split = nullptr;   // conv_bf16 mode: the arena as [bf16 hi x 4 | bf16 mid x 4] slots (ensure_split_arena)
  size_t darena_split_floats = 0;
  bool split_valid = false;

  // packed weights
  struct Layer { PConv qkv, o, ffn1, ffn2; PVec ek, ev, g1, b1, g2, b2; };
  std::vector<Layer> enc;
  PVec emb;
  PConv enc_proj;
  PConv dp1, dp2;
  PVec dp_g1, dp_b1, dp_g2, dp_b2, dp_pw, dp_pb, dp_cw, dp_cb;
  // StochasticDurationPredictor (models.py:20-52), reverse direction only
  struct Dds { PVec sw[3], sb[3], g1[3], b1[3], g2[3], b2[3]; PConv c1[3]; };
  struct SdpFlow { PVec pre_w, pre_b; Dds dds; PConv proj; };
  struct Sdp { PConv pre, proj; Dds dds; SdpFlow flow[3]; PVec m, logs; float edge_const = 0.f; } sdp;
  struct Flow { PConv pre, post, in[kFlowLayers], rs[kFlowLayers], in16[kFlowLayers], rsp[kFlowLayers]; PVec cw, cb;
                PConv rspf[kFlowLayers];      // rspf: res/skip convs with `post` folded into their skip rows (wn_fused.hip, r03)
                PConv in16f0, pref; int Gi = 0; };   // `pre` folded too: layer 0's gate conv on [x0 ; mask] (composite weights), W_pre' for the residual rows
  Flow flow[kNFlows];
  PConv conv_pre, conv_post;
  static constexpr int kEncQLayers = 16;     // models.py:646
  struct EncQ { PConv pre, proj, in[kEncQLayers], rs[kEncQLayers], in16[kEncQLayers], rsp[kEncQLayers]; PVec cw, cb; int cin_pad = 0; } encq;
  PConv upc[2];              // ups (ConvTranspose1d k 16, stride us) as (16/us + 1)-tap convs over the output phases (EPI_CONVT)
  struct RB { PConv c1[3], c2[3]; PVec cw, cb; } rb[6];
  PVec emb_g;
  PVec filt;                 // synthesis-bank table of the fused iSTFT+PQMF kernel (352 floats)

  // scratch
  float* conv_ws = nullptr; size_t conv_ws_floats = 0;   // split-K partials of small conv launches
  unsigned* conv_cnt = nullptr; int conv_ncnt = 0;        // one ticket counter per tile (zero between launches)
  int wn_fused = 1;           // MBV_WN_FUSED=0: the two-launch WN layer (gate conv, then res/skip conv)
  int splitk = 0;             // option "splitk": split-K for small conv launches (default: MBV_CONV_SPLITK or 0)
  Scratch scrA, scrB;
  float* user_tab = nullptr;   // polyphase table of the stand-alone mbv_istft_pqmf entry
  unsigned* peak_buf = nullptr; int peak_cap = 0;   // per-utterance peaks of mbv_pcm16
  struct ResampleBank { float* d = nullptr; ResampleGeom g{}; };
  std::map<std::array<int, 3>, ResampleBank> resample_banks;   // (L, M, filter) -> fp32 bank on the device (mbv_resample)
  struct SpectrogramTables { float* tw = nullptr; float* win = nullptr; };
  std::map<std::array<int, 2>, SpectrogramTables> spec_tables;   // (n_fft, win) -> twiddles + window (mbv_spectrogram)
  bool user_tab_is_pqmf = false;
  int xpost_F = 1;             // frames per row of the last x_post stage tensor
  int xpost_rows = 72;         // 72 (4 bands x 18) or 18 (single band)
  int exact_math = 0;          // MBV_ISTFT_EXACT=1: libm transcendentals in the iSTFT kernel
  int trim = 0;                    // option "trim": opt-in trimmed decode (run_decoder)
  int tail_once = 1;               // option "tail_once": the zero-input tail of a padded batch computed once (run_decoder)
  unsigned long long* tail_cnt = nullptr;   // device: column tiles dropped by tail maps since mbv_create (mbv_tail_dropped)
  std::vector<DecLaunch> dec_table;   // decoder_table(cfg), built once at mbv_create
  std::vector<int> ragged_first;   // row-exact ragged decode: first length of every class up to ragged_scanned (ragged_classes)
  int ragged_scanned = 0, ragged_splitk = -1;
  int64_t decoder_runs = 0;        // run_decoder calls since mbv_create (mbv_decoder_runs)
  int64_t wire_runs = 0;           // resample / int16 launches of the ranged and the pooled wire step (mbv_wire_runs)
  int64_t input_runs = 0;          // launches of the live-input resampler (mbv_input_runs)
  int64_t warp_runs = 0;           // launches of the time-warp kernel (mbv_warp_runs)
  int64_t seam_runs = 0;           // launches of the chunk-seam kernel (mbv_seam_runs)
  int64_t text_runs = 0;           // mbv_take_tokens_rows + mbv_expand_ranges launches (mbv_text_runs)
  int64_t flow_runs = 0;           // flow runs of mbv_flow_ranges (mbv_flow_runs)
  float* warp_win[2] = {nullptr, nullptr};   // filter -> fp32 window and its differences on the device (mbv_warp_ranges)
  // blended voices (mbv_speakers_define): the rows, the defined words and the definition table on the device, all
  // allocated by the first definition and outside the weight arena; `voices` is every slot's host copy
  struct Voice { bool defined = false, vector = false; VoiceDef def{}; };
  std::vector<Voice> voices;       // empty until the first definition, then kVoiceSlots entries
  float* voice_rows = nullptr;     // [kVoiceSlots][gin]
  int* voice_defined = nullptr;    // [kVoiceSlots]
  VoiceDef* voice_defs = nullptr;  // [kVoiceSlots], the table of the launch in flight
  int64_t speaker_runs = 0;        // launches of the blend kernel (mbv_speaker_runs)
  // the second table of every emb_g gather: empty until a voice was defined
  VoiceTable voice_table() const { return VoiceTable{voice_rows, voice_defined, voice_rows ? kVoiceSlots : 0}; }
  // a speaker id a host-side check accepts: a row of emb_g or a defined voice
  bool speaker_ok(long long sid) const {
    const long long ns = cfg.n_speakers;
    return sid >= 0 && (sid < ns || (sid - ns < (long long)voices.size() && voices[(size_t)(sid - ns)].defined));
  }
  int64_t noise_runs = 0;          // mbv_randn_blocks launches (mbv_noise_runs)
  int64_t loudness_runs = 0;       // launches of the loudness kernel (mbv_loudness_runs)
  std::map<int, LoudnessParams> loudness_params;    // rate -> K-weighting tables (built once a rate, host only)
  std::map<const void*, int64_t> loudness_next;     // state buffer of a measured row -> its next segment
  Scratch noise_tab;               // mbv_randn_blocks' table: its own buffer, so that a fill between an encode and its
                                   // synthesize disturbs no scratch
  int64_t encoder_runs = 0;        // run_text_encoder calls since mbv_create (mbv_encoder_runs)
  int64_t shape_runs = 0;          // launches of the prosody kernel (mbv_shape_runs)
  int64_t gain_runs = 0;           // launches of the frame-gain kernel (mbv_gain_runs)
  int64_t converter_runs = 0;      // posterior-encoder runs of mbv_convert_rows since mbv_create (mbv_converter_runs)
  int64_t xpost_chunk_bytes = 0;   // option "xpost_chunk_bytes": sub-batch cap of conv_post + iSTFT (0: 2 GiB - 1)

  std::map<std::string, StageRef> stages;
  void stage(const char* name, const float* ptr, int64_t numel, Scratch& home) { stages[name] = StageRef{{&home, home.claim}, ptr, numel}; }
  // runs[0] is what mbv_encode and mbv_encode_rows(slot 0) write, in scrA; every further slot of the pooled admission
  // keeps its run in a buffer of its own.  cur: the run the plain entries act on, the one encoded or synthesised last
  static constexpr int kSlots = 64;
  EncRun runs[kSlots];
  int cur = -1;

  static constexpr int kEvRing = 8;
  hipEvent_t evr[kEvRing][7]{};    // stage events of the last kEvRing encode (+ synthesize) calls
  hipEvent_t* ev = evr[0];         // ... of the current call
  int64_t ticket = 0;              // calls of mbv_encode so far; slot = ticket % kEvRing
  bool evr_a[kEvRing]{}, evr_b[kEvRing]{};
  hipEvent_t evk[3]{};          // decoder start / before istft / after istft
  // the three ResBlocks of a decoder stage on three streams when one of them cannot fill the chip (run_decoder)
  hipStream_t aux[2]{};
  hipEvent_t ev_fork{}, ev_rb[3]{};
  bool aux_ok = false;
  int dec_streams = 1;          // option "dec_streams" / MBV_DEC_STREAMS: 0 = always one stream
  int conv_bf16 = 0;            // option "conv_bf16" / MBV_CONV_BF16: 3 = opt-in split-bf16 arithmetic in the large conv launches
  bool ev_ok = false, ev_a = false, ev_b = false, evk_set = false;
  bool evk_split = false;          // the last decoder run split its batch: evk[1] does not separate conv stack and iSTFT

  int fail(const char* fmt, ...) {
    char buf[1024];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
    err = buf;
    return 1;
  }
  const float* W(size_t off) const { return darena + off; }
  const float* Wsplit(size_t off) const { return (conv_bf16 == 3 && split_valid) ? darena_split + off : nullptr; }
};

#define HIPCHK(m, call)                                                              \
  do {                                                                               \
    hipError_t e_ = (call);                                                          \
    if (e_ != hipSuccess) return (m)->fail("%s failed: %s", #call, hipGetErrorString(e_)); \
  } while (0)

namespace {

// conv_bf16 mode: (re)build the split copy of the weight arena (ops.hip launch_split_planes)
int ensure_split_arena(mbv_model* m, hipStream_t stream) {
  if (m->split_valid) return 0;
  if (!m->darena) return m->fail("conv_bf16: no weights on the device yet");
  if (m->darena_split && m->darena_split_floats < m->darena_floats) {
    HIPCHK(m, hipFree(m->darena_split));
    m->darena_split = nullptr;
  }
  if (!m->darena_split) {
    HIPCHK(m, hipMalloc((void**)&m->darena_split, m->darena_floats * sizeof(float)));
    m->darena_split_floats = m->darena_floats;
  }
  launch_split_planes(m->darena, m->darena_split, m->darena_floats, stream);
  HIPCHK(m, hipStreamSynchronize(stream));
  m->split_valid = true;
  return 0;
}

// Blended voices: the validated definitions go up as a table and ONE launch writes their rows (ops.hip
// speaker_blend_kernel).  The buffers exist from the first definition on.
int blend_voices(mbv_model* m, const std::vector<VoiceDef>& defs, hipStream_t s) {
  if (defs.empty()) return 0;
  const int gin = m->cfg.gin_channels;
  if (!m->voice_rows) {
    float* rows = nullptr; int* defined = nullptr; VoiceDef* tab = nullptr;
    if (hipMalloc((void**)&rows, (size_t)kVoiceSlots * gin * sizeof(float)) != hipSuccess ||
        hipMalloc((void**)&defined, kVoiceSlots * sizeof(int)) != hipSuccess ||
        hipMalloc((void**)&tab, kVoiceSlots * sizeof(VoiceDef)) != hipSuccess ||
        hipMemsetAsync(rows, 0, (size_t)kVoiceSlots * gin * sizeof(float), s) != hipSuccess ||
        hipMemsetAsync(defined, 0, kVoiceSlots * sizeof(int), s) != hipSuccess) {
      if (rows) (void)hipFree(rows);
      if (defined) (void)hipFree(defined);
      if (tab) (void)hipFree(tab);
      return m->fail("hipMalloc of the voice table failed");
    }
    m->voice_rows = rows; m->voice_defined = defined; m->voice_defs = tab;
  }
  upload_rows<kVoiceChunk>(defs.size(), m->voice_defs, s, [&](size_t i) { return defs[i]; });
  launch_speaker_blend(m->voice_defs, (int)defs.size(), m->W(m->emb_g.off), m->voice_rows, m->voice_defined, gin, s);
  ++m->speaker_runs;
  HIPCHK(m, hipGetLastError());
  return 0;
}
// after a weight refresh: every blend again from the new table, in one launch (vector voices stay as given)
int reblend_voices(mbv_model* m, hipStream_t s) {
  std::vector<VoiceDef> defs;
  for (const auto& v : m->voices)
    if (v.defined && !v.vector) defs.push_back(v.def);
  return blend_voices(m, defs, s);
}

// Every entry point runs on the model's device and hands the caller's current device back on
// every exit path (a process may host models on several GPUs; hipSetDevice is per host thread).
struct DeviceGuard {
  int prev = -1;
  bool ok = true;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != dev) ok = hipSetDevice(dev) == hipSuccess; else prev = -1;
  }
  ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
  DeviceGuard(const DeviceGuard&) = delete;
  DeviceGuard& operator=(const DeviceGuard&) = delete;
};
#define DEVICE_GUARD(m)                                                          \
  DeviceGuard dev_guard_((m)->cfg.device);                                       \
  if (!dev_guard_.ok) return (m)->fail("hipSetDevice(%d) failed", (m)->cfg.device)

// ------------------------------------------------------------------ key table
void add_key(mbv_model* m, const std::string& k, std::initializer_list<int64_t> shape) {
  m->expected[k] = std::vector<int64_t>(shape);
}

void build_expected(mbv_model* m) {
  const mbv_config& c = m->cfg;
  const int H = c.hidden_channels, I = c.inter_channels, Fc = c.filter_channels;
  const int dk = H / c.n_heads, gin = c.gin_channels, C0 = c.upsample_initial_channel;
  char p[160];
  add_key(m, "enc_p.emb.weight", {c.n_vocab, H});
  for (int i = 0; i < c.n_layers; ++i) {
    snprintf(p, sizeof p, "enc_p.encoder.attn_layers.%d.", i);
    add_key(m, std::string(p) + "emb_rel_k", {1, 2 * kWindow + 1, dk});
    add_key(m, std::string(p) + "emb_rel_v", {1, 2 * kWindow + 1, dk});
    for (const char* n : {"conv_q", "conv_k", "conv_v", "conv_o"}) {
      add_key(m, std::string(p) + n + ".weight", {H, H, 1});
      add_key(m, std::string(p) + n + ".bias", {H});
    }
    for (int j = 1; j <= 2; ++j) {
      snprintf(p, sizeof p, "enc_p.encoder.norm_layers_%d.%d.", j, i);
      add_key(m, std::string(p) + "gamma", {H});
      add_key(m, std::string(p) + "beta", {H});
    }
    snprintf(p, sizeof p, "enc_p.encoder.ffn_layers.%d.", i);
    add_key(m, std::string(p) + "conv_1.weight", {Fc, H, c.kernel_size});
    add_key(m, std::string(p) + "conv_1.bias", {Fc});
    add_key(m, std::string(p) + "conv_2.weight", {H, Fc, c.kernel_size});
    add_key(m, std::string(p) + "conv_2.bias", {H});
  }
  add_key(m, "enc_p.proj.weight", {2 * I, H, 1});
  add_key(m, "enc_p.proj.bias", {2 * I});
  if (c.decoder == MBV_DEC_MULTISTREAM) add_key(m, "dec.updown_filter", {4, 4, 4});
  add_key(m, "dec.conv_pre.bias", {C0});
  add_key(m, "dec.conv_pre.weight_g", {C0, 1, 1});
  add_key(m, "dec.conv_pre.weight_v", {C0, I, 7});
  const bool sb = c.decoder == MBV_DEC_SINGLEBAND;
  const int post_rows = sb ? 18 : 72;
  const char* post_name = sb ? "dec.conv_post" : "dec.subband_conv_post";
  for (int i = 0; i < 2; ++i) {
    const int cin = C0 >> i, cout = C0 >> (i + 1);
    snprintf(p, sizeof p, "dec.ups.%d.", i);
    add_key(m, std::string(p) + "bias", {cout});
    add_key(m, std::string(p) + "weight_g", {cin, 1, 1});
    add_key(m, std::string(p) + "weight_v", {cin, cout, 16});
  }
  for (int i = 0; i < 2; ++i) {
    const int ch = C0 >> (i + 1);
    for (int j = 0; j < 3; ++j) {
      const int k = c.resblock_kernel_sizes[j];
      const bool rb1 = c.resblock_type == 1;
      for (const char* grp : {"convs1", "convs2", "convs"}) {
        const bool is2 = std::strcmp(grp, "convs") == 0;
        if (is2 == rb1) continue;                      // ResBlock1: convs1/convs2 x3, ResBlock2: convs x2
        for (int q = 0; q < (rb1 ? 3 : 2); ++q) {
          snprintf(p, sizeof p, "dec.resblocks.%d.%s.%d.", i * 3 + j, grp, q);
          add_key(m, std::string(p) + "bias", {ch});
          add_key(m, std::string(p) + "weight_g", {ch, 1, 1});
          add_key(m, std::string(p) + "weight_v", {ch, ch, k});
        }
      }
      if (gin) {
        snprintf(p, sizeof p, "dec.resblocks.%d.cond.", i * 3 + j);
        add_key(m, std::string(p) + "weight", {ch, gin, 1});
        add_key(m, std::string(p) + "bias", {ch});
      }
    }
  }
  add_key(m, std::string(post_name) + ".bias", {post_rows});
  add_key(m, std::string(post_name) + ".weight_g", {post_rows, 1, 1});
  add_key(m, std::string(post_name) + ".weight_v", {post_rows, C0 >> 2, 7});
  if (c.decoder == MBV_DEC_MULTISTREAM) {
    add_key(m, "dec.multistream_conv_post.weight_g", {1, 1, 1});
    add_key(m, "dec.multistream_conv_post.weight_v", {1, 4, 63});
  }
  // enc_q (PosteriorEncoder, models.py:217-246): only voice_conversion reads it, but it is part of
  // every reference checkpoint, so the keys are accepted and required like the rest
  add_key(m, "enc_q.pre.weight", {H, c.spec_channels, 1});
  add_key(m, "enc_q.pre.bias", {H});
  for (int l = 0; l < mbv_model::kEncQLayers; ++l) {
    const int rs = l < mbv_model::kEncQLayers - 1 ? 2 * H : H;
    char q[64];
    snprintf(q, sizeof q, "enc_q.enc.in_layers.%d.", l);
    add_key(m, std::string(q) + "bias", {2 * H});
    add_key(m, std::string(q) + "weight_g", {2 * H, 1, 1});
    add_key(m, std::string(q) + "weight_v", {2 * H, H, 5});
    snprintf(q, sizeof q, "enc_q.enc.res_skip_layers.%d.", l);
    add_key(m, std::string(q) + "bias", {rs});
    add_key(m, std::string(q) + "weight_g", {rs, 1, 1});
    add_key(m, std::string(q) + "weight_v", {rs, H, 1});
  }
  if (gin) {
    add_key(m, "enc_q.enc.cond_layer.bias", {2 * H * mbv_model::kEncQLayers});
    add_key(m, "enc_q.enc.cond_layer.weight_g", {2 * H * mbv_model::kEncQLayers, 1, 1});
    add_key(m, "enc_q.enc.cond_layer.weight_v", {2 * H * mbv_model::kEncQLayers, gin, 1});
  }
  add_key(m, "enc_q.proj.weight", {2 * I, H, 1});
  add_key(m, "enc_q.proj.bias", {2 * I});
  for (int f = 0; f < kNFlows; ++f) {
    snprintf(p, sizeof p, "flow.flows.%d.", 2 * f);
    const std::string s(p);
    add_key(m, s + "pre.weight", {H, I / 2, 1});
    add_key(m, s + "pre.bias", {H});
    for (int l = 0; l < kFlowLayers; ++l) {
      const int rs = l < kFlowLayers - 1 ? 2 * H : H;
      char q[64];
      snprintf(q, sizeof q, "enc.in_layers.%d.", l);
      add_key(m, s + q + "bias", {2 * H});
      add_key(m, s + q + "weight_g", {2 * H, 1, 1});
      add_key(m, s + q + "weight_v", {2 * H, H, kFlowK});
      snprintf(q, sizeof q, "enc.res_skip_layers.%d.", l);
      add_key(m, s + q + "bias", {rs});
      add_key(m, s + q + "weight_g", {rs, 1, 1});
      add_key(m, s + q + "weight_v", {rs, H, 1});
    }
    if (gin) {
      add_key(m, s + "enc.cond_layer.bias", {2 * H * kFlowLayers});
      add_key(m, s + "enc.cond_layer.weight_g", {2 * H * kFlowLayers, 1, 1});
      add_key(m, s + "enc.cond_layer.weight_v", {2 * H * kFlowLayers, gin, 1});
    }
    add_key(m, s + "post.weight", {I / 2, H, 1});
    add_key(m, s + "post.bias", {I / 2});
  }
  if (c.use_sdp) {
    // models.py:20-52 (filter_channels := in_channels); post_* is training-only but part of the checkpoint
    auto dds = [&](const std::string& q) {
      for (int i = 0; i < 3; ++i) {
        const std::string n = std::to_string(i);
        add_key(m, q + "convs_sep." + n + ".weight", {H, 1, 3});
        add_key(m, q + "convs_sep." + n + ".bias", {H});
        add_key(m, q + "convs_1x1." + n + ".weight", {H, H, 1});
        add_key(m, q + "convs_1x1." + n + ".bias", {H});
        for (const char* g : {"norms_1.", "norms_2."}) {
          add_key(m, q + g + n + ".gamma", {H});
          add_key(m, q + g + n + ".beta", {H});
        }
      }
    };
    auto flows = [&](const std::string& q) {
      add_key(m, q + "0.m", {2, 1});
      add_key(m, q + "0.logs", {2, 1});
      for (int f = 1; f <= 7; f += 2) {
        const std::string r = q + std::to_string(f) + ".";
        add_key(m, r + "pre.weight", {H, 1, 1});
        add_key(m, r + "pre.bias", {H});
        dds(r + "convs.");
        add_key(m, r + "proj.weight", {29, H, 1});
        add_key(m, r + "proj.bias", {29});
      }
    };
    flows("dp.flows.");
    add_key(m, "dp.post_pre.weight", {H, 1, 1});
    add_key(m, "dp.post_pre.bias", {H});
    add_key(m, "dp.post_proj.weight", {H, H, 1});
    add_key(m, "dp.post_proj.bias", {H});
    dds("dp.post_convs.");
    flows("dp.post_flows.");
    add_key(m, "dp.pre.weight", {H, H, 1});
    add_key(m, "dp.pre.bias", {H});
    add_key(m, "dp.proj.weight", {H, H, 1});
    add_key(m, "dp.proj.bias", {H});
    dds("dp.convs.");
  } else {
    add_key(m, "dp.conv_1.weight", {kDpFilter, H, 3});
    add_key(m, "dp.conv_1.bias", {kDpFilter});
    add_key(m, "dp.norm_1.gamma", {kDpFilter});
    add_key(m, "dp.norm_1.beta", {kDpFilter});
    add_key(m, "dp.conv_2.weight", {kDpFilter, kDpFilter, 3});
    add_key(m, "dp.conv_2.bias", {kDpFilter});
    add_key(m, "dp.norm_2.gamma", {kDpFilter});
    add_key(m, "dp.norm_2.beta", {kDpFilter});
    add_key(m, "dp.proj.weight", {1, kDpFilter, 1});
    add_key(m, "dp.proj.bias", {1});
  }
  if (gin) {
    add_key(m, "dp.cond.weight", {H, gin, 1});
    add_key(m, "dp.cond.bias", {H});
  }
  if (c.n_speakers > 1) add_key(m, "emb_g.weight", {c.n_speakers, gin});
}

// ------------------------------------------------------------------ packing
// k-interleaved weight order the conv kernel copies verbatim into LDS (conv1d.hip):
//   Wp[tap][Cin/8][h = ci & 1][Mpad][s = (ci % 8) / 2]
inline size_t conv_pack_index(int tap, int ci, int m, int Cin, int Mpad) {
  return ((((size_t)tap * (Cin / 8) + ci / 8) * 2 + (ci & 1)) * Mpad + m) * 4 + ((ci & 7) >> 1);
}

// w [Cout][Cin][K] (reference layout) -> dst [K * Cin * Mpad] packed; rows[mrow] -> source output channel (or -1 =
// zero row), cin_map[ci] -> source ci (nullptr: identity)
void pack_conv_rows(const float* w, int Cin, int K, const int* rows, int M, const int* cin_map, int Mpad, float* dst) {
  for (int k = 0; k < K; ++k)
    for (int ci = 0; ci < Cin; ++ci) {
      const int sci = cin_map ? cin_map[ci] : ci;
      for (int mrow = 0; mrow < M; ++mrow) {
        const int co = rows[mrow];
        dst[conv_pack_index(k, ci, mrow, Cin, Mpad)] = co < 0 ? 0.f : w[((size_t)co * Cin + sci) * K + k];
      }
    }
}

// ConvTranspose1d(k = 16, stride us, padding (16 - us) / 2), w [Cin][Cout][16] (reference layout), as ONE
// (16/us + 1)-tap conv on the conv1d kernel (EPI_CONVT):
//   y[co, us m + r] = sum_ci sum_j W[ci][co][kr + us j] x[ci, m + sh_r - j],  kr = (r + pad) % us,
//   sh_r = (r + pad - kr) / us;  tap tau reads x[m - pl + tau]  ->  j = sh_r + pl - tau, with
//   pl = tpp - 1 - pad / us  (us 4: 5 taps, pl 2;  us 8: 3 taps, pl 1).
// Packed rows: groups of 64 = 64/us channels x [first us/2 phases (32 rows) | last us/2 phases
// (32 rows)], row k of a half = channel k / (us/2), phase k % (us/2).  The last tap is zero for
// the first half, tap 0 for the second; the kernel skips those MFMAs.
// dst_w [(16/us + 1) * Cin * Mpad] packed (Mpad >= us * Cout), dst_bias [us * Cout] in row order.
void pack_convt_rows(const float* w, const float* bias, int Cin, int Cout, int us, int Mpad, float* dst_w,
                     float* dst_bias) {
  const int tpp = kConvtK / us, pad = (kConvtK - us) / 2;
  const int Mp = us * Cout, PH = us / 2, CG = 32 / PH, Kc = convt_taps(us), pl = tpp - 1 - pad / us;   // (pl = convt_pad_left(us))
  for (int row = 0; row < Mp; ++row) {
    const int grp = row / 64, half = (row % 64) / 32, k = row % 32;
    const int co = grp * CG + k / PH, r = half * PH + k % PH;
    const int kr = (r + pad) % us, sh = (r + pad - kr) / us;
    dst_bias[row] = bias[co];
    for (int tau = 0; tau < Kc; ++tau) {
      const int j = sh + pl - tau;
      for (int ci = 0; ci < Cin; ++ci)
        dst_w[conv_pack_index(tau, ci, row, Cin, Mpad)] =
            (j >= 0 && j < tpp) ? w[((size_t)ci * Cout + co) * 16 + kr + us * j] : 0.f;
    }
  }
}

struct Packer {
  mbv_model* m;
  std::vector<float>& a;
  size_t alloc(size_t n) {
    const size_t off = align_up(a.size(), 64);
    a.resize(off + n, 0.f);
    return off;
  }
  const HostTensor& t(const std::string& k) const { return m->raw.at(k); }
  bool has(const std::string& k) const { return m->raw.count(k) != 0; }

  // conv weight [d0, d1, K] as stored; folds weight-norm over dim 0 if *_v/_g
  std::vector<float> dense(const std::string& prefix) const {
    if (has(prefix + ".weight")) return t(prefix + ".weight").data;
    const HostTensor& v = t(prefix + ".weight_v");
    const HostTensor& g = t(prefix + ".weight_g");
    const int64_t d0 = v.shape[0], inner = v.numel() / d0;
    std::vector<float> w(v.data.size());
    if (m->import_src) return w;                   // layout-only pass: the contents come from the imported arena
    for (int64_t i = 0; i < d0; ++i) {
      double n2 = 0;
      for (int64_t j = 0; j < inner; ++j) { const double x = v.data[i * inner + j]; n2 += x * x; }
      const float scale = g.data[i] / (float)std::sqrt(n2);
      for (int64_t j = 0; j < inner; ++j) w[i * inner + j] = v.data[i * inner + j] * scale;
    }
    return w;
  }
  PVec vec(const std::string& k) {
    PVec r;
    if (!has(k)) return r;
    const HostTensor& x = t(k);
    r.off = alloc(x.data.size());
    r.n = (int)x.data.size();
    r.present = true;
    std::memcpy(&a[r.off], x.data.data(), x.data.size() * sizeof(float));
    return r;
  }
  PVec vec_data(const std::vector<float>& d) {
    PVec r;
    r.off = alloc(d.size()); r.n = (int)d.size(); r.present = true;
    std::memcpy(&a[r.off], d.data(), d.size() * sizeof(float));
    return r;
  }
  // generic conv: rows[m] -> source output channel (or -1 = zero row), cin_map[ci] -> source ci
  PConv conv(const std::vector<float>& w, int Cout, int Cin, int K, const std::vector<int>& rows,
             const std::vector<int>& cin_map, const std::vector<float>* bias,
             const std::vector<int>* bias_rows) {
    PConv p;
    p.M = (int)rows.size(); p.Mpad = (int)align_up(p.M, 128); p.Cin = Cin; p.K = K;
    p.w = alloc((size_t)K * Cin * p.Mpad);
    pack_conv_rows(w.data(), Cin, K, rows.data(), p.M, cin_map.empty() ? nullptr : cin_map.data(), p.Mpad, &a[p.w]);
    if (bias) {
      const std::vector<int>& br = bias_rows ? *bias_rows : rows;
      p.bias = alloc(br.size());
      p.has_bias = true;
      for (size_t i = 0; i < br.size(); ++i) a[p.bias + i] = br[i] < 0 ? 0.f : (*bias)[br[i]];
    }
    (void)Cout;
    return p;
  }
  PConv conv_plain(const std::string& prefix) {
    const std::vector<float> w = dense(prefix);
    const auto& sh = has(prefix + ".weight") ? t(prefix + ".weight").shape : t(prefix + ".weight_v").shape;
    const int Cout = (int)sh[0], Cin = (int)sh[1], K = (int)sh[2];
    std::vector<int> rows(Cout);
    for (int i = 0; i < Cout; ++i) rows[i] = i;
    const std::vector<float>* b = has(prefix + ".bias") ? &t(prefix + ".bias").data : nullptr;
    return conv(w, Cout, Cin, K, rows, {}, b, nullptr);
  }
};

// WN in_layer (modules.py:130-135): gated packing, 32-row tiles alternate tanh half / sigmoid half
PConv pack_gated(Packer& P, const std::string& prefix, int H, int K) {
  const std::vector<float> w = P.dense(prefix);
  std::vector<int> rows(2 * H), brows(2 * H);
  for (int ch = 0; ch < H; ++ch) {
    rows[(ch / 32) * 64 + (ch % 32)] = ch;
    rows[(ch / 32) * 64 + 32 + (ch % 32)] = H + ch;
  }
  for (int r = 0; r < 2 * H; ++r) brows[r] = r;        // bias stays in reference order
  return P.conv(w, 2 * H, H, K, rows, {}, &P.t(prefix + ".bias").data, &brows);
}

// The same in_layer for the fused WN kernel (wn_fused.hip): 32-row tiles of
// [tanh 16t..16t+7 | sigmoid 16t..16t+7 | tanh 16t+8..16t+15 | sigmoid 16t+8..16t+15], which puts the
// tanh and the sigmoid row of a channel into the same lane of the 32x32 accumulator.  The bias
// stays in reference order.
PConv pack_gated16(Packer& P, const std::string& prefix, int H, int K) {
  const std::vector<float> w = P.dense(prefix);
  std::vector<int> rows(2 * H), brows(2 * H);
  for (int r = 0; r < 2 * H; ++r) {
    const int tile = r / 32, rho = r % 32;
    const int ch = tile * 16 + (rho & 7) + 8 * (rho >> 4);
    rows[r] = (rho & 8) ? H + ch : ch;
    brows[r] = r;
  }
  return P.conv(w, 2 * H, H, K, rows, {}, &P.t(prefix + ".bias").data, &brows);
}
// res_skip 1x1 with the input channels in the order the gated tile leaves the accumulators
PConv pack_rs_permuted(Packer& P, const std::string& prefix) {
  const std::vector<float> w = P.dense(prefix);
  const auto& sh = P.t(prefix + ".weight_v").shape;
  const int Cout = (int)sh[0], Cin = (int)sh[1];
  std::vector<int> rows(Cout), cmap(Cin);
  for (int i = 0; i < Cout; ++i) rows[i] = i;
  for (int ci = 0; ci < Cin; ++ci) cmap[ci] = 8 * (ci / 8) + 4 * (ci & 1) + ((ci & 7) >> 1);
  return P.conv(w, Cout, Cin, 1, rows, cmap, &P.t(prefix + ".bias").data, nullptr);
}

// modified Bessel I0 (power series; converges fast for x <= 9)
double bessel_i0(double x) {
  double sum = 1.0, term = 1.0;
  const double q = x * x / 4.0;
  for (int k = 1; k < 200; ++k) {
    term *= q / ((double)k * k);
    sum += term;
    if (term < 1e-18 * sum) break;
  }
  return sum;
}

// pqmf.py:15-43: Kaiser-windowed sinc prototype (taps 62, cutoff 0.15, beta 9), float64
std::vector<double> pqmf_prototype() {
  const int taps = 62;
  const double cutoff = 0.15, beta = 9.0;
  std::vector<double> proto(taps + 1);
  for (int n = 0; n <= taps; ++n) {
    const double c = n - 0.5 * taps;
    const double h = n == taps / 2 ? cutoff : std::sin(M_PI * cutoff * c) / (M_PI * c);
    const double alpha = taps / 2.0;
    const double r = (n - alpha) / alpha;
    proto[n] = h * bessel_i0(beta * std::sqrt(std::max(0.0, 1.0 - r * r))) / bessel_i0(beta);
  }
  return proto;
}

// pqmf.py:53-75: cosine-modulated synthesis bank h_syn[k][n], float64 -> float32
std::vector<float> pqmf_synthesis_filter() {
  const int taps = 62, K = 4;
  const std::vector<double> proto = pqmf_prototype();
  std::vector<float> h(K * (taps + 1));
  for (int k = 0; k < K; ++k)
    for (int n = 0; n <= taps; ++n) {
      const double sign = (k % 2 == 0) ? 1.0 : -1.0;
      h[k * (taps + 1) + n] = (float)(2.0 * proto[n] *
          std::cos((2 * k + 1) * (M_PI / (2.0 * K)) * (n - (taps - 1) / 2.0) - sign * M_PI / 4.0));
    }
  return h;
}

// Device table of the fused iSTFT+PQMF kernel (352 floats, layout in istft_pqmf.hip):
//   generic taps t[band][p][i] = 4 h[band][3 - p + 4 i] (x4 up-sampling gain folded, exact),
//   and for the fixed PQMF design its factorisation 4 h_k[j] = g[j] * c[k][j mod 8].
constexpr int kFiltTable = 352;
std::vector<float> synthesis_table(const float* h63) {
  std::vector<float> t(kFiltTable, 0.f);
  for (int band = 0; band < 4; ++band)
    for (int p = 0; p < 4; ++p)
      for (int i = 0; i < 16; ++i) {
        const int j = 3 - p + 4 * i;
        t[band * 64 + p * 16 + i] = j <= 62 ? 4.f * h63[band * 63 + j] : 0.f;
      }
  // fixed-bank factors (pqmf.py:66-75): theta_k(j) = (2k+1)(pi/8)(j - 30.5) - (-1)^k pi/4
  for (int k = 0; k < 4; ++k)
    for (int q = 0; q < 8; ++q) {
      const double sign = (k % 2 == 0) ? 1.0 : -1.0;
      t[256 + k * 8 + q] = (float)std::cos((2 * k + 1) * (M_PI / 8.0) * (q - 30.5) - sign * M_PI / 4.0);
    }
  const std::vector<double> proto = pqmf_prototype();
  for (int j = 0; j <= 62; ++j) t[288 + j] = (float)(8.0 * proto[j] * (((j / 8) % 2) ? -1.0 : 1.0));
  return t;
}

int do_finalize(mbv_model* m, hipStream_t stream) {
  if (m->import_src) {                 // zero tensors of the expected shapes stand in for the checkpoint
    m->raw.clear();
    for (auto& kv : m->expected) {
      HostTensor t;
      t.shape = kv.second;
      t.data.assign((size_t)t.numel(), 0.f);
      m->raw[kv.first] = std::move(t);
    }
  }
  for (auto& kv : m->expected)
    if (!m->raw.count(kv.first)) return m->fail("missing weight '%s'", kv.first.c_str());
  const mbv_config& c = m->cfg;
  const int H = c.hidden_channels, I = c.inter_channels, gin = c.gin_channels;
  std::vector<float> arena;
  Packer P{m, arena};
  char p[160];

  m->emb = P.vec("enc_p.emb.weight");
  m->enc.assign(c.n_layers, mbv_model::Layer());
  for (int i = 0; i < c.n_layers; ++i) {
    auto& L = m->enc[i];
    snprintf(p, sizeof p, "enc_p.encoder.attn_layers.%d.", i);
    const std::string s(p);
    {   // fused q|k|v 1x1 conv: rows [q(0..H) | k | v]
      std::vector<float> w(3 * (size_t)H * H), b(3 * (size_t)H);
      const char* names[3] = {"conv_q", "conv_k", "conv_v"};
      for (int j = 0; j < 3; ++j) {
        std::memcpy(&w[(size_t)j * H * H], P.t(s + names[j] + ".weight").data.data(), (size_t)H * H * 4);
        std::memcpy(&b[(size_t)j * H], P.t(s + names[j] + ".bias").data.data(), (size_t)H * 4);
      }
      std::vector<int> rows(3 * H);
      for (int r = 0; r < 3 * H; ++r) rows[r] = r;
      L.qkv = P.conv(w, 3 * H, H, 1, rows, {}, &b, nullptr);
    }
    L.o = P.conv_plain(s + "conv_o");
    L.ek = P.vec(s + "emb_rel_k");
    L.ev = P.vec(s + "emb_rel_v");
    snprintf(p, sizeof p, "enc_p.encoder.norm_layers_1.%d.", i);
    L.g1 = P.vec(std::string(p) + "gamma"); L.b1 = P.vec(std::string(p) + "beta");
    snprintf(p, sizeof p, "enc_p.encoder.norm_layers_2.%d.", i);
    L.g2 = P.vec(std::string(p) + "gamma"); L.b2 = P.vec(std::string(p) + "beta");
    snprintf(p, sizeof p, "enc_p.encoder.ffn_layers.%d.", i);
    L.ffn1 = P.conv_plain(std::string(p) + "conv_1");
    L.ffn2 = P.conv_plain(std::string(p) + "conv_2");
  }
  m->enc_proj = P.conv_plain("enc_p.proj");
  if (c.use_sdp) {
    auto dds = [&](const std::string& q) {
      mbv_model::Dds d;
      for (int i = 0; i < 3; ++i) {
        const std::string n = std::to_string(i);
        d.sw[i] = P.vec(q + "convs_sep." + n + ".weight");     // [C, 1, 3] -> [C][3]
        d.sb[i] = P.vec(q + "convs_sep." + n + ".bias");
        d.c1[i] = P.conv_plain(q + "convs_1x1." + n);
        d.g1[i] = P.vec(q + "norms_1." + n + ".gamma"); d.b1[i] = P.vec(q + "norms_1." + n + ".beta");
        d.g2[i] = P.vec(q + "norms_2." + n + ".gamma"); d.b2[i] = P.vec(q + "norms_2." + n + ".beta");
      }
      return d;
    };
    m->sdp.pre = P.conv_plain("dp.pre");
    m->sdp.proj = P.conv_plain("dp.proj");
    m->sdp.dds = dds("dp.convs.");
    for (int k = 0; k < 3; ++k) {               // reverse order of use: flows 7, 5, 3 (models.py:92-93)
      const std::string q = "dp.flows." + std::to_string(7 - 2 * k) + ".";
      m->sdp.flow[k].pre_w = P.vec(q + "pre.weight");
      m->sdp.flow[k].pre_b = P.vec(q + "pre.bias");
      m->sdp.flow[k].dds = dds(q + "convs.");
      m->sdp.flow[k].proj = P.conv_plain(q + "proj");
    }
    m->sdp.m = P.vec("dp.flows.0.m");
    m->sdp.logs = P.vec("dp.flows.0.logs");
    m->sdp.edge_const = (float)std::log(std::exp(1.0 - 1e-3) - 1.0);   // transforms.py:74
  } else {
    m->dp1 = P.conv_plain("dp.conv_1");
    m->dp2 = P.conv_plain("dp.conv_2");
    m->dp_g1 = P.vec("dp.norm_1.gamma"); m->dp_b1 = P.vec("dp.norm_1.beta");
    m->dp_g2 = P.vec("dp.norm_2.gamma"); m->dp_b2 = P.vec("dp.norm_2.beta");
    m->dp_pw = P.vec("dp.proj.weight"); m->dp_pb = P.vec("dp.proj.bias");
  }
  m->dp_cw = P.vec("dp.cond.weight"); m->dp_cb = P.vec("dp.cond.bias");
  m->emb_g = P.vec("emb_g.weight");

  // ---- flows: the channel Flip (modules.py:280-287) is folded into the packing.
  // Reverse pass order is f = 3,2,1,0, each preceded by a flip, so layers 3 and 1
  // see the physical buffer flipped, 2 and 0 see it straight.
  const int half = I / 2;
  for (int f = 0; f < kNFlows; ++f) {
    auto& F = m->flow[f];
    const bool flipped = (f % 2) == 1;
    snprintf(p, sizeof p, "flow.flows.%d.", 2 * f);
    const std::string s(p);
    {
      const std::vector<float> w = P.dense(s + "pre");
      std::vector<int> rows(H), cmap(half);
      for (int r = 0; r < H; ++r) rows[r] = r;
      for (int ci = 0; ci < half; ++ci) cmap[ci] = flipped ? half - 1 - ci : ci;
      F.pre = P.conv(w, H, half, 1, rows, cmap, &P.t(s + "pre.bias").data, nullptr);
    }
    // (only where the x0' window fits the kernel's staging loop and `post` is folded too, see run_coupling: otherwise
    // in16f0.M stays 0 and run_coupling launches F.pre itself)
    if (wn_prefold_fits(H, I) && wn_postfold_fits(H, I)) {
      // r03: `pre` folded into the first fused WN layer.  h = (W_pre x0 + b_pre) mask = W_pre' x0' with
      // x0' = [x0 ; mask ; 0 ..] (Cin' = half + 1 channels padded to a multiple of 8) and W_pre' = [W_pre | b_pre | 0 ..]
      // (input channels in the physical order of the half, the Flip folded as in F.pre).  The gate conv of layer 0
      // is linear in h, so it runs on x0' with W_in0[tap] W_pre' (composed in fp64): 13 channel groups per tap instead of 24.
      const int Cp = (int)align_up((size_t)half + 1, 8);
      F.Gi = Cp / 8;
      const std::vector<float> wpre = P.dense(s + "pre");                     // [H][half][1]
      const std::vector<float>& bpre = P.t(s + "pre.bias").data;
      std::vector<float> wp((size_t)H * Cp, 0.f);                             // W_pre' [H][Cp]
      for (int r = 0; r < H; ++r) {
        for (int ci = 0; ci < half; ++ci) wp[(size_t)r * Cp + ci] = wpre[(size_t)r * half + (flipped ? half - 1 - ci : ci)];
        wp[(size_t)r * Cp + half] = bpre[r];
      }
      {   // rows past H must exist and be zero: every wave runs all its tile slots over it (wn_fused.hip pre_loop)
        const int Mrows = (int)align_up((size_t)H, 128) < 384 ? 384 : (int)align_up((size_t)H, 128);
        std::vector<int> rws(Mrows);
        for (int i = 0; i < Mrows; ++i) rws[i] = i < H ? i : -1;
        F.pref = P.conv(wp, H, Cp, 1, rws, {}, nullptr, nullptr);
      }
      {
        const std::vector<float> win = P.dense(s + "enc.in_layers.0");        // [2H][H][K]
        std::vector<float> wc((size_t)2 * H * Cp * kFlowK);
        std::vector<double> acc(Cp);
        for (int r = 0; r < 2 * H; ++r)
          for (int tap = 0; tap < kFlowK; ++tap) {
            std::fill(acc.begin(), acc.end(), 0.0);
            for (int k = 0; k < H; ++k) {
              const double wv = win[((size_t)r * H + k) * kFlowK + tap];
              const float* src = &wp[(size_t)k * Cp];
              for (int ci = 0; ci <= half; ++ci) acc[ci] += wv * src[ci];
            }
            for (int ci = 0; ci < Cp; ++ci) wc[((size_t)r * Cp + ci) * kFlowK + tap] = (float)acc[ci];
          }
        std::vector<int> rows(2 * H), brows(2 * H);                            // row order of pack_gated16
        for (int r = 0; r < 2 * H; ++r) {
          const int tile = r / 32, rho = r % 32;
          const int ch = tile * 16 + (rho & 7) + 8 * (rho >> 4);
          rows[r] = (rho & 8) ? H + ch : ch;
          brows[r] = r;
        }
        F.in16f0 = P.conv(wc, 2 * H, Cp, kFlowK, rows, {}, &P.t(s + "enc.in_layers.0.bias").data, &brows);
      }
    }
    for (int l = 0; l < kFlowLayers; ++l) {
      char q[64];
      snprintf(q, sizeof q, "enc.in_layers.%d", l);
      F.in[l] = pack_gated(P, s + q, H, kFlowK);
      if (wn_fused_supported(H, kFlowK)) F.in16[l] = pack_gated16(P, s + q, H, kFlowK);
      snprintf(q, sizeof q, "enc.res_skip_layers.%d", l);
      F.rs[l] = P.conv_plain(s + q);
      if (wn_fused_supported(H, kFlowK)) F.rsp[l] = pack_rs_permuted(P, s + q);
    }
    if (gin) {
      F.cw = P.vec_data(P.dense(s + "enc.cond_layer"));
      F.cb = P.vec(s + "enc.cond_layer.bias");
    }
    {
      const std::vector<float> w = P.dense(s + "post");
      std::vector<int> rows(half);
      for (int r = 0; r < half; ++r) rows[r] = flipped ? half - 1 - r : r;
      F.post = P.conv(w, half, H, 1, rows, {}, &P.t(s + "post.bias").data, nullptr);
      // r03: `post` folded into the res/skip convs of the fused WN layers.  m = post(sum_l skip_l) is linear in the
      // layers' gated tiles: m = sum_l (W_post W_rs_l[skip rows]) acts_l + (W_post sum_l b_rs_l[skip] + b_post), so
      // layer l's res/skip conv gets `half` skip rows (W_post W_rs_l[skip rows], composed in fp64) instead of H,
      // `skip` accumulates m itself and the last layer applies the coupling (WnLayerArgs::x1).  Row r of m is the
      // physical channel r of the half being updated (the Flip folded as in F.post above).  Only where H + half rows
      // fit the kernel's row tiles: otherwise rspf[0].M stays 0 and run_coupling launches F.post (EPI_COUPLE) itself.
      if (wn_postfold_fits(H, I)) {
        const std::vector<float>& bpost = P.t(s + "post.bias").data;
        for (int l = 0; l < kFlowLayers; ++l) {
          const std::string q = s + "enc.res_skip_layers." + std::to_string(l);
          const std::vector<float> wrs = P.dense(q);                 // [2H or H][H][1]
          const std::vector<float>& brs = P.t(q + ".bias").data;
          const bool lastl = l == kFlowLayers - 1;
          const int skip0 = lastl ? 0 : H;                            // first skip row of W_rs_l
          const int Mrows = (lastl ? 0 : H) + half;
          std::vector<float> wc((size_t)Mrows * H), bc(Mrows);
          for (int r = 0; r < (lastl ? 0 : H); ++r) {
            std::memcpy(&wc[(size_t)r * H], &wrs[(size_t)r * H], (size_t)H * sizeof(float));
            bc[r] = brs[r];
          }
          for (int r = 0; r < half; ++r) {
            const int pr = rows[r];
            std::vector<double> acc(H, 0.0);
            double bacc = lastl ? (double)bpost[pr] : 0.0;
            for (int k = 0; k < H; ++k) {
              const double wp = w[(size_t)pr * H + k];
              const float* src = &wrs[(size_t)(skip0 + k) * H];
              for (int cch = 0; cch < H; ++cch) acc[cch] += wp * src[cch];
              bacc += wp * brs[skip0 + k];
            }
            float* dst = &wc[(size_t)((lastl ? 0 : H) + r) * H];
            for (int cch = 0; cch < H; ++cch) dst[cch] = (float)acc[cch];
            bc[(lastl ? 0 : H) + r] = (float)bacc;
          }
          std::vector<int> rws(Mrows), cmap(H);
          for (int i = 0; i < Mrows; ++i) rws[i] = i;
          for (int ci = 0; ci < H; ++ci) cmap[ci] = 8 * (ci / 8) + 4 * (ci & 1) + ((ci & 7) >> 1);     // as pack_rs_permuted
          F.rspf[l] = P.conv(wc, Mrows, H, 1, rws, cmap, &bc, nullptr);
        }
      }
    }
  }

  // ---- posterior encoder (voice conversion only)
  {
    auto& Q = m->encq;
    const int cin = c.spec_channels, cpad = (int)align_up(cin, 32);
    Q.cin_pad = cpad;
    const std::vector<float>& w0 = P.t("enc_q.pre.weight").data;       // [H][cin][1]
    std::vector<float> w((size_t)H * cpad, 0.f);
    for (int co = 0; co < H; ++co)
      std::memcpy(&w[(size_t)co * cpad], &w0[(size_t)co * cin], (size_t)cin * sizeof(float));
    std::vector<int> rows(H);
    for (int r = 0; r < H; ++r) rows[r] = r;
    Q.pre = P.conv(w, H, cpad, 1, rows, {}, &P.t("enc_q.pre.bias").data, nullptr);
    for (int l = 0; l < mbv_model::kEncQLayers; ++l) {
      char q[64];
      snprintf(q, sizeof q, "enc_q.enc.in_layers.%d", l);
      Q.in[l] = pack_gated(P, q, H, 5);
      if (wn_fused_supported(H, 5)) Q.in16[l] = pack_gated16(P, q, H, 5);
      snprintf(q, sizeof q, "enc_q.enc.res_skip_layers.%d", l);
      Q.rs[l] = P.conv_plain(q);
      if (wn_fused_supported(H, 5)) Q.rsp[l] = pack_rs_permuted(P, q);
    }
    if (gin) {
      Q.cw = P.vec_data(P.dense("enc_q.enc.cond_layer"));
      Q.cb = P.vec("enc_q.enc.cond_layer.bias");
    }
    Q.proj = P.conv_plain("enc_q.proj");
  }

  // ---- decoder
  m->conv_pre = P.conv_plain("dec.conv_pre");
  for (int i = 0; i < 2; ++i) {
    snprintf(p, sizeof p, "dec.ups.%d", i);
    const std::vector<float> w = P.dense(p);            // [Cin][Cout][16], norm per Cin
    const auto& sh = P.t(std::string(p) + ".weight_v").shape;
    const int Cin = (int)sh[0], Cout = (int)sh[1];
    const int us = dec_us(c);
    if (Cout % 32 || Cin % 16)
      return m->fail("%s: ConvTranspose1d %d -> %d channels: the EPI_CONVT conv needs Cout %% 32 == 0 and Cin %% 16 == 0",
                     p, Cin, Cout);
    PConv& pc = m->upc[i];
    pc.M = us * Cout; pc.Mpad = (int)align_up(pc.M, 128); pc.Cin = Cin; pc.K = convt_taps(us);
    pc.w = P.alloc((size_t)pc.K * Cin * pc.Mpad);
    pc.bias = P.alloc(pc.M);
    pc.has_bias = true;
    pack_convt_rows(w.data(), P.t(std::string(p) + ".bias").data.data(), Cin, Cout, us, pc.Mpad, &arena[pc.w],
                    &arena[pc.bias]);
  }
  for (int n = 0; n < 6; ++n) {
    if (c.resblock_type == 1) {
      for (int q = 0; q < 3; ++q) {
        snprintf(p, sizeof p, "dec.resblocks.%d.convs1.%d", n, q);
        m->rb[n].c1[q] = P.conv_plain(p);
        snprintf(p, sizeof p, "dec.resblocks.%d.convs2.%d", n, q);
        m->rb[n].c2[q] = P.conv_plain(p);
      }
    } else {
      for (int q = 0; q < 2; ++q) {
        snprintf(p, sizeof p, "dec.resblocks.%d.convs.%d", n, q);
        m->rb[n].c1[q] = P.conv_plain(p);
      }
    }
    if (gin) {
      snprintf(p, sizeof p, "dec.resblocks.%d.cond.", n);
      m->rb[n].cw = P.vec(std::string(p) + "weight");
      m->rb[n].cb = P.vec(std::string(p) + "bias");
    }
  }
  {   // subband_conv_post, rows pre-scaled for the fused iSTFT kernel: exp(x) = 2^(x log2 e),
      // sin(x) = sin_turns(x / 2 pi)  (istft_pqmf.hip, template PRE)
    const std::string pn = c.decoder == MBV_DEC_SINGLEBAND ? "dec.conv_post" : "dec.subband_conv_post";
    std::vector<float> w = P.dense(pn);
    std::vector<float> bsc = P.t(pn + ".bias").data;
    const auto& sh = P.t(pn + ".weight_v").shape;
    const int Cout = (int)sh[0], Cin = (int)sh[1], K = (int)sh[2];
    for (int co = 0; co < Cout; ++co) {
      const float sc = (co % 18) < 9 ? 1.44269504088896341f : 0.15915494309189535f;
      for (int j = 0; j < Cin * K; ++j) w[(size_t)co * Cin * K + j] *= sc;
      bsc[co] *= sc;
    }
    std::vector<int> rows(Cout);
    for (int i = 0; i < Cout; ++i) rows[i] = i;
    m->conv_post = P.conv(w, Cout, Cin, K, rows, {}, &bsc, nullptr);
  }
  if (c.decoder == MBV_DEC_MULTISTREAM) {
    const std::vector<float> h = P.dense("dec.multistream_conv_post");   // [1][4][63]
    m->filt = P.vec_data(synthesis_table(h.data()));
  } else if (c.decoder == MBV_DEC_MULTIBAND) {
    const std::vector<float> h = pqmf_synthesis_filter();
    m->filt = P.vec_data(synthesis_table(h.data()));
  }

  // ---- upload
  if (m->darena && m->darena_floats < arena.size()) { HIPCHK(m, hipFree(m->darena)); m->darena = nullptr; }
  if (!m->darena) {
    HIPCHK(m, hipMalloc((void**)&m->darena, arena.size() * sizeof(float)));
    m->darena_floats = arena.size();
  }
  if (m->import_src) {
    if ((int64_t)arena.size() != m->import_n)
      return m->fail("mbv_import_arena: %lld floats offered, this configuration's arena has %zu (exported by another configuration or library build?)",
                     (long long)m->import_n, arena.size());
    HIPCHK(m, hipMemcpyAsync(m->darena, m->import_src, arena.size() * sizeof(float), hipMemcpyDeviceToDevice, stream));
    m->raw.clear();
  } else {
    HIPCHK(m, hipMemcpyAsync(m->darena, arena.data(), arena.size() * sizeof(float),
                             hipMemcpyHostToDevice, stream));
  }
  HIPCHK(m, hipStreamSynchronize(stream));
  m->arena_used = arena.size();
  m->harena.swap(arena);
  m->finalized = true;
  m->split_valid = false;
  if (m->conv_bf16 == 3 && ensure_split_arena(m, stream)) return 1;
  return reblend_voices(m, stream);
}

// ------------------------------------------------------------------ scratch
struct Bump {
  char* base; size_t cap, off = 0;     // base == nullptr: a measuring pass, take advances `off` as ever and returns null
  template <typename Tp> Tp* take(size_t n) {
    off = align_up(off, 256);
    Tp* p = base ? reinterpret_cast<Tp*>(base + off) : nullptr;
    off += n * sizeof(Tp);
    return p;
  }
  bool fits() const { return off <= cap; }
};

int ensure(mbv_model* m, Scratch& sc, size_t need) {
  ++sc.claim;                            // grown or not, the caller writes from offset 0: what pointed in here is dead
  if (sc.bytes >= need) return 0;
  if (sc.p) { HIPCHK(m, hipDeviceSynchronize()); HIPCHK(m, hipFree(sc.p)); sc.p = nullptr; sc.bytes = 0; }
  need = align_up(need + (need >> 3), 1 << 20);
  HIPCHK(m, hipMalloc((void**)&sc.p, need));
  sc.bytes = need;
  return 0;
}

// An entry's scratch is written ONCE, as `carve(Bump&)`: run on a measuring Bump for the byte count, then, with the
// buffer grown to that, on the buffer itself.  A tensor that may go to a caller's pointer instead is decided inside
// `carve`, so both passes agree on it; what a take depends on must be a host fact, never a pointer carved before it
// (the measuring pass hands out null).  Nothing carved may be used before this returns 0.  An arena that already
// holds the layout — every call but the first of a larger size — is carved at once: that one pass is all.  So a carve
// may run up to three times per call and must do nothing but set its outputs; a pass that does not fit hands out
// pointers past the arena, which nobody may read before lay_out has returned 0.
template <typename Carve>
int lay_out(mbv_model* m, const char* who, Scratch& buf, Carve&& carve) {
  ++buf.claim;                           // (ensure's rule, for the call that fits: before anything is carved or freed)
  Bump sc{buf.p, buf.bytes};
  if (buf.p) carve(sc);
  if (buf.p && sc.fits()) return 0;
  Bump measure{nullptr, 0};
  carve(measure);
  if (ensure(m, buf, measure.off)) return 1;
  sc = Bump{buf.p, buf.bytes};
  carve(sc);
  return sc.fits() ? 0 : m->fail("%s: scratch layout exceeds its buffer", who);
}

// The integer half of a ConvArgs, all that conv1d_plan, conv1d_trim_bn and conv1d_narrow_supported read besides which
// optional tensors are given: B rows of Cin x Tin -> M x T, dense, "same" padding, plain store.
ConvArgs conv_shape(int Cin, int M, int K, int dil, int Tin, int T, int B, int splitk) {
  ConvArgs a{};
  a.Cin = Cin; a.M = M; a.Mpad = (int)align_up(M, 128); a.K = K; a.dil = dil; a.pad_left = (K - 1) * dil / 2;
  a.Tin = Tin; a.x_rstride = Tin; a.x_bstride = (int64_t)Cin * Tin;
  a.T = T; a.y_bstride = (int64_t)M * T; a.epi = EPI_STORE; a.in_slope = 1.f; a.out_scale = 1.f; a.B = B;
  a.splitk = splitk;
  return a;
}

// ... of a packed conv of the handle, on real tensors
ConvArgs conv_bind(const mbv_model* m, const PConv& p, ConvArgs a, const float* x, float* y) {
  a.x = x; a.y = y;
  a.w = m->W(p.w); a.bias = p.has_bias ? m->W(p.bias) : nullptr;
  a.w_split = m->Wsplit(p.w);
  a.ws = m->conv_ws; a.ws_floats = m->conv_ws_floats; a.counters = m->conv_cnt; a.n_counters = m->conv_ncnt;
  a.prec = a.w_split ? 3 : 0;
  return a;
}

ConvArgs conv_args(const mbv_model* m, const PConv& p, const float* x, int64_t x_bstride, int Tin,
                   float* y, int64_t y_bstride, int T, int B, int dil = 1) {
  ConvArgs a = conv_shape(p.Cin, p.M, p.K, dil, Tin, T, B, m->splitk);
  a.x_bstride = x_bstride; a.y_bstride = y_bstride;
  return conv_bind(m, p, a, x, y);
}

// decoder + waveform tail on z [B, I, zstride] (first Td frames valid)

// "tail_once" as the handle's options leave it: 0 off (or excluded by split-K, "trim", "conv_bf16"), 1 the stages
// whose ResBlock convs exceed one round of the 256-workgroup grid, 2 every stage (tests).  Below one round a
// dropped tile saves no time and the map and fill launches would only add launch gaps (B = 8: + 0.1 ms).
int tail_mode(const mbv_model* m) { return (!m->trim && !m->splitk && m->conv_bf16 != 3) ? m->tail_once : 0; }
bool tail_stage(int mode, int B, long conv_tiles) { return B > 1 && (mode == 2 || (mode == 1 && conv_tiles > 256)); }
// ... on the packed route: the stages whose rows are at most kTailPackMaxTiles column tiles long.  A row
// loses half a tile on average to whole-tile dropping, whatever its length, and a packed row pays its gap and the
// table lookup (1.3 - 2 % per tile, profiles/tail_pack_gate.jsonl): at 6 tiles a row (the headline batch's stage 0)
// the maps leave out 1.3 % of the tiles and packing 8 %; at 24 tiles a row (its stage 1) 7.6 % against 9.0 %,
// which the lookup eats.  Between the two nothing was measured: the threshold sits near the lower end.
constexpr int kTailPackMaxTiles = 8;
bool tail_pack_stage(int Lo, int bn) { return (Lo + bn - 1) / bn <= kTailPackMaxTiles; }

// The three ResBlocks of a decoder stage on three streams?  Only when one of their convs (ch channels, Lo
// frames) is at most 192 tiles of 128 x 384, i.e. cannot fill the chip by itself.
// With tail maps (option "tail_once") at any size: a launch that lost its tail tiles ends in a partial round of the
// persistent grid, which only a launch of another ResBlock can fill.
bool decoder_stage_concurrent(const mbv_model* m, int B, int ch, int Lo, bool tail = false) {
  const long conv_tiles = (long)B * ((Lo + 383) / 384) * ((ch + 127) / 128);
  return m->dec_streams && m->aux_ok && m->cfg.resblock_type != 2 && (conv_tiles <= 192 || tail) && !m->trim;   // (trim: its tile maps are built on the caller's stream)
}

// The streaming decode (mbv_decode_range): run_decoder on a z-window of Td frames whose first frame is z-frame
// `first - keep_first` of an utterance of t_full frames.  The tail stores only window frames [keep_first,
// keep_first + keep_count), at o + b o_row_stride (o already offset to the chunk's first sample).
// Pooled (mbv_decode_chunks; together with RaggedRows): every row is the window of its own chunk of its own
// utterance.  `rows` (device [B]) then holds each row's kept range and destination, max_keep >= the longest kept
// range in tail units (64 per z-frame), t_full = the longest utterance of the run — all of one class, so it plans
// every conv as each of them does — and keep_first / keep_count / o / o_row_stride are not read.
struct DecodeRange {
  int t_full;
  int keep_first, keep_count;
  float* o;
  int64_t o_row_stride;
  const PoolRow* rows = nullptr;
  int max_keep = 0;
};

// ------------------------------------------------------------------ the decoder, stated once
// Every launch of the decoder in launch order, as integers.  kind: conv_pre, ups[stage], the first / second conv of
// step q of ResBlock j of `stage` (ResBlock2: its one conv counts as the second), conv_post behind
// ReflectionPad1d((1, 0)), the waveform tail.  A conv of a row of len z-frames runs over num len input columns and
// T = num len + add launch columns; rate = output columns per z-frame (ups runs over INPUT frames: convt_u num).
// res / chan_add / res_chan_add: the optional tensors of the launch (the latter two with speaker-conditioned
// ResBlocks); lens: which of a ragged row's lengths (len, us len, us^2 len) masks the input.
std::vector<DecLaunch> decoder_table(const mbv_config& c) {
  const bool sb = c.decoder == MBV_DEC_SINGLEBAND;
  const int us = dec_us(c), C0 = c.upsample_initial_channel;
  const int kPre = 7, kPost = 7;                        // conv_pre, conv_post / subband_conv_post (models.py)
  const int n_fft = 16, hop = 4;                        // TorchSTFT
  const int bands = sb ? 1 : 4, taps = 63;              // PQMF synthesis / multistream_conv_post
  const int nq = c.resblock_type == 2 ? 2 : 3;
  std::vector<DecLaunch> t;
  auto conv = [&](int kind, int stage, int j, int q, int Cin, int M, int K, int dil, int num, int epi) -> DecLaunch& {
    DecLaunch e{};
    e.kind = kind; e.stage = stage; e.j = j; e.q = q;
    e.Cin = Cin; e.M = M; e.K = K; e.dil = dil; e.pad_left = (K - 1) * dil / 2;
    e.num = e.rate = num; e.lens = stage + 1; e.epi = epi; e.res = epi == EPI_RESID || epi == EPI_RESID_ACC;
    t.push_back(e);
    return t.back();
  };
  conv(DL_PRE, -1, 0, 0, c.inter_channels, C0, kPre, 1, 1, EPI_STORE);
  int num = 1;
  for (int i = 0; i < 2; ++i) {
    const int ch = C0 >> (i + 1);
    DecLaunch& u = conv(DL_UP, i, 0, 0, C0 >> i, us * ch, convt_taps(us), 1, num, EPI_CONVT);
    u.pad_left = convt_pad_left(us); u.convt_u = us; u.rate = us * num; u.lens = i;
    u.tk = kConvtK; u.tp = (kConvtK - us) / 2;
    num *= us;
    for (int j = 0; j < 3; ++j) {
      const int k = c.resblock_kernel_sizes[j];
      for (int q = 0; q < nq; ++q) {                  // each step: x = conv(...)(x) + x; the last one adds into xs
        const int d = c.resblock_dilations[j][q];
        const int last = q == nq - 1 ? EPI_RESID_ACC : EPI_RESID;
        if (c.resblock_type == 2) {
          DecLaunch& e = conv(DL_C2, i, j, q, ch, ch, k, d, num, last);
          e.chan_add = e.res_chan_add = q == 0;
        } else {
          conv(DL_C1, i, j, q, ch, ch, k, d, num, EPI_STORE).chan_add = q == 0;
          conv(DL_C2, i, j, q, ch, ch, k, 1, num, last).res_chan_add = q == 0;
        }
      }
    }
  }
  DecLaunch& p = conv(DL_POST, 2, 0, 0, C0 >> 2, 2 * (n_fft / 2 + 1) * bands, kPost, 1, num, EPI_STORE);
  p.add = 1; p.reflect1 = 1; p.lens = 2;               // frame f reads padded[f - 3 .. f + 3] = x[f - 4 .. f + 2]
  DecLaunch w{};
  w.kind = DL_TAIL; w.stage = 2; w.num = num; w.add = 1; w.rate = num * hop * bands;
  w.n_fft = n_fft; w.hop = hop; w.bands = bands; w.taps = taps;
  t.push_back(w);
  return t;
}

// The integer shape of entry e for B rows of len z-frames: what run_decoder launches (it adds tensors, the strides of
// its real buffers and the per-call options) and what the planner-side readers plan.
ConvArgs dec_shape(const DecLaunch& e, int len, int B, int splitk) {
  ConvArgs a = conv_shape(e.Cin, e.M, e.K, e.dil, e.num * len, e.num * len + e.add, B, splitk);
  a.pad_left = e.pad_left; a.epi = e.epi; a.convt_u = e.convt_u; a.reflect1 = e.reflect1;
  if (e.res) a.res_bstride = a.y_bstride;
  return a;
}
// ... for conv1d_plan / conv1d_trim_bn / conv1d_narrow_supported alone, which test data pointers against null: the
// one place that hands out a placeholder.  Never launched.
ConvArgs dec_planner_args(const DecLaunch& e, int len, int B, int splitk, int prec = 0, bool cond = false) {
  static const float kSome = 0.f;                   // "a tensor is given"
  ConvArgs a = dec_shape(e, len, B, splitk);
  if (e.res) a.res = &kSome;
  if (cond && e.chan_add) a.chan_add = &kSome;      // (cond: a speaker vector reaches conditioned ResBlocks)
  if (cond && e.res_chan_add) a.res_chan_add = &kSome;
  a.prec = prec;
  return a;
}

// Receptive field of the decoder in whole z-frames (mbv_decoder_context): the interval of z-frames any sample of
// frame t can depend on is [t - L, t + R].  Walked backwards over the table from the samples of one frame far from
// both edges; every index interval is at the rate of the layer it belongs to.
struct Span { int64_t lo, hi; };
static Span span_conv(Span y, int K, int dil, int pad_left) { return {y.lo - pad_left, y.hi + (int64_t)(K - 1) * dil - pad_left}; }
static int64_t floor_div(int64_t a, int64_t b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }
static int64_t ceil_div(int64_t a, int64_t b) { return -floor_div(-a, b); }
// ConvTranspose1d(k, stride u, padding p): y[j] = sum_i x[i] w[j + p - u i], 0 <= j + p - u i < k
static Span span_convt(Span y, int k, int u, int p) { return {ceil_div(y.lo + p - k + 1, u), floor_div(y.hi + p, u)}; }
static Span span_union(Span a, Span b) { return {a.lo < b.lo ? a.lo : b.lo, a.hi > b.hi ? a.hi : b.hi}; }

void decoder_context(const std::vector<DecLaunch>& table, int* Lc, int* Rc) {
  const int64_t t = 1 << 20;                            // a frame far from both edges
  Span x{}, need{}, r{};                                // of a stage: its output xs, its input u, the ResBlock in hand
  for (size_t n = table.size(); n-- > 0;) {
    const DecLaunch& e = table[n];
    switch (e.kind) {
      case DL_TAIL:
        x = {e.rate * t, e.rate * t + e.rate - 1};      // the waveform samples of frame t
        if (e.bands > 1) x = {ceil_div(x.lo - e.taps / 2, e.bands), floor_div(x.hi + e.taps / 2, e.bands)};   // sub-band samples (zero-stuffed x bands)
        // iSTFT, center: output sample m is position m + n_fft / 2 of the overlap-add; frame f covers [hop f, hop f + n_fft)
        x = {ceil_div(x.lo + e.n_fft / 2 - (e.n_fft - 1), e.hop), floor_div(x.hi + e.n_fft / 2, e.hop)};
        break;
      case DL_POST:
        need = r = x = span_conv(x, e.K, e.dil, e.pad_left + e.reflect1);
        break;
      case DL_C1: case DL_C2:
        if (e.epi == EPI_RESID_ACC) { need = span_union(need, r); r = x; }    // a ResBlock's last launch: xs / 3 needs x of it
        r = span_conv(r, e.K, e.dil, e.pad_left);
        break;
      case DL_UP:
        need = r = x = span_convt(span_union(need, r), e.tk, e.convt_u, e.tp);
        break;
      case DL_PRE:
        x = span_conv(x, e.K, e.dil, e.pad_left);
        break;
    }
  }
  *Lc = (int)(t - x.lo);
  *Rc = (int)(x.hi - t);
}

// "tail_once": how far to the right a z-frame reaches at every launch of the decoder (mbv_tail_plan).  Walked
// forwards with the same index rules as decoder_context walks backwards: `hi` is the last output column the input
// columns up to x.hi can influence.
static int64_t reach_conv(int64_t hi, int pad_left) { return hi + pad_left; }                  // y[t] reads x[t - pad_left + k dil]
static int64_t reach_convt(int64_t hi, int k, int u, int p) { return (int64_t)u * hi - p + k - 1; }   // j = u i - p + [0, k)
// One entry per entry of the table, with its kind / stage / j / q.  rate = output columns per z-frame; reach = output
// columns past rate len - 1 that a valid z-frame of a row of len frames can still influence (ResBlock launches that
// write the running sum xs: the maximum over the ResBlocks summed so far).  Row b's output at and past column
// rate len_b + reach is the zero-input response: a function of the column alone.
struct TailLaunch { int kind, stage, j, q, rate, reach; };
void decoder_tail_plan(const std::vector<DecLaunch>& table, std::vector<TailLaunch>* out) {
  out->clear();
  const int64_t len = 1 << 20;                        // a row far from both edges; every hi below is relative to it
  int64_t sum_hi = len - 1;                           // the last valid z-frame; then xs: the ResBlocks summed so far
  int64_t hi = sum_hi, r = sum_hi;                    // a stage's input u (each ResBlock holds its skip path: >= hi), the ResBlock in hand
  for (const DecLaunch& e : table) {
    int64_t h = 0;
    switch (e.kind) {
      case DL_PRE:
        h = sum_hi = reach_conv(sum_hi, e.pad_left);
        break;
      case DL_UP:
        h = hi = r = sum_hi = reach_convt(sum_hi, e.tk, e.convt_u, e.tp);
        break;
      case DL_C1: case DL_C2:
        h = r = reach_conv(r, e.pad_left);            // (+ the skip path: r only grows)
        if (e.epi == EPI_RESID_ACC) { h = sum_hi = sum_hi > r ? sum_hi : r; r = hi; }
        break;
      case DL_POST:
        h = sum_hi = reach_conv(sum_hi, e.pad_left + e.reflect1);
        break;
      case DL_TAIL:
        h = e.hop * sum_hi + e.n_fft / 2 - 1;         // frame f covers sub-band samples [hop f - n_fft / 2, hop f + n_fft / 2)
        if (e.bands > 1) h = e.bands * h + e.taps / 2;   // sample n reads sub-band samples [(n - 31) / bands, (n + 31) / bands]
        break;
    }
    out->push_back({e.kind, e.stage, e.j, e.q, e.rate, (int)(h - ((int64_t)e.rate * len - 1))});
  }
}

// The row-exact ragged decode (mbv_decode_ragged): run_decoder on the rows of one class (run_decoder_ragged below).
// Row b is an utterance of len[b] <= Td frames and is decoded as if alone: every conv masks its input at the
// row's own length at that conv's rate (true zeros: the padding a stand-alone decode applies), only the column
// tiles that hold columns below it exist as work, the waveform tail takes the row's own frame count, and the row
// is stored at row row_map[b] of o.  Whatever a conv stores at columns past a row's end (its bias, the residual it
// read there) is never loaded by a consumer.
struct RaggedRows {
  const int* len;          // device [B]: len_b
  const int* len_u;        // us len_b
  const int* len_uu;       // us^2 len_b
  const int* row_map;      // device [B]: the row of o
  float* o;
  int64_t o_row_stride;
  int t_min;               // host: the shortest row of the run (run_decoder checks that it plans like the longest);
                           // pooled: the shortest UTTERANCE a row of the run is cut from
};

// What the scratch of one decoder run depends on, host facts all: z [B, I, zstride], first Td frames valid; lens: frame
// lengths are given; cond: a speaker vector reaches a conditioned model; own_o: no caller takes the waveform.
struct DecCall { int B, Td, zstride; bool lens, cond, own_o, ranged, ragged; };

// The scratch of one run (carve_decoder), and the two modes decided with it.
// trim — the opt-in trimmed decode (option "trim"; the caller takes only `o` and trims by y_lengths): a conv computes
// the column tiles that hold frames below (len_b + kTrimMargin) * rate of its utterance and nothing behind them.  The
// decoder's one-sided receptive field is 25.2 z-frames (conv_pre 3 + ups 2 + 0.5, the k = 11 ResBlocks 15 + 3.75,
// conv_post / iSTFT / PQMF < 1), so whatever sits behind an utterance's limit — stale scratch — stays more than
// 6 frames away from its valid samples: those are bitwise the default's.  Column-tile maps are built on the device
// from the lengths, one per (num, add, T, tile width) geometry; the ragged mode uses them with a margin of zero.
// tail — "tail_once" (default on): the decoder gets z * y_mask, so behind S_b = rate len_b + reach of a
// ResBlock launch (decoder_tail_plan) row b's output is the zero-input response, a function of the column alone
// and the same in every row.  Only the donor — the shortest row — computes it: the other rows drop the column
// tiles that lie wholly behind their S_b from the launch (the trim-map path of the conv kernel), and a copy kernel
// behind the launch writes the donor's values there.  An output element's chain of operations does not depend on
// its tile or row, so every tensor holds bitwise what it held.  A launch that lost tiles ends in a partial round
// of the persistent grid: the three ResBlocks then run on three streams at any batch size, so that another launch
// fills it.  Not with per-row conditioning (the tails differ), split-K, conv_bf16, one row, or modes with own maps.
constexpr int kTrimMargin = 32;
struct DecBufs {
  DecCall call;
  bool trim, tail;
  float* x0;
  struct TrimMap { int num, add, T, bn; int* map; bool built; };
  TrimMap trim_maps[12]; int n_trim;   // one per geometry: at most two tile widths for each of four (num, add)
  int trim_of[48];                 // per table entry (1 + 2 (1 + 18) + 2 at most): its trim map, -1 none
  struct TailMap { int kind, j, q, bn; const int* map; int pack_blocks; };   // pack_blocks > 0: a packed job's block table
  // per stage: u, t1 / r of each ResBlock (its own when the three run concurrently), xs, cond vectors, tail maps
  struct Stage { float *u, *t1s[3], *rs[3], *xs, *cb[3]; bool conc; int n_tail; TailMap tail_maps[kTailMapJobs]; TailMapJobs jobs; } st[2];
  int Bc;                          // rows per conv_post + tail sub-batch; 0: one utterance's x_post reaches 2 GiB
  float *xpost, *otmp;
};

void carve_decoder(const mbv_model* m, const DecCall& k, Bump& sc, DecBufs* out) {
  const mbv_config& c = m->cfg;
  const std::vector<DecLaunch>& table = m->dec_table;
  const int B = k.B, Td = k.Td;
  DecBufs& d = *out;                                // (plain data, filled in place: a carve allocates nothing)
  std::memset(&d, 0, sizeof d); d.call = k;
  d.trim = k.ragged ? !m->splitk : (m->trim && k.lens && !m->splitk && c.decoder != MBV_DEC_SINGLEBAND);
  d.tail = tail_mode(m) && !d.trim && !k.ragged && !k.ranged && k.lens && B > 1 && B <= 65535 && !k.cond;
  auto planned = [&](const DecLaunch& e) {
    ConvArgs a = dec_planner_args(e, Td, B, m->splitk, m->Wsplit(0) ? 3 : 0,
                                  k.cond && e.stage >= 0 && e.stage < 2 && m->rb[e.stage * 3 + e.j].cw.present);
    if (e.kind == DL_PRE) { a.x_rstride = k.zstride; a.x_bstride = (int64_t)e.Cin * k.zstride; }   // (z as the caller holds it)
    return a;
  };
  std::vector<TailLaunch> tail_plan;
  if (d.tail) decoder_tail_plan(table, &tail_plan);
  d.x0 = sc.take<float>((size_t)B * table[0].M * Td);
  for (const DecLaunch& up : table) {
    if (up.kind != DL_UP) continue;
    DecBufs::Stage& st = d.st[up.stage];
    const int ch = up.M / up.convt_u, Lo = up.rate * Td;
    const size_t n = (size_t)B * ch * Lo;
    // tail maps of this stage's ResBlock launches; a route that takes no map (narrow, split-batch, half-height) is kept
    const long stage_tiles = (long)B * ((Lo + 383) / 384) * ((ch + 127) / 128);
    if (d.tail && tail_stage(tail_mode(m), B, stage_tiles))
      for (size_t n_e = 0; n_e < table.size() && st.n_tail < kTailMapJobs; ++n_e) {
        const DecLaunch& e = table[n_e];
        if (e.stage != up.stage || (e.kind != DL_C1 && e.kind != DL_C2)) continue;
        const ConvArgs a = planned(e);
        const int bn = conv1d_trim_bn(a);
        if (!bn || conv1d_plan(a, false).route != conv1d_plan(a, true).route) continue;
        // Few column tiles per row (tail_pack_stage): whole tiles rarely fit behind S_b, so the rows' kept columns
        // are packed into shared tiles instead (CONV_TAIL_PACK) where the planner grants that route.  A rule on the
        // launch shape alone: the lengths are on the device.
        ConvArgs ap = a;
        ap.tail_pack = 1;
        if (tail_pack_stage(Lo, bn) && conv1d_plan(ap, true).route == CONV_TAIL_PACK) {
          const int halo = (a.K - 1) * a.dil, gap = tail_pack_gap(halo);
          st.jobs.job[st.n_tail] = {e.rate, tail_plan[n_e].reach, Lo, bn, nullptr, gap, halo - a.pad_left};
          st.tail_maps[st.n_tail++] = {e.kind, e.j, e.q, bn, nullptr, tail_pack_blocks(B, Lo, gap, bn)};
          continue;
        }
        st.jobs.job[st.n_tail] = {e.rate, tail_plan[n_e].reach, Lo, bn, nullptr};
        st.tail_maps[st.n_tail++] = {e.kind, e.j, e.q, bn, nullptr, 0};
      }
    // The three ResBlocks of a stage read the same input and only meet in the running sum xs.  When one of their convs
    // cannot fill the chip (decoder_stage_concurrent) they run on three streams — own temporaries each, the three xs
    // updates chained by events in the order of the one-stream schedule, so the result is bitwise the same.
    st.conc = decoder_stage_concurrent(m, B, ch, Lo, st.n_tail > 0) && !d.trim;
    st.u = sc.take<float>(n);
    for (int j = 0; j < 3; ++j) {
      st.t1s[j] = j == 0 || st.conc ? sc.take<float>(n) : st.t1s[0];
      st.rs[j] = j == 0 || st.conc ? sc.take<float>(n) : st.rs[0];
    }
    st.xs = sc.take<float>(n);
  }
  // ---- cond vectors: x = x + cond(g)   (modules.py:214-215)
  for (const DecLaunch& up : table)
    for (int j = 0; j < 3 && up.kind == DL_UP; ++j)
      if (k.cond && m->rb[up.stage * 3 + j].cw.present) d.st[up.stage].cb[j] = sc.take<float>((size_t)B * (up.M / up.convt_u));
  // ---- x_post.  The fused iSTFT kernels address it with 32-bit byte offsets: a batch whose x_post would reach 2 GiB
  // runs conv_post + iSTFT in sub-batches (same T', same kernels: bitwise an unsplit launch).
  const DecLaunch& post = table[table.size() - 2];
  const int64_t utt_bytes = (int64_t)post.M * (post.num * (int64_t)Td + post.add) * 4;
  int64_t cap_bytes = (1LL << 31) - 1;
  if (m->xpost_chunk_bytes > 0 && m->xpost_chunk_bytes < cap_bytes) cap_bytes = m->xpost_chunk_bytes;
  d.Bc = utt_bytes > (1LL << 31) - 1 ? 0 : (int)std::min<int64_t>(B, std::max<int64_t>(1, cap_bytes / utt_bytes));
  // ---- trim maps, one per geometry among the launches (a split conv_post keeps every tile: the maps are per full batch)
  // trim_of[entry]: its map, or -1 where the launch takes none (a route without trimmed launches: conv1d_trim_bn 0)
  for (size_t n_e = 0; n_e < table.size(); ++n_e) {
    const DecLaunch& e = table[n_e];
    d.trim_of[n_e] = -1;
    if (!d.trim || e.kind == DL_TAIL || (e.kind == DL_POST && d.Bc != B)) continue;
    const ConvArgs a = planned(e);
    const int bn = conv1d_trim_bn(a);
    for (int t = 0; bn && t < d.n_trim && d.trim_of[n_e] < 0; ++t)
      if (d.trim_maps[t].num == e.num && d.trim_maps[t].add == e.add && d.trim_maps[t].T == a.T && d.trim_maps[t].bn == bn) d.trim_of[n_e] = t;
    if (bn && d.trim_of[n_e] < 0 && d.n_trim < 12) {
      d.trim_of[n_e] = d.n_trim;
      d.trim_maps[d.n_trim++] = {e.num, e.add, a.T, bn, sc.take<int>(launch_trim_map_ints(B, a.T, bn)), false};
    }
  }
  for (auto& st : d.st)
    for (int i = 0; i < st.n_tail; ++i)
      st.tail_maps[i].map = st.jobs.job[i].out = sc.take<int>(
          st.jobs.job[i].pack_gap ? tail_pack_ints(B, st.jobs.job[i].T, st.jobs.job[i].pack_gap, st.jobs.job[i].BN)
                                  : launch_tail_map_ints(B, st.jobs.job[i].T, st.jobs.job[i].BN));
  d.xpost = sc.take<float>((size_t)d.Bc * (utt_bytes / 4));
  if (k.own_o) d.otmp = sc.take<float>((size_t)B * table.back().rate * Td);
}

// One decoder run on scratch laid out for it (lay_out with carve_decoder for the same call).
int run_decoder(mbv_model* m, const float* z, const int* zlens, const float* gvec, const mbv_outputs* outs,
                hipStream_t s, DecBufs& d, const DecodeRange* rg = nullptr, const RaggedRows* rr = nullptr) {
  const mbv_config& c = m->cfg;
  const std::vector<DecLaunch>& table = m->dec_table;
  const int B = d.call.B, Td = d.call.Td, zstride = d.call.zstride, gin = c.gin_channels;
  ++m->decoder_runs;
  if (rr) zlens = rr->len;
  float* o = rg ? rg->o : rr ? rr->o : outs ? outs->o : nullptr;
  const bool pooled = rg && rg->rows;      // (every row stores through its own table entry)
  if (d.call.lens != (zlens != nullptr) || d.call.cond != (gvec && gin) || d.call.ranged != (rg != nullptr) ||
      d.call.ragged != (rr != nullptr) || d.call.own_o != (!o && !pooled))
    return m->fail("internal error: the decoder's scratch was laid out for another call");
  if (!d.Bc)
    return m->fail("utterance too long for one launch: %d frames (x_post of ONE utterance must stay below 2 GiB)", Td);
  if (!o) o = d.otmp;
  // ranged decode, default mode: the length rules of the conv planner see the one-shot lengths (conv1d_plan)
  const int rt_num = rg && !m->splitk ? rg->t_full : 0;
  hipStream_t const s_main = s;
  const int* const rr_lens[3] = {rr ? rr->len : nullptr, rr ? rr->len_u : nullptr, rr ? rr->len_uu : nullptr};
  // an entry's launch: its shape from the table, on real tensors (nb rows: the sub-batches of conv_post)
  auto conv = [&](const DecLaunch& e, const PConv& p, const float* x, float* y, float in_slope, int nb) {
    ConvArgs a = conv_bind(m, p, dec_shape(e, Td, nb, m->splitk), x, y);
    a.in_slope = in_slope;
    if (rr) a.in_lens = rr_lens[e.lens];
    return a;
  };
  HIPCHK(m, hipEventRecord(m->evk[0], s));
  // Ragged mode: the classes come from ragged_classes' reading of the table.  Tie them to what is really launched:
  // every conv, planned for one utterance of the run's shortest row and of its longest, must fall on the same side of
  // the narrow / tiled divide — else rows of this run would sum in an order their stand-alone decode does not use.
  // Pooled (rg and rr): the rows are windows, and what must agree is the plan of the UTTERANCES they are cut from:
  // the shortest (rr->t_min) against the longest (rg->t_full), and the launch itself, which plans with the longest
  // in place of its own columns (route_T), against both.
  bool route_drift = false, tail_drift = false;
  auto narrow_alone = [&](const ConvArgs& a, int num, int add, int len) {
    ConvArgs s1 = a;
    s1.B = 1; s1.trim_map = nullptr;
    s1.T = num * len + add;
    s1.Tin = a.Tin - a.T + s1.T;
    s1.x_rstride = s1.Tin; s1.x_bstride = (int64_t)a.Cin * s1.Tin;
    s1.y_bstride = a.y_bstride / a.T * s1.T;
    s1.res_bstride = a.res ? (int64_t)a.M * s1.T : 0;
    const int r = conv1d_plan(s1, false).route;
    return r == CONV_NARROW_M || r == CONV_NARROW_LAUNCH;
  };
  auto with_trim = [&](ConvArgs& a, const DecLaunch& e) {
    if (rr && !m->splitk) {
      const bool narrow_long = narrow_alone(a, e.num, e.add, rg ? rg->t_full : Td);
      if (narrow_alone(a, e.num, e.add, rr->t_min) != narrow_long) route_drift = true;
      if (rg) {
        const int r = conv1d_plan(a, false, rt_num * e.num + e.add).route;
        if ((r == CONV_NARROW_M || r == CONV_NARROW_LAUNCH) != narrow_long) route_drift = true;
      }
    }
    if (!d.trim) return;
    // (the map was laid out from the entry's shape alone, like a tail map: the launch itself must agree)
    const int at = d.trim_of[&e - table.data()], bn = conv1d_trim_bn(a);
    if (bn != (at < 0 ? 0 : d.trim_maps[at].bn)) { tail_drift = true; return; }
    if (at < 0) return;
    DecBufs::TrimMap& k = d.trim_maps[at];
    if (!k.built) launch_trim_map(zlens, B, e.num, e.num * (rr ? 0 : kTrimMargin) + e.add, a.T, bn, k.map, s_main);
    k.built = true;
    a.trim_map = k.map; a.trim_bn = bn;
  };
  const DecBufs::Stage* tail_stage_bufs = nullptr;  // the current stage, for its tail maps
  auto with_tail = [&](ConvArgs& a, const DecLaunch& e) -> const DecBufs::TailMap* {
    for (int n_t = 0; n_t < tail_stage_bufs->n_tail; ++n_t) {
      const DecBufs::TailMap& t = tail_stage_bufs->tail_maps[n_t];
      if (t.kind != e.kind || t.j != e.j || t.q != e.q) continue;
      // (the map was planned before the fork from the launch's shape alone: the launch itself must agree)
      if (conv1d_trim_bn(a) != t.bn) { tail_drift = true; return nullptr; }
      if (t.pack_blocks) {
        a.tail_pack = 1; a.pack_tbl = t.map; a.pack_blocks = t.pack_blocks;
        if (conv1d_plan(a, true, rt_num * e.num).route != CONV_TAIL_PACK) { tail_drift = true; return nullptr; }
        return &t;
      }
      a.trim_map = t.map; a.trim_bn = t.bn;
      return &t;
    }
    return nullptr;
  };
  {
    const DecLaunch& e = table[0];
    ConvArgs a = conv(e, m->conv_pre, z, d.x0, 1.f, B);
    a.x_bstride = (int64_t)e.Cin * zstride;
    a.x_rstride = zstride;
    a.in_lens = zlens;
    with_trim(a, e);
    launch_conv1d(a, s, rt_num);
  }
  m->stage("dec_conv_pre", d.x0, (int64_t)B * table[0].M * Td, m->scrB);
  const float* cur = d.x0;
  size_t next = 1;                                   // the table entry of the next launch
  for (int i = 0; i < 2; ++i) {
    DecBufs::Stage& bufs = d.st[i];
    const DecLaunch& up = table[next++];
    const int ch = up.M / up.convt_u;
    const size_t n = (size_t)B * ch * up.rate * Td;
    float *const u = bufs.u, *const xs = bufs.xs;
    const bool conc = bufs.conc;
    // tail maps of this stage's ResBlock launches, all from one launch on the caller's stream (before the fork)
    tail_stage_bufs = &bufs;
    launch_tail_maps(zlens, B, bufs.jobs, bufs.n_tail, m->tail_cnt, s_main);
    {
      ConvArgs a = conv(up, m->upc[i], cur, u, kLrelu, B);
      with_trim(a, up);                             // tiles run over INPUT frames (rate of the stage below)
      launch_conv1d(a, s);
    }
    m->stage(i == 0 ? "dec_up_0" : "dec_up_1", u, (int64_t)n, m->scrB);
    if (conc) {
      HIPCHK(m, hipEventRecord(m->ev_fork, s_main));
      for (auto& st : m->aux) HIPCHK(m, hipStreamWaitEvent(st, m->ev_fork, 0));
    }
    // (an early return between the fork and the join below would leave work queued on the aux streams that
    // the caller's stream never waits for, while the next call reuses this scratch: the loop runs in a lambda
    // and a failure drains the aux streams first)
    auto resblocks = [&]() -> int {
    for (int j = 0; j < 3; ++j) {
      const auto& R = m->rb[i * 3 + j];
      hipStream_t s = (conc && j > 0) ? m->aux[j - 1] : s_main;   // this ResBlock's stream
      float* const t1 = bufs.t1s[j];
      float* const r = bufs.rs[j];
      // split-K scratch (low-latency mode): a third each, so that concurrent convs never share partials or tickets
      auto own_ws = [&](ConvArgs& a) {
        if (!conc) return;
        const size_t third = a.ws_floats / 3;
        const int cthird = a.n_counters / 3;
        a.ws += (size_t)j * third; a.ws_floats = third;
        a.counters += (size_t)j * cthird; a.n_counters = cthird;
      };
      const float* cadd = nullptr;
      if (gvec && gin && R.cw.present) {           // x = x + cond(g)   (modules.py:214-215)
        launch_cond_gemv(gvec, nullptr, nullptr, m->W(R.cw.off), m->W(R.cb.off), bufs.cb[j], B, gin, ch, s);
        cadd = bufs.cb[j];
      }
      // ResBlock1: x = c2(lrelu(c1_d(lrelu(x)))) + x per dilation, c1 into t1; ResBlock2 (modules.py:251-262): x =
      // conv_d(lrelu(x)) + x with the one conv of its steps in c1.  The step's result goes to r, the last one's into xs.
      const float* state = u;
      for (; table[next].stage == i && table[next].j == j; ++next) {
        const DecLaunch& e = table[next];
        const bool first = e.kind == DL_C1, second = !first && c.resblock_type != 2;
        ConvArgs a = conv(e, second ? R.c2[e.q] : R.c1[e.q], second ? t1 : state, first ? t1 : r, kLrelu, B);
        if (e.res) a.res = state;
        if (e.chan_add) a.chan_add = cadd;
        if (e.res_chan_add) a.res_chan_add = cadd;
        if (e.epi == EPI_RESID_ACC) {                // xs (+)= resblock output ; /3 on the last
          a.y = xs;
          a.accum_in = j == 0 ? nullptr : xs;
          a.out_scale = j == 2 ? (1.f / 3.f) : 1.f;
          if (conc && j > 0) HIPCHK(m, hipStreamWaitEvent(s, m->ev_rb[j - 1], 0));   // xs of the ResBlock before
        }
        own_ws(a);
        with_trim(a, e);
        const DecBufs::TailMap* tm = with_tail(a, e);
        launch_conv1d(a, s, rt_num * e.num);
        if (tm) launch_tail_fill(a.y, a.y_bstride, B, a.M, a.T, tm->bn, tm->map, s, tm->pack_blocks > 0);
        if (conc && e.epi == EPI_RESID_ACC) HIPCHK(m, hipEventRecord(m->ev_rb[j], s));
        if (!first) state = r;
      }
    }
    return 0;
    };
    if (resblocks()) {
      if (conc) for (auto& st : m->aux) (void)hipStreamSynchronize(st);
      return 1;
    }
    if (conc) HIPCHK(m, hipStreamWaitEvent(s_main, m->ev_rb[2], 0));
    m->stage(i == 0 ? "dec_res_0" : "dec_res_1", xs, (int64_t)n, m->scrB);
    cur = xs;
  }
  const DecLaunch &post = table[next], &wave = table[next + 1];
  const bool sb = wave.bands == 1;
  const int L = post.num * Td, Fr = L + post.add, prow = post.M, Bc = d.Bc;
  const int bins = wave.n_fft / 2 + 1;             // rows of spec / phase per band
  float* const xpost = d.xpost;
  // ranged: window sub-band samples (MB / MS) or output quads (SB) of the kept frames, 64 per z-frame either way
  const int upf = wave.rate / 4;                   // those units per z-frame
  IstftRange keep{rg ? upf * rg->keep_first : 0, rg ? upf * (rg->keep_first + rg->keep_count) : 0,
                  rg ? rg->o_row_stride : 0, nullptr, nullptr};
  if (rr) keep = IstftRange{0, upf * Td, rr->o_row_stride, rr->len, rr->row_map};      // every tile of the class, cut per row in the kernel
  const int64_t M4 = (int64_t)wave.rate * Td;      // waveform samples per utterance
  for (int b0 = 0; b0 < B; b0 += Bc) {
    const int nb = B - b0 < Bc ? B - b0 : Bc;
    {
      ConvArgs a = conv(post, m->conv_post, cur + (size_t)b0 * post.Cin * L, xpost, 0.01f, nb);   // F.leaky_relu default slope (models.py:363)
      if (rr) a.in_lens += b0;                         // (in frames of the unpadded input: us^2 len_b + 1 padded ones)
      if (nb == B) with_trim(a, post);                 // (a split run keeps every tile: the maps are per full batch)
      launch_conv1d(a, s);
    }
    if (b0 == 0) HIPCHK(m, hipEventRecord(m->evk[1], s));   // (a split run interleaves conv_post and iSTFT launches: evk_split below)
    // Only the one-shot decode takes o_mb / spec / phase and "trim" in the tail.  Ranged: this sub-batch's rows of the
    // caller's o; ragged: every row finds its own through row_map; pooled: through its PoolRow.
    const bool plain = !rg && !rr;
    float* const ob = pooled ? nullptr : rr ? o : o + (size_t)b0 * (rg ? rg->o_row_stride : M4);
    auto extra = [&](float* p, int64_t per_row) { return plain && p ? p + (size_t)b0 * per_row : nullptr; };
    IstftRange kb = keep;
    if (rr) { kb.row_lens += b0; kb.row_map += b0; }
    if (sb) {
      IstftSbArgs ia{};
      ia.x_post = xpost; ia.o = ob;
      ia.spec = extra(outs ? outs->spec : nullptr, bins * Fr);
      ia.phase = extra(outs ? outs->phase : nullptr, bins * Fr);
      ia.B = nb; ia.F = Fr; ia.exact_math = m->exact_math; ia.prescaled = 1;
      if (pooled) launch_istft_single_pool(ia, rg->rows + b0, rg->max_keep, s);
      else if (!plain) launch_istft_single_range(ia, kb, s);
      else launch_istft_single(ia, s);
    } else {
      IstftArgs ia{};
      const bool ms = c.decoder == MBV_DEC_MULTISTREAM;
      ia.x_post = xpost; ia.filt = m->W(m->filt.off); ia.o = ob;
      ia.o_mb = extra(outs ? outs->o_mb : nullptr, (ms ? wave.bands : 1) * M4);
      ia.spec = extra(outs ? outs->spec : nullptr, wave.bands * bins * Fr);
      ia.phase = extra(outs ? outs->phase : nullptr, wave.bands * bins * Fr);
      ia.B = nb; ia.Tp = Td; ia.multistream = ms;
      ia.fixed_bank = !ia.multistream; ia.exact_math = m->exact_math; ia.prescaled = 1;
      if (plain && d.trim && nb == B && !ia.o_mb && !ia.spec && !ia.phase) ia.trim_lens = zlens;
      if (pooled) launch_istft_pqmf_pool(ia, rg->rows + b0, rg->max_keep, s);
      else if (!plain) launch_istft_pqmf_range(ia, kb, s);
      else launch_istft_pqmf(ia, s);
    }
  }
  if (Bc == B) m->stage("x_post", xpost, (int64_t)B * prow * Fr, m->scrB);     // (a split run keeps only its last chunk)
  m->xpost_F = Fr;
  m->xpost_rows = prow;
  HIPCHK(m, hipEventRecord(m->evk[2], s));
  m->evk_set = true;
  m->evk_split = Bc < B;
  if (tail_drift) return m->fail("internal error: a tile map was planned for another tile width than its launch uses");
  if (route_drift) return m->fail("internal error: a %s run holds rows whose convs plan differently (ragged_classes out of step with run_decoder)", pooled ? "pooled" : "ragged");
  return 0;
}

// ------------------------------------------------------------------ row-exact ragged decode
// Classes of z-lengths 1 .. t_max: two lengths share a class iff every conv of the decoder, planned for an
// utterance of that length alone, lands on the same side of the one divide that changes a sample's chain of
// operations — the narrow kernel (sums start from the bias) or a tiled kernel (bias added last; BIG / SMALL / M64 /
// HALF / VS / SPLIT_BATCH compute an element with the same chain).  first[i] = the first length of class i.  In the
// split-K mode nothing is bitwise across launch sizes anyway: one class.
void ragged_classes(const mbv_config& c, int splitk, int t_max, std::vector<int>* first) {
  first->assign(1, 1);
  if (splitk) return;
  const std::vector<DecLaunch> table = decoder_table(c);
  std::vector<char> prev, cur;
  for (int len = 1; len <= t_max; ++len) {
    cur.clear();
    for (const DecLaunch& e : table) {
      if (e.kind == DL_TAIL) continue;
      const int r = conv1d_plan(dec_planner_args(e, len, 1, 0), false).route;
      cur.push_back(r == CONV_NARROW_M || r == CONV_NARROW_LAUNCH);
    }
    if (len > 1 && cur != prev) first->push_back(len);
    prev.swap(cur);
  }
}

// null, or why the lengths are refused
const char* ragged_lens_error(const int64_t* lens, int B, int Tp) {
  if (!lens) return "the per-row lengths are missing";
  for (int b = 0; b < B; ++b)
    if (lens[b] < 0 || lens[b] > Tp) return "a row length lies outside [0, t_frames]";
  return nullptr;
}

// One decoder run of the ragged decode: rows of one class, T = the longest of them
struct RaggedRun { std::vector<int> rows, lens; int Tc; };

// Host: the runs of a ragged decode of B rows with HOST lengths (already checked; clamped to Td here).  Rows of
// length 0 belong to no run.  A run's tensors stay below 2 GiB each, as a stand-alone decode's do
// (conv1d_narrow_supported tests it, and the route of a conv must not depend on the batch).
void ragged_plan(const mbv_config& c, const std::vector<int>& first, int B, int Td, const int64_t* lens,
                 std::vector<RaggedRun>* runs) {
  const int us = dec_us(c), I = c.inter_channels, C0 = c.upsample_initial_channel;
  std::vector<std::vector<int>> rows(first.size());
  auto len_of = [&](int b) { return (int)(lens[b] < Td ? lens[b] : Td); };
  for (int b = 0; b < B; ++b) {
    const int len = len_of(b);
    if (len <= 0) continue;
    size_t k = 0;
    while (k + 1 < first.size() && first[k + 1] <= len) ++k;
    rows[k].push_back(b);
  }
  runs->clear();
  for (const auto& cls : rows) {
    for (size_t at = 0; at < cls.size();) {
      RaggedRun r;
      r.Tc = 0;
      while (at < cls.size() && r.rows.size() < 65535) {
        const int len = len_of(cls[at]);
        const int64_t Tn = len > r.Tc ? len : r.Tc;
        int64_t per_row = (int64_t)I * Tn;
        if ((int64_t)(C0 >> 2) * us * us * Tn > per_row) per_row = (int64_t)(C0 >> 2) * us * us * Tn;
        if (72 * ((int64_t)us * us * Tn + 1) > per_row) per_row = 72 * ((int64_t)us * us * Tn + 1);
        if (!r.rows.empty() && (int64_t)(r.rows.size() + 1) * per_row * 4 >= (1ll << 31)) break;
        r.Tc = (int)Tn;
        r.rows.push_back(cls[at]); r.lens.push_back(len);
        ++at;
      }
      runs->push_back(std::move(r));
    }
  }
}

// ... with the classes of the handle's mode, scanned once up to the longest T' seen
void ragged_plan(mbv_model* m, int B, int Td, const int64_t* lens, std::vector<RaggedRun>* runs) {
  if (m->ragged_scanned < Td || m->ragged_splitk != m->splitk) {
    ragged_classes(m->cfg, m->splitk, Td, &m->ragged_first);
    m->ragged_scanned = Td; m->ragged_splitk = m->splitk;
  }
  ragged_plan(m->cfg, m->ragged_first, B, Td, lens, runs);
}

// Scratch of one run of a ragged or pooled decode: the rows' tables (ragged: source row, then the length at the three
// rates; pooled: a PoolRow each, then the three lengths), their z of `width` frames and g gathered, the decoder's.
// The runs of a call are ordered on the stream and share the arena: each is carved from the same offset.
struct RunBufs { PoolRow* rows; int* ints; float *zc, *gc; DecBufs dec; };
void carve_runs(const mbv_model* m, const std::vector<RaggedRun>& runs, const std::vector<int>* widths, bool with_g,
                Bump& sc, std::vector<RunBufs>* out) {
  const int I = m->cfg.inter_channels, gin = m->cfg.gin_channels;
  out->resize(runs.size());
  const size_t base = sc.off;
  size_t end = base;
  for (size_t r = 0; r < runs.size(); ++r) {
    const size_t n = runs[r].rows.size();
    const int T = widths ? (*widths)[r] : runs[r].Tc;
    RunBufs& b = (*out)[r];
    sc.off = base;
    b.rows = widths ? sc.take<PoolRow>(n) : nullptr;
    b.ints = sc.take<int>((widths ? 3 : 4) * n);
    b.zc = sc.take<float>(n * I * T);
    b.gc = with_g ? sc.take<float>(n * gin) : nullptr;
    carve_decoder(m, DecCall{(int)n, T, T, true, with_g, false, widths != nullptr, true}, sc, &b.dec);
    if (sc.off > end) end = sc.off;
  }
  sc.off = end;
}

// The ragged decode of z [B, I, zstride]: o row b = the stand-alone decode of z[b, :, :len_b] over [0, spf len_b),
// zeros behind.  One decoder run per RaggedRun, on its rows gathered into scratch (carve_runs, without widths).
int run_decoder_ragged(mbv_model* m, const float* z, int zstride, const float* gvec, int B, int Td,
                       const std::vector<RaggedRun>& runs, float* o, int64_t o_row_stride, hipStream_t s,
                       std::vector<RunBufs>& bufs) {
  const mbv_config& c = m->cfg;
  const int us = dec_us(c), I = c.inter_channels, gin = c.gin_channels;
  const int64_t spf = m->dec_table.back().rate;
  HIPCHK(m, hipMemset2DAsync(o, (size_t)o_row_stride * sizeof(float), 0, (size_t)(spf * Td) * sizeof(float), B, s));
  for (size_t k = 0; k < runs.size(); ++k) {
    const RaggedRun& run = runs[k];
    RunBufs& b = bufs[k];
    const size_t n = run.rows.size();
    const int Tc = run.Tc;
    int* const ints = b.ints;
    for (size_t f = 0; f < n; f += kRaggedChunk) {
      RaggedRowsArg r{};
      const int nn = (int)(n - f < (size_t)kRaggedChunk ? n - f : (size_t)kRaggedChunk);
      for (int i = 0; i < nn; ++i) { r.row[i] = run.rows[f + i]; r.len[i] = run.lens[f + i]; }
      launch_ragged_rows(r, nn, (int)f, us, ints, (int)n, s);
    }
    launch_gather_frames(z, (int64_t)I * zstride, zstride, ints, ints + n, (int)n, I, Tc, b.zc, s);
    if (b.gc) launch_gather_frames(gvec, gin, 1, ints, nullptr, (int)n, gin, 1, b.gc, s);
    const RaggedRows rr{ints + n, ints + 2 * n, ints + 3 * n, ints, o, o_row_stride,
                        *std::min_element(run.lens.begin(), run.lens.end())};
    if (run_decoder(m, b.zc, nullptr, b.gc, nullptr, s, b.dec, nullptr, &rr)) return 1;
  }
  return 0;
}

// ------------------------------------------------------------------ pooled ranged decode (mbv_decode_chunks)
// One chunk of one utterance as a row of a run: the z-window [wa, wa + len) that mbv_decode_range would decode for
// it, and the frames of the window that are kept.
struct ChunkWindow { int wa, len, keep_first; };
ChunkWindow chunk_window(const mbv_chunk& k, int Lc, int Rc) {
  const int wa = k.first - Lc > 0 ? k.first - Lc : 0;
  const int wb = (int64_t)k.first + k.count + Rc < k.t_frames ? k.first + k.count + Rc : k.t_frames;
  return {wa, wb - wa, k.first - wa};
}

// A pooled run's widest window and longest chunk
void pooled_run_extent(const mbv_chunk* chunks, const RaggedRun& run, int Lc, int Rc, int* Tw, int* max_count) {
  *Tw = 0; *max_count = 0;
  for (int i : run.rows) {
    const int len = chunk_window(chunks[i], Lc, Rc).len;
    if (len > *Tw) *Tw = len;
    if (chunks[i].count > *max_count) *max_count = chunks[i].count;
  }
}

// The chunks of one call, one decoder run per RaggedRun of their utterances' lengths (the classes of the ragged
// decode): the run's rows are the chunks' windows gathered into scratch (carve_runs, as wide as the run's widest
// window), decoded as ragged rows of their window lengths, planned as their utterances plan.  The tables travel as
// kernel arguments (upload_rows).
int run_decoder_pooled(mbv_model* m, const mbv_chunk* chunks, bool with_g, const std::vector<RaggedRun>& runs, int Lc, int Rc,
                       hipStream_t s, std::vector<RunBufs>& bufs) {
  const mbv_config& c = m->cfg;
  const int us = dec_us(c), I = c.inter_channels, gin = with_g ? c.gin_channels : 0;
  const int spf = m->dec_table.back().rate, upf = spf / 4;      // samples, and units of a kept range, per z-frame
  for (size_t r = 0; r < runs.size(); ++r) {
    const RaggedRun& run = runs[r];
    RunBufs& b = bufs[r];
    const size_t n = run.rows.size();
    int Tw, max_count;
    pooled_run_extent(chunks, run, Lc, Rc, &Tw, &max_count);
    int* const lens = b.ints;
    upload_rows<kPoolChunk>(n, b.rows, s, [&](size_t i) {
      const mbv_chunk& k = chunks[run.rows[i]];
      const ChunkWindow w = chunk_window(k, Lc, Rc);
      return PoolRow{k.z, k.z_stride, gin ? k.g : nullptr, k.o + (int64_t)spf * k.first, w.wa, w.len,
                     upf * w.keep_first, upf * (w.keep_first + k.count)};
    }, PoolRowLens{lens, (int)n, us});
    launch_gather_windows(b.rows, (int)n, I, Tw, b.zc, gin, b.gc, s);
    const RaggedRows rr{lens, lens + n, lens + 2 * n, nullptr, nullptr, 0,
                        *std::min_element(run.lens.begin(), run.lens.end())};
    DecodeRange rg{run.Tc, 0, max_count, nullptr, 0};
    rg.rows = b.rows; rg.max_keep = upf * max_count;
    if (run_decoder(m, b.zc, nullptr, b.gc, nullptr, s, b.dec, &rg, &rr)) return 1;
  }
  return 0;
}


// scratch of a WN stack: hbuf / acts [B, H, T], skip [B, max(H, I / 2), T], gc [B, 2 H layers], ustart wn_units_ints(B, T)
struct FlowBufs { float *hbuf, *acts, *skip, *gc; int* ustart; };
FlowBufs carve_flow(Bump& sc, const mbv_config& c, int B, int T, int layers) {
  const size_t BTH = (size_t)B * T * c.hidden_channels;
  FlowBufs p{};
  p.hbuf = sc.take<float>(BTH);
  p.acts = sc.take<float>(BTH);
  // (with `post` folded, `skip` holds m: I / 2 channel rows, which is more than H where inter_channels > 2 hidden_channels)
  p.skip = sc.take<float>((size_t)B * T * std::max(c.hidden_channels, c.inter_channels / 2));
  p.gc = sc.take<float>((size_t)B * 2 * c.hidden_channels * layers);
  p.ustart = sc.take<int>(wn_units_ints(B, T));
  return p;
}

// WN stack (modules.py:148-176): h -> skip; `nl` layers, gate conditioning from gvec.
// Fused path (default): one launch per layer over the units that hold valid frames, h ping-pongs
// between hbuf and acts (the old path's gated-activation buffer); afterwards only `skip` is meaningful,
// and only where the frame mask is 1 (every reader masks on load).
// Two-launch path (MBV_WN_FUSED=0, and large launches in the split-bf16 mode, see wn_takes_fused): gate conv,
// then res/skip conv.
struct WnFold { const PConv* rspf; int Cs; float* x1; int64_t x1_bstride; float sign;
                const PConv* in16f0; const PConv* pref; int Gi; const float* x0; int in_cb; };   // in16f0 != nullptr: `pre` folded as well
// can this WN stack take the fused one-launch-per-layer kernel (run_wn's test; run_coupling asks before it folds `post`)
// (r02f: the fused layer wins or ties at every size measured, down to one utterance = 9 workgroups —
// ljs_mini B=1 3.55 -> 3.11 ms, B=8 4.33 -> 3.68, ljs_mb B=8 9.69 -> 9.04, B=1 5.10 -> 5.14.
// Split-bf16 mode: the two-launch layer on the conv kernel, which has the mode — from ~12 k frames up the
// gate conv + res/skip conv in split-bf16 beat the fused exact layer: ljs_mb B=64 23.6 -> 22.3 ms per infer,
// uudb B=32 15.7 -> 14.9; B=16: 8.9 -> 9.0, so smaller launches keep the fused layer.)
bool wn_takes_fused(const mbv_model* m, const PConv* in_l, const PConv* in16_l, int B, int T) {
  const int H = m->cfg.hidden_channels;
  const bool two_launch_bf16 = m->Wsplit(0) != nullptr && (long)B * T >= 12288;
  return !two_launch_bf16 && m->wn_fused && in16_l[0].M && wn_fused_supported(H, in_l[0].K) && wn_fused_fits(B, H, T);
}
[[nodiscard]] int run_wn(mbv_model* m, const PConv* in_l, const PConv* rs_l, const PConv* in16_l, const PConv* rsp_l,
                         int nl, const PVec& cw, const PVec& cb, const float* gvec, const FlowBufs& p, const int* lens,
                         int B, int T, hipStream_t s, const WnFold* fold = nullptr) {
  float *const hbuf = p.hbuf, *const acts = p.acts, *const skip = p.skip, *const gc = p.gc;
  int* const ustart = p.ustart;
  const mbv_config& c = m->cfg;
  const int H = c.hidden_channels, gin = c.gin_channels;
  const int64_t bsH = (int64_t)H * T;
  const bool cond = gvec && gin && cw.present;
  if (cond) launch_cond_gemv(gvec, nullptr, nullptr, m->W(cw.off), m->W(cb.off), gc, B, gin, 2 * H * nl, s);
  if (wn_takes_fused(m, in_l, in16_l, B, T)) {
    int* hmap = ustart + B + 1;
    launch_wn_units(lens, B, T, ustart, hmap, s);
    float* hin = hbuf;
    float* hout = acts;
    for (int l = 0; l < nl; ++l) {
      WnLayerArgs a{};
      a.h_in = hin; a.h_out = hout; a.skip = skip; a.lens = lens; a.ustart = ustart; a.hmap = hmap;
      a.wg = m->W(in16_l[l].w); a.bg = m->W(in16_l[l].bias);
      int Mg_pad = in16_l[l].Mpad;
      if (fold && fold->in16f0 && l == 0) {          // the first layer reads the x0 half of z itself
        a.h_in = fold->x0; a.in_cb = fold->in_cb; a.Gi = fold->Gi;
        a.wg = m->W(fold->in16f0->w); a.bg = m->W(fold->in16f0->bias); Mg_pad = fold->in16f0->Mpad;
        a.wpre = m->W(fold->pref->w); a.wpre_Mpad = fold->pref->Mpad;
      }
      if (cond) { a.gcond = gc + (size_t)l * 2 * H; a.gcond_bstride = 2 * H * nl; }
      const PConv& R = fold ? fold->rspf[l] : rsp_l[l];
      a.wr = m->W(R.w); a.br = m->W(R.bias);
      a.B = B; a.H = H; a.T = T;
      a.Mg_pad = Mg_pad; a.Mr = R.M; a.Mr_pad = R.Mpad;
      a.last = l == nl - 1; a.skip_accum = l > 0;
      if (fold) {
        a.Cs = fold->Cs;
        if (a.last) { a.x1 = fold->x1; a.x1_bstride = fold->x1_bstride; a.couple_sign = fold->sign; }
      }
      launch_wn_layer(a, s);
      float* tmp = hin; hin = hout; hout = tmp;
    }
    return 0;
  }
  for (int l = 0; l < nl; ++l) {
    {
      ConvArgs a = conv_args(m, in_l[l], hbuf, bsH, T, acts, bsH, T, B);
      a.epi = EPI_GATE; a.gate_half = H;
      if (cond) { a.gate_cond = gc + (size_t)l * 2 * H; a.gate_cond_bstride = 2 * H * nl; }
      launch_conv1d(a, s);
    }
    {
      ConvArgs a = conv_args(m, rs_l[l], acts, bsH, T, hbuf, bsH, T, B);
      a.epi = EPI_RES_SKIP; a.out_lens = lens; a.skip = skip;
      a.split = l < nl - 1 ? H : 0;
      a.skip_accum = l > 0;
      launch_conv1d(a, s);
    }
  }
  return 0;
}

// One ResidualCouplingLayer (modules.py:334-353) in place on z [B, I, T]; the channel Flip that
// precedes (reverse) / follows (forward) it is folded into the packing, see do_finalize.
//   reverse: x1 = (x1 - m) * mask          forward: x1 = m + x1 * mask = (x1 + m) * mask
[[nodiscard]] int run_coupling(mbv_model* m, int f, bool reverse, float* z, const float* gvec, const FlowBufs& p,
                               const int* lens, int B, int T, hipStream_t s, int route_T = 0) {
  const mbv_config& c = m->cfg;
  const int H = c.hidden_channels, I = c.inter_channels, half = I / 2;
  const int64_t bsI = (int64_t)I * T, bsH = (int64_t)H * T;
  const auto& F = m->flow[f];
  const bool flipped = (f % 2) == 1;
  float* x0 = flipped ? z + (size_t)half * T : z;
  float* x1 = flipped ? z : z + (size_t)half * T;
  // (the folded layers address x0 and x1 through whole-tensor views of z with 32-bit offsets, like h and skip)
  const bool fold_post = F.rspf[0].M && wn_takes_fused(m, F.in, F.in16, B, T) && wn_fused_fits(B, I, T);
  const bool fold_pre = fold_post && F.in16f0.M && F.pref.M;
  if (!fold_pre) {
    ConvArgs a = conv_args(m, F.pre, x0, bsI, T, p.hbuf, bsH, T, B);
    a.out_lens = lens;
    launch_conv1d(a, s, route_T);
  }
  if (fold_post) {
    // `post` lives in the res/skip convs (do_finalize): the last WN layer applies the coupling on the valid frames.
    // Frames at and beyond lens[b] are not touched: z arrives masked (expand_kernel / posterior_sample) and stays so.
    const WnFold fold{F.rspf, half, x1, bsI, reverse ? -1.f : 1.f,
                      fold_pre ? &F.in16f0 : nullptr, fold_pre ? &F.pref : nullptr, F.Gi, x0, I};
    return run_wn(m, F.in, F.rs, F.in16, F.rsp, kFlowLayers, F.cw, F.cb, gvec, p, lens, B, T, s, &fold);
  }
  if (int rc = run_wn(m, F.in, F.rs, F.in16, F.rsp, kFlowLayers, F.cw, F.cb, gvec, p, lens, B, T, s)) return rc;
  {
    ConvArgs a = conv_args(m, F.post, p.skip, bsH, T, x1, bsI, T, B);
    a.in_lens = lens; a.epi = EPI_COUPLE; a.out_lens = lens;
    a.couple_sign = reverse ? -1.f : 1.f;
    launch_conv1d(a, s, route_T);
  }
  return 0;
}

// The flow in place on z [B, I, T]: forward (models.py:207-211) the couplings 0 .. 3, reverse (:212-214) 3 .. 0.
// Returns the first non-zero status.
[[nodiscard]] int run_flows(mbv_model* m, bool reverse, float* z, const float* g, const FlowBufs& p, const int* lens,
                            int B, int T, hipStream_t s, int route_T = 0) {
  for (int i = 0; i < kNFlows; ++i)
    if (int rc = run_coupling(m, reverse ? kNFlows - 1 - i : i, reverse, z, g, p, lens, B, T, s, route_T)) return rc;
  return 0;
}

}  // namespace

// ======================================================================== C ABI
extern "C" {

int mbv_abi_version(void) { return MBV_ABI_VERSION; }

const char* mbv_last_error(const mbv_model* m) { return m ? m->err.c_str() : g_create_error.c_str(); }

int mbv_create(const mbv_config* cfg, mbv_model** out) {
  if (!out) { g_create_error = "out is NULL"; return 1; }
  *out = nullptr;
  if (!cfg || cfg->struct_bytes != (int32_t)sizeof(mbv_config)) {
    g_create_error = "mbv_config.struct_bytes does not match this library (ABI mismatch)";
    return 1;
  }
  auto bad = [&](const char* why) { g_create_error = why; return 1; };
  if (cfg->n_vocab <= 0) return bad("n_vocab must be > 0");
  if (cfg->hidden_channels % 32 || cfg->inter_channels % 64 || cfg->filter_channels % 32)
    return bad("hidden/filter channels must be multiples of 32, inter_channels of 64");
  if (cfg->hidden_channels > kDpFilter) return bad("hidden_channels > 256 not supported (LayerNorm tile)");
  if (cfg->n_heads <= 0 || cfg->hidden_channels % cfg->n_heads || (cfg->hidden_channels / cfg->n_heads) % 2 ||
      cfg->hidden_channels / cfg->n_heads > 128)
    return bad("hidden_channels / n_heads must be an even integer <= 128");
  if (cfg->upsample_initial_channel % 128) return bad("upsample_initial_channel must be a multiple of 128");
  if (cfg->decoder != MBV_DEC_MULTIBAND && cfg->decoder != MBV_DEC_MULTISTREAM &&
      cfg->decoder != MBV_DEC_SINGLEBAND)
    return bad("unknown decoder");
  if (cfg->n_speakers > 1 && cfg->gin_channels <= 0) return bad("n_speakers > 1 needs gin_channels > 0");
  for (int j = 0; j < 3; ++j)
    if (cfg->resblock_kernel_sizes[j] < 1 || cfg->resblock_kernel_sizes[j] % 2 == 0)
      return bad("resblock kernel sizes must be odd");
  if (cfg->resblock_type != 1 && cfg->resblock_type != 2) return bad("resblock_type must be 1 or 2");
  for (int j = 0; j < 3; ++j)
    for (int q = 0; q < (cfg->resblock_type == 1 ? 3 : 2); ++q)
      if (cfg->resblock_dilations[j][q] < 1 ||
          !conv1d_supported(cfg->resblock_kernel_sizes[j], cfg->resblock_dilations[j][q]))
        return bad("resblock kernel size / dilation outside the built range (k <= 11, (k-1)*d <= 72)");
  if (!conv1d_supported(cfg->kernel_size, 1)) return bad("FFN kernel_size outside the built range");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return bad("no HIP device visible: this library has no CPU fallback");
  if (cfg->device < 0 || cfg->device >= ndev) return bad("device ordinal out of range");
  DeviceGuard dev_guard_(cfg->device);
  if (!dev_guard_.ok) return bad("hipSetDevice failed");
  mbv_model* m = new (std::nothrow) mbv_model();
  if (!m) return bad("out of host memory");
  m->cfg = *cfg;
  m->dec_table = decoder_table(m->cfg);
  { const char* e = getenv("MBV_ISTFT_EXACT"); m->exact_math = (e && e[0] == '1') ? 1 : 0; }
  { const char* e = getenv("MBV_CONV_SPLITK"); m->splitk = (e && atoi(e) != 0) ? 1 : 0; }
  { const char* e = getenv("MBV_WN_FUSED"); m->wn_fused = e ? (atoi(e) != 0) : 1; }
  build_expected(m);
  for (auto& set : m->evr)
    for (auto& e : set)
      if (hipEventCreate(&e) != hipSuccess) { delete m; return bad("hipEventCreate failed"); }
  for (auto& e : m->evk)
    if (hipEventCreate(&e) != hipSuccess) { delete m; return bad("hipEventCreate failed"); }
  m->ev_ok = true;
  { const char* e = getenv("MBV_DEC_STREAMS"); m->dec_streams = e ? (atoi(e) != 0) : 1; }
  { const char* e = getenv("MBV_CONV_BF16"); m->conv_bf16 = (e && atoi(e) == 3) ? 3 : 0; }
  {
    bool ok = hipEventCreateWithFlags(&m->ev_fork, hipEventDisableTiming) == hipSuccess;
    for (auto& e : m->ev_rb) ok = ok && hipEventCreateWithFlags(&e, hipEventDisableTiming) == hipSuccess;
    for (auto& st : m->aux) ok = ok && hipStreamCreateWithFlags(&st, hipStreamNonBlocking) == hipSuccess;
    if (!ok) { delete m; return bad("creating the decoder's auxiliary streams failed"); }
    m->aux_ok = true;
  }
  {   // split-K scratch of small conv launches: 64 MB of partials, 8192 ticket counters (zeroed once;
      // the kernel resets a counter when its last split has arrived)
    constexpr size_t kWsFloats = (size_t)16 << 20;
    constexpr int kCounters = 8192;
    if (hipMalloc((void**)&m->conv_ws, kWsFloats * sizeof(float)) != hipSuccess ||
        hipMalloc((void**)&m->conv_cnt, kCounters * sizeof(unsigned)) != hipSuccess ||
        hipMemset(m->conv_cnt, 0, kCounters * sizeof(unsigned)) != hipSuccess) {
      mbv_destroy(m);
      return bad("hipMalloc of the split-K workspace failed");
    }
    m->conv_ws_floats = kWsFloats;
    m->conv_ncnt = kCounters;
  }
  // (the counter of mbv_tail_dropped: eight bytes the tail-map kernel adds to; only tests read it)
  if (hipMalloc((void**)&m->tail_cnt, sizeof(unsigned long long)) != hipSuccess ||
      hipMemset(m->tail_cnt, 0, sizeof(unsigned long long)) != hipSuccess) {
    mbv_destroy(m);
    return bad("hipMalloc of the tail-map counter failed");
  }
  *out = m;
  return 0;
}

int mbv_set_option(mbv_model* m, const char* name, int value) {
  if (!m) return 1;
  if (!name) return m->fail("mbv_set_option: name is NULL");
  DEVICE_GUARD(m);                 // conv_bf16 allocates and launches on the model's device, whatever the caller's current one
  if (!strcmp(name, "splitk")) { m->splitk = value != 0; return 0; }
  if (!strcmp(name, "istft_exact")) { m->exact_math = value != 0; return 0; }
  if (!strcmp(name, "wn_fused")) { m->wn_fused = value != 0; return 0; }
  if (!strcmp(name, "xpost_chunk_bytes")) { m->xpost_chunk_bytes = value > 0 ? value : 0; return 0; }
  if (!strcmp(name, "dec_streams")) { m->dec_streams = value != 0; return 0; }
  if (!strcmp(name, "trim")) { m->trim = value != 0; return 0; }
  if (!strcmp(name, "tail_once")) {
    if (value < 0 || value > 2) return m->fail("mbv_set_option: tail_once takes 0 (off), 1 (launches beyond one round of the grid) or 2 (every size)");
    m->tail_once = value;
    return 0;
  }
  if (!strcmp(name, "conv_bf16")) {
    if (value != 0 && value != 3) return m->fail("mbv_set_option: conv_bf16 takes 0 (exact fp32) or 3 (split-bf16, three products)");
    m->conv_bf16 = value;
    if (value == 3 && m->finalized && ensure_split_arena(m, nullptr)) return 1;
    return 0;
  }
  return m->fail("mbv_set_option: unknown option '%s' (known: splitk, istft_exact, wn_fused, xpost_chunk_bytes, dec_streams, trim, tail_once, conv_bf16)", name);
}

int mbv_get_option(mbv_model* m, const char* name) {
  if (!m || !name) return -1;
  if (!strcmp(name, "splitk")) return m->splitk;
  if (!strcmp(name, "istft_exact")) return m->exact_math;
  if (!strcmp(name, "wn_fused")) return m->wn_fused;
  if (!strcmp(name, "dec_streams")) return m->dec_streams;
  if (!strcmp(name, "trim")) return m->trim;
  if (!strcmp(name, "tail_once")) return m->tail_once;
  if (!strcmp(name, "conv_bf16")) return m->conv_bf16;
  m->fail("mbv_get_option: unknown option '%s' (known: splitk, istft_exact, wn_fused, dec_streams, trim, tail_once, conv_bf16)", name);
  return -1;
}

void mbv_destroy(mbv_model* m) {
  if (!m) return;
  DeviceGuard dev_guard_(m->cfg.device);
  if (m->darena) (void)hipFree(m->darena);
  if (m->darena_split) (void)hipFree(m->darena_split);
  if (m->conv_ws) (void)hipFree(m->conv_ws);
  if (m->conv_cnt) (void)hipFree(m->conv_cnt);
  if (m->tail_cnt) (void)hipFree(m->tail_cnt);
  if (m->scrA.p) (void)hipFree(m->scrA.p);
  if (m->scrB.p) (void)hipFree(m->scrB.p);
  if (m->noise_tab.p) (void)hipFree(m->noise_tab.p);
  if (m->voice_rows) (void)hipFree(m->voice_rows);
  if (m->voice_defined) (void)hipFree(m->voice_defined);
  if (m->voice_defs) (void)hipFree(m->voice_defs);
  for (auto& r : m->runs)
    if (r.own.p) (void)hipFree(r.own.p);
  if (m->user_tab) (void)hipFree(m->user_tab);
  if (m->peak_buf) (void)hipFree(m->peak_buf);
  for (auto& kv : m->resample_banks) (void)hipFree(kv.second.d);
  for (float* w : m->warp_win)
    if (w) (void)hipFree(w);
  for (auto& kv : m->spec_tables) { (void)hipFree(kv.second.tw); (void)hipFree(kv.second.win); }
  if (m->ev_ok) { for (auto& set : m->evr) for (auto& e : set) if (e) (void)hipEventDestroy(e); for (auto& e : m->evk) (void)hipEventDestroy(e); }
  if (m->aux_ok) {
    for (auto& st : m->aux) { (void)hipStreamSynchronize(st); (void)hipStreamDestroy(st); }
    (void)hipEventDestroy(m->ev_fork);
    for (auto& e : m->ev_rb) (void)hipEventDestroy(e);
  }
  delete m;
}

int mbv_load_weight(mbv_model* m, const char* name, const float* data, const int64_t* shape, int ndim) {
  if (!m) return 1;
  if (!name || !data || !shape || ndim <= 0) return m->fail("mbv_load_weight: NULL argument");
  auto it = m->expected.find(name);
  if (it == m->expected.end())
    return m->fail("'%s' is not a weight of the infer path (enc_q.* and training-only keys are not accepted)", name);
  const auto& want = it->second;
  bool ok = (int)want.size() == ndim;
  for (int i = 0; ok && i < ndim; ++i) ok = want[i] == shape[i];
  if (!ok) {
    std::string w, g;
    for (auto v : want) w += std::to_string(v) + ",";
    for (int i = 0; i < ndim; ++i) g += std::to_string(shape[i]) + ",";
    return m->fail("shape mismatch for '%s': expected [%s] got [%s]", name, w.c_str(), g.c_str());
  }
  HostTensor t;
  t.shape.assign(shape, shape + ndim);
  t.data.assign(data, data + t.numel());
  m->raw[name] = std::move(t);
  m->finalized = false;
  return 0;
}

int mbv_missing_weights(mbv_model* m, char* buf, size_t cap) {
  if (!m) return -1;
  int n = 0;
  std::string list;
  for (auto& kv : m->expected)
    if (!m->raw.count(kv.first)) { ++n; list += kv.first; list += ","; }
  if (buf && cap) { strncpy(buf, list.c_str(), cap - 1); buf[cap - 1] = 0; }
  return n;
}

int mbv_finalize_weights(mbv_model* m, void* stream) {
  if (!m) return 1;
  DEVICE_GUARD(m);
  return do_finalize(m, (hipStream_t)stream);
}

int64_t mbv_arena_floats(mbv_model* m) {
  if (!m) return -1;
  if (!m->finalized) { m->fail("weights not finalized"); return -1; }
  return (int64_t)m->arena_used;
}

int mbv_export_arena(mbv_model* m, float* dst, int64_t capacity, void* stream) {
  if (!m) return 1;
  if (!m->finalized) return m->fail("weights not finalized");
  if (!dst || capacity < (int64_t)m->arena_used) return m->fail("mbv_export_arena: destination holds %lld floats, the arena %zu", (long long)capacity, m->arena_used);
  DEVICE_GUARD(m);
  HIPCHK(m, hipMemcpyAsync(dst, m->darena, m->arena_used * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return 0;
}

int mbv_import_arena(mbv_model* m, const float* src, int64_t n_floats, void* stream) {
  if (!m) return 1;
  if (!src || n_floats <= 0) return m->fail("mbv_import_arena: bad arguments");
  DEVICE_GUARD(m);
  // the arena's layout is a function of the configuration alone (every offset comes from a tensor SHAPE): the same
  // packing pass runs over zero tensors, skipping the weight-norm folds, and the contents arrive from `src`
  m->import_src = src;
  m->import_n = n_floats;
  m->finalized = false;
  const int rc = do_finalize(m, (hipStream_t)stream);
  m->import_src = nullptr;
  if (rc) m->raw.clear();
  return rc;
}

int mbv_speaker_embedding(mbv_model* m, const int64_t* sid, int B, float* out, void* stream) {
  if (!m) return 1;
  if (!m->finalized) return m->fail("weights not finalized");
  if (!m->emb_g.present) return m->fail("model has no speaker embedding (n_speakers <= 1)");
  DEVICE_GUARD(m);
  launch_gather_rows(m->W(m->emb_g.off), sid, out, B, m->cfg.gin_channels, m->cfg.n_speakers, nullptr,
                     (hipStream_t)stream, m->voice_table());
  HIPCHK(m, hipGetLastError());
  return 0;
}

int mbv_speakers_define(mbv_model* m, const mbv_speaker_def* defs, int n, void* stream) {
  if (!m) return 1;
  const char* who = "mbv_speakers_define";
  if (!m->finalized) return m->fail("weights not finalized");
  if (!m->emb_g.present) return m->fail("model has no speaker embedding (n_speakers <= 1)");
  if (!defs || n < 1 || n > kVoiceSlots) return m->fail("%s: needs 1 .. %d definitions, got %d", who, kVoiceSlots, n);
  const int ns = m->cfg.n_speakers;
  std::vector<VoiceDef> rows((size_t)n);
  std::vector<char> seen(kVoiceSlots, 0);
  for (int i = 0; i < n; ++i) {
    const mbv_speaker_def& k = defs[i];
    if (k.slot < 0 || k.slot >= kVoiceSlots)
      return m->fail("%s: definition %d: slot %d outside [0, %d)", who, i, k.slot, kVoiceSlots);
    if (seen[k.slot]) return m->fail("%s: definition %d: slot %d is named twice", who, i, k.slot);
    seen[k.slot] = 1;
    VoiceDef& r = rows[i];
    r = VoiceDef{};
    r.slot = k.slot;
    r.vector = k.vector;
    if (k.vector) continue;
    if (k.count < 1 || k.count > kBlendMax)
      return m->fail("%s: definition %d: %d terms outside [1, %d]", who, i, k.count, kBlendMax);
    r.count = k.count;
    for (int j = 0; j < k.count; ++j) {
      if (k.ids[j] < 0 || k.ids[j] >= ns)
        return m->fail("%s: definition %d: term %d: speaker id %d outside [0, %d) (a blend names real speakers only)",
                       who, i, j, k.ids[j], ns);
      if (!std::isfinite(k.weights[j])) return m->fail("%s: definition %d: term %d: the weight is not finite", who, i, j);
      r.ids[j] = k.ids[j];
      r.weights[j] = k.weights[j];
    }
  }
  DEVICE_GUARD(m);
  if (blend_voices(m, rows, (hipStream_t)stream)) return 1;
  if (m->voices.empty()) m->voices.resize(kVoiceSlots);
  for (const VoiceDef& r : rows) {
    mbv_model::Voice& v = m->voices[r.slot];
    v.defined = true;
    v.vector = r.vector != nullptr;
    v.def = r;
    v.def.vector = nullptr;             // the row was copied: the caller's buffer is not kept
  }
  return 0;
}

int mbv_speaker_release(mbv_model* m, int slot, void* stream) {
  if (!m) return 1;
  if (slot < 0 || slot >= kVoiceSlots) return m->fail("mbv_speaker_release: slot %d outside [0, %d)", slot, kVoiceSlots);
  if ((size_t)slot >= m->voices.size() || !m->voices[slot].defined)
    return m->fail("mbv_speaker_release: slot %d is not defined", slot);
  DEVICE_GUARD(m);
  HIPCHK(m, hipMemsetAsync(m->voice_defined + slot, 0, sizeof(int), (hipStream_t)stream));
  m->voices[slot] = mbv_model::Voice{};
  return 0;
}

int mbv_speaker_slots(void) { return kVoiceSlots; }

int mbv_speaker_defined(mbv_model* m, int64_t sid) {
  if (!m) return -1;
  return sid >= m->cfg.n_speakers && m->speaker_ok(sid) ? 1 : 0;
}

int64_t mbv_speaker_runs(mbv_model* m) { return m ? m->speaker_runs : -1; }

namespace {
// DDSConv (modules.py:98-111) on x [B, C, T] in place; t1, t2: scratch of the same size
void run_dds(mbv_model* m, const EncRun& r, const mbv_model::Dds& d, float* x, float* t1, float* t2, int B, int C, int T,
             hipStream_t s) {
  const int64_t bs = (int64_t)C * T;
  int dil = 1;
  for (int i = 0; i < 3; ++i, dil *= 3) {
    launch_dds_sep(x, r.lens32, m->W(d.sw[i].off), m->W(d.sb[i].off), m->W(d.g1[i].off),
                   m->W(d.b1[i].off), t1, B, C, T, 3, dil, s);
    launch_conv1d(conv_args(m, d.c1[i], t1, bs, T, t2, bs, T, B), s);
    launch_dds_res(t2, x, m->W(d.g2[i].off), m->W(d.b2[i].off), x, B, C, T,
                   i == 2 ? r.lens32 : nullptr, s);
  }
}
struct ExactScope {
  mbv_model* m; int saved;
  explicit ExactScope(mbv_model* mm) : m(mm), saved(mm->conv_bf16) { m->conv_bf16 = 0; }
  ~ExactScope() { m->conv_bf16 = saved; }
};
// Phase A of mbv_encode: embedding, the attention layers and enc_p.proj (models.py:183-195) -> x [B, H, T] and
// r.stats = [m_text | logs_text] of the run it is given; shared with mbv_align.  Runs in the caller's ExactScope.
struct TextEncBufs { float *x, *x1, *qkv, *att, *y, *ffn; };
TextEncBufs carve_text(Bump& sc, const mbv_model* m, EncRun& r, int B, int T) {      // and r.stats [B, 2I, T]
  const size_t BT = (size_t)B * T, H = m->cfg.hidden_channels;
  TextEncBufs e{};
  e.x = sc.take<float>(BT * H);
  e.x1 = sc.take<float>(BT * H);
  e.qkv = sc.take<float>(BT * 3 * H);
  e.att = sc.take<float>(BT * H);
  e.y = sc.take<float>(BT * H);
  e.ffn = sc.take<float>(BT * m->cfg.filter_channels);
  r.stats = sc.take<float>(BT * 2 * m->cfg.inter_channels);
  return e;
}
// (a rule on T alone: rows stay batch-independent; the opt-in low-latency mode may look at the launch
// size: fused, a conv + LayerNorm is one workgroup per 32 frames walking the whole K loop alone)
bool text_fuse_ln_at(int splitk, int B, int T) { return T <= 256 && !(splitk && (long)B * ((T + 15) / 16) < 128); }
bool text_fuse_ln(const mbv_model* m, int B, int T) { return text_fuse_ln_at(m->splitk, B, T); }
void run_text_encoder(mbv_model* m, const EncRun& r, const int64_t* ids, const int64_t* lengths, const TextEncBufs& e, int* bad, int B,
                      int T, hipStream_t s) {
  const mbv_config& c = m->cfg;
  const int H = c.hidden_channels, I = c.inter_channels, Fc = c.filter_channels;
  float *x = e.x, *x1 = e.x1, *qkv = e.qkv, *att = e.att, *y = e.y, *ffn = e.ffn;
  ++m->encoder_runs;
  launch_embed(ids, lengths, m->W(m->emb.off), x, r.lens32, bad, B, T, H, c.n_vocab, s);
  const int64_t bsH = (int64_t)H * T;
  const bool fuse_ln = text_fuse_ln(m, B, T);
  for (int i = 0; i < c.n_layers; ++i) {
    const auto& L = m->enc[i];
    launch_conv1d(conv_args(m, L.qkv, x, bsH, T, qkv, 3 * bsH, T, B), s);
    launch_rel_attention(qkv, m->W(L.ek.off), m->W(L.ev.off), r.lens32, att, B, H, c.n_heads, T, s);
    // conv_o and the LayerNorm(x + y) behind it (attentions.py:40-41): one launch on the narrow kernel
    // for sequences it covers (a rule on T and H only), else conv + LayerNorm
    {
      ConvArgs a = conv_args(m, L.o, att, bsH, T, x1, bsH, T, B);
      a.epi = EPI_LN; a.res = x; a.res_bstride = bsH;
      a.ln_gamma = m->W(L.g1.off); a.ln_beta = m->W(L.b1.off);
      if (fuse_ln && conv1d_narrow_supported(a)) {
        launch_conv1d(a, s);
      } else {
        launch_conv1d(conv_args(m, L.o, att, bsH, T, y, bsH, T, B), s);
        launch_layernorm(x, y, m->W(L.g1.off), m->W(L.b1.off), x1, B, H, T, 0, nullptr, s);
      }
    }
    {
      ConvArgs a = conv_args(m, L.ffn1, x1, bsH, T, ffn, (int64_t)Fc * T, T, B);
      a.pad_left = (c.kernel_size - 1) / 2;            // attentions.py:296-303
      a.in_lens = r.lens32; a.relu = 1;
      launch_conv1d(a, s);
    }
    const bool last = i == c.n_layers - 1;
    {   // FFN's second conv (output masked, attentions.py:303) and LayerNorm(x1 + y) (+ the final mask, :45-46)
      ConvArgs a = conv_args(m, L.ffn2, ffn, (int64_t)Fc * T, T, x, bsH, T, B);
      a.pad_left = (c.kernel_size - 1) / 2;
      a.in_lens = r.lens32; a.out_lens = r.lens32;
      a.epi = EPI_LN; a.res = x1; a.res_bstride = bsH;
      a.ln_gamma = m->W(L.g2.off); a.ln_beta = m->W(L.b2.off);
      a.ln_out_lens = last ? r.lens32 : nullptr;
      if (fuse_ln && conv1d_narrow_supported(a)) {
        launch_conv1d(a, s);
      } else {
        a.epi = EPI_STORE; a.res = nullptr; a.y = y; a.ln_gamma = a.ln_beta = nullptr; a.ln_out_lens = nullptr;
        launch_conv1d(a, s);
        launch_layernorm(x1, y, m->W(L.g2.off), m->W(L.b2.off), x, B, H, T, 0, last ? r.lens32 : nullptr, s);
      }
    }
  }
  {
    ConvArgs a = conv_args(m, m->enc_proj, x, bsH, T, r.stats, (int64_t)2 * I * T, T, B);
    a.out_lens = r.lens32;
    launch_conv1d(a, s);
  }
}
// mbv_encode; rows_host != nullptr: mbv_encode_rows — the per-call scalars and the SDP noise come from the table,
// and rows with given durations have them set in the same call (the launches of mbv_set_durations).  `r` is the run it
// makes: laid out in r's own scratch (which ends the run r held), live and the handle's current one once all is launched
int encode(mbv_model* m, EncRun& r, const int64_t* ids, const int64_t* lengths, const int64_t* sid, int B,
           int T, float length_scale, const float* noise_w, float noise_scale_w, const mbv_enc_row* rows_host,
           int64_t* y_lengths_out, void* stream) {
  const char* const who = rows_host ? "mbv_encode_rows" : "mbv_encode";
  if (!m->finalized) return m->fail("weights not finalized (call mbv_finalize_weights)");
  if (!ids || !lengths || B <= 0 || T <= 0) return m->fail("%s: bad arguments", who);
  const mbv_config& c = m->cfg;
  if (c.n_speakers > 0 && !sid) return m->fail("sid is required when n_speakers > 0 (models.py:704-705)");
  if (c.n_speakers > 0 && !m->emb_g.present) return m->fail("n_speakers == 1: the reference has no emb_g either");
  DEVICE_GUARD(m);
  // The text encoder and the duration predictor ALWAYS run exact: the durations (ceil of an exponential) must
  // not depend on the opt-in split-bf16 mode, which is for the waveform path only.  (Long texts, T > 256,
  // use the conv kernels that have the mode; short ones the narrow kernel, which does not.)
  ExactScope exact_scope(m);
  hipStream_t s = (hipStream_t)stream;
  const int H = c.hidden_channels, I = c.inter_channels, gin = c.gin_channels;
  const size_t BT = (size_t)B * T;
  TextEncBufs te{};
  float *h1, *h2, *dpc;
  float *cond = nullptr, *hh = nullptr, *t1 = nullptr, *t2 = nullptr, *h29 = nullptr, *zf = nullptr;   // the SDP's
  AdmitEncRow* rows = nullptr;
  m->cur = -1;
  r.home = &r == m->runs ? &m->scrA : &r.own;
  if (lay_out(m, who, *r.home, [&](Bump& b) {
        te = carve_text(b, m, r, B, T);
        h1 = b.take<float>(BT * kDpFilter);
        h2 = b.take<float>(BT * kDpFilter);
        r.logw = b.take<float>(BT);
        r.w_ceil = b.take<float>(BT);
        r.cum = b.take<int>(BT);
        r.lens32 = b.take<int>(B);
        r.ylen32 = b.take<int>(B);
        r.bad32 = b.take<int>(B);
        r.gvec = b.take<float>((size_t)B * (gin ? gin : 1));
        dpc = b.take<float>((size_t)B * H);
        r.fit = b.take<float>((size_t)2 * B);
        if (rows_host) rows = b.take<AdmitEncRow>(B);
        if (c.use_sdp) {
          cond = b.take<float>(BT * H);
          hh = b.take<float>(BT * H);
          t1 = b.take<float>(BT * H);
          t2 = b.take<float>(BT * H);
          h29 = b.take<float>(BT * 32);
          zf = b.take<float>(BT * 2);
        }
      })) return 1;
  int* const bad = r.bad32;
  float* const x = te.x;
  bool any_given = false;
  if (rows_host)
    upload_rows<kAdmitChunk>(B, rows, (hipStream_t)stream, [&](size_t i) {
      const mbv_enc_row& k = rows_host[i];
      any_given = any_given || k.durations;
      return AdmitEncRow{k.length_scale, k.noise_scale_w, k.noise_w, k.durations, k.durations_dtype, k.t_text};
    });
  m->stages.clear();
  r.rows = rows_host != nullptr;
  r.scales.assign(r.rows ? (size_t)B : 1, length_scale);
  r.t_text.assign(r.rows ? (size_t)B : 0, 0);
  for (int i = 0; r.rows && i < B; ++i) { r.scales[i] = rows_host[i].length_scale; r.t_text[i] = rows_host[i].t_text; }

  ++m->ticket;                                     // a new call: its own set of stage events (mbv_stage_times_ms_at)
  m->ev = m->evr[m->ticket % mbv_model::kEvRing];
  m->evr_a[m->ticket % mbv_model::kEvRing] = false;
  m->evr_b[m->ticket % mbv_model::kEvRing] = false;
  HIPCHK(m, hipEventRecord(m->ev[0], s));
  run_text_encoder(m, r, ids, lengths, te, bad, B, T, s);
  const int64_t bsH = (int64_t)H * T;
  const bool fuse_ln = text_fuse_ln(m, B, T);
  r.x_enc = x;
  HIPCHK(m, hipEventRecord(m->ev[1], s));

  // ---- speaker embedding + duration predictor (models.py:704-713)
  r.has_g = c.n_speakers > 0;
  const float* cadd = nullptr;
  if (r.has_g) {
    launch_gather_rows(m->W(m->emb_g.off), sid, r.gvec, B, gin, c.n_speakers, bad, s, m->voice_table());
    if (m->dp_cw.present) {
      launch_cond_gemv(r.gvec, nullptr, nullptr, m->W(m->dp_cw.off), m->W(m->dp_cb.off), dpc, B, gin, H, s);
      cadd = dpc;
    }
  }
  if (c.use_sdp) {
    // models.py:53-60: conditioning trunk; :89-100: z through [Flip, ConvFlow] x 3, Flip, affine
    launch_conv1d(conv_args(m, m->sdp.pre, x, bsH, T, hh, bsH, T, B), s);
    if (cadd) launch_chan_add(hh, cadd, B, H, T, s);
    run_dds(m, r, m->sdp.dds, hh, t1, t2, B, H, T, s);
    {
      ConvArgs a = conv_args(m, m->sdp.proj, hh, bsH, T, cond, bsH, T, B);
      a.out_lens = r.lens32;
      launch_conv1d(a, s);
    }
    if (rows) launch_sdp_noise_rows(rows, zf, B, T, s);
    else launch_sdp_noise(noise_w, noise_scale_w, zf, (int64_t)BT * 2, s);
    for (int k = 0; k < 3; ++k) {
      const auto& f = m->sdp.flow[k];
      launch_sdp_pre(zf, 1, m->W(f.pre_w.off), m->W(f.pre_b.off), cond, hh, B, H, T, s);   // x0 = z[:, 1] after the Flip
      run_dds(m, r, f.dds, hh, t1, t2, B, H, T, s);
      {
        ConvArgs a = conv_args(m, f.proj, hh, bsH, T, h29, (int64_t)29 * T, T, B);
        a.out_lens = r.lens32;
        launch_conv1d(a, s);
      }
      launch_sdp_spline(h29, zf, r.lens32, B, H, T, m->sdp.edge_const, s);
    }
    launch_sdp_logw(zf, m->W(m->sdp.m.off), m->W(m->sdp.logs.off), r.lens32, h29, B, T, s);
    if (rows) launch_durations_rows(h29, nullptr, nullptr, r.lens32, rows, r.logw, r.w_ceil, r.cum, r.ylen32,
                                    y_lengths_out, bad, B, 1, T, s);
    else launch_durations(h29, nullptr, nullptr, r.lens32, length_scale, r.logw, r.w_ceil, r.cum,
                          r.ylen32, y_lengths_out, bad, B, 1, T, s);
    m->stage("sdp_cond", cond, (int64_t)BT * H, *r.home);
    m->stage("sdp_z", zf, (int64_t)BT * 2, *r.home);
  } else {
  // conv -> relu -> LayerNorm twice (models.py:128-135): each pair one launch where the narrow kernel applies
  const float* dp_out = h2;
  {
    ConvArgs a = conv_args(m, m->dp1, x, bsH, T, h2, (int64_t)kDpFilter * T, T, B);
    a.in_lens = r.lens32; a.chan_add = cadd;
    a.epi = EPI_LN; a.relu = 1; a.ln_gamma = m->W(m->dp_g1.off); a.ln_beta = m->W(m->dp_b1.off);
    if (fuse_ln && conv1d_narrow_supported(a)) {
      launch_conv1d(a, s);
    } else {
      a.epi = EPI_STORE; a.relu = 0; a.y = h1; a.ln_gamma = a.ln_beta = nullptr;
      launch_conv1d(a, s);
      launch_layernorm(h1, nullptr, m->W(m->dp_g1.off), m->W(m->dp_b1.off), h2, B, kDpFilter, T, 1, nullptr, s);
    }
  }
  {
    ConvArgs a = conv_args(m, m->dp2, h2, (int64_t)kDpFilter * T, T, h1, (int64_t)kDpFilter * T, T, B);
    a.in_lens = r.lens32;
    a.epi = EPI_LN; a.relu = 1; a.ln_gamma = m->W(m->dp_g2.off); a.ln_beta = m->W(m->dp_b2.off);
    if (fuse_ln && conv1d_narrow_supported(a)) {
      launch_conv1d(a, s);
      dp_out = h1;
    } else {
      a.epi = EPI_STORE; a.relu = 0; a.ln_gamma = a.ln_beta = nullptr;
      launch_conv1d(a, s);
      launch_layernorm(h1, nullptr, m->W(m->dp_g2.off), m->W(m->dp_b2.off), h2, B, kDpFilter, T, 1, nullptr, s);
    }
  }
  if (rows) launch_durations_rows(dp_out, m->W(m->dp_pw.off), m->W(m->dp_pb.off), r.lens32, rows, r.logw,
                                  r.w_ceil, r.cum, r.ylen32, y_lengths_out, bad, B, kDpFilter, T, s);
  else launch_durations(dp_out, m->W(m->dp_pw.off), m->W(m->dp_pb.off), r.lens32, length_scale, r.logw,
                        r.w_ceil, r.cum, r.ylen32, y_lengths_out, bad, B, kDpFilter, T, s);
  }
  if (any_given) launch_set_durations_rows(rows, r.lens32, r.w_ceil, r.cum, r.ylen32, y_lengths_out, bad, B, T, s);
  HIPCHK(m, hipEventRecord(m->ev[2], s));
  HIPCHK(m, hipGetLastError());
  r.B = B; r.T = T; r.claim = r.home->claim; m->cur = (int)(&r - m->runs); m->ev_a = true; m->ev_b = false;
  m->evr_a[m->ticket % mbv_model::kEvRing] = true;
  m->stage("x_enc", x, (int64_t)BT * H, *r.home);
  m->stage("stats", r.stats, (int64_t)BT * 2 * I, *r.home);
  m->stage("logw", r.logw, (int64_t)BT, *r.home);
  m->stage("w_ceil", r.w_ceil, (int64_t)BT, *r.home);
  return 0;
}
}  // namespace

int mbv_encode(mbv_model* m, const int64_t* ids, const int64_t* lengths, const int64_t* sid, int B,
               int T, float length_scale, const float* noise_w, float noise_scale_w,
               int64_t* y_lengths_out, void* stream) {
  if (!m) return 1;
  return encode(m, m->runs[0], ids, lengths, sid, B, T, length_scale, noise_w, noise_scale_w, nullptr, y_lengths_out, stream);
}

}  // extern "C"

namespace {
// The run a plain entry acts on: the one encoded or synthesised last, while nothing has laid out its scratch since
// (null, with the error set, otherwise).
EncRun* cur_run(mbv_model* m, const char* who) {
  if (!m) return nullptr;
  if (m->cur >= 0 && m->runs[m->cur].live()) return &m->runs[m->cur];
  m->fail("%s without a preceding mbv_encode", who);
  return nullptr;
}
// ... and the one a _rows entry acts on: slot's, live, made by mbv_encode_rows, of n rows
EncRun* rows_run(mbv_model* m, const char* who, int slot, const void* rows_host, int n) {
  if (!m) return nullptr;
  EncRun* r = slot >= 0 && slot < mbv_model::kSlots ? &m->runs[slot] : nullptr;
  if (!r || !r->live()) return m->fail("%s without a preceding mbv_encode_rows on slot %d", who, slot), nullptr;
  if (!r->rows) return m->fail("%s: slot %d holds no mbv_encode_rows run", who, slot), nullptr;
  if (!rows_host || n != r->B) return m->fail("%s: one row per encoded utterance expected (%d), got %d", who, r->B, n), nullptr;
  return r;
}

// what the ragged mode refuses, before anything is launched (null: nothing)
const char* ragged_mode_error(const mbv_model* m, const mbv_outputs* outs) {
  if (outs && (outs->o_mb || outs->spec || outs->phase)) return "the ragged decode writes the waveform only: o_mb / spec / phase must be NULL";
  if (m->trim) return "the options \"trim\" and the ragged decode exclude each other";
  if (m->conv_bf16) return "the ragged decode is not built for the \"conv_bf16\" mode";
  return nullptr;
}

// mbv_synthesize; y_lens_host != nullptr: the decoder in the row-exact ragged mode (mbv_synthesize_ragged)
int synthesize(mbv_model* m, const EncRun& r, int t_frames, const float* noise, float noise_scale, int max_len,
               const mbv_outputs* outs, const int64_t* y_lens_host, void* stream) {
  const char* const who = y_lens_host ? "mbv_synthesize_ragged" : "mbv_synthesize";
  if (t_frames <= 0) return m->fail("t_frames must be > 0");
  const mbv_config& c = m->cfg;
  std::vector<RaggedRun> runs;
  if (y_lens_host) {
    const char* why = ragged_mode_error(m, outs);
    if (!why) why = ragged_lens_error(y_lens_host, r.B, t_frames);
    if (why) return m->fail("%s: %s", who, why);
  }
  DEVICE_GUARD(m);
  hipStream_t s = (hipStream_t)stream;
  const int B = r.B, T = r.T, Tp = t_frames, I = c.inter_channels;
  const int Td = (max_len > 0 && max_len < Tp) ? max_len : Tp;
  const size_t BTp = (size_t)B * Tp;
  const bool run_dec = outs && (outs->o || outs->o_mb || outs->spec || outs->phase);
  if (y_lens_host && run_dec) ragged_plan(m, B, Td, y_lens_host, &runs);
  float* z;
  FlowBufs fb{};
  const bool with_g = r.has_g && c.gin_channels;
  DecBufs dec;
  std::vector<RunBufs> run_bufs;
  if (lay_out(m, who, m->scrB, [&](Bump& b) {
        z = outs && outs->z ? outs->z : b.take<float>(BTp * I);
        fb = carve_flow(b, c, B, Tp, kFlowLayers);
        if (run_dec && y_lens_host) carve_runs(m, runs, nullptr, with_g, b, &run_bufs);
        else if (run_dec) carve_decoder(m, DecCall{B, Td, Tp, true, with_g, !outs->o, false, false}, b, &dec);
      })) return 1;

  HIPCHK(m, hipEventRecord(m->ev[3], s));
  // m_text / logs_text are the two halves of enc_p.proj's output [B, 2I, T]
  launch_expand(r.stats, r.stats + (size_t)I * T, (int64_t)2 * I * T, r.cum, r.ylen32,
                noise_scale != 0.f ? noise : nullptr, noise_scale,
                outs ? outs->m_p : nullptr, outs ? outs->logs_p : nullptr, outs ? outs->z_p : nullptr, z,
                outs ? outs->attn : nullptr, outs ? outs->y_mask : nullptr, B, I, T, Tp, s);
  HIPCHK(m, hipEventRecord(m->ev[4], s));

  // ---- reverse flows, in place on z (models.py:207-214, modules.py:334-353)
  if (int rc = run_flows(m, true, z, r.has_g ? r.gvec : nullptr, fb, r.ylen32, B, Tp, s)) return rc;
  HIPCHK(m, hipEventRecord(m->ev[5], s));
  if (run_dec && y_lens_host) {
    if (run_decoder_ragged(m, z, Tp, r.has_g ? r.gvec : nullptr, B, Td, runs, outs->o, (int64_t)m->dec_table.back().rate * Td, s, run_bufs)) return 1;
  } else if (run_dec) {
    if (run_decoder(m, z, r.ylen32, r.has_g ? r.gvec : nullptr, outs, s, dec)) return 1;
  }
  HIPCHK(m, hipEventRecord(m->ev[6], s));
  HIPCHK(m, hipGetLastError());
  m->ev_b = true;
  m->evr_b[m->ticket % mbv_model::kEvRing] = true;
  return 0;
}

// ------------------------------------------------------------------ pooled admission
// Which side of the planner's one arithmetic divide — the narrow kernel or a tiled one — every conv in front of the
// flows takes when B utterances padded to T tokens are encoded in one run (the shapes run_text_encoder and encode
// build; data pointers are only ever tested against null), and whether the conv + LayerNorm pairs run fused.
void front_signature(const mbv_config& c, int splitk, int B, int T, std::vector<char>* sig) {
  static const float kSome = 0.f;                   // "a tensor is given"
  const int H = c.hidden_channels, I = c.inter_channels, Fc = c.filter_channels;
  auto conv = [&](int Cin, int M, int K) { return conv_shape(Cin, M, K, 1, T, T, B, splitk); };
  sig->clear();
  const bool fuse = text_fuse_ln_at(splitk, B, T);
  auto plain = [&](const ConvArgs& a) {
    const int r = conv1d_plan(a, false).route;
    sig->push_back(r == CONV_NARROW_M || r == CONV_NARROW_LAUNCH);
  };
  auto with_ln = [&](ConvArgs a, bool res) {       // fused with its LayerNorm where encode fuses, else a plain conv
    ConvArgs l = a;
    l.epi = EPI_LN; l.ln_gamma = l.ln_beta = &kSome;
    if (res) { l.res = &kSome; l.res_bstride = a.y_bstride; }
    const bool fused = fuse && conv1d_narrow_supported(l);
    sig->push_back(fused);
    if (!fused) plain(a);
  };
  plain(conv(H, 3 * H, 1));                         // attention: qkv, conv_o + LayerNorm
  with_ln(conv(H, H, 1), true);
  plain(conv(H, Fc, c.kernel_size));                // FFN
  with_ln(conv(Fc, H, c.kernel_size), true);
  plain(conv(H, 2 * I, 1));                         // enc_p.proj
  if (c.use_sdp) {
    plain(conv(H, H, 1));                           // dp.pre / dp.proj / the DDSConv 1x1 convs
    plain(conv(H, 29, 1));                          // ConvFlow.proj
  } else {
    with_ln(conv(H, kDpFilter, 3), false);
    with_ln(conv(kDpFilter, kDpFilter, 3), false);
  }
}

// The greedy planner of every pooled entry.  Each length's B = 1 signature is cached; a request joins the first open run
// of its class (its signature) that still fits and still plans the same way at B + 1 rows padded to the new maximum,
// else that run is closed — later requests of the class start a new one — and a new run is opened.  signature(B, T,
// &sig) may leave sig empty: one class.  Per-request refusals are the caller's, in front of the call.  Returns the
// number of runs.
template <typename Signature, typename Fits>
int plan_runs(int n, const int32_t* lengths, Signature signature, Fits fits, int32_t* run_of) {
  struct Run { std::vector<char> sig; int B = 0, T = 0; bool open = true; };
  std::vector<Run> runs;
  std::map<int, std::vector<char>> sig_of;          // length -> its stand-alone signature
  std::vector<char> sig;
  for (int i = 0; i < n; ++i) {
    const int T = lengths[i];
    auto it = sig_of.find(T);
    if (it == sig_of.end()) {
      signature(1, T, &sig);
      it = sig_of.emplace(T, sig).first;
    }
    int r = -1;
    for (size_t k = 0; k < runs.size() && r < 0; ++k) {
      if (!runs[k].open || runs[k].sig != it->second) continue;
      const int Tn = T > runs[k].T ? T : runs[k].T;
      bool ok = fits(runs[k].B + 1, Tn);
      if (ok) { signature(runs[k].B + 1, Tn, &sig); ok = sig == runs[k].sig; }
      if (ok) { r = (int)k; runs[k].T = Tn; ++runs[k].B; }
      else runs[k].open = false;
    }
    if (r < 0) {
      Run nr; nr.sig = it->second; nr.B = 1; nr.T = T;
      runs.push_back(nr);
      r = (int)runs.size() - 1;
    }
    if (run_of) run_of[i] = r;
  }
  return (int)runs.size();
}
inline void no_signature(int, int, std::vector<char>* sig) { sig->clear(); }   // split-K, live windows: one class

// Runs of one pooled admission for requests of t_text[i] tokens: requests share a front-half run iff their texts,
// each encoded alone, put every conv on the same side of the divide (front_signature at B = 1) — and a run is cut
// where its own launches, B rows padded to its longest text, would leave that side (tensors beyond the narrow
// kernel's 32-bit offsets) or the grid's 65535 rows.  Split-K mode: nothing is bitwise across launch sizes anyway,
// one class.  Returns the number of runs, -1 on a bad argument.
int admit_plan(const mbv_config& c, int splitk, int n, const int32_t* t_text, int32_t* run_of_request) {
  if (n <= 0 || !t_text) return -1;
  for (int i = 0; i < n; ++i)
    if (t_text[i] < 1) return -1;
  auto fits = [](int B, int) { return B <= 65535; };
  if (splitk) return plan_runs(n, t_text, no_signature, fits, run_of_request);
  return plan_runs(n, t_text, [&](int B, int T, std::vector<char>* sig) { front_signature(c, 0, B, T, sig); }, fits, run_of_request);
}
}  // namespace

extern "C" {

int mbv_synthesize(mbv_model* m, int t_frames, const float* noise, float noise_scale, int max_len,
                   const mbv_outputs* outs, void* stream) {
  const EncRun* r = cur_run(m, "mbv_synthesize");
  return r ? synthesize(m, *r, t_frames, noise, noise_scale, max_len, outs, nullptr, stream) : 1;
}

int mbv_synthesize_ragged(mbv_model* m, int t_frames, const float* noise, float noise_scale, int max_len,
                          const mbv_outputs* outs, const int64_t* y_lengths_host, void* stream) {
  if (!m) return 1;
  if (!y_lengths_host) return m->fail("mbv_synthesize_ragged: y_lengths_host is NULL");
  const EncRun* r = cur_run(m, "mbv_synthesize_ragged");
  return r ? synthesize(m, *r, t_frames, noise, noise_scale, max_len, outs, y_lengths_host, stream) : 1;
}

int mbv_admit_plan(const mbv_config* cfg, int splitk, int n, const int32_t* t_text, int32_t* run_of_request) {
  if (!cfg) return -1;
  return admit_plan(*cfg, splitk != 0, n, t_text, run_of_request);
}

int64_t mbv_encoder_runs(mbv_model* m) { return m ? m->encoder_runs : -1; }

int mbv_encode_rows(mbv_model* m, int slot, const int64_t* ids, const int64_t* lengths, const int64_t* sid, int B, int T,
                    const mbv_enc_row* rows_host, int64_t* y_lengths_out, void* stream) {
  if (!m) return 1;
  const char* who = "mbv_encode_rows";
  if (!rows_host || !y_lengths_out || B <= 0 || T <= 0) return m->fail("%s: bad arguments", who);
  if (slot < 0 || slot >= mbv_model::kSlots) return m->fail("%s: slot must be in [0, %d)", who, mbv_model::kSlots);
  if (B > 65535) return m->fail("%s: at most 65535 rows a run (mbv_admit_plan cuts there)", who);
  if (m->conv_bf16) return m->fail("%s: pooled admission is not built for the \"conv_bf16\" mode", who);
  for (int i = 0; i < B; ++i) {
    const mbv_enc_row& k = rows_host[i];
    if (k.t_text < 1 || k.t_text > T) return m->fail("%s: row %d: t_text %d outside [1, %d]", who, i, k.t_text, T);
    if (m->cfg.use_sdp && !k.noise_w) return m->fail("%s: row %d: noise_w is required with the stochastic duration predictor", who, i);
    if (k.durations && (k.durations_dtype < 0 || k.durations_dtype > 2))
      return m->fail("%s: row %d: durations_dtype must be 0 (int32), 1 (int64) or 2 (fp32)", who, i);
    if (k.durations && k.length_scale != 1.f)
      return m->fail("%s: row %d: given durations are used as they are: length_scale must be 1", who, i);
  }
  {   // the rows must be ONE run of the plan: a second class in the launch would move some row to another route
    std::vector<int32_t> tt(B);
    for (int i = 0; i < B; ++i) tt[i] = rows_host[i].t_text;
    if (admit_plan(m->cfg, m->splitk, B, tt.data(), nullptr) != 1)
      return m->fail("%s: the rows belong to more than one run of mbv_admit_plan", who);
  }
  return encode(m, m->runs[slot], ids, lengths, sid, B, T, 1.f, nullptr, 1.f, rows_host, y_lengths_out, stream);
}

int mbv_synthesize_rows(mbv_model* m, int slot, int t_frames, const mbv_row* rows_host, int n, void* stream) {
  const char* who = "mbv_synthesize_rows";
  const EncRun* r = rows_run(m, who, slot, rows_host, n);
  if (!r) return 1;
  if (t_frames <= 0) return m->fail("t_frames must be > 0");
  if (m->conv_bf16) return m->fail("%s: pooled admission is not built for the \"conv_bf16\" mode", who);
  const mbv_config& c = m->cfg;
  const int B = r->B, T = r->T, Tp = t_frames, I = c.inter_channels;
  int max_keep = 0;
  std::vector<AdmitSynRow> rows_h(n);
  for (int i = 0; i < n; ++i) {
    const mbv_row& k = rows_host[i];
    if (!k.z || k.keep < 1 || k.keep > Tp) return m->fail("%s: row %d: z missing or keep %d outside [1, %d]", who, i, k.keep, Tp);
    if (k.noise_scale != 0.f && (!k.noise || k.noise_stride < 1 || k.noise_stride > Tp))
      return m->fail("%s: row %d: noise missing or noise_stride outside [1, %d]", who, i, Tp);
    if (k.keep > max_keep) max_keep = k.keep;
    rows_h[i] = AdmitSynRow{k.noise, k.noise_stride, k.noise_scale, k.keep, k.z};
  }
  // the flows must take, for the whole run, the route every utterance takes alone: the fused WN layers, which work
  // on 16-frame half-units below each row's own length (the two-launch layers route on T')
  for (int f = 0; f < kNFlows; ++f)
    if (!wn_takes_fused(m, m->flow[f].in, m->flow[f].in16, B, Tp) || !wn_fused_fits(B, I, Tp))
      return m->fail("%s: a run of %d x %d frames is outside the fused WN layers (option \"wn_fused\" off, a hidden size they "
                     "do not cover, or tensors beyond their 32-bit offsets): admit fewer requests at a time", who, B, Tp);
  DEVICE_GUARD(m);
  hipStream_t s = (hipStream_t)stream;
  const size_t BTp = (size_t)B * Tp;
  float* z;
  FlowBufs fb{};
  AdmitSynRow* rows;
  if (lay_out(m, who, m->scrB, [&](Bump& b) {
        z = b.take<float>(BTp * I);
        fb = carve_flow(b, c, B, Tp, kFlowLayers);
        rows = b.take<AdmitSynRow>(B);
      })) return 1;
  m->cur = slot;                    // the plain entries act on this run from here on, as if mbv_encode had just made it
  upload_rows<kAdmitChunk>(B, rows, s, [&](size_t i) { return rows_h[i]; });
  launch_expand_rows(r->stats, r->stats + (size_t)I * T, (int64_t)2 * I * T, r->cum, r->ylen32, rows, z, B, I, T, Tp, s);
  if (int rc = run_flows(m, true, z, r->has_g ? r->gvec : nullptr, fb, r->ylen32, B, Tp, s)) return rc;
  launch_scatter_z_rows(z, r->ylen32, rows, B, I, Tp, max_keep, s);
  HIPCHK(m, hipGetLastError());
  return 0;
}

int mbv_ragged_classes(const mbv_config* cfg, int splitk, int t_max, int32_t* first, int capacity) {
  if (!cfg || t_max < 1 || capacity < 0 || (capacity > 0 && !first)) return -1;
  if (cfg->decoder != MBV_DEC_MULTIBAND && cfg->decoder != MBV_DEC_MULTISTREAM && cfg->decoder != MBV_DEC_SINGLEBAND) return -1;
  std::vector<int> f;
  ragged_classes(*cfg, splitk != 0, t_max, &f);
  for (size_t i = 0; i < f.size() && i < (size_t)capacity; ++i) first[i] = f[i];
  return (int)f.size();
}

// the runs of B rows of these lengths (classes scanned up to t_max); run_of_row[b] = -1 for an empty row
static int plan_rows(const mbv_config& cfg, int splitk, int B, int t_max, const int64_t* lengths, int32_t* run_of_row) {
  std::vector<int> first;
  ragged_classes(cfg, splitk != 0, t_max, &first);
  std::vector<RaggedRun> runs;
  ragged_plan(cfg, first, B, t_max, lengths, &runs);
  if (run_of_row) {
    for (int b = 0; b < B; ++b) run_of_row[b] = -1;
    for (size_t r = 0; r < runs.size(); ++r)
      for (int b : runs[r].rows) run_of_row[b] = (int32_t)r;
  }
  return (int)runs.size();
}

int mbv_ragged_plan(const mbv_config* cfg, int splitk, int B, int t_frames, const int64_t* lengths, int32_t* run_of_row) {
  if (!cfg || B <= 0 || t_frames < 1 || ragged_lens_error(lengths, B, t_frames)) return -1;
  if (cfg->decoder != MBV_DEC_MULTIBAND && cfg->decoder != MBV_DEC_MULTISTREAM && cfg->decoder != MBV_DEC_SINGLEBAND) return -1;
  return plan_rows(*cfg, splitk, B, t_frames, lengths, run_of_row);
}

int mbv_decode_ragged(mbv_model* m, const float* z, const float* g, int B, int t_frames, const int64_t* lengths_host,
                      float* o, void* stream) {
  if (!m) return 1;
  if (!m->finalized) return m->fail("weights not finalized");
  if (!z || !o || B <= 0 || t_frames <= 0) return m->fail("mbv_decode_ragged: bad arguments");
  const char* why = ragged_mode_error(m, nullptr);
  if (!why) why = ragged_lens_error(lengths_host, B, t_frames);
  if (why) return m->fail("mbv_decode_ragged: %s", why);
  const mbv_config& c = m->cfg;
  DEVICE_GUARD(m);
  std::vector<RaggedRun> runs;
  ragged_plan(m, B, t_frames, lengths_host, &runs);
  if (!c.gin_channels) g = nullptr;
  std::vector<RunBufs> bufs;
  if (lay_out(m, "mbv_decode_ragged", m->scrB, [&](Bump& b) { carve_runs(m, runs, nullptr, g != nullptr, b, &bufs); }))
    return 1;
  m->stages.clear();
  if (run_decoder_ragged(m, z, t_frames, g, B, t_frames, runs, o, (int64_t)m->dec_table.back().rate * t_frames, (hipStream_t)stream, bufs))
    return 1;
  HIPCHK(m, hipGetLastError());
  return 0;
}

// mbv_decode / mbv_decode_masked: one decoder run on the caller's z (lengths null: z as it is)
static int decode_entry(mbv_model* m, const char* who, const float* z, const float* g, const int32_t* lengths, int B,
                        int t_frames, const mbv_outputs* outs, void* stream) {
  if (!m) return 1;
  if (!m->finalized) return m->fail("weights not finalized");
  if (!z || B <= 0 || t_frames <= 0 || !outs) return m->fail("%s: bad arguments", who);
  const mbv_config& c = m->cfg;
  DEVICE_GUARD(m);
  if (!c.gin_channels) g = nullptr;
  DecBufs dec;
  if (lay_out(m, who, m->scrB, [&](Bump& b) {
        carve_decoder(m, DecCall{B, t_frames, t_frames, lengths != nullptr, g != nullptr, !outs->o, false, false}, b, &dec);
      })) return 1;
  m->stages.clear();
  if (run_decoder(m, z, lengths, g, outs, (hipStream_t)stream, dec)) return 1;
  HIPCHK(m, hipGetLastError());
  return 0;
}

int mbv_decode(mbv_model* m, const float* z, const float* g, int B, int t_frames,
               const mbv_outputs* outs, void* stream) {
  return decode_entry(m, "mbv_decode", z, g, nullptr, B, t_frames, outs, stream);
}

int mbv_decode_masked(mbv_model* m, const float* z, const float* g, const int32_t* lengths, int B, int t_frames,
                      const mbv_outputs* outs, void* stream) {
  if (m && !lengths) return m->fail("mbv_decode_masked: bad arguments");
  return decode_entry(m, "mbv_decode_masked", z, g, lengths, B, t_frames, outs, stream);
}

int mbv_decoder_context(const mbv_config* cfg, int32_t out[2]) {
  if (!cfg || !out) return 1;
  if (cfg->decoder != MBV_DEC_MULTIBAND && cfg->decoder != MBV_DEC_MULTISTREAM && cfg->decoder != MBV_DEC_SINGLEBAND) return 1;
  decoder_context(decoder_table(*cfg), &out[0], &out[1]);
  return 0;
}

int mbv_decode_range(mbv_model* m, const float* z, const float* g, int B, int t_frames, int first, int count,
                     float* o, int64_t o_row_stride, void* stream) {
  if (!m) return 1;
  if (!m->finalized) return m->fail("weights not finalized");
  if (!z || !o || B <= 0 || t_frames <= 0) return m->fail("mbv_decode_range: bad arguments");
  if (first < 0 || count <= 0 || first >= t_frames || count > t_frames - first)
    return m->fail("mbv_decode_range: frames [%d, %d + %d) outside [0, %d)", first, first, count, t_frames);
  const mbv_config& c = m->cfg;
  const int64_t spf = m->dec_table.back().rate;
  if (o_row_stride < spf * t_frames)
    return m->fail("mbv_decode_range: o_row_stride %lld < %lld samples per row", (long long)o_row_stride,
                   (long long)(spf * t_frames));
  if ((o_row_stride & 3) || ((uintptr_t)o & 15))
    return m->fail("mbv_decode_range: o must be 16-byte aligned and o_row_stride a multiple of 4");
  int Lc = 0, Rc = 0;
  decoder_context(m->dec_table, &Lc, &Rc);
  const int wa = first - Lc > 0 ? first - Lc : 0;
  const int wb = (int64_t)first + count + Rc < t_frames ? first + count + Rc : t_frames;
  const int Tw = wb - wa;
  DEVICE_GUARD(m);
  if (!c.gin_channels) g = nullptr;
  DecBufs dec;
  if (lay_out(m, "mbv_decode_range", m->scrB, [&](Bump& b) {
        carve_decoder(m, DecCall{B, Tw, t_frames, false, g != nullptr, false, true, false}, b, &dec);
      })) return 1;
  m->stages.clear();
  // the window [wa, wb) of the caller's z: conv_pre reads Tw frames at row stride t_frames, zeros beyond (a window
  // edge is padded exactly as a stand-alone decode pads its edges); the samples of frames within L / R of a window
  // edge that is not an utterance edge are not stored
  const DecodeRange rg{t_frames, first - wa, count, o + spf * first, o_row_stride};
  if (run_decoder(m, z + wa, nullptr, g, nullptr, (hipStream_t)stream, dec, &rg)) return 1;
  HIPCHK(m, hipGetLastError());
  return 0;
}

int mbv_chunks_plan(const mbv_config* cfg, int splitk, int n, const int32_t* t_frames, int32_t* run_of_chunk) {
  if (!cfg || n <= 0 || !t_frames) return -1;
  if (cfg->decoder != MBV_DEC_MULTIBAND && cfg->decoder != MBV_DEC_MULTISTREAM && cfg->decoder != MBV_DEC_SINGLEBAND) return -1;
  std::vector<int64_t> lens(n);
  int t_max = 0;
  for (int i = 0; i < n; ++i) {
    if (t_frames[i] < 1) return -1;
    lens[i] = t_frames[i];
    if (t_frames[i] > t_max) t_max = t_frames[i];
  }
  return plan_rows(*cfg, splitk, n, t_max, lens.data(), run_of_chunk);       // (no length is 0: every chunk is in a run)
}

int mbv_decode_chunks(mbv_model* m, const mbv_chunk* chunks_host, int n, void* stream) {
  return mbv_decode_chunks_routed(m, chunks_host, nullptr, n, stream);
}

int mbv_decode_chunks_routed(mbv_model* m, const mbv_chunk* chunks_host, const int32_t* route_frames, int n, void* stream) {
  if (!m) return 1;
  if (!m->finalized) return m->fail("weights not finalized");
  if (!chunks_host || n <= 0) return m->fail("mbv_decode_chunks: bad arguments");
  const char* why = ragged_mode_error(m, nullptr);
  if (why) return m->fail("mbv_decode_chunks: %s", why);
  const mbv_config& c = m->cfg;
  std::vector<int64_t> lens(n);
  int t_max = 0, with_g = 0;
  for (int i = 0; i < n; ++i) {
    const mbv_chunk& k = chunks_host[i];
    if (!k.z || !k.o || k.t_frames <= 0 || k.z_stride < k.t_frames)
      return m->fail("mbv_decode_chunks: chunk %d: z / o missing, t_frames <= 0 or z_stride < t_frames", i);
    if (k.first < 0 || k.count <= 0 || k.first >= k.t_frames || k.count > k.t_frames - k.first)
      return m->fail("mbv_decode_chunks: chunk %d: frames [%d, %d + %d) outside [0, %d)", i, k.first, k.first, k.count, k.t_frames);
    if ((uintptr_t)k.o & 15) return m->fail("mbv_decode_chunks: chunk %d: o must be 16-byte aligned", i);
    if (c.gin_channels && k.g) ++with_g;
    // the length that decides the class (and, through the run, the route of every conv): the utterance's own, or the
    // one the caller names for an utterance that is still growing
    const int route = route_frames && route_frames[i] ? route_frames[i] : k.t_frames;
    if (route < k.t_frames)
      return m->fail("mbv_decode_chunks: chunk %d: route_frames %d < t_frames %d", i, route, k.t_frames);
    lens[i] = route;
    if (route > t_max) t_max = route;
  }
  if (with_g && with_g != n) return m->fail("mbv_decode_chunks: g is given for %d of %d chunks (all or none)", with_g, n);
  int Lc = 0, Rc = 0;
  decoder_context(m->dec_table, &Lc, &Rc);
  DEVICE_GUARD(m);
  std::vector<RaggedRun> runs;
  ragged_plan(m, n, t_max, lens.data(), &runs);
  std::vector<int> widths(runs.size());
  for (size_t r = 0; r < runs.size(); ++r) { int mc; pooled_run_extent(chunks_host, runs[r], Lc, Rc, &widths[r], &mc); }
  std::vector<RunBufs> bufs;
  if (lay_out(m, "mbv_decode_chunks", m->scrB, [&](Bump& b) { carve_runs(m, runs, &widths, with_g != 0, b, &bufs); }))
    return 1;
  m->stages.clear();
  if (run_decoder_pooled(m, chunks_host, with_g != 0, runs, Lc, Rc, (hipStream_t)stream, bufs)) return 1;
  HIPCHK(m, hipGetLastError());
  return 0;
}

int64_t mbv_decoder_runs(mbv_model* m) { return m ? m->decoder_runs : -1; }

int mbv_tail_plan(const mbv_config* cfg, int32_t* out, int capacity) {
  if (!cfg || (capacity > 0 && !out) || capacity < 0) return -1;
  if (cfg->decoder != MBV_DEC_MULTIBAND && cfg->decoder != MBV_DEC_MULTISTREAM && cfg->decoder != MBV_DEC_SINGLEBAND) return -1;
  if (cfg->resblock_type != 1 && cfg->resblock_type != 2) return -1;
  std::vector<TailLaunch> plan;
  decoder_tail_plan(decoder_table(*cfg), &plan);
  for (size_t i = 0; i < plan.size() && (int)i < capacity; ++i) {
    const int32_t v[6] = {plan[i].kind, plan[i].stage, plan[i].j, plan[i].q, plan[i].rate, plan[i].reach};
    std::memcpy(out + 6 * i, v, sizeof v);
  }
  return (int)plan.size();
}

int64_t mbv_tail_dropped(mbv_model* m) {
  if (!m) return -1;
  DeviceGuard dev_guard_(m->cfg.device);
  unsigned long long v = 0;
  if (!dev_guard_.ok || hipDeviceSynchronize() != hipSuccess ||
      hipMemcpy(&v, m->tail_cnt, sizeof v, hipMemcpyDeviceToHost) != hipSuccess) { m->fail("mbv_tail_dropped: reading the counter failed"); return -1; }
  return (int64_t)v;
}

int mbv_stage_times_ms(mbv_model* m, float out[5]) {
  if (!m || !out) return 1;
  DEVICE_GUARD(m);
  if (!m->ev_a || !m->ev_b) return m->fail("no completed encode+synthesize pair to time");
  HIPCHK(m, hipEventSynchronize(m->ev[6]));
  HIPCHK(m, hipEventElapsedTime(&out[0], m->ev[0], m->ev[1]));
  HIPCHK(m, hipEventElapsedTime(&out[1], m->ev[1], m->ev[2]));
  HIPCHK(m, hipEventElapsedTime(&out[2], m->ev[3], m->ev[4]));
  HIPCHK(m, hipEventElapsedTime(&out[3], m->ev[4], m->ev[5]));
  HIPCHK(m, hipEventElapsedTime(&out[4], m->ev[5], m->ev[6]));
  return 0;
}

int64_t mbv_ticket(mbv_model* m) { return m ? m->ticket : -1; }

int mbv_stage_times_ms_at(mbv_model* m, int64_t ticket, float out[5]) {
  if (!m || !out) return 1;
  DEVICE_GUARD(m);
  if (ticket <= 0 || ticket > m->ticket) return m->fail("mbv_stage_times_ms_at: ticket %lld was never issued", (long long)ticket);
  if (ticket <= m->ticket - mbv_model::kEvRing)
    return m->fail("mbv_stage_times_ms_at: the events of call %lld were reused (%d calls are kept)", (long long)ticket, mbv_model::kEvRing);
  const int slot = (int)(ticket % mbv_model::kEvRing);
  if (!m->evr_a[slot] || !m->evr_b[slot]) return m->fail("call %lld has no completed encode+synthesize pair to time", (long long)ticket);
  hipEvent_t* ev = m->evr[slot];
  HIPCHK(m, hipEventSynchronize(ev[6]));
  HIPCHK(m, hipEventElapsedTime(&out[0], ev[0], ev[1]));
  HIPCHK(m, hipEventElapsedTime(&out[1], ev[1], ev[2]));
  HIPCHK(m, hipEventElapsedTime(&out[2], ev[3], ev[4]));
  HIPCHK(m, hipEventElapsedTime(&out[3], ev[4], ev[5]));
  HIPCHK(m, hipEventElapsedTime(&out[4], ev[5], ev[6]));
  return 0;
}

int mbv_kernel_times_ms(mbv_model* m, float out[2]) {
  if (!m || !out) return 1;
  DEVICE_GUARD(m);
  if (!m->evk_set) return m->fail("no decoder run to time");
  if (m->evk_split)
    return m->fail("kernel times unavailable: the last decoder run split its batch into sub-batches (x_post >= 2 GiB or "
                   "xpost_chunk_bytes), so conv_post and iSTFT launches interleave");
  HIPCHK(m, hipEventSynchronize(m->evk[2]));
  HIPCHK(m, hipEventElapsedTime(&out[0], m->evk[0], m->evk[1]));
  HIPCHK(m, hipEventElapsedTime(&out[1], m->evk[1], m->evk[2]));
  return 0;
}

int mbv_istft_pqmf(mbv_model* m, const float* x_post, int B, int t_frames, const float* filter,
                   int multistream, float* o, float* o_mb, float* spec, float* phase, void* stream) {
  if (!m) return 1;
  if (!x_post || !o || B <= 0 || t_frames <= 0) return m->fail("mbv_istft_pqmf: bad arguments");
  if ((int64_t)B * 72 * (16 * (int64_t)t_frames + 1) * 4 >= (1LL << 31))
    return m->fail("mbv_istft_pqmf: B * T' too large for one launch (x_post must stay below 2 GiB)");
  DEVICE_GUARD(m);
  hipStream_t s = (hipStream_t)stream;
  float*& d_tab = m->user_tab;
  if (!d_tab) HIPCHK(m, hipMalloc((void**)&d_tab, kFiltTable * sizeof(float)));
  if (filter || !m->user_tab_is_pqmf) {     // the default PQMF table is uploaded once, then launch-only
    std::vector<float> h63(4 * 63);
    if (filter) {
      HIPCHK(m, hipMemcpyAsync(h63.data(), filter, h63.size() * 4, hipMemcpyDeviceToHost, s));
      HIPCHK(m, hipStreamSynchronize(s));
    } else {
      h63 = pqmf_synthesis_filter();
    }
    const std::vector<float> tab = synthesis_table(h63.data());
    HIPCHK(m, hipMemcpyAsync(d_tab, tab.data(), kFiltTable * sizeof(float), hipMemcpyHostToDevice, s));
    HIPCHK(m, hipStreamSynchronize(s));
    m->user_tab_is_pqmf = filter == nullptr;
  }
  IstftArgs a{};
  a.x_post = x_post; a.filt = d_tab; a.o = o; a.o_mb = o_mb; a.spec = spec; a.phase = phase;
  a.B = B; a.Tp = t_frames; a.multistream = multistream & 1;
  a.fixed_bank = filter == nullptr; a.exact_math = m->exact_math; a.prescaled = (multistream >> 1) & 1;
  launch_istft_pqmf(a, s);
  HIPCHK(m, hipGetLastError());
  return 0;
}

}  // extern "C"

namespace {
// scratch of the posterior side (every entry that runs enc_q): ypad [B, cin_pad, T], the WN stack's of kEncQLayers
// layers (which the couplings' shorter stacks then use), stats [B, 2I, T]
struct PosteriorBufs : FlowBufs { float *ypad, *stats; };
PosteriorBufs carve_posterior(Bump& sc, const mbv_model* m, int B, int T) {
  const size_t BT = (size_t)B * T;
  PosteriorBufs p{};
  p.ypad = sc.take<float>(BT * m->encq.cin_pad);
  static_cast<FlowBufs&>(p) = carve_flow(sc, m->cfg, B, T, mbv_model::kEncQLayers);
  p.stats = sc.take<float>(BT * 2 * m->cfg.inter_channels);
  return p;
}
// enc_q (models.py:239-246): pre * mask -> WN(g) -> proj * mask -> z = (m_q + noise * noise_scale * exp(logs_q)) * mask.
// g == nullptr: the unconditioned WN of a single-speaker model.  y == nullptr: p.ypad holds the channel-padded input
// already (mbv_convert_rows: the spectrogram kernel wrote it); rows: per-row noise and noise_scale (the same entry).
// route_T > 0 (mbv_convert_ranges): the length the conv planner's narrow / tiled rule sees for pre and proj.
int run_enc_q(mbv_model* m, const float* y, const int* lens, const float* g, const float* noise, float noise_scale,
              const PosteriorBufs& p, float* z, int B, int T, hipStream_t s, const AdmitSynRow* rows = nullptr,
              int route_T = 0) {
  const mbv_config& c = m->cfg;
  const int H = c.hidden_channels, I = c.inter_channels, SC = c.spec_channels;
  const auto& Q = m->encq;
  const size_t BT = (size_t)B * T;
  // the 1x1 `pre` conv reads channel groups of 32: zero-pad spec_channels (513) to a multiple of 32
  if (y) {
    launch_fill(p.ypad, 0.f, (int64_t)BT * Q.cin_pad, s);
    HIPCHK(m, hipMemcpy2DAsync(p.ypad, (size_t)Q.cin_pad * T * 4, y, (size_t)SC * T * 4, (size_t)SC * T * 4, B,
                               hipMemcpyDeviceToDevice, s));
  }
  const int64_t bsH = (int64_t)H * T;
  {
    ConvArgs a = conv_args(m, Q.pre, p.ypad, (int64_t)Q.cin_pad * T, T, p.hbuf, bsH, T, B);
    a.out_lens = lens;
    launch_conv1d(a, s, route_T);
  }
  if (int rc = run_wn(m, Q.in, Q.rs, Q.in16, Q.rsp, mbv_model::kEncQLayers, Q.cw, Q.cb, g, p, lens, B, T, s)) return rc;
  {
    ConvArgs a = conv_args(m, Q.proj, p.skip, bsH, T, p.stats, (int64_t)2 * I * T, T, B);
    a.in_lens = lens; a.out_lens = lens;
    launch_conv1d(a, s, route_T);
  }
  if (rows) launch_posterior_sample_rows(p.stats, rows, lens, z, B, I, T, s);
  else launch_posterior_sample(p.stats, noise, lens, z, B, I, T, s, noise_scale);
  return 0;
}
}  // namespace

extern "C" {

int mbv_voice_conversion(mbv_model* m, const float* y, const int64_t* y_lengths, const int64_t* sid_src,
                         const int64_t* sid_tgt, int B, int T, const float* noise, const mbv_outputs* outs,
                         int32_t* status, void* stream) {
  if (!m) return 1;
  if (!m->finalized) return m->fail("weights not finalized");
  const mbv_config& c = m->cfg;
  if (c.n_speakers <= 0 || !m->emb_g.present)
    return m->fail("n_speakers have to be larger than 0.");              // models.py:791 assert
  if (!y || !y_lengths || !sid_src || !sid_tgt || !outs || B <= 0 || T <= 0)
    return m->fail("mbv_voice_conversion: bad arguments");
  DEVICE_GUARD(m);
  hipStream_t s = (hipStream_t)stream;
  const int I = c.inter_channels, gin = c.gin_channels;
  const size_t BT = (size_t)B * T;
  PosteriorBufs pb{};
  float *zbuf, *zhat, *g_src, *g_tgt;
  int *lens, *bad;
  DecBufs dec;
  if (lay_out(m, "mbv_voice_conversion", m->scrB, [&](Bump& b) {
        pb = carve_posterior(b, m, B, T);
        zbuf = outs->z ? outs->z : b.take<float>(BT * I);
        zhat = outs->m_p ? outs->m_p : b.take<float>(BT * I);
        g_src = b.take<float>((size_t)B * gin);
        g_tgt = b.take<float>((size_t)B * gin);
        lens = b.take<int>(B);
        bad = b.take<int>(B);
        carve_decoder(m, DecCall{B, T, T, true, gin > 0, !outs->o, false, false}, b, &dec);
      })) return 1;
  m->stages.clear();

  launch_lens_to_i32(y_lengths, lens, B, T, bad, s);
  launch_gather_rows(m->W(m->emb_g.off), sid_src, g_src, B, gin, c.n_speakers, bad, s, m->voice_table());
  launch_gather_rows(m->W(m->emb_g.off), sid_tgt, g_tgt, B, gin, c.n_speakers, bad, s, m->voice_table());
  if (status) HIPCHK(m, hipMemcpyAsync(status, bad, (size_t)B * sizeof(int), hipMemcpyDeviceToDevice, s));
  if (run_enc_q(m, y, lens, g_src, noise, 1.f, pb, zbuf, B, T, s)) return 1;
  // forward flow with the source speaker (models.py:795), then reverse with the target (:796)
  HIPCHK(m, hipMemcpyAsync(zhat, zbuf, BT * I * 4, hipMemcpyDeviceToDevice, s));
  if (int rc = run_flows(m, false, zhat, g_src, pb, lens, B, T, s)) return rc;
  if (outs->z_p) HIPCHK(m, hipMemcpyAsync(outs->z_p, zhat, BT * I * 4, hipMemcpyDeviceToDevice, s));
  if (int rc = run_flows(m, true, zhat, g_tgt, pb, lens, B, T, s)) return rc;
  if (outs->y_mask) launch_sequence_mask(lens, outs->y_mask, B, T, s);
  if (run_decoder(m, zhat, lens, g_tgt, outs, s, dec)) return 1;
  HIPCHK(m, hipGetLastError());
  return 0;
}

int mbv_align(mbv_model* m, const int64_t* ids, const int64_t* lengths, const float* y, const int64_t* y_lengths,
              const int64_t* sid, int B, int T_text, int T_spec, const float* noise, float noise_scale,
              const mbv_align_outputs* outs, int32_t* status, void* stream) {
  if (!m) return 1;
  if (!m->finalized) return m->fail("weights not finalized");
  if (!ids || !lengths || !y || !y_lengths || !outs || B <= 0 || T_text <= 0 || T_spec <= 0)
    return m->fail("mbv_align: bad arguments");
  const mbv_config& c = m->cfg;
  if ((c.n_speakers > 0) != (sid != nullptr))
    return m->fail("mbv_align: sid is required when n_speakers > 0 and must be NULL otherwise (models.py:661-664)");
  if (c.n_speakers > 0 && !m->emb_g.present) return m->fail("n_speakers == 1: the reference has no emb_g either");
  if (B > 65535 || T_spec > 65535) return m->fail("mbv_align: B and T_spec must be <= 65535");
  if (!max_path_supported(T_text)) return m->fail("mbv_align: T_text must be <= %d", kMaxPathMaxTs);
  DEVICE_GUARD(m);
  ExactScope exact_scope(m);                 // the text statistics as mbv_encode computes them; the path must not depend on the mode
  hipStream_t s = (hipStream_t)stream;
  const int I = c.inter_channels, gin = c.gin_channels;
  const int T = T_text, Tp = T_spec;
  const size_t BT = (size_t)B * T, BTp = (size_t)B * Tp;
  // ---- text side, in the scratch of mbv_encode: the claim ends the run that lived there, and `r` is this call's alone
  m->cur = -1;
  m->stages.clear();
  EncRun r;
  TextEncBufs te{};
  int *w32, *bad_y, *ylens, *mas;
  if (lay_out(m, "mbv_align", m->scrA, [&](Bump& b) {
        te = carve_text(b, m, r, B, T);
        r.cum = b.take<int>(BT);
        w32 = b.take<int>(BT);
        r.lens32 = b.take<int>(B);
        r.ylen32 = b.take<int>(B);
        r.bad32 = b.take<int>(B);
        bad_y = b.take<int>(B);
        ylens = b.take<int>(B);
        mas = b.take<int>(B);
        r.gvec = b.take<float>((size_t)B * (gin ? gin : 1));
      })) return 1;
  int* const bad_x = r.bad32;
  // ---- posterior side
  const size_t bits_bytes = max_path_scratch_bytes(B, Tp, T);
  PosteriorBufs pb{};
  float *zbuf, *zp, *value;
  void* bits = nullptr;
  if (lay_out(m, "mbv_align", m->scrB, [&](Bump& b) {
        pb = carve_posterior(b, m, B, Tp);
        zbuf = outs->z ? outs->z : b.take<float>(BTp * I);
        zp = outs->z_p ? outs->z_p : b.take<float>(BTp * I);
        value = outs->neg_cent ? outs->neg_cent : b.take<float>(BTp * T);
        if (bits_bytes) bits = b.take<char>(bits_bytes);
      })) return 1;
  int* w_out = outs->w ? outs->w : w32;

  run_text_encoder(m, r, ids, lengths, te, bad_x, B, T, s);
  const float* g = nullptr;
  if (c.n_speakers > 0) {
    launch_gather_rows(m->W(m->emb_g.off), sid, r.gvec, B, gin, c.n_speakers, bad_x, s, m->voice_table());
    g = r.gvec;
  }
  launch_lens_to_i32(y_lengths, ylens, B, Tp, bad_y, s);
  if (run_enc_q(m, y, ylens, g, noise_scale != 0.f ? noise : nullptr, noise_scale, pb, zbuf, B, Tp, s)) return 1;
  HIPCHK(m, hipMemcpyAsync(zp, zbuf, BTp * I * 4, hipMemcpyDeviceToDevice, s));
  if (int rc = run_flows(m, false, zp, g, pb, ylens, B, Tp, s)) return rc;
  // ---- neg_cent, the search, the durations (models.py:668-680)
  launch_neg_cent(zp, r.stats, r.stats + (size_t)I * T, (int64_t)2 * I * T, ylens, r.lens32, value, B, I, Tp, T, s);
  launch_max_path(value, ylens, r.lens32, w_out, nullptr, mas, bits, B, Tp, T, s);
  launch_align_status(bad_x, bad_y, mas, status, nullptr, nullptr, B, T, s);
  // ---- the path as length regulation takes it, and the expanded prior (:690-691)
  if (outs->attn || outs->m_p || outs->logs_p) {
    launch_set_durations(w_out, 0, r.lens32, nullptr, r.cum, r.ylen32, nullptr, nullptr, B, T, s);
    // (a refused row has w = 0: y_len 1 and no token for its frame; pb.stats is free again and takes the copy `z`)
    launch_expand(r.stats, r.stats + (size_t)I * T, (int64_t)2 * I * T, r.cum, r.ylen32, nullptr, 0.f, outs->m_p,
                  outs->logs_p, nullptr, pb.stats, outs->attn, nullptr, B, I, T, Tp, s);
  }
  if (outs->x_mask) launch_sequence_mask(r.lens32, outs->x_mask, B, T, s);
  if (outs->y_mask) launch_sequence_mask(ylens, outs->y_mask, B, Tp, s);
  HIPCHK(m, hipGetLastError());
  return 0;
}

int mbv_set_durations(mbv_model* m, const void* w, int dtype, int B, int T, int64_t* y_lengths_out, void* stream) {
  const EncRun* r = cur_run(m, "mbv_set_durations");
  if (!r) return 1;
  if (!w || !y_lengths_out) return m->fail("mbv_set_durations: NULL argument");
  if (dtype < 0 || dtype > 2) return m->fail("mbv_set_durations: dtype must be 0 (int32), 1 (int64) or 2 (fp32)");
  if (B != r->B || T != r->T) return m->fail("mbv_set_durations: w must be [%d, %d] as the encoded batch, got [%d, %d]", r->B, r->T, B, T);
  DEVICE_GUARD(m);
  launch_set_durations(w, dtype, r->lens32, r->w_ceil, r->cum, r->ylen32, y_lengths_out, r->bad32, B, T, (hipStream_t)stream);
  HIPCHK(m, hipGetLastError());
  return 0;
}

int mbv_token_marks(mbv_model* m, int64_t* marks, int64_t marks_stride, void* stream) {
  const EncRun* r = cur_run(m, "mbv_token_marks");
  if (!r) return 1;
  if (!marks || marks_stride < (int64_t)r->T + 1)
    return m->fail("mbv_token_marks: marks must be [%d, marks_stride >= %d]", r->B, r->T + 1);
  if (r->B > 65535) return m->fail("mbv_token_marks: more than 65535 rows");
  DEVICE_GUARD(m);
  launch_token_marks(r->cum, r->B, r->T, marks, marks_stride, r->T + 1, nullptr, (hipStream_t)stream);
  HIPCHK(m, hipGetLastError());
  return 0;
}

int mbv_token_marks_rows(mbv_model* m, int slot, const mbv_mark_row* rows_host, int n, void* stream) {
  const char* who = "mbv_token_marks_rows";
  const EncRun* r = rows_run(m, who, slot, rows_host, n);
  if (!r) return 1;
  const int B = r->B, T = r->T;
  bool any = false;
  for (int i = 0; i < n; ++i) {
    const mbv_mark_row& k = rows_host[i];
    if (k.marks && (k.count < 1 || k.count > T + 1))
      return m->fail("%s: row %d: count %d outside [1, t_text + 1 <= %d]", who, i, k.count, T + 1);
    any = any || k.marks;
  }
  if (!any) return 0;                                      // nothing to write
  DEVICE_GUARD(m);
  if (ensure(m, m->scrB, (size_t)n * sizeof(MarkRow))) return 1;
  hipStream_t s = (hipStream_t)stream;
  MarkRow* rows = reinterpret_cast<MarkRow*>(m->scrB.p);
  upload_rows<kAdmitChunk>(n, rows, s, [&](size_t i) { return MarkRow{rows_host[i].marks, rows_host[i].marks ? rows_host[i].count : 0, 0}; });
  launch_token_marks(r->cum, B, T, nullptr, 0, 0, rows, s);
  HIPCHK(m, hipGetLastError());
  return 0;
}

namespace {
// what a fit entry must be; null: fine (frames == 0: the row is not fitted)
const char* fit_error(const mbv_fit& f) {
  if (f.frames < 0) return "fit: frames must be >= 1 (0: no fit)";
  if (f.frames > 0 && !(f.lo > 0.f && f.lo <= f.hi && f.hi < INFINITY)) return "fit: the bounds must be 0 < lo <= hi < inf";
  return nullptr;
}
// the fit table of the batched forms (only frames / lo / hi are read), into scrB; *out = null when no row is fitted
int upload_fit(mbv_model* m, const mbv_fit* fit_host, int B, const ShapeRow** out, hipStream_t s) {
  *out = nullptr;
  bool any = false;
  for (int b = 0; fit_host && b < B; ++b) any = any || fit_host[b].frames > 0;
  if (!any) return 0;
  if (ensure(m, m->scrB, (size_t)B * sizeof(ShapeRow))) return 1;
  ShapeRow* t = reinterpret_cast<ShapeRow*>(m->scrB.p);
  upload_rows<kShapeChunk>(B, t, s, [&](size_t b) {
    ShapeRow r{};
    r.frames = fit_host[b].frames; r.lo = fit_host[b].lo; r.hi = fit_host[b].hi;
    return r;
  });
  *out = t;
  return 0;
}
}  // namespace

int mbv_shape_durations(mbv_model* m, const float* scale, const int32_t* extra, const mbv_fit* fit_host, int B, int T,
                        mbv_fit_result* fit_out, int64_t* y_lengths_out, void* stream) {
  const char* who = "mbv_shape_durations";
  const EncRun* r = cur_run(m, who);
  if (!r) return 1;
  if (!y_lengths_out) return m->fail("%s: NULL argument", who);
  if (B != r->B || T != r->T) return m->fail("%s: the tables must be [%d, %d] as the encoded batch, got [%d, %d]", who, r->B, r->T, B, T);
  if (r->rows) return m->fail("%s: the last encode was mbv_encode_rows (use mbv_shape_durations_rows)", who);
  bool any_fit = false;
  for (int b = 0; fit_host && b < B; ++b) {
    if (const char* why = fit_error(fit_host[b])) return m->fail("%s: row %d: %s", who, b, why);
    any_fit = any_fit || fit_host[b].frames > 0;
  }
  if (!scale && !extra && !any_fit) return m->fail("%s: nothing to do (no scale table, no extra frames, no fit)", who);
  if (scale && r->scales[0] != 1.f) return m->fail("%s: a scale table needs an encode with length_scale 1 (it was %g)", who, r->scales[0]);
  DEVICE_GUARD(m);
  hipStream_t s = (hipStream_t)stream;
  const ShapeRow* fit = nullptr;
  if (upload_fit(m, fit_host, B, &fit, s)) return 1;
  launch_shape_durations(r->logw, r->lens32, scale, extra, r->scales[0], fit, r->w_ceil, r->cum, r->ylen32, y_lengths_out,
                         r->bad32, r->fit, reinterpret_cast<FitOut*>(fit_out), B, T, s);
  ++m->shape_runs;
  HIPCHK(m, hipGetLastError());
  m->stage("fit_scale", r->fit, (int64_t)B, *r->home);
  m->stage("fit_status", r->fit + B, (int64_t)B, *r->home);
  return 0;
}

int mbv_shape_durations_rows(mbv_model* m, int slot, const mbv_shape_row* rows_host, int n, int64_t* y_lengths_out,
                             void* stream) {
  const char* who = "mbv_shape_durations_rows";
  const EncRun* r = rows_run(m, who, slot, y_lengths_out ? rows_host : nullptr, n);
  if (!r) return 1;
  const int T = r->T;
  std::vector<int> live;
  for (int i = 0; i < n; ++i) {
    const mbv_shape_row& k = rows_host[i];
    if (const char* why = fit_error(k.fit)) return m->fail("%s: row %d: %s", who, i, why);
    if (k.scale && r->scales[i] != 1.f)
      return m->fail("%s: row %d: a scale table needs a row encoded with length_scale 1 (it was %g)", who, i, r->scales[i]);
    if (k.scale || k.extra || k.fit.frames > 0) live.push_back(i);
  }
  if (live.empty()) return m->fail("%s: nothing to do (no row has a scale table, extra frames or a fit)", who);
  DEVICE_GUARD(m);
  if (ensure(m, m->scrB, live.size() * sizeof(ShapeRow))) return 1;
  hipStream_t s = (hipStream_t)stream;
  ShapeRow* rows = reinterpret_cast<ShapeRow*>(m->scrB.p);
  // (t_text: the row's tensors end there; the kernel also stops at the row's x_length)
  upload_rows<kShapeChunk>(live.size(), rows, s, [&](size_t j) {
    const mbv_shape_row& k = rows_host[live[j]];
    return ShapeRow{k.scale, k.extra, reinterpret_cast<FitOut*>(k.fit_out), k.fit.frames, k.fit.lo, k.fit.hi,
                    r->scales[live[j]], live[j], r->t_text[live[j]], 0};
  });
  launch_shape_durations_rows(r->logw, r->lens32, rows, (int)live.size(), r->w_ceil, r->cum, r->ylen32,
                              y_lengths_out, r->bad32, T, s);
  ++m->shape_runs;
  HIPCHK(m, hipGetLastError());
  return 0;
}

int64_t mbv_shape_runs(mbv_model* m) { return m ? m->shape_runs : -1; }

int mbv_frame_gain(mbv_model* m, const float* gain, float* out, int64_t out_stride, int frames, void* stream) {
  const char* who = "mbv_frame_gain";
  const EncRun* r = cur_run(m, who);
  if (!r) return 1;
  if (!gain || !out) return m->fail("%s: NULL argument", who);
  if (frames < 1 || frames > (1 << 30)) return m->fail("%s: frames must be in [1, 2^30], got %d", who, frames);
  if (out_stride < (int64_t)frames + 1) return m->fail("%s: out must be [%d, out_stride >= frames + 1 = %d]", who, r->B, frames + 1);
  if (r->B > 65535) return m->fail("%s: more than 65535 rows", who);
  DEVICE_GUARD(m);
  launch_frame_gain(r->cum, r->ylen32, nullptr, gain, out, out_stride, frames, r->B, r->T, (hipStream_t)stream);
  ++m->gain_runs;
  HIPCHK(m, hipGetLastError());
  return 0;
}

int mbv_frame_gain_rows(mbv_model* m, int slot, const mbv_gain_row* rows_host, int n, void* stream) {
  const char* who = "mbv_frame_gain_rows";
  const EncRun* r = rows_run(m, who, slot, rows_host, n);
  if (!r) return 1;
  const int T = r->T;
  std::vector<int> live;
  int max_frames = 0;
  for (int i = 0; i < n; ++i) {
    const mbv_gain_row& k = rows_host[i];
    if (!k.gain) {
      if (k.out || k.frames) return m->fail("%s: row %d: out / frames given without a gain", who, i);
      continue;
    }
    if (!k.out) return m->fail("%s: row %d: out missing", who, i);
    if (k.frames < 1 || k.frames > (1 << 30)) return m->fail("%s: row %d: frames must be in [1, 2^30], got %d", who, i, k.frames);
    live.push_back(i);
    max_frames = std::max(max_frames, (int)k.frames);
  }
  if (live.empty()) return 0;                              // nothing to write (a run holds at most 65535 rows: the grid's y)
  DEVICE_GUARD(m);
  if (ensure(m, m->scrB, live.size() * sizeof(GainRow))) return 1;
  hipStream_t s = (hipStream_t)stream;
  GainRow* rows = reinterpret_cast<GainRow*>(m->scrB.p);
  upload_rows<kAdmitChunk>(live.size(), rows, s, [&](size_t j) {
    const mbv_gain_row& k = rows_host[live[j]];
    return GainRow{k.gain, k.out, live[j], r->t_text[live[j]], k.frames, 0};
  });
  launch_frame_gain_rows(r->cum, r->ylen32, rows, (int)live.size(), max_frames, T, s);
  ++m->gain_runs;
  HIPCHK(m, hipGetLastError());
  return 0;
}

int64_t mbv_gain_runs(mbv_model* m) { return m ? m->gain_runs : -1; }

int mbv_istft_finalize(mbv_model* m, const float* spec, const float* phase, int B, int frames,
                       float* o, float* o_mb, void* stream) {
  if (!m) return 1;
  if (!m->finalized) return m->fail("weights not finalized");
  if (!spec || !phase || !o || B <= 0 || frames < 2) return m->fail("mbv_istft_finalize: bad arguments");
  const mbv_config& c = m->cfg;
  DEVICE_GUARD(m);
  hipStream_t s = (hipStream_t)stream;
  if (c.decoder == MBV_DEC_SINGLEBAND) {
    IstftSbArgs a{};
    a.o = o; a.spec = const_cast<float*>(spec); a.phase = const_cast<float*>(phase);
    a.B = B; a.F = frames; a.exact_math = m->exact_math; a.polar_in = 1;
    launch_istft_single(a, s);
  } else {
    if ((frames - 1) % 16) return m->fail("mbv_istft_finalize: frames must be 16 n + 1 for the 4-band decoders");
    if ((int64_t)B * 36 * frames * 4 >= (1LL << 31)) return m->fail("mbv_istft_finalize: tensor too large for one launch");
    IstftArgs a{};
    a.filt = m->W(m->filt.off); a.o = o; a.o_mb = o_mb;
    a.spec = const_cast<float*>(spec); a.phase = const_cast<float*>(phase);
    a.B = B; a.Tp = (frames - 1) / 16; a.multistream = c.decoder == MBV_DEC_MULTISTREAM;
    a.fixed_bank = !a.multistream; a.exact_math = m->exact_math; a.polar_in = 1;
    launch_istft_pqmf(a, s);
  }
  HIPCHK(m, hipGetLastError());
  return 0;
}

namespace {
// mbv_pcm16 (spf 256: lengths in z-frames) and mbv_pcm16_samples (spf 1: lengths in samples)
int pcm16(mbv_model* m, const char* who, const float* wave, const int64_t* lens, int B, int64_t stride, int spf,
          int auto_normalize, int16_t* pcm, void* stream) {
  if (!m) return 1;
  if (!wave || !pcm || B <= 0 || stride <= 0) return m->fail("%s: bad arguments", who);
  if (spf == 1 && B > 65535) return m->fail("%s: more than 65535 rows", who);
  DEVICE_GUARD(m);
  if (m->peak_cap < B) {
    if (m->peak_buf) HIPCHK(m, hipFree(m->peak_buf));
    HIPCHK(m, hipMalloc((void**)&m->peak_buf, (size_t)B * sizeof(unsigned)));
    m->peak_cap = B;
  }
  launch_pcm16(wave, lens, B, stride, spf, auto_normalize, m->peak_buf, reinterpret_cast<short*>(pcm), (hipStream_t)stream);
  HIPCHK(m, hipGetLastError());
  return 0;
}
}  // namespace

int mbv_pcm16(mbv_model* m, const float* wave, const int64_t* y_lengths, int B, int64_t stride,
              int auto_normalize, int16_t* pcm, void* stream) {
  return pcm16(m, "mbv_pcm16", wave, y_lengths, B, stride, 256, auto_normalize, pcm, stream);
}

int mbv_pcm16_samples(mbv_model* m, const float* wave, const int64_t* valid_samples, int B, int64_t stride,
                      int auto_normalize, int16_t* pcm, void* stream) {
  return pcm16(m, "mbv_pcm16_samples", wave, valid_samples, B, stride, 1, auto_normalize, pcm, stream);
}

int mbv_resample_bank(int orig_sr, int target_sr, int filter, float* dst, int64_t capacity, int32_t* phases,
                      int32_t* taps, int32_t* left) {
  ResampleGeom g{};
  std::vector<float> bank;
  const char* why = resample_bank(orig_sr, target_sr, filter, dst ? &bank : nullptr, &g);
  if (why) { g_create_error = std::string("mbv_resample_bank: ") + why; return 1; }
  if (phases) *phases = g.L;
  if (taps) *taps = g.K;
  if (left) *left = g.left;
  if (dst) {
    if (capacity < (int64_t)bank.size()) { g_create_error = "mbv_resample_bank: capacity too small"; return 1; }
    std::memcpy(dst, bank.data(), bank.size() * sizeof(float));
  }
  return 0;
}

}  // extern "C"

namespace {
// The rate pair and filter of a wire entry: validated and reduced to L / M.  Unequal rates (fir) also get the geometry
// and, with a handle, its device bank of the pair: the first call builds it on the host and uploads it once
// (synchronous copy).  Equal rates get neither (the sample itself), unless equal_is_fir asks for the L = M = 1 bank.
// Returns 0, or 1 with the reason in m->err (g_create_error without a handle).
struct RatePair {
  int L = 0, M = 0;
  bool fir = false;
  ResampleGeom g{};
  const float* bank = nullptr;
};
int rate_pair(mbv_model* m, const char* who, int orig_sr, int target_sr, int filter, RatePair* rp, bool equal_is_fir = false) {
  auto fail = [&](const std::string& why) { (m ? m->err : g_create_error) = std::string(who) + ": " + why; return 1; };
  if (filter != MBV_RESAMPLE_KAISER_BEST && filter != MBV_RESAMPLE_KAISER_FAST)
    return fail("unknown filter " + std::to_string(filter) + " (0 = kaiser_best, 1 = kaiser_fast)");
  if (resample_reduce(orig_sr, target_sr, &rp->L, &rp->M)) return fail("sample rates must be positive");
  rp->fir = equal_is_fir || orig_sr != target_sr;
  if (!rp->fir) return 0;
  if (!m) {
    const char* why = resample_bank(orig_sr, target_sr, filter, nullptr, &rp->g);
    return why ? fail(why) : 0;
  }
  const std::array<int, 3> key{rp->L, rp->M, filter};
  auto it = m->resample_banks.find(key);
  if (it == m->resample_banks.end()) {
    mbv_model::ResampleBank rb;
    std::vector<float> bank;
    const char* why = resample_bank(orig_sr, target_sr, filter, &bank, &rb.g);
    if (why) return m->fail("%s(%d -> %d): %s", who, orig_sr, target_sr, why);
    HIPCHK(m, hipMalloc((void**)&rb.d, bank.size() * sizeof(float)));
    if (hipMemcpy(rb.d, bank.data(), bank.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
      (void)hipFree(rb.d);
      return m->fail("%s: uploading the filter bank failed", who);
    }
    it = m->resample_banks.emplace(key, rb).first;
  }
  rp->g = it->second.g;
  rp->bank = it->second.d;
  return 0;
}

// Two rows of a pooled call must not write one sample.  Row i writes bytes(i) bytes from address lo(i); empty rows
// write nothing.  Returns the first pair that shares a byte, in address order, as (lower index, higher index), or
// (-1, -1).
template <typename Lo, typename Bytes>
std::pair<int, int> ranges_overlap(int n, Lo lo, Bytes bytes) {
  std::vector<int> order;
  for (int i = 0; i < n; ++i)
    if (bytes(i) > 0) order.push_back(i);
  std::sort(order.begin(), order.end(), [&](int a, int b) { return lo(a) < lo(b); });
  for (size_t j = 1; j < order.size(); ++j) {
    const int a = order[j - 1], b = order[j];
    if (lo(a) + bytes(a) > lo(b)) return {std::min(a, b), std::max(a, b)};
  }
  return {-1, -1};
}

// The grid's y limit: the table rows of a pooled call in slices of 65535, launch(first, rows, longest count of the slice)
template <typename Count, typename Launch>
int grid_y_slices(const std::vector<int>& live, Count count, Launch launch) {
  for (size_t f = 0; f < live.size(); f += 65535) {
    const size_t nn = std::min<size_t>(live.size() - f, 65535);
    int64_t max_count = 0;
    for (size_t i = 0; i < nn; ++i) max_count = std::max<int64_t>(max_count, count(live[f + i]));
    if (int rc = launch(f, (int)nn, max_count)) return rc;
  }
  return 0;
}
}  // namespace

extern "C" {

int mbv_resample(mbv_model* m, const float* wave, const int64_t* valid_samples, int B, int64_t in_stride,
                 int orig_sr, int target_sr, int filter, float* out, int64_t out_stride, int64_t* out_samples,
                 void* stream) {
  if (!m) return 1;
  if (!wave || !out || B <= 0 || in_stride <= 0 || out_stride <= 0) return m->fail("mbv_resample: bad arguments");
  if (B > 65535) return m->fail("mbv_resample: more than 65535 rows");
  if ((out_stride + kResampleTile - 1) / kResampleTile > 0x7fffffff) return m->fail("mbv_resample: out_stride too large");
  DEVICE_GUARD(m);
  RatePair rp;
  if (rate_pair(m, "mbv_resample", orig_sr, target_sr, filter, &rp, true)) return 1;
  if ((double)out_stride * rp.M >= 0x1p62) return m->fail("mbv_resample: out_stride * M overflows the 64-bit time index");
  launch_resample(wave, valid_samples, B, in_stride, rp.bank, rp.g, out, out_stride, out_samples, (hipStream_t)stream);
  HIPCHK(m, hipGetLastError());
  return 0;
}

int64_t mbv_resample_ready(int orig_sr, int target_sr, int filter, int64_t in_avail, int64_t in_total) {
  if (in_total < 0) { g_create_error = "mbv_resample_ready: in_total must be >= 0"; return -1; }
  RatePair rp;
  if (rate_pair(nullptr, "mbv_resample_ready", orig_sr, target_sr, filter, &rp)) return -1;
  if (!rp.fir) return in_avail < 0 ? 0 : (in_avail < in_total ? in_avail : in_total);
  return resample_ready(rp.g, in_avail, in_total);
}

}  // extern "C"

namespace {
// final outputs of a row with its first in_avail of in_total samples, under a limiter of that lookahead (0: none)
int64_t wire_ready(const RatePair& rp, int64_t in_avail, int64_t in_total, int lookahead) {
  const int64_t ready = rp.fir ? resample_ready(rp.g, in_avail, in_total) : (in_avail < in_total ? in_avail : in_total);
  return limiter_ready(ready, ready, in_avail >= in_total, lookahead);
}

// the limiter of a wire entry: refused, or too large for the LDS stage with this rate pair
const char* limit_refusal(const RatePair& rp, const mbv_pcm_limit& l) {
  const LimiterParams p{l.ceiling, l.lookahead, l.hold};
  if (const char* why = limiter_refusal(p)) return why;
  if (limiter_lds_floats(rp.g, rp.fir, p) > kResampleMaxLdsFloats)
    return "rate pair and limiter need a halo window larger than the LDS stage";
  return nullptr;
}

static_assert(MBV_G711_ULAW == kLawUlaw && MBV_G711_ALAW == kLawAlaw && MBV_WAVE_ULAW == kWaveUlaw &&
              MBV_WAVE_ALAW == kWaveAlaw, "G.711 numbers of the C-ABI and the kernels");

// the ramp factor of a fade of `count` samples, as mbv_pcm_fade_make computes it
float fade_inv(int64_t count) { return 1.0f / (float)(count + 1); }

// the fade of a *_faded entry (count < 0: none), or why it is refused
const char* fade_refusal(const mbv_pcm_fade& f) {
  if (f.count < 0) return nullptr;
  if (f.first < 0) return "fade first must be >= 0";
  const float want = fade_inv(f.count);
  if (memcmp(&f.inv, &want, sizeof want) != 0) return "fade inv is not the value mbv_pcm_fade_make gives for this count";
  return nullptr;
}

PcmFade fade_of(const mbv_pcm_fade* f) { return f && f->count >= 0 ? PcmFade{f->first, f->count, f->inv, 0} : kNoFade; }

// the envelope of a *_shaped entry over a row (or segment) of `in_total` model-rate samples (gain NULL: none), or why
// it is refused
const char* envelope_refusal(const mbv_pcm_envelope& e, int64_t in_total) {
  if (!e.gain) return e.frames || e.hop || e.inv_hop != 0.f ? "envelope without a gain table must be all zero" : nullptr;
  if (e.hop < 1) return "envelope hop must be >= 1";
  if (e.frames < 1) return "envelope frames must be >= 1";
  const float want = 1.0f / (float)e.hop;
  if (memcmp(&e.inv_hop, &want, sizeof want) != 0) return "envelope inv_hop is not 1.0f / (float)hop";
  if ((double)e.frames * (double)e.hop < (double)in_total) return "envelope covers frames * hop samples, fewer than the row holds";
  return nullptr;
}

PcmEnv env_of(const mbv_pcm_envelope* e) { return e && e->gain ? PcmEnv{e->gain, e->frames, e->hop, e->inv_hop} : kNoEnv; }

// the codec of a G.711 entry, or why it is refused
const char* law_refusal(int law) {
  return law == MBV_G711_ULAW || law == MBV_G711_ALAW ? nullptr : "unknown law (MBV_G711_ULAW 1, MBV_G711_ALAW 2)";
}

// mbv_resample_pcm16_range, its limited form, mbv_resample_g711_range and their faded forms: one body, lim null = no
// limiter, law kLawNone = int16 (else pcm holds bytes and pcm_stride counts them; the entry has checked law), fade null
// (or count < 0) = no fade
int pcm16_range(mbv_model* m, const char* who, const float* wave, const int64_t* valid_samples, int B, int64_t in_stride,
                int orig_sr, int target_sr, int filter, int64_t in_avail, int64_t out_first, int64_t out_count,
                const float* peak, void* pcm, int64_t pcm_stride, float* running_peak, int64_t* out_samples,
                const mbv_pcm_limit* lim, int law, void* stream, const mbv_pcm_fade* fade = nullptr,
                const mbv_pcm_envelope* env = nullptr, int64_t env_stride = 0) {
  if (!m) return 1;
  if (fade)
    if (const char* why = fade_refusal(*fade)) return m->fail("%s: %s", who, why);
  if (!wave || !pcm || B <= 0 || in_stride <= 0 || pcm_stride <= 0) return m->fail("%s: bad arguments", who);
  if (env) {
    if (const char* why = envelope_refusal(*env, in_stride)) return m->fail("%s: %s", who, why);
    if (!env->gain ? env_stride != 0 : (B > 1 && env_stride < env->frames + 1))
      return m->fail("%s: env_stride must be >= frames + 1 for B > 1 (0 without a gain table)", who);
  }
  if (B > 65535) return m->fail("%s: more than 65535 rows", who);
  if (in_avail < 0 || out_first < 0 || out_count < 0)
    return m->fail("%s: in_avail, out_first and out_count must be >= 0", who);
  DEVICE_GUARD(m);
  RatePair rp;
  if (rate_pair(m, who, orig_sr, target_sr, filter, &rp)) return 1;
  if (out_first > pcm_stride || out_count > pcm_stride - out_first)
    return m->fail("%s: outputs [%lld, %lld) lie outside the row of pcm_stride %lld", who, (long long)out_first,
                   (long long)(out_first + out_count), (long long)pcm_stride);
  if ((double)pcm_stride * rp.M >= 0x1p62) return m->fail("%s: pcm_stride * M overflows the 64-bit time index", who);
  if (lim)
    if (const char* why = limit_refusal(rp, *lim)) return m->fail("%s: %s", who, why);
  const int64_t ready = wire_ready(rp, in_avail, in_stride, lim ? lim->lookahead : 0);
  if (out_first + out_count > ready)
    return m->fail("%s: outputs up to %lld asked for, but %lld input samples of %lld make only %lld final", who,
                   (long long)(out_first + out_count), (long long)in_avail, (long long)in_stride, (long long)ready);
  if (out_count == 0 && !out_samples) return 0;           // nothing to write
  ++m->wire_runs;
  const LimiterParams lp = lim ? LimiterParams{lim->ceiling, lim->lookahead, lim->hold} : LimiterParams{};
  launch_resample_pcm16_range(wave, valid_samples, B, in_stride, in_avail, rp.bank, rp.g, out_first, out_count, peak,
                              pcm, pcm_stride, reinterpret_cast<unsigned*>(running_peak), out_samples,
                              lim ? &lp : nullptr, law, fade_of(fade), env_of(env), env_stride, (hipStream_t)stream);
  HIPCHK(m, hipGetLastError());
  return 0;
}
}  // namespace

extern "C" {

int mbv_resample_pcm16_range(mbv_model* m, const float* wave, const int64_t* valid_samples, int B, int64_t in_stride,
                             int orig_sr, int target_sr, int filter, int64_t in_avail, int64_t out_first,
                             int64_t out_count, const float* peak, int16_t* pcm, int64_t pcm_stride,
                             float* running_peak, int64_t* out_samples, void* stream) {
  return pcm16_range(m, "mbv_resample_pcm16_range", wave, valid_samples, B, in_stride, orig_sr, target_sr, filter,
                     in_avail, out_first, out_count, peak, pcm, pcm_stride, running_peak, out_samples, nullptr, kLawNone,
                     stream);
}

int mbv_resample_pcm16_range_limited(mbv_model* m, const float* wave, const int64_t* valid_samples, int B,
                                     int64_t in_stride, int orig_sr, int target_sr, int filter, int64_t in_avail,
                                     int64_t out_first, int64_t out_count, const float* peak, int16_t* pcm,
                                     int64_t pcm_stride, float* running_peak, int64_t* out_samples,
                                     const mbv_pcm_limit* limit, void* stream) {
  if (m && !limit) return m->fail("mbv_resample_pcm16_range_limited: limit missing");
  return pcm16_range(m, "mbv_resample_pcm16_range_limited", wave, valid_samples, B, in_stride, orig_sr, target_sr,
                     filter, in_avail, out_first, out_count, peak, pcm, pcm_stride, running_peak, out_samples, limit,
                     kLawNone, stream);
}

int mbv_resample_g711_range(mbv_model* m, const float* wave, const int64_t* valid_samples, int B, int64_t in_stride,
                            int orig_sr, int target_sr, int filter, int64_t in_avail, int64_t out_first,
                            int64_t out_count, const float* peak, uint8_t* out, int64_t out_stride, float* running_peak,
                            int64_t* out_samples, const mbv_pcm_limit* limit, int law, void* stream) {
  if (!m) return 1;
  if (const char* why = law_refusal(law)) return m->fail("mbv_resample_g711_range: %s, got %d", why, law);
  return pcm16_range(m, "mbv_resample_g711_range", wave, valid_samples, B, in_stride, orig_sr, target_sr, filter,
                     in_avail, out_first, out_count, peak, out, out_stride, running_peak, out_samples, limit, law, stream);
}

int mbv_pcm_fade_make(int64_t first, int64_t count, mbv_pcm_fade* out) {
  if (!out || first < 0 || count < 0) {
    g_create_error = "mbv_pcm_fade_make: first and count must be >= 0, out given";
    return -1;
  }
  *out = mbv_pcm_fade{first, count, fade_inv(count)};
  return 0;
}

int mbv_resample_pcm16_range_faded(mbv_model* m, const float* wave, const int64_t* valid_samples, int B,
                                   int64_t in_stride, int orig_sr, int target_sr, int filter, int64_t in_avail,
                                   int64_t out_first, int64_t out_count, const float* peak, int16_t* pcm,
                                   int64_t pcm_stride, float* running_peak, int64_t* out_samples,
                                   const mbv_pcm_limit* limit, const mbv_pcm_fade* fade, void* stream) {
  return pcm16_range(m, "mbv_resample_pcm16_range_faded", wave, valid_samples, B, in_stride, orig_sr, target_sr,
                     filter, in_avail, out_first, out_count, peak, pcm, pcm_stride, running_peak, out_samples, limit,
                     kLawNone, stream, fade);
}

int mbv_resample_g711_range_faded(mbv_model* m, const float* wave, const int64_t* valid_samples, int B,
                                  int64_t in_stride, int orig_sr, int target_sr, int filter, int64_t in_avail,
                                  int64_t out_first, int64_t out_count, const float* peak, uint8_t* out,
                                  int64_t out_stride, float* running_peak, int64_t* out_samples,
                                  const mbv_pcm_limit* limit, int law, const mbv_pcm_fade* fade, void* stream) {
  if (!m) return 1;
  if (const char* why = law_refusal(law)) return m->fail("mbv_resample_g711_range_faded: %s, got %d", why, law);
  return pcm16_range(m, "mbv_resample_g711_range_faded", wave, valid_samples, B, in_stride, orig_sr, target_sr, filter,
                     in_avail, out_first, out_count, peak, out, out_stride, running_peak, out_samples, limit, law, stream,
                     fade);
}

int mbv_resample_pcm16_range_shaped(mbv_model* m, const float* wave, const int64_t* valid_samples, int B,
                                    int64_t in_stride, int orig_sr, int target_sr, int filter, int64_t in_avail,
                                    int64_t out_first, int64_t out_count, const float* peak, void* out,
                                    int64_t out_stride, float* running_peak, int64_t* out_samples,
                                    const mbv_pcm_limit* limit, int law, const mbv_pcm_fade* fade,
                                    const mbv_pcm_envelope* envelope, int64_t env_stride, void* stream) {
  if (!m) return 1;
  const char* who = "mbv_resample_pcm16_range_shaped";
  if (law != kLawNone)
    if (const char* why = law_refusal(law)) return m->fail("%s: %s (0: int16), got %d", who, why, law);
  return pcm16_range(m, who, wave, valid_samples, B, in_stride, orig_sr, target_sr, filter, in_avail, out_first, out_count,
                     peak, out, out_stride, running_peak, out_samples, limit, law, stream, fade, envelope, env_stride);
}

int64_t mbv_limiter_ready(int orig_sr, int target_sr, int filter, int64_t in_avail, int64_t in_total, int lookahead) {
  const char* who = "mbv_limiter_ready";
  if (lookahead < 0 || lookahead > kLimiterMaxLookahead) {
    g_create_error = std::string(who) + ": limiter lookahead must be in [0, 255] output samples";
    return -1;
  }
  RatePair rp;
  if (rate_pair(nullptr, who, orig_sr, target_sr, filter, &rp)) return -1;
  if (in_avail < 0) in_avail = 0;
  if (in_total < 0) return limiter_ready(rp.fir ? resample_ready_open(rp.g, in_avail) : in_avail, 0, false, lookahead);
  return wire_ready(rp, in_avail, in_total, lookahead);
}

}  // extern "C"

namespace {
// The checks mbv_resample_pcm16_range makes on its row, for every chunk of a pooled call (integer fields only).
// Fills packed_first (may be null) with the running sum of the out_count and returns the packed total, or -1 with
// *err naming the offending chunk.
// `at(i)` is row i's mbv_pcm_chunk and `noun` what the messages call a row ("chunk", or "turn": mbv_turn_plan).
template <typename At>
int64_t pcm_rows_check(const char* who, const char* noun, At at, int n, const RatePair& rp, int64_t* packed_first,
                       std::string* err, const mbv_pcm_limit* limits) {
  char buf[512];
  int64_t total = 0;
  for (int i = 0; i < n; ++i) {
    const mbv_pcm_chunk& k = at(i);
    const char* why = nullptr;
    if (k.in_total <= 0 || k.pcm_capacity <= 0) why = "in_total and pcm_capacity must be > 0";
    else if (k.in_avail < 0 || k.out_first < 0 || k.out_count < 0) why = "in_avail, out_first and out_count must be >= 0";
    else if ((double)k.pcm_capacity * rp.M >= 0x1p62) why = "pcm_capacity * M overflows the 64-bit time index";
    if (why) {
      snprintf(buf, sizeof buf, "%s: %s %d: %s", who, noun, i, why);
      *err = buf;
      return -1;
    }
    if (k.out_first > k.pcm_capacity || k.out_count > k.pcm_capacity - k.out_first) {
      snprintf(buf, sizeof buf, "%s: %s %d: outputs [%lld, %lld) lie outside the row of pcm_capacity %lld", who, noun, i,
               (long long)k.out_first, (long long)(k.out_first + k.out_count), (long long)k.pcm_capacity);
      *err = buf;
      return -1;
    }
    const bool limited = limits && limits[i].ceiling != 0.f;
    if (limited)
      if (const char* bad = limit_refusal(rp, limits[i])) {
        snprintf(buf, sizeof buf, "%s: %s %d: %s", who, noun, i, bad);
        *err = buf;
        return -1;
      }
    const int64_t ready = wire_ready(rp, k.in_avail, k.in_total, limited ? limits[i].lookahead : 0);
    if (k.out_first + k.out_count > ready) {
      snprintf(buf, sizeof buf, "%s: %s %d: outputs up to %lld asked for, but %lld input samples of %lld make only %lld final",
               who, noun, i, (long long)(k.out_first + k.out_count), (long long)k.in_avail, (long long)k.in_total, (long long)ready);
      *err = buf;
      return -1;
    }
    if (packed_first) packed_first[i] = total;
    total += k.out_count;
  }
  return total;
}

int64_t pcm_chunks_check(const char* who, const mbv_pcm_chunk* chunks, int n, const RatePair& rp, int64_t* packed_first,
                         std::string* err, const mbv_pcm_limit* limits = nullptr) {
  return pcm_rows_check(who, "chunk", [&](int i) -> const mbv_pcm_chunk& { return chunks[i]; }, n, rp, packed_first, err,
                        limits);
}
}  // namespace

extern "C" {

int64_t mbv_pcm_chunks_plan(int orig_sr, int target_sr, int filter, const mbv_pcm_chunk* chunks, int n,
                            int64_t* packed_first) {
  const char* who = "mbv_pcm_chunks_plan";
  if (n < 0 || (n > 0 && !chunks)) { g_create_error = std::string(who) + ": bad arguments"; return -1; }
  RatePair rp;
  if (rate_pair(nullptr, who, orig_sr, target_sr, filter, &rp)) return -1;
  std::string err;
  const int64_t total = pcm_chunks_check(who, chunks, n, rp, packed_first, &err);
  if (total < 0) g_create_error = err;
  return total;
}

}  // extern "C"

namespace {
// The body the pooled wire entries share (mbv_resample_pcm16_chunks and its forms, mbv_resample_turns), behind their own
// checks: `at(i)` is row i's mbv_pcm_chunk, `noun` what the messages call a row, `off` / `total` what the plan returned.
// The rows without a limiter go through the unlimited instantiation and the limited ones through theirs: one row table
// and one launch per kind, and a kind with a fading row gets a fade table beside its rows, read by the same launch.
// `side` is what an entry has beside its rows: nothing (ChunkSide), or a turn's tables (TurnSide): `head_bytes` in front
// of everything, written by head(); `row_bytes` per row beside each kind's rows, written by rows(kind, ..); and
// turn_fields(launch, side rows, head), which names them in the launch of a slice.
template <typename At, typename Side>
int pooled_wire(mbv_model* m, const char* who, const char* noun, At at, const mbv_pcm_limit* limits,
                const mbv_pcm_fade* fades, int n, const RatePair& rp, const std::vector<int64_t>& off, int64_t total,
                int law, void* packed, int64_t packed_capacity, void* stream, const Side& side,
                const mbv_pcm_envelope* envs = nullptr) {
  if (packed && packed_capacity < total)
    return m->fail("%s: packed_capacity %lld is below the %lld samples of the call", who, (long long)packed_capacity, (long long)total);
  const uintptr_t sample_bytes = law == kLawNone ? sizeof(int16_t) : 1;
  const auto clash = ranges_overlap(n, [&](int i) { return (uintptr_t)at(i).pcm + sample_bytes * (uintptr_t)at(i).out_first; },
                                    [&](int i) { return sample_bytes * (uintptr_t)at(i).out_count; });
  if (clash.first >= 0)
    return m->fail("%s: %ss %d and %d write overlapping ranges of one pcm", who, noun, clash.first, clash.second);
  // rows with something to write (an empty range still carries out_samples), by kind: [0] unlimited, [1] limited
  std::vector<int> live[2];
  int64_t lds_floats = 0;
  for (int i = 0; i < n; ++i) {
    if (!(at(i).out_count > 0 || at(i).out_samples)) continue;
    const bool limited = limits && limits[i].ceiling != 0.f;
    if (limited)
      lds_floats = std::max(lds_floats, limiter_lds_floats(rp.g, rp.fir, LimiterParams{limits[i].ceiling, limits[i].lookahead, limits[i].hold}));
    live[limited].push_back(i);
  }
  if (live[0].empty() && live[1].empty()) return 0;
  // the scratch: the head, then per kind its rows, its side rows, (with a fading row) its fades and (with a shaped
  // row) its envelopes
  size_t end = 0;
  auto take = [&](size_t bytes) { const size_t a = end; end = align_up(end + bytes, 256); return a; };
  const size_t head_at = take(side.head_bytes);
  struct Kind { size_t rows, side, fades, envs; bool fade, env; } kinds[2];
  for (int k = 0; k < 2; ++k) {
    const std::vector<int>& kind = live[k];
    Kind& t = kinds[k];
    t = Kind{take(kind.size() * sizeof(PcmPoolRow)), take(kind.size() * side.row_bytes), 0, 0, false, false};
    for (int i : kind) {
      t.fade = t.fade || (fades && fades[i].count >= 0);
      t.env = t.env || (envs && envs[i].gain);
    }
    if (t.fade) t.fades = take(kind.size() * sizeof(PcmFade));
    if (t.env) t.envs = take(kind.size() * sizeof(PcmEnv));
  }
  if (ensure(m, m->scrB, end)) return 1;
  hipStream_t s = (hipStream_t)stream;
  const char* head = m->scrB.p + head_at;
  side.head(m->scrB.p + head_at, s);
  // per kind: its row table, its side rows, its fade and envelope tables in the order of the row table (null for a
  // kind without one), and one launch per 65535 rows
  for (int k = 0; k < 2; ++k) {
    const std::vector<int>& kind = live[k];
    if (kind.empty()) continue;
    const Kind& t = kinds[k];
    PcmPoolRow* rows = reinterpret_cast<PcmPoolRow*>(m->scrB.p + t.rows);
    upload_rows<kPcmPoolChunk>(kind.size(), rows, s, [&](size_t j) {
      const int i = kind[j];
      const mbv_pcm_chunk& c = at(i);
      return PcmPoolRow{c.wave, c.in_total, c.valid_samples, c.in_avail, c.out_first, c.out_first + c.out_count, c.peak,
                        reinterpret_cast<short*>(c.pcm), c.pcm_capacity, reinterpret_cast<unsigned*>(c.running_peak),
                        c.out_samples, packed ? off[i] : (int64_t)-1,
                        k ? LimiterParams{limits[i].ceiling, limits[i].lookahead, limits[i].hold} : LimiterParams{}, 0};
    });
    side.rows(kind, m->scrB.p + t.side, s);
    PcmFade* ft = t.fade ? reinterpret_cast<PcmFade*>(m->scrB.p + t.fades) : nullptr;
    if (ft) upload_rows<kPcmPoolChunk>(kind.size(), ft, s, [&](size_t j) { return fade_of(&fades[kind[j]]); });
    PcmEnv* et = t.env ? reinterpret_cast<PcmEnv*>(m->scrB.p + t.envs) : nullptr;
    if (et) upload_rows<kPcmPoolChunk>(kind.size(), et, s, [&](size_t j) { return env_of(&envs[kind[j]]); });
    grid_y_slices(kind, [&](int i) { return at(i).out_count; }, [&](size_t f, int nn, int64_t max_count) {
      ++m->wire_runs;
      PcmPoolLaunch a{rows + f, k == 1, nullptr, nullptr, et ? et + f : nullptr, ft ? ft + f : nullptr, nn, max_count,
                      lds_floats, packed, law};
      side.turn_fields(&a, m->scrB.p + t.side + f * side.row_bytes, head);
      launch_resample_pcm16_pool(a, rp.bank, rp.g, s);
      return 0;
    });
  }
  HIPCHK(m, hipGetLastError());
  return 0;
}

// the chunk entries have nothing beside their rows
struct ChunkSide {
  size_t head_bytes = 0, row_bytes = 0;
  void head(char*, hipStream_t) const {}
  void rows(const std::vector<int>&, char*, hipStream_t) const {}
  void turn_fields(PcmPoolLaunch*, const char*, const char*) const {}
};

// mbv_resample_pcm16_chunks, its limited form and mbv_resample_g711_chunks: one body, limits null = no row limited,
// law kLawNone = int16 (else every pcm and packed hold bytes; the entry has checked law), fades null (or every
// count < 0) = no row fades
int pcm16_chunks(mbv_model* m, const char* who, const mbv_pcm_chunk* chunks_host, const mbv_pcm_limit* limits, int n,
                 int orig_sr, int target_sr, int filter, void* packed, int64_t packed_capacity, int law, void* stream,
                 const mbv_pcm_fade* fades = nullptr, const mbv_pcm_envelope* envs = nullptr) {
  if (!m) return 1;
  if (n < 0 || (n > 0 && !chunks_host)) return m->fail("%s: bad arguments", who);
  if (envs)
    for (int i = 0; i < n; ++i)
      if (const char* why = envelope_refusal(envs[i], chunks_host[i].in_total)) return m->fail("%s: chunk %d: %s", who, i, why);
  if (fades)
    for (int i = 0; i < n; ++i)
      if (const char* why = fade_refusal(fades[i])) return m->fail("%s: chunk %d: %s", who, i, why);
  for (int i = 0; i < n; ++i)
    if (!chunks_host[i].wave || !chunks_host[i].pcm) return m->fail("%s: chunk %d: wave / pcm missing", who, i);
  DEVICE_GUARD(m);
  RatePair rp;
  if (rate_pair(m, who, orig_sr, target_sr, filter, &rp)) return 1;
  std::string err;
  std::vector<int64_t> off(n > 0 ? n : 1);
  const int64_t total = pcm_chunks_check(who, chunks_host, n, rp, off.data(), &err, limits);
  if (total < 0) return m->fail("%s", err.c_str());
  return pooled_wire(m, who, "chunk", [&](int i) -> const mbv_pcm_chunk& { return chunks_host[i]; }, limits, fades, n, rp,
                     off, total, law, packed, packed_capacity, stream, ChunkSide{}, envs);
}
}  // namespace

extern "C" {

int mbv_resample_pcm16_chunks(mbv_model* m, const mbv_pcm_chunk* chunks_host, int n, int orig_sr, int target_sr,
                              int filter, int16_t* packed, int64_t packed_capacity, void* stream) {
  return pcm16_chunks(m, "mbv_resample_pcm16_chunks", chunks_host, nullptr, n, orig_sr, target_sr, filter, packed,
                      packed_capacity, kLawNone, stream);
}

int mbv_resample_pcm16_chunks_limited(mbv_model* m, const mbv_pcm_chunk* chunks_host, const mbv_pcm_limit* limits_host,
                                      int n, int orig_sr, int target_sr, int filter, int16_t* packed,
                                      int64_t packed_capacity, void* stream) {
  return pcm16_chunks(m, "mbv_resample_pcm16_chunks_limited", chunks_host, limits_host, n, orig_sr, target_sr, filter,
                      packed, packed_capacity, kLawNone, stream);
}

int mbv_resample_g711_chunks(mbv_model* m, const mbv_pcm_chunk* chunks_host, const mbv_pcm_limit* limits_host, int n,
                             int orig_sr, int target_sr, int filter, int law, uint8_t* packed, int64_t packed_capacity,
                             void* stream) {
  if (!m) return 1;
  if (const char* why = law_refusal(law)) return m->fail("mbv_resample_g711_chunks: %s, got %d", why, law);
  return pcm16_chunks(m, "mbv_resample_g711_chunks", chunks_host, limits_host, n, orig_sr, target_sr, filter, packed,
                      packed_capacity, law, stream);
}

int mbv_resample_pcm16_chunks_faded(mbv_model* m, const mbv_pcm_chunk* chunks_host, const mbv_pcm_limit* limits_host,
                                    const mbv_pcm_fade* fades_host, int n, int orig_sr, int target_sr, int filter,
                                    int16_t* packed, int64_t packed_capacity, void* stream) {
  return pcm16_chunks(m, "mbv_resample_pcm16_chunks_faded", chunks_host, limits_host, n, orig_sr, target_sr, filter,
                      packed, packed_capacity, kLawNone, stream, fades_host);
}

int mbv_resample_g711_chunks_faded(mbv_model* m, const mbv_pcm_chunk* chunks_host, const mbv_pcm_limit* limits_host,
                                   const mbv_pcm_fade* fades_host, int n, int orig_sr, int target_sr, int filter,
                                   int law, uint8_t* packed, int64_t packed_capacity, void* stream) {
  if (!m) return 1;
  if (const char* why = law_refusal(law)) return m->fail("mbv_resample_g711_chunks_faded: %s, got %d", why, law);
  return pcm16_chunks(m, "mbv_resample_g711_chunks_faded", chunks_host, limits_host, n, orig_sr, target_sr, filter,
                      packed, packed_capacity, law, stream, fades_host);
}

int mbv_resample_pcm16_chunks_shaped(mbv_model* m, const mbv_pcm_chunk* chunks_host, const mbv_pcm_limit* limits_host,
                                     const mbv_pcm_fade* fades_host, const mbv_pcm_envelope* envelopes_host, int n,
                                     int orig_sr, int target_sr, int filter, int law, void* packed,
                                     int64_t packed_capacity, void* stream) {
  if (!m) return 1;
  const char* who = "mbv_resample_pcm16_chunks_shaped";
  if (law != kLawNone)
    if (const char* why = law_refusal(law)) return m->fail("%s: %s (0: int16), got %d", who, why, law);
  return pcm16_chunks(m, who, chunks_host, limits_host, n, orig_sr, target_sr, filter, packed, packed_capacity, law,
                      stream, fades_host, envelopes_host);
}

}  // extern "C"

namespace {
static_assert(MBV_TURN_MAX_SEGS == kTurnMaxSegs, "segment bound of the C-ABI and the kernels");
constexpr int kTurnSegChunk = 96;   // segments per upload_rows launch: 3 KiB of kernel arguments

// The checks of mbv_turn_plan: every turn's `chunk` as pcm_chunks_check checks a chunk, then its segments (integer
// fields only).  Returns the packed total, or -1 with *err naming the offending turn.
int64_t turns_check(const char* who, const mbv_turn_chunk* turns, int n, const RatePair& rp, int64_t* packed_first,
                    std::string* err, const mbv_pcm_limit* limits) {
  const int64_t total = pcm_rows_check(who, "turn", [&](int i) -> const mbv_pcm_chunk& { return turns[i].chunk; }, n, rp,
                                       packed_first, err, limits);
  if (total < 0) return -1;
  char buf[512];
  int64_t all_segs = 0;
  for (int i = 0; i < n; ++i) {
    const mbv_turn_chunk& t = turns[i];
    if (t.n_segs < 0 || (t.n_segs > 0 && !t.segs)) {
      snprintf(buf, sizeof buf, "%s: turn %d: n_segs must be >= 0 and segs given", who, i);
      *err = buf;
      return -1;
    }
    all_segs += t.n_segs;
    if (all_segs > MBV_TURN_MAX_SEGS) {
      snprintf(buf, sizeof buf, "%s: turn %d: more than %d segments in one call (MBV_TURN_MAX_SEGS)", who, i, MBV_TURN_MAX_SEGS);
      *err = buf;
      return -1;
    }
    int64_t end = 0;
    for (int s = 0; s < t.n_segs; ++s) {
      const mbv_turn_seg& sg = t.segs[s];
      buf[0] = 0;
      if (sg.start < 0 || sg.length <= 0 || (double)sg.start + (double)sg.length >= 0x1p62)
        snprintf(buf, sizeof buf, "%s: turn %d: segment %d: start must be >= 0 and length > 0", who, i, s);
      else if (sg.ramp < 0 || sg.ramp > sg.length / 2)
        snprintf(buf, sizeof buf, "%s: turn %d: segment %d: ramp %d must be in [0, length / 2 = %lld]", who, i, s, sg.ramp,
                 (long long)(sg.length / 2));
      else if (sg.start < end)
        snprintf(buf, sizeof buf, "%s: turn %d: segment %d starts at %lld, below the end %lld of the one before: segments "
                 "are ascending and disjoint", who, i, s, (long long)sg.start, (long long)end);
      if (buf[0]) {
        *err = buf;
        return -1;
      }
      end = sg.start + sg.length;
    }
  }
  return total;
}

// what mbv_resample_turns has beside its rows: the call's segment table in front, a slice of it per row
struct TurnSide {
  const std::vector<TurnSeg>& segs;
  const std::vector<int>& seg_first;
  const mbv_turn_chunk* turns;
  size_t head_bytes, row_bytes = sizeof(TurnSlice);
  const std::vector<PcmEnv>* seg_envs = nullptr;           // one per segment, behind the segment table; null: none shaped
  const PcmEnv* envs_in(const char* head) const {
    return seg_envs ? reinterpret_cast<const PcmEnv*>(head + align_up(segs.size() * sizeof(TurnSeg), 256)) : nullptr;
  }
  void head(char* dst, hipStream_t s) const {
    upload_rows<kTurnSegChunk>(segs.size(), reinterpret_cast<TurnSeg*>(dst), s, [&](size_t i) { return segs[i]; });
    if (seg_envs)
      upload_rows<kTurnSegChunk>(seg_envs->size(), const_cast<PcmEnv*>(envs_in(dst)), s,
                                 [&](size_t i) { return (*seg_envs)[i]; });
  }
  void rows(const std::vector<int>& kind, char* dst, hipStream_t s) const {
    upload_rows<kPcmPoolChunk>(kind.size(), reinterpret_cast<TurnSlice*>(dst), s,
                               [&](size_t i) { return TurnSlice{seg_first[kind[i]], turns[kind[i]].n_segs}; });
  }
  // the launch of a slice of turn rows reads their slices, the segment table and the segments' envelopes
  void turn_fields(PcmPoolLaunch* a, const char* slices, const char* head) const {
    a->slices = reinterpret_cast<const TurnSlice*>(slices);
    a->segs = reinterpret_cast<const TurnSeg*>(head);
    a->envs = envs_in(head);
  }
};

// mbv_resample_turns: the chunk entries' body (pooled_wire) for rows whose input is a timeline
int pcm16_turns(mbv_model* m, const char* who, const mbv_turn_chunk* turns, const mbv_pcm_limit* limits,
                const mbv_pcm_fade* fades, int n, int orig_sr, int target_sr, int filter, int law, void* packed,
                int64_t packed_capacity, void* stream, const mbv_pcm_envelope* seg_envs_host = nullptr) {
  if (!m) return 1;
  if (n < 0 || (n > 0 && !turns)) return m->fail("%s: bad arguments", who);
  if (law != kLawNone)
    if (const char* why = law_refusal(law)) return m->fail("%s: %s (0: int16), got %d", who, why, law);
  if (fades)
    for (int i = 0; i < n; ++i)
      if (const char* why = fade_refusal(fades[i])) return m->fail("%s: turn %d: %s", who, i, why);
  for (int i = 0; i < n; ++i) {
    if (turns[i].chunk.wave) return m->fail("%s: turn %d: chunk.wave must be NULL (the input is the segments)", who, i);
    if (!turns[i].chunk.pcm) return m->fail("%s: turn %d: pcm missing", who, i);
  }
  DEVICE_GUARD(m);
  RatePair rp;
  if (rate_pair(m, who, orig_sr, target_sr, filter, &rp)) return 1;
  std::string err;
  std::vector<int64_t> off(n > 0 ? n : 1);
  const int64_t total = turns_check(who, turns, n, rp, off.data(), &err, limits);
  if (total < 0) return m->fail("%s", err.c_str());
  std::vector<int> seg_first(n > 0 ? n : 1);
  std::vector<TurnSeg> segs;
  std::vector<PcmEnv> seg_envs;                            // the call's envelopes, one per segment in call order
  bool any_env = false;
  for (int i = 0; i < n; ++i) {
    seg_first[i] = (int)segs.size();
    for (int k = 0; k < turns[i].n_segs; ++k) {
      const mbv_turn_seg& sg = turns[i].segs[k];
      if (!sg.wave) return m->fail("%s: turn %d: segment %d: wave missing", who, i, k);
      if (seg_envs_host) {
        const mbv_pcm_envelope& e = seg_envs_host[segs.size()];
        if (const char* why = envelope_refusal(e, sg.length)) return m->fail("%s: turn %d: segment %d: %s", who, i, k, why);
        seg_envs.push_back(env_of(&e));
        any_env = any_env || e.gain;
      }
      segs.push_back(TurnSeg{sg.wave, sg.start, sg.length, sg.ramp, fade_inv(sg.ramp)});
    }
  }
  TurnSide side{segs, seg_first, turns, segs.size() * sizeof(TurnSeg)};
  if (any_env) {
    side.seg_envs = &seg_envs;
    side.head_bytes = align_up(side.head_bytes, 256) + seg_envs.size() * sizeof(PcmEnv);
  }
  return pooled_wire(m, who, "turn", [&](int i) -> const mbv_pcm_chunk& { return turns[i].chunk; }, limits, fades, n, rp,
                     off, total, law, packed, packed_capacity, stream, side);
}
}  // namespace

extern "C" {

int64_t mbv_turn_plan(int orig_sr, int target_sr, int filter, const mbv_turn_chunk* turns, const mbv_pcm_limit* limits,
                      int n, int64_t* packed_first) {
  const char* who = "mbv_turn_plan";
  if (n < 0 || (n > 0 && !turns)) { g_create_error = std::string(who) + ": bad arguments"; return -1; }
  RatePair rp;
  if (rate_pair(nullptr, who, orig_sr, target_sr, filter, &rp)) return -1;
  std::string err;
  const int64_t total = turns_check(who, turns, n, rp, packed_first, &err, limits);
  if (total < 0) g_create_error = err;
  return total;
}

int mbv_resample_turns(mbv_model* m, const mbv_turn_chunk* turns_host, const mbv_pcm_limit* limits_host,
                       const mbv_pcm_fade* fades_host, int n, int orig_sr, int target_sr, int filter, int law,
                       void* packed, int64_t packed_capacity, void* stream) {
  return pcm16_turns(m, "mbv_resample_turns", turns_host, limits_host, fades_host, n, orig_sr, target_sr, filter, law,
                     packed, packed_capacity, stream);
}

int mbv_resample_turns_shaped(mbv_model* m, const mbv_turn_chunk* turns_host, const mbv_pcm_limit* limits_host,
                              const mbv_pcm_fade* fades_host, const mbv_pcm_envelope* seg_envelopes_host, int n,
                              int orig_sr, int target_sr, int filter, int law, void* packed, int64_t packed_capacity,
                              void* stream) {
  return pcm16_turns(m, "mbv_resample_turns_shaped", turns_host, limits_host, fades_host, n, orig_sr, target_sr, filter,
                     law, packed, packed_capacity, stream, seg_envelopes_host);
}

int mbv_g711_encode(mbv_model* m, const int16_t* pcm, int64_t n, int law, uint8_t* out, void* stream) {
  if (!m) return 1;
  if (const char* why = law_refusal(law)) return m->fail("mbv_g711_encode: %s, got %d", why, law);
  if (n < 0 || (n > 0 && (!pcm || !out))) return m->fail("mbv_g711_encode: bad arguments");
  if ((n + 255) / 256 > 0x7fffffff) return m->fail("mbv_g711_encode: too many samples for one grid");
  if (n == 0) return 0;
  DEVICE_GUARD(m);
  launch_g711_encode(reinterpret_cast<const short*>(pcm), n, law, out, (hipStream_t)stream);
  HIPCHK(m, hipGetLastError());
  return 0;
}

int mbv_g711_decode(mbv_model* m, const uint8_t* in, int64_t n, int law, int16_t* pcm, void* stream) {
  if (!m) return 1;
  if (const char* why = law_refusal(law)) return m->fail("mbv_g711_decode: %s, got %d", why, law);
  if (n < 0 || (n > 0 && (!in || !pcm))) return m->fail("mbv_g711_decode: bad arguments");
  if ((n + 255) / 256 > 0x7fffffff) return m->fail("mbv_g711_decode: too many samples for one grid");
  if (n == 0) return 0;
  DEVICE_GUARD(m);
  launch_g711_decode(in, n, law, reinterpret_cast<short*>(pcm), (hipStream_t)stream);
  HIPCHK(m, hipGetLastError());
  return 0;
}

int64_t mbv_wire_runs(mbv_model* m) { return m ? m->wire_runs : -1; }

int64_t mbv_resample_ready_open(int orig_sr, int target_sr, int filter, int64_t in_avail) {
  RatePair rp;
  if (rate_pair(nullptr, "mbv_resample_ready_open", orig_sr, target_sr, filter, &rp)) return -1;
  if (in_avail < 0) in_avail = 0;
  return rp.fir ? resample_ready_open(rp.g, in_avail) : in_avail;
}

int mbv_resample_ranges(mbv_model* m, const mbv_resample_range* rows_host, int n, int orig_sr, int target_sr,
                        int filter, void* stream) {
  if (!m) return 1;
  const char* who = "mbv_resample_ranges";
  if (n < 0 || (n > 0 && !rows_host)) return m->fail("%s: bad arguments", who);
  DEVICE_GUARD(m);
  RatePair rp;
  if (rate_pair(m, who, orig_sr, target_sr, filter, &rp)) return 1;
  if (!rp.fir)
    return m->fail("%s: equal rates (%d) take no kernel: the samples are the model's input as they are", who, orig_sr);
  for (int i = 0; i < n; ++i) {
    const mbv_resample_range& k = rows_host[i];
    if (!k.wave || !k.out) return m->fail("%s: row %d: wave / out missing", who, i);
    if (k.wave_dtype != MBV_WAVE_F32 && k.wave_dtype != MBV_WAVE_PCM16 && k.wave_dtype != MBV_WAVE_ULAW &&
        k.wave_dtype != MBV_WAVE_ALAW)
      return m->fail("%s: row %d: unknown wave_dtype %d", who, i, (int)k.wave_dtype);
    if (k.in_avail < 0 || k.in_total < -1 || k.out_first < 0 || k.out_count < 0 || k.out_capacity < 0)
      return m->fail("%s: row %d: in_avail, out_first, out_count and out_capacity must be >= 0, in_total >= -1", who, i);
    if (k.in_total >= 0 && k.in_avail != k.in_total)
      return m->fail("%s: row %d: a closed recording has all its samples (in_avail %lld, in_total %lld)", who, i,
                     (long long)k.in_avail, (long long)k.in_total);
    if (k.out_first > k.out_capacity || k.out_count > k.out_capacity - k.out_first)
      return m->fail("%s: row %d: outputs [%lld, %lld) lie outside the row of out_capacity %lld", who, i,
                     (long long)k.out_first, (long long)(k.out_first + k.out_count), (long long)k.out_capacity);
    if ((double)k.out_capacity * rp.M >= 0x1p62 || (double)k.in_avail * rp.L >= 0x1p62)
      return m->fail("%s: row %d: out_capacity * M or in_avail * L overflows the 64-bit time index", who, i);
  }
  std::vector<int> live;
  for (int i = 0; i < n; ++i) {
    const mbv_resample_range& k = rows_host[i];
    int64_t ready;
    if (k.in_total >= 0) {
      ready = (int64_t)std::ceil((double)k.in_total * rp.g.ratio);         // fix_length of the whole row, as mbv_resample
      if (ready > k.out_capacity) ready = k.out_capacity;
    } else {
      ready = resample_ready_open(rp.g, k.in_avail);
    }
    if (k.out_first + k.out_count > ready)
      return m->fail("%s: row %d: outputs up to %lld asked for, but %lld input samples (%s) make only %lld final", who, i,
                     (long long)(k.out_first + k.out_count), (long long)k.in_avail, k.in_total >= 0 ? "closed" : "open",
                     (long long)ready);
    if (k.out_count > 0) live.push_back(i);
  }
  if (live.empty()) return 0;
  const auto clash = ranges_overlap(n, [&](int i) { return (uintptr_t)(rows_host[i].out + rows_host[i].out_first); },
                                    [&](int i) { return sizeof(float) * (uintptr_t)rows_host[i].out_count; });
  if (clash.first >= 0)
    return m->fail("%s: rows %d and %d write overlapping ranges of one out", who, clash.first, clash.second);
  if (ensure(m, m->scrB, live.size() * sizeof(ResampleRangeRow))) return 1;
  hipStream_t s = (hipStream_t)stream;
  ResampleRangeRow* rows = reinterpret_cast<ResampleRangeRow*>(m->scrB.p);
  upload_rows<kPcmPoolChunk>(live.size(), rows, s, [&](size_t i) {
    const mbv_resample_range& k = rows_host[live[i]];
    return ResampleRangeRow{k.wave, k.wave_dtype, k.in_total >= 0 ? 1 : 0, k.in_avail, k.out_first,
                            k.out_first + k.out_count, k.out};
  });
  if (grid_y_slices(live, [&](int i) { return rows_host[i].out_count; }, [&](size_t f, int nn, int64_t max_count) {
        if ((max_count + kResampleTile - 1) / kResampleTile > 0x7fffffff) return m->fail("%s: a range too long for one grid", who);
        ++m->input_runs;
        launch_resample_ranges(rows + f, nn, max_count, rp.bank, rp.g, s);
        return 0;
      })) return 1;
  HIPCHK(m, hipGetLastError());
  return 0;
}

int64_t mbv_input_runs(mbv_model* m) { return m ? m->input_runs : -1; }

namespace {
constexpr int kWarpZeros[2] = {64, 16};   // num_zeros of kaiser_best / kaiser_fast

int warp_fail(mbv_model* m, const std::string& why) { (m ? m->err : g_create_error) = why; return 1; }

// the device window of a filter: [nwin] fp32 values, then their [nwin] forward differences (fp64, rounded once)
int warp_window(mbv_model* m, const char* who, int filter, const float** out) {
  if (!m->warp_win[filter]) {
    std::vector<double> win;
    resample_window(filter, &win, nullptr, nullptr);
    const size_t nwin = win.size();
    std::vector<float> tab(2 * nwin, 0.f);
    for (size_t i = 0; i < nwin; ++i) tab[i] = (float)win[i];
    for (size_t i = 0; i + 1 < nwin; ++i) tab[nwin + i] = (float)(win[i + 1] - win[i]);
    float* d = nullptr;
    HIPCHK(m, hipMalloc((void**)&d, tab.size() * sizeof(float)));
    if (hipMemcpy(d, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
      (void)hipFree(d);
      return m->fail("%s: uploading the filter window failed", who);
    }
    m->warp_win[filter] = d;
  }
  *out = m->warp_win[filter];
  return 0;
}
}  // namespace

int mbv_warp_plan(int hop, int64_t frames, const float* rate_host, double* U_out_host, int64_t* n_out) {
  const char* who = "mbv_warp_plan";
  if (hop < 1 || frames < 1 || !rate_host || !U_out_host || !n_out)
    return warp_fail(nullptr, std::string(who) + ": hop and frames must be >= 1 and no pointer NULL");
  const int64_t bad = warp_plan(hop, frames, rate_host, U_out_host, n_out);
  if (bad >= 0)
    return warp_fail(nullptr, std::string(who) + ": frame " + std::to_string(bad) + ": rate " +
                                  std::to_string(rate_host[bad]) + " is not a finite value in [0.5, 2]");
  return 0;
}

int64_t mbv_warp_ready(int hop, int64_t frames, const float* rate_host, const double* U_host, int res_type,
                       int64_t in_avail) {
  const char* who = "mbv_warp_ready";
  if (hop < 1 || frames < 1 || !rate_host || !U_host) {
    warp_fail(nullptr, std::string(who) + ": hop and frames must be >= 1 and no pointer NULL");
    return -1;
  }
  if (res_type != MBV_RESAMPLE_KAISER_BEST && res_type != MBV_RESAMPLE_KAISER_FAST) {
    warp_fail(nullptr, std::string(who) + ": unknown res_type " + std::to_string(res_type) +
                           " (0 = kaiser_best, 1 = kaiser_fast)");
    return -1;
  }
  if (in_avail < 0) in_avail = 0;
  return warp_ready(hop, frames, rate_host, U_host, kWarpZeros[res_type], in_avail);
}

int mbv_warp_ranges(mbv_model* m, const mbv_warp_row* rows_host, int n, void* stream) {
  if (!m) return 1;
  const char* who = "mbv_warp_ranges";
  if (n < 1 || !rows_host) return m->fail("%s: n must be >= 1 and rows_host given", who);
  DEVICE_GUARD(m);
  std::vector<int> live, hw(n);
  for (int i = 0; i < n; ++i) {
    const mbv_warp_row& k = rows_host[i];
    if (!k.wave || !k.U || !k.rate || !k.U_host || !k.rate_host || !k.out)
      return m->fail("%s: row %d: wave, U, rate, U_host, rate_host or out missing", who, i);
    if (k.res_type != MBV_RESAMPLE_KAISER_BEST && k.res_type != MBV_RESAMPLE_KAISER_FAST)
      return m->fail("%s: row %d: unknown res_type %d (0 = kaiser_best, 1 = kaiser_fast)", who, i, (int)k.res_type);
    if (k.frames < 1 || k.hop < 1 || k.samples != (int64_t)k.frames * k.hop)
      return m->fail("%s: row %d: frames and hop must be >= 1 and samples (%lld) = frames * hop", who, i,
                     (long long)k.samples);
    if (k.in_avail < 0 || k.out_first < 0 || k.out_count < 0 || k.out_capacity < 0)
      return m->fail("%s: row %d: in_avail, out_first, out_count and out_capacity must be >= 0", who, i);
    if (k.out_first > k.out_capacity || k.out_count > k.out_capacity - k.out_first)
      return m->fail("%s: row %d: outputs [%lld, %lld) lie outside the row of out_capacity %lld", who, i,
                     (long long)k.out_first, (long long)(k.out_first + k.out_count), (long long)k.out_capacity);
    for (int f = 0; f < k.frames; ++f)
      if (!(k.rate_host[f] >= kPitchMin && k.rate_host[f] <= kPitchMax))
        return m->fail("%s: row %d: frame %d: rate %g is not a finite value in [0.5, 2]", who, i, f,
                       (double)k.rate_host[f]);
    const mbv_pcm_envelope& e = k.envelope;
    if (!e.gain) {
      if (e.frames || e.hop || e.inv_hop != 0.f)
        return m->fail("%s: row %d: an envelope without a gain table has frames, hop and inv_hop 0", who, i);
    } else {
      const float inv = e.hop >= 1 ? 1.0f / (float)e.hop : 0.f;
      if (e.hop < 1 || e.frames < 1 || memcmp(&inv, &e.inv_hop, sizeof inv) != 0)
        return m->fail("%s: row %d: an envelope has hop >= 1, frames >= 1 and inv_hop = 1.0f / (float)hop", who, i);
      if (e.frames * (int64_t)e.hop < k.samples)
        return m->fail("%s: row %d: the envelope's %lld frames of %d samples do not cover the row's %lld samples", who,
                       i, (long long)e.frames, (int)e.hop, (long long)k.samples);
    }
    const int zeros = kWarpZeros[k.res_type];
    const int64_t ready = warp_ready(k.hop, k.frames, k.rate_host, k.U_host, zeros, k.in_avail);
    if (k.out_first + k.out_count > ready)
      return m->fail("%s: row %d: outputs up to %lld asked for, but %lld of %lld model samples make only %lld final",
                     who, i, (long long)(k.out_first + k.out_count), (long long)k.in_avail, (long long)k.samples,
                     (long long)ready);
    hw[i] = warp_half_width(zeros, k.frames, k.rate_host);
    if (k.out_count > 0) live.push_back(i);
  }
  if (live.empty()) return 0;
  const auto clash = ranges_overlap(n, [&](int i) { return (uintptr_t)(rows_host[i].out + rows_host[i].out_first); },
                                    [&](int i) { return sizeof(float) * (uintptr_t)rows_host[i].out_count; });
  if (clash.first >= 0)
    return m->fail("%s: rows %d and %d write overlapping ranges of one out", who, clash.first, clash.second);
  const float* win[2] = {nullptr, nullptr};
  for (int i : live) {
    const int ft = rows_host[i].res_type;
    if (!win[ft] && warp_window(m, who, ft, &win[ft])) return 1;
  }
  if (ensure(m, m->scrB, live.size() * sizeof(WarpRow))) return 1;
  hipStream_t s = (hipStream_t)stream;
  WarpRow* rows = reinterpret_cast<WarpRow*>(m->scrB.p);
  upload_rows<kPcmPoolChunk>(live.size(), rows, s, [&](size_t i) {
    const mbv_warp_row& k = rows_host[live[i]];
    return WarpRow{k.wave, k.samples, k.in_avail, k.U, k.rate, k.frames, k.hop, env_of(&k.envelope), k.out_first,
                   k.out_first + k.out_count, k.out, win[k.res_type], kWarpZeros[k.res_type], hw[live[i]]};
  });
  if (grid_y_slices(live, [&](int i) { return rows_host[i].out_count; }, [&](size_t f, int nn, int64_t max_count) {
        if ((max_count + kWarpTile - 1) / kWarpTile > 0x7fffffff) return m->fail("%s: a range too long for one grid", who);
        ++m->warp_runs;
        launch_warp_ranges(rows + f, nn, max_count, s);
        return 0;
      })) return 1;
  HIPCHK(m, hipGetLastError());
  return 0;
}

int64_t mbv_warp_runs(mbv_model* m) { return m ? m->warp_runs : -1; }

// ------------------------------------------------------------------ chunk seams of a bounded look-ahead
int mbv_seam_rows(mbv_model* m, const mbv_seam_row* rows_host, int n, void* stream) {
  if (!m) return 1;
  const char* who = "mbv_seam_rows";
  if (n < 1 || n > 65535 || !rows_host) return m->fail("%s: bad arguments (1 .. 65535 rows expected)", who);
  DEVICE_GUARD(m);
  std::vector<int> live;
  int max_seam = 0;
  for (int i = 0; i < n; ++i) {
    const mbv_seam_row& k = rows_host[i];
    if (!k.o || !k.stash) return m->fail("%s: row %d: o or stash missing", who, i);
    if (k.seam < 1 || k.seam > kSeamMax) return m->fail("%s: row %d: seam %d outside [1, %d] samples", who, i, k.seam, kSeamMax);
    if (k.head_count < 0 || k.head_count > k.seam || k.over_count < 0 || k.over_count > k.seam)
      return m->fail("%s: row %d: head_count and over_count lie in [0, seam = %d]", who, i, k.seam);
    if (k.head_first < 0 || k.over_first < 0 || k.o_samples < 0 || k.head_first + k.head_count > k.o_samples ||
        k.over_first + k.over_count > k.o_samples)
      return m->fail("%s: row %d: head [%lld, +%d) or overhang [%lld, +%d) outside the %lld samples of o", who, i,
                     (long long)k.head_first, k.head_count, (long long)k.over_first, k.over_count, (long long)k.o_samples);
    if (k.head_count && k.over_count && k.head_first < k.over_first + k.over_count && k.over_first < k.head_first + k.head_count)
      return m->fail("%s: row %d: the head and the overhang overlap", who, i);
    if (k.head_count || k.over_count) live.push_back(i);
    if (k.seam > max_seam) max_seam = k.seam;
  }
  // a row owns its stash and the samples it blends: two rows on one of them would race
  auto clash = ranges_overlap(n, [&](int i) { return (uintptr_t)rows_host[i].stash; },
                              [&](int i) { return sizeof(float) * (uintptr_t)rows_host[i].seam; });
  if (clash.first >= 0) return m->fail("%s: rows %d and %d share a stash", who, clash.first, clash.second);
  clash = ranges_overlap(n, [&](int i) { return (uintptr_t)(rows_host[i].o + rows_host[i].head_first); },
                         [&](int i) { return sizeof(float) * (uintptr_t)rows_host[i].head_count; });
  if (clash.first >= 0) return m->fail("%s: rows %d and %d blend overlapping samples of one o", who, clash.first, clash.second);
  if (live.empty()) return 0;
  if (ensure(m, m->scrB, live.size() * sizeof(SeamRow))) return 1;
  hipStream_t s = (hipStream_t)stream;
  SeamRow* rows = reinterpret_cast<SeamRow*>(m->scrB.p);
  upload_rows<kSeamChunk>(live.size(), rows, s, [&](size_t i) {
    const mbv_seam_row& k = rows_host[live[i]];
    return SeamRow{k.o + k.head_first, k.o + k.over_first, k.stash, k.head_count, k.over_count, k.seam,
                   1.0f / (float)(k.seam + 1)};
  });
  ++m->seam_runs;
  launch_seam_rows(rows, (int)live.size(), max_seam, s);
  HIPCHK(m, hipGetLastError());
  return 0;
}

int64_t mbv_seam_runs(mbv_model* m) { return m ? m->seam_runs : -1; }

namespace {
// what mbv_randn_blocks and mbv_randn_host refuse about one block's range and purpose, or null
const char* randn_range_error(int64_t first, int64_t count, uint32_t purpose) {
  if (first < 0 || count < 0) return "first and count must be >= 0";
  if (first > (int64_t(1) << 30) || count > (int64_t(1) << 30) - first) return "first + count exceeds 2^30 frames";
  if (purpose > MBV_NOISE_POSTERIOR) return "unknown purpose (MBV_NOISE_PRIOR 0, MBV_NOISE_SDP 1, MBV_NOISE_POSTERIOR 2)";
  return nullptr;
}
}  // namespace

int mbv_randn_blocks(mbv_model* m, const mbv_randn_block* blocks_host, int n, void* stream) {
  if (!m) return 1;
  const char* who = "mbv_randn_blocks";
  if (n < 1 || !blocks_host) return m->fail("%s: bad arguments (n >= 1 blocks expected)", who);
  DEVICE_GUARD(m);
  std::vector<RandnRow> live;
  int64_t total = 0;
  for (int i = 0; i < n; ++i) {
    const mbv_randn_block& k = blocks_host[i];
    if (const char* e = randn_range_error(k.first, k.count, k.purpose)) return m->fail("%s: block %d: %s", who, i, e);
    if (k.channels < 1) return m->fail("%s: block %d: channels must be >= 1", who, i);
    if (k.stride < k.count) return m->fail("%s: block %d: stride %lld < count %lld", who, i, (long long)k.stride, (long long)k.count);
    if (!k.dst && k.count > 0) return m->fail("%s: block %d: dst missing", who, i);
    if (k.count == 0) continue;
    const int64_t quads = ((k.first + k.count + 3) >> 2) - (k.first >> 2);
    live.push_back(RandnRow{k.dst, k.stride, total, (uint32_t)k.seed, (uint32_t)(k.seed >> 32), k.purpose, k.row,
                            (int32_t)k.first, (int32_t)k.count, (int32_t)quads, 0});
    total += quads * k.channels;             // < 2^28 * 2^31 a block
    if ((total + 255) / 256 > 0x7fffffff) return m->fail("%s: more work than one grid holds (block %d)", who, i);
  }
  if (live.empty()) return 0;
  if (ensure(m, m->noise_tab, live.size() * sizeof(RandnRow))) return 1;
  hipStream_t s = (hipStream_t)stream;
  RandnRow* rows = reinterpret_cast<RandnRow*>(m->noise_tab.p);
  upload_rows<kRandnChunk>(live.size(), rows, s, [&](size_t i) { return live[i]; });
  ++m->noise_runs;
  launch_randn_blocks(rows, (int)live.size(), total, s);
  HIPCHK(m, hipGetLastError());
  return 0;
}

int mbv_randn_host(uint64_t seed, uint32_t purpose, uint32_t row, uint32_t c, int64_t first, int64_t count, float* dst) {
  if (const char* e = randn_range_error(first, count, purpose)) {
    g_create_error = std::string("mbv_randn_host: ") + e;
    return 1;
  }
  if (!dst && count > 0) {
    g_create_error = "mbv_randn_host: dst missing";
    return 1;
  }
  randn_host(seed, purpose, row, c, first, count, dst);
  return 0;
}

int64_t mbv_noise_runs(mbv_model* m) { return m ? m->noise_runs : -1; }

}  // extern "C"

namespace {
// the rate of a loudness entry, or why it is refused (the upper end bounds the host's H-step matrix product)
const char* loudness_rate_refusal(int rate) {
  if (rate < 1000) return "rate must be at least 1000 Hz";
  if (rate > 768000) return "rate must be at most 768000 Hz";
  return nullptr;
}

const LoudnessParams& loudness_params(mbv_model* m, int rate) {
  auto it = m->loudness_params.find(rate);
  if (it == m->loudness_params.end()) {
    LoudnessParams p{};
    kweighting_host(rate, &p);
    it = m->loudness_params.emplace(rate, p).first;
  }
  return it->second;
}

// mbv_loudness_range and mbv_loudness_chunks: the checks on every row, then ONE launch for the rows with segments
int loudness_chunks(mbv_model* m, const char* who, const mbv_loudness_chunk* chunks, int n, int rate, void* stream) {
  if (const char* why = loudness_rate_refusal(rate)) return m->fail("%s: %s, got %d", who, why, rate);
  const LoudnessParams& p = loudness_params(m, rate);
  std::vector<int> live;
  std::set<const void*> states;
  for (int i = 0; i < n; ++i) {
    const mbv_loudness_chunk& k = chunks[i];
    if (!k.wave) return m->fail("%s: chunk %d: wave missing", who, i);
    if (!k.state || !k.energies || !k.loudness) return m->fail("%s: chunk %d: state / energies / loudness missing", who, i);
    if (k.in_total <= 0 || k.in_avail < 0 || k.in_avail > k.in_total || k.seg_first < 0 || k.seg_count < 0 || k.energy_capacity < 0)
      return m->fail("%s: chunk %d: need in_total > 0, 0 <= in_avail <= in_total, seg_first, seg_count and energy_capacity >= 0", who, i);
    const int64_t have = k.in_avail / p.H, end = k.seg_first + k.seg_count;
    if (end > have)
      return m->fail("%s: chunk %d: segments up to %lld asked for, but %lld samples hold only %lld complete segments of %d",
                     who, i, (long long)end, (long long)k.in_avail, (long long)have, (int)p.H);
    if (end > k.energy_capacity)
      return m->fail("%s: chunk %d: segments up to %lld lie outside the energies of capacity %lld", who, i, (long long)end,
                     (long long)k.energy_capacity);
    if (k.seg_first != 0) {
      const auto it = m->loudness_next.find(k.state);
      const int64_t next = it == m->loudness_next.end() ? 0 : it->second;
      if (next != k.seg_first)
        return m->fail("%s: chunk %d: the range starts at segment %lld, but the row's next segment is %lld", who, i,
                       (long long)k.seg_first, (long long)next);
    }
    if (!states.insert(k.state).second) return m->fail("%s: chunk %d: a state buffer appears twice in one call", who, i);
    if (k.seg_count > 0) live.push_back(i);
  }
  // (a row that starts over is remembered even when it brings no segment: its buffer's earlier use is forgotten)
  for (int i = 0; i < n; ++i)
    if (chunks[i].seg_count == 0) m->loudness_next[chunks[i].state] = chunks[i].seg_first;
  if (live.empty()) return 0;
  DEVICE_GUARD(m);
  if (ensure(m, m->scrB, live.size() * sizeof(LoudnessRow))) return 1;
  hipStream_t s = (hipStream_t)stream;
  LoudnessRow* rows = reinterpret_cast<LoudnessRow*>(m->scrB.p);
  upload_rows<kLoudnessChunk>(live.size(), rows, s, [&](size_t i) {
    const mbv_loudness_chunk& k = chunks[live[i]];
    return LoudnessRow{k.wave, k.valid_samples, k.in_avail, k.seg_first, k.seg_first + k.seg_count, k.state, k.energies,
                       k.loudness};
  });
  ++m->loudness_runs;
  launch_loudness(rows, (int)live.size(), p, s);
  HIPCHK(m, hipGetLastError());
  for (int i : live) m->loudness_next[chunks[i].state] = chunks[i].seg_first + chunks[i].seg_count;
  return 0;
}
}  // namespace

extern "C" {

int mbv_kweighting(int rate, double* coeffs, double* M) {
  if (const char* why = loudness_rate_refusal(rate)) {
    g_create_error = std::string("mbv_kweighting: ") + why;
    return 1;
  }
  if (!coeffs || !M) {
    g_create_error = "mbv_kweighting: coeffs / M missing";
    return 1;
  }
  LoudnessParams p{};
  kweighting_host(rate, &p);
  memcpy(coeffs, p.coef, sizeof p.coef);
  memcpy(M, p.M, sizeof p.M);
  return 0;
}

int64_t mbv_loudness_segments(int rate, int64_t samples, int32_t* hop) {
  if (const char* why = loudness_rate_refusal(rate)) {
    g_create_error = std::string("mbv_loudness_segments: ") + why;
    return -1;
  }
  if (samples < 0) {
    g_create_error = "mbv_loudness_segments: samples must be >= 0";
    return -1;
  }
  const int32_t H = (rate + 5) / 10;
  if (hop) *hop = H;
  return samples / H;
}

int mbv_loudness(mbv_model* m, const float* wave, const int64_t* valid_samples, int B, int64_t in_stride, int rate,
                 float* loudness, double* energies, void* stream) {
  if (!m) return 1;
  const char* who = "mbv_loudness";
  if (const char* why = loudness_rate_refusal(rate)) return m->fail("%s: %s, got %d", who, why, rate);
  if (!wave || !loudness || B <= 0 || in_stride <= 0) return m->fail("%s: bad arguments", who);
  const LoudnessParams& p = loudness_params(m, rate);
  const int64_t segs = in_stride / p.H;
  DEVICE_GUARD(m);
  // scratch: the rows' states, their energies where the caller wants none, then the table
  const size_t energy_at = align_up((size_t)B * 4 * sizeof(double), 256);
  const size_t table_at = energy_at + (energies ? 0 : align_up((size_t)B * (size_t)segs * sizeof(double), 256));
  if (ensure(m, m->scrB, table_at + (size_t)B * sizeof(LoudnessRow))) return 1;
  hipStream_t s = (hipStream_t)stream;
  double* state = reinterpret_cast<double*>(m->scrB.p);
  double* e = energies ? energies : reinterpret_cast<double*>(m->scrB.p + energy_at);
  LoudnessRow* rows = reinterpret_cast<LoudnessRow*>(m->scrB.p + table_at);
  upload_rows<kLoudnessChunk>((size_t)B, rows, s, [&](size_t b) {
    return LoudnessRow{wave + b * in_stride, valid_samples ? valid_samples + b : nullptr, in_stride, 0, segs,
                       state + 4 * b, e + b * segs, loudness + b};
  });
  ++m->loudness_runs;
  launch_loudness(rows, B, p, s);
  HIPCHK(m, hipGetLastError());
  return 0;
}

int mbv_loudness_range(mbv_model* m, const float* wave, const int64_t* valid_samples, int B, int64_t in_stride, int rate,
                       int64_t in_avail, int64_t seg_first, int64_t seg_count, double* state, double* energies,
                       int64_t energy_stride, float* loudness, void* stream) {
  if (!m) return 1;
  const char* who = "mbv_loudness_range";
  if (B <= 0 || in_stride <= 0 || energy_stride < 0) return m->fail("%s: bad arguments", who);
  if (!state || !energies) return m->fail("%s: state / energies missing", who);
  if (!wave || !loudness) return m->fail("%s: wave / loudness missing", who);
  std::vector<mbv_loudness_chunk> rows((size_t)B);
  for (int b = 0; b < B; ++b)
    rows[b] = mbv_loudness_chunk{wave + (int64_t)b * in_stride, in_stride, valid_samples ? valid_samples + b : nullptr,
                                 in_avail, seg_first, seg_count, state + 4 * b, energies + (int64_t)b * energy_stride,
                                 energy_stride, loudness + b};
  return loudness_chunks(m, who, rows.data(), B, rate, stream);
}

int mbv_loudness_chunks(mbv_model* m, const mbv_loudness_chunk* chunks_host, int n, int rate, void* stream) {
  if (!m) return 1;
  if (n < 0 || (n > 0 && !chunks_host)) return m->fail("mbv_loudness_chunks: bad arguments");
  return loudness_chunks(m, "mbv_loudness_chunks", chunks_host, n, rate, stream);
}

int64_t mbv_loudness_runs(mbv_model* m) { return m ? m->loudness_runs : -1; }

namespace {
const char* spectrogram_args_error(int n_fft, int hop, int win) {
  if (n_fft < 256 || n_fft > 4096 || (n_fft & (n_fft - 1))) return "n_fft must be a power of two in [256, 4096]";
  if (hop < 1 || hop > n_fft) return "hop must be in [1, n_fft]";
  if (win < 1 || win > n_fft) return "win must be in [1, n_fft]";
  return nullptr;
}
// the handle's twiddle and window tables of an (n_fft, win) pair; the first call builds them in float64 on the host
// and uploads them once (synchronous copy).  0 on success, else m->fail(...) has been called.
int spectrogram_tables_of(mbv_model* m, const char* who, int n_fft, int win, const mbv_model::SpectrogramTables** out) {
  const std::array<int, 2> key{n_fft, win};
  auto it = m->spec_tables.find(key);
  if (it == m->spec_tables.end()) {
    std::vector<float> tw, window;
    spectrogram_tables(n_fft, win, &tw, &window);
    mbv_model::SpectrogramTables t;
    HIPCHK(m, hipMalloc((void**)&t.tw, tw.size() * sizeof(float)));
    if (hipMalloc((void**)&t.win, window.size() * sizeof(float)) != hipSuccess ||
        hipMemcpy(t.tw, tw.data(), tw.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(t.win, window.data(), window.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
      (void)hipFree(t.tw);
      if (t.win) (void)hipFree(t.win);
      return m->fail("%s: uploading the twiddle / window tables failed", who);
    }
    it = m->spec_tables.emplace(key, t).first;
  }
  *out = &it->second;
  return 0;
}
}  // namespace

int64_t mbv_spectrogram_frames(int64_t n_samples, int n_fft, int hop) {
  if (n_samples < 0 || spectrogram_args_error(n_fft, hop, 1)) return -1;
  return spectrogram_frames(n_samples, n_fft, hop);
}

int mbv_spectrogram(mbv_model* m, const void* wave, int wave_dtype, const int64_t* valid_samples, int B,
                    int64_t in_stride, int n_fft, int hop, int win, float* spec, int64_t frames,
                    int64_t* spec_lengths, void* stream) {
  if (!m) return 1;
  if (const char* why = spectrogram_args_error(n_fft, hop, win)) return m->fail("mbv_spectrogram: %s", why);
  if (wave_dtype != MBV_WAVE_F32 && wave_dtype != MBV_WAVE_PCM16)
    return m->fail("mbv_spectrogram: unknown wave_dtype %d", wave_dtype);
  if (!wave || B <= 0 || in_stride <= 0) return m->fail("mbv_spectrogram: bad arguments");
  if (B > 65535) return m->fail("mbv_spectrogram: more than 65535 rows");
  if (in_stride > ((int64_t)1 << 60)) return m->fail("mbv_spectrogram: in_stride too large");
  const int64_t F = spectrogram_frames(in_stride, n_fft, hop);
  if (frames != F)
    return m->fail("mbv_spectrogram: frames is %lld, mbv_spectrogram_frames(in_stride) gives %lld", (long long)frames,
                   (long long)F);
  if (F > 0 && !spec) return m->fail("mbv_spectrogram: spec is NULL");
  if (F / spectrogram_block_frames(n_fft, hop) >= 0x7fffffff) return m->fail("mbv_spectrogram: too many frames per row");
  DEVICE_GUARD(m);
  const mbv_model::SpectrogramTables* tab = nullptr;
  if (spectrogram_tables_of(m, "mbv_spectrogram", n_fft, win, &tab)) return 1;
  launch_spectrogram(wave, wave_dtype, valid_samples, B, in_stride, n_fft, hop, tab->tw, tab->win, spec, F,
                     spec_lengths, (hipStream_t)stream);
  HIPCHK(m, hipGetLastError());
  return 0;
}

// ------------------------------------------------------------------ pooled voice conversion
namespace {
// Which side of the planner's narrow / tiled divide the convs of the posterior path take when B utterances padded to
// T frames run together: enc_q.pre (on the channel-padded spectrogram), enc_q.proj, and a coupling layer's pre / post
// (the shapes run_enc_q and run_coupling build; the fused WN layers fold the latter two and are no conv launches).
void posterior_signature(const mbv_config& c, int splitk, int B, int T, std::vector<char>* sig) {
  static const int kSome = 0;                       // "a length table is given"
  const int H = c.hidden_channels, I = c.inter_channels, cpad = (int)align_up(c.spec_channels, 32);
  auto side = [&](ConvArgs a, bool in_lens) {
    a.out_lens = &kSome;
    if (in_lens) a.in_lens = &kSome;
    const int r = conv1d_plan(a, false).route;
    sig->push_back(r == CONV_NARROW_M || r == CONV_NARROW_LAUNCH);
  };
  sig->clear();
  side(conv_shape(cpad, H, 1, 1, T, T, B, splitk), false);                       // enc_q.pre
  side(conv_shape(H, 2 * I, 1, 1, T, T, B, splitk), true);                       // enc_q.proj
  ConvArgs pre = conv_shape(I / 2, H, 1, 1, T, T, B, splitk);                    // flow.pre, on a half of z
  pre.x_bstride = (int64_t)I * T;
  side(pre, false);
  ConvArgs post = conv_shape(H, I / 2, 1, 1, T, T, B, splitk);                   // flow.post, onto the other half
  post.y_bstride = (int64_t)I * T; post.epi = EPI_COUPLE; post.couple_sign = 1.f;
  side(post, true);
}

// a run of B rows padded to T frames stays inside the grid and inside what the fused WN layers take
bool convert_run_fits(const mbv_config& c, int B, int T) {
  return B <= 65535 && wn_fused_fits(B, c.hidden_channels, T) && wn_fused_fits(B, c.inter_channels, T);
}

// Runs of one pooled conversion for requests of t_frames[i] frames (plan_runs): requests share a run iff their
// posterior_signature at B = 1 agree, and a run is cut where the padded run would plan differently, exceed 65535 rows
// or exceed the fused WN layers' 32-bit offsets.  Split-K: one class.  -1 on a bad argument (a request that alone is
// beyond the fused WN layers included).
int convert_plan(const mbv_config& c, int splitk, int n, const int32_t* t_frames, int32_t* run_of_request) {
  if (n <= 0 || !t_frames) return -1;
  for (int i = 0; i < n; ++i)
    if (t_frames[i] < 1 || !convert_run_fits(c, 1, t_frames[i])) return -1;
  auto fits = [&](int B, int T) { return convert_run_fits(c, B, T); };
  if (splitk) return plan_runs(n, t_frames, no_signature, fits, run_of_request);
  return plan_runs(n, t_frames, [&](int B, int T, std::vector<char>* sig) { posterior_signature(c, 0, B, T, sig); }, fits, run_of_request);
}

// What mbv_convert_rows ("pooled") and mbv_convert_ranges ("live") both refuse: of the call (bad_args: the entry's own
// argument test, in its place among the others) and of a row; of the planned run: run_posterior_rows.
int convert_call_refusal(mbv_model* m, const char* who, const char* kind, bool bad_args, int hop, int win) {
  if (!m->finalized) return m->fail("weights not finalized");
  const mbv_config& c = m->cfg;
  if (c.n_speakers <= 0 || !m->emb_g.present)
    return m->fail("n_speakers have to be larger than 0.");              // models.py:791 assert
  if (bad_args) return m->fail("%s: bad arguments", who);
  if (m->conv_bf16) return m->fail("%s: %s conversion is not built for the \"conv_bf16\" mode", who, kind);
  const int n_fft = 2 * (c.spec_channels - 1);
  if (const char* why = spectrogram_args_error(n_fft, hop, win))
    return m->fail("%s: %s (n_fft = 2 (spec_channels - 1) = %d)", who, why, n_fft);
  return 0;
}
int convert_row_refusal(mbv_model* m, const char* who, int i, int wave_dtype, int sid_src, int sid_tgt, float noise_scale) {
  const int ns = m->cfg.n_speakers;
  if (wave_dtype != MBV_WAVE_F32 && wave_dtype != MBV_WAVE_PCM16)
    return m->fail("%s: row %d: unknown wave_dtype %d", who, i, wave_dtype);
  if (!m->speaker_ok(sid_src) || !m->speaker_ok(sid_tgt))
    return m->fail("%s: row %d: speaker id outside [0, %d) and no defined voice", who, i, ns);
  if (!(noise_scale >= 0.f)) return m->fail("%s: row %d: noise_scale must be >= 0", who, i);
  return 0;
}

// One pooled posterior run over validated rows (crows[i].frames <= T): the two tables go up in kAdmitChunk pieces, then
// the speaker vectors, the spectrograms into enc_q's padded input, enc_q, the forward flow with the source speaker
// (models.py:795) and the reverse flow with the target (:796) in place, and every row's kept frames to its own z.
// g_out: where the target speaker vectors [B, gin] go (null: scratch).  route_T: see run_enc_q.
int run_posterior_rows(mbv_model* m, const char* who, const std::vector<ConvertRow>& crows_h,
                       const std::vector<AdmitSynRow>& srows_h, int T, int max_keep, int route_T, float* g_out, int hop,
                       int win, hipStream_t s) {
  const mbv_config& c = m->cfg;
  const int B = (int)crows_h.size(), I = c.inter_channels, gin = c.gin_channels, n_fft = 2 * (c.spec_channels - 1);
  // the whole run must take the route every row takes alone: the fused WN layers, which work on 16-frame half-units
  // below each row's own length (the two-launch layers route on T)
  bool fused = wn_takes_fused(m, m->encq.in, m->encq.in16, B, T) && wn_fused_fits(B, I, T);
  for (int f = 0; f < kNFlows; ++f) fused = fused && wn_takes_fused(m, m->flow[f].in, m->flow[f].in16, B, T);
  if (!fused)
    return m->fail("%s: a run of %d x %d frames is outside the fused WN layers (option \"wn_fused\" off, a hidden size they "
                   "do not cover, or tensors beyond their 32-bit offsets)", who, B, T);
  DEVICE_GUARD(m);
  const mbv_model::SpectrogramTables* tab = nullptr;
  if (spectrogram_tables_of(m, who, n_fft, win, &tab)) return 1;
  const size_t BT = (size_t)B * T;
  PosteriorBufs pb{};
  float *z, *g_src, *g_tgt;
  int* lens;
  ConvertRow* crows;
  AdmitSynRow* srows;
  int64_t *sid_src, *sid_tgt;
  if (lay_out(m, who, m->scrB, [&](Bump& b) {
        pb = carve_posterior(b, m, B, T);
        z = b.take<float>(BT * I);
        g_src = b.take<float>((size_t)B * gin);
        g_tgt = g_out ? g_out : b.take<float>((size_t)B * gin);
        lens = b.take<int>(B);
        crows = b.take<ConvertRow>(B);
        srows = b.take<AdmitSynRow>(B);
        sid_src = b.take<int64_t>(B);
        sid_tgt = b.take<int64_t>(B);
      })) return 1;
  m->stages.clear();
  m->stage("convert_ypad", pb.ypad, (int64_t)(BT * m->encq.cin_pad), m->scrB);
  upload_rows<kAdmitChunk>(B, crows, s, [&](size_t i) { return crows_h[i]; }, ConvertRowCols{lens, sid_src, sid_tgt});
  upload_rows<kAdmitChunk>(B, srows, s, [&](size_t i) { return srows_h[i]; });
  ++m->converter_runs;
  launch_gather_rows(m->W(m->emb_g.off), sid_src, g_src, B, gin, c.n_speakers, nullptr, s, m->voice_table());
  launch_gather_rows(m->W(m->emb_g.off), sid_tgt, g_tgt, B, gin, c.n_speakers, nullptr, s, m->voice_table());
  launch_spectrogram_rows(crows, B, n_fft, hop, tab->tw, tab->win, pb.ypad, m->encq.cin_pad, T, s);
  if (run_enc_q(m, nullptr, lens, g_src, nullptr, 1.f, pb, z, B, T, s, srows, route_T)) return 1;
  if (int rc = run_flows(m, false, z, g_src, pb, lens, B, T, s, route_T)) return rc;
  if (int rc = run_flows(m, true, z, g_tgt, pb, lens, B, T, s, route_T)) return rc;
  launch_scatter_z_rows(z, lens, srows, B, I, T, max_keep, s);
  HIPCHK(m, hipGetLastError());
  return 0;
}
}  // namespace

int mbv_convert_plan(const mbv_config* cfg, int splitk, int n, const int32_t* t_frames, int32_t* run_of_request) {
  if (!cfg) return -1;
  return convert_plan(*cfg, splitk != 0, n, t_frames, run_of_request);
}

int64_t mbv_converter_runs(mbv_model* m) { return m ? m->converter_runs : -1; }

int mbv_convert_rows(mbv_model* m, const mbv_convert_row* rows_host, int n, int t_frames, int hop, int win, float* g_out,
                     void* stream) {
  if (!m) return 1;
  const char* who = "mbv_convert_rows";
  if (convert_call_refusal(m, who, "pooled", !rows_host || !g_out || n <= 0 || t_frames <= 0, hop, win)) return 1;
  const mbv_config& c = m->cfg;
  const int n_fft = 2 * (c.spec_channels - 1), B = n, T = t_frames;
  std::vector<ConvertRow> crows(B);
  std::vector<AdmitSynRow> srows(B);
  std::vector<int32_t> fr(B);
  int longest = 0;
  for (int i = 0; i < B; ++i) {
    const mbv_convert_row& k = rows_host[i];
    if (!k.wave || !k.z || k.samples < 1) return m->fail("%s: row %d: wave or z missing, or no samples", who, i);
    if (convert_row_refusal(m, who, i, k.wave_dtype, k.sid_src, k.sid_tgt, k.noise_scale)) return 1;
    const int64_t f = spectrogram_frames(k.samples, n_fft, hop);
    if (f < 1 || f > T) return m->fail("%s: row %d: %lld frames outside [1, %d]", who, i, (long long)f, T);
    fr[i] = (int32_t)f;
    if (fr[i] > longest) longest = fr[i];
    if (k.noise_scale != 0.f && !k.noise) return m->fail("%s: row %d: noise missing", who, i);
    crows[i] = ConvertRow{k.wave, k.samples, k.wave_dtype, fr[i], k.sid_src, k.sid_tgt};
    srows[i] = AdmitSynRow{k.noise, fr[i], k.noise_scale, fr[i], k.z};
  }
  // the run is planned at its longest row (mbv_convert_plan): a wider launch could take a route no row takes alone
  if (T != longest)
    return m->fail("%s: t_frames is %d, the longest row has %d frames: a run is padded to its longest row", who, T, longest);
  // the rows must be ONE run of the plan: a second class in the launch would move some row to another route
  if (convert_plan(c, m->splitk, B, fr.data(), nullptr) != 1)
    return m->fail("%s: the rows belong to more than one run of mbv_convert_plan", who);
  return run_posterior_rows(m, who, crows, srows, T, longest, 0, g_out, hop, win, (hipStream_t)stream);
}

// ------------------------------------------------------------------ live voice conversion (audio that is still arriving)
namespace {
// Any length past the narrow kernel's 256: what the conv planner sees for a window of a recording whose final length is
// not known yet (conv1d_plan's route_T).  The tiled kernels compute an element with one chain of operations whatever the
// launch size, so every window of a recording, and its one-shot conversion once it is longer than 256 frames, agree.
constexpr int kLiveRouteFrames = 257;

// spectrogram frames [0, n) whose samples all exist: frame f reads [f hop - pad, f hop - pad + n_fft)
int64_t spectrogram_ready(int64_t arrived, int closed, int n_fft, int hop) {
  if (closed) return spectrogram_frames(arrived, n_fft, hop);
  const int64_t pad = (n_fft - hop) / 2;
  return arrived + pad < n_fft ? 0 : (arrived + pad - n_fft) / hop + 1;
}

// z_hat frame t depends on spectrogram frames [t - L, t + R] only: enc_q's WN and the couplings' WNs of both flow
// passes are stacks of k = kFlowK, dilation-1 convs (every other conv of the path is 1x1), each reaching (k - 1) / 2
// frames to either side.  The plain sum of the layers (the Flip between couplings lets half of the channels lag by a
// layer stack, so the reach seen is a little smaller: DESIGN 7.11).
void converter_context(int* L, int* R) {
  const int reach = (mbv_model::kEncQLayers + 2 * kNFlows * kFlowLayers) * ((kFlowK - 1) / 2);
  *L = reach; *R = reach;
}

// The spectrogram window from which z_hat frames [first, first + count) are computed when `final` frames are final: the
// context to either side, clipped to the recording, its start aligned down to a whole 32-frame unit of the fused WN
// layers (so that a frame sits in its unit where the whole-recording run has it).
// ahead < 0: the full reach R.  ahead in [0, R] (a bounded look-ahead): the window ends `ahead` frames
// behind the range, and the row of the padded run ends there as a recording whose spectrogram ends there would.
void convert_window(int first, int count, int64_t final_frames, int* wa, int* wb, int ahead = -1) {
  int L, R;
  converter_context(&L, &R);
  const int a = first - L > 0 ? first - L : 0;
  *wa = a & ~31;
  const int64_t b = (int64_t)first + count + (ahead < 0 ? R : ahead);
  *wb = (int)(b < final_frames ? b : final_frames);
}
}  // namespace

int mbv_converter_context(const mbv_config* cfg, int32_t out[2]) {
  if (!cfg || !out) return 1;
  int L, R;
  converter_context(&L, &R);
  out[0] = L; out[1] = R;
  return 0;
}

int64_t mbv_spectrogram_ready(int64_t arrived, int closed, int n_fft, int hop) {
  if (arrived < 0 || spectrogram_args_error(n_fft, hop, 1)) return -1;
  return spectrogram_ready(arrived, closed != 0, n_fft, hop);
}

int mbv_convert_window(const mbv_config* cfg, int first, int count, int64_t final_frames, int32_t out[2]) {
  if (!cfg || !out || first < 0 || count < 1 || final_frames < (int64_t)first + count || final_frames > 0x7fffffff) return 1;
  int wa, wb;
  convert_window(first, count, final_frames, &wa, &wb);
  out[0] = wa; out[1] = wb;
  return 0;
}

int mbv_convert_window_ahead(const mbv_config* cfg, int first, int count, int ahead, int64_t final_frames, int32_t out[2]) {
  int L, R;
  converter_context(&L, &R);
  if (ahead < 0 || ahead > R) return 1;
  if (mbv_convert_window(cfg, first, count, final_frames, out)) return 1;
  int wa, wb;
  convert_window(first, count, final_frames, &wa, &wb, ahead);
  out[0] = wa; out[1] = wb;
  return 0;
}

int mbv_convert_ranges_plan(const mbv_config* cfg, int n, const int32_t* window_frames, int32_t* run_of_range) {
  if (!cfg || n <= 0 || !window_frames) return -1;
  for (int i = 0; i < n; ++i)
    if (window_frames[i] < 1 || !convert_run_fits(*cfg, 1, window_frames[i])) return -1;
  // With a single class, at most one run is ever open: the generic loop gives exactly the sequential cut.
  return plan_runs(n, window_frames, no_signature, [&](int B, int T) { return convert_run_fits(*cfg, B, T); }, run_of_range);
}

int mbv_convert_ranges(mbv_model* m, const mbv_convert_range* rows_host, int n, int hop, int win, void* stream) {
  return mbv_convert_ranges_ahead(m, rows_host, nullptr, n, hop, win, stream);
}

int mbv_convert_ranges_ahead(mbv_model* m, const mbv_convert_range* rows_host, const int32_t* ahead_host, int n, int hop,
                             int win, void* stream) {
  if (!m) return 1;
  const char* who = ahead_host ? "mbv_convert_ranges_ahead" : "mbv_convert_ranges";
  if (convert_call_refusal(m, who, "live", !rows_host || n <= 0, hop, win)) return 1;
  const mbv_config& c = m->cfg;
  const int n_fft = 2 * (c.spec_channels - 1), B = n;
  int Lv, Rv;
  converter_context(&Lv, &Rv);
  std::vector<ConvertRow> crows(B);
  std::vector<AdmitSynRow> srows(B);
  std::vector<int32_t> wlen(B);
  int T = 0, max_keep = 0;
  for (int i = 0; i < B; ++i) {
    const mbv_convert_range& k = rows_host[i];
    if (!k.wave || !k.z || k.arrived < 1) return m->fail("%s: row %d: wave or z missing, or no samples", who, i);
    if (convert_row_refusal(m, who, i, k.wave_dtype, k.sid_src, k.sid_tgt, k.noise_scale)) return 1;
    const int64_t fin = spectrogram_ready(k.arrived, k.closed != 0, n_fft, hop);
    if (fin > 0x7fffffff) return m->fail("%s: row %d: too many frames", who, i);
    if (k.first < 0 || k.count < 1 || (int64_t)k.first + k.count > fin)
      return m->fail("%s: row %d: frames [%d, %d + %d) outside the %lld final spectrogram frames", who, i, k.first, k.first,
                     k.count, (long long)fin);
    const int ah = ahead_host ? ahead_host[i] : Rv;
    if (ah < 0 || ah > Rv) return m->fail("%s: row %d: ahead %d outside [0, %d]", who, i, ah, Rv);
    if (!k.closed && (int64_t)k.first + k.count + ah > fin)
      return m->fail("%s: row %d: frames [%d, %d + %d) are not final yet: they need spectrogram frames up to %lld, and "
                     "%lld are final (the recording is open)", who, i, k.first, k.first, k.count,
                     (long long)k.first + k.count + ah, (long long)fin);
    int wa, wb;
    convert_window(k.first, k.count, fin, &wa, &wb, ah);
    if (k.noise_scale != 0.f && (!k.noise || k.noise_stride < wb))
      return m->fail("%s: row %d: noise missing, or noise_stride %lld < the window's end %d", who, i, (long long)k.noise_stride, wb);
    if (k.z_stride < (int64_t)k.first + k.count)
      return m->fail("%s: row %d: z_stride %lld < first + count = %d", who, i, (long long)k.z_stride, k.first + k.count);
    wlen[i] = wb - wa;
    if (wlen[i] > T) T = wlen[i];
    if (k.count > max_keep) max_keep = k.count;
    crows[i] = ConvertRow{k.wave, k.arrived, k.wave_dtype, wlen[i], k.sid_src, k.sid_tgt, wa, 0};
    // the noise of the window's frames at the block's stride; the kept frames [first, first + count) of the window
    // go to frame `first` of the stream's own z
    srows[i] = AdmitSynRow{k.noise ? k.noise + wa : nullptr, k.noise_stride, k.noise_scale, k.count,
                           k.z + k.first, wlen[i], k.first - wa, k.z_stride};
  }
  // several ranges of one recording may share a run (the grid blocks of a bounded look-ahead), never a frame of its z
  const auto clash = ranges_overlap(B, [&](int i) { return (uintptr_t)(rows_host[i].z + rows_host[i].first); },
                                    [&](int i) { return sizeof(float) * (uintptr_t)rows_host[i].count; });
  if (clash.first >= 0)
    return m->fail("%s: rows %d and %d write overlapping ranges of one z", who, clash.first, clash.second);
  if (mbv_convert_ranges_plan(&c, B, wlen.data(), nullptr) != 1)
    return m->fail("%s: the %d rows (widest window %d frames) belong to more than one run of mbv_convert_ranges_plan", who, B, T);
  // the target speaker vectors stay in scratch; the planner sees a length past the narrow kernel's for every window
  return run_posterior_rows(m, who, crows, srows, T, max_keep, T > kLiveRouteFrames ? T : kLiveRouteFrames, nullptr, hop,
                            win, (hipStream_t)stream);
}

// ------------------------------------------------------------------ live text (tokens that are still arriving)
namespace {
// z frame t depends on z_p frames [t - R, t + R] only: the reverse pass is kNFlows couplings, each a WN of kFlowLayers
// k = kFlowK, dilation-1 convs between 1x1 convs (the plain sum, as converter_context takes it).
int text_context() { return kNFlows * kFlowLayers * ((kFlowK - 1) / 2); }

// The z_p window from which z frames [first, first + count) are computed when P frames are expanded (convert_window's
// rule: the start on a whole 32-frame unit of the fused WN layers, where the whole-utterance run has the frame).
void flow_window(int first, int count, int64_t P, int* wa, int* wb) {
  const int R = text_context();
  const int a = first - R > 0 ? first - R : 0;
  *wa = a & ~31;
  const int64_t b = (int64_t)first + count + R;
  *wb = (int)(b < P ? b : P);
}
}  // namespace

int mbv_text_context(const mbv_config* cfg, int32_t out[2]) {
  if (!cfg || !out) return 1;
  out[0] = out[1] = text_context();
  return 0;
}

int mbv_flow_window(const mbv_config* cfg, int first, int count, int64_t P, int32_t out[2]) {
  if (!cfg || !out || first < 0 || count < 1 || P < (int64_t)first + count || P > 0x7fffffff) return 1;
  int wa, wb;
  flow_window(first, count, P, &wa, &wb);
  out[0] = wa; out[1] = wb;
  return 0;
}

int mbv_flow_ranges_plan(const mbv_config* cfg, int n, const int32_t* window_frames, int32_t* run_of_range) {
  return mbv_convert_ranges_plan(cfg, n, window_frames, run_of_range);      // the same single class, the same cuts
}

int64_t mbv_text_runs(mbv_model* m) { return m ? m->text_runs : -1; }
int64_t mbv_flow_runs(mbv_model* m) { return m ? m->flow_runs : -1; }

int mbv_take_tokens_rows(mbv_model* m, int slot, const mbv_take_row* rows_host, int n, void* stream) {
  if (!m) return 1;
  const char* who = "mbv_take_tokens_rows";
  EncRun* r = slot >= 0 && slot < mbv_model::kSlots ? &m->runs[slot] : nullptr;
  if (!r || !r->live()) return m->fail("%s without a preceding mbv_encode_rows on slot %d", who, slot);
  if (!r->rows) return m->fail("%s: slot %d holds no mbv_encode_rows run", who, slot);
  if (!rows_host || n < 1 || n > 65535) return m->fail("%s: bad arguments (1 .. 65535 rows expected)", who);
  int max_cols = 0;
  for (int i = 0; i < n; ++i) {
    const mbv_take_row& k = rows_host[i];
    if (k.src < 0 || k.src >= r->B) return m->fail("%s: row %d: src %d outside the run's %d rows", who, i, k.src, r->B);
    if (k.a < 0 || k.b <= k.a || k.b > r->t_text[k.src])
      return m->fail("%s: row %d: tokens [%d, %d) outside the %d tokens of run row %d", who, i, k.a, k.b, r->t_text[k.src], k.src);
    if (!k.y_length || !k.stats || !k.dur) return m->fail("%s: row %d: y_length, stats or dur missing", who, i);
    if (k.stride < k.b) return m->fail("%s: row %d: stride %lld < b = %d", who, i, (long long)k.stride, k.b);
    if (k.b - k.a > max_cols) max_cols = k.b - k.a;
  }
  DEVICE_GUARD(m);
  if (ensure(m, m->scrB, (size_t)n * sizeof(TakeRow))) return 1;
  hipStream_t s = (hipStream_t)stream;
  TakeRow* rows = reinterpret_cast<TakeRow*>(m->scrB.p);
  upload_rows<kTextChunk>(n, rows, s, [&](size_t i) {
    const mbv_take_row& k = rows_host[i];
    return TakeRow{k.y_length, k.stats, k.dur, k.dur_copy, k.stride, k.src, k.a, k.b, 0};
  });
  ++m->text_runs;
  launch_take_tokens_rows(r->stats, r->w_ceil, rows, n, 2 * m->cfg.inter_channels, r->T, max_cols, s);
  HIPCHK(m, hipGetLastError());
  return 0;
}

int mbv_expand_ranges(mbv_model* m, const mbv_expand_range* rows_host, int n, void* stream) {
  if (!m) return 1;
  const char* who = "mbv_expand_ranges";
  if (!m->finalized) return m->fail("weights not finalized");
  if (!rows_host || n < 1 || n > 65535) return m->fail("%s: bad arguments (1 .. 65535 rows expected)", who);
  std::vector<int> live, frames(n);
  int most = 0;
  for (int i = 0; i < n; ++i) {
    const mbv_expand_range& k = rows_host[i];
    if (!k.stats || !k.dur || !k.dur_host || !k.z_p) return m->fail("%s: row %d: stats, dur, dur_host or z_p missing", who, i);
    if (k.a < 0 || k.b <= k.a || k.stride < k.b)
      return m->fail("%s: row %d: tokens [%d, %d) empty or beyond the tables' stride %lld", who, i, k.a, k.b, (long long)k.stride);
    if (k.frame < 0 || k.max_frames < 1 || k.z_stride < k.max_frames)
      return m->fail("%s: row %d: frame %d < 0, or max_frames %d outside [1, z_stride = %lld]", who, i, k.frame, k.max_frames,
                     (long long)k.z_stride);
    if (!(k.noise_scale >= 0.f)) return m->fail("%s: row %d: noise_scale must be >= 0", who, i);
    if (k.noise_scale != 0.f && (!k.noise || k.noise_stride < k.max_frames))
      return m->fail("%s: row %d: noise missing, or noise_stride %lld < max_frames %d", who, i, (long long)k.noise_stride, k.max_frames);
    int64_t sum = 0;
    for (int j = 0; j < k.b - k.a; ++j) {
      if (k.dur_host[j] < 0) return m->fail("%s: row %d: token %d has a negative duration (%d)", who, i, k.a + j, k.dur_host[j]);
      sum += k.dur_host[j];
    }
    if ((int64_t)k.frame + sum > k.max_frames)
      return m->fail("%s: row %d: frames [%d, %d + %lld) do not fit max_frames = %d", who, i, k.frame, k.frame, (long long)sum, k.max_frames);
    frames[i] = (int)sum;
    if (sum) live.push_back(i);
    if (frames[i] > most) most = frames[i];
  }
  const auto clash = ranges_overlap(n, [&](int i) { return (uintptr_t)(rows_host[i].z_p + rows_host[i].frame); },
                                    [&](int i) { return sizeof(float) * (uintptr_t)frames[i]; });
  if (clash.first >= 0) return m->fail("%s: rows %d and %d write overlapping frames of one z_p", who, clash.first, clash.second);
  if (live.empty()) return 0;
  DEVICE_GUARD(m);
  if (ensure(m, m->scrB, live.size() * sizeof(ExpandRange))) return 1;
  hipStream_t s = (hipStream_t)stream;
  ExpandRange* rows = reinterpret_cast<ExpandRange*>(m->scrB.p);
  upload_rows<kTextChunk>(live.size(), rows, s, [&](size_t i) {
    const mbv_expand_range& k = rows_host[live[i]];
    return ExpandRange{k.stats, k.dur, k.stride, k.noise, k.noise_stride, k.z_p, k.z_stride, k.noise_scale,
                       k.a, k.b, k.frame, frames[live[i]], 0};
  });
  ++m->text_runs;
  launch_expand_ranges(rows, (int)live.size(), m->cfg.inter_channels, most, s);
  HIPCHK(m, hipGetLastError());
  return 0;
}

int mbv_flow_ranges(mbv_model* m, const mbv_flow_range* rows_host, int n, void* stream) {
  if (!m) return 1;
  const char* who = "mbv_flow_ranges";
  if (!m->finalized) return m->fail("weights not finalized");
  if (!rows_host || n < 1) return m->fail("%s: bad arguments", who);
  if (m->conv_bf16) return m->fail("%s: live text is not built for the \"conv_bf16\" mode", who);
  const mbv_config& c = m->cfg;
  const bool has_g = c.n_speakers > 0 && m->emb_g.present;
  const int B = n, I = c.inter_channels, gin = c.gin_channels, R = text_context();
  std::vector<FlowRow> frows(B);
  std::vector<AdmitSynRow> srows(B);
  std::vector<int32_t> wlen(B);
  int T = 0, max_keep = 0;
  for (int i = 0; i < B; ++i) {
    const mbv_flow_range& k = rows_host[i];
    if (!k.z_p || !k.z) return m->fail("%s: row %d: z_p or z missing", who, i);
    if (k.first < 0 || k.count < 1 || k.P < 1 || (int64_t)k.first + k.count > k.P)
      return m->fail("%s: row %d: frames [%d, %d + %d) outside the %d expanded frames", who, i, k.first, k.first, k.count, k.P);
    if (!k.complete && (int64_t)k.first + k.count + R > k.P)
      return m->fail("%s: row %d: frames [%d, %d + %d) are not computable yet: they need z_p frames up to %lld, and %d are "
                     "expanded (the text is open)", who, i, k.first, k.first, k.count, (long long)k.first + k.count + R, k.P);
    if (k.z_p_stride < k.P) return m->fail("%s: row %d: z_p_stride %lld < P = %d", who, i, (long long)k.z_p_stride, k.P);
    if (k.z_stride < (int64_t)k.first + k.count)
      return m->fail("%s: row %d: z_stride %lld < first + count = %d", who, i, (long long)k.z_stride, k.first + k.count);
    if (has_g && !m->speaker_ok(k.sid))
      return m->fail("%s: row %d: speaker id outside [0, %d) and no defined voice", who, i, c.n_speakers);
    int wa, wb;
    flow_window(k.first, k.count, k.P, &wa, &wb);
    wlen[i] = wb - wa;
    if (wlen[i] > T) T = wlen[i];
    if (k.count > max_keep) max_keep = k.count;
    frows[i] = FlowRow{k.z_p, k.z_p_stride, has_g ? k.sid : 0, wa, wlen[i]};
    srows[i] = AdmitSynRow{nullptr, 0, 0.f, k.count, k.z + k.first, wlen[i], k.first - wa, k.z_stride};
  }
  const auto clash = ranges_overlap(B, [&](int i) { return (uintptr_t)(rows_host[i].z + rows_host[i].first); },
                                    [&](int i) { return sizeof(float) * (uintptr_t)rows_host[i].count; });
  if (clash.first >= 0) return m->fail("%s: rows %d and %d write overlapping ranges of one z", who, clash.first, clash.second);
  if (mbv_flow_ranges_plan(&c, B, wlen.data(), nullptr) != 1)
    return m->fail("%s: the %d rows (widest window %d frames) belong to more than one run of mbv_flow_ranges_plan", who, B, T);
  for (int f = 0; f < kNFlows; ++f)
    if (!wn_takes_fused(m, m->flow[f].in, m->flow[f].in16, B, T) || !wn_fused_fits(B, I, T))
      return m->fail("%s: a run of %d x %d frames is outside the fused WN layers (option \"wn_fused\" off, a hidden size they "
                     "do not cover, or tensors beyond their 32-bit offsets)", who, B, T);
  DEVICE_GUARD(m);
  hipStream_t s = (hipStream_t)stream;
  float *z, *g;
  FlowBufs fb{};
  int* lens;
  int64_t* sid;
  FlowRow* rows;
  AdmitSynRow* scat;
  if (lay_out(m, who, m->scrB, [&](Bump& b) {
        z = b.take<float>((size_t)B * T * I);
        fb = carve_flow(b, c, B, T, kFlowLayers);
        g = b.take<float>((size_t)B * (gin ? gin : 1));
        lens = b.take<int>(B);
        sid = b.take<int64_t>(B);
        rows = b.take<FlowRow>(B);
        scat = b.take<AdmitSynRow>(B);
      })) return 1;
  upload_rows<kAdmitChunk>(B, rows, s, [&](size_t i) { return frows[i]; }, FlowRowCols{lens, sid});
  upload_rows<kAdmitChunk>(B, scat, s, [&](size_t i) { return srows[i]; });
  ++m->flow_runs;
  if (has_g) launch_gather_rows(m->W(m->emb_g.off), sid, g, B, gin, c.n_speakers, nullptr, s, m->voice_table());
  launch_gather_windows(rows, z, B, I, T, s);
  // the planner sees a length past the narrow kernel's for every window (kLiveRouteFrames): what a window computes does
  // not depend on how the utterance was cut, and equals the whole-utterance run of more than 256 frames
  if (int rc = run_flows(m, true, z, has_g ? g : nullptr, fb, lens, B, T, s, T > kLiveRouteFrames ? T : kLiveRouteFrames)) return rc;
  launch_scatter_z_rows(z, lens, scat, B, I, T, max_keep, s);
  HIPCHK(m, hipGetLastError());
  return 0;
}


int64_t mbv_read_stage(mbv_model* m, const char* name, float* dst, int64_t capacity, void* stream) {
  if (!m || !name) return -1;
  const mbv_config& c = m->cfg;
  DeviceGuard dev_guard_(c.device);
  if (!dev_guard_.ok) { m->fail("hipSetDevice(%d) failed", c.device); return -1; }
  std::string n(name);
  const float* src = nullptr;
  int64_t numel = 0;
  // m_text / logs_text are strided halves of `stats` [B, 2I, T]
  if (n == "m_text" || n == "logs_text") {
    auto it = m->stages.find("stats");
    const EncRun* r = m->cur >= 0 ? &m->runs[m->cur] : nullptr;     // (the stage must be this run's: a later pooled run may be current)
    if (it == m->stages.end() || !it->second.live() || !r || it->second.ptr != r->stats) { m->fail("stage '%s' not available", name); return -1; }
    const int I = c.inter_channels, B = r->B, T = r->T;
    numel = (int64_t)B * I * T;
    if (!dst) return numel;
    if (capacity < numel) { m->fail("capacity too small"); return -1; }
    const float* base = it->second.ptr + (n == "logs_text" ? (size_t)I * T : 0);
    if (hipMemcpy2DAsync(dst, (size_t)I * T * 4, base, (size_t)2 * I * T * 4, (size_t)I * T * 4,
                         B, hipMemcpyDeviceToDevice, (hipStream_t)stream) != hipSuccess) {
      m->fail("hipMemcpy2DAsync failed"); return -1;
    }
    return numel;
  }
  auto it = m->stages.find(n);
  if (it == m->stages.end() || !it->second.live()) { m->fail("stage '%s' not available", name); return -1; }
  src = it->second.ptr; numel = it->second.numel;
  if (!dst) return numel;
  if (capacity < numel) { m->fail("capacity too small"); return -1; }
  if (n == "x_post") {     // stored pre-scaled for the iSTFT kernel: hand back the reference's units
    launch_unscale_xpost(src, dst, (int)(numel / (m->xpost_rows * (int64_t)m->xpost_F)), m->xpost_rows, m->xpost_F, (hipStream_t)stream);
    return numel;
  }
  if (hipMemcpyAsync(dst, src, numel * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream) != hipSuccess) {
    m->fail("hipMemcpyAsync failed"); return -1;
  }
  return numel;
}

int mbv_op_rel_attention(mbv_model* m, const float* qkv, const float* emb_k, const float* emb_v, const int64_t* lengths,
                         float* o, int B, int H, int n_heads, int T, void* stream) {
  if (!m) return 1;
  if (!qkv || !emb_k || !emb_v || !lengths || !o || B <= 0 || T <= 0 || n_heads <= 0 || H % n_heads || (H / n_heads) % 2 || H / n_heads > 128)
    return m->fail("mbv_op_rel_attention: bad arguments (head dimension must be even and <= 128, as in mbv_create)");
  DEVICE_GUARD(m);
  hipStream_t s = (hipStream_t)stream;
  int* lens32 = nullptr;
  HIPCHK(m, hipMalloc((void**)&lens32, (size_t)B * sizeof(int) * 2));
  launch_lens_to_i32(lengths, lens32, B, T, lens32 + B, s);
  launch_rel_attention(qkv, emb_k, emb_v, lens32, o, B, H, n_heads, T, s);
  const hipError_t e = hipStreamSynchronize(s);
  (void)hipFree(lens32);
  HIPCHK(m, e);
  HIPCHK(m, hipGetLastError());
  return 0;
}

// ---- the small kernels by themselves (tests): the launchers of ops.hip / sdp.hip with the argument patterns of
// mbv_encode / mbv_synthesize / mbv_voice_conversion.  Arguments are checked before anything is launched.
#define OP_REFUSE(cond, msg) \
  do { if (cond) return m->fail("%s: %s", __func__, msg); } while (0)
#define OP_BEGIN()       \
  DEVICE_GUARD(m);       \
  hipStream_t s = (hipStream_t)stream
#define OP_END()                       \
  HIPCHK(m, hipGetLastError());        \
  HIPCHK(m, hipStreamSynchronize(s));  \
  return 0
namespace {
constexpr int kGridYZ = 65535;     // a grid's y / z extent (the batch, and a channel count in some kernels)
constexpr int kLnMaxC = 256;       // the channel LayerNorm tiles of ops.hip / sdp.hip: 8 groups x 32 values per thread
}  // namespace

int mbv_op_embed(mbv_model* m, const int64_t* ids, const int64_t* lengths, const float* emb, float* x, int32_t* lens32,
                 int32_t* bad, int B, int T, int H, int n_vocab, void* stream) {
  if (!m) return 1;
  OP_REFUSE(!ids || !lengths || !emb || !x || !lens32 || !bad, "NULL argument");
  OP_REFUSE(B <= 0 || T <= 0 || H <= 0 || n_vocab <= 0, "B, T, H and n_vocab must be > 0");
  OP_REFUSE(B > kGridYZ || H > kGridYZ, "B and H must be <= 65535");
  OP_BEGIN();
  launch_embed(ids, lengths, emb, x, lens32, bad, B, T, H, n_vocab, s);
  OP_END();
}

int mbv_op_layernorm(mbv_model* m, const float* a, const float* r, const float* gamma, const float* beta, float* y,
                     int B, int C, int T, int pre_relu, const int32_t* out_lens, void* stream) {
  if (!m) return 1;
  OP_REFUSE(!a || !gamma || !beta || !y, "NULL argument");
  OP_REFUSE(B <= 0 || T <= 0 || B > kGridYZ, "B in [1, 65535] and T > 0 required");
  OP_REFUSE(C <= 0 || C > kLnMaxC, "C must be in [1, 256]");
  OP_BEGIN();
  launch_layernorm(a, r, gamma, beta, y, B, C, T, pre_relu, out_lens, s);
  OP_END();
}

int mbv_op_durations(mbv_model* m, const float* h, const float* w, const float* bias, const int32_t* lens,
                     float length_scale, float* logw, float* w_ceil, int32_t* cum, int32_t* ylen32, int64_t* ylen64,
                     const int32_t* bad, int B, int C, int T, void* stream) {
  if (!m) return 1;
  OP_REFUSE(!h || !lens || !logw || !w_ceil || !cum || !ylen32, "NULL argument");
  OP_REFUSE((w != nullptr) != (bias != nullptr), "w and bias come together (both NULL: h is logw)");
  OP_REFUSE(B <= 0 || T <= 0, "B and T must be > 0");
  OP_REFUSE(w ? C <= 0 : C != 1, "C must be > 0 with w, 1 without");
  OP_REFUSE(!(length_scale > 0.f) || !(length_scale < INFINITY), "length_scale must be positive and finite");
  OP_BEGIN();
  launch_durations(h, w, bias, lens, length_scale, logw, w_ceil, cum, ylen32, ylen64, bad, B, C, T, s);
  OP_END();
}

int mbv_op_shape_durations(mbv_model* m, const float* logw, const int32_t* lens, const float* scale, const int32_t* extra,
                           float scalar, const mbv_fit* fit_host, float* w_ceil, int32_t* cum, int32_t* ylen32,
                           int64_t* ylen64, const int32_t* bad, mbv_fit_result* fit_out, int B, int T, void* stream) {
  if (!m) return 1;
  OP_REFUSE(!logw || !lens || !w_ceil || !cum || !ylen32, "NULL argument");
  OP_REFUSE(B <= 0 || T <= 0, "B and T must be > 0");
  OP_REFUSE(!(scalar >= 0.f) || !(scalar < INFINITY), "scalar must be finite and >= 0");
  OP_REFUSE(scale && scalar != 1.f, "a scale table needs scalar 1");
  bool any_fit = false;
  for (int b = 0; fit_host && b < B; ++b) {
    if (const char* why = fit_error(fit_host[b])) return m->fail("%s: row %d: %s", __func__, b, why);
    any_fit = any_fit || fit_host[b].frames > 0;
  }
  OP_REFUSE(!scale && !extra && !any_fit, "nothing to do (no scale table, no extra frames, no fit)");
  OP_BEGIN();
  const ShapeRow* fit = nullptr;
  if (upload_fit(m, fit_host, B, &fit, s)) return 1;
  launch_shape_durations(logw, lens, scale, extra, scalar, fit, w_ceil, cum, ylen32, ylen64, bad, nullptr,
                         reinterpret_cast<FitOut*>(fit_out), B, T, s);
  ++m->shape_runs;
  OP_END();
}

int mbv_op_frame_gain(mbv_model* m, const int32_t* cum, const int64_t* y_lengths, const float* gain, float* out,
                      int64_t out_stride, int frames, int B, int T, void* stream) {
  if (!m) return 1;
  OP_REFUSE(!cum || !y_lengths || !gain || !out, "NULL argument");
  OP_REFUSE(B <= 0 || T <= 0, "B and T must be > 0");
  OP_REFUSE(B > kGridYZ, "B <= 65535 required");
  OP_REFUSE(frames < 1 || frames > (1 << 30), "frames must be in [1, 2^30]");
  OP_REFUSE(out_stride < (int64_t)frames + 1, "out_stride must be >= frames + 1");
  OP_BEGIN();
  launch_frame_gain(cum, nullptr, y_lengths, gain, out, out_stride, frames, B, T, s);
  ++m->gain_runs;
  OP_END();
}

int mbv_op_expand(mbv_model* m, const float* stats, const int32_t* cum, const int32_t* ylen32, const float* noise,
                  float noise_scale, float* m_p, float* logs_p, float* z_p, float* z, float* attn, float* y_mask,
                  int B, int I, int T, int Tp, void* stream) {
  if (!m) return 1;
  OP_REFUSE(!stats || !cum || !ylen32 || !z, "NULL argument");
  OP_REFUSE(B <= 0 || I <= 0 || T <= 0 || Tp <= 0, "B, I, T and Tp must be > 0");
  OP_REFUSE(B > kGridYZ || Tp > kGridYZ || (I + 15) / 16 > kGridYZ, "B, Tp <= 65535 required");
  OP_BEGIN();
  // m_text / logs_text: the two halves of the [B, 2I, T] buffer, as mbv_synthesize passes them
  launch_expand(stats, stats + (size_t)I * T, (int64_t)2 * I * T, cum, ylen32, noise_scale != 0.f ? noise : nullptr,
                noise_scale, m_p, logs_p, z_p, z, attn, y_mask, B, I, T, Tp, s);
  OP_END();
}

int mbv_op_cond_gemv(mbv_model* m, const float* g, const float* W, const float* bias, float* out, int B, int Cin,
                     int Cout, void* stream) {
  if (!m) return 1;
  OP_REFUSE(!g || !W || !out, "NULL argument");
  OP_REFUSE(B <= 0 || Cin <= 0 || Cout <= 0 || B > kGridYZ, "B in [1, 65535], Cin and Cout > 0 required");
  OP_BEGIN();
  launch_cond_gemv(g, nullptr, nullptr, W, bias, out, B, Cin, Cout, s);
  OP_END();
}

int mbv_op_gather_rows(mbv_model* m, const float* table, const int64_t* sid, float* out, int B, int C, int n_rows,
                       int32_t* bad, void* stream) {
  if (!m) return 1;
  OP_REFUSE(!table || !sid || !out, "NULL argument");
  OP_REFUSE(B <= 0 || C <= 0 || n_rows <= 0 || B > kGridYZ, "B in [1, 65535], C and n_rows > 0 required");
  OP_BEGIN();
  launch_gather_rows(table, sid, out, B, C, n_rows, bad, s);
  OP_END();
}

int mbv_op_posterior_sample(mbv_model* m, const float* stats, const float* noise, const int32_t* lens, float* z,
                            int B, int I, int T, void* stream) {
  if (!m) return 1;
  OP_REFUSE(!stats || !lens || !z, "NULL argument");
  OP_REFUSE(B <= 0 || I <= 0 || T <= 0 || B > kGridYZ || I > kGridYZ, "B, I in [1, 65535] and T > 0 required");
  OP_BEGIN();
  launch_posterior_sample(stats, noise, lens, z, B, I, T, s);
  OP_END();
}

int mbv_op_lens(mbv_model* m, const int64_t* lengths, int32_t* lens32, int32_t* bad, float* mask, int B, int T,
                void* stream) {
  if (!m) return 1;
  OP_REFUSE(!lengths || !lens32 || !bad, "NULL argument");
  OP_REFUSE(B <= 0 || T <= 0 || B > kGridYZ, "B in [1, 65535] and T > 0 required");
  OP_BEGIN();
  launch_lens_to_i32(lengths, lens32, B, T, bad, s);
  if (mask) launch_sequence_mask(lens32, mask, B, T, s);
  OP_END();
}

int mbv_op_dds_sep(mbv_model* m, const float* x, const int32_t* lens, const float* w, const float* bias,
                   const float* gamma, const float* beta, float* y, int B, int C, int T, int K, int dil, void* stream) {
  if (!m) return 1;
  OP_REFUSE(!x || !lens || !w || !bias || !gamma || !beta || !y, "NULL argument");
  OP_REFUSE(x == y, "y must not be x (columns read their neighbours)");
  OP_REFUSE(B <= 0 || T <= 0 || B > kGridYZ, "B in [1, 65535] and T > 0 required");
  OP_REFUSE(C <= 0 || C > kLnMaxC, "C must be in [1, 256]");
  OP_REFUSE(K != 3 || (dil != 1 && dil != 3 && dil != 9), "K = 3 and dil in {1, 3, 9} (the DDSConv of the model)");
  OP_BEGIN();
  launch_dds_sep(x, lens, w, bias, gamma, beta, y, B, C, T, K, dil, s);
  OP_END();
}

int mbv_op_dds_res(mbv_model* m, const float* a, const float* xres, const float* gamma, const float* beta, float* y,
                   int B, int C, int T, const int32_t* out_lens, void* stream) {
  if (!m) return 1;
  OP_REFUSE(!a || !xres || !gamma || !beta || !y, "NULL argument");
  OP_REFUSE(B <= 0 || T <= 0 || B > kGridYZ, "B in [1, 65535] and T > 0 required");
  OP_REFUSE(C <= 0 || C > kLnMaxC, "C must be in [1, 256]");
  OP_BEGIN();
  launch_dds_res(a, xres, gamma, beta, y, B, C, T, out_lens, s);
  OP_END();
}

int mbv_op_sdp_pre(mbv_model* m, const float* z, int zc, const float* pre_w, const float* pre_b, const float* cond,
                   float* h, int B, int C, int T, void* stream) {
  if (!m) return 1;
  OP_REFUSE(!z || !pre_w || !pre_b || !cond || !h, "NULL argument");
  OP_REFUSE(zc != 0 && zc != 1, "zc must be 0 or 1");
  OP_REFUSE(B <= 0 || C <= 0 || T <= 0 || B > kGridYZ || C > kGridYZ, "B, C in [1, 65535] and T > 0 required");
  OP_BEGIN();
  launch_sdp_pre(z, zc, pre_w, pre_b, cond, h, B, C, T, s);
  OP_END();
}

int mbv_op_sdp_spline(mbv_model* m, const float* h, float* z, const int32_t* lens, int B, int C, int T,
                      float edge_const, void* stream) {
  if (!m) return 1;
  OP_REFUSE(!h || !z || !lens, "NULL argument");
  OP_REFUSE(B <= 0 || C <= 0 || T <= 0 || B > kGridYZ, "B in [1, 65535], C and T > 0 required");
  OP_BEGIN();
  launch_sdp_spline(h, z, lens, B, C, T, edge_const, s);
  OP_END();
}

int mbv_op_sdp_logw(mbv_model* m, const float* z, const float* mean, const float* logs, const int32_t* lens,
                    float* logw, int B, int T, void* stream) {
  if (!m) return 1;
  OP_REFUSE(!z || !mean || !logs || !lens || !logw, "NULL argument");
  OP_REFUSE(B <= 0 || T <= 0 || B > kGridYZ, "B in [1, 65535] and T > 0 required");
  OP_BEGIN();
  launch_sdp_logw(z, mean, logs, lens, logw, B, T, s);
  OP_END();
}

int mbv_op_sdp_noise(mbv_model* m, const float* noise, float scale, float* z, int64_t n, void* stream) {
  if (!m) return 1;
  OP_REFUSE(!z, "NULL argument");
  OP_REFUSE(n <= 0 || n > ((int64_t)1 << 31), "n must be in [1, 2^31]");
  OP_BEGIN();
  launch_sdp_noise(noise, scale, z, n, s);
  OP_END();
}

int mbv_op_chan_add(mbv_model* m, float* x, const float* v, int B, int C, int T, void* stream) {
  if (!m) return 1;
  OP_REFUSE(!x || !v, "NULL argument");
  OP_REFUSE(B <= 0 || C <= 0 || T <= 0 || B > kGridYZ || C > kGridYZ, "B, C in [1, 65535] and T > 0 required");
  OP_BEGIN();
  launch_chan_add(x, v, B, C, T, s);
  OP_END();
}

int mbv_op_istft_single(mbv_model* m, const float* x_post, int B, int frames, int prescaled, float* o, float* spec,
                        float* phase, void* stream) {
  if (!m) return 1;
  OP_REFUSE(!x_post || !o, "NULL argument");
  OP_REFUSE(B <= 0 || frames < 2, "B > 0 and frames >= 2 required");
  OP_REFUSE((int64_t)B * 18 * frames * 4 >= (1LL << 31), "x_post must stay below 2 GiB");
  OP_BEGIN();
  IstftSbArgs a{};
  a.x_post = x_post; a.o = o; a.spec = spec; a.phase = phase;
  a.B = B; a.F = frames; a.exact_math = m->exact_math; a.prescaled = prescaled != 0;
  launch_istft_single(a, s);
  OP_END();
}

int mbv_op_neg_cent(mbv_model* m, const float* z_p, const float* m_p, const float* logs_p, const int32_t* t_y32,
                    const int32_t* t_x32, float* value, int B, int I, int T_t, int T_s, void* stream) {
  if (!m) return 1;
  OP_REFUSE(!z_p || !m_p || !logs_p || !t_y32 || !t_x32 || !value, "NULL argument");
  OP_REFUSE(B <= 0 || I <= 0 || T_t <= 0 || T_s <= 0, "B, I, T_t and T_s must be > 0");
  OP_REFUSE(B > kGridYZ || (T_t + 63) / 64 > kGridYZ, "B <= 65535 and T_t <= 64 * 65535 required");
  OP_BEGIN();
  launch_neg_cent(z_p, m_p, logs_p, (int64_t)I * T_s, t_y32, t_x32, value, B, I, T_t, T_s, s);
  OP_END();
}

int mbv_op_max_path(mbv_model* m, const float* value, const int32_t* t_y32, const int32_t* t_x32, int32_t* w_out,
                    int32_t* path_out, int32_t* status, int B, int T_t, int T_s, void* stream) {
  if (!m) return 1;
  OP_REFUSE(!value || !t_y32 || !t_x32 || !w_out, "NULL argument");
  OP_REFUSE(B <= 0 || T_t <= 0 || T_s <= 0, "B, T_t and T_s must be > 0");
  OP_REFUSE(!max_path_supported(T_s), "T_s must be <= 1024");
  OP_BEGIN();
  const size_t bits_bytes = max_path_scratch_bytes(B, T_t, T_s);
  if (bits_bytes && ensure(m, m->scrB, bits_bytes)) return 1;
  launch_max_path(value, t_y32, t_x32, w_out, path_out, status, bits_bytes ? m->scrB.p : nullptr, B, T_t, T_s, s);
  OP_END();
}
#undef OP_REFUSE
#undef OP_BEGIN
#undef OP_END

int mbv_op_conv1d(mbv_model* m, const float* x, const float* w_host, const float* bias_host, float* y,
                  int B, int Cin, int Cout, int T, int K, int dilation, float in_slope, void* stream) {
  if (!m) return 1;
  if (Cin % 32) return m->fail("mbv_op_conv1d: Cin must be a multiple of 32");
  if (!conv1d_supported(K, dilation)) return m->fail("mbv_op_conv1d: K <= 11 and (K-1)*dilation <= 72 required");
  DEVICE_GUARD(m);
  hipStream_t s = (hipStream_t)stream;
  const int Mpad = (int)align_up(Cout, 128);
  std::vector<float> packed((size_t)K * Cin * Mpad, 0.f);
  for (int k = 0; k < K; ++k)
    for (int ci = 0; ci < Cin; ++ci)
      for (int co = 0; co < Cout; ++co)
        packed[conv_pack_index(k, ci, co, Cin, Mpad)] = w_host[((size_t)co * Cin + ci) * K + k];
  float *dw = nullptr, *db = nullptr;
  HIPCHK(m, hipMalloc((void**)&dw, packed.size() * 4));
  HIPCHK(m, hipMemcpy(dw, packed.data(), packed.size() * 4, hipMemcpyHostToDevice));
  if (bias_host) {
    HIPCHK(m, hipMalloc((void**)&db, (size_t)Cout * 4));
    HIPCHK(m, hipMemcpy(db, bias_host, (size_t)Cout * 4, hipMemcpyHostToDevice));
  }
  ConvArgs a{};
  a.x = x; a.x_bstride = (int64_t)Cin * T; a.Tin = T; a.x_rstride = T; a.Cin = Cin;
  a.w = dw; a.bias = db; a.M = Cout; a.Mpad = Mpad; a.K = K; a.dil = dilation;
  a.pad_left = (K - 1) * dilation / 2; a.in_slope = in_slope;
  a.y = y; a.y_bstride = (int64_t)Cout * T; a.T = T; a.epi = EPI_STORE; a.out_scale = 1.f; a.B = B;
  a.ws = m->conv_ws; a.ws_floats = m->conv_ws_floats; a.counters = m->conv_cnt; a.n_counters = m->conv_ncnt;
  a.splitk = m->splitk;
  float* dws = nullptr;
  if (m->conv_bf16 == 3) {                           // the split copy of this call's weights
    HIPCHK(m, hipMalloc((void**)&dws, packed.size() * 4));
    launch_split_planes(dw, dws, packed.size(), s);
    a.w_split = dws;
  }
  a.prec = a.w_split ? 3 : 0;
  launch_conv1d(a, s);
  HIPCHK(m, hipStreamSynchronize(s));
  HIPCHK(m, hipFree(dw));
  if (dws) HIPCHK(m, hipFree(dws));
  if (db) HIPCHK(m, hipFree(db));
  return 0;
}

}  // extern "C"

// ---- mbv_op_conv / mbv_conv_plan: a descriptor as ConvArgs (shape and options; no weights)
namespace {
static_assert(MBV_ROUTE_NARROW_M == CONV_NARROW_M && MBV_ROUTE_NARROW_LAUNCH == CONV_NARROW_LAUNCH &&
              MBV_ROUTE_M64 == CONV_M64 && MBV_ROUTE_HALF == CONV_HALF && MBV_ROUTE_SMALL == CONV_SMALL &&
              MBV_ROUTE_BIG == CONV_BIG && MBV_ROUTE_SPLIT_BATCH == CONV_SPLIT_BATCH && MBV_ROUTE_VS == CONV_VS &&
              MBV_ROUTE_TAIL_PACK == CONV_TAIL_PACK,
              "route numbers of the C-ABI and the launcher");
static_assert(MBV_CONV_EPI_LN == EPI_LN, "epilogue numbers of the C-ABI and the launcher");

// null on success, else why the descriptor is refused
const char* conv_desc_args(const mbv_conv_desc& d, ConvArgs* out) {
  const bool convt = d.kind == MBV_CONV_KIND_CONVT4 || d.kind == MBV_CONV_KIND_CONVT8;
  if (d.kind != MBV_CONV_KIND_CONV && !convt) return "kind must be MBV_CONV_KIND_CONV, _CONVT4 or _CONVT8";
  if (d.B <= 0 || d.Cin <= 0 || d.Cout <= 0 || d.Tin <= 0 || d.T <= 0) return "B, Cin, Cout, Tin and T must be > 0";
  if (d.x_rstride != 0 && d.x_rstride < d.Tin) return "x_rstride must be 0 or >= Tin";
  const bool ln = d.epi == MBV_CONV_EPI_LN;
  if ((d.epi < MBV_CONV_EPI_STORE || d.epi > MBV_CONV_EPI_RESID_ACC) && !ln) return "epi must be STORE, RESID, RESID_ACC or LN";
  if (d.prec != 0 && d.prec != 3) return "prec must be 0 or 3";
  if (d.epi == MBV_CONV_EPI_STORE && (d.res || d.res_chan_add)) return "res / res_chan_add need a RESID epilogue";
  if (d.epi != MBV_CONV_EPI_STORE && !ln && !d.res) return "RESID and RESID_ACC need res";
  if (d.epi != MBV_CONV_EPI_STORE && !ln && (d.out_lens || d.relu)) return "out_lens / relu belong to STORE and LN";
  if (!ln && (d.ln_gamma || d.ln_beta || d.ln_out_lens)) return "ln_gamma / ln_beta / ln_out_lens belong to LN";
  if (ln) {
    if (convt) return "LN: a conv only";
    if (!d.ln_gamma || !d.ln_beta) return "LN needs ln_gamma and ln_beta";
    if (d.res_chan_add || d.trim_lens || d.prec) return "LN takes no res_chan_add, no trimmed launch and no prec 3";
    if (d.T > 256) return "LN: T <= 256 (the narrow kernel's rule in mbv_encode)";
  }
  if (d.epi != MBV_CONV_EPI_RESID_ACC && d.accum_in) return "accum_in belongs to RESID_ACC";
  if (d.legacy_convt) return "legacy_convt must be 0 (the stand-alone ConvTranspose kernel was removed)";
  if (d.trim_lens && d.splitk) return "a trimmed launch takes no split-K";
  if (d.tail_once < 0 || d.tail_once > 2) return "tail_once must be 0, 1 or 2";
  if (d.tail_once && (!d.trim_lens || convt || ln)) return "tail_once needs trim_lens and a conv with a STORE / RESID / RESID_ACC epilogue";
  const int U = d.kind;
  if (convt) {
    if (d.T != d.Tin) return "ConvTranspose: T must equal Tin (input frames)";
    if (d.epi != MBV_CONV_EPI_STORE || d.out_lens || d.relu || d.reflect1) return "ConvTranspose: plain STORE only";
    if (d.Cin % 16 || d.Cout % 32) return "ConvTranspose: Cin % 16 == 0 and Cout % 32 == 0";
  } else {
    if (d.Cin % 32) return "conv: Cin must be a multiple of 32";
    if (!conv1d_supported(d.K, d.dil)) return "conv: K <= 11 and (K - 1) * dil <= 72 required";
  }
  ConvArgs a{};
  a.Tin = d.Tin; a.x_rstride = d.x_rstride ? d.x_rstride : d.Tin; a.Cin = d.Cin;
  a.x_bstride = (int64_t)d.Cin * a.x_rstride;
  a.M = convt ? U * d.Cout : d.Cout;
  a.Mpad = (int)align_up(a.M, 128);
  a.K = convt ? convt_taps(U) : d.K;
  a.dil = convt ? 1 : d.dil;
  a.pad_left = convt ? convt_pad_left(U) : (a.K - 1) * a.dil / 2;        // (decoder_table)
  a.in_slope = d.in_slope;
  a.in_lens = d.in_lens; a.chan_add = d.chan_add; a.reflect1 = d.reflect1;
  a.T = d.T;
  a.y_bstride = (int64_t)d.Cout * d.T * (convt ? U : 1);
  a.epi = convt ? EPI_CONVT : d.epi;
  a.convt_u = convt ? U : 0;
  a.relu = d.relu; a.out_lens = d.out_lens;
  a.res = d.res; a.res_bstride = (int64_t)d.Cout * d.T; a.res_chan_add = d.res_chan_add;
  a.accum_in = d.accum_in; a.out_scale = d.epi == MBV_CONV_EPI_RESID_ACC ? d.out_scale : 1.f;
  a.B = d.B;
  a.splitk = d.splitk != 0;
  a.prec = d.prec;
  a.tail_pack = d.tail_once == 2;        // (the planner grants the packed route where the kernel is built for it)
  if ((a.epi == EPI_RESID || a.epi == EPI_RESID_ACC) && (unsigned long long)a.M * a.T * 4ull >= (1ull << 32))
    return "one utterance's output exceeds 4 GiB";
  if (ln) {
    a.ln_gamma = d.ln_gamma; a.ln_beta = d.ln_beta; a.ln_out_lens = d.ln_out_lens;
    if (!conv1d_narrow_supported(a)) return "LN outside the narrow kernel's range (conv1d_narrow_supported)";
  }
  *out = a;
  return nullptr;
}

void plan_ints(const ConvPlan& p, int32_t* out) {
  const int32_t v[8] = {p.route, p.bm, p.bn, p.threads, p.ck, p.nb_big, p.vs_tv, p.S};
  std::memcpy(out, v, sizeof v);
}

// the plan of a (validated) descriptor; trimmed launches take the tile width conv1d_trim_bn names (0: refused)
const char* conv_desc_plan(const mbv_conv_desc& d, const ConvArgs& a, ConvPlan* p) {
  if (d.trim_lens) {
    const int bn = conv1d_trim_bn(a);
    if (!bn) return "this conv runs on a kernel without trimmed launches (conv1d_trim_bn 0)";
    *p = conv1d_plan(a, true);
    if (p->bn != bn) return "internal error: conv1d_trim_bn and the trimmed plan disagree";
    return nullptr;
  }
  *p = conv1d_plan(a, false);
  return nullptr;
}

struct DevAllocs {                 // frees on every exit path (after the launch: the caller synchronised)
  std::vector<void*> p;
  ~DevAllocs() { for (void* q : p) (void)hipFree(q); }
};
}  // namespace

extern "C" {

int mbv_conv_plan(const mbv_conv_desc* d, int32_t out[8]) {
  if (!d || !out) { g_create_error = "mbv_conv_plan: NULL argument"; return 1; }
  ConvArgs a{};
  const char* why = conv_desc_args(*d, &a);
  ConvPlan p{};
  if (!why) {
    a.ws_floats = d->ws_floats > 0 ? (size_t)d->ws_floats : 0;
    a.n_counters = d->n_counters > 0 ? d->n_counters : 0;
    why = conv_desc_plan(*d, a, &p);
  }
  if (why) { g_create_error = std::string("mbv_conv_plan: ") + why; return 1; }
  plan_ints(p, out);
  return 0;
}

int mbv_op_conv(mbv_model* m, const mbv_conv_desc* d, const float* x, const float* w_host, const float* bias_host,
                float* y, int32_t* plan_out, void* stream) {
  if (!m) return 1;
  if (!d || !x || !w_host || !y) return m->fail("mbv_op_conv: NULL argument");
  ConvArgs a{};
  const char* why = conv_desc_args(*d, &a);
  if (why) return m->fail("mbv_op_conv: %s", why);
  a.ws = m->conv_ws; a.ws_floats = m->conv_ws_floats; a.counters = m->conv_cnt; a.n_counters = m->conv_ncnt;
  if (m->splitk && !d->trim_lens) a.splitk = 1;      // the handle's low-latency mode (an explicit trim wins)
  ConvPlan p{};
  if ((why = conv_desc_plan(*d, a, &p))) return m->fail("mbv_op_conv: %s", why);
  DEVICE_GUARD(m);
  hipStream_t s = (hipStream_t)stream;
  DevAllocs mem;
  auto upload = [&](const void* src, size_t bytes, void** dst) -> int {
    HIPCHK(m, hipMalloc(dst, bytes));
    mem.p.push_back(*dst);
    HIPCHK(m, hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice));
    return 0;
  };
  const bool convt = a.epi == EPI_CONVT;
  const int U = a.convt_u;
  std::vector<float> zero_bias;
  if (!bias_host) { zero_bias.assign(d->Cout, 0.f); bias_host = zero_bias.data(); }
  std::vector<float> wp((size_t)a.K * a.Cin * a.Mpad, 0.f), bp(a.M);
  if (convt) {
    pack_convt_rows(w_host, bias_host, a.Cin, d->Cout, U, a.Mpad, wp.data(), bp.data());
  } else {
    std::vector<int> rows(a.M);
    for (int i = 0; i < a.M; ++i) rows[i] = i;
    pack_conv_rows(w_host, a.Cin, a.K, rows.data(), a.M, nullptr, a.Mpad, wp.data());
    std::memcpy(bp.data(), bias_host, (size_t)a.M * 4);
  }
  void *dw = nullptr, *db = nullptr;
  if (upload(wp.data(), wp.size() * 4, &dw) || upload(bp.data(), bp.size() * 4, &db)) return 1;
  a.w = (const float*)dw; a.bias = (const float*)db;
  if (a.prec == 3) {                               // the split copy of this call's weights
    void* dws = nullptr;
    HIPCHK(m, hipMalloc(&dws, wp.size() * 4));
    mem.p.push_back(dws);
    launch_split_planes(a.w, (float*)dws, wp.size(), s);
    a.w_split = (const float*)dws;
  }
  a.x = x; a.y = y;
  if (d->trim_lens) {
    std::vector<int> l32(d->B);
    for (int b = 0; b < d->B; ++b) {
      const int64_t v = d->trim_lens[b];
      l32[b] = v < 0 ? 0 : (v > a.T ? a.T : (int)v);
    }
    void* dl = nullptr;
    if (upload(l32.data(), l32.size() * 4, &dl)) return 1;
    void* map = nullptr;
    HIPCHK(m, hipMalloc(&map, launch_trim_map_ints(d->B, a.T, p.bn) * sizeof(int)));
    mem.p.push_back(map);
    if (d->tail_once) {
      if (d->B > 65535) return m->fail("mbv_op_conv: tail_once takes at most 65535 rows");
      const bool packed = p.route == CONV_TAIL_PACK;
      const int halo = (a.K - 1) * a.dil, gap = tail_pack_gap(halo);
      void* tmap = nullptr;
      HIPCHK(m, hipMalloc(&tmap, (packed ? tail_pack_ints(d->B, a.T, gap, p.bn) : launch_tail_map_ints(d->B, a.T, p.bn)) * sizeof(int)));
      mem.p.push_back(tmap);
      TailMapJobs jobs{};
      jobs.job[0] = {d->trim_num, d->trim_add, a.T, p.bn, (int*)tmap, packed ? gap : 0, packed ? halo - a.pad_left : 0};
      launch_tail_maps((const int*)dl, d->B, jobs, 1, m->tail_cnt, s);
      if (packed) {
        a.pack_tbl = (const int*)tmap; a.pack_blocks = tail_pack_blocks(d->B, a.T, gap, p.bn);
        launch_conv1d(a, s);
        launch_tail_fill(a.y, a.y_bstride, a.B, a.M, a.T, p.bn, a.pack_tbl, s, true);
        HIPCHK(m, hipGetLastError());
        HIPCHK(m, hipStreamSynchronize(s));
        if (plan_out) plan_ints(p, plan_out);
        return 0;
      }
      map = tmap;
    } else {
      launch_trim_map((const int*)dl, d->B, d->trim_num, d->trim_add, a.T, p.bn, (int*)map, s);
    }
    a.trim_map = (const int*)map; a.trim_bn = p.bn;
  }
  launch_conv1d(a, s);
  if (d->tail_once) launch_tail_fill(a.y, a.y_bstride, a.B, a.M, a.T, a.trim_bn, a.trim_map, s);
  HIPCHK(m, hipGetLastError());
  HIPCHK(m, hipStreamSynchronize(s));
  if (plan_out) plan_ints(p, plan_out);
  return 0;
}

int mbv_tail_pack_table(const int64_t* lens, int B, int num, int reach, int T, int halo, int pad_right, int bn,
                        int32_t* out, int64_t capacity) {
  if (!lens || B <= 0 || T <= 0 || halo < 0 || pad_right < 0 || pad_right > halo || bn < 32 || bn % 32) return -1;
  const int gap = tail_pack_gap(halo);
  const int64_t n = (int64_t)tail_pack_ints(B, T, gap, bn);
  if (!out) return n > 0x7fffffff ? -1 : (int)n;
  if (capacity < n || n > 0x7fffffff) return -1;
  auto len_of = [&](int b) { return lens[b] < 0 ? 0 : (lens[b] > T ? (int64_t)T : lens[b]); };   // (mbv_op_conv's clamp)
  int donor = 0;
  for (int b = 1; b < B; ++b) if (len_of(b) < len_of(donor)) donor = b;
  int run = 0;
  for (int b = 0; b < B; ++b) {
    const int sp = tail_pack_sp(len_of(b), num, reach, T, b == donor);
    out[kTailPackHdr + b] = sp;
    tail_pack_row(out, B, b, run, sp, gap, pad_right);
    run += tail_pack_row_blocks(sp, gap);
  }
  for (int i = kTailPackHdr + B; i < tail_pack_entries_at(B); ++i) out[i] = 0;
  tail_pack_finish(out, B, T, gap, bn, donor, run);
  return (int)n;
}

}  // extern "C"
