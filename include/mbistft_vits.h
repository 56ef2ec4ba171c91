/*
 * mbistft_vits.h — C-ABI of the MI355X-native MB-iSTFT-VITS inference path.
 *
 * The reference has no FFI/plugin layer: its boundary for this path is the
 * Python class surface `models.SynthesizerTrn` (+ `utils.HParams`).  This
 * header is what a reference-side binding (ctypes) binds
 * to replace the body of each method; every entry point names the reference
 * interface it replaces (file:line under the reference repo).
 *
 * Conventions
 *   - plain C, no torch types: raw device pointers + sizes; all tensors are
 *     fp32, contiguous, [B, C, time] with time fastest (ids/lengths int64).
 *   - every call returns 0 on success, non-zero on failure; the message is
 *     available from mbv_last_error().  No C++ exception crosses the ABI.
 *   - kernels are enqueued on the caller's `stream` (a hipStream_t passed as
 *     void*; NULL = default stream).  Calls never synchronise the device
 *     except where stated.
 *   - a handle is not re-entrant (reference callers are single-threaded
 *     w.r.t. the model: tts_vits.py:145,181); handles on different devices are
 *     independent.
 *   - the library owns only its folded-weight arena and scratch workspace;
 *     all inputs/outputs are borrowed for the duration of the call.
 */
#ifndef MBISTFT_VITS_H
#define MBISTFT_VITS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MBV_ABI_VERSION 3   /* 3 (r03): + arena export / import, call tickets, option "trim", mbv_op_rel_attention; structs unchanged
                             * (later additions are new entry points, mbv_randn_blocks / mbv_randn_host / mbv_noise_runs
                             * among them; the test-only mbv_conv_desc grew at its end) */

#define MBV_DEC_MULTIBAND   0   /* models.py:309 Multiband_iSTFT_Generator (fixed PQMF)        */
#define MBV_DEC_MULTISTREAM 1   /* models.py:387 Multistream_iSTFT_Generator (trainable filter)*/
#define MBV_DEC_SINGLEBAND  2   /* models.py:248 iSTFT_Generator (ups 8x8, no filter bank)      */

typedef struct mbv_model mbv_model;   /* opaque */

/* Hyper-parameters: the ctor arguments of models.py:573-599 that shape the
 * infer path (p_dropout, segment_size, n_layers_q … do not).  `struct_bytes` must be sizeof(mbv_config). */
typedef struct mbv_config {
  int32_t struct_bytes;
  int32_t n_vocab;
  int32_t inter_channels;            /* 192 */
  int32_t hidden_channels;           /* 192 (mini: 96) */
  int32_t filter_channels;           /* 768 */
  int32_t n_heads;                   /* 2 */
  int32_t n_layers;                  /* 6 (mini: 3) */
  int32_t kernel_size;               /* FFN kernel, 3 */
  int32_t upsample_initial_channel;  /* 512 (mini: 256) */
  int32_t spec_channels;             /* filter_length / 2 + 1 = 513: input of enc_q (voice conversion) */
  int32_t resblock_kernel_sizes[3];  /* 3,7,11 */
  int32_t resblock_dilations[3][3];  /* 1,3,5 each (ResBlock2: first two used) */
  int32_t resblock_type;             /* 1 = ResBlock1 (modules.py:187), 2 = ResBlock2 (modules.py:237) */
  int32_t n_speakers;                /* 0 = single speaker */
  int32_t gin_channels;              /* 0 or 256 */
  int32_t decoder;                   /* MBV_DEC_* */
  int32_t device;                    /* HIP device ordinal */
  int32_t use_sdp;                   /* 1: dp is the StochasticDurationPredictor (models.py:649-650) */
} mbv_config;

/* Output bundle of phase B / decode.  Any pointer may be NULL to skip
 * materialising that tensor (the reference always returns all of them:
 * models.py:737).  T' = frames, F = 16 T' + 1, all device pointers. */
typedef struct mbv_outputs {
  float *o;        /* [B, 1, 256 T']                         waveform           */
  float *o_mb;     /* MB: [B, 4, 64 T'];  MS: [B, 4, 256 T'] (zero-stuffed); SB: unused */
  float *spec;     /* [B, 4, 9, F]      (SB: [B, 9, F] with F = 64 T' + 1)      */
  float *phase;    /* same shape as spec                                         */
  float *attn;     /* [B, 1, T', T]                          (synthesize only)   */
  float *y_mask;   /* [B, 1, T']                             (synthesize only)   */
  float *z;        /* [B, 192, T']                           (synthesize only)   */
  float *z_p;      /* [B, 192, T']                                               */
  float *m_p;      /* [B, 192, T']                                               */
  float *logs_p;   /* [B, 192, T']                                               */
} mbv_outputs;

/* ---- life cycle ---------------------------------------------------------
 * replaces SynthesizerTrn.__init__ (models.py:573-655). */
int  mbv_abi_version(void);
int  mbv_create(const mbv_config *cfg, mbv_model **out);
void mbv_destroy(mbv_model *m);
/* Message of the last failed call on `m` (or of the last failed mbv_create
 * when m == NULL).  Valid until the next call. */
const char *mbv_last_error(const mbv_model *m);

/* ---- weights --------------------------------------------------------------
 * replaces nn.Module.load_state_dict as used by utils.load_checkpoint
 * (utils.py:22-47).  `name` is the reference state-dict key
 * ("dec.ups.0.weight_v", …); `data` is a HOST pointer to fp32 values of
 * `shape[0..ndim)`.  Keys no module of models.SynthesizerTrn owns (discriminators, optimizer
 * state) are rejected; enc_q.* (voice conversion) and, with use_sdp, the SDP's training-only
 * dp.post_* half are accepted so that a reference checkpoint loads strictly.
 * mbv_finalize_weights folds weight-norm (w = g v/||v||),
 * packs every conv for the kernels, uploads once, and may be called again
 * after further mbv_load_weight calls.  It synchronises `stream`. */
int mbv_load_weight(mbv_model *m, const char *name, const float *data,
                    const int64_t *shape, int ndim);
int mbv_finalize_weights(mbv_model *m, void *stream);

/* ---- the folded weight arena across processes (no reference counterpart; SURVEY §8e: "RCCL broadcast of the
 * folded weight arena from rank 0").  One rank loads the checkpoint and finalizes; the others receive the arena
 * over the collective of their choice (device buffers) and import it: its layout is a function of mbv_config
 * alone, so no state dict, no host-side weight-norm fold and no host->device upload happens on the receivers.
 *   mbv_arena_floats   size of the finalized arena in floats (-1: not finalized)
 *   mbv_export_arena   device-to-device copy of it into dst (capacity in floats)
 *   mbv_import_arena   lay the arena out and fill it from src (device); n_floats must equal the exporter's
 *                      mbv_arena_floats (same configuration, same library build), else the call fails */
int64_t mbv_arena_floats(mbv_model *m);
int mbv_export_arena(mbv_model *m, float *dst, int64_t capacity, void *stream);
int mbv_import_arena(mbv_model *m, const float *src, int64_t n_floats, void *stream);
/* Number of state-dict keys still missing before finalize can succeed;
 * writes up to `cap` bytes of a comma-separated list into `buf` if non-NULL. */
int mbv_missing_weights(mbv_model *m, char *buf, size_t cap);

/* ---- phase A: text encoder + duration predictor + durations ---------------
 * replaces models.py:701-719 (enc_p, emb_g, dp, exp/ceil/sum).
 *   ids      int64 [B, T]   device     token ids
 *   lengths  int64 [B]      device     valid tokens per utterance
 *   sid      int64 [B]      device     speaker ids, NULL iff n_speakers == 0
 *   y_lengths_out int64 [B] device     frames per utterance (clamped >= 1); -1 marks an utterance
 *                                      with a token id, length or speaker id out of range (the
 *                                      reference's nn.Embedding raises IndexError there), or with
 *                                      a duration outside the supported range: a token of 2^20
 *                                      frames or more (inf and NaN included) or more than 2^30 in all
 *   noise_w  fp32 [B, 2, T]  device     use_sdp only: the standard-normal draws of models.py:94
 *                                      (NULL == zeros); scaled by noise_scale_w inside.  Ignored
 *                                      by the deterministic DurationPredictor.
 * The caller reads max(y_lengths) back (the one host sync of the path,
 * mirroring commons.py:123) and passes it to mbv_synthesize. */
int mbv_encode(mbv_model *m, const int64_t *ids, const int64_t *lengths, const int64_t *sid,
               int B, int T, float length_scale, const float *noise_w, float noise_scale_w,
               int64_t *y_lengths_out, void *stream);

/* ---- phase B: length regulation + prior + reverse flow + decoder ----------
 * replaces models.py:720-734.
 *   t_frames  T' = max(y_lengths) as read back by the caller
 *   noise     fp32 [B, 192, T'] standard-normal draws (models.py:729), or NULL
 *             (== noise_scale 0)
 *   max_len   decoder input is truncated to this many frames (<=0: none)
 * Output shapes use T'_dec = min(T', max_len) for o/o_mb/spec/phase. */
int mbv_synthesize(mbv_model *m, int t_frames, const float *noise, float noise_scale,
                   int max_len, const mbv_outputs *outs, void *stream);

/* ---- decoder only ----------------------------------------------------------
 * replaces `net.dec(z, g)` (models.py:344-377 / 430-467; callers
 * synthesis_module.py:160, chunked decoding notebooks).
 *   z  fp32 [B, 192, T']   g  fp32 [B, gin, 1] or NULL */
int mbv_decode(mbv_model *m, const float *z, const float *g, int B, int t_frames,
               const mbv_outputs *outs, void *stream);

/* ---- streaming decode (no reference counterpart; replaces the notebooks' chunk stitching) ----------------
 * mbv_decoder_context (host only, like mbv_conv_plan): out = (L, R), the whole z-frames of left and right
 * context any output sample of z-frame t can depend on, [t - L, t + R], derived from the decoder of cfg
 * (conv_pre, the two ConvTranspose1d, the ResBlocks' kernels and dilations, ReflectionPad1d((1,0)) + conv_post,
 * the iSTFT, the 63-tap synthesis filter).  ljs / uudb MB and MS: (25, 24); single band: (13, 13).
 *
 * mbv_decode_range: `net.dec(z, g)[0]` for z-frames [first, first + count) only.  z is the caller's whole
 * [B, 192, t_frames] tensor; only frames [max(0, first - L), min(t_frames, first + count + R)) are read.  Writes
 * samples [256 first, 256 (first + count)) of every row, at o + b o_row_stride, and nothing else (o 16-byte
 * aligned, o_row_stride >= 256 t_frames and a multiple of 4).  In the default mode the samples are bitwise those of
 * mbv_decode on the whole z; with "splitk" within fp32 rounding of it.  Honours "splitk", "dec_streams" and the
 * batch split of x_post; never uses a trim map.  Errors leave the handle usable. */
int mbv_decoder_context(const mbv_config *cfg, int32_t out[2]);
int mbv_decode_range(mbv_model *m, const float *z, const float *g, int B, int t_frames, int first, int count,
                     float *o, int64_t o_row_stride, void *stream);

/* ---- row-exact ragged decode (no reference counterpart: the reference service, tts_vits.py:122-139, decodes one
 * utterance per request; this is what lets a service batch requests and still emit that audio) ----------------
 * OPT-IN, never the default.  Row b of a batch is an utterance of lengths[b] z-frames and is decoded as if alone:
 * its samples [0, 256 lengths[b]) are BITWISE what mbv_decode returns for z[b, :, :lengths[b]] (g[b]) by itself
 * in the default mode, the samples at and past 256 lengths[b] are zeros, and nothing of z at or behind a row's end
 * is read.  (The default decoder is unmasked, as the reference's is — models.py:344-377 / 430-467 / 286-300 —
 * so in a batch the last ~25 z-frames of every row but the longest depend on its batch-mates' lengths.)
 * Every conv masks its input at the row's own length at its rate, only the column tiles below it run, the
 * waveform tail takes the row's own frame count.  The narrow conv kernel (<= 256 columns) and the tiled kernels
 * sum in different orders, so the rows are decoded in one run per CLASS of lengths:
 *
 * mbv_ragged_classes (host only, like mbv_conv_plan): the classes of z-lengths 1 .. t_max for cfg — two lengths
 * share a class iff every conv of the decoder, planned for one utterance of that length, takes the narrow kernel
 * or not alike.  Classes are intervals; first[i] = the first length of class i (first[0] = 1), at most `capacity`
 * are written.  Returns the number of classes, -1 on a bad argument.  splitk != 0: one class (no bitwise claim).
 *
 * mbv_ragged_plan (host only): the decoder runs a ragged call makes for B rows of the given HOST lengths — one per
 * non-empty class, cut further only where a run's largest tensor would reach 2 GiB (as a stand-alone decode's
 * may not either) or 65535 rows.  run_of_row [B] (or NULL) receives the run of every row, -1 for a row of length 0.
 * Returns the number of runs, -1 on a bad argument (a length outside [0, t_frames] included).
 *
 * mbv_decode_ragged: z DEVICE [B, 192, t_frames], g DEVICE [B, gin] or NULL, lengths_host HOST int64 [B] (the
 * class of a row decides its launches, so the lengths are needed on the host; nothing is copied or synchronised),
 * o DEVICE [B, 256 t_frames], written whole.  A row of length 0 is all zeros.  With "splitk": within fp32 rounding
 * of the stand-alone decode (the split factor depends on the launch size), bitwise run to run.  Refused with a
 * message, launching nothing: a length outside [0, t_frames], the options "trim" or "conv_bf16" set.
 *
 * mbv_synthesize_ragged: mbv_synthesize with the decoder in this mode; y_lengths_host HOST int64 [B] = the
 * y_lengths mbv_encode wrote, read back by the caller in its one host sync (lengths above max_len are cut to it).
 * outs->o_mb / spec / phase must be NULL (refused otherwise). */
int mbv_ragged_classes(const mbv_config *cfg, int splitk, int t_max, int32_t *first, int capacity);
int mbv_ragged_plan(const mbv_config *cfg, int splitk, int B, int t_frames, const int64_t *lengths, int32_t *run_of_row);
int mbv_decode_ragged(mbv_model *m, const float *z, const float *g, int B, int t_frames, const int64_t *lengths_host,
                      float *o, void *stream);
int mbv_synthesize_ragged(mbv_model *m, int t_frames, const float *noise, float noise_scale, int max_len,
                          const mbv_outputs *outs, const int64_t *y_lengths_host, void *stream);

/* ---- pooled streaming decode: the next chunk of many concurrent streams in shared launches (no reference
 * counterpart: the reference service decodes one request at a time) ----------------
 * One call takes n chunks, each the z-frames [first, first + count) of its OWN utterance (own z, g, length and
 * waveform row), and makes one decoder run per class of the utterances' lengths (mbv_ragged_classes) instead of one
 * mbv_decode_range per chunk.  A run's rows are the chunks' z-windows [max(0, first - L), min(t_frames, first +
 * count + R)), gathered into scratch and decoded as rows of the ragged decode of their window lengths, while every
 * conv is planned as for the whole utterances (of one class: alike).  Each stored sample is BITWISE what
 * mbv_decode_range, and so mbv_decode on the whole z, gives for that utterance alone (default mode; with "splitk"
 * within fp32 rounding, bitwise run to run).  Only samples [256 first, 256 (first + count)) of each o are written,
 * and no z-frame outside a chunk's window is read.  Two chunks of one call may belong to one utterance when their
 * sample ranges are disjoint.
 *
 * mbv_chunks_plan (host only): the decoder runs a call makes for chunks of utterances of t_frames[i] z-frames — one
 * per non-empty class, cut further exactly where mbv_ragged_plan cuts rows of those lengths (a 2 GiB tensor, 65535
 * rows).  run_of_chunk [n] (or NULL) receives the run of every chunk.  Returns the number of runs, -1 on a bad
 * argument (a t_frames < 1 included).
 *
 * mbv_decode_chunks: chunks_host HOST [n]; its values travel to the device as kernel arguments, so the array may be
 * freed when the call returns; nothing is copied from caller memory and nothing is synchronised.  Refused with a
 * message, launching nothing and leaving the handle usable: a range outside its utterance, an o that is not
 * 16-byte aligned, a z_stride < t_frames, g given for some chunks and not for others (a model with gin_channels),
 * the options "trim" or "conv_bf16" set.
 *
 * mbv_decoder_runs: decoder runs (passes through the decoder's conv chain) made on this handle since mbv_create,
 * by any entry; the difference across a call is what that call cost in launch chains. */
typedef struct mbv_chunk {
  const float *z;        /* DEVICE, one utterance: [192, t_frames] at row stride z_stride (in floats) */
  int64_t z_stride;
  const float *g;        /* DEVICE [gin] or NULL */
  int32_t t_frames;      /* the utterance's whole length: decides the class */
  int32_t first, count;  /* z-frames [first, first + count) */
  float *o;              /* DEVICE, the utterance's waveform row (>= 256 t_frames floats, 16-byte aligned); only
                            samples [256 first, 256 (first + count)) are written */
} mbv_chunk;
int mbv_chunks_plan(const mbv_config *cfg, int splitk, int n, const int32_t *t_frames, int32_t *run_of_chunk);
int mbv_decode_chunks(mbv_model *m, const mbv_chunk *chunks_host, int n, void *stream);
/* mbv_decode_chunks with the length that decides a chunk's class given apart from t_frames: route_frames HOST [n] (or
 * NULL = mbv_decode_chunks), entry i 0 = t_frames, else >= t_frames (a smaller value is refused).  For an utterance
 * that is still growing (live conversion below): t_frames = the z-frames that are final now, which clips the window,
 * and route_frames = a length of the class the finished utterance is to be decoded in.  Chunks share a run iff
 * mbv_chunks_plan puts their route lengths into one run, so rows whose routes differ never share a launch. */
int mbv_decode_chunks_routed(mbv_model *m, const mbv_chunk *chunks_host, const int32_t *route_frames, int n,
                             void *stream);
int64_t mbv_decoder_runs(mbv_model *m);

/* ---- "tail_once" (default 1; mbv_set_option("tail_once", 0) turns it off, 2 applies it at every size) -----------
 * The decoder gets z * y_mask: behind the reach of row b's valid frames every activation is the zero-input response,
 * the same in every row of a padded batch.  With the option on, the ResBlock convs of every row but the shortest
 * (the donor) leave out the column tiles that lie wholly in that tail, and a copy kernel writes the donor's values
 * there: every output and stage tensor is bitwise what it is with the option off.  Inert for B = 1, without
 * y_lengths (mbv_decode), with "splitk", "trim", "conv_bf16", the ranged / ragged / pooled decodes and per-row
 * speaker conditioning in the decoder (gin_channels > 0 with g given).
 * A stage whose rows are at most 8 column tiles long takes the packed route instead (MBV_ROUTE_TAIL_PACK): every
 * row keeps its columns below rate * len_b + reach rounded up to 32, the rows' kept columns are laid end to end and
 * share the tiles, and the copy kernel writes the rest.  The same bits again.
 *
 * mbv_tail_plan (host only, like mbv_conv_plan): one row of 6 ints per launch of the decoder, in launch order:
 * kind (0 conv_pre, 1 ups[stage], 2 / 3 first / second conv of step q of ResBlock j, 4 conv_post, 5 the waveform
 * tail), stage, j, q, rate (output columns per z-frame), reach (output columns past rate * len - 1 that a valid
 * z-frame of a row of len frames can influence; for a launch that writes the running ResBlock sum, the maximum over
 * the ResBlocks summed so far).  Row b's tail starts at column rate * len_b + reach.  At most `capacity` rows are
 * written; returns the number of launches, -1 on a bad argument.
 * mbv_tail_dropped: column tiles the tail maps left out on this handle since mbv_create (synchronises the device);
 * for a packed launch, the column tiles of the full grid that were not launched. */
int mbv_tail_plan(const mbv_config *cfg, int32_t *out, int capacity);
/* mbv_decode on z * sequence_mask(lengths): the decoder run mbv_synthesize makes, on a z of the caller's.
 * lengths: DEVICE int32 [B], frames per row; z at and past a row's length is read as zero. */
int mbv_decode_masked(mbv_model *m, const float *z, const float *g, const int32_t *lengths, int B, int t_frames,
                      const mbv_outputs *outs, void *stream);
int64_t mbv_tail_dropped(mbv_model *m);
/* The block table of a packed tail_once launch (MBV_ROUTE_TAIL_PACK), host only, no GPU: what the device builds for
 * lens (HOST [B], clamped to [0, T]), S_b = lens[b] * num + reach, a launch of T columns with halo (K - 1) * dil,
 * pad_right of it on the right, tiles of bn columns.  out: [0] column tiles, [1] donor, [2] 32-column blocks in use,
 * [3] 0, [4 .. 4 + B) the kept columns S_b' of every row, then from the next multiple of 4 one {row, first column,
 * read limit, 1 = output / 0 = gap or empty} per block.  Returns the ints written (out NULL: the ints needed),
 * -1 on a bad argument or a capacity too small. */
int mbv_tail_pack_table(const int64_t *lens, int B, int num, int reach, int T, int halo, int pad_right, int bn,
                        int32_t *out, int64_t capacity);

/* ---- pooled admission: the front half (text encoder, duration predictor, length regulation, flows) of many
 * requests in one padded run (no reference counterpart: the reference service runs one request at a time,
 * synthesis_module.py:141 taking the scales per request) ----------------
 * What mbv_encode / mbv_synthesize take as one value per call — length_scale, noise_scale_w, noise_scale, given
 * durations, max_len — comes per row, every row's noise is a block of the row's own shape, and each row's masked z,
 * cut to the frames it keeps, lands in a tensor of its own.  In the default mode every such z is BITWISE the z of
 * that utterance encoded and synthesised alone with the same noise (B = 1, T = its own length): the kernels in front
 * of the decoder work below each row's length in units that do not depend on the padding, and the table-reading
 * kernels run the scalar kernels' chains of operations.  With "splitk" (routes follow the launch size) the result is
 * deterministic and within fp32 rounding of the stand-alone call; a predicted duration may then differ by one frame.
 *
 * mbv_admit_plan (host only): which requests may share a run.  Two text lengths share a class iff every conv in front
 * of the flows, planned for either utterance alone, lands on the same side of the conv planner's one divide (today:
 * T <= 256 the narrow kernel, beyond it the tiled ones); a class is cut into further runs only where B rows padded to
 * the run's longest text would plan differently (2 GiB tensors) or exceed 65535 rows.  Runs are numbered in the order
 * of their first request; run_of_request [n] (or NULL) receives each request's run.  "splitk": one class.  Returns
 * the number of runs, -1 on a bad argument (n < 1, a length < 1).
 *
 * mbv_encode_rows: mbv_encode for the B rows of one run, ids [B, T] zero-padded, lengths[b] = rows[b].t_text.  The
 * state the run leaves for its mbv_synthesize_rows is kept under `slot` (0 .. 63), so that several runs can be
 * encoded, their lengths read back and their noise drawn before any is synthesised.  Slot 0 and the plain mbv_encode
 * are ONE state in one scratch: either call replaces what the other left, and the `_rows` entries take slot 0 only
 * while it holds an mbv_encode_rows run.  Whatever lays out a run's scratch ends the run: the next mbv_encode_rows on
 * its slot, and for slot 0 also mbv_encode and mbv_align; slots 1 .. 63 have a buffer each that no other entry
 * touches.  A `_rows` entry on an ended run is refused before any launch ("without a preceding mbv_encode_rows on
 * slot k").  The plain entries act on the run encoded or synthesised last, by either form.
 * rows_host is HOST memory and travels as kernel arguments (free it on return).  Rows with
 * durations have them set as mbv_set_durations does (same range rules, same -1 marker); the others keep the predicted
 * ones.  y_lengths_out as in mbv_encode: -1 flags a row (token id / sid / duration), read it before synthesising.
 * Refused before any launch: t_text outside [1, T], noise_w missing on a model with the stochastic duration
 * predictor, durations together with length_scale != 1, the option "conv_bf16" (there the flows' route follows the
 * launch size), rows that mbv_admit_plan would not put into one run.
 *
 * mbv_synthesize_rows: length regulation + reverse flows of the run under `slot` (n = its B rows), t_frames >= every
 * row's y_length, then ONE scatter launch: rows[b].z [inter, keep] = (z * y_mask)[b, :, :keep].  No decoder: the
 * per-request z feed mbv_decode_chunks.  Refused before any launch: keep outside [1, t_frames], a noise_stride outside
 * [1, t_frames] where noise_scale != 0, "conv_bf16", a run the fused WN layers do not take (option "wn_fused" off, or
 * B * hidden * t_frames * 4 bytes >= 4 GiB).
 *
 * mbv_encoder_runs: passes through the text encoder made on this handle since mbv_create, by any entry. */
typedef struct mbv_enc_row {
  float length_scale, noise_scale_w;
  const float *noise_w;          /* DEVICE [2, t_text], this row's own draw; NULL without the stochastic predictor */
  const void *durations;         /* DEVICE [t_text] given frames per token, or NULL: the predicted ones */
  int32_t durations_dtype;       /* 0 int32, 1 int64, 2 fp32 (as mbv_set_durations) */
  int32_t t_text;                /* the row's text length = lengths[b] */
} mbv_enc_row;
typedef struct mbv_row {
  const float *noise;            /* DEVICE [inter, noise_stride], this row's own prior draw (not read at noise_scale 0) */
  int64_t noise_stride;          /* its row stride in floats: the row's y_length */
  float noise_scale;
  int32_t keep;                  /* frames of z kept: min(y_length, max_len) */
  float *z;                      /* DEVICE [inter, keep], the request's own tensor */
} mbv_row;
int mbv_admit_plan(const mbv_config *cfg, int splitk, int n, const int32_t *t_text, int32_t *run_of_request);
int mbv_encode_rows(mbv_model *m, int slot, const int64_t *ids, const int64_t *lengths, const int64_t *sid, int B, int T,
                    const mbv_enc_row *rows_host, int64_t *y_lengths_out, void *stream);
int mbv_synthesize_rows(mbv_model *m, int slot, int t_frames, const mbv_row *rows_host, int n, void *stream);
int64_t mbv_encoder_runs(mbv_model *m);

/* speaker embedding lookup: replaces `net.emb_g(sid)` (models.py:705).
 * out fp32 [B, gin] */
int mbv_speaker_embedding(mbv_model *m, const int64_t *sid, int B, float *out, void *stream);

/* ---- blended voices: virtual speakers behind the embedding table (no reference counterpart) -------------------------
 * A voice is defined once into slot j and is from then on the speaker id n_speakers + j wherever a speaker id is taken
 * (host ints and device int64 tensors alike, mixed with plain ids at will); an id >= n_speakers whose slot is not
 * defined is refused or flagged exactly like any other id outside the table.  The model consumes a speaker only as its
 * row g [gin]; a voice's row is
 *   a blend   acc = weights[0] * emb_g[ids[0]][c], then acc = fmaf(weights[k], emb_g[ids[k]][c], acc) for
 *             k = 1 .. count - 1 in that order, all fp32: this order is part of the contract, so a one-hot blend is
 *             bitwise the table row; ids name real speakers only (0 <= id < n_speakers, no blends of blends); or
 *   a vector  the gin floats at `vector` (DEVICE), copied in stream order: a row made elsewhere.
 * Rows live in a buffer of the model outside the weight arena: mbv_export_arena / mbv_import_arena do not carry them.
 * After mbv_finalize_weights or mbv_import_arena every blend is recomputed from the new table in one launch; a vector
 * voice stays as given.  MBV_SPEAKER_SLOTS and MBV_BLEND_MAX are conventions of this build, not properties of the
 * model: a slot costs one row of gin floats, a term one id and one weight.
 *
 * mbv_speakers_define   n definitions (HOST array) in ONE blend launch.  Checked on the host, and refused before
 *                       anything is launched, the message naming the definition: n outside [1, MBV_SPEAKER_SLOTS], a
 *                       slot outside [0, MBV_SPEAKER_SLOTS) or named twice, count outside [1, MBV_BLEND_MAX] (with
 *                       vector == NULL), an id outside [0, n_speakers), a weight that is not finite; a model without a
 *                       speaker table.  A defined slot may be defined again: the new row replaces the old one in
 *                       stream order.  No synchronisation after the first call (which allocates the buffers).
 * mbv_speaker_release   the slot is undefined again (host at once, device in stream order); refuses a slot outside the
 *                       range or not defined.
 * mbv_speaker_slots     MBV_SPEAKER_SLOTS of the library.
 * mbv_speaker_defined   1: sid >= n_speakers names a defined voice; 0: it does not (real speakers included); -1: m NULL.
 * mbv_speaker_runs      blend launches since mbv_create (one per mbv_speakers_define, one per weight refresh with a
 *                       blend defined); -1: m NULL. */
#define MBV_SPEAKER_SLOTS 256
#define MBV_BLEND_MAX 16
typedef struct mbv_speaker_def {
  int32_t slot;
  int32_t count;                 /* terms of the blend; ignored with `vector` */
  int32_t ids[MBV_BLEND_MAX];
  float weights[MBV_BLEND_MAX];
  const float *vector;           /* DEVICE [gin] or NULL */
} mbv_speaker_def;
int mbv_speakers_define(mbv_model *m, const mbv_speaker_def *defs, int n, void *stream);
int mbv_speaker_release(mbv_model *m, int slot, void *stream);
int mbv_speaker_slots(void);
int mbv_speaker_defined(mbv_model *m, int64_t sid);
int64_t mbv_speaker_runs(mbv_model *m);

/* ---- run-time options (no reference counterpart) ------------------------------
 *   "splitk"       1: split the input-channel loop of conv launches that leave most of the chip
 *                  idle over several workgroups (single-utterance latency: ljs_mb batch 1
 *                  10.3 -> 6.5 ms).  Deterministic, within fp32 rounding of the default; a row is
 *                  then no longer bitwise independent of the batch it is computed in.  Default 0
 *                  (or the MBV_CONV_SPLITK environment variable at mbv_create time).
 *   "istft_exact"  1: libm transcendentals in the fused iSTFT kernel (default 0 / MBV_ISTFT_EXACT).
 *   "xpost_chunk_bytes"  the fused iSTFT kernels address their input with 32-bit byte offsets, so a
 *                  batch whose x_post ([B, 72, F] fp32) would reach 2 GiB runs subband_conv_post +
 *                  iSTFT in sub-batches (same T', bitwise the unsplit result).  This option lowers
 *                  the cap (bytes; 0 = 2 GiB - 1) — tests use it to take the split path at small sizes.
 *   "dec_streams"  1 (default; MBV_DEC_STREAMS): when one ResBlock conv of a decoder stage cannot fill the
 *                  chip (single utterances, small batches) the stage's three ResBlocks (models.py:353-359)
 *                  run on three internal streams forked from / joined to `stream`; bitwise the result of
 *                  the one-stream schedule (0).  With "tail_once" at work also at any batch size.
 *   "tail_once"    1 (default): the zero-input tail of a padded batch is computed for the shortest row only and
 *                  copied to the others (see mbv_tail_plan), in the decoder stages whose ResBlock convs exceed one
 *                  round of the 256-workgroup grid (smaller launches have no round to save).  2: in every stage
 *                  (tests).  0: off.  Every output and stage tensor is bitwise the same for all three values.
 *   "trim"         0 (default).  1: OPT-IN trimmed decode for ragged batches whose caller takes only the waveform
 *                  and cuts it by y_lengths (tts_vits.py:134-137 takes [0][0,0] of one utterance): in mbv_synthesize
 *                  the decoder computes, per utterance, only the tiles that hold frames below y_lengths[b] + 32
 *                  (its one-sided receptive field is 25 z-frames) and the fused iSTFT stops at 256 y_lengths[b]
 *                  samples.  Valid samples are bitwise those of the default; the padded region of `o` — defined
 *                  output of the reference, computed by the default — is left as the caller allocated it
 *                  (the Python shim zero-fills it).  Requires o_mb / spec / phase NULL; multiband / multistream
 *                  decoders, not the low-latency mode.  Never the headline configuration.
 *   "conv_bf16"    0 (default; MBV_CONV_BF16): every contraction in exact fp32.  3: OPT-IN split-bf16
 *                  arithmetic in the large conv launches (the decoder's ResBlock convs of a batch): each
 *                  fp32 operand is split into bf16(x) and bf16(x - bf16(x)), the three leading products
 *                  are accumulated in fp32 on the bf16 matrix instruction.  Not IEEE fp32 multiplication
 *                  (relative error of a product ~2^-16): ~1.9x faster decoder stage, waveform within 3e-6
 *                  RMS of the exact mode at batch 64 (bar 1e-4).  Any other value is refused. */
int mbv_set_option(mbv_model *m, const char *name, int value);
/* the current value of an integer option ("xpost_chunk_bytes" excepted), -1 for an unknown name */
int mbv_get_option(mbv_model *m, const char *name);

/* ---- stage timers -----------------------------------------------------------
 * replaces the `timings` dict (models.py:698-737): milliseconds of the five
 * stages of the last encode+synthesize pair, from HIP events on `stream`:
 * [text_encoder, duration_predictor, alignment_and_projection, flow,
 * waveform_decoder].  Synchronises on the recorded events. */
int mbv_stage_times_ms(mbv_model *m, float out[5]);
/* The same for an earlier call of this handle: mbv_ticket() after mbv_encode names the call (1, 2, ...); the stage
 * events of the last 8 calls are kept, so a caller that reads its timings late (the reference's `timings` dict is
 * often never read) still gets them after newer calls have started.  Fails for a call older than that. */
int64_t mbv_ticket(mbv_model *m);
int mbv_stage_times_ms_at(mbv_model *m, int64_t ticket, float out[5]);

/* Kernel-level timers of the last mbv_synthesize / mbv_decode (HIP events on the
 * launch stream, used by bench.py for the roofline lines):
 *   out[0] = decoder conv stack (conv_pre .. subband_conv_post), ms
 *   out[1] = the single fused iSTFT+PQMF launch, ms
 * Synchronises on the recorded events. */
int mbv_kernel_times_ms(mbv_model *m, float out[2]);

/* ---- stand-alone signal stage ------------------------------------------------
 * The fused iSTFT + PQMF kernel on its own: replaces TorchSTFT.inverse
 * (stft.py:197-202) + PQMF.synthesis (pqmf.py:105-116) or the MS tail
 * (models.py:463-465), including exp / pi*sin of models.py:368-369.
 *   x_post  fp32 [B, 72, F]  F = 16 T' + 1 (output of subband_conv_post)
 *   filter  fp32 [4, 63] device synthesis filter, NULL = the PQMF design
 *   multistream  bit 0: o_mb is the zero-stuffed [B,4,256T'] tensor (MS decoder);
 *                bit 1: x_post is in the library's internal units (log-magnitude rows times
 *                log2 e, phase rows divided by 2 pi), as the decoder stack produces it
 * Does not need a model handle's weights; `m` provides device + scratch. */
int mbv_istft_pqmf(mbv_model *m, const float *x_post, int B, int t_frames, const float *filter,
                   int multistream, float *o, float *o_mb, float *spec, float *phase,
                   void *stream);

/* ---- voice conversion -------------------------------------------------------------
 * replaces SynthesizerTrn.voice_conversion (models.py:790-798): posterior encoder on the source
 * spectrogram, forward flow with the source speaker, reverse flow + decoder with the target.
 *   y          fp32 [B, spec_channels, T] linear spectrogram     y_lengths int64 [B]
 *   sid_src, sid_tgt  int64 [B]
 *   noise      fp32 [B, 192, T] standard-normal draws of PosteriorEncoder (models.py:245), or
 *              NULL for the deterministic z = m_q
 *   outs       o, o_mb, spec, phase as in mbv_decode (T' = T); y_mask [B,1,T];
 *              z -> z (posterior sample), z_p -> z_p (source-normalised), m_p -> z_hat
 *   status     int32 [B] device, optional: non-zero where y_lengths / sid were out of range */
int mbv_voice_conversion(mbv_model *m, const float *y, const int64_t *y_lengths,
                         const int64_t *sid_src, const int64_t *sid_tgt, int B, int T,
                         const float *noise, const mbv_outputs *outs, int32_t *status, void *stream);

/* ---- forced alignment ---------------------------------------------------------------
 * The alignment of SynthesizerTrn.forward (models.py:659-680, :690-691) for utterances whose audio and text both
 * exist: enc_p, enc_q, the forward flow, the negative cross-entropy matrix, Monotonic Alignment Search
 * (monotonic_align/core.pyx) and the expanded prior.  The text encoder runs exact, as in mbv_encode.  No host
 * synchronisation.  The call uses the scratch of mbv_encode: an mbv_synthesize needs a fresh mbv_encode after it.
 *   ids, lengths   int64 [B, T_text] / [B]                  y, y_lengths  fp32 [B, spec_channels, T_spec] / int64 [B]
 *   sid            int64 [B]; NULL iff n_speakers == 0
 *   noise          fp32 [B, inter, T_spec] draws of PosteriorEncoder (models.py:245); z = m_q + noise * noise_scale *
 *                  exp(logs_q); NULL or noise_scale == 0: z = m_q
 *   outs           every member optional (NULL: not wanted, its stores never happen)
 *   status         int32 [B] device, optional: bit 0 a token id / length / sid outside its table or tensor,
 *                  bit 1 more tokens than frames (t_x > t_y: no monotone path), bit 2 an empty text or recording.
 *                  A flagged row has w = 0; nothing faults. */
typedef struct mbv_align_outputs {
  int32_t *w;        /* [B, T_text]            frames per token (attn.sum(2), models.py:680); 0 behind the text */
  float *attn;       /* [B, 1, T_spec, T_text] the path */
  float *x_mask;     /* [B, 1, T_text] */
  float *y_mask;     /* [B, 1, T_spec] */
  float *z;          /* [B, inter, T_spec]     posterior sample */
  float *z_p;        /* [B, inter, T_spec]     flow(z) */
  float *m_p;        /* [B, inter, T_spec]     text statistics expanded by the path (models.py:690-691) */
  float *logs_p;     /* [B, inter, T_spec] */
  float *neg_cent;   /* [B, T_spec, T_text]    cells [y < y_lengths[b], x < lengths[b]) only; the rest is not written */
} mbv_align_outputs;
int mbv_align(mbv_model *m, const int64_t *ids, const int64_t *lengths, const float *y, const int64_t *y_lengths,
              const int64_t *sid, int B, int T_text, int T_spec, const float *noise, float noise_scale,
              const mbv_align_outputs *outs, int32_t *status, void *stream);

/* Synthesis with given durations: valid after mbv_encode, before mbv_synthesize.  Replaces the predicted durations
 * (w_ceil, their cumulated sums, the frame counts) by those of w, masked by the text lengths, with
 * y_lengths = max(sum w, 1) (models.py:717-719); mbv_synthesize then proceeds unchanged.  Without the call nothing
 * changes.
 *   w              [B, T] non-negative integers: dtype 0 int32, 1 int64, 2 fp32
 *   y_lengths_out  int64 [B] device; -1 under the rules of mbv_encode (whose flags are kept), and for a negative or
 *                  non-integer duration */
int mbv_set_durations(mbv_model *m, const void *w, int dtype, int B, int T, int64_t *y_lengths_out, void *stream);

/* ---- spectrogram -> waveform ("istft_finalize") -------------------------------
 * The last step of the reference's chunked decoding (inferz_test.ipynb cells 6-7,
 * `istft_finalize`; intent of synthesis_module.py:306-353): chunks of z go through
 * mbv_decode, the caller cross-fades the returned (spec, phase) along time, and this
 * entry turns the stitched spectrogram into audio with the MODEL's synthesis bank
 * (PQMF / trained multistream filter / none for the single-band decoder).
 *   spec, phase  fp32 [B, 4, 9, F] (single band: [B, 9, F]), phase in radians
 *   frames       F; must be 16 n + 1 for mb / ms (F - 1 sub-band hops = whole z-frames)
 *   o            fp32 [B, 1, 16 (F - 1)]  (single band: [B, 1, 4 (F - 1)])
 *   o_mb         optional, as in mbv_outputs */
int mbv_istft_finalize(mbv_model *m, const float *spec, const float *phase, int B, int frames,
                       float *o, float *o_mb, void *stream);

/* ---- wire-format epilogue -----------------------------------------------------
 * replaces the NumPy post-processing of the service wrapper (tts_vits.py:204-217):
 * per-utterance peak normalisation to 0.9 (if auto_normalize and peak > 0.01), clip to
 * [-1, 1], * 32767, truncation to int16.  Bit-exact with the reference's fp32 NumPy.
 *   wave        fp32 [B, 1, stride] device
 *   y_lengths   int64 [B] device frames per utterance (valid samples = 256 * y_lengths),
 *               or NULL = every row is `stride` valid samples
 *   pcm         int16 [B, stride] device; samples past the valid length are 0 */
int mbv_pcm16(mbv_model *m, const float *wave, const int64_t *y_lengths, int B, int64_t stride,
              int auto_normalize, int16_t *pcm, void *stream);

/* The same with the valid length of every row given in samples rather than frames, for rows that are no
 * longer 256 samples per frame (the output of mbv_resample):
 *   valid_samples  int64 [B] device (clamped to [0, stride]; the out_samples of mbv_resample), or NULL */
int mbv_pcm16_samples(mbv_model *m, const float *wave, const int64_t *valid_samples, int B, int64_t stride,
                      int auto_normalize, int16_t *pcm, void *stream);

/* ---- resampling -----------------------------------------------------------------
 * replaces librosa.resample(audio, orig_sr=model_sr, target_sr=rate) of the service wrapper
 * (tts_vits.py:199-200), librosa 0.9.2 (requirements_py39.txt:2): res_type "kaiser_best" (its default) or
 * "kaiser_fast", i.e. resampy's windowed-sinc interpolator followed by fix_length to ceil(n * target / orig)
 * samples.  Computed as a polyphase FIR (target / orig = L / M in lowest terms, L phases of K fp32 taps)
 * whose bank restates resampy's float64 table arithmetic and is rounded to fp32 once; parity is pinned to
 * that restatement (tests/resample_ref.py), not to the library.  Every row is resampled as if alone
 * (zeros outside [0, valid)).  Refused: L > 4096 phases, K > 4096 taps, or an input window per 256 outputs
 * beyond 64 KiB of LDS (downsampling by more than about 60x).
 *   wave           fp32 [B, 1, in_stride] device
 *   valid_samples  int64 [B] device, clamped to [0, in_stride]; NULL = every row is in_stride samples
 *   filter         MBV_RESAMPLE_KAISER_BEST / MBV_RESAMPLE_KAISER_FAST
 *   out            fp32 [B, 1, out_stride] device; row b holds int(n_b * ratio) resampled samples
 *                  (ratio = (double)target_sr / orig_sr, n_b its valid input samples), zeros after them
 *   out_samples    int64 [B] device, optional: min(ceil(n_b * ratio), out_stride) computed in fp64 as
 *                  librosa does, the length of the row after fix_length.  out_stride =
 *                  ceil(in_stride * ratio) holds every row.
 * The first call for a rate pair and filter builds the bank on the host and uploads it with a synchronous
 * copy (cached in the handle); later calls only enqueue one kernel.  Needs no weights. */
#define MBV_RESAMPLE_KAISER_BEST 0   /* num_zeros 64, precision 9, Kaiser beta 14.769656459379492, rolloff 0.9475937167399596 */
#define MBV_RESAMPLE_KAISER_FAST 1   /* num_zeros 16, precision 9, Kaiser beta 8.555504641634386, rolloff 0.85 */
int mbv_resample(mbv_model *m, const float *wave, const int64_t *valid_samples, int B, int64_t in_stride,
                 int orig_sr, int target_sr, int filter, float *out, int64_t out_stride, int64_t *out_samples,
                 void *stream);
/* Host only (no handle, no GPU): the fp32 bank mbv_resample uses for a rate pair, [phases + 1][taps]
 * row-major, phases = L = target / gcd(orig, target), M = orig / gcd.  Row r < L weighs x[floor(t * M / L)
 * - left + k] (tap k) for every output t with (t * M) mod L == r; row L (fraction 1) weighs
 * x[t * M / L - 1 - left + k] instead of row 0 for the outputs t > 0 whose fp64 time t / ratio rounds
 * below the integer t * M / L (resampy then interpolates from the sample before).
 * dst == NULL only queries phases / taps / left (any of them may be NULL).  On failure the message is
 * available from mbv_last_error(NULL). */
int mbv_resample_bank(int orig_sr, int target_sr, int filter, float *dst, int64_t capacity, int32_t *phases,
                      int32_t *taps, int32_t *left);

/* ---- streamed wire output -------------------------------------------------------
 * replaces the resample / normalise / int16 steps of the service wrapper (tts_vits.py:196-217) for a waveform
 * that is still being decoded (mbv_decode_range): one step turns the samples that have become final into int16,
 * and the concatenation of all steps is bitwise mbv_resample + mbv_pcm16_samples on the finished waveform.
 *
 * mbv_resample_ready (host only: no handle, no GPU): how many outputs of a row of in_total input samples are
 * final once its samples [0, in_avail) exist.  With target / orig = L / M in lowest terms and the (taps K, left)
 * of mbv_resample_bank, output t reads x[floor(t M / L) - left - (row L ? 1 : 0) + k], k < K, hence
 *   in_avail <  in_total:  max(0, ceil((in_avail - K + left + 1) L / M))
 *   in_avail >= in_total:  ceil(in_total * ratio) in fp64, the out_stride that holds every row of mbv_resample
 * so no counted output has a tap (a padded zero tap included) at or past in_avail.  The stream lags the decoder
 * by K - left - 1 input samples: 64 (kaiser_best, upsampling), 88 (22050 -> 16000), 16 / 22 (kaiser_fast).
 * Equal rates: min(in_avail, in_total), no lag.  < 0 (message from mbv_last_error(NULL)) for a rate pair
 * mbv_resample refuses, an unknown filter or in_total < 0.
 *
 * mbv_resample_pcm16_range: one launch for outputs [out_first, out_first + out_count) of every row.
 *   wave, valid_samples, B, in_stride, orig_sr, target_sr, filter   as mbv_resample; in_stride is in_total
 *   in_avail       input samples [0, in_avail) of every row exist; nothing at or past it is read
 *   out_first, out_count   must end at or below min(mbv_resample_ready(.., in_avail, in_stride), pcm_stride)
 *   peak           fp32 [B] device or NULL.  NULL: no normalisation (auto_normalize = 0 of mbv_pcm16).  Else
 *                  v = (v / peak[b]) * 0.9 where peak[b] > 0.01, the operations of mbv_pcm16 in its order: fed
 *                  the peak of the whole resampled row the stream is bitwise auto_normalize = 1
 *   pcm            int16 [B, pcm_stride] device; only the range is written.  Samples at or past
 *                  int(n_b * ratio) are 0, as mbv_resample + mbv_pcm16_samples leave them
 *   running_peak   fp32 [B] device or NULL, owned and zeroed by the caller before the first step: raised to the
 *                  largest |sample| of the row's resampled outputs in the range (an atomic max on the bits of the
 *                  non-negative floats).  After the last step it is bitwise the peak mbv_pcm16_samples would have
 *                  normalised by
 *   out_samples    int64 [B] device or NULL: min(ceil(n_b * ratio), pcm_stride), as mbv_resample writes it
 * Equal rates skip the FIR (a ranged mbv_pcm16_samples with a given peak).  All per-stream state is in the
 * caller's buffers; the handle only caches the filter bank (first call for a rate pair: synchronous upload, as
 * mbv_resample).  Argument errors, a range beyond what in_avail makes final included, return non-zero with a
 * message, launch nothing and leave the handle usable. */
int64_t mbv_resample_ready(int orig_sr, int target_sr, int filter, int64_t in_avail, int64_t in_total);
int mbv_resample_pcm16_range(mbv_model *m, const float *wave, const int64_t *valid_samples, int B, int64_t in_stride,
                             int orig_sr, int target_sr, int filter, int64_t in_avail, int64_t out_first,
                             int64_t out_count, const float *peak, int16_t *pcm, int64_t pcm_stride,
                             float *running_peak, int64_t *out_samples, void *stream);

/* ---- pooled wire output: the ranged step of many concurrent streams in ONE launch (no reference counterpart: the
 * reference service handles one request at a time) ----------------
 * One call takes n chunks, each the outputs [out_first, out_first + out_count) of its OWN stream (own wave row,
 * length, frontier, peak and pcm row), and makes one resample / int16 launch for all of them instead of one
 * mbv_resample_pcm16_range per stream.  Every stored int16, running peak and out_samples is BITWISE what
 * mbv_resample_pcm16_range gives for that row alone: an output is computed by the same device code from the same
 * staged input, whichever tile of whichever launch holds it, and a max does not depend on order.  The fields of a
 * chunk are the arguments of mbv_resample_pcm16_range for one row (B = 1, in_stride = in_total, pcm_stride =
 * pcm_capacity); peak may be given for some chunks and not for others.  Two chunks of one call may belong to one
 * stream when their output ranges are disjoint (they may share running_peak and out_samples).
 *
 * mbv_pcm_chunks_plan (host only: no handle, no GPU; reads the integer fields only): checks every chunk as
 * mbv_resample_pcm16_range checks its row — out_first >= 0, out_count >= 0 (in_avail >= 0, in_total > 0,
 * pcm_capacity > 0) and out_first + out_count <= min(mbv_resample_ready(.., in_avail, in_total), pcm_capacity) —
 * and fills packed_first[i] (or NULL) with the running sum of the out_count in chunk order: where chunk i starts
 * in the packed buffer.  Returns the packed total (0 for n = 0), or -1 with a message that names the offending
 * chunk ("chunk i: ...", mbv_last_error(NULL)); also -1 for an unknown filter or a rate pair mbv_resample refuses.
 *
 * mbv_resample_pcm16_chunks: chunks_host HOST [n]; its values travel to the device as kernel arguments (written
 * to the handle's scratch by a one-workgroup kernel), so the array may be freed when the call returns; nothing is
 * copied from caller memory and nothing is synchronised (beyond the first call for a rate pair, as mbv_resample).
 *   packed, packed_capacity   int16 DEVICE or NULL: chunk i's samples are ALSO stored at packed[packed_first[i] ..),
 *                             back to back in chunk order, so one copy takes the whole call to the host
 * One rate pair and filter per call.  Refused with a message, launching nothing and leaving the handle usable:
 * whatever the plan refuses, a missing wave or pcm, a packed_capacity below the packed total, two chunks that
 * write overlapping ranges of one pcm.  A call whose chunks are all empty and carry no out_samples launches nothing.
 *
 * mbv_wire_runs: launches of the resample / int16 kernels made by mbv_resample_pcm16_range and
 * mbv_resample_pcm16_chunks on this handle since mbv_create (table writers are not counted): the counterpart of
 * mbv_decoder_runs for the wire step. */
typedef struct mbv_pcm_chunk {
  const float *wave; int64_t in_total;      /* DEVICE, one row */
  const int64_t *valid_samples;             /* DEVICE, one int64, or NULL */
  int64_t in_avail, out_first, out_count;
  const float *peak;                        /* DEVICE, one float, or NULL (per chunk: mixed is allowed) */
  int16_t *pcm; int64_t pcm_capacity;       /* the stream's own full-length row (mbv_resample_g711_chunks: bytes) */
  float *running_peak; int64_t *out_samples;/* DEVICE, one value each, or NULL */
} mbv_pcm_chunk;
int64_t mbv_pcm_chunks_plan(int orig_sr, int target_sr, int filter, const mbv_pcm_chunk *chunks, int n,
                            int64_t *packed_first);
int mbv_resample_pcm16_chunks(mbv_model *m, const mbv_pcm_chunk *chunks_host, int n, int orig_sr, int target_sr,
                              int filter, int16_t *packed, int64_t packed_capacity, void *stream);
int64_t mbv_wire_runs(mbv_model *m);

/* ---- look-ahead limiter on the wire step (no reference counterpart: the service normalises a finished utterance
 * by its own peak, tts_vits.py:204-213, which a stream does not have) -------------------------------------------
 * A causal level control with a bounded lag, fused into the ranged and the pooled wire step between the static
 * peak gain and the clip.  With v[t] the fp32 sample those steps clip ((v / peak) * 0.9 included where peak is
 * given; zero for t < 0 and at or past the row's computed outputs int(n * ratio)), all in fp32:
 *   r[t] = |v[t]| > c ? c / |v[t]| : 1
 *   m[j] = min r[k], k in [j - hold, j + lookahead]
 *   g[t] = (m[t - lookahead] + ... + m[t]) / (float)(lookahead + 1), added in ascending order from m[t - lookahead]
 *   y[t] = v[t] * g[t], then clip to [-1, 1], * 32767, truncate, as before
 * so |y| <= c up to rounding, the gain ramps down over `lookahead` outputs before a peak, holds for `hold` after it
 * and ramps back over `lookahead`; where nothing in reach exceeds c, g is exactly 1 and the int16 is bitwise the
 * unlimited one.  The step is stateless (every workgroup recomputes the v its outputs read), so an int16 is a pure
 * function of the finished waveform: it does not depend on how the stream was cut, pooled or pushed.
 *   ceiling in (0, 1], lookahead in [0, 255], hold in [0, 1024] (output samples); anything else is refused.
 *
 * mbv_limiter_ready (host only: no handle, no GPU): how many outputs are final under a limiter with that lookahead.
 * Output t reads v up to t + lookahead, so with R = mbv_resample_ready(.., in_avail, in_total) it is
 *   in_avail >= in_total >= 0:  R (everything: the last step flushes the lag)
 *   otherwise:                  max(0, R - lookahead); in_total < 0 is an OPEN recording, R = mbv_resample_ready_open
 * -1 with a message (mbv_last_error(NULL)) for whatever those two refuse or a lookahead outside [0, 255].
 *
 * mbv_resample_pcm16_range_limited: mbv_resample_pcm16_range with one limiter for all rows; the range must end at
 * or below min(mbv_limiter_ready(.., in_avail, in_stride, lookahead), pcm_stride).  running_peak keeps its meaning:
 * the largest |resampled sample| (before any gain) of the outputs emitted.
 *
 * mbv_resample_pcm16_chunks_limited: mbv_resample_pcm16_chunks with limits HOST [n] (or NULL = no row limited),
 * one per chunk; ceiling == 0 marks a chunk without a limiter, which is then exactly a chunk of
 * mbv_resample_pcm16_chunks.  The limited chunks of a call share ONE launch, whatever their parameters, and the
 * others share one: a mixed call costs two launches (mbv_wire_runs), a call of one kind one.  Each chunk is bitwise
 * its own ranged call.  Both entries refuse what their unlimited forms refuse, bad limiter parameters ("chunk i: ..."
 * in the pooled form), and a rate pair whose halo window does not fit the 64 KiB LDS stage, launching nothing. */
typedef struct mbv_pcm_limit {
  float ceiling;               /* c; 0 in a pooled call: this chunk has no limiter */
  int32_t lookahead, hold;     /* output samples */
} mbv_pcm_limit;
int64_t mbv_limiter_ready(int orig_sr, int target_sr, int filter, int64_t in_avail, int64_t in_total, int lookahead);
int mbv_resample_pcm16_range_limited(mbv_model *m, const float *wave, const int64_t *valid_samples, int B,
                                     int64_t in_stride, int orig_sr, int target_sr, int filter, int64_t in_avail,
                                     int64_t out_first, int64_t out_count, const float *peak, int16_t *pcm,
                                     int64_t pcm_stride, float *running_peak, int64_t *out_samples,
                                     const mbv_pcm_limit *limit, void *stream);
int mbv_resample_pcm16_chunks_limited(mbv_model *m, const mbv_pcm_chunk *chunks_host, const mbv_pcm_limit *limits_host,
                                      int n, int orig_sr, int target_sr, int filter, int16_t *packed,
                                      int64_t packed_capacity, void *stream);

/* ---- live input: recordings that are still arriving, resampled to the model's rate range by range ----------
 * The polyphase resampler puts zeros outside [0, n).  An output whose taps all lie below the samples that have
 * arrived therefore has the value it will have in the finished row, whatever n turns out to be; the total matters
 * only for the flush at close (the outputs whose taps reach past the end, and the zeros of fix_length) and for the
 * row's length.  mbv_resample_ranges computes fp32 outputs [out_first, out_first + out_count) of n recordings in
 * ONE launch, each from its own raw row (read in place, fp32 or int16 scaled by exactly 1 / 32768) into its own
 * model-rate row; only the range is written.  Every stored value is BITWISE what mbv_resample stores there for the
 * finished recording (int16: for pcm / 32768): same staged taps, same tap order, same four-accumulator sum.
 *
 * mbv_resample_ready_open (host only: no handle, no GPU): how many outputs are final once in_avail raw samples of an
 * OPEN recording exist: the open branch of mbv_resample_ready, which does not depend on the total.  Equal rates:
 * in_avail.  -1 with a message (mbv_last_error(NULL)) for an unknown filter or a rate pair mbv_resample refuses.
 * A closed row (in_total >= 0) is ready up to min(ceil(in_total * target / orig), out_capacity); a closed row's
 * outputs in [int(n ratio), ceil(n ratio)) are written as zeros, as mbv_resample writes them.
 *
 * rows_host is HOST memory [n]; its values travel to the device as kernel arguments (written to the handle's
 * scratch by a one-workgroup kernel), so the array may be freed when the call returns; nothing is copied from
 * caller memory and nothing is synchronised (beyond the first call for a rate pair, as mbv_resample).  Nothing at
 * or past in_avail is read from wave.  Refused with a message that names the row, launching nothing and leaving
 * the handle usable: a range that ends beyond what is ready, out_first + out_count > out_capacity, a negative field
 * (in_total below -1), in_total >= 0 with in_avail != in_total, a missing pointer, an unknown dtype or filter, a
 * rate pair mbv_resample refuses, equal rates (they take no kernel), two rows that write overlapping ranges of one
 * out, n < 0.  n == 0, or a call whose ranges are all empty, launches nothing and counts nothing.
 *
 * mbv_input_runs: launches of the live-input resampler on this handle since mbv_create (table writers are not
 * counted), the counterpart of mbv_wire_runs for the input side. */
typedef struct mbv_resample_range {
  const void *wave; int32_t wave_dtype;  /* DEVICE raw recording at orig_sr, MBV_WAVE_F32 / _PCM16 / _ULAW / _ALAW, read in place */
  int64_t in_avail;                      /* raw samples that exist */
  int64_t in_total;                      /* -1: open; >= 0: closed at that many samples (then in_avail == in_total) */
  int64_t out_first, out_count;          /* outputs [out_first, out_first + out_count) */
  float *out; int64_t out_capacity;      /* DEVICE, the recording's own model-rate row; only the range is written */
} mbv_resample_range;
int64_t mbv_resample_ready_open(int orig_sr, int target_sr, int filter, int64_t in_avail);
int mbv_resample_ranges(mbv_model *m, const mbv_resample_range *rows_host, int n, int orig_sr, int target_sr,
                        int filter, void *stream);
int64_t mbv_input_runs(mbv_model *m);

/* ---- G.711 on the wire: mu-law / A-law bytes out of the wire step and into the live input (no reference
 * counterpart: the reference service emits 16-bit linear PCM only) ------------------------------------------------
 * The codec is BITWISE CPython 3.10's audioop.lin2ulaw / lin2alaw / ulaw2lin / alaw2lin at width 2 (the arithmetic
 * of Sun's g711.c): mu-law works on s >> 2 clipped to 8159 with bias 33, A-law on s >> 3; encode(0) is 0xFF / 0xD5;
 * encode(decode(b)) == b for every byte but mu-law 0x7F (negative zero), which re-encodes to 0xFF.
 *
 * mbv_g711_encode / mbv_g711_decode: n samples, DEVICE int16 <-> DEVICE bytes, one launch (n == 0: none).
 *
 * mbv_resample_g711_range: mbv_resample_pcm16_range (limit NULL) or mbv_resample_pcm16_range_limited (limit given)
 * with the codec as the epilogue: out is uint8 [B, out_stride] and every byte written is encode(q) of the int16 q
 * that entry stores at the same index, the zeros of the padding included (0xFF / 0xD5).  running_peak, out_samples,
 * the readiness rules and every refusal are that entry's; out_stride counts bytes.
 *
 * mbv_resample_g711_chunks: mbv_resample_pcm16_chunks_limited (limits_host NULL: no chunk limited) likewise.  The
 * chunk's `pcm` then points to BYTES (cast the uint8_t pointer) and pcm_capacity counts bytes; packed receives bytes
 * and packed_capacity counts them; mbv_pcm_chunks_plan counts samples, which are the bytes.  One codec per call.  One
 * launch per kind (limited / unlimited) as there, counted by mbv_wire_runs with the int16 launches.
 *
 * A law other than MBV_G711_ULAW / MBV_G711_ALAW is refused before anything is launched, the handle stays usable.
 *
 * Input: a row of mbv_resample_ranges may hold G.711 bytes (wave_dtype MBV_WAVE_ULAW / MBV_WAVE_ALAW); it is staged
 * as (float)decode(byte) * (1 / 32768), exactly, so every output is bitwise that of the int16 row decode(bytes).
 * Only mbv_resample_ranges takes these two: telephone audio arrives at 8 kHz, no model runs at that rate, so it
 * always passes through the resampler; mbv_spectrogram, mbv_convert_rows and mbv_convert_ranges refuse them. */
#define MBV_G711_ULAW 1
#define MBV_G711_ALAW 2
int mbv_g711_encode(mbv_model *m, const int16_t *pcm, int64_t n, int law, uint8_t *out, void *stream);
int mbv_g711_decode(mbv_model *m, const uint8_t *in, int64_t n, int law, int16_t *pcm, void *stream);
int mbv_resample_g711_range(mbv_model *m, const float *wave, const int64_t *valid_samples, int B, int64_t in_stride,
                            int orig_sr, int target_sr, int filter, int64_t in_avail, int64_t out_first,
                            int64_t out_count, const float *peak, uint8_t *out, int64_t out_stride,
                            float *running_peak, int64_t *out_samples, const mbv_pcm_limit *limit, int law,
                            void *stream);
int mbv_resample_g711_chunks(mbv_model *m, const mbv_pcm_chunk *chunks_host, const mbv_pcm_limit *limits_host, int n,
                             int orig_sr, int target_sr, int filter, int law, uint8_t *packed,
                             int64_t packed_capacity, void *stream);

/* ---- fade-out on the wire: a stream that is revoked ends without a click --------
 * A fade is (first, count) in output samples of the wire stream.  With k = t - first, the fp32 value of output t that
 * the entries above clip and quantise (after the static gain, and after the limiter's gain where there is one) is
 * first multiplied by
 *   1                            k < 0: the sample is bitwise what the unfaded entry stores
 *   (float)(count - k) * inv     0 <= k < count;  inv = 1.0f / (float)(count + 1), computed once on the host
 *   0                            k >= count: a range that overshoots the fade stores silence (int16 0, encode(0))
 * The ramp is a pure function of t, so every chunk-invariance of the unfaded entries holds for the faded ones, and it
 * is below 1, so a limited stream still never clips.  count == 0 is a hard cut at `first`; count < 0 means "no fade"
 * (a row of a pooled call that plays on).  A caller that shortens a stream to first + count simply never asks for
 * the outputs beyond.
 *
 * mbv_pcm_fade_make (host only): fills *out, inv included; -1 when first < 0, count < 0 or out is NULL.
 *
 * The four *_faded entries are mbv_resample_pcm16_range_limited, mbv_resample_pcm16_chunks_limited,
 * mbv_resample_g711_range and mbv_resample_g711_chunks with a fade (range: one for all rows, NULL = none; chunks:
 * fades_host [n] beside chunks_host, NULL = none) and with limit / limits_host optional (NULL = no limiter).  A row
 * without a fade is bitwise its row in the unfaded entry.  The launches are those of the unfaded call (one per kind,
 * mbv_wire_runs); fading rows only add a table upload beside the row table.  Refused before anything is launched,
 * the handle stays usable: first < 0, and an inv that is not bitwise the one mbv_pcm_fade_make gives for count. */
typedef struct mbv_pcm_fade { int64_t first; int64_t count; float inv; } mbv_pcm_fade;  /* count < 0: no fade on this row */
int mbv_pcm_fade_make(int64_t first, int64_t count, mbv_pcm_fade *out);
int mbv_resample_pcm16_range_faded(mbv_model *m, const float *wave, const int64_t *valid_samples, int B,
                                   int64_t in_stride, int orig_sr, int target_sr, int filter, int64_t in_avail,
                                   int64_t out_first, int64_t out_count, const float *peak, int16_t *pcm,
                                   int64_t pcm_stride, float *running_peak, int64_t *out_samples,
                                   const mbv_pcm_limit *limit, const mbv_pcm_fade *fade, void *stream);
int mbv_resample_pcm16_chunks_faded(mbv_model *m, const mbv_pcm_chunk *chunks_host, const mbv_pcm_limit *limits_host,
                                    const mbv_pcm_fade *fades_host, int n, int orig_sr, int target_sr, int filter,
                                    int16_t *packed, int64_t packed_capacity, void *stream);
int mbv_resample_g711_range_faded(mbv_model *m, const float *wave, const int64_t *valid_samples, int B,
                                  int64_t in_stride, int orig_sr, int target_sr, int filter, int64_t in_avail,
                                  int64_t out_first, int64_t out_count, const float *peak, uint8_t *out,
                                  int64_t out_stride, float *running_peak, int64_t *out_samples,
                                  const mbv_pcm_limit *limit, int law, const mbv_pcm_fade *fade, void *stream);
int mbv_resample_g711_chunks_faded(mbv_model *m, const mbv_pcm_chunk *chunks_host, const mbv_pcm_limit *limits_host,
                                   const mbv_pcm_fade *fades_host, int n, int orig_sr, int target_sr, int filter,
                                   int law, uint8_t *packed, int64_t packed_capacity, void *stream);

/* ---- turns on the wire: several utterances as ONE gapless wire stream (no reference counterpart: the reference
 * synthesises every unit of a turn alone and butt-joins their int16, tts_vits.py) ---------------------------------
 * The input of a turn row is a TIMELINE at the model's rate, never materialised: segment s, the waveform of one
 * utterance of `length` valid samples, sits at `start`; segments are ascending and disjoint, and what lies between
 * them is silence (0.f).  Each segment is multiplied at its two ends by a de-click ramp of `ramp` samples, in fp32
 * with one rounding, i the index inside the segment:
 *   i < ramp:             wave[i] * ((float)(i + 1) * inv)
 *   i >= length - ramp:   wave[i] * ((float)(ramp - (i - (length - ramp))) * inv)
 * with inv the value mbv_pcm_fade_make gives for count = ramp (the fade's ramp, mirrored for the rise), and is not
 * touched anywhere else; ramp <= length / 2, so the two never overlap, ramp = 0 is none.  The wire step over that
 * timeline is the one of the chunk entries: every stored int16 / G.711 byte, running peak and out_samples is BITWISE
 * what mbv_resample_pcm16_chunks_faded / mbv_resample_g711_chunks_faded store for a chunk whose `wave` is the
 * timeline written out as one fp32 row (the same device code behind the staging of the input window).
 *
 * mbv_turn_chunk: `chunk` as in those entries with chunk.wave NULL; in_total is the timeline's total (or, while the
 * turn is open, a capacity that stands in for it: an open row's final outputs do not depend on it) and in_avail its
 * frontier: every timeline sample below it exists (decoded, or silence), and nothing at or past it is read.  segs is
 * HOST memory [n_segs]: the segments that intersect the input window of the chunk's outputs (more may be given).
 *
 * mbv_turn_plan (host only: no handle, no GPU; reads the integer fields only): the checks of mbv_pcm_chunks_plan on
 * every `chunk` — with limits (HOST [n] or NULL, ceiling == 0 = not limited) the range must end at or below
 * min(mbv_limiter_ready(.., in_avail, in_total, lookahead), pcm_capacity), the open branch being
 * mbv_resample_ready_open(in_avail) — and on its segments: start >= 0, length > 0, 0 <= ramp <= length / 2, ascending
 * and disjoint, at most MBV_TURN_MAX_SEGS segments in one call.  Fills packed_first (or NULL) and returns the packed
 * total as mbv_pcm_chunks_plan does, or -1 with a message that names the turn ("turn i: ...").
 *
 * mbv_resample_turns: turns_host, limits_host (or NULL), fades_host (or NULL) are HOST [n] and travel as kernel
 * arguments like the chunk tables, the segments in one table for the call; nothing is synchronised and the arrays may
 * be freed on return.  law 0 stores int16, MBV_G711_ULAW / MBV_G711_ALAW bytes (pcm, pcm_capacity, packed and
 * packed_capacity then count bytes).  ONE launch for the unlimited turns of a call and one for the limited ones
 * (mbv_wire_runs).  Refused before anything is launched, the handle stays usable: whatever the plan refuses, a
 * non-NULL chunk.wave, a missing pcm or segment wave, a law other than those three, a bad fade, a packed_capacity
 * below the total, two turns that write overlapping ranges of one pcm, and a limited turn whose halo window does not
 * fit the LDS stage. */
#define MBV_TURN_MAX_SEGS 4096
typedef struct mbv_turn_seg {
  const float *wave;           /* DEVICE, the utterance's wave row */
  int64_t start, length;       /* its place on the timeline and its valid samples */
  int32_t ramp;                /* de-click samples at either end */
} mbv_turn_seg;
typedef struct mbv_turn_chunk {
  mbv_pcm_chunk chunk;         /* chunk.wave NULL */
  const mbv_turn_seg *segs;    /* HOST [n_segs] */
  int32_t n_segs;
} mbv_turn_chunk;
int64_t mbv_turn_plan(int orig_sr, int target_sr, int filter, const mbv_turn_chunk *turns,
                      const mbv_pcm_limit *limits, int n, int64_t *packed_first);
int mbv_resample_turns(mbv_model *m, const mbv_turn_chunk *turns_host, const mbv_pcm_limit *limits_host,
                       const mbv_pcm_fade *fades_host, int n, int orig_sr, int target_sr, int filter, int law,
                       void *packed, int64_t packed_capacity, void *stream);

/* ---- token marks: where every token starts, in z-frames ------------------------
 * The exclusive prefix sums of the per-token durations the length regulator uses (predicted, or given with
 * mbv_set_durations / mbv_enc_row.durations): marks[0] = 0, marks[j] = d_0 + .. + d_{j-1}; entry t_text is the sum, and
 * entries behind a row's own text repeat it.  They are what a dialogue manager needs to tell which tokens a listener
 * heard before a stream was revoked.  The scan is the one the duration kernels already ran on the device; these
 * entries store it as int64 so that the caller can place it next to y_lengths and read both back in ONE copy.  One
 * launch each, no synchronisation, and no part in mbv_encoder_runs.
 *
 * mbv_token_marks: after mbv_encode (and mbv_set_durations): row b of the encoded batch -> marks[b * marks_stride + j],
 * j in [0, T]; marks_stride >= T + 1 (DEVICE int64).
 *
 * mbv_token_marks_rows: after mbv_encode_rows on `slot`, one table row per encoded row, in ONE launch for the run:
 * `count` entries (1 .. t_text + 1 <= T + 1) to `marks` (DEVICE), nothing where marks is NULL.  rows_host is HOST memory
 * and travels as kernel arguments.  A call whose rows are all NULL launches nothing. */
typedef struct mbv_mark_row { int64_t *marks; int32_t count; int32_t reserved; } mbv_mark_row;
int mbv_token_marks(mbv_model *m, int64_t *marks, int64_t marks_stride, void *stream);
int mbv_token_marks_rows(mbv_model *m, int slot, const mbv_mark_row *rows_host, int n, void *stream);

/* ---- per-token prosody: rate, pauses and fit-to-length on the predicted durations ------------------------------
 * After an encode, replace the durations the length regulator will use by
 *     w_t = ceilf(expf(logw_t) * fl32(s_t * f)) + extra_t        for t < x_lengths[b]
 * from the logw the encode left (the duration predictor's or the SDP's): the arithmetic of the encode's own
 * durations with a scale s_t PER TOKEN (rate), extra_t further frames of the token's own prior (a pause of known
 * length on a blank or "sp" token), and one factor f per row that makes the row fit a frame count.  What follows
 * (mbv_token_marks, mbv_synthesize, their _rows forms) proceeds unchanged: a token's span includes its extras.
 *
 *   scale   DEVICE fp32, finite and >= 0; 0 drops the token.  NULL: s_t = the length_scale given to the encode.  With
 *           a table that length_scale must have been 1.
 *   extra   DEVICE int32, >= 0, or NULL.
 *   fit     frames >= 1 and 0 < lo <= hi < inf: f = the LARGEST fp32 in [lo, hi] with D(f) <= frames, where
 *           D(f) = sum over t < x_lengths[b] of w_t.  D is non-decreasing in f and positive floats order like their
 *           bit patterns, so a bisection on the bit pattern finds f exactly, in at most 32 evaluations of D.  If even
 *           D(lo) > frames: f = lo and status = 1 (the row did not fit; not an error).  If D(hi) <= frames: f = hi.
 *           Nothing is padded.  During the search a token counts min(frames, 2^20) and the sums are 64-bit.
 *           frames == 0 in a HOST fit entry: this row is not fitted (f = 1, status 0; s_t is used as it is).
 * The range rules of mbv_encode hold for a token's total (2^20 frames) and a row's (2^30); a negative, infinite or NaN
 * scale, or a negative extra, below x_lengths[b] flags the row the same way: y_lengths = -1.  The encode's own flags
 * are kept.  One launch, no synchronisation, no part in mbv_encoder_runs; mbv_shape_runs counts these launches.
 * Refused before any launch: bounds not 0 < lo <= hi < inf, frames < 0 (or < 1 where a row asks for a fit), a scale
 * table after an encode whose length_scale was not 1, and a call with nothing to do.
 *
 * mbv_shape_durations: after mbv_encode; scale / extra [B, T] or NULL, fit_host HOST [B] or NULL, fit_out DEVICE [B]
 * or NULL (8 bytes a row, so that it can stand next to y_lengths in one read-back), y_lengths_out DEVICE int64 [B].
 * Afterwards mbv_read_stage knows "fit_scale" [B] and "fit_status" [B] (0.0 / 1.0).
 *
 * mbv_shape_durations_rows: after mbv_encode_rows on `slot`, one table row per encoded row (n = the run's rows), in
 * ONE launch for the rows that carry a control; the others keep their durations.  scale / extra are the row's own
 * [t_text] tensors; y_lengths_out is the run's array as given to mbv_encode_rows.  rows_host is HOST memory.
 *
 * mbv_op_shape_durations: the kernel by itself on a caller's logw [B, T] and lens32 [B] (tests), like
 * mbv_op_durations; `scalar` is s_t without a table.  Synchronises the stream. */
typedef struct mbv_fit { int64_t frames; float lo, hi; } mbv_fit;
typedef struct mbv_fit_result { float scale; int32_t status; } mbv_fit_result;
typedef struct mbv_shape_row {
  const float *scale;            /* DEVICE [t_text] or NULL */
  const int32_t *extra;          /* DEVICE [t_text] or NULL */
  mbv_fit fit;                   /* frames == 0: no fit */
  mbv_fit_result *fit_out;       /* DEVICE, or NULL */
} mbv_shape_row;
int mbv_shape_durations(mbv_model *m, const float *scale, const int32_t *extra, const mbv_fit *fit_host, int B, int T,
                        mbv_fit_result *fit_out, int64_t *y_lengths_out, void *stream);
int mbv_shape_durations_rows(mbv_model *m, int slot, const mbv_shape_row *rows_host, int n, int64_t *y_lengths_out,
                             void *stream);
int mbv_op_shape_durations(mbv_model *m, const float *logw, const int32_t *lens, const float *scale,
                           const int32_t *extra, float scalar, const mbv_fit *fit_host, float *w_ceil, int32_t *cum,
                           int32_t *ylen32, int64_t *ylen64, const int32_t *bad, mbv_fit_result *fit_out, int B, int T,
                           void *stream);
int64_t mbv_shape_runs(mbv_model *m);

/* ---- per-token volume: a gain envelope from the tokens into the wire kernels (no reference counterpart) ---------
 * `gain` holds one linear factor per token (fp32, 0 <= g <= 16 by convention, checked by the Python layer).  Two
 * steps, both on the device:
 *
 * 1. FRAME GAINS.  For a row with y kept frames inside a stream of `frames` frames, G is fp32 [frames + 1]:
 *      G[t] = gain[j(t)]   for t < y,   j(t) = the first token whose inclusive duration sum exceeds t: the token the
 *                          length regulator gave frame t (after mbv_set_durations / mbv_shape_durations); tokens of
 *                          zero frames are skipped by that rule
 *      G[t] = G[y - 1]     for y <= t <= frames
 *      G[t] = 1.0f         everywhere for a flagged row, for y = 0, and for a frame no token holds
 *    A copy, so bitwise.  One launch, no synchronisation, no part in mbv_encoder_runs; mbv_gain_runs counts them.
 *    mbv_frame_gain: after mbv_encode (and set / shape durations); gain DEVICE [B, T], out DEVICE [B, out_stride],
 *      out_stride >= frames + 1; y = min(the row's frame count, frames).
 *    mbv_frame_gain_rows: after mbv_encode_rows on `slot`, one table row per encoded row (n = the run's rows), in ONE
 *      launch for the rows that carry a gain (gain DEVICE [t_text], out DEVICE [frames + 1]); a row without one is all
 *      NULL / 0.  A call in which no row carries one launches nothing.  rows_host is HOST memory.
 *    mbv_op_frame_gain: the kernel by itself on a caller's cum [B, T] (int32, the inclusive scan) and y_lengths [B]
 *      (int64, negative = flagged), for tests.  Synchronises the stream.
 *
 * 2. THE ENVELOPE.  A pure function of the model-rate sample index j of the row (no state, no halo), with
 *    hop = samples per frame, f = j / hop, r = j - f hop:
 *      e(j) = G[f] + ((float)r * inv_hop) * (G[f + 1] - G[f]),       inv_hop = 1.0f / (float)hop
 *    every operation rounded to fp32 on its own (no fma), and the wire kernels read fl32(wave[j] * e(j)) where they
 *    read wave[j] today: in front of the FIR, the running peak, the static gain, the limiter, the fade and the clip.
 *    So the limiter sees the shaped signal and still guarantees its ceiling, the running peak is the shaped signal's,
 *    and the G.711 byte is the byte of the emitted int16.  A token's gain is reached at the start of its first frame;
 *    the move to the next token's gain takes that token's last frame.  Continuous, so free of clicks by construction.
 *    G all 1.0f gives e = 1.0f exactly and the bits of the unshaped entry.
 *
 * mbv_pcm_envelope: gain DEVICE [frames + 1]; gain NULL = no envelope on this row (frames, hop, inv_hop then 0): the
 * row executes no multiply and is bitwise its row in the unshaped entry.
 *
 * The three *_shaped entries are supersets of the existing ones: each takes a law (0: int16, MBV_G711_ULAW /
 * MBV_G711_ALAW: bytes), an optional limiter, an optional fade and the envelope.
 *   mbv_resample_pcm16_range_shaped: mbv_resample_g711_range_faded with law 0 allowed; `envelope` (or NULL) is the
 *     envelope of row 0, row b reads gain + b * env_stride (env_stride >= frames + 1 when B > 1).
 *   mbv_resample_pcm16_chunks_shaped: mbv_resample_g711_chunks_faded with law 0 allowed; envelopes_host HOST [n] beside
 *     chunks_host (or NULL).
 *   mbv_resample_turns_shaped: mbv_resample_turns; seg_envelopes_host HOST, one per SEGMENT of the call in call order
 *     (turn 0's segments, then turn 1's, ..), or NULL.  A segment's envelope runs over its own sample index and is
 *     applied before its de-click ramp: the timeline of the shaped waves.
 * The launches are those of the unshaped call (mbv_wire_runs): a launch in which a row is shaped reads an envelope
 * table beside its row table, a launch without one is the unshaped launch.  Refused before anything is launched, the
 * handle stays usable: whatever the unshaped entry refuses; hop < 1; frames < 1; an inv_hop that is not bitwise
 * 1.0f / (float)hop; frames * hop below the row's in_total (in_stride; a segment's length); a NULL gain with non-zero
 * sibling fields; an env_stride below frames + 1 with B > 1, or non-zero without a gain. */
typedef struct mbv_gain_row { const float *gain; float *out; int32_t frames; int32_t reserved; } mbv_gain_row;
int mbv_frame_gain(mbv_model *m, const float *gain, float *out, int64_t out_stride, int frames, void *stream);
int mbv_frame_gain_rows(mbv_model *m, int slot, const mbv_gain_row *rows_host, int n, void *stream);
int mbv_op_frame_gain(mbv_model *m, const int32_t *cum, const int64_t *y_lengths, const float *gain, float *out,
                      int64_t out_stride, int frames, int B, int T, void *stream);
int64_t mbv_gain_runs(mbv_model *m);
typedef struct mbv_pcm_envelope { const float *gain; int64_t frames; int32_t hop; float inv_hop; } mbv_pcm_envelope;
int mbv_resample_pcm16_range_shaped(mbv_model *m, const float *wave, const int64_t *valid_samples, int B,
                                    int64_t in_stride, int orig_sr, int target_sr, int filter, int64_t in_avail,
                                    int64_t out_first, int64_t out_count, const float *peak, void *out,
                                    int64_t out_stride, float *running_peak, int64_t *out_samples,
                                    const mbv_pcm_limit *limit, int law, const mbv_pcm_fade *fade,
                                    const mbv_pcm_envelope *envelope, int64_t env_stride, void *stream);
int mbv_resample_pcm16_chunks_shaped(mbv_model *m, const mbv_pcm_chunk *chunks_host, const mbv_pcm_limit *limits_host,
                                     const mbv_pcm_fade *fades_host, const mbv_pcm_envelope *envelopes_host, int n,
                                     int orig_sr, int target_sr, int filter, int law, void *packed,
                                     int64_t packed_capacity, void *stream);
int mbv_resample_turns_shaped(mbv_model *m, const mbv_turn_chunk *turns_host, const mbv_pcm_limit *limits_host,
                              const mbv_pcm_fade *fades_host, const mbv_pcm_envelope *seg_envelopes_host, int n,
                              int orig_sr, int target_sr, int filter, int law, void *packed, int64_t packed_capacity,
                              void *stream);

/* ---- per-token pitch: a time-warp kernel between the decoder and the wire (no reference counterpart) ------------
 * Varispeed: a token that is synthesised p times longer (per-token length_scale) and played p times faster keeps its
 * length and sounds p higher.  Formants move with the pitch; nothing here measures quality.  MBV_PITCH_MIN / _MAX are
 * refusal bounds and a convention.
 *
 * One row has `frames` frames of `hop` model-rate samples, n = frames * hop, and
 *   rate  fp32 [frames]      the playback rate R[f] of frame f, MBV_PITCH_MIN <= R[f] <= MBV_PITCH_MAX
 *   U     fp64 [frames + 1]  U[0] = 0, U[f + 1] = U[f] + (double)hop / (double)R[f], added in ascending order
 *   n_out = (int64)floor(U[frames])
 * Output t in [0, n_out) lies in the largest frame f with U[f] <= (double)t, at the model time
 *   tau = (double)(f * hop) + ((double)t - U[f]) * (double)R[f]          every operation rounded to fp64 on its own
 * and is resampy's interpolator evaluated at time tau with ratio 1 / R[f]: scale = R[f] > 1 ? 1.0 / R[f] : 1.0, index
 * step (int)(scale * 512), the window (MBV_RESAMPLE_KAISER_BEST / _FAST, one fp64 table per filter, fp32 on the device)
 * times scale, both tap loops bounded by [0, n).  The sample at model index j is wave[j], or with an envelope
 * fl32(wave[j] * e(j)) as the shaped wire entries read it; nothing at or past min(n, in_avail) and nothing below 0 is
 * loaded: a zero stands there.  fp32 weights and accumulation.  A pure function of t: a row does not depend on how
 * it is cut into ranges or on the rows that share its launch.
 *
 * mbv_warp_plan (host only): U_out_host [frames + 1] and *n_out from rate_host.  Refuses (mbv_last_error(NULL)) hop or
 *   frames < 1 and a rate that is not finite or lies outside the bounds, naming the frame.
 * mbv_warp_ready (host only): how many outputs are final once the model samples [0, in_avail) exist; -1 when refused.
 *   n_out for in_avail >= n.  Else HW = ceil(num_zeros * max(1, max_f R[f])) + 2 (num_zeros 64 / 16), a = in_avail - HW,
 *   0 for a <= 0, and with g = a / hop:  max(0, floor(U[g] + (double)(a - g * hop) / (double)R[g]) - 1).
 * mbv_warp_ranges: outputs [out_first, out_first + out_count) of n rows, each into its own fp32 row, in ONE launch;
 *   rows_host is HOST memory.  wave, U, rate (and the envelope's gain) are DEVICE; U_host / rate_host are the HOST copies
 *   of the same tables, from which the entry recomputes the row's readiness.  envelope.gain NULL = none (sibling fields 0).
 *   No synchronisation; mbv_warp_runs counts the launches.  Refused before anything is launched, the handle stays usable
 *   and the message names the row: n < 1; a NULL pointer; frames or hop < 1, samples != frames * hop; negative in_avail,
 *   out_first or out_count; outputs beyond mbv_warp_ready of the row or beyond out_capacity; an unknown res_type; a rate
 *   outside the bounds; an envelope the shaped entries would refuse or whose frames * hop is below samples; two rows
 *   that write one sample. */
#define MBV_PITCH_MIN 0.5f
#define MBV_PITCH_MAX 2.0f
typedef struct mbv_warp_row {
  const float *wave;
  int64_t samples;
  int64_t in_avail;
  const double *U;
  const float *rate;
  const double *U_host;
  const float *rate_host;
  int32_t frames;
  int32_t hop;
  mbv_pcm_envelope envelope;
  int64_t out_first;
  int64_t out_count;
  float *out;
  int64_t out_capacity;
  int32_t res_type;
  int32_t reserved;
} mbv_warp_row;
int mbv_warp_plan(int hop, int64_t frames, const float *rate_host, double *U_out_host, int64_t *n_out);
int64_t mbv_warp_ready(int hop, int64_t frames, const float *rate_host, const double *U_host, int res_type,
                       int64_t in_avail);
int mbv_warp_ranges(mbv_model *m, const mbv_warp_row *rows_host, int n, void *stream);
int64_t mbv_warp_runs(mbv_model *m);

/* ---- loudness: ITU-R BS.1770 integrated loudness of a mono waveform, on the device ------------------------------
 * K-weighting (two cascaded biquads, zero state at sample 0), segments of H = (rate + 5) / 10 samples (100 ms; a half
 * rounds up), blocks of four segments (400 ms, 75 % overlap), the absolute gate at -70 LKFS and the relative gate 10 LU
 * below the loudness of the absolute-gated blocks; L = -0.691 + 10 log10(mean z of the blocks that pass both), -inf
 * when there are fewer than four complete segments or no block passes.  An incomplete last segment is dropped.
 *
 * The cascade runs in transposed direct form II in fp64, state s = (shelf s1, s2, high-pass s1, s2):
 *   y = b0 x + s1;  s1 = b1 x - a1 y + s2;  s2 = b2 x - a2 y     per stage, the shelf's y being the high-pass's x
 * The kernel is parallel over segments: the zero-state end state r_k of every segment, the chain s_{k+1} = M s_k + r_k
 * in segment order (M the H-step zero-input transition of s), then every energy e_k = sum y^2 from its true start
 * state.  Inside a segment the arithmetic is a fixed function of the samples and s_k, so e_k, the state and L do not
 * depend on how the segments were cut into calls.  One launch a call, one workgroup a row; no synchronisation.
 *
 * mbv_kweighting (host only): coeffs = shelf {b0, b1, b2, a1, a2}, high-pass {b0, b1, b2, a1, a2} for `rate` by the
 * bilinear re-derivation of the standard's 48 kHz table (which it reproduces to 1e-14); M row-major 4 x 4.
 * mbv_loudness_segments (host only): -> samples / H, and H to *hop (may be NULL); -1 when refused.
 *
 * mbv_loudness: row b of wave [B, in_stride] (DEVICE fp32) over its first valid_samples[b] samples (DEVICE int64,
 * clamped to the row; NULL = whole rows) -> loudness[b] (DEVICE fp32).  energies: NULL, or DEVICE fp64
 * [B, in_stride / H]: e_k of every complete segment, 0 behind the row's valid length.
 *
 * mbv_loudness_range: segments [seg_first, seg_first + seg_count) of every row, of which the first in_avail samples
 * exist.  state (DEVICE fp64 [B, 4]) carries s between calls; a call with seg_first == 0 starts from zero whatever it
 * holds.  energies (DEVICE fp64 [B, energy_stride]) receives the range and is read below it; loudness[b] becomes the
 * integrated loudness of segments [0, seg_first + seg_count).  A row whose valid_samples ends inside the range
 * measures up to there.
 *
 * mbv_loudness_chunks: the same with every per-row quantity from a table row, ONE launch for all rows that have
 * segments (a call in which none has launches nothing).  chunks_host is HOST memory and travels as kernel arguments.
 *
 * Refused before anything is launched, the handle stays usable: a rate below 1000 Hz; a range that does not start at
 * the row's next segment (the handle remembers, by state buffer, where the last call on it ended; 0 always starts
 * over); a range that ends beyond in_avail / H or beyond the energies; a NULL state, energies or loudness.
 * mbv_loudness_runs counts the launches. */
typedef struct mbv_loudness_chunk {
  const float *wave; int64_t in_total; const int64_t *valid_samples; int64_t in_avail;
  int64_t seg_first; int64_t seg_count; double *state; double *energies; int64_t energy_capacity; float *loudness;
} mbv_loudness_chunk;
int mbv_kweighting(int rate, double *coeffs /* [10] */, double *M /* [16] */);
int64_t mbv_loudness_segments(int rate, int64_t samples, int32_t *hop);
int mbv_loudness(mbv_model *m, const float *wave, const int64_t *valid_samples, int B, int64_t in_stride, int rate,
                 float *loudness, double *energies, void *stream);
int mbv_loudness_range(mbv_model *m, const float *wave, const int64_t *valid_samples, int B, int64_t in_stride, int rate,
                       int64_t in_avail, int64_t seg_first, int64_t seg_count, double *state, double *energies,
                       int64_t energy_stride, float *loudness, void *stream);
int mbv_loudness_chunks(mbv_model *m, const mbv_loudness_chunk *chunks_host, int n, int rate, void *stream);
int64_t mbv_loudness_runs(mbv_model *m);

/* ---- seeded noise: standard normals as a pure function of (seed, purpose, row, channel, frame) ---------------
 * Every entry above that takes `noise` / `noise_w` reads a device buffer the caller fills.  These entries fill such
 * buffers from a counter-based generator, so that a request's noise depends on its seed alone: not on a global
 * generator, the requests before it, its place in a batch, padding, chunking or how a recording was pushed.  The
 * consumers are unchanged and keep every bitwise relation they have.  The generator is part of the contract:
 *   Philox4x32-10, multipliers 0xD2511F53 / 0xCD9E8D57, Weyl constants 0x9E3779B9 / 0xBB67AE85
 *   key      (seed & 0xffffffff, seed >> 32)
 *   counter  (t >> 2, c, purpose, row): t the frame, c the channel, purpose MBV_NOISE_*, row a sub-stream index
 *   the output words w0..w3 give the normals of frames 4 (t >> 2) + 0..3 of channel c: (w0, w1) -> (n0, n1) and
 *   (w2, w3) -> (n2, n3) by Box-Muller in fp32, u1 = ((wa >> 8) + 1) 2^-24 in (0, 1], u2 = (wb >> 8) 2^-24,
 *   r = sqrtf(-2 logf(u1)), n_even = r cos(2 pi u2), n_odd = r sin(2 pi u2) (sincospif(2 u2); accurate libm only)
 * Element (c, t) is lane t & 3 of block t >> 2 ALWAYS, also when a fill starts or ends inside a block: a fill of
 * [first, first + count) is bitwise the slice of a fill of [0, first + count).
 * Known answer: counter 0, key 0 -> 6627e8d5 e169c58d bc57ac4c 9b00dbd8.
 *
 * mbv_randn_blocks fills the n blocks of a table in ONE launch: dst[c * stride + (t - first)] for c < channels and
 * t in [first, first + count); nothing else is written.  blocks_host is HOST memory [n] and travels as kernel
 * arguments like the other row tables (it may be freed when the call returns); no copy, no synchronisation.
 * Refused before any launch, with a message that names the block: n < 1, a null dst with count > 0, stride < count,
 * channels < 1, first < 0, count < 0, first + count > 2^30 (the frame limit of an utterance), purpose > 2.  A block
 * with count 0 is legal and writes nothing; a call whose blocks are all empty launches and counts nothing.
 *
 * mbv_randn_host computes frames [first, first + count) of one channel on the host with the same Philox function and
 * logf / sqrtf / sinf / cosf in fp32: no GPU, no handle.  Host and device libm differ in the last bits, so the two
 * agree within 1e-5 absolute (measured: DESIGN 7.13), not bitwise.  Returns 1 for the arguments mbv_randn_blocks
 * refuses.
 *
 * mbv_noise_runs: mbv_randn_blocks launches on this handle since mbv_create (table writers are not counted). */
#define MBV_NOISE_PRIOR     0   /* models.py:729  z_p = m_p + noise * exp(logs_p) * noise_scale: [inter, T']      */
#define MBV_NOISE_SDP       1   /* models.py:94   the duration predictor's draw: [2, T_text]                      */
#define MBV_NOISE_POSTERIOR 2   /* models.py:245  z = m + noise * exp(logs): [inter, T_spec]                      */
typedef struct mbv_randn_block {
  float *dst;                 /* DEVICE; row c of the block starts at dst + c * stride */
  int64_t stride;             /* floats between channel rows, >= count */
  int32_t channels, reserved;
  int64_t first, count;       /* frames [first, first + count) */
  uint64_t seed;
  uint32_t purpose, row;      /* MBV_NOISE_*, sub-stream index */
} mbv_randn_block;
int mbv_randn_blocks(mbv_model *m, const mbv_randn_block *blocks_host, int n, void *stream);
int mbv_randn_host(uint64_t seed, uint32_t purpose, uint32_t row, uint32_t c, int64_t first, int64_t count, float *dst);
int64_t mbv_noise_runs(mbv_model *m);

/* ---- linear spectrogram ------------------------------------------------------
 * replaces spectrogram_torch(y, n_fft, sr, hop, win, center=False) (mel_processing.py:51-70), the input of
 * mbv_voice_conversion: |STFT| with (n_fft - hop) / 2 zeros on each side of the row, no centring, the
 * periodic Hann window of length win centred in n_fft as torch.stft centres it, onesided, and abs() with no
 * epsilon.  Every row is transformed as if alone (zeros at and past its valid length; samples there are never
 * read) and padded with zero frames, as the collate function pads a ragged batch (data_utils.py:125-147).
 * Computed as a real FFT (complex FFT of n_fft / 2 points + split post-pass) on fp32 twiddle and window tables
 * built in float64.  Refused: n_fft not a power of two in [256, 4096], hop or win outside [1, n_fft].
 *   wave           [B, in_stride] device: fp32 (MBV_WAVE_F32) or int16 (MBV_WAVE_PCM16, scaled by exactly
 *                  1 / 32768 as data_utils.py:75 does, so it equals the fp32 path on pcm / 32768 bitwise)
 *   valid_samples  int64 [B] device, clamped to [0, in_stride]; NULL = every row is in_stride samples
 *   spec           fp32 [B, n_fft / 2 + 1, frames] device, frames = mbv_spectrogram_frames(in_stride, ...)
 *                  (any other value is refused); row b holds frames(valid_b) frames, zeros after them
 *   spec_lengths   int64 [B] device, optional: frames(valid_b), computed on the device
 * The first call for an (n_fft, win) pair builds the tables on the host and uploads them with a synchronous
 * copy (cached in the handle); later calls only enqueue one kernel.  Needs no weights. */
#define MBV_WAVE_F32   0
#define MBV_WAVE_PCM16 1          /* int16, scaled by 1/32768 (data_utils.py:75) */
#define MBV_WAVE_ULAW  8          /* G.711 mu-law bytes: rows of mbv_resample_ranges ONLY (2..7 are no dtype) */
#define MBV_WAVE_ALAW  9          /* G.711 A-law bytes, likewise */
int mbv_spectrogram(mbv_model *m, const void *wave, int wave_dtype, const int64_t *valid_samples, int B,
                    int64_t in_stride, int n_fft, int hop, int win, float *spec, int64_t frames,
                    int64_t *spec_lengths, void *stream);
/* Host only (no handle, no GPU): frames of an n-sample row, 0 if n + 2 ((n_fft - hop) / 2) < n_fft (where
 * torch.stft raises), else 1 + (n + 2 ((n_fft - hop) / 2) - n_fft) / hop.  -1 on bad arguments (n < 0, or
 * n_fft / hop refused as above). */
int64_t mbv_spectrogram_frames(int64_t n_samples, int n_fft, int hop);

/* ---- pooled voice conversion: audio requests admitted as decode streams ---------
 * The front half of mbv_voice_conversion — spectrogram, posterior encoder, forward flow with the source speaker,
 * reverse flow with the target — for many audio requests as ONE padded run, stopping at z_hat: each row's
 * (z_hat * y_mask)[:, :frames] lands in a tensor of the request's own, which feeds mbv_decode_chunks like the z of
 * mbv_synthesize_rows.  In the default mode every such z is BITWISE the z of that request converted alone (n = 1,
 * t_frames = its own frame count) with the same noise, and at noise_scale 1 bitwise the z_hat * y_mask of
 * mbv_spectrogram + mbv_voice_conversion on that row: nothing on the posterior path looks behind a row's length, and
 * the table-reading kernels run the scalar kernels' chains of operations.  With "splitk" the result is deterministic
 * and within fp32 rounding of the stand-alone call.
 *
 * mbv_convert_plan (host only): which requests may share a run, by their frame counts (mbv_spectrogram_frames of the
 * sample counts, n_fft = 2 (spec_channels - 1)).  Two requests share a class iff enc_q.pre, enc_q.proj and the
 * coupling layers' pre / post convs, planned for either alone, land on the same side of the conv planner's narrow /
 * tiled divide; a class is cut into further runs only where B rows padded to the run's longest request would plan
 * differently, exceed 65535 rows, or exceed what the fused WN layers take (B * channels * t_frames * 4 bytes < 4 GiB).
 * Runs are numbered in the order of their first request; run_of_request [n] (or NULL) receives each request's run.
 * "splitk": one class.  Returns the number of runs, -1 on a bad argument (n < 1, a count < 1 or beyond that limit).
 *
 * mbv_convert_rows: one run.  rows_host is HOST memory and travels as kernel arguments (free it on return); the
 * spectrogram kernel reads every row's samples in place through the table (no padded copy of the audio) and writes
 * the posterior encoder's channel-padded input itself.  t_frames = the longest row's frame count (the run is planned
 * at that width; any other value is refused); hop / win as
 * mbv_spectrogram takes them.  g_out fp32 [n, gin] device receives emb_g(sid_tgt), the decoder's conditioning.
 * Refused before any launch: a model without speakers (the reference's assertion text), "conv_bf16", a row without
 * samples, with 0 frames or more than t_frames, a speaker id outside [0, n_speakers), noise_scale < 0, noise missing
 * where noise_scale != 0, rows that mbv_convert_plan would not put into one run, a run the fused WN layers do not
 * take (option "wn_fused" off).  No host synchronisation (beyond the first call's table upload for a win).
 *
 * mbv_converter_runs: posterior-encoder runs mbv_convert_rows and mbv_convert_ranges made on this handle since
 * mbv_create. */
typedef struct mbv_convert_row {
  const void *wave;              /* DEVICE [samples] at the model's rate, read in place */
  int64_t samples;
  int32_t wave_dtype;            /* MBV_WAVE_F32 or MBV_WAVE_PCM16 */
  int32_t sid_src, sid_tgt;
  const float *noise;            /* DEVICE [inter, frames], this row's own draw (not read at noise_scale 0) */
  float noise_scale;
  float *z;                      /* DEVICE [inter, frames], the request's own tensor */
} mbv_convert_row;
int mbv_convert_plan(const mbv_config *cfg, int splitk, int n, const int32_t *t_frames, int32_t *run_of_request);
int mbv_convert_rows(mbv_model *m, const mbv_convert_row *rows_host, int n, int t_frames, int hop, int win,
                     float *g_out, void *stream);
int64_t mbv_converter_runs(mbv_model *m);

/* ---- live voice conversion: a recording that is still arriving -----------------
 * Nothing on the way from audio to z_hat looks far: spectrogram frame f reads samples [f hop - pad, f hop - pad +
 * n_fft) (pad = (n_fft - hop) / 2, zeros outside the recording), and z_hat frame t depends on spectrogram frames
 * [t - L, t + R] only, (L, R) = mbv_converter_context.  So z_hat frames [first, first + count) of a recording are
 * computed from the spectrogram window mbv_convert_window names, as one row of a padded run, and only those frames are
 * stored, in place, into the recording's own z.  The convs of a window are planned as for a recording longer than 256
 * frames (the conv planner's narrow-kernel rule cannot be known while the recording is open): in the default mode the
 * stored frames do not depend on how the recording was cut into ranges, and for a recording of more than 256 frames
 * they are BITWISE the z of mbv_convert_rows on the whole recording with the same noise.  For a shorter one they are
 * within fp32 rounding of it (the other kernel family sums in another order).  "splitk": deterministic, within
 * rounding.
 *
 * mbv_converter_context (host only): out = (L, R) in frames, the plain sum of the reaches of the posterior encoder's and
 * both flow passes' k = 5 layers (96 for every supported model; the reach observed is 88).
 * mbv_spectrogram_ready (host only): how many leading spectrogram frames are final once `arrived` samples exist:
 * mbv_spectrogram_frames(arrived) when closed, else the frames all of whose samples exist, max(0, (arrived + pad -
 * n_fft) / hop + 1).  -1 on bad arguments.
 * mbv_convert_window (host only): out = [wa, wb), the spectrogram window for z_hat frames [first, first + count) when
 * final_frames are final: [first - L, first + count + R) clipped to [0, final_frames), wa rounded down to a multiple
 * of 32 (the fused WN layers' unit).  1 on bad arguments.
 * mbv_convert_ranges_plan (host only): the runs for windows of window_frames[i] frames, in order; a run is cut where
 * one more row would exceed 65535 rows or what the fused WN layers take.  Returns the number of runs, -1 on a bad
 * argument (a window alone beyond that limit included).
 *
 * mbv_convert_ranges: one padded run, one row per recording.  rows_host is HOST memory and travels as kernel
 * arguments; the samples are read in place; no host synchronisation (beyond the first call's table upload for a
 * win).  Counted by mbv_converter_runs.  Refused before any launch, naming the row: frames that are not final yet
 * (first + count + R beyond mbv_spectrogram_ready while open, or first + count beyond it), a speaker id outside
 * [0, n_speakers), noise missing or its stride shorter than the window, z_stride < first + count, rows of more than
 * one run of mbv_convert_ranges_plan, "conv_bf16", a model without speakers (the reference's assertion text). */
typedef struct mbv_convert_range {
  const void *wave;              /* DEVICE, the recording's buffer at the model's rate, read in place */
  int64_t arrived;               /* samples that exist so far */
  int32_t closed;                /* != 0: no more samples will come (the right padding of the spectrogram applies) */
  int32_t wave_dtype;            /* MBV_WAVE_F32 or MBV_WAVE_PCM16 */
  int32_t sid_src, sid_tgt;
  int32_t first, count;          /* z_hat frames [first, first + count) */
  const float *noise;            /* DEVICE [inter, noise_stride], the recording's block (not read at noise_scale 0) */
  int64_t noise_stride;
  float noise_scale;
  float *z;                      /* DEVICE [inter, z_stride], the recording's own z; only the range is written */
  int64_t z_stride;
} mbv_convert_range;
int mbv_converter_context(const mbv_config *cfg, int32_t out[2]);
int64_t mbv_spectrogram_ready(int64_t arrived, int closed, int n_fft, int hop);
int mbv_convert_window(const mbv_config *cfg, int first, int count, int64_t final_frames, int32_t out[2]);
int mbv_convert_ranges_plan(const mbv_config *cfg, int n, const int32_t *window_frames, int32_t *run_of_range);
int mbv_convert_ranges(mbv_model *m, const mbv_convert_range *rows_host, int n, int hop, int win, void *stream);

/* ---- live voice conversion with a bounded look-ahead (opt-in) ------
 * The reach R of mbv_converter_context is what the layers CAN see, and a live call cannot wait that long.  A window
 * that ends `ahead` frames behind its range, 0 <= ahead <= R, is well defined: the row of the padded run ends there,
 * every layer is masked there, and the kept frames are what the model gives for a recording whose spectrogram ends
 * there.  It is an approximation of the full-context z_hat; how close is a property of the weights, not of this code.
 *
 * mbv_convert_window_ahead (host only): mbv_convert_window with the window's end at first + count + ahead, clipped to
 * final_frames.  1 on bad arguments (those of mbv_convert_window, ahead outside [0, R]).
 * mbv_convert_ranges_ahead: mbv_convert_ranges with one look-ahead per row, ahead_host [n] HOST memory; ahead_host ==
 * NULL is mbv_convert_ranges (every row at R).  Several rows may name disjoint ranges of one recording (the blocks of
 * a fixed grid that came due together).  Refused before any launch, naming the row: an ahead outside [0, R], first +
 * count + ahead beyond mbv_spectrogram_ready while open, two rows whose ranges overlap in one z, and everything
 * mbv_convert_ranges refuses.  Counted by mbv_converter_runs.
 *
 * Seams.  With a short look-ahead of the decoder, the end of chunk k and the start of chunk k + 1 are two
 * approximations of one signal.  A stream that wants them to meet decodes chunk k a little past its end (the
 * overhang), keeps the first `seam` overhang samples p, and cross-fades the first `seam` samples q of chunk k + 1:
 *   q[i] <- p[i] w_p(i) + q[i] w_q(i),  w_p = (float)(seam - i) inv,  w_q = (float)(i + 1) inv,  inv = 1.0f / (float)(seam + 1)
 * every product and the sum rounded to fp32 once, in that order (no fused multiply-add).
 * mbv_seam_rows: ONE launch for n streams.  Per row: the blend of o[head_first + i], i < head_count, with stash[i];
 * then stash[i] = o[over_first + i], i < over_count.  Rows with both counts 0 are skipped.  rows_host is HOST memory.
 * Refused before any launch, naming the row: a NULL pointer, seam outside [1, 2^20], a count outside [0, seam], a
 * range outside [0, o_samples), a head that overlaps its overhang, two rows that share a stash or blend the same
 * samples.  No synchronisation.  mbv_seam_runs counts the launches since mbv_create. */
typedef struct mbv_seam_row {
  float *o;                      /* DEVICE [o_samples], the stream's waveform */
  int64_t o_samples;
  int64_t head_first;            /* the decoded chunk's first sample */
  int64_t over_first;            /* the first sample behind the chunk */
  float *stash;                  /* DEVICE [seam], the stream's own */
  int32_t head_count, over_count, seam, reserved;
} mbv_seam_row;
int mbv_convert_window_ahead(const mbv_config *cfg, int first, int count, int ahead, int64_t final_frames,
                             int32_t out[2]);
int mbv_convert_ranges_ahead(mbv_model *m, const mbv_convert_range *rows_host, const int32_t *ahead_host, int n, int hop,
                             int win, void *stream);
int mbv_seam_rows(mbv_model *m, const mbv_seam_row *rows_host, int n, void *stream);
int64_t mbv_seam_runs(mbv_model *m);

/* ---- live text: an utterance whose tokens are still arriving ------
 * The text mirror of live voice conversion (no reference counterpart as code: tts_vits.py receives its text unit by
 * unit, synthesis_module.py:258-353 decodes one shared latent piece by piece).  The tokens of ONE utterance come in
 * blocks of bt.  Block k, tokens [k bt, (k + 1) bt), is encoded from the text prefix of E_k = min((k + 1) bt + A, N)
 * tokens as a stand-alone utterance (one row of an mbv_encode_rows run: the text encoder attends over its whole
 * input, so every block re-encodes its prefix); the block's columns of that run's text-level m_p / logs_p and of its
 * durations go into the stream's own token tables (mbv_take_tokens_rows), the block is length-regulated into the
 * stream's own z_p at the running frame offset (mbv_expand_ranges), and the reverse flows run on windows of that z_p
 * (mbv_flow_ranges): z frame t depends on z_p frames [t - R, t + R] only, (R, R) = mbv_text_context.  The decoder side
 * is the one of live conversion (mbv_decode_chunks_routed, mbv_seam_rows).  With A = the whole text, a finished stream
 * of more than 256 frames is BITWISE mbv_encode + mbv_synthesize of the text with the same noise; a shorter one is
 * within fp32 rounding of it (the other kernel family sums in another order), as for mbv_convert_ranges.
 *
 * mbv_text_context (host only): out = (R, R) in frames, the plain sum of the reaches of the reverse pass's k = 5
 * layers (n_flows x n_layers x 2 = 32 for every supported model).  1 on a NULL argument.
 * mbv_flow_window (host only): out = [wa, wb), the z_p window for z frames [first, first + count) of P expanded
 * frames: [first - R, first + count + R) clipped to [0, P), wa rounded down to a multiple of 32 (the rule of
 * mbv_convert_window).  1 on bad arguments (first < 0, count < 1, P < first + count).
 * mbv_flow_ranges_plan (host only): the runs for windows of window_frames[i] frames, in order, as
 * mbv_convert_ranges_plan cuts them.  Returns the number of runs, -1 on a bad argument.
 *
 * mbv_take_tokens_rows: after mbv_encode_rows on `slot`.  Row i copies token columns [a, b) of run row `src`: the
 * run's text-level m_p | logs_p into stats [2 inter, stride] and (int)w_ceil into dur [stride], both at [a, b); a row
 * whose y_length (the run row's entry of y_lengths_out, still on the device) is -1 writes -1 durations.  dur_copy (or
 * NULL) receives the same b - a durations packed, so that one read-back serves a tick.  ONE launch, copies only.
 * Refused before any launch, the handle still usable: an ended run ("without a preceding mbv_encode_rows on slot
 * k"), src outside the run, [a, b) empty or outside the row's t_text, a NULL pointer, stride < b.
 *
 * mbv_expand_ranges: row i regulates tokens [a, b) of the stream's tables into z_p[:, frame : frame + sum dur): an
 * in-kernel scan of the block's durations, then per element the chain of operations of the length regulator of
 * mbv_synthesize (BITWISE mbv_op_expand on the same inputs).  dur_host is HOST memory, the b - a durations as read
 * back.  ONE launch for all rows.  Refused before any launch, naming the row: a NULL pointer, a negative duration,
 * frame < 0, frame + sum dur > max_frames, max_frames beyond z_stride or (where noise_scale != 0) noise_stride, noise
 * missing where noise_scale != 0, stride < b, two rows writing overlapping frames of one z_p.  Rows without frames
 * are skipped.
 *
 * mbv_flow_ranges: ONE padded run: a window gather, the reverse flows by the launcher every other entry uses, planned
 * as for an utterance of more than 256 frames, and a ranged masked scatter of [first, first + count) into z, in
 * place.  Nothing behind P is read.  sid is ignored on a model without speakers; a defined voice is valid.  Refused
 * before any launch, naming the row: a NULL pointer, a range that is not computable yet (first + count + R > P while
 * not complete, or first + count > P), a stride < first + count (z) or < P (z_p), a speaker id outside the tables,
 * two rows writing overlapping frames of one z, rows of more than one run of mbv_flow_ranges_plan, a run outside the
 * fused WN layers, "conv_bf16".
 *
 * mbv_text_runs counts the mbv_take_tokens_rows and mbv_expand_ranges launches, mbv_flow_runs the flow runs, since
 * mbv_create; the encoder passes count in mbv_encoder_runs. */
typedef struct mbv_take_row {
  int32_t src;                   /* the row of the run */
  int32_t a, b;                  /* tokens [a, b) */
  int32_t reserved;
  const int64_t *y_length;       /* DEVICE, the run row's entry of mbv_encode_rows' y_lengths_out */
  float *stats;                  /* DEVICE [2 inter, stride], the stream's m_p | logs_p per token */
  int32_t *dur;                  /* DEVICE [stride], the stream's frames per token */
  int64_t stride;
  int32_t *dur_copy;             /* DEVICE [b - a], a packed second copy of the durations, or NULL */
} mbv_take_row;
typedef struct mbv_expand_range {
  const float *stats;            /* DEVICE [2 inter, stride] */
  const int32_t *dur;            /* DEVICE [stride] */
  int64_t stride;
  const int32_t *dur_host;       /* HOST [b - a], the block's durations as read back */
  int32_t a, b;                  /* tokens [a, b) */
  int32_t frame;                 /* F_a, the frame at which token a starts */
  int32_t max_frames;            /* the stream's capacity in frames */
  const float *noise;            /* DEVICE [inter, noise_stride], the stream's block (not read at noise_scale 0) */
  int64_t noise_stride;
  float noise_scale;
  int32_t reserved;
  float *z_p;                    /* DEVICE [inter, z_stride], the stream's own z_p; only the block's frames are written */
  int64_t z_stride;
} mbv_expand_range;
typedef struct mbv_flow_range {
  const float *z_p;              /* DEVICE [inter, z_p_stride] */
  int64_t z_p_stride;
  int32_t P;                     /* frames of z_p that are expanded */
  int32_t complete;              /* != 0: the text is closed and P is its last frame */
  int64_t sid;
  int32_t first, count;          /* z frames [first, first + count) */
  float *z;                      /* DEVICE [inter, z_stride], the stream's own z; only the range is written */
  int64_t z_stride;
} mbv_flow_range;
int mbv_text_context(const mbv_config *cfg, int32_t out[2]);
int mbv_flow_window(const mbv_config *cfg, int first, int count, int64_t P, int32_t out[2]);
int mbv_flow_ranges_plan(const mbv_config *cfg, int n, const int32_t *window_frames, int32_t *run_of_range);
int mbv_take_tokens_rows(mbv_model *m, int slot, const mbv_take_row *rows_host, int n, void *stream);
int mbv_expand_ranges(mbv_model *m, const mbv_expand_range *rows_host, int n, void *stream);
int mbv_flow_ranges(mbv_model *m, const mbv_flow_range *rows_host, int n, void *stream);
int64_t mbv_text_runs(mbv_model *m);
int64_t mbv_flow_runs(mbv_model *m);

/* ---- introspection (tests, debugging) ---------------------------------------
 * Copies an internal stage tensor of the last call into `dst` (device).
 * Names: "x_enc" [B,H,T], "m_text", "logs_text" [B,I,T], "logw", "w_ceil"
 * [B,1,T], "x_post" [B,72,F], "dec_conv_pre", "dec_up_0", "dec_res_0",
 * "dec_up_1", "dec_res_1"; after mbv_convert_rows / mbv_convert_ranges "convert_ypad" [B, cin_pad, T], the posterior encoder's
 * channel-padded input as the spectrogram kernel wrote it (cin_pad = spec_channels rounded up to 32); after
 * mbv_shape_durations "fit_scale" and "fit_status" [B].  Returns the element count, or < 0 on error;
 * dst == NULL only queries the count. */
int64_t mbv_read_stage(mbv_model *m, const char *name, float *dst, int64_t capacity,
                       void *stream);

/* The text encoder's windowed relative-position attention by itself (tests; attentions.py:148-243):
 * qkv DEVICE [B, 3H, T] (q | k | v as the fused projection leaves them), emb_k / emb_v DEVICE [9, H / n_heads]
 * (heads share), lengths DEVICE int64 [B], o DEVICE [B, H, T].  Synchronises the stream. */
int mbv_op_rel_attention(mbv_model *m, const float *qkv, const float *emb_k, const float *emb_v,
                         const int64_t *lengths, float *o, int B, int H, int n_heads, int T, void *stream);

/* Generic conv1d through the MFMA kernel (tests): y = conv(x, w) + bias,
 * 'same' padding.  w HOST [Cout, Cin, K], bias HOST [Cout] or NULL,
 * x/y DEVICE [B, Cin, T] / [B, Cout, T]; in_slope: leaky-relu slope applied
 * to x first (1 = none). */
int mbv_op_conv1d(mbv_model *m, const float *x, const float *w_host, const float *bias_host,
                  float *y, int B, int Cin, int Cout, int T, int K, int dilation,
                  float in_slope, void *stream);

/* One conv of the decoder's kinds through the launcher the decoder uses (tests): any route, any of the
 * epilogues below.  Semantics, per utterance b (act = leaky-relu with in_slope, applied after chan_add;
 * positions outside [0, Tin) and at or past in_lens[b] read as 0):
 *   kind CONV:   y[co, t] = bias[co] + sum_ci,k w[co, ci, k] act(xp[ci, t + k dil - (K - 1) dil / 2])
 *                with xp = x, or ReflectionPad1d((1, 0))(x) (Tin + 1 frames) when reflect1;
 *                STORE: y = relu?(.) * (t < out_lens[b]);  RESID: y = . + res + res_chan_add[b, co];
 *                RESID_ACC: y = (. + res + res_chan_add[b, co] + accum_in) * out_scale  (accum_in may be y);
 *   kind CONVT4 / CONVT8: ConvTranspose1d(k 16, stride U, padding (16 - U) / 2) of act(x), T == Tin input
 *                frames, y [B, Cout, U Tin]; epilogue STORE only.
 * x DEVICE [B, Cin, x_rstride] (first Tin frames valid), y DEVICE [B, Cout, T] (conv) / [B, Cout, U T] (ConvTranspose).
 * w HOST in the reference layout: conv [Cout, Cin, K], ConvTranspose [Cin, Cout, 16]; bias HOST [Cout] or NULL.
 * Weights are packed by the weight loader's own packers.  Allocates, launches on `stream`, synchronises, frees. */
#define MBV_CONV_KIND_CONV 0
#define MBV_CONV_KIND_CONVT4 4
#define MBV_CONV_KIND_CONVT8 8
#define MBV_CONV_EPI_STORE 0
#define MBV_CONV_EPI_RESID 1
#define MBV_CONV_EPI_RESID_ACC 2
#define MBV_CONV_EPI_LN 7         /* conv + channel LayerNorm in one launch (narrow kernel only: T <= 256, Cout % 32 == 0, Cout <= 768):
                                   * y = (LN_c(relu?(conv) * (t < out_lens[b]) + res) * ln_gamma + ln_beta) * (t < ln_out_lens[b]); res optional */
typedef struct mbv_conv_desc {
  int32_t B, Cin, Cout, Tin, T, K, dil;
  int32_t x_rstride;              /* elements between channel rows of x (0: Tin) */
  int32_t kind;                   /* MBV_CONV_KIND_* (ConvTranspose: K and dil are implied) */
  int32_t epi;                    /* MBV_CONV_EPI_* */
  float in_slope;                 /* 1: no activation */
  int32_t relu, reflect1;
  const int32_t *in_lens;         /* DEVICE [B] or NULL */
  const int32_t *out_lens;        /* DEVICE [B] or NULL (STORE, LN) */
  const float *chan_add;          /* DEVICE [B, Cin] or NULL: added to x before the activation */
  const float *res;               /* DEVICE [B, Cout, T] (RESID, RESID_ACC; LN: or NULL) */
  const float *res_chan_add;      /* DEVICE [B, Cout] or NULL */
  const float *accum_in;          /* DEVICE [B, Cout, T] or NULL (RESID_ACC) */
  float out_scale;                /* RESID_ACC */
  const int64_t *trim_lens;       /* HOST [B] or NULL: trimmed launch, column tiles below min(T, trim_lens[b] * trim_num + trim_add) */
  int32_t trim_num, trim_add;
  int32_t splitk;                 /* 1: split-K allowed (mbv_op_conv: also when the handle's option "splitk" is on, unless trimmed) */
  int32_t prec;                   /* 0 exact fp32, 3 split-bf16 (as mbv_set_option "conv_bf16") */
  int32_t legacy_convt;           /* must be 0 (a kernel that is gone; the slot keeps the layout) */
  int64_t ws_floats;              /* mbv_conv_plan only: the handle's split-K workspace (mbv_op_conv uses its own) */
  int32_t n_counters;             /* ... and ticket counters */
  const float *ln_gamma;          /* LN: DEVICE [Cout] */
  const float *ln_beta;           /* LN: DEVICE [Cout] */
  const int32_t *ln_out_lens;     /* LN: DEVICE [B] or NULL, the mask behind the LayerNorm */
  int32_t tail_once;              /* 1 (with trim_lens; conv with STORE / RESID / RESID_ACC): the launch of "tail_once" — the row with the
                                   * smallest trim_lens keeps every tile, the tiles the others drop are copied from it (trim_add = reach).
                                   * 2: the same on the packed route (MBV_ROUTE_TAIL_PACK) where the planner grants it: every other
                                   * row keeps its columns below trim_lens[b] * trim_num + trim_add rounded up to 32, the rows' kept
                                   * columns laid end to end share the tiles, and the rest is copied from the donor */
} mbv_conv_desc;
/* plan[8] = route, tile rows, tile columns, threads, input-channel chunk, nb_big, vs_tv, split-K factor
 * (tile fields 0 on the narrow kernel; see conv1d_plan in csrc/kernels.h) */
#define MBV_ROUTE_NARROW_M 1
#define MBV_ROUTE_NARROW_LAUNCH 2
#define MBV_ROUTE_M64 3
#define MBV_ROUTE_HALF 4
#define MBV_ROUTE_SMALL 5
#define MBV_ROUTE_BIG 6
#define MBV_ROUTE_SPLIT_BATCH 7
#define MBV_ROUTE_VS 8
#define MBV_ROUTE_TAIL_PACK 9   /* 128 x 384 tiles over the packed column axis of a tail_once = 2 launch */
/* plan_out may be NULL. */
int mbv_op_conv(mbv_model *m, const mbv_conv_desc *d, const float *x, const float *w_host, const float *bias_host,
                float *y, int32_t *plan_out, void *stream);
/* Host only (no handle, no GPU): the plan mbv_op_conv would execute for `d` (device pointers are only tested
 * against NULL).  On failure the message is available from mbv_last_error(NULL). */
int mbv_conv_plan(const mbv_conv_desc *d, int32_t out[8]);

/* ---- the small kernels between the convs, each by itself (tests) ---------------
 * One entry per launcher of csrc/ops.hip and csrc/sdp.hip that mbv_encode / mbv_synthesize / mbv_voice_conversion
 * call, with the argument patterns those use (the in-place forms are the caller's choice of pointers).  Every
 * pointer is a DEVICE pointer; "or NULL" marks the optional ones.  Each call checks its arguments (a refusal
 * returns non-zero with a message, launches nothing and leaves the handle usable), launches on `stream`,
 * synchronises it and reports a launch error.  None needs weights.
 *   mbv_op_embed            x [B, H, T] = emb[ids] * sqrt(H) * mask; lens32 [B] = lengths clamped to [0, T]; bad [B]
 *                           = 1 for an id outside [0, n_vocab) or a length outside [0, T] (zeroed first)
 *   mbv_op_layernorm        y = (LN_c(relu?(a + r)) * gamma + beta) * (t < out_lens[b]); r, out_lens or NULL; C <= 256
 *   mbv_op_durations        w [C] given: logw = (w . h[:, :, t] + bias[0]) for t < lens[b], else 0; w NULL: h is
 *                           logw [B, T].  w_ceil = ceil(exp(logw) * length_scale), cum = inclusive sums (int32),
 *                           ylen32 = max(total, 1), ylen64 (or NULL) = that, or -1 where bad[b] (bad or NULL)
 *                           Supported range: a token below 2^20 frames, an utterance at most 2^30; beyond it (or a
 *                           duration that is inf / NaN) the token counts 0, ylen32 = 1 and ylen64 = -1
 *   mbv_op_expand           length regulation from cum / ylen32 [B]: stats [B, 2 I, T] holds m_text | logs_text;
 *                           noise [B, I, Tp] or NULL; m_p, logs_p, z_p, attn [B, Tp, T], y_mask [B, Tp] or NULL; z required
 *   mbv_op_cond_gemv        out [B, Cout] = W [Cout, Cin] g[b] + bias (bias or NULL)
 *   mbv_op_gather_rows      out [B, C] = table[sid[b]]; bad [B] or NULL is set (never cleared) for sid outside [0, n_rows)
 *   mbv_op_posterior_sample z [B, I, T] = (m + noise * exp(logs)) * mask, stats [B, 2 I, T] = m | logs; noise or NULL
 *   mbv_op_lens             lens32 [B], bad [B] from int64 lengths (as mbv_op_embed), then mask [B, T] (or NULL) from lens32
 *   mbv_op_dds_sep          y = gelu(LN_c(depth-wise conv_K,dil(x * mask) + bias)); w [C, K]; K = 3, C <= 256
 *   mbv_op_dds_res          y = (xres + gelu(LN_c(a))) * (t < out_lens[b]); out_lens or NULL; y may be xres
 *   mbv_op_sdp_pre          h [B, C, T] = pre_w[c] * z[b, zc, t] + pre_b[c] + cond; z [B, 2, T], zc 0 or 1
 *   mbv_op_sdp_spline       Flip + inverse rational-quadratic spline + mask in place on z [B, 2, T]; h [B, 29, T]
 *   mbv_op_sdp_logw         logw [B, T] = (z[:, 1] - m[0]) * exp(-logs[0]) * mask
 *   mbv_op_sdp_noise        z [n] = noise * scale, or zeros when noise is NULL
 *   mbv_op_chan_add         x [B, C, T] += v [B, C]
 *   mbv_op_istft_single     the single-band waveform tail by itself: x_post [B, 18, frames] (log-magnitude | phase
 *                           pre-activations; prescaled != 0: rows already times log2(e) | 1 / (2 pi), as the packed
 *                           conv_post leaves them) -> o [B, 4 (frames - 1)], spec / phase [B, 9, frames] or NULL;
 *                           frames >= 2; exact or hardware transcendentals as the handle's "istft_exact" option says */
int mbv_op_embed(mbv_model *m, const int64_t *ids, const int64_t *lengths, const float *emb, float *x, int32_t *lens32,
                 int32_t *bad, int B, int T, int H, int n_vocab, void *stream);
int mbv_op_layernorm(mbv_model *m, const float *a, const float *r, const float *gamma, const float *beta, float *y,
                     int B, int C, int T, int pre_relu, const int32_t *out_lens, void *stream);
int mbv_op_durations(mbv_model *m, const float *h, const float *w, const float *bias, const int32_t *lens,
                     float length_scale, float *logw, float *w_ceil, int32_t *cum, int32_t *ylen32, int64_t *ylen64,
                     const int32_t *bad, int B, int C, int T, void *stream);
int mbv_op_expand(mbv_model *m, const float *stats, const int32_t *cum, const int32_t *ylen32, const float *noise,
                  float noise_scale, float *m_p, float *logs_p, float *z_p, float *z, float *attn, float *y_mask,
                  int B, int I, int T, int Tp, void *stream);
int mbv_op_cond_gemv(mbv_model *m, const float *g, const float *W, const float *bias, float *out, int B, int Cin,
                     int Cout, void *stream);
int mbv_op_gather_rows(mbv_model *m, const float *table, const int64_t *sid, float *out, int B, int C, int n_rows,
                       int32_t *bad, void *stream);
int mbv_op_posterior_sample(mbv_model *m, const float *stats, const float *noise, const int32_t *lens, float *z,
                            int B, int I, int T, void *stream);
int mbv_op_lens(mbv_model *m, const int64_t *lengths, int32_t *lens32, int32_t *bad, float *mask, int B, int T,
                void *stream);
int mbv_op_dds_sep(mbv_model *m, const float *x, const int32_t *lens, const float *w, const float *bias,
                   const float *gamma, const float *beta, float *y, int B, int C, int T, int K, int dil, void *stream);
int mbv_op_dds_res(mbv_model *m, const float *a, const float *xres, const float *gamma, const float *beta, float *y,
                   int B, int C, int T, const int32_t *out_lens, void *stream);
int mbv_op_sdp_pre(mbv_model *m, const float *z, int zc, const float *pre_w, const float *pre_b, const float *cond,
                   float *h, int B, int C, int T, void *stream);
int mbv_op_sdp_spline(mbv_model *m, const float *h, float *z, const int32_t *lens, int B, int C, int T,
                      float edge_const, void *stream);
int mbv_op_sdp_logw(mbv_model *m, const float *z, const float *mean, const float *logs, const int32_t *lens,
                    float *logw, int B, int T, void *stream);
int mbv_op_sdp_noise(mbv_model *m, const float *noise, float scale, float *z, int64_t n, void *stream);
int mbv_op_chan_add(mbv_model *m, float *x, const float *v, int B, int C, int T, void *stream);
int mbv_op_istft_single(mbv_model *m, const float *x_post, int B, int frames, int prescaled, float *o, float *spec,
                        float *phase, void *stream);
/* the two kernels of mbv_align by themselves (align.hip).
 *   neg_cent: z_p [B, I, T_t], m_p / logs_p [B, I, T_s] (dense), t_y32 / t_x32 int32 [B] -> value [B, T_t, T_s]
 *             (cells outside [t_y, t_x) are not written; lengths are clamped to the tensors)
 *   max_path: value is left untouched and not read outside [t_y, t_x); w_out int32 [B, T_s]; path_out int32
 *             [B, T_t, T_s] or NULL; status int32 [B] or NULL: 0 ok, 1 t_x > t_y, 2 t_x < 1 or t_y < 1,
 *             3 a length outside the tensors (such rows: w = 0, path = 0).  T_s <= 1024. */
int mbv_op_neg_cent(mbv_model *m, const float *z_p, const float *m_p, const float *logs_p, const int32_t *t_y32,
                    const int32_t *t_x32, float *value, int B, int I, int T_t, int T_s, void *stream);
int mbv_op_max_path(mbv_model *m, const float *value, const int32_t *t_y32, const int32_t *t_x32, int32_t *w_out,
                    int32_t *path_out, int32_t *status, int B, int T_t, int T_s, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MBISTFT_VITS_H */
