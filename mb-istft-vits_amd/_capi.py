"""ctypes binding of `include/mbistft_vits.h` (the C-ABI of the HIP path).

There is deliberately no fallback: if the shared library is missing or a call
fails, an exception is raised.
"""
import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
# MBV_LIB: another build of the same library (A/B measurements of compile-time switches, scripts/stage_ab.py)
LIB_PATH = os.environ.get("MBV_LIB") or os.path.join(CSRC, "libmbistft_vits.so")

ABI_VERSION = 3             # MBV_ABI_VERSION of include/mbistft_vits.h


class MbvConfig(C.Structure):
    _fields_ = [
        ("struct_bytes", C.c_int32), ("n_vocab", C.c_int32), ("inter_channels", C.c_int32),
        ("hidden_channels", C.c_int32), ("filter_channels", C.c_int32), ("n_heads", C.c_int32),
        ("n_layers", C.c_int32), ("kernel_size", C.c_int32),
        ("upsample_initial_channel", C.c_int32), ("spec_channels", C.c_int32),
        ("resblock_kernel_sizes", C.c_int32 * 3), ("resblock_dilations", (C.c_int32 * 3) * 3),
        ("resblock_type", C.c_int32),
        ("n_speakers", C.c_int32), ("gin_channels", C.c_int32), ("decoder", C.c_int32),
        ("device", C.c_int32), ("use_sdp", C.c_int32),
    ]


class MbvOutputs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in
                ("o", "o_mb", "spec", "phase", "attn", "y_mask", "z", "z_p", "m_p", "logs_p")]


class MbvChunk(C.Structure):
    """mbv_chunk of include/mbistft_vits.h (mbv_decode_chunks)."""
    _fields_ = [("z", C.c_void_p), ("z_stride", C.c_int64), ("g", C.c_void_p), ("t_frames", C.c_int32),
                ("first", C.c_int32), ("count", C.c_int32), ("o", C.c_void_p)]


class MbvPcmChunk(C.Structure):
    """mbv_pcm_chunk of include/mbistft_vits.h (mbv_resample_pcm16_chunks)."""
    _fields_ = [("wave", C.c_void_p), ("in_total", C.c_int64), ("valid_samples", C.c_void_p),
                ("in_avail", C.c_int64), ("out_first", C.c_int64), ("out_count", C.c_int64), ("peak", C.c_void_p),
                ("pcm", C.c_void_p), ("pcm_capacity", C.c_int64), ("running_peak", C.c_void_p),
                ("out_samples", C.c_void_p)]


class MbvPcmLimit(C.Structure):
    """mbv_pcm_limit of include/mbistft_vits.h (the limited wire entries); ceiling 0 = this chunk has no limiter."""
    _fields_ = [("ceiling", C.c_float), ("lookahead", C.c_int32), ("hold", C.c_int32)]


class MbvPcmFade(C.Structure):
    """mbv_pcm_fade of include/mbistft_vits.h (the faded wire entries); count < 0 = this chunk has no fade."""
    _fields_ = [("first", C.c_int64), ("count", C.c_int64), ("inv", C.c_float)]


def pcm_fade(first, count):
    """`mbv_pcm_fade_make` (host only): the `MbvPcmFade` of (first, count), `inv` included; ValueError when refused."""
    f = MbvPcmFade()
    if lib().mbv_pcm_fade_make(int(first), int(count), C.byref(f)):
        raise ValueError("a fade is (first, count) with first >= 0 and count >= 0, got (%r, %r)" % (first, count))
    return f


NO_FADE = (0, -1, 0.0)          # the fields of a table row that does not fade


class MbvTurnSeg(C.Structure):
    """mbv_turn_seg of include/mbistft_vits.h (mbv_resample_turns): one utterance on a turn's timeline."""
    _fields_ = [("wave", C.c_void_p), ("start", C.c_int64), ("length", C.c_int64), ("ramp", C.c_int32)]


class MbvTurnChunk(C.Structure):
    """mbv_turn_chunk of include/mbistft_vits.h (mbv_resample_turns); chunk.wave stays None."""
    _fields_ = [("chunk", MbvPcmChunk), ("segs", C.POINTER(MbvTurnSeg)), ("n_segs", C.c_int32)]


TURN_MAX_SEGS = 4096            # MBV_TURN_MAX_SEGS


class MbvMarkRow(C.Structure):
    """mbv_mark_row of include/mbistft_vits.h (mbv_token_marks_rows); marks None = this row has none."""
    _fields_ = [("marks", C.c_void_p), ("count", C.c_int32), ("reserved", C.c_int32)]


class MbvFit(C.Structure):
    """mbv_fit of include/mbistft_vits.h (the prosody entries); frames 0 = this row is not fitted."""
    _fields_ = [("frames", C.c_int64), ("lo", C.c_float), ("hi", C.c_float)]


class MbvShapeRow(C.Structure):
    """mbv_shape_row of include/mbistft_vits.h (mbv_shape_durations_rows); all None / 0 = this row keeps its durations."""
    _fields_ = [("scale", C.c_void_p), ("extra", C.c_void_p), ("fit", MbvFit), ("fit_out", C.c_void_p)]


class MbvGainRow(C.Structure):
    """mbv_gain_row of include/mbistft_vits.h (mbv_frame_gain_rows); all None / 0 = this row carries no gain."""
    _fields_ = [("gain", C.c_void_p), ("out", C.c_void_p), ("frames", C.c_int32), ("reserved", C.c_int32)]


class MbvPcmEnvelope(C.Structure):
    """mbv_pcm_envelope of include/mbistft_vits.h (the shaped wire entries); gain None (all zero) = no envelope."""
    _fields_ = [("gain", C.c_void_p), ("frames", C.c_int64), ("hop", C.c_int32), ("inv_hop", C.c_float)]


class MbvWarpRow(C.Structure):
    """mbv_warp_row of include/mbistft_vits.h (mbv_warp_ranges): U / rate on the device, U_host / rate_host their host
    copies."""
    _fields_ = [("wave", C.c_void_p), ("samples", C.c_int64), ("in_avail", C.c_int64), ("U", C.c_void_p),
                ("rate", C.c_void_p), ("U_host", C.c_void_p), ("rate_host", C.c_void_p), ("frames", C.c_int32),
                ("hop", C.c_int32), ("envelope", MbvPcmEnvelope), ("out_first", C.c_int64), ("out_count", C.c_int64),
                ("out", C.c_void_p), ("out_capacity", C.c_int64), ("res_type", C.c_int32), ("reserved", C.c_int32)]


PITCH_MIN, PITCH_MAX = 0.5, 2.0     # MBV_PITCH_MIN / MBV_PITCH_MAX


SPEAKER_SLOTS, BLEND_MAX = 256, 16  # MBV_SPEAKER_SLOTS / MBV_BLEND_MAX


class MbvSpeakerDef(C.Structure):
    """mbv_speaker_def of include/mbistft_vits.h (mbv_speakers_define); vector None = a blend of `count` terms."""
    _fields_ = [("slot", C.c_int32), ("count", C.c_int32), ("ids", C.c_int32 * BLEND_MAX),
                ("weights", C.c_float * BLEND_MAX), ("vector", C.c_void_p)]


def fit_result(word):
    """One int64 of a read-back that holds an `mbv_fit_result` -> (scale, status)."""
    import struct
    return struct.unpack("<fi", struct.pack("<q", int(word)))


class MbvLoudnessChunk(C.Structure):
    """mbv_loudness_chunk of include/mbistft_vits.h (mbv_loudness_chunks)."""
    _fields_ = [("wave", C.c_void_p), ("in_total", C.c_int64), ("valid_samples", C.c_void_p), ("in_avail", C.c_int64),
                ("seg_first", C.c_int64), ("seg_count", C.c_int64), ("state", C.c_void_p), ("energies", C.c_void_p),
                ("energy_capacity", C.c_int64), ("loudness", C.c_void_p)]


def kweighting(rate):
    """`mbv_kweighting` (host only) -> (coeffs, M): the ten K-weighting coefficients of `rate` (shelf b0 b1 b2 a1 a2,
    high-pass b0 b1 b2 a1 a2) and the 4 x 4 H-step transition matrix, row-major, as float64 lists; ValueError when
    the rate is refused."""
    c, m = (C.c_double * 10)(), (C.c_double * 16)()
    if lib().mbv_kweighting(int(rate), c, m):
        raise ValueError((lib().mbv_last_error(None) or b"mbv_kweighting failed").decode())
    return list(c), list(m)


def loudness_segments(rate, samples):
    """`mbv_loudness_segments` (host only, pure integers) -> (H, samples // H); ValueError when refused."""
    hop = C.c_int32()
    n = lib().mbv_loudness_segments(int(rate), int(samples), C.byref(hop))
    if n < 0:
        raise ValueError((lib().mbv_last_error(None) or b"mbv_loudness_segments failed").decode())
    return int(hop.value), int(n)


class MbvEncRow(C.Structure):
    """mbv_enc_row of include/mbistft_vits.h (mbv_encode_rows)."""
    _fields_ = [("length_scale", C.c_float), ("noise_scale_w", C.c_float), ("noise_w", C.c_void_p),
                ("durations", C.c_void_p), ("durations_dtype", C.c_int32), ("t_text", C.c_int32)]


class MbvRow(C.Structure):
    """mbv_row of include/mbistft_vits.h (mbv_synthesize_rows)."""
    _fields_ = [("noise", C.c_void_p), ("noise_stride", C.c_int64), ("noise_scale", C.c_float), ("keep", C.c_int32),
                ("z", C.c_void_p)]


class MbvConvertRow(C.Structure):
    """mbv_convert_row of include/mbistft_vits.h (mbv_convert_rows)."""
    _fields_ = [("wave", C.c_void_p), ("samples", C.c_int64), ("wave_dtype", C.c_int32), ("sid_src", C.c_int32),
                ("sid_tgt", C.c_int32), ("noise", C.c_void_p), ("noise_scale", C.c_float), ("z", C.c_void_p)]


class MbvConvertRange(C.Structure):
    """mbv_convert_range of include/mbistft_vits.h (mbv_convert_ranges)."""
    _fields_ = [("wave", C.c_void_p), ("arrived", C.c_int64), ("closed", C.c_int32), ("wave_dtype", C.c_int32),
                ("sid_src", C.c_int32), ("sid_tgt", C.c_int32), ("first", C.c_int32), ("count", C.c_int32),
                ("noise", C.c_void_p), ("noise_stride", C.c_int64), ("noise_scale", C.c_float), ("z", C.c_void_p),
                ("z_stride", C.c_int64)]


class MbvSeamRow(C.Structure):
    """mbv_seam_row of include/mbistft_vits.h (mbv_seam_rows)."""
    _fields_ = [("o", C.c_void_p), ("o_samples", C.c_int64), ("head_first", C.c_int64), ("over_first", C.c_int64),
                ("stash", C.c_void_p), ("head_count", C.c_int32), ("over_count", C.c_int32), ("seam", C.c_int32),
                ("reserved", C.c_int32)]


class MbvTakeRow(C.Structure):
    """mbv_take_row of include/mbistft_vits.h (mbv_take_tokens_rows)."""
    _fields_ = [("src", C.c_int32), ("a", C.c_int32), ("b", C.c_int32), ("reserved", C.c_int32),
                ("y_length", C.c_void_p), ("stats", C.c_void_p), ("dur", C.c_void_p), ("stride", C.c_int64),
                ("dur_copy", C.c_void_p)]


class MbvExpandRange(C.Structure):
    """mbv_expand_range of include/mbistft_vits.h (mbv_expand_ranges); dur_host is HOST memory."""
    _fields_ = [("stats", C.c_void_p), ("dur", C.c_void_p), ("stride", C.c_int64), ("dur_host", C.c_void_p),
                ("a", C.c_int32), ("b", C.c_int32), ("frame", C.c_int32), ("max_frames", C.c_int32),
                ("noise", C.c_void_p), ("noise_stride", C.c_int64), ("noise_scale", C.c_float),
                ("reserved", C.c_int32), ("z_p", C.c_void_p), ("z_stride", C.c_int64)]


class MbvFlowRange(C.Structure):
    """mbv_flow_range of include/mbistft_vits.h (mbv_flow_ranges)."""
    _fields_ = [("z_p", C.c_void_p), ("z_p_stride", C.c_int64), ("P", C.c_int32), ("complete", C.c_int32),
                ("sid", C.c_int64), ("first", C.c_int32), ("count", C.c_int32), ("z", C.c_void_p),
                ("z_stride", C.c_int64)]


class MbvResampleRange(C.Structure):
    """mbv_resample_range of include/mbistft_vits.h (mbv_resample_ranges)."""
    _fields_ = [("wave", C.c_void_p), ("wave_dtype", C.c_int32), ("in_avail", C.c_int64), ("in_total", C.c_int64),
                ("out_first", C.c_int64), ("out_count", C.c_int64), ("out", C.c_void_p), ("out_capacity", C.c_int64)]


class MbvRandnBlock(C.Structure):
    """mbv_randn_block of include/mbistft_vits.h (mbv_randn_blocks)."""
    _fields_ = [("dst", C.c_void_p), ("stride", C.c_int64), ("channels", C.c_int32), ("reserved", C.c_int32),
                ("first", C.c_int64), ("count", C.c_int64), ("seed", C.c_uint64), ("purpose", C.c_uint32),
                ("row", C.c_uint32)]


# MBV_G711_* / MBV_WAVE_* of include/mbistft_vits.h: the codec of a G.711 wire entry; the dtype of a raw recording
G711_LAWS = {"ulaw": 1, "alaw": 2}
WAVE_F32, WAVE_PCM16, WAVE_ULAW, WAVE_ALAW = 0, 1, 8, 9


# MBV_RESAMPLE_* of include/mbistft_vits.h, by librosa.resample's res_type: the filters of the warp and the wire
RESAMPLE_TYPES = {"kaiser_best": 0, "kaiser_fast": 1}


# MBV_NOISE_* of include/mbistft_vits.h: the `purpose` word of the generator's counter
NOISE_PRIOR, NOISE_SDP, NOISE_POSTERIOR = 0, 1, 2


class MbvAlignOutputs(C.Structure):
    """mbv_align_outputs of include/mbistft_vits.h: NULL = not wanted."""
    _fields_ = [(n, C.c_void_p) for n in
                ("w", "attn", "x_mask", "y_mask", "z", "z_p", "m_p", "logs_p", "neg_cent")]


class MbvConvDesc(C.Structure):
    """mbv_conv_desc of include/mbistft_vits.h (mbv_op_conv / mbv_conv_plan)."""
    _fields_ = [(n, C.c_int32) for n in ("B", "Cin", "Cout", "Tin", "T", "K", "dil", "x_rstride", "kind", "epi")] + [
        ("in_slope", C.c_float), ("relu", C.c_int32), ("reflect1", C.c_int32),
        ("in_lens", C.c_void_p), ("out_lens", C.c_void_p), ("chan_add", C.c_void_p), ("res", C.c_void_p),
        ("res_chan_add", C.c_void_p), ("accum_in", C.c_void_p), ("out_scale", C.c_float),
        ("trim_lens", C.c_void_p), ("trim_num", C.c_int32), ("trim_add", C.c_int32),
        ("splitk", C.c_int32), ("prec", C.c_int32), ("legacy_convt", C.c_int32),
        ("ws_floats", C.c_int64), ("n_counters", C.c_int32),
        ("ln_gamma", C.c_void_p), ("ln_beta", C.c_void_p), ("ln_out_lens", C.c_void_p),
        ("tail_once", C.c_int32),
    ]


# MBV_CONV_KIND_* / MBV_CONV_EPI_* / MBV_ROUTE_* of include/mbistft_vits.h
CONV_KIND_CONV, CONV_KIND_CONVT4, CONV_KIND_CONVT8 = 0, 4, 8
CONV_EPI_STORE, CONV_EPI_RESID, CONV_EPI_RESID_ACC, CONV_EPI_LN = 0, 1, 2, 7
ROUTES = {1: "NARROW_M", 2: "NARROW_LAUNCH", 3: "M64", 4: "HALF", 5: "SMALL", 6: "BIG", 7: "SPLIT_BATCH", 8: "VS",
          9: "TAIL_PACK"}
PLAN_FIELDS = ("route", "bm", "bn", "threads", "ck", "nb_big", "vs_tv", "S")


# the header's structs by their C names (mbv_model is opaque; mbv_fit_result has no class: `fit_result` unpacks it)
STRUCTS = {
    "mbv_config": MbvConfig, "mbv_outputs": MbvOutputs, "mbv_chunk": MbvChunk, "mbv_enc_row": MbvEncRow,
    "mbv_row": MbvRow, "mbv_speaker_def": MbvSpeakerDef, "mbv_align_outputs": MbvAlignOutputs,
    "mbv_pcm_chunk": MbvPcmChunk, "mbv_pcm_limit": MbvPcmLimit, "mbv_resample_range": MbvResampleRange,
    "mbv_pcm_fade": MbvPcmFade, "mbv_turn_seg": MbvTurnSeg, "mbv_turn_chunk": MbvTurnChunk,
    "mbv_mark_row": MbvMarkRow, "mbv_fit": MbvFit, "mbv_shape_row": MbvShapeRow, "mbv_gain_row": MbvGainRow,
    "mbv_pcm_envelope": MbvPcmEnvelope, "mbv_warp_row": MbvWarpRow, "mbv_loudness_chunk": MbvLoudnessChunk,
    "mbv_randn_block": MbvRandnBlock, "mbv_convert_row": MbvConvertRow, "mbv_convert_range": MbvConvertRange,
    "mbv_seam_row": MbvSeamRow, "mbv_conv_desc": MbvConvDesc, "mbv_take_row": MbvTakeRow,
    "mbv_expand_range": MbvExpandRange, "mbv_flow_range": MbvFlowRange,
}


# Every function include/mbistft_vits.h declares: name -> (restype, argtypes); tests/test_capi_header.py holds each
# entry to its prototype.  vp stands for every pointer the caller passes as an address (device or host memory, the
# model handle, the stream); a pointer to a struct or to a fixed array is spelled out.
P, vp, cstr = C.POINTER, C.c_void_p, C.c_char_p
i32, i64, u32, u64, f32, f64 = C.c_int, C.c_int64, C.c_uint32, C.c_uint64, C.c_float, C.c_double

# what every build has to export, a MBV_LIB baseline included
CORE = {
    "mbv_abi_version": (i32, []),
    "mbv_create": (i32, [P(MbvConfig), P(vp)]),
    "mbv_destroy": (None, [vp]),
    "mbv_last_error": (cstr, [vp]),
    "mbv_load_weight": (i32, [vp, cstr, vp, P(i64), i32]),
    "mbv_finalize_weights": (i32, [vp, vp]),
    "mbv_missing_weights": (i32, [vp, cstr, C.c_size_t]),
    "mbv_encode": (i32, [vp, vp, vp, vp, i32, i32, f32, vp, f32, vp, vp]),
    "mbv_synthesize": (i32, [vp, i32, vp, f32, i32, P(MbvOutputs), vp]),
    "mbv_decode": (i32, [vp, vp, vp, i32, i32, P(MbvOutputs), vp]),
    "mbv_speaker_embedding": (i32, [vp, vp, i32, vp, vp]),
    "mbv_stage_times_ms": (i32, [vp, P(f32 * 5)]),
    "mbv_istft_pqmf": (i32, [vp, vp, i32, i32, vp, i32, vp, vp, vp, vp, vp]),
    "mbv_read_stage": (i64, [vp, cstr, vp, i64, vp]),
    "mbv_op_conv1d": (i32, [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, f32, vp]),
    "mbv_kernel_times_ms": (i32, [vp, P(f32 * 2)]),
    "mbv_istft_finalize": (i32, [vp, vp, vp, i32, i32, vp, vp, vp]),
    "mbv_pcm16": (i32, [vp, vp, vp, i32, i64, i32, vp, vp]),
    "mbv_voice_conversion": (i32, [vp, vp, vp, vp, vp, i32, i32, vp, P(MbvOutputs), vp, vp]),
    "mbv_set_option": (i32, [vp, cstr, i32]),
    "mbv_arena_floats": (i64, [vp]),
    "mbv_export_arena": (i32, [vp, vp, i64, vp]),
    "mbv_import_arena": (i32, [vp, vp, i64, vp]),
    "mbv_ticket": (i64, [vp]),
    "mbv_stage_times_ms_at": (i32, [vp, i64, P(f32 * 5)]),
    "mbv_op_rel_attention": (i32, [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp]),
    "mbv_pcm16_samples": (i32, [vp, vp, vp, i32, i64, i32, vp, vp]),
    "mbv_resample": (i32, [vp, vp, vp, i32, i64, i32, i32, i32, vp, i64, vp, vp]),
    "mbv_resample_bank": (i32, [i32, i32, i32, vp, i64, P(i32), P(i32), P(i32)]),
    "mbv_op_conv": (i32, [vp, P(MbvConvDesc), vp, vp, vp, vp, vp, vp]),     # plan_out: `int32_t *`, 8 values or NULL
    "mbv_conv_plan": (i32, [P(MbvConvDesc), P(i32 * 8)]),
    "mbv_spectrogram": (i32, [vp, vp, i32, vp, i32, i64, i32, i32, i32, vp, i64, vp, vp]),
    "mbv_spectrogram_frames": (i64, [i64, i32, i32]),
    "mbv_decoder_context": (i32, [P(MbvConfig), P(i32 * 2)]),
    "mbv_decode_range": (i32, [vp, vp, vp, i32, i32, i32, i32, vp, i64, vp]),
    "mbv_resample_ready": (i64, [i32, i32, i32, i64, i64]),
    "mbv_resample_pcm16_range": (i32, [vp, vp, vp, i32, i64, i32, i32, i32, i64, i64, i64, vp, vp, i64, vp, vp, vp]),
    "mbv_op_embed": (i32, [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp]),
    "mbv_op_layernorm": (i32, [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp, vp]),
    "mbv_op_durations": (i32, [vp, vp, vp, vp, vp, f32, vp, vp, vp, vp, vp, vp, i32, i32, i32, vp]),
    "mbv_op_expand": (i32, [vp, vp, vp, vp, vp, f32, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp]),
    "mbv_op_cond_gemv": (i32, [vp, vp, vp, vp, vp, i32, i32, i32, vp]),
    "mbv_op_gather_rows": (i32, [vp, vp, vp, vp, i32, i32, i32, vp, vp]),
    "mbv_op_posterior_sample": (i32, [vp, vp, vp, vp, vp, i32, i32, i32, vp]),
    "mbv_op_lens": (i32, [vp, vp, vp, vp, vp, i32, i32, vp]),
    "mbv_op_dds_sep": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp]),
    "mbv_op_dds_res": (i32, [vp, vp, vp, vp, vp, vp, i32, i32, i32, vp, vp]),
    "mbv_op_sdp_pre": (i32, [vp, vp, i32, vp, vp, vp, vp, i32, i32, i32, vp]),
    "mbv_op_sdp_spline": (i32, [vp, vp, vp, vp, i32, i32, i32, f32, vp]),
    "mbv_op_sdp_logw": (i32, [vp, vp, vp, vp, vp, vp, i32, i32, vp]),
    "mbv_op_sdp_noise": (i32, [vp, vp, f32, vp, i64, vp]),
    "mbv_op_chan_add": (i32, [vp, vp, vp, i32, i32, i32, vp]),
    "mbv_op_istft_single": (i32, [vp, vp, i32, i32, i32, vp, vp, vp, vp]),
    "mbv_align": (i32, [vp, vp, vp, vp, vp, vp, i32, i32, i32, vp, f32, P(MbvAlignOutputs), vp, vp]),
    "mbv_set_durations": (i32, [vp, vp, i32, i32, i32, vp, vp]),
    "mbv_op_neg_cent": (i32, [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp]),
    "mbv_op_max_path": (i32, [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, vp]),
}
# what came after the row-exact ragged decode (the first baseline of the scripts/*_timing.py A/B runs): a MBV_LIB build
# may lack any of these, and calling one it lacks raises AttributeError.  New entries go here.
LATER = {
    "mbv_ragged_classes": (i32, [P(MbvConfig), i32, i32, P(i32), i32]),
    "mbv_decode_ragged": (i32, [vp, vp, vp, i32, i32, P(i64), vp, vp]),
    "mbv_synthesize_ragged": (i32, [vp, i32, vp, f32, i32, P(MbvOutputs), P(i64), vp]),
    "mbv_ragged_plan": (i32, [P(MbvConfig), i32, i32, i32, P(i64), P(i32)]),
    "mbv_chunks_plan": (i32, [P(MbvConfig), i32, i32, P(i32), P(i32)]),
    "mbv_decode_chunks": (i32, [vp, P(MbvChunk), i32, vp]),
    "mbv_decoder_runs": (i64, [vp]),
    "mbv_pcm_chunks_plan": (i64, [i32, i32, i32, P(MbvPcmChunk), i32, P(i64)]),
    "mbv_resample_pcm16_chunks": (i32, [vp, P(MbvPcmChunk), i32, i32, i32, i32, vp, i64, vp]),
    "mbv_wire_runs": (i64, [vp]),
    "mbv_admit_plan": (i32, [P(MbvConfig), i32, i32, P(i32), P(i32)]),
    "mbv_encode_rows": (i32, [vp, i32, vp, vp, vp, i32, i32, P(MbvEncRow), vp, vp]),
    "mbv_synthesize_rows": (i32, [vp, i32, i32, P(MbvRow), i32, vp]),
    "mbv_encoder_runs": (i64, [vp]),
    "mbv_get_option": (i32, [vp, cstr]),
    "mbv_tail_plan": (i32, [P(MbvConfig), P(i32), i32]),
    "mbv_tail_dropped": (i64, [vp]),
    "mbv_decode_masked": (i32, [vp, vp, vp, vp, i32, i32, P(MbvOutputs), vp]),
    "mbv_tail_pack_table": (i32, [P(i64), i32, i32, i32, i32, i32, i32, i32, P(i32), i64]),
    "mbv_convert_plan": (i32, [P(MbvConfig), i32, i32, P(i32), P(i32)]),
    "mbv_convert_rows": (i32, [vp, P(MbvConvertRow), i32, i32, i32, i32, vp, vp]),
    "mbv_converter_runs": (i64, [vp]),
    "mbv_decode_chunks_routed": (i32, [vp, P(MbvChunk), P(i32), i32, vp]),
    "mbv_converter_context": (i32, [P(MbvConfig), P(i32 * 2)]),
    "mbv_spectrogram_ready": (i64, [i64, i32, i32, i32]),
    "mbv_convert_window": (i32, [P(MbvConfig), i32, i32, i64, P(i32 * 2)]),
    "mbv_convert_ranges_plan": (i32, [P(MbvConfig), i32, P(i32), P(i32)]),
    "mbv_convert_ranges": (i32, [vp, P(MbvConvertRange), i32, i32, i32, vp]),
    "mbv_resample_ready_open": (i64, [i32, i32, i32, i64]),
    "mbv_resample_ranges": (i32, [vp, P(MbvResampleRange), i32, i32, i32, i32, vp]),
    "mbv_input_runs": (i64, [vp]),
    "mbv_randn_blocks": (i32, [vp, P(MbvRandnBlock), i32, vp]),
    "mbv_randn_host": (i32, [u64, u32, u32, u32, i64, i64, vp]),
    "mbv_noise_runs": (i64, [vp]),
    "mbv_limiter_ready": (i64, [i32, i32, i32, i64, i64, i32]),
    "mbv_resample_pcm16_range_limited": (i32, [vp, vp, vp, i32, i64, i32, i32, i32, i64, i64, i64, vp, vp, i64, vp, vp,
                                               P(MbvPcmLimit), vp]),
    "mbv_resample_pcm16_chunks_limited": (i32, [vp, P(MbvPcmChunk), P(MbvPcmLimit), i32, i32, i32, i32, vp, i64, vp]),
    "mbv_g711_encode": (i32, [vp, vp, i64, i32, vp, vp]),
    "mbv_g711_decode": (i32, [vp, vp, i64, i32, vp, vp]),
    "mbv_resample_g711_range": (i32, [vp, vp, vp, i32, i64, i32, i32, i32, i64, i64, i64, vp, vp, i64, vp, vp,
                                      P(MbvPcmLimit), i32, vp]),
    "mbv_resample_g711_chunks": (i32, [vp, P(MbvPcmChunk), P(MbvPcmLimit), i32, i32, i32, i32, i32, vp, i64, vp]),
    "mbv_pcm_fade_make": (i32, [i64, i64, P(MbvPcmFade)]),
    "mbv_resample_pcm16_range_faded": (i32, [vp, vp, vp, i32, i64, i32, i32, i32, i64, i64, i64, vp, vp, i64, vp, vp,
                                             P(MbvPcmLimit), P(MbvPcmFade), vp]),
    "mbv_resample_pcm16_chunks_faded": (i32, [vp, P(MbvPcmChunk), P(MbvPcmLimit), P(MbvPcmFade), i32, i32, i32, i32, vp,
                                              i64, vp]),
    "mbv_resample_g711_range_faded": (i32, [vp, vp, vp, i32, i64, i32, i32, i32, i64, i64, i64, vp, vp, i64, vp, vp,
                                            P(MbvPcmLimit), i32, P(MbvPcmFade), vp]),
    "mbv_resample_g711_chunks_faded": (i32, [vp, P(MbvPcmChunk), P(MbvPcmLimit), P(MbvPcmFade), i32, i32, i32, i32, i32,
                                             vp, i64, vp]),
    "mbv_token_marks": (i32, [vp, vp, i64, vp]),
    "mbv_token_marks_rows": (i32, [vp, i32, P(MbvMarkRow), i32, vp]),
    "mbv_kweighting": (i32, [i32, P(f64), P(f64)]),
    "mbv_loudness_segments": (i64, [i32, i64, P(i32)]),
    "mbv_loudness": (i32, [vp, vp, vp, i32, i64, i32, vp, vp, vp]),
    "mbv_loudness_range": (i32, [vp, vp, vp, i32, i64, i32, i64, i64, i64, vp, vp, i64, vp, vp]),
    "mbv_loudness_chunks": (i32, [vp, P(MbvLoudnessChunk), i32, i32, vp]),
    "mbv_loudness_runs": (i64, [vp]),
    "mbv_turn_plan": (i64, [i32, i32, i32, P(MbvTurnChunk), P(MbvPcmLimit), i32, P(i64)]),
    "mbv_resample_turns": (i32, [vp, P(MbvTurnChunk), P(MbvPcmLimit), P(MbvPcmFade), i32, i32, i32, i32, i32, vp, i64,
                                 vp]),
    "mbv_shape_durations": (i32, [vp, vp, vp, P(MbvFit), i32, i32, vp, vp, vp]),
    "mbv_shape_durations_rows": (i32, [vp, i32, P(MbvShapeRow), i32, vp, vp]),
    "mbv_op_shape_durations": (i32, [vp, vp, vp, vp, vp, f32, P(MbvFit), vp, vp, vp, vp, vp, vp, i32, i32, vp]),
    "mbv_shape_runs": (i64, [vp]),
    "mbv_frame_gain": (i32, [vp, vp, vp, i64, i32, vp]),
    "mbv_frame_gain_rows": (i32, [vp, i32, P(MbvGainRow), i32, vp]),
    "mbv_op_frame_gain": (i32, [vp, vp, vp, vp, vp, i64, i32, i32, i32, vp]),
    "mbv_gain_runs": (i64, [vp]),
    "mbv_resample_pcm16_range_shaped": (i32, [vp, vp, vp, i32, i64, i32, i32, i32, i64, i64, i64, vp, vp, i64, vp, vp,
                                              P(MbvPcmLimit), i32, P(MbvPcmFade), P(MbvPcmEnvelope), i64, vp]),
    "mbv_resample_pcm16_chunks_shaped": (i32, [vp, P(MbvPcmChunk), P(MbvPcmLimit), P(MbvPcmFade), P(MbvPcmEnvelope),
                                               i32, i32, i32, i32, i32, vp, i64, vp]),
    "mbv_resample_turns_shaped": (i32, [vp, P(MbvTurnChunk), P(MbvPcmLimit), P(MbvPcmFade), P(MbvPcmEnvelope), i32, i32,
                                        i32, i32, i32, vp, i64, vp]),
    "mbv_warp_plan": (i32, [i32, i64, vp, vp, P(i64)]),
    "mbv_warp_ready": (i64, [i32, i64, vp, vp, i32, i64]),
    "mbv_warp_ranges": (i32, [vp, P(MbvWarpRow), i32, vp]),
    "mbv_warp_runs": (i64, [vp]),
    "mbv_speakers_define": (i32, [vp, P(MbvSpeakerDef), i32, vp]),
    "mbv_speaker_release": (i32, [vp, i32, vp]),
    "mbv_speaker_slots": (i32, []),
    "mbv_speaker_defined": (i32, [vp, i64]),
    "mbv_speaker_runs": (i64, [vp]),
    "mbv_convert_window_ahead": (i32, [P(MbvConfig), i32, i32, i32, i64, P(i32 * 2)]),
    "mbv_convert_ranges_ahead": (i32, [vp, P(MbvConvertRange), P(i32), i32, i32, i32, vp]),
    "mbv_seam_rows": (i32, [vp, P(MbvSeamRow), i32, vp]),
    "mbv_seam_runs": (i64, [vp]),
    "mbv_text_context": (i32, [P(MbvConfig), P(i32 * 2)]),
    "mbv_flow_window": (i32, [P(MbvConfig), i32, i32, i64, P(i32 * 2)]),
    "mbv_flow_ranges_plan": (i32, [P(MbvConfig), i32, P(i32), P(i32)]),
    "mbv_take_tokens_rows": (i32, [vp, i32, P(MbvTakeRow), i32, vp]),
    "mbv_expand_ranges": (i32, [vp, P(MbvExpandRange), i32, vp]),
    "mbv_flow_ranges": (i32, [vp, P(MbvFlowRange), i32, vp]),
    "mbv_text_runs": (i64, [vp]),
    "mbv_flow_runs": (i64, [vp]),
}
TABLE = {**CORE, **LATER}
SYMBOLS = list(TABLE)


def declare(L, allow_missing):
    """Give every entry of TABLE that `L` has its restype and argtypes.  A CORE entry must be there; so must a LATER
    one unless `allow_missing`: an absent one is then left undeclared (AttributeError here, or at the call)."""
    for name, (restype, argtypes) in TABLE.items():
        if allow_missing and name in LATER and not hasattr(L, name):
            continue
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes


def build(force=False, verbose=False):
    """Compile the HIP sources for gfx950 in-tree (`csrc/build.sh`)."""
    if force:
        for f in os.listdir(CSRC):
            if f.endswith(".o") or f.endswith(".so"):
                os.remove(os.path.join(CSRC, f))
    r = subprocess.run(["bash", os.path.join(CSRC, "build.sh")], capture_output=True, text=True)
    if verbose or r.returncode:
        print(r.stdout, r.stderr)
    if r.returncode:
        raise RuntimeError("building libmbistft_vits.so failed:\n" + r.stderr[-4000:])
    return LIB_PATH


_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.isfile(LIB_PATH):
        raise RuntimeError("%s not found: build it with `python -c 'import __graft_entry__ as g; "
                           "g.build()'` (hipcc, gfx950). There is no CPU fallback." % LIB_PATH)
    # torch first: it ships its own libamdhip64; loading this library before torch would bring in the
    # system HIP runtime as a second instance, which then sees no device ("no HIP device visible")
    import torch  # noqa: F401
    L = C.CDLL(LIB_PATH)
    # the in-tree library must match the whole header; only a MBV_LIB baseline may lack LATER entries
    declare(L, allow_missing=bool(os.environ.get("MBV_LIB")))
    if L.mbv_abi_version() != ABI_VERSION:
        raise RuntimeError("libmbistft_vits.so ABI version mismatch")
    _lib = L
    return L


class MbvError(RuntimeError):
    pass


def check(handle, rc, what):
    if rc:
        msg = lib().mbv_last_error(handle)
        raise MbvError("%s failed: %s" % (what, msg.decode() if msg else "unknown error"))
