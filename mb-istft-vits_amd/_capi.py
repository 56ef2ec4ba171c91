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

# every symbol include/mbistft_vits.h declares
SYMBOLS = [
    "mbv_abi_version", "mbv_create", "mbv_destroy", "mbv_last_error", "mbv_load_weight",
    "mbv_finalize_weights", "mbv_missing_weights", "mbv_encode", "mbv_synthesize", "mbv_decode",
    "mbv_speaker_embedding", "mbv_stage_times_ms", "mbv_istft_pqmf", "mbv_read_stage",
    "mbv_op_conv1d", "mbv_kernel_times_ms", "mbv_istft_finalize", "mbv_pcm16", "mbv_voice_conversion",
    "mbv_set_option", "mbv_arena_floats", "mbv_export_arena", "mbv_import_arena", "mbv_ticket", "mbv_stage_times_ms_at", "mbv_op_rel_attention",
    "mbv_pcm16_samples", "mbv_resample", "mbv_resample_bank", "mbv_op_conv", "mbv_conv_plan",
    "mbv_spectrogram", "mbv_spectrogram_frames", "mbv_decoder_context", "mbv_decode_range",
    "mbv_resample_ready", "mbv_resample_pcm16_range",
    "mbv_ragged_classes", "mbv_decode_ragged", "mbv_synthesize_ragged", "mbv_ragged_plan",
    "mbv_chunks_plan", "mbv_decode_chunks", "mbv_decoder_runs",
    "mbv_pcm_chunks_plan", "mbv_resample_pcm16_chunks", "mbv_wire_runs",
    "mbv_op_embed", "mbv_op_layernorm", "mbv_op_durations", "mbv_op_expand", "mbv_op_cond_gemv", "mbv_op_gather_rows",
    "mbv_op_posterior_sample", "mbv_op_lens", "mbv_op_dds_sep", "mbv_op_dds_res", "mbv_op_sdp_pre", "mbv_op_sdp_spline",
    "mbv_op_sdp_logw", "mbv_op_sdp_noise", "mbv_op_chan_add", "mbv_op_istft_single",
    "mbv_align", "mbv_set_durations", "mbv_op_neg_cent", "mbv_op_max_path",
    "mbv_admit_plan", "mbv_encode_rows", "mbv_synthesize_rows", "mbv_encoder_runs", "mbv_get_option",
    "mbv_tail_plan", "mbv_tail_dropped", "mbv_decode_masked", "mbv_tail_pack_table",
    "mbv_convert_plan", "mbv_convert_rows", "mbv_converter_runs",
    "mbv_decode_chunks_routed", "mbv_converter_context", "mbv_spectrogram_ready", "mbv_convert_window",
    "mbv_convert_ranges_plan", "mbv_convert_ranges",
    "mbv_resample_ready_open", "mbv_resample_ranges", "mbv_input_runs",
    "mbv_randn_blocks", "mbv_randn_host", "mbv_noise_runs",
    "mbv_limiter_ready", "mbv_resample_pcm16_range_limited", "mbv_resample_pcm16_chunks_limited",
    "mbv_g711_encode", "mbv_g711_decode", "mbv_resample_g711_range", "mbv_resample_g711_chunks",
    "mbv_pcm_fade_make", "mbv_resample_pcm16_range_faded", "mbv_resample_pcm16_chunks_faded",
    "mbv_resample_g711_range_faded", "mbv_resample_g711_chunks_faded",
    "mbv_token_marks", "mbv_token_marks_rows",
    "mbv_kweighting", "mbv_loudness_segments", "mbv_loudness", "mbv_loudness_range", "mbv_loudness_chunks",
    "mbv_loudness_runs",
    "mbv_turn_plan", "mbv_resample_turns",
    "mbv_shape_durations", "mbv_shape_durations_rows", "mbv_op_shape_durations", "mbv_shape_runs",
    "mbv_frame_gain", "mbv_frame_gain_rows", "mbv_op_frame_gain", "mbv_gain_runs",
    "mbv_resample_pcm16_range_shaped", "mbv_resample_pcm16_chunks_shaped", "mbv_resample_turns_shaped",
    "mbv_warp_plan", "mbv_warp_ready", "mbv_warp_ranges", "mbv_warp_runs",
    "mbv_speakers_define", "mbv_speaker_release", "mbv_speaker_slots", "mbv_speaker_defined", "mbv_speaker_runs",
    "mbv_convert_window_ahead", "mbv_convert_ranges_ahead", "mbv_seam_rows", "mbv_seam_runs",
]


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
    vp, i32, i64p, fp = C.c_void_p, C.c_int, C.POINTER(C.c_int64), C.c_void_p
    L.mbv_abi_version.restype = i32
    L.mbv_create.argtypes = [C.POINTER(MbvConfig), C.POINTER(vp)]
    L.mbv_destroy.argtypes = [vp]
    L.mbv_destroy.restype = None
    L.mbv_last_error.argtypes = [vp]
    L.mbv_last_error.restype = C.c_char_p
    L.mbv_load_weight.argtypes = [vp, C.c_char_p, vp, i64p, i32]
    L.mbv_finalize_weights.argtypes = [vp, vp]
    L.mbv_missing_weights.argtypes = [vp, C.c_char_p, C.c_size_t]
    L.mbv_encode.argtypes = [vp, vp, vp, vp, i32, i32, C.c_float, vp, C.c_float, vp, vp]
    L.mbv_synthesize.argtypes = [vp, i32, vp, C.c_float, i32, C.POINTER(MbvOutputs), vp]
    L.mbv_decode.argtypes = [vp, vp, vp, i32, i32, C.POINTER(MbvOutputs), vp]
    L.mbv_decoder_context.argtypes = [C.POINTER(MbvConfig), C.POINTER(C.c_int32 * 2)]
    L.mbv_decode_range.argtypes = [vp, vp, vp, i32, i32, i32, i32, vp, C.c_int64, vp]
    L.mbv_speaker_embedding.argtypes = [vp, vp, i32, vp, vp]
    L.mbv_stage_times_ms.argtypes = [vp, C.POINTER(C.c_float * 5)]
    L.mbv_kernel_times_ms.argtypes = [vp, C.POINTER(C.c_float * 2)]
    L.mbv_istft_pqmf.argtypes = [vp, vp, i32, i32, vp, i32, vp, vp, vp, vp, vp]
    L.mbv_istft_finalize.argtypes = [vp, vp, vp, i32, i32, vp, vp, vp]
    L.mbv_voice_conversion.argtypes = [vp, vp, vp, vp, vp, i32, i32, vp, C.POINTER(MbvOutputs), vp, vp]
    L.mbv_pcm16.argtypes = [vp, vp, vp, i32, C.c_int64, i32, vp, vp]
    L.mbv_pcm16_samples.argtypes = [vp, vp, vp, i32, C.c_int64, i32, vp, vp]
    L.mbv_resample.argtypes = [vp, vp, vp, i32, C.c_int64, i32, i32, i32, vp, C.c_int64, vp, vp]
    L.mbv_resample_bank.argtypes = [i32, i32, i32, vp, C.c_int64, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                    C.POINTER(C.c_int32)]
    L.mbv_resample_ready.argtypes = [i32, i32, i32, C.c_int64, C.c_int64]
    L.mbv_resample_ready.restype = C.c_int64
    L.mbv_resample_pcm16_range.argtypes = [vp, vp, vp, i32, C.c_int64, i32, i32, i32, C.c_int64, C.c_int64, C.c_int64,
                                           vp, vp, C.c_int64, vp, vp, vp]
    L.mbv_spectrogram.argtypes = [vp, vp, i32, vp, i32, C.c_int64, i32, i32, i32, vp, C.c_int64, vp, vp]
    L.mbv_spectrogram_frames.argtypes = [C.c_int64, i32, i32]
    L.mbv_spectrogram_frames.restype = C.c_int64
    L.mbv_set_option.argtypes = [vp, C.c_char_p, i32]
    L.mbv_ticket.argtypes = [vp]
    L.mbv_ticket.restype = C.c_int64
    L.mbv_stage_times_ms_at.argtypes = [vp, C.c_int64, C.POINTER(C.c_float * 5)]
    L.mbv_arena_floats.argtypes = [vp]
    L.mbv_arena_floats.restype = C.c_int64
    L.mbv_export_arena.argtypes = [vp, vp, C.c_int64, vp]
    L.mbv_import_arena.argtypes = [vp, vp, C.c_int64, vp]
    L.mbv_read_stage.argtypes = [vp, C.c_char_p, vp, C.c_int64, vp]
    L.mbv_read_stage.restype = C.c_int64
    L.mbv_op_rel_attention.argtypes = [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp]
    L.mbv_op_conv1d.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, C.c_float, vp]
    L.mbv_op_conv.argtypes = [vp, C.POINTER(MbvConvDesc), vp, vp, vp, vp, C.POINTER(C.c_int32 * 8), vp]
    L.mbv_conv_plan.argtypes = [C.POINTER(MbvConvDesc), C.POINTER(C.c_int32 * 8)]
    f32 = C.c_float
    L.mbv_op_embed.argtypes = [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp]
    L.mbv_op_layernorm.argtypes = [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp, vp]
    L.mbv_op_durations.argtypes = [vp, vp, vp, vp, vp, f32, vp, vp, vp, vp, vp, vp, i32, i32, i32, vp]
    L.mbv_op_expand.argtypes = [vp, vp, vp, vp, vp, f32, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp]
    L.mbv_op_cond_gemv.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, vp]
    L.mbv_op_gather_rows.argtypes = [vp, vp, vp, vp, i32, i32, i32, vp, vp]
    L.mbv_op_posterior_sample.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, vp]
    L.mbv_op_lens.argtypes = [vp, vp, vp, vp, vp, i32, i32, vp]
    L.mbv_op_dds_sep.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp]
    L.mbv_op_dds_res.argtypes = [vp, vp, vp, vp, vp, vp, i32, i32, i32, vp, vp]
    L.mbv_op_sdp_pre.argtypes = [vp, vp, i32, vp, vp, vp, vp, i32, i32, i32, vp]
    L.mbv_op_sdp_spline.argtypes = [vp, vp, vp, vp, i32, i32, i32, f32, vp]
    L.mbv_op_sdp_logw.argtypes = [vp, vp, vp, vp, vp, vp, i32, i32, vp]
    L.mbv_op_sdp_noise.argtypes = [vp, vp, f32, vp, C.c_int64, vp]
    L.mbv_op_chan_add.argtypes = [vp, vp, vp, i32, i32, i32, vp]
    L.mbv_op_istft_single.argtypes = [vp, vp, i32, i32, i32, vp, vp, vp, vp]
    L.mbv_align.argtypes = [vp, vp, vp, vp, vp, vp, i32, i32, i32, vp, f32, C.POINTER(MbvAlignOutputs), vp, vp]
    L.mbv_set_durations.argtypes = [vp, vp, i32, i32, i32, vp, vp]
    L.mbv_op_neg_cent.argtypes = [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp]
    L.mbv_op_max_path.argtypes = [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, vp]
    # MBV_LIB may name the build BEFORE the row-exact ragged decode (the baseline of scripts/ragged_timing.py): only
    # those four entries, the pooled decode's three, the pooled wire output's three, pooled admission's five, the
    # three that came with "tail_once", pooled conversion's three, live conversion's six, the live wire's three, the
    # seeded noise's three, the limiter's three, G.711's four, the fade's five, the marks' two, loudness's six, the
    # turns' two, prosody's four, volume's seven, pitch's four, the voices' five and the bounded look-ahead's four may be absent there, and calling one then raises AttributeError.
    # Everything else, and the in-tree library always, must match the header.
    optional = ("mbv_ragged_classes", "mbv_ragged_plan", "mbv_decode_ragged", "mbv_synthesize_ragged",
                "mbv_chunks_plan", "mbv_decode_chunks", "mbv_decoder_runs",
                "mbv_pcm_chunks_plan", "mbv_resample_pcm16_chunks", "mbv_wire_runs",
                "mbv_admit_plan", "mbv_encode_rows", "mbv_synthesize_rows", "mbv_encoder_runs",
                "mbv_get_option", "mbv_tail_plan", "mbv_tail_dropped", "mbv_decode_masked",
                "mbv_convert_plan", "mbv_convert_rows", "mbv_converter_runs",
                "mbv_decode_chunks_routed", "mbv_converter_context", "mbv_spectrogram_ready", "mbv_convert_window",
                "mbv_convert_ranges_plan", "mbv_convert_ranges",
                "mbv_resample_ready_open", "mbv_resample_ranges", "mbv_input_runs",
                "mbv_randn_blocks", "mbv_randn_host", "mbv_noise_runs",
                "mbv_limiter_ready", "mbv_resample_pcm16_range_limited", "mbv_resample_pcm16_chunks_limited",
                "mbv_g711_encode", "mbv_g711_decode", "mbv_resample_g711_range",
                "mbv_resample_g711_chunks",
                "mbv_pcm_fade_make", "mbv_resample_pcm16_range_faded", "mbv_resample_pcm16_chunks_faded",
                "mbv_resample_g711_range_faded", "mbv_resample_g711_chunks_faded",
                "mbv_token_marks", "mbv_token_marks_rows",
                "mbv_kweighting", "mbv_loudness_segments", "mbv_loudness", "mbv_loudness_range", "mbv_loudness_chunks",
                "mbv_loudness_runs", "mbv_turn_plan", "mbv_resample_turns",
                "mbv_shape_durations", "mbv_shape_durations_rows", "mbv_op_shape_durations", "mbv_shape_runs",
                "mbv_frame_gain", "mbv_frame_gain_rows", "mbv_op_frame_gain", "mbv_gain_runs",
                "mbv_resample_pcm16_range_shaped", "mbv_resample_pcm16_chunks_shaped",
                "mbv_resample_turns_shaped",
                "mbv_warp_plan", "mbv_warp_ready", "mbv_warp_ranges", "mbv_warp_runs",
                "mbv_speakers_define", "mbv_speaker_release", "mbv_speaker_slots", "mbv_speaker_defined",
                "mbv_speaker_runs", "mbv_tail_pack_table",
                "mbv_convert_window_ahead", "mbv_convert_ranges_ahead", "mbv_seam_rows", "mbv_seam_runs") if os.environ.get("MBV_LIB") else ()
    if hasattr(L, "mbv_ragged_classes") or not optional:
        L.mbv_ragged_classes.argtypes = [C.POINTER(MbvConfig), i32, i32, C.POINTER(C.c_int32), i32]
        L.mbv_ragged_plan.argtypes = [C.POINTER(MbvConfig), i32, i32, i32, i64p, C.POINTER(C.c_int32)]
        L.mbv_decode_ragged.argtypes = [vp, vp, vp, i32, i32, i64p, vp, vp]
        L.mbv_synthesize_ragged.argtypes = [vp, i32, vp, C.c_float, i32, C.POINTER(MbvOutputs), i64p, vp]
    if hasattr(L, "mbv_decode_chunks") or not optional:
        L.mbv_chunks_plan.argtypes = [C.POINTER(MbvConfig), i32, i32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        L.mbv_decode_chunks.argtypes = [vp, C.POINTER(MbvChunk), i32, vp]
        L.mbv_decoder_runs.argtypes = [vp]
        L.mbv_decoder_runs.restype = C.c_int64
    if hasattr(L, "mbv_resample_pcm16_chunks") or not optional:
        L.mbv_pcm_chunks_plan.argtypes = [i32, i32, i32, C.POINTER(MbvPcmChunk), i32, i64p]
        L.mbv_pcm_chunks_plan.restype = C.c_int64
        L.mbv_resample_pcm16_chunks.argtypes = [vp, C.POINTER(MbvPcmChunk), i32, i32, i32, i32, vp, C.c_int64, vp]
        L.mbv_wire_runs.argtypes = [vp]
        L.mbv_wire_runs.restype = C.c_int64
    if hasattr(L, "mbv_encode_rows") or not optional:
        L.mbv_admit_plan.argtypes = [C.POINTER(MbvConfig), i32, i32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        L.mbv_encode_rows.argtypes = [vp, i32, vp, vp, vp, i32, i32, C.POINTER(MbvEncRow), vp, vp]
        L.mbv_synthesize_rows.argtypes = [vp, i32, i32, C.POINTER(MbvRow), i32, vp]
        L.mbv_encoder_runs.argtypes = [vp]
        L.mbv_encoder_runs.restype = C.c_int64
        L.mbv_get_option.argtypes = [vp, C.c_char_p]
    if hasattr(L, "mbv_tail_plan") or not optional:
        L.mbv_tail_plan.argtypes = [C.POINTER(MbvConfig), C.POINTER(C.c_int32), i32]
        L.mbv_tail_dropped.argtypes = [vp]
        L.mbv_tail_dropped.restype = C.c_int64
        L.mbv_decode_masked.argtypes = [vp, vp, vp, vp, i32, i32, C.POINTER(MbvOutputs), vp]
    if hasattr(L, "mbv_tail_pack_table") or not optional:
        L.mbv_tail_pack_table.argtypes = [i64p, i32, i32, i32, i32, i32, i32, i32, C.POINTER(C.c_int32), C.c_int64]
    if hasattr(L, "mbv_convert_rows") or not optional:
        L.mbv_convert_plan.argtypes = [C.POINTER(MbvConfig), i32, i32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        L.mbv_convert_rows.argtypes = [vp, C.POINTER(MbvConvertRow), i32, i32, i32, i32, vp, vp]
        L.mbv_converter_runs.argtypes = [vp]
        L.mbv_converter_runs.restype = C.c_int64
    if hasattr(L, "mbv_convert_ranges") or not optional:
        L.mbv_decode_chunks_routed.argtypes = [vp, C.POINTER(MbvChunk), C.POINTER(C.c_int32), i32, vp]
        L.mbv_converter_context.argtypes = [C.POINTER(MbvConfig), C.POINTER(C.c_int32 * 2)]
        L.mbv_spectrogram_ready.argtypes = [C.c_int64, i32, i32, i32]
        L.mbv_spectrogram_ready.restype = C.c_int64
        L.mbv_convert_window.argtypes = [C.POINTER(MbvConfig), i32, i32, C.c_int64, C.POINTER(C.c_int32 * 2)]
        L.mbv_convert_ranges_plan.argtypes = [C.POINTER(MbvConfig), i32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        L.mbv_convert_ranges.argtypes = [vp, C.POINTER(MbvConvertRange), i32, i32, i32, vp]
    if hasattr(L, "mbv_resample_ranges") or not optional:
        L.mbv_resample_ready_open.argtypes = [i32, i32, i32, C.c_int64]
        L.mbv_resample_ready_open.restype = C.c_int64
        L.mbv_resample_ranges.argtypes = [vp, C.POINTER(MbvResampleRange), i32, i32, i32, i32, vp]
        L.mbv_input_runs.argtypes = [vp]
        L.mbv_input_runs.restype = C.c_int64
    if hasattr(L, "mbv_randn_blocks") or not optional:
        L.mbv_randn_blocks.argtypes = [vp, C.POINTER(MbvRandnBlock), i32, vp]
        L.mbv_randn_host.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int64, C.c_int64, vp]
        L.mbv_noise_runs.argtypes = [vp]
        L.mbv_noise_runs.restype = C.c_int64
    if hasattr(L, "mbv_limiter_ready") or not optional:
        L.mbv_limiter_ready.argtypes = [i32, i32, i32, C.c_int64, C.c_int64, i32]
        L.mbv_limiter_ready.restype = C.c_int64
        L.mbv_resample_pcm16_range_limited.argtypes = [vp, vp, vp, i32, C.c_int64, i32, i32, i32, C.c_int64, C.c_int64,
                                                       C.c_int64, vp, vp, C.c_int64, vp, vp, C.POINTER(MbvPcmLimit), vp]
        L.mbv_resample_pcm16_chunks_limited.argtypes = [vp, C.POINTER(MbvPcmChunk), C.POINTER(MbvPcmLimit), i32, i32,
                                                        i32, i32, vp, C.c_int64, vp]
    if hasattr(L, "mbv_resample_g711_range") or not optional:
        L.mbv_g711_encode.argtypes = [vp, vp, C.c_int64, i32, vp, vp]
        L.mbv_g711_decode.argtypes = [vp, vp, C.c_int64, i32, vp, vp]
        L.mbv_resample_g711_range.argtypes = [vp, vp, vp, i32, C.c_int64, i32, i32, i32, C.c_int64, C.c_int64, C.c_int64,
                                              vp, vp, C.c_int64, vp, vp, C.POINTER(MbvPcmLimit), i32, vp]
        L.mbv_resample_g711_chunks.argtypes = [vp, C.POINTER(MbvPcmChunk), C.POINTER(MbvPcmLimit), i32, i32, i32, i32,
                                               i32, vp, C.c_int64, vp]
    if hasattr(L, "mbv_pcm_fade_make") or not optional:
        fadep = C.POINTER(MbvPcmFade)
        L.mbv_pcm_fade_make.argtypes = [C.c_int64, C.c_int64, fadep]
        L.mbv_resample_pcm16_range_faded.argtypes = [vp, vp, vp, i32, C.c_int64, i32, i32, i32, C.c_int64, C.c_int64,
                                                     C.c_int64, vp, vp, C.c_int64, vp, vp, C.POINTER(MbvPcmLimit),
                                                     fadep, vp]
        L.mbv_resample_pcm16_chunks_faded.argtypes = [vp, C.POINTER(MbvPcmChunk), C.POINTER(MbvPcmLimit), fadep, i32,
                                                      i32, i32, i32, vp, C.c_int64, vp]
        L.mbv_resample_g711_range_faded.argtypes = [vp, vp, vp, i32, C.c_int64, i32, i32, i32, C.c_int64, C.c_int64,
                                                    C.c_int64, vp, vp, C.c_int64, vp, vp, C.POINTER(MbvPcmLimit), i32,
                                                    fadep, vp]
        L.mbv_resample_g711_chunks_faded.argtypes = [vp, C.POINTER(MbvPcmChunk), C.POINTER(MbvPcmLimit), fadep, i32,
                                                     i32, i32, i32, i32, vp, C.c_int64, vp]
    if hasattr(L, "mbv_token_marks") or not optional:
        L.mbv_token_marks.argtypes = [vp, vp, C.c_int64, vp]
        L.mbv_token_marks_rows.argtypes = [vp, i32, C.POINTER(MbvMarkRow), i32, vp]
    if hasattr(L, "mbv_loudness") or not optional:
        dp = C.POINTER(C.c_double)
        L.mbv_kweighting.argtypes = [i32, dp, dp]
        L.mbv_loudness_segments.argtypes = [i32, C.c_int64, C.POINTER(C.c_int32)]
        L.mbv_loudness_segments.restype = C.c_int64
        L.mbv_loudness.argtypes = [vp, vp, vp, i32, C.c_int64, i32, vp, vp, vp]
        L.mbv_loudness_range.argtypes = [vp, vp, vp, i32, C.c_int64, i32, C.c_int64, C.c_int64, C.c_int64, vp, vp,
                                         C.c_int64, vp, vp]
        L.mbv_loudness_chunks.argtypes = [vp, C.POINTER(MbvLoudnessChunk), i32, i32, vp]
        L.mbv_loudness_runs.argtypes = [vp]
        L.mbv_loudness_runs.restype = C.c_int64
    if hasattr(L, "mbv_resample_turns") or not optional:
        L.mbv_turn_plan.argtypes = [i32, i32, i32, C.POINTER(MbvTurnChunk), C.POINTER(MbvPcmLimit), i32, i64p]
        L.mbv_turn_plan.restype = C.c_int64
        L.mbv_resample_turns.argtypes = [vp, C.POINTER(MbvTurnChunk), C.POINTER(MbvPcmLimit), C.POINTER(MbvPcmFade), i32,
                                         i32, i32, i32, i32, vp, C.c_int64, vp]
    if hasattr(L, "mbv_shape_durations") or not optional:
        L.mbv_shape_durations.argtypes = [vp, vp, vp, C.POINTER(MbvFit), i32, i32, vp, vp, vp]
        L.mbv_shape_durations_rows.argtypes = [vp, i32, C.POINTER(MbvShapeRow), i32, vp, vp]
        L.mbv_op_shape_durations.argtypes = [vp, vp, vp, vp, vp, f32, C.POINTER(MbvFit), vp, vp, vp, vp, vp, vp, i32, i32,
                                             vp]
        L.mbv_shape_runs.argtypes = [vp]
        L.mbv_shape_runs.restype = C.c_int64
    if hasattr(L, "mbv_frame_gain") or not optional:
        envp = C.POINTER(MbvPcmEnvelope)
        L.mbv_frame_gain.argtypes = [vp, vp, vp, C.c_int64, i32, vp]
        L.mbv_frame_gain_rows.argtypes = [vp, i32, C.POINTER(MbvGainRow), i32, vp]
        L.mbv_op_frame_gain.argtypes = [vp, vp, vp, vp, vp, C.c_int64, i32, i32, i32, vp]
        L.mbv_gain_runs.argtypes = [vp]
        L.mbv_gain_runs.restype = C.c_int64
        L.mbv_resample_pcm16_range_shaped.argtypes = [vp, vp, vp, i32, C.c_int64, i32, i32, i32, C.c_int64, C.c_int64,
                                                      C.c_int64, vp, vp, C.c_int64, vp, vp, C.POINTER(MbvPcmLimit), i32,
                                                      C.POINTER(MbvPcmFade), envp, C.c_int64, vp]
        L.mbv_resample_pcm16_chunks_shaped.argtypes = [vp, C.POINTER(MbvPcmChunk), C.POINTER(MbvPcmLimit),
                                                       C.POINTER(MbvPcmFade), envp, i32, i32, i32, i32, i32, vp,
                                                       C.c_int64, vp]
        L.mbv_resample_turns_shaped.argtypes = [vp, C.POINTER(MbvTurnChunk), C.POINTER(MbvPcmLimit),
                                                C.POINTER(MbvPcmFade), envp, i32, i32, i32, i32, i32, vp, C.c_int64, vp]
    if hasattr(L, "mbv_warp_ranges") or not optional:
        L.mbv_warp_plan.argtypes = [i32, C.c_int64, vp, vp, i64p]
        L.mbv_warp_ready.argtypes = [i32, C.c_int64, vp, vp, i32, C.c_int64]
        L.mbv_warp_ready.restype = C.c_int64
        L.mbv_warp_ranges.argtypes = [vp, C.POINTER(MbvWarpRow), i32, vp]
        L.mbv_warp_runs.argtypes = [vp]
        L.mbv_warp_runs.restype = C.c_int64
    if hasattr(L, "mbv_speakers_define") or not optional:
        L.mbv_speakers_define.argtypes = [vp, C.POINTER(MbvSpeakerDef), i32, vp]
        L.mbv_speaker_release.argtypes = [vp, i32, vp]
        L.mbv_speaker_slots.argtypes = []
        L.mbv_speaker_defined.argtypes = [vp, C.c_int64]
        L.mbv_speaker_runs.argtypes = [vp]
        L.mbv_speaker_runs.restype = C.c_int64
    if hasattr(L, "mbv_convert_ranges_ahead") or not optional:
        L.mbv_convert_window_ahead.argtypes = [C.POINTER(MbvConfig), i32, i32, i32, C.c_int64, C.POINTER(C.c_int32 * 2)]
        L.mbv_convert_ranges_ahead.argtypes = [vp, C.POINTER(MbvConvertRange), C.POINTER(C.c_int32), i32, i32, i32, vp]
        L.mbv_seam_rows.argtypes = [vp, C.POINTER(MbvSeamRow), i32, vp]
        L.mbv_seam_runs.argtypes = [vp]
        L.mbv_seam_runs.restype = C.c_int64
    for s in SYMBOLS:
        if s not in optional or hasattr(L, s):
            getattr(L, s)      # AttributeError if the header and the library ever drift
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
