"""Drop-in `models.SynthesizerTrn` for the infer path.

Same constructor signature, attribute names and return tuples as the
reference (`models.py:573-599`, `697-737`, `742-788`, `.dec` `344-377`), same
state-dict keys (so `utils.load_checkpoint` and reference checkpoints work),
but every forward computation happens in the gfx950 kernels behind
`libmbistft_vits.so`.  PyTorch is used for device memory, the current HIP
stream and the RNG only.  The training-side `forward` is out of scope and raises.
"""
import ctypes as C
import math
import weakref

import numpy as np
import torch
from torch import nn

from . import _capi, stream
from .spec import ModelConfig, config_from_ctor, param_shapes, DEC_MS, DEC_SB

RESAMPLE_TYPES = _capi.RESAMPLE_TYPES     # librosa.resample res_type -> MBV_RESAMPLE_* of include/mbistft_vits.h


ENCODINGS = ("pcm16", "ulaw", "alaw")     # what the wire step stores: 16-bit linear, or G.711 bytes


def _law_code(encoding, what="encoding"):
    """`encoding=` of a wire entry -> 0 (int16) or the MBV_G711_* code; ValueError for anything else."""
    if encoding == "pcm16":
        return 0
    law = _capi.G711_LAWS.get(encoding) if isinstance(encoding, str) else None
    if law is None:
        raise ValueError("%s must be one of %s, got %r" % (what, ", ".join(repr(e) for e in ENCODINGS), encoding))
    return law


def _g711_law(law):
    if not isinstance(law, str) or law not in _capi.G711_LAWS:
        raise ValueError("law must be 'ulaw' or 'alaw', got %r" % (law,))
    return _capi.G711_LAWS[law]


def _filter_code(res_type):
    """res_type -> its MBV_RESAMPLE_* code; ValueError for a filter the GPU path does not have."""
    filt = RESAMPLE_TYPES.get(res_type)
    if filt is None:
        raise ValueError("res_type %r is not supported on the GPU path (supported: %s)"
                         % (res_type, ", ".join(sorted(RESAMPLE_TYPES))))
    return filt


def _ints(values):
    """A tensor (either device; a device tensor is read back) or a sequence -> a list of ints."""
    return [int(v) for v in (values.tolist() if torch.is_tensor(values) else values)]


def _valid_samples(valid, B, dev, what="valid_samples"):
    """Per-row sample (or frame) counts -> contiguous int64 [B] on the device."""
    valid = valid.to(device=dev, dtype=torch.int64).contiguous()
    if valid.shape != (B,):
        raise ValueError("%s must be [B]" % what)
    return valid


def _durations_code(durations):
    """Given durations -> (tensor of a dtype mbv_set_durations reads, its dtype code): int32 0, int64 1, fp32 2."""
    if durations.dtype == torch.int32:
        return durations, 0
    if durations.dtype == torch.int64:
        return durations, 1
    if durations.dtype.is_floating_point:
        return durations.to(torch.float32), 2
    return durations.to(torch.int64), 1


FIT_BOUNDS = (0.5, 2.0)      # default `fit_bounds=`: a convention (half to double rate), not a measurement


def frames_of_ms(ms, model_sr, samples_per_frame):
    """Whole z-frames nearest to `ms` milliseconds at the model's rate (one frame = samples_per_frame samples of
    model_sr Hz), a half rounding up: (2 ms model_sr + 1000 spf) // (2000 spf).  Pure integers, like the other
    planners: what `extra_frames=` takes for a pause of known length.  ValueError for anything else."""
    for name, v in (("ms", ms), ("model_sr", model_sr), ("samples_per_frame", samples_per_frame)):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
            raise TypeError("frames_of_ms: %s must be an integer, got %s" % (name, type(v).__name__))
    ms, model_sr, spf = int(ms), int(model_sr), int(samples_per_frame)
    if ms < 0 or model_sr < 1 or spf < 1:
        raise ValueError("frames_of_ms: need ms >= 0, model_sr >= 1 and samples_per_frame >= 1")
    return (2 * ms * model_sr + 1000 * spf) // (2000 * spf)


def _prosody_args(who, length_scale, extra_frames, fit_frames, fit_bounds, durations, B, T, row=False):
    """The three prosody controls of an entry, checked on the host -> (scalar, scale, extra, fit):
      scalar  the float the encode takes (1.0 with a scale table)
      scale   None, or the per-token table as fp32 [B, T]
      extra   None, or the extra frames as int32 [B, T] (another integer dtype is clamped to [-1, 2^20] first: a
              negative entry stays negative and one past the range stays past it, so the kernel's flags still see both)
      fit     None, or [(frames, lo, hi)] * B
    row: the entry takes one utterance (`Request`): tables are [T] (or [1, T] / [1, 1, T]).  Values on the device are
    not looked at here (no synchronisation); the kernel flags them."""
    shapes = ((T,), (1, T), (1, 1, T)) if row else ((B, T), (B, 1, T))
    names = "[T_text]" if row else "[B, T_text] or [B, 1, T_text]"
    scale = None
    if torch.is_tensor(length_scale) and length_scale.dim() >= (1 if row else 2):
        if not length_scale.dtype.is_floating_point:
            raise TypeError("%s: a per-token length_scale must be a floating tensor, got %s" % (who, length_scale.dtype))
        if tuple(length_scale.shape) not in shapes:
            raise ValueError("%s: a per-token length_scale must be %s = %s, got %s"
                             % (who, names, shapes[0], tuple(length_scale.shape)))
        scale = length_scale.reshape(B, T).to(torch.float32).contiguous()
        scalar = 1.0
    else:
        scalar = float(length_scale)
    extra = None
    if extra_frames is not None:
        if not torch.is_tensor(extra_frames):
            raise ValueError("%s: extra_frames must be an integer tensor %s" % (who, names))
        if extra_frames.dtype.is_floating_point or extra_frames.dtype.is_complex or extra_frames.dtype == torch.bool:
            raise TypeError("%s: extra_frames must hold integers, got %s" % (who, extra_frames.dtype))
        if tuple(extra_frames.shape) not in shapes:
            raise ValueError("%s: extra_frames must be %s = %s, got %s" % (who, names, shapes[0], tuple(extra_frames.shape)))
        extra = extra_frames.reshape(B, T)
        if extra.dtype != torch.int32:
            extra = extra.clamp(-1, 1 << 20).to(torch.int32)
        extra = extra.contiguous()
    fit = None
    if fit_frames is not None:
        if torch.is_tensor(fit_frames):
            if fit_frames.is_cuda:
                raise ValueError("%s: fit_frames are host integers (an int, or B of them)" % who)
            fit_frames = fit_frames.reshape(-1).tolist() if fit_frames.dim() else fit_frames.item()
        elif isinstance(fit_frames, np.ndarray):
            fit_frames = fit_frames.reshape(-1).tolist() if fit_frames.ndim else fit_frames.item()
        frames = list(fit_frames) if isinstance(fit_frames, (list, tuple)) else [fit_frames] * B
        if len(frames) != B:
            raise ValueError("%s: %d fit_frames for %d rows" % (who, len(frames), B))
        for v in frames:
            if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
                raise TypeError("%s: fit_frames must be integers, got %s" % (who, type(v).__name__))
            if not 1 <= int(v) < 1 << 62:
                raise ValueError("%s: fit_frames must be >= 1, got %d" % (who, int(v)))
        try:
            lo, hi = (float(np.float32(v)) for v in fit_bounds)
        except (TypeError, ValueError):
            raise ValueError("%s: fit_bounds must be (lo, hi)" % who)
        if not (0.0 < lo <= hi < math.inf):
            raise ValueError("%s: fit_bounds must be 0 < lo <= hi < inf (in fp32), got %r" % (who, (fit_bounds,)))
        fit = [(int(v), lo, hi) for v in frames]
    if durations is not None and (scale is not None or extra is not None or fit is not None):
        raise ValueError("%s: durations= are used as given: a per-token length_scale, extra_frames= and fit_frames= "
                         "shape the PREDICTED durations and exclude it" % who)
    return scalar, scale, extra, fit


GAIN_MAX = 16.0              # largest per-token gain (about +24 dB): a convention, not a measurement


def gain_of_db(db):
    """A level change in dB -> the linear factor `gain=` takes: 10 ** (db / 20) in Python floats, then rounded to fp32;
    -inf gives 0 (silence).  NaN and +inf are a ValueError."""
    db = float(db)
    if db == -math.inf:
        return 0.0
    if not math.isfinite(db):
        raise ValueError("gain_of_db: need a finite level in dB (or -inf for silence), got %r" % db)
    return float(np.float32(10.0 ** (db / 20.0)))


def _gain_arg(who, gain, B, T, row=False):
    """`gain=` of an entry, checked on the host -> None, or the per-token linear gains as a CPU fp32 tensor [B, T]: a
    host sequence or CPU tensor (the mark-up is parsed on the host) of T_text values per row, finite, in [0, GAIN_MAX].
    A device tensor is refused."""
    if gain is None:
        return None
    shapes = ((T,), (1, T), (1, 1, T)) if row else ((B, T), (B, 1, T))
    names = "[T_text]" if row else "[B, T_text]"
    if torch.is_tensor(gain):
        if gain.is_cuda:
            raise TypeError("%s: gain must be a host sequence or a CPU tensor (it is checked on the host), got a "
                            "device tensor" % who)
        if gain.dtype.is_complex or gain.dtype == torch.bool:
            raise TypeError("%s: gain must hold real numbers, got %s" % (who, gain.dtype))
        g = gain.detach().to(torch.float64)
    else:
        if isinstance(gain, (str, bytes)):
            raise TypeError("%s: gain must be a sequence of numbers %s" % (who, names))
        try:
            arr = np.asarray(gain)
        except Exception:
            raise TypeError("%s: gain must be a sequence of numbers %s" % (who, names))
        if arr.dtype == np.bool_ or arr.dtype.kind not in "iuf":
            raise TypeError("%s: gain must hold real numbers, got %s" % (who, arr.dtype))
        g = torch.from_numpy(arr.astype(np.float64))
    if tuple(g.shape) not in shapes:
        raise ValueError("%s: gain must be %s = %s, got %s" % (who, names, shapes[0], tuple(g.shape)))
    g = g.reshape(B, T)
    if not bool(torch.isfinite(g).all()):
        raise ValueError("%s: gain must be finite" % who)
    if bool((g < 0).any()) or bool((g > GAIN_MAX).any()):
        raise ValueError("%s: gain must be in [0, GAIN_MAX = %g] (linear factors; gain_of_db converts)" % (who, GAIN_MAX))
    return g.to(torch.float32).contiguous()


PITCH_MIN, PITCH_MAX = _capi.PITCH_MIN, _capi.PITCH_MAX      # +-12 semitones: refusal bounds and a convention
PITCH_GLIDE_FRAMES = 2       # default `pitch_glide_frames=`: a convention, not a measurement


def pitch_of_semitones(st):
    """A pitch change in semitones -> the factor `pitch=` takes: 2 ** (st / 12)."""
    st = float(st)
    if not math.isfinite(st):
        raise ValueError("pitch_of_semitones: need a finite number of semitones, got %r" % st)
    return 2.0 ** (st / 12.0)


def _pitch_arg(who, pitch, B, T, row=False):
    """`pitch=` of an entry, checked on the host -> None, or the per-token pitch factors as a CPU fp32 tensor [B, T]: a
    host sequence or CPU tensor of T_text values per row, finite, in [PITCH_MIN, PITCH_MAX] after rounding to fp32.  A
    device tensor is refused."""
    if pitch is None:
        return None
    shapes = ((T,), (1, T), (1, 1, T)) if row else ((B, T), (B, 1, T))
    names = "[T_text]" if row else "[B, T_text]"
    if torch.is_tensor(pitch):
        if pitch.is_cuda:
            raise TypeError("%s: pitch must be a host sequence or a CPU tensor (the warp is planned on the host), got a "
                            "device tensor" % who)
        if pitch.dtype.is_complex or pitch.dtype == torch.bool:
            raise TypeError("%s: pitch must hold real numbers, got %s" % (who, pitch.dtype))
        p = pitch.detach().to(torch.float64)
    else:
        if isinstance(pitch, (str, bytes)):
            raise TypeError("%s: pitch must be a sequence of numbers %s" % (who, names))
        try:
            arr = np.asarray(pitch)
        except Exception:
            raise TypeError("%s: pitch must be a sequence of numbers %s" % (who, names))
        if arr.dtype == np.bool_ or arr.dtype.kind not in "iuf":
            raise TypeError("%s: pitch must hold real numbers, got %s" % (who, arr.dtype))
        p = torch.from_numpy(arr.astype(np.float64))
    if tuple(p.shape) not in shapes:
        raise ValueError("%s: pitch must be %s = %s, got %s" % (who, names, shapes[0], tuple(p.shape)))
    p = p.reshape(B, T)
    if not bool(torch.isfinite(p).all()):
        raise ValueError("%s: pitch must be finite" % who)
    p = p.to(torch.float32).contiguous()
    if bool((p < PITCH_MIN).any()) or bool((p > PITCH_MAX).any()):
        raise ValueError("%s: pitch must be in [PITCH_MIN = %g, PITCH_MAX = %g] (factors; pitch_of_semitones converts)"
                         % (who, PITCH_MIN, PITCH_MAX))
    return p


def _pitch_scale(who, pitch, length_scale, durations, compensate):
    """The `length_scale` an entry with `pitch=` encodes with: refused beside `durations=`; with `compensate` the
    per-token table fl32(length_scale) * pitch, formed in fp32 on the host (on the device of a tensor `length_scale`),
    so that every token keeps its length; else `length_scale` as it is (plain varispeed)."""
    if durations is not None:
        raise ValueError("%s: pitch= does not go with durations=: they are used as given, so no token can be "
                         "lengthened to be played faster; scale the durations by the pitch yourself and warp the "
                         "result with net.warp(wave, net.warp_map(pitch, durations))" % who)
    if not compensate:
        return length_scale
    if torch.is_tensor(length_scale):
        if not length_scale.dtype.is_floating_point:
            raise TypeError("%s: a per-token length_scale must be a floating tensor, got %s" % (who, length_scale.dtype))
        base = length_scale.to(torch.float32)
        if base.numel() != 1:
            if base.numel() != pitch.numel():
                raise ValueError("%s: a per-token length_scale must hold one value per token (%d), got %s"
                                 % (who, pitch.numel(), tuple(base.shape)))
            base = base.reshape(pitch.shape)
        return base * pitch.to(base.device)
    return torch.tensor(float(length_scale), dtype=torch.float32) * pitch


class Envelope:
    """The gain envelope of a wire call (`wire.Envelope`): the frame gains of `net.frame_gain` /
    `st.frame_gain` and the model's samples per frame.
      gain               fp32 device tensor [F + 1] (one row) or [B, F + 1] with unit stride along a row: G of the
                         row(s); model-rate sample j is scaled by G[f] + (j - f hop) / hop * (G[f + 1] - G[f]), f = j // hop
      samples_per_frame  hop >= 1
    A wire call refuses an envelope whose (F * hop) is below the samples of its row."""

    __slots__ = ("gain", "hop", "frames", "rows")

    def __init__(self, gain, samples_per_frame):
        if isinstance(samples_per_frame, (bool, np.bool_)) or not isinstance(samples_per_frame, (int, np.integer)):
            raise TypeError("Envelope: samples_per_frame must be an integer, got %s" % type(samples_per_frame).__name__)
        if int(samples_per_frame) < 1 or int(samples_per_frame) >= 1 << 31:
            raise ValueError("Envelope: samples_per_frame must be in [1, 2^31), got %d" % int(samples_per_frame))
        if not torch.is_tensor(gain):
            raise TypeError("Envelope: gain must be an fp32 device tensor [F + 1] or [B, F + 1] (net.frame_gain, "
                            "st.frame_gain), got %s" % type(gain).__name__)
        if gain.dtype != torch.float32:
            raise TypeError("Envelope: gain must be float32, got %s" % gain.dtype)
        if not gain.is_cuda:
            raise TypeError("Envelope: gain must live on the device (the wire kernels read it in place)")
        if gain.dim() not in (1, 2) or gain.shape[-1] < 2 or gain.stride(-1) != 1:
            raise ValueError("Envelope: gain must be [F + 1] or [B, F + 1] with F >= 1 and unit stride, got %s"
                             % (tuple(gain.shape),))
        self.gain, self.hop = gain, int(samples_per_frame)
        self.frames = gain.shape[-1] - 1
        self.rows = 1 if gain.dim() == 1 else gain.shape[0]

    def __repr__(self):
        return "Envelope(%d row%s, %d frames of %d samples)" % (self.rows, "" if self.rows == 1 else "s", self.frames, self.hop)

    def check(self, who, rows, samples, device=None):
        """ValueError unless the envelope has `rows` rows, covers `samples` model-rate samples and (when given) lives
        on `device`."""
        if self.rows != rows:
            raise ValueError("%s: the envelope has %d row(s), the call %d" % (who, self.rows, rows))
        if self.frames * self.hop < int(samples):
            raise ValueError("%s: the envelope covers %d frames x %d = %d samples, the row holds %d"
                             % (who, self.frames, self.hop, self.frames * self.hop, int(samples)))
        if device is not None and self.gain.device != device:
            raise ValueError("%s: the envelope's gain is on %s, the model on %s" % (who, self.gain.device, device))

    @property
    def stride(self):
        return self.gain.stride(0) if self.gain.dim() == 2 and self.rows > 1 else 0

    def c(self):
        """-> the `_capi.MbvPcmEnvelope` of row 0 (inv_hop = fp32 1 / fp32 hop, as the entries check it)."""
        return _capi.MbvPcmEnvelope(self.gain.data_ptr(), self.frames, self.hop,
                                    float(np.float32(1.0) / np.float32(self.hop)))


def _envelope_c(envelope):
    """None -> the all-zero table row of a row without an envelope."""
    return _capi.MbvPcmEnvelope(None, 0, 0, 0.0) if envelope is None else envelope.c()


def _limits_c(who, noun, limits, n):
    """`limits` (None, or one entry per `noun`, each None or (ceiling, lookahead, hold)) -> the `MbvPcmLimit` array of a
    wire entry (ceiling 0: that row has no limiter), or None when no row is limited."""
    if limits is None or all(l is None for l in limits):
        return None
    if len(limits) != n:
        raise ValueError("%s: one limit per %s expected (%d), got %d" % (who, noun, n, len(limits)))
    return (_capi.MbvPcmLimit * n)(*[_capi.MbvPcmLimit(*(l or (0.0, 0, 0))) for l in limits])


def _fades_c(who, noun, fades, n):
    """`fades` (None, or one entry per `noun`, each None, a (first, count) or a `_capi.MbvPcmFade`, which is passed as it
    is) -> the `MbvPcmFade` array of a wire entry (count -1: that row does not fade), or None when no row fades."""
    if fades is None or all(f is None for f in fades):
        return None
    if len(fades) != n:
        raise ValueError("%s: one fade per %s expected (%d), got %d" % (who, noun, n, len(fades)))
    return (_capi.MbvPcmFade * n)(*[f if isinstance(f, _capi.MbvPcmFade) else _capi.MbvPcmFade(*_capi.NO_FADE) if f is None
                                   else _capi.pcm_fade(*f) for f in fades])


def _packed_capacity(who, packed, law, dev):
    """The capacity of the `packed` buffer of a pooled wire entry (None: 0), a 1-D tensor of the codec's sample type."""
    if packed is None:
        return 0
    wire_dtype = torch.uint8 if law else torch.int16
    if packed.device != dev or packed.dtype != wire_dtype or packed.dim() != 1 or packed.stride(0) != 1:
        raise ValueError("%s: packed must be a 1-D %s tensor on %s with unit stride"
                         % (who, str(wire_dtype).replace("torch.", ""), dev))
    return packed.shape[0]


def _range_entry(lim, law, fade, envelope):
    """Which entry `resample_pcm16_range` calls -> (name, its arguments behind the ones every form takes)."""
    if envelope is not None:
        return "mbv_resample_pcm16_range_shaped", (lim, law, fade, C.byref(envelope.c()), envelope.stride)
    if fade is not None:
        return ("mbv_resample_g711_range_faded", (lim, law, fade)) if law else ("mbv_resample_pcm16_range_faded", (lim, fade))
    if law:
        return "mbv_resample_g711_range", (lim, law)
    return ("mbv_resample_pcm16_range", ()) if lim is None else ("mbv_resample_pcm16_range_limited", (lim,))


def _chunks_entry(lim, law, fade, env):
    """Which entry `resample_pcm16_chunks` calls -> (name, the tables it takes, whether it takes `law`)."""
    if env is not None:
        return "mbv_resample_pcm16_chunks_shaped", (lim, fade, env), True
    if fade is not None:
        return ("mbv_resample_g711_chunks_faded" if law else "mbv_resample_pcm16_chunks_faded"), (lim, fade), bool(law)
    if law:
        return "mbv_resample_g711_chunks", (lim,), True
    return ("mbv_resample_pcm16_chunks", (), False) if lim is None else ("mbv_resample_pcm16_chunks_limited", (lim,), False)


def _seed_value(v, what="seed"):
    """One seed of the device generator -> int in [0, 2^64).  TypeError for anything that is not an
    integer (bool and floats included), ValueError outside the range."""
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
        raise TypeError("%s must be an integer in [0, 2^64), got %s" % (what, type(v).__name__))
    v = int(v)
    if not 0 <= v < 1 << 64:
        raise ValueError("%s must be in [0, 2^64), got %d" % (what, v))
    return v


class RowSeeds(list):
    """(seed, row) of every row of a batched call, checked: what `_row_seeds` returns."""


def _row_seeds(seed, B, what="seed"):
    """`seed=` of a batched entry -> RowSeeds [(seed_b, row_b)] * B, or None for None: an int s gives row b the
    sub-stream (s, row=b); a length-B sequence or integer tensor gives row b (seed_b, row=0)."""
    if seed is None or isinstance(seed, RowSeeds):
        return seed
    if torch.is_tensor(seed):
        if seed.dtype.is_floating_point or seed.dtype.is_complex or seed.dtype == torch.bool:
            raise TypeError("%s must hold integers, got %s" % (what, seed.dtype))
        seed = seed.item() if seed.dim() == 0 else seed.reshape(-1).tolist()
    elif isinstance(seed, np.ndarray):
        seed = seed.reshape(-1).tolist() if seed.ndim else seed.item()
    if isinstance(seed, (list, tuple)):
        if len(seed) != B:
            raise ValueError("%s: %d seeds for %d rows" % (what, len(seed), B))
        return RowSeeds((_seed_value(v, what), 0) for v in seed)
    s = _seed_value(seed, what)
    return RowSeeds((s, b) for b in range(B))


SPEAKER_SLOTS, BLEND_MAX = _capi.SPEAKER_SLOTS, _capi.BLEND_MAX     # conventions of the library, DESIGN 7.24


def blend_weights(weights, normalize=True):
    """The fp32 weights a blended voice is defined with (`net.speaker`), as a list of Python floats that are exactly
    representable in fp32.  `normalize`: every weight divided by their float64 sum, then rounded to fp32 (needs a sum
    > 0); else the weights as given, rounded to fp32 (extrapolation such as [1.5, -0.5]).  ValueError: no weight, more
    than BLEND_MAX, a weight that is not finite (before or after rounding), a sum <= 0 under `normalize`."""
    if torch.is_tensor(weights):
        weights = weights.detach().reshape(-1).tolist()
    w = np.asarray(list(weights), dtype=np.float64).reshape(-1)
    if not 1 <= w.size <= BLEND_MAX:
        raise ValueError("a blend takes 1 .. %d weights, got %d" % (BLEND_MAX, w.size))
    if not np.all(np.isfinite(w)):
        raise ValueError("blend weights must be finite, got %s" % (w.tolist(),))
    if normalize:
        total = float(np.sum(w))
        if not total > 0:
            raise ValueError("normalize=True needs weights with a sum > 0 (got %r); normalize=False sends them as given"
                             % total)
        w = w / total
    with np.errstate(over="ignore"):
        w32 = w.astype(np.float32)
    if not np.all(np.isfinite(w32)):
        raise ValueError("a blend weight is beyond fp32")
    return [float(v) for v in w32]


class SpeakerSlots:
    """The voice slots of one model, on the host: `take()` hands out the lowest free slot, `free(slot)` returns one."""

    def __init__(self, n=SPEAKER_SLOTS):
        self.n = int(n)
        self._used = set()

    def take(self):
        for j in range(self.n):
            if j not in self._used:
                self._used.add(j)
                return j
        raise ValueError("all %d voice slots are taken: release() a voice first" % self.n)

    def free(self, slot):
        if slot not in self._used:
            raise ValueError("voice slot %r is not taken" % (slot,))
        self._used.remove(slot)

    def __contains__(self, slot):
        return slot in self._used

    def __len__(self):
        return len(self._used)


class Speaker:
    """A voice of `net.speaker` / `net.speakers`: a virtual speaker behind the embedding table.

      sid       the int that names it wherever a speaker id goes, n_speakers + its slot; put it into sid tensors
      ids, weights    the definition: real speaker ids and the fp32 weights actually sent (None for a vector voice)
      row()     its row [gin] on the device, through `mbv_speaker_embedding`
      release() frees the slot; refused (ValueError) while an open `LiveStream` converts with it
    The object itself goes wherever a host speaker id goes (`Request.sid`, `ConvertRequest`, `convert_stream`,
    `convert_live`, the wire converts) and, standing for a one-element tensor, wherever a sid tensor goes; a released
    one raises ValueError there."""

    def __init__(self, net, slot, ids, weights, vector):
        self._net = weakref.ref(net)
        self.slot = slot
        self._sid = net.n_speakers + slot
        self.ids = None if ids is None else tuple(ids)
        self.weights = None if weights is None else tuple(weights)
        self._vector = vector                 # the row of a vector voice: what a re-created handle is given again
        self.released = False

    @property
    def sid(self):
        if self.released:
            raise ValueError("%r was released: its slot may name another voice by now" % (self,))
        return self._sid

    def __index__(self):
        return self.sid

    __int__ = __index__

    def _owner(self):
        net = self._net()
        if net is None:
            raise ValueError("the model of %r is gone" % (self,))
        return net

    def row(self):
        net = self._owner()
        return net._speaker_embedding(torch.tensor([self.sid], dtype=torch.int64))[0]

    def release(self):
        if not self.released:
            self._owner()._release_speaker(self)

    def __repr__(self):
        what = "vector" if self.ids is None else "ids=%s, weights=%s" % (list(self.ids), list(self.weights))
        return "Speaker(sid=%d, %s%s)" % (self._sid, what, ", released" if self.released else "")


def _host_sid(sid):
    """A host speaker id as the entries take it: a `Speaker` gives its int (ValueError once released), anything else
    passes."""
    return sid.sid if isinstance(sid, Speaker) else sid


def _sid_tensor(sid):
    """A sid tensor as the entries take it: a `Speaker` stands for the one-element tensor of its id."""
    return torch.tensor([sid.sid], dtype=torch.int64) if isinstance(sid, Speaker) else sid


class Request:
    """One utterance of a pooled admission (`SynthesizerTrn.infer_streams`, `StreamPool.admit`, `PcmPool.admit`): the
    arguments one `infer_stream` call takes, for one text.

      x                  1-D token ids (tensor on either device, or a sequence of ints); at least one
      sid                speaker id (an int, or a `Speaker`; required by a multi-speaker model), or None
      noise_scale, length_scale, noise_scale_w, max_len       as `infer`
      chunk_frames, max_chunk_frames                          as `dec_stream`
      durations          frames per token, [T_text] (or [1, T_text] / [1, 1, T_text]), as `infer(durations=)`:
                         needs length_scale == 1
      length_scale       may also be a floating tensor [T_text]: one scale per token, as `infer` takes it
      extra_frames, fit_frames, fit_bounds      the other prosody controls of `infer`: an integer tensor
                         [T_text], one int, (lo, hi); none of the three goes with durations
      seed               None = the noise comes from torch's generators, as `infer_stream` draws it; an int in
                         [0, 2^64): the request's noise is a function of the seed alone, at row 0
      marks              True: the stream gets `marks`, the z-frame at which every token starts, as
                         `infer_stream(marks=True)` gives them
      gain               per-token volume, as `infer_stream(gain=)`: T_text linear factors in [0, GAIN_MAX] on the host
                         (`gain_of_db` converts); the stream gets `frame_gain` and the wire path shapes it
      pitch, pitch_compensate, pitch_glide_frames      per-token pitch, as `infer_stream(pitch=)`: T_text factors in
                         [PITCH_MIN, PITCH_MAX] on the host (`pitch_of_semitones` converts); the stream gets `warp` and
                         the wire path warps it.  Not with durations
    Everything that can be checked without the model is checked here (ValueError / TypeError)."""

    __slots__ = ("x", "sid", "noise_scale", "length_scale", "noise_scale_w", "max_len", "chunk_frames",
                 "max_chunk_frames", "durations", "durations_dtype", "seed", "marks", "scale", "extra", "fit", "gain",
                 "pitch", "pitch_glide_frames")

    def __init__(self, x, sid=None, noise_scale=1, length_scale=1, noise_scale_w=1., max_len=None,
                 chunk_frames=32, max_chunk_frames=256, durations=None, seed=None, marks=False, extra_frames=None,
                 fit_frames=None, fit_bounds=FIT_BOUNDS, gain=None, pitch=None, pitch_compensate=True,
                 pitch_glide_frames=PITCH_GLIDE_FRAMES):
        self.seed = None if seed is None else _seed_value(seed, "Request: seed")
        self.marks = bool(marks)
        if not torch.is_tensor(x):
            x = torch.as_tensor(x)
        if x.dim() != 1:
            raise ValueError("Request: x must be 1-D token ids (one utterance), got shape %s" % (tuple(x.shape),))
        if x.numel() < 1:
            raise ValueError("Request: empty text")
        if x.dtype.is_floating_point or x.dtype.is_complex or x.dtype == torch.bool:
            raise TypeError("Request: x must hold integer token ids, got %s" % x.dtype)
        self.x = x.to(torch.int64)
        # per-token pitch: the factors as [T_text] fp32 on the host, or None; the stream gets `warp`
        pitch = _pitch_arg("Request", pitch, 1, self.x.numel(), row=True)
        self.pitch = None if pitch is None else pitch.reshape(-1)
        self.pitch_glide_frames = int(pitch_glide_frames)
        if self.pitch_glide_frames < 0:
            raise ValueError("Request: pitch_glide_frames must be >= 0")
        if pitch is not None:
            length_scale = _pitch_scale("Request", self.pitch, length_scale, durations, pitch_compensate)
        sid = _host_sid(sid)
        if sid is not None:
            if torch.is_tensor(sid):
                if sid.numel() != 1:
                    raise ValueError("Request: sid must be one speaker id")
                sid = sid.reshape(()).item()
            if isinstance(sid, bool) or int(sid) != sid:
                raise TypeError("Request: sid must be an integer")
            sid = int(sid)
        self.sid = sid
        # scale / extra: the tables as [T_text] fp32 / int32 (or None); fit: (frames, lo, hi) or None
        self.length_scale, scale, extra, fit = _prosody_args("Request", length_scale, extra_frames, fit_frames,
                                                             fit_bounds, durations, 1, self.x.numel(), row=True)
        self.scale = None if scale is None else scale.reshape(-1)
        self.extra = None if extra is None else extra.reshape(-1)
        self.fit = None if fit is None else fit[0]
        gain = _gain_arg("Request", gain, 1, self.x.numel(), row=True)
        self.gain = None if gain is None else gain.reshape(-1)
        self.noise_scale = float(noise_scale)
        self.noise_scale_w = float(noise_scale_w)
        for name in ("noise_scale", "length_scale", "noise_scale_w"):
            if not math.isfinite(getattr(self, name)):
                raise ValueError("Request: %s must be finite" % name)
        if max_len is not None:
            max_len = int(max_len)
            if max_len < 1:
                raise ValueError("Request: max_len leaves no frames to decode")
        self.max_len = max_len
        self.chunk_frames, self.max_chunk_frames = int(chunk_frames), int(max_chunk_frames)
        if self.chunk_frames < 1 or self.max_chunk_frames < self.chunk_frames:
            raise ValueError("Request: need 1 <= chunk_frames <= max_chunk_frames (got %d, %d)"
                             % (self.chunk_frames, self.max_chunk_frames))
        self.durations_dtype = None
        if durations is not None:
            if self.length_scale != 1.0:
                raise ValueError("Request: durations= are used as given: length_scale must be 1 (scale the durations instead)")
            if not torch.is_tensor(durations):
                raise ValueError("Request: durations must be a tensor [T_text]")
            T = self.x.numel()
            if durations.numel() != T or tuple(durations.shape) not in ((T,), (1, T), (1, 1, T)):
                raise ValueError("Request: durations must be [T_text] = [%d] (or [1, %d] / [1, 1, %d]), got %s"
                                 % (T, T, T, tuple(durations.shape)))
            durations, self.durations_dtype = _durations_code(durations.reshape(T))
            durations = durations.contiguous()
        self.durations = durations

    def __repr__(self):
        return "Request(%d tokens, sid=%r%s)" % (self.x.numel(), self.sid, "" if self.durations is None else ", durations")


class ConvertRequest:
    """One utterance of a pooled voice conversion (`SynthesizerTrn.convert_streams`, `StreamPool.admit`,
    `PcmPool.admit`): the arguments one `convert_stream` call takes, for one recording.

      wave               1-D int16 (scaled by 1 / 32768, as data_utils.py:75 does) or fp32 samples at `in_sr`, on either
                         device; at least one
      sid_src, sid_tgt   speaker ids (ints, or `Speaker`s)
      model_sr, hop_size, win_size      the model's data config (sampling_rate, hop_length, win_length)
      in_sr              the rate of `wave`; None = model_sr
      noise_scale        scale of the posterior draw (1 = `voice_conversion`), >= 0
      chunk_frames, max_chunk_frames    as `dec_stream`
      seed               None = the posterior draw comes from torch's device generator; an int in [0, 2^64): it is a
                         function of the seed alone, at row 0
    n_fft is not a field: it is 2 (spec_channels - 1) of the model the request is given to, which also checks
    win_size <= n_fft.  Everything that can be checked without the model is checked here (ValueError / TypeError)."""

    __slots__ = ("wave", "sid_src", "sid_tgt", "model_sr", "hop_size", "win_size", "in_sr", "noise_scale",
                 "chunk_frames", "max_chunk_frames", "seed")

    MAX_N_FFT = 4096                # the largest transform `spectrogram` is built for

    def __init__(self, wave, sid_src, sid_tgt, model_sr, hop_size, win_size, in_sr=None, noise_scale=1.0,
                 chunk_frames=32, max_chunk_frames=256, seed=None):
        self.seed = None if seed is None else _seed_value(seed, "ConvertRequest: seed")
        if not torch.is_tensor(wave):
            wave = torch.as_tensor(wave)
        if wave.dtype not in (torch.int16, torch.float32):
            raise TypeError("ConvertRequest: wave must be int16 or float32, got %s" % wave.dtype)
        if wave.dim() != 1:
            raise ValueError("ConvertRequest: wave must be 1-D samples (one recording), got shape %s" % (tuple(wave.shape),))
        if wave.numel() < 1:
            raise ValueError("ConvertRequest: empty wave")
        self.wave = wave.contiguous()
        sids = []
        for name, sid in (("sid_src", _host_sid(sid_src)), ("sid_tgt", _host_sid(sid_tgt))):
            if torch.is_tensor(sid):
                if sid.numel() != 1:
                    raise ValueError("ConvertRequest: %s must be one speaker id" % name)
                sid = sid.reshape(()).item()
            if isinstance(sid, bool) or not isinstance(sid, (int, float, np.integer, np.floating)) or int(sid) != sid:
                raise TypeError("ConvertRequest: %s must be an integer" % name)
            sids.append(int(sid))
        self.sid_src, self.sid_tgt = sids
        self.model_sr, self.hop_size, self.win_size = int(model_sr), int(hop_size), int(win_size)
        self.in_sr = self.model_sr if in_sr is None else int(in_sr)
        if self.model_sr <= 0 or self.in_sr <= 0:
            raise ValueError("ConvertRequest: sample rates must be positive")
        if self.hop_size < 1:
            raise ValueError("ConvertRequest: hop_size must be >= 1")
        if not 1 <= self.win_size <= self.MAX_N_FFT:
            raise ValueError("ConvertRequest: win_size %d outside [1, n_fft] (n_fft <= %d)" % (self.win_size, self.MAX_N_FFT))
        self.noise_scale = float(noise_scale)
        if not math.isfinite(self.noise_scale) or self.noise_scale < 0:
            raise ValueError("ConvertRequest: noise_scale must be finite and >= 0")
        self.chunk_frames, self.max_chunk_frames = int(chunk_frames), int(max_chunk_frames)
        if self.chunk_frames < 1 or self.max_chunk_frames < self.chunk_frames:
            raise ValueError("ConvertRequest: need 1 <= chunk_frames <= max_chunk_frames (got %d, %d)"
                             % (self.chunk_frames, self.max_chunk_frames))

    def model_samples(self):
        """Samples at the model's rate: the length `resample` returns for the wave (librosa's fix_length)."""
        n = self.wave.numel()
        if self.in_sr == self.model_sr:
            return n
        return int(math.ceil(n * (float(self.model_sr) / self.in_sr)))

    def frames(self, n_fft):
        """Spectrogram frames of the request under an n_fft-point transform (DESIGN 7.2's formula, on the host)."""
        return spectrogram_frames(self.model_samples(), n_fft, self.hop_size)

    def __repr__(self):
        return "ConvertRequest(%d samples at %d Hz, sid %d -> %d)" % (self.wave.numel(), self.in_sr, self.sid_src, self.sid_tgt)


def spectrogram_frames(n_samples, n_fft, hop_size):
    """Frames `spectrogram` gives an n-sample row (`mbv_spectrogram_frames`, restated for the host side of pooled
    conversion): 0 where torch.stft would refuse a row that short."""
    padded = int(n_samples) + 2 * ((int(n_fft) - int(hop_size)) // 2)
    return 0 if padded < n_fft else 1 + (padded - int(n_fft)) // int(hop_size)


_STAGES = ("text_encoder", "duration_predictor", "alignment_and_projection", "flow",
           "waveform_decoder")


class _Node(nn.Module):
    """Parameter container mirroring one reference sub-module (no compute)."""

    def forward(self, *a, **k):
        raise NotImplementedError(
            "this sub-module only holds parameters; the computation runs inside "
            "SynthesizerTrn.infer / .dec on the HIP path")


class _Decoder(_Node):
    """`net.dec(z, g=None)` -> (y_g_hat, y_mb_hat, spec, phase)  (models.py:344-377 / 430-467).
    `net.dec(z, g=g, lengths=lens)` (extension) -> (o, None, None, None): the row-exact ragged decode, every row
    bitwise its stand-alone decode (`SynthesizerTrn._decode_ragged`)."""

    def forward(self, x, g=None, lengths=None):
        if lengths is not None:
            return self._owner()._decode_ragged(x, g, lengths), None, None, None
        return self._owner()._decode(x, g)


class _SpeakerEmbedding(_Node):
    """`net.emb_g(sid)` -> [B, gin]  (models.py:654-655, 705)."""

    def forward(self, sid):
        return self._owner()._speaker_embedding(sid)


class Timings(dict):
    """The reference's `timings` dict (seconds per stage, models.py:698-737), filled lazily from
    HIP events so that `infer` itself never blocks: the first READ of any kind (indexing, get,
    items/keys/values, iteration, copy, ==, repr, json.dumps, pickle, dict(t)) waits for the call's
    last kernel and fills in the five stage times.  Until then the stored values are NaN
    placeholders.  The handle keeps the events of its last 8 calls (`mbv_stage_times_ms_at`): a dict
    read after more than 7 later calls on the same model stays NaN."""

    def __init__(self, owner, ticket):
        super().__init__((k, float("nan")) for k in _STAGES)
        self._owner, self._ticket, self._done = owner, ticket, False

    def _resolve(self):
        if not self._done:
            self._done = True
            vals = self._owner._stage_times(self._ticket)
            self._owner = None
            for k, v in zip(_STAGES, vals):
                dict.__setitem__(self, k, v)
        return self

    def __getitem__(self, k):
        return dict.__getitem__(self._resolve(), k)

    def get(self, k, default=None):
        return dict.get(self._resolve(), k, default)

    def items(self):
        return dict.items(self._resolve())

    def keys(self):
        return dict.keys(self._resolve())

    def values(self):
        return dict.values(self._resolve())

    def __iter__(self):
        return dict.__iter__(self._resolve())

    def copy(self):
        return dict(dict.items(self._resolve()))

    def __eq__(self, other):
        if isinstance(other, Timings):
            other._resolve()
        return dict.__eq__(self._resolve(), other)

    def __ne__(self, other):
        return not self.__eq__(other)

    __hash__ = None

    def __reduce__(self):
        return (dict, (self.copy(),))

    def __repr__(self):
        return dict.__repr__(self._resolve())


class SynthesizerTrn(nn.Module):
    """Synthesizer (inference path) — constructor surface of `models.py:573-599`."""

    def __init__(self, n_vocab, spec_channels, segment_size, inter_channels, hidden_channels,
                 filter_channels, n_heads, n_layers, kernel_size, p_dropout, resblock,
                 resblock_kernel_sizes, resblock_dilation_sizes, upsample_rates,
                 upsample_initial_channel, upsample_kernel_sizes, gen_istft_n_fft,
                 gen_istft_hop_size, n_speakers=0, gin_channels=0, use_sdp=False,
                 ms_istft_vits=False, mb_istft_vits=False, subbands=False, istft_vits=False,
                 **kwargs):
        super().__init__()
        self.cfg: ModelConfig = config_from_ctor(
            n_vocab, spec_channels, segment_size, inter_channels, hidden_channels,
            filter_channels, n_heads, n_layers, kernel_size, p_dropout, resblock,
            resblock_kernel_sizes, resblock_dilation_sizes, upsample_rates,
            upsample_initial_channel, upsample_kernel_sizes, gen_istft_n_fft, gen_istft_hop_size,
            n_speakers=n_speakers, gin_channels=gin_channels, use_sdp=use_sdp,
            ms_istft_vits=ms_istft_vits, mb_istft_vits=mb_istft_vits, subbands=subbands,
            istft_vits=istft_vits)
        # attributes the reference exposes (models.py:602-624)
        self.n_vocab, self.spec_channels, self.segment_size = n_vocab, spec_channels, segment_size
        self.inter_channels, self.hidden_channels = inter_channels, hidden_channels
        self.filter_channels, self.n_heads, self.n_layers = filter_channels, n_heads, n_layers
        self.kernel_size, self.p_dropout, self.resblock = kernel_size, p_dropout, resblock
        self.resblock_kernel_sizes = resblock_kernel_sizes
        self.resblock_dilation_sizes = resblock_dilation_sizes
        self.upsample_rates, self.upsample_initial_channel = upsample_rates, upsample_initial_channel
        self.upsample_kernel_sizes = upsample_kernel_sizes
        self.n_speakers, self.gin_channels = n_speakers, gin_channels
        self.ms_istft_vits, self.mb_istft_vits, self.istft_vits = ms_istft_vits, mb_istft_vits, istft_vits
        self.use_sdp = use_sdp

        self._build_parameter_tree()
        self._handle = None
        self._handle_device = None
        self._synced_sig = None
        self._ticket = 0
        # blended voices: the slots, the live `Speaker` of each, and who holds which
        self._voice_slots = SpeakerSlots()
        self._voices = {}
        self._voice_holders = {}

    # ------------------------------------------------------------------ params
    def _build_parameter_tree(self):
        from . import synth
        init = synth.make_state_dict(self.cfg, seed=1234)    # deterministic "random init"
        roots = {"dec": _Decoder(), "emb_g": _SpeakerEmbedding()}
        for name, shape in param_shapes(self.cfg).items():
            parts = name.split(".")
            node = self
            for part in parts[:-1]:
                child = node._modules.get(part)
                if child is None:
                    if node is self and part in roots:
                        child = roots[part]
                        object.__setattr__(child, "_owner", weakref.ref(self))
                    else:
                        child = _Node()
                    node.add_module(part, child)
                node = child
            value = torch.from_numpy(np.ascontiguousarray(init[name]))
            if name == "dec.updown_filter":
                node.register_buffer(parts[-1], value)
            else:
                node.register_parameter(parts[-1], nn.Parameter(value, requires_grad=False))

    def _weights_signature(self):
        sig = []
        for t in list(self.parameters()) + list(self.buffers()):
            sig.append((t.data_ptr(), t._version))
        return tuple(sig)

    # ------------------------------------------------------------------ handle
    def _device(self):
        return next(self.parameters()).device

    def _ensure_handle(self):
        dev = self._device()
        if dev.type != "cuda":
            raise RuntimeError("SynthesizerTrn (MI355X path) has no CPU implementation: move the "
                               "model to a ROCm device with .to('cuda') before calling infer/dec")
        idx = dev.index if dev.index is not None else torch.cuda.current_device()
        L = _capi.lib()
        if self._handle is not None and self._handle_device != idx:
            L.mbv_destroy(self._handle)
            self._handle, self._synced_sig = None, None
        if self._handle is None:
            c = self._config_struct(idx)
            h = C.c_void_p()
            rc = L.mbv_create(C.byref(c), C.byref(h))
            if rc:
                raise _capi.MbvError("mbv_create failed: %s" % L.mbv_last_error(None).decode())
            self._handle, self._handle_device = h, idx
            fresh = True
        else:
            fresh = False
        sig = self._weights_signature()
        if sig != self._synced_sig:
            self._upload_weights()
            self._synced_sig = sig
        if fresh and self._voices:
            # a handle re-created on another device starts without voices: the catalogue is defined again (a
            # vector voice from the row it was given, moved along)
            voices = [self._voices[k] for k in sorted(self._voices)]
            for v in voices:
                if v._vector is not None:
                    v._vector = v._vector.to(dev)
            with torch.cuda.device(dev):
                self._define_voices(self._handle, voices)
        return self._handle

    def _config_struct(self, device_index=0):
        c = _capi.MbvConfig()
        c.struct_bytes = C.sizeof(_capi.MbvConfig)
        cfg = self.cfg
        c.n_vocab, c.inter_channels, c.hidden_channels = cfg.n_vocab, cfg.inter_channels, cfg.hidden_channels
        c.filter_channels, c.n_heads, c.n_layers = cfg.filter_channels, cfg.n_heads, cfg.n_layers
        c.kernel_size, c.upsample_initial_channel = cfg.kernel_size, cfg.upsample_initial_channel
        c.spec_channels = cfg.spec_channels
        for j in range(3):
            c.resblock_kernel_sizes[j] = cfg.resblock_kernel_sizes[j]
            for q, d in enumerate(cfg.resblock_dilation_sizes[j]):
                c.resblock_dilations[j][q] = d
        c.resblock_type = int(cfg.resblock)
        c.n_speakers, c.gin_channels = cfg.n_speakers, cfg.gin_channels
        c.decoder = int(cfg.decoder)
        c.device = device_index
        c.use_sdp = int(bool(cfg.use_sdp))
        return c

    def _upload_weights(self):
        L = _capi.lib()
        for name, t in self.state_dict().items():
            a = t.detach().to(device="cpu", dtype=torch.float32).contiguous().numpy()
            shape = (C.c_int64 * a.ndim)(*a.shape)
            _capi.check(self._handle, L.mbv_load_weight(self._handle, name.encode(),
                                                        a.ctypes.data_as(C.c_void_p), shape, a.ndim),
                        "mbv_load_weight(%s)" % name)
        self._launch(self._handle, "mbv_finalize_weights")

    def export_arena(self):
        """The folded, packed weight arena of this model as one flat fp32 device tensor (`mbv_export_arena`):
        what rank 0 broadcasts in a sharded run instead of the state dict (dist.broadcast_arena)."""
        h = self._ensure_handle()
        L = _capi.lib()
        n = int(L.mbv_arena_floats(h))
        if n <= 0:
            raise _capi.MbvError(L.mbv_last_error(h).decode())
        dev = self._device()
        flat = torch.empty(n, device=dev, dtype=torch.float32)
        with torch.cuda.device(dev):
            self._launch(h, "mbv_export_arena", flat, n)
        return flat

    def import_arena(self, flat):
        """Take the weights from another process's `export_arena()` (same configuration, same library build):
        no state dict, no host-side weight-norm fold, no upload.  The module's own parameters keep whatever
        they held (the synthetic init) and are NOT what the kernels use afterwards; a later `load_state_dict`
        replaces the imported weights again."""
        dev = self._device()
        if dev.type != "cuda":
            raise RuntimeError("move the model to a ROCm device first (.to('cuda')): the arena lives on the GPU")
        flat = flat.to(device=dev, dtype=torch.float32).contiguous()
        self._synced_sig = self._weights_signature()      # _ensure_handle: nothing to upload
        try:
            self._call("mbv_import_arena", flat, flat.numel())
        except Exception:
            self._synced_sig = None
            raise

    def refresh_weights(self):
        """Force a re-fold/re-upload (only needed after in-place edits through `.data`)."""
        self._synced_sig = None

    def _stream(self, dev=None):
        return C.c_void_p(torch.cuda.current_stream(self._device() if dev is None else dev).cuda_stream)

    def __del__(self):
        try:
            if getattr(self, "_handle", None) is not None:
                _capi.lib().mbv_destroy(self._handle)
                self._handle = None
        except Exception:
            pass

    # ------------------------------------------------------------------ helpers
    @staticmethod
    def _ptr(t):
        return C.c_void_p(t.data_ptr()) if t is not None else None

    def _launch(self, h, name, *args, stream=None):
        """The library entry `name` on handle `h`, inside a device scope the caller holds: tensors among `args` go as
        their addresses and the HIP stream goes last — `stream` when a caller with several launches looked it up once,
        else the current one; False: the entry takes none.  A failure raises MbvError."""
        args = [C.c_void_p(a.data_ptr()) if isinstance(a, torch.Tensor) else a for a in args]
        if stream is not False:
            args.append(self._stream() if stream is None else stream)     # (a null stream is falsy: test for None)
        _capi.check(h, getattr(_capi.lib(), name)(h, *args), name)

    def _call(self, name, *args, stream=None):
        """The preamble of every entry: the handle (created, weights uploaded), the model's device, then `_launch`."""
        h = self._ensure_handle()
        dev = self._device()
        with torch.cuda.device(dev):
            self._launch(h, name, *args, stream=self._stream(dev) if stream is None else stream)

    # ------------------------------------------------------------------ seeded noise
    def _fill_noise(self, h, blocks, stream=None):
        """ONE `mbv_randn_blocks` launch inside a device scope the caller holds: `blocks` is a list of
        (address, stride, channels, first, count, seed, purpose, row)."""
        arr = (_capi.MbvRandnBlock * len(blocks))()
        for k, (dst, stride, channels, first, count, seed, purpose, row) in zip(arr, blocks):
            k.dst, k.stride, k.channels, k.first, k.count = dst, stride, channels, first, count
            k.seed, k.purpose, k.row = seed, purpose, row
        self._launch(h, "mbv_randn_blocks", arr, len(blocks), stream=stream)

    def _seeded_rows(self, h, seeds, channels, frames, purpose, stream=None):
        """[B, channels, frames] fp32: row b from the sub-stream seeds[b] = (seed, row), in one launch."""
        out = torch.empty(len(seeds), channels, frames, device=self._device(), dtype=torch.float32)
        self._fill_noise(h, [(out.data_ptr() + 4 * b * channels * frames, frames, channels, 0, frames, s, purpose, row)
                             for b, (s, row) in enumerate(seeds)], stream=stream)
        return out

    @torch.no_grad()
    def randn(self, seed, channels, frames, purpose=0, row=0, first=0):
        """[channels, frames] fp32 standard normals on the model's device from the seeded generator (DESIGN 7.13,
        `mbv_randn_blocks`): element (c, t) is a function of (seed, purpose, row, c, first + t) alone.  purpose: 0 the
        prior draw of `infer`, 1 the SDP draw, 2 the posterior draw; `row` the sub-stream a batched entry gives its
        row b under an int seed.  Neither torch generator is touched."""
        seed = _seed_value(seed)
        channels, frames, purpose, row, first = int(channels), int(frames), int(purpose), int(row), int(first)
        if channels < 1 or frames < 0 or first < 0 or first + frames > 1 << 30:
            raise ValueError("randn: need channels >= 1 and 0 <= first <= first + frames <= 2^30")
        if purpose not in (0, 1, 2) or not 0 <= row < 1 << 32:
            raise ValueError("randn: purpose must be 0, 1 or 2 and row in [0, 2^32)")
        h = self._ensure_handle()
        dev = self._device()
        with torch.cuda.device(dev):
            out = torch.empty(channels, frames, device=dev, dtype=torch.float32)
            self._fill_noise(h, [(out.data_ptr(), frames, channels, first, frames, seed, purpose, row)])
        return out

    def noise_runs(self):
        """`mbv_randn_blocks` launches made on this model's handle so far (`mbv_noise_runs`): a seeded call costs one
        per noise tensor it needs, however many rows or requests it serves."""
        return int(_capi.lib().mbv_noise_runs(self._ensure_handle()))

    def _check_inputs(self, x, x_lengths, sid):
        dev = self._device()
        if x.dim() != 2:
            raise ValueError("x must be [B, T] token ids")
        if x_lengths.dim() != 1 or x_lengths.shape[0] != x.shape[0]:
            raise ValueError("x_lengths must be [B]")
        x = x.to(device=dev, dtype=torch.int64).contiguous()
        x_lengths = x_lengths.to(device=dev, dtype=torch.int64).contiguous()
        if self.n_speakers > 0:
            if sid is None:
                raise ValueError("sid is required for a multi-speaker model (models.py:704-705)")
            sid = _sid_tensor(sid).to(device=dev, dtype=torch.int64).contiguous()
            if sid.shape != (x.shape[0],):
                raise ValueError("sid must be [B]")
        else:
            sid = None
        return x, x_lengths, sid

    def _check_durations(self, durations, B, T, length_scale):
        """Given durations -> (contiguous device tensor [B, T], dtype code of mbv_set_durations)."""
        if float(length_scale) != 1.0:
            raise ValueError("durations= are used as given: length_scale must be 1 (scale the durations instead)")
        if not torch.is_tensor(durations):
            raise ValueError("durations must be a tensor [B, T_text] or [B, 1, T_text]")
        if durations.dim() == 3 and durations.shape[1] == 1:
            durations = durations[:, 0]
        if tuple(durations.shape) != (B, T):
            raise ValueError("durations must be [B, T_text] or [B, 1, T_text] = [%d, %d], got %s"
                             % (B, T, tuple(durations.shape)))
        durations, code = _durations_code(durations)
        return durations.to(device=self._device()).contiguous(), code

    def _stage_times(self, ticket):
        if self._handle is None or ticket[0] is not self._handle:
            return [float("nan")] * 5               # the handle was re-created (device move)
        buf = (C.c_float * 5)()
        with torch.cuda.device(self._device()):
            if _capi.lib().mbv_stage_times_ms_at(self._handle, ticket[1], C.byref(buf)):
                return [float("nan")] * 5           # more than 8 later calls: the events were reused
        return [v * 1e-3 for v in buf]              # reference reports seconds

    # ------------------------------------------------------------------ API
    _OUTPUT_NAMES = ("o", "o_mb", "spec", "phase", "attn", "y_mask", "z", "z_p", "m_p", "logs_p")

    @torch.no_grad()
    def _run(self, x, x_lengths, sid, noise_scale, length_scale, max_len, decode,
             frames_hook=None, noise_scale_w=1., noise_w=None, outputs=None, stat_reduce=None,
             prior_rows=None, trim=False, ragged=False, durations=None, seed=None, marks_out=None, extra_frames=None,
             fit_frames=None, fit_bounds=FIT_BOUNDS, gain=None, gain_out=None, gain_max_len=None):
        """One encode + synthesize pair.
          outputs      None = every tensor of the reference's 8-tuple; or a collection of names from
                       _OUTPUT_NAMES: only those are materialised (the others come back as None and
                       their stores never happen — `outputs=("o",)` is the waveform-only launch)
          stat_reduce  sharded runs: called with the device tensor [T'max, error flag] BEFORE the
                       one host read, reduces it in place over the ranks (all_reduce MAX), so that
                       every rank pads to the global T'max and every rank raises when any does
          frames_hook  host-side override of T' (tests: pad a sub-batch like its parent batch)
          prior_rows   (lo, hi, B_global): draw the prior noise for the whole global batch and use
                       rows lo:hi (ranks seeded alike then reproduce the single-process draw)
          trim         opt-in trimmed decode (see `infer`)
          ragged       opt-in row-exact ragged decode (see `infer`)
          durations    frames per token to use instead of the predicted ones (see `infer`)
          seed         None = both draws come from torch's generators; else (see `infer`) the SDP draw and the prior
                       draw are one `mbv_randn_blocks` launch each and no generator is touched.  A sharded caller
                       passes the `RowSeeds` of its own rows (row = the global row index)
          marks_out    a list: receives one host list per row, the token marks of `infer_stream(marks=True)` (one
                       `mbv_token_marks` launch; they ride in the read-back of T'max, with the rows' x_lengths)
          length_scale, extra_frames, fit_frames, fit_bounds    the prosody controls (see `infer`): with any of them one
                       `mbv_shape_durations` launch follows the encode, where `mbv_set_durations` would stand; the
                       fit's factors and statuses ride in the same read-back and are left in `self.last_fit`
          gain, gain_out, gain_max_len    per-token volume (see `infer_stream`): gain_out, a list, receives the frame
                       gains [B, F + 1], F = T'max clipped to gain_max_len, from one `mbv_frame_gain` launch behind
                       the read-back (which tells F), in front of the synthesize; no synchronisation of its own"""
        h = self._ensure_handle()
        L = _capi.lib()
        x, x_lengths, sid = self._check_inputs(x, x_lengths, sid)
        dev, B, T = x.device, x.shape[0], x.shape[1]
        seeds = _row_seeds(seed, B)
        if seeds is not None and noise_w is not None:
            raise ValueError("seed= and an explicit noise_w= exclude each other")
        length_scale, scale, extra, fit = _prosody_args("infer", length_scale, extra_frames, fit_frames, fit_bounds,
                                                        durations, B, T)
        shaped = scale is not None or extra is not None or fit is not None
        gain = _gain_arg("infer", gain, B, T)
        self.last_fit = None
        if durations is not None:
            durations, dur_dtype = self._check_durations(durations, B, T, length_scale)
        I = self.cfg.inter_channels
        if outputs is None:
            want = set(self._OUTPUT_NAMES)
        else:
            want = set(outputs)
            unknown = want - set(self._OUTPUT_NAMES)
            if unknown:
                raise ValueError("unknown output name(s) %s (known: %s)" % (sorted(unknown), ", ".join(self._OUTPUT_NAMES)))
        with torch.cuda.device(dev):
            stream = self._stream()
            y_lengths = torch.empty(B, dtype=torch.int64, device=dev)
            if self.cfg.use_sdp:
                # the reference draws on the default CPU generator and moves it over (models.py:94);
                # a sharded caller passes its block of the full-batch draw instead
                if seeds is not None:
                    noise_w = self._seeded_rows(h, seeds, 2, T, _capi.NOISE_SDP, stream=stream)
                elif noise_w is None:
                    noise_w = torch.randn(B, 2, T)
                if tuple(noise_w.shape) != (B, 2, T):
                    raise ValueError("noise_w must be [B, 2, T_text]")
                noise_w = noise_w.to(device=dev, dtype=torch.float32).contiguous()
            else:
                noise_w = None
            self._launch(h, "mbv_encode", x, x_lengths, sid, B, T, float(length_scale), noise_w, float(noise_scale_w),
                         y_lengths, stream=stream)
            if durations is not None:
                self._launch(h, "mbv_set_durations", durations, dur_dtype, B, T, y_lengths, stream=stream)
            fit_dev = None
            if shaped:
                scale = None if scale is None else scale.to(dev)
                extra = None if extra is None else extra.to(dev)
                fit_host = None
                if fit is not None:             # one mbv_fit_result (8 bytes) a row: it rides with the int64 lengths
                    fit_host = (_capi.MbvFit * B)(*fit)
                    fit_dev = torch.empty(B, dtype=torch.int64, device=dev)
                self._launch(h, "mbv_shape_durations", scale, extra, fit_host, B, T, fit_dev, y_lengths, stream=stream)
            lo, hi = torch.aminmax(y_lengths)
            stat = torch.stack((hi, -lo))           # [T'max, > 0 iff an utterance was flagged -1]
            if stat_reduce is not None:
                stat_reduce(stat)
            if marks_out is not None:               # [B, T + 1] exclusive prefix sums, in the same read-back
                marks_dev = torch.empty(B, T + 1, dtype=torch.int64, device=dev)
                self._launch(h, "mbv_token_marks", marks_dev, T + 1, stream=stream)
                host = torch.cat((stat, y_lengths, x_lengths.to(torch.int64), marks_dev.reshape(-1))
                                 + (() if fit_dev is None else (fit_dev,))).tolist()
                Tp, flag, y_host = int(host[0]), int(host[1]), host[2:2 + B]
                for b in range(B):
                    n = max(0, min(int(host[2 + B + b]), T))
                    marks_out.append([int(v) for v in host[2 + 2 * B + b * (T + 1):2 + 2 * B + b * (T + 1) + n + 1]])
            elif ragged or fit_dev is not None:     # the B lengths ride in the same read-back
                host = torch.cat((stat, y_lengths) + (() if fit_dev is None else (fit_dev,))).tolist()
                Tp, flag, y_host = int(host[0]), int(host[1]), host[2:2 + B]
            else:
                Tp, flag = (int(v) for v in stat.tolist())      # the one host sync (commons.py:123)
            if fit_dev is not None:
                res = [_capi.fit_result(v) for v in host[len(host) - B:]]
                self.last_fit = ([r[0] for r in res], [r[1] for r in res])
            if flag > 0:                            # flagged by the kernels, no extra sync
                raise IndexError("index out of range in self (token id, x_lengths or sid outside the "
                                 "model's tables, or a duration outside the supported range: 2^20 frames a token, "
                                 "2^30 an utterance%s%s)" % ("" if durations is None else "; given durations must be non-negative integers",
                                                             "; a per-token scale must be finite and >= 0, extra frames >= 0" if shaped else ""))
            if frames_hook is not None:
                Tp = int(frames_hook(Tp))
            if gain is not None:                    # the scan of the encode is still in place: spread it over the frames
                Fg = Tp if gain_max_len is None else max(0, min(Tp, int(gain_max_len)))
                if Fg <= 0:
                    raise ValueError("max_len leaves no frames to decode")
                frame_gain = torch.empty(B, Fg + 1, device=dev, dtype=torch.float32)
                gain_dev = gain.to(dev)
                self._launch(h, "mbv_frame_gain", gain_dev, frame_gain, Fg + 1, Fg, stream=stream)
                gain_out.append(frame_gain)
            # the reference draws randn_like(m_p) even at noise_scale == 0 (models.py:729)
            if seeds is not None:
                # a function of (seed, row, channel, frame): no generator, no dependence on the batch or its padding;
                # at noise_scale == 0 nothing reads it and no generator has to advance
                noise = None
                if float(noise_scale) != 0.0:
                    noise = self._seeded_rows(h, seeds, I, Tp, _capi.NOISE_PRIOR, stream=stream)
            elif prior_rows is not None:
                # sharded run: the draw of the WHOLE batch, this shard's rows — also at noise_scale == 0, so that
                # the device generator advances exactly as in a single-process run of the full batch (a later
                # noisy call in the same process then still reproduces the single-process draws).  Large draws take
                # only the Philox calls that hold the shard's rows (rows_of_randn.py, verified against the full draw
                # on first use), so the cost does not grow with the world size.
                r_lo, r_hi, b_all = prior_rows
                from .rows_of_randn import randn_rows       # own rows of the full-batch draw, generator state included
                noise = randn_rows(r_lo, r_hi, b_all, (I, Tp), dev)
                noise = noise.contiguous() if float(noise_scale) != 0.0 else None
            else:
                noise = torch.randn(B, I, Tp, device=dev, dtype=torch.float32)
            f32 = dict(device=dev, dtype=torch.float32)
            out = _capi.MbvOutputs()
            t = {}
            if "attn" in want:
                t["attn"] = torch.empty(B, 1, Tp, T, **f32)
            if "y_mask" in want:
                t["y_mask"] = torch.empty(B, 1, Tp, **f32)
            for k in ("z", "z_p", "m_p", "logs_p"):
                if k in want:
                    t[k] = torch.empty(B, I, Tp, **f32)
            Td = Tp if max_len is None else max(0, min(Tp, int(max_len)))
            if trim:
                if want & {"o_mb", "spec", "phase"}:
                    raise ValueError("trim=True materialises the waveform only: pass outputs=('o',) (+ attn / y_mask / z ...)")
                if self.cfg.decoder == DEC_SB:
                    raise ValueError("trim=True is built for the multiband / multistream decoders")
            if ragged:
                if trim:
                    raise ValueError("trim=True and ragged=True exclude each other")
                if want & {"o_mb", "spec", "phase"}:
                    raise ValueError("ragged=True materialises the waveform only: pass outputs=('o',) (+ attn / y_mask / z ...)")
            if decode and want & {"o", "o_mb", "spec", "phase"}:
                if Td <= 0:
                    raise ValueError("max_len leaves no frames to decode")
                o, o_mb, spec, phase = self._alloc_decoder_outputs(B, Td, dev, want)
                if trim and o is not None:
                    o.zero_()                         # tiles behind an utterance's end are never written
                t.update(o=o, o_mb=o_mb, spec=spec, phase=phase)
            for k, v in t.items():
                if v is not None:
                    setattr(out, k, v.data_ptr())
            self._ticket += 1
            keep = int(Td if max_len is not None else 0)
            if trim:
                self._launch(h, "mbv_set_option", b"trim", 1, stream=False)
            try:
                if ragged:
                    self._launch(h, "mbv_synthesize_ragged", Tp, noise, float(noise_scale), keep, C.byref(out),
                                 (C.c_int64 * B)(*y_host), stream=stream)
                else:
                    self._launch(h, "mbv_synthesize", Tp, noise, float(noise_scale), keep, C.byref(out), stream=stream)
            finally:
                if trim:
                    self._launch(h, "mbv_set_option", b"trim", 0, stream=False)
        timings = Timings(self, (h, int(L.mbv_ticket(h))))
        g = t.get
        return (g("o"), g("o_mb"), g("spec"), g("phase"), g("attn"), g("y_mask"),
                (g("z"), g("z_p"), g("m_p"), g("logs_p")), timings, y_lengths)

    def _alloc_decoder_outputs(self, B, Td, dev, want=None):
        f32 = dict(device=dev, dtype=torch.float32)
        spf = self.cfg.samples_per_frame
        w = (lambda k: True) if want is None else (lambda k: k in want)
        o = torch.empty(B, 1, spf * Td, **f32) if w("o") else None
        if self.cfg.decoder == DEC_SB:                         # models.py:300: (out, None, spec, phase)
            Fr = 64 * Td + 1
            return (o, None, torch.empty(B, 9, Fr, **f32) if w("spec") else None,
                    torch.empty(B, 9, Fr, **f32) if w("phase") else None)
        o_mb = None
        if w("o_mb"):
            if self.cfg.decoder == DEC_MS:
                o_mb = torch.empty(B, 4, spf * Td, **f32)     # zero-stuffed (models.py:463)
            else:
                o_mb = torch.empty(B, 4, (spf // 4) * Td, **f32)
        Fr = 16 * Td + 1
        spec = torch.empty(B, 4, 9, Fr, **f32) if w("spec") else None
        phase = torch.empty(B, 4, 9, Fr, **f32) if w("phase") else None
        return o, o_mb, spec, phase

    def infer(self, x, x_lengths, sid=None, noise_scale=1, length_scale=1, noise_scale_w=1.,
              max_len=None, outputs=None, trim=False, ragged=False, durations=None, seed=None, extra_frames=None,
              fit_frames=None, fit_bounds=FIT_BOUNDS):
        """-> (o, o_mb, spec, phase, attn, y_mask, (z, z_p, m_p, logs_p), timings)  (models.py:737)

        Per-token prosody (a float `length_scale` and nothing else launches what it always did).  With
        any of the three, ONE `mbv_shape_durations` launch follows the encode and replaces the predicted durations by
        w_t = ceil(exp(logw_t) * fl32(s_t * f)) + extra_t for the tokens below x_lengths:
          `length_scale`  may be a floating tensor [B, T_text] or [B, 1, T_text] (the reference's own broadcast,
                          models.py:717): s_t per token, finite and >= 0; 0 drops the token.  A tensor filled with s
                          is bitwise the float s.
          `extra_frames`  an integer tensor of that shape, >= 0: further frames of the token's own prior -- on a blank
                          or "sp" token a pause of known length (`frames_of_ms`).  Token marks include them.
          `fit_frames`    an int, or B ints on the host: each row gets the LARGEST fp32 factor f in `fit_bounds` whose
                          total D(f) stays within that many frames (found exactly, on the device).  A row that does not
                          fit even at the lower bound takes it and is reported with status 1 -- not an error; one that
                          fits at the upper bound takes that.  Nothing is padded: the remainder is the caller's, e.g. as
                          a turn pause.  `fit_bounds` = (lo, hi), default (0.5, 2.0): a convention for "still sounds
                          like speech", not a measurement.  Afterwards `net.last_fit` = ([f_b], [status_b]).
        Without a tensor, `extra_frames` and `fit_frames` use the float `length_scale` as s_t.  None of the three goes
        with `durations=` (ValueError).  A negative, infinite or NaN scale, or a negative extra, below x_lengths[b]
        raises IndexError after the call's one read-back, like an invalid token id.

        `seed` (extension, default None = the noise comes from torch's two generators, launch for launch as before):
        reproducible noise.  An int s gives row b the sub-stream (s, row=b); a length-B sequence or
        integer tensor gives row b (seed_b, row=0), so `infer(x[b:b+1], ..., seed=[s_b])` draws what row b of
        `infer(x, ..., seed=[s_0 .. s_{B-1}])` draws.  Seeds are integers in [0, 2^64) (TypeError for bool / float,
        ValueError for a wrong count or range).  The prior draw, and the SDP draw of a `use_sdp` model, are one
        `mbv_randn_blocks` launch each on the device (`net.randn` gives the same values); both torch generators stay
        exactly where they were.

        `durations` (extension, default None = the predicted durations, launch for launch as before): frames per
        token, [B, T_text] or [B, 1, T_text] (e.g. the `w` of `align`), non-negative integers of any dtype.  They
        are used as given, masked by x_lengths, with y_lengths = max(sum, 1): `length_scale` must stay 1 and
        `noise_scale_w` is without effect (the duration predictor still runs; its result is replaced).  A negative
        or non-integer entry raises IndexError after the call's one read-back, like an invalid token id.

        `outputs` (extension, default None = the reference's full tuple): names of the tensors to
        materialise; the rest of the tuple is None.  A caller that only takes `[0]`
        (tts_vits.py:134-137, synthesis_module.py:178-189) passes `outputs=("o",)` and gets the
        waveform-only launch of the fused iSTFT+PQMF stage (no spec / phase / o_mb / attn stores).

        `trim` (extension, default False; needs `outputs` without o_mb / spec / phase): opt-in trimmed decode for
        ragged batches — per utterance the decoder only computes what its valid 256 * y_lengths[b] samples depend
        on (frames below y_lengths[b] + 32).  Those samples are bitwise the default's; the padded region of `o`,
        which the reference's unmasked decoder fills with defined values, comes back as zeros.

        `ragged` (extension, default False; same condition on `outputs`; excludes `trim`): opt-in row-exact ragged
        decode — the valid 256 * y_lengths[b] samples of row b are bitwise `net.dec(z[b:b+1, :, :y_lengths[b]], g)`
        alone, i.e. what a one-utterance-per-call service (tts_vits.py:122-139) emits, whatever else is in the
        batch; the rest of the row is zeros.  The default (and `trim`) keep the reference's batched values, where
        the last ~25 frames of a row depend on what the unmasked decoder computes behind its end.  The B lengths
        are read back in the call's one host synchronisation."""
        r = self._run(x, x_lengths, sid, noise_scale, length_scale, max_len, decode=True,
                      noise_scale_w=noise_scale_w, outputs=outputs, trim=trim, ragged=ragged, durations=durations,
                      seed=seed, extra_frames=extra_frames, fit_frames=fit_frames, fit_bounds=fit_bounds)
        return r[:8]

    def infer_z_only(self, x, x_lengths, sid=None, noise_scale=1, length_scale=1, noise_scale_w=1.,
                     max_len=None, durations=None, seed=None, extra_frames=None, fit_frames=None,
                     fit_bounds=FIT_BOUNDS):
        """-> (attn, y_mask, (z, z_p, m_p, logs_p), timings)  (models.py:742-788); `durations`, `seed` and the prosody
        controls (a tensor `length_scale`, `extra_frames`, `fit_frames`, `fit_bounds`) as in `infer`"""
        r = self._run(x, x_lengths, sid, noise_scale, length_scale, None, decode=False,
                      noise_scale_w=noise_scale_w, durations=durations, seed=seed, extra_frames=extra_frames,
                      fit_frames=fit_frames, fit_bounds=fit_bounds)
        return r[4], r[5], r[6], r[7]

    def infer_with_lengths(self, x, x_lengths, sid=None, noise_scale=1, length_scale=1,
                           max_len=None, noise_scale_w=1., outputs=None, trim=False, ragged=False, seed=None,
                           extra_frames=None, fit_frames=None, fit_bounds=FIT_BOUNDS):
        """`infer` plus the per-utterance frame counts y_lengths [B] (int64) — what a batched
        caller needs to trim the padded waveforms (valid samples = 256 * y_lengths).  `seed` and the prosody controls
        as in `infer`."""
        r = self._run(x, x_lengths, sid, noise_scale, length_scale, max_len, decode=True,
                      noise_scale_w=noise_scale_w, outputs=outputs, trim=trim, ragged=ragged, seed=seed,
                      extra_frames=extra_frames, fit_frames=fit_frames, fit_bounds=fit_bounds)
        return r[:8], r[8]

    def _z_g(self, z, g, checked=True):
        """(z, g) as the decoder entries read them: fp32, contiguous, on the device, g as [B, gin].  `checked` (every
        caller but `_decode_into`, whose z and g are the model's own): z must be [B, inter, T'], and a model
        without speakers drops g."""
        dev = self._device()
        if checked and (z.dim() != 3 or z.shape[1] != self.cfg.inter_channels):
            raise ValueError("z must be [B, %d, T']" % self.cfg.inter_channels)
        z = z.to(device=dev, dtype=torch.float32).contiguous()
        if g is not None:
            if checked and self.cfg.gin_channels == 0:
                g = None
            else:
                g = g.to(device=dev, dtype=torch.float32).reshape(z.shape[0], self.cfg.gin_channels).contiguous()
        return z, g

    @staticmethod
    def _outputs_struct(outs, B):
        """(o, o_mb, spec, phase), any of them None -> the `MbvOutputs` that names them."""
        out = _capi.MbvOutputs()
        for name, t in zip(("o", "o_mb", "spec", "phase"), outs):
            if t is not None:
                if not t.is_contiguous() or t.shape[0] != B:
                    raise ValueError("%s: a contiguous block of %d rows expected" % (name, B))
                setattr(out, name, t.data_ptr())
        return out

    def _decode_rows(self, entry, z, g, outs, *extra):
        """The decoder entry `entry`(z, g, *extra, B, T', outputs) into (o, o_mb, spec, phase), any of them None."""
        B, _, Tp = z.shape
        self._call(entry, z, g, *extra, B, Tp, C.byref(self._outputs_struct(outs, B)))

    @torch.no_grad()
    def _decode(self, z, g=None):
        z, g = self._z_g(z, g)
        outs = self._alloc_decoder_outputs(z.shape[0], z.shape[2], z.device)
        self._decode_rows("mbv_decode", z, g, outs)
        return outs

    @torch.no_grad()
    def _decode_ragged(self, z, g, lengths):
        """`net.dec(z, g, lengths=lens)[0]`: o [B, 1, 256 T'] whose row b is, over its first 256 * lens[b] samples,
        bitwise `net.dec(z[b:b+1, :, :lens[b]], g[b:b+1])[0]` (default mode; with "splitk" within fp32 rounding)
        and zero behind; z at and past a row's length is never read.  `lengths`: a sequence of ints or an integer
        tensor on either device (a device tensor is read back: one synchronisation)."""
        z, g = self._z_g(z, g)
        B, _, Tp = z.shape
        lens = _ints(lengths)
        if len(lens) != B:
            raise ValueError("lengths must hold one length per row of z")
        o = torch.empty(B, 1, self.cfg.samples_per_frame * Tp, device=z.device, dtype=torch.float32)
        self._call("mbv_decode_ragged", z, g, B, Tp, (C.c_int64 * B)(*lens), o)
        return o

    def ragged_classes(self, t_max, splitk=False):
        """The first z-length of every class of the row-exact ragged decode for lengths 1 .. t_max
        (`mbv_ragged_classes`, host only: no GPU needed): rows of one class share their decoder launches."""
        cfg = self._config_struct()
        n = _capi.lib().mbv_ragged_classes(C.byref(cfg), int(bool(splitk)), int(t_max), None, 0)
        if n < 1:
            raise ValueError("mbv_ragged_classes refused t_max=%r" % (t_max,))
        buf = (C.c_int32 * n)()
        _capi.lib().mbv_ragged_classes(C.byref(cfg), int(bool(splitk)), int(t_max), buf, n)
        return list(buf)

    def ragged_plan(self, lengths, t_frames=None, splitk=False):
        """(runs, run_of_row): the decoder runs a ragged call makes for rows of these z-lengths (`mbv_ragged_plan`,
        host only) — one per non-empty class, cut further only at 2 GiB tensors; run_of_row[b] = -1 for an empty row."""
        lens = _ints(lengths)
        B = len(lens)
        t_frames = max(max(lens), 1) if t_frames is None else int(t_frames)
        cfg = self._config_struct()
        rows = (C.c_int32 * B)()
        n = _capi.lib().mbv_ragged_plan(C.byref(cfg), int(bool(splitk)), B, t_frames, (C.c_int64 * B)(*lens), rows)
        if n < 0:
            raise ValueError("mbv_ragged_plan refused the lengths (outside [0, %d]?)" % t_frames)
        return n, list(rows)

    @torch.no_grad()
    def _decode_into(self, z, g, outs):
        """`net.dec` on a block of rows, writing into caller-owned (o, o_mb, spec, phase) — any may be None.
        dist.sharded_infer(overlap="halves") decodes a shard in two pieces with it."""
        self._decode_rows("mbv_decode", *self._z_g(z, g, checked=False), outs)

    @torch.no_grad()
    def _decode_masked_into(self, z, g, lengths, outs):
        """`_decode_into` on z * sequence_mask(lengths) (`mbv_decode_masked`): the decoder run `infer` makes, on a z
        of the caller's.  `lengths`: ints, one per row."""
        z, g = self._z_g(z, g, checked=False)
        lens = torch.as_tensor([int(v) for v in lengths], dtype=torch.int32).to(z.device)
        if lens.shape[0] != z.shape[0]:
            raise ValueError("lengths must hold one length per row of z")
        self._decode_rows("mbv_decode_masked", z, g, outs, lens)

    def tail_plan(self):
        """Rows (kind, stage, j, q, rate, reach) of `mbv_tail_plan` for this model's decoder (host only)."""
        cs = self._config_struct()
        buf = (C.c_int32 * (6 * 64))()
        n = _capi.lib().mbv_tail_plan(C.byref(cs), buf, 64)
        if n < 0 or n > 64:
            raise ValueError("mbv_tail_plan refused the configuration")
        return [tuple(buf[6 * i:6 * i + 6]) for i in range(n)]

    def tail_dropped(self):
        """Column tiles the "tail_once" maps left out on this handle so far (`mbv_tail_dropped`; synchronises)."""
        return int(_capi.lib().mbv_tail_dropped(self._ensure_handle()))

    # ------------------------------------------------------------------ streaming decode (stream.py)
    def decoder_context(self):
        """(L, R): the z-frames of left / right context any output sample of frame t depends on, [t - L, t + R]
        (`mbv_decoder_context`, host only: no GPU needed)."""
        return stream.decoder_context(self._config_struct())

    def dec_stream(self, z, g=None, chunk_frames=32, max_chunk_frames=256):
        """`dec(z, g)[0]` chunk by chunk: a `stream.DecodeStream` whose iteration yields (first_sample, o[:, :, a:b])
        views of one full-length `o`, one `mbv_decode_range` call per chunk.  Chunks start at `chunk_frames` and
        double up to `max_chunk_frames`.  The concatenation is bitwise `dec(z, g)[0]` (default mode)."""
        h = self._ensure_handle()
        z, g = self._z_g(z, g)
        return stream.DecodeStream(self, h, z, g, chunk_frames, max_chunk_frames)

    def stream_pool(self):
        """A `stream.StreamPool` of this model: `pool.add(st)` single-utterance streams of `dec_stream` /
        `infer_stream`, then `pool.step()` decodes the next chunk of each in one `mbv_decode_chunks` call — one decoder
        run per class of lengths (`chunks_plan`), every sample bitwise what the stream yields alone."""
        return stream.StreamPool(self)

    def chunks_plan(self, t_frames, splitk=False):
        """(runs, run_of_chunk): the decoder runs one pooled step makes for chunks of utterances of these z-lengths
        (`mbv_chunks_plan`, host only: no GPU needed)."""
        return self._plan_runs("mbv_chunks_plan", t_frames, splitk,
                               "mbv_chunks_plan refused the lengths (every t_frames must be >= 1, and at least one chunk)")

    def _plan_runs(self, entry, lengths, splitk, refusal):
        """(runs, run_of_item) of a host-only planner `entry`(config, splitk, n, int32 lengths, int32 run_of_item):
        `lengths` is a sequence of ints or an integer tensor; a negative return raises ValueError(refusal)."""
        t = _ints(lengths)
        n = len(t)
        cfg = self._config_struct()
        runs = (C.c_int32 * max(n, 1))()
        r = getattr(_capi.lib(), entry)(C.byref(cfg), int(bool(splitk)), n, (C.c_int32 * max(n, 1))(*t), runs)
        if r < 0:
            raise ValueError(refusal)
        return r, list(runs)[:n]

    def decoder_runs(self):
        """Decoder runs made on this model's handle so far (`mbv_decoder_runs`): the difference across a call is the
        number of launch chains it cost."""
        return int(_capi.lib().mbv_decoder_runs(self._ensure_handle()))

    @torch.no_grad()
    def infer_stream(self, x, x_lengths, sid=None, noise_scale=1, length_scale=1, noise_scale_w=1., max_len=None,
                     chunk_frames=32, max_chunk_frames=256, durations=None, seed=None, marks=False, extra_frames=None,
                     fit_frames=None, fit_bounds=FIT_BOUNDS, gain=None, pitch=None, pitch_compensate=True,
                     pitch_glide_frames=PITCH_GLIDE_FRAMES):
        """`infer(...)[0]` chunk by chunk.  Runs the text encoder, the duration predictor, the prior noise draw and the
        flows exactly as `infer` does (same random draws; `durations` and `seed` as in `infer`), then returns `dec_stream` of
        z * y_mask (truncated to max_len) with `y_lengths` set on the stream.  The concatenation is bitwise
        `infer(...)[0]` (default mode).
          marks  True: `st.marks` is one host list per row (the list itself for a single utterance) of x_lengths + 1
                 integers, the z-frame at which every token starts: the exclusive prefix sums of the durations the
                 length regulator used (predicted or given), the last entry their sum, all clipped to the frames the
                 stream keeps (`max_len`).  One `mbv_token_marks` launch; the integers ride in the read-back the call
                 already makes, so there is no second host synchronisation.  False (default): `st.marks` is None and
                 nothing is added.
          a tensor `length_scale`, `extra_frames`, `fit_frames`, `fit_bounds`    the prosody controls of `infer`.  With
                 `fit_frames` the stream gets `st.fit_scale` and `st.fit_status`, one value per row (the value itself
                 for a single utterance); they too ride in the call's one read-back.  Else both are None.
          gain   per-token volume: a host sequence or CPU tensor [B, T_text] of linear factors, finite,
                 in [0, GAIN_MAX] (`gain_of_db` converts; checked here, a device tensor is refused).  The stream gets
                 `st.frame_gain`, fp32 [B, F + 1] on the device, F the frames the stream keeps: the gain of the token
                 that holds each frame, held behind a row's end (one `mbv_frame_gain` launch, no synchronisation).  The
                 decode is untouched: `st.o` is bitwise the stream without `gain=`.  The wire path (`stream_pcm16`,
                 `PcmPool.add`, `Turn.append`) picks `st.frame_gain` up and shapes the samples in front of its filter
                 and limiter.  None (default): `st.frame_gain` is None and nothing is launched.
          pitch  per-token pitch by varispeed, one utterance only (B = 1): a host sequence or CPU tensor
                 [1, T_text] of factors in [PITCH_MIN, PITCH_MAX] (`pitch_of_semitones` converts).  The model has no F0
                 input: token t is played p_t times faster by a time-warp kernel behind the decoder, so it sounds p_t
                 higher and its formants move with the pitch.  `pitch_compensate=True` (default) multiplies the
                 per-token `length_scale` by p_t (fp32, on the host; the tensor route of the prosody controls), so every
                 token keeps its length; False is plain varispeed.  Refused beside `durations=`.  The stream gets
                 `st.warp`, a `stream.WarpMap`: the rate of every kept frame (the pitch of the token that holds it, then
                 the mean over `pitch_glide_frames` frames either side; 0 = steps), the warped frame positions and the
                 warped length.  It needs the token marks, which ride in the read-back the call makes anyway (`st.marks`
                 is set too): no extra synchronisation, no extra encoder run.  The decode is untouched: `st.o` is bitwise
                 the stream made with the same effective `length_scale` and no pitch.  The wire path (`stream_pcm16`,
                 `PcmPool.add`, `Turn.append`) warps in front of its filter; `net.warp(o, st.warp)` is the one-shot
                 form.  None (default): `st.warp` is None and nothing is launched."""
        if pitch is not None:
            B, T = x.shape[0], x.shape[1]
            if B != 1:
                raise ValueError("infer_stream: pitch= takes ONE utterance (B = 1), got B = %d: the warped rows of a "
                                 "batch have different lengths; use infer_streams / PcmPool.admit" % B)
            pitch = _pitch_arg("infer_stream", pitch, B, T)
            if int(pitch_glide_frames) < 0:
                raise ValueError("infer_stream: pitch_glide_frames must be >= 0")
            length_scale = _pitch_scale("infer_stream", pitch, length_scale, durations, pitch_compensate)
        marks_out = [] if marks or pitch is not None else None
        gain_out = []
        r = self._run(x, x_lengths, sid, noise_scale, length_scale, None, decode=False,
                      noise_scale_w=noise_scale_w, outputs=("z", "y_mask"), durations=durations, seed=seed,
                      marks_out=marks_out, extra_frames=extra_frames, fit_frames=fit_frames, fit_bounds=fit_bounds,
                      gain=gain, gain_out=gain_out, gain_max_len=max_len)
        fitted = self.last_fit
        y_mask, z, y_lengths = r[5], r[6][0], r[8]
        Tp = z.shape[2]
        Td = Tp if max_len is None else max(0, min(Tp, int(max_len)))
        if Td <= 0:
            raise ValueError("max_len leaves no frames to decode")
        zd = (z * y_mask)[:, :, :Td].contiguous()
        g = None
        if self.n_speakers > 0:
            g = self._speaker_embedding(_sid_tensor(sid).to(self._device()))
        st = self.dec_stream(zd, g, chunk_frames, max_chunk_frames)
        st.y_lengths = y_lengths
        if marks_out is not None:
            rows = [[min(v, Td) for v in row] for row in marks_out]
            st.marks = rows[0] if len(rows) == 1 else rows
        if pitch is not None:
            st.warp = stream.WarpMap(stream.frame_rates(pitch[0].tolist(), st.marks, Td, pitch_glide_frames), st.spf,
                                     zd.device)
        if fitted is not None:
            st.fit_scale, st.fit_status = (v[0] if len(v) == 1 else v for v in fitted)
        if gain_out:
            st.frame_gain = gain_out[0]
        return st

    # ------------------------------------------------------------------ pooled admission
    @staticmethod
    def _pack_host(tensors, dev):
        """1-D tensors (or None), one per request -> (the device address of each, the tensors to keep alive while
        launches read them): host tensors travel in one concatenated copy per dtype, device tensors stay."""
        ptr, keep = [None] * len(tensors), []
        for dt in (torch.int32, torch.int64, torch.float32, torch.int16):
            host = [i for i, t in enumerate(tensors) if t is not None and not t.is_cuda and t.dtype == dt]
            if host:
                flat = torch.cat([tensors[i] for i in host]).to(dev)
                keep.append(flat)
                o = 0
                for i in host:
                    ptr[i] = flat.data_ptr() + flat.element_size() * o
                    o += tensors[i].numel()
        for i, t in enumerate(tensors):
            if t is not None and ptr[i] is None:
                t = t.to(dev)
                keep.append(t)
                ptr[i] = t.data_ptr()
        return ptr, keep

    @staticmethod
    def _draw_rows(I, lengths, dev):
        """One standard-normal block [1, I, T_i] per request, in list order, in one flat buffer -> (the buffer, the
        address of each block): the values and the generator's progress of N stand-alone randn(1, I, T_i) calls."""
        flat = torch.empty(I * sum(lengths), device=dev, dtype=torch.float32)
        ptr, o = [], 0
        for t in lengths:
            flat[o:o + I * t].view(1, I, t).normal_()
            ptr.append(flat.data_ptr() + 4 * o)
            o += I * t
        return flat, ptr

    def _seeded_blocks(self, h, items, seeds, channels, lengths, purpose, ptr, stream):
        """The blocks [channels, lengths[j]] of the seeded requests `items` (sub-stream (seeds[j], row 0)), back to
        back in one flat buffer, filled by ONE launch -> the buffer; ptr[items[j]] = the address of block j."""
        flat = torch.empty(channels * sum(lengths), device=self._device(), dtype=torch.float32)
        blocks, o = [], 0
        for i, s, t in zip(items, seeds, lengths):
            ptr[i] = flat.data_ptr() + 4 * o
            blocks.append((ptr[i], t, channels, 0, t, s, purpose, 0))
            o += channels * t
        self._fill_noise(h, blocks, stream=stream)
        return flat

    def _streams_of(self, reqs, z, g, y_all, pos):
        """One single-utterance `DecodeStream` per request over its own z and g; `y_lengths` is the one-element slice
        of `y_all` at the request's row."""
        out = []
        for i, r in enumerate(reqs):
            st = stream.DecodeStream(self, self._handle, z[i], g[i], r.chunk_frames, r.max_chunk_frames)
            st.y_lengths = y_all[pos[i]:pos[i] + 1]
            out.append(st)
        return out

    def admit_plan(self, t_text, splitk=False):
        """(runs, run_of_request): the front-half runs `infer_streams` makes for requests of these text lengths
        (`mbv_admit_plan`, host only: no GPU needed).  Requests share a padded run iff the conv planner sends every
        conv in front of the flows to the same kernel family for either text alone — today two classes, T <= 256 and
        beyond; with `splitk` one."""
        t = _ints(t_text)
        if not t:
            raise ValueError("admit_plan: no requests")
        if min(t) < 1:
            raise ValueError("admit_plan: empty text (every length must be >= 1)")
        return self._plan_runs("mbv_admit_plan", t, splitk, "mbv_admit_plan refused the lengths")

    def encoder_runs(self):
        """Text-encoder runs made on this model's handle so far (`mbv_encoder_runs`): the difference across a call is
        the number of front-half launch chains it cost."""
        return int(_capi.lib().mbv_encoder_runs(self._ensure_handle()))

    def shape_runs(self):
        """Launches of the prosody kernel made on this model's handle so far (`mbv_shape_runs`): one per call with a
        per-token `length_scale`, `extra_frames=` or `fit_frames=`, one per admission run that holds such a request,
        none otherwise."""
        return int(_capi.lib().mbv_shape_runs(self._ensure_handle()))

    def gain_runs(self):
        """Launches of the frame-gain kernel made on this model's handle so far (`mbv_gain_runs`): one per call with
        `gain=`, one per admission run that holds such a request, none otherwise."""
        return int(_capi.lib().mbv_gain_runs(self._ensure_handle()))

    @torch.no_grad()
    def frame_gain(self, gain, durations, y_lengths=None):
        """Per-token gains -> the frame gains a `wire.Envelope` takes, for users of the batch `infer` (DESIGN §7.20;
        `mbv_op_frame_gain`, the kernel `infer_stream(gain=)` runs).
          gain       host sequence / CPU tensor [B, T_text], as `infer_stream(gain=)`
          durations  what the length regulator used: `infer(...)[4]`, the path attn [B, 1, T', T_text] (summed over the
                     frames here), or frames per token [B, T_text] / [B, 1, T_text] (integers in any dtype)
          y_lengths  None = every row keeps the sum of its durations; else int64 [B] kept frames (after max_len)
        -> fp32 [B, F + 1] on the device, F = T' of attn, else the largest kept length (one host read)."""
        h = self._ensure_handle()
        dev = self._device()
        if not torch.is_tensor(durations):
            raise TypeError("frame_gain: durations must be a tensor (infer(...)[4], or frames per token)")
        F = None
        if durations.dim() == 4:
            if durations.shape[1] != 1:
                raise ValueError("frame_gain: attn must be [B, 1, T', T_text]")
            F = durations.shape[2]
            durations = durations.sum(2)
        if durations.dim() == 3 and durations.shape[1] == 1:
            durations = durations[:, 0]
        if durations.dim() != 2:
            raise ValueError("frame_gain: durations must be [B, T_text], [B, 1, T_text] or attn [B, 1, T', T_text]")
        B, T = durations.shape
        gain = _gain_arg("frame_gain", gain, B, T)
        with torch.cuda.device(dev):
            cum = torch.cumsum(durations.to(dev).round().to(torch.int64), 1)
            if y_lengths is None:
                y = cum[:, -1].contiguous()
            else:
                y = _valid_samples(y_lengths, B, dev, "y_lengths")
            if F is None:
                F = int(y.max())
            if F < 1:
                raise ValueError("frame_gain: no frames")
            out = torch.empty(B, F + 1, device=dev, dtype=torch.float32)
            self._launch(h, "mbv_op_frame_gain", cum.to(torch.int32).contiguous(), y, gain.to(dev), out, F + 1, F, B, T)
        return out

    @torch.no_grad()
    def infer_streams(self, requests):
        """Pooled admission: one single-utterance `DecodeStream` per `Request`, in order — what `StreamPool.add` takes —
        from ONE padded front-half run per class of `admit_plan` and ONE host read-back, instead of a launch chain and
        a read-back per request.

        Default mode: stream i is bitwise (z, g, y_lengths, schedule) what
        `infer_stream(x_i[None], [len_i], sid_i, noise_scale_i, length_scale_i, noise_scale_w_i, max_len_i,
        chunk_frames_i, max_chunk_frames_i, durations=d_i)` returns when those calls are made one after the other in
        list order from the same RNG state, and both generators (CPU: the SDP draws, device: the prior draws) end in
        the state those calls leave.  A request with `seed=` takes no part in that order: its stream is bitwise
        `infer_stream(x_i[None], ..., seed=[seed_i])` whatever else is in the list and wherever it stands, its draws touch
        no generator, and ONE `mbv_randn_blocks` launch fills the prior blocks of all seeded requests of the call (a
        second their SDP blocks); seeded and unseeded requests may be mixed, the unseeded ones drawing in list order
        among themselves.  With the option "splitk" the result is deterministic and within fp32 rounding
        of the stand-alone calls (a predicted duration may differ by a frame); "conv_bf16" is refused.

        All or nothing: a request with a token id / sid outside the model's tables or an unusable duration raises
        IndexError naming the request indices after the read-back, and no stream is created.  Refused before any
        launch (ValueError): a missing sid on a multi-speaker model, "conv_bf16"; `Request` itself refuses an empty
        text and durations with length_scale != 1."""
        reqs = list(requests)
        for i, r in enumerate(reqs):
            if not isinstance(r, Request):
                raise TypeError("infer_streams takes models.Request values (item %d is %s)" % (i, type(r).__name__))
            if self.n_speakers > 0 and r.sid is None:
                raise ValueError("request %d: sid is required for a multi-speaker model (models.py:704-705)" % i)
        if not reqs:
            return []
        h = self._handle_not_bf16("infer_streams", "admit with infer_stream, one request at a time")
        L = _capi.lib()
        dev = self._device()
        N, I = len(reqs), self.cfg.inter_channels
        t_text = [r.x.numel() for r in reqs]
        n_runs, run_of = self.admit_plan(t_text, splitk=L.mbv_get_option(h, b"splitk") != 0)
        members = [[i for i in range(N) if run_of[i] == k] for k in range(n_runs)]
        pos, first = [0] * N, []                   # request -> its row in y_all, run -> its first row
        for m in members:
            first.append(sum(len(q) for q in members[:len(first)]))
            for b, i in enumerate(m):
                pos[i] = first[-1] + b
        with torch.cuda.device(dev):
            hip_stream = self._stream(dev)
            keep = []                              # inputs of launches in flight
            noise_w = [None] * N
            seeded = [i for i in range(N) if reqs[i].seed is not None]
            drawn = [i for i in range(N) if reqs[i].seed is None]
            if self.cfg.use_sdp and drawn:         # the reference's draw, per request, on the default CPU generator
                flat_w = torch.cat([torch.randn(1, 2, t_text[i]).reshape(-1) for i in drawn]).to(dev)
                keep.append(flat_w)
                o = 0
                for i in drawn:
                    noise_w[i] = flat_w.data_ptr() + 4 * o
                    o += 2 * t_text[i]
            if self.cfg.use_sdp and seeded:        # every seeded request's [2, T_text], across classes: one launch
                keep.append(self._seeded_blocks(h, seeded, [reqs[i].seed for i in seeded], 2,
                                                [t_text[i] for i in seeded], _capi.NOISE_SDP, noise_w, hip_stream))
            dur, kept = self._pack_host([r.durations for r in reqs], dev)       # (None where none are given)
            keep += kept
            # [the N lengths | the marks of the requests that want them, t_text + 1 each]: one buffer, one read-back
            marked = [i for i in range(N) if reqs[i].marks or reqs[i].pitch is not None]
            mark_at, o = {}, N
            for i in marked:
                mark_at[i] = o
                o += t_text[i] + 1
            # ... | one mbv_fit_result (8 bytes) per request with fit_frames
            shaped = [r.scale is not None or r.extra is not None or r.fit is not None for r in reqs]
            fit_at = {}
            for i in range(N):
                if reqs[i].fit is not None:
                    fit_at[i] = o
                    o += 1
            # (the gains ride in the copy of the scale tables: one concatenated fp32 host tensor)
            f32_p, kept = self._pack_host([r.scale for r in reqs] + [r.gain for r in reqs], dev)
            scale_p, gain_p = f32_p[:N], f32_p[N:]
            keep += kept
            extra_p, kept = self._pack_host([r.extra for r in reqs], dev)
            keep += kept
            y_buf = torch.empty(o, dtype=torch.int64, device=dev)
            y_all = y_buf[:N]
            # ids (zero-padded to the run's longest text), lengths and sids of every run: ONE host tensor, one copy
            on_host = not any(r.x.is_cuda for r in reqs)
            parts = []
            for m in members:
                xs = [reqs[i].x for i in m] if on_host else [reqs[i].x.to(dev) for i in m]
                parts.append(torch.nn.utils.rnn.pad_sequence(xs, batch_first=True, padding_value=0).reshape(-1))
                tail = [t_text[i] for i in m] + ([reqs[i].sid for i in m] if self.n_speakers > 0 else [])
                parts.append(torch.tensor(tail, dtype=torch.int64) if on_host else torch.tensor(tail, dtype=torch.int64).to(dev))
            packed = torch.cat(parts).to(dev)
            keep.append(packed)
            sids, o = [], 0
            for k, m in enumerate(members):
                B, T = len(m), max(t_text[i] for i in m)
                ids, lens = packed.data_ptr() + 8 * o, packed.data_ptr() + 8 * (o + B * T)
                sid = packed[o + B * T + B:o + B * T + 2 * B] if self.n_speakers > 0 else None
                o += B * T + (2 * B if self.n_speakers > 0 else B)
                sids.append(sid)
                rows = (_capi.MbvEncRow * B)()
                for row, i in zip(rows, m):
                    r = reqs[i]
                    row.length_scale, row.noise_scale_w, row.noise_w = r.length_scale, r.noise_scale_w, noise_w[i]
                    row.durations, row.durations_dtype, row.t_text = dur[i], r.durations_dtype or 0, t_text[i]
                self._launch(h, "mbv_encode_rows", k, C.c_void_p(ids), C.c_void_p(lens), sid, B, T, rows,
                             C.c_void_p(y_all.data_ptr() + 8 * first[k]), stream=hip_stream)
                if any(shaped[i] for i in m):      # the run's shaped rows: one table-reading launch, in front of the marks
                    srows = (_capi.MbvShapeRow * B)()
                    for row, i in zip(srows, m):
                        if shaped[i]:
                            row.scale, row.extra = scale_p[i], extra_p[i]
                            if i in fit_at:
                                row.fit = _capi.MbvFit(*reqs[i].fit)
                                row.fit_out = y_buf.data_ptr() + 8 * fit_at[i]
                    self._launch(h, "mbv_shape_durations_rows", k, srows, B,
                                 C.c_void_p(y_all.data_ptr() + 8 * first[k]), stream=hip_stream)
                if any(i in mark_at for i in m):   # the run's marks: one table-reading launch
                    mrows = (_capi.MbvMarkRow * B)()
                    for row, i in zip(mrows, m):
                        if i in mark_at:
                            row.marks, row.count = y_buf.data_ptr() + 8 * mark_at[i], t_text[i] + 1
                    self._launch(h, "mbv_token_marks_rows", k, mrows, B, stream=hip_stream)
            y_host = y_buf.tolist()                # the one host sync: every run's lengths, -1 = flagged
            bad = [i for i in range(N) if y_host[pos[i]] < 0]
            if bad:
                raise IndexError("request%s %s: index out of range in self (token id or sid outside the model's tables, or "
                                 "a duration outside the supported range: 2^20 frames a token, 2^30 an utterance; given "
                                 "durations must be non-negative integers; a per-token scale must be finite and >= 0, "
                                 "extra frames >= 0)"
                                 % ("s" if len(bad) > 1 else "", ", ".join(str(i) for i in bad)))
            Tp = [int(y_host[pos[i]]) for i in range(N)]
            Td = [Tp[i] if r.max_len is None else min(Tp[i], r.max_len) for i, r in enumerate(reqs)]
            # the reference draws randn_like(m_p) even at noise_scale == 0 (models.py:729): per request, in list order,
            # into one buffer — the values and the generator's progress of N stand-alone randn(1, I, T'_i) calls.
            # Seeded requests take no part in that: their blocks are one launch, across classes
            noise = [None] * N
            if drawn:
                flat, ptr = self._draw_rows(I, [Tp[i] for i in drawn], dev)
                keep.append(flat)
                for i, a in zip(drawn, ptr):
                    noise[i] = a
            if seeded:
                keep.append(self._seeded_blocks(h, seeded, [reqs[i].seed for i in seeded], I, [Tp[i] for i in seeded],
                                                _capi.NOISE_PRIOR, noise, hip_stream))
            z = [torch.empty(1, I, Td[i], device=dev, dtype=torch.float32) for i in range(N)]
            g = [None] * N
            frame_gain = {i: torch.empty(1, Td[i] + 1, device=dev, dtype=torch.float32)
                          for i in range(N) if reqs[i].gain is not None}
            for k, m in enumerate(members):
                B = len(m)
                if any(i in frame_gain for i in m):    # the run's gains over its frames: one table-reading launch
                    grows = (_capi.MbvGainRow * B)()
                    for row, i in zip(grows, m):
                        if i in frame_gain:
                            row.gain, row.out, row.frames = gain_p[i], frame_gain[i].data_ptr(), Td[i]
                    self._launch(h, "mbv_frame_gain_rows", k, grows, B, stream=hip_stream)
                rows = (_capi.MbvRow * B)()
                for row, i in zip(rows, m):
                    row.noise, row.noise_stride, row.noise_scale = noise[i], Tp[i], reqs[i].noise_scale
                    row.keep, row.z = Td[i], z[i].data_ptr()
                self._launch(h, "mbv_synthesize_rows", k, max(Tp[i] for i in m), rows, B, stream=hip_stream)
                if self.n_speakers > 0:            # (the sids passed the encode's range check)
                    g_run = torch.empty(B, self.cfg.gin_channels, device=dev, dtype=torch.float32)
                    self._launch(h, "mbv_speaker_embedding", sids[k], B, g_run, stream=hip_stream)
                    for b, i in enumerate(m):
                        g[i] = g_run[b:b + 1]
            sts = self._streams_of(reqs, z, g, y_all, pos)
            for i in marked:
                sts[i].marks = [min(int(v), Td[i]) for v in y_host[mark_at[i]:mark_at[i] + t_text[i] + 1]]
            for i, at in fit_at.items():
                sts[i].fit_scale, sts[i].fit_status = _capi.fit_result(y_host[at])
            for i, t in frame_gain.items():
                sts[i].frame_gain = t
            for i, r in enumerate(reqs):
                if r.pitch is not None:            # the warp of a pitched request, planned on the host from its marks
                    sts[i].warp = stream.WarpMap(stream.frame_rates(r.pitch.tolist(), sts[i].marks, Td[i],
                                                                    r.pitch_glide_frames), sts[i].spf, dev)
            return sts

    # ------------------------------------------------------------------ pooled voice conversion
    def convert_plan(self, t_frames, splitk=False):
        """(runs, run_of_request): the posterior runs `convert_streams` makes for requests of these frame counts
        (`mbv_convert_plan`, host only: no GPU needed).  Requests share a padded run iff the conv planner sends
        enc_q.pre, enc_q.proj and the flows' convs to the same kernel family for either alone; a class is cut at
        65 535 rows and at what the fused WN layers take; with `splitk` one class."""
        t = _ints(t_frames)
        if not t:
            raise ValueError("convert_plan: no requests")
        if min(t) < 1:
            raise ValueError("convert_plan: a request without frames (every count must be >= 1)")
        return self._plan_runs("mbv_convert_plan", t, splitk,
                               "mbv_convert_plan refused the frame counts (one request beyond the fused WN layers?)")

    def converter_runs(self):
        """Posterior-encoder runs `convert_streams` / `convert_stream` made on this model's handle so far
        (`mbv_converter_runs`): the difference across a call is the number of launch chains it cost."""
        return int(_capi.lib().mbv_converter_runs(self._ensure_handle()))

    def seam_runs(self):
        """Launches of the chunk-seam kernel on this model's handle so far (`mbv_seam_runs`): one per `poll()` /
        `StreamPool.step()` decode call in which a live stream opened with `Ahead(seam_ms=)` decoded."""
        return int(_capi.lib().mbv_seam_runs(self._ensure_handle()))

    def convert_stream(self, wave, sid_src, sid_tgt, model_sr, hop_size, win_size, in_sr=None, noise_scale=1.0,
                       chunk_frames=32, max_chunk_frames=256, noise=None, seed=None):
        """Voice conversion of one recording up to z_hat, as a `DecodeStream`: resample to `model_sr` if `in_sr`
        differs, spectrogram, posterior encoder, forward flow with emb_g(sid_src), reverse flow with emb_g(sid_tgt);
        -> `dec_stream(z_hat * y_mask, g = emb_g(sid_tgt))` with `y_lengths` = the frame count.  Draws exactly one
        `torch.randn(1, inter, T)` on the device generator, as `voice_conversion` does for that spectrogram alone: at
        noise_scale 1 and in_sr == model_sr, `st.z` is bitwise that call's z_hat * y_mask and `st.run()` its o_hat
        (default mode).  Arguments as `ConvertRequest`.  `noise` [1, inter, T] fp32 replaces the draw and leaves the
        generator untouched (what `convert_live` is measured against); the default is the path as it was.  `seed` (an int,
        or a one-element sequence as the batched entries take it) makes the draw a function of the seed (DESIGN 7.13:
        purpose 2, row 0; one `mbv_randn_blocks` launch, no generator touched); it excludes `noise`."""
        if seed is not None:
            if noise is not None:
                raise ValueError("convert_stream: seed= and noise= exclude each other")
            seed = _row_seeds(seed, 1, "convert_stream: seed")[0][0]
        req = ConvertRequest(wave, sid_src, sid_tgt, model_sr, hop_size, win_size, in_sr=in_sr, noise_scale=noise_scale,
                             chunk_frames=chunk_frames, max_chunk_frames=max_chunk_frames, seed=seed)
        return self._convert([req], alone=True, noise=noise)[0]

    def converter_context(self):
        """(L, R) of `mbv_converter_context` (host only): z_hat frame t depends on spectrogram frames [t - L, t + R]."""
        return stream.converter_context(self._config_struct())

    def convert_live(self, sid_src, sid_tgt, model_sr, hop_size, win_size, max_samples, dtype=torch.float32,
                     noise_scale=1.0, noise=None, chunk_frames=32, max_chunk_frames=256, convert_frames=32, in_sr=None,
                     seed=None, ahead=None):
        """Voice conversion of a recording that is still arriving: a `stream.LiveStream` that takes the samples in
        `push` calls of any size and hands out decoded chunks from `poll` as soon as the audio they depend on exists
        (DESIGN 7.11).  The result does not depend on how the samples were cut into pushes; for a recording of more
        than 256 frames it is bitwise `convert_stream(whole, ..., noise=st.noise[:, :, :T])` chunk by chunk (default
        mode), for a shorter one within fp32 rounding of it.  Draws one `torch.randn(1, inter, max_frames)` on the device
        generator here, unless `noise` (that shape) is given, or `seed` (as `convert_stream` takes it; excludes
        `noise`): then the capacity buffer is filled once, as one `mbv_randn_blocks` block, and since element (c, t)
        does not depend on the buffer's length the stream equals `convert_stream(whole, ..., seed=[s])`.  Buffers are
        sized for `max_samples` once.  The audio must be at the model's rate; `wire.convert_live_pcm16` is the form that
        takes raw samples at any rate and hands out int16 at the service's rate.  `ahead` (a
        `stream.Ahead`, opt-in): conversion on a fixed grid of `convert_frames` with a bounded look-ahead,
        for a call that is live; an approximation of the full-context stream with an exact definition."""
        return stream.LiveStream(self, sid_src, sid_tgt, model_sr, hop_size, win_size, max_samples, dtype=dtype,
                                 noise_scale=noise_scale, noise=noise, chunk_frames=chunk_frames,
                                 max_chunk_frames=max_chunk_frames, convert_frames=convert_frames, in_sr=in_sr, seed=seed,
                                 ahead=ahead)

    def text_context(self):
        """(R, R) of `mbv_text_context` (host only): z frame t depends on z_p frames [t - R, t + R] only."""
        return stream.text_context(self._config_struct())

    def text_runs(self):
        """`mbv_take_tokens_rows` + `mbv_expand_ranges` launches made on this model's handle so far (`mbv_text_runs`)."""
        return int(_capi.lib().mbv_text_runs(self._ensure_handle()))

    def flow_runs(self):
        """Flow runs of `mbv_flow_ranges` made on this model's handle so far (`mbv_flow_runs`)."""
        return int(_capi.lib().mbv_flow_runs(self._ensure_handle()))

    def infer_live(self, sid=None, max_tokens=None, max_frames=None, noise_scale=1, length_scale=1, noise_scale_w=1.,
                   seed=None, noise=None, noise_w=None, block_tokens=16, ahead=None, chunk_frames=32,
                   max_chunk_frames=256, flow_frames=32, model_sr=None):
        """Synthesis of ONE utterance whose tokens are still arriving: a `stream.TextStream` that takes token ids in
        `push` calls of any size and hands out decoded chunks from `poll` as soon as the model's reach allows (DESIGN
        7.27), the text mirror of `convert_live`.  Token block k (`block_tokens` tokens) is encoded from the text
        prefix that ends `ahead.tokens` tokens behind it (`stream.TextAhead`; None = the whole text, every block then
        waits for `close()`), its columns of that prefix call's text-level statistics and durations are length-regulated
        into the stream's own z_p, the reverse flows run on windows of it, and the chunks are decoded as a live stream's.
        The result is a pure function of (ids, sid, scales, seed / noise, block_tokens, ahead, chunk schedule): it does
        not depend on the pushes, the polls or the pool.  With `TextAhead(tokens=None)` and more than 256 frames the
        finished stream is bitwise `infer_stream(ids, ..., seed=seed)`; with bounded `tokens` it is an approximation
        with an exact definition, and nothing is claimed about its quality.

        Buffers are sized once for `max_tokens` and `max_frames` (both required).  The prior noise is one
        `torch.randn(1, inter, max_frames)` on the device generator, unless `noise` (that shape) or `seed` is given; with
        the stochastic duration predictor `noise_w` [2, max_tokens] likewise (drawn on the CPU generator as the
        reference's).  `seed=` excludes `noise=` / `noise_w=`.  `model_sr` is only needed for `TextAhead(seam_ms=)`.
        Refused here: "conv_bf16", a missing or unknown sid, a `TextAhead` beyond the decoder's reach.  Not part of a
        text stream: per-token prosody, gain and pitch, `durations=`, `max_len`, the wire layer."""
        return stream.TextStream(self, sid=sid, max_tokens=max_tokens, max_frames=max_frames, noise_scale=noise_scale,
                                 length_scale=length_scale, noise_scale_w=noise_scale_w, seed=seed, noise=noise,
                                 noise_w=noise_w, block_tokens=block_tokens, ahead=ahead, chunk_frames=chunk_frames,
                                 max_chunk_frames=max_chunk_frames, flow_frames=flow_frames, model_sr=model_sr)

    def convert_streams(self, requests):
        """Pooled voice conversion: one single-utterance `DecodeStream` per `ConvertRequest`, in order — what
        `StreamPool.add` takes — from ONE padded posterior run per class of `convert_plan`, with no host read-back:
        frame counts follow from the sample counts and speaker ids are ints, so every refusal happens before the
        first launch.

        Default mode: stream i is bitwise (z, g, y_lengths, schedule) what `convert_stream(...)` returns for request
        i alone when those calls are made in list order from the same RNG state; the device generator ends where
        those calls leave it and the CPU generator is not touched.  Requests with `seed=` take no part in that order:
        each is bitwise `convert_stream(..., seed=[seed_i])` whatever else is in the list, and ONE `mbv_randn_blocks`
        launch fills the posterior blocks of all of them; the unseeded ones draw in list order among themselves.  With
        the option "splitk" the result is
        deterministic and within fp32 rounding of the stand-alone calls; "conv_bf16" is refused.

        All requests must agree on (model_sr, hop_size, win_size): one model has one data config.  Refused before any
        launch, naming the request: audio that gives 0 frames (ValueError), a speaker id outside [0, n_speakers)
        (IndexError); a single-speaker model raises the reference's assertion.  No stream is created then."""
        return self._convert(list(requests), alone=False)

    def _check_conversion(self, who, hop_size, win_size, n_fft_is=""):
        """What a conversion entry (`_convert`, `stream.LiveStream`) refuses about the model and the data config, on
        the host; -> n_fft.  `who` names the caller in the messages, `n_fft_is` is what its win_size message adds."""
        if not self.n_speakers > 0:
            raise AssertionError("n_speakers have to be larger than 0.")      # models.py:791
        n_fft = 2 * (self.cfg.spec_channels - 1)
        if _capi.lib().mbv_spectrogram_frames(1, n_fft, hop_size) < 0:
            raise ValueError("%s: n_fft = 2 (spec_channels - 1) = %d must be a power of two in [256, 4096] "
                             "and hop_size in [1, n_fft] (hop_size %d)" % (who, n_fft, hop_size))
        if not 1 <= win_size <= n_fft:
            raise ValueError("%s: win_size %d must be in [1, n_fft =%s %d]" % (who, win_size, n_fft_is, n_fft))
        return n_fft

    def _check_speakers(self, sid_src, sid_tgt, prefix=""):
        for name, sid in (("sid_src", sid_src), ("sid_tgt", sid_tgt)):
            if not (0 <= sid < self.n_speakers or self._voice_defined(sid)):
                raise IndexError("%sindex out of range in self (%s %d outside [0, %d))"
                                 % (prefix, name, sid, self.n_speakers))

    # ------------------------------------------------------------------ blended voices
    def _voice_defined(self, sid):
        """`mbv_speaker_defined`: sid >= n_speakers names a defined voice of this model's handle."""
        if sid < self.n_speakers or (self._handle is None and not self._voices):
            return False
        return _capi.lib().mbv_speaker_defined(self._ensure_handle(), int(sid)) == 1

    def _voice_spec(self, i, spec):
        """One definition, checked on the host -> (ids, weights, vector): ids / weights lists, or the device row."""
        unknown = set(spec) - {"ids", "weights", "vector", "normalize"} if isinstance(spec, dict) else {type(spec).__name__}
        if unknown:
            raise ValueError("voice %d: a definition is a dict of the arguments of `speaker` (ids, weights, vector, "
                             "normalize), got %s" % (i, sorted(unknown)))
        ids, weights, vector = spec.get("ids"), spec.get("weights"), spec.get("vector")
        normalize = spec.get("normalize", True)
        gin = self.cfg.gin_channels
        if vector is not None:
            if ids is not None or weights is not None:
                raise ValueError("voice %d: vector= excludes ids= and weights=" % i)
            vector = torch.as_tensor(vector).detach()
            if vector.dim() != 1 or vector.numel() != gin:
                raise ValueError("voice %d: vector must hold gin_channels = %d floats, got shape %s"
                                 % (i, gin, tuple(vector.shape)))
            vector = vector.to(device=self._device(), dtype=torch.float32).contiguous().clone()
            if not bool(torch.isfinite(vector).all()):
                raise ValueError("voice %d: vector must be finite" % i)
            return None, None, vector
        if ids is None:
            raise ValueError("voice %d: needs ids= (real speaker ids) or vector=" % i)
        ids = _ints(ids)
        if weights is None:
            weights = [1.0] * len(ids)             # the mean of a group under normalize=True
        try:
            weights = blend_weights(weights, normalize)
        except ValueError as e:
            raise ValueError("voice %d: %s" % (i, e))
        if len(ids) != len(weights):
            raise ValueError("voice %d: %d ids for %d weights" % (i, len(ids), len(weights)))
        for v in ids:
            if not 0 <= v < self.n_speakers:
                raise ValueError("voice %d: speaker id %d outside [0, %d): a blend names real speakers only (no blends "
                                 "of blends)" % (i, v, self.n_speakers))
        return ids, weights, None

    def _define_voices(self, h, voices):
        """ONE `mbv_speakers_define` call for `voices` (Speaker objects) inside a device scope the caller holds."""
        arr = (_capi.MbvSpeakerDef * len(voices))()
        for k, v in zip(arr, voices):
            k.slot = v.slot
            if v._vector is not None:
                k.vector = v._vector.data_ptr()
            else:
                k.count = len(v.ids)
                for j, (sid, w) in enumerate(zip(v.ids, v.weights)):
                    k.ids[j], k.weights[j] = sid, w
        self._launch(h, "mbv_speakers_define", arr, len(voices))

    @torch.no_grad()
    def speakers(self, specs):
        """Define several voices in ONE blend launch -> [Speaker].  A spec is a dict with the arguments of `speaker`
        (ids, weights, vector, normalize).  All or nothing: every spec is checked on the host
        first (ValueError naming it) and nothing is launched or taken when one is refused."""
        specs = list(specs)
        if not (self.n_speakers > 1 and self.cfg.gin_channels > 0):
            raise ValueError("voices need a speaker table: this model has n_speakers = %d" % self.n_speakers)
        if not specs:
            return []
        h = self._ensure_handle()
        parsed = [self._voice_spec(i, s) for i, s in enumerate(specs)]
        taken = []
        try:
            for ids, weights, vector in parsed:
                taken.append(Speaker(self, self._voice_slots.take(), ids, weights, vector))
            with torch.cuda.device(self._device()):
                self._define_voices(h, taken)
        except Exception:
            for v in taken:
                self._voice_slots.free(v.slot)
            raise
        for v in taken:
            self._voices[v.slot] = v
        return taken

    def speaker(self, ids=None, weights=None, vector=None, normalize=True):
        """A voice that is not in the table -> `Speaker`; its `.sid` = n_speakers + slot is valid wherever a speaker id
        is, in host ints and in device tensors, mixed with plain ids at will.

          ids, weights   real speaker ids (at most BLEND_MAX) and their weights (default: equal).  The row is the fp32
                         chain w_0 e_0, then fmaf(w_k, e_k, acc) in the order given: a one-hot blend is bitwise the
                         table row
          normalize      True: the weights are divided by their float64 sum, then rounded to fp32 (needs a sum > 0);
                         False: sent as given, which allows extrapolation such as [1.5, -0.5]
          vector         instead of ids: a ready row of gin_channels floats (an embedding tuned outside the checkpoint);
                         copied, and kept as given when the weights are refreshed, whereas a blend follows the table
        One blend launch (`speaker_runs`).  ValueError for anything refused; nothing is defined then."""
        return self.speakers([dict(ids=ids, weights=weights, vector=vector, normalize=normalize)])[0]

    def _hold_voices(self, holder, *sids):
        """`holder` (weakly kept) passes these ids on every tick: the voices among them cannot be released until it
        has `finished`."""
        for sid in sids:
            if sid >= self.n_speakers:
                self._voice_holders.setdefault(sid - self.n_speakers, weakref.WeakSet()).add(holder)

    def _release_speaker(self, v):
        if self._voices.get(v.slot) is not v:
            raise ValueError("%r is not a voice of this model" % (v,))
        for holder in list(self._voice_holders.get(v.slot, ())):
            if not holder.finished:
                raise ValueError("%r is held by %r, which passes its id on every tick: finish or drop the stream first"
                                 % (v, holder))
        self._call("mbv_speaker_release", v.slot)
        self._voice_holders.pop(v.slot, None)
        del self._voices[v.slot]
        self._voice_slots.free(v.slot)
        v.released = True

    def speaker_runs(self):
        """Launches of the blend kernel on this model's handle so far (`mbv_speaker_runs`): one per `speaker` /
        `speakers` call, one per weight refresh while a blend is defined."""
        return int(_capi.lib().mbv_speaker_runs(self._ensure_handle()))

    def _handle_not_bf16(self, who, instead, why=" (the flows' route follows the launch size there)"):
        """`_ensure_handle()` for the entries that are not built for the "conv_bf16" mode: ValueError there."""
        h = self._ensure_handle()
        if _capi.lib().mbv_get_option(h, b"conv_bf16") != 0:
            raise ValueError("%s is not built for the \"conv_bf16\" mode%s: %s" % (who, why, instead))
        return h

    @torch.no_grad()
    def _convert(self, reqs, alone, noise=None):
        for i, r in enumerate(reqs):
            if not isinstance(r, ConvertRequest):
                raise TypeError("convert_streams takes models.ConvertRequest values (item %d is %s)" % (i, type(r).__name__))
        if not reqs:
            return []
        r0 = reqs[0]
        for i, r in enumerate(reqs):
            if (r.model_sr, r.hop_size, r.win_size) != (r0.model_sr, r0.hop_size, r0.win_size):
                raise ValueError("request %d: (model_sr, hop_size, win_size) = %s differs from request 0's %s: one model "
                                 "has one data config" % (i, (r.model_sr, r.hop_size, r.win_size),
                                                          (r0.model_sr, r0.hop_size, r0.win_size)))
        n_fft = self._check_conversion("convert_streams", r0.hop_size, r0.win_size, " 2 * (spec_channels - 1) =")
        N, I = len(reqs), self.cfg.inter_channels
        samples = [r.model_samples() for r in reqs]
        frames = [r.frames(n_fft) for r in reqs]
        for i, r in enumerate(reqs):
            if frames[i] < 1:
                raise ValueError("request %d: %d samples at %d Hz give no spectrogram frame (n_fft %d, hop_size %d)"
                                 % (i, r.wave.numel(), r.in_sr, n_fft, r.hop_size))
            self._check_speakers(r.sid_src, r.sid_tgt, "request %d: " % i)
        h = self._handle_not_bf16("convert_streams", "convert with voice_conversion")
        L = _capi.lib()
        dev = self._device()
        try:
            n_runs, run_of = self.convert_plan(frames, splitk=L.mbv_get_option(h, b"splitk") != 0)
        except ValueError:
            raise ValueError("convert_streams: a request of %d frames is beyond what the fused WN layers take" % max(frames))
        members = [[i for i in range(N) if run_of[i] == k] for k in range(n_runs)]
        with torch.cuda.device(dev):
            hip_stream = self._stream(dev)
            keep = []                              # inputs of launches in flight
            wave_ptr = [None] * N
            # rows at another rate: one `resample` call per distinct in_sr over their padded batch; the result is read
            # in place, row by row
            for sr in sorted({r.in_sr for r in reqs if r.in_sr != r.model_sr}):
                idx = [i for i in range(N) if reqs[i].in_sr == sr]
                on_host = not any(reqs[i].wave.is_cuda for i in idx)
                ws = []
                for i in idx:
                    w = reqs[i].wave if on_host else reqs[i].wave.to(dev)
                    ws.append(w.float() / 32768.0 if w.dtype == torch.int16 else w)     # exact scaling, as convert_pcm16
                batch = torch.nn.utils.rnn.pad_sequence(ws, batch_first=True).unsqueeze(1)
                valid = None
                if len(idx) > 1:
                    valid = torch.tensor([reqs[i].wave.numel() for i in idx], dtype=torch.int64)
                out, _ = self.resample(batch.to(dev), sr, r0.model_sr, valid_samples=valid)
                keep.append(out)
                for b, i in enumerate(idx):
                    wave_ptr[i] = out.data_ptr() + 4 * b * out.shape[-1]
            # rows at the model's rate are read as they came
            same = [r.in_sr == r.model_sr for r in reqs]
            own_ptr, kept = self._pack_host([r.wave if same[i] else None for i, r in enumerate(reqs)], dev)
            keep += kept
            wave_ptr = [own_ptr[i] if same[i] else wave_ptr[i] for i in range(N)]
            wave_dtype = [_capi.WAVE_PCM16 if same[i] and r.wave.dtype == torch.int16 else _capi.WAVE_F32
                          for i, r in enumerate(reqs)]
            # the posterior draw, per request, in list order: the values and the generator's progress of N stand-alone
            # randn(1, I, T_i) calls (drawn at noise_scale == 0 too, as convert_stream does)
            if alone and noise is not None:
                if not torch.is_tensor(noise) or noise.dtype != torch.float32 or tuple(noise.shape) != (1, I, frames[0]):
                    raise ValueError("convert_stream: noise must be a float32 tensor [1, %d, %d] (inter_channels, frames)"
                                     % (I, frames[0]))
                flat = noise.to(dev).contiguous()
                noise = [flat.data_ptr()]
                y_all = torch.full((1,), frames[0], dtype=torch.int64, device=dev)
            elif alone and reqs[0].seed is None:
                flat = torch.randn(1, I, frames[0], device=dev, dtype=torch.float32)
                noise = [flat.data_ptr()]
                y_all = torch.full((1,), frames[0], dtype=torch.int64, device=dev)
            else:
                # seeded requests take no part in the list-order draw: their blocks are one launch, across classes
                seeded = [i for i in range(N) if reqs[i].seed is not None]
                drawn = [i for i in range(N) if reqs[i].seed is None]
                noise = [None] * N
                if drawn:
                    flat, ptr = self._draw_rows(I, [frames[i] for i in drawn], dev)
                    for i, a in zip(drawn, ptr):
                        noise[i] = a
                if seeded:
                    keep.append(self._seeded_blocks(h, seeded, [reqs[i].seed for i in seeded], I,
                                                    [frames[i] for i in seeded], _capi.NOISE_POSTERIOR, noise, hip_stream))
                if alone:
                    y_all = torch.full((1,), frames[0], dtype=torch.int64, device=dev)
                else:
                    y_all = torch.tensor(frames, dtype=torch.int64).to(dev)
            z = [torch.empty(1, I, frames[i], device=dev, dtype=torch.float32) for i in range(N)]
            g = [None] * N
            for m in members:
                B = len(m)
                rows = (_capi.MbvConvertRow * B)()
                for row, i in zip(rows, m):
                    r = reqs[i]
                    row.wave, row.samples, row.wave_dtype = wave_ptr[i], samples[i], wave_dtype[i]
                    row.sid_src, row.sid_tgt = r.sid_src, r.sid_tgt
                    row.noise, row.noise_scale, row.z = noise[i], r.noise_scale, z[i].data_ptr()
                g_run = torch.empty(B, self.cfg.gin_channels, device=dev, dtype=torch.float32)
                self._launch(h, "mbv_convert_rows", rows, B, max(frames[i] for i in m), r0.hop_size, r0.win_size, g_run,
                             stream=hip_stream)
                for b, i in enumerate(m):
                    g[i] = g_run[b:b + 1]
            return self._streams_of(reqs, z, g, y_all, range(N))

    @torch.no_grad()
    def istft_finalize(self, spec, phase):
        """(spec, phase) -> waveform [B, 1, samples] with the model's synthesis bank: the last step
        of the reference's chunked decoding (`istft_finalize` in inferz_test.ipynb cell 6; the
        cross-fade of the chunks' spectrograms stays in the caller).  Accepts the complex
        spectrogram too (`spec * exp(1j * phase)`), as the notebook passes it."""
        dev = self._device()
        if phase is None:
            if not torch.is_complex(spec):
                raise ValueError("istft_finalize(spec, phase): phase missing and spec is not complex")
            spec, phase = torch.abs(spec), torch.angle(spec)
        spec = spec.to(device=dev, dtype=torch.float32).contiguous()
        phase = phase.to(device=dev, dtype=torch.float32).contiguous()
        if spec.shape != phase.shape:
            raise ValueError("spec and phase must have the same shape")
        sb = self.cfg.decoder == DEC_SB
        if (spec.dim() != (3 if sb else 4)) or spec.shape[-2] != 9 or (not sb and spec.shape[1] != 4):
            raise ValueError("spec must be [B, 9, F]" if sb else "spec must be [B, 4, 9, F]")
        B, Fr = spec.shape[0], spec.shape[-1]
        n = (4 if sb else 16) * (Fr - 1)
        o = torch.empty(B, 1, n, device=dev, dtype=torch.float32)
        self._call("mbv_istft_finalize", spec, phase, B, Fr, o, None)
        return o

    @torch.no_grad()
    def to_pcm16(self, wave, y_lengths=None, auto_normalize=True, valid_samples=None):
        """Waveform [B, 1, n] -> int16 PCM [B, n] on the GPU: the normalise / clip / *32767 /
        astype(int16) sequence of the service wrapper (tts_vits.py:204-217), per utterance over
        its valid 256 * y_lengths samples (rest zero).  Bit-exact with the NumPy code.
        `valid_samples` (int64 [B], e.g. the lengths `resample` returns) gives the valid length in
        samples instead; it excludes `y_lengths`."""
        dev = self._device()
        wave = wave.to(device=dev, dtype=torch.float32).contiguous()
        B, n = wave.shape[0], wave.shape[-1]
        pcm = torch.empty(B, n, device=dev, dtype=torch.int16)
        if valid_samples is not None:
            if y_lengths is not None:
                raise ValueError("to_pcm16: give y_lengths (frames) or valid_samples (samples), not both")
            self._call("mbv_pcm16_samples", wave, _valid_samples(valid_samples, B, dev), B, n, int(bool(auto_normalize)), pcm)
            return pcm
        if y_lengths is not None:
            y_lengths = y_lengths.to(device=dev, dtype=torch.int64).contiguous()
        self._call("mbv_pcm16", wave, y_lengths, B, n, int(bool(auto_normalize)), pcm)
        return pcm

    @torch.no_grad()
    def resample(self, wave, orig_sr, target_sr, y_lengths=None, valid_samples=None, res_type="kaiser_best"):
        """Waveform [B, 1, n] at `orig_sr` -> (out [B, 1, ceil(n * target_sr / orig_sr)], out_samples int64 [B])
        on the GPU: `librosa.resample(row, orig_sr=orig_sr, target_sr=target_sr)` of librosa 0.9.2 for every
        row over its valid samples (tts_vits.py:199-200; res_type "kaiser_best", its default, or
        "kaiser_fast": resampy's interpolator + fix_length).  out_samples[b] = ceil(n_b * target / orig) is the
        length librosa returns for row b; the rest of the row is zero.  Valid input samples come from
        `y_lengths` (frames, x256, clamped to the row, negative -> 0, as in `to_pcm16`) or `valid_samples`
        (samples); neither = whole rows.  Equal rates return `wave` and the lengths unchanged.  No host
        synchronisation, except on the first call for a rate pair (the filter bank is built and uploaded).
        Parity is pinned to a float64 restatement of resampy's algorithm, not to the library itself."""
        filt = _filter_code(res_type)
        orig_sr, target_sr = int(orig_sr), int(target_sr)
        if orig_sr <= 0 or target_sr <= 0:
            raise ValueError("sample rates must be positive")
        if y_lengths is not None and valid_samples is not None:
            raise ValueError("resample: give y_lengths (frames) or valid_samples (samples), not both")
        h = self._ensure_handle()
        dev = self._device()
        if wave.dim() != 3 or wave.shape[1] != 1:
            raise ValueError("wave must be [B, 1, samples]")
        B, n = wave.shape[0], wave.shape[-1]
        if y_lengths is not None:
            valid_samples = (_valid_samples(y_lengths, B, dev, "y_lengths / valid_samples") * 256).clamp(0, n)
        elif valid_samples is not None:
            valid_samples = _valid_samples(valid_samples, B, dev, "y_lengths / valid_samples").clamp(0, n)
        if orig_sr == target_sr:
            if valid_samples is None:
                valid_samples = torch.full((B,), n, device=dev, dtype=torch.int64)
            return wave, valid_samples
        wave = wave.to(device=dev, dtype=torch.float32).contiguous()
        n_out = int(math.ceil(n * (float(target_sr) / orig_sr)))
        out = torch.empty(B, 1, max(n_out, 1), device=dev, dtype=torch.float32)
        out_samples = torch.empty(B, device=dev, dtype=torch.int64)
        if n == 0 or B == 0:
            out.zero_()
            out_samples.zero_()
            return out[..., :n_out], out_samples
        with torch.cuda.device(dev):
            self._launch(h, "mbv_resample", wave, valid_samples, B, n, orig_sr, target_sr, filt, out, out.shape[-1],
                         out_samples)
        return out, out_samples

    @torch.no_grad()
    def resample_pcm16_range(self, wave, orig_sr, target_sr, in_avail, out_first, out_count, pcm, valid_samples=None,
                             peak=None, running_peak=None, out_samples=None, res_type="kaiser_best", limiter=None,
                             encoding="pcm16", fade=None, envelope=None):
        """One step of the streamed wire output (`mbv_resample_pcm16_range`; `wire.stream_pcm16` drives it for a
        decode stream): int16 samples [out_first, out_first + out_count) of every row of `pcm` [B, n'] from the
        first `in_avail` samples of `wave` (fp32 [B, 1, n] or [B, n], contiguous, on the device; nothing at or
        past `in_avail` is read), bitwise what `resample` + `to_pcm16(valid_samples=...)` give there for the
        finished rows.  The range must end at or below `wire.resample_ready(orig_sr, target_sr, in_avail, n)`.
          valid_samples  int64 [B] device valid input samples per row, or None = whole rows
          peak           fp32 [B] device: divide by it (x 0.9) where it exceeds 0.01; None = no normalisation
          running_peak   fp32 [B] device, zeroed by the caller before the first step: raised to the peak of the
                         resampled samples of the range
          out_samples    int64 [B] device: receives the row lengths `resample` returns
          limiter        None, or (ceiling, lookahead, hold) in output samples (`wire.Limiter.resolve`): the
                         look-ahead limiter of DESIGN §7.14 between the gain and the clip
                         (`mbv_resample_pcm16_range_limited`); the range must then end at or below
                         `wire.limiter_ready(orig_sr, target_sr, in_avail, n, lookahead)`
          encoding       "pcm16", or "ulaw" / "alaw": `pcm` is then uint8 and receives the G.711 byte of the int16 the
                         call would have stored at the same index (`mbv_resample_g711_range`)
          fade           None, or (first, count) in output samples: the fade-out of DESIGN §7.16 on every row, through
                         `mbv_resample_pcm16_range_faded` / `mbv_resample_g711_range_faded`; a `_capi.MbvPcmFade` is
                         passed as it is (the entry checks it)
          envelope       None, or a `wire.Envelope` with B rows: per-token volume, multiplied into the
                         samples where the kernel reads them, in front of everything else
                         (`mbv_resample_pcm16_range_shaped`); the bytes are those of the call on `wave * e`
        Writes into the caller's tensors only; no host synchronisation (beyond the first call for a rate pair)."""
        filt = _filter_code(res_type)
        law = _law_code(encoding)
        dev = self._device()
        if wave.dim() == 3 and wave.shape[1] == 1:
            wave = wave[:, 0]
        if wave.dim() != 2 or pcm.dim() != 2 or pcm.shape[0] != wave.shape[0]:
            raise ValueError("wave must be [B, 1, n] or [B, n] and pcm [B, n']")
        B, n = wave.shape
        for name, t, dt in (("wave", wave, torch.float32), ("pcm", pcm, torch.uint8 if law else torch.int16),
                            ("peak", peak, torch.float32),
                            ("running_peak", running_peak, torch.float32), ("out_samples", out_samples, torch.int64),
                            ("valid_samples", valid_samples, torch.int64)):
            if t is None:
                continue
            if t.device != dev or t.dtype != dt or t.stride(-1) != 1 or (t.dim() == 1 and t.shape != (B,)):
                raise ValueError("resample_pcm16_range: %s must be a %s tensor on %s with unit stride%s"
                                 % (name, dt, dev, "" if t.dim() == 2 else ", shape [B]"))
        if B > 1 and wave.stride(0) != n:
            raise ValueError("resample_pcm16_range: wave rows must be contiguous")
        if int(out_first) + int(out_count) > pcm.shape[1]:
            raise ValueError("resample_pcm16_range: outputs [%d, %d) lie outside pcm [B, %d]"
                             % (int(out_first), int(out_first) + int(out_count), pcm.shape[1]))
        args = (wave, valid_samples, B, n, int(orig_sr), int(target_sr), filt, int(in_avail), int(out_first),
                int(out_count), peak, pcm, pcm.stride(0), running_peak, out_samples)
        who = "resample_pcm16_range"
        if envelope is not None:
            if not isinstance(envelope, Envelope):
                raise TypeError("%s: envelope must be a wire.Envelope, got %s" % (who, type(envelope).__name__))
            envelope.check(who, B, n, dev)
        fd = _fades_c(who, "call", [fade], 1)                # one fade and one limiter for every row of the call
        lim = _limits_c(who, "call", [limiter], 1)
        name, extra = _range_entry(lim, law, fd, envelope)
        self._call(name, *args, *extra)

    @torch.no_grad()
    def resample_pcm16_chunks(self, chunks, orig_sr, target_sr, packed=None, res_type="kaiser_best", limits=None,
                              encoding="pcm16", fades=None, envelopes=None):
        """The ranged wire step of many streams in ONE launch (`mbv_resample_pcm16_chunks`; `wire.pcm_pool` drives
        it): `chunks` is a ctypes array (or a list) of `_capi.MbvPcmChunk`, each the arguments of
        `resample_pcm16_range` for one row of its own stream, as device addresses.  Every stored value is bitwise
        what `resample_pcm16_range` stores for that row alone.  `packed` (int16, 1-D, device) also receives the
        chunks' samples back to back, in chunk order.  `limits`: None, or one entry per chunk, each None or the
        (ceiling, lookahead, hold) `resample_pcm16_range` takes as `limiter` (`mbv_resample_pcm16_chunks_limited`:
        one launch for the limited chunks, one for the others).  `encoding` "ulaw" / "alaw": every chunk's `pcm` and
        `packed` are uint8 and receive G.711 bytes (`mbv_resample_g711_chunks`; `pcm_capacity` counts bytes).  `fades`:
        None, or one entry per chunk, each None, a (first, count) or a `_capi.MbvPcmFade`: the fade-out of DESIGN §7.16
        on those chunks (`mbv_resample_pcm16_chunks_faded` / `mbv_resample_g711_chunks_faded`), in the launches the call
        makes without it; all None is the call without `fades`.  `envelopes`: None, or one entry per chunk, each None or
        a one-row `wire.Envelope`: per-token volume on those chunks (`mbv_resample_pcm16_chunks_shaped`),
        in the launches the call makes without it; all None is the call without `envelopes`.  No host synchronisation
        (beyond the first call for a rate pair)."""
        who = "resample_pcm16_chunks"
        filt = _filter_code(res_type)
        law = _law_code(encoding)
        if not isinstance(chunks, C.Array):
            chunks = (_capi.MbvPcmChunk * len(chunks))(*chunks)
        n = len(chunks)
        dev = self._device()
        cap = _packed_capacity(who, packed, law, dev)
        ev = None
        if envelopes is not None and any(e is not None for e in envelopes):
            for name, t in (("limit", limits), ("fade", fades), ("envelope", envelopes)):
                if t is not None and len(t) != n:
                    raise ValueError("%s: one %s per chunk expected (%d), got %d" % (who, name, n, len(t)))
            for i, e in enumerate(envelopes):
                if e is not None:
                    if not isinstance(e, Envelope):
                        raise TypeError("%s: envelopes hold wire.Envelope values or None" % who)
                    e.check("%s: chunk %d" % (who, i), 1, chunks[i].in_total, dev)
            ev = (_capi.MbvPcmEnvelope * n)(*[_envelope_c(e) for e in envelopes])
        lim = _limits_c(who, "chunk", limits, n)
        fd = _fades_c(who, "chunk", fades, n)
        name, tables, takes_law = _chunks_entry(lim, law, fd, ev)
        self._call(name, chunks, *tables, n, int(orig_sr), int(target_sr), filt, *((law,) if takes_law else ()), packed, cap)

    @torch.no_grad()
    def resample_turns(self, turns, orig_sr, target_sr, packed=None, res_type="kaiser_best", limits=None,
                       encoding="pcm16", fades=None, envelopes=None):
        """`resample_pcm16_chunks` for rows whose input is a TIMELINE of utterances (`mbv_resample_turns`, DESIGN §7.18;
        `wire.PcmPool` drives it for its `wire.Turn`s): `turns` is a ctypes array (or a list) of `_capi.MbvTurnChunk`,
        each a chunk with `wave` None, `in_total` / `in_avail` the timeline's total and frontier, and `segs` a ctypes
        array of the `_capi.MbvTurnSeg` its input window touches.  Every stored value is bitwise what
        `resample_pcm16_range` stores for the timeline written out as one row (`wire.assemble_turn`).  `packed`,
        `limits`, `encoding` and `fades` as `resample_pcm16_chunks` takes them; one launch for the unlimited turns and
        one for the limited ones.  `envelopes`: None, or one list per turn with one entry per SEGMENT the turn passes,
        each None or a one-row `wire.Envelope` over that segment's own samples, applied before its de-click ramp
        (`mbv_resample_turns_shaped`).  No host synchronisation (beyond the first call for a rate pair)."""
        who = "resample_turns"
        filt = _filter_code(res_type)
        law = _law_code(encoding)
        if not isinstance(turns, C.Array):
            turns = (_capi.MbvTurnChunk * len(turns))(*turns)
        n = len(turns)
        dev = self._device()
        cap = _packed_capacity(who, packed, law, dev)
        lim = _limits_c(who, "turn", limits, n)
        fd = _fades_c(who, "turn", fades, n)
        name, tables = "mbv_resample_turns", (lim, fd)
        if envelopes is not None and any(e is not None for per in envelopes for e in (per or ())):
            if len(envelopes) != n:
                raise ValueError("%s: one envelope list per turn expected (%d), got %d" % (who, n, len(envelopes)))
            flat = []
            for i, per in enumerate(envelopes):
                per = list(per or [None] * turns[i].n_segs)
                if len(per) != turns[i].n_segs:
                    raise ValueError("%s: turn %d: one envelope per segment expected (%d), got %d"
                                     % (who, i, turns[i].n_segs, len(per)))
                for k, e in enumerate(per):
                    if e is not None:
                        if not isinstance(e, Envelope):
                            raise TypeError("%s: envelopes hold wire.Envelope values or None" % who)
                        e.check("%s: turn %d: segment %d" % (who, i, k), 1, turns[i].segs[k].length, dev)
                    flat.append(_envelope_c(e))
            name, tables = "mbv_resample_turns_shaped", (lim, fd, (_capi.MbvPcmEnvelope * max(len(flat), 1))(*flat))
        self._call(name, turns, *tables, n, int(orig_sr), int(target_sr), filt, law, packed, cap)

    @torch.no_grad()
    def resample_ranges(self, rows, orig_sr, target_sr, res_type="kaiser_best"):
        """The input side of a live wire (`mbv_resample_ranges`; `wire.LiveWire` and `wire.PcmPool` drive it): `rows`
        is a ctypes array (or a list) of `_capi.MbvResampleRange`, each the raw buffer of one recording that is still
        arriving (fp32 or int16, device address), how much of it exists, and the range of its model-rate row to write.
        ONE launch for all rows; every stored value is bitwise what `resample` gives there for the finished recording.
        A range must end at or below `wire.resample_ready_open(orig_sr, target_sr, in_avail)` while the recording is
        open.  No host synchronisation (beyond the first call for a rate pair)."""
        filt = _filter_code(res_type)
        if not isinstance(rows, C.Array):
            rows = (_capi.MbvResampleRange * len(rows))(*rows)
        self._call("mbv_resample_ranges", rows, len(rows), int(orig_sr), int(target_sr), filt)

    # ------------------------------------------------------------------ per-token pitch
    def warp_runs(self):
        """Launches of the time-warp kernel made on this model's handle so far (`mbv_warp_runs`)."""
        return int(_capi.lib().mbv_warp_runs(self._ensure_handle()))

    def warp_map(self, pitch, durations, glide_frames=PITCH_GLIDE_FRAMES):
        """The `stream.WarpMap` of ONE utterance for users of the batch `infer`: `pitch` as `infer_stream(pitch=)` takes
        it ([T_text] factors on the host), `durations` the frames per token the utterance was made with ([T_text], or
        [1, 1, T_text] as `infer(...)[4]` returns them: a read-back when they live on the device).  The tables are
        uploaded to the model's device."""
        d = [int(round(float(v))) for v in (durations.reshape(-1).tolist() if torch.is_tensor(durations) else durations)]
        if min(d, default=0) < 0 or sum(d) < 1:
            raise ValueError("warp_map: durations must be non-negative frames per token with at least one frame")
        p = _pitch_arg("warp_map", pitch, 1, len(d), row=True)
        marks = [0]
        for v in d:
            marks.append(marks[-1] + v)
        return stream.WarpMap(stream.frame_rates(p.reshape(-1).tolist(), marks, marks[-1], glide_frames),
                              self.cfg.samples_per_frame, self._device())

    @torch.no_grad()
    def warp_ranges(self, rows):
        """`mbv_warp_ranges`: `rows` is a ctypes array (or a list) of `_capi.MbvWarpRow`, one per stream; ONE launch for
        all of them, no host synchronisation (beyond the first call for a filter)."""
        if not isinstance(rows, C.Array):
            rows = (_capi.MbvWarpRow * len(rows))(*rows)
        self._call("mbv_warp_ranges", rows, len(rows))

    @staticmethod
    def warp_row(wave, warp_map, in_avail, out_first, out_count, out, envelope=None, res_type="kaiser_best"):
        """The `_capi.MbvWarpRow` of one stream: outputs [out_first, out_first + out_count) of the warped row `out`
        ([.., n_out] fp32) from the first `in_avail` samples of `wave` (the decoded row, [.., F * hop])."""
        m = warp_map
        if m.rate_dev is None or m.rate_dev.device != wave.device:
            raise ValueError("warp: the WarpMap's tables are not on the wave's device (%s)" % (wave.device,))
        return _capi.MbvWarpRow(wave.data_ptr(), m.samples, int(in_avail), m.U_dev.data_ptr(), m.rate_dev.data_ptr(),
                                m.U.ctypes.data, m.rate.ctypes.data, m.frames, m.hop, _envelope_c(envelope),
                                int(out_first), int(out_count), out.data_ptr(), out.shape[-1], _filter_code(res_type), 0)

    @torch.no_grad()
    def warp(self, wave, warp_map, envelope=None, res_type="kaiser_best"):
        """The closed one-shot time warp: `wave` (fp32, one utterance: [n], [1, n] or [1, 1, n] with n >= F * hop of the
        map; the first F * hop samples are read) -> fp32 [1, n_out], played at the map's rates (`mbv_warp_ranges` with
        one closed row).  `envelope`: the samples are shaped where they are read, bitwise `warp(wave * e, map)`."""
        if not isinstance(warp_map, stream.WarpMap):
            raise TypeError("warp: warp_map must be a stream.WarpMap (st.warp, net.warp_map)")
        if not torch.is_tensor(wave) or wave.dtype != torch.float32:
            raise TypeError("warp: wave must be an fp32 tensor")
        if wave.numel() != wave.shape[-1]:
            raise ValueError("warp: ONE utterance ([n], [1, n] or [1, 1, n]), got %s" % (tuple(wave.shape),))
        if wave.shape[-1] < warp_map.samples:
            raise ValueError("warp: the map covers %d frames x %d = %d samples, the wave holds %d"
                             % (warp_map.frames, warp_map.hop, warp_map.samples, wave.shape[-1]))
        if envelope is not None:
            if not isinstance(envelope, Envelope):
                raise TypeError("warp: envelope must be a wire.Envelope, got %s" % type(envelope).__name__)
            envelope.check("warp", 1, warp_map.samples, self._device())
        x = wave.to(self._device()).reshape(-1).contiguous()
        out = torch.empty(1, max(warp_map.n_out, 1), device=x.device, dtype=torch.float32)[:, :warp_map.n_out]
        if warp_map.n_out:
            self.warp_ranges([self.warp_row(x, warp_map, warp_map.samples, 0, warp_map.n_out, out, envelope, res_type)])
        return out

    @torch.no_grad()
    def g711_encode(self, pcm, law):
        """int16 tensor (any shape) -> uint8 tensor of the same shape on the model's device: G.711 mu-law ("ulaw") or
        A-law ("alaw"), bitwise CPython's `audioop.lin2ulaw` / `lin2alaw` at width 2 (`mbv_g711_encode`)."""
        code = _g711_law(law)
        if not torch.is_tensor(pcm) or pcm.dtype != torch.int16:
            raise TypeError("g711_encode takes an int16 tensor")
        pcm = pcm.to(self._device()).contiguous()
        out = torch.empty(pcm.shape, device=pcm.device, dtype=torch.uint8)
        self._call("mbv_g711_encode", pcm, pcm.numel(), code, out)
        return out

    @torch.no_grad()
    def g711_decode(self, data, law):
        """uint8 tensor (any shape) of G.711 bytes -> int16 tensor of the same shape on the model's device: bitwise
        `audioop.ulaw2lin` / `alaw2lin` at width 2 (`mbv_g711_decode`)."""
        code = _g711_law(law)
        if not torch.is_tensor(data) or data.dtype != torch.uint8:
            raise TypeError("g711_decode takes a uint8 tensor")
        data = data.to(self._device()).contiguous()
        out = torch.empty(data.shape, device=data.device, dtype=torch.int16)
        self._call("mbv_g711_decode", data, data.numel(), code, out)
        return out

    # ------------------------------------------------------------------ loudness
    @torch.no_grad()
    def loudness(self, wave, rate, y_lengths=None, valid_samples=None, return_energies=False):
        """Waveform [B, 1, n] (fp32, mono, at `rate` Hz) -> fp32 [B] on the device: the ITU-R BS.1770 integrated
        loudness (LUFS) of every row over its valid samples (`mbv_loudness`): K-weighting, 400 ms blocks
        of four 100 ms segments, the -70 LKFS and the relative gate; -inf for a row with fewer than four complete
        segments or none that passes.  Valid samples come from `y_lengths` (frames, x256, clamped to the row) or
        `valid_samples` (samples); neither = whole rows.  One launch, no host synchronisation, nothing copied to the
        host.  `return_energies=True`: -> (L, energies fp64 [B, n // H]), the K-weighted energy of every 100 ms
        segment (0 behind a row's valid length)."""
        rate = int(rate)
        H, segs = _capi.loudness_segments(rate, wave.shape[-1])          # (refuses the rate before anything else)
        if y_lengths is not None and valid_samples is not None:
            raise ValueError("loudness: give y_lengths (frames) or valid_samples (samples), not both")
        if wave.dim() != 3 or wave.shape[1] != 1 or wave.shape[0] < 1 or wave.shape[-1] < 1:
            raise ValueError("wave must be [B, 1, samples]")
        dev = self._device()
        wave = wave.to(device=dev, dtype=torch.float32).contiguous()
        B, n = wave.shape[0], wave.shape[-1]
        if y_lengths is not None:
            valid_samples = (_valid_samples(y_lengths, B, dev, "y_lengths / valid_samples") * 256).clamp(0, n)
        elif valid_samples is not None:
            valid_samples = _valid_samples(valid_samples, B, dev, "y_lengths / valid_samples").clamp(0, n)
        out = torch.empty(B, device=dev, dtype=torch.float32)
        energies = torch.empty(B, segs, device=dev, dtype=torch.float64) if return_energies else None
        self._call("mbv_loudness", wave, valid_samples, B, n, rate, out, energies)
        return (out, energies) if return_energies else out

    @torch.no_grad()
    def loudness_range(self, wave, rate, in_avail, seg_first, seg_count, state, energies, loudness, valid_samples=None):
        """Segments [seg_first, seg_first + seg_count) of every row of `wave` (fp32 [B, n] or [B, 1, n], contiguous,
        device), of which the first `in_avail` samples exist (`mbv_loudness_range`; `wire.stream_pcm16(loudness=)`
        drives it): `state` fp64 [B, 4] carries the filter between calls (seg_first == 0 starts from zero),
        `energies` fp64 [B, >= segments] receives the range, `loudness` fp32 [B] the integrated loudness of segments
        [0, seg_first + seg_count).  Bitwise `loudness` of the finished rows however the segments were cut."""
        if wave.dim() == 3 and wave.shape[1] == 1:
            wave = wave[:, 0]
        dev = self._device()
        B, n = wave.shape
        for name, t, dt, shape in (("wave", wave, torch.float32, None), ("state", state, torch.float64, (B, 4)),
                                   ("energies", energies, torch.float64, None), ("loudness", loudness, torch.float32, (B,)),
                                   ("valid_samples", valid_samples, torch.int64, (B,))):
            if t is None and name == "valid_samples":
                continue
            if t is None:
                raise ValueError("loudness_range: %s is missing" % name)
            if t.device != dev or t.dtype != dt or not t.is_contiguous() or (shape and tuple(t.shape) != shape):
                raise ValueError("loudness_range: %s must be a contiguous %s tensor on %s%s"
                                 % (name, dt, dev, " of shape %s" % (shape,) if shape else ""))
        if energies.dim() != 2 or energies.shape[0] != B:
            raise ValueError("loudness_range: energies must be [B, segments]")
        self._call("mbv_loudness_range", wave, valid_samples, B, n, int(rate), int(in_avail), int(seg_first),
                   int(seg_count), state, energies, energies.shape[1], loudness)

    @torch.no_grad()
    def loudness_chunks(self, chunks, rate):
        """`loudness_range` for many rows, each of its own stream, in ONE launch (`mbv_loudness_chunks`; `wire.PcmPool`
        drives it): `chunks` is a ctypes array (or a list) of `_capi.MbvLoudnessChunk`, device addresses."""
        if not isinstance(chunks, C.Array):
            chunks = (_capi.MbvLoudnessChunk * len(chunks))(*chunks)
        self._call("mbv_loudness_chunks", chunks, len(chunks), int(rate))

    def loudness_runs(self):
        """Launches of the loudness kernel made on this model's handle so far (`mbv_loudness_runs`)."""
        return int(_capi.lib().mbv_loudness_runs(self._ensure_handle()))

    def input_runs(self):
        """Launches of the live-input resampler made on this model's handle so far (`mbv_input_runs`)."""
        return int(_capi.lib().mbv_input_runs(self._ensure_handle()))

    @torch.no_grad()
    def spectrogram(self, wave, n_fft, hop_size, win_size, valid_samples=None, center=False):
        """Waveform [B, n] or [B, 1, n] (fp32, or int16 PCM scaled by 1 / 32768 as data_utils.py:75 does) ->
        (spec fp32 [B, n_fft // 2 + 1, F], spec_lengths int64 [B]) on the GPU: spectrogram_torch(y, n_fft, sr,
        hop_size, win_size, center=False) (mel_processing.py:51-70) of every row over its valid samples
        (`valid_samples` int64 [B], clamped to the row; None = whole rows), as if alone, then padded with zero
        frames as the collate function pads a batch (data_utils.py:125-147).  spec_lengths[b] is the frame count
        of row b (0 where torch.stft would refuse a row that short); F = the frame count of a whole row.  The
        result is the `y, y_lengths` of `voice_conversion`.  No host synchronisation, except on the first call
        for an (n_fft, win_size) pair (the twiddle and window tables are built and uploaded)."""
        if center:
            raise ValueError("spectrogram: center=True is not supported (the reference calls it with center=False)")
        if wave.dtype == torch.int16:
            dtype = _capi.WAVE_PCM16
        elif wave.dtype == torch.float32:
            dtype = _capi.WAVE_F32
        else:
            raise ValueError("spectrogram: wave must be float32 or int16, got %s" % wave.dtype)
        if wave.dim() == 3 and wave.shape[1] == 1:
            wave = wave[:, 0]
        if wave.dim() != 2:
            raise ValueError("spectrogram: wave must be [B, n] or [B, 1, n]")
        n_fft, hop_size, win_size = int(n_fft), int(hop_size), int(win_size)
        L = _capi.lib()
        B, n = wave.shape
        F = L.mbv_spectrogram_frames(n, n_fft, hop_size)
        if F < 0:
            raise ValueError("spectrogram: n_fft must be a power of two in [256, 4096] and hop_size in [1, n_fft] "
                             "(n_fft %d, hop_size %d)" % (n_fft, hop_size))
        if not 1 <= win_size <= n_fft:
            raise ValueError("spectrogram: win_size must be in [1, n_fft] (win_size %d, n_fft %d)" % (win_size, n_fft))
        h = self._ensure_handle()
        dev = self._device()
        wave = wave.to(device=dev).contiguous()
        if valid_samples is not None:
            valid_samples = _valid_samples(valid_samples, B, dev)
        spec = torch.empty(B, n_fft // 2 + 1, F, device=dev, dtype=torch.float32)
        spec_lengths = torch.empty(B, device=dev, dtype=torch.int64)
        if B == 0 or n == 0:
            spec_lengths.zero_()
            return spec, spec_lengths
        with torch.cuda.device(dev):
            self._launch(h, "mbv_spectrogram", wave, dtype, valid_samples, B, n, n_fft, hop_size, win_size, spec, F,
                         spec_lengths)
        return spec, spec_lengths

    @torch.no_grad()
    def _speaker_embedding(self, sid):
        h = self._ensure_handle()
        dev = self._device()
        sid = _sid_tensor(sid).to(device=dev, dtype=torch.int64).contiguous()
        flat = sid.reshape(-1)
        if flat.numel() and (int(flat.min()) < 0 or int(flat.max()) >= self.n_speakers):
            # beyond the table: every such id must name a defined voice (`mbv_speaker_defined`)
            L = _capi.lib()
            if any(v < 0 or (v >= self.n_speakers and L.mbv_speaker_defined(h, v) != 1) for v in set(flat.tolist())):
                raise IndexError("index out of range in self")       # nn.Embedding's message
        out = torch.empty(flat.numel(), self.cfg.gin_channels, device=dev, dtype=torch.float32)
        with torch.cuda.device(dev):
            self._launch(h, "mbv_speaker_embedding", flat, flat.numel(), out)
        return out.reshape(*sid.shape, self.cfg.gin_channels)

    def kernel_times_ms(self):
        """(decoder conv stack ms, fused iSTFT+PQMF launch ms) of the last infer / dec call."""
        buf = (C.c_float * 2)()
        self._launch(self._handle, "mbv_kernel_times_ms", C.byref(buf), stream=False)
        return float(buf[0]), float(buf[1])

    def set_option(self, name, value):
        """Run-time options of the library (`mbv_set_option`): "splitk" (low-latency split-K for
        small launches), "istft_exact", "xpost_chunk_bytes", "wn_fused", "dec_streams", "tail_once", "conv_bf16" (0 / 3: opt-in split-bf16
        arithmetic in the large conv launches, see include/mbistft_vits.h).  Kept across weight refreshes; a
        handle re-created on another device starts from the defaults again."""
        self._call("mbv_set_option", name.encode(), int(value), stream=False)

    def read_stage(self, name):
        """Internal stage tensor of the last call as a flat fp32 tensor (tests/debugging)."""
        h = self._ensure_handle()
        L = _capi.lib()
        n = L.mbv_read_stage(h, name.encode(), None, 0, self._stream())
        if n < 0:
            raise _capi.MbvError(L.mbv_last_error(h).decode())
        t = torch.empty(n, device=self._device(), dtype=torch.float32)
        if L.mbv_read_stage(h, name.encode(), self._ptr(t), n, self._stream()) < 0:
            raise _capi.MbvError(L.mbv_last_error(h).decode())
        return t

    # ------------------------------------------------------------------ out of scope
    def forward(self, *a, **k):
        raise NotImplementedError("training forward (models.py:657-695) is outside the inference "
                                  "hot path this package implements; its alignment (enc_q, flow, neg_cent, "
                                  "monotonic alignment search: models.py:659-680) is `align`")

    _ALIGN_OUTPUT_NAMES = ("w", "attn", "x_mask", "y_mask", "z", "z_p", "m_p", "logs_p", "neg_cent")

    @torch.no_grad()
    def align(self, x, x_lengths, y, y_lengths, sid=None, noise_scale=1.0, outputs=None, noise=None, seed=None):
        """Forced alignment of recordings to their texts: the alignment half of the reference's `forward`
        (models.py:659-680, :690-691) -> (attn, w, x_mask, y_mask, (z, z_p, m_p, logs_p)).

          x, x_lengths   token ids [B, T_text], lengths [B]
          y, y_lengths   linear spectrogram [B, spec_channels, T_spec] (`spectrogram`), frame counts [B]
          sid            [B] for a multi-speaker model, else None
          attn           [B, 1, T_spec, T_text] the monotone path: one token per valid frame, at least one frame a token
          w              [B, 1, T_text] float frames per token = attn.sum(2); feed it to `infer(..., durations=w)`
          m_p, logs_p    the text statistics expanded by the path
          noise_scale    0: the deterministic z = m_q; else z = m_q + noise * noise_scale * exp(logs_q) with
                         noise = torch.randn(B, inter, T_spec) drawn as `voice_conversion` draws it (or `noise`)
          seed           as `infer` takes it: the posterior draw from the seeded generator instead (purpose
                         2; one launch, no torch generator touched); excludes `noise`
          outputs        None = all of the above; or names from _ALIGN_OUTPUT_NAMES: only those are materialised,
                         the rest come back as None (`outputs=("w",)` skips attn and the prior).  "neg_cent"
                         ([B, T_spec, T_text], defined for [y < y_lengths[b], x < x_lengths[b]) only) is returned as
                         a last, extra element of the tuple when named.
        Every row needs 1 <= x_lengths[b] <= y_lengths[b] (more tokens than frames have no monotone path): ValueError;
        ids / lengths / sid outside their tables: IndexError — both after the call's one host synchronisation."""
        h = self._ensure_handle()
        x, x_lengths, sid = self._check_inputs(x, x_lengths, sid)
        dev, B, T = x.device, x.shape[0], x.shape[1]
        if seed is not None and noise is not None:
            raise ValueError("align: seed= and noise= exclude each other")
        seeds = _row_seeds(seed, B)
        cfg = self.cfg
        I = cfg.inter_channels
        if y.dim() != 3 or y.shape[0] != B or y.shape[1] != cfg.spec_channels:
            raise ValueError("y must be [B, %d, T_spec] (linear spectrogram), B = %d" % (cfg.spec_channels, B))
        if y_lengths.dim() != 1 or y_lengths.shape[0] != B:
            raise ValueError("y_lengths must be [B]")
        Tp = y.shape[2]
        if T < 1 or Tp < 1:
            raise ValueError("empty text or spectrogram")
        if outputs is None:
            want = set(self._ALIGN_OUTPUT_NAMES) - {"neg_cent"}
        else:
            want = set(outputs)
            unknown = want - set(self._ALIGN_OUTPUT_NAMES)
            if unknown:
                raise ValueError("unknown output name(s) %s (known: %s)" % (sorted(unknown), ", ".join(self._ALIGN_OUTPUT_NAMES)))
        y = y.to(device=dev, dtype=torch.float32).contiguous()
        y_lengths = y_lengths.to(device=dev, dtype=torch.int64).contiguous()
        f32 = dict(device=dev, dtype=torch.float32)
        with torch.cuda.device(dev):
            if float(noise_scale) != 0.0:
                if seeds is not None:
                    noise = self._seeded_rows(h, seeds, I, Tp, _capi.NOISE_POSTERIOR)
                elif noise is None:
                    noise = torch.randn(B, I, Tp, **f32)             # randn_like(m) of models.py:245
                elif tuple(noise.shape) != (B, I, Tp):
                    raise ValueError("noise must be [B, %d, T_spec]" % I)
                noise = noise.to(**f32).contiguous()
            else:
                noise = None
            shapes = {"attn": (B, 1, Tp, T), "x_mask": (B, 1, T), "y_mask": (B, 1, Tp), "z": (B, I, Tp),
                      "z_p": (B, I, Tp), "m_p": (B, I, Tp), "logs_p": (B, I, Tp)}
            t = {k: torch.empty(*shapes[k], **f32) for k in shapes if k in want}
            if "neg_cent" in want:
                t["neg_cent"] = torch.zeros(B, Tp, T, **f32)
            w32 = torch.empty(B, T, dtype=torch.int32, device=dev)
            status = torch.empty(B, dtype=torch.int32, device=dev)
            out = _capi.MbvAlignOutputs()
            out.w = w32.data_ptr()
            for k, v in t.items():
                setattr(out, k, v.data_ptr())
            self._launch(h, "mbv_align", x, x_lengths, y, y_lengths, sid, B, T, Tp, noise, float(noise_scale), C.byref(out),
                         status)
            w = w32.to(torch.float32).unsqueeze(1) if "w" in want else None
            flags = int(status.max())                               # the one host sync
            if flags & 1:
                raise IndexError("index out of range in self (token id, x_lengths, y_lengths or sid outside the "
                                 "model's tables or the tensors)")
            if flags & 2:
                raise ValueError("align: an utterance has more tokens than frames (x_lengths > y_lengths): no monotone path")
            if flags & 4:
                raise ValueError("align: an utterance with x_lengths < 1 or y_lengths < 1")
        g = t.get
        r = (g("attn"), w, g("x_mask"), g("y_mask"), (g("z"), g("z_p"), g("m_p"), g("logs_p")))
        return r + (t["neg_cent"],) if "neg_cent" in want else r

    @torch.no_grad()
    def voice_conversion(self, y, y_lengths, sid_src, sid_tgt, seed=None):
        """-> (o_hat, o_hat_mb, y_mask, (z, z_p, z_hat))  (models.py:790-798).  `seed` (extension, as `infer` takes
        it): the posterior draw from the seeded generator (purpose 2) in one launch, no torch generator
        touched; the default draws torch.randn as before."""
        if not self.n_speakers > 0:
            raise AssertionError("n_speakers have to be larger than 0.")      # models.py:791
        h = self._ensure_handle()
        dev = self._device()
        cfg = self.cfg
        if y.dim() != 3 or y.shape[1] != cfg.spec_channels:
            raise ValueError("y must be [B, %d, T] (linear spectrogram)" % cfg.spec_channels)
        y = y.to(device=dev, dtype=torch.float32).contiguous()
        B, _, T = y.shape
        seeds = _row_seeds(seed, B)
        y_lengths = y_lengths.to(device=dev, dtype=torch.int64).contiguous()
        sid_src = _sid_tensor(sid_src).to(device=dev, dtype=torch.int64).contiguous()
        sid_tgt = _sid_tensor(sid_tgt).to(device=dev, dtype=torch.int64).contiguous()
        I = cfg.inter_channels
        f32 = dict(device=dev, dtype=torch.float32)
        with torch.cuda.device(dev):
            if seeds is not None:
                noise = self._seeded_rows(h, seeds, I, T, _capi.NOISE_POSTERIOR)
            else:
                noise = torch.randn(B, I, T, **f32)              # randn_like(m) of models.py:245
            o, o_mb, spec, phase = self._alloc_decoder_outputs(B, T, dev)
            y_mask = torch.empty(B, 1, T, **f32)
            z, z_p, z_hat = (torch.empty(B, I, T, **f32) for _ in range(3))
            status = torch.empty(B, dtype=torch.int32, device=dev)
            out = self._outputs_struct((o, o_mb, spec, phase), B)
            out.y_mask, out.z, out.z_p, out.m_p = y_mask.data_ptr(), z.data_ptr(), z_p.data_ptr(), z_hat.data_ptr()
            self._launch(h, "mbv_voice_conversion", y, y_lengths, sid_src, sid_tgt, B, T, noise, C.byref(out), status)
            if bool(status.any()):
                raise IndexError("index out of range in self (y_lengths or speaker id)")
        return o, o_mb, y_mask, (z, z_p, z_hat)
