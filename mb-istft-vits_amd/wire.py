"""Wire framing of the service wrapper (the step after `to_pcm16`): the int16 stream of one
utterance is cut into frames of `round(frame_length * rate)` samples (20 ms by default,
tts_vits.py:36-38) and every frame travels as the base64 text of its little-endian bytes
(tts_vits.py:219-226; the last frame is simply shorter).  Host-side by nature: the payload is text.

The steps before it run on the GPU: `service_pcm16` chains `SynthesizerTrn.resample` (the
`librosa.resample` of tts_vits.py:199-200, librosa 0.9.2's default res_type "kaiser_best", i.e.
resampy's windowed-sinc interpolator and fix_length) with the peak normalise / clip / int16 epilogue
(tts_vits.py:204-217).  The resampler's parity is pinned to a float64 restatement of resampy's
algorithm (tests/resample_ref.py), not to librosa / resampy themselves, which are not part of this
build: its filter tables are rebuilt from resampy's documented filter specs.  librosa >= 0.10
(the unpinned requirements.txt) defaults to soxr_hq, a different algorithm that is not provided.

`convert_pcm16` is the audio-in, audio-out form of `voice_conversion`: resample to the model's rate,
the linear spectrogram of the data path (`SynthesizerTrn.spectrogram`, mel_processing.py:51-70),
voice conversion, then `service_pcm16`.

`stream_pcm16` is the streamed form of `service_pcm16`: it follows a `stream.DecodeStream` chunk by chunk and
emits the int16 samples that have become final, bitwise those `service_pcm16` gives for the finished waveform
(`mbv_resample_pcm16_range`); `FrameCutter` is `frame_pcm16` for such a stream of pieces.

`pcm_pool` is `stream_pcm16` for many streams at once: a `PcmPool` steps a `stream.StreamPool` and wires the chunks
that step (and earlier ones) made final for ALL its streams in one `mbv_resample_pcm16_chunks` launch, and can
hand the pieces over in one pinned host buffer filled by one copy.

`convert_live_pcm16` is the live form of `convert_pcm16`: a `LiveWire` takes raw samples at the caller's rate while
they arrive, resamples what has become final into the model-rate buffer of the `stream.LiveStream` it owns
(`mbv_resample_ranges`), and wires the decoded frontier to int16 at the service's rate; `PcmPool.add_live` serves many
of them with one launch per stage and tick.

`Limiter` is the level control of all of these (`limiter=`): a look-ahead peak limiter fused into the wire step, so
that a streamed or live int16 output never reaches the hard clip, with a lag of `lookahead` output samples and the
same bytes however the stream was chunked, pooled or pushed.

`encoding="ulaw" | "alaw"` on all of these makes the wire step store G.711 bytes (8 bits per sample, what a telephony
media gateway takes at 8 kHz) where it stores int16: the codec is the epilogue of the same kernels, each byte the
`audioop.lin2ulaw` / `lin2alaw` of the int16 the call would have emitted, so every bitwise relation above carries
over.  `in_encoding=` lets a live wire take the caller's G.711 bytes as they arrive; `frame_g711` and
`FrameCutter(sample_bytes=1)` frame such a stream.

Barge-in: `PcmStream.revoke` / `PcmPool.revoke` take a stream back while it plays: the samples not yet
handed out fade to silence over a few milliseconds (a ramp inside the same wire kernels, a pure function of the output
index, so streamed = pooled = one-shot stays bitwise), the stream's length shrinks to the end of the fade, and decoding
stops with the first chunk that makes that many outputs final (`revoke_plan`).  `service_pcm16(fade=)` is the one-shot
counterpart.  `mark_samples` maps the token marks of `infer_stream(marks=True)` to wire samples, so that a caller can
fade at a token boundary (`at="token"`) and learn how many tokens the listener heard begin.

`Loudness` (`loudness=`) delivers at a programme-loudness target instead of by the peak rule: the one-shot
entries measure the ITU-R BS.1770 integrated loudness of the model-rate waveform on the device (`net.loudness`) and
choose the static gain from it; the streamed entries take the measured value as an input, as they take `peak=`, and
keep `.loudness`, the running value of what they have decoded (`mbv_loudness_range`; one `mbv_loudness_chunks` launch
per tick in a `PcmPool`).  The gain enters the wire kernels as their `peak`, so every bitwise relation above holds.

Turns: `PcmPool.add_turn` opens a `Turn`, the phrases of a dialogue turn as ONE gapless wire stream.  Its
segments are ordinary single-utterance decode streams of the pool; the wire kernels read their timeline in place
(`mbv_resample_turns`: silence in the pauses, a de-click ramp at both ends of every segment), so one resampler, one
limiter and one framing run over the joints.  `TurnPlan` is its integer planning, `assemble_turn` the timeline written
out as one row: the turn's bytes are bitwise `service_pcm16` of that row, `revoke` with `fade=` included.

Volume: a stream made with `gain=` carries `frame_gain`, the per-token gains spread over its z-frames;
`Envelope(gain, samples_per_frame)` hands them to the wire kernels, which multiply a continuous envelope into the
model-rate samples where they read them, in front of the filter, the peak, the limiter and the clip.  `stream_pcm16`,
`PcmPool.add` / `admit` and `Turn.append` / `admit` pick it up by themselves; `envelope=` names one explicitly.  The
bytes are those of `service_pcm16` on the waveform times that envelope; rows without one are bitwise what they were.

Pitch: a stream made with `pitch=` carries `warp`, a `stream.WarpMap`: the playback rate of every z-frame.
`stream_pcm16`, `PcmPool.add` / `admit` and `Turn.append` / `admit` then read the WARPED row, which they own and fill
behind the decoder with the time-warp kernel (`mbv_warp_ranges`: one launch per step of a stream, ONE per tick of a
pool for all its pitched members and segments), and everything behind it is the wire step that exists.  The bytes are
those of `service_pcm16(net.warp(st.o, st.warp))`; a stream without `pitch=` launches nothing and is bitwise what it was.
A gain envelope of such a stream goes to the warp, where the samples are read.  `.loudness` stays that of the decoded,
unwarped waveform.  Varispeed: formants move with the pitch.
"""
import base64
import collections
import ctypes as C
import math

import numpy as np
import torch

from . import _capi
# (RESAMPLE_TYPES and ENCODINGS stay names of this module)
from .models import ENCODINGS, RESAMPLE_TYPES, _filter_code, _g711_law, _law_code      # noqa: F401
from .models import Envelope, GAIN_MAX, gain_of_db                                      # noqa: F401
from .models import PITCH_MAX, PITCH_MIN, pitch_of_semitones                            # noqa: F401
from .stream import WarpMap                                                             # noqa: F401

G711_ZERO = {"ulaw": 0xFF, "alaw": 0xD5}      # the code of the int16 zero: what the wire kernels store as padding
# `wave_dtype` of a live wire's raw buffer (MBV_WAVE_*), by its dtype or, for uint8, its `in_encoding`
_WAVE_DTYPE = {torch.float32: _capi.WAVE_F32, torch.int16: _capi.WAVE_PCM16, "ulaw": _capi.WAVE_ULAW,
               "alaw": _capi.WAVE_ALAW}


def _wire_dtype(encoding):
    """The dtype of the samples a wire step stores: int16, or uint8 for the G.711 encodings (refuses any other)."""
    return torch.uint8 if _law_code(encoding) else torch.int16


def _in_law(in_encoding, in_sr, model_sr, who):
    """`in_encoding=` of an audio-in entry: None, or "ulaw" / "alaw" with rates that differ (G.711 input always passes
    through the resampler: telephone audio is at 8 kHz and no model runs at that rate)."""
    if in_encoding is None:
        return None
    _g711_law(in_encoding)
    if int(in_sr) == int(model_sr):
        raise ValueError("%s: in_encoding=%r needs in_sr != model_sr (G.711 input goes through the resampler; %d Hz "
                         "is the model's own rate)" % (who, in_encoding, int(in_sr)))
    return in_encoding


def chunk_size(rate, frame_length=0.02):
    """Samples per frame, as tts_vits.py:38 computes it."""
    return int(round(frame_length * rate))


def frame_pcm16(pcm, rate, frame_length=0.02, valid_samples=None):
    """pcm: 1-D int16 (numpy array or torch tensor, any device) of ONE utterance -> list of base64
    strings, one per frame.  `valid_samples` (e.g. 256 * y_lengths[b]) trims the zero padding of a
    batched row first."""
    if hasattr(pcm, "detach"):
        pcm = pcm.detach().cpu().numpy()
    pcm = np.ascontiguousarray(pcm)
    if pcm.dtype != np.int16 or pcm.ndim != 1:
        raise ValueError("pcm must be a 1-D int16 array (the output row of to_pcm16)")
    if valid_samples is not None:
        pcm = pcm[:int(valid_samples)]
    n = chunk_size(rate, frame_length)
    if n <= 0:
        raise ValueError("frame_length * rate must be at least one sample")
    pcm = pcm.astype("<i2", copy=False)                    # ndarray.tobytes() of the reference runs on little-endian hosts
    return [base64.b64encode(pcm[t:t + n].tobytes()).decode("utf-8") for t in range(0, len(pcm), n)]


def frame_g711(data, rate, frame_length=0.02, valid_samples=None):
    """`frame_pcm16` for G.711: data 1-D uint8 (numpy array or torch tensor, any device), one byte per sample, of ONE
    utterance -> list of base64 strings, one per frame of `chunk_size(rate, frame_length)` bytes (160 for 20 ms at
    8 kHz; the last frame is simply shorter)."""
    if hasattr(data, "detach"):
        data = data.detach().cpu().numpy()
    data = np.ascontiguousarray(data)
    if data.dtype != np.uint8 or data.ndim != 1:
        raise ValueError("data must be a 1-D uint8 array (a row of service_pcm16(encoding='ulaw' | 'alaw'))")
    if valid_samples is not None:
        data = data[:int(valid_samples)]
    n = chunk_size(rate, frame_length)
    if n <= 0:
        raise ValueError("frame_length * rate must be at least one sample")
    return [base64.b64encode(data[t:t + n].tobytes()).decode("utf-8") for t in range(0, len(data), n)]


class Limiter:
    """The look-ahead peak limiter of the wire step (`mbv_resample_pcm16_range_limited`):
      ceiling       c in (0, 1]: no output exceeds it (0.9 is the margin the service leaves, tts_vits.py:208)
      lookahead_ms  the gain ramps down over this long before a sample above c, and the stream lags by it
      hold_ms       the gain stays down this long after it, then ramps back over `lookahead_ms`
    The defaults (0.9, 5 ms, 20 ms) are conventions, not measurements.  `resolve(rate)` gives (c, L, H) in output
    samples at `rate`, L = round(lookahead_ms * rate / 1000) <= 255 and H = round(hold_ms * rate / 1000) <= 1024."""

    MAX_LOOKAHEAD, MAX_HOLD = 255, 1024

    def __init__(self, ceiling=0.9, lookahead_ms=5.0, hold_ms=20.0):
        self.ceiling, self.lookahead_ms, self.hold_ms = float(ceiling), float(lookahead_ms), float(hold_ms)
        if not 0.0 < self.ceiling <= 1.0:
            raise ValueError("Limiter: ceiling %r must be in (0, 1]" % (ceiling,))
        if not self.lookahead_ms >= 0.0 or not self.hold_ms >= 0.0:
            raise ValueError("Limiter: lookahead_ms and hold_ms must be >= 0")

    def __eq__(self, other):
        return isinstance(other, Limiter) and (self.ceiling, self.lookahead_ms, self.hold_ms) == (
            other.ceiling, other.lookahead_ms, other.hold_ms)

    def __hash__(self):
        return hash((self.ceiling, self.lookahead_ms, self.hold_ms))

    def __repr__(self):
        return "Limiter(ceiling=%r, lookahead_ms=%r, hold_ms=%r)" % (self.ceiling, self.lookahead_ms, self.hold_ms)

    def resolve(self, rate):
        """(ceiling, lookahead, hold) in output samples at `rate`; ValueError beyond the kernel's caps."""
        rate = int(rate)
        if rate <= 0:
            raise ValueError("sample rates must be positive")
        L, H = int(round(self.lookahead_ms * 1e-3 * rate)), int(round(self.hold_ms * 1e-3 * rate))
        if L > self.MAX_LOOKAHEAD:
            raise ValueError("Limiter: lookahead_ms %g is %d samples at %d Hz, more than the %d the kernel holds"
                             % (self.lookahead_ms, L, rate, self.MAX_LOOKAHEAD))
        if H > self.MAX_HOLD:
            raise ValueError("Limiter: hold_ms %g is %d samples at %d Hz, more than the %d the kernel holds"
                             % (self.hold_ms, H, rate, self.MAX_HOLD))
        return self.ceiling, L, H


def _limit_arg(limiter, rate):
    """`limiter=` of a wire entry -> None or (ceiling, lookahead, hold) at `rate`."""
    if limiter is None:
        return None
    if not isinstance(limiter, Limiter):
        raise TypeError("limiter must be a wire.Limiter or None, got %s" % type(limiter).__name__)
    return limiter.resolve(rate)


class Loudness:
    """Delivery at a programme-loudness target: the static gain of the wire step is chosen so that an
    utterance of integrated loudness L (ITU-R BS.1770, `net.loudness`) leaves at `target` LUFS, instead of as loud as
    its largest sample allows (the peak rule of tts_vits.py:205-208).
      target       LUFS; -23.0 is EBU R128's.  None: measure only, the gain stays what `peak=` makes it
      measured     None: the call measures the waveform itself (one-shot entries only).  A float, an fp32 [B] tensor or
                   another stream's `.loudness`: the L to aim from, e.g. the speaker's previous utterance; required on
                   a stream, whose own L does not exist before its last chunk (the convention of `peak=` there)
      max_gain_db  the gain never exceeds it, so that near-silence is not blown up; at most 39 dB, which keeps the
                   kernels' divisor 0.9 / g above their 0.01 threshold
    The gain is g = min(10^((target - L) / 20), 10^(max_gain_db / 20)), 1 where L is -inf, in fp32 on the device; it
    enters the wire kernels as `peak = 0.9 / g`, which they turn into the factor 0.9 / peak = g.  No kernel changes, so
    every bitwise relation of the wire path holds with that `peak`.  -23 LUFS and 20 dB are conventions, not
    measurements.  Without a `limiter` a positive gain can reach the hard clip.  The loudness is that of the model-rate
    waveform: what a lower wire rate (8 kHz G.711) removes is not accounted for."""

    MAX_GAIN_DB = 39.0

    def __init__(self, target=-23.0, measured=None, max_gain_db=20.0):
        self.target = None if target is None else float(target)
        self.max_gain_db = float(max_gain_db)
        if self.target is not None and not math.isfinite(self.target):
            raise ValueError("Loudness: target %r must be a finite LUFS value, or None to measure only" % (target,))
        if not 0.0 <= self.max_gain_db <= self.MAX_GAIN_DB:
            raise ValueError("Loudness: max_gain_db %r must be in [0, %g] (beyond it 0.9 / g falls below the wire "
                             "kernels' 0.01 threshold)" % (max_gain_db, self.MAX_GAIN_DB))
        if measured is not None and not torch.is_tensor(measured):
            measured = float(measured)
            if math.isnan(measured) or measured == math.inf:
                raise ValueError("Loudness: measured %r must be a LUFS value or -inf" % (measured,))
        self.measured = measured

    def __repr__(self):
        return "Loudness(target=%r, measured=%r, max_gain_db=%r)" % (self.target, self.measured, self.max_gain_db)

    def gain(self, L):
        """fp32 tensor of LUFS values -> the fp32 gain of each, on L's device (no read-back)."""
        if self.target is None:
            raise ValueError("Loudness(target=None) only measures: it has no gain")
        L = L.to(torch.float32)
        g = torch.pow(torch.full_like(L, 10.0), (self.target - L) / 20.0)
        g = torch.clamp(g, max=10.0 ** (self.max_gain_db / 20.0))
        return torch.where(torch.isneginf(L), torch.ones_like(g), g)

    def peak(self, L):
        """The `peak` that gives the wire kernels this gain: 0.9 / gain(L), fp32 on L's device."""
        return 0.9 / self.gain(L)

    def measured_rows(self, B, dev):
        """`measured` as an fp32 [B] tensor on `dev` (a float is a fill, not a host copy)."""
        m = self.measured
        if not torch.is_tensor(m):
            return torch.full((B,), m, device=dev, dtype=torch.float32)
        m = m.to(device=dev, dtype=torch.float32).contiguous()
        if m.shape != (B,):
            raise ValueError("Loudness: measured must be a float or an fp32 [%d] tensor, got shape %s" % (B, tuple(m.shape)))
        return m


def _loudness_arg(loudness, peak, who, stream):
    """`loudness=` of a wire entry -> None or the `Loudness`; refuses `peak=` beside it and, on a stream, a target
    without `measured`."""
    if loudness is None:
        return None
    if not isinstance(loudness, Loudness):
        raise TypeError("loudness must be a wire.Loudness or None, got %s" % type(loudness).__name__)
    if peak is not None:
        raise ValueError("%s: loudness= replaces the peak rule; give peak= or loudness=, not both" % who)
    if stream and loudness.target is not None and loudness.measured is None:
        raise ValueError("%s: a stream's own loudness does not exist before its last chunk: give "
                         "Loudness(measured=...) (a float, an fp32 tensor, another stream's .loudness), or "
                         "Loudness(target=None) to measure only" % who)
    if not stream and loudness.target is None:
        raise ValueError("%s: Loudness(target=None) only measures; net.loudness is the one-shot measurement" % who)
    return loudness


def _segments_due(done, in_avail, hop):
    """The segment count after a step that sees `in_avail` samples, `done` segments having been measured."""
    return max(int(in_avail) // hop, done)


def loudness_plan(avail, hop):
    """The segments a stream measures with each chunk, in pure integers (no tensor, no GPU): `avail` lists the
    model-rate samples that exist after each chunk (non-decreasing), `hop` the segment length H -> [(k0, k1), ...],
    chunk i measures segments [k0, k1): those its samples completed.  The ranges tile [0, avail[-1] // hop)."""
    hop = int(hop)
    if hop < 1:
        raise ValueError("loudness_plan: hop must be >= 1")
    out, done = [], 0
    for a in avail:
        k1 = _segments_due(done, a, hop)
        out.append((done, k1))
        done = k1
    return out


def _fade_arg(fade):
    """`fade=` of a one-shot wire entry -> None or (first, count), both >= 0."""
    if fade is None:
        return None
    first, count = (int(v) for v in fade)
    if first < 0 or count < 0:
        raise ValueError("fade is (first, count) in output samples, both >= 0, got %r" % (fade,))
    return first, count


def _envelope_arg(envelope, st, who):
    """`envelope=` of a wire stream over the decode stream `st` -> None or an `Envelope`: the one given, else the one of
    `st.frame_gain` (a stream made with `gain=`), else none."""
    if envelope is None:
        return None if st.frame_gain is None else Envelope(st.frame_gain, st.spf)
    if not isinstance(envelope, Envelope):
        raise TypeError("%s: envelope must be a wire.Envelope, got %s" % (who, type(envelope).__name__))
    return envelope


def _refuse_envelope(envelope, who):
    """The live wires carry no per-token volume: a converted recording has no tokens."""
    if envelope is not None:
        raise ValueError("%s: envelope= is not offered on a live wire or a converted recording (no tokens to take a "
                         "volume from); shape the finished waveform with service_pcm16(envelope=)" % who)


def _refuse_pitch(pitch, who):
    """The live wires carry no per-token pitch: a converted recording has no tokens."""
    if pitch is not None:
        raise ValueError("%s: pitch= is not offered on a live wire or a converted recording (no tokens to take a "
                         "pitch from); warp the finished waveform with net.warp(wave, net.warp_map(...))" % who)


def mark_samples(marks, samples_per_frame, model_sr, rate, lookahead=0, warp=None):
    """Token marks in z-frames (`infer_stream(marks=True)`) -> wire sample indices, in pure integers: a mark at frame f
    maps to ceil(f * samples_per_frame * rate / model_sr) + lookahead, the first wire sample at or after the token's
    first model sample, moved by the limiter's lag (a limited stream is the unlimited one `lookahead` samples later).
    `warp` (a `stream.WarpMap`): a pitched stream; the frames go through `warp.samples_of_frames` first,
    and the same integer mapping is applied to those model-rate samples of the warped row."""
    spf, model_sr, rate, lookahead = int(samples_per_frame), int(model_sr), int(rate), int(lookahead)
    if spf < 1 or model_sr < 1 or rate < 1 or lookahead < 0:
        raise ValueError("mark_samples: samples_per_frame and the rates must be positive, lookahead >= 0")
    at = [int(f) * spf for f in marks] if warp is None else warp.samples_of_frames(marks)
    return [-((-s * rate) // model_sr) + lookahead for s in at]


class _Warped:
    """The warped row of one pitched `DecodeStream`, owned by the wire stream or turn that reads it:
    `row` fp32 [1, n_out], filled range by range behind the decoder by `mbv_warp_ranges`.  A gain envelope is handed to
    the warp, where the samples are read, and not to the wire step behind it."""

    def __init__(self, net, st, env, res_type):
        self.net, self.st, self.map, self.env, self.res_type = net, st, st.warp, env, res_type
        if st.z.shape[0] != 1:
            raise ValueError("a pitched stream holds ONE utterance (this one has %d rows)" % st.z.shape[0])
        if self.map.samples != st.o.shape[-1] or self.map.rate_dev is None or self.map.rate_dev.device != st.o.device:
            raise ValueError("the stream's warp does not cover its waveform (%d frames x %d against %d samples)"
                             % (self.map.frames, self.map.hop, st.o.shape[-1]))
        self.n = self.map.n_out
        with torch.cuda.device(st.o.device):
            self.row = torch.empty(1, max(self.n, 1), device=st.o.device, dtype=torch.float32)[:, :self.n]
        self.done = 0                             # warped samples written so far

    def frontier(self, model_avail):
        """warped samples that are final once `model_avail` decoded samples exist"""
        return self.map.ready(model_avail, self.res_type)

    def due(self, model_avail):
        """-> (the `_capi.MbvWarpRow` of the range that `model_avail` decoded samples make final, its end), or None"""
        end = self.frontier(model_avail)
        if end <= self.done:
            return None
        return self.net.warp_row(self.st.o, self.map, model_avail, self.done, end - self.done, self.row, self.env,
                                 self.res_type), end


def _warp_launch(net, due):
    """ONE `mbv_warp_ranges` launch for [(a `_Warped`, (row, end))]; nothing for an empty list."""
    if due:
        net.warp_ranges([row for _, (row, _) in due])
        for w, (_, end) in due:
            w.done = end


def revoke_plan(ready, total, emitted, first, count):
    """The plan of a revoke in pure integers (no tensor, no GPU).
      ready    final outputs after each chunk of the schedule, non-decreasing (`resample_ready`, or `limiter_ready`
               with a limiter); the last is the whole row
      total    the stream's length in wire samples; emitted: those already handed out (E)
      first, count   the fade (F, N); F >= E
    -> (cut, last, ready'): the new length cut = min(total, F + N); the index of the last chunk to decode, the first
    whose end makes `ready` reach cut; and ready' = min(ready[i], cut) for i <= last: no step asks for an output at or
    beyond cut."""
    total, emitted, first, count = int(total), int(emitted), int(first), int(count)
    if count < 0:
        raise ValueError("revoke: the fade cannot be shorter than 0 samples")
    if first < emitted:
        raise ValueError("revoke: the fade cannot start at sample %d: %d samples have been handed out already"
                         % (first, emitted))
    cut = min(total, first + count)
    last = next(i for i, r in enumerate(ready) if r >= cut or i == len(ready) - 1)
    return cut, last, [min(r, cut) for r in ready[:last + 1]]


class Revoked:
    """What `revoke` reports: the fade starts at wire sample `first` and lasts `count` samples, the stream now ends at
    `valid_samples`, and (streams with marks; else None) `tokens_started` tokens begin in front of `first`: those the
    listener heard begin."""

    __slots__ = ("first", "count", "valid_samples", "tokens_started")

    def __init__(self, first, count, valid_samples, tokens_started):
        self.first, self.count, self.valid_samples, self.tokens_started = first, count, valid_samples, tokens_started

    def __repr__(self):
        return "Revoked(first=%d, count=%d, valid_samples=%d, tokens_started=%r)" % (
            self.first, self.count, self.valid_samples, self.tokens_started)


def _revoke_args(fade_ms, at, rate, emitted, total, marks=None, tokens=True, finished=False):
    """`fade_ms` and `at` of a revoke in pure integers -> (F, N): the fade starts at wire sample F, `at="now"`: `emitted`, an
    int: that sample, `at="token"`: the first of `marks` >= `emitted` (`total` when none is; None: a stream without marks;
    `tokens=False`: a turn, which offers no 'token'), and lasts N = round(fade_ms * rate / 1000) samples.  `finished`:
    nothing is left to fade, only `fade_ms` is checked, and the answer is None."""
    if not float(fade_ms) >= 0.0:
        raise ValueError("revoke: fade_ms must be >= 0")
    if finished:
        return None
    N = int(round(float(fade_ms) * 1e-3 * rate))
    if at == "now":
        F = emitted
    elif at == "token" and tokens:
        if marks is None:
            raise ValueError("revoke(at='token'): the stream has no token marks (infer_stream(marks=True); a "
                             "converted recording has no tokens)")
        F = next((m for m in marks if m >= emitted), total)
    elif isinstance(at, (int, np.integer)) and not isinstance(at, bool):
        F = int(at)
    else:
        raise ValueError("revoke: at must be 'now'%s or a wire sample index, got %r" % (", 'token'" if tokens else "", at))
    return F, N


def _service_limited(net, o, y_lengths, model_sr, rate, auto_normalize, res_type, limiter, peak, encoding="pcm16",
                     fade=None, envelope=None):
    """`service_pcm16` through the ranged wire kernel over the whole row, which is where the limiter and the G.711
    epilogue live: one launch with a given peak (or none), two with auto_normalize (the first measures the peak the
    second divides by)."""
    lim = _limit_arg(limiter, rate)
    dtype = _wire_dtype(encoding)
    dev = net._device()
    if o.dim() != 3 or o.shape[1] != 1:
        raise ValueError("wave must be [B, 1, samples]")
    wave = o.to(device=dev, dtype=torch.float32).contiguous()[:, 0]
    B, n = wave.shape
    stride = resample_ready(model_sr, rate, n, n, res_type)
    valid_in = None
    if y_lengths is not None:
        valid_in = (y_lengths.to(device=dev, dtype=torch.int64) * 256).clamp(0, n).contiguous()
    with torch.cuda.device(dev):
        pcm = torch.empty(B, stride, device=dev, dtype=dtype)
        valid = torch.zeros(B, device=dev, dtype=torch.int64)
        peak_in = _peak_arg(peak, B, dev)
        if peak_in is None and auto_normalize:
            peak_in = torch.zeros(B, device=dev, dtype=torch.float32)
            net.resample_pcm16_range(wave, model_sr, rate, n, 0, stride, pcm, valid_samples=valid_in,
                                     running_peak=peak_in, res_type=res_type, encoding=encoding, envelope=envelope)
    net.resample_pcm16_range(wave, model_sr, rate, n, 0, stride, pcm, valid_samples=valid_in, peak=peak_in,
                             out_samples=valid, res_type=res_type, limiter=lim, encoding=encoding, fade=fade,
                             envelope=envelope)
    if fade is not None:
        with torch.cuda.device(dev):
            valid.clamp_(max=fade[0] + fade[1])
    return pcm, valid


def service_pcm16(net, o, y_lengths, model_sr, rate, auto_normalize=True, res_type="kaiser_best", limiter=None,
                  peak=None, encoding="pcm16", fade=None, loudness=None, envelope=None):
    """tts_vits.py:196-217 for a batch as one GPU chain: resample every utterance from `model_sr` to
    `rate` (skipped when they are equal, as there), then peak-normalise / clip / int16 it.
      o          fp32 [B, 1, n] waveforms of `net.infer` (device)
      y_lengths  int64 [B] frames per utterance (valid samples = 256 * y_lengths, clamped to the row),
                 or None = whole rows
    -> (pcm int16 [B, n'], valid_samples int64 [B]); row b of `pcm` holds the int16 stream of utterance b
    in its first valid_samples[b] samples, ready for `frame_pcm16(pcm[b], rate, valid_samples=...)`.
    No host synchronisation (beyond the first call for a rate pair, see `SynthesizerTrn.resample`).
      limiter  a `Limiter`: the look-ahead limiter of DESIGN §7.14 between the gain and the clip; the bytes are then
               those `stream_pcm16(..., limiter=limiter)` emits for the same waveform and peak.  None: as before
      peak     with `limiter` only: a float or fp32 [B] tensor to divide by instead of the utterance's own peak, as
               `stream_pcm16` takes it (it overrides auto_normalize)
      encoding "ulaw" / "alaw": `pcm` is uint8, the G.711 byte of every int16 the call would have returned (the zero
               padding becomes 0xFF / 0xD5), fused into the ranged kernel as the limiter is: with auto_normalize one
               launch for the peak and one that encodes
      fade     (first, count) in output samples: the fade-out of a revoked stream on the finished waveform (DESIGN
               §7.16): sample t >= first is scaled by (count - (t - first)) / (count + 1) before the clip, silence from
               first + count on, and valid_samples becomes min(valid_samples, first + count).  The bytes are those a
               stream revoked with that fade emitted.  Through the ranged kernel, as `limiter` and `encoding` go
      loudness a `Loudness`: deliver at its target LUFS instead of by the peak rule.  With
               `measured=None` the call first measures the model-rate waveform (`net.loudness`, one launch more), then
               wires with the static gain that takes it to the target: the bytes are those of
               `service_pcm16(..., peak=loudness.peak(L))` on the limited path.  `auto_normalize` is ignored then (not
               refused: it is the default), `peak=` beside it is a ValueError.  Combines with `limiter`, `encoding`
               and `fade`; without a limiter a positive gain can reach the hard clip
      envelope an `Envelope` with B rows (`net.frame_gain`, or `Envelope(st.frame_gain, spf)`): per-token volume
               (DESIGN §7.20).  Every model-rate sample is scaled where the ranged kernel reads it, so the bytes are
               those of `service_pcm16(o * e)` with the same arguments: the `auto_normalize` peak is the shaped
               signal's, and the limiter holds its ceiling on it.  A `loudness` measurement stays on the UNSHAPED
               waveform: the static gain sets the normal level and the volume modulates around it"""
    law = _law_code(encoding)
    fade = _fade_arg(fade)
    if envelope is not None and not isinstance(envelope, Envelope):
        raise TypeError("service_pcm16: envelope must be a wire.Envelope, got %s" % type(envelope).__name__)
    loud = _loudness_arg(loudness, peak, "service_pcm16", stream=False)
    if loud is not None:
        _limit_arg(limiter, rate)                               # refuses bad parameters before the measuring launch
        dev = net._device()
        if o.dim() != 3 or o.shape[1] != 1:
            raise ValueError("wave must be [B, 1, samples]")
        if loud.measured is None:
            L = net.loudness(o, model_sr, y_lengths=y_lengths)
        else:
            L = loud.measured_rows(o.shape[0], dev)
        with torch.cuda.device(dev):
            peak = loud.peak(L)
        return _service_limited(net, o, y_lengths, model_sr, rate, False, res_type, limiter, peak, encoding, fade=fade,
                                envelope=envelope)
    if fade is not None or envelope is not None:
        if limiter is None and peak is not None:
            raise ValueError("service_pcm16: peak= is the static gain of the limited path; without limiter= the "
                             "utterance's own peak is used (auto_normalize)")
        return _service_limited(net, o, y_lengths, model_sr, rate, auto_normalize, res_type, limiter, peak, encoding,
                                fade=fade, envelope=envelope)
    if limiter is not None:
        return _service_limited(net, o, y_lengths, model_sr, rate, auto_normalize, res_type, limiter, peak, encoding)
    if peak is not None:
        raise ValueError("service_pcm16: peak= is the static gain of the limited path; without limiter= the "
                         "utterance's own peak is used (auto_normalize)")
    if law:
        return _service_limited(net, o, y_lengths, model_sr, rate, auto_normalize, res_type, None, None, encoding)
    wave, valid = net.resample(o, model_sr, rate, y_lengths=y_lengths, res_type=res_type)
    return net.to_pcm16(wave, auto_normalize=auto_normalize, valid_samples=valid), valid


def convert_pcm16(net, wave, valid_samples, sid_src, sid_tgt, in_sr, model_sr, rate, hop_size, win_size,
                  auto_normalize=True, res_type="kaiser_best", seed=None, limiter=None, encoding="pcm16",
                  in_encoding=None, fade=None, loudness=None, envelope=None, pitch=None):
    """Voice conversion from audio to audio as one GPU chain:
      1. `wave` int16 or fp32 [B, n] / [B, 1, n] at `in_sr` (int16 is scaled by 1 / 32768, data_utils.py:75),
         `valid_samples` int64 [B] samples per utterance or None = whole rows;
      2. `net.resample` to `model_sr` when the rates differ;
      3. `net.spectrogram` with n_fft = 2 (spec_channels - 1), the posterior encoder's input width;
      4. `net.voice_conversion(spec, spec_lengths, sid_src, sid_tgt, seed=seed)` (`seed` as `infer` takes it: None =
         torch's generator, as before);
      5. `service_pcm16(net, o, y_lengths, model_sr, rate, ...)`, with `limiter`, `encoding`, `fade` and `loudness` as
         it takes them (the loudness measured is that of the converted waveform).
    `in_encoding` "ulaw" / "alaw": `wave` is uint8 G.711 at `in_sr` != `model_sr`; it is expanded by `net.g711_decode`
    and goes on as int16.
    -> (pcm int16 [B, n'], valid_samples int64 [B]) as `service_pcm16` returns them.  Raises ValueError before
    anything is launched when win_size > n_fft or the model has no speakers.  The one host synchronisation is
    the status check `voice_conversion` already has (besides the first-call table uploads of `resample` and
    `spectrogram`)."""
    _refuse_envelope(envelope, "convert_pcm16")
    _refuse_pitch(pitch, "convert_pcm16")
    _limit_arg(limiter, rate)                                   # refuses bad parameters before anything is launched
    _law_code(encoding)
    _fade_arg(fade)
    _loudness_arg(loudness, None, "convert_pcm16", stream=False)
    in_law = _in_law(in_encoding, in_sr, model_sr, "convert_pcm16")
    if (wave.dtype == torch.uint8) != (in_law is not None):
        raise TypeError("convert_pcm16: uint8 samples need in_encoding='ulaw' | 'alaw', and in_encoding takes uint8 "
                        "samples (got %s, in_encoding=%r)" % (wave.dtype, in_encoding))
    n_fft = 2 * (net.cfg.spec_channels - 1)
    if not net.n_speakers > 0:
        raise ValueError("convert_pcm16: voice conversion needs a multi-speaker model (n_speakers > 0)")
    if not 1 <= int(win_size) <= n_fft:
        raise ValueError("convert_pcm16: win_size %d must be in [1, n_fft = 2 * (spec_channels - 1) = %d]"
                         % (int(win_size), n_fft))
    if in_law:
        wave = net.g711_decode(wave, in_law)
    if wave.dim() == 2:
        wave = wave.unsqueeze(1)
    if wave.dtype == torch.int16 and int(in_sr) != int(model_sr):
        wave = wave.float() / 32768.0                          # the resampler takes fp32; exact scaling
    wave, valid = net.resample(wave, in_sr, model_sr, valid_samples=valid_samples, res_type=res_type)
    spec, spec_lengths = net.spectrogram(wave, n_fft, hop_size, win_size, valid_samples=valid)
    o = net.voice_conversion(spec, spec_lengths, sid_src, sid_tgt, seed=seed)[0]
    return service_pcm16(net, o, spec_lengths, model_sr, rate, auto_normalize=auto_normalize, res_type=res_type,
                         limiter=limiter, encoding=encoding, fade=fade, loudness=loudness)


def _ready_call(name, *args):
    """A host-only entry of the library that answers with a count, or with a negative value and its reason in
    `mbv_last_error`: -> the count, or `_capi.MbvError`."""
    L = _capi.lib()
    r = getattr(L, name)(*args)
    if r < 0:
        msg = L.mbv_last_error(None)
        raise _capi.MbvError(msg.decode() if msg else name + " failed")
    return int(r)


def resample_ready(orig_sr, target_sr, in_avail, in_total, res_type="kaiser_best"):
    """How many resampled samples of a row of `in_total` input samples are final once its first `in_avail`
    exist (`mbv_resample_ready`, host only: no GPU needed); ceil(in_total * target / orig) once all do."""
    return _ready_call("mbv_resample_ready", int(orig_sr), int(target_sr), _filter_code(res_type), int(in_avail),
                       int(in_total))


def resample_ready_open(orig_sr, target_sr, in_avail, res_type="kaiser_best"):
    """How many resampled samples of a row that is still OPEN are final once its first `in_avail` samples exist
    (`mbv_resample_ready_open`, host only: no GPU needed): those no tap of which lies at or past `in_avail`.  The
    count does not depend on the length the row will have."""
    return _ready_call("mbv_resample_ready_open", int(orig_sr), int(target_sr), _filter_code(res_type), int(in_avail))


def limiter_ready(orig_sr, target_sr, in_avail, in_total, lookahead, res_type="kaiser_best"):
    """How many int16 samples are final under a limiter of `lookahead` output samples (the rule of
    `mbv_limiter_ready`, restated on `resample_ready` / `resample_ready_open`; host only): output t reads the
    resampled samples up to t + lookahead, so it is final once t + lookahead is below what the resampler has made
    final, and everything is once the row is complete.  `in_total` None or negative: an open recording."""
    lookahead = int(lookahead)
    if not 0 <= lookahead <= Limiter.MAX_LOOKAHEAD:
        raise ValueError("limiter lookahead must be in [0, %d] output samples" % Limiter.MAX_LOOKAHEAD)
    in_avail = max(int(in_avail), 0)
    if in_total is None or int(in_total) < 0:
        return max(resample_ready_open(orig_sr, target_sr, in_avail, res_type) - lookahead, 0)
    ready = resample_ready(orig_sr, target_sr, in_avail, in_total, res_type)
    return ready if in_avail >= int(in_total) else max(ready - lookahead, 0)


def _refuse_live(st):
    from .stream import LiveStream
    if isinstance(st, LiveStream):
        raise TypeError("a PcmStream does not follow a LiveStream (net.convert_live): its schedule, output length and "
                        "valid_samples need the recording's total length, which an open stream does not have. "
                        "wire.convert_live_pcm16 / PcmPool.add_live wire a live stream; or take the float chunks "
                        "from poll(), or convert the finished recording with convert_stream")


def _peak_arg(peak, B, dev, shape="B"):
    """`peak=` of a wire stream -> None (no normalisation) or a contiguous fp32 [B] device tensor."""
    if peak is None:
        return None
    if not torch.is_tensor(peak):
        peak = torch.full((B,), float(peak), device=dev, dtype=torch.float32)   # a fill, not a host copy
    peak = peak.to(device=dev, dtype=torch.float32).contiguous()
    if peak.shape != (B,):
        raise ValueError("peak must be a float or an fp32 [%s] tensor" % shape)
    return peak


def _per_request(who, noun, value, n):
    """`value`, one for all `n` requests or a list / tuple of one per request -> the list of n."""
    each = list(value) if isinstance(value, (list, tuple)) else [value] * n
    if len(each) != n:
        raise ValueError("%s: one %s per request expected (%d), got %d" % (who, noun, n, len(each)))
    return each


def _decoded_samples(st, i=None):
    """Model-rate samples of a `DecodeStream` that exist once its chunk i is decoded (None: as far as it is decoded)."""
    if i is None:
        i = st._decoded - 1
    return st.spf * sum(st.schedule[i]) if i >= 0 else 0


_KINDS = ("stream", "live wire", "turn")     # the kinds of wire stream, in the order `PcmPool.step` reports them
# What `_wire_chunk` answers with: k, the filled `_capi.MbvPcmChunk` (`MbvTurnChunk` of a turn); pieces, the [(a, b)] it makes
# final; final, whether it is the member's last step (None: a turn learns that from its plan); lim and fade, the member's
# `_lim` and `_fade`; env, the row's `Envelope` or None (a turn: one per segment of the row).
_Due = collections.namedtuple("_Due", "k pieces final lim fade env")


class _WireOut:
    """The output state of a wire stream and its membership of a `PcmPool`; `PcmStream`, `LiveWire` and `Turn` derive from
    it, and the state is opened here and nowhere else: pcm, valid_samples, peak (what the kernels write), _peak_in (from
    `peak=` or a `Loudness` with a target), _valid_in, limiter and _lim, _fade, _env, _warp, and with a measuring
    `Loudness` loudness, _lstate fp64 [B, 4], _lenergy fp64 [B, capacity // H] and _lseg, the segments measured so far.

    A wire step turns the first `in_avail` samples of `wave` [B, n] into the int16 samples [out_first, out_first +
    out_count); `lengths`: it also writes `valid_samples`.  Alone it is one `mbv_resample_pcm16_range` launch, in a pool
    one row of the tick's table; so its measuring half, over the segments those samples completed (`mbv_loudness_range`).

    The member protocol that `PcmPool.step` drives: _KIND, one of `_KINDS`; _TURNS, the row goes to
    `net.resample_turns` and not to `net.resample_pcm16_chunks`; _name, what `step` reports the pieces under and
    `streams=` names the member by; _decode_streams(), what `StreamPool.step` steps for it; _warp_dues(); _wire_chunk(),
    None or the `_Due` of the step due now; _measure_row(k), the `_capi.MbvLoudnessChunk` due beside the wire row k, or
    None; _chunk_wired(pieces, final), the step is issued; _wired_out, nothing more to wire: the member leaves the pool.

    `_check_handle` (needs `_h`) and `_revoke_begin` / `_revoke_end` (need `finished`, `_started`) serve a `PcmStream` and a
    `Turn` only: a `LiveWire` checks its `LiveStream`'s handle and is not revoked."""

    _KIND, _TURNS = None, False
    _name = property(lambda self: self)           # (a follower goes by its decode stream)
    _valid_in = _env = _warp = None               # what a wire step also reads; the class that has one sets it

    def __init__(self, net, dev, B, width, *, model_sr, rate, res_type, encoding, peak, limiter, loud, capacity, silent):
        """`loud`: the resolved `Loudness` or None, and `capacity`, the model-rate samples its measurement covers (0 or
        None: it gives a gain at most).  `silent`: the ONE row of a live wire or a turn, a capacity that starts as silence
        (and whose `peak=` refusal says "[1]"); else the B rows of a finished schedule, left unwritten."""
        self._net, self.model_sr, self.rate, self.res_type = net, int(model_sr), int(rate), res_type
        self.encoding, dtype = encoding, _wire_dtype(encoding)
        self.limiter, self._lim = limiter, _limit_arg(limiter, rate)
        self._loud, self.loudness = loud, None
        with torch.cuda.device(dev):
            if not silent:
                self.pcm = torch.empty(B, width, device=dev, dtype=dtype)
            elif _law_code(encoding):             # silence in G.711 is not the zero byte
                self.pcm = torch.full((B, width), G711_ZERO[encoding], device=dev, dtype=dtype)
            else:
                self.pcm = torch.zeros(B, width, device=dev, dtype=dtype)
            self.valid_samples = torch.zeros(B, device=dev, dtype=torch.int64)
            self.peak = torch.zeros(B, device=dev, dtype=torch.float32)
            self._peak_in = _peak_arg(peak, B, dev, shape="1" if silent else "B")
            if loud is not None and loud.target is not None:
                self._peak_in = loud.peak(loud.measured_rows(B, dev)).contiguous()
            if loud is not None and capacity:
                self._lhop, segs = _capi.loudness_segments(self.model_sr, capacity)
                self.loudness = torch.full((B,), -math.inf, device=dev, dtype=torch.float32)
                self._lstate = torch.zeros(B, 4, device=dev, dtype=torch.float64)
                self._lenergy = torch.zeros(B, max(segs, 1), device=dev, dtype=torch.float64)
                self._lseg = 0
        self._fade = None                         # (first, count) once revoked with a fade inside the stream
        self._revoked = None                      # the `Revoked` report of the revoke that stands

    def _check_handle(self, who):
        if self._net._handle is not self._h:
            raise RuntimeError("the model's handle was re-created (device move) since %s started" % who)

    # ---- the wire step and its measuring half, alone and as a row of a pool's tick
    def _wire_alone(self, wave, in_avail, out_first, out_count, lengths):
        self._net.resample_pcm16_range(wave, self.model_sr, self.rate, in_avail, out_first, out_count, self.pcm,
                                       valid_samples=self._valid_in, peak=self._peak_in, running_peak=self.peak,
                                       out_samples=self.valid_samples if lengths else None, res_type=self.res_type,
                                       limiter=self._lim, encoding=self.encoding, fade=self._fade, envelope=self._env)

    def _wire_row(self, wave, in_avail, out_first, out_count, lengths):
        k = _capi.MbvPcmChunk()
        k.wave, k.in_total = wave.data_ptr(), wave.shape[1]
        k.valid_samples = self._valid_in.data_ptr() if self._valid_in is not None else None
        k.in_avail, k.out_first, k.out_count = in_avail, out_first, out_count
        k.peak = self._peak_in.data_ptr() if self._peak_in is not None else None
        k.pcm, k.pcm_capacity = self.pcm.data_ptr(), self.pcm.shape[1]
        k.running_peak = self.peak.data_ptr()
        k.out_samples = self.valid_samples.data_ptr() if lengths else None
        return k

    def _loudness_alone(self, wave, in_avail):
        if self.loudness is None:
            return
        k1 = _segments_due(self._lseg, in_avail, self._lhop)
        if k1 > self._lseg:
            self._net.loudness_range(wave, self.model_sr, in_avail, self._lseg, k1 - self._lseg, self._lstate,
                                     self._lenergy, self.loudness, valid_samples=self._valid_in)
            self._lseg = k1

    def _loudness_row(self, wave_ptr, in_total, in_avail):
        """-> the `_capi.MbvLoudnessChunk` of the segments due now (`_lseg` moves once it is launched), or None."""
        k1 = _segments_due(self._lseg, in_avail, self._lhop)
        if k1 <= self._lseg:
            return None
        k = _capi.MbvLoudnessChunk()
        k.wave, k.in_total, k.in_avail = wave_ptr, in_total, in_avail
        k.valid_samples = self._valid_in.data_ptr() if self._valid_in is not None else None
        k.seg_first, k.seg_count = self._lseg, k1 - self._lseg
        k.state, k.energies, k.energy_capacity = self._lstate.data_ptr(), self._lenergy.data_ptr(), self._lenergy.shape[1]
        k.loudness = self.loudness.data_ptr()
        return k

    def _due(self, k, pieces, final, env):
        return _Due(k, pieces, final, self._lim, self._fade, env)

    def _measure_row(self, k):
        return None if self.loudness is None else self._loudness_row(k.wave, k.in_total, k.in_avail)

    def _warp_dues(self):
        return []

    # ---- barge-in: the halves of `revoke` that a stream and a turn share
    def _revoke_begin(self, fade_ms, at, emitted, total, marks=None, tokens=True):
        """-> (the report that stands, None) for a revoked or finished stream; else (None, (F, N)) of `_revoke_args`."""
        if self._revoked is not None:
            return self._revoked, None
        fade = _revoke_args(fade_ms, at, self.rate, emitted, total, marks, tokens, self.finished)
        return (Revoked(total, 0, total, self._started(total)) if fade is None else None), fade

    def _revoke_end(self, first, count, cut, total):
        """The fade (inside the stream only) and the `Revoked` report that now stands."""
        if first < total:
            self._fade = (first, count)
        self._revoked = Revoked(first, count, cut, self._started(first))
        return self._revoked


class PcmStream(_WireOut):
    """Iterator over (first_out_sample, pcm[:, a:b]) of one streamed decode: after every chunk of the wrapped
    `stream.DecodeStream` one `mbv_resample_pcm16_range` launch turns the resampled samples that chunk made final
    into int16, on the caller's current stream, and the view is ordered on that stream like every other output.
    The filter needs input on both sides of an output, so the wire lags the decoder by the filter's half-width
    (64 input samples for kaiser_best upsampling); the last chunk flushes it.  A chunk shorter than that lag
    yields an empty view.  With a `limiter` the lag grows by its lookahead, in output samples (`limiter_ready`).  No
    host synchronisation per chunk.

      pcm            int16 [B, out_stride], out_stride = ceil(spf T' * rate / model_sr); after the last chunk
                     bitwise the `service_pcm16` of the finished `st.o` (auto_normalize = `peak is not None`
                     when `peak` is the utterance's true peak).  uint8 G.711 bytes with `encoding` "ulaw" / "alaw",
                     then bitwise `service_pcm16(..., encoding=encoding)`
      valid_samples  int64 [B] device, the lengths `service_pcm16` returns (written by the first chunk)
      peak           fp32 [B] device, the running peak of the resampled samples emitted so far; after the last
                     chunk bitwise the peak `service_pcm16(auto_normalize=True)` would have divided by
      loudness       (streams opened with `loudness=`; else None) fp32 [B] device, the running BS.1770 integrated
                     loudness of the decoded model-rate samples so far, updated by the step that wires a chunk over the
                     100 ms segments that chunk completed (one `mbv_loudness_range` launch, none when it completed
                     none); after the last chunk bitwise `net.loudness(st.o, model_sr, y_lengths)`

    All state lives in tensors the stream owns, so paused and interleaved streams on one model do not mix.

    A `PcmPool` may wire chunks ahead of the iterator (`_wired` > the decode stream's `_next`): `next()` then hands
    such a piece out without launching anything, and launches alone otherwise — the same bytes either way.

    A pitched stream (`st.warp`) is read through `_src_row`, `_src_n` and `_src_frontier`: the warped row
    this stream owns, its length and its frontier, in place of `st.o`; `loudness` stays measured on the decoded row.

    `marks` (a stream made with `marks=True`; else None) lists the wire sample at which every token starts
    (`mark_samples`, the limiter's lag included).  `revoke()` takes the stream back with a fade-out; `finished` and
    `revoked` say where it stands."""

    def __init__(self, net, st, model_sr, rate, peak=None, res_type="kaiser_best", limiter=None, encoding="pcm16",
                 loudness=None, envelope=None):
        _refuse_live(st)
        loud = _loudness_arg(loudness, peak, "stream_pcm16", stream=True)
        # per-token volume: given, or the stream's own frame gains; None: the row is not shaped
        env = _envelope_arg(envelope, st, "stream_pcm16")
        if env is not None:
            env.check("stream_pcm16", st.o.shape[0], st.o.shape[-1], st.o.device)
        # per-token pitch: the wire reads the warped row this stream owns; the envelope goes to the warp
        warp = None if st.warp is None else _Warped(net, st, env, res_type)
        self._st, self._h, self._env, self._warp = st, st._h, (env if warp is None else None), warp
        _wire_dtype(encoding)                     # (refused here, in the order of before: encoding, limiter, rate pair)
        lim = _limit_arg(limiter, rate)
        lag = lim[1] if lim else 0
        o = st.o
        B, n, dev = o.shape[0], (o.shape[-1] if warp is None else warp.n), o.device
        self._src_n = n
        # final outputs after each decoded chunk (pure integers of the schedule: nothing to ask the device)
        self._front = [self._src_frontier(i) for i in range(len(st.schedule))]
        self._ready = [limiter_ready(model_sr, rate, a, n, lag, res_type) for a in self._front]
        self.out_stride = resample_ready(model_sr, rate, n, n, res_type)
        super().__init__(net, dev, B, self.out_stride, model_sr=model_sr, rate=rate, res_type=res_type, encoding=encoding,
                         peak=peak, limiter=limiter, loud=loud, capacity=o.shape[-1], silent=False)
        # valid input samples, as service_pcm16 counts them (a warped row is valid over its whole length)
        if st.y_lengths is not None and warp is None:
            self._valid_in = (st.y_lengths.to(device=dev, dtype=torch.int64) * 256).clamp(0, n).contiguous()
        self._done = 0                            # outputs emitted so far
        self._wired = 0                           # the first chunk whose final outputs are not emitted yet
        self._cut = None                          # the length a revoke left: valid_samples is clamped to it
        # token marks in wire samples (None: the stream carries none, e.g. a converted recording)
        self.marks = None
        if st.marks is not None:
            each = [mark_samples(m, st.spf, model_sr, rate, lag, warp=st.warp) for m in (st.marks if B > 1 else [st.marks])]
            self.marks = each if B > 1 else each[0]

    # ---- the input of the wire step: the decoded row, or the warped row of a pitched stream
    def _src_row(self):
        return self._st.o[:, 0] if self._warp is None else self._warp.row

    def _src_frontier(self, i):
        """input samples of the wire step that exist once chunk i is decoded"""
        a = _decoded_samples(self._st, i)
        return a if self._warp is None else self._warp.frontier(a)

    def _warp_dues(self, i=None):
        """[(the `_Warped`, (row, end))] of the warp range that chunk i made final (None: the last decoded, in a pool's
        tick), in front of its wire step; at most one"""
        i = self._st._decoded - 1 if i is None else i
        due = self._warp.due(_decoded_samples(self._st, i)) if self._warp is not None and i >= self._wired else None
        return [(self._warp, due)] if due else []

    def _measured(self, i):
        """what the loudness of step i is measured on: the DECODED row and frontier, warped or not"""
        return self._st.o[:, 0], _decoded_samples(self._st, i)

    def __len__(self):
        return len(self._st)

    @property
    def finished(self):
        """Every chunk the stream will decode is wired (after a revoke: every chunk up to the end of the fade)."""
        return self._wired >= len(self._st.schedule)

    @property
    def revoked(self):
        return self._revoked is not None

    def _total(self):
        """The stream's length in wire samples, on the host: what `valid_samples` holds for a single utterance, whose
        `y_lengths` covers at least the frames the stream keeps."""
        n = self._src_n
        v = n if self._st.y_lengths is None or self._warp is not None else min(256 * self._st.z.shape[2], n)
        return resample_ready(self.model_sr, self.rate, v, v, self.res_type)

    def _clamp_valid(self):
        # (the first wire step writes valid_samples; a revoke before it is applied right after that step)
        if self._cut is not None and self._wired > 0:
            with torch.cuda.device(self.valid_samples.device):
                self.valid_samples.clamp_(max=self._cut)
            self._cut = None

    def revoke(self, fade_ms=5.0, at="now"):
        """Takes the stream back (barge-in): what has been handed out stays, the rest fades to silence
        and the stream ends there.  With E the samples handed out so far and N = round(fade_ms * rate / 1000):
          at="now"    the fade starts at F = E
          at="token"  at the first token mark >= E (`marks`; ValueError on a stream without marks)
          at=int      at that wire sample (ValueError below E)
        The stream's length becomes min(old length, F + N) (`valid_samples`); sample t in [F, F + N) is scaled by
        (N - (t - F)) / (N + 1) before the clip, N = 0 is a hard cut.  Decoding stops with the first chunk whose end
        makes F + N outputs final (`revoke_plan`): the later chunks are never issued, and `finished` turns true after
        it.  The whole stream is bitwise `service_pcm16(..., fade=(F, N))` of the finished waveform over the new
        length.  -> a `Revoked` report.  Revoking a finished or already revoked stream changes nothing and returns
        the report of what stands.  The 5 ms default is a convention, like the limiter's, not a measurement.  Single
        utterances only (B = 1), as a pool takes them."""
        if self._revoked is None and self.pcm.shape[0] != 1:
            raise ValueError("revoke: a stream of ONE utterance is taken back (this one has %d rows)" % self.pcm.shape[0])
        total, E = self._total(), self._done
        report, fade = self._revoke_begin(fade_ms, at, E, total, self.marks)
        if fade is None:
            return report
        cut, last, ready = revoke_plan(self._ready, total, E, *fade)     # (refuses F < E before anything changes)
        st = self._st
        keep = max(last + 1, st._decoded, self._wired)
        st._truncate(keep)
        self._ready = ready + [cut] * (keep - len(ready))
        self._cut = cut
        self._clamp_valid()
        return self._revoke_end(*fade, cut, total)

    def _started(self, first):
        return None if self.marks is None else sum(1 for m in self.marks[:-1] if m < first)

    def __iter__(self):
        return self

    def __next__(self):
        st, net = self._st, self._net
        i = st._next
        next(st)                                  # decodes chunk i (StopIteration ends this stream too)
        self._check_handle("this stream")
        if i < self._wired:                       # a pool wired it already, on the stream current at its step
            a, b = (self._ready[i - 1] if i else 0), self._ready[i]
            return a, self.pcm[:, a:b]
        a, b = self._done, self._ready[i]
        step = self._step_through(i)
        _warp_launch(net, self._warp_dues(i))      # the newly ready warped range, in front of the wire step
        self._wire_alone(*step)
        self._loudness_alone(*self._measured(i))
        self._done, self._wired = b, i + 1
        self._clamp_valid()
        return a, self.pcm[:, a:b]

    def _step_through(self, i):
        """The wire step that takes in the decoded chunks up to chunk i."""
        return self._src_row(), self._front[i], self._done, self._ready[i] - self._done, self._wired == 0

    # ---- the member of a pool (the protocol of `_WireOut`)
    _KIND = "stream"
    _wired_out = finished
    _name = property(lambda self: self._st)

    def _decode_streams(self):
        return [self._st]

    def _wire_chunk(self):
        i = self._st._decoded - 1
        if i < self._wired:
            return None
        self._check_handle("a pooled stream")
        return self._due(self._wire_row(*self._step_through(i)), [(self._done, self._ready[i])],
                         i + 1 == len(self._st.schedule), self._env)

    def _measure_row(self, k):
        if self.loudness is None:
            return None
        o, avail = self._measured(self._st._decoded - 1)          # (a pitched member: its decoded row, not `k`'s)
        return self._loudness_row(o.data_ptr(), o.shape[-1], avail)

    def _chunk_wired(self, pieces, final):
        self._done, self._wired = pieces[-1][1], self._st._decoded
        self._clamp_valid()

    def run(self):
        """Every remaining chunk; -> (pcm, valid_samples)."""
        for _ in self:
            pass
        return self.pcm, self.valid_samples


def stream_pcm16(net, st, model_sr, rate, peak=None, res_type="kaiser_best", limiter=None, encoding="pcm16",
                 loudness=None, envelope=None):
    """The streamed `service_pcm16`: wraps a `stream.DecodeStream` (`net.dec_stream` / `net.infer_stream`, not yet
    iterated) in a `PcmStream`.
      peak  None: no normalisation (auto_normalize=False, exact).  A float or an fp32 [B] tensor: every sample is
            divided by it and scaled by 0.9 where it exceeds 0.01, as tts_vits.py:205-208 does with the peak of
            the whole resampled utterance.  That peak does not exist before the last chunk, so it is an input
            here (e.g. `PcmStream.peak` of the speaker's previous utterance), a static gain and no more: one
            chosen too small hard-clips (audible distortion), one chosen too large leaves the utterance quiet.
            Give a `limiter` to take the level off the guess.
      limiter  None, or a `Limiter`: the look-ahead limiter of DESIGN §7.14 after the static gain, so that no sample
            reaches the clip; `peak` and the limiter combine.  The stream then lags by the limiter's lookahead as
            well, and the bytes are those of `service_pcm16(..., limiter=limiter, peak=peak)` on the finished
            waveform.  Where nothing exceeds the ceiling they are the bytes without a limiter.
      encoding  "pcm16", or "ulaw" / "alaw": the pieces are uint8 G.711 bytes, those of
            `service_pcm16(..., encoding=encoding)` on the finished waveform.
      loudness  None, or a `Loudness`: the static gain comes from its `measured` LUFS (required with a
            target, as `peak` is an input here; `peak=` beside it is a ValueError) and the stream keeps `.loudness`,
            the running integrated loudness of what it has decoded, e.g. the `measured` of the speaker's next
            utterance.  `Loudness(target=None)` measures only: the bytes are those without `loudness=`.
      envelope  None, or an `Envelope`: per-token volume.  None on a stream made with `gain=` takes
            `Envelope(st.frame_gain, st.spf)` by itself.  The samples are scaled where the wire kernel reads them, in
            front of the filter, the peak, the limiter and the clip: the bytes are those of
            `service_pcm16(st.o, envelope=...)`, and of `service_pcm16(st.o * e)`.  The running `.loudness` stays that
            of the unshaped waveform.
    A stream made with `pitch=` (`st.warp`; one utterance) is wired from its WARPED row, which the wire
    stream owns and fills behind the decoder, one `mbv_warp_ranges` launch in front of each wire step: `pcm`,
    `valid_samples`, `marks` and `revoke` count warped samples, and the bytes are those of
    `service_pcm16(net.warp(st.o, st.warp), ...)`.  Its envelope, if any, is read by the warp.  The running `.loudness`
    stays that of the decoded, unwarped waveform."""
    if st._next:
        raise ValueError("stream_pcm16: the decode stream has already been advanced")
    return PcmStream(net, st, model_sr, rate, peak=peak, res_type=res_type, limiter=limiter, encoding=encoding,
                     loudness=loudness, envelope=envelope)


def pcm_chunks_plan(orig_sr, target_sr, chunks, res_type="kaiser_best"):
    """(total, packed_first) of `mbv_pcm_chunks_plan` for `_capi.MbvPcmChunk`s (host only: no GPU needed, only the
    integer fields are read): the checks `resample_pcm16_chunks` makes, and where every chunk starts in the packed
    buffer.  Raises `_capi.MbvError` naming the offending chunk."""
    filt = _filter_code(res_type)
    if not isinstance(chunks, C.Array):
        chunks = (_capi.MbvPcmChunk * len(chunks))(*chunks)
    n = len(chunks)
    first = (C.c_int64 * max(n, 1))()
    total = _ready_call("mbv_pcm_chunks_plan", int(orig_sr), int(target_sr), filt, chunks, n, first)
    return total, list(first)[:n]


def wire_runs(net):
    """Resample / int16 launches of the streamed wire step made on the model's handle so far (`mbv_wire_runs`):
    one per `resample_pcm16_range` call that had something to write, one per `resample_pcm16_chunks` call."""
    return int(_capi.lib().mbv_wire_runs(net._ensure_handle()))


class LiveWirePlan:
    """What a live wire may resample, and what it may hand out as int16, in pure integers (no tensor, no GPU); the
    conversion and decoding in between are the `stream.LivePlan` it wraps.

      input   model-rate sample t is final iff no tap of it lies at or past the raw samples that arrived
              (`resample_ready_open`), or the recording is closed; then there are ceil(n_raw * model_sr / in_sr) of
              them, the `out_samples` of `net.resample`.  `feed_due()` is the range to resample now; `fed(count)`
              records it and says whether it was the last of a closed recording, and the caller advances (and then
              closes) the `LivePlan` by it, as `LiveStream.fed(count, last)` does.  Equal rates: `push` and
              `close` go straight to the `LivePlan`.
      output  after decoded chunk (first, count), int16 sample u is final iff no tap of it lies at or past
              spf * (first + count); after the LAST chunk all ceil(spf * T * rate / model_sr) are.  One piece per
              decoded chunk, so the pieces do not depend on how the recording was cut into pushes.  Under a limiter
              u + `lookahead` must be final in that sense (`limiter_ready`)."""

    def __init__(self, in_sr, model_sr, rate, plan, spf, max_raw, res_type="kaiser_best", lookahead=0):
        self.in_sr, self.model_sr, self.rate, self.res_type = int(in_sr), int(model_sr), int(rate), res_type
        self.lookahead = int(lookahead)           # of the limiter on the output side: the pieces lag by it (0: none)
        if not 0 <= self.lookahead <= Limiter.MAX_LOOKAHEAD:
            raise ValueError("limiter lookahead must be in [0, %d] output samples" % Limiter.MAX_LOOKAHEAD)
        if min(self.in_sr, self.model_sr, self.rate) <= 0:
            raise ValueError("sample rates must be positive")
        self.plan, self.spf, self.max_raw = plan, int(spf), int(max_raw)
        if self.max_raw < 1:
            raise ValueError("max_samples must be >= 1")
        self.resamples = self.in_sr != self.model_sr
        if self.resamples:
            resample_ready_open(self.in_sr, self.model_sr, 0, res_type)      # refuses the rate pair / filter here
        self.capacity = self.model_total(self.max_raw)                       # model-rate samples
        frames = int(_capi.lib().mbv_spectrogram_frames(self.capacity, plan.n_fft, plan.hop))
        if frames < 1:
            raise ValueError("max_samples %d gives no spectrogram frame" % self.max_raw)
        self.o_capacity = self.spf * frames
        self.pcm_capacity = resample_ready(self.model_sr, self.rate, self.o_capacity, self.o_capacity, res_type)
        self._raw, self._closed = 0, False
        self.fed_samples = 0          # model-rate samples [0, fed_samples) are in the stream's buffer
        self.wired_chunks = 0         # decoded chunks whose final outputs are int16 already
        self.out_done = 0             # int16 samples [0, out_done) are final and written
        self.wire_done = False        # the last chunk is wired: valid is set
        self.valid = None

    def model_total(self, n_raw):
        """Model-rate samples of a finished recording of n_raw raw samples: `net.resample`'s out_samples."""
        if not self.resamples:
            return int(n_raw)
        return int(math.ceil(n_raw * (float(self.model_sr) / self.in_sr)))

    @property
    def raw(self):
        return self._raw if self.resamples else self.plan.arrived

    @property
    def closed(self):
        return self._closed if self.resamples else self.plan.closed

    def check_push(self, n):
        if self.closed:
            raise ValueError("push after close()")
        if self.raw + int(n) > self.max_raw:
            raise ValueError("push: %d + %d samples exceed the stream's capacity of %d (max_samples)"
                             % (self.raw, int(n), self.max_raw))

    def push(self, n):
        self.check_push(n)
        if self.resamples:
            self._raw += int(n)
        else:
            self.plan.push(n)

    def check_close(self):
        from .stream import check_closable
        check_closable(self.model_total(self.raw) if self.raw > 0 else 0, self.model_sr, self.plan.n_fft, self.plan.hop)

    def close(self):
        if self.closed:
            return
        self.check_close()
        if self.resamples:
            self._closed = True
        else:
            self.plan.close()

    @property
    def total(self):
        """Model-rate samples of the recording, once closed (None before)."""
        return self.model_total(self.raw) if self.closed else None

    def feed_due(self):
        """(first, count) of the model-rate samples to resample now (count 0: only the close is left to pass on), or
        None."""
        if not self.resamples or self.plan.closed:
            return None
        if self._closed:
            return self.fed_samples, self.total - self.fed_samples
        ready = min(resample_ready_open(self.in_sr, self.model_sr, self._raw, self.res_type), self.capacity)
        return (self.fed_samples, ready - self.fed_samples) if ready > self.fed_samples else None

    def fed(self, count):
        """`count` more model-rate samples are in the stream's buffer; -> True when they were the last of a closed
        recording: the caller then advances the `LivePlan` by `count` and closes it (`LiveStream.fed(count, last)`)."""
        self.fed_samples += int(count)
        if self._closed and self.fed_samples != self.total:
            raise ValueError("a closed recording is fed to its end")
        return self._closed

    def wire_due(self, chunks):
        """chunks: the (first, count) decoded so far, in order.  -> None, or (in_avail, in_total, out_first, out_count,
        final, pieces): the arguments of the ranged wire step that takes in every decoded chunk not wired yet, and the
        (a, b) of the piece each of them made final."""
        if self.wire_done or len(chunks) <= self.wired_chunks:
            return None
        final = self.plan.all_released                     # then the last decoded chunk is the recording's last
        in_avail = self.spf * (chunks[-1][0] + chunks[-1][1])  # the decoded frontier
        in_total = self.spf * self.plan.total if final else self.o_capacity
        pieces, a = [], self.out_done
        for i in range(self.wired_chunks, len(chunks)):
            first, count = chunks[i]
            if final and i == len(chunks) - 1:
                b = resample_ready(self.model_sr, self.rate, in_total, in_total, self.res_type)
            else:
                b = limiter_ready(self.model_sr, self.rate, self.spf * (first + count), self.o_capacity, self.lookahead,
                                  self.res_type)
            pieces.append((a, b))
            a = b
        return in_avail, in_total, self.out_done, a - self.out_done, final, pieces

    def wired(self, n_chunks, out_done, final):
        self.wired_chunks, self.out_done = int(n_chunks), int(out_done)
        if final:
            self.wire_done, self.valid = True, int(out_done)


class LiveWire(_WireOut):
    """One live voice conversion from raw samples to int16 (`convert_live_pcm16`): the live form of
    `convert_pcm16`.

    `push(raw)` appends 1-D int16 / fp32 samples at `in_sr` to a device buffer allocated once (no kernel).  `poll()`
    makes at most one `mbv_resample_ranges` launch, which writes the model-rate samples that have become final
    straight into `live.samples`, lets the `stream.LiveStream` it owns convert and decode, then wires what the decoded
    frontier made final in one ranged resample + int16 launch and returns `[(first_out_sample, view of pcm[0, a:b])]`.
    `close()` ends the recording: the model-rate total is ceil(n_raw * model_sr / in_sr), `net.resample`'s.

      pcm            int16 [1, ceil(capacity of live.o * rate / model_sr)]
      valid_samples  int64 [1] device, written with the last piece
      peak           fp32 [1] device, the running peak of the resampled output so far; the `peak=` and the `limiter=`
                     given when the stream was opened are inputs, as for `stream_pcm16`
      loudness       (opened with `loudness=`; else None) fp32 [1] device, the running integrated loudness of the
                     converted model-rate samples decoded so far, as on a `PcmStream`; after the last piece bitwise
                     `net.loudness` of the finished `live.o` over its 256 * frames samples
    With `in_sr == model_sr` the samples go to `LiveStream.push` as they are (int16 stays int16) and no input kernel
    runs.  `encoding` "ulaw" / "alaw": `pcm` is uint8 G.711 bytes (unwritten samples hold the code of zero).
    `in_encoding` "ulaw" / "alaw" with `dtype=torch.uint8`: `push` takes the caller's G.711 bytes, which the input
    kernel expands while it stages them (`in_sr` must differ from `model_sr`); DESIGN §7.15.  A `PcmPool` may feed, step and wire for many at once; pieces it wired are handed out by the next `poll()`
    without a launch, the same bytes either way."""

    def __init__(self, net, sid_src, sid_tgt, in_sr, model_sr, rate, hop_size, win_size, max_samples,
                 dtype=torch.int16, peak=None, res_type="kaiser_best", noise_scale=1.0, noise=None,
                 chunk_frames=32, max_chunk_frames=256, convert_frames=32, seed=None, limiter=None,
                 encoding="pcm16", in_encoding=None, loudness=None, envelope=None, pitch=None, ahead=None):
        from .stream import LiveStream
        _refuse_envelope(envelope, "convert_live_pcm16")
        _refuse_pitch(pitch, "convert_live_pcm16")
        _filter_code(res_type)
        loud = _loudness_arg(loudness, peak, "convert_live_pcm16", stream=True)
        lim = _limit_arg(limiter, rate)           # (refused here, before the `LiveStream` reserves anything)
        _law_code(encoding)
        self.in_encoding = _in_law(in_encoding, in_sr, model_sr, "convert_live_pcm16")
        if (dtype == torch.uint8) != (self.in_encoding is not None):
            raise TypeError("convert_live_pcm16: dtype=torch.uint8 and in_encoding='ulaw' | 'alaw' go together "
                            "(got dtype %s, in_encoding=%r)" % (dtype, in_encoding))
        if dtype not in (torch.float32, torch.int16, torch.uint8):
            raise TypeError("convert_live_pcm16: dtype must be int16 or float32, got %s" % dtype)
        self.in_sr, model_sr, rate = int(in_sr), int(model_sr), int(rate)
        if min(self.in_sr, model_sr, rate) <= 0:
            raise ValueError("sample rates must be positive")
        self.max_samples, self.dtype = int(max_samples), dtype
        if self.max_samples < 1:
            raise ValueError("convert_live_pcm16: max_samples must be >= 1")
        resamples = self.in_sr != model_sr
        if resamples:
            resample_ready_open(self.in_sr, model_sr, 0, res_type)           # refuses the rate pair before any buffer
        if rate != model_sr:
            resample_ready(model_sr, rate, 0, 1, res_type)
        cap = int(math.ceil(self.max_samples * (float(model_sr) / self.in_sr))) if resamples else self.max_samples
        self.live = LiveStream(net, sid_src, sid_tgt, model_sr, hop_size, win_size, cap,
                               dtype=torch.float32 if resamples else dtype, noise_scale=noise_scale, noise=noise,
                               chunk_frames=chunk_frames, max_chunk_frames=max_chunk_frames,
                               convert_frames=convert_frames, seed=seed, ahead=ahead)
        live = self.live
        self._plan = LiveWirePlan(self.in_sr, model_sr, rate, live.plan, live.spf, self.max_samples, res_type,
                                  lookahead=lim[1] if lim else 0)
        assert self._plan.o_capacity == live.o.shape[-1] and self._plan.capacity == live.max_samples
        dev = live.z.device
        super().__init__(net, dev, 1, self._plan.pcm_capacity, model_sr=model_sr, rate=rate, res_type=res_type,
                         encoding=encoding, peak=peak, limiter=limiter, loud=loud, capacity=self._plan.o_capacity,
                         silent=True)
        with torch.cuda.device(dev):
            # raw samples beyond the frontier are never read, so the buffer is not cleared
            self.raw = torch.empty(self.max_samples, device=dev, dtype=dtype) if resamples else None
            # valid input samples of the wire step: the capacity of o while the total is unknown
            self._valid_in = torch.full((1,), self._plan.o_capacity, device=dev, dtype=torch.int64)
        self._pieces = []             # (a, b) of every piece wired so far, in order
        self._handed = 0              # the piece poll() hands out next

    # ---- the recording
    @property
    def arrived(self):
        """Raw samples pushed so far."""
        return self._plan.raw

    @property
    def closed(self):
        return self._plan.closed

    @property
    def finished(self):
        return self._plan.wire_done and self._handed >= len(self._pieces)

    def push(self, samples):
        if self.raw is None:
            self.live.push(samples)                # equal rates: the stream's own push, unchanged
            return
        if not torch.is_tensor(samples):
            raise TypeError("push takes a 1-D tensor of %s samples" % self.dtype)
        if samples.dtype != self.dtype:
            raise TypeError("push: the stream was opened for %s samples, got %s" % (self.dtype, samples.dtype))
        if samples.dim() != 1:
            raise ValueError("push takes 1-D samples, got shape %s" % (tuple(samples.shape),))
        n, a = samples.numel(), self._plan.raw
        self._plan.check_push(n)
        if n:
            self.raw[a:a + n].copy_(samples)
            self._plan.push(n)

    def close(self):
        if self.raw is None:
            self.live.close()
        else:
            self._plan.close()

    # ---- what a pool shares (PcmPool.step); poll() is the stand-alone form of the same steps
    def _feed_row(self, row):
        """Fills `row` with the input range due now; -> its count, or None when nothing is due (a count of 0: only the
        close is left to pass on)."""
        due = self._plan.feed_due()
        if due is None:
            return None
        self.live.check_handle()
        p = self._plan
        row.wave, row.wave_dtype = self.raw.data_ptr(), _WAVE_DTYPE[self.in_encoding or self.dtype]
        row.in_avail, row.in_total = p.raw, p.raw if p.closed else -1
        row.out_first, row.out_count = due
        row.out, row.out_capacity = self.live.samples.data_ptr(), p.capacity
        return due[1]

    def _feed(self):
        rows = (_capi.MbvResampleRange * 1)()
        n = self._feed_row(rows[0])
        if n is None:
            return
        if n:
            self._net.resample_ranges(rows, self.in_sr, self.model_sr, self.res_type)
        self._fed(n)

    def _fed(self, n):
        self.live.fed(n, last=self._plan.fed(n))

    def _wire_due(self):
        """-> None, or ((the arguments of the wire step due now), pieces, final) from `LiveWirePlan.wire_due` of the
        chunks decoded so far; with the last chunk the valid input samples become 256 T, as `service_pcm16` counts them
        (a device fill)."""
        w = self._plan.wire_due(self.live.chunks)
        if w is None:
            return None
        self.live.check_handle()
        in_avail, in_total, out_first, out_count, final, pieces = w
        if final:
            with torch.cuda.device(self.pcm.device):
                self._valid_in.fill_(min(256 * self.live.frames, in_total))
        return (self.live.o[:, 0, :in_total], in_avail, out_first, out_count, final), pieces, final

    def _wire(self):
        w = self._wire_due()
        if w is not None:
            step, pieces, final = w
            self._wire_alone(*step)
            self._loudness_alone(step[0], step[1])
            self._chunk_wired(pieces, final)

    def poll(self):
        """-> [(first_out_sample, int16 view of pcm[0, a:b]), ...]: every piece not handed out yet, one per decoded
        chunk (an empty piece is possible while the chunk is shorter than the filter's lag)."""
        self._feed()
        self.live.poll()
        self._wire()
        out = [(a, self.pcm[0, a:b]) for a, b in self._pieces[self._handed:]]
        self._handed = len(self._pieces)
        return out

    # ---- the member of a pool (the protocol of `_WireOut`; `_feed_row` and `_fed` are the live members' own)
    _KIND = "live wire"

    _wired_out = property(lambda self: self._plan.wire_done)

    def _decode_streams(self):
        return [self.live]

    def _wire_chunk(self):
        w = self._wire_due()
        return None if w is None else self._due(self._wire_row(*w[0]), w[1], w[2], self._env)

    def _chunk_wired(self, pieces, final):
        self._pieces.extend(pieces)
        self._plan.wired(len(self.live.chunks), pieces[-1][1], final)


def convert_live_pcm16(net, sid_src, sid_tgt, in_sr, model_sr, rate, hop_size, win_size, max_samples,
                       dtype=torch.int16, peak=None, res_type="kaiser_best", noise_scale=1.0, noise=None,
                       chunk_frames=32, max_chunk_frames=256, convert_frames=32, seed=None, limiter=None,
                       encoding="pcm16", in_encoding=None, loudness=None, envelope=None, pitch=None, ahead=None):
    """The live form of `convert_pcm16`: raw samples in at `in_sr` (int16 or fp32; G.711 bytes with `dtype=torch.uint8,
    in_encoding="ulaw" | "alaw"`, which needs `in_sr != model_sr`) while the recording arrives, int16 out at `rate`
    (G.711 bytes with `encoding="ulaw" | "alaw"`); -> a `LiveWire`.  `max_samples` counts raw samples; `noise`, when given, is the block of the
    `LiveStream` it opens, [1, inter, frames of ceil(max_samples * model_sr / in_sr)].  `peak` and `limiter` as
    `stream_pcm16` takes them: the level of a live recording is whatever the microphone delivers, so there is no
    earlier utterance to take a peak from, and the limiter is the level control.  For a recording of more than 256 frames, `pcm` and `valid_samples` end bitwise as
    `stream_pcm16(net, convert_stream(whole, ..., in_sr=in_sr, noise=...), model_sr, rate, peak=peak).run()`.  `seed`
    (as `convert_live` takes it; excludes `noise`) fills that block from the seeded generator instead.  `loudness` as
    `stream_pcm16` takes it: `measured` is required with a target, and the wire keeps `.loudness`.  `envelope` is refused
    (ValueError): a converted recording has no tokens to take a volume from; `pitch` likewise (§7.22).
    `ahead` (a `stream.Ahead`) goes to the `LiveStream`'s plan: a bounded look-ahead of the conversion and
    the decoder, for a call that is live; it is not the limiter's `lookahead`, which delays the int16 pieces.  Then
    `pcm` ends bitwise as the wiring of the finished bounded `live.o`."""
    _refuse_envelope(envelope, "convert_live_pcm16")
    _refuse_pitch(pitch, "convert_live_pcm16")
    return LiveWire(net, sid_src, sid_tgt, in_sr, model_sr, rate, hop_size, win_size, max_samples, dtype=dtype,
                    peak=peak, res_type=res_type, noise_scale=noise_scale, noise=noise, chunk_frames=chunk_frames,
                    max_chunk_frames=max_chunk_frames, convert_frames=convert_frames, seed=seed, limiter=limiter,
                    encoding=encoding, in_encoding=in_encoding, loudness=loudness, ahead=ahead)


# ---- turns: several utterances as one gapless wire stream
def turn_ramp(ramp, n):
    """De-click samples at either end of a segment of `n` samples under a turn's ramp of `ramp`: min(ramp, n // 2), so
    that the two ramps of a segment never overlap."""
    return min(int(ramp), int(n) // 2)


def assemble_turn(waves, lengths, pauses, ramp):
    """The timeline of a turn written out as ONE fp32 row [1, 1, total], in torch and on the device of `waves[0]`: the
    one-shot form of what a `Turn` streams, and the row its bytes are defined by (`service_pcm16` of it, with the
    turn's `peak`, `limiter`, `encoding` and `fade`).
      waves    the segments' waveforms (`st.o` of each finished stream; any shape, read flat)
      lengths  valid samples n_s of each
      pauses   model-rate samples of silence in front of segments 1 .. S-1
      ramp     N, the de-click ramp in model-rate samples (round(ramp_ms * model_sr / 1000))
    Segment s starts at p_0 = 0, p_{s+1} = p_s + n_s + pauses[s]; with N_s = min(N, n_s // 2) its sample i is multiplied
    by (i + 1) * inv for i < N_s and by (N_s - (i - (n_s - N_s))) * inv for i >= n_s - N_s, inv = 1.0f / (N_s + 1) as
    `mbv_pcm_fade_make` gives it, in fp32 with one rounding each, and is copied anywhere else.  Exact in fp32, so it is
    bitwise the timeline `mbv_resample_turns` reads."""
    waves, lengths, pauses = list(waves), [int(n) for n in lengths], [int(p) for p in pauses]
    if not waves or len(lengths) != len(waves) or len(pauses) != len(waves) - 1:
        raise ValueError("assemble_turn: S >= 1 waves, S lengths and S - 1 pauses expected")
    if min(lengths) < 1 or (pauses and min(pauses) < 0) or int(ramp) < 0:
        raise ValueError("assemble_turn: lengths must be >= 1, pauses and ramp >= 0")
    dev = waves[0].device
    out = torch.zeros(1, 1, sum(lengths) + sum(pauses), device=dev, dtype=torch.float32)
    p = 0
    for s, (w, n) in enumerate(zip(waves, lengths)):
        if s:
            p += pauses[s - 1]
        seg = w.detach().reshape(-1)[:n].to(device=dev, dtype=torch.float32).clone()
        if seg.numel() != n:
            raise ValueError("assemble_turn: wave %d holds %d samples, fewer than its length %d" % (s, seg.numel(), n))
        k = turn_ramp(ramp, n)
        if k:
            inv = torch.tensor(_capi.pcm_fade(0, k).inv, device=dev, dtype=torch.float32)
            g = torch.arange(1, k + 1, device=dev, dtype=torch.float32) * inv
            seg[:k] *= g
            seg[n - k:] *= g.flip(0)
        out[0, 0, p:p + n] = seg
        p += n
    return out


def resample_geometry(orig_sr, target_sr, res_type="kaiser_best"):
    """(L, M, K, left) of the polyphase bank of a rate pair (`mbv_resample_bank`, host only): output t reads the inputs
    floor(t M / L) - left - 1 .. floor(t M / L) - left + K - 1.  Equal rates: (1, 1, 0, 0), the sample itself."""
    filt = _filter_code(res_type)
    orig_sr, target_sr = int(orig_sr), int(target_sr)
    if min(orig_sr, target_sr) <= 0:
        raise ValueError("sample rates must be positive")
    if orig_sr == target_sr:
        return 1, 1, 0, 0
    lib = _capi.lib()
    taps, left = C.c_int32(), C.c_int32()
    if lib.mbv_resample_bank(orig_sr, target_sr, filt, None, 0, None, C.byref(taps), C.byref(left)):
        msg = lib.mbv_last_error(None)
        raise _capi.MbvError(msg.decode() if msg else "mbv_resample_bank failed")
    g = math.gcd(orig_sr, target_sr)
    return target_sr // g, orig_sr // g, int(taps.value), int(left.value)


def turn_plan(orig_sr, target_sr, turns, res_type="kaiser_best", limits=None):
    """(total, packed_first) of `mbv_turn_plan` for `_capi.MbvTurnChunk`s (host only: no GPU needed, only the integer
    fields are read): the checks `resample_turns` makes on every turn and its segments, and where every turn starts in
    the packed buffer.  Raises `_capi.MbvError` naming the offending turn."""
    filt = _filter_code(res_type)
    if not isinstance(turns, C.Array):
        turns = (_capi.MbvTurnChunk * len(turns))(*turns)
    n = len(turns)
    lim = None
    if limits is not None and any(l is not None for l in limits):
        lim = (_capi.MbvPcmLimit * n)(*[_capi.MbvPcmLimit(*(l or (0.0, 0, 0))) for l in limits])
    first = (C.c_int64 * max(n, 1))()
    total = _ready_call("mbv_turn_plan", int(orig_sr), int(target_sr), filt, turns, lim, n, first)
    return total, list(first)[:n]


class TurnPlan:
    """What a turn may hand out as int16, in pure integers (no tensor, no GPU).

    A turn is a timeline at the model's rate: `append(n, pause)` puts a segment of n samples `pause` samples behind the
    end of the one before (the first at 0), `decoded(s, avail)` says how much of segment s exists, `close()` fixes the
    total at the end of the last segment.  `frontier()` is the contiguous decoded prefix: it runs through a finished
    segment, the pause behind it and the decoded part of the next one; while the turn is open it stops at the end of
    the last segment.  Wire sample u is final iff no tap of it lies at or past the frontier (`resample_ready_open`), or
    the turn is closed and wholly decoded; under a limiter u + `lookahead` must be final in that sense
    (`limiter_ready`).  `wire_due()` is the range that has become final since the last `wired()`; `segments_for` the
    segments its input window touches (with the limiter's halo of `lookahead + hold` outputs in front and `lookahead`
    behind).  The ranges are monotone and tile [0, total at the wire rate); they do not depend on what is appended
    later.  `cut_at(cut, keep)` is a revoke: nothing at or past wire sample `cut` is handed out, and the segments
    behind the first `keep` are dropped (the frontier never passes where they began)."""

    def __init__(self, model_sr, rate, max_samples, res_type="kaiser_best", lookahead=0, hold=0):
        self.model_sr, self.rate, self.res_type = int(model_sr), int(rate), res_type
        self.lookahead, self.hold = int(lookahead), int(hold)
        if not 0 <= self.lookahead <= Limiter.MAX_LOOKAHEAD or not 0 <= self.hold <= Limiter.MAX_HOLD:
            raise ValueError("limiter lookahead must be in [0, %d] and hold in [0, %d] output samples"
                             % (Limiter.MAX_LOOKAHEAD, Limiter.MAX_HOLD))
        self.max_samples = int(max_samples)
        if self.max_samples < 1:
            raise ValueError("max_samples must be >= 1")
        self.L, self.M, self.K, self.left = resample_geometry(model_sr, rate, res_type)   # refuses the rate pair here
        # model-rate samples that stand in for the total while the turn is open: int(capacity * ratio) >= max_samples,
        # and no timeline that fits max_samples reaches it
        self.capacity = int(math.ceil(self.max_samples * (float(self.model_sr) / self.rate))) + 1
        self.starts, self.lengths, self.avail = [], [], []
        self.closed = False
        self.out_done = 0             # wire samples [0, out_done) are final and handed out
        self.cut = None               # the length a revoke left
        self._fence = None            # where the first dropped segment began

    @property
    def end(self):
        """The end of the last segment: the timeline's total once closed."""
        return self.starts[-1] + self.lengths[-1] if self.starts else 0

    @property
    def total(self):
        return self.end if self.closed else None

    def out_total(self, n=None):
        """Wire samples of a timeline of n model-rate samples (default: this one's, as it stands)."""
        n = self.end if n is None else int(n)
        return resample_ready(self.model_sr, self.rate, n, n, self.res_type)

    def check_append(self, n, pause=0):
        """-> the start of a segment of n samples appended `pause` behind the last; ValueError when refused."""
        n, pause = int(n), int(pause)
        if self.closed:
            raise ValueError("append after close()")
        if n < 1 or pause < 0:
            raise ValueError("append: a segment has n >= 1 samples and a pause >= 0")
        if not self.starts and pause:
            raise ValueError("append: the first segment starts the turn (pause %d must be 0)" % pause)
        p = self.end + pause
        if self.out_total(p + n) > self.max_samples:
            raise ValueError("append: %d + %d + %d model-rate samples are %d wire samples, beyond the turn's capacity of "
                             "%d (max_samples)" % (self.end, pause, n, self.out_total(p + n), self.max_samples))
        return p

    def append(self, n, pause=0):
        p = self.check_append(n, pause)
        self.starts.append(p)
        self.lengths.append(int(n))
        self.avail.append(0)
        return len(self.starts) - 1

    def decoded(self, s, avail):
        self.avail[s] = max(self.avail[s], min(int(avail), self.lengths[s]))

    def close(self):
        self.closed = True

    @property
    def complete(self):
        """Closed, and every segment wholly decoded."""
        return self.closed and self._fence is None and self.avail == self.lengths

    def frontier(self):
        f = self.end
        for p, n, a in zip(self.starts, self.lengths, self.avail):
            if a < n:
                f = p + a
                break
        return f if self._fence is None else min(f, self._fence)

    def in_total(self):
        """`in_total` of the wire step: the total, or the capacity that stands in for it while the turn is open."""
        return self.end if self.closed else self.capacity

    def ready(self):
        f = self.frontier()
        if self.closed:
            r = limiter_ready(self.model_sr, self.rate, f, self.end, self.lookahead, self.res_type)
        else:
            r = min(limiter_ready(self.model_sr, self.rate, f, None, self.lookahead, self.res_type), self.max_samples)
        return r if self.cut is None else min(r, self.cut)

    @property
    def done(self):
        """Every final sample is handed out: the turn is closed and either complete or wired up to a revoke's cut."""
        if not self.closed:
            return False
        if self.cut is not None:
            return self.out_done >= self.cut
        return self.complete and self.out_done >= self.out_total()

    def wire_due(self):
        """-> None, or (out_first, out_count): the wire samples that have become final since the last `wired()`."""
        b = self.ready()
        return (self.out_done, b - self.out_done) if b > self.out_done else None

    def wired(self, out_done):
        self.out_done = int(out_done)

    def window(self, out_first, out_count):
        """[lo, hi): the timeline samples the taps of outputs [out_first, out_first + out_count) touch, the limiter's
        halo included."""
        a = max(int(out_first) - self.lookahead - self.hold, 0)
        b = int(out_first) + int(out_count) + self.lookahead
        if self.K == 0:
            return a, b
        return (a * self.M) // self.L - self.left - 1, ((b - 1) * self.M) // self.L - self.left + self.K

    def segments_for(self, out_first, out_count):
        """-> (s0, s1): segments [s0, s1) intersect the window of the range (s0 == s1: none does)."""
        if int(out_count) <= 0:
            return 0, 0
        lo, hi = self.window(out_first, out_count)
        hit = [s for s, (p, n) in enumerate(zip(self.starts, self.lengths)) if p < hi and p + n > lo]
        return (hit[0], hit[-1] + 1) if hit else (0, 0)

    def revoke_events(self, avails):
        """The turn's readiness after every chunk of every segment, in timeline order, were it closed now: what
        `revoke_plan` takes as `ready`.  avails[s] lists the model-rate samples of segment s that exist after each of
        its chunks (ascending; the last is the whole segment).  -> [(s, i, ready), ...]; after a segment's last chunk
        the frontier stands at the next segment's start (the end of the turn behind the last one)."""
        end, out = self.end, []
        for s, each in enumerate(avails):
            for i, a in enumerate(each):
                if i + 1 < len(each):
                    f = self.starts[s] + min(int(a), self.lengths[s])
                else:
                    f = self.starts[s + 1] if s + 1 < len(self.starts) else end
                out.append((s, i, limiter_ready(self.model_sr, self.rate, f, end, self.lookahead, self.res_type)))
        return out

    def cut_at(self, cut, keep):
        self.closed = True
        self.cut = int(cut)
        if keep < len(self.starts):
            self._fence = self.starts[keep]


def _segment_length(st):
    """Valid model-rate samples of a single-utterance stream, on the host: what `PcmStream` takes as its valid input
    (the warped length of a pitched stream)."""
    if st.warp is not None:
        return st.warp.n_out
    n = st.o.shape[-1]
    return n if st.y_lengths is None else min(256 * st.z.shape[2], n)


class Turn(_WireOut):
    """Several utterances as ONE gapless wire stream (`PcmPool.add_turn`): the phrases of a dialogue turn,
    appended while earlier ones play, resampled, limited and framed as one continuous piece of audio.

    The segments are ordinary single-utterance `DecodeStream`s in the pool's `StreamPool`, untouched: each `st.o` is
    bitwise its stand-alone decode.  The turn's input is their timeline (`TurnPlan`, `assemble_turn`), read in place by
    `mbv_resample_turns`; `PcmPool.step()` wires every turn with something due in ONE such call and returns
    `(turn, first, piece)` entries.  The concatenated pieces are bitwise `service_pcm16` of `assemble_turn` of the
    finished waveforms with the turn's `peak`, `limiter` and `encoding` (and `fade`, once revoked), however the turn
    was appended to, ticked or pooled.
      pcm            int16 (uint8 under G.711) [1, max_samples]; unwritten samples hold silence
      valid_samples  int64 [1] device, written when the turn is closed and its last piece is wired
      peak           fp32 [1] device, the running peak of the resampled samples handed out so far
      marks          one entry per segment: the wire sample at which each of its tokens starts (the segment's offset and
                     the limiter's lag included), or None for a segment without marks
      finished       every final sample has been handed out
    The ramp of `ramp_ms` (5 ms by default: a convention like the fade's, not a measurement) scales both ends of every
    segment, so a joint never depends on what is appended later."""

    def __init__(self, pool, max_samples, peak=None, limiter=None, loudness=None, ramp_ms=5.0):
        self._pool, net = pool, pool._net
        lim = _limit_arg(limiter, pool.rate)
        loud = _loudness_arg(loudness, peak, "PcmPool.add_turn", stream=True)
        if loud is not None and loud.target is None:
            raise ValueError("PcmPool.add_turn: a turn keeps no running loudness; loudness= takes Loudness(measured=...) "
                             "for the static gain only")
        if not float(ramp_ms) >= 0.0:
            raise ValueError("PcmPool.add_turn: ramp_ms must be >= 0")
        self.ramp_ms, self.ramp = float(ramp_ms), int(round(float(ramp_ms) * 1e-3 * pool.model_sr))
        self._plan = TurnPlan(pool.model_sr, pool.rate, max_samples, pool.res_type,
                              lookahead=lim[1] if lim else 0, hold=lim[2] if lim else 0)
        self._h = net._ensure_handle()
        super().__init__(net, net._device(), 1, self._plan.max_samples, model_sr=pool.model_sr, rate=pool.rate,
                         res_type=pool.res_type, encoding=pool.encoding, peak=peak, limiter=limiter, loud=loud,
                         capacity=None, silent=True)
        self.segments = []            # the `DecodeStream`s, in timeline order
        self.envelopes = []           # per segment: its `Envelope` (per-token volume) or None
        self.warped = []              # per segment: the `_Warped` row of a pitched stream or None
        self.marks = []
        self._valid_set = False

    # ---- where it stands
    @property
    def closed(self):
        return self._plan.closed

    @property
    def finished(self):
        return self._plan.done

    @property
    def revoked(self):
        return self._revoked is not None

    def _pause(self, pause_ms):
        if not float(pause_ms) >= 0.0:
            raise ValueError("append: pause_ms must be >= 0")
        return int(round(float(pause_ms) * 1e-3 * self.model_sr))

    def _check_segment(self, st):
        from .stream import DecodeStream, LiveStream
        pool = self._pool
        if isinstance(st, LiveStream):
            raise ValueError("Turn.append: a LiveStream is not a segment of a turn (its length is not known)")
        if not isinstance(st, DecodeStream):
            raise ValueError("Turn.append takes a DecodeStream (net.infer_stream / StreamPool.admit)")
        if st._net is not self._net or st._h is not self._h or self._net._handle is not self._h:
            raise ValueError("Turn.append: the stream belongs to another model or handle")
        if st.z.shape[0] != 1:
            raise ValueError("Turn.append takes a stream of ONE utterance (this one has %d rows)" % st.z.shape[0])
        if pool.follower(st) is not None:
            raise ValueError("Turn.append: the stream is a plain member of the pool (PcmPool.add): it has its own wire stream")
        if any(st is m for t in pool.turns for m in t.segments) or any(st is m for m in self.segments):
            raise ValueError("Turn.append: the stream is a segment of a turn already")

    def append(self, st, pause_ms=0.0, envelope=None):
        """Appends the single-utterance `DecodeStream` `st` (a member of the pool's `StreamPool`; it joins it otherwise)
        `pause_ms` of silence behind the last segment; -> its index.  `envelope`: None, or a one-row `Envelope` over the
        segment's own samples (None on a stream made with `gain=` takes its `frame_gain`): per-token volume, applied
        before the segment's de-click ramp.  The first segment starts the turn (p_0 = 0): it
        takes no pause.  ValueError, with nothing changed: a `LiveStream`, a plain member of this pool, a segment of a
        turn, a stream of another model or handle, a turn that would pass `max_samples`, a closed turn, a non-zero
        `pause_ms` on the first segment (silence in front of a turn is the caller's to send, not part of it)."""
        self._check_segment(st)
        n = _segment_length(st)
        env = _envelope_arg(envelope, st, "Turn.append")
        if env is not None:
            env.check("Turn.append", 1, st.o.shape[-1] if st.warp is not None else n, st.o.device)
        self._plan.check_append(n, self._pause(pause_ms))
        if not st._drained():
            self._pool.pool.add(st)                   # (refuses another device; a member stays one)
        # a pitched segment is its warped row, which the turn owns, with the warped length and frontier; its envelope
        # is handed to the warp, where the samples are read
        wp = _Warped(self._net, st, env, self.res_type) if st.warp is not None else None
        s = self._plan.append(n, self._pause(pause_ms))
        self.segments.append(st)
        self.envelopes.append(env if wp is None else None)
        self.warped.append(wp)
        lag = self._lim[1] if self._lim else 0
        marks = st.marks
        at = None if marks is None else ([st.spf * int(f) for f in marks] if wp is None
                                         else wp.map.samples_of_frames(marks))
        self.marks.append(None if marks is None else mark_samples(
            [self._plan.starts[s] + a for a in at], 1, self.model_sr, self.rate, lag))
        return s

    def admit(self, requests, pauses_ms=None):
        """`StreamPool.admit(requests)` followed by `append` in order (`pauses_ms`: None, or one per request); -> the
        streams.  All or nothing: when a request is refused, the turn would pass `max_samples` or the first segment of
        the turn is given a non-zero pause (as `append` refuses it), no stream stays in the pool and the turn is
        unchanged."""
        reqs = list(requests)
        pauses = [0.0] * len(reqs) if pauses_ms is None else list(pauses_ms)
        if len(pauses) != len(reqs):
            raise ValueError("admit: one pause per request expected (%d), got %d" % (len(reqs), len(pauses)))
        if self.closed:
            raise ValueError("append after close()")
        steps = [self._pause(p) for p in pauses]
        sts = self._pool.pool.admit(reqs)
        try:
            trial = TurnPlan(self.model_sr, self.rate, self._plan.max_samples, self.res_type)
            trial.starts, trial.lengths = list(self._plan.starts), list(self._plan.lengths)
            for st, p in zip(sts, steps):
                self._check_segment(st)
                trial.starts.append(trial.check_append(_segment_length(st), p))
                trial.lengths.append(_segment_length(st))
        except ValueError:
            for st in sts:
                if any(st is m for m in self._pool.pool.streams):
                    self._pool.pool.remove(st)
            raise
        for st, p in zip(sts, pauses):
            self.append(st, p)
        return sts

    def close(self):
        """No segment follows: the timeline's total is the end of the last one, and the turn finishes with the piece
        that flushes the filter's lag."""
        self._plan.close()
        self._settle()
        self._pool._drop_finished()               # (a turn that this finished leaves at once, as before)

    # ---- the member of a pool (the protocol of `_WireOut`)
    _KIND, _TURNS = "turn", True
    _wired_out = finished

    def _decode_streams(self):
        return self.segments

    def _wire_chunk(self):
        plan = self._plan
        for s, st in enumerate(self.segments):
            plan.decoded(s, self._seg_frontier(s, _decoded_samples(st)))
        due = plan.wire_due()
        if due is None:
            return None
        self._check_handle("this turn")
        a, count = due
        k = _capi.MbvTurnChunk()
        c = k.chunk
        c.wave, c.in_total, c.valid_samples, c.in_avail = None, plan.in_total(), None, plan.frontier()
        c.out_first, c.out_count = a, count
        c.peak = self._peak_in.data_ptr() if self._peak_in is not None else None
        c.pcm, c.pcm_capacity = self.pcm.data_ptr(), self.pcm.shape[1]
        c.running_peak, c.out_samples = self.peak.data_ptr(), None
        s0, s1 = plan.segments_for(a, count)
        segs = (_capi.MbvTurnSeg * max(s1 - s0, 1))()
        for sg, s in zip(segs, range(s0, s1)):
            wave = self.segments[s].o if self.warped[s] is None else self.warped[s].row
            sg.wave, sg.start, sg.length = wave.data_ptr(), plan.starts[s], plan.lengths[s]
            sg.ramp = turn_ramp(self.ramp, plan.lengths[s])
        k.segs, k.n_segs = segs, s1 - s0
        return self._due(k, [(a, a + count)], None, self.envelopes[s0:s1])

    def _chunk_wired(self, pieces, final):
        self._plan.wired(pieces[-1][1])
        self._settle()

    def _seg_frontier(self, s, model_avail):
        """samples of segment s that exist once `model_avail` of its decoded samples do"""
        return model_avail if self.warped[s] is None else self.warped[s].frontier(model_avail)

    def _warp_dues(self):
        dues = []
        for st, wp in zip(self.segments, self.warped):
            due = wp.due(_decoded_samples(st)) if wp is not None else None
            if due:
                dues.append((wp, due))
        return dues

    def _settle(self):
        """Once the last piece is out: `valid_samples` (a device fill of a host integer), the segments still in the
        `StreamPool` leave it.  (Leaving the `PcmPool` is the pool's: `step`, or `close` / `revoke` asking it.)"""
        plan = self._plan
        if not plan.done or self._valid_set:
            return
        self._valid_set = True
        with torch.cuda.device(self.pcm.device):
            self.valid_samples.fill_(plan.out_total() if plan.cut is None else plan.cut)
        for st in self.segments:
            if any(st is m for m in self._pool.pool.streams):
                self._pool.pool.remove(st)

    # ---- barge-in
    def _started(self, first):
        if any(m is None for m in self.marks):
            return None
        return sum(1 for ms in self.marks for m in ms[:-1] if m < first)

    def revoke(self, fade_ms=5.0, at="now"):
        """Takes the turn back (barge-in, DESIGN §7.16 over a turn): what has been handed out stays, the rest fades to
        silence over N = round(fade_ms * rate / 1000) samples from F (`at="now"`: the samples handed out so far; an int:
        that wire sample) and the turn, closed by this, ends at min(its length, F + N) (`valid_samples`).  The segment
        the cut falls in decodes up to the first chunk that makes F + N outputs final (`revoke_plan` over the turn's
        readiness), the segments behind it leave the `StreamPool` undecoded.  The bytes are bitwise
        `service_pcm16(assemble_turn(...), fade=(F, N))`.  -> a `Revoked`; `tokens_started` counts over all segments'
        marks (None when a segment has none).  Revoking a finished or revoked turn changes nothing."""
        plan = self._plan
        total, E = plan.out_total(), plan.out_done
        report, fade = self._revoke_begin(fade_ms, at, E, total, tokens=False)
        if fade is None:
            return report
        events = plan.revoke_events([[self._seg_frontier(s, _decoded_samples(st, i)) for i in range(len(st.schedule))]
                                     for s, st in enumerate(self.segments)]) or [(0, 0, 0)]
        cut, last, _ = revoke_plan([r for _, _, r in events], total, E, *fade)  # (refuses F < E before anything changes)
        s_cut, i_cut, _ = events[last]
        for s, st in enumerate(self.segments):
            if s == s_cut:
                st._truncate(max(i_cut + 1, st._decoded))
            elif s > s_cut and any(st is m for m in self._pool.pool.streams):
                self._pool.pool.remove(st)
        keep = s_cut + 1 if self.segments else 0
        whole = last == len(events) - 1                       # the cut needs the whole turn: nothing is dropped
        plan.cut_at(cut, len(self.segments) if whole else keep)
        if not whole:
            self.segments = self.segments[:keep]              # (`marks` keeps every segment's: the report counts over all)
            self.envelopes = self.envelopes[:keep]
            self.warped = self.warped[:keep]
        report = self._revoke_end(*fade, cut, total)
        self._settle()
        self._pool._drop_finished()
        return report


class PcmPool:
    """The wire output of many `DecodeStream`s of one model: `step()` steps the wrapped `stream.StreamPool` (one
    `mbv_decode_chunks` call) and then turns what has become final on ALL pooled streams into int16 in ONE
    `mbv_resample_pcm16_chunks` launch, instead of one `mbv_resample_pcm16_range` launch per stream.

    `add(st, peak=None, limiter=None)` returns the stream's `PcmStream` follower, which holds the state it holds alone (`pcm`,
    `valid_samples`, `peak`); the pieces count as wired ahead on it, so `next(follower)` afterwards hands them out
    without a launch.  A stream may be driven through the pool, alone, or both in turn: the same bytes, those
    `service_pcm16` gives for the finished waveform.  Finished streams drop out.  Members with a `Limiter` (each its
    own) share one launch of the limited kernel and the others one of the unlimited: two launches in a mixed tick.
    One `encoding` per pool, like `rate` and `res_type`: with "ulaw" / "alaw" the followers' `pcm`, the packed buffer
    and the pinned host buffer are uint8 (`mbv_resample_g711_chunks`), at the same launch counts.
    `revoke(st)` takes a member back: its fade rides in the tick's launch and it leaves when the fade is out.
    Members added with `loudness=` keep their running `.loudness`: ONE `mbv_loudness_chunks` launch per tick measures
    the segments completed on all of them; a tick in which none completed one, and a pool without such members,
    launches nothing for it.
    `add_turn(max_samples, ...)` opens a `Turn`: several utterances as one gapless wire stream, wired by `step()` in
    ONE `mbv_resample_turns` call per tick for all turns of the pool."""

    def __init__(self, net, pool, model_sr, rate, res_type="kaiser_best", encoding="pcm16"):
        _filter_code(res_type)
        self.encoding, self._dtype = encoding, _wire_dtype(encoding)
        if pool._net is not net:
            raise ValueError("the stream pool belongs to another model")
        self._net, self.pool = net, pool
        self.model_sr, self.rate, self.res_type = int(model_sr), int(rate), res_type
        self._members = []                        # every `PcmStream`, `LiveWire` and `Turn` of the pool, in the order added
        self._packed = None                       # device, the call's pieces back to back (host=True)
        self._host = self._host_np = None         # its pinned host copy, and that as a NumPy array
        self._event = None

    def __len__(self):
        return len(self._members)

    # views: the followers of `add`, the `LiveWire`s of `add_live`, the `Turn`s of `add_turn`, each in the order added
    followers = property(lambda self: [m for m in self._members if m._KIND == "stream"])
    lives = property(lambda self: [m for m in self._members if m._KIND == "live wire"])
    turns = property(lambda self: [m for m in self._members if m._KIND == "turn"])

    def _drop_finished(self):
        """The one leave rule: a member with nothing more to wire leaves the pool."""
        self._members = [m for m in self._members if not m._wired_out]

    def follower(self, st):
        return next((f for f in self.followers if f._st is st), None)

    def add(self, st, peak=None, limiter=None, loudness=None, envelope=None):
        """-> the stream's `PcmStream` follower.  `envelope`: per-token volume as `stream_pcm16` takes it; a stream made
        with `gain=` brings its own."""
        _refuse_live(st)
        if any(st is m for t in self.turns for m in t.segments):
            raise ValueError("PcmPool.add: the stream is a segment of a turn of this pool: the turn is its wire stream")
        _limit_arg(limiter, self.rate)            # refuses bad parameters before the stream joins the pool
        _loudness_arg(loudness, peak, "PcmPool.add", stream=True)
        self.pool.add(st)                         # (refuses B > 1, another model, another device)
        f = self.follower(st)
        if f is None:
            f = PcmStream(self._net, st, self.model_sr, self.rate, peak=peak, res_type=self.res_type, limiter=limiter,
                          encoding=self.encoding, loudness=loudness, envelope=envelope)
            self._members.append(f)
        return f

    def admit(self, requests, peak=None, limiter=None, loudness=None):
        """`StreamPool.admit(requests)` + a follower for each new stream (`peak`: None, one value for all, or one per
        request, as `add` takes it; `limiter` and `loudness` likewise); -> the followers, in order.  `requests` is all `models.Request` or all
        `models.ConvertRequest` (audio), as `StreamPool.admit` takes them.  All or nothing, like `StreamPool.admit`."""
        reqs = list(requests)
        peaks = _per_request("admit", "peak", peak, len(reqs))
        limiters = _per_request("admit", "limiter", limiter, len(reqs))
        for lim in limiters:
            _limit_arg(lim, self.rate)
        louds = _per_request("admit", "loudness", loudness, len(reqs))
        for p, loud in zip(peaks, louds):
            _loudness_arg(loud, p, "PcmPool.admit", stream=True)
        return [self.add(st, peak=p, limiter=lim, loudness=loud)
                for st, p, lim, loud in zip(self.pool.admit(reqs), peaks, limiters, louds)]

    def revoke(self, st, fade_ms=5.0, at="now"):
        """`PcmStream.revoke` for a member added with `add` or `admit` (a text request or a converted recording; `st`
        is the decode stream or its follower): the fade rides in the pool's one wire launch per tick, the member's
        later chunks are never decoded, and it leaves this pool and the wrapped `StreamPool` when the fade is out
        (at once, when nothing is left to wire).  -> the `Revoked` report.  A live member is not revoked (ValueError,
        nothing launched): a caller who hangs up stops pushing and drops the wire.  The 5 ms default is a convention,
        not a measurement."""
        if isinstance(st, LiveWire) or any(st is lw.live for lw in self.lives):
            raise ValueError("PcmPool.revoke: a live member is not revoked (stop pushing and drop the LiveWire)")
        f = st if isinstance(st, PcmStream) else self.follower(st)
        if f is None or not any(f is m for m in self.followers):
            raise ValueError("PcmPool.revoke names a stream that is not in the pool")
        report = f.revoke(fade_ms=fade_ms, at=at)
        if f.finished and any(f._st is m for m in self.pool.streams):
            self.pool.remove(f._st)
        self._drop_finished()
        return report

    def add_live(self, lw, limiter=None, loudness=None, envelope=None, pitch=None):
        """Adds a `LiveWire` (`convert_live_pcm16`): its `LiveStream` joins the wrapped `StreamPool`, and `step()` then
        feeds, steps and wires it along with the others; -> `lw`.  The wire keeps the limiter it was opened with;
        `limiter`, when given, must be that one (the lag is part of the pieces it has planned); `loudness` likewise
        (its state is the wire's)."""
        _refuse_envelope(envelope, "add_live")
        _refuse_pitch(pitch, "add_live")
        if not isinstance(lw, LiveWire):
            raise TypeError("add_live takes a wire.LiveWire (wire.convert_live_pcm16)")
        if limiter is not None and limiter != lw.limiter:
            raise ValueError("add_live: the live wire was opened with %r, not %r" % (lw.limiter, limiter))
        if loudness is not None and loudness is not lw._loud:
            raise ValueError("add_live: the live wire was opened with %r, not %r" % (lw._loud, loudness))
        if (lw.model_sr, lw.rate) != (self.model_sr, self.rate):
            raise ValueError("the live wire runs %d -> %d Hz, the pool %d -> %d Hz"
                             % (lw.model_sr, lw.rate, self.model_sr, self.rate))
        if lw.res_type != self.res_type:
            raise ValueError("the live wire resamples with %r, the pool with %r" % (lw.res_type, self.res_type))
        if lw.encoding != self.encoding:
            raise ValueError("the live wire was opened with encoding %r, the pool with %r" % (lw.encoding, self.encoding))
        self.pool.add(lw.live)                    # (refuses another model, another device)
        if not any(lw is m for m in self._members):
            self._members.append(lw)
        return lw

    def add_turn(self, max_samples, peak=None, limiter=None, loudness=None, ramp_ms=5.0):
        """Opens a `Turn`: several utterances as one gapless wire stream at the pool's rates, filter and
        encoding; -> the turn.  `max_samples` is its capacity in WIRE samples (only that int16 row is reserved; no
        model-rate memory is).  `peak`, `limiter` and `loudness` as `add` takes them, for the whole turn; `loudness`
        takes `Loudness(measured=...)` for the static gain only (a turn keeps no running `.loudness`).  `ramp_ms`: the
        de-click ramp at both ends of every segment (5 ms: a convention, not a measurement; 0: none).  `step()` then
        wires the turn along with the other members, ONE `mbv_resample_turns` call per tick for all turns, and
        `step(streams=[turn])` names it."""
        t = Turn(self, max_samples, peak=peak, limiter=limiter, loudness=loudness, ramp_ms=ramp_ms)
        self._members.append(t)
        return t

    def _feed_lives(self, lives):
        """The input ranges due on all live members in one `mbv_resample_ranges` launch (one per raw rate among them)."""
        by_sr = {}
        for lw in lives:
            row = _capi.MbvResampleRange()
            n = lw._feed_row(row)
            if n is not None:
                by_sr.setdefault(lw.in_sr, []).append((lw, row, n))
        for in_sr, todo in by_sr.items():
            rows = (_capi.MbvResampleRange * len(todo))(*[row for _, row, _ in todo])
            if any(n for _, _, n in todo):
                self._net.resample_ranges(rows, in_sr, self.model_sr, self.res_type)
            for lw, _, n in todo:
                lw._fed(n)

    def step(self, streams=None, host=False):
        """-> [(st, first_out_sample, piece), ...]: one entry per stream whose decoded frontier made outputs final
        (an empty piece is possible, as for `PcmStream`); for a live member `st` is its `LiveWire`, one entry per
        decoded chunk.  `piece` is the 1-D view `follower.pcm[0, a:b]` on the device, ordered on the current stream;
        with host=True it is a NumPy int16 (uint8 in a G.711 pool) view of ONE pinned buffer that one copy and one event wait filled, valid
        until the next `step(host=True)`.  Live members first resample what has arrived in ONE `mbv_resample_ranges`
        launch; `streams` may name them by their `LiveWire`.  A `Turn` (`add_turn`) with something due gives one
        `(turn, first, piece)` entry; all turns of a tick share ONE `mbv_resample_turns` call, their pieces lie behind
        the members' in the pinned buffer, and `streams` may name a turn (its segments are then stepped)."""
        net = self._net
        members = list(self._members) if streams is None else [self._named(st) for st in streams]
        members = [m for kind in _KINDS for m in members if m._KIND == kind]      # the order of `out`
        self._feed_lives([m for m in members if m._KIND == "live wire"])
        named = None
        if streams is not None:
            named = [st for m in members for st in m._decode_streams() if not st._drained()]
        if named is None or named:
            self.pool.step(named)
        # the pitched followers and turn segments of the tick: ONE mbv_warp_ranges launch in front of the wire launches
        _warp_launch(net, [d for m in members for d in m._warp_dues()])
        # (member, the `_Due` of its wire step) per member with one
        rows = [(m, due) for m in members if (due := m._wire_chunk()) is not None]
        out = []
        if rows:
            chunk_rows = [due for m, due in rows if not m._TURNS]         # the two tables; in `rows` the turns' come last
            turn_rows = [due for m, due in rows if m._TURNS]
            arr = (_capi.MbvPcmChunk * len(chunk_rows))(*[d.k for d in chunk_rows])
            tarr = (_capi.MbvTurnChunk * len(turn_rows))(*[d.k for d in turn_rows])
            tlimits = [d.lim for d in turn_rows]
            dev = net._device()
            packed, offs = None, [None] * len(rows)
            if host:
                total, offs = pcm_chunks_plan(self.model_sr, self.rate, arr, self.res_type)
                first_turn = total
                t_total, toffs = turn_plan(self.model_sr, self.rate, tarr, self.res_type, tlimits) if turn_rows else (0, [])
                total += t_total                  # the turns' pieces lie behind the members' in the one buffer
                offs = offs + [first_turn + o for o in toffs]
                if self._packed is None or self._packed.shape[0] < total:
                    cap = max(2 * total, 1 << 16)
                    self._packed = torch.empty(cap, device=dev, dtype=self._dtype)
                    self._host = torch.empty(cap, dtype=self._dtype, pin_memory=True)
                    self._host_np = self._host.numpy()
                    self._event = torch.cuda.Event()
                packed = self._packed
            if chunk_rows:                        # every chunk row of the tick in ONE call (two launches when some are limited)
                net.resample_pcm16_chunks(arr, self.model_sr, self.rate, packed=packed, res_type=self.res_type,
                                          limits=[d.lim for d in chunk_rows], encoding=self.encoding,
                                          fades=[d.fade for d in chunk_rows], envelopes=[d.env for d in chunk_rows])
            if turn_rows:                         # every turn of the tick in ONE call
                net.resample_turns(tarr, self.model_sr, self.rate, packed=packed[first_turn:] if host else None,
                                   res_type=self.res_type, limits=tlimits, encoding=self.encoding,
                                   fades=[d.fade for d in turn_rows], envelopes=[d.env for d in turn_rows])
            # the measuring members of the tick: the segments their frontier completed, in ONE launch
            measuring = [(m, lk) for m, due in rows if (lk := m._measure_row(due.k)) is not None]
            if measuring:
                net.loudness_chunks([lk for _, lk in measuring], self.model_sr)
                for m, lk in measuring:
                    m._lseg = lk.seg_first + lk.seg_count
            for m, due in rows:
                m._chunk_wired(due.pieces, due.final)
            if host and total:
                with torch.cuda.device(dev):
                    self._host[:total].copy_(packed[:total], non_blocking=True)
                    self._event.record(torch.cuda.current_stream(dev))
                    self._event.synchronize()
            for (m, due), o in zip(rows, offs):   # a piece lies in the member's row, or in the pinned buffer from `o` on
                first = due.pieces[0][0]
                out += [(m._name, a, self._host_np[o + a - first:o + b - first] if host else m.pcm[0, a:b])
                        for a, b in due.pieces]
        self._drop_finished()
        return out

    def _named(self, st):
        """The member that `step(streams=)` names by `st`: a decode stream, a `LiveWire` or a `Turn` of this pool."""
        for m in self._members:
            if m._name is st:
                return m
        raise ValueError("step(streams=...) names a %s that is not in the pool"
                         % (st._KIND if isinstance(st, _WireOut) else "stream"))


def pcm_pool(net, pool, model_sr, rate, res_type="kaiser_best", encoding="pcm16"):
    """The pooled `stream_pcm16`: a `PcmPool` over a `stream.StreamPool` (`net.stream_pool()`) of the same model.
    `add(st, peak=None, limiter=None, loudness=None)` takes `peak`, `limiter` and `loudness` as `stream_pcm16` does;
    `encoding` is the pool's."""
    return PcmPool(net, pool, model_sr, rate, res_type=res_type, encoding=encoding)


class FrameCutter:
    """`frame_pcm16` for an int16 stream that arrives in pieces: `push` returns the whole frames of
    `chunk_size(rate, frame_length)` samples that are complete, as base64 text, and carries the remainder;
    `close` returns the short last frame, if any.  The frames of all calls are those of `frame_pcm16` on the
    concatenation.  `sample_bytes=1`: a G.711 stream, uint8 pieces, frames of that many BYTES (`frame_g711`)."""

    def __init__(self, rate, frame_length=0.02, sample_bytes=2):
        if sample_bytes not in (1, 2):
            raise ValueError("sample_bytes must be 2 (int16) or 1 (G.711 bytes), got %r" % (sample_bytes,))
        self.n = chunk_size(rate, frame_length)
        if self.n <= 0:
            raise ValueError("frame_length * rate must be at least one sample")
        self.sample_bytes = sample_bytes
        self._wire = np.dtype("<i2" if sample_bytes == 2 else "u1")
        self._rest = np.zeros(0, self._wire)

    def push(self, pcm):
        """pcm: 1-D int16 (uint8 with sample_bytes=1; numpy array or torch tensor, any device; may be empty) ->
        [base64, ...]"""
        if hasattr(pcm, "detach"):
            pcm = pcm.detach().cpu().numpy()
        pcm = np.asarray(pcm)
        if pcm.dtype != (np.int16 if self.sample_bytes == 2 else np.uint8) or pcm.ndim != 1:
            raise ValueError("pcm must be a 1-D %s array" % ("int16" if self.sample_bytes == 2 else "uint8"))
        buf = np.concatenate([self._rest, pcm.astype(self._wire, copy=False)])
        whole = len(buf) // self.n * self.n
        self._rest = buf[whole:]
        return [base64.b64encode(buf[t:t + self.n].tobytes()).decode("utf-8") for t in range(0, whole, self.n)]

    def close(self):
        rest, self._rest = self._rest, np.zeros(0, self._wire)
        return [base64.b64encode(rest.tobytes()).decode("utf-8")] if len(rest) else []
