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
"""
import base64
import ctypes as C

import numpy as np
import torch

from . import _capi
from .models import RESAMPLE_TYPES


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


def service_pcm16(net, o, y_lengths, model_sr, rate, auto_normalize=True, res_type="kaiser_best"):
    """tts_vits.py:196-217 for a batch as one GPU chain: resample every utterance from `model_sr` to
    `rate` (skipped when they are equal, as there), then peak-normalise / clip / int16 it.
      o          fp32 [B, 1, n] waveforms of `net.infer` (device)
      y_lengths  int64 [B] frames per utterance (valid samples = 256 * y_lengths, clamped to the row),
                 or None = whole rows
    -> (pcm int16 [B, n'], valid_samples int64 [B]); row b of `pcm` holds the int16 stream of utterance b
    in its first valid_samples[b] samples, ready for `frame_pcm16(pcm[b], rate, valid_samples=...)`.
    No host synchronisation (beyond the first call for a rate pair, see `SynthesizerTrn.resample`)."""
    wave, valid = net.resample(o, model_sr, rate, y_lengths=y_lengths, res_type=res_type)
    return net.to_pcm16(wave, auto_normalize=auto_normalize, valid_samples=valid), valid


def convert_pcm16(net, wave, valid_samples, sid_src, sid_tgt, in_sr, model_sr, rate, hop_size, win_size,
                  auto_normalize=True, res_type="kaiser_best"):
    """Voice conversion from audio to audio as one GPU chain:
      1. `wave` int16 or fp32 [B, n] / [B, 1, n] at `in_sr` (int16 is scaled by 1 / 32768, data_utils.py:75),
         `valid_samples` int64 [B] samples per utterance or None = whole rows;
      2. `net.resample` to `model_sr` when the rates differ;
      3. `net.spectrogram` with n_fft = 2 (spec_channels - 1), the posterior encoder's input width;
      4. `net.voice_conversion(spec, spec_lengths, sid_src, sid_tgt)`;
      5. `service_pcm16(net, o, y_lengths, model_sr, rate, ...)`.
    -> (pcm int16 [B, n'], valid_samples int64 [B]) as `service_pcm16` returns them.  Raises ValueError before
    anything is launched when win_size > n_fft or the model has no speakers.  The one host synchronisation is
    the status check `voice_conversion` already has (besides the first-call table uploads of `resample` and
    `spectrogram`)."""
    n_fft = 2 * (net.cfg.spec_channels - 1)
    if not net.n_speakers > 0:
        raise ValueError("convert_pcm16: voice conversion needs a multi-speaker model (n_speakers > 0)")
    if not 1 <= int(win_size) <= n_fft:
        raise ValueError("convert_pcm16: win_size %d must be in [1, n_fft = 2 * (spec_channels - 1) = %d]"
                         % (int(win_size), n_fft))
    if wave.dim() == 2:
        wave = wave.unsqueeze(1)
    if wave.dtype == torch.int16 and int(in_sr) != int(model_sr):
        wave = wave.float() / 32768.0                          # the resampler takes fp32; exact scaling
    wave, valid = net.resample(wave, in_sr, model_sr, valid_samples=valid_samples, res_type=res_type)
    spec, spec_lengths = net.spectrogram(wave, n_fft, hop_size, win_size, valid_samples=valid)
    o = net.voice_conversion(spec, spec_lengths, sid_src, sid_tgt)[0]
    return service_pcm16(net, o, spec_lengths, model_sr, rate, auto_normalize=auto_normalize, res_type=res_type)


def resample_ready(orig_sr, target_sr, in_avail, in_total, res_type="kaiser_best"):
    """How many resampled samples of a row of `in_total` input samples are final once its first `in_avail`
    exist (`mbv_resample_ready`, host only: no GPU needed); ceil(in_total * target / orig) once all do."""
    filt = RESAMPLE_TYPES.get(res_type)
    if filt is None:
        raise ValueError("res_type %r is not supported on the GPU path (supported: %s)"
                         % (res_type, ", ".join(sorted(RESAMPLE_TYPES))))
    L = _capi.lib()
    r = L.mbv_resample_ready(int(orig_sr), int(target_sr), filt, int(in_avail), int(in_total))
    if r < 0:
        msg = L.mbv_last_error(None)
        raise _capi.MbvError(msg.decode() if msg else "mbv_resample_ready failed")
    return int(r)


def _refuse_live(st):
    from .stream import LiveStream
    if isinstance(st, LiveStream):
        raise TypeError("the wire output of a LiveStream (net.convert_live) is not built: the resampler's output length "
                        "and valid_samples need the recording's total length, which an open stream does not have. "
                        "Take the float chunks from poll(), or convert the finished recording with convert_stream")


class PcmStream:
    """Iterator over (first_out_sample, pcm[:, a:b]) of one streamed decode: after every chunk of the wrapped
    `stream.DecodeStream` one `mbv_resample_pcm16_range` launch turns the resampled samples that chunk made final
    into int16, on the caller's current stream, and the view is ordered on that stream like every other output.
    The filter needs input on both sides of an output, so the wire lags the decoder by the filter's half-width
    (64 input samples for kaiser_best upsampling); the last chunk flushes it.  A chunk shorter than that lag
    yields an empty view.  No host synchronisation per chunk.

      pcm            int16 [B, out_stride], out_stride = ceil(spf T' * rate / model_sr); after the last chunk
                     bitwise the `service_pcm16` of the finished `st.o` (auto_normalize = `peak is not None`
                     when `peak` is the utterance's true peak)
      valid_samples  int64 [B] device, the lengths `service_pcm16` returns (written by the first chunk)
      peak           fp32 [B] device, the running peak of the resampled samples emitted so far; after the last
                     chunk bitwise the peak `service_pcm16(auto_normalize=True)` would have divided by

    All state lives in tensors the stream owns, so paused and interleaved streams on one model do not mix.

    A `PcmPool` may wire chunks ahead of the iterator (`_wired` > the decode stream's `_next`): `next()` then hands
    such a piece out without launching anything, and launches alone otherwise — the same bytes either way."""

    def __init__(self, net, st, model_sr, rate, peak=None, res_type="kaiser_best"):
        _refuse_live(st)
        self._net, self._st, self._h = net, st, st._h
        self.model_sr, self.rate, self.res_type = int(model_sr), int(rate), res_type
        o = st.o
        B, n = o.shape[0], o.shape[-1]
        dev = o.device
        # final outputs after each decoded chunk (pure integers of the schedule: nothing to ask the device)
        self._ready = [resample_ready(model_sr, rate, st.spf * (first + count), n, res_type)
                       for first, count in st.schedule]
        self.out_stride = resample_ready(model_sr, rate, n, n, res_type)
        self.pcm = torch.empty(B, self.out_stride, device=dev, dtype=torch.int16)
        self.valid_samples = torch.zeros(B, device=dev, dtype=torch.int64)
        self.peak = torch.zeros(B, device=dev, dtype=torch.float32)
        self._valid_in = None                     # valid input samples, as service_pcm16 counts them
        if st.y_lengths is not None:
            self._valid_in = (st.y_lengths.to(device=dev, dtype=torch.int64) * 256).clamp(0, n).contiguous()
        if peak is not None:
            if not torch.is_tensor(peak):
                peak = torch.full((B,), float(peak), device=dev, dtype=torch.float32)   # a fill, not a host copy
            peak = peak.to(device=dev, dtype=torch.float32).contiguous()
            if peak.shape != (B,):
                raise ValueError("peak must be a float or an fp32 [B] tensor")
        self._peak_in = peak
        self._done = 0                            # outputs emitted so far
        self._wired = 0                           # the first chunk whose final outputs are not emitted yet

    def __len__(self):
        return len(self._st)

    def __iter__(self):
        return self

    def __next__(self):
        st, net = self._st, self._net
        i = st._next
        next(st)                                  # decodes chunk i (StopIteration ends this stream too)
        if net._handle is not self._h:
            raise RuntimeError("the model's handle was re-created (device move) since this stream started")
        first, count = st.schedule[i]
        if i < self._wired:                       # a pool wired it already, on the stream current at its step
            a, b = (self._ready[i - 1] if i else 0), self._ready[i]
            return a, self.pcm[:, a:b]
        a, b = self._done, self._ready[i]
        net.resample_pcm16_range(st.o, self.model_sr, self.rate, st.spf * (first + count), a, b - a, self.pcm,
                                 valid_samples=self._valid_in, peak=self._peak_in, running_peak=self.peak,
                                 out_samples=self.valid_samples if self._wired == 0 else None,
                                 res_type=self.res_type)
        self._done, self._wired = b, i + 1
        return a, self.pcm[:, a:b]

    def run(self):
        """Every remaining chunk; -> (pcm, valid_samples)."""
        for _ in self:
            pass
        return self.pcm, self.valid_samples


def stream_pcm16(net, st, model_sr, rate, peak=None, res_type="kaiser_best"):
    """The streamed `service_pcm16`: wraps a `stream.DecodeStream` (`net.dec_stream` / `net.infer_stream`, not yet
    iterated) in a `PcmStream`.
      peak  None: no normalisation (auto_normalize=False, exact).  A float or an fp32 [B] tensor: every sample is
            divided by it and scaled by 0.9 where it exceeds 0.01, as tts_vits.py:205-208 does with the peak of
            the whole resampled utterance.  That peak does not exist before the last chunk, so it is an input
            here (e.g. `PcmStream.peak` of the speaker's previous utterance); the clip that follows bounds
            what a peak chosen too small can do."""
    if st._next:
        raise ValueError("stream_pcm16: the decode stream has already been advanced")
    return PcmStream(net, st, model_sr, rate, peak=peak, res_type=res_type)


def pcm_chunks_plan(orig_sr, target_sr, chunks, res_type="kaiser_best"):
    """(total, packed_first) of `mbv_pcm_chunks_plan` for `_capi.MbvPcmChunk`s (host only: no GPU needed, only the
    integer fields are read): the checks `resample_pcm16_chunks` makes, and where every chunk starts in the packed
    buffer.  Raises `_capi.MbvError` naming the offending chunk."""
    filt = RESAMPLE_TYPES.get(res_type)
    if filt is None:
        raise ValueError("res_type %r is not supported on the GPU path (supported: %s)"
                         % (res_type, ", ".join(sorted(RESAMPLE_TYPES))))
    if not isinstance(chunks, C.Array):
        chunks = (_capi.MbvPcmChunk * len(chunks))(*chunks)
    n = len(chunks)
    first = (C.c_int64 * max(n, 1))()
    L = _capi.lib()
    total = L.mbv_pcm_chunks_plan(int(orig_sr), int(target_sr), filt, chunks, n, first)
    if total < 0:
        msg = L.mbv_last_error(None)
        raise _capi.MbvError(msg.decode() if msg else "mbv_pcm_chunks_plan failed")
    return int(total), list(first)[:n]


def wire_runs(net):
    """Resample / int16 launches of the streamed wire step made on the model's handle so far (`mbv_wire_runs`):
    one per `resample_pcm16_range` call that had something to write, one per `resample_pcm16_chunks` call."""
    return int(_capi.lib().mbv_wire_runs(net._ensure_handle()))


class PcmPool:
    """The wire output of many `DecodeStream`s of one model: `step()` steps the wrapped `stream.StreamPool` (one
    `mbv_decode_chunks` call) and then turns what has become final on ALL pooled streams into int16 in ONE
    `mbv_resample_pcm16_chunks` launch, instead of one `mbv_resample_pcm16_range` launch per stream.

    `add(st, peak=None)` returns the stream's `PcmStream` follower, which holds the state it holds alone (`pcm`,
    `valid_samples`, `peak`); the pieces count as wired ahead on it, so `next(follower)` afterwards hands them out
    without a launch.  A stream may be driven through the pool, alone, or both in turn: the same bytes, those
    `service_pcm16` gives for the finished waveform.  Finished streams drop out."""

    def __init__(self, net, pool, model_sr, rate, res_type="kaiser_best"):
        if RESAMPLE_TYPES.get(res_type) is None:
            raise ValueError("res_type %r is not supported on the GPU path (supported: %s)"
                             % (res_type, ", ".join(sorted(RESAMPLE_TYPES))))
        if pool._net is not net:
            raise ValueError("the stream pool belongs to another model")
        self._net, self.pool = net, pool
        self.model_sr, self.rate, self.res_type = int(model_sr), int(rate), res_type
        self.followers = []
        self._packed = None                       # int16 device, the call's pieces back to back (host=True)
        self._host = self._host_np = None         # its pinned host copy, and that as a NumPy array
        self._event = None

    def __len__(self):
        return len(self.followers)

    def follower(self, st):
        for f in self.followers:
            if f._st is st:
                return f
        return None

    def add(self, st, peak=None):
        _refuse_live(st)
        self.pool.add(st)                         # (refuses B > 1, another model, another device)
        f = self.follower(st)
        if f is None:
            f = PcmStream(self._net, st, self.model_sr, self.rate, peak=peak, res_type=self.res_type)
            self.followers.append(f)
        return f

    def admit(self, requests, peak=None):
        """`StreamPool.admit(requests)` + a follower for each new stream (`peak`: None, one value for all, or one per
        request, as `add` takes it); -> the followers, in order.  `requests` is all `models.Request` or all
        `models.ConvertRequest` (audio), as `StreamPool.admit` takes them.  All or nothing, like `StreamPool.admit`."""
        reqs = list(requests)
        peaks = list(peak) if isinstance(peak, (list, tuple)) else [peak] * len(reqs)
        if len(peaks) != len(reqs):
            raise ValueError("admit: one peak per request expected (%d), got %d" % (len(reqs), len(peaks)))
        return [self.add(st, peak=p) for st, p in zip(self.pool.admit(reqs), peaks)]

    def step(self, streams=None, host=False):
        """-> [(st, first_out_sample, piece), ...]: one entry per stream whose decoded frontier made outputs final
        (an empty piece is possible, as for `PcmStream`).  `piece` is the 1-D view `follower.pcm[0, a:b]` on the
        device, ordered on the current stream; with host=True it is a NumPy int16 view of ONE pinned buffer that
        one copy and one event wait filled, valid until the next `step(host=True)`."""
        net = self._net
        if streams is None:
            members = list(self.followers)
        else:
            members = []
            for st in streams:
                f = self.follower(st)
                if f is None:
                    raise ValueError("step(streams=...) names a stream that is not in the pool")
                members.append(f)
        named = None if streams is None else [f._st for f in members if f._st._decoded < len(f._st.schedule)]
        if named is None or named:
            self.pool.step(named)
        todo = [f for f in members if f._st._decoded > f._wired]
        out = []
        if todo:
            arr = (_capi.MbvPcmChunk * len(todo))()
            for k, f in zip(arr, todo):
                st = f._st
                if net._handle is not f._h:
                    raise RuntimeError("the model's handle was re-created (device move) since a pooled stream started")
                first, count = st.schedule[st._decoded - 1]
                a, b = f._done, f._ready[st._decoded - 1]
                k.wave, k.in_total = st.o.data_ptr(), st.o.shape[-1]
                k.valid_samples = f._valid_in.data_ptr() if f._valid_in is not None else None
                k.in_avail, k.out_first, k.out_count = st.spf * (first + count), a, b - a
                k.peak = f._peak_in.data_ptr() if f._peak_in is not None else None
                k.pcm, k.pcm_capacity = f.pcm.data_ptr(), f.out_stride
                k.running_peak = f.peak.data_ptr()
                k.out_samples = f.valid_samples.data_ptr() if f._wired == 0 else None
                out.append((st, a, b))
            dev = net._device()
            packed = None
            if host:
                total, offs = pcm_chunks_plan(self.model_sr, self.rate, arr, self.res_type)
                if self._packed is None or self._packed.shape[0] < total:
                    cap = max(2 * total, 1 << 16)
                    self._packed = torch.empty(cap, device=dev, dtype=torch.int16)
                    self._host = torch.empty(cap, dtype=torch.int16, pin_memory=True)
                    self._host_np = self._host.numpy()
                    self._event = torch.cuda.Event()
                packed = self._packed
            net.resample_pcm16_chunks(arr, self.model_sr, self.rate, packed=packed, res_type=self.res_type)
            for f in todo:
                f._done, f._wired = f._ready[f._st._decoded - 1], f._st._decoded
            if host:
                if total:
                    with torch.cuda.device(dev):
                        self._host[:total].copy_(packed[:total], non_blocking=True)
                        self._event.record(torch.cuda.current_stream(dev))
                        self._event.synchronize()
                out = [(st, a, self._host_np[o:o + b - a]) for (st, a, b), o in zip(out, offs)]
            else:
                out = [(st, a, f.pcm[0, a:b]) for (st, a, b), f in zip(out, todo)]
        self.followers = [f for f in self.followers if f._wired < len(f._st.schedule)]
        return out


def pcm_pool(net, pool, model_sr, rate, res_type="kaiser_best"):
    """The pooled `stream_pcm16`: a `PcmPool` over a `stream.StreamPool` (`net.stream_pool()`) of the same model.
    `add(st, peak=None)` takes `peak` as `stream_pcm16` does."""
    return PcmPool(net, pool, model_sr, rate, res_type=res_type)


class FrameCutter:
    """`frame_pcm16` for an int16 stream that arrives in pieces: `push` returns the whole frames of
    `chunk_size(rate, frame_length)` samples that are complete, as base64 text, and carries the remainder;
    `close` returns the short last frame, if any.  The frames of all calls are those of `frame_pcm16` on the
    concatenation."""

    def __init__(self, rate, frame_length=0.02):
        self.n = chunk_size(rate, frame_length)
        if self.n <= 0:
            raise ValueError("frame_length * rate must be at least one sample")
        self._rest = np.zeros(0, "<i2")

    def push(self, pcm):
        """pcm: 1-D int16 (numpy array or torch tensor, any device; may be empty) -> [base64, ...]"""
        if hasattr(pcm, "detach"):
            pcm = pcm.detach().cpu().numpy()
        pcm = np.asarray(pcm)
        if pcm.dtype != np.int16 or pcm.ndim != 1:
            raise ValueError("pcm must be a 1-D int16 array")
        buf = np.concatenate([self._rest, pcm.astype("<i2", copy=False)])
        whole = len(buf) // self.n * self.n
        self._rest = buf[whole:]
        return [base64.b64encode(buf[t:t + self.n].tobytes()).decode("utf-8") for t in range(0, whole, self.n)]

    def close(self):
        rest, self._rest = self._rest, np.zeros(0, "<i2")
        return [base64.b64encode(rest.tobytes()).decode("utf-8")] if len(rest) else []
