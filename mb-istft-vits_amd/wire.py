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
"""
import base64

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

    All state lives in tensors the stream owns, so paused and interleaved streams on one model do not mix."""

    def __init__(self, net, st, model_sr, rate, peak=None, res_type="kaiser_best"):
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
        a, b = self._done, self._ready[i]
        net.resample_pcm16_range(st.o, self.model_sr, self.rate, st.spf * (first + count), a, b - a, self.pcm,
                                 valid_samples=self._valid_in, peak=self._peak_in, running_peak=self.peak,
                                 out_samples=self.valid_samples if i == 0 else None, res_type=self.res_type)
        self._done = b
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
