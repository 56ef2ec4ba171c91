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
"""
import base64

import numpy as np
import torch


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
