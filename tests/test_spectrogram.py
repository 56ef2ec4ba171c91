"""CPU: the float64 restatement of the linear spectrogram (tests/spectrogram_ref.py) against torch.stft,
the function spectrogram_torch (mel_processing.py:51-70) calls, and the host-only frame rule of the C ABI."""
import numpy as np
import pytest
import torch

import spectrogram_ref as SR
from mb_istft_vits_amd import _capi

PARAMS = [(1024, 256, 1024), (512, 128, 512), (2048, 512, 2048), (1024, 256, 800), (1024, 255, 1024),
          (1024, 300, 1024)]


def _torch_spec(x, n_fft, hop, win):
    """spectrogram_torch's steps in float64: constant padding, torch.stft(center=False), abs()."""
    y = torch.from_numpy(x).view(1, 1, -1)
    p = int((n_fft - hop) / 2)
    y = torch.nn.functional.pad(y, (p, p), mode="constant", value=0).squeeze(1)
    s = torch.stft(y, n_fft, hop_length=hop, win_length=win, window=torch.hann_window(win, dtype=torch.float64),
                   center=False, pad_mode="reflect", normalized=False, onesided=True, return_complex=True)
    return torch.abs(s)[0].numpy()


@pytest.mark.parametrize("n_fft,hop,win", PARAMS)
def test_restatement_matches_torch_stft(n_fft, hop, win):
    rs = np.random.RandomState(n_fft + hop + win)
    for n in (n_fft - 2 * ((n_fft - hop) // 2), 3 * n_fft + 17, 22050):
        x = rs.uniform(-1, 1, n)
        ref, got = _torch_spec(x, n_fft, hop, win), SR.spectrogram(x, n_fft, hop, win)
        assert got.shape == ref.shape == (n_fft // 2 + 1, SR.frames(n, n_fft, hop))
        assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()


@pytest.mark.parametrize("n_fft,hop,win", PARAMS + [(256, 256, 256), (4096, 1, 4096), (256, 1, 7)])
def test_frame_rule_matches_torch(n_fft, hop, win):
    L = _capi.lib()
    p = (n_fft - hop) // 2
    zero_frame_cases = 0
    for n in range(0, 3 * n_fft + 1):
        want = SR.frames(n, n_fft, hop)
        assert L.mbv_spectrogram_frames(n, n_fft, hop) == want, n
        if n + 2 * p < n_fft:
            assert want == 0
            zero_frame_cases += 1
            with pytest.raises(RuntimeError):                  # torch.stft refuses a signal shorter than n_fft
                torch.stft(torch.zeros(1, n + 2 * p), n_fft, hop_length=hop, window=torch.ones(n_fft), center=False,
                           return_complex=True)
        elif n % 97 == 0 or n == n_fft - 2 * p:
            got = torch.stft(torch.zeros(1, n + 2 * p), n_fft, hop_length=hop, window=torch.ones(n_fft), center=False,
                           return_complex=True)
            assert got.shape[-1] == want, n
    assert zero_frame_cases == max(0, n_fft - 2 * p)
    assert L.mbv_spectrogram_frames(1 << 40, n_fft, hop) == SR.frames(1 << 40, n_fft, hop)


def test_frame_rule_refuses_bad_arguments():
    L = _capi.lib()
    for n, n_fft, hop in [(-1, 1024, 256), (100, 1000, 256), (100, 128, 64), (100, 8192, 256), (100, 1024, 0),
                          (100, 1024, 1025), (100, 1024, -3), (100, 0, 1)]:
        assert L.mbv_spectrogram_frames(n, n_fft, hop) == -1, (n, n_fft, hop)
    assert L.mbv_spectrogram_frames(0, 1024, 1024) == 0
    assert L.mbv_spectrogram_frames(1024, 1024, 1024) == 1
