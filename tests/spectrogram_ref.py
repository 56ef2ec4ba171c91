"""Float64 NumPy statement of the linear spectrogram of the data path (mel_processing.py:51-70 with
center=False, as data_utils.py:75-86 calls it), for one utterance:

  * pad = (n_fft - hop) // 2 zeros on both sides of the samples;
  * frame f is padded[f * hop : f * hop + n_fft] for f < frames(n) (see `frames`);
  * the window is the periodic Hann of length win, 0.5 - 0.5 cos(2 pi j / win), placed in the middle of
    n_fft with (n_fft - win) // 2 zeros before it;
  * the result is |rfft(window * frame)|, bins 0 .. n_fft // 2 along axis 0, frames along axis 1.
"""
import numpy as np


def frames(n, n_fft, hop):
    """Frames of an n-sample utterance: 0 when the padded signal is shorter than one window."""
    padded = n + 2 * ((n_fft - hop) // 2)
    return 0 if padded < n_fft else 1 + (padded - n_fft) // hop


def window(n_fft, win):
    w = np.zeros(n_fft)
    j = np.arange(win)
    left = (n_fft - win) // 2
    w[left:left + win] = 0.5 - 0.5 * np.cos(2.0 * np.pi * j / win)
    return w


def spectrogram(x, n_fft, hop, win):
    """x: 1-D samples -> float64 [n_fft // 2 + 1, frames(len(x))]."""
    x = np.asarray(x, np.float64)
    p = (n_fft - hop) // 2
    xp = np.concatenate([np.zeros(p), x, np.zeros(p)])
    nf = frames(len(x), n_fft, hop)
    if nf == 0:
        return np.zeros((n_fft // 2 + 1, 0))
    idx = np.arange(nf)[:, None] * hop + np.arange(n_fft)[None, :]
    seg = xp[idx] * window(n_fft, win)[None, :]
    return np.abs(np.fft.rfft(seg, axis=1)).T


def frame_norms(x, n_fft, hop, win):
    """||w * x_f||_2 per frame: the scale of the per-frame error bound."""
    x = np.asarray(x, np.float64)
    p = (n_fft - hop) // 2
    xp = np.concatenate([np.zeros(p), x, np.zeros(p)])
    nf = frames(len(x), n_fft, hop)
    idx = np.arange(nf)[:, None] * hop + np.arange(n_fft)[None, :]
    return np.sqrt(((xp[idx] * window(n_fft, win)[None, :]) ** 2).sum(axis=1)) if nf else np.zeros(0)
