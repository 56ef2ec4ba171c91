"""ITU-R BS.1770-4 integrated loudness of a mono signal, restated from the standard in float64 (numpy only, no audio
library): the reference of tests/test_loudness.py and tests/test_gpu_loudness.py.

Sequential over the whole row, in direct form I: no segment chain, no transposed form, no transition matrix, so it
shares neither the structure nor the rounding of the kernel it checks.

  K-weighting  two cascaded biquads, zero state at sample 0.  The standard tabulates 48 kHz; other rates use the
               bilinear re-derivation from the analogue prototypes (f0, G, Q below), which gives the table at 48 kHz
  segments     H = floor(fs / 10 + 1 / 2) samples (100 ms); an incomplete tail is dropped
  blocks       four segments (400 ms, 75 % overlap): z_j = (e_j + .. + e_{j+3}) / (4 H), l_j = -0.691 + 10 log10 z_j
  gates        l_j > -70, then l_j > -0.691 + 10 log10(mean z of those) - 10
  L            -0.691 + 10 log10(mean z of the blocks that pass both), -inf without one
"""
import math

import numpy as np

SHELF = dict(f0=1681.974450955533, G=3.999843853973347, Q=0.7071752369554196)
HIGHPASS = dict(f0=38.13547087602444, Q=0.5003270373238773)
VB_EXP = 0.4996667741545416

# the standard's 48 kHz table (BS.1770-4, tables 1 and 2)
TABLE_48K = dict(shelf_b=(1.53512485958697, -2.69169618940638, 1.19839281085285),
                 shelf_a=(-1.69065929318241, 0.73248077421585),
                 highpass_a=(-1.99004745483398, 0.99007225036621))


def hop(fs):
    return int(math.floor(fs / 10.0 + 0.5))


def kweighting(fs):
    """-> ((b0, b1, b2), (a1, a2)) of the shelf, then of the high-pass."""
    fs = float(fs)
    K = math.tan(math.pi * SHELF["f0"] / fs)
    Q = SHELF["Q"]
    Vh = 10.0 ** (SHELF["G"] / 20.0)
    Vb = Vh ** VB_EXP
    a0 = 1.0 + K / Q + K * K
    shelf = (((Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0),
             (2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0))
    K = math.tan(math.pi * HIGHPASS["f0"] / fs)
    Q = HIGHPASS["Q"]
    a0 = 1.0 + K / Q + K * K
    highpass = ((1.0, -2.0, 1.0), (2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0))
    return shelf, highpass


def _biquad(x, b, a):
    """y[n] = b0 x[n] + b1 x[n-1] + b2 x[n-2] - a1 y[n-1] - a2 y[n-2], zero history; x a list of floats."""
    b0, b1, b2 = b
    a1, a2 = a
    x1 = x2 = y1 = y2 = 0.0
    out = [0.0] * len(x)
    for n, xn in enumerate(x):
        yn = b0 * xn + b1 * x1 + b2 * x2 - a1 * y1 - a2 * y2
        out[n] = yn
        x2, x1, y2, y1 = x1, xn, y1, yn
    return out


def state_matrix(fs):
    """One zero-input step of the cascade's transposed-direct-form-II state (shelf s1, s2, high-pass s1, s2), the
    form the C-ABI documents: y = b0 x + s1; s1' = b1 x - a1 y + s2; s2' = b2 x - a2 y, with x = 0 into the shelf."""
    (b, a), (c, d) = kweighting(fs)
    return np.array([[-a[0], 1.0, 0.0, 0.0],
                     [-a[1], 0.0, 0.0, 0.0],
                     [c[1] - d[0] * c[0], 0.0, -d[0], 1.0],
                     [c[2] - d[1] * c[0], 0.0, -d[1], 0.0]], dtype=np.float64)


def measure(x, fs, n=None):
    """x: 1-D samples (any float dtype), n: valid samples (None = all) -> dict:
      L          integrated loudness (float, -inf without a block)
      energies   float64 [n // H]
      l          float64 [blocks] block loudness (-inf for a silent block)
      abs_keep   bool [blocks], rel_thr (float, -inf without an absolute-gated block), keep bool [blocks]"""
    x = np.asarray(x, dtype=np.float64)
    if n is not None:
        x = x[:int(n)]
    H = hop(fs)
    S = len(x) // H
    shelf, highpass = kweighting(fs)
    y = np.asarray(_biquad(_biquad(x[:S * H].tolist(), *shelf), *highpass), dtype=np.float64)
    energies = np.array([float(np.sum(y[k * H:(k + 1) * H] ** 2)) for k in range(S)], dtype=np.float64)
    nb = max(S - 3, 0)
    z = np.array([(energies[j] + energies[j + 1] + energies[j + 2] + energies[j + 3]) / (4.0 * H) for j in range(nb)],
                 dtype=np.float64)
    with np.errstate(divide="ignore"):
        l = -0.691 + 10.0 * np.log10(z) if nb else np.zeros(0)
    abs_keep = l > -70.0
    rel_thr = -math.inf
    keep = np.zeros(nb, dtype=bool)
    L = -math.inf
    if abs_keep.any():
        rel_thr = -0.691 + 10.0 * math.log10(float(np.mean(z[abs_keep]))) - 10.0
        keep = abs_keep & (l > rel_thr)
        if keep.any():
            L = -0.691 + 10.0 * math.log10(float(np.mean(z[keep])))
    return dict(L=L, energies=energies, l=l, abs_keep=abs_keep, rel_thr=rel_thr, keep=keep, hop=H)
