"""The signals of tests/test_gpu_loudness.py and their float64 reference, computed once per rate and shared.

Seeded fp32 uniform noise of amplitude 0.25, 3 fs + 137 samples:
  a     scaled by -30 dB after the first second: the relative gate drops blocks
  b     scaled by 1e-5 in the middle second: the absolute gate drops blocks
  zero  all zero: -inf
  s3, s4, s5m   rows of 3 H, 4 H and 5 H - 1 valid samples: no block, one, one
"""
import numpy as np

import loudness_ref

RATES = [8000, 22050, 48000]
SEED = 2024
MARGIN = 0.1          # LU: no block may lie this close to a gate, so that a rounding difference cannot flip it
_CASES = {}


def signals(fs):
    """-> (x fp32 [6, n], valid [6], names)"""
    n = 3 * fs + 137
    H = loudness_ref.hop(fs)
    rs = np.random.RandomState(SEED + fs % 1000)
    base = rs.uniform(-0.25, 0.25, size=(4, n)).astype(np.float32)
    a = base[0].copy()
    a[fs:] *= np.float32(10.0 ** (-30.0 / 20.0))
    b = base[1].copy()
    b[fs:2 * fs] *= np.float32(1e-5)
    x = np.stack([a, b, np.zeros(n, np.float32), base[2], base[3], base[2][::-1].copy()])
    valid = [n, n, n, 3 * H, 4 * H, 5 * H - 1]
    return x, valid, ["a", "b", "zero", "s3", "s4", "s5m"]


def case(fs):
    """-> dict(x, valid, names, ref): ref[i] = loudness_ref.measure of row i over its valid length"""
    if fs not in _CASES:
        x, valid, names = signals(fs)
        _CASES[fs] = dict(x=x, valid=valid, names=names, ref=[loudness_ref.measure(r, fs, v) for r, v in zip(x, valid)])
    return _CASES[fs]


def margins(ref):
    """(distance of the closest block to the -70 gate, distance of the closest absolute-gated block to the relative
    gate), in LU; inf where there is no block to compare"""
    l = ref["l"]
    finite = l[np.isfinite(l)]
    d_abs = float(np.min(np.abs(finite + 70.0))) if len(finite) else np.inf
    kept = l[ref["abs_keep"]]
    d_rel = float(np.min(np.abs(kept - ref["rel_thr"]))) if len(kept) else np.inf
    return d_abs, d_rel
