"""Float64 restatement of the wire step's fade-out and of the token marks, straight from their
definitions, on top of tests/resample_ref.py and tests/limiter_ref.py.

    ramp[t] = 1                          t < first
              (count - k) / (count + 1)  k = t - first, 0 <= k < count
              0                          k >= count
    y[t] = v[t] g[t] ramp[t] (g: the limiter's gain, 1 without one), then clip to [-1, 1], * 32767, truncate
    the stream's length becomes min(length, first + count)
    a mark at z-frame f is the wire sample ceil(f * samples_per_frame * rate / model_sr) + lookahead
"""
from fractions import Fraction
import math

import numpy as np

import limiter_ref
import resample_ref


def ramp(n, first, count):
    """float64 [n]: the factor of every output index."""
    k = np.arange(n, dtype=np.int64) - int(first)
    inside = (count - k) / float(count + 1)
    return np.where(k < 0, 1.0, np.where(k < count, inside, 0.0))


def length(total, first, count):
    """The length of a stream of `total` samples revoked with the fade (first, count)."""
    return min(int(total), int(first) + int(count))


def pcm16(v, first, count, limiter=None):
    """int16 [len(v)]: the samples v (the static gain included) through the optional limiter (ceiling, lookahead, hold),
    the fade and the wire epilogue (clip, * 32767, truncate)."""
    v = np.asarray(v, dtype=np.float64)
    y = v if limiter is None else limiter_ref.limit(v, *limiter)
    y = np.clip(y * ramp(len(v), first, count), -1.0, 1.0) * 32767.0
    return np.trunc(y).astype(np.int16)


def wire_pcm16(x, orig_sr, target_sr, first, count, limiter=None, res_type="kaiser_best"):
    """(int16, length): one row from its input samples, everything in float64: resample_ref.resample, then `pcm16`;
    the length is that of the faded stream."""
    v = resample_ref.resample(x, orig_sr, target_sr, res_type)
    return pcm16(v, first, count, limiter), length(len(v), first, count)


def mark_samples(marks, samples_per_frame, model_sr, rate, lookahead=0):
    """The wire sample of every mark, in exact rationals: the first sample at or after the token's first model sample
    f * samples_per_frame, i.e. at time f * samples_per_frame / model_sr, moved by the limiter's lag."""
    return [math.ceil(Fraction(int(f) * int(samples_per_frame), int(model_sr)) * int(rate)) + int(lookahead)
            for f in marks]
