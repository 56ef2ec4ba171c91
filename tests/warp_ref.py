"""Float64 NumPy restatement of the time warp of DESIGN §7.22 (per-token pitch by varispeed): the rate table from the
tokens, the glide, the output positions U, the model time tau of an output, resampy's loop evaluated there, and the
readiness count.  It reuses `resample_ref.table` and does not import the package; parity of the GPU kernel and of the
host planner is pinned to this module.

A rate table is fp32 in the package (its values are what `(double)R[f]` reads).  The functions here take any array and
compute in float64 from its values, so a test may also hand them a float64 table.
"""
import math

import numpy as np

import resample_ref

PITCH_MIN, PITCH_MAX = 0.5, 2.0


def pitch_of_semitones(st):
    return 2.0 ** (st / 12.0)


def frame_rates(pitch, marks, frames):
    """The step table: the pitch of the token that holds frame f (`marks` [T + 1]: the frame at which every token
    starts, the last entry the end), 1.0 for a frame no token holds; fp32 [frames]."""
    R = np.ones(frames, np.float32)
    for j, p in enumerate(pitch):
        R[min(int(marks[j]), frames):min(int(marks[j + 1]), frames)] = np.float32(p)
    return R


def glide(R, g):
    """R'[f] = the float64 mean of R over [f - g, f + g] within [0, F), added in ascending order, rounded to fp32."""
    R = np.asarray(R, np.float32)
    F = len(R)
    if g == 0:
        return R.copy()
    out = np.empty(F, np.float32)
    for f in range(F):
        lo, hi = max(0, f - g), min(F, f + g + 1)
        acc = 0.0
        for k in range(lo, hi):
            acc += float(R[k])
        out[f] = np.float32(acc / float(hi - lo))
    return out


def plan(R, hop):
    """-> (U float64 [F + 1], n_out): U[f + 1] = U[f] + hop / R[f] in ascending order, n_out = floor(U[F])."""
    U = np.zeros(len(R) + 1, np.float64)
    u = 0.0
    for f in range(len(R)):
        u += float(hop) / float(R[f])
        U[f + 1] = u
    return U, int(math.floor(u))


def frame_of(t, U):
    """the largest f < F with U[f] <= t"""
    return min(int(np.searchsorted(U, float(t), side="right")) - 1, len(U) - 2)


def tau(t, U, R, hop):
    f = frame_of(t, U)
    return float(f * hop) + (float(t) - float(U[f])) * float(R[f]), f


_tables = {}


def _window(res_type, scale):
    key = (res_type, scale)
    if key not in _tables:
        win, nb = resample_ref.table(res_type)
        win = win * scale if scale != 1.0 else win
        delta = np.zeros_like(win)
        delta[:-1] = np.diff(win)
        _tables[key] = (win, delta, nb)
    return _tables[key]


def _wings(t, U, R, hop, res_type):
    """the two wings of output t: [(source indices, weights)] as resampy's loop visits them, unbounded by the row"""
    tm, f = tau(t, U, R, hop)
    r = float(R[f])
    scale = 1.0 / r if r > 1.0 else 1.0
    win, delta, nb = _window(res_type, scale)
    step = int(scale * nb)
    nwin = len(win)
    n = int(tm)
    frac = scale * (tm - n)
    out = []
    for side in (0, 1):
        fr = frac if side == 0 else scale - frac
        idx = fr * nb
        off = int(idx)
        eta = idx - off
        k = np.arange((nwin - off) // step)
        j = off + k * step
        out.append((n - k if side == 0 else n + 1 + k, win[j] + eta * delta[j]))
    return out


def tap_extent(t, U, R, hop, res_type="kaiser_best"):
    """(lowest, highest) model index output t reads, before the row's ends cut the loops"""
    (left, _), (right, _) = _wings(t, U, R, hop, res_type)
    return int(left.min()), int(right.max() if len(right) else left.max())


def warp(x, R, hop, res_type="kaiser_best", in_avail=None, first=0, end=None):
    """Outputs [first, end) (default: all n_out) of the row x [F * hop]: float64.  Taps outside [0, min(n, in_avail))
    read a zero and nothing there is looked at."""
    x = np.asarray(x, np.float64)
    F = len(R)
    assert len(x) == F * hop
    U, n_out = plan(R, hop)
    limit = len(x) if in_avail is None else min(len(x), int(in_avail))
    end = n_out if end is None else end
    y = np.zeros(end - first)
    for t in range(first, end):
        acc = 0.0
        for src, w in _wings(t, U, R, hop, res_type):
            ok = (src >= 0) & (src < limit)
            acc += float(np.sum(w[ok] * x[src[ok]]))
        y[t - first] = acc
    return y


def half_width(R, res_type="kaiser_best"):
    return int(math.ceil(resample_ref.FILTERS[res_type][0] * max(1.0, max(float(r) for r in R)))) + 2


def ready(R, U, hop, in_avail, res_type="kaiser_best"):
    """How many outputs are final once the model samples [0, in_avail) exist."""
    F = len(R)
    if in_avail >= F * hop:
        return int(math.floor(U[F]))
    a = int(in_avail) - half_width(R, res_type)
    if a <= 0:
        return 0
    g = a // hop
    return max(0, int(math.floor(float(U[g]) + float(a - g * hop) / float(R[g]))) - 1)


def samples_of_frames(U, frames):
    """ceil(U[f]) of every frame index: the first warped sample at or behind the frame's start"""
    return [int(math.ceil(float(U[f]))) for f in frames]
