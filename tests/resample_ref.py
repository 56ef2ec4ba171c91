"""Float64 NumPy restatement of librosa 0.9.2's `resample(y, orig_sr, target_sr)` with res_type
"kaiser_best" (its default) / "kaiser_fast": resampy's windowed-sinc interpolator followed by
librosa's fix_length.  librosa / resampy are not part of this build, so this restates the algorithm from
resampy's documented filter specs; parity of the GPU path is pinned to this module, not to the library.

Output t sits at the float64 input time t / ratio (resampy >= 0.3 computes `arange(n_out) / ratio`;
older releases accumulated `time += 1 / ratio`, which differs where that sum lands on the other side of
an integer).
"""
import math

import numpy as np

# resampy's filter specs: num_zeros, precision (table bits), Kaiser beta, rolloff
FILTERS = {
    "kaiser_best": (64, 9, 14.769656459379492, 0.9475937167399596),
    "kaiser_fast": (16, 9, 8.555504641634386, 0.85),
}


def table(res_type="kaiser_best"):
    """The right half of the interpolation window: kaiser(2n+1)[n:] * rolloff * sinc(rolloff * x)."""
    num_zeros, precision, beta, rolloff = FILTERS[res_type]
    nb = 2 ** precision
    n = nb * num_zeros
    win = np.kaiser(2 * n + 1, beta)[n:] * rolloff * np.sinc(rolloff * np.linspace(0, num_zeros, n + 1))
    return win, nb


def _setup(orig_sr, target_sr, res_type):
    win, nb = table(res_type)
    ratio = float(target_sr) / orig_sr
    if ratio < 1:
        win = win * ratio
    delta = np.zeros_like(win)
    delta[:-1] = np.diff(win)
    scale = min(1.0, ratio)
    step = int(scale * nb)                 # truncated, as resampy does
    return win, delta, ratio, scale, step, nb


def out_len(n, orig_sr, target_sr):
    """librosa 0.9.2 fix_length target: int(np.ceil(n * ratio)) in float64."""
    return int(np.ceil(n * (float(target_sr) / orig_sr)))


def resample_loop(x, orig_sr, target_sr, res_type="kaiser_best"):
    """resampy's loop, one output and one tap at a time (slow: short signals only)."""
    x = np.asarray(x, np.float64)
    if orig_sr == target_sr:
        return x.copy()
    win, delta, ratio, scale, step, nb = _setup(orig_sr, target_sr, res_type)
    n_in = len(x)
    n_out = int(n_in * ratio)
    nwin = len(win)
    y = np.zeros(n_out)
    for t in range(n_out):
        time = t / ratio
        n = int(time)
        frac = scale * (time - n)
        idx = frac * nb
        off = int(idx)
        eta = idx - off
        for i in range(min(n + 1, (nwin - off) // step)):
            y[t] += (win[off + i * step] + eta * delta[off + i * step]) * x[n - i]
        frac = scale - frac
        idx = frac * nb
        off = int(idx)
        eta = idx - off
        for k in range(min(n_in - n - 1, (nwin - off) // step)):
            y[t] += (win[off + k * step] + eta * delta[off + k * step]) * x[n + k + 1]
    return _fix_length(y, out_len(n_in, orig_sr, target_sr))


def resample(x, orig_sr, target_sr, res_type="kaiser_best"):
    """The same arithmetic as `resample_loop`, vectorised over outputs."""
    x = np.asarray(x, np.float64)
    if orig_sr == target_sr:
        return x.copy()
    win, delta, ratio, scale, step, nb = _setup(orig_sr, target_sr, res_type)
    n_in = len(x)
    n_out = int(n_in * ratio)
    nwin = len(win)
    y = np.zeros(n_out)
    if n_out:
        time = np.arange(n_out) / ratio
        n = time.astype(np.int64)
        frac = scale * (time - n)
        xp = np.concatenate([x, [0.0]])           # index n_in: a harmless target for masked-off taps
        for side in (0, 1):
            f = frac if side == 0 else scale - frac
            idx = f * nb
            off = idx.astype(np.int64)
            eta = idx - off
            cnt = (nwin - off) // step
            cnt = np.minimum(n + 1, cnt) if side == 0 else np.minimum(n_in - n - 1, cnt)
            taps = np.arange(int(cnt.max()) if cnt.size and cnt.max() > 0 else 0)
            if not taps.size:
                continue
            live = taps[None, :] < cnt[:, None]
            j = np.where(live, off[:, None] + taps[None, :] * step, 0)
            w = np.where(live, win[j] + eta[:, None] * delta[j], 0.0)
            src = n[:, None] - taps[None, :] if side == 0 else n[:, None] + 1 + taps[None, :]
            src = np.where(live, src, n_in)
            y += (w * xp[src]).sum(axis=1)
    return _fix_length(y, out_len(n_in, orig_sr, target_sr))


def _fix_length(y, size):
    if len(y) >= size:
        return y[:size]
    return np.concatenate([y, np.zeros(size - len(y))])


def apply_bank(x, bank, orig_sr, target_sr, left):
    """The polyphase form the GPU kernel computes, in float64 NumPy: out[t] = sum_k bank[r][k] x[n_t - left + k]
    with n_t = floor(t M / L), r = (t M) mod L, zeros outside [0, len(x)); then fix_length.  Bank row L
    (fraction 1, read around n_t - 1) replaces row 0 where t / ratio rounds below the integer n_t."""
    g = math.gcd(orig_sr, target_sr)
    L, M = target_sr // g, orig_sr // g
    K = bank.shape[1]
    n_in = len(x)
    n_out = int(n_in * (float(target_sr) / orig_sr))
    t = np.arange(n_out, dtype=np.int64)
    nt, r = (t * M) // L, (t * M) % L
    below = (r == 0) & (t / (float(target_sr) / orig_sr) < nt)
    r, nt = np.where(below, L, r), np.where(below, nt - 1, nt)
    xp = np.concatenate([np.zeros(left + 1), np.asarray(x, np.float64), np.zeros(K + 1)])
    idx = 1 + nt[:, None] + np.arange(K)[None, :]      # index into xp (shifted by `left` + 1)
    y = (bank[r].astype(np.float64) * xp[idx]).sum(axis=1) if n_out else np.zeros(0)
    return _fix_length(y, out_len(n_in, orig_sr, target_sr))

