"""Float64 restatement of the wire step's look-ahead limiter, straight from its definition and with
nothing of the kernel's scheme in it: a window minimum taken over the window itself, a plain mean.

    r[t] = |v[t]| > c ? c / |v[t]| : 1                      v is zero outside [0, len(v))
    m[j] = min r[k], k in [j - H, j + L]
    g[t] = (m[t - L] + ... + m[t]) / (L + 1)
    y[t] = v[t] g[t], then clip to [-1, 1], * 32767, truncate towards zero
"""
import numpy as np


def gain(v, ceiling, lookahead, hold):
    """(g, m, r) float64, each [len(v)]: the gain of every sample, the window minima m[j] and the ratios r[t] for
    j, t in [0, len(v)); outside that range r = 1, so m and g there are whatever the windows reach."""
    v = np.asarray(v, dtype=np.float64)
    n, L, H = len(v), int(lookahead), int(hold)
    a = np.abs(v)
    r = np.where(a > ceiling, ceiling / np.where(a > ceiling, a, 1.0), 1.0)
    # m[j] for j in [-L, n): rp[i] = r[i - (L + H)], ones outside the row
    rp = np.concatenate([np.ones(L + H), r, np.ones(L)])
    m_ext = np.array([rp[i:i + H + L + 1].min() for i in range(n + L)])       # m_ext[i] = m[i - L]
    g = np.array([m_ext[t:t + L + 1].sum() for t in range(n)]) / float(L + 1)
    return g, m_ext[L:], r


def limit(v, ceiling, lookahead, hold):
    """y float64 [len(v)]: the limited samples, before the clip."""
    return np.asarray(v, dtype=np.float64) * gain(v, ceiling, lookahead, hold)[0]


def pcm16(v, ceiling, lookahead, hold):
    """int16 [len(v)]: the limited samples through the wire epilogue (clip, * 32767, truncate)."""
    y = np.clip(limit(v, ceiling, lookahead, hold), -1.0, 1.0) * 32767.0
    return np.trunc(y).astype(np.int16)
