"""Reference of a turn's timeline, independent of `wire.assemble_turn` and `wire.TurnPlan`: the assembly
restated in NumPy fp32, and a brute-force readiness that walks every tap of every output."""
import math

import numpy as np


def starts(lengths, pauses):
    """p_0 = 0, p_{s+1} = p_s + n_s + pauses[s]"""
    p, out = 0, []
    for s, n in enumerate(lengths):
        if s:
            p += pauses[s - 1]
        out.append(p)
        p += n
    return out


def ramp_gain(n, ramp):
    """fp32 gains of a segment of n samples (1 where there is no ramp), and where they apply."""
    k = min(int(ramp), n // 2)
    g = np.ones(n, np.float32)
    on = np.zeros(n, bool)
    if k:
        inv = np.float32(1.0) / np.float32(k + 1)
        for i in range(k):
            g[i] = np.float32(i + 1) * inv
            g[n - k + i] = np.float32(k - i) * inv
            on[i] = on[n - k + i] = True
    return g, on


def assemble(waves, lengths, pauses, ramp):
    """The timeline as one fp32 row: every segment times its ramps (one fp32 multiply), zeros in the pauses."""
    p = starts(lengths, pauses)
    out = np.zeros(p[-1] + lengths[-1], np.float32)
    for w, n, a in zip(waves, lengths, p):
        w = np.asarray(w, np.float32).reshape(-1)[:n]
        g, on = ramp_gain(n, ramp)
        out[a:a + n] = np.where(on, w * g, w)
    return out


def frontier(lengths, pauses, avail, closed):
    """The contiguous decoded prefix of the timeline, sample by sample: a pause is decoded once the segment behind it
    exists, and nothing exists behind the last segment's end while the turn is open."""
    p = starts(lengths, pauses) if lengths else []
    end = p[-1] + lengths[-1] if lengths else 0
    exists = np.zeros(end, bool)
    for s, (a, n, have) in enumerate(zip(p, lengths, avail)):
        exists[a:a + have] = True
        if s:
            exists[p[s - 1] + lengths[s - 1]:a] = True
    missing = np.flatnonzero(~exists)
    return int(missing[0]) if len(missing) else end


def ref_tap_span(orig_sr, target_sr, res_type):
    """(taps to the left of n_t, n_t included; taps to the right) that resampy's loop can touch at most, from the
    restatement in tests/resample_ref.py: a geometry (K, left) must cover x[n_t - lmax + 1 .. n_t + rmax]."""
    import resample_ref
    win, _, _, _, step, _ = resample_ref._setup(orig_sr, target_sr, res_type)
    return len(win) // step, len(win) // step


def taps_of(t, L, M, K, left):
    """Timeline indices output t may read (the bank's row L reads one sample earlier); equal rates (K = 0): t itself."""
    if K == 0:
        return t, t
    nt = (t * M) // L
    return nt - left - 1, nt - left + K - 1


def ready_brute(front, total, geom, model_sr, rate, lookahead, complete, cap):
    """Final outputs by brute force: u is final iff every tap of every resampled sample in [u, u + lookahead] lies below
    the frontier; everything once the turn is complete."""
    if complete:
        return int(math.ceil(total * (float(rate) / model_sr)))
    L, M, K, left = geom
    u = 0
    while u < cap:
        hi = taps_of(u + lookahead, L, M, K, left)[1]
        if hi >= front:
            break
        u += 1
    if total is not None:
        u = min(u, max(int(math.ceil(total * (float(rate) / model_sr))) - lookahead, 0))
    return u
