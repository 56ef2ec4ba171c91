"""Per-token volume restated in NumPy float32: the frame gains a row's tokens give its z-frames, and the
envelope the wire kernels multiply into the model-rate samples.  Every operation is one float32 operation with one
rounding, in the order the header states, so the kernels are compared with this BITWISE."""
import numpy as np

GAIN_MAX = 16.0


def gain_of_db(db):
    """10 ** (db / 20) in Python floats, then fp32; -inf gives 0"""
    if db == float("-inf"):
        return 0.0
    return float(np.float32(10.0 ** (float(db) / 20.0)))


def frame_gain(gain, cum, y, frames):
    """One row: gain [T] fp32, cum [T] the INCLUSIVE sums of the durations the length regulator used, y the row's kept
    frames (negative: the row is flagged), frames = F of the stream -> G fp32 [F + 1].
      G[t] = gain[j(t)] for t < y, j(t) the first token with cum[j] > t (tokens of zero frames are skipped by the rule)
      G[t] = G[y - 1] for y <= t <= F;   all 1.0 for a flagged row, y = 0, and a frame no token holds"""
    gain = np.asarray(gain, np.float32)
    cum = np.asarray(cum, np.int64)
    G = np.ones(frames + 1, np.float32)
    y = min(int(y), frames)
    if y <= 0:
        return G
    for t in range(frames + 1):
        tt = min(t, y - 1)
        j = int(np.searchsorted(cum, tt, side="right"))       # first j with cum[j] > tt
        if j < len(cum):
            G[t] = gain[j]
    return G


def frame_gain_of_marks(gain, marks, frames):
    """The same from a stream's token marks (exclusive sums, the last entry the total, all clipped to the kept frames)"""
    marks = [int(m) for m in marks]
    return frame_gain(gain, marks[1:], marks[-1], frames)


def envelope(G, hop, n):
    """e(j) for j < n <= (len(G) - 1) * hop: G[f] + w * (G[f + 1] - G[f]), f = j // hop, w = fp32(j - f hop) * inv_hop"""
    G = np.asarray(G, np.float32)
    hop = int(hop)
    assert hop >= 1 and n <= (len(G) - 1) * hop
    j = np.arange(n, dtype=np.int64)
    f = j // hop
    r = (j - f * hop).astype(np.float32)
    inv_hop = np.float32(1.0) / np.float32(hop)
    w = r * inv_hop
    d = G[f + 1] - G[f]
    e = G[f] + w * d
    assert e.dtype == np.float32
    return e


def shaped(x, G, hop):
    """x fp32 [n] -> fp32 [n]: every sample times its envelope value, rounded once"""
    x = np.asarray(x, np.float32)
    return x * envelope(G, hop, x.shape[-1])
