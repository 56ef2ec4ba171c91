"""NumPy restatement of G.711 as CPython 3.10's `audioop` computes it at width 2 (`lin2ulaw`, `lin2alaw`, `ulaw2lin`,
`alaw2lin`: the arithmetic of Sun's g711.c), vectorised.  The reference every G.711 test applies to int16 results;
itself pinned to tables written from `audioop` (tests/golden/g711_tables.npz, tests/test_g711.py).

  mu-law  s >> 2, magnitude clipped to 8159, + 33; segment = first i with v <= (0x40 << i) - 1; all bits inverted
  A-law   s >> 3, negative: -v - 1; segment = first i with v <= (0x20 << i) - 1; even bits inverted
"""
import numpy as np

LAWS = ("ulaw", "alaw")
ZERO = {"ulaw": 0xFF, "alaw": 0xD5}          # encode(0): what the wire kernels store where the int16 path stores 0

_UEND = np.array([0x3F, 0x7F, 0xFF, 0x1FF, 0x3FF, 0x7FF, 0xFFF, 0x1FFF], np.int64)
_AEND = np.array([0x1F, 0x3F, 0x7F, 0xFF, 0x1FF, 0x3FF, 0x7FF, 0xFFF], np.int64)


def _check_law(law):
    if law not in LAWS:
        raise ValueError("law must be 'ulaw' or 'alaw', got %r" % (law,))


def _pcm(pcm):
    pcm = np.asarray(pcm)
    if pcm.dtype != np.int16:
        raise ValueError("encode takes int16 samples, got %s" % pcm.dtype)
    return pcm.astype(np.int64)


def lin2ulaw(pcm):
    v = _pcm(pcm) >> 2
    mask = np.where(v < 0, 0x7F, 0xFF)
    v = np.minimum(np.abs(v), 8159) + 33
    seg = np.searchsorted(_UEND, v, side="left")             # first i with v <= _UEND[i]; 8 past the table
    code = (seg << 4) | ((v >> (seg + 1)) & 0xF)
    return (np.where(seg >= 8, 0x7F, code) ^ mask).astype(np.uint8)


def lin2alaw(pcm):
    v = _pcm(pcm) >> 3
    mask = np.where(v < 0, 0x55, 0xD5)
    v = np.where(v < 0, -v - 1, v)
    seg = np.searchsorted(_AEND, v, side="left")
    code = (seg << 4) | ((v >> np.where(seg < 2, 1, seg)) & 0xF)
    return (np.where(seg >= 8, 0x7F, code) ^ mask).astype(np.uint8)


def _bytes(data):
    data = np.asarray(data)
    if data.dtype != np.uint8:
        raise ValueError("decode takes uint8 bytes, got %s" % data.dtype)
    return data.astype(np.int64)


def ulaw2lin(data):
    u = ~_bytes(data) & 0xFF
    t = (((u & 0xF) << 3) + 0x84) << ((u & 0x70) >> 4)
    return np.where(u & 0x80, 0x84 - t, t - 0x84).astype(np.int16)


def alaw2lin(data):
    a = _bytes(data) ^ 0x55
    seg = (a & 0x70) >> 4
    t = (a & 0xF) << 4
    t = np.where(seg == 0, t + 8, (t + 0x108) << np.maximum(seg - 1, 0))
    return np.where(a & 0x80, t, -t).astype(np.int16)


def encode(pcm, law):
    """int16 array (any shape) -> uint8 array of the same shape"""
    _check_law(law)
    return lin2ulaw(pcm) if law == "ulaw" else lin2alaw(pcm)


def decode(data, law):
    """uint8 array (any shape) -> int16 array of the same shape"""
    _check_law(law)
    return ulaw2lin(data) if law == "ulaw" else alaw2lin(data)
