"""Plain-integer restatement of the seeded noise generator: Philox4x32-10 on Python ints, the
Box-Muller transform in float64 with exact math.log / cos / sin.  What `mbv_randn_host` and `mbv_randn_blocks` are
measured against; it shares no code with them."""
import math

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57             # Philox multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85             # Weyl constants
MASK = 0xFFFFFFFF
PRIOR, SDP, POSTERIOR = 0, 1, 2             # the `purpose` word of the counter


def philox4x32_10(counter, key):
    """(c0, c1, c2, c3), (k0, k1) -> the four output words after ten rounds."""
    c0, c1, c2, c3 = (int(v) & MASK for v in counter)
    k0, k1 = (int(v) & MASK for v in key)
    for r in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & MASK, p1 & MASK, ((p0 >> 32) ^ c3 ^ k1) & MASK, p0 & MASK
        if r < 9:
            k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def words(seed, purpose, row, c, block):
    """The four words of frames 4 block .. 4 block + 3 of channel c."""
    seed = int(seed)
    assert 0 <= seed < 1 << 64
    return philox4x32_10((block, c, purpose, row), (seed & MASK, seed >> 32))


def normals_of(w):
    """Four words -> four float64 normals: (w0, w1) -> (n0, n1), (w2, w3) -> (n2, n3)."""
    out = []
    for wa, wb in ((w[0], w[1]), (w[2], w[3])):
        u1 = ((wa >> 8) + 1) * 2.0 ** -24
        u2 = (wb >> 8) * 2.0 ** -24
        r = math.sqrt(-2.0 * math.log(u1))
        out += [r * math.cos(2.0 * math.pi * u2), r * math.sin(2.0 * math.pi * u2)]
    return out


def randn_row(seed, purpose, row, c, first, count):
    """float64 [count]: frames [first, first + count) of channel c; element t is lane t & 3 of block t >> 2."""
    out = np.empty(count, dtype=np.float64)
    block, lanes = None, None
    for i in range(count):
        t = first + i
        if t >> 2 != block:
            block = t >> 2
            lanes = normals_of(words(seed, purpose, row, c, block))
        out[i] = lanes[t & 3]
    return out


def randn(seed, channels, frames, purpose=0, row=0, first=0):
    """float64 [channels, frames], what `net.randn` returns in fp32."""
    return np.stack([randn_row(seed, purpose, row, c, first, frames) for c in range(channels)]) if channels else \
        np.empty((0, frames))
