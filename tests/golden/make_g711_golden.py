"""Generate the G.711 fixture (g711_tables.npz) from CPython's `audioop` (3.10; the module left the standard library
in 3.13, which is why the tables are committed):

    python tests/golden/make_g711_golden.py

  ulaw_encode, alaw_encode  uint8 [65536]: audioop.lin2ulaw / lin2alaw at width 2 of every int16, index s + 32768
  ulaw_decode, alaw_decode  int16 [256]:   audioop.ulaw2lin / alaw2lin at width 2 of every byte

Only data is stored.  tests/test_g711.py pins tests/g711_ref.py to these tables, and the GPU tests pin the kernels to
g711_ref.
"""
import audioop
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def tables():
    pcm = np.arange(-32768, 32768, dtype=np.int64).astype("<i2").tobytes()
    codes = bytes(range(256))
    return {
        "ulaw_encode": np.frombuffer(audioop.lin2ulaw(pcm, 2), np.uint8).copy(),
        "alaw_encode": np.frombuffer(audioop.lin2alaw(pcm, 2), np.uint8).copy(),
        "ulaw_decode": np.frombuffer(audioop.ulaw2lin(codes, 2), "<i2").astype(np.int16),
        "alaw_decode": np.frombuffer(audioop.alaw2lin(codes, 2), "<i2").astype(np.int16),
    }


if __name__ == "__main__":
    out = os.path.join(HERE, "g711_tables.npz")
    np.savez_compressed(out, **tables())
    print("wrote %s (%d bytes)" % (out, os.path.getsize(out)))
