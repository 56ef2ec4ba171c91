"""CPU: G.711 on the wire.  The NumPy reference of the codec (tests/g711_ref.py) against tables written
from CPython's `audioop` (tests/golden/g711_tables.npz) and, where it still imports, against `audioop` itself; the
framing of byte streams; the new C entries' declarations; the keyword refusals that need no GPU."""
import base64
import os
import re

import numpy as np
import pytest
import torch

from mb_istft_vits_amd import _capi, models, wire

import g711_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL16 = np.arange(-32768, 32768).astype(np.int16)         # table index s + 32768
ALL8 = np.arange(256).astype(np.uint8)


@pytest.fixture(scope="module")
def tables():
    t = np.load(os.path.join(ROOT, "tests", "golden", "g711_tables.npz"))
    assert t["ulaw_encode"].shape == t["alaw_encode"].shape == (65536,) and t["ulaw_encode"].dtype == np.uint8
    assert t["ulaw_decode"].shape == t["alaw_decode"].shape == (256,) and t["ulaw_decode"].dtype == np.int16
    return t


@pytest.mark.parametrize("law", g711_ref.LAWS)
def test_reference_equals_the_committed_tables(tables, law):
    assert np.array_equal(g711_ref.encode(ALL16, law), tables[law + "_encode"])
    assert np.array_equal(g711_ref.decode(ALL8, law), tables[law + "_decode"])
    got = g711_ref.encode(ALL16.reshape(256, 256), law)            # any shape
    assert got.shape == (256, 256) and got.dtype == np.uint8


def test_reference_equals_audioop():
    audioop = pytest.importorskip("audioop")
    pcm, codes = ALL16.astype("<i2").tobytes(), ALL8.tobytes()
    assert g711_ref.encode(ALL16, "ulaw").tobytes() == audioop.lin2ulaw(pcm, 2)
    assert g711_ref.encode(ALL16, "alaw").tobytes() == audioop.lin2alaw(pcm, 2)
    assert g711_ref.decode(ALL8, "ulaw").astype("<i2").tobytes() == audioop.ulaw2lin(codes, 2)
    assert g711_ref.decode(ALL8, "alaw").astype("<i2").tobytes() == audioop.alaw2lin(codes, 2)


def test_known_answers():
    enc = {0: (0xFF, 0xD5), -1: (0x7E, 0x55), 4: (0xFE, None), 1000: (0xCE, 0xFA), -1000: (0x4E, 0x7A),
           32767: (0x80, 0xAA), -32768: (0x00, 0x2A)}
    for s, (u, a) in enc.items():
        x = np.array([s], np.int16)
        assert int(g711_ref.encode(x, "ulaw")[0]) == u, s
        if a is not None:
            assert int(g711_ref.encode(x, "alaw")[0]) == a, s
    for b, v in {0x00: -32124, 0x7F: 0, 0x80: 32124, 0xFF: 0}.items():
        assert int(g711_ref.decode(np.array([b], np.uint8), "ulaw")[0]) == v, b
    for b, v in {0x55: -8, 0xD5: 8, 0x2A: -32256, 0xAA: 32256}.items():
        assert int(g711_ref.decode(np.array([b], np.uint8), "alaw")[0]) == v, b
    assert g711_ref.ZERO == wire.G711_ZERO == {"ulaw": 0xFF, "alaw": 0xD5}


@pytest.mark.parametrize("law", g711_ref.LAWS)
def test_round_trip(law):
    back = g711_ref.encode(g711_ref.decode(ALL8, law), law)
    want = ALL8.copy()
    if law == "ulaw":
        want[0x7F] = 0xFF                      # negative zero decodes to 0, which encodes as positive zero
    assert np.array_equal(back, want)


def test_reference_refuses_other_types_and_laws():
    with pytest.raises(ValueError, match="law"):
        g711_ref.encode(ALL16, "mulaw")
    with pytest.raises(ValueError, match="int16"):
        g711_ref.encode(ALL16.astype(np.int32), "ulaw")
    with pytest.raises(ValueError, match="uint8"):
        g711_ref.decode(ALL16, "alaw")


# ------------------------------------------------------------------------------------------------ framing
def _bytes(n, seed=0):
    return np.random.RandomState(seed).randint(0, 256, size=n).astype(np.uint8)


def test_frame_g711_cuts_160_byte_frames_at_8_khz():
    data = _bytes(1000)
    frames = wire.frame_g711(data, 8000)
    assert wire.chunk_size(8000) == 160
    assert [len(base64.b64decode(f)) for f in frames] == [160] * 6 + [40]          # the short last frame
    assert b"".join(base64.b64decode(f) for f in frames) == data.tobytes()
    assert wire.frame_g711(torch.from_numpy(data), 8000) == frames
    assert wire.frame_g711(data, 8000, valid_samples=320) == frames[:2]
    assert wire.frame_g711(data[:0], 8000) == []
    assert len(wire.frame_g711(data, 8000, frame_length=0.03)[0]) == len(base64.b64encode(bytes(240)))
    with pytest.raises(ValueError, match="uint8"):
        wire.frame_g711(data.astype(np.int16), 8000)
    with pytest.raises(ValueError, match="uint8"):
        wire.frame_g711(data.reshape(2, 500), 8000)
    with pytest.raises(ValueError, match="at least one sample"):
        wire.frame_g711(data, 8000, frame_length=0.0)


@pytest.mark.parametrize("cuts", [[1000], [1, 159, 160, 161, 0, 319, 200], [7] * 142 + [6]])
def test_frame_cutter_of_pushed_bytes_equals_the_frames_of_the_concatenation(cuts):
    data = _bytes(sum(cuts), 1)
    want = wire.frame_g711(data, 8000)
    fc = wire.FrameCutter(8000, sample_bytes=1)
    assert fc.n == 160
    got, off = [], 0
    for i, k in enumerate(cuts):
        piece = data[off:off + k]
        got += fc.push(torch.from_numpy(piece) if i % 2 else piece)
        off += k
    got += fc.close()
    assert got == want and fc.close() == []
    assert len(base64.b64decode(got[-1])) == sum(cuts) % 160 or sum(cuts) % 160 == 0


def test_frame_cutter_keeps_its_int16_form_and_refuses_the_wrong_sample_type():
    pcm = np.arange(-500, 500).astype(np.int16)
    fc = wire.FrameCutter(8000)                             # sample_bytes=2: frames of 160 int16 = 320 bytes
    frames = fc.push(pcm) + fc.close()
    assert frames == wire.frame_pcm16(pcm, 8000) and len(base64.b64decode(frames[0])) == 320
    with pytest.raises(ValueError, match="int16"):
        wire.FrameCutter(8000).push(_bytes(10))
    with pytest.raises(ValueError, match="uint8"):
        wire.FrameCutter(8000, sample_bytes=1).push(pcm)
    with pytest.raises(ValueError, match="sample_bytes"):
        wire.FrameCutter(8000, sample_bytes=4)


# ------------------------------------------------------------------------------------------------ the C surface
def test_new_entries_are_declared_exported_and_numbered():
    hdr = open(os.path.join(ROOT, "include", "mbistft_vits.h")).read()
    L = _capi.lib()
    for sym in ("mbv_g711_encode", "mbv_g711_decode", "mbv_resample_g711_range", "mbv_resample_g711_chunks"):
        assert re.search(r"\bint %s\(mbv_model \*m," % sym, hdr), sym
        assert sym in _capi.SYMBOLS and getattr(L, sym) is not None
    defines = dict(re.findall(r"#define (MBV_(?:G711|WAVE)_[A-Z0-9]+)\s+(\d+)", hdr))
    assert {k: int(v) for k, v in defines.items()} == {"MBV_G711_ULAW": 1, "MBV_G711_ALAW": 2, "MBV_WAVE_F32": 0,
                                                       "MBV_WAVE_PCM16": 1, "MBV_WAVE_ULAW": 8, "MBV_WAVE_ALAW": 9}
    assert _capi.G711_LAWS == {"ulaw": 1, "alaw": 2} and (_capi.WAVE_ULAW, _capi.WAVE_ALAW) == (8, 9)
    assert L.mbv_abi_version() == 3                         # added entries, no struct changed
    # without a handle the entries fail instead of launching
    assert L.mbv_g711_encode(None, None, 0, 1, None, None) != 0
    assert L.mbv_resample_g711_chunks(None, None, None, 0, 22050, 8000, 0, 1, None, 0, None) != 0


# ------------------------------------------------------------------------------------------------ keywords
def test_keyword_refusals_that_need_no_gpu():
    assert models.ENCODINGS == ("pcm16", "ulaw", "alaw")
    o = torch.zeros(1, 1, 512)
    for bad in ("mulaw", "g711", None, 1):
        with pytest.raises(ValueError, match="encoding"):
            wire.service_pcm16(None, o, None, 22050, 8000, encoding=bad)
        with pytest.raises(ValueError, match="encoding"):
            wire.PcmPool(None, None, 22050, 8000, encoding=bad)
        with pytest.raises(ValueError, match="encoding"):
            wire.LiveWire(None, 0, 1, 8000, 22050, 8000, 256, 1024, 8000, encoding=bad)
        with pytest.raises(ValueError, match="encoding"):
            wire.convert_pcm16(None, torch.zeros(1, 800, dtype=torch.int16), None, 0, 1, 8000, 22050, 8000, 256, 1024,
                               encoding=bad)
    live = (None, 0, 1)
    # G.711 input always goes through the resampler
    with pytest.raises(ValueError, match="in_sr != model_sr"):
        wire.convert_live_pcm16(*live, 22050, 22050, 8000, 256, 1024, 8000, dtype=torch.uint8, in_encoding="ulaw")
    with pytest.raises(ValueError, match="in_sr != model_sr"):
        wire.convert_pcm16(None, torch.zeros(1, 800, dtype=torch.uint8), None, 0, 1, 22050, 22050, 8000, 256, 1024,
                           in_encoding="alaw")
    with pytest.raises(ValueError, match="law"):
        wire.convert_live_pcm16(*live, 8000, 22050, 8000, 256, 1024, 8000, dtype=torch.uint8, in_encoding="pcm16")
    # dtype and in_encoding go together
    with pytest.raises(TypeError, match="in_encoding"):
        wire.convert_live_pcm16(*live, 8000, 22050, 8000, 256, 1024, 8000, dtype=torch.uint8)
    with pytest.raises(TypeError, match="in_encoding"):
        wire.convert_live_pcm16(*live, 8000, 22050, 8000, 256, 1024, 8000, dtype=torch.int16, in_encoding="ulaw")
    with pytest.raises(TypeError, match="in_encoding"):
        wire.convert_pcm16(None, torch.zeros(1, 800, dtype=torch.int16), None, 0, 1, 8000, 22050, 8000, 256, 1024,
                           in_encoding="ulaw")
    with pytest.raises(TypeError, match="in_encoding"):
        wire.convert_pcm16(None, torch.zeros(1, 800, dtype=torch.uint8), None, 0, 1, 8000, 22050, 8000, 256, 1024)
    with pytest.raises(TypeError, match="int16 or float32"):                         # as before
        wire.convert_live_pcm16(*live, 8000, 22050, 8000, 256, 1024, 8000, dtype=torch.float64)
