"""CPU-only checks of per-token volume: the NumPy restatement of the frame gains and the envelope
(tests/gain_ref.py) against hand-computed cases, `gain_of_db`, every refusal the host makes before anything is launched
(on `Request`, `Envelope` and the live wires), and the ctypes mirrors of the new C structs.  No GPU is touched."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

from mb_istft_vits_amd import _capi, models, wire
from mb_istft_vits_amd.models import Request

import gain_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the definition
def test_all_ones_is_exactly_one():
    G = gain_ref.frame_gain([1.0] * 4, [2, 2, 5, 6], 6, 9)
    assert G.dtype == np.float32 and G.shape == (10,) and (G == 1.0).all()
    for hop in (1, 100, 256):
        e = gain_ref.envelope(G, hop, 9 * hop)
        assert e.dtype == np.float32 and (e.view(np.int32) == np.float32(1.0).view(np.int32)).all()
        x = np.random.RandomState(0).uniform(-2, 2, 9 * hop).astype(np.float32)
        assert np.array_equal(gain_ref.shaped(x, G, hop).view(np.int32), x.view(np.int32))


def test_frame_gains_follow_the_length_regulator():
    gain = [0.5, 3.0, 2.0, 0.25]
    # durations 2, 0, 3, 1: the zero-length token 1 holds no frame
    G = gain_ref.frame_gain(gain, [2, 2, 5, 6], 6, 6)
    assert G.tolist() == [0.5, 0.5, 2.0, 2.0, 2.0, 0.25, 0.25]          # entry F holds the last kept frame's gain
    # the max_len clip: 4 frames kept of 6, in a stream of 4
    G = gain_ref.frame_gain(gain, [2, 2, 5, 6], 4, 4)
    assert G.tolist() == [0.5, 0.5, 2.0, 2.0, 2.0]
    # hold behind y: a short row inside a longer stream
    G = gain_ref.frame_gain(gain, [2, 2, 5, 6], 6, 9)
    assert G.tolist() == [0.5, 0.5, 2.0, 2.0, 2.0, 0.25, 0.25, 0.25, 0.25, 0.25]
    G = gain_ref.frame_gain(gain, [2, 2, 5, 6], 3, 9)
    assert G.tolist() == [0.5, 0.5, 2.0] + [2.0] * 7
    # a flagged row, no frames, and durations that are all zero
    assert (gain_ref.frame_gain(gain, [2, 2, 5, 6], -1, 5) == 1.0).all()
    assert (gain_ref.frame_gain(gain, [2, 2, 5, 6], 0, 5) == 1.0).all()
    assert (gain_ref.frame_gain(gain, [0, 0, 0, 0], 1, 3) == 1.0).all()
    # token marks (exclusive sums, clipped to the kept frames) give the same table
    assert gain_ref.frame_gain_of_marks(gain, [0, 2, 2, 4, 4], 4).tolist() == [0.5, 0.5, 2.0, 2.0, 2.0]


@pytest.mark.parametrize("hop", [1, 3, 100, 256])
def test_envelope_reaches_a_frames_gain_at_its_first_sample(hop):
    G = np.asarray([0.5, 0.5, 2.0, 1e-3, 0.0, 4.0, 4.0], np.float32)
    F = len(G) - 1
    e = gain_ref.envelope(G, hop, F * hop)
    assert np.array_equal(e[::hop], G[:F])                              # e(f * hop) == G[f] exactly (w = 0)
    inv = np.float32(1.0) / np.float32(hop)
    for f in range(F):
        for r in {0, min(1, hop - 1), hop // 2, hop - 1}:
            w = np.float32(r) * inv
            want = np.float32(G[f] + np.float32(w * np.float32(G[f + 1] - G[f])))
            assert e[f * hop + r].view(np.int32) == want.view(np.int32)
        lo, hi = min(G[f], G[f + 1]), max(G[f], G[f + 1])
        seg = e[f * hop:(f + 1) * hop]
        assert (seg >= lo).all() and (seg <= hi).all()                  # continuous: it never leaves the two gains
    assert (e[:hop] == 0.5).all()                                       # inside a token: flat
    with pytest.raises(AssertionError):
        gain_ref.envelope(G, hop, F * hop + 1)


def test_gain_of_db():
    assert models.gain_of_db(0) == 1.0 and models.gain_of_db(-math.inf) == 0.0
    for db in (-60.0, -6.0, -3.0, 6.0, 20.0, 24.0):
        want = float(np.float32(10.0 ** (db / 20.0)))
        assert models.gain_of_db(db) == want == gain_ref.gain_of_db(db)
    assert models.gain_of_db(24.0) < models.GAIN_MAX == gain_ref.GAIN_MAX == 16.0 < models.gain_of_db(24.1)
    assert wire.gain_of_db is models.gain_of_db and wire.GAIN_MAX == 16.0
    for bad in (math.nan, math.inf):
        with pytest.raises(ValueError):
            models.gain_of_db(bad)


# ------------------------------------------------------------------------------------------------ refusals on the host
def test_request_checks_the_gains():
    ids = [3, 4, 5, 6]
    r = Request(ids, gain=[0.0, 1.0, 16.0, 1e-3])
    assert r.gain.dtype == torch.float32 and r.gain.tolist() == [0.0, 1.0, 16.0, float(np.float32(1e-3))]
    assert not r.gain.is_cuda and Request(ids).gain is None
    assert Request(ids, gain=torch.tensor([[1.0, 2.0, 3.0, 4.0]], dtype=torch.float64)).gain.shape == (4,)
    assert Request(ids, gain=np.asarray([1, 2, 3, 4])).gain.tolist() == [1.0, 2.0, 3.0, 4.0]
    for bad in ([1.0] * 3, [1.0] * 5, [[1.0] * 4] * 2, [1.0, math.nan, 1.0, 1.0], [1.0, math.inf, 1.0, 1.0],
                [1.0, -0.5, 1.0, 1.0], [1.0, 16.5, 1.0, 1.0], torch.tensor([1.0, 1.0, 1.0, -1e-9])):
        with pytest.raises(ValueError):
            Request(ids, gain=bad)
    for bad in ("loud", [True, False, True, True], torch.tensor([True] * 4), ["a", "b", "c", "d"],
                torch.ones(4, dtype=torch.complex64)):
        with pytest.raises(TypeError):
            Request(ids, gain=bad)
    # the same check serves the batched entries
    assert models._gain_arg("infer", [[1.0, 2.0], [0.5, 0.0]], 2, 2).shape == (2, 2)
    with pytest.raises(ValueError):
        models._gain_arg("infer", [1.0, 2.0], 2, 2)


def _envelope(frames, hop, rows=1):
    """an `Envelope` without its device tensor: the integer checks need none"""
    e = wire.Envelope.__new__(wire.Envelope)
    e.gain, e.hop, e.frames, e.rows = None, hop, frames, rows
    return e


def test_envelope_checks_its_arguments():
    g = torch.ones(9)
    for bad_hop in (0, -1, 1 << 31):
        with pytest.raises(ValueError):
            wire.Envelope(g, bad_hop)
    for bad_hop in (256.0, True, "256", None):
        with pytest.raises(TypeError):
            wire.Envelope(g, bad_hop)
    with pytest.raises(TypeError):
        wire.Envelope([1.0] * 9, 256)                                   # not a tensor
    with pytest.raises(TypeError):
        wire.Envelope(g.double(), 256)                                  # not fp32
    with pytest.raises(TypeError):
        wire.Envelope(g, 256)                                           # not on the device: the kernels read it in place
    # frames * hop must cover the row; one row per row of the call
    _envelope(8, 256).check("t", 1, 2048)
    for frames, hop, rows, samples in ((8, 256, 1, 2049), (7, 256, 1, 2048), (20, 100, 1, 2001), (8, 256, 2, 2048)):
        with pytest.raises(ValueError):
            _envelope(frames, hop).check("t", rows, samples)


def test_live_wires_refuse_an_envelope_before_anything_else():
    """A converted recording has no tokens: `envelope=` is refused on every live entry, before any argument is looked
    at (no model, no device)."""
    env = _envelope(8, 256)
    with pytest.raises(ValueError, match="envelope"):
        wire.convert_pcm16(None, None, None, 0, 1, 16000, 22050, 24000, 256, 1024, envelope=env)
    with pytest.raises(ValueError, match="envelope"):
        wire.convert_live_pcm16(None, 0, 1, 16000, 22050, 24000, 256, 1024, 1000, envelope=env)
    with pytest.raises(ValueError, match="envelope"):
        wire.LiveWire(None, 0, 1, 16000, 22050, 24000, 256, 1024, 1000, envelope=env)
    with pytest.raises(ValueError, match="envelope"):
        wire.PcmPool.add_live(None, None, envelope=env)
    with pytest.raises(TypeError):
        wire.service_pcm16(None, None, None, 22050, 24000, envelope=[1.0, 2.0])
    with pytest.raises(TypeError):
        wire._envelope_arg("not an envelope", None, "t")


# ------------------------------------------------------------------------------------------------ the C structs
def _fields(name):
    hdr = open(os.path.join(ROOT, "include", "mbistft_vits.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    types = {"int64_t": C.c_int64, "int32_t": C.c_int32, "float": C.c_float}
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype = C.c_void_p if "*" in decl else types[decl.split()[0]]
        for part in decl.replace("*", " ").split(","):
            fields.append((part.split()[-1], ctype))
    return fields


def test_struct_layouts_match_the_header():
    assert [(n, t) for n, t in _capi.MbvPcmEnvelope._fields_] == _fields("mbv_pcm_envelope")
    assert [n for n, _ in _capi.MbvPcmEnvelope._fields_] == ["gain", "frames", "hop", "inv_hop"]
    assert C.sizeof(_capi.MbvPcmEnvelope) == 24
    assert [getattr(_capi.MbvPcmEnvelope, n).offset for n, _ in _capi.MbvPcmEnvelope._fields_] == [0, 8, 16, 20]
    assert [(n, t) for n, t in _capi.MbvGainRow._fields_] == _fields("mbv_gain_row")
    assert C.sizeof(_capi.MbvGainRow) == 24
    assert [getattr(_capi.MbvGainRow, n).offset for n, _ in _capi.MbvGainRow._fields_] == [0, 8, 16, 20]
    for s in ("mbv_frame_gain", "mbv_frame_gain_rows", "mbv_op_frame_gain", "mbv_gain_runs",
              "mbv_resample_pcm16_range_shaped", "mbv_resample_pcm16_chunks_shaped", "mbv_resample_turns_shaped"):
        assert s in _capi.SYMBOLS
    # the structs the wire tables already had do not change
    assert C.sizeof(_capi.MbvPcmChunk) == 88 and C.sizeof(_capi.MbvPcmFade) == 24 and C.sizeof(_capi.MbvPcmLimit) == 12
    assert C.sizeof(_capi.MbvTurnSeg) == 32
