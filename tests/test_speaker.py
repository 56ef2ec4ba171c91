"""Blended voices, host side (no GPU): the float64 reference, the weights `net.speaker` sends, the slot bookkeeping,
what `Speaker` gives the host entries, and the C entries' declarations."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from mb_istft_vits_amd import _capi, models

import speaker_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mbv_speakers_define", "mbv_speaker_release", "mbv_speaker_slots", "mbv_speaker_defined", "mbv_speaker_runs"]


# ------------------------------------------------------------------ the reference
def test_ref_blend_known_answers():
    table = np.array([[1.0, 2.0, -4.0], [3.0, 0.5, 8.0], [-2.0, 0.0, 1.0]])
    assert np.array_equal(speaker_ref.blend(table, [1], [1.0]), table[1])
    assert np.array_equal(speaker_ref.blend(table, [0, 1], [0.5, 0.5]), [2.0, 1.25, 2.0])
    assert np.array_equal(speaker_ref.blend(table, [0, 2], [1.5, -0.5]), [2.5, 3.0, -6.5])
    assert np.array_equal(speaker_ref.blend(table, [2, 1, 0], [0.0, 1.0, 0.0]), table[1])
    assert speaker_ref.blend(table.astype(np.float32), [0], [1]).dtype == np.float64
    # the bound: K 2^-23 sum |w e|
    assert np.array_equal(speaker_ref.bound(table, [0, 2], [1.5, -0.5]), 2 * 2.0 ** -23 * np.array([2.5, 3.0, 6.5]))


# ------------------------------------------------------------------ blend_weights
def test_blend_weights_normalise():
    assert models.blend_weights([1.0]) == [1.0]
    assert models.blend_weights([2, 2]) == [0.5, 0.5]
    assert models.blend_weights([1, 3]) == [0.25, 0.75]
    assert models.blend_weights([0, 5, 0]) == [0.0, 1.0, 0.0]                  # one-hot stays exact
    assert models.blend_weights([3, -1]) == [1.5, -0.5]                        # a negative entry with a positive sum
    w = models.blend_weights([0.7, 0.3])
    assert w == [float(np.float32(0.7 / (0.7 + 0.3))), float(np.float32(0.3 / (0.7 + 0.3)))]
    # divided in float64 first, rounded to fp32 once: not the fp32 quotient of fp32 values
    third = models.blend_weights([1, 1, 1])
    assert third == [float(np.float32(1.0 / 3.0))] * 3
    assert all(float(np.float32(v)) == v for v in w + third)                   # what is returned is what is sent
    assert models.blend_weights(torch.tensor([1.0, 1.0])) == [0.5, 0.5]
    assert len(models.blend_weights([1.0] * 16)) == 16


def test_blend_weights_as_given():
    assert models.blend_weights([1.5, -0.5], normalize=False) == [1.5, -0.5]
    assert models.blend_weights([0.0, 0.0], normalize=False) == [0.0, 0.0]     # a sum of 0 is the caller's business
    assert models.blend_weights([0.1], normalize=False) == [float(np.float32(0.1))]


def test_blend_weights_refusals():
    for bad in ([float("nan"), 1.0], [1.0, float("inf")], [-float("inf")]):
        for norm in (True, False):
            with pytest.raises(ValueError):
                models.blend_weights(bad, normalize=norm)
    with pytest.raises(ValueError):
        models.blend_weights([])
    with pytest.raises(ValueError):
        models.blend_weights([1.0] * 17)
    with pytest.raises(ValueError):
        models.blend_weights([1.0] * 17, normalize=False)
    for bad in ([0.0, 0.0], [1.0, -1.0], [-2.0, 1.0]):
        with pytest.raises(ValueError):
            models.blend_weights(bad)
    with pytest.raises(ValueError):
        models.blend_weights([1e39], normalize=False)                          # beyond fp32


# ------------------------------------------------------------------ SpeakerSlots
def test_slots_lowest_free_reuse_and_exhaustion():
    s = models.SpeakerSlots()
    assert s.n == models.SPEAKER_SLOTS == 256 and models.BLEND_MAX == 16
    assert [s.take() for _ in range(4)] == [0, 1, 2, 3]
    s.free(1)
    s.free(2)
    assert 1 not in s and 3 in s and len(s) == 2
    assert s.take() == 1 and s.take() == 2 and s.take() == 4                   # the lowest free one, then on
    with pytest.raises(ValueError):
        s.free(9)
    with pytest.raises(ValueError):
        s.free(-1)
    for _ in range(256 - 5):
        s.take()
    assert len(s) == 256
    with pytest.raises(ValueError, match="256"):
        s.take()
    s.free(200)
    assert s.take() == 200
    small = models.SpeakerSlots(2)
    assert (small.take(), small.take()) == (0, 1)
    with pytest.raises(ValueError):
        small.take()


# ------------------------------------------------------------------ Speaker on the host entries
class _Net:
    n_speakers = 12

    def _release_speaker(self, v):
        v.released = True


def test_speaker_is_a_host_sid_until_released():
    net = _Net()
    v = models.Speaker(net, 3, [3, 7], [0.75, 0.25], None)
    assert v.sid == 15 and v.ids == (3, 7) and v.weights == (0.75, 0.25)
    assert models.Request([1, 2, 3], sid=v).sid == 15
    wave = torch.zeros(4000)
    r = models.ConvertRequest(wave, 3, v, 22050, 256, 1024)
    assert (r.sid_src, r.sid_tgt) == (3, 15)
    r = models.ConvertRequest(wave, v, 4, 22050, 256, 1024)                    # a voice as the source is allowed
    assert (r.sid_src, r.sid_tgt) == (15, 4)
    assert torch.tensor([2, v.sid]).tolist() == [2, 15]
    v.release()
    assert v.released and "released" in repr(v)
    with pytest.raises(ValueError, match="released"):
        v.sid
    with pytest.raises(ValueError, match="released"):
        models.Request([1, 2, 3], sid=v)
    with pytest.raises(ValueError, match="released"):
        models.ConvertRequest(wave, 3, v, 22050, 256, 1024)


# ------------------------------------------------------------------ the C entries
def _header():
    return open(os.path.join(ROOT, "include", "mbistft_vits.h")).read()


def test_the_new_symbols_are_declared_and_exported():
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    L = _capi.lib()
    for sym in NEW:
        assert re.search(r"\b%s\s*\(" % sym, code), sym
        assert sym in _capi.SYMBOLS and getattr(L, sym) is not None
    assert re.search(r"#define MBV_SPEAKER_SLOTS 256\b", code) and re.search(r"#define MBV_BLEND_MAX 16\b", code)
    assert L.mbv_speaker_slots() == _capi.SPEAKER_SLOTS == 256 and _capi.BLEND_MAX == 16
    assert L.mbv_speaker_runs.restype is C.c_int64
    assert L.mbv_speaker_runs(None) == -1 and L.mbv_speaker_defined(None, 12) == -1
    assert L.mbv_speakers_define(None, None, 0, None) != 0 and L.mbv_speaker_release(None, 0, None) != 0


def test_speaker_def_struct_layout_matches_header():
    body = re.search(r"typedef struct mbv_speaker_def \{(.*?)\} mbv_speaker_def;", _header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.sub(r"\[.*?\]", "", d.replace("*", " ").split()[-1]) for d in body.split(";") if d.strip()]
    assert names == [n for n, _ in _capi.MbvSpeakerDef._fields_] == ["slot", "count", "ids", "weights", "vector"]
    off = {n: getattr(_capi.MbvSpeakerDef, n).offset for n in names}
    assert off == {"slot": 0, "count": 4, "ids": 8, "weights": 72, "vector": 136}
    assert C.sizeof(_capi.MbvSpeakerDef) == 144
