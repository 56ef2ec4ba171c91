"""CPU-only checks of per-token pitch: the host planner of the time warp (`mbv_warp_plan`,
`mbv_warp_ready`) against the NumPy restatement (tests/warp_ref.py), that restatement against the project's own
resampler restatement (tests/resample_ref.py) at constant rates, readiness as a property over random maps, and the
host logic of `pitch=` (arguments, glide, marks, refusals, the ctypes mirror).  No GPU is touched."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

from mb_istft_vits_amd import _capi, models, stream, wire
from mb_istft_vits_amd.models import Request

import resample_ref
import warp_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOP = 256


def _plan(rate, hop=HOP):
    rate = np.ascontiguousarray(rate, np.float32)
    U = np.full(len(rate) + 1, -1.0, np.float64)
    n_out = C.c_int64(-1)
    rc = _capi.lib().mbv_warp_plan(hop, len(rate), rate.ctypes.data, U.ctypes.data, C.byref(n_out))
    return rc, U, int(n_out.value)


def _tables():
    rs = np.random.RandomState(11)
    out = [np.full(7, warp_ref.PITCH_MIN, np.float32), np.full(7, warp_ref.PITCH_MAX, np.float32),
           np.asarray([1.3], np.float32), np.asarray([0.5], np.float32), np.ones(40, np.float32)]
    for F in (1, 2, 5, 33, 400):
        out.append(rs.uniform(warp_ref.PITCH_MIN, warp_ref.PITCH_MAX, F).astype(np.float32))
    return out


# ------------------------------------------------------------------------------------------------ the planner
@pytest.mark.parametrize("hop", [256, 100, 1])
def test_plan_is_bitwise_the_restatement(hop):
    for rate in _tables():
        rc, U, n_out = _plan(rate, hop)
        U_ref, n_ref = warp_ref.plan(rate, hop)
        assert rc == 0 and n_out == n_ref
        assert np.array_equal(U.view(np.int64), U_ref.view(np.int64))
        m = stream.WarpMap(rate, hop)
        assert m.n_out == n_ref and np.array_equal(m.U, U_ref) and m.frames == len(rate) and m.samples == len(rate) * hop
    # all-ones is the identity map
    _, U, n_out = _plan(np.ones(9, np.float32))
    assert n_out == 9 * HOP and U.tolist() == [float(f * HOP) for f in range(10)]


def test_plan_refusals_name_the_frame():
    L = _capi.lib()
    for bad, frame in ((math.nan, 3), (math.inf, 0), (0.49999, 5), (2.0001, 2), (-1.0, 1), (0.0, 4)):
        rate = np.ones(6, np.float32)
        rate[frame] = bad
        rc, _, _ = _plan(rate)
        assert rc != 0 and ("frame %d:" % frame) in L.mbv_last_error(None).decode()
        with pytest.raises(ValueError, match="frame %d:" % frame):
            stream.WarpMap(rate, HOP)
    rate = np.ones(2, np.float32)
    U, n = np.zeros(3), C.c_int64()
    assert L.mbv_warp_plan(0, 2, rate.ctypes.data, U.ctypes.data, C.byref(n)) != 0
    assert L.mbv_warp_plan(HOP, 0, rate.ctypes.data, U.ctypes.data, C.byref(n)) != 0
    assert L.mbv_warp_plan(HOP, 2, None, U.ctypes.data, C.byref(n)) != 0
    assert L.mbv_warp_ready(HOP, 2, rate.ctypes.data, U.ctypes.data, 2, 100) == -1       # an unknown res_type
    assert "res_type" in L.mbv_last_error(None).decode()
    assert L.mbv_warp_runs(None) == -1 and L.mbv_warp_ranges(None, None, 0, None) != 0


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("res_type", ["kaiser_best", "kaiser_fast"])
@pytest.mark.parametrize("rate,orig,target", [(1.25, 20000, 16000), (0.8, 16000, 20000)])
def test_constant_rate_is_the_resampler(rate, orig, target, res_type):
    """A constant rate R is resampy at ratio 1 / R; the only difference is tau against t / ratio, about 1e-12 of a
    sample.  The table is handed over in float64 here (0.8 is no fp32 value; fp64 on both sides)."""
    F = 3
    x = np.random.RandomState(5).uniform(-1, 1, F * HOP)
    y = warp_ref.warp(x, np.full(F, rate, np.float64), HOP, res_type)
    z = resample_ref.resample(x, orig, target, res_type)
    n = min(len(y), len(z))
    assert n >= len(z) - 1 and n >= int(F * HOP / rate) - 1
    assert np.abs(y[:n] - z[:n]).max() <= 1e-8


# ------------------------------------------------------------------------------------------------ readiness
@pytest.mark.parametrize("res_type", ["kaiser_best", "kaiser_fast"])
def test_readiness_is_safe_monotone_and_closes(res_type):
    """For every frontier, every output below `mbv_warp_ready` has all its taps below the frontier."""
    rs = np.random.RandomState(17)
    code = {"kaiser_best": 0, "kaiser_fast": 1}[res_type]
    for case in range(50):
        F = int(rs.randint(1, 9))
        if case % 5 == 0:
            rate = np.full(F, (warp_ref.PITCH_MIN, warp_ref.PITCH_MAX)[case % 2], np.float32)
        elif case % 5 == 1:
            rate = rs.choice([0.5, 2.0], F).astype(np.float32)
        else:
            rate = rs.uniform(warp_ref.PITCH_MIN, warp_ref.PITCH_MAX, F).astype(np.float32)
        m = stream.WarpMap(rate, HOP)
        U, n_out = warp_ref.plan(rate, HOP)
        highest = np.asarray([warp_ref.tap_extent(t, U, rate, HOP, res_type)[1] for t in range(n_out)])
        top = np.maximum.accumulate(highest)                      # the highest index any output up to t reads
        last = 0
        for in_avail in list(range(0, F * HOP, 37)) + [F * HOP - 1]:
            r = m.ready(in_avail, res_type)
            assert r == warp_ref.ready(rate, U, HOP, in_avail, res_type)
            assert r == _capi.lib().mbv_warp_ready(HOP, F, m.rate.ctypes.data, m.U.ctypes.data, code, in_avail)
            assert last <= r <= n_out
            last = r
            if r:
                assert top[r - 1] < in_avail, (case, in_avail, r)
        assert m.ready(F * HOP, res_type) == n_out == m.ready(F * HOP + 1000, res_type)
        # the half width the kernel stages covers the reach of every output on both sides of floor(tau)
        floors = np.asarray([int(warp_ref.tau(t, U, rate, HOP)[0]) for t in range(n_out)])
        lowest = np.asarray([warp_ref.tap_extent(t, U, rate, HOP, res_type)[0] for t in range(n_out)])
        hw = warp_ref.half_width(rate, res_type)
        assert (highest - floors).max() <= hw and (floors - lowest).max() <= hw


# ------------------------------------------------------------------------------------------------ host logic
def test_pitch_of_semitones_and_bounds():
    assert models.pitch_of_semitones(0) == 1.0 and models.pitch_of_semitones(12) == 2.0 == models.PITCH_MAX
    assert models.pitch_of_semitones(-12) == 0.5 == models.PITCH_MIN
    assert models.pitch_of_semitones(7) == 2.0 ** (7 / 12.0) == warp_ref.pitch_of_semitones(7)
    assert wire.pitch_of_semitones is models.pitch_of_semitones and (wire.PITCH_MIN, wire.PITCH_MAX) == (0.5, 2.0)
    for bad in (math.nan, math.inf):
        with pytest.raises(ValueError):
            models.pitch_of_semitones(bad)


def test_pitch_arg_refusals():
    ids = [3, 4, 5, 6]
    r = Request(ids, pitch=[0.5, 1.0, 2.0, 1.25])
    assert r.pitch.dtype == torch.float32 and r.pitch.tolist() == [0.5, 1.0, 2.0, 1.25] and not r.pitch.is_cuda
    assert Request(ids).pitch is None and Request(ids).scale is None
    assert Request(ids, pitch=torch.tensor([[1.0, 1.5, 1.0, 1.0]], dtype=torch.float64)).pitch.shape == (4,)
    for bad in ([1.0] * 3, [1.0] * 5, [[1.0] * 4] * 2, [1.0, math.nan, 1.0, 1.0], [1.0, math.inf, 1.0, 1.0],
                [1.0, 0.49, 1.0, 1.0], [1.0, 2.01, 1.0, 1.0], [1.0, -1.0, 1.0, 1.0]):
        with pytest.raises(ValueError):
            Request(ids, pitch=bad)
    for bad in ("high", [True, False, True, True], ["a", "b", "c", "d"], torch.ones(4, dtype=torch.complex64)):
        with pytest.raises(TypeError):
            Request(ids, pitch=bad)
    assert models._pitch_arg("infer_stream", [[1.0, 2.0]], 1, 2).shape == (1, 2)
    with pytest.raises(ValueError):
        models._pitch_arg("infer_stream", [1.0, 2.0, 1.0], 1, 2)
    with pytest.raises(ValueError):
        Request(ids, pitch=[1.0] * 4, pitch_glide_frames=-1)


def test_pitch_compensation_goes_through_the_scale_table():
    ids = [3, 4, 5, 6]
    p = np.asarray([0.5, 1.0, 2.0, 1.25], np.float32)
    r = Request(ids, pitch=p, length_scale=1.3)
    assert r.length_scale == 1.0 and r.scale.dtype == torch.float32
    assert np.array_equal(r.scale.numpy(), np.float32(1.3) * p)
    s = torch.tensor([1.0, 0.7, 1.1, 2.0])
    r = Request(ids, pitch=p, length_scale=s)
    assert np.array_equal(r.scale.numpy(), s.numpy() * p)
    r = Request(ids, pitch=p, length_scale=1.3, pitch_compensate=False)          # plain varispeed
    assert r.scale is None and r.length_scale == float(1.3) and r.pitch is not None


def test_pitch_with_durations_is_refused():
    ids = [3, 4, 5, 6]
    with pytest.raises(ValueError, match="scale the durations"):
        Request(ids, pitch=[1.0] * 4, durations=torch.tensor([2, 3, 1, 4]))
    with pytest.raises(ValueError, match="scale the durations"):
        Request(ids, pitch=[1.0] * 4, durations=torch.tensor([2, 3, 1, 4]), pitch_compensate=False)
    net = models.SynthesizerTrn.__new__(models.SynthesizerTrn)                    # the checks come before the model
    x = torch.tensor([ids])
    with pytest.raises(ValueError, match="scale the durations"):
        models.SynthesizerTrn.infer_stream.__wrapped__(net, x, torch.tensor([4]), pitch=[[1.0] * 4],
                                                       durations=torch.tensor([[2, 3, 1, 4]]))
    with pytest.raises(ValueError, match="B = 1"):
        models.SynthesizerTrn.infer_stream.__wrapped__(net, torch.tensor([ids, ids]), torch.tensor([4, 4]),
                                                       pitch=[[1.0] * 4] * 2)


def test_glide_values():
    marks = [0, 3, 3, 7]                         # token 1 holds no frame
    step = stream.frame_rates([2.0, 0.5, 1.0], marks, 7, 0)
    assert step.dtype == np.float32 and step.tolist() == [2.0, 2.0, 2.0, 1.0, 1.0, 1.0, 1.0]
    assert np.array_equal(step, warp_ref.frame_rates([2.0, 0.5, 1.0], marks, 7))
    g1 = stream.frame_rates([2.0, 0.5, 1.0], marks, 7, 1)
    want = [2.0, 2.0, np.float32(5.0 / 3.0), np.float32(4.0 / 3.0), 1.0, 1.0, 1.0]
    assert g1.tolist() == [float(v) for v in want]
    g2 = stream.frame_rates([2.0, 0.5, 1.0], marks, 7)                            # the default: two frames either side
    assert g2.tolist() == [float(np.float32(v)) for v in (2.0, 7 / 4.0, 8 / 5.0, 7 / 5.0, 6 / 5.0, 1.0, 1.0)]
    rs = np.random.RandomState(2)
    p = rs.uniform(0.5, 2.0, 9).astype(np.float32)
    marks = np.concatenate([[0], np.cumsum(rs.randint(0, 6, 9))])
    for g in (0, 1, 2, 5, 100):
        got = stream.frame_rates(p.tolist(), marks, int(marks[-1]), g)
        assert np.array_equal(got.view(np.int32), warp_ref.glide(warp_ref.frame_rates(p, marks, int(marks[-1])), g).view(np.int32))
        assert got.min() >= 0.5 and got.max() <= 2.0
    # a stream clipped by max_len keeps the frames in front of the clip; a frame no token holds plays at 1
    assert stream.frame_rates([2.0, 0.5], [0, 2, 4], 3, 0).tolist() == [2.0, 2.0, 0.5]
    assert stream.frame_rates([2.0], [0, 2], 4, 0).tolist() == [2.0, 2.0, 1.0, 1.0]
    with pytest.raises(ValueError):
        stream.frame_rates([2.0], [0, 2], 2, -1)


def test_mark_samples_through_the_warp():
    rate = np.asarray([2.0, 2.0, 0.5, 1.0, 1.25], np.float32)
    m = stream.WarpMap(rate, HOP)
    U, _ = warp_ref.plan(rate, HOP)
    frames = [0, 1, 2, 3, 5]
    at = m.samples_of_frames(frames)
    assert at == warp_ref.samples_of_frames(U, frames) == [0, 128, 256, 768, 1229]
    assert all(isinstance(v, int) for v in at)
    for model_sr, out_sr, lag in ((22050, 24000, 0), (22050, 8000, 7), (22050, 22050, 0)):
        got = wire.mark_samples(frames, HOP, model_sr, out_sr, lag, warp=m)
        assert got == [-((-s * out_sr) // model_sr) + lag for s in at]
        assert got == wire.mark_samples(at, 1, model_sr, out_sr, lag)             # the existing mapping of model samples
    ident = stream.WarpMap(np.ones(5, np.float32), HOP)
    assert wire.mark_samples(frames, HOP, 22050, 24000, 3, warp=ident) == wire.mark_samples(frames, HOP, 22050, 24000, 3)


def test_live_wires_refuse_pitch_before_anything_else():
    with pytest.raises(ValueError, match="pitch"):
        wire.convert_pcm16(None, None, None, 0, 1, 16000, 22050, 24000, 256, 1024, pitch=[1.0])
    with pytest.raises(ValueError, match="pitch"):
        wire.convert_live_pcm16(None, 0, 1, 16000, 22050, 24000, 256, 1024, 1000, pitch=[1.0])
    with pytest.raises(ValueError, match="pitch"):
        wire.LiveWire(None, 0, 1, 16000, 22050, 24000, 256, 1024, 1000, pitch=[1.0])
    with pytest.raises(ValueError, match="pitch"):
        wire.PcmPool.add_live(None, None, pitch=[1.0])


# ------------------------------------------------------------------------------------------------ the C struct
def _fields(name):
    hdr = open(os.path.join(ROOT, "include", "mbistft_vits.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    types = {"int64_t": C.c_int64, "int32_t": C.c_int32, "float": C.c_float, "mbv_pcm_envelope": _capi.MbvPcmEnvelope}
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype = C.c_void_p if "*" in decl else types[decl.split()[0]]
        for part in decl.replace("*", " ").split(","):
            fields.append((part.split()[-1], ctype))
    return fields


def test_struct_layout_matches_the_header():
    assert [(n, t) for n, t in _capi.MbvWarpRow._fields_] == _fields("mbv_warp_row")
    assert [n for n, _ in _capi.MbvWarpRow._fields_] == [
        "wave", "samples", "in_avail", "U", "rate", "U_host", "rate_host", "frames", "hop", "envelope", "out_first",
        "out_count", "out", "out_capacity", "res_type", "reserved"]
    assert C.sizeof(_capi.MbvWarpRow) == 128
    assert [getattr(_capi.MbvWarpRow, n).offset for n, _ in _capi.MbvWarpRow._fields_] == [
        0, 8, 16, 24, 32, 40, 48, 56, 60, 64, 88, 96, 104, 112, 120, 124]
    hdr = open(os.path.join(ROOT, "include", "mbistft_vits.h")).read()
    for s in ("mbv_warp_plan", "mbv_warp_ready", "mbv_warp_ranges", "mbv_warp_runs"):
        assert s in _capi.SYMBOLS and re.search(r"\b%s\(" % s, hdr)
    assert "#define MBV_PITCH_MIN 0.5f" in hdr and "#define MBV_PITCH_MAX 2.0f" in hdr
    assert (_capi.PITCH_MIN, _capi.PITCH_MAX) == (0.5, 2.0)
    # the structs the wire tables already had do not change
    assert C.sizeof(_capi.MbvPcmEnvelope) == 24 and C.sizeof(_capi.MbvPcmChunk) == 88
