"""Barge-in, host side (no GPU): the token marks in wire samples (`wire.mark_samples`) against their statement in
exact rationals, the integer plan of a revoke (`wire.revoke_plan`) against a brute-force statement of its rules, and
`mbv_pcm_fade_make`."""
import ctypes as C

import numpy as np
import pytest

import fade_ref
from mb_istft_vits_amd import _capi, stream, wire

SPF = 256
PAIRS = [(22050, 24000), (22050, 8000), (16000, 24000)]


@pytest.mark.parametrize("lookahead", [0, 120])
@pytest.mark.parametrize("model_sr,rate", PAIRS)
def test_mark_samples_is_the_ceiling_of_the_exact_time(model_sr, rate, lookahead):
    frames = 411
    marks = [0, 1, 2, 3, 7, 7, 86, 255, 256, 257, 300, frames - 1, frames]      # frame 0, a silent token, the last frame
    got = wire.mark_samples(marks, SPF, model_sr, rate, lookahead)
    assert got == fade_ref.mark_samples(marks, SPF, model_sr, rate, lookahead)
    assert all(isinstance(v, int) for v in got)
    assert got[0] == lookahead and got == sorted(got)
    for f, u in zip(marks, got):
        # the first wire sample at or after the token's first model sample: u - 1 lies before it
        u -= lookahead
        assert u * model_sr >= f * SPF * rate > (u - 1) * model_sr
    assert wire.mark_samples([], SPF, model_sr, rate) == []
    with pytest.raises(ValueError):
        wire.mark_samples(marks, SPF, model_sr, rate, -1)


def _ready(model_sr, rate, frames, lookahead):
    """the schedule of a stream of `frames` frames and the final outputs after each of its chunks"""
    n = SPF * frames
    schedule = stream.chunk_schedule(frames)
    return n, [wire.limiter_ready(model_sr, rate, SPF * (first + count), n, lookahead) for first, count in schedule]


@pytest.mark.parametrize("lookahead", [0, 120])
@pytest.mark.parametrize("model_sr,rate", PAIRS)
def test_revoke_plan_stops_at_the_first_chunk_that_makes_the_fade_final(model_sr, rate, lookahead):
    for frames in (1, 33, 200, 700):
        n, ready = _ready(model_sr, rate, frames, lookahead)
        total = wire.resample_ready(model_sr, rate, n, n)
        assert ready == sorted(ready) and ready[-1] == total
        emitted = sorted({0, ready[0], ready[len(ready) // 2], ready[-1]})
        for E in emitted:
            for fade_ms in (0.0, 0.3, 5.0, 40.0, 1e5):
                N = int(round(fade_ms * rate / 1000))
                for F in sorted({E, E + 1, E + 977, max(E, total - 3), max(E, total), max(E, total) + 50}):
                    cut, last, new = wire.revoke_plan(ready, total, E, F, N)
                    assert cut == min(total, F + N) == fade_ref.length(total, F, N)
                    # the last chunk issued is the first whose end makes the readiness rule reach F + N (clamped)
                    assert ready[last] >= cut and all(r < cut for r in ready[:last])
                    # no step asks for an output at or beyond the cut, and nothing in front of it is lost
                    assert len(new) == last + 1 and new[-1] == cut
                    assert all(a == min(b, cut) for a, b in zip(new, ready)) and max(new) <= cut
                    if F + N >= total:
                        assert last == len(ready) - 1 and new == ready      # beyond the end: the stream plays out
                    if N == 0 and F == E and E in ready:
                        assert last == ready.index(E)                       # a hard cut now: nothing more is needed
    n, ready = _ready(model_sr, rate, 200, lookahead)
    with pytest.raises(ValueError, match="handed out"):
        wire.revoke_plan(ready, ready[-1], ready[1], ready[1] - 1, 10)
    with pytest.raises(ValueError):
        wire.revoke_plan(ready, ready[-1], 0, 0, -1)


def test_a_long_fade_saves_nothing_and_a_short_one_most_chunks():
    n, ready = _ready(22050, 24000, 860, 0)                   # ~10 s
    total = ready[-1]
    E = next(r for r in ready if r >= 24000)                  # revoked after ~1 s
    cut, last, _ = wire.revoke_plan(ready, total, E, E, 120)
    # (the schedule's chunks grow to 256 frames: E is the end of chunk 1, and chunk 2 alone covers the fade)
    assert last == 2 < len(ready) - 2 and cut == E + 120
    assert wire.revoke_plan(ready, total, E, E, 10 ** 7)[1] == len(ready) - 1


@pytest.mark.parametrize("count", [0, 1, 2, 13, 119, 120, 400, 65535, 2 ** 24 + 1, 2 ** 40])
def test_pcm_fade_make_fills_inv_in_fp32(count):
    f = _capi.pcm_fade(250, count)
    assert (f.first, f.count) == (250, count)
    want = np.float32(1) / np.float32(count + 1)
    assert np.float32(f.inv).tobytes() == want.tobytes()
    assert C.sizeof(_capi.MbvPcmFade) == 24


def test_pcm_fade_make_refuses_negative_arguments():
    L = _capi.lib()
    f = _capi.MbvPcmFade()
    assert L.mbv_pcm_fade_make(-1, 4, C.byref(f)) == -1
    assert L.mbv_pcm_fade_make(0, -1, C.byref(f)) == -1
    assert L.mbv_pcm_fade_make(0, 4, None) == -1
    with pytest.raises(ValueError):
        _capi.pcm_fade(3, -2)
