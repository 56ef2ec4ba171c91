"""CPU-only checks of the limiter's host side: `mbv_limiter_ready` (pure integers, no device) against its restatement
`wire.limiter_ready`, the plans built on it (`PcmStream`'s list, `LiveWirePlan`), the ctypes mirror of `mbv_pcm_limit`
and every refusal with its message."""
import ctypes as C
import os
import re

import pytest

from mb_istft_vits_amd import _capi, wire

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = [(22050, 24000), (48000, 16000), (22050, 22050)]
LOOKAHEADS = [0, 1, 7, 255]


def _err():
    msg = _capi.lib().mbv_last_error(None)
    return msg.decode() if msg else ""


@pytest.mark.parametrize("lookahead", LOOKAHEADS)
@pytest.mark.parametrize("orig,target", PAIRS)
def test_planner_parity_closed_and_open(orig, target, lookahead):
    lib = _capi.lib()
    n = 3001
    all_out = wire.resample_ready(orig, target, n, n)
    prev_closed = prev_open = 0
    for avail in list(range(0, 400)) + list(range(400, n - 300, 97)) + list(range(n - 300, n + 3)):
        want = wire.limiter_ready(orig, target, avail, n, lookahead)
        assert lib.mbv_limiter_ready(orig, target, 0, avail, n, lookahead) == want, avail
        # the rule itself: the resampler's count, L outputs later; everything once the row is complete
        r = wire.resample_ready(orig, target, avail, n)
        assert want == (all_out if avail >= n else max(r - lookahead, 0)), avail
        assert prev_closed <= want <= all_out
        prev_closed = want
        got = lib.mbv_limiter_ready(orig, target, 0, avail, -1, lookahead)
        assert got == wire.limiter_ready(orig, target, avail, None, lookahead) == wire.limiter_ready(orig, target, avail, -1, lookahead)
        assert got == max(wire.resample_ready_open(orig, target, avail) - lookahead, 0) and got >= prev_open
        prev_open = got
        if avail < n:
            assert got == want or want == all_out - lookahead          # open and closed agree below the end
    assert prev_closed == all_out
    assert lib.mbv_limiter_ready(orig, target, 0, -5, n, lookahead) == 0
    assert lib.mbv_limiter_ready(orig, target, 0, -5, -1, lookahead) == 0
    # lookahead 0 is the resampler's own readiness
    assert lib.mbv_limiter_ready(orig, target, 0, 1500, n, 0) == lib.mbv_resample_ready(orig, target, 0, 1500, n)
    assert lib.mbv_limiter_ready(orig, target, 1, 1500, n, lookahead) == wire.limiter_ready(orig, target, 1500, n, lookahead, "kaiser_fast")


def test_planner_refusals_carry_their_message():
    lib = _capi.lib()
    for args, what in (((22050, 24000, 0, 100, 1000, -1), "lookahead must be in [0, 255]"),
                       ((22050, 24000, 0, 100, 1000, 256), "lookahead must be in [0, 255]"),
                       ((22050, 24000, 2, 100, 1000, 7), "unknown filter"),
                       ((22050, 22050, 2, 100, 1000, 7), "unknown filter"),
                       ((0, 24000, 0, 100, 1000, 7), "sample rates must be positive"),
                       ((22050, 24001, 0, 100, -1, 7), "polyphase phases")):
        assert lib.mbv_limiter_ready(*args) == -1, args
        assert "mbv_limiter_ready" in _err() and what in _err(), (args, _err())
    for bad in (-1, 256):
        with pytest.raises(ValueError, match=r"lookahead must be in \[0, 255\]"):
            wire.limiter_ready(22050, 24000, 100, 1000, bad)
    with pytest.raises(ValueError, match="res_type"):
        wire.limiter_ready(22050, 24000, 100, 1000, 7, "soxr_hq")
    with pytest.raises(_capi.MbvError, match="polyphase phases"):
        wire.limiter_ready(22050, 24001, 100, 1000, 7)


def test_entries_and_struct_mirror_the_header():
    hdr = open(os.path.join(ROOT, "include", "mbistft_vits.h")).read()
    body = re.search(r"typedef struct mbv_pcm_limit \{(.*?)\} mbv_pcm_limit;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.split(None, 1)[1].split(",")]
    assert names == [f[0] for f in _capi.MbvPcmLimit._fields_] == ["ceiling", "lookahead", "hold"]
    assert C.sizeof(_capi.MbvPcmLimit) == 12
    lib = _capi.lib()
    for sym in ("mbv_limiter_ready", "mbv_resample_pcm16_range_limited", "mbv_resample_pcm16_chunks_limited"):
        assert sym in _capi.SYMBOLS and getattr(lib, sym) is not None
    assert lib.mbv_limiter_ready.restype is C.c_int64
    # the existing entries and the chunk's layout are as they were
    assert "int mbv_resample_pcm16_range(mbv_model *m, const float *wave, const int64_t *valid_samples, int B, int64_t in_stride," in hdr
    assert C.sizeof(_capi.MbvPcmChunk) == 88
    # without a handle the device entries return at once
    assert lib.mbv_resample_pcm16_range_limited(None, None, None, 1, 1, 22050, 24000, 0, 0, 0, 0, None, None, 1, None,
                                                None, None, None) != 0
    assert lib.mbv_resample_pcm16_chunks_limited(None, None, None, 0, 22050, 24000, 0, None, 0, None) != 0


def test_live_wire_plan_lags_by_the_lookahead_and_flushes_at_the_end():
    """The pieces of a live wire under a limiter: those of the plain plan, L outputs behind, all of it after the last
    chunk; they do not depend on how the recording was pushed (one piece per decoded chunk)."""
    model_sr, rate, spf, n_fft, hop = 22050, 24000, 256, 1024, 256
    chunks = [(0, 8), (8, 16), (24, 32), (56, 44)]
    pieces = {}
    for L in (0, 7, 255):
        plan = _FakePlan(total=100, n_fft=n_fft, hop=hop)
        w = wire.LiveWirePlan(model_sr, model_sr, rate, plan, spf, 40000, lookahead=L)
        assert w.lookahead == L
        out = []
        for k in range(1, len(chunks) + 1):
            plan.all_released = k == len(chunks)
            due = w.wire_due(chunks[:k])
            in_avail, in_total, first, count, final, ps = due
            assert in_avail == spf * sum(chunks[k - 1]) and final == plan.all_released and len(ps) == 1
            assert first + count == ps[-1][1] == _capi.lib().mbv_limiter_ready(model_sr, rate, 0, in_avail, in_total, L)
            w.wired(k, ps[-1][1], final)
            out += ps
        assert w.wire_done and w.valid == wire.resample_ready(model_sr, rate, spf * 100, spf * 100)
        pieces[L] = out
    for L in (7, 255):
        for (a0, b0), (a, b) in zip(pieces[0][:-1], pieces[L][:-1]):
            assert b == b0 - L
        assert pieces[L][-1][1] == pieces[0][-1][1]
    with pytest.raises(ValueError, match=r"lookahead must be in \[0, 255\]"):
        wire.LiveWirePlan(model_sr, model_sr, rate, _FakePlan(100, n_fft, hop), spf, 40000, lookahead=256)


class _FakePlan:
    """What `LiveWirePlan.wire_due` reads of a `stream.LivePlan`: the geometry, the total and whether all is released."""

    def __init__(self, total, n_fft, hop):
        self.total, self.n_fft, self.hop = total, n_fft, hop
        self.all_released, self.arrived, self.closed = False, 0, False
