"""CPU checks of the streamed wire output: the readiness rule of `mbv_resample_ready` (host only, no GPU) against
the float64 restatement of resampy (tests/resample_ref.py) and against the library's own bank, and `FrameCutter`
against `frame_pcm16`."""
import base64
import ctypes as C
import math

import numpy as np
import pytest

import resample_ref as RR
from mb_istft_vits_amd import _capi, wire

PAIRS = [(22050, 24000), (22050, 16000), (16000, 24000), (24000, 22050), (22050, 44100), (16000, 8000)]
FILTERS = {"kaiser_best": 0, "kaiser_fast": 1}
N = 2304
FRONTIERS = [1, 37, 256, 300, 512, 1024, 2048, N - 1, N]


def ready(orig, target, res_type, in_avail, in_total):
    return _capi.lib().mbv_resample_ready(orig, target, FILTERS[res_type], in_avail, in_total)


def geometry(orig, target, res_type):
    L = _capi.lib()
    phases, taps, left = C.c_int32(), C.c_int32(), C.c_int32()
    assert L.mbv_resample_bank(orig, target, FILTERS[res_type], None, 0, C.byref(phases), C.byref(taps),
                               C.byref(left)) == 0, L.mbv_last_error(None)
    return phases.value, taps.value, left.value


@pytest.mark.parametrize("res_type", sorted(FILTERS))
@pytest.mark.parametrize("orig,target", PAIRS)
def test_ready_outputs_do_not_depend_on_the_future(orig, target, res_type):
    """Inputs at and past the frontier replaced by garbage: outputs [0, ready) are the clean run's, and the first
    output that does change lies at most 4 outputs after `ready` (the rule is not "wait for everything")."""
    rs = np.random.RandomState(orig % 1000 + target % 1000 + len(res_type))
    x = rs.uniform(-1, 1, N)
    clean = RR.resample(x, orig, target, res_type)
    for f in FRONTIERS:
        r = ready(orig, target, res_type, f, N)
        assert 0 <= r <= len(clean)
        if f >= N:
            assert r == len(clean)
            continue
        dirty = x.copy()
        dirty[f:] = 1e6 * (1 + rs.uniform(0, 1, N - f))
        got = RR.resample(dirty, orig, target, res_type)
        assert got.shape == clean.shape
        assert np.array_equal(got[:r], clean[:r]), (f, r)
        changed = np.nonzero(got != clean)[0]
        assert changed.size, f
        first = int(changed[0])
        print("%d -> %d %s frontier %d: ready %d, first changed output %d" % (orig, target, res_type, f, r, first))
        assert r <= first <= r + 4, (f, r, first)


@pytest.mark.parametrize("res_type", sorted(FILTERS))
@pytest.mark.parametrize("orig,target", PAIRS)
def test_ready_properties(orig, target, res_type):
    g = math.gcd(orig, target)
    Lp, M = target // g, orig // g
    phases, K, left = geometry(orig, target, res_type)
    assert phases == Lp
    ratio = float(target) / orig
    for n in (1, 255, N, 147 * 20, 256 * 300):
        total = RR.out_len(n, orig, target)
        for f in list(range(0, min(n, 700))) + [n - 1, n, n + 1, n + 10 ** 6]:
            r = ready(orig, target, res_type, f, n)
            if f >= n:
                assert r == int(np.ceil(n * ratio)) == total
            else:
                assert r == min(max(0, -((-(f - K + left + 1) * Lp) // M)), total)   # the rule, in integers
                assert r >= ((f - K) * Lp) // M                                       # the lag is at most K inputs
        if n <= 147 * 20:
            rs = [ready(orig, target, res_type, f, n) for f in range(0, n + 3)]
            assert all(a <= b for a, b in zip(rs, rs[1:]))                            # non-decreasing in in_avail
    assert ready(orig, target, res_type, -5, N) == 0


def test_ready_lag_is_the_filter_half_width():
    """K - left - 1 input samples are held back: the figures of the header comment."""
    lag = lambda o, t, r: (lambda g: g[1] - g[2] - 1)(geometry(o, t, r))
    assert lag(22050, 24000, "kaiser_best") == 64 and lag(16000, 24000, "kaiser_best") == 64
    assert lag(22050, 16000, "kaiser_best") == 88
    assert lag(22050, 24000, "kaiser_fast") == 16 and lag(22050, 16000, "kaiser_fast") == 22


def test_ready_equal_rates_and_refusals():
    L = _capi.lib()
    for f, n in ((0, 10), (7, 10), (10, 10), (11, 10), (256 * 32, 256 * 300)):
        assert ready(22050, 22050, "kaiser_best", f, n) == min(f, n)
        assert wire.resample_ready(16000, 16000, f, n) == min(f, n)
    assert L.mbv_resample_ready(22050, 24001, 0, 100, 1000) < 0          # 24001 phases
    assert b"4096" in L.mbv_last_error(None)
    assert L.mbv_resample_ready(0, 24000, 0, 100, 1000) < 0
    assert L.mbv_resample_ready(22050, 24000, 2, 100, 1000) < 0          # unknown filter
    assert L.mbv_resample_ready(22050, 22050, 2, 100, 1000) < 0
    assert L.mbv_resample_ready(22050, 24000, 0, 100, -1) < 0
    with pytest.raises(_capi.MbvError, match="4096"):
        wire.resample_ready(22050, 24001, 100, 1000)
    with pytest.raises(ValueError):
        wire.resample_ready(22050, 24000, 100, 1000, res_type="soxr_hq")
    assert wire.resample_ready(22050, 24000, 256 * 32, 256 * 300) == ready(22050, 24000, "kaiser_best", 8192, 76800)


@pytest.mark.parametrize("res_type", sorted(FILTERS))
@pytest.mark.parametrize("orig,target", PAIRS)
def test_ready_against_the_bank_rows(orig, target, res_type):
    """For every t < ready the highest tap index of the full padded bank row is below in_avail, whichever row
    serves t (row L reads one sample earlier)."""
    Lp, K, left = geometry(orig, target, res_type)
    M = orig // math.gcd(orig, target)
    for n in (N, 256 * 40):
        for f in sorted(set(FRONTIERS + list(range(0, 400, 7)) + [n - 1])):
            if f >= n:
                continue
            r = ready(orig, target, res_type, f, n)
            t = np.arange(r, dtype=np.int64)
            if r:
                assert int(((t * M) // Lp - left + K - 1).max()) < f, (f, r)
            # tight to within one phase period: output r (if it exists in the row) does reach the frontier
            if r < RR.out_len(n, orig, target) and f - K + left + 1 > 0:
                assert (r * M) // Lp - left + K - 1 >= f, (f, r)


def test_frame_cutter_matches_frame_pcm16():
    rs = np.random.RandomState(11)
    for rate, fl in ((24000, 0.02), (16000, 0.02), (22050, 0.02), (8000, 0.0101)):
        n = wire.chunk_size(rate, fl)
        for total in (0, 1, n - 1, n, n + 1, 5 * n, 7 * n + 13, 20000):
            pcm = rs.randint(-32768, 32768, total).astype(np.int16)
            cuts = np.sort(rs.randint(0, total + 1, rs.randint(0, 12)))
            cuts = np.concatenate([[0], cuts, cuts[:2], [total]])       # repeated cuts: empty pushes
            cuts.sort()
            fc = wire.FrameCutter(rate, fl)
            frames = []
            for a, b in zip(cuts[:-1], cuts[1:]):
                got = fc.push(pcm[a:b])
                assert all(len(base64.b64decode(s)) == 2 * n for s in got)     # push emits whole frames only
                frames += got
            frames += fc.close()
            assert frames == wire.frame_pcm16(pcm, rate, fl)
            assert len(frames) == -(-total // n)
            assert fc.close() == []
    # pushes shorter than a frame, one sample at a time
    pcm = rs.randint(-32768, 32768, 1000).astype(np.int16)
    fc = wire.FrameCutter(24000)
    frames = [f for i in range(1000) for f in fc.push(pcm[i:i + 1])] + fc.close()
    assert frames == wire.frame_pcm16(pcm, 24000)
    assert wire.FrameCutter(24000).close() == []                        # an empty stream gives no frame
    with pytest.raises(ValueError):
        wire.FrameCutter(24000).push(np.zeros(4, np.float32))
    with pytest.raises(ValueError):
        wire.FrameCutter(10, 0.01)


def test_frame_cutter_takes_torch_tensors():
    import torch
    rs = np.random.RandomState(2)
    pcm = rs.randint(-32768, 32768, 1500).astype(np.int16)
    fc = wire.FrameCutter(24000)
    frames = fc.push(torch.from_numpy(pcm[:700])) + fc.push(torch.from_numpy(pcm[700:])) + fc.close()
    assert frames == wire.frame_pcm16(pcm, 24000)
