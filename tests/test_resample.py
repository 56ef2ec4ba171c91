"""CPU checks of the resampler (librosa 0.9.2 resample, kaiser_best / kaiser_fast): the restatement of
resampy in tests/resample_ref.py against known answers, and the library's host-built polyphase bank
(mbv_resample_bank, no GPU needed) against that restatement."""
import ctypes as C

import numpy as np
import pytest

import resample_ref as RR
from mb_istft_vits_amd import _capi

PAIRS = [(22050, 24000), (16000, 24000), (22050, 16000), (16000, 22050), (22050, 44100), (24000, 22050)]
# M = 147 and downsampling: t / ratio rounds below the integer at about half of the r = 0 outputs, where bank row L
# (read around n_t - 1) is another filter than row 0 (tests/resample_cases.py)
PAIRS += [(44100, 24000), (22050, 12000), (44100, 12000)]
FILTERS = {"kaiser_best": 0, "kaiser_fast": 1}


def bank(orig, target, res_type):
    L = _capi.lib()
    phases, taps, left = C.c_int32(), C.c_int32(), C.c_int32()
    rc = L.mbv_resample_bank(orig, target, FILTERS[res_type], None, 0, C.byref(phases), C.byref(taps), C.byref(left))
    assert rc == 0, L.mbv_last_error(None)
    b = np.zeros((phases.value + 1, taps.value), np.float32)
    rc = L.mbv_resample_bank(orig, target, FILTERS[res_type], b.ctypes.data_as(C.c_void_p), b.size, None, None, None)
    assert rc == 0, L.mbv_last_error(None)
    return b, left.value


def test_table_length_and_shape():
    for res_type, n in (("kaiser_best", 32769), ("kaiser_fast", 8193)):
        num_zeros, precision, beta, rolloff = RR.FILTERS[res_type]
        win, nb = RR.table(res_type)
        assert len(win) == n and nb == 512
        assert win[0] == pytest.approx(rolloff, abs=1e-15)
        # right half of a symmetric Kaiser window (closed form: I0(beta sqrt(1 - (x / n)^2)) / I0(beta))
        half = n - 1
        x = np.arange(n) / half
        kw = np.i0(beta * np.sqrt(1 - x ** 2)) / np.i0(beta)
        sinc = rolloff * np.sinc(rolloff * np.arange(n) / nb)
        np.testing.assert_allclose(win, kw * sinc, rtol=0, atol=1e-14)
        full = np.kaiser(2 * half + 1, beta)
        np.testing.assert_allclose(full, full[::-1], rtol=0, atol=1e-15)
        # zeros of the sinc at multiples of nb / rolloff are not on the grid; at the end the window is ~0
        assert abs(win[-1]) < 1e-3 * rolloff


def test_vectorised_restatement_is_the_loop():
    rs = np.random.RandomState(5)
    x = rs.uniform(-1, 1, 400)
    for orig, target in PAIRS:
        for res_type in FILTERS:
            a = RR.resample_loop(x, orig, target, res_type)
            b = RR.resample(x, orig, target, res_type)
            assert a.shape == b.shape
            np.testing.assert_allclose(a, b, rtol=0, atol=1e-12)


@pytest.mark.parametrize("res_type", sorted(FILTERS))
@pytest.mark.parametrize("orig,target", PAIRS)
def test_bank_matches_restatement(orig, target, res_type):
    b, left = bank(orig, target, res_type)
    assert b.shape[1] % 4 == 0
    if target > orig and res_type == "kaiser_best":
        assert b.shape[1] == 128
    rs = np.random.RandomState(orig + target)
    for n in (0, 1, 63, 64, 65, 147, 147 * 7, 147 * 20, int(rs.randint(100, 3000))):
        x = rs.uniform(-1, 1, n)
        ref = RR.resample(x, orig, target, res_type)
        got = RR.apply_bank(x, b, orig, target, left)
        assert got.shape == ref.shape == (RR.out_len(n, orig, target),)
        if n:
            assert np.abs(got - ref).max() < 1e-6, (n, np.abs(got - ref).max())


def test_bank_refuses_unsupported_pairs():
    L = _capi.lib()
    p = C.c_int32()
    assert L.mbv_resample_bank(22050, 24001, 0, None, 0, C.byref(p), None, None) != 0    # 24001 phases
    assert b"4096" in L.mbv_last_error(None)
    assert L.mbv_resample_bank(0, 24000, 0, None, 0, None, None, None) != 0
    assert L.mbv_resample_bank(22050, 24000, 2, None, 0, None, None, None) != 0
    assert L.mbv_resample_bank(22050, 24000, 0, None, 0, C.byref(p), None, None) == 0 and p.value == 160
    small = np.zeros(10, np.float32)
    assert L.mbv_resample_bank(22050, 24000, 0, small.ctypes.data_as(C.c_void_p), small.size, None, None, None) != 0


def test_length_rule():
    for orig, target in PAIRS:
        ratio = float(target) / orig
        for n in list(range(0, 300)) + [147 * k for k in range(1, 400)] + [10 ** 6 + 3]:
            assert RR.out_len(n, orig, target) == int(np.ceil(n * ratio))
    # n a multiple of 147 at 22050 -> 24000: n * ratio lands just above the integer for some n, and
    # librosa keeps one more (zero) sample there than the exact rational length
    exact = [147 * k for k in range(1, 400) if RR.out_len(147 * k, 22050, 24000) != 160 * k]
    assert exact, "expected float64 rounding to add a sample for some multiples of 147"
    assert all(RR.out_len(n, 22050, 24000) == n * 160 // 147 + 1 for n in exact)


def test_known_answers():
    sr_in = 22050
    n = 6000
    t = np.arange(n) / sr_in
    tone = lambda tt: 0.5 * np.sin(2 * np.pi * 440 * tt) + 0.3 * np.cos(2 * np.pi * 3000 * tt + 0.3)
    for target in (24000, 44100):
        y = RR.resample(tone(t), sr_in, target)
        tt = np.arange(len(y)) / target
        mid = slice(len(y) // 4, 3 * len(y) // 4)
        assert np.abs(y[mid] - tone(tt[mid])).max() < 1e-6
    # DC gain: 1 when upsampling; the truncated index step of resampy costs ~0.1 % at 22050 -> 16000
    dc_up = RR.resample(np.ones(4000), 22050, 24000)
    assert abs(dc_up[len(dc_up) // 2] - 1) < 1e-6
    dc_down = RR.resample(np.ones(4000), 22050, 16000)
    g = dc_down[len(dc_down) // 4: 3 * len(dc_down) // 4]
    assert 1e-4 < np.abs(g - 1).max() < 3e-3, (g.min(), g.max())
    # equal rates: the input, unchanged
    x = np.random.RandomState(0).standard_normal(100)
    assert np.array_equal(RR.resample(x, 22050, 22050), x)


def test_cross_check_against_scipy():
    signal = pytest.importorskip("scipy.signal")
    sr_in = 22050
    t = np.arange(8000) / sr_in
    x = 0.5 * np.sin(2 * np.pi * 440 * t) + 0.3 * np.sin(2 * np.pi * 3000 * t)
    for orig, target in ((22050, 24000), (22050, 16000)):
        y = RR.resample(x, orig, target)
        g = np.gcd(orig, target)
        z = signal.resample_poly(x, target // g, orig // g)
        m = min(len(y), len(z))
        mid = slice(m // 4, 3 * m // 4)
        assert np.abs(y[mid] - z[mid]).max() < 2e-3
