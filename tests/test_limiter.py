"""CPU checks of the look-ahead limiter's definition on its float64 restatement, tests/limiter_ref.py:
the consequences the contract names, which the GPU tests then rely on when they compare the kernel with it."""
import numpy as np
import pytest

import limiter_ref
from mb_istft_vits_amd import wire

C = 0.9
SETTINGS = [(7, 19), (0, 0), (120, 480), (255, 1024), (1, 0), (0, 5)]


def _loud(n, seed):
    rs = np.random.RandomState(seed)
    v = rs.uniform(-0.5, 0.5, n)
    for p in rs.randint(0, n, 12):
        v[p:p + rs.randint(1, 9)] *= rs.uniform(2.0, 9.0)
    v[:3] = 3.0                                          # above the ceiling at both ends of the row
    v[-2:] = -2.5
    return v


@pytest.mark.parametrize("L,H", SETTINGS)
def test_output_never_exceeds_the_ceiling(L, H):
    v = _loud(3000, L + H)
    assert np.abs(v).max() > 2 * C
    g, m, r = limiter_ref.gain(v, C, L, H)
    # every m[j] in the sum of g[t] has t in its window, so g[t] <= r[t]
    assert (g <= r * (1 + 1e-15)).all()
    y = limiter_ref.limit(v, C, L, H)
    assert np.abs(y).max() <= C * (1 + 1e-15)
    assert np.abs(limiter_ref.pcm16(v, C, L, H).astype(np.int64)).max() <= int(np.floor(C * 32767))
    assert (g > 0).all() and (g <= 1).all()


@pytest.mark.parametrize("L,H", SETTINGS)
def test_a_quiet_signal_is_untouched(L, H):
    v = np.random.RandomState(3).uniform(-C, C, 2000)
    v[17], v[18] = C, -C                                 # at the ceiling is not above it
    g, m, r = limiter_ref.gain(v, C, L, H)
    assert (g == 1.0).all() and (m == 1.0).all()
    assert np.array_equal(limiter_ref.limit(v, C, L, H), v)
    # fp32, as the kernel adds: L + 1 ones and one division are exact
    s = np.float32(0)
    for _ in range(L + 1):
        s = np.float32(s + np.float32(1))
    assert np.float32(s / np.float32(L + 1)) == np.float32(1)


@pytest.mark.parametrize("L,H,half", [(7, 19, 27), (7, 19, 10), (120, 480, 601), (0, 0, 1), (0, 3, 4), (255, 1024, 1280)])
def test_steady_state_gain_on_a_loud_sine_is_constant(L, H, half):
    """Amplitude A > c and a half period of at most H + L + 1 samples: every window holds a crest, so once settled
    the gain is c / A everywhere: a scaled copy, no distortion.  (A sine sampled on its crests: period 2 * half.)"""
    assert half <= H + L + 1
    A = 2.0
    n = 6 * (H + 2 * L + 1) + 8 * half
    t = np.arange(n)
    v = A * np.cos(np.pi * t / half)                     # crests at multiples of `half`
    g, _, _ = limiter_ref.gain(v, C, L, H)
    settled = slice(H + 2 * L + half, n - (H + 2 * L + half))
    assert np.allclose(g[settled], C / A, rtol=1e-12, atol=0)
    y = limiter_ref.limit(v, C, L, H)
    assert np.allclose(y[settled], (C / A) * v[settled], rtol=1e-12, atol=1e-15)


@pytest.mark.parametrize("L,H", [(7, 19), (120, 480), (0, 0), (0, 4), (3, 0)])
def test_ramp_hold_and_release_around_one_impulse(L, H):
    n, p, A = 4 * (L + H) + 50, 2 * L + H + 20, 3.0
    v = np.full(n, 0.1)
    v[p] = A
    g, m, r = limiter_ref.gain(v, C, L, H)
    low = C / A
    # m is down on [p - L, p + H]; g is down wherever [t - L, t] meets that: [p - L, p + H + L]
    assert (m[p - L:p + H + 1] == low).all() and (m[:p - L] == 1).all() and (m[p + H + 1:] == 1).all()
    assert (g[:p - L] == 1).all() and (g[p + H + L + 1:] == 1).all()
    # ramps down over L samples before the peak, one step of (1 - low) / (L + 1) per sample
    for k in range(L + 1):
        want = 1 - (k + 1) * (1 - low) / (L + 1)
        assert abs(g[p - L + k] - want) < 1e-12, k
    # fully down from the peak on, for H samples after it
    assert np.allclose(g[p:p + H + 1], low, rtol=1e-12)
    # and back up over L samples
    for k in range(1, L + 1):
        want = low + k * (1 - low) / (L + 1)
        assert abs(g[p + H + k] - want) < 1e-12, k
    assert (np.diff(g[p - L - 1:p + 1]) < 0).all() and (np.diff(g[p + H:p + H + L + 2]) > 0).all()
    assert abs(limiter_ref.limit(v, C, L, H)[p] - C) < 1e-12


def test_samples_outside_the_row_are_silence():
    """v is zero before the first and after the last sample: a peak at either end still gets its full reduction, and
    nothing else changes."""
    v = np.full(200, 0.2)
    v[0], v[-1] = 4.0, -4.0
    g, _, _ = limiter_ref.gain(v, C, 7, 19)
    assert abs(g[0] - C / 4) < 1e-15 and abs(g[-1] - C / 4) < 1e-15
    assert (g[7 + 19 + 7 + 1:200 - 8] == 1).all()


def test_limiter_resolves_to_samples_and_refuses_what_the_kernel_does_not_hold():
    lim = wire.Limiter()
    assert (lim.ceiling, lim.lookahead_ms, lim.hold_ms) == (0.9, 5.0, 20.0)
    assert lim.resolve(24000) == (0.9, 120, 480) and lim.resolve(16000) == (0.9, 80, 320)
    assert lim.resolve(22050) == (0.9, 110, 441) and lim.resolve(48000) == (0.9, 240, 960)
    assert wire.Limiter(1.0, 0.0, 0.0).resolve(8000) == (1.0, 0, 0)
    assert wire.Limiter(0.5, 1.0, 2.0) == wire.Limiter(0.5, 1.0, 2.0) != wire.Limiter(0.5, 1.0, 2.5)
    for c in (0.0, -0.1, 1.0001, float("nan")):
        with pytest.raises(ValueError, match=r"ceiling .* must be in \(0, 1\]"):
            wire.Limiter(ceiling=c)
    with pytest.raises(ValueError, match="must be >= 0"):
        wire.Limiter(lookahead_ms=-1.0)
    with pytest.raises(ValueError, match="must be >= 0"):
        wire.Limiter(hold_ms=-0.5)
    with pytest.raises(ValueError, match=r"lookahead_ms 5 is 480 samples at 96000 Hz, more than the 255"):
        lim.resolve(96000)
    with pytest.raises(ValueError, match=r"hold_ms 50 is 1200 samples at 24000 Hz, more than the 1024"):
        wire.Limiter(hold_ms=50.0).resolve(24000)
    with pytest.raises(ValueError, match="sample rates must be positive"):
        lim.resolve(0)
    with pytest.raises(TypeError, match="wire.Limiter"):
        wire._limit_arg((0.9, 7, 19), 24000)
    assert wire._limit_arg(None, 24000) is None
