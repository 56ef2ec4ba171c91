"""No GPU: the host half of the loudness measurement: `mbv_kweighting`, `mbv_loudness_segments`, the
float64 reference itself (tests/loudness_ref.py) against the standard's numbers, `wire.Loudness` and the streamed
plan."""
import math

import numpy as np
import pytest
import torch

from mb_istft_vits_amd import _capi, wire

import loudness_ref

RATES = [48000, 44100, 24000, 22050, 16000, 8000]


def test_kweighting_at_48k_is_the_standards_table():
    coeffs, _ = _capi.kweighting(48000)
    t = loudness_ref.TABLE_48K
    want = list(t["shelf_b"]) + list(t["shelf_a"]) + [1.0, -2.0, 1.0] + list(t["highpass_a"])
    assert np.max(np.abs(np.array(coeffs) - np.array(want))) < 1e-12
    # and the reference's own re-derivation gives the same table
    (b, a), (c, d) = loudness_ref.kweighting(48000)
    assert np.max(np.abs(np.array(list(b) + list(a) + list(c) + list(d)) - np.array(want))) < 1e-12


@pytest.mark.parametrize("rate", [8000, 22050, 48000])
def test_transition_matrix_is_the_h_step_product_of_the_state_matrix(rate):
    H = loudness_ref.hop(rate)
    assert H == {8000: 800, 22050: 2205, 48000: 4800}[rate]
    coeffs, M = _capi.kweighting(rate)
    (b, a), (c, d) = loudness_ref.kweighting(rate)
    assert np.max(np.abs(np.array(coeffs) - np.array(list(b) + list(a) + list(c) + list(d)))) < 1e-12
    # the product itself in extended precision: in float64 the 4800 steps alone lose 4e-12 (poles at 0.995), which
    # would make the yardstick coarser than the bound it carries
    A = loudness_ref.state_matrix(rate).astype(np.longdouble)
    P = np.eye(4, dtype=np.longdouble)
    for _ in range(H):
        P = A @ P
    M = np.array(M).reshape(4, 4)
    scale = float(np.max(np.abs(P)))
    assert scale > 0 and float(np.max(np.abs(M.astype(np.longdouble) - P))) <= 1e-12 * scale


def test_the_state_matrix_is_the_zero_input_step_of_the_documented_form():
    """the documented transposed direct form II, run sample by sample, against the direct form I of the reference: the
    same outputs, and its zero-input state step is `state_matrix`."""
    rate = 22050
    (b, a), (c, d) = loudness_ref.kweighting(rate)
    rs = np.random.RandomState(3)
    x = rs.uniform(-1, 1, 500)
    s = np.zeros(4)
    ys = []
    for xn in list(x) + [0.0] * 3:
        y1 = b[0] * xn + s[0]
        y2 = c[0] * y1 + s[2]
        nxt = np.array([b[1] * xn - a[0] * y1 + s[1], b[2] * xn - a[1] * y1, c[1] * y1 - d[0] * y2 + s[3],
                        c[2] * y1 - d[1] * y2])
        if xn == 0.0 and len(ys) >= 500:
            assert np.allclose(nxt, loudness_ref.state_matrix(rate) @ s, rtol=1e-13, atol=1e-15)
        s = nxt
        ys.append(y2)
    want = loudness_ref._biquad(loudness_ref._biquad(list(x), b, a), c, d)
    assert np.allclose(ys[:500], want, rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize("rate", RATES)
def test_reference_reads_a_full_scale_997_hz_sine_at_minus_3_01(rate):
    """EBU Tech 3341's meter tolerance is +-0.1 LU."""
    t = np.arange(5 * rate) / rate
    got = loudness_ref.measure(np.sin(2 * np.pi * 997.0 * t), rate)
    assert abs(got["L"] - (-3.01)) <= 0.1, got["L"]
    assert got["keep"].all() and len(got["keep"]) == 50 - 3


def test_reference_edge_cases():
    rate = 8000
    H = loudness_ref.hop(rate)
    rs = np.random.RandomState(0)
    x = rs.uniform(-0.25, 0.25, 5 * H)
    assert loudness_ref.measure(x, rate, 3 * H)["L"] == -math.inf
    one, also_one = loudness_ref.measure(x, rate, 4 * H), loudness_ref.measure(x, rate, 5 * H - 1)
    assert len(one["l"]) == len(also_one["l"]) == 1 and one["L"] == also_one["L"] and math.isfinite(one["L"])
    assert loudness_ref.measure(np.zeros(4 * H), rate)["L"] == -math.inf


@pytest.mark.parametrize("rate", RATES + [1000, 11025, 96000])
def test_segments_agree_with_integer_division_around_every_boundary(rate):
    H = loudness_ref.hop(rate)
    assert H == (rate + 5) // 10
    if rate % 10 != 5:
        assert H == round(rate / 10)
    for k in range(0, 40):
        for d in (-1, 0, 1):
            n = k * H + d
            if n < 0:
                continue
            assert _capi.loudness_segments(rate, n) == (H, n // H), (rate, n)
    assert _capi.loudness_segments(rate, 3 * rate + 137) == (H, (3 * rate + 137) // H)


def test_host_entries_refuse_bad_arguments():
    for rate in (999, 0, -5):
        with pytest.raises(ValueError, match="at least 1000 Hz"):
            _capi.kweighting(rate)
        with pytest.raises(ValueError, match="at least 1000 Hz"):
            _capi.loudness_segments(rate, 100)
    with pytest.raises(ValueError, match="samples must be >= 0"):
        _capi.loudness_segments(8000, -1)


def test_loudness_arguments():
    assert wire.Loudness().target == -23.0 and wire.Loudness().max_gain_db == 20.0 and wire.Loudness().measured is None
    assert wire.Loudness(target=None).target is None
    for bad in (dict(target=float("nan")), dict(target=float("inf")), dict(max_gain_db=-1.0), dict(max_gain_db=39.5),
                dict(max_gain_db=float("nan")), dict(measured=float("nan")), dict(measured=float("inf"))):
        with pytest.raises(ValueError):
            wire.Loudness(**bad)
    assert wire.Loudness(measured=-math.inf).measured == -math.inf
    with pytest.raises(ValueError, match="only measures"):
        wire.Loudness(target=None).gain(torch.zeros(1))
    # the arguments of the entries, refused before anything touches a device
    with pytest.raises(TypeError):
        wire._loudness_arg(-23.0, None, "x", stream=True)
    with pytest.raises(ValueError, match="not both"):
        wire._loudness_arg(wire.Loudness(measured=-20.0), 0.5, "x", stream=True)
    with pytest.raises(ValueError, match="measured"):
        wire._loudness_arg(wire.Loudness(), None, "x", stream=True)
    with pytest.raises(ValueError, match="only measures"):
        wire._loudness_arg(wire.Loudness(target=None), None, "x", stream=False)
    assert wire._loudness_arg(None, 0.5, "x", stream=True) is None
    loud = wire.Loudness(target=None)
    assert wire._loudness_arg(loud, None, "x", stream=True) is loud
    with pytest.raises(ValueError, match="shape"):
        wire.Loudness(measured=torch.zeros(3)).measured_rows(2, "cpu")


def test_loudness_gain_and_peak_mapping():
    loud = wire.Loudness(target=-23.0, max_gain_db=20.0)
    L = torch.tensor([-23.0, -33.0, -13.0, -43.0, -60.0, -math.inf, -16.5], dtype=torch.float32)
    g = loud.gain(L)
    assert g.dtype == torch.float32
    want = [1.0, 10.0 ** 0.5, 10.0 ** -0.5, 10.0, 10.0, 1.0, 10.0 ** (-6.5 / 20)]
    assert np.allclose(g.numpy(), want, rtol=1e-6)
    assert float(g[3]) == float(g[4]) == float(np.float32(10.0))          # the cap, exactly
    assert float(g[5]) == 1.0                                             # -inf: unity
    # the documented fp32 formula, operation by operation
    f = torch.clamp(torch.pow(torch.full_like(L, 10.0), (-23.0 - L) / 20.0), max=10.0 ** (20.0 / 20.0))
    f = torch.where(torch.isneginf(L), torch.ones_like(f), f)
    assert torch.equal(g, f) and torch.equal(loud.peak(L), 0.9 / f)
    # the largest cap keeps the divisor above the kernels' 0.01 threshold
    p = wire.Loudness(target=0.0, max_gain_db=wire.Loudness.MAX_GAIN_DB).peak(torch.tensor([-200.0]))
    assert float(p[0]) > 0.01
    # measured as a float or a tensor
    assert torch.equal(wire.Loudness(measured=-20.0).measured_rows(2, "cpu"), torch.full((2,), -20.0))
    t = torch.tensor([-20.0, -30.0])
    assert torch.equal(wire.Loudness(measured=t).measured_rows(2, "cpu"), t)


@pytest.mark.parametrize("seed", range(6))
def test_streamed_plan_tiles_the_segments(seed):
    """for seeded chunk schedules the segments released per chunk tile [0, S), each at the first chunk that completes
    it"""
    rs = np.random.RandomState(seed)
    hop = int(rs.choice([800, 2205, 4800]))
    spf = 256
    frames, avail = 0, []
    for _ in range(int(rs.randint(1, 30))):
        frames += int(rs.choice([1, 5, 8, 16, 32, 64, 256]))
        avail.append(spf * frames)
    plan = wire.loudness_plan(avail, hop)
    S = avail[-1] // hop
    assert len(plan) == len(avail)
    done = 0
    for (k0, k1), a in zip(plan, avail):
        assert k0 == done and k1 == a // hop            # everything complete is released, nothing incomplete
        done = k1
    assert done == S
    # each segment at the FIRST chunk that completes it
    for k in range(S):
        first = next(i for i, a in enumerate(avail) if (k + 1) * hop <= a)
        assert plan[first][0] <= k < plan[first][1]
    with pytest.raises(ValueError):
        wire.loudness_plan(avail, 0)
