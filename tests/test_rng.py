"""The seeded noise generator without a GPU: the float64 / plain-integer restatement against the
specification's known answers, `mbv_randn_host` against the restatement, and the argument checks of `seed=`."""
import ctypes as C

import numpy as np
import pytest

import rng_ref
from mb_istft_vits_amd import _capi, models

# |n| <= sqrt(2 * 24 * ln 2) = 5.77; fp32 logf, sqrtf and the sine / cosine are each good to a few ulp, which puts the
# fp32 transform below about 3e-6 of the float64 one.  1e-5 leaves 3x over that and is five orders below what a wrong
# word or lane gives.
TOL = 1e-5


def _host(seed, purpose, row, c, first, count):
    buf = np.full(count + 2, 7.0, dtype=np.float32)           # one sentinel either side
    rc = _capi.lib().mbv_randn_host(seed, purpose, row, c, first, count, C.c_void_p(buf.ctypes.data + 4))
    assert rc == 0, _capi.lib().mbv_last_error(None)
    assert buf[0] == 7.0 and buf[-1] == 7.0
    return buf[1:-1].copy()


def test_reference_known_answers():
    hexs = lambda w: " ".join("%08x" % v for v in w)
    assert hexs(rng_ref.philox4x32_10((0, 0, 0, 0), (0, 0))) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    f = 0xFFFFFFFF
    assert hexs(rng_ref.philox4x32_10((f, f, f, f), (f, f))) == "408f276d 41c83b0e a20bc7c6 6d5451fd"
    assert hexs(rng_ref.philox4x32_10((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0))) \
        == "d16cfe09 94fdcceb 5001e420 24126ea1"


def test_reference_worked_draw():
    assert rng_ref.words(1234, 0, 0, 3, 2) == (4238247082, 2737379594, 2501674739, 3420831989)
    got = rng_ref.randn_row(1234, 0, 0, 3, 8, 4)
    want = [-0.10601855956, -0.12388860715, 0.29930284658, -0.99568311786]
    assert np.abs(got - want).max() < 1e-10, got


SHAPES = [(1, 0), (3, 1), (4, 0), (5, 3), (9, 2), (64, 5)]            # (count, first)


@pytest.mark.parametrize("seed", [0, 1234, 2 ** 64 - 1])
def test_host_entry_matches_reference(seed):
    worst = 0.0
    for count, first in SHAPES:
        for c in (0, 3, 191):
            for purpose in (0, 1, 2):
                for row in (0, 7):
                    got = _host(seed, purpose, row, c, first, count)
                    ref = rng_ref.randn_row(seed, purpose, row, c, first, count)
                    err = float(np.abs(got.astype(np.float64) - ref).max())
                    worst = max(worst, err)
                    assert err < TOL, (seed, purpose, row, c, first, count, err)
    print("mbv_randn_host vs float64 reference, seed %d: max abs err %.3e" % (seed, worst))


def test_host_entry_lane_rule():
    """A fill of [first, first + count) is bitwise the slice of a fill of [0, first + count)."""
    for count, first in SHAPES:
        for seed, purpose, row, c in ((0, 0, 0, 0), (1234, 1, 7, 3), (2 ** 64 - 1, 2, 7, 191)):
            whole = _host(seed, purpose, row, c, 0, first + count)
            part = _host(seed, purpose, row, c, first, count)
            assert np.array_equal(part.view(np.uint32), whole[first:].view(np.uint32)), (count, first)


def test_host_entry_refusals():
    L = _capi.lib()
    buf = np.zeros(4, dtype=np.float32)
    p = C.c_void_p(buf.ctypes.data)
    assert L.mbv_randn_host(1, 3, 0, 0, 0, 1, p) == 1 and b"purpose" in L.mbv_last_error(None)
    assert L.mbv_randn_host(1, 0, 0, 0, -1, 1, p) == 1
    assert L.mbv_randn_host(1, 0, 0, 0, 0, -1, p) == 1
    assert L.mbv_randn_host(1, 0, 0, 0, (1 << 30) - 1, 2, p) == 1 and b"2^30" in L.mbv_last_error(None)
    assert L.mbv_randn_host(1, 0, 0, 0, 0, 1, None) == 1
    assert L.mbv_randn_host(1, 0, 0, 0, 0, 0, None) == 0                  # nothing to write
    assert L.mbv_randn_host(1, 0, 0, 0, (1 << 30) - 1, 1, p) == 0        # the last frame an utterance can have
    assert np.abs(buf[0] - rng_ref.randn_row(1, 0, 0, 0, (1 << 30) - 1, 1)[0]) < TOL


def test_reference_distribution_guard():
    """A condition on the specified generator, not a measurement: 80 000 draws of seed 1234."""
    x = np.concatenate([rng_ref.normals_of(rng_ref.words(1234, 0, 0, 0, b)) for b in range(20000)])
    assert abs(x.mean()) < 0.02 and abs(x.std() - 1.0) < 0.02, (x.mean(), x.std())


def test_request_seed_checks():
    for bad in (-1, 2 ** 64):
        with pytest.raises(ValueError):
            models.Request([1, 2, 3], seed=bad)
    for bad in (1.5, True):
        with pytest.raises(TypeError):
            models.Request([1, 2, 3], seed=bad)
    assert models.Request([1, 2, 3], seed=5).seed == 5
    assert models.Request([1, 2, 3], seed=2 ** 64 - 1).seed == 2 ** 64 - 1
    assert models.Request([1, 2, 3]).seed is None
    wave = np.zeros(8, dtype=np.float32)
    for bad, exc in ((-1, ValueError), (2 ** 64, ValueError), (1.5, TypeError), (True, TypeError)):
        with pytest.raises(exc):
            models.ConvertRequest(wave, 0, 1, 22050, 256, 1024, seed=bad)
    assert models.ConvertRequest(wave, 0, 1, 22050, 256, 1024, seed=np.int64(9)).seed == 9


def test_row_seeds():
    """An int gives row b the sub-stream (s, b); a sequence or an integer tensor gives row b (seed_b, 0)."""
    import torch
    assert models._row_seeds(None, 3) is None
    assert list(models._row_seeds(7, 3)) == [(7, 0), (7, 1), (7, 2)]
    assert list(models._row_seeds([5, 6, 2 ** 64 - 1], 3)) == [(5, 0), (6, 0), (2 ** 64 - 1, 0)]
    assert list(models._row_seeds(torch.tensor([5, 6], dtype=torch.int64), 2)) == [(5, 0), (6, 0)]
    for bad in ([1, 2], torch.tensor([1, 2, 3, 4])):
        with pytest.raises(ValueError):
            models._row_seeds(bad, 3)
    with pytest.raises(ValueError):
        models._row_seeds([1, -2, 3], 3)
    for bad in (1.5, True, [1, 2.0, 3], torch.tensor([1.0, 2.0, 3.0])):
        with pytest.raises(TypeError):
            models._row_seeds(bad, 3)
