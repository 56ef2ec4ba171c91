"""Live voice conversion with a bounded look-ahead, the rules in integers (no GPU): `mbv_convert_window_ahead`,
`stream.Ahead`, the grid of `stream.LivePlan(ahead=)`, the canonical t_frames of every chunk, `LivePlan.lag()` and the
refusals."""
import ctypes as C

import numpy as np
import pytest

from mb_istft_vits_amd import _capi, stream
from mb_istft_vits_amd.stream import Ahead, LivePlan, chunk_schedule, spectrogram_ready

N_FFT, HOP, SPF, SR = 1024, 256, 256, 16000
R_CONV, R_DEC = 96, 24


def _cfg():
    from mb_istft_vits_amd import models, utils as mutils
    hps = mutils.get_hparams_from_file(mutils.builtin_config("uudb_ms_istft_vits_ms"))
    net = models.SynthesizerTrn(59, hps.data.filter_length // 2 + 1, hps.train.segment_size // hps.data.hop_length,
                                n_speakers=hps.data.n_speakers, **hps.model)
    return net._config_struct()


def test_the_contexts_are_the_ones_this_file_assumes():
    cfg = _cfg()
    assert stream.converter_context(cfg)[1] == R_CONV and stream.decoder_context(cfg)[1] == R_DEC


def test_convert_window_ahead_against_a_restatement():
    cfg, L, out = _cfg(), _capi.lib(), (C.c_int32 * 2)()
    n = 0
    for first in (0, 1, 31, 32, 95, 96, 97, 127, 128, 129, 200):
        for count in (1, 4, 32):
            for ahead in (0, 1, 8, 95, 96):
                for final in {first + count, first + count + ahead - 1, first + count + ahead, first + count + ahead + 1,
                              first + count + 200}:
                    if final < first + count:
                        continue
                    assert L.mbv_convert_window_ahead(C.byref(cfg), first, count, ahead, final, C.byref(out)) == 0
                    assert (out[0], out[1]) == (max(first - R_CONV, 0) // 32 * 32, min(first + count + ahead, final))
                    n += 1
            # the full reach is mbv_convert_window
            ref = (C.c_int32 * 2)()
            assert L.mbv_convert_window(C.byref(cfg), first, count, first + count + 50, C.byref(ref)) == 0
            assert L.mbv_convert_window_ahead(C.byref(cfg), first, count, R_CONV, first + count + 50, C.byref(out)) == 0
            assert tuple(ref) == tuple(out)
    assert n > 500
    for bad in [(0, 4, -1, 10), (0, 4, R_CONV + 1, 200), (-1, 4, 8, 10), (0, 0, 8, 10), (0, 4, 8, 3)]:
        assert L.mbv_convert_window_ahead(C.byref(cfg), *bad, C.byref(out)) == 1
    assert L.mbv_convert_window_ahead(None, 0, 4, 8, 10, C.byref(out)) == 1


def _plan(ahead, cf, c, cap, **kw):
    return LivePlan(N_FFT, HOP, R_CONV, R_DEC, c, cap, cf, ahead=ahead, **kw)


def _samples_of(T, rem):
    """A recording of T frames: mbv_spectrogram_frames(n) = n // hop for this n_fft / hop."""
    n = HOP * T + rem
    assert spectrogram_ready(n, True, N_FFT, HOP) == T
    return n


def _pushes(n, rs):
    kind = rs.randint(4)
    if kind == 0:
        return [n]
    hi = (HOP // 2, 2 * HOP, 5000, 30000)[rs.randint(4)]
    out, left = [], n
    while left:
        k = min(left, int(rs.randint(1, hi + 1)))
        out.append(k)
        left -= k
    return out


def _run(plan, sizes):
    """Drive a plan as `LiveStream.poll` does after every push; -> (blocks [(a, b, arrived, closed)], chunks [(first,
    count, t_frames, overhang, arrived, closed)])."""
    blocks, chunks = [], []

    def poll():
        for a, b in plan.due_blocks():
            blocks.append((a, b, plan.arrived, plan.closed))
            plan.converted(a, b)
        for first, count in plan.decodable():
            chunks.append((first, count, plan.t_frames(first, count), plan.overhang(first, count), plan.arrived, plan.closed))
            plan.released(first, count)

    for k in sizes:
        plan.push(k)
        poll()
    plan.close()
    poll()
    assert plan.all_released and plan.due_blocks() == [] and plan.decodable() == []
    return blocks, chunks


SETTINGS = [(Ahead(8, 4), 4, 4, 4), (Ahead(0, 1), 1, 1, 1), (Ahead(8, 4), 8, 8, 8), (Ahead(16, 8), 5, 3, 24),
            (Ahead(0, 0), 7, 2, 256), (Ahead(32, 12, seam_ms=5.0), 4, 4, 64), (Ahead(R_CONV, R_DEC), 32, 32, 256)]


@pytest.mark.parametrize("T", [1, 17, 256, 257, 300])
def test_the_grid_and_the_chunks_do_not_depend_on_the_pushes(T):
    rs = np.random.RandomState(T)
    for p in range(200):
        ahead, cf, c, cap = SETTINGS[p % len(SETTINGS)]
        n = _samples_of(T, int(rs.randint(HOP)))
        sizes = _pushes(n, rs)
        plan = _plan(ahead, cf, c, cap, model_sr=SR, samples_per_frame=SPF)
        blocks, chunks = _run(plan, sizes)
        what = (T, ahead, cf, c, cap, sizes[:4])
        # the converted ranges are exactly the grid blocks
        assert [(a, b) for a, b, _, _ in blocks] == [(a, min(a + cf, T)) for a in range(0, T, cf)], what
        # ... each at the first push after which its window's end E_k is final (or at the close)
        arrived_after = np.cumsum(sizes)
        for a, b, arrived, closed in blocks:
            need = b + ahead.conv
            ok = [int(x) for x in arrived_after if spectrogram_ready(int(x), False, N_FFT, HOP) >= need and b == a + cf]
            assert (arrived, closed) == ((ok[0], False) if ok else (n, True)), what + (a, b)
        # the chunks are the schedule, each with t_frames = D and the overhang of the seam
        assert [(f, k) for f, k, _, _, _, _ in chunks] == chunk_schedule(T, c, cap), what
        over = -(-plan.seam // SPF)
        uncut = chunk_schedule(T + cap, c, cap)
        for (f, k, t, ov, arrived, closed), (_, full) in zip(chunks, uncut):
            D = min(f + k + ahead.dec, T)
            assert t == D and ov == min(over, D - f - k), what + (f, k)
            # ... released at the first poll at which the blocks up to D are converted; while the recording is open T is
            # not known, so that is D of the uncut chunk, unclipped
            ok = [(x, cl) for _, b, x, cl in blocks if b >= f + full + ahead.dec and not cl]
            assert (arrived, closed) == (ok[0] if ok else (n, True)), what + (f, k)


def test_the_full_reach_releases_what_the_plain_plan_releases():
    """Ahead(R_conv, R_dec) converts on a grid where the plain plan converts whatever came due, so the ranges differ;
    the chunks, and the push after which each is handed out, agree whenever conversion keeps up (convert_frames 1)."""
    rs = np.random.RandomState(5)
    for T in (1, 17, 256, 257, 300):
        for p in range(40):
            c, cap = ((4, 4), (8, 32), (32, 256))[p % 3]
            n = _samples_of(T, int(rs.randint(HOP)))
            sizes = _pushes(n, rs)
            _, got = _run(_plan(Ahead(R_CONV, R_DEC), 1, c, cap), sizes)
            _, want = _run(_plan(None, 1, c, cap), sizes)
            assert [(f, k, a, cl) for f, k, _, _, a, cl in got] == [(f, k, a, cl) for f, k, _, _, a, cl in want]
            assert all(t == min(f + k + R_DEC, T) for f, k, t, _, _, _ in got)


@pytest.mark.parametrize("ahead,cf,c,cap", [(Ahead(8, 4), 4, 4, 4), (Ahead(0, 1), 1, 1, 1), (Ahead(16, 8), 5, 3, 24),
                                            (None, 8, 8, 8), (Ahead(4, 2), 3, 2, 7)])
def test_lag_equals_a_brute_force_simulation(ahead, cf, c, cap):
    arrived, steady = _plan(ahead, cf, c, cap).lag()
    # sample by sample around the predicted count: nothing is released one sample earlier
    for n, want in ((arrived - 1, 0), (arrived, 1)):
        plan = _plan(ahead, cf, c, cap)
        got = 0
        whole = (n - 2 * HOP) // HOP                       # frame by frame, then the rest one sample at a time
        for k in [n - 2 * HOP - HOP * (whole - 1)] + [HOP] * (whole - 1) + [1] * (2 * HOP):
            plan.push(k)
            for a, b in plan.due_blocks():
                plan.converted(a, b)
            for ch in plan.decodable():
                plan.released(*ch)
                got += 1
        assert min(got, 1) == want
    # frame by frame over a long recording: the distance from a full-size chunk's first frame to the final frames at its
    # release, the largest over the chunks
    plan, worst = _plan(ahead, cf, c, cap), 0
    base = N_FFT - (N_FFT - HOP) // 2 - HOP
    plan.push(base)
    assert plan.spec_final == 0
    for f in range(1, 40 * cap + 400):
        plan.push(HOP)
        assert plan.spec_final == f
        for a, b in plan.due_blocks():
            plan.converted(a, b)
        for first, count in plan.decodable():
            plan.released(first, count)
            if count == cap:
                worst = max(worst, f - first)
    assert worst == steady


def test_the_worked_example():
    """uudb: n_fft 1024, hop 256, convert_frames 4, chunks of 4, Ahead(8, 4): first audio after 4 480 samples."""
    assert _plan(Ahead(8, 4), 4, 4, 4).lag() == (4480, 16)
    assert _plan(None, 8, 8, 8).lag()[0] == 127 * HOP + 640         # 2.07 s at 16 kHz: (8 + 24 + 96) frames


def test_ahead_refusals():
    for bad in [(1.0, 2), (2, "3"), (True, 2), (None, 1)]:
        with pytest.raises(TypeError):
            Ahead(*bad)
    with pytest.raises(TypeError):
        Ahead(1, 1, seam_ms="5")
    for bad in [(-1, 2), (2, -1)]:
        with pytest.raises(ValueError):
            Ahead(*bad)
    for ms in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            Ahead(1, 1, seam_ms=ms)
    assert (Ahead(np.int64(3), 2).conv, Ahead(3, 2).dec, Ahead(3, 2, seam_ms=5).seam_samples(SR)) == (3, 2, 80)


def test_plan_refusals():
    with pytest.raises(TypeError):
        _plan((8, 4), 4, 4, 4)
    with pytest.raises(ValueError, match="further"):
        _plan(Ahead(R_CONV + 1, 4), 4, 4, 4)
    with pytest.raises(ValueError, match="further"):
        _plan(Ahead(8, R_DEC + 1), 4, 4, 4)
    with pytest.raises(ValueError, match="model_sr"):
        _plan(Ahead(8, 4, seam_ms=5.0), 4, 4, 4)
    kw = dict(model_sr=SR, samples_per_frame=SPF)
    assert _plan(Ahead(8, 4, seam_ms=5.0), 4, 4, 4, **kw).seam == 80
    with pytest.raises(ValueError, match="seam"):
        _plan(Ahead(8, 0, seam_ms=5.0), 4, 4, 4, **kw)              # no decoder look-ahead to take an overhang from
    with pytest.raises(ValueError, match="seam"):
        _plan(Ahead(8, 1, seam_ms=20.0), 4, 4, 4, **kw)             # 320 samples > 256 = spf * dec
    with pytest.raises(ValueError, match="seam"):
        _plan(Ahead(8, 4, seam_ms=0.01), 4, 4, 4, **kw)             # rounds to 0 samples
    with pytest.raises(ValueError, match="seam"):
        _plan(Ahead(8, 4, seam_ms=20.0), 4, 1, 4, **kw)             # longer than the smallest chunk
    plan = _plan(Ahead(8, 4), 4, 4, 4)
    plan.push(HOP * 40)
    (a, b), *_ = plan.due_blocks()
    with pytest.raises(ValueError):
        plan.converted(a + 4, b + 4)                                # blocks are converted in order
