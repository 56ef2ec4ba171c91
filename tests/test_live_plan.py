"""Live voice conversion, host side (no GPU): which spectrogram frames, z_hat frames and decoder chunks of a recording
that is still arriving are final (`mbv_spectrogram_ready`, `stream.LivePlan`), against brute-force statements of the
rules."""
import ctypes as C

import numpy as np
import pytest

from mb_istft_vits_amd import _capi, models, stream, utils as mutils

N_FFT, HOP = 1024, 256


def _net(name="uudb_ms_istft_vits_ms"):
    hps = mutils.get_hparams_from_file(mutils.builtin_config(name))
    return models.SynthesizerTrn(59, hps.data.filter_length // 2 + 1, hps.train.segment_size // hps.data.hop_length,
                                 n_speakers=hps.data.n_speakers, **hps.model)


def _ready_brute(arrived, n_fft, hop):
    """Leading frames every sample of which exists: frame f reads [f hop - pad, f hop - pad + n_fft), and the samples
    below 0 are the left padding."""
    pad = (n_fft - hop) // 2
    f = 0
    while all(j < arrived for j in range(max(f * hop - pad, 0), f * hop - pad + n_fft)):
        f += 1
    return f


@pytest.mark.parametrize("n_fft", [256, 1024])
@pytest.mark.parametrize("hop", [64, 256, 1024])
def test_spectrogram_ready_is_every_sample_of_the_frame_exists(n_fft, hop):
    L = _capi.lib()
    if hop > n_fft:
        assert L.mbv_spectrogram_ready(1000, 0, n_fft, hop) == -1 and L.mbv_spectrogram_ready(1000, 1, n_fft, hop) == -1
        return
    pad = (n_fft - hop) // 2
    counts = {0, 1, n_fft - 1, n_fft, n_fft + 1}
    for f in range(6):
        b = f * hop - pad + n_fft                        # the first count at which frame f is final
        counts |= {max(b + d, 0) for d in (-2, -1, 0, 1, 2)}
    seen = set()
    for n in sorted(counts):
        want = _ready_brute(n, n_fft, hop)
        assert L.mbv_spectrogram_ready(n, 0, n_fft, hop) == want == stream.spectrogram_ready(n, False, n_fft, hop), n
        total = L.mbv_spectrogram_frames(n, n_fft, hop)
        assert L.mbv_spectrogram_ready(n, 1, n_fft, hop) == total
        assert want <= total                             # closing never takes a frame back
        seen.add(want)
    assert seen >= set(range(6))                         # every boundary was crossed
    assert L.mbv_spectrogram_ready(-1, 0, n_fft, hop) == -1 and L.mbv_spectrogram_ready(5, 0, 300, hop) == -1


def test_converter_context_is_the_layer_sum():
    for name in ("uudb_ms_istft_vits_ms", "ljs_ms_istft_vits", "ljs_mini_mb_istft_vits"):
        net = _net(name)
        assert net.converter_context() == (96, 96)       # (16 + 2 * 4 * 4) layers of k = 5, dilation 1: 2 frames a side
    assert _capi.lib().mbv_converter_context(None, None) != 0


def test_convert_window_is_the_context_clipped_and_aligned():
    net = _net()
    cfg = net._config_struct()
    L, R = net.converter_context()
    out = (C.c_int32 * 2)()
    for first, count, final in [(0, 32, 200), (100, 32, 400), (133, 7, 236), (300, 50, 350), (97, 1, 98), (500, 64, 10000)]:
        assert _capi.lib().mbv_convert_window(C.byref(cfg), first, count, final, C.byref(out)) == 0
        wa, wb = out[0], out[1]
        assert wa % 32 == 0 and wa <= max(0, first - L) < wa + 32
        assert wb == min(final, first + count + R)
    assert _capi.lib().mbv_convert_window(C.byref(cfg), 10, 5, 14, C.byref(out)) != 0      # frames that do not exist
    assert _capi.lib().mbv_convert_window(C.byref(cfg), -1, 5, 100, C.byref(out)) != 0
    wl = (C.c_int32 * 3)(224, 300, 64)
    run_of = (C.c_int32 * 3)()
    assert _capi.lib().mbv_convert_ranges_plan(C.byref(cfg), 3, wl, run_of) == 1 and list(run_of) == [0, 0, 0]
    assert _capi.lib().mbv_convert_ranges_plan(C.byref(cfg), 3, (C.c_int32 * 3)(224, 0, 64), run_of) == -1


def _pushes(rs, n):
    """A random way of cutting n samples: a few sizes of scale, so that pushes of one sample and of seconds both occur."""
    out, left = [], n
    top = int(rs.choice([40 if n < 100000 else 400, 700, 5000, 60000]))
    while left:
        k = min(left, int(rs.randint(1, top + 1)))
        out.append(k)
        left -= k
    return out


@pytest.mark.parametrize("T", [1, 17, 256, 257, 300, 1000])
def test_random_push_patterns_release_the_schedule_at_the_first_moment(T):
    net = _net()
    cfg = net._config_struct()
    r_conv, r_dec = net.converter_context()[1], stream.decoder_context(cfg)[1]
    pad = (N_FFT - HOP) // 2
    rs = np.random.RandomState(1000 + T)
    need = np.arange(T) * HOP - pad + N_FFT               # the sample count at which frame f has all its samples
    for case in range(200):
        n = HOP * T + int(rs.randint(0, HOP))             # T frames (center=False with pad (n_fft - hop) / 2 each side)
        assert _capi.lib().mbv_spectrogram_frames(n, N_FFT, HOP) == T
        sched = stream.chunk_schedule(T, *((8, 32) if case % 2 else (32, 256)))
        cf = (1, 16, 32, 64)[case % 4]
        plan = stream.LivePlan(N_FFT, HOP, r_conv, r_dec, *((8, 32) if case % 2 else (32, 256)), convert_frames=cf)
        ranges, chunks = [], []
        z_done, arrived = 0, 0                            # the brute-force side
        events = _pushes(rs, n) + [None]                  # None = close()
        for ev in events:
            if ev is None:
                plan.close()
            else:
                plan.push(ev)
                arrived += ev
            closed = ev is None
            # the rules, restated: frames whose samples all exist; z frames with their right context; the batching
            spec_final = T if closed else int((need <= arrived).sum())
            z_may = T if closed else max(0, spec_final - r_conv)
            want_range = (z_done, z_may) if z_may > z_done and (closed or z_may - z_done >= cf) else None
            got = plan.convert_due()
            assert got == want_range, (case, ev, got, want_range)
            if got:
                plan.converted(*got)
                ranges.append(got)
                z_done = got[1]
            want_chunks = [c for c in sched[len(chunks):] if closed or z_done >= c[0] + c[1] + r_dec]
            if not closed:                                # an open recording never releases past a gap
                k = 0
                while k < len(want_chunks) and want_chunks[k] == sched[len(chunks) + k]:
                    k += 1
                want_chunks = want_chunks[:k]
            got_chunks = plan.decodable()
            assert got_chunks == want_chunks, (case, ev, got_chunks, want_chunks)
            for c in got_chunks:
                plan.released(*c)
                chunks.append(c)
            assert plan.convert_due() is None and plan.decodable() == []      # one pass takes everything
        assert chunks == sched and plan.all_released
        # the converted ranges tile [0, T): no frame twice, none left out
        assert ranges[0][0] == 0 and ranges[-1][1] == T
        assert all(a[1] == b[0] for a, b in zip(ranges, ranges[1:])) and all(b > a for a, b in ranges)
        with pytest.raises(ValueError):
            plan.push(1)


def test_plan_refuses_out_of_order_marks():
    plan = stream.LivePlan(N_FFT, HOP, 96, 26, 8, 32, 4)
    plan.push(HOP * 400)
    a, b = plan.convert_due()
    with pytest.raises(ValueError):
        plan.converted(a + 1, b)
    plan.converted(a, b)
    with pytest.raises(ValueError):
        plan.converted(a, b)                              # a frame is converted once
    with pytest.raises(ValueError):
        plan.released(8, 16)
    with pytest.raises(ValueError):
        stream.LivePlan(N_FFT, HOP, 96, 26, 8, 4, 4)
    with pytest.raises(ValueError):
        stream.LivePlan(N_FFT, HOP, 96, 26, 8, 32, 0)
