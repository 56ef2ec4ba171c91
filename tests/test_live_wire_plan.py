"""The live wire, host side (no GPU): which resampled samples of a recording that is still arriving are final
(`mbv_resample_ready_open`), that their values do not depend on what arrives later (float64 restatement of resampy),
and the integer planning of a whole live wire (`wire.LiveWirePlan`) against brute-force statements of the rules
(DESIGN §7.12)."""
import ctypes as C
import math

import numpy as np
import pytest

import resample_ref
from mb_istft_vits_amd import _capi, models, stream, utils as mutils, wire

PAIRS = [(48000, 22050), (44100, 22050), (16000, 22050), (8000, 16000), (22050, 24000)]
FILTERS = ["kaiser_best", "kaiser_fast"]
N_FFT, HOP, SPF = 1024, 256, 256
IN_SR, MODEL_SR, RATE = 48000, 22050, 24000


def _geom(orig, target, res_type):
    taps, left, phases = C.c_int32(), C.c_int32(), C.c_int32()
    filt = models.RESAMPLE_TYPES[res_type]
    assert _capi.lib().mbv_resample_bank(orig, target, filt, None, 0, C.byref(phases), C.byref(taps), C.byref(left)) == 0
    g = math.gcd(orig, target)
    assert phases.value == target // g
    return target // g, orig // g, taps.value, left.value            # L, M, K, left


@pytest.mark.parametrize("res_type", FILTERS)
@pytest.mark.parametrize("pair", PAIRS)
def test_ready_open_is_every_tap_below_the_frontier_and_needs_no_total(pair, res_type):
    orig, target = pair
    L, M, K, left = _geom(orig, target, res_type)
    lib, filt = _capi.lib(), models.RESAMPLE_TYPES[res_type]
    t, prev, steps = 0, 0, 0                                       # t: the brute-force count, carried (it is monotone)
    for avail in range(0, 3 * K + 1):
        got = lib.mbv_resample_ready_open(orig, target, filt, avail)
        assert got == wire.resample_ready_open(orig, target, avail, res_type)
        # the open branch of mbv_resample_ready, whatever the total
        assert got == lib.mbv_resample_ready(orig, target, filt, avail, avail + 1), avail
        assert got == lib.mbv_resample_ready(orig, target, filt, avail, avail + 10 ** 6), avail
        assert got >= prev
        # brute force: output t is final iff every index it may read (row L reads one further left) exists
        while all(j < avail for j in range(t * M // L - left - 1, t * M // L - left + K)):
            t += 1
        assert got == t, (avail, got, t)
        steps += got > prev
        prev = got
    assert steps >= K and prev > 0                                 # the count moved: every step of it was crossed
    assert lib.mbv_resample_ready_open(orig, target, filt, -5) == 0
    assert lib.mbv_resample_ready_open(orig, orig, filt, 77) == 77   # equal rates: the samples themselves


@pytest.mark.parametrize("res_type", FILTERS)
@pytest.mark.parametrize("pair", [(48000, 22050), (16000, 22050)])
def test_final_outputs_do_not_change_when_more_arrives(pair, res_type):
    """Float64 restatement of resampy: the outputs below the open count computed from x[:in_avail] alone equal those
    of the whole row.  Observed here: 0.0 in all twelve cases (the same taps times the same weights in the same order;
    the samples that differ meet no weight), against the bar of 1e-12."""
    orig, target = pair
    x = np.random.RandomState(5).standard_normal(2000)
    whole = resample_ref.resample(x, orig, target, res_type)
    for avail in (500, 501, 1237):
        r = wire.resample_ready_open(orig, target, avail, res_type)
        assert 0 < r <= resample_ref.out_len(avail, orig, target)
        part = resample_ref.resample(x[:avail], orig, target, res_type)
        diff = float(np.max(np.abs(part[:r] - whole[:r])))
        print("%d -> %d %s, %d of 2000 samples: %d outputs final, max difference %.3e" % (orig, target, res_type, avail, r, diff))
        assert diff <= 1e-12, (avail, diff)


def _net(name="uudb_ms_istft_vits_ms"):
    hps = mutils.get_hparams_from_file(mutils.builtin_config(name))
    return models.SynthesizerTrn(59, hps.data.filter_length // 2 + 1, hps.train.segment_size // hps.data.hop_length,
                                 n_speakers=hps.data.n_speakers, **hps.model)


def _pushes(rs, n):
    out, left = [], n
    top = int(rs.choice([90, 1500, 11000, 130000]))
    while left:
        k = min(left, int(rs.randint(1, top + 1)))
        out.append(k)
        left -= k
    return out


def _model_total(n_raw):
    return int(math.ceil(n_raw * (float(MODEL_SR) / IN_SR)))


@pytest.mark.parametrize("T", [1, 17, 256, 257, 300])
def test_random_push_patterns_feed_decode_and_wire_at_the_first_moment(T):
    net = _net()
    cfg = net._config_struct()
    r_conv, r_dec = net.converter_context()[1], stream.decoder_context(cfg)[1]
    pad = (N_FFT - HOP) // 2
    rs = np.random.RandomState(2000 + T)
    need = np.arange(T) * HOP - pad + N_FFT               # the model-rate sample count at which frame f has all its samples
    lib = _capi.lib()
    for case in range(200):
        # a raw length that gives T frames at the model's rate
        n = int(math.ceil((HOP * T + int(rs.randint(0, HOP - 1))) * IN_SR / MODEL_SR))
        total = _model_total(n)
        assert lib.mbv_spectrogram_frames(total, N_FFT, HOP) == T
        sc = (8, 32) if case % 2 else (32, 256)
        sched = stream.chunk_schedule(T, *sc)
        cf = (1, 16, 32, 64)[case % 4]
        plan = stream.LivePlan(N_FFT, HOP, r_conv, r_dec, *sc, convert_frames=cf)
        wp = wire.LiveWirePlan(IN_SR, MODEL_SR, RATE, plan, SPF, n + int(rs.randint(0, 5000)))
        assert wp.capacity == _model_total(wp.max_raw) and wp.o_capacity == SPF * lib.mbv_spectrogram_frames(wp.capacity, N_FFT, HOP)
        valid = wire.resample_ready(MODEL_SR, RATE, SPF * T, SPF * T)
        chunks, pieces, fed, raw, z_done = [], [], 0, 0, 0
        for ev in _pushes(rs, n) + [None]:                # None = close()
            closed = ev is None
            if closed:
                wp.close()
            else:
                wp.push(ev)
                raw += ev
            # -- input: the rules restated
            arrived = total if closed else wire.resample_ready_open(IN_SR, MODEL_SR, raw)
            due = wp.feed_due()
            assert due == ((fed, arrived - fed) if arrived > fed or closed else None), (case, ev)
            if due:
                assert due[1] >= 0
                plan.push(due[1])                         # what LiveStream.fed(count, last) does
                if wp.fed(due[1]):
                    plan.close()
                fed += due[1]
            assert plan.arrived == fed == wp.fed_samples and plan.closed == closed
            assert wp.feed_due() is None
            # -- conversion and decoding, as tests/test_live_plan.py restates them, on the fed samples
            spec_final = T if closed else int((need <= fed).sum())
            z_may = T if closed else max(0, spec_final - r_conv)
            got = plan.convert_due()
            assert got == ((z_done, z_may) if z_may > z_done and (closed or z_may - z_done >= cf) else None), (case, ev)
            if got:
                plan.converted(*got)
                z_done = got[1]
            want_chunks = []
            for c in sched[len(chunks):]:
                if not (closed or z_done >= c[0] + c[1] + r_dec):
                    break
                want_chunks.append(c)
            got_chunks = plan.decodable()
            assert got_chunks == want_chunks, (case, ev)
            for c in got_chunks:
                plan.released(*c)
                chunks.append(c)
            # -- output: one piece per decoded chunk, final with the last chunk
            w = wp.wire_due(chunks)
            if not got_chunks:
                assert w is None
                continue
            in_avail, in_total, out_first, out_count, final, new = w
            assert final == (closed and len(chunks) == len(sched)) and len(new) == len(got_chunks)
            assert in_avail == SPF * (chunks[-1][0] + chunks[-1][1])
            assert in_total == (SPF * T if final else wp.o_capacity)
            a = pieces[-1][1] if pieces else 0
            assert out_first == a and out_count == new[-1][1] - a
            for k, (first, count) in enumerate(got_chunks):
                end = SPF * (first + count)
                last = final and k == len(got_chunks) - 1
                b = valid if last else wire.resample_ready(MODEL_SR, RATE, end, 10 ** 9)
                assert new[k] == (a, b) and b <= valid
                a = b
            # what the C entry will check for this launch
            assert out_first + out_count <= wire.resample_ready(MODEL_SR, RATE, in_avail, in_total)
            pieces += new
            wp.wired(len(chunks), new[-1][1], final)
            assert wp.wire_due(chunks) is None
        assert fed == total and chunks == sched and plan.all_released
        assert wp.wire_done and wp.valid == valid
        assert pieces[0][0] == 0 and pieces[-1][1] == valid and len(pieces) == len(sched)
        assert all(p[1] == q[0] for p, q in zip(pieces, pieces[1:])) and all(b >= a for a, b in pieces)
        with pytest.raises(ValueError):
            wp.push(1)


def test_equal_rates_push_straight_through_and_refusals():
    plan = stream.LivePlan(N_FFT, HOP, 96, 26, 8, 32, 4)
    wp = wire.LiveWirePlan(MODEL_SR, MODEL_SR, MODEL_SR, plan, SPF, HOP * 40)
    assert not wp.resamples and wp.capacity == HOP * 40 and wp.pcm_capacity == wp.o_capacity == SPF * 40
    wp.push(1000)
    assert plan.arrived == 1000 == wp.raw and wp.feed_due() is None
    with pytest.raises(ValueError, match="capacity"):
        wp.push(HOP * 40)
    wp.close()
    assert plan.closed and wp.total == 1000
    with pytest.raises(ValueError, match="after close"):
        wp.push(1)
    # a recording that gives no frame cannot be closed, and stays open
    wp = wire.LiveWirePlan(IN_SR, MODEL_SR, RATE, stream.LivePlan(N_FFT, HOP, 96, 26, 8, 32, 4), SPF, 48000)
    wp.push(100)
    with pytest.raises(ValueError, match="no spectrogram frame"):
        wp.close()
    assert not wp.closed
    wp.push(2000)
    wp.close()
    assert wp.total == _model_total(2100) and wp.feed_due() == (0, wp.total)
    with pytest.raises(ValueError):
        wire.LiveWirePlan(IN_SR, MODEL_SR, RATE, plan, SPF, 0)
    with pytest.raises(ValueError):
        wire.LiveWirePlan(IN_SR, MODEL_SR, RATE, plan, SPF, 1000, res_type="soxr_hq")
    with pytest.raises(_capi.MbvError):
        wire.LiveWirePlan(44100, 48001, RATE, plan, SPF, 48000)          # more than 4096 phases
