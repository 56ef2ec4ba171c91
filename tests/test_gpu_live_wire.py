"""The live wire on the MI355X: raw samples at the caller's rate in while the recording arrives, int16 at the service's
rate out (`wire.convert_live_pcm16`, `PcmPool.add_live`, `mbv_resample_ranges`).  The result does not depend on how
the recording was cut into pushes, and for more than 256 frames it is bitwise the one-shot chain."""
import math

import numpy as np
import pytest
import torch

from mb_istft_vits_amd import _capi, stream, synth, wire
from mb_istft_vits_amd.models import ConvertRequest

from gpu_util import make_net

pytestmark = pytest.mark.gpu

MODEL_SR, HOP, WIN, N_FFT, SPF = 22050, 256, 1024, 1024, 256
CHAINS = [(48000, 24000), (16000, 22050)]            # (in_sr, rate) around the model's 22050
SRC, TGT = 3, 7
SCHEDULES = [(32, 256), (8, 32)]
PATTERNS = ["one", "20ms", "random", "short_of_boundaries", "all_then_close"]
_NETS = {}


def _net(name="uudb_ms_istft_vits_ms"):
    if name not in _NETS:
        _NETS[name] = make_net(name)
    return _NETS[name][0]


def _counters(net):
    return net.input_runs(), net.converter_runs(), net.decoder_runs(), wire.wire_runs(net)


def _audio(n, seed, sr, pcm):
    rs = np.random.RandomState(seed)
    t = np.arange(n) / sr
    x = (0.3 * np.sin(2 * np.pi * (180 + 7 * (seed % 40)) * t) + 0.2 * np.sin(2 * np.pi * 1234.5 * t + seed)
         + 0.05 * rs.standard_normal(n)).astype(np.float32)
    return torch.from_numpy((x * 32767).astype(np.int16) if pcm else x)


def _as_float(w):
    return w.float() / 32768.0 if w.dtype == torch.int16 else w


def _max_raw(in_sr):
    return int((HOP * 310 + 100) * in_sr / MODEL_SR)


def _cap_frames(in_sr):
    cap = int(math.ceil(_max_raw(in_sr) * (float(MODEL_SR) / in_sr)))
    return int(_capi.lib().mbv_spectrogram_frames(cap, N_FFT, HOP))


def _raw_len(T, rem, in_sr):
    """Raw samples that give T frames at the model's rate."""
    frames = lambda n: _capi.lib().mbv_spectrogram_frames(int(math.ceil(n * (float(MODEL_SR) / in_sr))), N_FFT, HOP)
    n = int(math.ceil((HOP * T + rem) * in_sr / MODEL_SR))
    while frames(n) > T:                      # (rounding up twice may pass the last sample of frame T)
        n -= 1
    assert frames(n) == T
    return n


def _noise(net, seed, in_sr):
    return torch.randn(1, net.cfg.inter_channels, _cap_frames(in_sr), generator=torch.Generator().manual_seed(seed)).cuda()


def _raw_min(in_sr, x):
    """The fewest raw samples that make x model-rate samples final while the recording is open."""
    r = max(0, x * in_sr // MODEL_SR)
    while wire.resample_ready_open(in_sr, MODEL_SR, r) < x:
        r += 1
    while r > 0 and wire.resample_ready_open(in_sr, MODEL_SR, r - 1) >= x:
        r -= 1
    return r


def _boundaries(net, in_sr, n_raw, T, cf):
    """The raw sample counts at which conversion j = 1, 2, ... becomes due when every earlier one ran at its own
    boundary: cf * j z_hat frames need 96 + cf * j final spectrogram frames, the last of which needs all its samples
    at the model's rate, and those need their taps at the raw rate.  Chunks become decodable with a conversion."""
    r_conv, pad, out, j = net.converter_context()[1], (N_FFT - HOP) // 2, [], 1
    while r_conv + cf * j <= T:
        r = _raw_min(in_sr, (r_conv + cf * j - 1) * HOP - pad + N_FFT)
        if r >= n_raw:
            break
        out.append(r)
        j += 1
    return out


def _cuts(net, pattern, in_sr, n, T, cf, seed):
    if pattern in ("one", "all_then_close"):
        return [n]
    if pattern == "20ms":
        k = in_sr // 50
        return [k] * (n // k) + ([n % k] if n % k else [])
    if pattern == "short_of_boundaries":
        out, prev = [], 0
        for b in _boundaries(net, in_sr, n, T, cf):
            out += [b - 1 - prev, 1]
            prev = b
        return out + [n - prev]
    rs, out, left = np.random.RandomState(seed), [], n
    while left:
        k = min(left, int(rs.randint(1, 40001)))
        out.append(k)
        left -= k
    return out


def _open(net, in_sr, rate, dtype, noise, peak=None, cf=32, sched=(32, 256), **kw):
    return wire.convert_live_pcm16(net, SRC, TGT, in_sr, MODEL_SR, rate, HOP, WIN, _max_raw(in_sr), dtype=dtype,
                                   peak=peak, noise=noise, chunk_frames=sched[0], max_chunk_frames=sched[1],
                                   convert_frames=cf, **kw)


def _drive(net, raw, in_sr, rate, noise, pattern, peak, cf, sched, T, seed=0):
    """-> (the finished LiveWire, [(first_out_sample, length)] of its pieces, pieces handed out before close())."""
    lw = _open(net, in_sr, rate, raw.dtype, noise, peak, cf, sched)
    host = raw.cpu()
    sizes = _cuts(net, pattern, in_sr, raw.numel(), T, cf, seed)
    assert sum(sizes) == raw.numel() and min(sizes) > 0
    pieces, off = [], 0

    def take():
        for a, v in lw.poll():
            assert v.dtype == torch.int16 and (v.numel() == 0 or v.data_ptr() == lw.pcm.data_ptr() + 2 * a)
            pieces.append((a, v.numel()))

    for i, k in enumerate(sizes):
        z0 = lw.live.z_frames
        lw.push((host if i % 2 else raw)[off:off + k])
        off += k
        if pattern == "all_then_close":
            continue
        runs = net.input_runs()
        take()
        assert net.input_runs() - runs <= 1
        if pattern == "short_of_boundaries" and i + 1 < len(sizes):
            # one sample short: nothing converts; the sample that completes the rule: exactly cf frames more
            assert lw.live.z_frames == (z0 if i % 2 == 0 else z0 + cf), (i, k, z0, lw.live.z_frames)
    early = len(pieces)
    assert not lw.finished and int(lw.valid_samples[0]) == 0
    lw.close()
    take()                                # one poll flushes the input, converts and decodes the rest and wires it
    assert lw.finished and lw.poll() == [] and lw.live.finished
    return lw, pieces, early


def _whole_resampled(net, raw, in_sr):
    out, n = net.resample(_as_float(raw)[None, None], in_sr, MODEL_SR)
    return out[0, 0], int(n[0])


def _check_tiles(pieces, valid):
    assert pieces[0][0] == 0 and sum(n for _, n in pieces) == valid
    assert all(a + n == b for (a, n), (b, _) in zip(pieces, pieces[1:]))


# ------------------------------------------------------------------------------------------------ the kernel alone
def _range(buf, in_avail, in_total, first, count, out, cap=None):
    r = _capi.MbvResampleRange()
    r.wave, r.wave_dtype = buf.data_ptr(), 1 if buf.dtype == torch.int16 else 0
    r.in_avail, r.in_total, r.out_first, r.out_count = in_avail, in_total, first, count
    r.out, r.out_capacity = out.data_ptr(), out.numel() if cap is None else cap
    return r


CANARY = 7.5e8


def _unarrived(n, pcm):
    """A raw buffer before anything arrived: what must never be read (a NaN meets no weight unharmed)."""
    return torch.full((n,), -32768, dtype=torch.int16).cuda() if pcm else torch.full((n,), float("nan")).cuda()


@pytest.mark.parametrize("pcm", [False, True])
@pytest.mark.parametrize("in_sr", [48000, 16000])
def test_ranges_are_bitwise_the_one_shot_resample_and_touch_nothing_else(in_sr, pcm):
    net = _net()
    n = 3000
    whole = _audio(n, 11 + pcm, in_sr, pcm).cuda()
    want, total = _whole_resampled(net, whole, in_sr)
    assert total == want.numel() == int(math.ceil(n * (float(MODEL_SR) / in_sr)))
    out = torch.full((total + 300,), CANARY).cuda()
    buf = _unarrived(n + 64, pcm)
    pos, starts = 0, []
    for c in [0, 1, 255, 256, 257, 0, 256, 1, 257, 255, 256, 257, 256, 257, 255, 256]:
        need = _raw_min(in_sr, pos + c)                    # the tightest frontier: the range ends where readiness ends
        if need >= n:
            break
        buf[:need] = whole[:need]
        runs = net.input_runs()
        net.resample_ranges([_range(buf, need, -1, pos, c, out)], in_sr, MODEL_SR)
        assert net.input_runs() - runs == (1 if c else 0)
        if c:
            starts.append(pos % 256)
        pos += c
        assert torch.equal(out[:pos], want[:pos]), (pos, c)
        assert bool((out[pos:] == CANARY).all()), (pos, c)
    assert pos >= 1025 and 0 in starts and any(starts)     # ranges that start at a tile boundary and inside a tile
    buf[:n] = whole
    runs = net.input_runs()
    net.resample_ranges([_range(buf, n, n, pos, total - pos, out)], in_sr, MODEL_SR)      # close: the flush
    assert net.input_runs() - runs == 1 and total > pos
    assert torch.equal(out[:total], want) and bool((out[total:] == CANARY).all())


def test_rows_at_different_stages_share_one_launch():
    net = _net()
    in_sr, n = 48000, 3000
    raws = [_audio(n, 21, in_sr, True).cuda(), _audio(n, 22, in_sr, False).cuda(), _audio(n, 23, in_sr, True).cuda()]
    wants = [_whole_resampled(net, w, in_sr) for w in raws]
    total = wants[0][1]
    # an open row from its start, an open row inside, a closed row's flush
    avail = [_raw_min(in_sr, 300), _raw_min(in_sr, 300 + 257), n]
    spans = [(0, 300), (300, 257), (900, total - 900)]
    bufs = []
    for w, a in zip(raws, avail):
        b = _unarrived(n, w.dtype == torch.int16)
        b[:a] = w[:a]
        bufs.append(b)

    def rows(outs):
        return [_range(b, a, n if a == n else -1, f, c, o) for b, a, (f, c), o in zip(bufs, avail, spans, outs)]

    alone = [torch.full((total + 50,), CANARY).cuda() for _ in raws]
    for r in rows(alone):
        net.resample_ranges([r], in_sr, MODEL_SR)
    both = [torch.full((total + 50,), CANARY).cuda() for _ in raws]
    runs = net.input_runs()
    net.resample_ranges(rows(both), in_sr, MODEL_SR)
    assert net.input_runs() - runs == 1
    for a, b, (want, _), (f, c) in zip(alone, both, wants, spans):
        assert torch.equal(a, b) and torch.equal(b[f:f + c], want[f:f + c])
        assert bool((b[:f] == CANARY).all()) and bool((b[f + c:] == CANARY).all())
    # nothing to do: no launch, nothing counted
    runs = net.input_runs()
    net.resample_ranges([], in_sr, MODEL_SR)
    net.resample_ranges([_range(bufs[0], avail[0], -1, 10, 0, both[0]), _range(bufs[2], n, n, total, 0, both[2])], in_sr, MODEL_SR)
    assert net.input_runs() == runs


def test_a_table_longer_than_one_upload_launch():
    """33 rows, int16 and fp32, open and closed: the table goes up in two launches, and an offset wrong in the second
    one shows in table row 32.  Every row bitwise its own call and the one-shot resample, one input run."""
    net = _net()
    in_sr, n = 48000, 1500
    raws = [_audio(n, 40 + k, in_sr, k % 2 == 0).cuda() for k in range(33)]
    wants = [_whole_resampled(net, w, in_sr) for w in raws]
    total = wants[0][1]
    spans, avail = [], []
    for k in range(33):
        if k % 3 == 2:                                      # a closed row's flush
            spans.append((200 + k, total - 200 - k))
            avail.append(n)
        else:                                               # an open row, from its start or inside
            f = 0 if k % 3 == 0 else 100 + k
            spans.append((f, 150 + 7 * k))
            avail.append(_raw_min(in_sr, f + 150 + 7 * k))
    assert max(avail[k] for k in range(33) if k % 3 != 2) < n
    bufs = []
    for w, a in zip(raws, avail):
        b = _unarrived(n, w.dtype == torch.int16)
        b[:a] = w[:a]
        bufs.append(b)

    def rows(outs):
        return [_range(b, a, n if a == n else -1, f, c, o) for b, a, (f, c), o in zip(bufs, avail, spans, outs)]

    alone = [torch.full((total + 50,), CANARY).cuda() for _ in raws]
    for r in rows(alone):
        net.resample_ranges([r], in_sr, MODEL_SR)
    both = [torch.full((total + 50,), CANARY).cuda() for _ in raws]
    runs = net.input_runs()
    net.resample_ranges(rows(both), in_sr, MODEL_SR)
    assert net.input_runs() - runs == 1
    for a, b, (want, _), (f, c) in zip(alone, both, wants, spans):
        assert torch.equal(a, b) and torch.equal(b[f:f + c], want[f:f + c])
        assert bool((b[:f] == CANARY).all()) and bool((b[f + c:] == CANARY).all())


# ------------------------------------------------------------------------------------------------ contract clause 3
LONG = [(T, pcm, chain) for T in (257, 300) for pcm in (True, False) for chain in CHAINS]


@pytest.mark.parametrize("r", range(len(LONG)))
def test_long_recordings_are_bitwise_the_one_shot_chain(r):
    """Contract clauses 1 - 3: every push pattern with `peak=None` and `peak=0.5`; convert_frames and the schedule
    rotate with the pattern."""
    net = _net()
    T, pcm, (in_sr, rate) = LONG[r]
    raw = _audio(_raw_len(T, (0, 1, 254)[r % 3], in_sr), 10 + r, in_sr, pcm).cuda()
    noise = _noise(net, 100 + r, in_sr)
    samples, total = _whole_resampled(net, raw, in_sr)
    refs = {}
    for peak in (None, 0.5):
        ref = net.convert_stream(raw, SRC, TGT, MODEL_SR, HOP, WIN, in_sr=in_sr, noise=noise[:, :, :T])
        f = wire.stream_pcm16(net, ref, MODEL_SR, rate, peak=peak)
        pcm_ref, valid_ref = f.run()
        refs[peak] = (ref, pcm_ref, valid_ref, f.peak)
    ref = refs[None][0]
    assert ref.z.shape[2] == T
    svc, svc_valid = wire.service_pcm16(net, ref.o, ref.y_lengths, MODEL_SR, rate, auto_normalize=False)
    valid = int(svc_valid[0])
    tiles = {}
    for p, pattern in enumerate(PATTERNS):
        for peak in (None, 0.5):
            cf = 32 if pattern == "short_of_boundaries" else (1, 32)[(r + p) % 2]
            sched = SCHEDULES[p % 2]
            what = (T, pcm, in_sr, rate, pattern, peak, cf, sched)
            lw, pieces, early = _drive(net, raw, in_sr, rate, noise, pattern, peak, cf, sched, T, seed=r)
            live = lw.live
            # clause 2: the model-rate samples are the one-shot resample, zeros behind
            assert live.arrived == total and torch.equal(live.samples[:total], samples), what
            assert int(torch.count_nonzero(live.samples[total:])) == 0
            # clause 3
            _, pcm_ref, valid_ref, peak_ref = refs[peak]
            assert torch.equal(live.z[:, :, :T], ref.z) and torch.equal(live.result(), ref.o), what
            assert torch.equal(lw.valid_samples, valid_ref) and int(valid_ref[0]) == valid, what
            assert torch.equal(lw.pcm[:, :valid], pcm_ref[:, :valid]), what
            assert int(torch.count_nonzero(lw.pcm[:, valid:])) == 0
            assert torch.equal(lw.peak, peak_ref), what
            if peak is None:
                assert torch.equal(lw.pcm[:, :valid], svc[:, :valid]) and torch.equal(lw.valid_samples, svc_valid), what
            # the pieces: one per chunk of the schedule, tiling [0, valid), the same for every cut
            _check_tiles(pieces, valid)
            assert len(pieces) == len(stream.chunk_schedule(T, *sched)) == len(live.schedule)
            assert tiles.setdefault(sched, pieces) == pieces, what
            if T == 300 and pattern not in ("all_then_close",):
                assert early >= 1, what               # int16 left before the recording ended


# ------------------------------------------------------------------------------------------------ clauses 1 and 4
SHORT = [(1, True, CHAINS[0]), (17, False, CHAINS[1]), (256, True, CHAINS[0])]


@pytest.mark.parametrize("r", range(len(SHORT)))
def test_short_recordings_do_not_depend_on_the_pushes_and_are_within_rounding(r):
    net = _net()
    T, pcm, (in_sr, rate) = SHORT[r]
    raw = _audio(_raw_len(T, (0, 1, 254)[r], in_sr), 40 + r, in_sr, pcm).cuda()
    noise = _noise(net, 140 + r, in_sr)
    samples, total = _whole_resampled(net, raw, in_sr)
    first, tiles = {}, {}
    for p, pattern in enumerate(PATTERNS):
        peak = (None, 0.5)[p % 2]
        cf = 32 if pattern == "short_of_boundaries" else (1, 32)[(r + p) % 2]
        sched = SCHEDULES[(p // 2) % 2]
        what = (T, pattern, peak, cf, sched)
        lw, pieces, _ = _drive(net, raw, in_sr, rate, noise, pattern, peak, cf, sched, T, seed=r)
        live = lw.live
        assert live.arrived == total and torch.equal(live.samples[:total], samples), what
        valid = int(lw.valid_samples[0])
        assert valid == wire.resample_ready(MODEL_SR, rate, SPF * T, SPF * T)
        _check_tiles(pieces, valid)
        assert tiles.setdefault(sched, pieces) == pieces, what
        got = (live.z.clone(), live.result().clone(), lw.peak.clone())
        for a, b in zip(got, first.setdefault("f", got)):
            assert torch.equal(a, b), what
        assert torch.equal(lw.pcm, first.setdefault(peak, lw.pcm.clone())), what
    ref = net.convert_stream(raw, SRC, TGT, MODEL_SR, HOP, WIN, in_sr=in_sr, noise=noise[:, :, :T])
    ref_o = ref.run()
    z, o, _ = first["f"]
    z = z[:, :, :T]
    rel = float(torch.sqrt(torch.mean((z - ref.z).double() ** 2)) / torch.sqrt(torch.mean(ref.z.double() ** 2)))
    err = float(torch.sqrt(torch.mean((o - ref_o).double() ** 2)))
    print("live wire against convert_stream, %d frames: z relative rms %.3e, o rms %.3e" % (T, rel, err))
    assert rel <= 5e-5, (T, rel)
    assert err <= 1e-4, (T, err)


# ------------------------------------------------------------------------------------------------ equal input rate
@pytest.mark.parametrize("pcm", [True, False])
def test_equal_input_rate_pushes_straight_through(pcm):
    net = _net()
    T, rate = 300, 24000
    raw = _audio(HOP * T + 5, 50 + pcm, MODEL_SR, pcm).cuda()
    noise = _noise(net, 150, MODEL_SR)
    runs = net.input_runs()
    lw, pieces, early = _drive(net, raw, MODEL_SR, rate, noise, "20ms", 0.5, 32, (32, 256), T)
    assert net.input_runs() == runs and lw.raw is None and lw.live.dtype == raw.dtype and early >= 1
    st = net.convert_live(SRC, TGT, MODEL_SR, HOP, WIN, _max_raw(MODEL_SR), dtype=raw.dtype, noise=noise)
    st.push(raw)
    st.close()
    st.poll()
    assert st.finished and torch.equal(st.samples, lw.live.samples)
    assert torch.equal(st.z, lw.live.z) and torch.equal(st.result(), lw.live.result())
    ds = net.dec_stream(st.z[:, :, :T].contiguous(), st.g)
    f = wire.stream_pcm16(net, ds, MODEL_SR, rate, peak=0.5)
    pcm_ref, valid_ref = f.run()
    assert torch.equal(ds.o, st.result())
    valid = int(valid_ref[0])
    assert torch.equal(lw.valid_samples, valid_ref) and torch.equal(lw.pcm[:, :valid], pcm_ref[:, :valid])
    assert torch.equal(lw.peak, f.peak)
    _check_tiles(pieces, valid)


# ------------------------------------------------------------------------------------------------ the pool
def _text_batch(net, B, T, seed):
    x, xl, sid = synth.synthetic_batch(net.cfg, B, T, seed=seed, ragged=True)
    return torch.from_numpy(x).cuda(), torch.from_numpy(xl).cuda(), torch.from_numpy(sid).cuda()


def test_a_pcm_pool_serves_live_wires_next_to_finished_streams():
    """Three live wires at different stages, one text stream and one admitted recording in a PcmPool: at most one input
    launch and one wire launch per step, decoder runs as the StreamPool alone makes them, every member's bytes those of
    its stand-alone run, on the device and through the pinned host buffer; other calls use the scratch in between."""
    net = _net()
    in_sr, rate = 48000, 24000
    frames, scheds = [300, 257, 100], [(8, 32), (32, 256), (8, 32)]
    raws = [_audio(_raw_len(T, (0, 1, 254)[k], in_sr), 60 + k, in_sr, pcm=k != 1).cuda() for k, T in enumerate(frames)]
    noises = [_noise(net, 160 + k, in_sr) for k in range(3)]
    peaks = [None, 0.5, 0.25]
    solo = []
    for w, nz, s, pk, T in zip(raws, noises, scheds, peaks, frames):
        lw, pieces, _ = _drive(net, w, in_sr, rate, nz, "random", pk, 32, s, T, seed=3)
        solo.append((lw.pcm.clone(), lw.valid_samples.clone(), lw.peak.clone(), pieces))
    x, xl, sid = _text_batch(net, 1, 20, 4)
    torch.manual_seed(5)
    torch.cuda.manual_seed(5)
    text = net.infer_stream(x, xl, sid, noise_scale=0.5, chunk_frames=8, max_chunk_frames=32)
    pool = net.stream_pool()
    pp = wire.pcm_pool(net, pool, MODEL_SR, rate)
    req = ConvertRequest(_audio(HOP * 270, 70, MODEL_SR, False), 1, 2, MODEL_SR, HOP, WIN, chunk_frames=16, max_chunk_frames=64)
    fa = pp.admit([req])[0]
    ft = pp.add(text, peak=0.5)
    other_want = []
    for f, pk in ((fa, None), (ft, 0.5)):
        alone = wire.stream_pcm16(net, net.dec_stream(f._st.z.clone(), f._st.g), MODEL_SR, rate, peak=pk)
        other_want.append(tuple(t.clone() for t in alone.run()))
    lws = [_open(net, in_sr, rate, w.dtype, nz, pk, 32, s) for w, nz, s, pk in zip(raws, noises, scheds, peaks)]
    # stages: the first has all its audio (open), the second half of it, the third none yet
    lws[0].push(raws[0])
    lws[1].push(raws[1][:raws[1].numel() // 2])
    fed = [raws[0].numel(), raws[1].numel() // 2, 0]
    for lw in lws:
        assert pp.add_live(lw) is lw
    assert len(pp) == 5 and len(pool) == 5
    # the refusals of the parent commit still stand
    with pytest.raises(TypeError, match="LiveStream"):
        wire.stream_pcm16(net, lws[0].live, MODEL_SR, rate)
    with pytest.raises(TypeError, match="total length"):
        pp.add(lws[2].live)
    with pytest.raises(ValueError, match="model's rate"):
        net.convert_live(SRC, TGT, MODEL_SR, HOP, WIN, 10000, in_sr=48000)
    bx, bxl, bsid = _text_batch(net, 3, 25, 3)
    ref_infer = net.infer(bx, bxl, bsid, noise_scale=0)[0].clone()
    decoded = []
    pool_step = pool.step
    pool.step = lambda streams=None: decoded.append(pool_step(streams)) or decoded[-1]
    got = {id(m): [] for m in lws}
    input_steps = 0
    for step in range(60):
        for k, lw in enumerate(lws):
            if not lw.closed:
                n = min(45 * in_sr // 86 + 13, raws[k].numel() - fed[k])
                if n:
                    lw.push(raws[k][fed[k]:fed[k] + n])
                    fed[k] += n
                elif step >= 2 + k:
                    lw.close()
        due = [lw._plan.feed_due() for lw in pp.lives]
        c0 = _counters(net)
        host = step % 2 == 1
        out = pp.step(host=host)
        c1 = _counters(net)
        assert c1[0] - c0[0] == (1 if any(d and d[1] for d in due) else 0), step
        input_steps += c1[0] - c0[0]
        assert int(any(len(v) for _, _, v in out)) <= c1[3] - c0[3] <= 1, step
        dec = decoded.pop()
        assert not decoded
        if dec:
            routes = [max(st.z_frames, 257) if isinstance(st, stream.LiveStream) else st.z.shape[2] for st, _, _ in dec]
            assert c1[2] - c0[2] == net.chunks_plan(routes)[0], (step, routes)
        else:
            assert c1[2] == c0[2]
        for m, a, v in out:
            if id(m) in got:
                assert isinstance(v, np.ndarray) == host
                got[id(m)].append((a, torch.from_numpy(v.copy()) if host else v.cpu()))
        # the same scratch serves other calls between the steps
        assert torch.equal(net.infer(bx, bxl, bsid, noise_scale=0)[0], ref_infer)
        if step % 3 == 0:
            loud = net.infer(bx, bxl, bsid, noise_scale=3.0, length_scale=1.5)[0]
            assert bool(torch.isfinite(loud).all())
        if not len(pp):
            break
    pool.step = pool_step
    assert len(pp) == 0 and len(pool) == 0 and input_steps >= 3
    for lw, (pcm, valid, peak, pieces) in zip(lws, solo):
        assert torch.equal(lw.pcm, pcm) and torch.equal(lw.valid_samples, valid) and torch.equal(lw.peak, peak)
        mine = got[id(lw)]
        assert [(a, v.numel()) for a, v in mine] == pieces
        host_pcm = pcm[0].cpu()
        for a, v in mine:
            assert torch.equal(v, host_pcm[a:a + v.numel()]), a
        c0 = _counters(net)
        assert not lw.finished
        handed = lw.poll()                                 # wired ahead by the pool: handed out without a launch
        assert [(a, v.numel()) for a, v in handed] == pieces and lw.finished and _counters(net) == c0
    for f, (pcm, valid) in zip((fa, ft), other_want):
        assert torch.equal(f.pcm, pcm) and torch.equal(f.valid_samples, valid)


def test_poll_and_pool_in_turn_give_the_same_bytes():
    net = _net()
    in_sr, rate, T = 16000, 22050, 257
    raw = _audio(_raw_len(T, 3, in_sr), 75, in_sr, True).cuda()
    noise = _noise(net, 175, in_sr)
    want, pieces, _ = _drive(net, raw, in_sr, rate, noise, "one", None, 32, (8, 32), T)
    lw = _open(net, in_sr, rate, raw.dtype, noise, None, 32, (8, 32))
    pp = wire.pcm_pool(net, net.stream_pool(), MODEL_SR, rate)
    pp.add_live(lw)
    got, k = [], in_sr // 4
    for i, off in enumerate(range(0, raw.numel(), k)):
        lw.push(raw[off:off + k])
        if i % 2:
            got += [(a, v.numel()) for a, v in lw.poll()]
        else:
            pp.step()
    lw.close()
    for _ in range(40):
        if lw._plan.wire_done:
            break
        pp.step()
    got += [(a, v.numel()) for a, v in lw.poll()]
    assert lw.finished and got == pieces
    assert torch.equal(lw.pcm, want.pcm) and torch.equal(lw.valid_samples, want.valid_samples)
    assert torch.equal(lw.peak, want.peak) and torch.equal(lw.live.z, want.live.z)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_launch_nothing_and_the_wire_serves_on():
    net = _net()
    in_sr, rate, T = 48000, 24000, 300
    raw = _audio(_raw_len(T, 9, in_sr), 90, in_sr, True).cuda()
    noise = _noise(net, 190, in_sr)
    want, pieces, _ = _drive(net, raw, in_sr, rate, noise, "one", None, 32, (32, 256), T)
    lw = _open(net, in_sr, rate, raw.dtype, noise)
    half = raw.numel() // 2
    lw.push(raw[:half])
    got = [(a, v.numel()) for a, v in lw.poll()]
    c0 = _counters(net)
    with pytest.raises(TypeError, match="int16"):
        lw.push(raw[:10].float())
    with pytest.raises(ValueError, match="capacity"):
        lw.push(torch.zeros(_max_raw(in_sr), dtype=torch.int16))
    with pytest.raises(ValueError, match="1-D"):
        lw.push(raw[:10][None])
    assert lw.arrived == half
    with pytest.raises(TypeError, match="dtype"):
        _open(net, in_sr, rate, torch.float64, noise)
    with pytest.raises(ValueError, match="res_type"):
        _open(net, in_sr, rate, raw.dtype, noise, res_type="soxr_hq")
    net.set_option("conv_bf16", 3)
    try:
        with pytest.raises(ValueError, match="conv_bf16"):
            _open(net, in_sr, rate, raw.dtype, noise)
    finally:
        net.set_option("conv_bf16", 0)
    # another rate pair, filter or kind of object than the pool's
    pp = wire.pcm_pool(net, net.stream_pool(), MODEL_SR, rate)
    with pytest.raises(ValueError, match="Hz"):
        pp.add_live(_open(net, in_sr, 16000, raw.dtype, noise))
    with pytest.raises(ValueError, match="kaiser_fast"):
        pp.add_live(_open(net, in_sr, rate, raw.dtype, noise, res_type="kaiser_fast"))
    with pytest.raises(TypeError, match="LiveWire"):
        pp.add_live(lw.live)
    assert len(pp) == 0
    # the C entry, each refusal naming the row
    h, L = net._ensure_handle(), _capi.lib()
    out = torch.zeros(1000).cuda()
    ready = wire.resample_ready_open(in_sr, MODEL_SR, 2000)
    ok = lambda: _range(raw, 2000, -1, 0, 10, out)

    def refused(rows, what, orig=in_sr, filt=0, n=None):
        arr = (_capi.MbvResampleRange * len(rows))(*rows)
        assert L.mbv_resample_ranges(h, arr, len(rows) if n is None else n, orig, MODEL_SR, filt, None) != 0, what
        assert what in L.mbv_last_error(h), (what, L.mbv_last_error(h))

    bad = ok()
    bad.out_first, bad.out_count = ready - 4, 5
    refused([ok(), bad], b"row 1: outputs up to %d asked for" % (ready + 1))
    bad = ok()
    bad.in_total, bad.in_avail, bad.out_first, bad.out_count = 2000, 2000, 0, 920         # closed: ceil(2000 ratio) = 919
    refused([bad], b"row 0: outputs up to 920 asked for")
    bad = ok()
    bad.out_first, bad.out_count = 995, 6
    refused([ok(), ok(), bad], b"row 2: outputs [995, 1001) lie outside")
    for field in ("in_avail", "out_first", "out_count", "out_capacity"):
        bad = ok()
        setattr(bad, field, -1)
        refused([bad], b"row 0: in_avail, out_first")
    bad = ok()
    bad.in_total = -2
    refused([bad], b"row 0: in_avail, out_first")
    bad = ok()
    bad.in_total = 2001
    refused([bad], b"row 0: a closed recording has all its samples")
    for field in ("wave", "out"):
        bad = ok()
        setattr(bad, field, None)
        refused([ok(), bad], b"row 1: wave / out missing")
    bad = ok()
    bad.wave_dtype = 2
    refused([bad], b"row 0: unknown wave_dtype")
    refused([ok()], b"unknown filter", filt=2)
    refused([ok()], b"equal rates", orig=MODEL_SR)
    refused([ok()], b"4096", orig=22051)
    refused([ok()], b"positive", orig=0)
    refused([ok()], b"bad arguments", n=-1)
    bad = ok()
    bad.out_first = 9                                     # [9, 19) meets row 0's [0, 10) in the same buffer
    refused([ok(), bad], b"rows 0 and 1 write overlapping ranges")
    assert int(torch.count_nonzero(out)) == 0 and _counters(net) == c0
    # the handle and the wire serve on
    lw.push(raw[half:])
    got += [(a, v.numel()) for a, v in lw.poll()]
    lw.close()
    c1 = _counters(net)
    with pytest.raises(ValueError, match="after close"):
        lw.push(raw[:1])
    assert _counters(net) == c1 and lw.arrived == raw.numel()
    # a pooled wire refuses the same way, and the pool serves on
    other = _open(net, in_sr, rate, raw.dtype, noise)
    pp.add_live(other)
    other.push(raw[:half])
    pp.step()
    other.close()
    c1 = _counters(net)
    with pytest.raises(ValueError, match="after close"):
        other.push(raw[:1])
    with pytest.raises(ValueError, match="Hz"):
        pp.add_live(_open(net, in_sr, 16000, raw.dtype, noise))
    assert _counters(net) == c1 and len(pp) == 1
    for _ in range(40):
        if not len(pp):
            break
        pp.step()
    assert len(pp) == 0 and other.poll() != [] and other.finished
    got += [(a, v.numel()) for a, v in lw.poll()]
    assert lw.finished and got == pieces
    assert torch.equal(lw.pcm, want.pcm) and torch.equal(lw.valid_samples, want.valid_samples)
    # a recording that gives no frame cannot be closed
    empty = _open(net, in_sr, rate, raw.dtype, noise)
    with pytest.raises(ValueError, match="no spectrogram frame"):
        empty.close()
    empty.push(raw[:400])
    with pytest.raises(ValueError, match="no spectrogram frame"):
        empty.close()
    assert not empty.closed
    empty.push(raw[400:600])
    empty.close()
    assert len(empty.poll()) == 1 and empty.finished and int(empty.valid_samples[0]) == wire.resample_ready(MODEL_SR, rate, 256, 256)


def test_splitk_mode_is_deterministic_and_within_rounding():
    net = _net()
    in_sr, rate, T = 48000, 24000, 300
    raw = _audio(_raw_len(T, 1, in_sr), 95, in_sr, True).cuda()
    noise = _noise(net, 195, in_sr)
    default = _drive(net, raw, in_sr, rate, noise, "random", None, 32, (8, 32), T)[0]
    net.set_option("splitk", 1)
    try:
        a, b = [_drive(net, raw, in_sr, rate, noise, "random", None, 32, (8, 32), T)[0] for _ in range(2)]
    finally:
        net.set_option("splitk", 0)
    assert torch.equal(a.live.z, b.live.z) and torch.equal(a.pcm, b.pcm) and torch.equal(a.valid_samples, b.valid_samples)
    assert torch.equal(a.live.samples, default.live.samples)          # the resampler has one mode
    zd = default.live.z[:, :, :T].double()
    rel = float(torch.sqrt(torch.mean((a.live.z[:, :, :T] - zd) ** 2)) / torch.sqrt(torch.mean(zd ** 2)))
    print("splitk, %d frames: z relative rms against the default mode %.3e" % (T, rel))
    assert rel <= 5e-5, rel
