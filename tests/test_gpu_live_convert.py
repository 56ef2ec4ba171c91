"""Live voice conversion on the MI355X: a recording pushed piece by piece through `net.convert_live` is converted and
decoded while it arrives; the result does not depend on how it was cut into pushes, and for a recording of more than
256 frames it is bitwise `net.convert_stream(whole, noise=...)` chunk by chunk."""
import ctypes as C

import numpy as np
import pytest
import torch

from mb_istft_vits_amd import _capi, stream, synth, wire
from mb_istft_vits_amd.models import ConvertRequest

from gpu_util import make_net

pytestmark = pytest.mark.gpu

MODEL_SR, HOP, WIN, N_FFT = 16000, 256, 1024, 1024
CAP = HOP * 310 + 100                    # max_samples of every stream here: 310 frames, so the block's stride is not T
CAP_F = 310
SRC, TGT = 3, 7
SCHEDULES = [(8, 32), (32, 256)]
PATTERNS = ["one", "320_poll_each", "1000", "random", "one_then_rest"]
_NETS = {}


def _net(name="uudb_ms_istft_vits_ms"):
    if name not in _NETS:
        _NETS[name] = make_net(name)
    return _NETS[name][0]


def _seed(s):
    torch.manual_seed(s)
    torch.cuda.manual_seed(s)


def _audio(n, seed, pcm=False):
    rs = np.random.RandomState(seed)
    t = np.arange(n) / MODEL_SR
    x = (0.3 * np.sin(2 * np.pi * (180 + 7 * (seed % 40)) * t) + 0.2 * np.sin(2 * np.pi * 1234.5 * t + seed)
         + 0.05 * rs.standard_normal(n)).astype(np.float32)
    return torch.from_numpy((x * 32767).astype(np.int16) if pcm else x)


def _noise(net, seed):
    return torch.randn(1, net.cfg.inter_channels, CAP_F, generator=torch.Generator().manual_seed(seed)).cuda()


def _cuts(pattern, n, seed):
    """(push sizes, poll after every k-th push)."""
    if pattern == "one":
        return [n], 1
    if pattern == "320_poll_each":
        return [320] * (n // 320) + ([n % 320] if n % 320 else []), 1
    if pattern == "1000":
        return [1000] * (n // 1000) + ([n % 1000] if n % 1000 else []), 3
    if pattern == "one_then_rest":
        return ([1, n - 1] if n > 1 else [1]), 1
    rs, out, left = np.random.RandomState(seed), [], n
    while left:
        k = min(left, int(rs.randint(1, 20001)))
        out.append(k)
        left -= k
    return out, 1


def _open(net, wave, noise, cf=32, sched=(32, 256), **kw):
    return net.convert_live(kw.pop("sid_src", SRC), kw.pop("sid_tgt", TGT), MODEL_SR, HOP, WIN, CAP, dtype=wave.dtype,
                            noise=noise, chunk_frames=sched[0], max_chunk_frames=sched[1], convert_frames=cf, **kw)


def _drive(net, wave, noise, pattern, cf, sched, seed=0):
    """Push `wave` (device) in the pattern's pieces, from host and device tensors in turn; -> (stream, chunks, chunks
    handed out before close())."""
    st = _open(net, wave, noise, cf, sched)
    host = wave.cpu()
    sizes, every = _cuts(pattern, wave.numel(), seed)
    got, off = [], 0

    def take():
        for a, v in st.poll():
            got.append((a, v.clone()))

    for i, k in enumerate(sizes):
        st.push((host if i % 2 else wave)[off:off + k])
        off += k
        if (i + 1) % every == 0:
            take()
    take()
    early = len(got)
    assert not st.finished and st.y_lengths is None
    st.close()
    take()                                # one poll converts the rest and decodes every remaining chunk
    assert st.finished and st.poll() == []
    return st, got, early


def _one_shot(net, wave, noise, F, sched):
    ref = net.convert_stream(wave, SRC, TGT, MODEL_SR, HOP, WIN, noise=noise[:, :, :F], chunk_frames=sched[0],
                             max_chunk_frames=sched[1])
    chunks = [(a, v.clone()) for a, v in ref]
    return ref, chunks


LONG = [(F, rem, pcm) for F in (257, 300) for rem in (0, 1, 255) for pcm in (False, True)]


@pytest.mark.parametrize("r", range(len(LONG)))
def test_long_recordings_are_bitwise_the_one_shot_path(r):
    """Contract clauses 2 and 3.  Every push pattern runs on every recording; convert_frames (1, 32) and the schedule
    rotate with (recording, pattern), so each pattern meets all four combinations three times over the twelve
    recordings."""
    net = _net()
    F, rem, pcm = LONG[r]
    wave = _audio(HOP * F + rem, 10 + r, pcm).cuda()
    noise = _noise(net, 100 + r)
    refs = {s: _one_shot(net, wave, noise, F, s) for s in SCHEDULES}
    assert refs[SCHEDULES[0]][0].z.shape[2] == F
    state = torch.cuda.get_rng_state().clone()
    for p, pattern in enumerate(PATTERNS):
        q = (r + p) % 4
        cf, sched = (1, 32)[q % 2], SCHEDULES[q // 2]
        ref, want = refs[sched]
        st, got, early = _drive(net, wave, noise, pattern, cf, sched, seed=r)
        what = (F, rem, pcm, pattern, cf, sched)
        assert [(a, v.shape[-1]) for a, v in got] == [(a, v.shape[-1]) for a, v in want], what
        assert [(a // 256, v.shape[-1] // 256) for a, v in got] == stream.chunk_schedule(F, *sched) == st.schedule
        for (a, v), (_, w) in zip(got, want):
            assert torch.equal(v, w), what + (a,)
        assert torch.equal(st.z[:, :, :F], ref.z), what
        assert torch.equal(st.result(), ref.o) and st.result().shape == (1, 1, 256 * F), what
        assert torch.equal(st.g, ref.g) and st.y_lengths.tolist() == [F] and st.y_lengths.dtype == torch.int64
        if F == 300:
            assert early >= 1, what               # audio left before the recording ended
    assert torch.equal(torch.cuda.get_rng_state(), state)          # noise= given: the generator is untouched


SHORT = [(1, 0, False), (17, 1, True), (100, 255, False), (256, 0, True)]


@pytest.mark.parametrize("r", range(len(SHORT)))
def test_short_recordings_do_not_depend_on_the_pushes_and_are_within_rounding(r):
    """Contract clauses 1 and 4: T <= 256 plans with the long route, so the live result is bitwise the same for every
    push pattern and within rounding of `convert_stream`, which takes the narrow kernel there."""
    net = _net()
    F, rem, pcm = SHORT[r]
    wave = _audio(HOP * F + rem, 40 + r, pcm).cuda()
    noise = _noise(net, 140 + r)
    first, chunks_of = None, {}
    for p, pattern in enumerate(PATTERNS):
        q = (r + p) % 4
        cf, sched = (1, 32)[q % 2], SCHEDULES[q // 2]
        st, got, _ = _drive(net, wave, noise, pattern, cf, sched, seed=r)
        assert [(a // 256, v.shape[-1] // 256) for a, v in got] == stream.chunk_schedule(F, *sched)
        z, o = st.z[:, :, :F].clone(), st.result().clone()
        assert torch.equal(torch.cat([v for _, v in got], dim=-1), o)
        if first is None:
            first = (z, o)
        assert torch.equal(z, first[0]) and torch.equal(o, first[1]), (F, pattern, cf, sched)
        if sched in chunks_of:
            assert all(torch.equal(v, w) for (_, v), (_, w) in zip(got, chunks_of[sched]))
        chunks_of[sched] = got
    ref, _ = _one_shot(net, wave, noise, F, SCHEDULES[1])
    z, o = first
    rel = float(torch.sqrt(torch.mean((z - ref.z).double() ** 2)) / torch.sqrt(torch.mean(ref.z.double() ** 2)))
    err = float(torch.sqrt(torch.mean((o - ref.o).double() ** 2)))
    print("live against convert_stream, %d frames: z relative rms %.3e, o rms %.3e (o rms level %.3e)"
          % (F, rel, err, float(torch.sqrt(torch.mean(ref.o.double() ** 2)))))
    assert rel <= 5e-5, (F, rel)
    assert err <= 1e-4, (F, err)


def test_the_stream_draws_once_when_it_is_opened():
    net = _net()
    I = net.cfg.inter_channels
    wave = _audio(HOP * 300 + 7, 3).cuda()
    _seed(77)
    want_noise = torch.randn(1, I, CAP_F, device="cuda", dtype=torch.float32)
    state = torch.cuda.get_rng_state().clone()
    cpu_state = torch.get_rng_state().clone()
    _seed(77)
    st = _open(net, wave, None, 32, (32, 256))
    assert torch.equal(torch.cuda.get_rng_state(), state) and torch.equal(st.noise, want_noise)
    for off in range(0, wave.numel(), 5000):
        st.push(wave[off:off + 5000])
        st.poll()
    st.close()
    st.poll()
    assert st.finished
    assert torch.equal(torch.cuda.get_rng_state(), state) and torch.equal(torch.get_rng_state(), cpu_state)
    ref, _ = _one_shot(net, wave, want_noise, 300, (32, 256))
    assert torch.equal(st.z[:, :, :300], ref.z) and torch.equal(st.result(), ref.run())


@pytest.mark.parametrize("F", [17, 300])
def test_convert_stream_takes_the_noise_it_would_have_drawn(F):
    net = _net()
    wave = _audio(HOP * F + 1, 5, pcm=F == 17)
    _seed(200 + F)
    a = net.convert_stream(wave, SRC, TGT, MODEL_SR, HOP, WIN, chunk_frames=8, max_chunk_frames=32)
    after = torch.cuda.get_rng_state().clone()
    _seed(200 + F)
    noise = torch.randn(1, net.cfg.inter_channels, F, device="cuda", dtype=torch.float32)
    assert torch.equal(torch.cuda.get_rng_state(), after)
    _seed(9)
    state = torch.cuda.get_rng_state().clone()
    runs = net.converter_runs()
    b = net.convert_stream(wave, SRC, TGT, MODEL_SR, HOP, WIN, chunk_frames=8, max_chunk_frames=32, noise=noise)
    assert net.converter_runs() - runs == 1
    assert torch.equal(torch.cuda.get_rng_state(), state), "noise= leaves the generator untouched"
    assert torch.equal(a.z, b.z) and torch.equal(a.g, b.g) and a.schedule == b.schedule
    assert torch.equal(a.y_lengths, b.y_lengths) and torch.equal(a.run(), b.run())
    # a slice of a wider block is taken by value
    block = torch.zeros(1, net.cfg.inter_channels, F + 9, device="cuda")
    block[:, :, :F] = noise
    c = net.convert_stream(wave, SRC, TGT, MODEL_SR, HOP, WIN, chunk_frames=8, max_chunk_frames=32, noise=block[:, :, :F])
    assert torch.equal(c.z, a.z)
    with pytest.raises(ValueError, match="noise must be a float32 tensor"):
        net.convert_stream(wave, SRC, TGT, MODEL_SR, HOP, WIN, noise=block)


def _loud(net):
    reqs = [ConvertRequest(torch.full((HOP * 320,), 0.99) * torch.sign(torch.randn(HOP * 320, generator=torch.Generator().manual_seed(k))),
                           k, k + 1, MODEL_SR, HOP, WIN) for k in range(4)]
    for st in net.convert_streams(reqs):
        assert bool(torch.isfinite(st.z).all())


def _text_batch(net, B, T, seed):
    x, xl, sid = synth.synthetic_batch(net.cfg, B, T, seed=seed, ragged=True)
    return torch.from_numpy(x).cuda(), torch.from_numpy(xl).cuda(), torch.from_numpy(sid).cuda()


def test_a_pool_serves_live_streams_next_to_finished_ones():
    """Three live streams at different stages, one text stream and two admitted recordings in one StreamPool: every
    chunk bitwise what its stream gives alone, one posterior run per step whenever a live member converts, decoder runs
    as `mbv_chunks_plan` names them; other calls use the same scratch between the steps."""
    net = _net()
    frames = [300, 257, 100]
    waves = [_audio(HOP * F + (0, 1, 255)[k], 60 + k, pcm=k == 1).cuda() for k, F in enumerate(frames)]
    noises = [_noise(net, 160 + k) for k in range(3)]
    scheds = [(8, 32), (32, 256), (8, 32)]
    # alone: one push, polled (the result does not depend on the pattern)
    solo = []
    for w, nz, s in zip(waves, noises, scheds):
        st, got, _ = _drive(net, w, nz, "1000", 32, s)
        solo.append((dict((a, v) for a, v in got), st.z.clone(), st.result().clone()))
    # the finished kinds, and what they give alone
    x, xl, sid = _text_batch(net, 1, 20, 4)
    _seed(5)
    text = net.infer_stream(x, xl, sid, noise_scale=0.5, chunk_frames=8, max_chunk_frames=32)
    reqs = [ConvertRequest(_audio(HOP * F, 70 + F), 1, 2, MODEL_SR, HOP, WIN, chunk_frames=16, max_chunk_frames=64) for F in (40, 270)]
    pool = net.stream_pool()
    admitted = pool.admit(reqs)
    pool.add(text)
    others = [text] + admitted
    other_want = [net.dec_stream(st.z.clone(), st.g).run().clone() for st in others]
    live = [_open(net, w, nz, 32, s) for w, nz, s in zip(waves, noises, scheds)]
    # stages: the first has all its audio (open), the second half of it, the third none yet
    live[0].push(waves[0])
    live[1].push(waves[1][:HOP * 150])
    fed = [waves[0].numel(), HOP * 150, 0]
    for st in live:
        pool.add(st)
    with pytest.raises(TypeError, match="LiveStream"):
        wire.stream_pcm16(net, live[0], MODEL_SR, 24000)
    with pytest.raises(TypeError, match="total length"):
        wire.PcmPool(net, pool, MODEL_SR, 24000).add(live[2])
    bx, bxl, bsid = _text_batch(net, 3, 25, 3)
    ref_infer = net.infer(bx, bxl, bsid, noise_scale=0)[0].clone()
    spec, lens = net.spectrogram(waves[2][None].float() / (32768.0 if waves[2].dtype == torch.int16 else 1.0), N_FFT, HOP, WIN)
    seen = [set() for _ in live]
    converted_steps = 0
    for step in range(40):
        for k, st in enumerate(live):                  # more audio for the second and third; close when it is all in
            if not st.closed:
                n = min(HOP * 45 + 13, waves[k].numel() - fed[k])
                if n:
                    st.push(waves[k][fed[k]:fed[k] + n])
                    fed[k] += n
                elif step >= 2 + k:
                    st.close()
        due = any(st.pending() is not None for st in pool.streams if isinstance(st, stream.LiveStream))
        c0, d0 = net.converter_runs(), net.decoder_runs()
        out = pool.step()
        assert net.converter_runs() - c0 == (1 if due else 0), step
        converted_steps += int(due)
        if out:
            routes = [max(st.z_frames, 257) if isinstance(st, stream.LiveStream) else st.z.shape[2] for st, _, _ in out]
            assert net.decoder_runs() - d0 == net.chunks_plan(routes)[0], (step, routes)
        else:
            assert net.decoder_runs() == d0
        assert len({id(st) for st, _, _ in out}) == len(out)          # at most one chunk per member
        for st, a, v in out:
            for k, lv in enumerate(live):
                if st is lv:
                    assert torch.equal(v, solo[k][0][a]), (step, k, a)
                    seen[k].add(a)
        # the same scratch serves other calls between the steps
        assert torch.equal(net.infer(bx, bxl, bsid, noise_scale=0)[0], ref_infer)
        net.voice_conversion(spec, lens, torch.tensor([1]).cuda(), torch.tensor([2]).cuda())
        if step % 4 == 0:
            _loud(net)
        if not len(pool):
            break
    assert len(pool) == 0 and converted_steps >= 3
    for k, st in enumerate(live):
        assert seen[k] == set(solo[k][0]), k
        assert st.poll() != [] and st.finished                         # handed out without a launch
        assert torch.equal(st.z, solo[k][1]) and torch.equal(st.result(), solo[k][2])
    for st, want in zip(others, other_want):
        assert torch.equal(st.o, want)


def test_the_window_input_has_exact_zeros_and_the_recordings_frames():
    """Stage "convert_ypad" of a pooled live conversion [B, cin_pad, T]: row b holds spectrogram frames [wa, wb) of its
    recording bitwise, zeros bit for bit in the pad channels and behind its window, whatever the scratch held."""
    net = _net()
    SC = net.cfg.spec_channels
    cpad = -(-SC // 32) * 32
    _loud(net)
    assert int(torch.count_nonzero(net.read_stage("convert_ypad"))) > 0
    waves = [_audio(HOP * 300, 80).cuda(), _audio(HOP * 290 + 1, 81, pcm=True).cuda()]
    # (chunks of 256 frames: none is decodable while these recordings are open, and a decode would clear the stage)
    sts = [_open(net, w, _noise(net, 180 + k), 32, (256, 256)) for k, w in enumerate(waves)]
    pool = net.stream_pool()
    for st, w, n in zip(sts, waves, (260, 240)):
        pool.add(st)
        st.push(w[:HOP * n])
    pool.step()                                         # the first windows start at frame 0
    sts[0].push(waves[0][HOP * 260:])
    sts[1].push(waves[1][HOP * 240:HOP * 275])
    due = [st.pending() for st in sts]
    finals = [stream.spectrogram_ready(st.arrived, False, N_FFT, HOP) for st in sts]
    assert all(d is not None and d[0] > 96 + 32 for d in due)          # windows that start inside the recording
    out = (C.c_int32 * 2)()
    wins = []
    for st, (a, b), fin in zip(sts, due, finals):
        assert _capi.lib().mbv_convert_window(C.byref(st._cfg_struct), a, b - a, fin, C.byref(out)) == 0
        wins.append((int(out[0]), int(out[1])))
    T = max(wb - wa for wa, wb in wins)
    assert len({wb - wa for wa, wb in wins}) == 2       # a short row next to a long one
    runs = net.converter_runs()
    pool.step()
    assert net.converter_runs() - runs == 1
    y = net.read_stage("convert_ypad")
    assert y.numel() == 2 * cpad * T
    y = y.view(2, cpad, T)
    bits = y.view(torch.int32)
    for k, (w, (wa, wb)) in enumerate(zip(waves, wins)):
        n = wb - wa
        assert int(torch.count_nonzero(bits[k, SC:])) == 0 and int(torch.count_nonzero(bits[k, :, n:])) == 0, k
        fw = w.float() / 32768.0 if w.dtype == torch.int16 else w
        spec, _ = net.spectrogram(fw[None], N_FFT, HOP, WIN)
        assert torch.equal(y[k, :SC, :n], spec[0, :, wa:wb]), k        # frames that do not read past `arrived`


def test_refusals_launch_nothing_and_the_stream_serves_on():
    net = _net()
    wave = _audio(HOP * 300, 90).cuda()
    noise = _noise(net, 190)
    want, want_chunks = _one_shot(net, wave, noise, 300, (32, 256))
    st = _open(net, wave, noise, 32, (32, 256))
    pool = net.stream_pool()
    pool.add(st)
    st.push(wave[:HOP * 200])
    got = list(st.poll())
    c0, d0 = net.converter_runs(), net.decoder_runs()
    arrived, zf = st.arrived, st.z_frames
    with pytest.raises(TypeError, match="float32"):
        st.push(wave[:10].to(torch.int16))
    with pytest.raises(ValueError, match="capacity"):
        st.push(torch.zeros(CAP))
    assert st.arrived == arrived
    with pytest.raises(ValueError, match="model's rate"):
        _open(net, wave, noise, in_sr=24000)
    with pytest.raises(IndexError, match="sid_tgt %d" % net.n_speakers):
        _open(net, wave, noise, sid_tgt=net.n_speakers)
    with pytest.raises(AssertionError, match="n_speakers have to be larger than 0."):
        _open(_net("ljs_mini_mb_istft_vits"), wave, None)
    net.set_option("conv_bf16", 3)
    try:
        with pytest.raises(ValueError, match="conv_bf16"):
            _open(net, wave, noise)
        st.push(wave[HOP * 200:HOP * 240])
        with pytest.raises(_capi.MbvError, match="conv_bf16"):
            st.poll()
        with pytest.raises(_capi.MbvError, match="conv_bf16"):
            pool.step()
    finally:
        net.set_option("conv_bf16", 0)
    assert st.z_frames == zf
    # the C entry: a range whose context is not final, and its other checks, each naming the row
    h, L = net._ensure_handle(), _capi.lib()
    z = torch.zeros(1, net.cfg.inter_channels, CAP_F).cuda()
    rows = (_capi.MbvConvertRange * 2)()
    for row in rows:
        row.wave, row.arrived, row.closed, row.wave_dtype = wave.data_ptr(), HOP * 250, 0, 0
        row.sid_src, row.sid_tgt, row.first, row.count = 0, 1, 0, 32
        row.noise, row.noise_stride, row.noise_scale = noise.data_ptr(), CAP_F, 1.0
        row.z, row.z_stride = z.data_ptr(), CAP_F
    final = stream.spectrogram_ready(HOP * 250, False, N_FFT, HOP)
    for change, what in ((lambda: setattr(rows[1], "count", final - 96 + 1), b"row 1: frames [0, 0 + %d) are not final yet" % (final - 95)),
                         (lambda: setattr(rows[1], "count", final + 1), b"row 1: frames"),
                         (lambda: (setattr(rows[1], "count", 32), setattr(rows[1], "sid_src", 12)), b"row 1: speaker id"),
                         (lambda: (setattr(rows[1], "sid_src", 1), setattr(rows[1], "noise", None)), b"row 1: noise missing"),
                         (lambda: (setattr(rows[1], "noise", noise.data_ptr()), setattr(rows[1], "noise_stride", 100)), b"row 1: noise missing"),
                         (lambda: (setattr(rows[1], "noise_stride", CAP_F), setattr(rows[1], "z_stride", 31)), b"row 1: z_stride"),
                         (lambda: (setattr(rows[1], "z_stride", CAP_F), setattr(rows[1], "wave_dtype", 2)), b"row 1: unknown wave_dtype"),
                         (lambda: (setattr(rows[1], "wave_dtype", 0), setattr(rows[1], "arrived", 0)), b"row 1: wave or z missing, or no samples")):
        change()
        assert L.mbv_convert_ranges(h, rows, 2, HOP, WIN, None) != 0
        assert what in L.mbv_last_error(h), (what, L.mbv_last_error(h))
    rows[1].arrived = HOP * 250
    assert L.mbv_convert_ranges(h, rows, 2, HOP, 2048, None) != 0 and b"win" in L.mbv_last_error(h)
    chunk = (_capi.MbvChunk * 1)()
    chunk[0].z, chunk[0].z_stride, chunk[0].t_frames, chunk[0].first, chunk[0].count = z.data_ptr(), CAP_F, 100, 0, 8
    chunk[0].o = st.o.data_ptr()
    assert L.mbv_decode_chunks_routed(h, chunk, (C.c_int32 * 1)(99), 1, None) != 0 and b"route_frames" in L.mbv_last_error(h)
    assert net.converter_runs() == c0 and net.decoder_runs() == d0
    # the stream and the pool serve on
    st.push(wave[HOP * 240:])
    assert len(pool.step()) == 1                        # (its chunk is handed out by the next poll, without a launch)
    got += st.poll()
    st.close()
    with pytest.raises(ValueError, match="after close"):
        st.push(wave[:1])
    while len(pool):
        pool.step()
    got += st.poll()
    assert st.finished and torch.equal(st.z[:, :, :300], want.z) and torch.equal(st.result(), want.o)
    assert [a for a, _ in got] == [a for a, _ in want_chunks]
    assert all(torch.equal(v, w) for (_, v), (_, w) in zip(got, want_chunks))
    # an empty recording, and one that gives no frame
    empty = _open(net, wave, noise)
    with pytest.raises(ValueError, match="no spectrogram frame"):
        empty.close()
    empty.push(wave[:HOP - 1])
    with pytest.raises(ValueError, match="255 samples .*no spectrogram frame"):
        empty.close()
    assert not empty.closed
    empty.push(wave[HOP - 1:HOP])
    empty.close()
    assert len(empty.poll()) == 1 and empty.finished and empty.result().shape[-1] == 256


def test_splitk_mode_is_deterministic_and_within_rounding():
    net = _net()
    cases = [(300, _audio(HOP * 300 + 1, 95).cuda(), _noise(net, 195)), (100, _audio(HOP * 100, 96).cuda(), _noise(net, 196))]
    default = [_drive(net, w, nz, "1000", 32, (8, 32))[0] for _, w, nz in cases]
    net.set_option("splitk", 1)
    try:
        got = [[_drive(net, w, nz, "1000", 32, (8, 32))[0] for _, w, nz in cases] for _ in range(2)]
    finally:
        net.set_option("splitk", 0)
    for (F, _, _), a, b, d in zip(cases, got[0], got[1], default):
        assert torch.equal(a.z, b.z) and torch.equal(a.result(), b.result()), F
        zd = d.z[:, :, :F].double()
        rel = float(torch.sqrt(torch.mean((a.z[:, :, :F] - zd) ** 2)) / torch.sqrt(torch.mean(zd ** 2)))
        print("splitk, %d frames: z relative rms against the default mode %.3e" % (F, rel))
        assert rel <= 5e-5, (F, rel)
