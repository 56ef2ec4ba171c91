"""Pooled voice conversion on the MI355X: `net.convert_stream` is the existing `spectrogram` + `voice_conversion` path
up to z_hat as a decode stream, and `net.convert_streams(requests)` runs that front half for many audio requests as
one padded run per class of `convert_plan`, every stream bitwise the stand-alone one."""
import numpy as np
import pytest
import torch

import spectrogram_ref as SR
from helpers import rms
from oracle import ref_infer as R

from mb_istft_vits_amd import _capi, wire
from mb_istft_vits_amd.models import ConvertRequest, Request

from gpu_util import make_net

pytestmark = pytest.mark.gpu

MODEL_SR, HOP, WIN, N_FFT, RATE = 16000, 256, 1024, 1024, 24000
# both sides of the 16-frame half-units, the 32-frame WN units and the route rule (T <= 256); not sorted
FRAMES = [33, 1, 300, 16, 100, 2, 257, 15, 64, 17, 256, 32]
REMAINDERS = (0, 1, 255)                # samples on top of hop * F: the sample count is no multiple of the hop
SCHEDULES = [(32, 256), (8, 32), (16, 64), (5, 40), (24, 24), (64, 256), (12, 96)]      # those of test_gpu_admit.py
OTHER_SR = {3: 24000, 8: 24000, 5: 22050, 10: 22050}        # request index -> its in_sr
_NETS = {}


def _net(name="uudb_ms_istft_vits_ms"):
    if name not in _NETS:
        _NETS[name] = make_net(name)
    return _NETS[name][0]


def _seed(s):
    torch.manual_seed(s)
    torch.cuda.manual_seed(s)


def _audio(n, seed, sr=MODEL_SR, pcm=False):
    """n samples of two tones and noise, fp32 in (-1, 1) or that as int16."""
    rs = np.random.RandomState(seed)
    t = np.arange(n) / sr
    x = (0.3 * np.sin(2 * np.pi * (180 + 7 * (seed % 40)) * t) + 0.2 * np.sin(2 * np.pi * 1234.5 * t + seed)
         + 0.05 * rs.standard_normal(n)).astype(np.float32)
    return torch.from_numpy((x * 32767).astype(np.int16) if pcm else x)


def _samples_in(n_model, in_sr):
    """A sample count at in_sr that `resample` turns into exactly n_model samples at the model's rate."""
    if in_sr == MODEL_SR:
        return n_model
    guess = int(n_model * in_sr / MODEL_SR)
    for n in range(max(guess - 3, 1), guess + 4):
        if int(np.ceil(n * (float(MODEL_SR) / in_sr))) == n_model:
            return n
    raise AssertionError((n_model, in_sr))


def _request(F, k, seed=0, in_sr=MODEL_SR, **kw):
    n_model = HOP * F + REMAINDERS[k % 3]
    w = _audio(_samples_in(n_model, in_sr), 100 * seed + k, sr=in_sr, pcm=k % 2 == 1)
    if k % 4 == 0:
        w = w.cuda()
    r = ConvertRequest(w, kw.pop("sid_src", (3 * k + 1) % 12), kw.pop("sid_tgt", (5 * k + 2) % 12), MODEL_SR, HOP, WIN,
                       in_sr=in_sr, **kw)
    assert r.model_samples() == n_model and r.frames(N_FFT) == F
    return r


def _requests(seed=0, frames=FRAMES, other_sr=OTHER_SR):
    """Mixed lengths, dtypes, devices, sid pairs, noise scales, rates and chunk schedules."""
    reqs = [_request(F, k, seed, in_sr=other_sr.get(k, MODEL_SR), noise_scale=(0.0, 0.5, 1.0)[(k + k // 3) % 3],
                     chunk_frames=SCHEDULES[k % 7][0], max_chunk_frames=SCHEDULES[k % 7][1])
            for k, F in enumerate(frames)]
    return reqs


def _solo(net, r):
    """The stand-alone call the contract names for a request."""
    return net.convert_stream(r.wave, r.sid_src, r.sid_tgt, r.model_sr, r.hop_size, r.win_size, in_sr=r.in_sr,
                              noise_scale=r.noise_scale, chunk_frames=r.chunk_frames, max_chunk_frames=r.max_chunk_frames)


def _solo_text(net, r):
    return net.infer_stream(r.x[None].cuda(), torch.tensor([r.x.numel()]).cuda(), torch.tensor([r.sid]).cuda(),
                            r.noise_scale, r.length_scale, r.noise_scale_w, r.max_len, r.chunk_frames, r.max_chunk_frames)


def _same(a, b):
    """z, g, y_lengths and schedule of two streams, bitwise."""
    if a.z.shape != b.z.shape or not torch.equal(a.z, b.z):
        return False
    if a.g.shape != b.g.shape or not torch.equal(a.g, b.g):
        return False
    return torch.equal(a.y_lengths, b.y_lengths) and a.schedule == b.schedule and a.o.shape == b.o.shape


def _true_peak(net, o, frames):
    """The peak `service_pcm16(auto_normalize=True)` divides by, for a finished waveform [1, 1, n]."""
    w, valid = net.resample(o, MODEL_SR, RATE, y_lengths=torch.tensor([frames]).cuda())
    return w[0, 0, :int(valid[0])].abs().max().reshape(1)


def _plan_runs(net, reqs, splitk=False):
    return net.convert_plan([r.frames(N_FFT) for r in reqs], splitk=splitk)[0]


@pytest.mark.parametrize("F", [1, 17, 64, 257])
def test_convert_stream_is_the_existing_path(F):
    """Contract clause 1: z, the finished waveform and the int16 of the wire against `spectrogram` +
    `voice_conversion` and `wire.convert_pcm16`, from the same device RNG state."""
    net = _net()
    k = FRAMES.index(F)
    r = _request(F, k, seed=1)
    src, tgt = torch.tensor([r.sid_src]).cuda(), torch.tensor([r.sid_tgt]).cuda()
    _seed(100 + F)
    spec, lens = net.spectrogram(r.wave[None].cuda(), N_FFT, HOP, WIN)
    assert spec.shape[-1] == F and int(lens[0]) == F
    o, _, y_mask, (_, _, z_hat) = net.voice_conversion(spec, lens, src, tgt)
    state = torch.cuda.get_rng_state().clone()
    _seed(100 + F)
    runs = net.converter_runs()
    st = _solo(net, r)
    assert net.converter_runs() - runs == 1
    assert torch.equal(torch.cuda.get_rng_state(), state), "one randn(1, I, T) on the device generator"
    assert st.z.shape == (1, net.cfg.inter_channels, F) and torch.equal(st.z, z_hat * y_mask)
    assert torch.equal(st.g, net.emb_g(tgt)) and st.y_lengths.tolist() == [F] and st.y_lengths.dtype == torch.int64
    assert torch.equal(st.run(), o)
    # the wire, given the true peak
    _seed(100 + F)
    want, want_v = wire.convert_pcm16(net, r.wave[None].cuda(), None, src, tgt, MODEL_SR, MODEL_SR, RATE, HOP, WIN)
    _seed(100 + F)
    pcm, valid = wire.stream_pcm16(net, _solo(net, r), MODEL_SR, RATE, peak=_true_peak(net, o, F)).run()
    assert pcm.dtype == torch.int16 and torch.equal(pcm, want) and torch.equal(valid, want_v)
    assert int(valid[0]) == -(-HOP * F * RATE // MODEL_SR) and bool((pcm != 0).any())


def test_convert_stream_resamples_as_convert_pcm16_does():
    net = _net()
    r = _request(33, 3, seed=2, in_sr=24000)                  # int16 at 24 kHz
    assert r.wave.dtype == torch.int16
    src, tgt = torch.tensor([r.sid_src]).cuda(), torch.tensor([r.sid_tgt]).cuda()
    _seed(7)
    want, want_v = wire.convert_pcm16(net, r.wave[None].cuda(), None, src, tgt, 24000, MODEL_SR, RATE, HOP, WIN)
    _seed(7)
    st = _solo(net, r)
    assert st.z.shape[2] == 33
    o = st.run().clone()
    _seed(7)
    pcm, valid = wire.stream_pcm16(net, _solo(net, r), MODEL_SR, RATE, peak=_true_peak(net, o, 33)).run()
    assert torch.equal(pcm, want) and torch.equal(valid, want_v)


def test_the_arguments_reach_z_and_z_matches_the_oracle():
    """Not vacuous: noise_scale, sid_src and sid_tgt change z; and at noise_scale 0.5 (an exact scaling of the draw)
    z is within 5e-5 relative (the bar of DESIGN §7.2's voice conversion test) of the oracle's `voice_conversion`
    given 0.5 * noise on the float64 reference spectrogram."""
    net = _net()
    sd = _NETS["uudb_ms_istft_vits_ms"][1]
    F = 33
    x = _audio(HOP * F + 1, 5)
    got = {}
    for name, kw in (("base", {}), ("noise_scale", dict(noise_scale=1.0)), ("sid_src", dict(sid_src=4)),
                     ("sid_tgt", dict(sid_tgt=8)), ("zero", dict(noise_scale=0.0))):
        a = dict(sid_src=3, sid_tgt=7, noise_scale=0.5)
        a.update(kw)
        _seed(9)
        got[name] = net.convert_stream(x, a["sid_src"], a["sid_tgt"], MODEL_SR, HOP, WIN, noise_scale=a["noise_scale"]).z
    for name in ("noise_scale", "sid_src", "sid_tgt", "zero"):
        assert got[name].shape == got["base"].shape and not torch.equal(got[name], got["base"]), name
    _seed(9)
    noise = torch.randn(1, net.cfg.inter_channels, F, device="cuda")
    ref_spec = SR.spectrogram(x.numpy(), N_FFT, HOP, WIN)[None]
    assert ref_spec.shape == (1, N_FFT // 2 + 1, F)
    ref = R.voice_conversion(sd, net.cfg, ref_spec.astype(np.float32), np.array([F]), np.array([3]), np.array([7]),
                             noise=(0.5 * noise).cpu().numpy())
    zr = (ref["z_hat"] * ref["y_mask"]).numpy()
    rel = rms(got["base"].cpu().numpy() - zr) / max(rms(zr), 1e-3)
    print("convert_stream z against the oracle at noise_scale 0.5: relative rms %.3e" % rel)
    assert rel < 5e-5


@pytest.mark.timeout(600)
def test_streams_are_bitwise_the_stand_alone_streams():
    """Contract clause 2 over the twelve requests."""
    net = _net()
    reqs = _requests()
    assert {r.noise_scale for r in reqs} == {0.0, 0.5, 1.0} and {r.in_sr for r in reqs} == {16000, 22050, 24000}
    assert {r.wave.dtype for r in reqs} == {torch.int16, torch.float32} and {r.wave.is_cuda for r in reqs} == {True, False}
    assert {(r.wave.dtype, r.in_sr != MODEL_SR) for r in reqs} == {(d, o) for d in (torch.int16, torch.float32) for o in (False, True)}
    # a long, loud batch first: the scratch the spectrogram kernel writes into is reused, and whatever is left in
    # the channels past spec_channels and the frames past a row's own must not reach a later run
    loud = [ConvertRequest(torch.full((HOP * 320,), 0.99) * torch.sign(torch.randn(HOP * 320, generator=torch.Generator().manual_seed(k))),
                           k, k + 1, MODEL_SR, HOP, WIN) for k in range(4)]
    for st in net.convert_streams(loud):
        assert bool(torch.isfinite(st.z).all())
    # the N stand-alone calls, in order
    _seed(11)
    runs = net.converter_runs()
    solo = [_solo(net, r) for r in reqs]
    assert net.converter_runs() - runs == len(reqs)
    state = torch.cuda.get_rng_state().clone()
    assert [s.z.shape[2] for s in solo] == FRAMES
    # ... and the one admission
    _seed(11)
    cpu_state = torch.get_rng_state().clone()
    runs = net.converter_runs()
    sts = net.convert_streams(reqs)
    assert net.converter_runs() - runs == _plan_runs(net, reqs) == 2
    assert len(sts) == len(reqs)
    for k, (a, b, r) in enumerate(zip(sts, solo, reqs)):
        assert a.z.shape[0] == 1 and a.z.is_contiguous() and a.y_lengths.shape == (1,)
        assert _same(a, b), (k, r, tuple(a.z.shape), tuple(b.z.shape),
                             float((a.z - b.z).abs().max()) if a.z.shape == b.z.shape else None)
    assert torch.equal(torch.cuda.get_rng_state(), state), "the device generator ends elsewhere"
    assert torch.equal(torch.get_rng_state(), cpu_state), "the CPU generator was touched"
    # downstream: a pool of the admitted streams decodes what the stand-alone streams decode
    pool = net.stream_pool()
    for st in sts[:3]:
        pool.add(st)
    while len(pool):
        pool.step()
    for a, b in zip(sts[:3], solo[:3]):
        assert torch.equal(a.o, b.run())


def test_the_spectrogram_kernel_writes_exact_zeros_into_the_reused_scratch():
    """The posterior encoder's channel-padded input [B, cin_pad, T] is written by the spectrogram kernel alone, into
    scratch that earlier runs used: channels spec_channels .. cin_pad and frames at and past a row's own count are
    exact zeros whatever was there, and the rest is bitwise `net.spectrogram` of the row."""
    net = _net()
    SC = net.cfg.spec_channels
    cpad = -(-SC // 32) * 32
    assert cpad > SC
    loud = [ConvertRequest(torch.full((HOP * 320,), 0.99) * torch.sign(torch.randn(HOP * 320, generator=torch.Generator().manual_seed(k))),
                           k, k + 1, MODEL_SR, HOP, WIN) for k in range(4)]
    net.convert_streams(loud)
    before = net.read_stage("convert_ypad").clone()
    assert before.numel() == 4 * cpad * 320
    frames = [5, 40, 17]
    reqs = [_request(F, k, seed=8) for k, F in enumerate(frames)]
    T = max(frames)
    # not vacuous: where this run's pad channels and tail frames will lie, the scratch holds the loud run's values
    old = before[:3 * cpad * T].view(3, cpad, T)
    assert int(torch.count_nonzero(old[:, SC:])) > 0 and int(torch.count_nonzero(old[0, :, frames[0]:])) > 0
    net.convert_streams(reqs)
    y = net.read_stage("convert_ypad")
    assert y.numel() == 3 * cpad * T
    y = y.view(3, cpad, T)
    bits = y.view(torch.int32)
    assert int(torch.count_nonzero(bits[:, SC:])) == 0, "pad channels"
    for b, (F, r) in enumerate(zip(frames, reqs)):
        assert int(torch.count_nonzero(bits[b, :, F:])) == 0, ("tail frames", b)
        spec, lens = net.spectrogram(r.wave[None].cuda(), N_FFT, HOP, WIN)
        assert int(lens[0]) == F and torch.equal(y[b, :SC, :F], spec[0]) and int(torch.count_nonzero(spec[0])) > 0


@pytest.mark.timeout(600)
def test_admitted_audio_reaches_the_wire_bitwise():
    """Two waves of audio requests through `PcmPool.admit`, text requests admitted in between, steps between the
    admissions: every stream's int16 is bitwise `wire.stream_pcm16` of its stand-alone stream."""
    net = _net()
    frames = [33, 100, 257, 16, 64, 2]
    audio = [_request(F, k, seed=3, in_sr=(MODEL_SR, 24000)[k == 1], noise_scale=(0.5, 1.0)[k % 2],
                      chunk_frames=SCHEDULES[k][0], max_chunk_frames=SCHEDULES[k][1]) for k, F in enumerate(frames)]
    ids = lambda T, s: torch.randint(1, 59, (T,), generator=torch.Generator().manual_seed(s))
    text = [Request(ids(12, 1), sid=2, noise_scale=0.5, chunk_frames=8, max_chunk_frames=32), Request(ids(30, 2), sid=5)]
    arrivals = {0: audio[:3], 1: text, 3: audio[3:]}
    _seed(21)
    want = []
    for step in sorted(arrivals):
        for r in arrivals[step]:
            st = _solo(net, r) if isinstance(r, ConvertRequest) else _solo_text(net, r)
            p = wire.stream_pcm16(net, st, MODEL_SR, RATE)
            pcm, valid = p.run()
            want.append((pcm.clone(), valid.clone(), p.peak.clone()))
    _seed(21)
    sp = net.stream_pool()
    pp = wire.pcm_pool(net, sp, MODEL_SR, RATE)
    fol, steps = [], 0
    while steps <= max(arrivals) or len(pp):
        if steps in arrivals:
            new_reqs = arrivals[steps]
            cr, er = net.converter_runs(), net.encoder_runs()
            new = pp.admit(new_reqs)
            if isinstance(new_reqs[0], ConvertRequest):
                assert net.converter_runs() - cr == _plan_runs(net, new_reqs) and net.encoder_runs() == er
            else:
                assert net.encoder_runs() - er == net.admit_plan([r.x.numel() for r in new_reqs])[0] and net.converter_runs() == cr
            assert len(new) == len(new_reqs) and all(pp.follower(f._st) is f for f in new)
            fol += new
        stepped = [st for st in sp.streams if st._decoded < len(st.schedule)]
        dec, wr = net.decoder_runs(), wire.wire_runs(net)
        out = pp.step()
        steps += 1
        assert net.decoder_runs() - dec == (net.chunks_plan([st.z.shape[2] for st in stepped])[0] if stepped else 0)
        assert wire.wire_runs(net) - wr == (1 if out else 0)
    assert len(fol) == 8 and steps < sum(len(f._st) for f in fol)
    for k, (f, (pcm, valid, peak)) in enumerate(zip(fol, want)):
        assert f.pcm.dtype == torch.int16 and torch.equal(f.pcm, pcm), k
        assert torch.equal(f.valid_samples, valid) and torch.equal(f.peak.view(torch.int32), peak.view(torch.int32)), k


def test_refusals_launch_nothing_and_the_pool_serves_on():
    net = _net()
    good = [_request(F, k, seed=4, noise_scale=0.5, chunk_frames=8, max_chunk_frames=32) for k, F in enumerate([17, 33, 9, 64, 2])]
    _seed(31)
    live_req = [_request(40, 1, seed=5, chunk_frames=4, max_chunk_frames=8), _request(12, 2, seed=5, chunk_frames=2, max_chunk_frames=4)]
    live_want = [_solo(net, r).run().clone() for r in live_req]
    _seed(31)
    pool = net.stream_pool()
    live = pool.admit(live_req)
    pool.step()
    runs, members, state = net.converter_runs(), list(pool.streams), torch.cuda.get_rng_state().clone()
    bad_sid = ConvertRequest(good[2].wave, 3, net.n_speakers, MODEL_SR, HOP, WIN)
    no_frame = ConvertRequest(torch.zeros(HOP - 1), 0, 1, MODEL_SR, HOP, WIN)
    with pytest.raises(IndexError, match="request 2: .*sid_tgt %d" % net.n_speakers):
        pool.admit([good[0], good[1], bad_sid, good[3]])
    with pytest.raises(ValueError, match="request 1: 255 samples .*no spectrogram frame"):
        pool.admit([good[0], no_frame])
    with pytest.raises(ValueError, match="request 1: .*one data config"):
        pool.admit([good[0], ConvertRequest(good[1].wave, 0, 1, MODEL_SR, HOP, 800)])
    with pytest.raises(TypeError, match="all models.Request or all models.ConvertRequest"):
        pool.admit([good[0], Request([1, 2, 3], sid=0)])
    net.set_option("conv_bf16", 3)
    try:
        with pytest.raises(ValueError, match="conv_bf16"):
            pool.admit(good)
        with pytest.raises(ValueError, match="conv_bf16"):
            _solo(net, good[0])
    finally:
        net.set_option("conv_bf16", 0)
    mini = _net("ljs_mini_mb_istft_vits")
    with pytest.raises(AssertionError, match="n_speakers have to be larger than 0."):
        mini.stream_pool().admit([good[0]])
    # the C entry refuses what the plan would not put into one run, and rows it cannot read
    h, L = net._ensure_handle(), _capi.lib()
    I = net.cfg.inter_channels
    w = torch.zeros(HOP * 300).cuda()
    z, noise, g2 = torch.zeros(2, I, 300).cuda(), torch.zeros(2, I, 300).cuda(), torch.zeros(2, net.cfg.gin_channels).cuda()
    two = (_capi.MbvConvertRow * 2)()
    for b, (row, F) in enumerate(zip(two, (300, 20))):
        row.wave, row.samples, row.wave_dtype, row.sid_src, row.sid_tgt = w.data_ptr(), HOP * F, 0, 0, 1
        row.noise, row.noise_scale, row.z = noise[b].data_ptr(), 1.0, z[b].data_ptr()
    for change, what in ((lambda: None, b"more than one run"), (lambda: setattr(two[1], "samples", HOP * 301), b"frames outside"),
                         (lambda: setattr(two[1], "samples", 0), b"no samples"),
                         (lambda: (setattr(two[1], "samples", HOP * 290), setattr(two[1], "sid_src", 12)), b"speaker id"),
                         (lambda: (setattr(two[1], "sid_src", 1), setattr(two[1], "noise_scale", -1.0)), b"noise_scale"),
                         (lambda: (setattr(two[1], "noise_scale", 1.0), setattr(two[1], "wave_dtype", 2)), b"wave_dtype")):
        change()
        assert L.mbv_convert_rows(h, two, 2, 300, HOP, WIN, g2.data_ptr(), None) != 0
        assert what in L.mbv_last_error(h), (what, L.mbv_last_error(h))
    two[1].wave_dtype = 0
    assert L.mbv_convert_rows(h, two, 2, 300, HOP, 2048, g2.data_ptr(), None) != 0 and b"win" in L.mbv_last_error(h)
    # a run wider than its longest row could take a conv route that none of its rows takes alone
    two[0].samples, two[1].samples = HOP * 30, HOP * 20
    assert L.mbv_convert_rows(h, two, 2, 300, HOP, WIN, g2.data_ptr(), None) != 0
    assert b"longest row has 30 frames" in L.mbv_last_error(h)
    assert net.converter_runs() == runs and torch.equal(torch.cuda.get_rng_state(), state)
    assert len(pool.streams) == len(members) and all(a is b for a, b in zip(pool.streams, members))
    # the next valid admission is right, and so are the streams that were live all along
    _seed(41)
    want = [_solo(net, r) for r in good]
    _seed(41)
    sts = pool.admit(good)
    assert len(pool.streams) == 7
    for a, b in zip(sts, want):
        assert _same(a, b)
    while len(pool):
        pool.step()
    for st, o in zip(live, live_want):
        assert torch.equal(st.o, o)
    for a, b in zip(sts, want):
        assert torch.equal(a.o, b.run())


def test_splitk_mode_is_deterministic_and_within_rounding():
    """Contract clause 3: in the low-latency mode the routes follow the launch size, so admission is one class, two
    admissions are bitwise equal, and every z is within 5e-5 relative (rms) of the stand-alone call."""
    net = _net()
    reqs = _requests(seed=6, other_sr={3: 24000})
    net.set_option("splitk", 1)
    try:
        _seed(51)
        solo = [_solo(net, r) for r in reqs]
        got = []
        for _ in range(2):
            _seed(51)
            runs = net.converter_runs()
            got.append(net.convert_streams(reqs))
            assert net.converter_runs() - runs == 1 == _plan_runs(net, reqs, splitk=True)
    finally:
        net.set_option("splitk", 0)
    for k, (a, b, s) in enumerate(zip(got[0], got[1], solo)):
        assert _same(a, b), k
        assert a.z.shape == s.z.shape and torch.equal(a.y_lengths, s.y_lengths) and a.schedule == s.schedule
        rel = float(torch.sqrt(torch.mean((a.z - s.z) ** 2)) / torch.sqrt(torch.mean(s.z ** 2)))
        print("splitk: request %d (%d frames): z relative rms %.3e" % (k, a.z.shape[2], rel))
        assert rel <= 5e-5, (k, rel)


@pytest.mark.timeout(600)
def test_side_stream_and_interleaved_calls():
    net = _net()
    reqs = _requests(seed=7, frames=[33, 1, 257, 16, 100, 17], other_sr={3: 24000})
    _seed(61)
    want = [_solo(net, r) for r in reqs]
    full = [s.run().clone() for s in want]
    torch.cuda.synchronize()
    a = torch.randn(6144, 6144, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    for _ in range(6):                                        # a long kernel queue on the default stream
        a = (a @ a) * 1e-4
    with torch.cuda.stream(side):
        _seed(61)
        pool = net.stream_pool()
        sts = pool.admit(reqs)
        while len(pool):
            pool.step()
    side.synchronize()
    torch.cuda.synchronize()
    for s, b, o in zip(sts, want, full):
        assert _same(s, b) and torch.equal(s.o, o)
    # an infer and a voice_conversion between the admission and the pool's steps, and between two admissions
    x = torch.randint(1, 59, (3, 30), generator=torch.Generator().manual_seed(1)).cuda()
    xl, sid = torch.tensor([25, 30, 12]).cuda(), torch.tensor([0, 1, 2]).cuda()
    ref = net.infer(x, xl, sid, noise_scale=0)[0].clone()
    spec, lens = net.spectrogram(_audio(HOP * 40, 3)[None].cuda(), N_FFT, HOP, WIN)
    _seed(5)
    vc = net.voice_conversion(spec, lens, sid[:1], sid[1:2])[0].clone()
    _seed(61)
    pool = net.stream_pool()
    half = len(reqs) // 2
    sts = pool.admit(reqs[:half])
    state = torch.get_rng_state().clone(), torch.cuda.get_rng_state().clone()
    assert torch.equal(net.infer(x, xl, sid, noise_scale=0)[0], ref)        # (draws its noise too)
    _seed(5)
    assert torch.equal(net.voice_conversion(spec, lens, sid[:1], sid[1:2])[0], vc)
    torch.set_rng_state(state[0])
    torch.cuda.set_rng_state(state[1])
    pool.step()
    sts += pool.admit(reqs[half:])
    state = torch.get_rng_state().clone(), torch.cuda.get_rng_state().clone()
    while len(pool):
        pool.step()
        assert torch.equal(net.infer(x, xl, sid, noise_scale=0)[0], ref)
        _seed(5)
        assert torch.equal(net.voice_conversion(spec, lens, sid[:1], sid[1:2])[0], vc)
    for s, b, o in zip(sts, want, full):
        assert _same(s, b) and torch.equal(s.o, o)


@pytest.mark.timeout(600)
def test_a_table_longer_than_one_upload_launch():
    """65 recordings of 0.1 to 0.2 s in one run: both tables go up in two launches, and an offset wrong in the second
    one shows in table row 64.  Every stream bitwise its stand-alone call, one converter run."""
    net = _net()
    reqs = [_request(7 + k % 5, k, seed=5, noise_scale=(0.0, 0.5, 1.0)[k % 3], chunk_frames=SCHEDULES[k % 7][0],
                     max_chunk_frames=SCHEDULES[k % 7][1]) for k in range(65)]
    assert all(0.1 <= r.model_samples() / MODEL_SR <= 0.2 for r in reqs)
    _seed(17)
    solo = [_solo(net, r) for r in reqs]
    state = torch.cuda.get_rng_state().clone()
    _seed(17)
    runs = net.converter_runs()
    sts = net.convert_streams(reqs)
    assert net.converter_runs() - runs == _plan_runs(net, reqs) == 1
    assert len(sts) == 65
    for k, (a, b, r) in enumerate(zip(sts, solo, reqs)):
        assert _same(a, b), (k, r, tuple(a.z.shape), tuple(b.z.shape))
    assert torch.equal(torch.cuda.get_rng_state(), state), "the device generator ends elsewhere"
