"""Live voice conversion with a bounded look-ahead on the MI355X (`stream.Ahead`): the bounded stream is a
pure function of the recording; every block of z_hat frames is what `net.voice_conversion` gives for the spectrogram
cut at the block's window end, every chunk what `net.dec` gives for the z_hat frames cut at its D; the seam is the
fp32 formula; the wire carries the bounded waveform."""
import ctypes as C

import numpy as np
import pytest
import torch

from mb_istft_vits_amd import _capi, stream, synth, wire
from mb_istft_vits_amd.stream import Ahead

from gpu_util import make_net

pytestmark = pytest.mark.gpu

MODEL_SR, HOP, WIN, N_FFT, SPF = 16000, 256, 1024, 1024, 256
CAP_F = 310
CAP = HOP * CAP_F + 100
SRC, TGT = 3, 7
RECS = {263: (1, False), 300: (255, True)}          # frames -> (samples past the last whole hop, int16)
A = (Ahead(8, 4), 8, (8, 8))                        # (ahead, convert_frames, (chunk_frames, max_chunk_frames))
B = (Ahead(0, 1), 1, (1, 1))
A_SEAM = (Ahead(8, 4, seam_ms=5.0), 8, (8, 8))
SEAM = 80                                           # 5 ms at 16 kHz
PATTERNS = ["one", "320_poll_each", "random"]
_CACHE = {}


def _net():
    if "net" not in _CACHE:
        _CACHE["net"] = make_net("uudb_ms_istft_vits_ms")[0]
    return _CACHE["net"]


def _wave(F):
    if ("wave", F) not in _CACHE:
        rem, pcm = RECS[F]
        n = HOP * F + rem
        rs = np.random.RandomState(F)
        t = np.arange(n) / MODEL_SR
        x = (0.3 * np.sin(2 * np.pi * (180 + F % 40) * t) + 0.2 * np.sin(2 * np.pi * 1234.5 * t + F)
             + 0.05 * rs.standard_normal(n)).astype(np.float32)
        _CACHE["wave", F] = torch.from_numpy((x * 32767).astype(np.int16) if pcm else x).cuda()
    return _CACHE["wave", F]


def _spec(F):
    if ("spec", F) not in _CACHE:
        spec, lens = _net().spectrogram(_wave(F)[None], N_FFT, HOP, WIN)
        assert lens.tolist() == [F] and spec.shape[2] == F
        _CACHE["spec", F] = spec
    return _CACHE["spec", F]


def _open(F, setting, **kw):
    ahead, cf, sched = setting
    return _net().convert_live(SRC, TGT, MODEL_SR, HOP, WIN, CAP, dtype=_wave(F).dtype, seed=1000 + F,
                               chunk_frames=sched[0], max_chunk_frames=sched[1], convert_frames=cf, ahead=ahead, **kw)


def _cuts(pattern, n, seed):
    if pattern == "one":
        return [n]
    if pattern == "320_poll_each":
        return [320] * (n // 320) + ([n % 320] if n % 320 else [])
    rs, out, left = np.random.RandomState(seed), [], n
    while left:
        k = min(left, int(rs.randint(1, 20001)))
        out.append(k)
        left -= k
    return out


def _drive(F, setting, pattern="one"):
    """-> (the finished stream, [(first_sample, clone of the chunk as handed out)], chunks handed out before close)."""
    st, wave, got, off = _open(F, setting), _wave(F), [], 0

    def take():
        for a, v in st.poll():
            got.append((a, v.clone()))

    for k in _cuts(pattern, wave.numel(), F):
        st.push(wave[off:off + k])
        off += k
        take()
    early = len(got)
    st.close()
    take()
    assert st.finished and st.poll() == [] and st.frames == F and st.y_lengths.tolist() == [F]
    return st, got, early


def _done(F, setting, pattern="one"):
    """A finished stream per (recording, setting, pattern), driven once and shared (nothing below writes to it)."""
    key = ("done", F, repr(setting), pattern)
    if key not in _CACHE:
        _CACHE[key] = _drive(F, setting, pattern)
    return _CACHE[key]


def _z_hat_cut(F, E):
    """z_hat of `net.voice_conversion` on the spectrogram of the whole recording cut at E frames, the stream's seed."""
    key = ("vc", F, E)
    if key not in _CACHE:
        dev = _spec(F).device
        out = _net().voice_conversion(_spec(F)[:, :, :E].contiguous(), torch.tensor([E], device=dev),
                                      torch.tensor([SRC], device=dev), torch.tensor([TGT], device=dev), seed=1000 + F)
        _CACHE[key] = out[3][2]
    return _CACHE[key]


def _dec_cut(st, key, D):
    """`net.dec(z_live[:, :, :D], g)[0]` [1, 1, 256 D]."""
    key = ("dec", key, D)
    if key not in _CACHE:
        _CACHE[key] = _net().dec(st.z[:, :, :D].contiguous(), st.g)[0]
    return _CACHE[key]


def _blocks(F, setting):
    """[(a, b, E_k)] of the grid."""
    ahead, cf, _ = setting
    return [(a, min(a + cf, F), min(a + cf + ahead.conv, F)) for a in range(0, F, cf)]


def _chunks(F, setting):
    """[(first, count, D)] of the schedule."""
    ahead, _, sched = setting
    return [(f, n, min(f + n + ahead.dec, F)) for f, n in stream.chunk_schedule(F, *sched)]


# ---------------------------------------------------------------------------------------- 1: the full reach is today
@pytest.mark.parametrize("F", sorted(RECS))
def test_the_full_reach_is_bitwise_the_unbounded_stream(F):
    net = _net()
    r_conv, r_dec = net.converter_context()[1], stream.decoder_context(net._config_struct())[1]
    for cf, sched in ((32, (32, 256)), (1, (8, 32))):
        want, want_chunks, _ = _drive(F, (None, cf, sched), "320_poll_each")
        s0 = net.seam_runs()
        got, got_chunks, _ = _drive(F, (Ahead(r_conv, r_dec), cf, sched), "320_poll_each")
        assert net.seam_runs() == s0
        assert torch.equal(got.z, want.z) and torch.equal(got.result(), want.result()), (F, cf, sched)
        assert [a for a, _ in got_chunks] == [a for a, _ in want_chunks] and got.schedule == want.schedule
        assert all(torch.equal(v, w) for (_, v), (_, w) in zip(got_chunks, want_chunks)), (F, cf, sched)


# ---------------------------------------------------------------------------------------- 2: a pure function
@pytest.mark.parametrize("F", sorted(RECS))
@pytest.mark.parametrize("name", ["A", "B"])
def test_the_bounded_stream_does_not_depend_on_the_pushes(F, name):
    setting = {"A": A, "B": B}[name]
    first, first_chunks, _ = _done(F, setting)
    assert [(a // SPF, v.shape[-1] // SPF) for a, v in first_chunks] == stream.chunk_schedule(F, *setting[2])
    assert torch.equal(torch.cat([v for _, v in first_chunks], dim=-1), first.result())
    early = []
    for pattern in PATTERNS[1:]:
        st, got, e = _drive(F, setting, pattern)
        early.append(e)
        assert torch.equal(st.z, first.z) and torch.equal(st.result(), first.result()), (F, name, pattern)
        assert [a for a, _ in got] == [a for a, _ in first_chunks]
        assert all(torch.equal(v, w) for (_, v), (_, w) in zip(got, first_chunks)), (F, name, pattern)
    # 320 samples a push: audio leaves long before the recording ends (the unbounded stream waits for 120 frames)
    ahead, cf, sched = setting
    lag_samples = _open(F, setting).plan.lag()[0]
    assert early[0] >= (HOP * F - lag_samples) // (HOP * sched[1]) - 1 > 20


@pytest.mark.parametrize("F,setting", [(300, A), (263, B), (300, A_SEAM)])
def test_a_pool_serves_bounded_streams_next_to_the_others(F, setting):
    """A bounded live stream, an unbounded live stream and a text stream in one StreamPool: the blocks of the bounded
    member and the range of the unbounded one share ONE converter run per step, the chunks one decode call, the seamed
    member adds one seam launch per step in which it decoded; every chunk is bitwise the stream alone."""
    net = _net()
    solo, solo_chunks, _ = _done(F, setting)
    want = dict(solo_chunks)
    plain_solo, plain_chunks, _ = _done(300, (None, 32, (32, 256)))
    x, xl, sid = synth.synthetic_batch(net.cfg, 1, 20, seed=4, ragged=True)
    text = net.infer_stream(torch.from_numpy(x).cuda(), torch.from_numpy(xl).cuda(), torch.from_numpy(sid).cuda(),
                            noise_scale=0.5, chunk_frames=8, max_chunk_frames=32, seed=5)
    text_want = net.dec_stream(text.z.clone(), text.g).run().clone()
    pool = net.stream_pool()
    st, plain = _open(F, setting), _open(300, (None, 32, (32, 256)))
    for m in (text, st, plain):
        pool.add(m)
    waves, fed, seen, plain_seen, seams = {id(st): _wave(F), id(plain): _wave(300)}, {id(st): 0, id(plain): 0}, {}, {}, 0
    for step in range(400):
        for m in (st, plain):
            w = waves[id(m)]
            if not m.closed:
                n = min(HOP * 45 + 13, w.numel() - fed[id(m)])
                if n:
                    m.push(w[fed[id(m)]:fed[id(m)] + n])
                    fed[id(m)] += n
                else:
                    m.close()
        due = bool(st.pending()) or plain.pending() is not None
        c0, d0, s0 = net.converter_runs(), net.decoder_runs(), net.seam_runs()
        out = pool.step()
        assert net.converter_runs() - c0 == int(due), step
        if out:
            routes = []
            for m, a, v in out:
                if m is st:
                    f, n = a // SPF, v.shape[-1] // SPF
                    routes.append(max(st.plan.t_frames(f, n), 257))
                else:
                    routes.append(max(m.z_frames, 257) if m is plain else m.z.shape[2])
            assert net.decoder_runs() - d0 == net.chunks_plan(routes)[0], (step, routes)
        else:
            assert net.decoder_runs() == d0
        assert len({id(m) for m, _, _ in out}) == len(out)
        decoded = [a for m, a, _ in out if m is st]
        # a seam launch iff the seamed member decoded a chunk with a head to blend or an overhang to keep
        acts = bool(decoded) and bool(st.seam) and (decoded[0] > 0 or SPF * F - decoded[0] > SPF * setting[2][0])
        assert net.seam_runs() - s0 == int(acts), (step, decoded)
        seams += int(acts)
        for m, a, v in out:
            if m is st:
                seen[a] = v.clone()
            elif m is plain:
                plain_seen[a] = v.clone()
        if not len(pool):
            break
    assert len(pool) == 0
    assert sorted(seen) == sorted(want) and all(torch.equal(seen[a], want[a]) for a in want)
    assert all(torch.equal(plain_seen[a], v) for a, v in plain_chunks) and len(plain_seen) == len(plain_chunks)
    assert st.poll() != [] and st.finished and torch.equal(st.z, solo.z) and torch.equal(st.result(), solo.result())
    assert plain.poll() != [] and torch.equal(plain.result(), plain_solo.result()) and torch.equal(text.o, text_want)
    assert seams == (len(want) if st.seam else 0)


# ---------------------------------------------------------------------------------------- 3, 4: past 256 frames, bitwise
@pytest.mark.parametrize("F", sorted(RECS))
@pytest.mark.parametrize("name", ["A", "B"])
def test_every_block_past_256_is_the_conversion_of_the_cut_spectrogram(F, name):
    setting = {"A": A, "B": B}[name]
    st, _, _ = _done(F, setting)
    n = 0
    for a, b, E in _blocks(F, setting):
        if E > 256:
            assert torch.equal(st.z[:, :, a:b], _z_hat_cut(F, E)[:, :, a:b]), (F, name, a, b, E)
            n += 1
    assert n >= (F - 256) // setting[1]


@pytest.mark.parametrize("F", sorted(RECS))
@pytest.mark.parametrize("name", ["A", "B"])
def test_every_chunk_past_256_is_the_decode_of_the_cut_z(F, name):
    setting = {"A": A, "B": B}[name]
    st, chunks, _ = _done(F, setting)
    got, n = dict(chunks), 0
    for f, c, D in _chunks(F, setting):
        if D > 256:
            want = _dec_cut(st, (F, name), D)
            assert want.shape[-1] == SPF * D
            assert torch.equal(got[SPF * f], want[:, :, SPF * f:SPF * (f + c)]), (F, name, f, c, D)
            assert torch.equal(st.result()[:, :, SPF * f:SPF * (f + c)], got[SPF * f])
            n += 1
    assert n >= (F - 256) // setting[2][1]


# ---------------------------------------------------------------------------------------- 5: up to 256 frames, rounding
def test_blocks_and_chunks_up_to_256_are_within_the_live_bars():
    """E_k, D <= 256: `net.voice_conversion` and `net.dec` take the narrow kernel there, the live path the tiled one (the
    final length is not known while the recording is open), so the two agree to rounding: the bars of DESIGN §7.11
    clause 4, z 5e-5 relative rms and o 1e-4 rms.  The first block (also the smallest), a middle one and the one that
    ends at 256 exactly, of both settings; the same for the chunks."""
    F = 300
    rel_worst = rms_worst = 0.0
    for name, setting, ends, ds in (("A", A, (16, 136, 256), (12, 132)), ("B", B, (1, 128, 256), (2, 256))):
        st, chunks, _ = _done(F, setting)
        blocks = {E: (a, b) for a, b, E in _blocks(F, setting)}
        for E in ends:
            a, b = blocks[E]
            want = _z_hat_cut(F, E)[:, :, a:b].double()
            rel = float(torch.sqrt(torch.mean((st.z[:, :, a:b] - want) ** 2)) / torch.sqrt(torch.mean(want ** 2)))
            print("%s: z_hat[%d, %d) from the window cut at %d: relative rms %.3e" % (name, a, b, E, rel))
            rel_worst = max(rel_worst, rel)
        got = dict(chunks)
        by_d = {D: (f, c) for f, c, D in _chunks(F, setting)}
        for D in ds:
            f, c = by_d[D]
            want = _dec_cut(st, (F, name), D)[:, :, SPF * f:SPF * (f + c)].double()
            rms = float(torch.sqrt(torch.mean((got[SPF * f] - want) ** 2)))
            print("%s: chunk (%d, %d) decoded from z cut at %d: rms %.3e" % (name, f, c, D, rms))
            rms_worst = max(rms_worst, rms)
    assert rel_worst <= 5e-5, rel_worst
    assert rms_worst <= 1e-4, rms_worst


# ---------------------------------------------------------------------------------------- 6: the seam
@pytest.mark.parametrize("F", sorted(RECS))
def test_the_seam_is_the_fp32_formula_and_touches_nothing_else(F):
    net = _net()
    plain, _, _ = _done(F, A)
    s0 = net.seam_runs()
    st, got, early = _drive(F, A_SEAM, "320_poll_each")
    chunks = _chunks(F, A)
    # one launch per decode call, none for a chunk with neither a head nor an overhang (there is none here)
    assert net.seam_runs() - s0 == len(chunks) and early > 20
    assert st.seam == SEAM and torch.equal(st.z, plain.z)
    o, ref = st.result(), plain.result()
    i = np.arange(SEAM)
    inv = np.float32(1.0) / np.float32(SEAM + 1)
    w_p, w_q = (SEAM - i).astype(np.float32) * inv, (i + 1).astype(np.float32) * inv
    assert w_p.dtype == w_q.dtype == np.float32
    outside = torch.ones(SPF * F, dtype=torch.bool, device=o.device)
    checked = 0
    for (fp, cp, Dp), (f, c, D) in zip(chunks, chunks[1:]):
        head = min(SEAM, SPF * c)
        a = SPF * f
        outside[a:a + head] = False
        if Dp > 256 and D > 256:
            p = _dec_cut(plain, (F, "A"), Dp)[0, 0, a:a + head].cpu().numpy()
            q = _dec_cut(plain, (F, "A"), D)[0, 0, a:a + head].cpu().numpy()
            want = p * w_p[:head] + q * w_q[:head]                 # fp32 products, one fp32 sum: no contraction in NumPy
            assert want.dtype == np.float32
            assert np.array_equal(o[0, 0, a:a + head].cpu().numpy().view(np.int32), want.view(np.int32)), (F, f)
            checked += 1
        # the head starts at what the previous decode gave and ends at the chunk's own samples
        assert torch.equal(ref[0, 0, a + head:SPF * (f + c)], o[0, 0, a + head:SPF * (f + c)])
    assert checked >= (F - 256) // 8 - 2 and checked >= 1
    assert torch.equal(o[0, 0][outside], ref[0, 0][outside])
    assert not torch.equal(o, ref)
    # nothing handed out changed afterwards
    assert [a for a, _ in got] == [SPF * f for f, _, _ in chunks]
    assert all(torch.equal(v, o[:, :, a:a + v.shape[-1]]) for a, v in got)
    # ... and it is the same stream under another cut
    again, _, _ = _drive(F, A_SEAM, "random")
    assert torch.equal(again.result(), o) and torch.equal(again.z, st.z)


# ---------------------------------------------------------------------------------------- 7: the wire
@pytest.mark.parametrize("setting", [A, A_SEAM])
def test_the_live_wire_carries_the_bounded_waveform(setting):
    net = _net()
    in_sr, rate, F = 48000, 8000, 300
    ahead, cf, sched = setting
    n_raw = HOP * F * 3 + 300
    rs = np.random.RandomState(9)
    t = np.arange(n_raw) / in_sr
    raw = torch.from_numpy(((0.3 * np.sin(2 * np.pi * 200 * t) + 0.2 * np.sin(2 * np.pi * 1234.5 * t)
                             + 0.05 * rs.standard_normal(n_raw)) * 32767).astype(np.int16)).cuda()
    results = []
    for peak in (None, 0.5):
        for pattern in ("20ms", "random"):
            lw = wire.convert_live_pcm16(net, SRC, TGT, in_sr, MODEL_SR, rate, HOP, WIN, 3 * CAP, dtype=torch.int16,
                                         peak=peak, seed=77, chunk_frames=sched[0], max_chunk_frames=sched[1],
                                         convert_frames=cf, ahead=ahead)
            assert lw.live.ahead is ahead and lw.live.plan.ahead is ahead
            k20 = in_sr // 50
            sizes = [k20] * (n_raw // k20) + [n_raw % k20] if pattern == "20ms" else _cuts("random", n_raw, 3)
            assert min(sizes) > 0
            off, pieces = 0, []
            for k in sizes:
                lw.push(raw[off:off + k])
                off += k
                pieces += [(a, v.numel()) for a, v in lw.poll()]
            early = len(pieces)
            lw.close()
            pieces += [(a, v.numel()) for a, v in lw.poll()]
            assert lw.finished and lw.live.finished and lw.live.frames == F
            if pattern == "20ms":
                assert early > 20
            live = lw.live
            # the wiring of the finished bounded o: a DecodeStream that counts as decoded, chunk by chunk through
            # `stream_pcm16`, and (without a given peak) the one-shot `service_pcm16`
            ds = net.dec_stream(live.z[:, :, :F].clone(), live.g, *sched)
            ds.o.copy_(live.result())
            ds._decoded = len(ds.schedule)
            d0 = net.decoder_runs()
            f = wire.stream_pcm16(net, ds, MODEL_SR, rate, peak=peak)
            pcm_ref, valid_ref = f.run()
            assert net.decoder_runs() == d0 and torch.equal(ds.o, live.result())
            valid = int(valid_ref[0])
            assert torch.equal(lw.valid_samples, valid_ref) and torch.equal(lw.pcm[:, :valid], pcm_ref[:, :valid])
            assert int(torch.count_nonzero(lw.pcm[:, valid:])) == 0 and torch.equal(lw.peak, f.peak)
            if peak is None:
                svc, svc_valid = wire.service_pcm16(net, live.result(), live.y_lengths, MODEL_SR, rate, auto_normalize=False)
                assert torch.equal(svc_valid, valid_ref) and torch.equal(lw.pcm[:, :valid], svc[:, :valid])
            assert pieces[0][0] == 0 and sum(n for _, n in pieces) == valid and len(pieces) == len(ds.schedule)
            results.append((peak, live.z.clone(), live.result().clone(), lw.pcm.clone()))
    for (pk, z, o, pcm), (pk2, z2, o2, pcm2) in zip(results, results[1:]):
        assert torch.equal(z, z2) and torch.equal(o, o2) and (pk != pk2 or torch.equal(pcm, pcm2))


# ---------------------------------------------------------------------------------------- 8: refusals
def test_refusals_launch_nothing_and_the_next_call_is_unaffected():
    net = _net()
    F = 300
    wave = _wave(F)
    want, _, _ = _done(F, A)
    for bad in (Ahead(97, 4), Ahead(8, 25), Ahead(8, 0, seam_ms=5.0), Ahead(8, 4, seam_ms=200.0)):
        with pytest.raises(ValueError):
            _open(F, (bad, 8, (8, 8)))
    with pytest.raises(TypeError):
        _open(F, ((8, 4), 8, (8, 8)))
    with pytest.raises(ValueError, match="envelope|volume"):
        wire.convert_live_pcm16(net, SRC, TGT, 48000, MODEL_SR, 8000, HOP, WIN, 3 * CAP, ahead=Ahead(8, 4), envelope=[1.0])
    with pytest.raises(ValueError, match="pitch"):
        wire.convert_live_pcm16(net, SRC, TGT, 48000, MODEL_SR, 8000, HOP, WIN, 3 * CAP, ahead=Ahead(8, 4), pitch=[1.0])
    net.set_option("conv_bf16", 3)
    try:
        with pytest.raises(ValueError, match="conv_bf16"):
            _open(F, A)
    finally:
        net.set_option("conv_bf16", 0)
    st = _open(F, A)
    st.push(wave[:HOP * 200])
    st.poll()
    h, L = net._ensure_handle(), _capi.lib()
    c0, d0, s0 = net.converter_runs(), net.decoder_runs(), net.seam_runs()
    I = net.cfg.inter_channels
    z = torch.zeros(1, I, CAP_F).cuda()
    noise = torch.zeros(1, I, CAP_F).cuda()
    rows = (_capi.MbvConvertRange * 2)()
    for k, row in enumerate(rows):
        row.wave, row.arrived, row.closed, row.wave_dtype = wave.data_ptr(), HOP * 250, 0, 1
        row.sid_src, row.sid_tgt, row.first, row.count = 0, 1, 8 * k, 8
        row.noise, row.noise_stride, row.noise_scale = noise.data_ptr(), CAP_F, 1.0
        row.z, row.z_stride = z.data_ptr(), CAP_F
    final = stream.spectrogram_ready(HOP * 250, False, N_FFT, HOP)
    ahead = (C.c_int32 * 2)(8, 8)

    def refused(what):
        assert L.mbv_convert_ranges_ahead(h, rows, ahead, 2, HOP, WIN, None) != 0
        assert what in L.mbv_last_error(h), (what, L.mbv_last_error(h))

    ahead[1] = 97
    refused(b"row 1: ahead 97 outside [0, 96]")
    ahead[1] = -1
    refused(b"row 1: ahead -1 outside")
    ahead[1] = 8
    rows[1].first = final - 8 - 7                        # first + count + ahead = final + 1
    refused(b"row 1: frames [%d, %d + 8) are not final yet: they need spectrogram frames up to %d" % (final - 15, final - 15, final + 1))
    rows[1].first = 4                                    # [4, 12) meets row 0's [0, 8) in the same z
    refused(b"rows 0 and 1 write overlapping ranges of one z")
    rows[1].first = 8
    rows[1].sid_src = 12
    refused(b"row 1: speaker id")
    rows[1].sid_src = 0
    assert L.mbv_convert_ranges_ahead(h, rows, ahead, 0, HOP, WIN, None) != 0
    # the seam entry
    o, stash = torch.zeros(SPF * 20).cuda(), torch.zeros(2 * SEAM).cuda()
    srow = (_capi.MbvSeamRow * 2)()
    for k, r in enumerate(srow):
        r.o, r.o_samples, r.stash, r.seam = o.data_ptr(), o.numel(), stash.data_ptr() + 4 * SEAM * k, SEAM
        r.head_first, r.head_count, r.over_first, r.over_count = 1024 * k, SEAM, 1024 * k + 512, SEAM

    def seam_refused(n, what):
        assert L.mbv_seam_rows(h, srow, n, None) != 0
        assert what in L.mbv_last_error(h), (what, L.mbv_last_error(h))

    seam_refused(0, b"bad arguments")
    srow[0].seam = 0
    seam_refused(1, b"row 0: seam 0 outside")
    srow[0].seam = SEAM
    srow[0].head_count = SEAM + 1
    seam_refused(1, b"row 0: head_count and over_count")
    srow[0].head_count = SEAM
    srow[0].over_first = o.numel() - SEAM + 1
    seam_refused(1, b"outside the %d samples of o" % o.numel())
    srow[0].over_first = SEAM - 1
    seam_refused(1, b"row 0: the head and the overhang overlap")
    srow[0].over_first = 512
    srow[0].stash = None
    seam_refused(1, b"row 0: o or stash missing")
    srow[0].stash = stash.data_ptr()
    srow[1].stash = stash.data_ptr()
    seam_refused(2, b"rows 0 and 1 share a stash")
    assert (net.converter_runs(), net.decoder_runs(), net.seam_runs()) == (c0, d0, s0)
    assert int(torch.count_nonzero(z)) == 0 and int(torch.count_nonzero(o)) == 0 and int(torch.count_nonzero(stash)) == 0
    # the kernel alone, on a valid row: the blend, then the stash
    rs = np.random.RandomState(1)
    o_h, p_h = rs.standard_normal(o.numel()).astype(np.float32), rs.standard_normal(SEAM).astype(np.float32)
    o.copy_(torch.from_numpy(o_h))
    stash[:SEAM].copy_(torch.from_numpy(p_h))
    srow[0].head_first, srow[0].head_count, srow[0].over_first, srow[0].over_count = 300, 70, 512, 33
    assert L.mbv_seam_rows(h, srow, 1, net._stream()) == 0 and net.seam_runs() == s0 + 1
    i = np.arange(70)
    inv = np.float32(1.0) / np.float32(SEAM + 1)
    blend = o_h.copy()
    blend[300:370] = p_h[:70] * ((SEAM - i).astype(np.float32) * inv) + o_h[300:370] * ((i + 1).astype(np.float32) * inv)
    assert np.array_equal(o.cpu().numpy().view(np.int32), blend.view(np.int32))
    assert np.array_equal(stash.cpu().numpy(), np.concatenate([o_h[512:545], p_h[33:], np.zeros(SEAM, np.float32)]))
    # two blocks of one recording as two rows of one run: bitwise the two runs of one row each
    assert L.mbv_convert_ranges_ahead(h, rows, ahead, 2, HOP, WIN, net._stream()) == 0, L.mbv_last_error(h)
    assert net.converter_runs() == c0 + 1
    both = z.clone()
    z.zero_()
    for k in range(2):
        one = (_capi.MbvConvertRange * 1)(rows[k])
        assert L.mbv_convert_ranges_ahead(h, one, (C.c_int32 * 1)(8), 1, HOP, WIN, net._stream()) == 0
    assert int(torch.count_nonzero(both[:, :, :16])) > 0 and int(torch.count_nonzero(both[:, :, 16:])) == 0
    assert torch.equal(both, z)
    # the stream serves on
    st.push(wave[HOP * 200:])
    st.poll()
    st.close()
    st.poll()
    assert st.finished and torch.equal(st.z, want.z) and torch.equal(st.result(), want.result())
