"""Pooled wire output on the MI355X: `mbv_resample_pcm16_chunks` / `wire.pcm_pool` turn what has become final on many
streams into int16 in ONE launch per tick.  Every stored value is compared bitwise: with the same steps made row by
row through `mbv_resample_pcm16_range`, and end to end with `wire.service_pcm16` of the finished waveform."""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

from mb_istft_vits_amd import _capi, synth, wire

import test_gpu_live_wire as LW
from gpu_util import make_net, ptr

pytestmark = pytest.mark.gpu

SENTINEL = -12345
T_MAX = 300
# (chunk_frames, max_chunk_frames), dealt round the streams
SCHEDULES = [(32, 256), (8, 32), (16, 64), (5, 40), (24, 24), (64, 256), (12, 96)]
_NETS = {}


def _net(name="ljs_mini_mb_istft_vits"):
    if name not in _NETS:
        _NETS[name] = make_net(name)[0]
    return _NETS[name]


def _lag(orig, target, res_type):
    if orig == target:
        return 0
    taps, left = C.c_int32(), C.c_int32()
    assert _capi.lib().mbv_resample_bank(orig, target, {"kaiser_best": 0, "kaiser_fast": 1}[res_type], None, 0, None,
                                         C.byref(taps), C.byref(left)) == 0
    return taps.value - left.value - 1


# ------------------------------------------------------------------------------------------------ the raw call
class Row:
    """One stream's state for the raw call, twice: driven row by row through the ranged step (ref) and pooled."""

    def __init__(self, k, n, valid, orig, target, res_type, lag):
        g = torch.Generator().manual_seed(1000 * k + n)
        self.n, self.k = n, k
        self.x = (torch.rand(n, generator=g) * 3 - 1.5).cuda()              # |x| up to 1.5: the conversion clips
        self.valid = None if valid is None else torch.tensor([valid], device="cuda", dtype=torch.int64)
        self.width = wire.resample_ready(orig, target, n, n, res_type)
        a, b = [lag + 1, 301, lag + 9, 777, 1, lag, 1500, 7][k % 8], [lag + 17, 1501, 778, 2999, lag + 2, 900, 2000, 64][k % 8]
        self.frontiers = sorted([min(n, a), min(n, max(a, b)), n - 1 if k % 3 == 0 else n, n])
        self.peak = None
        self.state = [self._fresh(), self._fresh()]                         # [ref, pooled]
        self.done = 0

    def _fresh(self):
        return dict(pcm=torch.full((1, self.width), SENTINEL, device="cuda", dtype=torch.int16),
                    running=torch.zeros(1, device="cuda"), ns=torch.full((1,), -1, device="cuda", dtype=torch.int64))

    def chunk(self, x, in_avail, first, count, with_ns):
        s = self.state[1]
        c = _capi.MbvPcmChunk()
        c.wave, c.in_total = x.data_ptr(), self.n
        c.valid_samples = self.valid.data_ptr() if self.valid is not None else None
        c.in_avail, c.out_first, c.out_count = in_avail, first, count
        c.peak = self.peak.data_ptr() if self.peak is not None else None
        c.pcm, c.pcm_capacity = s["pcm"].data_ptr(), self.width
        c.running_peak = s["running"].data_ptr()
        c.out_samples = s["ns"].data_ptr() if with_ns else None
        return c


def _rows(net, orig, target, res_type):
    lag = _lag(orig, target, res_type)
    # (n, valid): whole rows, trimmed rows, a row shorter than the filter's half-width, a valid length below it, an empty row
    spec = [(3001, None), (2500, 2000), (1800, None), (777, 700), (300, None), (64, 64), (13, None), (2000, 0),
            (2000, 13), (1500, 1000), (4000, None), (5000, 4999)]
    rows = [Row(k, n, v, orig, target, res_type, lag) for k, (n, v) in enumerate(spec)]
    for r in rows[0::2]:                                                    # every other row is normalised by its true peak
        out, ns = net.resample(r.x.view(1, 1, -1), orig, target, valid_samples=r.valid, res_type=res_type)
        m = int(ns[0])
        r.peak = (out[0, 0, :m].abs().max() if m else out.new_zeros(())).reshape(1).clone()
    assert float(rows[0].peak) > 0.01 and float(rows[8].peak) >= 0.0
    return rows


@pytest.mark.timeout(900)
@pytest.mark.parametrize("res_type", ["kaiser_best", "kaiser_fast"])
@pytest.mark.parametrize("orig,target", [(22050, 24000), (22050, 16000), (22050, 22050)])
def test_raw_call_is_bitwise_the_ranged_step_row_by_row(orig, target, res_type):
    net = _net()
    for poison in (float("nan"), 1e30):
        rows = _rows(net, orig, target, res_type)
        packed_rows = 0
        for step in range(4):
            chunks, pieces, xs = [], [], []
            for r in rows:
                f = r.frontiers[step]
                ready = wire.resample_ready(orig, target, f, r.n, res_type)
                a, b = r.done, ready
                x = r.x.clone()
                x[f:] = poison                                              # nothing at or past in_avail may be read
                xs.append(x)
                ref = r.state[0]
                net.resample_pcm16_range(x.view(1, 1, -1), orig, target, f, a, b - a, ref["pcm"], valid_samples=r.valid,
                                         peak=r.peak, running_peak=ref["running"],
                                         out_samples=ref["ns"] if step == 0 else None, res_type=res_type)
                if r.k == 0 and b - a >= 2:                                 # two chunks of one row, disjoint ranges
                    mid = a + (b - a) // 2
                    chunks += [r.chunk(x, f, mid, b - mid, step == 0), r.chunk(x, f, a, mid - a, step == 0)]
                    pieces += [(r, mid, b), (r, a, mid)]
                else:
                    chunks.append(r.chunk(x, f, a, b - a, step == 0))
                    pieces.append((r, a, b))
                r.done = b
            total, first = wire.pcm_chunks_plan(orig, target, chunks, res_type)
            assert total == sum(b - a for _, a, b in pieces)
            packed = torch.full((total + 64,), SENTINEL, device="cuda", dtype=torch.int16)
            runs = wire.wire_runs(net)
            net.resample_pcm16_chunks(chunks, orig, target, packed=packed, res_type=res_type)
            assert wire.wire_runs(net) - runs == 1
            torch.cuda.synchronize()
            for r in rows:
                ref, got = r.state
                assert torch.equal(got["pcm"], ref["pcm"]), (r.k, step, poison, int((got["pcm"] != ref["pcm"]).sum()))
                assert torch.equal(got["running"].view(torch.int32), ref["running"].view(torch.int32)), (r.k, step)
                assert torch.equal(got["ns"], ref["ns"]) and int(got["ns"]) >= 0, (r.k, step)
                assert bool((got["pcm"][:, r.done:] == SENTINEL).all())     # only the ranges were written
            want = [r.state[0]["pcm"][0, a:b] for r, a, b in pieces]
            assert torch.equal(packed[:total], torch.cat(want)) and bool((packed[total:] == SENTINEL).all())
            assert first == [sum(b - a for _, a, b in pieces[:i]) for i in range(len(pieces))]
            packed_rows += sum(1 for _, a, b in pieces if b > a)
        assert packed_rows > len(rows)
        for r in rows:                                                      # the yardstick of the ranged step itself
            assert r.done == r.width
            out, ns = net.resample(r.x.view(1, 1, -1), orig, target, valid_samples=r.valid, res_type=res_type)
            if orig == target:
                out = r.x.view(1, 1, -1)
            full = net.to_pcm16(out, auto_normalize=r.peak is not None, valid_samples=ns)
            assert torch.equal(r.state[1]["pcm"], full), (r.k, poison)
            assert torch.equal(r.state[1]["ns"], ns)
    # a call without a packed buffer, and one whose chunks are all empty and carry no out_samples: no launch
    r = rows[0]
    runs = wire.wire_runs(net)
    net.resample_pcm16_chunks([r.chunk(r.x, r.n, 5, 0, False), r.chunk(r.x, 10, 0, 0, False)], orig, target, res_type=res_type)
    assert wire.wire_runs(net) == runs
    before = r.state[1]["pcm"].clone()
    net.resample_pcm16_chunks([r.chunk(r.x, r.n, 5, 100, False)], orig, target, res_type=res_type)
    assert wire.wire_runs(net) == runs + 1 and torch.equal(r.state[1]["pcm"], before)


@pytest.mark.timeout(600)
def test_a_table_longer_than_one_upload_launch():
    """33 chunks: the table goes up in two launches, and an offset wrong in the second one shows in table row 32.
    Every row bitwise its ranged step alone, one wire run, the packed buffer in chunk order."""
    net = _net()
    orig, target, res_type = 22050, 24000, "kaiser_fast"
    lag = _lag(orig, target, res_type)
    rows = [Row(k, 257 + 31 * k, None if k % 3 else 200 + 30 * k, orig, target, res_type, lag) for k in range(33)]
    chunks = []
    for r in rows:
        ref = r.state[0]
        net.resample_pcm16_range(r.x.view(1, 1, -1), orig, target, r.n, 0, r.width, ref["pcm"], valid_samples=r.valid,
                                 running_peak=ref["running"], out_samples=ref["ns"], res_type=res_type)
        chunks.append(r.chunk(r.x, r.n, 0, r.width, True))
    total, first = wire.pcm_chunks_plan(orig, target, chunks, res_type)
    assert total == sum(r.width for r in rows) and first == [sum(r.width for r in rows[:i]) for i in range(33)]
    packed = torch.full((total + 64,), SENTINEL, device="cuda", dtype=torch.int16)
    runs = wire.wire_runs(net)
    net.resample_pcm16_chunks(chunks, orig, target, packed=packed, res_type=res_type)
    assert wire.wire_runs(net) - runs == 1
    torch.cuda.synchronize()
    for r in rows:
        ref, got = r.state
        assert torch.equal(got["pcm"], ref["pcm"]), (r.k, int((got["pcm"] != ref["pcm"]).sum()))
        assert torch.equal(got["running"].view(torch.int32), ref["running"].view(torch.int32)), r.k
        assert torch.equal(got["ns"], ref["ns"]) and int(got["ns"]) >= 0, r.k
    assert torch.equal(packed[:total], torch.cat([r.state[0]["pcm"][0] for r in rows]))
    assert bool((packed[total:] == SENTINEL).all())


# ------------------------------------------------------------------------------------------------ end to end
def _text(net, T, seed):
    x, xl, sid = synth.synthetic_batch(net.cfg, 1, T, seed=seed, ragged=False)
    sid = torch.from_numpy(sid).cuda() if sid is not None else None
    return torch.from_numpy(x).cuda(), torch.from_numpy(xl).cuda(), sid


def _wanted_lengths(net):
    """z-lengths on both sides of every class cut, plus 9, 41, 120 and T_MAX; not sorted"""
    first = net.ragged_classes(T_MAX)
    lens = [T_MAX, 9, 41, 120]
    for f in first[1:]:
        lens += [f, f - 1]
    lens = sorted(set(lens), reverse=True)
    while len(lens) < 12:
        lens.append(lens[len(lens) % 5] + 3)
    return (lens[1::2] + lens[0::2])[:12]


def _streams(net, seed):
    """12 single-utterance infer_streams, cut to the wanted lengths (max_len), different chunk schedules"""
    sts = []
    for k, want in enumerate(_wanted_lengths(net)):
        x, xl, sid = _text(net, 60, seed + k)
        torch.manual_seed(seed + k)
        torch.cuda.manual_seed(seed + k)
        chunk, cap = SCHEDULES[k % len(SCHEDULES)]
        sts.append(net.infer_stream(x, xl, sid=sid, noise_scale=0.667, length_scale=3.0, max_len=want,
                                    chunk_frames=chunk, max_chunk_frames=cap))
    return sts


def _drive(net, sts, model_sr, rate, peaks, host, valid=None):
    """Streams added in three waves; PcmPool.step() until empty, with the launch counts of every step checked.
    -> (followers, pieces per stream [(first_out, piece)], frames per stream or None)"""
    sp = net.stream_pool()
    pp = wire.pcm_pool(net, sp, model_sr, rate)
    waves = [list(range(0, 12, 3)), list(range(1, 12, 3)), list(range(2, 12, 3))]
    fol, pieces = {}, {id(st): [] for st in sts}
    cutters = {id(st): wire.FrameCutter(rate) for st in sts} if host else None
    frames = {id(st): [] for st in sts} if host else None
    steps = 0
    while waves or len(pp):
        if waves and steps in (0, 1, 3):
            for k in waves.pop(0):
                f = pp.add(sts[k], peak=peaks[k])
                assert pp.add(sts[k]) is f and f._st is sts[k]
                fol[id(sts[k])] = f
        stepped = [st for st in sp.streams if st._decoded < len(st.schedule)]
        dec, wr = net.decoder_runs(), wire.wire_runs(net)
        out = pp.step(host=host)
        steps += 1
        assert net.decoder_runs() - dec == (net.chunks_plan([st.z.shape[2] for st in stepped])[0] if stepped else 0)
        assert wire.wire_runs(net) - wr == (1 if out else 0)                 # ONE launch for all streams of the tick
        assert out or not stepped
        for st, a, piece in out:
            got = pieces[id(st)]
            assert a == (got[-1][0] + len(got[-1][1]) if got else 0)         # pieces follow one another
            if host:
                assert isinstance(piece, np.ndarray) and piece.dtype == np.int16 and piece.ndim == 1
                take = max(0, min(len(piece), valid[id(st)] - a))            # a row's stream ends at its valid length
                frames[id(st)] += cutters[id(st)].push(piece[:take])
                piece = piece.copy()                                         # (the view is valid until the next step)
            else:
                assert piece.dtype == torch.int16 and piece.dim() == 1 and piece.is_cuda
            got.append((a, piece))
    assert len(pp) == 0 and pp.step() == [] and steps < sum(len(st) for st in sts)
    if host:
        for st in sts:
            frames[id(st)] += cutters[id(st)].close()
    return fol, pieces, frames


@pytest.mark.timeout(1200)
@pytest.mark.parametrize("name,model_sr,rate", [("ljs_mini_mb_istft_vits", 22050, 24000),
                                                ("uudb_ms_istft_vits_ms", 16000, 24000)])
def test_end_to_end_is_bitwise_service_pcm16(name, model_sr, rate):
    net = _net(name)
    sts = _streams(net, 70)
    lens = [st.z.shape[2] for st in sts]
    first = net.ragged_classes(T_MAX)
    assert len({max(i for i, f in enumerate(first) if f <= n) for n in lens}) >= 2, (lens, first)   # several classes
    assert (net.cfg.gin_channels > 0) == (sts[0].g is not None)
    # first pass: no normalisation, device views
    fol, pieces, _ = _drive(net, sts, model_sr, rate, [None] * 12, host=False)
    true_peaks, valid = [], {}
    for st in sts:
        f = fol[id(st)]
        ref, v = wire.service_pcm16(net, st.o, st.y_lengths, model_sr, rate, auto_normalize=False)
        assert f.pcm.dtype == torch.int16 and torch.equal(f.pcm, ref), st.z.shape[2]
        assert torch.equal(f.valid_samples, v)
        assert torch.equal(torch.cat([p for _, p in pieces[id(st)]]), ref[0])
        wave, ns = net.resample(st.o, model_sr, rate, y_lengths=st.y_lengths)
        assert torch.equal(f.peak.view(torch.int32), wave[0, 0, :int(ns[0])].abs().max().reshape(1).view(torch.int32))
        with pytest.raises(StopIteration):                                  # wired ahead: handed out, then the end
            for _ in range(len(f) + 1):
                next(f)
        true_peaks.append(f.peak.clone())
    # second pass: the same utterances, every other one fed its true peak; the pieces through ONE host buffer
    sts2 = _streams(net, 70)
    peaks = [true_peaks[k] if k % 2 else None for k in range(12)]
    for st, st2 in zip(sts, sts2):
        valid[id(st2)] = int(fol[id(st)].valid_samples[0])
    fol2, pieces2, frames = _drive(net, sts2, model_sr, rate, peaks, host=True, valid=valid)
    for k, (st, st2) in enumerate(zip(sts, sts2)):
        f = fol2[id(st2)]
        assert torch.equal(st2.o, st.o)
        ref, v = wire.service_pcm16(net, st2.o, st2.y_lengths, model_sr, rate, auto_normalize=bool(k % 2))
        assert torch.equal(f.pcm, ref) and torch.equal(f.valid_samples, v), (k, st2.z.shape[2])
        assert np.array_equal(np.concatenate([p for _, p in pieces2[id(st2)]]), ref[0].cpu().numpy())
        assert frames[id(st2)] == wire.frame_pcm16(ref[0], rate, valid_samples=int(v[0])), k


# ------------------------------------------------------------------------------------------------ launch counts
def _z(net, Tp, seed):
    return torch.randn(1, net.cfg.inter_channels, Tp, generator=torch.Generator().manual_seed(seed)).cuda()


def _count_syncs(fn):
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            fn()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    return sum("synchroniz" in str(v.message).lower() for v in w)


@pytest.mark.timeout(600)
def test_one_launch_per_tick_and_no_host_synchronisation():
    net = _net()
    lens = [9, 12, 16, 17, 30, 64, 65, 100, 200, 256, 257, 258, 300, 400, 3, 70]
    pooled = [net.dec_stream(_z(net, Tp, 400 + k), None, 32, 64) for k, Tp in enumerate(lens)]
    alone = [net.dec_stream(_z(net, Tp, 400 + k), None, 32, 64) for k, Tp in enumerate(lens)]
    pp = wire.pcm_pool(net, net.stream_pool(), 22050, 24000)
    fol = [pp.add(st) for st in pooled]
    sp = net.stream_pool()
    pcms = [wire.stream_pcm16(net, sp.add(st), 22050, 24000) for st in alone]
    ticks = 0
    while len(pp):
        live = [st for st in pooled if st._decoded < len(st.schedule)]
        dec, wr = net.decoder_runs(), wire.wire_runs(net)
        if ticks == 1:                                                      # (the first tick uploaded the bank)
            out = []
            n = _count_syncs(lambda: out.extend(pp.step()))
            print("host synchronisations in a pooled wire tick of %d streams: %d" % (len(live), n))
            assert n == 0
        else:
            out = pp.step()
        assert len(out) == len(live)
        assert net.decoder_runs() - dec == net.chunks_plan([st.z.shape[2] for st in live])[0]
        assert wire.wire_runs(net) - wr == 1
        # the same streams driven by next(pcm): one launch per stream
        wr = wire.wire_runs(net)
        stepped = sp.step()
        assert len(stepped) == len(live)
        dec = net.decoder_runs()
        for p in pcms:
            if p._st._next < len(p._st.schedule):
                next(p)
        assert net.decoder_runs() == dec and wire.wire_runs(net) - wr == len(live)
        ticks += 1
    assert ticks == max(len(st) for st in pooled) >= 5
    for f, p in zip(fol, pcms):
        assert torch.equal(f.pcm, p.pcm) and torch.equal(f.valid_samples, p.valid_samples)
        assert torch.equal(f.peak.view(torch.int32), p.peak.view(torch.int32))


# ------------------------------------------------------------------------------------------------ mixed driving
@pytest.mark.timeout(600)
def test_mixed_driving_and_a_follower_left_behind():
    net = _net()
    z, z2 = _z(net, 300, 7), _z(net, 200, 8)
    solo = wire.stream_pcm16(net, net.dec_stream(z, None, 8, 64), 22050, 24000, peak=0.7)
    solo_pieces = [(a, v.clone()) for a, v in solo]
    assert len(solo_pieces) >= 6
    sp = net.stream_pool()
    pp = wire.pcm_pool(net, sp, 22050, 24000)
    st, st2 = net.dec_stream(z, None, 8, 64), net.dec_stream(z2, None, 16, 32)
    f, f2 = pp.add(st, peak=0.7), pp.add(st2)
    out = pp.step([st])                                         # pool
    assert len(out) == 1 and out[0][0] is st and out[0][1] == 0 and torch.equal(out[0][2], solo_pieces[0][1][0])
    assert st2._decoded == 0 and f2._wired == 0                 # only the named stream
    dec, wr = net.decoder_runs(), wire.wire_runs(net)
    a, v = next(f)                                              # wired by the pool: handed out, nothing launched
    assert (net.decoder_runs(), wire.wire_runs(net)) == (dec, wr) and a == 0 and torch.equal(v, solo_pieces[0][1])
    a, v = next(f)                                              # not wired yet: alone
    assert (net.decoder_runs(), wire.wire_runs(net)) == (dec + 1, wr + 1)
    assert a == solo_pieces[1][0] and torch.equal(v, solo_pieces[1][1])
    out = pp.step([st])                                         # pool again
    assert out[0][1] == solo_pieces[2][0] and torch.equal(out[0][2], solo_pieces[2][1][0])
    # two plain steps of the decode pool leave the followers behind; one call catches both up
    sp.step()
    sp.step()
    assert st._decoded == 5 and f._wired == 3 and st2._decoded == 2 and f2._wired == 0
    wr = wire.wire_runs(net)
    out = dict((id(s), (a, p)) for s, a, p in pp.step())
    assert wire.wire_runs(net) - wr == 1
    assert st._decoded == 6 and f._wired == 6 and st2._decoded == 3 and f2._wired == 3
    a, p = out[id(st)]
    assert a == solo_pieces[3][0] and torch.equal(p, torch.cat([v[0] for _, v in solo_pieces[3:6]]))
    a, p = out[id(st2)]
    assert a == 0 and len(p) == f2._ready[2] and bool((f2.valid_samples >= 0).all())
    for k in (2, 3, 4, 5):                                      # handed out chunk by chunk, as the stream alone yields them
        a, v = next(f)
        assert a == solo_pieces[k][0] and torch.equal(v, solo_pieces[k][1])
    f.run()
    while len(pp):
        pp.step()
    assert torch.equal(f.pcm, solo.pcm) and torch.equal(f.valid_samples, solo.valid_samples)
    assert torch.equal(f.peak.view(torch.int32), solo.peak.view(torch.int32))
    full2 = net.dec(z2)[0]
    ref2, v2 = wire.service_pcm16(net, full2, None, 22050, 24000, auto_normalize=False)
    assert torch.equal(st2.o, full2) and torch.equal(f2.pcm, ref2) and torch.equal(f2.valid_samples, v2)


# ------------------------------------------------------------------------------------------------ isolation
@pytest.mark.timeout(600)
def test_side_stream_and_interleaved_calls():
    net = _net("uudb_ms_istft_vits_ms")
    gen = torch.Generator().manual_seed(3)
    zs = [_z(net, Tp, 30 + k) for k, Tp in enumerate([120, 17, 64, 258, 9, 65])]
    gs = [(0.3 * torch.randn(1, net.cfg.gin_channels, 1, generator=gen)).cuda() for _ in zs]
    refs = [wire.service_pcm16(net, net.dec(z, g)[0], None, 16000, 24000, auto_normalize=False) for z, g in zip(zs, gs)]

    def drive(between=None, host=False):
        pp = wire.pcm_pool(net, net.stream_pool(), 16000, 24000)
        fol = [pp.add(net.dec_stream(z, g, *SCHEDULES[k % len(SCHEDULES)])) for k, (z, g) in enumerate(zip(zs, gs))]
        while len(pp):
            pp.step(host=host)
            if between:
                between()
        return fol

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fol = drive()
        fol_h = drive(host=True)
    side.synchronize()
    for f, fh, (ref, v) in zip(fol, fol_h, refs):
        assert torch.equal(f.pcm, ref) and torch.equal(f.valid_samples, v)
        assert torch.equal(fh.pcm, ref) and torch.equal(fh.valid_samples, v)
    # an infer and a ragged decode between two steps
    x, xl, sid = synth.synthetic_batch(net.cfg, 3, 25, seed=3, ragged=True)
    x, xl, sid = torch.from_numpy(x).cuda(), torch.from_numpy(xl).cuda(), torch.from_numpy(sid).cuda()
    want = net.infer(x, xl, sid, noise_scale=0)[0].clone()
    zr = torch.randn(3, net.cfg.inter_channels, 120, generator=torch.Generator().manual_seed(5)).cuda()
    gr = (0.3 * torch.randn(3, net.cfg.gin_channels, 1, generator=torch.Generator().manual_seed(6))).cuda()
    rag = net.dec(zr, g=gr, lengths=[120, 40, 9])[0].clone()

    def between():
        assert torch.equal(net.infer(x, xl, sid, noise_scale=0)[0], want)
        assert torch.equal(net.dec(zr, g=gr, lengths=[120, 40, 9])[0], rag)

    for f, (ref, v) in zip(drive(between), refs):
        assert torch.equal(f.pcm, ref) and torch.equal(f.valid_samples, v)


# ------------------------------------------------------------------------------------------------ error paths
@pytest.mark.timeout(600)
def test_error_paths_launch_nothing_and_the_handle_serves_on():
    net = _net()
    L, h = _capi.lib(), net._ensure_handle()
    n = 2000
    xa = (torch.rand(n, generator=torch.Generator().manual_seed(1)) * 2 - 1).cuda()
    xb = (torch.rand(n, generator=torch.Generator().manual_seed(2)) * 2 - 1).cuda()
    width = wire.resample_ready(22050, 24000, n, n)
    pa = torch.full((1, width), SENTINEL, device="cuda", dtype=torch.int16)
    pb = torch.full((1, width), SENTINEL, device="cuda", dtype=torch.int16)
    packed = torch.full((4 * width,), SENTINEL, device="cuda", dtype=torch.int16)
    r = wire.resample_ready(22050, 24000, 1000, n)

    def chunk(x, pcm, in_avail, first, count, cap=width, in_total=n, pcm_ptr=True):
        c = _capi.MbvPcmChunk()
        c.wave, c.in_total, c.in_avail, c.out_first, c.out_count = x.data_ptr(), in_total, in_avail, first, count
        c.pcm, c.pcm_capacity = (pcm.data_ptr() if pcm_ptr else None), cap
        return c

    def call(*chunks, orig=22050, target=24000, filt=0, pk=packed, cap=None):
        arr = (_capi.MbvPcmChunk * len(chunks))(*chunks)
        return L.mbv_resample_pcm16_chunks(h, arr, len(chunks), orig, target, filt, ptr(pk),
                                           (pk.shape[0] if pk is not None else 0) if cap is None else cap, net._stream())

    good = chunk(xa, pa, 1000, 0, r)
    runs = wire.wire_runs(net)
    cases = [((good, chunk(xb, pb, 1000, 0, r + 1)), {}, b"chunk 1:"),        # one output beyond what is final
             ((good, chunk(xb, pb, 1000, r, 1)), {}, b"chunk 1:"),
             ((chunk(xb, pb, 1000, -1, 2), good), {}, b"chunk 0:"),
             ((good, chunk(xb, pb, 1000, 0, -1)), {}, b"chunk 1:"),
             ((good, chunk(xb, pb, -1, 0, 0)), {}, b"chunk 1:"),
             ((good, chunk(xb, pb, n, 0, width, cap=width - 1)), {}, b"outside"),
             ((good, chunk(xb, pb, n, 0, 10, in_total=0)), {}, b"chunk 1:"),
             ((good, chunk(xb, pb, 1000, 0, r, pcm_ptr=False)), {}, b"missing"),
             ((good, chunk(xb, pb, 1000, 0, r)), dict(cap=2 * r - 1), b"packed_capacity"),
             ((good, chunk(xb, pb, 1000, 0, r), chunk(xa, pa, 1000, r - 1, 1)), {}, b"overlapping"),
             ((chunk(xa, pa, 1000, 10, 20), chunk(xa, pa, 1000, 0, 11)), {}, b"overlapping"),
             ((good,), dict(filt=2), b"filter"),
             ((good,), dict(target=22051), b"phases"),
             ((good,), dict(orig=0), b"positive")]
    for chunks, kw, word in cases:
        assert call(*chunks, **kw) != 0, word
        assert word in L.mbv_last_error(h), (word, L.mbv_last_error(h))
    assert L.mbv_resample_pcm16_chunks(h, None, 2, 22050, 24000, 0, None, 0, net._stream()) != 0
    assert L.mbv_resample_pcm16_chunks(h, None, -1, 22050, 24000, 0, None, 0, net._stream()) != 0
    assert L.mbv_resample_pcm16_chunks(h, None, 0, 22050, 24000, 0, None, 0, net._stream()) == 0     # nothing to do
    with pytest.raises(_capi.MbvError, match="chunk 1:"):
        net.resample_pcm16_chunks([good, chunk(xb, pb, 1000, 0, r + 1)], 22050, 24000)
    with pytest.raises(ValueError, match="res_type"):
        net.resample_pcm16_chunks([good], 22050, 24000, res_type="soxr_hq")
    with pytest.raises(ValueError, match="packed"):
        net.resample_pcm16_chunks([good], 22050, 24000, packed=packed.float())
    pp = wire.pcm_pool(net, net.stream_pool(), 22050, 24000)
    with pytest.raises(ValueError, match="ONE utterance"):
        pp.add(net.dec_stream(torch.cat([_z(net, 40, 1), _z(net, 40, 2)])))
    with pytest.raises(ValueError, match="another model"):
        pp.add(_net("uudb_ms_istft_vits_ms").dec_stream(_z(_net("uudb_ms_istft_vits_ms"), 40, 1)))
    torch.cuda.synchronize()
    assert wire.wire_runs(net) == runs and len(pp) == 0                      # the refusals launched nothing ...
    for t in (pa, pb, packed):
        assert bool((t == SENTINEL).all())                                  # ... and wrote nothing
    # the handle serves the next call: two disjoint chunks of one row (adjacent ranges are not overlapping) and another row
    assert call(chunk(xa, pa, 1000, 10, r - 10), chunk(xb, pb, 1000, 0, r), chunk(xa, pa, 1000, 0, 10)) == 0
    assert wire.wire_runs(net) == runs + 1
    refa = torch.full_like(pa, SENTINEL)
    refb = torch.full_like(pb, SENTINEL)
    net.resample_pcm16_range(xa.view(1, -1), 22050, 24000, 1000, 0, r, refa)
    net.resample_pcm16_range(xb.view(1, -1), 22050, 24000, 1000, 0, r, refb)
    assert wire.wire_runs(net) == runs + 3
    assert torch.equal(pa, refa) and torch.equal(pb, refb)
    assert torch.equal(packed[:2 * r], torch.cat([refa[0, 10:r], refb[0, :r], refa[0, :10]]))
    assert bool((packed[2 * r:] == SENTINEL).all())


# ------------------------------------------------------------------------------------------------ every kind of member
MIXED_SR, MIXED_RATE, MIXED_IN_SR = 22050, 24000, 48000
MIXED_LIMITER = wire.Limiter(0.9, lookahead_ms=2.0, hold_ms=4.0)
MIXED_PITCH = [1.0, 1.26, 1.26, 0.8, 0.8, 1.5, 1.0, 1.12, 0.9, 1.0, 2.0, 0.5, 1.0, 1.0]
MIXED_GAIN = [1.0, 0.5, 0.5, 2.0, 2.0, 1.0, 0.0, 1.0, 3.0, 1.0, 1.0, 0.25, 1.0, 1.0]
MIXED_PAUSE_MS = 80.0
MIXED_KINDS = ("limited", "pitched", "measured", "live", "turn")


def _mixed_text(net, T, seed, **kw):
    x = torch.randint(1, 59, (T,), generator=torch.Generator().manual_seed(seed)).view(1, -1).cuda()
    return net.infer_stream(x, torch.tensor([T]).cuda(), torch.tensor([seed % 4]).cuda(), noise_scale=0.5, length_scale=3.0,
                            seed=[seed], chunk_frames=8, max_chunk_frames=16, **kw)


def _mixed_streams(net):
    """the decode streams of (a), (b), (c) and of the two segments of (e), from the same seeds every time"""
    return dict(limited=_mixed_text(net, 12, 801), pitched=_mixed_text(net, 14, 802, pitch=[MIXED_PITCH], gain=[MIXED_GAIN]),
                measured=_mixed_text(net, 9, 803),
                turn=[_mixed_text(net, 8, 804), _mixed_text(net, 10, 805, gain=[MIXED_GAIN[:10]])])


def _mixed_live(net, raw, noise):
    """(d): a live wire that has its whole recording, closed"""
    lw = LW._open(net, MIXED_IN_SR, MIXED_RATE, raw.dtype, noise)
    lw.push(raw)
    lw.close()
    return lw


def _mixed_turn(pp, segments):
    turn = pp.add_turn(1 << 17)
    turn.append(segments[0])
    turn.append(segments[1], pause_ms=MIXED_PAUSE_MS)
    turn.close()
    return turn


def _state(w):
    valid, loudness = int(w.valid_samples[0]), getattr(w, "loudness", None)     # (a turn keeps no running loudness)
    return dict(pcm=w.pcm[:, :valid].clone(), valid=w.valid_samples.clone(), peak=w.peak.clone(),
                loudness=None if loudness is None else loudness.clone())


def _mixed_alone(net, raw, noise):
    """every member driven alone -> {kind: (its concatenated pieces, its final state)}"""
    sts, want = _mixed_streams(net), {}
    for kind, kw in (("limited", dict(limiter=MIXED_LIMITER)), ("pitched", {}),
                     ("measured", dict(loudness=wire.Loudness(target=None)))):
        f = wire.stream_pcm16(net, sts[kind], MIXED_SR, MIXED_RATE, **kw)
        pieces = [v[0].clone() for _, v in f]
        assert len(pieces) >= 3, (kind, len(pieces))                          # several ticks each
        want[kind] = (torch.cat(pieces), _state(f))
    lw, pieces = _mixed_live(net, raw, noise), []
    while not lw.finished:
        pieces += [v.clone() for _, v in lw.poll()]
    want["live"] = (torch.cat(pieces), _state(lw))
    pp = wire.pcm_pool(net, net.stream_pool(), MIXED_SR, MIXED_RATE)
    turn, pieces = _mixed_turn(pp, sts["turn"]), []
    while not turn.finished:
        pieces += [p.clone() for _, _, p in pp.step()]
    assert len(pp) == 0 and len(pp.pool) == 0
    want["turn"] = (torch.cat(pieces), _state(turn))
    return want


def _mixed_pooled(net, raw, noise, host):
    """all five in ONE pool, driven to the end -> ({kind: ([(first, piece)], final state)}, the launches of the first
    tick in which all five had something due)"""
    sts = _mixed_streams(net)
    sp = net.stream_pool()
    pp = wire.pcm_pool(net, sp, MIXED_SR, MIXED_RATE)
    turn = _mixed_turn(pp, sts["turn"])                                       # (the turn first: `out` is ordered by kind)
    lw = pp.add_live(_mixed_live(net, raw, noise))
    members = dict(measured=pp.add(sts["measured"], loudness=wire.Loudness(target=None)),
                   pitched=pp.add(sts["pitched"]), limited=pp.add(sts["limited"], limiter=MIXED_LIMITER), live=lw, turn=turn)
    assert len(pp) == 5 and pp.followers == [members[k] for k in ("measured", "pitched", "limited")]
    assert pp.lives == [lw] and pp.turns == [turn] and members["pitched"]._warp is not None
    kind_of = {id(sts[k]): k for k in ("limited", "pitched", "measured")}
    kind_of.update({id(lw): "live", id(turn): "turn"})
    pieces, full_tick, ticks = {k: [] for k in MIXED_KINDS}, None, 0
    while len(pp):
        before = wire.wire_runs(net), net.warp_runs(), net.loudness_runs()
        out = pp.step(host=host)
        after = wire.wire_runs(net), net.warp_runs(), net.loudness_runs()
        kinds = [kind_of[id(who)] for who, _, _ in out]
        order = [k for k in ("measured", "pitched", "limited", "live", "turn") if k in kinds]
        assert [k for i, k in enumerate(kinds) if k not in kinds[:i]] == order, kinds     # followers, live wires, turns
        if full_tick is None and set(kinds) == set(MIXED_KINDS):
            full_tick = tuple(b - a for a, b in zip(before, after))
        for who, a, piece in out:
            pieces[kind_of[id(who)]].append((a, torch.from_numpy(piece.copy()).cuda() if host else piece.clone()))
        ticks += 1
        assert ticks < 100
    assert len(pp) == 0 and len(sp) == 0 and pp.step() == []
    return {k: (pieces[k], _state(members[k])) for k in MIXED_KINDS}, full_tick


@pytest.mark.timeout(600)
def test_every_kind_of_member_in_one_pool_is_bitwise_the_member_alone():
    """A limited follower, a pitched and shaped one, a measuring one, a live wire and a turn of two segments in ONE
    `PcmPool`: every member's pieces, `pcm`, `valid_samples`, `peak` and `.loudness` are bitwise those of the member
    driven alone, on the device and through the pinned host buffer, and a tick that serves all five makes three wire
    launches (unlimited rows, limited rows, turn rows), one warp launch and at most one loudness launch."""
    net = _net("uudb_ms_istft_vits_ms")
    raw = LW._audio(LW._raw_len(257, 1, MIXED_IN_SR), 61, MIXED_IN_SR, True).cuda()
    noise = LW._noise(net, 161, MIXED_IN_SR)
    alone = _mixed_alone(net, raw, noise)
    assert alone["measured"][1]["loudness"] is not None and bool(torch.isfinite(alone["measured"][1]["loudness"]).all())
    runs = {}
    for host in (False, True):
        got, full_tick = _mixed_pooled(net, raw, noise, host)
        print("host=%s: pieces per member %s, launches of the full tick (wire, warp, loudness) %s"
              % (host, {k: len(got[k][0]) for k in MIXED_KINDS}, full_tick))
        assert full_tick is not None and full_tick[0] == 3 and full_tick[1] == 1 and full_tick[2] <= 1, full_tick
        for kind in MIXED_KINDS:
            (want_pieces, want), (pieces, state) = alone[kind], got[kind]
            assert [a for a, _ in pieces] == [sum(len(p) for _, p in pieces[:i]) for i in range(len(pieces))], kind
            assert torch.equal(torch.cat([p for _, p in pieces]), want_pieces), (kind, host)
            assert int(want["valid"][0]) > 0 and torch.equal(state["valid"], want["valid"]), (kind, host)
            assert torch.equal(state["pcm"], want["pcm"]), (kind, host)
            assert torch.equal(state["peak"].view(torch.int32), want["peak"].view(torch.int32)), (kind, host)
            assert (state["loudness"] is None) == (want["loudness"] is None), kind
            if want["loudness"] is not None:
                assert torch.equal(state["loudness"].view(torch.int32), want["loudness"].view(torch.int32)), (kind, host)
        runs[host] = got
    for kind in MIXED_KINDS:                                                  # the host pieces are the device pieces
        dev, hst = runs[False][kind][0], runs[True][kind][0]
        assert len(dev) == len(hst) and all(a == b and torch.equal(p, q) for (a, p), (b, q) in zip(dev, hst)), kind
