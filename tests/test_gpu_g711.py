"""-m gpu: G.711 on the wire (`mbv_g711_encode` / `_decode`, `mbv_resample_g711_range`,
`mbv_resample_g711_chunks`, MBV_WAVE_ULAW / MBV_WAVE_ALAW rows of `mbv_resample_ranges`, `encoding=` / `in_encoding=`
of the wire entries).  The codec is an integer function of the int16 the existing kernels store, so everything here is
bitwise: the bytes are `g711_ref.encode` of the int16 call on the same arguments, and a G.711 recording is the int16
recording `g711_ref.decode` gives."""
import numpy as np
import pytest
import torch

from mb_istft_vits_amd import _capi, wire
from mb_istft_vits_amd.models import ConvertRequest

import g711_ref
from test_gpu_limiter import (CEILING, _again, _chunk, _n_out, _net, _same, _setting, _small_peak, _text_stream,
                              signal)
from test_gpu_limiter import _run as _run_pcm16
from test_gpu_live_wire import HOP, MODEL_SR, WIN, _audio, _cuts, _noise, _open, _raw_len

pytestmark = pytest.mark.gpu

LAWS = ["ulaw", "alaw"]
PAIRS = [(22050, 8000), (16000, 8000), (8000, 8000)]     # L = 160, M = 441: the long filter; 1 / 2; FIR = false
LIMITS = [None, (7, 19), (0, 0), "defaults"]             # no limiter; (L, H); Limiter()'s defaults at the target rate
SENTINEL = 0x5A
PAD = 5                                                  # bytes past the row: an odd row stride, rows off the dword grid
RATE = 8000
LIM = wire.Limiter()                                     # 0.9, 5 ms, 20 ms: 40 and 160 samples at 8 kHz


def _lim(limit, target):
    if limit is None:
        return None
    return _setting(None if limit == "defaults" else limit, target)


def _case(orig, target):
    net = _net()
    x, valid = signal(orig, target)
    return net, x.cuda(), valid.cuda()


def _encoded(pcm, law):
    """g711_ref.encode of an int16 tensor, as a uint8 tensor on its device"""
    return torch.from_numpy(g711_ref.encode(pcm.cpu().numpy(), law)).to(pcm.device)


def _run(net, x, valid, orig, target, lim, law, cuts=None, peak=None, frontiers=None, poison=None):
    """test_gpu_limiter._run with `encoding=law`: the rows are uint8 [B, width + PAD], sentinel bytes wherever nothing
    has been written yet.  -> (bytes [B, width], running, out_samples)"""
    B, n = x.shape[0], x.shape[-1]
    width = wire.resample_ready(orig, target, n, n)
    out = torch.full((B, width + PAD), SENTINEL, device="cuda", dtype=torch.uint8)
    running = torch.zeros(B, device="cuda")
    ns = torch.full((B,), -1, device="cuda", dtype=torch.int64)
    if frontiers is None:
        steps = [(n, c) for c in sorted(set(cuts or []) | {width})]
    else:
        steps = [(f, wire.limiter_ready(orig, target, f, n, lim[1] if lim else 0)) for f in frontiers]
    done = 0
    for i, (f, end) in enumerate(steps):
        xx = x
        if poison is not None and f < n:
            xx = x.clone()
            xx[:, :, f:] = poison
        net.resample_pcm16_range(xx, orig, target, f, done, end - done, out, valid_samples=valid, peak=peak,
                                 running_peak=running, out_samples=ns if i == 0 else None, limiter=lim, encoding=law)
        assert (out[:, end:] == SENTINEL).all()                       # nothing past the range is written
        done = end
    assert done == width
    return out[:, :width], running, ns


# ------------------------------------------------------------------------------------------------ 1. the codec alone
@pytest.mark.parametrize("law", LAWS)
def test_codec_entries_are_exhaustively_the_tables(law):
    import os
    t = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g711_tables.npz"))
    net = _net()
    every = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16)
    got = net.g711_encode(every, law)
    assert got.dtype == torch.uint8 and got.is_cuda and np.array_equal(got.cpu().numpy(), t[law + "_encode"])
    back = net.g711_decode(torch.arange(256, dtype=torch.int32).to(torch.uint8), law)
    assert back.dtype == torch.int16 and np.array_equal(back.cpu().numpy(), t[law + "_decode"])
    # any shape, an odd count, nothing at all
    odd = every[1000:1000 + 3 * 259].reshape(3, 259).cuda()
    assert torch.equal(net.g711_encode(odd, law), _encoded(odd, law))
    assert net.g711_encode(every[:0], law).shape == (0,) and net.g711_decode(got[:0], law).shape == (0,)
    with pytest.raises(ValueError, match="law"):
        net.g711_encode(every, "pcm16")
    with pytest.raises(TypeError, match="int16"):
        net.g711_encode(every.float(), law)
    with pytest.raises(TypeError, match="uint8"):
        net.g711_decode(every, law)


# ------------------------------------------------------------------------------------------------ 2. the ranged entry
@pytest.mark.parametrize("law", LAWS)
@pytest.mark.parametrize("limit", LIMITS)
@pytest.mark.parametrize("orig,target", PAIRS)
def test_ranged_entry_is_the_encoded_int16_entry(orig, target, limit, law):
    net, x, valid = _case(orig, target)
    lim = _lim(limit, target)
    zero = g711_ref.ZERO[law]
    for peak in (None, torch.tensor([0.4, 0.0, 1.7], device="cuda")):     # row 1: below 0.01, not normalised
        pcm, running, ns = _run_pcm16(net, x, valid, orig, target, lim, peak=peak)
        runs = wire.wire_runs(net)
        got, got_running, got_ns = _run(net, x, valid, orig, target, lim, law, peak=peak)
        assert wire.wire_runs(net) - runs == 1
        assert torch.equal(got, _encoded(pcm, law))
        assert _same((got_running, got_ns), (running, ns))
        for b, n in enumerate(valid.tolist()):                            # the padding holds encode(0)
            assert (got[b, _n_out(n, orig, target):] == zero).all()
        assert int((got[1] == zero).sum()) >= got.shape[1] - _n_out(int(valid[1]), orig, target) > 0
        assert len(torch.unique(got[0])) > 100                            # and the rows are not silence


# ------------------------------------------------------------------------------------------------ 3. chunk invariance
@pytest.mark.parametrize("law", LAWS)
@pytest.mark.parametrize("limit", [None, (7, 19)])
@pytest.mark.parametrize("orig,target", PAIRS)
def test_chunk_invariance_is_bitwise(orig, target, limit, law):
    net, x, valid = _case(orig, target)
    lim = _lim(limit, target)
    L = lim[1] if lim else 0
    n = x.shape[-1]
    width = wire.resample_ready(orig, target, n, n)
    peak = torch.tensor([0.4, 0.0, 1.7], device="cuda")
    want = _run(net, x, valid, orig, target, lim, law, peak=peak)
    # ranges of one sample that start at out_first % 4 = 0, 1, 2; one of 257 samples from % 4 = 3, across a tile;
    # 257 more from % 4 = 0; a start at % 4 = 1; ranges that end inside the row's last partial tile
    cuts = [1, 2, 3, 260, 517, 518, 600, width - 5, width - 1]
    assert width - 5 > 600
    got = _run(net, x, valid, orig, target, lim, law, cuts=cuts, peak=peak)
    assert _same(got, want)
    # an empty range writes nothing but the lengths
    out = torch.full((3, width + PAD), SENTINEL, device="cuda", dtype=torch.uint8)
    ns = torch.full((3,), -1, device="cuda", dtype=torch.int64)
    net.resample_pcm16_range(x, orig, target, n, 257, 0, out, valid_samples=valid, peak=peak, out_samples=ns,
                             limiter=lim, encoding=law)
    assert (out == SENTINEL).all() and torch.equal(ns, want[2])
    # the stream as it runs: nothing at or past the frontier is read
    frontiers = sorted([1, 64, 65, 66 + L, 130, 301, 777, 778, 1500, 2000, n - 1, n])
    for poison in (float("nan"), 1e30):
        got = _run(net, x, valid, orig, target, lim, law, peak=peak, frontiers=frontiers, poison=poison)
        assert _same(got, want), poison


# ------------------------------------------------------------------------------------------------ 4. the pooled entry
@pytest.mark.parametrize("law", LAWS)
@pytest.mark.parametrize("orig,target", PAIRS)
def test_pooled_rows_are_bitwise_their_ranged_calls(orig, target, law):
    net, x, valid = _case(orig, target)
    n = x.shape[-1]
    width = wire.resample_ready(orig, target, n, n)
    limits = [(CEILING, 7, 19), None, _setting(None, target), (0.5, 255, 1024), None, (1.0, 0, 3)]
    rows = [(k % 3, limits[k]) for k in range(6)]
    peak = torch.tensor([0.5], device="cuda")
    frontiers = [700, 1500, n]
    # every row's bytes live in one buffer at offsets 1, 2, 3 mod 4: no row starts on the dword grid
    pitch = (width + 8) // 4 * 4 + 1
    arena = torch.full((6 * pitch + 4,), SENTINEL, device="cuda", dtype=torch.uint8)
    want, state = [], []
    for k, (b, lim) in enumerate(rows):
        xb, vb = x[b:b + 1], valid[b:b + 1]
        want.append(_run(net, xb, vb, orig, target, lim, law, peak=peak, frontiers=frontiers))
        out = arena[1 + k * pitch:1 + k * pitch + width]
        assert out.data_ptr() % 4 == (1 + k) % 4
        state.append((xb[0, 0].contiguous(), vb.clone(), out, torch.zeros(1, device="cuda"),
                      torch.full((1,), -1, device="cuda", dtype=torch.int64), [0]))
    for step, f in enumerate(frontiers):
        # steps 0 and 2: all rows in one call (two launches); step 1: the kinds in a call each (one launch each)
        for kinds in ((None,), (False, True), (None,))[step]:
            chunks, lims, ends = [], [], []
            for (b, lim), (xb, vb, out, running, ns, done) in zip(rows, state):
                if kinds is not None and (lim is not None) != kinds:
                    continue
                end = wire.limiter_ready(orig, target, f, n, lim[1] if lim else 0)
                if step < 2 and not chunks and end > done[0] and (end - done[0]) % 2 == 0:
                    end -= 1                       # an odd count first: the next chunk starts at an odd packed offset
                chunks.append(_chunk(xb, vb, f, done[0], end - done[0], out, running, ns if step == 0 else None, peak))
                lims.append(lim)
                ends.append((out, done, end))
            total = sum(k.out_count for k in chunks)
            assert wire.pcm_chunks_plan(orig, target, chunks)[0] == total      # the plan counts samples: the bytes
            packed = torch.full((total + 8,), SENTINEL, device="cuda", dtype=torch.uint8)
            runs = wire.wire_runs(net)
            net.resample_pcm16_chunks(chunks, orig, target, packed=packed, limits=lims, encoding=law)
            assert wire.wire_runs(net) - runs == (2 if kinds is None else 1), (step, kinds)
            off, odd = 0, 0
            for k, (out, done, end) in zip(chunks, ends):
                assert torch.equal(packed[off:off + k.out_count], out[done[0]:end])
                assert (out[end:] == SENTINEL).all()
                odd += off % 4 != 0
                off += k.out_count
                done[0] = end
            assert (packed[total:] == SENTINEL).all()
            assert odd >= 1 or step == 2                                       # packed offsets off the dword grid
    for k, ((out_w, run_w, ns_w), (_, _, out, running, ns, done)) in enumerate(zip(want, state)):
        assert done[0] == width
        assert torch.equal(out, out_w[0]) and torch.equal(ns, ns_w)
        assert torch.equal(running.view(torch.int32), run_w.view(torch.int32))
    # nothing between the rows was touched
    gaps = torch.ones_like(arena, dtype=torch.bool)
    for k in range(6):
        gaps[1 + k * pitch:1 + k * pitch + width] = False
    assert (arena[gaps] == SENTINEL).all()


# ------------------------------------------------------------------------------------------------ 5. the streams
def _frames_of(pieces, close=True):
    fc = wire.FrameCutter(RATE, sample_bytes=1)
    out = []
    for v in pieces:
        out += fc.push(v)
    return out + fc.close()


@pytest.mark.parametrize("law", LAWS)
@pytest.mark.parametrize("limited", [False, True])
def test_streams_and_pools_are_bitwise_the_one_shot_service(law, limited):
    net = _net()
    st = _text_stream(net, 20, 4)
    st.run()                                                          # the finished waveform st.o
    lim = LIM if limited else None
    peak = _small_peak(net, st) if limited else None                  # without the limiter this peak hard-clips
    kw = dict(limiter=lim, peak=peak) if limited else dict(auto_normalize=False)
    plain, valid = wire.service_pcm16(net, st.o, st.y_lengths, MODEL_SR, RATE, **kw)
    runs = wire.wire_runs(net)
    ref, ref_valid = wire.service_pcm16(net, st.o, st.y_lengths, MODEL_SR, RATE, encoding=law, **kw)
    assert wire.wire_runs(net) - runs == 1                            # the codec is fused on the one-shot path too
    assert ref.dtype == torch.uint8 and torch.equal(ref, _encoded(plain, law)) and torch.equal(ref_valid, valid)
    if not limited:                                                   # auto_normalize: one launch for the peak, one to encode
        auto, _ = wire.service_pcm16(net, st.o, st.y_lengths, MODEL_SR, RATE)
        runs = wire.wire_runs(net)
        got, _ = wire.service_pcm16(net, st.o, st.y_lengths, MODEL_SR, RATE, encoding=law)
        assert wire.wire_runs(net) - runs == 2 and torch.equal(got, _encoded(auto, law))
    # the streamed form
    f = wire.stream_pcm16(net, _again(net, st), MODEL_SR, RATE, peak=peak, limiter=lim, encoding=law)
    pieces = [(a, v[0].clone()) for a, v in f]
    assert len(pieces) >= 3 and all(v.dtype == torch.uint8 for _, v in pieces)
    assert torch.equal(f.pcm, ref) and torch.equal(f.valid_samples, ref_valid)
    n_valid = int(ref_valid[0])
    frames = wire.frame_g711(ref[0], RATE, valid_samples=n_valid)
    assert len(frames) == -(-n_valid // 160)
    assert _frames_of([torch.cat([v for _, v in pieces])[:n_valid]]) == frames
    cut, left = [], n_valid                                           # piece by piece, trimmed to the valid length
    for _, v in pieces:
        cut.append(v[:max(min(left, v.numel()), 0)])
        left -= v.numel()
    assert _frames_of(cut) == frames
    # a pool of the same decode next to another stream, every other tick through the pinned host buffer
    pp = wire.pcm_pool(net, net.stream_pool(), MODEL_SR, RATE, encoding=law)
    other = _text_stream(net, 14, 11)
    alone = wire.stream_pcm16(net, _again(net, other), MODEL_SR, RATE, encoding=law).run()
    fa = pp.add(_again(net, st), peak=peak, limiter=lim)
    fb = pp.add(_again(net, other))
    got, hosts = {id(fa._st): [], id(fb._st): []}, set()
    for step in range(60):
        runs = wire.wire_runs(net)
        out = pp.step(host=step % 2 == 1)
        kinds = {id(m) == id(fa._st) and limited for m, _, v in out if len(v)}
        assert len(kinds) <= wire.wire_runs(net) - runs <= (2 if limited else 1)
        for m, a, v in out:
            if isinstance(v, np.ndarray):
                assert v.dtype == np.uint8
                at = v.__array_interface__["data"][0] - pp._host_np.__array_interface__["data"][0]
                hosts.add(0 <= at <= pp._host_np.size - v.size)
                v = torch.from_numpy(v.copy())
            else:
                assert v.dtype == torch.uint8
            got[id(m)].append((a, v.cpu()))
        if not len(pp):
            break
    assert len(pp) == 0 and hosts == {True}                           # views of ONE pinned uint8 buffer
    assert pp._host.dtype == torch.uint8 and pp._host.is_pinned() and pp._packed.dtype == torch.uint8
    assert torch.equal(fa.pcm, ref) and torch.equal(fa.valid_samples, ref_valid)
    assert torch.equal(fb.pcm, alone[0]) and torch.equal(fb.valid_samples, alone[1])
    for f_, whole in ((fa, ref), (fb, alone[0])):
        host = whole[0].cpu()
        assert sum(v.numel() for _, v in got[id(f_._st)]) == whole.shape[1]
        for a, v in got[id(f_._st)]:
            assert torch.equal(v, host[a:a + v.numel()])
    assert _frames_of([torch.cat([v for _, v in got[id(fa._st)]])[:n_valid]]) == frames


@pytest.mark.parametrize("law", LAWS)
def test_admitted_requests_and_convert_pcm16_take_the_encoding(law):
    net = _net()
    wave = _audio(HOP * 60, 77, MODEL_SR, False).cuda()[None]
    src, tgt = torch.tensor([3]).cuda(), torch.tensor([7]).cuda()
    args = (net, wave, None, src, tgt, MODEL_SR, MODEL_SR, RATE, HOP, WIN)
    plain, valid = wire.convert_pcm16(*args, seed=9, limiter=LIM)
    got, got_valid = wire.convert_pcm16(*args, seed=9, limiter=LIM, encoding=law)
    assert torch.equal(got, _encoded(plain, law)) and torch.equal(got_valid, valid)
    req = ConvertRequest(wave[0].cpu(), 3, 7, MODEL_SR, HOP, WIN, chunk_frames=8, max_chunk_frames=32, seed=9)
    pp = wire.pcm_pool(net, net.stream_pool(), MODEL_SR, RATE, encoding=law)
    f = pp.admit([req], limiter=LIM)[0]
    assert f.encoding == law and f.pcm.dtype == torch.uint8
    while len(pp):
        pp.step()
    ref, ref_valid = wire.service_pcm16(net, f._st.o, f._st.y_lengths, MODEL_SR, RATE, auto_normalize=False,
                                        limiter=LIM, encoding=law)
    assert torch.equal(f.pcm, ref) and torch.equal(f.valid_samples, ref_valid)
    # G.711 in, one shot: the recording is expanded by net.g711_decode and goes on as int16
    pcm8k = _audio(8000, 78, 8000, True)
    data = torch.from_numpy(g711_ref.encode(pcm8k.numpy(), law))[None].cuda()
    lin = torch.from_numpy(g711_ref.decode(data.cpu().numpy(), law)).cuda()
    a = wire.convert_pcm16(net, data, None, src, tgt, 8000, MODEL_SR, RATE, HOP, WIN, seed=5, in_encoding=law)
    b = wire.convert_pcm16(net, lin, None, src, tgt, 8000, MODEL_SR, RATE, HOP, WIN, seed=5)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ------------------------------------------------------------------------------------------------ 6. G.711 in
IN_SR, T_LIVE = 8000, 100


def _recording(law, seed):
    """(bytes uint8, the int16 they decode to), both on the device"""
    pcm = _audio(_raw_len(T_LIVE, 1, IN_SR), seed, IN_SR, True).numpy()
    data = g711_ref.encode(pcm, law)
    return torch.from_numpy(data).cuda(), torch.from_numpy(g711_ref.decode(data, law)).cuda()


def _drive(net, raw, noise, pattern, **kw):
    """-> (the finished wire, [(first, bytes or int16 of every piece)])"""
    lw = _open(net, IN_SR, kw.pop("rate", RATE), raw.dtype, noise, kw.pop("peak", None), 32, (8, 32), **kw)
    pieces, off = [], 0
    for k in _cuts(net, pattern, IN_SR, raw.numel(), T_LIVE, 32, 1):
        lw.push(raw[off:off + k])
        off += k
        runs = net.input_runs()
        pieces += [(a, v.clone()) for a, v in lw.poll()]
        assert net.input_runs() - runs <= 1
    lw.close()
    pieces += [(a, v.clone()) for a, v in lw.poll()]
    assert lw.finished
    return lw, pieces


def _same_wire(a, pa, b, pb):
    assert torch.equal(a.live.samples.view(torch.int32), b.live.samples.view(torch.int32))
    assert torch.equal(a.pcm, b.pcm) and torch.equal(a.valid_samples, b.valid_samples)
    assert torch.equal(a.peak.view(torch.int32), b.peak.view(torch.int32))
    assert len(pa) == len(pb) and all(x == y and torch.equal(v, w) for (x, v), (y, w) in zip(pa, pb))


@pytest.mark.parametrize("law", LAWS)
def test_g711_input_is_the_decoded_int16_input(law):
    net = _net()
    data, lin = _recording(law, 41)
    noise = _noise(net, 141, IN_SR)
    for pattern in ("20ms", "random"):
        want, want_pieces = _drive(net, lin, noise, pattern, rate=MODEL_SR)
        got, got_pieces = _drive(net, data, noise, pattern, rate=MODEL_SR, in_encoding=law)
        assert got.in_encoding == law and got.raw.dtype == torch.uint8
        _same_wire(got, got_pieces, want, want_pieces)
        assert int(got.valid_samples[0]) > 0 and float(got.peak[0]) > 0


def test_two_live_wires_with_different_laws_share_the_input_launch():
    net = _net()
    recs = {law: _recording(law, 50 + k) for k, law in enumerate(LAWS)}
    noise = {law: _noise(net, 150 + k, IN_SR) for k, law in enumerate(LAWS)}
    solo = {law: _drive(net, recs[law][1], noise[law], "20ms") for law in LAWS}          # int16 in, int16 out
    pp = wire.pcm_pool(net, net.stream_pool(), MODEL_SR, RATE)
    lws = {law: pp.add_live(_open(net, IN_SR, RATE, torch.uint8, noise[law], None, 32, (8, 32), in_encoding=law))
           for law in LAWS}
    got = {law: [] for law in LAWS}
    n = recs["ulaw"][0].numel()
    assert recs["alaw"][0].numel() == n
    off, k, shared = 0, IN_SR // 50, 0
    for _ in range(200):
        if not len(pp):
            break
        if off < n:
            for law in LAWS:
                lws[law].push(recs[law][0][off:off + k])
            off += k
        else:
            for law in LAWS:
                if not lws[law].closed:
                    lws[law].close()
        runs = net.input_runs()
        for m, a, v in pp.step():
            got[[law for law in LAWS if lws[law] is m][0]].append((a, v.clone()))
        assert net.input_runs() - runs <= 1                           # both laws in ONE input launch
        shared += net.input_runs() - runs
    assert len(pp) == 0 and shared >= 3
    for law in LAWS:
        _same_wire(lws[law], got[law], *solo[law])


def test_the_telephone_loop_does_not_depend_on_the_pushes():
    """mu-law in at 8 kHz, A-law out at 8 kHz, limiter on."""
    net = _net()
    data, lin = _recording("ulaw", 61)
    noise = _noise(net, 161, IN_SR)
    plain, _ = _drive(net, lin, noise, "one")
    peak = float(plain.peak[0]) * 0.25                                # "chosen too small": the limiter has work to do
    kw = dict(peak=peak, limiter=LIM, in_encoding="ulaw", encoding="alaw")
    a, pa = _drive(net, data, noise, "20ms", **kw)
    b, pb = _drive(net, data, noise, "random", **kw)
    _same_wire(a, pa, b, pb)
    assert a.pcm.dtype == torch.uint8 and pa[0][0] == 0 and sum(v.numel() for _, v in pa) == int(a.valid_samples[0])
    # and it is the A-law of the int16 loop on the decoded recording, unwritten samples included
    c, pc = _drive(net, lin, noise, "one", peak=peak, limiter=LIM)
    assert torch.equal(a.pcm, _encoded(c.pcm, "alaw")) and torch.equal(a.valid_samples, c.valid_samples)
    assert int(c.pcm.abs().max()) <= int(np.floor(float(np.float32(CEILING)) * 32767)) + 1
    valid = int(a.valid_samples[0])
    assert wire.frame_g711(a.pcm[0], RATE, valid_samples=valid) == _frames_of([v for _, v in pa])


# ------------------------------------------------------------------------------------------------ 7. refusals
def _counters(net):
    return wire.wire_runs(net), net.input_runs(), net.converter_runs(), net.decoder_runs()


def test_refusals_launch_nothing_and_the_stream_serves_on():
    net, x, valid = _case(22050, 8000)
    n = x.shape[-1]
    width = wire.resample_ready(22050, 8000, n, n)
    h, L = net._ensure_handle(), _capi.lib()
    want = _run(net, x, valid, 22050, 8000, None, "ulaw")
    out = torch.full((3, width), SENTINEL, device="cuda", dtype=torch.uint8)
    c0 = _counters(net)
    ptr = lambda t: t.data_ptr()
    # an unknown law at the four C entries
    run0, run1 = torch.zeros(1).cuda(), torch.zeros(1).cuda()
    ks = (_capi.MbvPcmChunk * 1)(_chunk(x[0, 0], valid[:1], n, 0, 10, out[0], run0, None, None))
    every = torch.zeros(16, dtype=torch.int16).cuda()
    for law in (0, 3):
        assert L.mbv_resample_g711_range(h, ptr(x), ptr(valid), 3, n, 22050, 8000, 0, n, 0, 10, None, ptr(out), width,
                                         None, None, None, law, None) != 0
        assert b"mbv_resample_g711_range: unknown law" in L.mbv_last_error(h)
        assert L.mbv_resample_g711_chunks(h, ks, None, 1, 22050, 8000, 0, law, None, 0, None) != 0
        assert b"mbv_resample_g711_chunks: unknown law" in L.mbv_last_error(h)
        assert L.mbv_g711_encode(h, ptr(every), 16, law, ptr(out), None) != 0
        assert b"mbv_g711_encode: unknown law" in L.mbv_last_error(h)
        assert L.mbv_g711_decode(h, ptr(out), 16, law, ptr(every), None) != 0
        assert b"mbv_g711_decode: unknown law" in L.mbv_last_error(h)
    # what the int16 entries refuse, through the same code
    ready = wire.resample_ready(22050, 8000, 1000, n)
    with pytest.raises(_capi.MbvError, match="make only %d final" % (ready - 7)):
        net.resample_pcm16_range(x, 22050, 8000, 1000, 0, ready, out, limiter=(0.9, 7, 19), encoding="alaw")
    with pytest.raises(_capi.MbvError, match="ceiling"):
        net.resample_pcm16_range(x, 22050, 8000, n, 0, 10, out, limiter=(1.5, 7, 19), encoding="alaw")
    with pytest.raises(ValueError, match="torch.uint8"):
        net.resample_pcm16_range(x, 22050, 8000, n, 0, 10, out.to(torch.int16), encoding="alaw")
    with pytest.raises(ValueError, match="torch.int16"):
        net.resample_pcm16_range(x, 22050, 8000, n, 0, 10, out)
    with pytest.raises(ValueError, match="uint8"):
        net.resample_pcm16_chunks(ks, 22050, 8000, packed=torch.zeros(64, dtype=torch.int16).cuda(), encoding="ulaw")
    two = [_chunk(x[0, 0], valid[:1], n, 0, 10, out[0], run0, None, None),
           _chunk(x[0, 0], valid[:1], n, 9, 10, out[0], run1, None, None)]                     # [9, 19) meets [0, 10)
    with pytest.raises(_capi.MbvError, match="chunks 0 and 1 write overlapping"):
        net.resample_pcm16_chunks(two, 22050, 8000, encoding="ulaw")
    two[1].out_first = 10                                             # bytes [10, 20): disjoint (int16 rows would be too)
    # wave_dtype 2..7 stay refused with the existing message; 8 and 9 by everything but the live-input resampler
    raw = torch.zeros(4000, dtype=torch.uint8).cuda()
    model_row = torch.zeros(1000).cuda()
    rr = (_capi.MbvResampleRange * 1)()
    rr[0].wave, rr[0].in_avail, rr[0].in_total, rr[0].out_first, rr[0].out_count = ptr(raw), 2000, -1, 0, 10
    rr[0].out, rr[0].out_capacity = ptr(model_row), 1000
    for dt in range(2, 8):
        rr[0].wave_dtype = dt
        assert L.mbv_resample_ranges(h, rr, 1, 8000, MODEL_SR, 0, None) != 0
        assert b"row 0: unknown wave_dtype %d" % dt in L.mbv_last_error(h)
    I = net.cfg.inter_channels
    w = torch.zeros(HOP * 300).cuda()
    z, noise, g1 = torch.zeros(1, I, 300).cuda(), torch.zeros(1, I, 300).cuda(), torch.zeros(1, net.cfg.gin_channels).cuda()
    spec = torch.zeros(1, 513, 300).cuda()
    frames = int(L.mbv_spectrogram_frames(HOP * 300, 1024, HOP))
    for dt in (_capi.WAVE_ULAW, _capi.WAVE_ALAW):
        assert L.mbv_spectrogram(h, ptr(w), dt, None, 1, HOP * 300, 1024, HOP, WIN, ptr(spec), frames, None, None) != 0
        assert b"mbv_spectrogram: unknown wave_dtype %d" % dt in L.mbv_last_error(h)
        row = (_capi.MbvConvertRow * 1)()
        row[0].wave, row[0].samples, row[0].wave_dtype, row[0].sid_src, row[0].sid_tgt = ptr(w), HOP * 300, dt, 0, 1
        row[0].noise, row[0].noise_scale, row[0].z = ptr(noise), 1.0, ptr(z)
        assert L.mbv_convert_rows(h, row, 1, 300, HOP, WIN, ptr(g1), None) != 0
        assert b"row 0: unknown wave_dtype %d" % dt in L.mbv_last_error(h)
        rng = (_capi.MbvConvertRange * 1)()
        rng[0].wave, rng[0].arrived, rng[0].closed, rng[0].wave_dtype = ptr(w), HOP * 250, 0, dt
        rng[0].sid_src, rng[0].sid_tgt, rng[0].first, rng[0].count = 0, 1, 0, 32
        rng[0].noise, rng[0].noise_stride, rng[0].noise_scale = ptr(noise), 300, 1.0
        rng[0].z, rng[0].z_stride = ptr(z), 300
        assert L.mbv_convert_ranges(h, rng, 1, HOP, WIN, None) != 0
        assert b"row 0: unknown wave_dtype %d" % dt in L.mbv_last_error(h)
    assert int(torch.count_nonzero(spec)) == 0 and int(torch.count_nonzero(z)) == 0
    # the Python entries
    st = _text_stream(net, 12, 3)
    with pytest.raises(ValueError, match="encoding"):
        wire.stream_pcm16(net, st, MODEL_SR, RATE, encoding="g722")
    live_noise = _noise(net, 170, IN_SR)
    with pytest.raises(ValueError, match="in_sr != model_sr"):
        wire.convert_live_pcm16(net, 3, 7, MODEL_SR, MODEL_SR, RATE, HOP, WIN, 8000, dtype=torch.uint8, in_encoding="ulaw")
    with pytest.raises(TypeError, match="in_encoding"):
        _open(net, IN_SR, RATE, torch.uint8, live_noise)
    pp = wire.pcm_pool(net, net.stream_pool(), MODEL_SR, RATE, encoding="ulaw")
    with pytest.raises(ValueError, match="encoding 'alaw', the pool with 'ulaw'"):
        pp.add_live(_open(net, IN_SR, RATE, torch.uint8, live_noise, in_encoding="ulaw", encoding="alaw"))
    with pytest.raises(ValueError, match="encoding 'pcm16', the pool with 'ulaw'"):
        pp.add_live(_open(net, IN_SR, RATE, torch.int16, live_noise))
    lw = _open(net, IN_SR, RATE, torch.uint8, live_noise, in_encoding="ulaw", encoding="ulaw")
    with pytest.raises(TypeError, match="uint8"):
        lw.push(torch.zeros(10, dtype=torch.int16).cuda())
    assert pp.add_live(lw) is lw and len(pp) == 1
    # nothing was launched or written, and the next valid calls are bitwise as if nothing had been refused
    assert _counters(net) == c0 and (out == SENTINEL).all() and int(torch.count_nonzero(model_row)) == 0
    assert st._next == 0
    assert _same(_run(net, x, valid, 22050, 8000, None, "ulaw"), want)
    net.resample_pcm16_chunks(two, 22050, 8000, encoding="ulaw")
    assert torch.equal(out[0, :20], want[0][0, :20]) and (out[0, 20:] == SENTINEL).all()
    rr[0].wave_dtype = _capi.WAVE_ULAW                                 # bytes 0x00: -32124 / 32768 everywhere
    assert L.mbv_resample_ranges(h, rr, 1, 8000, MODEL_SR, 0, None) == 0
    lin = torch.full((4000,), -32124, dtype=torch.int16).cuda()
    rr[0].wave, rr[0].wave_dtype, rr[0].out = ptr(lin), _capi.WAVE_PCM16, ptr(spec)
    assert L.mbv_resample_ranges(h, rr, 1, 8000, MODEL_SR, 0, None) == 0
    assert torch.equal(model_row[:10].view(torch.int32), spec.flatten()[:10].view(torch.int32))
    assert float(model_row[:10].abs().max()) > 0 and net.input_runs() == c0[1] + 2
