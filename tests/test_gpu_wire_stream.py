"""-m gpu: the streamed wire output (`mbv_resample_pcm16_range`, `wire.stream_pcm16`, `wire.FrameCutter`) against
the one-shot chain of the same process (`resample` -> `to_pcm16` / `wire.service_pcm16` -> `wire.frame_pcm16`).
Every comparison is bitwise."""
import ctypes as C

import pytest
import torch

from mb_istft_vits_amd import _capi, synth, wire

from gpu_util import make_net, ptr

pytestmark = pytest.mark.gpu

PAIRS = [(22050, 24000), (22050, 16000), (16000, 24000), (24000, 22050), (22050, 44100), (16000, 8000)]
_NETS = {}
SENTINEL = -12345


def _net(name="ljs_mini_mb_istft_vits"):
    if name not in _NETS:
        _NETS[name] = make_net(name)[0]
    return _NETS[name]


def _lag(orig, target, res_type):
    """input samples the stream holds back: K - left - 1 of the bank geometry"""
    taps, left = C.c_int32(), C.c_int32()
    assert _capi.lib().mbv_resample_bank(orig, target, {"kaiser_best": 0, "kaiser_fast": 1}[res_type], None, 0, None,
                                         C.byref(taps), C.byref(left)) == 0
    return taps.value - left.value - 1


def _ragged(n, seed):
    """B = 3: a full row, a row shorter than any filter half-width, an empty row; |x| up to 1.5 so that the
    unnormalised conversion clips"""
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(3, 1, n, generator=g) * 3 - 1.5).cuda()
    return x, torch.tensor([n, 13, 0], device="cuda", dtype=torch.int64)


def _one_shot(net, x, valid, orig, target, res_type):
    out, ns = net.resample(x, orig, target, valid_samples=valid, res_type=res_type)
    peaks = torch.stack([out[b, 0, :int(ns[b])].abs().max() if int(ns[b]) else out.new_zeros(())
                         for b in range(x.shape[0])])
    return out, ns, peaks


def _frontiers(n, lag):
    """not multiples of 256; steps of 1 and 7 samples around the lag; the first two make nothing ready"""
    f = [1, 7, lag - 1, lag, lag + 1, lag + 2, lag + 9, lag + 16, lag + 17, 301, 777, 778, 1500, n - 1, n]
    return sorted(set(v for v in f if 0 < v <= n))


def _feed(net, x, valid, orig, target, res_type, frontiers, peak, poison=None):
    """drive the raw step over `frontiers`; -> (pcm, running peak, out_samples, counts per step)"""
    B, n = x.shape[0], x.shape[-1]
    width = wire.resample_ready(orig, target, n, n, res_type)
    pcm = torch.full((B, width), SENTINEL, device="cuda", dtype=torch.int16)
    running = torch.zeros(B, device="cuda")
    ns = torch.full((B,), -1, device="cuda", dtype=torch.int64)
    done, counts = 0, []
    for i, f in enumerate(frontiers):
        xx = x
        if poison is not None:
            xx = x.clone()
            xx[:, :, f:] = poison
        r = wire.resample_ready(orig, target, f, n, res_type)
        net.resample_pcm16_range(xx, orig, target, f, done, r - done, pcm, valid_samples=valid, peak=peak,
                                 running_peak=running, out_samples=ns if i == 0 else None, res_type=res_type)
        assert (pcm[:, r:] == SENTINEL).all()                         # nothing past the range is written
        counts.append(r - done)
        done = r
    assert done == width
    return pcm, running, ns, counts


@pytest.mark.parametrize("res_type", ["kaiser_best", "kaiser_fast"])
@pytest.mark.parametrize("orig,target", PAIRS)
def test_raw_step_bitwise(orig, target, res_type):
    net = _net()
    n = 3001
    x, valid = _ragged(n, orig + target)
    out, ns, peaks = _one_shot(net, x, valid, orig, target, res_type)
    fr = _frontiers(n, _lag(orig, target, res_type))
    for auto in (False, True):
        ref = net.to_pcm16(out, auto_normalize=auto, valid_samples=ns)
        pcm, running, got_ns, counts = _feed(net, x, valid, orig, target, res_type, fr, peaks if auto else None)
        assert 0 in counts[:2] and min(counts) >= 0                   # a step that made nothing ready
        assert torch.equal(pcm, ref), (auto, int((pcm != ref).sum()))
        assert torch.equal(got_ns, ns)
        assert torch.equal(running.view(torch.int32), peaks.view(torch.int32))
    assert float(peaks[0]) > 0.01 and float(peaks[2]) == 0.0            # row 0 is normalised, the empty row is not
    # one step for everything, and every row on its own
    pcm, running, got_ns, _ = _feed(net, x, valid, orig, target, res_type, [n], None)
    assert torch.equal(pcm, net.to_pcm16(out, auto_normalize=False, valid_samples=ns))
    assert torch.equal(running.view(torch.int32), peaks.view(torch.int32))


def test_raw_step_equal_rates_and_small_peak():
    net = _net()
    n = 1000
    x, valid = _ragged(n, 5)
    x[1] *= 0.005                                                     # peak below the 0.01 threshold: not normalised
    peaks = torch.stack([x[b, 0, :int(valid[b])].abs().max() if int(valid[b]) else x.new_zeros(()) for b in range(3)])
    for auto in (False, True):
        ref = net.to_pcm16(x, auto_normalize=auto, valid_samples=valid)
        pcm, running, ns, counts = _feed(net, x, valid, 22050, 22050, "kaiser_best", [1, 7, 300, 999, 1000],
                                         peaks if auto else None, poison=float("nan"))
        assert counts == [1, 6, 293, 699, 1]                          # no lag
        assert torch.equal(pcm, ref)
        assert torch.equal(ns, valid)
        assert torch.equal(running.view(torch.int32), peaks.view(torch.int32))
    # a peak below the true one: the clip bounds it, as the reference's own clip does
    small = peaks * 0.5
    pcm, *_ = _feed(net, x, valid, 22050, 22050, "kaiser_best", [1000], small)
    v = torch.clamp(x[0, 0] / small[0] * 0.9, -1, 1) * 32767
    assert torch.equal(pcm[0], v.to(torch.int32).to(torch.int16))


@pytest.mark.parametrize("res_type", ["kaiser_best", "kaiser_fast"])
@pytest.mark.parametrize("orig,target", PAIRS)
def test_never_reads_ahead(orig, target, res_type):
    """Input at and past in_avail is NaN, then 1e30, before every step: results unchanged."""
    net = _net()
    n = 3001
    x, valid = _ragged(n, orig + 3 * target)
    valid = torch.tensor([n, n - 500, 13], device="cuda", dtype=torch.int64)
    out, ns, peaks = _one_shot(net, x, valid, orig, target, res_type)
    ref = net.to_pcm16(out, auto_normalize=True, valid_samples=ns)
    fr = _frontiers(n, _lag(orig, target, res_type))
    for poison in (float("nan"), 1e30):
        pcm, running, got_ns, _ = _feed(net, x, valid, orig, target, res_type, fr, peaks, poison=poison)
        assert torch.equal(pcm, ref), poison
        assert torch.equal(running.view(torch.int32), peaks.view(torch.int32))
        assert torch.equal(got_ns, ns)


def _text(net, B, seed):
    x, xl, sid = synth.synthetic_batch(net.cfg, B, 30, seed=seed, ragged=B > 1)
    sid = torch.from_numpy(sid).cuda() if sid is not None else None
    return torch.from_numpy(x).cuda(), torch.from_numpy(xl).cuda(), sid


def _infer_stream(net, x, xl, sid, chunk, seed=5, **kw):
    torch.manual_seed(seed)
    torch.cuda.manual_seed(seed)
    return net.infer_stream(x, xl, sid=sid, noise_scale=0.667, chunk_frames=chunk, max_chunk_frames=64, **kw)


def _drain(ws, rate):
    """iterate a PcmStream as a service would: pieces to the host, one FrameCutter per row; -> frames per row"""
    B = ws.pcm.shape[0]
    cutters = [wire.FrameCutter(rate) for _ in range(B)]
    frames = [[] for _ in range(B)]
    pieces, nxt = [], 0
    for a, v in ws:
        assert a == nxt and v.dtype == torch.int16
        nxt = a + v.shape[1]
        pieces.append(v.cpu())
    assert nxt == ws.pcm.shape[1]
    valid = ws.valid_samples.cpu()
    for b in range(B):
        off = 0
        for p in pieces:                                              # a row's stream ends at its valid length
            take = max(0, min(p.shape[1], int(valid[b]) - off))
            frames[b] += cutters[b].push(p[b, :take])
            off += p.shape[1]
        frames[b] += cutters[b].close()
    return torch.cat(pieces, dim=1), frames


def _check_end_to_end(net, model_sr, rate, B, chunk, res_type="kaiser_best"):
    x, xl, sid = _text(net, B, 11 + B)
    st = _infer_stream(net, x, xl, sid, chunk)
    ws = wire.stream_pcm16(net, st, model_sr, rate, peak=None, res_type=res_type)
    assert len(ws) == len(st)
    cat, frames = _drain(ws, rate)
    o, yl = st.o, st.y_lengths
    for auto in (False, True):
        ref, valid = wire.service_pcm16(net, o, yl, model_sr, rate, auto_normalize=auto, res_type=res_type)
        if auto:
            # the stream's own running peak of the first pass is the true peak: feed it to a second pass
            st2 = _infer_stream(net, x, xl, sid, chunk)
            ws2 = wire.stream_pcm16(net, st2, model_sr, rate, peak=ws.peak.clone(), res_type=res_type)
            cat, frames = _drain(ws2, rate)
            assert torch.equal(st2.o, o)
            assert torch.equal(ws2.peak.view(torch.int32), ws.peak.view(torch.int32))
            assert torch.equal(ws2.pcm, ref)
        else:
            assert torch.equal(ws.pcm, ref)
            wave, ns = net.resample(o, model_sr, rate, y_lengths=yl, res_type=res_type)
            peaks = torch.stack([wave[b, 0, :int(ns[b])].abs().max() for b in range(B)])
            assert torch.equal(ws.peak.view(torch.int32), peaks.view(torch.int32))
        assert torch.equal(cat, ref.cpu())
        assert torch.equal(ws.valid_samples, valid)
        for b in range(B):
            assert frames[b] == wire.frame_pcm16(ref[b], rate, valid_samples=int(valid[b])), (auto, b)


@pytest.mark.parametrize("chunk", [8, 32])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("name,model_sr,rate", [
    ("ljs_mini_mb_istft_vits", 22050, 24000), ("ljs_mini_mb_istft_vits", 22050, 16000),
    ("uudb_ms_istft_vits_ms", 16000, 24000), ("uudb_ms_istft_vits_ms", 16000, 16000)])
def test_end_to_end_bitwise(name, model_sr, rate, B, chunk):
    _check_end_to_end(_net(name), model_sr, rate, B, chunk)


def test_end_to_end_splitk_and_kaiser_fast():
    net = _net("ljs_mini_mb_istft_vits")
    net.set_option("splitk", 1)
    try:
        _check_end_to_end(net, 22050, 24000, 3, 8)
        _check_end_to_end(net, 22050, 22050, 1, 32)
    finally:
        net.set_option("splitk", 0)
    _check_end_to_end(net, 22050, 24000, 1, 8, res_type="kaiser_fast")


def test_side_stream_and_interleaved_streams():
    net = _net("ljs_mini_mb_istft_vits")
    xa, xla, _ = _text(net, 3, 21)
    xb, xlb, _ = _text(net, 1, 22)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        st = _infer_stream(net, xa, xla, None, 8)
        ws = wire.stream_pcm16(net, st, 22050, 24000, peak=0.5)
        pcm, valid = ws.run()
        ref, rv = wire.service_pcm16(net, st.o, st.y_lengths, 22050, 24000, auto_normalize=False)
        wave, ns = net.resample(st.o, 22050, 24000, y_lengths=st.y_lengths)
    side.synchronize()
    assert torch.equal(valid, rv)
    peaks = torch.stack([wave[b, 0, :int(ns[b])].abs().max() for b in range(3)])
    assert torch.equal(ws.peak.view(torch.int32), peaks.view(torch.int32))
    # a float peak: the pcm16 epilogue with that constant for every row
    v = torch.clamp(wave[:, 0] / 0.5 * 0.9, -1, 1) * 32767
    mask = torch.arange(v.shape[1], device="cuda")[None, :] < ns[:, None]
    assert torch.equal(pcm, torch.where(mask, v, torch.zeros_like(v)).to(torch.int32).to(torch.int16))
    # two wire streams on one model advanced alternately, other calls in between
    refs = {}
    for key, (x, xl) in (("a", (xa, xla)), ("b", (xb, xlb))):
        s0 = _infer_stream(net, x, xl, None, 8, seed=7)
        s0.run()
        refs[key] = (wire.service_pcm16(net, s0.o, s0.y_lengths, 22050, 24000, auto_normalize=False),
                     wire.stream_pcm16(net, _infer_stream(net, x, xl, None, 8, seed=7), 22050, 24000))
        refs[key][1].run()
    sa = wire.stream_pcm16(net, _infer_stream(net, xa, xla, None, 8, seed=7), 22050, 24000)
    sb = wire.stream_pcm16(net, _infer_stream(net, xb, xlb, None, 8, seed=7), 22050, 24000)
    ia, ib = iter(sa), iter(sb)
    live = [ia, ib]
    while live:
        for it in list(live):
            if next(it, None) is None:
                live.remove(it)
        net.infer(xb, xlb, noise_scale=0)
    for key, s in (("a", sa), ("b", sb)):
        (ref, rv), solo = refs[key]
        assert torch.equal(s.pcm, ref) and torch.equal(s.valid_samples, rv)
        assert torch.equal(s.peak.view(torch.int32), solo.peak.view(torch.int32))
    with pytest.raises(ValueError):
        wire.stream_pcm16(net, sa._st, 22050, 24000)                  # a decode stream that has already run


def test_errors_launch_nothing_and_leave_the_handle_usable():
    net = _net()
    L, h, s = _capi.lib(), net._ensure_handle(), net._stream()
    n = 2000
    x, valid = _ragged(n, 1)
    width = wire.resample_ready(22050, 24000, n, n)
    pcm = torch.full((3, width), SENTINEL, device="cuda", dtype=torch.int16)
    running = torch.zeros(3, device="cuda")
    ns = torch.full((3,), -1, device="cuda", dtype=torch.int64)
    r = wire.resample_ready(22050, 24000, 1000, n)

    def call(orig=22050, target=24000, filt=0, in_avail=1000, first=0, count=r, wave=x, out=pcm, B=3, stride=width):
        return L.mbv_resample_pcm16_range(h, ptr(wave), ptr(valid), B, n, orig, target, filt, in_avail, first, count,
                                          None, ptr(out), stride, ptr(running), ptr(ns), s)
    bad = [dict(count=r + 1),                       # one output beyond what 1000 input samples make final
           dict(first=r, count=1),
           dict(in_avail=n, first=width + 1, count=0),          # out_first past out_stride
           dict(in_avail=n, first=width - 1, count=2),
           dict(filt=2),                            # unknown filter
           dict(target=24001),                      # refused pair: 24001 phases
           dict(orig=0),
           dict(first=-1), dict(count=-1), dict(in_avail=-1), dict(B=0), dict(stride=0),
           dict(wave=None), dict(out=None)]
    for kw in bad:
        assert call(**kw) != 0, kw
        assert L.mbv_last_error(h), kw
    assert b"4096" in (call(target=24001) and L.mbv_last_error(h))
    torch.cuda.synchronize()
    assert (pcm == SENTINEL).all() and not running.any() and (ns == -1).all()      # errors wrote nothing
    with pytest.raises(_capi.MbvError, match="final"):
        net.resample_pcm16_range(x, 22050, 24000, 1000, 0, r + 1, pcm, valid_samples=valid)
    with pytest.raises(ValueError):
        net.resample_pcm16_range(x, 22050, 24000, n, 0, width + 1, pcm, valid_samples=valid)
    with pytest.raises(ValueError):
        net.resample_pcm16_range(x, 22050, 24000, n, 0, width, pcm, valid_samples=valid, res_type="soxr_hq")
    with pytest.raises(ValueError):
        net.resample_pcm16_range(x, 22050, 24000, n, 0, width, pcm.float(), valid_samples=valid)
    # the next valid calls on the same handle succeed
    assert call() == 0 and call(in_avail=n, first=r, count=width - r) == 0
    out, ons, _ = _one_shot(net, x, valid, 22050, 24000, "kaiser_best")
    assert torch.equal(pcm, net.to_pcm16(out, auto_normalize=False, valid_samples=ons))
    assert torch.equal(ns, ons)
