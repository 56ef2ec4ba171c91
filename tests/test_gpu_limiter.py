"""-m gpu: the look-ahead limiter of the wire step (`mbv_resample_pcm16_range_limited`,
`mbv_resample_pcm16_chunks_limited`, `wire.Limiter`).  There is no reference implementation to compare with, so
the kernel is pinned to the float64 restatement of its definition (tests/limiter_ref.py) within one int16 step, and
every relation between the one-shot, chunked, pooled and live forms is bitwise."""
import numpy as np
import pytest
import torch

from mb_istft_vits_amd import _capi, wire
from mb_istft_vits_amd.models import ConvertRequest

import limiter_ref
from gpu_util import make_net
# the live-wire helpers: recordings, noise blocks, push patterns
from test_gpu_live_wire import HOP, MODEL_SR, WIN, _audio, _cuts, _noise, _open, _raw_len, _text_batch

pytestmark = pytest.mark.gpu

CEILING = 0.9
C32 = float(np.float32(CEILING))                     # the kernel's ceiling is an fp32
PAIRS = [(22050, 24000), (48000, 16000), (22050, 22050)]     # the extra bank row; downsampling; FIR = false
SETTINGS = [(7, 19), (0, 0), None]                   # (L, H); None: Limiter()'s defaults at the target rate
N_IN = 3001
SENTINEL = -12345
_NETS = {}


def _net(name="uudb_ms_istft_vits_ms"):
    if name not in _NETS:
        _NETS[name] = make_net(name)[0]
    return _NETS[name]


def _setting(setting, target):
    c, L, H = wire.Limiter(CEILING).resolve(target)
    return (CEILING,) + (tuple(setting) if setting else (L, H))


def _n_out(n, orig, target):
    """the row's computed outputs: resampy's int(n * ratio); the samples themselves at equal rates"""
    return n if orig == target else int(n * (float(target) / orig))


def burst_outputs(n_out):
    """where the loud rows go above the ceiling, in output samples: the first outputs, across the first tile
    boundary, two pairs closer together than the hold (10 apart for H = 19, 150 apart for the defaults' H >= 320), the
    row's last computed outputs"""
    return [p for p in (0, 254, 600, 610, 760, 910) if p < n_out - 16] + [n_out - 3]


def signal(orig, target, seed=0):
    """x fp32 [3, 1, N_IN], valid [3]: two loud rows of different valid lengths and one that stays below the ceiling"""
    rs = np.random.RandomState(1000 + seed + orig % 97 + target % 89)
    x = rs.uniform(-0.25, 0.25, size=(3, N_IN)).astype(np.float32)
    valid = [N_IN, N_IN - 640, N_IN - 300]
    width = max(5, int(np.ceil(4.0 * orig / target)))
    for b in (0, 1):
        for k, p in enumerate(burst_outputs(_n_out(valid[b], orig, target))):
            i = int(round(p * float(orig) / target))
            i = max(0, min(i, valid[b] - width))
            x[b, i:i + width] = (2.5 if k % 2 == 0 else -2.0) * (1.0 + 0.1 * b)
    return torch.from_numpy(x[:, None, :]), torch.tensor(valid, dtype=torch.int64)


def _resampled(net, x, valid, orig, target):
    """v fp32 numpy [B, n'] from the one-shot resampler (the ranged FIR is bitwise that kernel: test_gpu_wire_stream)
    and the row lengths"""
    out, ns = net.resample(x, orig, target, valid_samples=valid)
    v = out[:, 0].cpu().numpy().copy()
    for row, n in zip(v, valid.tolist()):
        row[_n_out(n, orig, target):] = 0          # (equal rates hand the input back, padding and all)
    return v, ns


def _gained(v, peak):
    """the static gain of the wire epilogue in fp32, in its order: (v / peak) * 0.9 where peak > 0.01"""
    if peak is None:
        return v
    out = v.copy()
    for b, p in enumerate(peak.cpu().numpy().astype(np.float32)):
        if p > np.float32(0.01):
            out[b] = (v[b] / p) * np.float32(0.9)
    return out


def _run(net, x, valid, orig, target, lim, cuts=None, peak=None, frontiers=None, poison=None):
    """the ranged entry over the whole row: in one call, cut at `cuts` (output samples, the input complete), or fed
    along `frontiers` (input samples; the range of every step ends at limiter_ready, or resample_ready without a
    limiter).  -> (pcm, running, out_samples)"""
    B, n = x.shape[0], x.shape[-1]
    width = wire.resample_ready(orig, target, n, n)
    pcm = torch.full((B, width), SENTINEL, device="cuda", dtype=torch.int16)
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
        net.resample_pcm16_range(xx, orig, target, f, done, end - done, pcm, valid_samples=valid, peak=peak,
                                 running_peak=running, out_samples=ns if i == 0 else None, limiter=lim)
        assert (pcm[:, end:] == SENTINEL).all()                       # nothing past the range is written
        done = end
    assert done == width
    return pcm, running, ns


def _same(got, want):
    """bitwise, floats by their bits"""
    return all(torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                           b.view(torch.int32) if b.dtype == torch.float32 else b) for a, b in zip(got, want))


def _case(orig, target):
    net = _net()
    x, valid = signal(orig, target)
    return net, x.cuda(), valid.cuda()


@pytest.mark.parametrize("setting", SETTINGS)
@pytest.mark.parametrize("orig,target", PAIRS)
def test_ranged_entry_against_the_float64_definition(orig, target, setting):
    net, x, valid = _case(orig, target)
    lim = _setting(setting, target)
    v, ns_ref = _resampled(net, x, valid, orig, target)
    plain, plain_running, _ = _run(net, x, valid, orig, target, None)
    n_out = [_n_out(int(n), orig, target) for n in valid]
    # the inputs are what the issue asks for: above the ceiling at the first outputs, the last computed ones, across
    # the tile boundary, twice within one hold; and one row that stays below
    for b in (0, 1):
        loud = np.flatnonzero(np.abs(v[b]) > C32)
        assert loud.min() <= 3 and loud.max() >= n_out[b] - 4 and loud.max() < n_out[b]
        assert np.abs(v[b, 255]) > C32 and np.abs(v[b, 256]) > C32
        assert len(burst_outputs(n_out[b])) >= 6
        for p in burst_outputs(n_out[b])[2:-1]:
            assert (np.abs(v[b, p - 2:p + 6]) > C32).any(), (b, p)
    assert np.abs(v[2]).max() < C32
    true_peak = torch.from_numpy(np.abs(v).max(axis=1)).cuda()
    assert torch.equal(plain_running.view(torch.int32), true_peak.view(torch.int32))
    top = int(np.floor(C32 * 32767)) + 1
    for peak in (None, true_peak * 0.25):                 # a peak "chosen too small": everything is four times louder
        pcm, running, ns = _run(net, x, valid, orig, target, lim, peak=peak)
        vv = _gained(v, peak)
        ref = np.stack([limiter_ref.pcm16(vv[b], C32, lim[1], lim[2]) for b in range(3)])
        got = pcm.cpu().numpy()
        diff = np.abs(got.astype(np.int64) - ref.astype(np.int64))
        # derived, not measured: g is an ordered sum of at most 256 fp32 terms, off by at most 255 * 2^-24 relative,
        # under half an int16 step at the ceiling, so the truncation differs by at most one step
        print("limiter %d -> %d, (L, H) = %s, peak %s: max |int16 - float64 reference| = %d, max |int16| = %d (bound %d)"
              % (orig, target, lim[1:], "given" if peak is not None else "none", diff.max(), np.abs(got).max(), top))
        assert diff.max() <= 1
        assert np.abs(got.astype(np.int64)).max() <= top
        assert torch.equal(ns, ns_ref)
        assert torch.equal(running.view(torch.int32), true_peak.view(torch.int32))    # before any gain, as ever
        g = limiter_ref.gain(vv[0], C32, lim[1], lim[2])[0]
        assert g.min() < 0.5                                  # the limiter worked
        for b in range(3):
            assert (got[b, n_out[b]:] == 0).all()
        if peak is None:
            assert torch.equal(pcm[2], plain[2])              # the quiet row: bitwise the unlimited kernel
            assert not torch.equal(pcm[0], plain[0])
            quiet = g == 1.0                                  # and so is every sample the gain leaves alone
            assert quiet.sum() > 100 or lim[1] + lim[2] > 100     # (the defaults reach every sample of a short row)
            assert np.array_equal(got[0][quiet], plain[0].cpu().numpy()[quiet])


@pytest.mark.parametrize("setting", SETTINGS)
@pytest.mark.parametrize("orig,target", PAIRS)
def test_chunk_invariance_is_bitwise(orig, target, setting):
    net, x, valid = _case(orig, target)
    lim = _setting(setting, target)
    L = lim[1]
    n = x.shape[-1]
    width = wire.resample_ready(orig, target, n, n)
    peak = torch.tensor([0.4, 0.0, 1.7], device="cuda")   # row 1: below the 0.01 threshold, not normalised
    want = _run(net, x, valid, orig, target, lim, peak=peak)
    # single outputs, an empty range (cuts are a set: the empty one is the explicit call below), ranges shorter than
    # L, the tile boundary on both sides, tiles that start off the 256 grid, the last outputs one by one
    cuts = [1, 2, 3, 4, 4 + max(L - 1, 1), 255, 256, 257, 258, 300, 511, 513, 600 + L // 2, 601 + L // 2, 900,
            width - 2, width - 1]
    got = _run(net, x, valid, orig, target, lim, cuts=cuts, peak=peak)
    assert _same(got, want)
    # an empty range writes nothing but the lengths
    pcm = torch.full_like(want[0], SENTINEL)
    ns = torch.full((3,), -1, device="cuda", dtype=torch.int64)
    net.resample_pcm16_range(x, orig, target, n, 257, 0, pcm, valid_samples=valid, peak=peak, out_samples=ns, limiter=lim)
    assert (pcm == SENTINEL).all() and torch.equal(ns, want[2])
    # the stream as it runs: the input arrives, nothing at or past the frontier is read, the range ends L outputs
    # below what the resampler has made final, the last step flushes
    frontiers = sorted([1, 64, 65, 66 + L, 130, 301, 777, 778, 1500, 2000, n - 1, n])
    for poison in (float("nan"), 1e30):
        got = _run(net, x, valid, orig, target, lim, peak=peak, frontiers=frontiers, poison=poison)
        assert _same(got, want), poison
    assert wire.limiter_ready(orig, target, 1500, n, L) == max(wire.resample_ready(orig, target, 1500, n) - L, 0)


# ------------------------------------------------------------------------------------------------ the pooled entry
def _chunk(x, valid, in_avail, first, count, pcm, running, ns, peak):
    k = _capi.MbvPcmChunk()
    k.wave, k.in_total = x.data_ptr(), x.numel()
    k.valid_samples = valid.data_ptr()
    k.in_avail, k.out_first, k.out_count = in_avail, first, count
    k.peak = peak.data_ptr() if peak is not None else None
    k.pcm, k.pcm_capacity = pcm.data_ptr(), pcm.numel()
    k.running_peak = running.data_ptr()
    k.out_samples = ns.data_ptr() if ns is not None else None
    return k


@pytest.mark.parametrize("orig,target", PAIRS)
def test_pooled_rows_are_bitwise_their_ranged_calls_and_a_mixed_call_costs_two_launches(orig, target):
    net, x, valid = _case(orig, target)
    n = x.shape[-1]
    width = wire.resample_ready(orig, target, n, n)
    limits = [(CEILING, 7, 19), None, _setting(None, target), (0.5, 255, 1024), None, (1.0, 0, 3)]
    rows = [(k % 3, limits[k]) for k in range(6)]
    peak = torch.tensor([0.5], device="cuda")
    frontiers = [700, 1500, n]
    want, state = [], []
    for b, lim in rows:
        xb, vb = x[b:b + 1], valid[b:b + 1]
        want.append(_run(net, xb, vb, orig, target, lim, peak=peak, frontiers=frontiers))
        state.append((xb[0, 0].contiguous(), vb.clone(), torch.full((width,), SENTINEL, device="cuda", dtype=torch.int16),
                      torch.zeros(1, device="cuda"), torch.full((1,), -1, device="cuda", dtype=torch.int64), [0]))
    for step, f in enumerate(frontiers):
        # steps 0 and 2: all rows in one call (two launches); step 1: the kinds in a call each (one launch each)
        for kinds in ((None,), (False, True), (None,))[step]:
            chunks, lims, ends = [], [], []
            for (b, lim), (xb, vb, pcm, running, ns, done) in zip(rows, state):
                if kinds is not None and (lim is not None) != kinds:
                    continue
                end = wire.limiter_ready(orig, target, f, n, lim[1] if lim else 0)
                chunks.append(_chunk(xb, vb, f, done[0], end - done[0], pcm, running, ns if step == 0 else None, peak))
                lims.append(lim)
                ends.append((pcm, done, end))
            total = sum(k.out_count for k in chunks)
            packed = torch.full((total + 8,), SENTINEL, device="cuda", dtype=torch.int16)
            runs = wire.wire_runs(net)
            net.resample_pcm16_chunks(chunks, orig, target, packed=packed, limits=lims)
            assert wire.wire_runs(net) - runs == (2 if kinds is None else 1), (step, kinds)
            off = 0
            for k, (pcm, done, end) in zip(chunks, ends):
                assert torch.equal(packed[off:off + k.out_count], pcm[done[0]:end])     # (empty at step 0 for L = 255)
                assert (pcm[end:] == SENTINEL).all()
                off += k.out_count
                done[0] = end
            assert (packed[total:] == SENTINEL).all()
    for (pcm_w, run_w, ns_w), (_, _, pcm, running, ns, done) in zip(want, state):
        assert done[0] == width
        assert torch.equal(pcm, pcm_w[0]) and torch.equal(ns, ns_w)
        assert torch.equal(running.view(torch.int32), run_w.view(torch.int32))


# ------------------------------------------------------------------------------------------------ the followers
RATE = 24000
LIM = wire.Limiter()                                     # 0.9, 5 ms, 20 ms
LIM2 = wire.Limiter(ceiling=0.8, lookahead_ms=1.0, hold_ms=3.0)


def _text_stream(net, T, seed, chunk=8, cap=32):
    x, xl, sid = _text_batch(net, 1, T, seed)
    torch.manual_seed(seed)
    torch.cuda.manual_seed(seed)
    return net.infer_stream(x, xl, sid, noise_scale=0.5, chunk_frames=chunk, max_chunk_frames=cap)


def _again(net, st, chunk=8, cap=32):
    """the same decode once more (its z and g), as a fresh stream"""
    return net.dec_stream(st.z.clone(), st.g, chunk, cap)


def _small_peak(net, st):
    """a quarter of the utterance's true peak: the "chosen too small" of stream_pcm16's docstring"""
    f = wire.stream_pcm16(net, _again(net, st), MODEL_SR, RATE)
    f.run()
    return f.peak.clone() * 0.25


def test_stream_is_bitwise_the_one_shot_service_and_never_clips():
    net = _net()
    st = _text_stream(net, 20, 4)
    peak = _small_peak(net, st)
    clipped = wire.stream_pcm16(net, _again(net, st), MODEL_SR, RATE, peak=peak).run()[0]
    assert int((clipped.abs() >= 32767).sum()) > 0                    # without the limiter this peak hard-clips
    f = wire.stream_pcm16(net, st, MODEL_SR, RATE, peak=peak, limiter=LIM)
    pieces = [(a, v.shape[1]) for a, v in f]
    assert len(pieces) >= 3 and pieces[0][0] == 0 and all(a + n == b for (a, n), (b, _) in zip(pieces, pieces[1:]))
    assert pieces[-1][0] + pieces[-1][1] == f.pcm.shape[1]
    lag = LIM.resolve(RATE)[1]
    assert pieces[0][1] == wire.resample_ready(MODEL_SR, RATE, st.spf * st.schedule[0][1], st.o.shape[-1]) - lag
    ref, valid = wire.service_pcm16(net, st.o, st.y_lengths, MODEL_SR, RATE, limiter=LIM, peak=peak)
    assert torch.equal(f.pcm, ref) and torch.equal(f.valid_samples, valid)
    assert int(f.pcm.abs().max()) <= int(np.floor(C32 * 32767)) + 1
    # auto_normalize with a limiter: the utterance's own peak and the 0.9 margin leave the limiter nothing to do
    auto, _ = wire.service_pcm16(net, st.o, st.y_lengths, MODEL_SR, RATE, limiter=LIM)
    plain, _ = wire.service_pcm16(net, st.o, st.y_lengths, MODEL_SR, RATE)
    assert torch.equal(auto, plain)
    with pytest.raises(ValueError, match="limiter"):
        wire.service_pcm16(net, st.o, st.y_lengths, MODEL_SR, RATE, peak=peak)


def _live_inputs(net, T, seed, in_sr=48000):
    return _audio(_raw_len(T, 1, in_sr), seed, in_sr, True).cuda(), _noise(net, 100 + seed, in_sr)


def _drive_live(net, raw, noise, pattern, T, limiter, peak, in_sr=48000):
    lw = _open(net, in_sr, RATE, raw.dtype, noise, peak, 32, (8, 32), limiter=limiter)
    pieces, off = [], 0
    for k in _cuts(net, pattern, in_sr, raw.numel(), T, 32, 1):
        lw.push(raw[off:off + k])
        off += k
        pieces += [(a, v.numel()) for a, v in lw.poll()]
    lw.close()
    pieces += [(a, v.numel()) for a, v in lw.poll()]
    assert lw.finished
    return lw, pieces


def test_live_wire_does_not_depend_on_the_pushes():
    net = _net()
    T = 100
    raw, noise = _live_inputs(net, T, 31)
    plain, _ = _drive_live(net, raw, noise, "one", T, None, None)
    peak = float(plain.peak[0]) * 0.25
    a, pa = _drive_live(net, raw, noise, "20ms", T, LIM, peak)
    b, pb = _drive_live(net, raw, noise, "random", T, LIM, peak)
    assert pa == pb and pa[0][0] == 0 and sum(n for _, n in pa) == int(a.valid_samples[0])
    assert torch.equal(a.pcm, b.pcm) and torch.equal(a.valid_samples, b.valid_samples) and torch.equal(a.peak, b.peak)
    assert torch.equal(a.peak, plain.peak)                            # the running peak keeps its meaning
    valid = int(a.valid_samples[0])
    assert 0 < int(a.pcm[0, :valid].abs().max()) <= int(np.floor(C32 * 32767)) + 1
    clipped, _ = _drive_live(net, raw, noise, "one", T, None, peak)
    assert int((clipped.pcm.abs() >= 32767).sum()) > 0
    # and it is the one-shot chain of the decoded waveform
    o = a.live.result()
    ref, ref_valid = wire.service_pcm16(net, o, torch.tensor([T]).cuda(), MODEL_SR, RATE, limiter=LIM, peak=peak)
    assert int(ref_valid[0]) == valid and torch.equal(a.pcm[:, :valid], ref[:, :valid])


def test_a_pool_of_limited_unlimited_and_live_members_is_bitwise_each_alone():
    """Two limited streams with different limiters, one unlimited stream and one limited live wire in a PcmPool: every
    member's bytes are those of its stand-alone run, and a tick costs one launch per kind that has something to write
    (two in a mixed tick)."""
    net = _net()
    sts = [_text_stream(net, T, 10 + k) for k, T in enumerate((20, 14, 17))]
    peaks = [_small_peak(net, st) for st in sts]
    lims = [LIM, LIM2, None]
    alone = []
    for st, pk, lim in zip(sts, peaks, lims):
        f = wire.stream_pcm16(net, _again(net, st), MODEL_SR, RATE, peak=pk, limiter=lim)
        alone.append(tuple(t.clone() for t in f.run()) + (f.peak.clone(),))
    T = 100
    raw, noise = _live_inputs(net, T, 32)
    solo, solo_pieces = _drive_live(net, raw, noise, "20ms", T, LIM2, 0.05)
    pp = wire.pcm_pool(net, net.stream_pool(), MODEL_SR, RATE)
    fol = [pp.add(st, peak=pk, limiter=lim) for st, pk, lim in zip(sts, peaks, lims)]
    lw = _open(net, 48000, RATE, raw.dtype, noise, 0.05, 32, (8, 32), limiter=LIM2)
    with pytest.raises(ValueError, match="opened with"):
        pp.add_live(lw, limiter=LIM)
    assert pp.add_live(lw, limiter=LIM2) is lw and len(pp) == 4
    got = {id(m): [] for m in sts + [lw]}
    limited = {id(st): lim is not None for st, lim in zip(sts, lims)}
    limited[id(lw)] = True
    off, step_size, mixed = 0, 48000 // 10, 0
    for step in range(80):
        if off < raw.numel():
            lw.push(raw[off:off + step_size])
            off += step_size
        elif not lw.closed:
            lw.close()
        runs = wire.wire_runs(net)
        out = pp.step(host=step % 2 == 1)
        runs = wire.wire_runs(net) - runs
        kinds = {limited[id(m)] for m, _, v in out if len(v)}
        assert len(kinds) <= runs <= 2, (step, runs, kinds)
        mixed += runs == 2
        for m, a, v in out:
            got[id(m)].append((a, torch.as_tensor(np.array(v)) if isinstance(v, np.ndarray) else v.cpu()))
        if not len(pp):
            break
    assert len(pp) == 0 and mixed >= 1
    for st, f, (pcm, valid, peak) in zip(sts, fol, alone):
        assert torch.equal(f.pcm, pcm) and torch.equal(f.valid_samples, valid) and torch.equal(f.peak, peak)
        host = pcm[0].cpu()
        assert sum(v.numel() for _, v in got[id(st)]) == pcm.shape[1]
        for a, v in got[id(st)]:
            assert torch.equal(v, host[a:a + v.numel()])
    assert torch.equal(lw.pcm, solo.pcm) and torch.equal(lw.valid_samples, solo.valid_samples)
    assert torch.equal(lw.peak, solo.peak)
    assert [(a, v.numel()) for a, v in got[id(lw)]] == solo_pieces
    host = solo.pcm[0].cpu()
    for a, v in got[id(lw)]:
        assert torch.equal(v, host[a:a + v.numel()])


def test_convert_pcm16_and_admit_take_the_limiter():
    net = _net()
    wave = _audio(HOP * 60, 77, MODEL_SR, False).cuda()[None]
    src, tgt = torch.tensor([3]).cuda(), torch.tensor([7]).cuda()
    args = (net, wave, None, src, tgt, MODEL_SR, MODEL_SR, RATE, HOP, WIN)
    plain, valid = wire.convert_pcm16(*args, seed=9)
    auto, auto_valid = wire.convert_pcm16(*args, seed=9, limiter=LIM)
    assert torch.equal(auto, plain) and torch.equal(auto_valid, valid)     # its own peak leaves the limiter nothing to do
    raw, _ = wire.convert_pcm16(*args, seed=9, auto_normalize=False)
    loudest = int(raw.abs().max())
    assert loudest >= 16
    ceiling = loudest / 32767.0 / 4                                   # a quarter of what the conversion reaches
    low = wire.Limiter(ceiling=ceiling, lookahead_ms=1.0, hold_ms=2.0)
    got, _ = wire.convert_pcm16(*args, seed=9, auto_normalize=False, limiter=low)
    top = int(np.floor(float(np.float32(ceiling)) * 32767)) + 1
    assert loudest > top >= int(got.abs().max()) > 0
    # admitted as a pooled request: the follower carries the limiter, and the bytes are the stand-alone stream's
    req = ConvertRequest(wave[0].cpu(), 3, 7, MODEL_SR, HOP, WIN, chunk_frames=8, max_chunk_frames=32, seed=9)
    pp = wire.pcm_pool(net, net.stream_pool(), MODEL_SR, RATE)
    f = pp.admit([req], limiter=low)[0]
    assert f.limiter is low
    alone = wire.stream_pcm16(net, net.dec_stream(f._st.z.clone(), f._st.g, 8, 32), MODEL_SR, RATE, limiter=low).run()
    while len(pp):
        pp.step()
    assert torch.equal(f.pcm, alone[0]) and torch.equal(f.valid_samples, alone[1])
    assert int(f.pcm.abs().max()) <= top
    with pytest.raises(ValueError, match="one limiter per request"):
        pp.admit([req], limiter=[low, low])


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_launch_nothing_and_the_stream_serves_on():
    net, x, valid = _case(22050, 24000)
    n = x.shape[-1]
    width = wire.resample_ready(22050, 24000, n, n)
    pcm = torch.full((3, width), SENTINEL, device="cuda", dtype=torch.int16)
    runs = wire.wire_runs(net)
    for lim, what in (((0.0, 7, 19), "ceiling"), ((1.5, 7, 19), "ceiling"), ((float("nan"), 7, 19), "ceiling"),
                      ((0.9, -1, 19), "lookahead"), ((0.9, 256, 19), "lookahead"), ((0.9, 7, -1), "hold"),
                      ((0.9, 7, 1025), "hold")):
        with pytest.raises(_capi.MbvError, match=what):
            net.resample_pcm16_range(x, 22050, 24000, n, 0, 10, pcm, limiter=lim)
    # a range that ends beyond what the limiter has made final: the unlimited readiness is not enough
    ready = wire.resample_ready(22050, 24000, 1000, n)
    with pytest.raises(_capi.MbvError, match="make only %d final" % (ready - 7)):
        net.resample_pcm16_range(x, 22050, 24000, 1000, 0, ready, pcm, limiter=(0.9, 7, 19))
    with pytest.raises(_capi.MbvError, match="chunk 1: limiter hold"):
        ks = [_chunk(x[0, 0], valid[:1], n, 0, 10, pcm[0], torch.zeros(1).cuda(), None, None),
              _chunk(x[1, 0], valid[1:2], n, 0, 10, pcm[1], torch.zeros(1).cuda(), None, None)]
        net.resample_pcm16_chunks(ks, 22050, 24000, limits=[(0.9, 7, 19), (0.9, 7, 2000)])
    with pytest.raises(ValueError, match="one limit per chunk"):
        net.resample_pcm16_chunks(ks, 22050, 24000, limits=[(0.9, 7, 19)])
    assert wire.wire_runs(net) == runs and (pcm == SENTINEL).all()
    # the Python entries refuse before anything is launched
    st = _text_stream(net, 12, 3)
    for bad, what in ((wire.Limiter(lookahead_ms=20.0), "lookahead_ms"), (wire.Limiter(hold_ms=60.0), "hold_ms")):
        with pytest.raises(ValueError, match=what):
            wire.stream_pcm16(net, st, MODEL_SR, RATE, limiter=bad)
        with pytest.raises(ValueError, match=what):
            wire.service_pcm16(net, torch.zeros(1, 1, 512).cuda(), None, MODEL_SR, RATE, limiter=bad)
        with pytest.raises(ValueError, match=what):
            wire.pcm_pool(net, net.stream_pool(), MODEL_SR, RATE).add(st, limiter=bad)
    with pytest.raises(TypeError, match="wire.Limiter"):
        wire.stream_pcm16(net, st, MODEL_SR, RATE, limiter=(0.9, 7, 19))
    raw, noise = _live_inputs(net, 100, 33)
    net.set_option("conv_bf16", 3)
    try:
        with pytest.raises(ValueError, match="conv_bf16"):                # as on the unlimited path
            _open(net, 48000, RATE, raw.dtype, noise, limiter=LIM)
    finally:
        net.set_option("conv_bf16", 0)
    assert st._next == 0 and wire.wire_runs(net) == runs
    # a handle re-created mid-stream: the follower refuses as the unlimited one does, and serves on afterwards
    f = wire.stream_pcm16(net, st, MODEL_SR, RATE, peak=0.05, limiter=LIM)
    next(f)
    h = net._handle
    net._handle = object()
    try:
        with pytest.raises(RuntimeError, match="re-created"):
            next(f)
    finally:
        net._handle = h
    f.run()
    ref, _ = wire.service_pcm16(net, st.o, st.y_lengths, MODEL_SR, RATE, limiter=LIM, peak=0.05)
    assert torch.equal(f.pcm, ref)
