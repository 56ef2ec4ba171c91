"""-m gpu: barge-in on the wire: the fade-out inside the wire kernels (`mbv_resample_pcm16_range_faded`,
`mbv_resample_pcm16_chunks_faded` and their G.711 forms), `PcmStream.revoke` / `PcmPool.revoke`, and the token marks
of `infer_stream(marks=True)`.  The fade is pinned to the float64 restatement of its definition (tests/fade_ref.py)
within one int16 step, as the limiter is; every relation between the one-shot, chunked, pooled and streamed forms is
bitwise."""
import numpy as np
import pytest
import torch

from mb_istft_vits_amd import _capi, wire
from mb_istft_vits_amd.models import ConvertRequest, Request

import fade_ref
import g711_ref
from test_gpu_limiter import (C32, CEILING, LIM, SENTINEL, _again, _chunk, _gained, _n_out, _net, _resampled, _same,
                              _small_peak, _text_stream)
from test_gpu_live_wire import HOP, MODEL_SR, WIN, _audio, _noise, _open, _text_batch

pytestmark = pytest.mark.gpu

PAIRS = [(22050, 24000), (22050, 8000)]
N_IN = 2000
VALID = [N_IN, N_IN - 500, N_IN - 200]
# straddles a 256-output workgroup edge; the first sample; a hard cut; runs past the end of the row
FADES = [(250, 13), (0, 1), (700, 0), (1900, 400)]
LIMIT = (CEILING, 7, 19)
RATE = 24000
_CASES = {}


def _case(orig, target):
    """x fp32 [3, 1, N_IN] (two rows with bursts above the ceiling, one quiet), valid [3], and what every test of a pair
    shares: the resampled rows v (the one-shot kernel's, bitwise the ranged FIR) and the unfaded entries' outputs"""
    if (orig, target) not in _CASES:
        net = _net()
        rs = np.random.RandomState(7 + target % 97)
        x = rs.uniform(-0.3, 0.3, size=(3, N_IN)).astype(np.float32)
        for b in (0, 1):
            for k, p in enumerate((3, 230, 600, 690, 1100, 1400)):
                x[b, p:p + 12] = (2.2 if k % 2 == 0 else -1.9) * (1.0 + 0.1 * b)
        x = torch.from_numpy(x[:, None, :]).cuda()
        valid = torch.tensor(VALID, dtype=torch.int64).cuda()
        v, ns = _resampled(net, x, valid, orig, target)
        plain = {(lim, law): _ranged(net, x, valid, orig, target, lim, law, None)
                 for lim in (None, LIMIT) for law in ("pcm16", "ulaw")}
        _CASES[(orig, target)] = (net, x, valid, v, ns, plain)
    return _CASES[(orig, target)]


def _ranged(net, x, valid, orig, target, lim, law, fade, cuts=(), peak=None):
    """the ranged entry over the whole row, in one call or cut at `cuts`; -> (samples [B, width], out_samples)"""
    B, n = x.shape[0], x.shape[-1]
    width = wire.resample_ready(orig, target, n, n)
    dtype, sentinel = (torch.int16, SENTINEL) if law == "pcm16" else (torch.uint8, 0x5A)
    out = torch.full((B, width), sentinel, device="cuda", dtype=dtype)
    ns = torch.full((B,), -1, device="cuda", dtype=torch.int64)
    done = 0
    for i, end in enumerate(sorted({c for c in cuts if 0 < c < width} | {width})):
        net.resample_pcm16_range(x, orig, target, n, done, end - done, out, valid_samples=valid, peak=peak,
                                 out_samples=ns if i == 0 else None, limiter=lim, encoding=law, fade=fade)
        assert (out[:, end:] == sentinel).all()                           # nothing past the range is written
        done = end
    return out, ns


# ------------------------------------------------------------------------------------------------ 1. the definition
@pytest.mark.parametrize("lim", [None, LIMIT], ids=["plain", "limited"])
@pytest.mark.parametrize("orig,target", PAIRS)
def test_ranged_faded_entry_against_the_float64_definition(orig, target, lim):
    net, x, valid, v, ns_ref, plain = _case(orig, target)
    width = v.shape[1]
    n_out = [_n_out(n, orig, target) for n in VALID]
    assert (np.abs(v[:2]).max(axis=1) > C32).all() and np.abs(v[2]).max() < C32
    peak = torch.tensor([0.5, 0.0, 0.25], device="cuda")                  # row 1: below the 0.01 threshold
    for fade in FADES:
        F, N = fade
        for pk in (None, peak):
            got_t, ns = _ranged(net, x, valid, orig, target, lim, "pcm16", fade, peak=pk)
            got = got_t.cpu().numpy()
            vv = _gained(v, pk)
            ref = np.stack([fade_ref.pcm16(vv[b], F, N, (C32,) + lim[1:] if lim else None) for b in range(3)])
            diff = np.abs(got.astype(np.int64) - ref.astype(np.int64))
            print("fade %s, %d -> %d, %s, peak %s: max |int16 - float64 reference| = %d"
                  % (fade, orig, target, "limited" if lim else "plain", "given" if pk is not None else "none", diff.max()))
            # the bar of test_gpu_limiter.py::test_ranged_entry_against_the_float64_definition; the ramp adds one fp32
            # product of relative error 2^-23 to a value of at most 1
            assert diff.max() <= 1
            assert torch.equal(ns, ns_ref)                                # the kernel's lengths are the unfaded ones
            assert (got[:, min(F + N, width):] == 0).all()                # a range that overshoots stores silence
            for b in range(3):
                assert (got[b, n_out[b]:] == 0).all()
            if lim:
                assert np.abs(got.astype(np.int64)).max() <= int(np.floor(C32 * 32767)) + 1
            if pk is None:
                # in front of the fade: bitwise the unfaded entry; inside it the ramp did something
                assert torch.equal(got_t[:, :F], plain[(lim, "pcm16")][0][:, :F])
                if F < min(n_out) and N > 0:
                    assert not torch.equal(got_t[:, F:F + N], plain[(lim, "pcm16")][0][:, F:F + N])
                # mu-law: the byte is the encoding of the faded int16
                by, by_ns = _ranged(net, x, valid, orig, target, lim, "ulaw", fade)
                assert np.array_equal(by.cpu().numpy(), g711_ref.encode(got, "ulaw")) and torch.equal(by_ns, ns_ref)
                assert (by[:, min(F + N, width):] == g711_ref.ZERO["ulaw"]).all()
                assert torch.equal(by[:, :F], plain[(lim, "ulaw")][0][:, :F])
    assert fade_ref.length(width, 250, 13) == 263 and fade_ref.length(width, 1900, 400) == min(width, 2300)


# ------------------------------------------------------------------------------------------------ 2. chunk invariance
@pytest.mark.parametrize("law", ["pcm16", "ulaw"])
@pytest.mark.parametrize("lim", [None, LIMIT], ids=["plain", "limited"])
@pytest.mark.parametrize("orig,target", PAIRS)
def test_faded_ranges_do_not_depend_on_the_cuts(orig, target, lim, law):
    net, x, valid, v, _, _ = _case(orig, target)
    peak = torch.tensor([0.5, 0.0, 1.7], device="cuda")
    for F, N in FADES:
        want = _ranged(net, x, valid, orig, target, lim, law, (F, N), peak=peak)
        # before the fade, inside it (two cuts), at its end, and behind it
        cuts = [F - 40, F, F + max(N // 3, 1), F + max(2 * N // 3, 2), F + N, F + N + 7]
        got = _ranged(net, x, valid, orig, target, lim, law, (F, N), cuts=cuts, peak=peak)
        assert _same(got, want), (F, N)


# ------------------------------------------------------------------------------------------------ 3. the pooled entry
@pytest.mark.parametrize("law", ["pcm16", "alaw"])
@pytest.mark.parametrize("mixed", [False, True], ids=["unlimited", "mixed"])
def test_pooled_rows_are_their_ranged_calls_at_the_launches_of_the_unfaded_call(mixed, law):
    orig, target = 22050, 24000
    net, x, valid, v, _, _ = _case(orig, target)
    n = x.shape[-1]
    width = v.shape[1]
    fades = [(250, 13), None, (700, 0), None, (1900, 400), (0, 1)]
    limits = [LIMIT, None, None, (0.5, 40, 100), LIMIT, None] if mixed else [None] * 6
    rows = [(k % 3, fades[k], limits[k]) for k in range(6)]
    dtype, sentinel = (torch.int16, SENTINEL) if law == "pcm16" else (torch.uint8, 0x5A)
    peak = torch.tensor([0.5], device="cuda")

    def call(with_fades, first, count):
        state, chunks = [], []
        for b, _, _ in rows:
            xb, vb = x[b, 0].contiguous(), valid[b:b + 1].clone()
            pcm = torch.full((width,), sentinel, device="cuda", dtype=dtype)
            ns = torch.full((1,), -1, device="cuda", dtype=torch.int64)
            running = torch.zeros(1, device="cuda")       # kept in `state`: the launch writes it after this loop
            state.append((xb, vb, pcm, ns, running))
            chunks.append(_chunk(xb, vb, n, first, count, pcm, running, ns, peak))
        packed = torch.full((6 * count + 8,), sentinel, device="cuda", dtype=dtype)
        runs = wire.wire_runs(net)
        net.resample_pcm16_chunks(chunks, orig, target, packed=packed, limits=limits, encoding=law,
                                  fades=[f for _, f, _ in rows] if with_fades else None)
        return state, packed, wire.wire_runs(net) - runs

    today, _, runs_today = call(False, 0, width)
    got, packed, runs = call(True, 0, width)
    assert runs == runs_today == (2 if mixed else 1)                      # fading rows cost no launch
    for k, (b, fade, lim) in enumerate(rows):
        want, want_ns = _ranged(net, x[b:b + 1], valid[b:b + 1], orig, target, lim, law, fade, peak=peak)
        assert torch.equal(got[k][2], want[0]) and torch.equal(got[k][3], want_ns), k
        assert torch.equal(packed[k * width:(k + 1) * width], want[0])
        if fade is None:
            assert torch.equal(got[k][2], today[k][2])                    # bitwise its row in today's entry
        else:
            assert torch.equal(got[k][2][:fade[0]], today[k][2][:fade[0]])
    assert (packed[6 * width:] == sentinel).all()
    # a partial range that ends inside the fades, then the rest: the same bytes
    part, _, r1 = call(True, 0, 256)
    assert r1 == runs_today
    for k in range(6):
        assert torch.equal(part[k][2][:256], got[k][2][:256]) and (part[k][2][256:] == sentinel).all()


# ------------------------------------------------------------------------------------------------ 4. a revoked stream
def _play(net, st0, peak, limiter, encoding, revoke=None):
    """the stream over the decode of `st0` once more, revoked after its second piece when `revoke` (the keyword
    arguments) is given; -> (follower, pieces, decoder runs, report)"""
    f = wire.stream_pcm16(net, _again(net, st0), MODEL_SR, RATE, peak=peak, limiter=limiter, encoding=encoding)
    runs = net.decoder_runs()
    pieces, report = [], None
    for a, view in f:
        pieces.append((a, view.clone()))
        if revoke is not None and len(pieces) == 2:
            report = f.revoke(**revoke)
    return f, pieces, net.decoder_runs() - runs, report


@pytest.mark.parametrize("kind", ["plain", "limited", "alaw"])
def test_a_revoked_stream_is_the_faded_one_shot_and_stops_decoding(kind):
    net = _net()
    st0 = _text_stream(net, 60, 5)
    limiter = LIM if kind == "limited" else None
    encoding = "alaw" if kind == "alaw" else "pcm16"
    peak = _small_peak(net, st0) if limiter else None
    full, full_pieces, full_runs, _ = _play(net, st0, peak, limiter, encoding)
    assert len(full_pieces) >= 5 and full.finished and not full.revoked       # chunks of 8, 16, 32, 32, .. frames
    f, pieces, runs, rep = _play(net, st0, peak, limiter, encoding, revoke=dict(fade_ms=5.0))
    E = full_pieces[1][0] + full_pieces[1][1].shape[1]
    N = int(round(5.0 * RATE / 1000))
    assert (rep.first, rep.count, rep.valid_samples, rep.tokens_started) == (E, N, E + N, None)
    assert f.finished and f.revoked and runs < full_runs and len(pieces) < len(full_pieces)
    # the pieces handed out before the revoke are the un-revoked stream's; afterwards they run on to the cut, no further
    for (a, got), (b, want) in zip(pieces[:2], full_pieces[:2]):
        assert a == b and torch.equal(got, want)
    assert pieces[0][0] == 0 and all(a + v.shape[1] == b for (a, v), (b, _) in zip(pieces, pieces[1:]))
    assert pieces[-1][0] + pieces[-1][1].shape[1] == E + N
    # the whole: bitwise the one-shot chain of the FINISHED waveform with the same fade, over the new length
    ref, ref_valid = wire.service_pcm16(net, full._st.o, None, MODEL_SR, RATE, auto_normalize=False, limiter=limiter,
                                        peak=peak, encoding=encoding, fade=(E, N))
    assert int(ref_valid[0]) == int(f.valid_samples[0]) == E + N
    assert torch.equal(f.pcm[:, :E + N], ref[:, :E + N])
    assert torch.equal(torch.cat([v for _, v in pieces], dim=1), ref[:, :E + N])
    assert not torch.equal(ref[:, E:E + N], full.pcm[:, E:E + N])         # the fade did something
    if limiter:
        assert int(f.pcm[:, :E + N].abs().max()) <= int(np.floor(C32 * 32767)) + 1
    # revoking again, or a finished stream, changes nothing
    again = f.revoke(fade_ms=50.0)
    assert again is rep and int(f.valid_samples[0]) == E + N
    total = int(full.valid_samples[0])
    done = full.revoke()
    assert (done.first, done.count, done.valid_samples) == (total, 0, total) and int(full.valid_samples[0]) == total


def test_a_hard_cut_and_a_fade_beyond_the_end():
    net = _net()
    st0 = _text_stream(net, 40, 5)
    full, full_pieces, full_runs, _ = _play(net, st0, None, None, "pcm16")
    total = int(full.valid_samples[0])
    E = full_pieces[1][0] + full_pieces[1][1].shape[1]
    f, pieces, runs, rep = _play(net, st0, None, None, "pcm16", revoke=dict(fade_ms=0.0))
    assert (rep.first, rep.count, rep.valid_samples) == (E, 0, E) and len(pieces) == 2 and runs < full_runs
    assert int(f.valid_samples[0]) == E and torch.equal(f.pcm[:, :E], full.pcm[:, :E])
    # a fade that would end beyond the stream clamps: the stream plays to its end, fading
    f, pieces, runs, rep = _play(net, st0, None, None, "pcm16", revoke=dict(fade_ms=1e4, at=E + 100))
    N = int(round(1e4 * RATE / 1000))
    assert (rep.first, rep.count, rep.valid_samples) == (E + 100, N, total) and runs == full_runs
    ref, ref_valid = wire.service_pcm16(net, full._st.o, None, MODEL_SR, RATE, auto_normalize=False, fade=(E + 100, N))
    assert int(ref_valid[0]) == total == int(f.valid_samples[0]) and torch.equal(f.pcm, ref)
    assert torch.equal(f.pcm[:, :E + 100], full.pcm[:, :E + 100])


# ------------------------------------------------------------------------------------------------ 5. a revoked member
def test_a_pool_with_a_revoked_member_is_bitwise_each_alone():
    net = _net()
    sts = [_text_stream(net, 40, 21), _text_stream(net, 30, 22)]
    wave = _audio(HOP * 150, 78, MODEL_SR, False)
    req = ConvertRequest(wave, 3, 7, MODEL_SR, HOP, WIN, chunk_frames=8, max_chunk_frames=32, seed=11)
    pp = wire.pcm_pool(net, net.stream_pool(), MODEL_SR, RATE)
    fol = [pp.add(_again(net, st)) for st in sts] + pp.admit([req])
    chunks_before = len(fol[0]._st.schedule)
    alone = []
    for k, f in enumerate(fol[1:]):
        a = wire.stream_pcm16(net, net.dec_stream(f._st.z.clone(), f._st.g, 8, 32), MODEL_SR, RATE)
        alone.append(tuple(t.clone() for t in a.run()))
    assert len(pp) == 3 and len(pp.pool) == 3
    rep, left_at, sizes = None, None, []
    for step in range(200):
        if step == 2:
            rep = pp.revoke(fol[0]._st, fade_ms=5.0)
            assert rep.first == fol[0]._done and rep.valid_samples == rep.first + rep.count
        runs = wire.wire_runs(net)
        out = pp.step()
        runs = wire.wire_runs(net) - runs
        assert runs <= 1 and (runs == 1 or not any(v.numel() for _, _, v in out)), step    # one launch a tick, fade or not
        sizes.append(len(pp))
        if left_at is None and fol[0].finished:
            left_at = step
            assert len(pp) == 2 and len(pp.pool) == 2                     # it left both pools, the others play on
            assert not any(m is fol[0]._st for m in pp.pool.streams)
        if not len(pp):
            break
    assert left_at is not None and 2 <= left_at < step and len(pp) == 0
    assert len(fol[0]._st.schedule) < chunks_before                       # the later chunks were never issued
    for f, (pcm, valid) in zip(fol[1:], alone):
        assert torch.equal(f.pcm, pcm) and torch.equal(f.valid_samples, valid)
    # the revoked member: bitwise the stand-alone stream revoked with the same fade (from its start)
    a = wire.stream_pcm16(net, _again(net, sts[0]), MODEL_SR, RATE)
    a.revoke(fade_ms=5.0, at=rep.first)
    a.run()
    cut = rep.valid_samples
    assert int(a.valid_samples[0]) == int(fol[0].valid_samples[0]) == cut
    assert torch.equal(a.pcm[:, :cut], fol[0].pcm[:, :cut])
    # a member revoked with nothing left to wire leaves at once; a stranger is refused
    pp = wire.pcm_pool(net, net.stream_pool(), MODEL_SR, RATE)
    f = pp.add(_again(net, sts[1]))
    pp.step()
    rep = pp.revoke(f, fade_ms=0.0)
    assert rep.count == 0 and f.finished and len(pp) == 0 and len(pp.pool) == 0
    with pytest.raises(ValueError, match="not in the pool"):
        pp.revoke(_again(net, sts[1]))
    # the bare form: a pool without a wire drops a member
    pool = net.stream_pool()
    a, b = pool.add(_again(net, sts[0])), pool.add(_again(net, sts[1]))
    pool.step()
    pool.remove(a)
    assert len(pool) == 1 and all(st is b for st, _, _ in pool.step()) and a._decoded == 1
    with pytest.raises(ValueError, match="not in the pool"):
        pool.remove(a)


# ------------------------------------------------------------------------------------------------ 6. token marks
def _durations_of(net, x, xl, sid, seed, **kw):
    """the integer durations of a request from the dense path `infer` returns: attn [1, 1, T', T] summed over T'"""
    attn = net.infer(x, xl, sid, noise_scale=0.5, seed=[seed], outputs=("attn",), **kw)[4]
    return [int(v) for v in attn[0, 0].sum(dim=0).round().long().tolist()]


def _prefix(d, keep=None):
    out = [0]
    for v in d:
        out.append(out[-1] + v)
    return out if keep is None else [min(v, keep) for v in out]


def test_marks_are_the_exclusive_prefix_sums_of_the_durations():
    net = _net()
    x, xl, sid = _text_batch(net, 1, 20, 31)
    T = int(xl[0])
    d = _durations_of(net, x, xl, sid, 77)
    runs = net.encoder_runs()
    st = net.infer_stream(x, xl, sid, noise_scale=0.5, chunk_frames=8, max_chunk_frames=32, seed=[77], marks=True)
    with_marks = net.encoder_runs() - runs
    runs = net.encoder_runs()
    bare = net.infer_stream(x, xl, sid, noise_scale=0.5, chunk_frames=8, max_chunk_frames=32, seed=[77])
    assert net.encoder_runs() - runs == with_marks
    assert bare.marks is None and st.marks == _prefix(d) and len(st.marks) == T + 1
    assert st.marks[-1] == sum(d) == st.z.shape[2] == int(st.y_lengths[0])
    assert torch.equal(st.z, bare.z) and torch.equal(st.y_lengths, bare.y_lengths)
    # clipped to the frames the stream keeps
    keep = sum(d) // 2
    cl = net.infer_stream(x, xl, sid, noise_scale=0.5, max_len=keep, seed=[77], marks=True)
    assert cl.marks == _prefix(d, keep) and cl.z.shape[2] == keep
    # the audio is bitwise the stream's without marks; the wire follower maps the marks
    f = wire.stream_pcm16(net, st, MODEL_SR, RATE, limiter=LIM)
    g = wire.stream_pcm16(net, bare, MODEL_SR, RATE, limiter=LIM)
    lag = LIM.resolve(RATE)[1]
    assert g.marks is None and f.marks == fade_ref.mark_samples(st.marks, st.spf, MODEL_SR, RATE, lag)
    next(f), next(f)
    E = f._done
    rep = f.revoke(fade_ms=2.0, at="token")
    assert rep.first in f.marks and rep.first >= E and rep.first == min(m for m in f.marks if m >= E)
    assert rep.tokens_started == sum(1 for m in f.marks[:-1] if m < rep.first) > 0
    f.run(), g.run()
    assert torch.equal(f.pcm[:, :rep.first], g.pcm[:, :rep.first])
    assert int(f.valid_samples[0]) == min(int(g.valid_samples[0]), rep.first + rep.count)


def test_admitted_requests_carry_their_marks_in_the_one_read_back():
    net = _net()
    reqs, want = [], []
    for k, T in enumerate((40, 300, 257)):
        x, xl, sid = _text_batch(net, 1, T, 40 + k)
        n = int(xl[0])
        kw = {}
        if k == 2:                                                        # given durations: used as they are
            kw["durations"] = torch.from_numpy(np.random.RandomState(5).randint(0, 4, size=(1, x.shape[1])))
        d = _durations_of(net, x, xl, sid, 90 + k, **kw)[:n]
        max_len = sum(d) - 5 if k == 0 else None
        want.append(_prefix(d, max_len))
        reqs.append(dict(x=x[0, :n].cpu(), sid=int(sid[0]), noise_scale=0.5, seed=90 + k, max_len=max_len,
                         chunk_frames=8, max_chunk_frames=32,
                         durations=kw["durations"][0, :n] if kw else None))
        if kw:
            assert d == kw["durations"][0, :n].tolist()
    assert min(len(w) for w in want) - 1 <= 256 < max(len(w) for w in want) - 1       # both of admit_plan's classes
    runs = net.encoder_runs()
    sts = net.infer_streams([Request(marks=True, **r) for r in reqs])
    with_marks = net.encoder_runs() - runs
    runs = net.encoder_runs()
    bare = net.infer_streams([Request(**r) for r in reqs])
    assert net.encoder_runs() - runs == with_marks
    for st, b, w in zip(sts, bare, want):
        assert st.marks == w and b.marks is None
        assert torch.equal(st.z, b.z) and torch.equal(st.y_lengths, b.y_lengths)
    # a mixed call: only the requests that ask get marks; a pool's followers expose them mapped
    pp = wire.pcm_pool(net, net.stream_pool(), MODEL_SR, RATE)
    fol = pp.admit([Request(marks=True, **reqs[0]), Request(**reqs[0])])
    assert fol[0].marks == fade_ref.mark_samples(want[0], fol[0]._st.spf, MODEL_SR, RATE) and fol[1].marks is None
    assert torch.equal(fol[0]._st.z, fol[1]._st.z)


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_refusals_launch_nothing_and_the_stream_plays_on():
    net = _net()
    st0 = _text_stream(net, 30, 6)
    full = wire.stream_pcm16(net, _again(net, st0), MODEL_SR, RATE)
    full.run()
    f = wire.stream_pcm16(net, _again(net, st0), MODEL_SR, RATE)
    next(f), next(f)
    counters = (wire.wire_runs(net), net.decoder_runs(), net.encoder_runs())
    with pytest.raises(ValueError, match="handed out"):
        f.revoke(at=f._done - 1)
    with pytest.raises(ValueError, match="no token marks"):
        f.revoke(at="token")
    with pytest.raises(ValueError, match="at must be"):
        f.revoke(at="soon")
    with pytest.raises(ValueError, match="fade_ms"):
        f.revoke(fade_ms=-1.0)
    assert (wire.wire_runs(net), net.decoder_runs(), net.encoder_runs()) == counters and not f.revoked
    # a converted recording has no tokens
    wave = _audio(HOP * 60, 79, MODEL_SR, False)
    pp = wire.pcm_pool(net, net.stream_pool(), MODEL_SR, RATE)
    conv = pp.admit([ConvertRequest(wave, 3, 7, MODEL_SR, HOP, WIN, chunk_frames=8, max_chunk_frames=32, seed=3)])[0]
    assert conv.marks is None
    counters = (wire.wire_runs(net), net.decoder_runs(), net.encoder_runs())
    with pytest.raises(ValueError, match="no token marks"):
        pp.revoke(conv, at="token")
    # a live member is not revoked
    lw = pp.add_live(_open(net, 48000, RATE, torch.int16, _noise(net, 170, 48000), None, 32, (8, 32)))
    with pytest.raises(ValueError, match="live member"):
        pp.revoke(lw)
    with pytest.raises(ValueError, match="live member"):
        pp.revoke(lw.live)
    # the C entries: a fade that starts below zero, an inv that is not mbv_pcm_fade_make's
    x = torch.zeros(1, 1, 2000, device="cuda")
    pcm = torch.full((1, 2177), SENTINEL, device="cuda", dtype=torch.int16)
    good = _capi.pcm_fade(100, 13)
    for bad, what in ((_capi.MbvPcmFade(-1, 13, good.inv), "first"), (_capi.MbvPcmFade(100, 13, 1.0 / 13.0), "inv"),
                      (_capi.MbvPcmFade(100, 13, float(np.nextafter(np.float32(good.inv), np.float32(1)))), "inv")):
        with pytest.raises(_capi.MbvError, match=what):
            net.resample_pcm16_range(x, 22050, 24000, 2000, 0, 500, pcm, fade=bad)
        with pytest.raises(_capi.MbvError, match="chunk 1: fade " + what):
            ks = [_chunk(x[0, 0], torch.tensor([2000]).cuda(), 2000, 0, 10, pcm[0], torch.zeros(1).cuda(), None, None)
                  for _ in range(2)]
            net.resample_pcm16_chunks(ks, 22050, 24000, fades=[good, bad])
    with pytest.raises(ValueError, match="one fade per chunk"):
        net.resample_pcm16_chunks(ks, 22050, 24000, fades=[good])
    with pytest.raises(ValueError):
        wire.service_pcm16(net, x, None, 22050, 24000, fade=(-1, 5))
    assert (wire.wire_runs(net), net.decoder_runs(), net.encoder_runs()) == counters and (pcm == SENTINEL).all()
    # the handle is usable, and the stream that refused plays on to its un-revoked end, bitwise
    net.resample_pcm16_range(x, 22050, 24000, 2000, 0, 500, pcm, fade=good)
    assert (pcm[:, :500] == 0).all() and (pcm[:, 500:] == SENTINEL).all()
    f.run()
    assert not f.revoked and torch.equal(f.pcm, full.pcm) and torch.equal(f.valid_samples, full.valid_samples)
