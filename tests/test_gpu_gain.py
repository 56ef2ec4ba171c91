"""-m gpu: per-token volume: the frame-gain kernel (`mbv_op_frame_gain`, `mbv_frame_gain`,
`mbv_frame_gain_rows`) and the gain envelope inside the wire kernels (`mbv_resample_pcm16_range_shaped`,
`mbv_resample_pcm16_chunks_shaped`, `mbv_resample_turns_shaped`).  The definition is the float32 NumPy restatement in
tests/gain_ref.py; every relation here is BITWISE: a shaped call equals the existing entry on the waveform multiplied by
that envelope on the host, and a row without an envelope equals the unshaped entry.  No tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest
import torch

from mb_istft_vits_amd import _capi, wire
from mb_istft_vits_amd.models import Request

import gain_ref
from test_gpu_barge_in import LIMIT, N_IN, VALID, _case
from test_gpu_limiter import SENTINEL, _chunk, _same
from test_gpu_turns import MODEL_SR, RATE, _ids, _net as _mini, _turn_row  # noqa: F401  (ljs_mini_mb_istft_vits)

pytestmark = pytest.mark.gpu

PAIRS = [(22050, 24000), (22050, 8000), (22050, 22050)]       # the extra bank row; downsampling; FIR = false
HOPS = [256, 100]                                             # 8 frames; 20 frames, not a power of two
FADE = (250, 13)
CUTS = (250, 257, 1000)
# 0, 1, a value that drives the +-0.3 noise floor over the ceiling, and 1e-3; neighbours differ, so every frame ramps
VALUES = [1.0, 4.0, 4.0, 0.0, 1e-3, 1.0, 2.5, 0.0, 4.0, 1.0, 1e-3]


def _frames(hop):
    return -(-N_IN // hop)


def _tables(hop):
    """G fp32 [3, F + 1] on the host: each row the values above from another offset"""
    F = _frames(hop)
    return np.asarray([[VALUES[(3 * b + t) % len(VALUES)] for t in range(F + 1)] for b in range(3)], np.float32)


def _premultiplied(x, G, hop):
    """x [B, 1, n] device -> x * e on the host in fp32 (gain_ref), back on the device"""
    xs = x[:, 0].cpu().numpy()
    return torch.from_numpy(np.stack([gain_ref.shaped(xs[b], G[b], hop) for b in range(xs.shape[0])])[:, None, :]).cuda()


def _ranged(net, x, valid, orig, target, lim, law, fade, env=None, cuts=(), peak=None):
    """the ranged entry over the whole row, in one call or cut at `cuts`; -> (samples, out_samples, running peak)"""
    B, n = x.shape[0], x.shape[-1]
    width = wire.resample_ready(orig, target, n, n)
    dtype, sentinel = (torch.int16, SENTINEL) if law == "pcm16" else (torch.uint8, 0x5A)
    out = torch.full((B, width), sentinel, device="cuda", dtype=dtype)
    ns = torch.full((B,), -1, device="cuda", dtype=torch.int64)
    running = torch.zeros(B, device="cuda")
    done = 0
    for i, end in enumerate(sorted({c for c in cuts if 0 < c < width} | {width})):
        net.resample_pcm16_range(x, orig, target, n, done, end - done, out, valid_samples=valid, peak=peak,
                                 running_peak=running, out_samples=ns if i == 0 else None, limiter=lim, encoding=law,
                                 fade=fade, envelope=env)
        assert (out[:, end:] == sentinel).all()                           # nothing past the range is written
        done = end
    return out, ns, running


# ------------------------------------------------------------------------------------------------ 1. the frame gains
def test_frame_gain_kernel_against_the_restatement():
    net = _mini()
    B, T = 3, 7
    dur = np.asarray([[2, 0, 3, 1, 0, 4, 2],          # a zero-duration token in front of others, and one inside
                      [5, 1, 1, 0, 2, 300, 1],        # clipped below (y < its sum), and longer than one workgroup
                      [1, 2, 3, 4, 5, 6, 7]], np.int64)
    cum = np.cumsum(dur, 1)
    y = np.asarray([12, 150, -1], np.int64)           # the whole row; clipped by max_len; flagged
    gain = np.random.RandomState(3).uniform(0, 16, (B, T)).astype(np.float32)
    gain[0, 0], gain[1, 5], gain[2, 3] = 0.0, 16.0, 1e-3
    for F in (150, 300, 12):                          # the stream's frames: a row may end before it (hold) or be cut by it
        out = torch.full((B, F + 4), -7.0, device="cuda")
        runs = net.gain_runs()
        net._call("mbv_op_frame_gain", torch.from_numpy(cum.astype(np.int32)).cuda(), torch.from_numpy(y).cuda(),
                  torch.from_numpy(gain).cuda(), out, out.stride(0), F, B, T)
        assert net.gain_runs() - runs == 1
        got = out.cpu().numpy()
        for b in range(B):
            want = gain_ref.frame_gain(gain[b], cum[b], y[b], F)
            assert np.array_equal(got[b, :F + 1].view(np.int32), want.view(np.int32)), (F, b)
        assert (got[:, F + 1:] == -7.0).all()                                  # nothing past F is written
        assert (got[2, :F + 1] == 1.0).all()                                   # the flagged row
    # the stand-alone op of the batch interface, from durations
    G = net.frame_gain(gain.tolist(), torch.from_numpy(dur), y_lengths=torch.tensor([12, 150, 28]))
    assert G.shape == (3, 151)
    for b, yy in enumerate((12, 150, 28)):
        assert np.array_equal(G[b].cpu().numpy(), gain_ref.frame_gain(gain[b], cum[b], yy, 150))
    G = net.frame_gain(gain, torch.from_numpy(dur).float().view(B, 1, T))      # y = the sums, F = the longest
    assert G.shape == (3, 311) and np.array_equal(G[0].cpu().numpy(), gain_ref.frame_gain(gain[0], cum[0], 12, 310))


# ------------------------------------------------------------------------------------------------ 2. the ranged entry
@pytest.mark.parametrize("hop", HOPS)
@pytest.mark.parametrize("orig,target", PAIRS)
def test_shaped_ranged_entry_is_the_entry_on_the_premultiplied_wave(orig, target, hop):
    net, x, valid = _case(22050, 24000)[:3]           # x [3, 1, 2000]: two rows with bursts, one quiet; VALID
    assert x.shape[-1] == N_IN and valid.tolist() == VALID
    G = _tables(hop)
    F = G.shape[1] - 1
    assert F == {256: 8, 100: 20}[hop] and {0.0, 1.0, 4.0}.issubset(set(G.ravel().tolist()))
    Gd = torch.from_numpy(G).cuda()
    env = wire.Envelope(Gd, hop)
    ones = wire.Envelope(torch.ones(3, F + 1, device="cuda"), hop)
    xm = _premultiplied(x, G, hop)
    assert float(xm.abs().max()) > 1.0 and not torch.equal(xm, x)
    checked = 0
    for lim in (None, LIMIT):
        for law in ("pcm16", "ulaw"):
            for fade in (None, FADE):
                want = _ranged(net, xm, valid, orig, target, lim, law, fade)
                unshaped = _ranged(net, x, valid, orig, target, lim, law, fade)
                assert not torch.equal(want[0], unshaped[0])
                for cuts in ((), CUTS):
                    got = _ranged(net, x, valid, orig, target, lim, law, fade, env=env, cuts=cuts)
                    assert _same(got, want), (lim, law, fade, cuts, int((got[0] != want[0]).sum()))
                    checked += 1
                # an all-ones table is bitwise the unshaped entry: bytes, lengths and running peak
                assert _same(_ranged(net, x, valid, orig, target, lim, law, fade, env=ones, cuts=CUTS[:1]), unshaped)
                if lim is not None and law == "pcm16" and fade is None:
                    # the limiter saw the shaped signal: the ceiling holds although the gain drove the input over it
                    assert int(got[0].abs().max()) <= int(np.floor(float(np.float32(LIMIT[0])) * 32767)) + 1
                    assert float(got[2].max()) > 1.0                           # (running peak of the shaped rows)
    assert checked == 16
    # one row with its own envelope is the row of the batch
    one = _ranged(net, x[1:2], valid[1:2], orig, target, LIMIT, "pcm16", None, env=wire.Envelope(Gd[1], hop))
    all3 = _ranged(net, x, valid, orig, target, LIMIT, "pcm16", None, env=env)
    assert torch.equal(one[0][0], all3[0][1]) and torch.equal(one[2].view(torch.int32), all3[2][1:2].view(torch.int32))


# ------------------------------------------------------------------------------------------------ 3. the pooled entry
@pytest.mark.parametrize("law", ["pcm16", "alaw"])
def test_pooled_rows_are_their_ranged_calls_at_the_launches_of_the_unshaped_call(law):
    orig, target = 22050, 24000
    net, x, valid = _case(orig, target)[:3]
    n, hop = x.shape[-1], 256
    width = wire.resample_ready(orig, target, n, n)
    Gd = torch.from_numpy(_tables(hop)).cuda()
    # (row of x, shaped, limiter): a limited pair and a plain pair, one of each shaped
    rows = [(0, True, LIMIT), (1, False, LIMIT), (0, True, None), (2, False, None)]
    envs = [wire.Envelope(Gd[b], hop) if shaped else None for b, shaped, _ in rows]
    limits = [lim for _, _, lim in rows]
    dtype, sentinel = (torch.int16, SENTINEL) if law == "pcm16" else (torch.uint8, 0x5A)
    peak = torch.tensor([0.5], device="cuda")

    def call(envelopes, first, count, state=None):
        state = state or []
        chunks = []
        for k, (b, _, _) in enumerate(rows):
            if len(state) <= k:
                state.append((x[b, 0].contiguous(), valid[b:b + 1].clone(),
                              torch.full((width,), sentinel, device="cuda", dtype=dtype),
                              torch.zeros(1, device="cuda"), torch.full((1,), -1, device="cuda", dtype=torch.int64)))
            xb, vb, pcm, running, ns = state[k]
            chunks.append(_chunk(xb, vb, n, first, count, pcm, running, ns if first == 0 else None, peak))
        packed = torch.full((len(rows) * count + 8,), sentinel, device="cuda", dtype=dtype)
        runs = wire.wire_runs(net)
        net.resample_pcm16_chunks(chunks, orig, target, packed=packed, limits=limits, encoding=law, envelopes=envelopes)
        return state, packed, wire.wire_runs(net) - runs

    today, _, runs_today = call(None, 0, width)
    got, packed, runs = call(envs, 0, width)
    assert runs == runs_today == 2                                        # shaped rows cost no launch
    for k, (b, shaped, lim) in enumerate(rows):
        want = _ranged(net, x[b:b + 1], valid[b:b + 1], orig, target, lim, law, None,
                       env=envs[k], peak=peak)
        assert torch.equal(got[k][2], want[0][0]) and torch.equal(got[k][4], want[1]), k
        assert torch.equal(got[k][3].view(torch.int32), want[2].view(torch.int32)), k
        assert torch.equal(packed[k * width:(k + 1) * width], want[0][0])
        if shaped:
            assert not torch.equal(got[k][2], today[k][2])
        else:
            assert _same(got[k][2:], today[k][2:])                        # bitwise its row in the unshaped call
    assert (packed[len(rows) * width:] == sentinel).all()
    # two ticks that meet off a tile edge: the same bytes
    part, _, r1 = call(envs, 0, 257)
    part, _, r2 = call(envs, 257, width - 257, state=part)
    assert r1 == r2 == 2
    for k in range(len(rows)):
        assert torch.equal(part[k][2], got[k][2]) and torch.equal(part[k][3].view(torch.int32), got[k][3].view(torch.int32))
    # all None is the call without envelopes
    none, _, r0 = call([None] * 4, 0, width)
    assert r0 == 2 and all(_same(a[2:], b[2:]) for a, b in zip(none, today))


# ------------------------------------------------------------------------------------------------ 4. a turn
@pytest.mark.parametrize("lim", [None, (0.9, 8, 16)], ids=["plain", "limited"])
@pytest.mark.parametrize("orig,target", PAIRS[:1] + PAIRS[2:])
def test_a_turn_applies_the_envelope_of_a_segment_before_its_ramp(orig, target, lim):
    net = _mini()
    hop, ramp, lengths, pause = 100, 64, [730, 500], 300
    g = torch.Generator().manual_seed(11)
    xs = [(torch.rand(n + 5, generator=g) * 0.8 - 0.4).cuda() for n in lengths]
    G = np.asarray([VALUES[t % len(VALUES)] for t in range(9)], np.float32)        # 8 frames of 100 cover 730
    env = wire.Envelope(torch.from_numpy(G).cuda(), hop)
    shaped0 = torch.from_numpy(gain_ref.shaped(xs[0][:lengths[0]].cpu().numpy(), G, hop)).cuda()
    row = wire.assemble_turn([shaped0, xs[1]], lengths, [pause], ramp)
    total = sum(lengths) + pause
    assert row.shape[-1] == total
    width = wire.resample_ready(orig, target, total, total)
    peak = torch.tensor([0.6], device="cuda")
    want = _ranged(net, row, None, orig, target, lim, "pcm16", None, peak=peak)
    plan = wire.TurnPlan(orig, target, width, lookahead=lim[1] if lim else 0, hold=lim[2] if lim else 0)
    for s, n in enumerate(lengths):
        plan.append(n, pause if s else 0)
        plan.decoded(s, n)
    plan.close()
    pcm = torch.full((1, width), SENTINEL, device="cuda", dtype=torch.int16)
    running = torch.zeros(1, device="cuda")
    ns = torch.full((1,), -1, device="cuda", dtype=torch.int64)
    tiles = [(0, 257), (257, width - 257)]
    turns = [_turn_row(plan, xs, ramp, pcm, running, peak, a, c, ns=ns if a == 0 else None, every=True) for a, c in tiles]
    assert all(k.n_segs == 2 for k in turns)
    runs = wire.wire_runs(net)
    net.resample_turns(turns, orig, target, limits=[lim] * 2, envelopes=[[env, None], [env, None]])
    assert wire.wire_runs(net) - runs == 1
    assert _same((pcm, ns, running), want), int((pcm != want[0]).sum())
    # without envelopes the same call is the unshaped turn: the second segment's samples did not move
    pcm0, run0 = torch.full_like(pcm, SENTINEL), torch.zeros(1, device="cuda")
    net.resample_turns([_turn_row(plan, xs, ramp, pcm0, run0, peak, 0, width, every=True)], orig, target, limits=[lim],
                       envelopes=[[None, None]])
    plain = _ranged(net, wire.assemble_turn(xs, lengths, [pause], ramp), None, orig, target, lim, "pcm16", None, peak=peak)
    assert torch.equal(pcm0, plain[0]) and not torch.equal(pcm0, pcm)


# ------------------------------------------------------------------------------------------------ 5. end to end
T_TEXT, SEED = 11, 41
GAINS = [1.0, 4.0, 0.0, 1e-3, 2.0, 1.0, 0.25, 4.0, 1.0, 0.5, 3.0]
KW = dict(noise_scale=0.5, length_scale=3.0, chunk_frames=8, max_chunk_frames=16)
_E2E = {}


def _stream(net, gain=None, marks=False, T=T_TEXT, seed=SEED, max_len=None):
    x = _ids(T, seed).view(1, -1).cuda()
    return net.infer_stream(x, torch.tensor([T]).cuda(), None, seed=[seed], marks=marks, max_len=max_len,
                            **({} if gain is None else {"gain": [gain]}), **KW)


def _e2e():
    """the finished plain decode, the shaped stream's frame gains on the host, and a peak that makes the gain count"""
    if not _E2E:
        net = _mini()
        plain = _stream(net)
        plain.run()
        st = _stream(net, GAINS, marks=True)
        G = st.frame_gain.cpu().numpy()
        peak = (plain.o.abs().max() * 0.5).reshape(1)
        _E2E.update(plain=plain, G=G, marks=st.marks, peak=peak)
    return _E2E["plain"], _E2E["G"], _E2E["marks"], _E2E["peak"]


def test_infer_stream_gives_the_frame_gains_and_leaves_the_decode_alone():
    net = _mini()
    runs, enc = net.gain_runs(), net.encoder_runs()
    st = _stream(net, GAINS, marks=True)
    assert net.gain_runs() - runs == 1 and net.encoder_runs() - enc == 1
    F = st.z.shape[2]
    assert st.frame_gain.shape == (1, F + 1) and st.frame_gain.dtype == torch.float32 and st.frame_gain.is_cuda
    want = gain_ref.frame_gain_of_marks(GAINS, st.marks, F)
    assert np.array_equal(st.frame_gain[0].cpu().numpy().view(np.int32), want.view(np.int32))
    assert len(set(want.tolist())) >= 5                                   # most tokens got frames of their own
    plain, G, _, _ = _e2e()
    st.run()
    assert torch.equal(st.z, plain.z) and torch.equal(st.o, plain.o)      # bitwise the stream without gain=
    runs = net.gain_runs()
    assert _stream(net).frame_gain is None and net.gain_runs() == runs    # without gain= nothing is launched
    # max_len: the table covers the kept frames, and holds the gain of the last one
    cut = _stream(net, GAINS, marks=True, max_len=F - 5)
    assert cut.frame_gain.shape == (1, F - 4)
    assert np.array_equal(cut.frame_gain[0].cpu().numpy(), gain_ref.frame_gain_of_marks(GAINS, cut.marks, F - 5))
    assert np.array_equal(cut.frame_gain[0, :F - 5].cpu().numpy(), want[:F - 5])
    # a batch of two rows of different lengths: each row its own table, held behind its end
    x = torch.stack([_ids(T_TEXT, SEED), _ids(T_TEXT, SEED + 1)]).cuda()
    xl = torch.tensor([T_TEXT, 7]).cuda()
    two = net.infer_stream(x, xl, None, seed=5, marks=True, gain=[GAINS, GAINS[::-1]], **KW)
    F2 = two.z.shape[2]
    for b, g in enumerate((GAINS, GAINS[::-1])):
        ref = gain_ref.frame_gain_of_marks(g[:len(two.marks[b]) - 1], two.marks[b], F2)
        assert np.array_equal(two.frame_gain[b].cpu().numpy(), ref), b


@pytest.mark.parametrize("limited", [True, False], ids=["limited", "plain"])
def test_streamed_service_and_premultiplied_bytes_are_the_same(limited):
    net = _mini()
    plain, G, _, peak = _e2e()
    limiter = wire.Limiter(0.9, lookahead_ms=1.0, hold_ms=2.0) if limited else None
    st = _stream(net, GAINS)
    f = wire.stream_pcm16(net, st, MODEL_SR, RATE, peak=peak if limited else None, limiter=limiter)
    pieces = [v.clone() for _, v in f]
    assert len(pieces) >= 3 and torch.equal(torch.cat(pieces, 1), f.pcm)
    env = wire.Envelope(st.frame_gain, st.spf)
    xm = torch.from_numpy(gain_ref.shaped(plain.o[0, 0].cpu().numpy(), G[0], st.spf)).cuda().view(1, 1, -1)
    kw = dict(limiter=limiter, peak=peak) if limited else dict(auto_normalize=False)
    a = wire.service_pcm16(net, plain.o, st.y_lengths, MODEL_SR, RATE, envelope=env, **kw)
    b = wire.service_pcm16(net, xm, st.y_lengths, MODEL_SR, RATE, **kw)
    unshaped = wire.service_pcm16(net, plain.o, st.y_lengths, MODEL_SR, RATE, **kw)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and not torch.equal(a[0], unshaped[0])
    assert torch.equal(f.pcm, a[0]) and torch.equal(f.valid_samples, a[1])
    # the running peak is the shaped signal's, and auto_normalize divides by it
    ref = wire.stream_pcm16(net, net.dec_stream(plain.z.clone(), None, 8, 16), MODEL_SR, RATE)
    ref_m = wire.PcmStream(net, net.dec_stream(plain.z.clone(), None, 8, 16), MODEL_SR, RATE, envelope=env)
    ref.run(), ref_m.run()
    assert not torch.equal(ref.peak, ref_m.peak)
    if limited:
        assert int(f.pcm.abs().max()) <= int(np.floor(float(np.float32(0.9)) * 32767)) + 1
        auto_a = wire.service_pcm16(net, plain.o, st.y_lengths, MODEL_SR, RATE, envelope=env, encoding="ulaw")
        auto_b = wire.service_pcm16(net, xm, st.y_lengths, MODEL_SR, RATE, encoding="ulaw")
        assert torch.equal(auto_a[0], auto_b[0]) and torch.equal(auto_a[1], auto_b[1])


def _request(gain=None, T=T_TEXT, seed=SEED, marks=False):
    return Request(_ids(T, seed), seed=seed, gain=gain, marks=marks, **KW)


def test_pooled_admission_is_bitwise_the_stand_alone_streams():
    net = _mini()
    alone = [_stream(net, GAINS), _stream(net, None, T=9, seed=SEED + 1)]
    enc = net.encoder_runs()
    net.infer_streams([_request(), _request(T=9, seed=SEED + 1)])
    enc_plain = net.encoder_runs() - enc
    runs, enc = net.gain_runs(), net.encoder_runs()
    sts = net.infer_streams([_request(GAINS), _request(T=9, seed=SEED + 1)])
    assert net.gain_runs() - runs == 1 and net.encoder_runs() - enc == enc_plain
    for st, ref in zip(sts, alone):
        assert torch.equal(st.z, ref.z) and torch.equal(st.y_lengths, ref.y_lengths)
    assert sts[1].frame_gain is None
    assert torch.equal(sts[0].frame_gain.view(torch.int32), alone[0].frame_gain.view(torch.int32))
    runs = net.gain_runs()
    net.infer_streams([_request(), _request(T=9, seed=SEED + 1)])
    assert net.gain_runs() == runs                                        # no request carries a gain: no launch
    # two shaped requests of one run: still one launch
    runs = net.gain_runs()
    both = net.infer_streams([_request(GAINS), _request(GAINS[:9], T=9, seed=SEED + 1, marks=True)])
    assert net.gain_runs() - runs == 1
    F = both[1].z.shape[2]
    assert np.array_equal(both[1].frame_gain[0].cpu().numpy(), gain_ref.frame_gain_of_marks(GAINS[:9], both[1].marks, F))


def test_pool_and_turn_pick_the_envelope_up_by_themselves():
    net = _mini()
    plain, G, _, peak = _e2e()
    limiter = wire.Limiter(0.9, lookahead_ms=1.0, hold_ms=2.0)
    want = wire.stream_pcm16(net, _stream(net, GAINS), MODEL_SR, RATE, peak=peak, limiter=limiter)
    want.run()
    want2 = wire.stream_pcm16(net, _stream(net, None, T=9, seed=SEED + 1), MODEL_SR, RATE, peak=peak, limiter=limiter)
    want2.run()
    pp = wire.pcm_pool(net, net.stream_pool(), MODEL_SR, RATE)
    fs = pp.admit([_request(GAINS), _request(T=9, seed=SEED + 1)], peak=peak, limiter=limiter)
    assert fs[0]._env is not None and fs[1]._env is None
    runs, ticks = wire.wire_runs(net), 0
    while len(pp):
        pp.step()
        ticks += 1
        assert ticks < 100
    assert wire.wire_runs(net) - runs <= ticks                           # shaped and unshaped members: one launch a tick
    assert torch.equal(fs[0].pcm, want.pcm) and torch.equal(fs[1].pcm, want2.pcm)
    assert torch.equal(fs[0].peak.view(torch.int32), want.peak.view(torch.int32))
    # a turn: the shaped phrase, a pause, the plain one
    pp = wire.pcm_pool(net, net.stream_pool(), MODEL_SR, RATE)
    turn = pp.add_turn(1 << 17, peak=peak, limiter=limiter)
    sts = turn.admit([_request(GAINS), _request(T=9, seed=SEED + 1)], pauses_ms=[0.0, 80.0])
    turn.close()
    assert turn.envelopes[0] is not None and turn.envelopes[1] is None
    ticks = 0
    while not turn.finished:
        pp.step()
        ticks += 1
        assert ticks < 100
    lengths = [min(256 * st.z.shape[2], st.o.shape[-1]) for st in sts]
    assert torch.equal(sts[0].o, plain.o)
    shaped0 = torch.from_numpy(gain_ref.shaped(plain.o[0, 0, :lengths[0]].cpu().numpy(), G[0], sts[0].spf)).cuda()
    row = wire.assemble_turn([shaped0, sts[1].o], lengths, [round(80.0 * 1e-3 * MODEL_SR)], turn.ramp)
    ref = _ranged(net, row, None, MODEL_SR, RATE, turn._lim, "pcm16", None, peak=peak)
    total = int(ref[1])
    assert torch.equal(turn.pcm[:, :total], ref[0]) and torch.equal(turn.valid_samples, ref[1])
    assert torch.equal(turn.peak.view(torch.int32), ref[2].view(torch.int32))


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_refused_calls_launch_nothing_and_the_handle_serves_on():
    orig, target = 22050, 24000
    net, x, valid = _case(orig, target)[:3]
    n, hop = x.shape[-1], 256
    width = wire.resample_ready(orig, target, n, n)
    G = torch.from_numpy(_tables(hop)).cuda()
    env = wire.Envelope(G, hop)
    want = _ranged(net, x, valid, orig, target, LIMIT, "pcm16", None, env=env)
    pcm = torch.full((3, width), SENTINEL, device="cuda", dtype=torch.int16)
    inv = float(np.float32(1.0) / np.float32(hop))
    runs, gruns = wire.wire_runs(net), net.gain_runs()

    def raw(e, stride, B=3):
        net._call("mbv_resample_pcm16_range_shaped", x, valid, B, n, orig, target, 0, n, 0, width, None, pcm,
                  pcm.stride(0), None, None, None, 0, None, C.byref(e), stride)

    E = _capi.MbvPcmEnvelope
    bad = [(E(G.data_ptr(), 7, hop, inv), 9),                             # frames * hop < in_total
           (E(G.data_ptr(), 8, 0, 0.0), 9), (E(G.data_ptr(), 8, -3, inv), 9),            # hop < 1
           (E(G.data_ptr(), 0, hop, inv), 9),                             # no frames
           (E(G.data_ptr(), 8, hop, float(np.nextafter(np.float32(inv), np.float32(1)))), 9),   # not 1.0f / hop
           (E(None, 8, hop, inv), 0), (E(None, 0, 0, 0.0), 9),            # a NULL gain with sibling fields / a stride
           (E(G.data_ptr(), 8, hop, inv), 8), (E(G.data_ptr(), 8, hop, inv), 0)]         # rows would overlap
    for e, stride in bad:
        with pytest.raises(_capi.MbvError):
            raw(e, stride)
    with pytest.raises(_capi.MbvError):                                   # whatever the unshaped entry refuses
        net.resample_pcm16_range(x, orig, target, n - 500, 0, width, pcm, valid_samples=valid, envelope=env)
    # the Python layer refuses the same before the library is asked
    for e in (wire.Envelope(G[:, :8], hop), wire.Envelope(G[:2], hop), wire.Envelope(G, hop - 7)):
        with pytest.raises(ValueError):
            net.resample_pcm16_range(x, orig, target, n, 0, width, pcm, valid_samples=valid, envelope=e)
    with pytest.raises(TypeError):
        net.resample_pcm16_range(x, orig, target, n, 0, width, pcm, valid_samples=valid, envelope=G)
    # pooled and turn entries: a bad table row refuses the call
    xb, vb = x[0, 0].contiguous(), valid[:1].clone()
    one = torch.full((width,), SENTINEL, device="cuda", dtype=torch.int16)
    chunk = _chunk(xb, vb, n, 0, width, one, torch.zeros(1, device="cuda"), None, None)
    ev = (E * 1)(E(G.data_ptr(), 7, hop, inv))
    with pytest.raises(_capi.MbvError):
        net._call("mbv_resample_pcm16_chunks_shaped", (_capi.MbvPcmChunk * 1)(chunk), None, None, ev, 1, orig, target,
                  0, 0, None, 0)
    with pytest.raises(ValueError):
        net.resample_pcm16_chunks([chunk], orig, target, envelopes=[wire.Envelope(G[0, :8], hop)])
    with pytest.raises(ValueError):
        net.resample_pcm16_chunks([chunk], orig, target, envelopes=[None, wire.Envelope(G[0], hop)])
    # gains on the device, and of the wrong length, are refused by every entry that takes them
    ids = _ids(5, 1).view(1, -1).cuda()
    mini = _mini()
    mruns = mini.gain_runs()
    with pytest.raises(TypeError):
        mini.infer_stream(ids, torch.tensor([5]).cuda(), None, gain=torch.ones(1, 5).cuda())
    with pytest.raises(TypeError):
        Request(_ids(5, 1), gain=torch.ones(5).cuda())
    with pytest.raises(ValueError):
        mini.infer_stream(ids, torch.tensor([5]).cuda(), None, gain=[[1.0] * 4])
    with pytest.raises(ValueError):
        mini.infer_stream(ids, torch.tensor([5]).cuda(), None, gain=[[1.0, 1.0, 17.0, 1.0, 1.0]])
    with pytest.raises(_capi.MbvError):
        mini._call("mbv_frame_gain", torch.ones(1, 5).cuda(), torch.ones(1, 3).cuda(), 3, 7)    # out_stride < frames + 1
    assert wire.wire_runs(net) == runs and net.gain_runs() == gruns and mini.gain_runs() == mruns
    assert (pcm == SENTINEL).all() and (one == SENTINEL).all()
    # ... and the handle serves the next call
    assert _same(_ranged(net, x, valid, orig, target, LIMIT, "pcm16", None, env=env), want)
