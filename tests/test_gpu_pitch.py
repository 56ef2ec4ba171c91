"""-m gpu: per-token pitch end to end on ljs_mini_mb_istft_vits: `infer_stream(pitch=)`, `Request(pitch=)`,
`stream_pcm16`, `PcmPool.admit`, `Turn.admit` and `revoke` over a pitched stream.  Every relation is BITWISE: the
streamed, the pooled and the turn's bytes are those of the existing one-shot chain on `net.warp(o, st.warp)`, and a
stream without `pitch=` is what it was."""
import numpy as np
import pytest
import torch

from mb_istft_vits_amd import stream, wire
from mb_istft_vits_amd.models import Request

import gain_ref
import warp_ref
from test_gpu_turns import MODEL_SR, RATE, _ids, _net as _mini      # (ljs_mini_mb_istft_vits)

pytestmark = pytest.mark.gpu

T, SEED, SCALE = 14, 71, 2.5
PITCH = [1.0, 1.0, 1.26, 1.26, 1.5, 2.0, 0.5, 0.8, 0.8, 1.0, 1.12, 0.9, 1.0, 1.0]
GAINS = [1.0, 0.5, 0.5, 2.0, 2.0, 1.0, 0.0, 1.0, 3.0, 1.0, 1.0, 0.25, 1.0, 1.0]
KW = dict(noise_scale=0.5, chunk_frames=8, max_chunk_frames=16)
_REF = {}


def _stream(net, pitch=PITCH, T=T, seed=SEED, length_scale=SCALE, chunk=8, cap=16, **kw):
    x = _ids(T, seed).view(1, -1).cuda()
    return net.infer_stream(x, torch.tensor([T]).cuda(), None, noise_scale=0.5, length_scale=length_scale, seed=[seed],
                            chunk_frames=chunk, max_chunk_frames=cap, pitch=None if pitch is None else [pitch[:T]], **kw)


def _request(pitch=PITCH, T=T, seed=SEED, **kw):
    return Request(_ids(T, seed), length_scale=SCALE, seed=seed, pitch=None if pitch is None else pitch[:T], **KW, **kw)


def _full(net):
    """the pitched request decoded in one piece, and its warped wave [1, 1, n_out]: once"""
    if "full" not in _REF:
        st = _stream(net, chunk=256, cap=256)
        assert len(st.schedule) == 1
        st.run()
        _REF["full"] = (st, net.warp(st.o, st.warp)[:, None, :].contiguous())
    return _REF["full"]


def _play(ps):
    pieces = [(a, v.clone()) for a, v in ps]
    assert pieces[0][0] == 0 and all(a + v.shape[1] == b for (a, v), (b, _) in zip(pieces, pieces[1:]))
    return pieces


def _same(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


# ------------------------------------------------------------------------------------------------ the stream itself
def test_the_decode_is_untouched_and_the_map_is_the_restatement():
    net = _mini()
    enc, runs = net.encoder_runs(), net.warp_runs()
    st = _stream(net)
    assert net.encoder_runs() - enc == 1 and net.warp_runs() == runs          # the marks ride along; nothing is warped yet
    assert len(st.schedule) >= 3 and isinstance(st.warp, stream.WarpMap) and st.marks is not None
    F = st.z.shape[2]
    assert st.warp.frames == F and st.warp.hop == st.spf and st.warp.samples == st.o.shape[-1]
    R = warp_ref.glide(warp_ref.frame_rates(np.asarray(PITCH, np.float32), st.marks, F), 2)
    U, n_out = warp_ref.plan(R, st.spf)
    assert np.array_equal(st.warp.rate.view(np.int32), R.view(np.int32)) and np.array_equal(st.warp.U, U)
    assert st.warp.n_out == n_out and np.array_equal(st.warp.rate_dev.cpu().numpy(), R)
    assert np.array_equal(st.warp.U_dev.cpu().numpy(), U)
    # pitch_compensate: the effective length_scale is fl32(s) * p as a tensor, nothing else changes: bitwise z and o
    eff = torch.tensor([PITCH]) * torch.tensor(SCALE, dtype=torch.float32)
    plain = _stream(net, None, length_scale=eff)
    assert plain.warp is None and plain.z.shape == st.z.shape and _same(plain.z, st.z)
    st.run(), plain.run()
    assert _same(plain.o, st.o)
    # plain varispeed: the stream of the scalar length_scale, warped
    vs = _stream(net, pitch_compensate=False)
    base = _stream(net, None)
    assert _same(vs.z, base.z) and vs.warp is not None and vs.warp.n_out != vs.o.shape[-1]
    steps = _stream(net, pitch_glide_frames=0)
    assert set(np.unique(steps.warp.rate)) <= set(np.float32(PITCH))
    # without pitch= nothing is planned
    assert base.warp is None and base.marks is None
    with pytest.raises(TypeError):                                            # a device tensor is refused
        net.infer_stream(_ids(T, SEED).view(1, -1).cuda(), torch.tensor([T]).cuda(), None, pitch=torch.ones(1, T).cuda())


# ------------------------------------------------------------------------------------------------ streamed = one-shot
@pytest.mark.parametrize("kind", ["plain", "limited", "ulaw"])
def test_the_streamed_wire_is_the_one_shot_chain_on_the_warped_wave(kind):
    net = _mini()
    full, warped = _full(net)
    rate = 8000 if kind == "ulaw" else RATE
    limiter = wire.Limiter(0.9, lookahead_ms=1.0, hold_ms=2.0) if kind == "limited" else None
    encoding = "ulaw" if kind == "ulaw" else "pcm16"
    peak = 0.05 if kind == "limited" else None
    st = _stream(net)
    assert len(st.schedule) >= 3
    runs, wruns = net.warp_runs(), wire.wire_runs(net)
    ps = wire.stream_pcm16(net, st, MODEL_SR, rate, peak=peak, limiter=limiter, encoding=encoding)
    pieces = _play(ps)
    assert len(pieces) == len(st.schedule)
    assert 1 <= net.warp_runs() - runs <= len(st.schedule)                    # one warp launch in front of a wire step
    assert wire.wire_runs(net) - wruns == len(st.schedule)                    # the wire steps of a stream without pitch
    assert _same(ps._warp.row, warped[:, 0]) and _same(st.o, full.o)
    ref, ref_valid = wire.service_pcm16(net, warped, None, MODEL_SR, rate, auto_normalize=False, limiter=limiter,
                                        peak=peak, encoding=encoding)
    assert torch.equal(ps.valid_samples, ref_valid)
    assert int(ref_valid[0]) == wire.resample_ready(MODEL_SR, rate, st.warp.n_out, st.warp.n_out)
    assert torch.equal(ps.pcm, ref) and torch.equal(torch.cat([v for _, v in pieces], dim=1), ref)
    # the running peak: that of the resampled warped wave
    wave, valid = net.resample(warped, MODEL_SR, rate)
    if kind != "limited":
        assert _same(ps.peak, wave[0, 0, :int(valid[0])].abs().max().reshape(1))
    # the marks go through the warp
    assert ps.marks == wire.mark_samples(st.marks, st.spf, MODEL_SR, rate, ps._lim[1] if ps._lim else 0, warp=st.warp)


def test_gain_and_pitch_compose():
    net = _mini()
    full, _ = _full(net)
    st = _stream(net, gain=[GAINS])
    assert st.frame_gain is not None and st.warp is not None
    ps = wire.stream_pcm16(net, st, MODEL_SR, RATE)
    assert ps._env is None and ps._warp.env is not None                       # the envelope is handed to the warp
    ps.run()
    assert _same(st.o, full.o)
    G = st.frame_gain[0].cpu().numpy()
    shaped = torch.from_numpy(gain_ref.shaped(full.o[0, 0].cpu().numpy(), G, st.spf)).cuda()
    composed = net.warp(shaped, st.warp)[:, None, :].contiguous()             # warp(o * e)
    assert _same(net.warp(full.o, st.warp, envelope=wire.Envelope(st.frame_gain[0], st.spf))[:, None, :], composed)
    ref, ref_valid = wire.service_pcm16(net, composed, None, MODEL_SR, RATE, auto_normalize=False)
    assert torch.equal(ps.pcm, ref) and torch.equal(ps.valid_samples, ref_valid)


# ------------------------------------------------------------------------------------------------ pooled
def test_pooled_streams_are_their_stand_alone_streams_with_one_warp_launch_a_tick():
    net = _mini()
    specs = [(PITCH, T, SEED), (None, 12, SEED + 1), (PITCH[::-1] + [1.0, 1.3], 16, SEED + 2), (None, T, SEED + 3),
             ([1.5] * 20, 20, SEED + 4)]
    alone = []
    for p, t, seed in specs:
        ps = wire.stream_pcm16(net, _stream(net, p, T=t, seed=seed), MODEL_SR, RATE)
        ps.run()
        alone.append(ps)
    # the plain ones are what they are without the feature: a stream opened without pitch=
    for (p, t, seed), ps in zip(specs, alone):
        if p is None:
            x = _ids(t, seed).view(1, -1).cuda()
            old = wire.stream_pcm16(net, net.infer_stream(x, torch.tensor([t]).cuda(), None, noise_scale=0.5,
                                                           length_scale=SCALE, seed=[seed], chunk_frames=8,
                                                           max_chunk_frames=16), MODEL_SR, RATE)
            old.run()
            assert ps._warp is None and torch.equal(ps.pcm, old.pcm) and _same(ps.peak, old.peak)

    def drive(reqs):
        pp = wire.pcm_pool(net, net.stream_pool(), MODEL_SR, RATE)
        enc = net.encoder_runs()
        fs = pp.admit(reqs)
        enc = net.encoder_runs() - enc
        ticks, warps, wires = 0, [], []
        while len(pp):
            w0, r0 = net.warp_runs(), wire.wire_runs(net)
            pp.step()
            warps.append(net.warp_runs() - w0)
            wires.append(wire.wire_runs(net) - r0)
            ticks += 1
            assert ticks < 100
        return fs, warps, wires, enc

    fs, warps, wires, enc = drive([_request(p, T=t, seed=seed) for p, t, seed in specs])
    assert max(warps) == 1 and sum(warps) >= 3                                # ONE warp launch per tick for all members
    for f, ps, (p, _, _) in zip(fs, alone, specs):
        assert (f._warp is not None) == (p is not None)
        assert torch.equal(f.pcm, ps.pcm) and torch.equal(f.valid_samples, ps.valid_samples) and _same(f.peak, ps.peak)
        assert _same(f._st.o, ps._st.o)
    # the same five requests without pitch: the wire launches per tick and the encoder runs are those
    _, warps0, wires0, enc0 = drive([Request(_ids(t, seed), length_scale=SCALE, seed=seed, **KW) for _, t, seed in specs])
    assert sum(warps0) == 0 and enc == enc0
    assert max(wires) == max(wires0) == 1


# ------------------------------------------------------------------------------------------------ a turn
def test_a_turn_with_a_pitched_segment_is_the_assembled_timeline():
    net = _mini()
    full, warped = _full(net)
    pp = wire.pcm_pool(net, net.stream_pool(), MODEL_SR, RATE)
    turn = pp.add_turn(1 << 17)
    sts = turn.admit([_request(), _request(None, T=9, seed=SEED + 1)], pauses_ms=[0.0, 80.0])
    turn.close()
    assert turn.warped[0] is not None and turn.warped[1] is None
    ticks, warps = 0, 0
    while not turn.finished:
        w0 = net.warp_runs()
        pp.step()
        assert net.warp_runs() - w0 <= 1
        warps += net.warp_runs() - w0
        ticks += 1
        assert ticks < 100
    assert warps >= 1 and _same(sts[0].o, full.o) and _same(turn.warped[0].row, warped[:, 0])
    plain = _stream(net, None, T=9, seed=SEED + 1)
    plain.run()
    assert _same(sts[1].o, plain.o)
    lengths = [sts[0].warp.n_out, min(256 * sts[1].z.shape[2], sts[1].o.shape[-1])]
    row = wire.assemble_turn([warped[0, 0], plain.o], lengths, [round(80.0 * 1e-3 * MODEL_SR)], turn.ramp)
    n = row.shape[-1]
    width = wire.resample_ready(MODEL_SR, RATE, n, n)
    out = torch.zeros(1, width, device="cuda", dtype=torch.int16)
    ns = torch.zeros(1, device="cuda", dtype=torch.int64)
    running = torch.zeros(1, device="cuda")
    net.resample_pcm16_range(row, MODEL_SR, RATE, n, 0, width, out, running_peak=running, out_samples=ns)
    total = int(ns[0])
    assert torch.equal(turn.pcm[:, :total], out[:, :total]) and torch.equal(turn.valid_samples, ns)
    assert _same(turn.peak, running)
    assert turn.marks[0] == wire.mark_samples(sts[0].marks, sts[0].spf, MODEL_SR, RATE, warp=sts[0].warp)


# ------------------------------------------------------------------------------------------------ barge-in
def test_revoke_at_a_token_on_a_pitched_stream():
    net = _mini()
    full, warped = _full(net)
    st = _stream(net, marks=True)
    ps = wire.stream_pcm16(net, st, MODEL_SR, RATE)
    a0, first_piece = next(ps)
    E = a0 + first_piece.shape[1]
    rep = ps.revoke(fade_ms=5.0, at="token")
    N = int(round(5.0 * RATE / 1000))
    marks = wire.mark_samples(st.marks, st.spf, MODEL_SR, RATE, warp=st.warp)
    F = next(m for m in marks if m >= E)
    assert ps.marks == marks and (rep.first, rep.count) == (F, N)             # the fade starts at the mapped mark
    assert rep.tokens_started == sum(1 for m in marks[:-1] if m < F)
    for _ in ps:
        pass
    assert ps.finished and ps.revoked
    ref, ref_valid = wire.service_pcm16(net, warped, None, MODEL_SR, RATE, auto_normalize=False, fade=(F, N))
    cut = int(ref_valid[0])
    assert cut == int(ps.valid_samples[0]) == rep.valid_samples == min(F + N, wire.resample_ready(
        MODEL_SR, RATE, st.warp.n_out, st.warp.n_out))
    assert torch.equal(ps.pcm[:, :cut], ref[:, :cut])
