"""-m gpu: ITU-R BS.1770 loudness on the device (`mbv_loudness`, `mbv_loudness_range`,
`mbv_loudness_chunks`, `net.loudness`, `wire.Loudness`).  The kernel is pinned to the float64 restatement of the
standard (tests/loudness_ref.py: sequential, direct form I, no segment chain) within 0.01 LU and 1e-4 in every segment
energy; every relation between the one-shot, ranged, pooled, streamed and live forms is bitwise."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from mb_istft_vits_amd import _capi, wire
from mb_istft_vits_amd.models import Request

import loudness_cases
from test_gpu_limiter import LIM, RATE, _again, _drive_live, _live_inputs, _net, _text_stream
from test_gpu_live_wire import MODEL_SR, _cuts, _open, _text_batch

pytestmark = pytest.mark.gpu

L_TOL = 0.01             # LU: a tenth of EBU Tech 3341's meter tolerance, about 0.1 % in gain
E_RTOL = 1e-4            # segment energies, relative: 25 times inside the loudness bar
E_FLOOR, E_ATOL = 1e-12, 1e-16
MEASURE = wire.Loudness(target=None)


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int64) if t.dtype == torch.float64 else t


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _case(fs):
    c = loudness_cases.case(fs)
    x = torch.from_numpy(c["x"]).cuda()[:, None, :].contiguous()
    valid = torch.tensor(c["valid"], dtype=torch.int64).cuda()
    return c, x, valid


def _fresh(B, segs):
    return (torch.full((B, 4), 7.5, device="cuda", dtype=torch.float64),
            torch.full((B, segs), -1.0, device="cuda", dtype=torch.float64),
            torch.full((B,), 123.0, device="cuda", dtype=torch.float32))


def _ranged(net, x, valid, fs, cuts, avail=None):
    """the ranged entry over every segment of the rows, cut at `cuts`; -> (L, energies, state, launches)"""
    B, n = x.shape[0], x.shape[-1]
    H, segs = _capi.loudness_segments(fs, n)
    state, energies, L = _fresh(B, segs)
    runs, done = net.loudness_runs(), 0
    for k in sorted(set(cuts) | {segs}):
        net.loudness_range(x, fs, n if avail is None else avail(k), done, k - done, state, energies, L, valid_samples=valid)
        done = k
    return L, energies, state, net.loudness_runs() - runs


# ------------------------------------------------------------------------------------------------ 1. the definition
@pytest.mark.parametrize("fs", loudness_cases.RATES)
def test_loudness_and_energies_against_the_float64_reference(fs):
    net = _net()
    c, x, valid = _case(fs)
    refs = dict(zip(c["names"], c["ref"]))
    # the condition of the comparison, on the reference: both gates drop blocks, none within MARGIN of a threshold
    a, b = refs["a"], refs["b"]
    assert a["abs_keep"].all() and 0 < a["keep"].sum() < len(a["keep"])              # the relative gate drops blocks
    assert 0 < b["abs_keep"].sum() < len(b["abs_keep"])                              # the absolute gate drops blocks
    for name, r in refs.items():
        d_abs, d_rel = loudness_cases.margins(r)
        assert d_abs >= loudness_cases.MARGIN and d_rel >= loudness_cases.MARGIN, (fs, name, d_abs, d_rel)
    assert [len(refs[k]["l"]) for k in ("s3", "s4", "s5m")] == [0, 1, 1]
    runs = net.loudness_runs()
    L, E = net.loudness(x, fs, valid_samples=valid, return_energies=True)
    assert net.loudness_runs() - runs == 1                                           # one launch for the batch
    assert L.dtype == torch.float32 and E.dtype == torch.float64 and E.shape == (6, (3 * fs + 137) // refs["a"]["hop"])
    L, E = L.cpu().numpy(), E.cpu().numpy()
    worst_l = worst_e = worst_abs = 0.0
    for i, (name, r) in enumerate(refs.items()):
        S = len(r["energies"])
        assert (E[i, S:] == 0.0).all(), (fs, name)                                   # absent segments
        if math.isinf(r["L"]):
            assert L[i] == -np.inf and np.isneginf(L[i]), (fs, name, L[i])
        else:
            worst_l = max(worst_l, abs(float(L[i]) - r["L"]))
        big = r["energies"] >= E_FLOOR
        if big.any():
            worst_e = max(worst_e, float(np.max(np.abs(E[i, :S][big] - r["energies"][big]) / r["energies"][big])))
        if (~big).any():
            worst_abs = max(worst_abs, float(np.max(np.abs(E[i, :S][~big] - r["energies"][~big]))))
    print("loudness fs=%d: max |L - ref| = %.3e LU, max energy error = %.3e relative, %.3e absolute below the floor"
          % (fs, worst_l, worst_e, worst_abs))
    assert worst_l <= L_TOL and worst_e <= E_RTOL and worst_abs <= E_ATOL
    # without the energies, and by frames: the same bits
    assert _same(net.loudness(x, fs, valid_samples=valid), torch.from_numpy(L).cuda())
    frames = torch.tensor([v // 256 for v in c["valid"]]).cuda()
    by_frames = net.loudness(x, fs, y_lengths=frames)
    assert _same(by_frames, net.loudness(x, fs, valid_samples=frames * 256))


# ------------------------------------------------------------------------------------------------ 2. chunk invariance
@pytest.mark.parametrize("fs", loudness_cases.RATES)
def test_ranged_calls_are_bitwise_the_one_shot_however_the_segments_are_cut(fs):
    net = _net()
    c, x, valid = _case(fs)
    H, segs = _capi.loudness_segments(fs, x.shape[-1])
    L1, E1 = net.loudness(x, fs, valid_samples=valid, return_energies=True)
    L0, E0, S0, runs = _ranged(net, x, valid, fs, [])
    assert runs == 1 and _same(L0, L1) and _same(E0, E1)
    assert bool((S0 != 7.5).all())                                                   # the end state was written
    rs = np.random.RandomState(fs)
    schedules = [list(range(1, segs)), [segs - 1], [1], [3, 4, 5]]                   # one at a time; the last segment
    schedules += [sorted(rs.choice(np.arange(1, segs), size=int(rs.randint(2, 9)), replace=False).tolist())
                  for _ in range(5)]
    for cuts in schedules:
        # every step sees only the samples that complete its range: the frontier is part of what is cut
        for avail in (None, lambda k: min(k * H + (H - 1 if k < segs else 137), x.shape[-1])):
            L, E, S, runs = _ranged(net, x, valid, fs, cuts, avail)
            assert runs == len(set(cuts) | {segs})
            assert _same(L, L1) and _same(E, E1) and _same(S, S0), (fs, cuts)


def _chunk(x_row, valid_row, avail, first, count, state, energies, L):
    k = _capi.MbvLoudnessChunk()
    k.wave, k.in_total, k.in_avail = x_row.data_ptr(), x_row.numel(), avail
    k.valid_samples = valid_row.data_ptr() if valid_row is not None else None
    k.seg_first, k.seg_count = first, count
    k.state, k.energies, k.energy_capacity, k.loudness = state.data_ptr(), energies.data_ptr(), energies.numel(), L.data_ptr()
    return k


@pytest.mark.parametrize("fs", loudness_cases.RATES)
def test_pooled_rows_at_different_stages_share_one_launch(fs):
    net = _net()
    c, x, valid = _case(fs)
    B, n = x.shape[0], x.shape[-1]
    H, segs = _capi.loudness_segments(fs, n)
    L1, E1 = net.loudness(x, fs, valid_samples=valid, return_energies=True)
    _, _, S1, _ = _ranged(net, x, valid, fs, [])
    rows = [x[b, 0] for b in range(B)]
    bufs = [_fresh(1, segs) for _ in range(B)]
    # stage of every row before the shared launches: untouched, one segment in, half way, all but one, ...
    stage = [0, 1, segs // 2, segs - 1, 2, 0]
    for b, k in enumerate(stage):
        if k:
            net.loudness_chunks([_chunk(rows[b], valid[b:b + 1], n, 0, k, *bufs[b])], fs)
    mid = [min(k + 7, segs) for k in stage]
    runs = net.loudness_runs()
    net.loudness_chunks([_chunk(rows[b], valid[b:b + 1], n, stage[b], mid[b] - stage[b], *bufs[b]) for b in range(B)], fs)
    assert net.loudness_runs() - runs == 1
    # the next tick: the rows that are done have nothing to add and ride along with a count of 0
    net.loudness_chunks([_chunk(rows[b], valid[b:b + 1], n, mid[b], segs - mid[b], *bufs[b]) for b in range(B)], fs)
    assert net.loudness_runs() - runs == 2
    for b in range(B):
        S, E, L = bufs[b]
        assert _same(L, L1[b:b + 1]) and _same(E, E1[b:b + 1]) and _same(S, S1[b:b + 1]), (fs, b)
    # nothing to do: no launch, nothing counted
    runs = net.loudness_runs()
    net.loudness_chunks([], fs)
    net.loudness_chunks([_chunk(rows[0], None, n, segs, 0, *bufs[0])], fs)
    assert net.loudness_runs() == runs


def test_a_table_longer_than_one_upload_launch():
    """33 rows: the table goes up in two launches; an offset wrong in the second shows in row 32."""
    net = _net()
    fs = 8000
    c, x, valid = _case(fs)
    n = x.shape[-1]
    H, segs = _capi.loudness_segments(fs, n)
    L1, E1 = net.loudness(x, fs, valid_samples=valid, return_energies=True)
    bufs = [_fresh(1, segs) for _ in range(33)]
    runs = net.loudness_runs()
    net.loudness_chunks([_chunk(x[k % 6, 0], valid[k % 6:k % 6 + 1], n, 0, segs, *bufs[k]) for k in range(33)], fs)
    assert net.loudness_runs() - runs == 1
    for k in range(33):
        assert _same(bufs[k][2], L1[k % 6:k % 6 + 1]) and _same(bufs[k][1], E1[k % 6:k % 6 + 1]), k


# ------------------------------------------------------------------------------------------------ 3. what is read
@pytest.mark.parametrize("poison", [float("nan"), 1e30])
def test_nothing_behind_the_valid_length_or_the_last_complete_segment_is_read(poison):
    net = _net()
    fs = 22050
    c, x, valid = _case(fs)
    H, segs = _capi.loudness_segments(fs, x.shape[-1])
    L1, E1 = net.loudness(x, fs, valid_samples=valid, return_energies=True)
    bad = x.clone()
    for b, v in enumerate(c["valid"]):
        bad[b, 0, v // H * H:] = poison             # behind the last complete segment, which includes behind valid
    L, E = net.loudness(bad, fs, valid_samples=valid, return_energies=True)
    assert _same(L, L1) and _same(E, E1)
    only_valid = x.clone()
    for b, v in enumerate(c["valid"]):
        only_valid[b, 0, v:] = poison
    assert _same(net.loudness(only_valid, fs, valid_samples=valid), L1)
    # a ranged step reads nothing at or past the last complete segment of ITS frontier
    state, energies, L = _fresh(6, segs)
    k = 11
    early = x.clone()
    early[:, :, k * H:] = poison
    net.loudness_range(early, fs, k * H + H - 1, 0, k, state, energies, L, valid_samples=valid)
    net.loudness_range(x, fs, x.shape[-1], k, segs - k, state, energies, L, valid_samples=valid)
    assert _same(L, L1) and _same(energies, E1)


# ------------------------------------------------------------------------------------------------ 4. refusals
def test_refusals_launch_nothing():
    net = _net()
    fs = 8000
    c, x, valid = _case(fs)
    n = x.shape[-1]
    H, segs = _capi.loudness_segments(fs, n)
    state, energies, L = _fresh(6, segs)
    runs = net.loudness_runs()
    with pytest.raises(ValueError, match="at least 1000 Hz"):
        net.loudness(x, 999)
    with pytest.raises(_capi.MbvError, match="at least 1000 Hz"):
        net.loudness_range(x, 999, n, 0, 1, state, energies, L)
    net.loudness_range(x, fs, n, 0, 0, state, energies, L)                         # these buffers start over
    with pytest.raises(_capi.MbvError, match="next segment is 0"):                 # nothing measured yet
        net.loudness_range(x, fs, n, 2, 3, state, energies, L)
    with pytest.raises(_capi.MbvError, match="hold only 10 complete segments"):
        net.loudness_range(x, fs, 11 * H - 1, 0, 11, state, energies, L)
    with pytest.raises(_capi.MbvError, match="outside the energies"):
        net.loudness_range(x, fs, n, 0, segs, state, energies[:, :segs - 1].contiguous(), L)
    h, lib, s = net._ensure_handle(), _capi.lib(), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for st, en in ((None, energies), (state, None)):
        rc = lib.mbv_loudness_range(h, x.data_ptr(), None, 6, n, fs, n, 0, segs, st.data_ptr() if st is not None else None,
                                    en.data_ptr() if en is not None else None, segs, L.data_ptr(), s)
        assert rc != 0 and b"state / energies missing" in lib.mbv_last_error(h)
    k = _chunk(x[0, 0], None, n, 0, segs, state[:1], energies[:1], L[:1])
    k.state = None
    with pytest.raises(_capi.MbvError, match="chunk 0: state / energies / loudness missing"):
        net.loudness_chunks([k], fs)
    assert net.loudness_runs() == runs
    torch.cuda.synchronize()
    assert bool((state == 7.5).all()) and bool((energies == -1.0).all()) and bool((L == 123.0).all())
    # after a step the next one starts where it ended, and nowhere else; 0 starts over
    net.loudness_range(x, fs, n, 0, 5, state, energies, L)
    with pytest.raises(_capi.MbvError, match="next segment is 5"):
        net.loudness_range(x, fs, n, 6, 1, state, energies, L)
    with pytest.raises(_capi.MbvError, match="next segment is 5"):
        net.loudness_range(x, fs, n, 4, 2, state, energies, L)
    assert net.loudness_runs() == runs + 1
    net.loudness_range(x, fs, n, 5, segs - 5, state, energies, L, valid_samples=None)
    net.loudness_range(x, fs, n, 0, segs, state, energies, L, valid_samples=None)
    assert _same(L, net.loudness(x, fs))
    # the Python entries: peak and loudness together, a stream without a measured value
    st = _text_stream(net, 12, 3)
    with pytest.raises(ValueError, match="not both"):
        wire.service_pcm16(net, st.o, None, MODEL_SR, RATE, limiter=LIM, peak=0.5, loudness=wire.Loudness())
    with pytest.raises(ValueError, match="measured"):
        wire.stream_pcm16(net, st, MODEL_SR, RATE, loudness=wire.Loudness())
    with pytest.raises(ValueError, match="not both"):
        wire.stream_pcm16(net, st, MODEL_SR, RATE, peak=0.5, loudness=wire.Loudness(measured=-20.0))
    with pytest.raises(ValueError, match="only measures"):
        wire.service_pcm16(net, st.o, None, MODEL_SR, RATE, loudness=MEASURE)


# ------------------------------------------------------------------------------------------------ 5. streams
def _stream(net, T, seed, sched):
    x, xl, sid = _text_batch(net, 1, T, seed)
    return net.infer_stream(x, xl, sid, noise_scale=0.5, chunk_frames=sched[0], max_chunk_frames=sched[1], seed=[seed])


@pytest.mark.parametrize("sched", [(8, 32), (32, 256)])
def test_a_measuring_stream_ends_bitwise_at_the_one_shot_loudness(sched):
    net = _net()
    T, seed = 60, 5
    plain = wire.stream_pcm16(net, _stream(net, T, seed, sched), MODEL_SR, RATE)
    plain_counts = []
    for _ in range(len(plain)):
        w = wire.wire_runs(net)
        next(plain)
        plain_counts.append(wire.wire_runs(net) - w)
    assert plain.loudness is None
    f = wire.stream_pcm16(net, _stream(net, T, seed, sched), MODEL_SR, RATE, loudness=MEASURE)
    st = f._st
    H, segs = _capi.loudness_segments(MODEL_SR, st.o.shape[-1])
    assert segs >= 8, segs
    plan = wire.loudness_plan([st.spf * (a + b) for a, b in st.schedule], H)
    assert float(f.loudness[0]) == -math.inf
    for i in range(len(f)):
        w, d, m = wire.wire_runs(net), net.decoder_runs(), net.loudness_runs()
        next(f)
        assert wire.wire_runs(net) - w == plain_counts[i] and net.decoder_runs() - d == 1
        assert net.loudness_runs() - m == (1 if plan[i][1] > plan[i][0] else 0), (i, plan[i])
    assert plan[-1][1] == int(st.y_lengths[0]) * 256 // H
    want = net.loudness(st.o, MODEL_SR, y_lengths=st.y_lengths)
    print("stream %r: %d segments, L = %.3f LUFS" % (sched, segs, float(want[0])))
    assert math.isfinite(float(want[0])) and _same(f.loudness, want)
    assert torch.equal(f.pcm, plain.pcm) and torch.equal(f.valid_samples, plain.valid_samples)
    assert _same(f.peak, plain.peak)


def test_a_pool_measures_all_its_members_in_one_launch_per_tick():
    net = _net()
    specs = [(60, 5, (8, 32)), (45, 6, (32, 256)), (70, 7, (8, 32)), (50, 8, (8, 32))]
    alone = []
    for T, seed, sched in specs:
        a = wire.stream_pcm16(net, _stream(net, T, seed, sched), MODEL_SR, RATE)
        alone.append(tuple(t.clone() for t in a.run()))
    # the decoder runs of the same pool without measuring
    pp = wire.pcm_pool(net, net.stream_pool(), MODEL_SR, RATE)
    for T, seed, sched in specs:
        pp.add(_stream(net, T, seed, sched))
    d, m = net.decoder_runs(), net.loudness_runs()
    while len(pp):
        pp.step()
    plain_decodes = net.decoder_runs() - d
    assert net.loudness_runs() == m                                                  # nobody asked: nothing launched
    pp = wire.pcm_pool(net, net.stream_pool(), MODEL_SR, RATE)
    fol = [pp.add(_stream(net, T, seed, sched), loudness=MEASURE if k < 3 else None)
           for k, (T, seed, sched) in enumerate(specs)]
    assert fol[3].loudness is None
    d, ticks, measured = net.decoder_runs(), 0, 0
    while len(pp):
        w, m = wire.wire_runs(net), net.loudness_runs()
        before = [f._lseg for f in fol[:3]]
        pp.step()
        ticks += 1
        assert wire.wire_runs(net) - w <= 1
        grew = any(f._lseg > b for f, b in zip(fol[:3], before))
        assert net.loudness_runs() - m == (1 if grew else 0)
        measured += net.loudness_runs() - m
    assert net.decoder_runs() - d == plain_decodes and 0 < measured <= ticks
    for f, (pcm, valid) in zip(fol, alone):
        assert torch.equal(f.pcm, pcm) and torch.equal(f.valid_samples, valid)
    for f in fol[:3]:
        want = net.loudness(f._st.o, MODEL_SR, y_lengths=f._st.y_lengths)
        assert math.isfinite(float(want[0])) and _same(f.loudness, want)
    # admitted requests take loudness= as add does
    x, xl, sid = _text_batch(net, 1, 30, 9)
    pp = wire.pcm_pool(net, net.stream_pool(), MODEL_SR, RATE)
    req = dict(x=x[0, :int(xl[0])], sid=int(sid[0]), noise_scale=0.5, seed=9, chunk_frames=8, max_chunk_frames=32)
    a, b = pp.admit([Request(**req), Request(**req)], loudness=[MEASURE, None])
    while len(pp):
        pp.step()
    assert b.loudness is None and _same(a.loudness, net.loudness(a._st.o, MODEL_SR, y_lengths=a._st.y_lengths))
    assert torch.equal(a.pcm, b.pcm)


def test_a_live_wire_measures_whatever_the_pushes():
    net = _net()
    T, in_sr = 100, 48000
    raw, noise = _live_inputs(net, T, 31)
    plain, _ = _drive_live(net, raw, noise, "one", T, None, None)
    assert plain.loudness is None
    got = []
    for pattern in ("20ms", "random"):
        lw = _open(net, in_sr, RATE, raw.dtype, noise, None, 32, (8, 32), loudness=MEASURE)
        off = 0
        for k in _cuts(net, pattern, in_sr, raw.numel(), T, 32, 1):
            lw.push(raw[off:off + k])
            off += k
            w, m = wire.wire_runs(net), net.loudness_runs()
            lw.poll()
            assert wire.wire_runs(net) - w <= 1 and net.loudness_runs() - m <= 1
        lw.close()
        lw.poll()
        assert lw.finished
        want = net.loudness(lw.live.result(), MODEL_SR, y_lengths=torch.tensor([T]).cuda())
        assert math.isfinite(float(want[0])) and _same(lw.loudness, want), pattern
        assert torch.equal(lw.pcm, plain.pcm) and torch.equal(lw.valid_samples, plain.valid_samples)
        got.append(lw)
    # in a pool: the live member's segments ride in the tick's one launch
    pp = wire.pcm_pool(net, net.stream_pool(), MODEL_SR, RATE)
    f = pp.add(_stream(net, 40, 12, (8, 32)), loudness=MEASURE)
    lw = _open(net, in_sr, RATE, raw.dtype, noise, None, 32, (8, 32), loudness=MEASURE)
    with pytest.raises(ValueError, match="opened with"):
        pp.add_live(lw, loudness=wire.Loudness(target=None))
    pp.add_live(lw, loudness=MEASURE)
    off = 0
    for k in _cuts(net, "20ms", in_sr, raw.numel(), T, 32, 1):
        lw.push(raw[off:off + k])
        off += k
        m = net.loudness_runs()
        pp.step()
        assert net.loudness_runs() - m <= 1
    lw.close()
    while len(pp):
        m = net.loudness_runs()
        pp.step()
        assert net.loudness_runs() - m <= 1
    assert _same(lw.loudness, got[0].loudness) and torch.equal(lw.pcm, plain.pcm)
    assert _same(f.loudness, net.loudness(f._st.o, MODEL_SR, y_lengths=f._st.y_lengths))


# ------------------------------------------------------------------------------------------------ 6. the gain
def _peak_of(L, target=-23.0, cap_db=20.0):
    """the documented fp32 formula, operation by operation, on L's device"""
    g = torch.clamp(torch.pow(torch.full_like(L, 10.0), (target - L) / 20.0), max=10.0 ** (cap_db / 20.0))
    return 0.9 / torch.where(torch.isneginf(L), torch.ones_like(g), g)


def test_the_target_gain_is_the_static_gain_of_the_wire_kernels():
    net = _net()
    x, xl, sid = _text_batch(net, 3, 40, 21)
    out = net.infer(x, xl, sid, noise_scale=0.5, seed=4)
    o, y_lengths = out[0], out[5].sum(dim=(1, 2)).long()                              # (y_mask [B, 1, T'])
    # rows of different loudness, one silent
    o = o * torch.tensor([1.0, 0.05, 0.0], device=o.device).view(3, 1, 1)
    L = net.loudness(o, MODEL_SR, y_lengths=y_lengths)
    print("utterances: L =", L.tolist())
    assert math.isfinite(float(L[0])) and float(L[2]) == -math.inf
    p = _peak_of(L)
    assert float(p[2]) == float(np.float32(0.9))
    loud = wire.Loudness(-23.0)
    for encoding, rate in (("pcm16", RATE), ("ulaw", 8000)):
        m, w = net.loudness_runs(), wire.wire_runs(net)
        got = wire.service_pcm16(net, o, y_lengths, MODEL_SR, rate, limiter=LIM, loudness=loud, encoding=encoding)
        assert net.loudness_runs() - m == 1 and wire.wire_runs(net) - w == 1         # one measuring step in front
        want = wire.service_pcm16(net, o, y_lengths, MODEL_SR, rate, limiter=LIM, peak=p, encoding=encoding)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
        # auto_normalize is ignored, and a measured value skips the measuring step
        m = net.loudness_runs()
        again = wire.service_pcm16(net, o, y_lengths, MODEL_SR, rate, auto_normalize=False, limiter=LIM, encoding=encoding,
                                   loudness=wire.Loudness(-23.0, measured=L))
        assert net.loudness_runs() == m and torch.equal(again[0], want[0])
    # the gain does something: the quiet row comes out louder than by its samples alone, and the cap holds
    plain = wire.service_pcm16(net, o, y_lengths, MODEL_SR, RATE, auto_normalize=False, limiter=LIM)
    got = wire.service_pcm16(net, o, y_lengths, MODEL_SR, RATE, limiter=LIM, loudness=loud)
    assert int(got[0][1].abs().max()) > int(plain[0][1].abs().max())
    assert not bool(got[0][2].any())
    # a stream takes the measured value as an input
    st = _stream(net, 50, 5, (8, 32))
    Ls = torch.tensor([-31.5], device="cuda")                                        # e.g. the previous utterance's
    a = wire.stream_pcm16(net, st, MODEL_SR, RATE, loudness=wire.Loudness(-23.0, measured=Ls))
    b = wire.stream_pcm16(net, _stream(net, 50, 5, (8, 32)), MODEL_SR, RATE, peak=_peak_of(Ls))
    a.run(), b.run()
    assert torch.equal(a.pcm, b.pcm) and torch.equal(a.valid_samples, b.valid_samples)
    assert _same(a.loudness, net.loudness(a._st.o, MODEL_SR, y_lengths=a._st.y_lengths)) and b.loudness is None
    c = wire.stream_pcm16(net, _stream(net, 50, 5, (8, 32)), MODEL_SR, RATE, loudness=wire.Loudness(-23.0, measured=-31.5))
    c.run()
    assert torch.equal(c.pcm, a.pcm)
