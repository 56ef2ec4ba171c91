"""-m gpu: turns on the wire: several utterances as ONE gapless int16 stream.  `mbv_resample_turns` reads
a timeline of segments in place; every byte is compared BITWISE with the existing ranged entry
(`net.resample_pcm16_range`, as `service_pcm16` runs it over [0, total)) on the timeline written out as one fp32 row,
which tests/turn_ref.py restates in NumPy.  No tolerance anywhere: the assembly is exact in fp32."""
import warnings

import numpy as np
import pytest
import torch

from mb_istft_vits_amd import _capi, wire
from mb_istft_vits_amd.models import Request

import turn_ref
from gpu_util import make_net

pytestmark = pytest.mark.gpu

MODEL_SR, RATE = 22050, 24000
LENGTHS, PAUSES = [40, 7, 300, 1, 129], [3, 0, 500, 1]
PAIRS = [(22050, 24000, "kaiser_best"), (22050, 8000, "kaiser_fast"), (22050, 22050, "kaiser_best")]
LIMIT = (0.9, 8, 16)                           # lookahead 8, hold 16 at the wire rate
SENTINEL = {"pcm16": -12345, "ulaw": 0x5A}
_NETS = {}


def _net(name="ljs_mini_mb_istft_vits"):
    if name not in _NETS:
        _NETS[name] = make_net(name)[0]
    return _NETS[name]


def _segments(seed=0):
    """random fp32 device rows, |x| up to 1.5 (the clip and the limiter both work), 5 samples longer than valid"""
    g = torch.Generator().manual_seed(100 + seed)
    return [(torch.rand(n + 5, generator=g) * 3 - 1.5).cuda() for n in LENGTHS]


def _assembled(xs, ramp):
    """the timeline as one device row [1, 1, total], from the NumPy restatement"""
    row = turn_ref.assemble([x.cpu().numpy() for x in xs], LENGTHS, PAUSES, ramp)
    return torch.from_numpy(row).cuda().view(1, 1, -1)


def _reference(net, row, orig, target, res_type, peak, lim, enc, fade):
    """the existing ranged entry over [0, total) of the assembled row, as `service_pcm16` runs it"""
    n = row.shape[-1]
    width = wire.resample_ready(orig, target, n, n, res_type)
    pcm = torch.full((1, width), SENTINEL[enc], device="cuda", dtype=torch.int16 if enc == "pcm16" else torch.uint8)
    ns = torch.full((1,), -1, device="cuda", dtype=torch.int64)
    running = torch.zeros(1, device="cuda")
    net.resample_pcm16_range(row, orig, target, n, 0, width, pcm, peak=peak, running_peak=running, out_samples=ns,
                             res_type=res_type, limiter=lim, encoding=enc, fade=fade)
    return pcm, ns, running


def _turn_row(plan, xs, ramp, pcm, running, peak, first, count, in_avail=None, in_total=None, ns=None, every=False):
    """one `_capi.MbvTurnChunk`: outputs [first, first + count) of the timeline of `plan` into `pcm`"""
    k = _capi.MbvTurnChunk()
    c = k.chunk
    c.wave, c.valid_samples = None, None
    c.in_total = plan.in_total() if in_total is None else in_total
    c.in_avail = plan.frontier() if in_avail is None else in_avail
    c.out_first, c.out_count = first, count
    c.peak = peak.data_ptr() if peak is not None else None
    c.pcm, c.pcm_capacity = pcm.data_ptr(), pcm.shape[1]
    c.running_peak = running.data_ptr()
    c.out_samples = ns.data_ptr() if ns is not None else None
    s0, s1 = (0, len(xs)) if every else plan.segments_for(first, count)
    segs = (_capi.MbvTurnSeg * max(s1 - s0, 1))()
    for sg, s in zip(segs, range(s0, s1)):
        sg.wave, sg.start, sg.length = xs[s].data_ptr(), plan.starts[s], plan.lengths[s]
        sg.ramp = wire.turn_ramp(ramp, plan.lengths[s])
    k.segs, k.n_segs = segs, s1 - s0
    return k


def _plan(orig, target, res_type, lim, cap, decoded=True, close=True):
    plan = wire.TurnPlan(orig, target, cap, res_type, lookahead=lim[1] if lim else 0, hold=lim[2] if lim else 0)
    for s, n in enumerate(LENGTHS):
        plan.append(n, PAUSES[s - 1] if s else 0)
        if decoded:
            plan.decoded(s, n)
    if close:
        plan.close()
    return plan


def _tiling(cuts, width):
    cuts = sorted({min(c, width) for c in cuts} | {0, width})
    return [(a, b - a) for a, b in zip(cuts, cuts[1:])]


# ------------------------------------------------------------------------------------------------ the raw call
@pytest.mark.timeout(600)
@pytest.mark.parametrize("orig,target,res_type", PAIRS)
def test_raw_call_is_bitwise_the_ranged_entry_on_the_assembled_row(orig, target, res_type):
    net = _net()
    xs = _segments()
    L, M, K, left = wire.resample_geometry(orig, target, res_type)
    if K:                                      # one output's taps span three segments and a pause; the one-sample
        assert K > 7 + 3 + 2 and K > 1 + 1 + 2  # segment lies inside a filter window
    peak = torch.tensor([0.8], device="cuda")
    total = sum(LENGTHS) + sum(PAUSES)
    width = wire.resample_ready(orig, target, total, total, res_type)
    joint = -(-41 * target // orig)            # a fade that starts inside the joint between segments 0 and 1
    launches = 0
    for ramp in (0, 4, 64):
        row = _assembled(xs, ramp)
        assert row.shape[-1] == total
        if ramp:
            assert not torch.equal(row, _assembled(xs, 0))
        for enc in ("pcm16", "ulaw"):
            for lim in (None, LIMIT):
                for fade in (None, (joint, 30)):
                    want, want_ns, want_run = _reference(net, row, orig, target, res_type, peak, lim, enc, fade)
                    plan = _plan(orig, target, res_type, lim, width)
                    # two tilings of the same turn in ONE call: ranges cut at out-of-tile offsets, counts 1, 255, 257
                    got = [torch.full_like(want, SENTINEL[enc]) for _ in range(2)]
                    run = [torch.zeros(1, device="cuda") for _ in range(2)]
                    ns = torch.full((1,), -1, device="cuda", dtype=torch.int64)
                    tiles = [_tiling([1, 256, 513], width), _tiling([3, 260], width)]
                    assert (1, 255) in tiles[0] and (3, 257) in tiles[1] and (0, 1) in tiles[0]
                    rows = [_turn_row(plan, xs, ramp, got[i], run[i], peak, a, n, ns=ns if (i, a) == (0, 0) else None)
                            for i in range(2) for a, n in tiles[i]]
                    rows.reverse()             # (the order of the rows in the call does not matter)
                    n_rows = len(rows)
                    tot, firsts = wire.turn_plan(orig, target, rows, res_type, [lim] * n_rows)
                    assert tot == 2 * width
                    packed = torch.full((tot + 8,), SENTINEL[enc], device="cuda", dtype=want.dtype)
                    runs = wire.wire_runs(net)
                    net.resample_turns(rows, orig, target, packed=packed, res_type=res_type, limits=[lim] * n_rows,
                                       encoding=enc, fades=[fade] * n_rows)
                    assert wire.wire_runs(net) - runs == 1
                    launches += 1
                    for i in range(2):
                        assert torch.equal(got[i], want), (ramp, enc, lim, fade, i, int((got[i] != want).sum()))
                        assert torch.equal(run[i].view(torch.int32), want_run.view(torch.int32))
                    assert torch.equal(ns, want_ns) and int(ns) == width
                    pieces = [want[0, k.chunk.out_first:k.chunk.out_first + k.chunk.out_count] for k in rows]
                    assert torch.equal(packed[:tot], torch.cat(pieces)) and bool((packed[tot:] == SENTINEL[enc]).all())
    assert launches == 24
    # limited and unlimited turns in one call: two launches; rows with nothing to write: none
    row = _assembled(xs, 4)
    plan_u, plan_l = _plan(orig, target, res_type, None, width), _plan(orig, target, res_type, LIMIT, width)
    got = [torch.full((1, width), SENTINEL["pcm16"], device="cuda", dtype=torch.int16) for _ in range(2)]
    run = [torch.zeros(1, device="cuda") for _ in range(2)]
    runs = wire.wire_runs(net)
    net.resample_turns([_turn_row(plan_u, xs, 4, got[0], run[0], None, 0, width),
                        _turn_row(plan_l, xs, 4, got[1], run[1], None, 0, width)], orig, target, res_type=res_type,
                       limits=[None, LIMIT])
    assert wire.wire_runs(net) - runs == 2
    assert torch.equal(got[0], _reference(net, row, orig, target, res_type, None, None, "pcm16", None)[0])
    assert torch.equal(got[1], _reference(net, row, orig, target, res_type, None, LIMIT, "pcm16", None)[0])
    runs = wire.wire_runs(net)
    net.resample_turns([_turn_row(plan_u, xs, 4, got[0], run[0], None, 5, 0)], orig, target, res_type=res_type)
    net.resample_turns([], orig, target, res_type=res_type)
    assert wire.wire_runs(net) == runs


@pytest.mark.timeout(600)
@pytest.mark.parametrize("lim", [None, LIMIT], ids=["plain", "limited"])
@pytest.mark.parametrize("orig,target,res_type", PAIRS)
def test_nothing_at_or_past_the_frontier_is_read(orig, target, res_type, lim):
    """The frontier in the middle of segment 2; every segment buffer holds NaN (then 1e30) beyond what is decoded, the
    undecoded segments wholly.  The outputs the plan allows are bitwise the finished turn's, and the peak is no NaN."""
    net = _net()
    xs = _segments(1)
    total = sum(LENGTHS) + sum(PAUSES)
    width = wire.resample_ready(orig, target, total, total, res_type)
    want, _, _ = _reference(net, _assembled(xs, 4), orig, target, res_type, None, lim, "pcm16", None)
    avail = [40, 7, 150, 0, 0]
    plan = _plan(orig, target, res_type, lim, width, decoded=False, close=False)
    for s, a in enumerate(avail):
        plan.decoded(s, a)
    assert plan.frontier() == 50 + 150 and plan.in_total() == plan.capacity > total
    first, count = plan.wire_due()
    assert first == 0 and 0 < count < width
    for poison in (float("nan"), 1e30):
        dirty = [x.clone() for x in xs]
        for x, a in zip(dirty, avail):
            x[a:] = poison
        got = torch.full((1, width), SENTINEL["pcm16"], device="cuda", dtype=torch.int16)
        running = torch.zeros(1, device="cuda")
        net.resample_turns([_turn_row(plan, dirty, 4, got, running, None, 0, count, every=True)], orig, target,
                           res_type=res_type, limits=[lim])
        assert torch.equal(got[:, :count], want[:, :count]), int((got[:, :count] != want[:, :count]).sum())
        assert bool((got[:, count:] == SENTINEL["pcm16"]).all())
        assert bool(torch.isfinite(running).all()) and float(running) > 0.0
    # one output more is refused, by the plan and by the call; nothing is launched and the handle stays usable
    runs = wire.wire_runs(net)
    k = _turn_row(plan, xs, 4, got, running, None, 0, count + 1, every=True)
    with pytest.raises(_capi.MbvError, match="turn 0: outputs up to"):
        wire.turn_plan(orig, target, [k], res_type, [lim])
    with pytest.raises(_capi.MbvError, match="turn 0: outputs up to"):
        net.resample_turns([k], orig, target, res_type=res_type, limits=[lim])
    assert wire.wire_runs(net) == runs


# ------------------------------------------------------------------------------------------------ end to end
def _ids(T, seed):
    return torch.randint(1, 59, (T,), generator=torch.Generator().manual_seed(seed))


def _request(T, seed, marks=False, chunk=8, cap=16):
    return Request(_ids(T, seed), noise_scale=0.5, length_scale=3.0, seed=seed, chunk_frames=chunk, max_chunk_frames=cap,
                   marks=marks)


def _alone(net, T, seed, marks=False, chunk=8, cap=16):
    """the same request as a stand-alone `infer_stream`, decoded to its end"""
    x = _ids(T, seed).view(1, -1).cuda()
    st = net.infer_stream(x, torch.tensor([T]).cuda(), None, noise_scale=0.5, length_scale=3.0, seed=[seed],
                          chunk_frames=chunk, max_chunk_frames=cap, marks=marks)
    st.run()
    return st


def _valid(st):
    return min(256 * st.z.shape[2], st.o.shape[-1])


TEXTS = [(5, 31), (9, 32), (3, 33)]            # (tokens, seed)
PAUSES_MS = [0.0, 120.0, 0.0]
_REF = {}


def _finished():
    """the three finished stand-alone decodes, once"""
    if "sts" not in _REF:
        _REF["sts"] = [_alone(_net(), T, seed) for T, seed in TEXTS]
    return _REF["sts"]


def _drive(net, mode, limiter=None, peak=None, encoding="pcm16"):
    """Three texts admitted on different ticks while earlier pieces are handed out; -> (turn, streams, pieces)."""
    sp = net.stream_pool()
    pp = wire.pcm_pool(net, sp, MODEL_SR, RATE, encoding=encoding)
    turn = pp.add_turn(1 << 18, peak=peak, limiter=limiter)
    assert turn.ramp == round(5e-3 * MODEL_SR) and len(pp) == 1
    other = None
    if mode == "named":                        # a plain member beside the turn, stepped by name in another order
        other = pp.add(net.dec_stream(torch.randn(1, net.cfg.inter_channels, 70, generator=torch.Generator().manual_seed(4)).cuda(),
                                      None, 8, 16))
    sts, pieces, tick = [], [], 0
    while not turn.finished:
        if tick in (0, 2, 3) and len(sts) < 3:
            T, seed = TEXTS[len(sts)]
            sts += turn.admit([_request(T, seed)], pauses_ms=[PAUSES_MS[len(sts)]])
        if tick == 5:
            turn.close()
        if mode == "named":
            names = [turn] + ([other._st] if pp.follower(other._st) is not None else [])
            out = pp.step(streams=names[::-1] if tick % 2 else names)
        else:
            out = pp.step(host=mode == "host")
        for who, a, piece in out:
            if who is turn:
                assert a == sum(len(p) for p in pieces)                      # the pieces follow one another
                pieces.append(piece.copy() if mode == "host" else piece.clone())
        tick += 1
        assert tick < 200
    assert len(pp.turns) == 0 and all(not any(st is m for m in sp.streams) for st in sts)
    return turn, sts, pieces


@pytest.mark.timeout(600)
@pytest.mark.parametrize("mode", ["all", "named", "host"])
def test_end_to_end_is_bitwise_the_ranged_entry_on_the_assembled_turn(mode):
    net = _net()
    want_sts = _finished()
    limiter = wire.Limiter(0.9, lookahead_ms=8 * 1e3 / RATE, hold_ms=16 * 1e3 / RATE) if mode != "all" else None
    peak = 0.5 if mode == "named" else None
    turn, sts, pieces = _drive(net, mode, limiter=limiter, peak=peak)
    print("turn of %s frames, %s chunks, %d pieces" % ([st.z.shape[2] for st in sts], [len(st.schedule) for st in sts],
                                                        len(pieces)))
    assert len(pieces) >= 3 and len(sts) == 3 and max(len(st.schedule) for st in sts) >= 2
    for st, ref in zip(sts, want_sts):         # every segment bitwise its stand-alone infer_stream
        assert st._drained() and torch.equal(st.o, ref.o)
    lengths = [_valid(st) for st in sts]
    pauses = [round(ms * 1e-3 * MODEL_SR) for ms in PAUSES_MS[1:]]
    row = wire.assemble_turn([st.o for st in sts], lengths, pauses, turn.ramp)
    numpy_row = turn_ref.assemble([st.o.cpu().numpy() for st in sts], lengths, pauses, turn.ramp)
    assert np.array_equal(row[0, 0].cpu().numpy().view(np.int32), numpy_row.view(np.int32))
    pk = None if peak is None else torch.tensor([peak], device="cuda")
    want, ns, running = _reference(net, row, MODEL_SR, RATE, "kaiser_best", pk, turn._lim, "pcm16", None)
    total = int(ns)
    got = np.concatenate(pieces) if mode == "host" else torch.cat(pieces).cpu().numpy()
    assert np.array_equal(got, want[0].cpu().numpy())
    assert torch.equal(turn.pcm[:, :total], want) and torch.equal(turn.valid_samples, ns)
    assert torch.equal(turn.peak.view(torch.int32), running.view(torch.int32))
    # 20 ms frames of the pieces: those of the whole turn, one short frame at the very end only
    cutter, frames = wire.FrameCutter(RATE), []
    for p in pieces:
        frames += cutter.push(p)
    assert frames + cutter.close() == wire.frame_pcm16(want[0], RATE, valid_samples=total)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("limited", [False, True], ids=["plain", "limited"])
def test_one_segment_without_a_ramp_is_bitwise_stream_pcm16(limited):
    net = _net()
    limiter = wire.Limiter(0.9, 1.0, 2.0) if limited else None
    T, seed = TEXTS[1]
    alone = wire.stream_pcm16(net, net.infer_streams([_request(T, seed)])[0], MODEL_SR, RATE, peak=0.4, limiter=limiter)
    alone.run()
    pp = wire.pcm_pool(net, net.stream_pool(), MODEL_SR, RATE)
    turn = pp.add_turn(alone.pcm.shape[1], peak=0.4, limiter=limiter, ramp_ms=0.0)
    st = turn.admit([_request(T, seed)])[0]
    turn.close()
    while not turn.finished:
        pp.step()
    n = int(alone.valid_samples[0])
    assert torch.equal(st.o, alone._st.o) and n == alone.pcm.shape[1]
    assert torch.equal(turn.pcm, alone.pcm) and torch.equal(turn.valid_samples, alone.valid_samples)
    assert torch.equal(turn.peak.view(torch.int32), alone.peak.view(torch.int32))


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
def test_one_launch_for_all_turns_of_a_tick_and_no_host_synchronisation():
    net = _net()
    pp = wire.pcm_pool(net, net.stream_pool(), MODEL_SR, RATE)
    turns = [pp.add_turn(1 << 17), pp.add_turn(1 << 17)]
    for k, t in enumerate(turns):
        t.append(net.dec_stream(_z(net, 60 + k, 20 + k), None, 8, 16))
        t.append(net.dec_stream(_z(net, 40, 30 + k), None, 8, 16), pause_ms=30.0)
    pp.step()                                  # (the first tick uploads the bank)
    runs = wire.wire_runs(net)
    out = pp.step()
    assert sorted(id(t) for t, _, _ in out) == sorted(id(t) for t in turns) and wire.wire_runs(net) - runs == 1
    member = pp.add(net.dec_stream(_z(net, 50, 40), None, 8, 16))
    runs = wire.wire_runs(net)
    out = pp.step()
    assert len(out) == 3 and wire.wire_runs(net) - runs == 2 and any(st is member._st for st, _, _ in out)
    runs, got = wire.wire_runs(net), []
    n = _count_syncs(lambda: got.extend(pp.step()))
    print("host synchronisations in a tick of two turns and one plain member: %d" % n)
    assert n == 0 and len(got) == 3 and wire.wire_runs(net) - runs == 2


# ------------------------------------------------------------------------------------------------ barge-in
@pytest.mark.timeout(600)
@pytest.mark.parametrize("limited", [False, True], ids=["plain", "limited"])
def test_revoke_in_the_middle_of_the_second_of_three_segments(limited):
    net = _net()
    texts = [(12, 51), (40, 52), (10, 53)]
    limiter = wire.Limiter(0.9, lookahead_ms=8 * 1e3 / RATE, hold_ms=16 * 1e3 / RATE) if limited else None
    lag = 8 if limited else 0
    whole = [_alone(net, T, seed, marks=True, chunk=4, cap=8) for T, seed in texts]
    lengths = [_valid(st) for st in whole]
    pause = round(0.05 * MODEL_SR)
    starts = turn_ref.starts(lengths, [pause, pause])
    sp = net.stream_pool()
    pp = wire.pcm_pool(net, sp, MODEL_SR, RATE)
    turn = pp.add_turn(1 << 19, peak=0.5, limiter=limiter)
    sts = turn.admit([_request(T, seed, True, 4, 8) for T, seed in texts[:2]], pauses_ms=[0.0, 50.0])
    a_wire, b_wire = -(-starts[1] * RATE // MODEL_SR), (starts[1] + lengths[1]) * RATE // MODEL_SR
    pieces = []
    while turn._plan.out_done <= a_wire + 100:
        pieces += [p.clone() for t, _, p in pp.step()]
    E = turn._plan.out_done
    assert a_wire < E < b_wire - 2000, (a_wire, E, b_wire)       # in the middle of segment 2
    sts += turn.admit([_request(*texts[2], True, 4, 8)], pauses_ms=[50.0])
    assert any(sts[2] is m for m in sp.streams) and sts[2]._decoded == 0
    rep = turn.revoke(fade_ms=5.0)
    F, N = E, round(5e-3 * RATE)
    total = wire.resample_ready(MODEL_SR, RATE, starts[2] + lengths[2], starts[2] + lengths[2])
    assert (rep.first, rep.count, rep.valid_samples) == (F, N, min(total, F + N)) and turn.closed and turn.revoked
    assert turn.revoke() is rep
    # segment 3 is gone undecoded; segment 2 decodes no further than the cut needs
    assert not any(sts[2] is m for m in sp.streams) and sts[2]._decoded == 0
    assert len(sts[1].schedule) < len(whole[1].schedule)
    ticks = 0
    while not turn.finished:
        pieces += [p.clone() for t, _, p in pp.step()]
        ticks += 1
        assert ticks < 50
    dec, runs = net.decoder_runs(), wire.wire_runs(net)
    assert pp.step() == [] and net.decoder_runs() == dec and wire.wire_runs(net) == runs
    assert len(sp.streams) == 0 and len(pp) == 0 and sts[2]._decoded == 0
    # the bytes: the ranged entry on the assembled row of the FINISHED waveforms, with fade = (F, N)
    row = wire.assemble_turn([st.o for st in whole], lengths, [pause, pause], turn.ramp)
    want, _, _ = _reference(net, row, MODEL_SR, RATE, "kaiser_best", torch.tensor([0.5], device="cuda"), turn._lim,
                            "pcm16", (F, N))
    cut = rep.valid_samples
    assert torch.equal(torch.cat(pieces), want[0, :cut]) and torch.equal(turn.pcm[0, :cut], want[0, :cut])
    assert int(turn.valid_samples[0]) == cut == min(total, F + N)
    assert bool((turn.pcm[0, cut:] == 0).all())
    # tokens the listener heard begin, against the marks of the stand-alone streams
    started = 0
    for st, p in zip(whole, starts):
        assert st.marks is not None
        started += sum(1 for f in st.marks[:-1] if -(-(p + st.spf * f) * RATE // MODEL_SR) + lag < F)
    assert rep.tokens_started == started and 12 < started < 52
    assert [len(m) for m in turn.marks] == [len(st.marks) for st in whole]


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.timeout(600)
def test_refusals_launch_nothing_and_the_next_tick_works():
    net = _net()
    sp = net.stream_pool()
    pp = wire.pcm_pool(net, sp, MODEL_SR, RATE)
    st = net.dec_stream(_z(net, 40, 1), None, 8, 16)
    n_out = wire.resample_ready(MODEL_SR, RATE, 256 * 40, 256 * 40)
    turn = pp.add_turn(n_out + 100, limiter=wire.Limiter(0.9, 1.0, 2.0))
    turn.append(st)
    pp.step()
    counters = (wire.wire_runs(net), net.decoder_runs(), len(sp.streams), len(turn.segments))
    plain = pp.add(net.dec_stream(_z(net, 30, 2), None, 8, 16))
    other_turn = pp.add_turn(1 << 16)
    theirs = net.dec_stream(_z(net, 30, 3), None, 8, 16)
    other_turn.append(theirs)
    members = len(sp.streams)
    other = make_net("uudb_ms_istft_vits_ms")[0]
    live = other.convert_live(3, 7, MODEL_SR, 256, 1024, 256 * 40 + 100)
    for bad, why in ((live, "LiveStream"), (plain._st, "plain member"), (theirs, "segment of a turn"),
                     (st, "segment of a turn"), (other.dec_stream(_z(other, 20, 4), None, 8, 16), "another model"),
                     (net.dec_stream(_z(net, 2, 5), None, 8, 16), "max_samples"),
                     (net.dec_stream(torch.cat([_z(net, 9, 6)] * 2), None, 8, 16), "ONE utterance")):
        with pytest.raises(ValueError, match=why):
            turn.append(bad, pause_ms=10.0)
    with pytest.raises(ValueError, match="max_samples"):      # all or nothing: the admitted stream does not stay
        turn.admit([_request(9, 32)])
    with pytest.raises(ValueError, match="segment of a turn"):    # the other order: a segment does not join as a member
        pp.add(st)
    with pytest.raises(ValueError, match="segment of a turn"):
        pp.add(theirs, peak=0.5)
    with pytest.raises(ValueError, match="one pause per request"):
        turn.admit([_request(9, 32)], pauses_ms=[])
    with pytest.raises(ValueError, match="pause_ms"):
        turn.append(net.dec_stream(_z(net, 1, 5), None, 8, 16), pause_ms=-1.0)
    with pytest.raises(ValueError, match="handed out"):
        turn.revoke(at=turn._plan.out_done - 1)
    with pytest.raises(ValueError, match="at must be"):
        turn.revoke(at="token")
    with pytest.raises(ValueError, match="not in the pool"):
        pp.step(streams=[wire.Turn(wire.pcm_pool(net, net.stream_pool(), MODEL_SR, RATE), 100)])
    with pytest.raises(ValueError, match="running loudness"):
        pp.add_turn(100, loudness=wire.Loudness(target=None))
    with pytest.raises(ValueError, match="ramp_ms"):
        pp.add_turn(100, ramp_ms=-1.0)
    assert len(sp.streams) == members and len(turn.segments) == 1 and not turn.revoked
    # the C entry: a wave beside the segments, a missing segment wave, a bad law; nothing is launched
    xs = _segments(2)
    width = wire.resample_ready(MODEL_SR, RATE, 981, 981)
    plan = _plan(MODEL_SR, RATE, "kaiser_best", None, width)
    pcm = torch.full((1, width), SENTINEL["pcm16"], device="cuda", dtype=torch.int16)
    running = torch.zeros(1, device="cuda")
    good = _turn_row(plan, xs, 4, pcm, running, None, 0, 100)
    k = _turn_row(plan, xs, 4, pcm, running, None, 100, 100)
    k.chunk.wave = xs[0].data_ptr()
    with pytest.raises(_capi.MbvError, match="turn 1: chunk.wave must be NULL"):
        net.resample_turns([good, k], MODEL_SR, RATE)
    k = _turn_row(plan, xs, 4, pcm, running, None, 100, 100)
    k.segs[0].wave = None
    with pytest.raises(_capi.MbvError, match="turn 1: segment 0: wave missing"):
        net.resample_turns([good, k], MODEL_SR, RATE)
    with pytest.raises(_capi.MbvError, match="turns 0 and 1 write overlapping"):
        net.resample_turns([good, _turn_row(plan, xs, 4, pcm, running, None, 99, 10)], MODEL_SR, RATE)
    with pytest.raises(_capi.MbvError, match="turn 1: .*hold"):
        net.resample_turns([good, _turn_row(plan, xs, 4, pcm, running, None, 100, 10)], MODEL_SR, RATE,
                           limits=[None, (0.9, 8, 2000)])
    with pytest.raises(_capi.MbvError, match="packed_capacity"):
        net.resample_turns([good], MODEL_SR, RATE, packed=torch.zeros(99, device="cuda", dtype=torch.int16))
    h = net._ensure_handle()
    arr = (_capi.MbvTurnChunk * 1)(good)
    assert _capi.lib().mbv_resample_turns(h, arr, None, None, 1, MODEL_SR, RATE, 0, 3, None, 0, None) != 0
    assert b"law" in _capi.lib().mbv_last_error(h)
    assert bool((pcm == SENTINEL["pcm16"]).all())
    assert (wire.wire_runs(net), net.decoder_runs()) == counters[:2]
    # a limited turn whose halo does not fit the LDS stage: the limiter is inside its ranges, but 48 kHz -> 8 kHz reads
    # six inputs per output and 255 + 1024 outputs of halo beside the tile need more than the stage holds
    wide, fits = (0.9, 255, 1024), (0.9, 255, 64)
    narrow = wire.resample_ready(48000, 8000, 981, 981)
    low = torch.full((1, narrow), SENTINEL["pcm16"], device="cuda", dtype=torch.int16)
    other_low = torch.full_like(low, SENTINEL["pcm16"])
    rows = [_turn_row(_plan(48000, 8000, "kaiser_best", lim, narrow), xs, 4, pcm_, running, None, 0, narrow)
            for lim, pcm_ in ((wide, other_low), (fits, low))]
    net.resample_pcm16_range(_assembled(xs, 4), 48000, 8000, 981, 0, 1, torch.zeros(1, narrow, device="cuda", dtype=torch.int16))
    runs = wire.wire_runs(net)                 # (the call above uploaded the pair's bank)
    with pytest.raises(_capi.MbvError, match="mbv_resample_turns: turn 1: .*halo window larger than the LDS stage"):
        net.resample_turns([rows[1], rows[0]], 48000, 8000, limits=[fits, wide])
    assert wire.wire_runs(net) == runs
    assert bool((low == SENTINEL["pcm16"]).all()) and bool((other_low == SENTINEL["pcm16"]).all())
    net.resample_turns([rows[1]], 48000, 8000, limits=[fits])             # the next call works, bitwise
    assert wire.wire_runs(net) == runs + 1
    assert torch.equal(low, _reference(net, _assembled(xs, 4), 48000, 8000, "kaiser_best", None, fits, "pcm16", None)[0])
    # the next tick works, and the turn that refused plays to its end, bitwise
    turn.close()
    while not turn.finished:
        pp.step()
    row = wire.assemble_turn([st.o], [256 * 40], [], turn.ramp)
    want, ns, _ = _reference(net, row, MODEL_SR, RATE, "kaiser_best", None, turn._lim, "pcm16", None)
    assert torch.equal(turn.pcm[:, :n_out], want) and torch.equal(turn.valid_samples, ns)
    with pytest.raises(ValueError, match="after close"):
        turn.append(net.dec_stream(_z(net, 1, 7), None, 8, 16))
