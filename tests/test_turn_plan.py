"""Turns on the wire, host side (no GPU): `wire.TurnPlan` against a brute force that walks every tap
(tests/turn_ref.py), `revoke_plan` over a turn's readiness, the refusals of `mbv_turn_plan`, and the frames of a turn."""
import base64
import random

import numpy as np
import pytest
import torch

from mb_istft_vits_amd import _capi, wire

import turn_ref

PAIRS = [(22050, 24000, "kaiser_best"), (22050, 8000, "kaiser_fast"), (22050, 22050, "kaiser_best")]


def _geom(orig, target, res_type):
    return wire.resample_geometry(orig, target, res_type)


@pytest.mark.parametrize("orig,target,res_type", PAIRS)
def test_geometry_covers_the_reference_taps(orig, target, res_type):
    L, M, K, left = _geom(orig, target, res_type)
    if orig == target:
        assert (L, M, K, left) == (1, 1, 0, 0)
        return
    lmax, rmax = turn_ref.ref_tap_span(orig, target, res_type)
    # x[n_t - lmax + 1 .. n_t + rmax] of resampy's loop inside x[n_t - left - 1 .. n_t - left + K - 1]
    assert left >= lmax - 1 and K - left - 1 >= rmax
    assert wire.resample_ready_open(orig, target, 1000, res_type) == -(-(1000 - K + left + 1) * L // M)


def _random_turn(rng, width):
    S = rng.randint(1, 6)
    lengths = [rng.choice([1, 2, 3, 7, 40, 129, 300, 1000]) for _ in range(S)]
    pauses = [rng.choice([0, 0, 1, 3, width + 5, 2 * width + 1]) for _ in range(S - 1)]
    return lengths, pauses


@pytest.mark.parametrize("lookahead", [0, 8])
@pytest.mark.parametrize("orig,target,res_type", PAIRS)
def test_plan_against_the_brute_force(orig, target, res_type, lookahead):
    geom = _geom(orig, target, res_type)
    width = geom[2] + 2
    rng = random.Random(orig + target + lookahead)
    for trial in range(40):
        lengths, pauses = _random_turn(rng, width)
        S = len(lengths)
        cap = int(np.ceil((sum(lengths) + sum(pauses)) * target / orig)) + rng.choice([0, 5])
        plan = wire.TurnPlan(orig, target, cap, res_type, lookahead=lookahead, hold=16)
        close_early = trial % 2 == 0               # close() before the last chunk, or after it
        appended, avail, ranges, closed = 0, [], [], False
        while True:
            moves = []
            if appended < S:
                moves.append("append")
            if any(a < n for a, n in zip(avail, lengths[:appended])):
                moves += ["decode"] * 3
            if appended == S and not closed and (close_early or not moves):
                moves.append("close")
            if not moves:
                break
            move = rng.choice(moves)
            if move == "append":
                s = plan.append(lengths[appended], pauses[appended - 1] if appended else 0)
                assert s == appended and plan.starts[s] == turn_ref.starts(lengths, pauses)[s]
                appended += 1
                avail.append(0)
            elif move == "decode":
                s = rng.choice([s for s in range(appended) if avail[s] < lengths[s]])
                avail[s] = min(lengths[s], avail[s] + rng.choice([1, 5, 64, 400]))
                plan.decoded(s, avail[s])
            else:
                plan.close()
                closed = True
            n_now, p_now = lengths[:appended], pauses[:max(appended - 1, 0)]
            front = turn_ref.frontier(n_now, p_now, avail, closed)
            assert plan.frontier() == front
            end = sum(n_now) + sum(p_now)
            complete = closed and avail == n_now
            assert plan.complete == complete
            want = turn_ref.ready_brute(front, end if closed else None, geom, orig, target, lookahead, complete, cap)
            assert plan.ready() == want, (trial, move, front, end, closed)
            due = plan.wire_due()
            if due is not None:
                a, count = due
                assert a == plan.out_done and count > 0 and a + count == want
                s0, s1 = plan.segments_for(a, count)
                lo = turn_ref.taps_of(max(a - lookahead - 16, 0), *geom)[0]
                hi = turn_ref.taps_of(a + count - 1 + lookahead, *geom)[1]
                starts = turn_ref.starts(n_now, p_now)
                hit = [s for s in range(appended) if starts[s] <= hi and starts[s] + n_now[s] > lo]
                assert list(range(s0, s1)) == list(range(hit[0], hit[-1] + 1)) if hit else s0 == s1
                ranges.append((a, a + count))
                plan.wired(a + count)
            assert plan.done == (complete and plan.out_done == plan.out_total())
        total = plan.out_total()
        assert plan.done and ranges[0][0] == 0 and ranges[-1][1] == total == int(np.ceil(plan.end * target / orig))
        assert all(b == c for (_, b), (c, _) in zip(ranges, ranges[1:]))   # monotone, and they tile [0, total)


def test_append_refusals_change_nothing():
    plan = wire.TurnPlan(22050, 24000, 1000)
    with pytest.raises(ValueError, match="first segment"):
        plan.append(10, 3)
    plan.append(400)
    with pytest.raises(ValueError, match="max_samples"):
        plan.append(600)                          # ceil(1000 * 24000 / 22050) = 1089 > 1000
    with pytest.raises(ValueError, match="n >= 1"):
        plan.append(0)
    assert plan.append(500, 18) == 1 and plan.out_total() == 1000
    plan.close()
    with pytest.raises(ValueError, match="after close"):
        plan.append(1)
    assert (plan.starts, plan.lengths) == ([0, 418], [400, 500])
    with pytest.raises(ValueError):
        wire.TurnPlan(22050, 24000, 1000, lookahead=256)
    with pytest.raises(_capi.MbvError, match="4096"):
        wire.TurnPlan(22050, 24001, 1000)        # 24001 phases: refused where the plan is made


@pytest.mark.parametrize("lookahead", [0, 8])
@pytest.mark.parametrize("orig,target,res_type", PAIRS)
def test_revoke_plan_over_a_turn(orig, target, res_type, lookahead):
    geom = _geom(orig, target, res_type)
    rng = random.Random(7 * lookahead + target)
    for trial in range(30):
        lengths, pauses = _random_turn(rng, geom[2] + 2)
        plan = wire.TurnPlan(orig, target, 1 << 20, res_type, lookahead=lookahead)
        for s, n in enumerate(lengths):
            plan.append(n, pauses[s - 1] if s else 0)
        avails = []
        for n in lengths:
            cuts = sorted(set(rng.sample(range(1, n + 1), min(n, rng.randint(1, 4)))) | {n})
            avails.append(cuts)
        events = plan.revoke_events(avails)
        ready = [r for _, _, r in events]
        total = plan.out_total()
        assert ready == sorted(ready) and ready[-1] == total and len(events) == sum(len(a) for a in avails)
        E = rng.randint(0, total)
        F, N = E + rng.choice([0, 3, 50]), rng.choice([0, 1, 120])
        cut, last, clipped = wire.revoke_plan(ready, total, E, F, N)
        assert cut == min(total, F + N) and clipped == [min(r, cut) for r in ready[:last + 1]]
        # the brute force, with the frontier where event `last` leaves it: the cut is final there, and not one event earlier
        starts = turn_ref.starts(lengths, pauses)

        def front_after(k):
            s, i, _ = events[k]
            if i + 1 < len(avails[s]):
                return starts[s] + avails[s][i]
            return starts[s + 1] if s + 1 < len(lengths) else plan.end

        def final_at(k):
            whole = k == len(events) - 1
            return turn_ref.ready_brute(front_after(k), plan.end, geom, orig, target, lookahead, whole, total)

        assert final_at(last) >= cut
        assert last == 0 or final_at(last - 1) < cut


def _turn(segs, in_total, in_avail, out_first, out_count, cap=4000):
    k = _capi.MbvTurnChunk()
    c = k.chunk
    c.wave, c.in_total, c.in_avail, c.out_first, c.out_count = None, in_total, in_avail, out_first, out_count
    c.pcm, c.pcm_capacity = 4096, cap             # (the plan reads the integer fields only)
    arr = (_capi.MbvTurnSeg * max(len(segs), 1))()
    for sg, (start, length, ramp) in zip(arr, segs):
        sg.wave, sg.start, sg.length, sg.ramp = 4096, start, length, ramp
    k.segs, k.n_segs = arr, len(segs)
    k._keep = arr
    return k


def test_turn_plan_totals_and_refusals():
    good = _turn([(0, 40, 4), (43, 7, 3), (50, 300, 64)], 2000, 350, 0, 200)
    also = _turn([(0, 1000, 0)], 1000, 1000, 10, 1079)
    assert wire.turn_plan(22050, 24000, [good, also]) == (1279, [0, 200])
    assert wire.turn_plan(22050, 24000, []) == (0, [])
    lim = (0.9, 8, 16)
    assert wire.turn_plan(22050, 24000, [good, also], limits=[lim, None]) == (1279, [0, 200])
    ready = wire.resample_ready_open(22050, 24000, 350)
    assert wire.turn_plan(22050, 24000, [_turn([(0, 40, 4)], 2000, 350, 0, ready)])[0] == ready
    bad = [
        (_turn([(0, 40, 4)], 2000, 350, 0, ready + 1), None, "make only %d final" % ready),
        (_turn([(0, 40, 4)], 2000, 350, 0, ready - 7), lim, "make only %d final" % (ready - 8)),   # the limiter's lag
        (_turn([(0, 40, 4)], 2000, 2000, 0, 2177, cap=2176), None, "pcm_capacity"),
        (_turn([(0, 40, 4)], 0, 0, 0, 0), None, "in_total"),
        (_turn([(0, 40, 21)], 2000, 350, 0, 10), None, "segment 0: ramp 21"),
        (_turn([(0, 40, -1)], 2000, 350, 0, 10), None, "segment 0: ramp -1"),
        (_turn([(0, 0, 0)], 2000, 350, 0, 10), None, "segment 0: start must be >= 0 and length > 0"),
        (_turn([(-1, 5, 0)], 2000, 350, 0, 10), None, "segment 0: start"),
        (_turn([(0, 40, 0), (39, 7, 0)], 2000, 350, 0, 10), None, "segment 1 starts at 39"),
        (_turn([(50, 7, 0), (0, 40, 0)], 2000, 350, 0, 10), None, "ascending and disjoint"),
        (_turn([(0, 40, 4)], 2000, 350, 0, 10), (1.5, 8, 16), "ceiling"),
    ]
    for k, limit, why in bad:
        with pytest.raises(_capi.MbvError, match="turn 1: .*" + why):
            wire.turn_plan(22050, 24000, [good, k], limits=[None, limit])
    many = _turn([(3 * i, 2, 1) for i in range(_capi.TURN_MAX_SEGS - 3)], 20000, 20000, 0, 10, cap=30000)
    assert wire.turn_plan(22050, 24000, [good, many])[0] == 210
    with pytest.raises(_capi.MbvError, match="turn 2: more than 4096 segments"):
        wire.turn_plan(22050, 24000, [good, many, good])
    missing = _turn([(0, 40, 4)], 2000, 350, 0, 10)
    missing.segs = None
    with pytest.raises(_capi.MbvError, match="turn 0: n_segs"):
        wire.turn_plan(22050, 24000, [missing])
    L = _capi.lib()
    assert L.mbv_turn_plan(22050, 24000, 5, None, None, 0, None) == -1 and b"filter" in L.mbv_last_error(None)
    # a limiter inside its ranges whose halo window does not fit the LDS stage with this rate pair: 48 kHz -> 8 kHz reads
    # six inputs per output, and 255 + 1024 outputs of halo on top of the tile need more than the 16384 floats
    wide = (0.9, 255, 1024)
    for k in (good, also):
        k.chunk.pcm_capacity = 400
    good.chunk.in_avail, good.chunk.out_count, also.chunk.out_first, also.chunk.out_count = 2000, 5, 0, 100
    assert wire.turn_plan(48000, 8000, [good, also], limits=[None, (0.9, 255, 64)])[0] == 105
    assert wire.turn_plan(22050, 24000, [good, also], limits=[None, wide])[0] == 105      # (fits with this pair)
    with pytest.raises(_capi.MbvError, match="turn 1: .*halo window larger than the LDS stage"):
        wire.turn_plan(48000, 8000, [good, also], limits=[None, wide])


def test_assemble_turn_is_the_numpy_restatement():
    rng = np.random.RandomState(3)
    lengths, pauses = [40, 7, 300, 1, 129], [3, 0, 500, 1]
    waves = [rng.randn(n + 5).astype(np.float32) for n in lengths]          # (longer than valid: only n_s are read)
    for ramp in (0, 4, 64, 110):
        got = wire.assemble_turn([torch.from_numpy(w).view(1, 1, -1) for w in waves], lengths, pauses, ramp)
        want = turn_ref.assemble(waves, lengths, pauses, ramp)
        assert got.shape == (1, 1, 981) and got.dtype == torch.float32
        assert np.array_equal(got[0, 0].numpy().view(np.int32), want.view(np.int32)), ramp
    assert float(wire.assemble_turn([torch.ones(9)], [9], [], 4)[0, 0, 0]) == float(np.float32(1) / np.float32(5))
    assert wire.turn_ramp(64, 7) == 3 and wire.turn_ramp(64, 1) == 0 and wire.turn_ramp(4, 300) == 4
    with pytest.raises(ValueError):
        wire.assemble_turn([torch.ones(9)], [10], [], 0)
    with pytest.raises(ValueError):
        wire.assemble_turn([torch.ones(9), torch.ones(3)], [9, 3], [], 0)


def test_frames_of_a_turn_are_those_of_the_whole_turn():
    """20 ms framing over the pieces of a turn: the frames of `frame_pcm16` on the whole turn, ONE short frame at the end
    of the turn and none at a joint."""
    rate = 24000
    plan = wire.TurnPlan(22050, rate, 1 << 16)
    rng = random.Random(5)
    pcm = np.random.RandomState(1).randint(-30000, 30000, size=1 << 16).astype(np.int16)
    cutter, frames, pieces = wire.FrameCutter(rate), [], 0
    for s, n in enumerate([5000, 333, 7001]):
        plan.append(n, 700 if s else 0)
        for have in sorted(rng.sample(range(1, n), 3)) + [n]:
            plan.decoded(s, have)
            if s == 2 and have == n:
                plan.close()
            due = plan.wire_due()
            if due:
                frames += cutter.push(pcm[due[0]:due[0] + due[1]])
                plan.wired(due[0] + due[1])
                pieces += 1
    frames += cutter.close()
    total = plan.out_total()
    assert plan.done and pieces >= 6 and total % wire.chunk_size(rate) != 0
    assert frames == wire.frame_pcm16(pcm, rate, valid_samples=total)
    sizes = [len(base64.b64decode(f)) for f in frames]
    assert all(n == 2 * wire.chunk_size(rate) for n in sizes[:-1]) and 0 < sizes[-1] < 2 * wire.chunk_size(rate)
