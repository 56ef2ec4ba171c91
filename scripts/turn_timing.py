"""Turns on the wire, timing: ljs_mb, 22 050 -> 24 000 Hz.

1. A pooled tick whose rows are turn rows against the same streams wired as plain members.  N streams of one 3 s
   utterance each (258 z-frames; chunks 32, 64, 128, 34), on the same build in the same process:

     members   every stream a plain member of a `PcmPool` (`mbv_resample_pcm16_chunks`, one launch per tick)
     turns     every stream the only segment of its own `Turn` (`mbv_resample_turns`, one launch per tick); the same
               samples pass through the segmented staging and the de-click ramps

   Both decode through the same `mbv_decode_chunks` call and hand their pieces over with `step(host=True)`.

2. A three-phrase reply.  The phrases are admitted one per tick as segments of one turn (the front half of a phrase
   runs when it is admitted), against the same tokens joined into ONE `infer_stream` request behind a plain follower.
   Reported: time to the first audio on the host, and the total until the last piece.  The two are different audio
   (three utterances with ramps and pauses against one utterance), so nothing is compared bytewise here.

The variants alternate round by round (the order within a round alternates too); medians over --reps rounds, with the
fastest and slowest round kept beside them.

    python scripts/turn_timing.py [--reps 9] [--out profiles/turn_timing.jsonl]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from gpu_util import make_net                      # noqa: E402
from mb_istft_vits_amd import wire                 # noqa: E402
from mb_istft_vits_amd.models import Request       # noqa: E402

CONFIG = "ljs_mb_istft_vits"
MODEL_SR, RATE = 22050, 24000
T_3S = 258
CHUNK, CAP = 32, 256
PHRASES = [12, 30, 18]                             # tokens of the three phrases of the reply
PAUSE_MS = 150.0


def stats(values):
    return dict(median=round(statistics.median(values), 3), min=round(min(values), 3), max=round(max(values), 3))


# ---------------------------------------------------------------------------------------------- 1. the pooled tick
def tick_round(net, zs, turns):
    """-> (ms per tick, wire launches per tick, int16 per stream)"""
    sts = [net.dec_stream(z, None, CHUNK, CAP) for z in zs]
    pp = wire.pcm_pool(net, net.stream_pool(), MODEL_SR, RATE)
    key = {}
    for st in sts:
        if turns:
            t = pp.add_turn(wire.resample_ready(MODEL_SR, RATE, st.o.shape[-1], st.o.shape[-1]), ramp_ms=5.0)
            t.append(st)
            t.close()
            key[id(t)] = id(st)
        else:
            pp.add(st)
            key[id(st)] = id(st)
    host = {id(st): [] for st in sts}
    ticks, runs = [], []
    torch.cuda.synchronize()
    while len(pp):
        r0 = wire.wire_runs(net)
        t0 = time.perf_counter()
        for who, _, piece in pp.step(host=True):
            host[key[id(who)]].append(piece.copy())
        torch.cuda.synchronize()
        ticks.append(1e3 * (time.perf_counter() - t0))
        runs.append(wire.wire_runs(net) - r0)
    return ticks, runs, [np.concatenate(host[id(st)]) for st in sts]


def measure_tick(net, n, reps):
    g = torch.Generator().manual_seed(n)
    zs = [torch.randn(1, net.cfg.inter_channels, T_3S, generator=g).cuda() for _ in range(n)]
    for turns in (True, False, True, False):
        tick_round(net, zs, turns)
    res = {True: [], False: []}
    for r in range(reps):
        for turns in ((True, False) if r % 2 == 0 else (False, True)):
            res[turns].append(tick_round(net, zs, turns))
    # the two differ only by the ramps: the samples outside them are the same bytes
    ramp = int(round(5e-3 * MODEL_SR * RATE / MODEL_SR)) + 80
    for a, b in zip(res[True][-1][2], res[False][-1][2]):
        if len(a) != len(b) or not np.array_equal(a[ramp:-ramp], b[ramp:-ramp]):
            raise SystemExit("turn rows and plain members differ outside the ramps (%d streams): nothing is reported" % n)
    n_ticks = len(res[True][0][0])
    rec = dict(what="pooled_tick", config=CONFIG, model_sr=MODEL_SR, rate=RATE, streams=n, frames=T_3S,
               chunk_frames=CHUNK, max_chunk_frames=CAP, ticks=n_ticks, reps=reps, bytes_equal_outside_ramps=True)
    for turns, name in ((True, "turns"), (False, "members")):
        rec[name + "_ticks_ms"] = [stats([r[0][k] for r in res[turns]]) for k in range(n_ticks)]
        rec[name + "_all_ticks_ms"] = stats([sum(r[0]) for r in res[turns]])
        rec[name + "_wire_runs_per_tick"] = res[turns][0][1]
    rec["all_ticks_ratio"] = round(rec["turns_all_ticks_ms"]["median"] / rec["members_all_ticks_ms"]["median"], 3)
    return rec


# ---------------------------------------------------------------------------------------------- 2. the reply
def ids(n, seed):
    return torch.randint(1, 59, (n,), generator=torch.Generator().manual_seed(seed))


def reply_round(net, as_turn):
    """-> (ms to the first audio on the host, ms to the last piece, wire samples)"""
    phrases = [ids(n, 70 + k) for k, n in enumerate(PHRASES)]
    pp = wire.pcm_pool(net, net.stream_pool(), MODEL_SR, RATE)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    first, samples = None, 0
    if as_turn:
        turn = pp.add_turn(1 << 21)
        for k, x in enumerate(phrases):
            turn.admit([Request(x, noise_scale=0.5, seed=70 + k, chunk_frames=CHUNK, max_chunk_frames=CAP)],
                       pauses_ms=[PAUSE_MS if k else 0.0])
            if k == len(phrases) - 1:
                turn.close()
            for _, _, piece in pp.step(host=True):
                samples += len(piece)
                if first is None and len(piece):
                    first = 1e3 * (time.perf_counter() - t0)
    else:
        pp.admit([Request(torch.cat(phrases), noise_scale=0.5, seed=70, chunk_frames=CHUNK, max_chunk_frames=CAP)])
    while len(pp):
        for _, _, piece in pp.step(host=True):
            samples += len(piece)
            if first is None and len(piece):
                first = 1e3 * (time.perf_counter() - t0)
    torch.cuda.synchronize()
    return first, 1e3 * (time.perf_counter() - t0), samples


def measure_reply(net, reps):
    for as_turn in (True, False, True, False):
        reply_round(net, as_turn)
    res = {True: [], False: []}
    for r in range(reps):
        for as_turn in ((True, False) if r % 2 == 0 else (False, True)):
            res[as_turn].append(reply_round(net, as_turn))
    rec = dict(what="three_phrase_reply", config=CONFIG, model_sr=MODEL_SR, rate=RATE, phrase_tokens=PHRASES,
               pause_ms=PAUSE_MS, chunk_frames=CHUNK, max_chunk_frames=CAP, reps=reps)
    for as_turn, name in ((True, "turn"), (False, "one_request")):
        rec[name + "_first_audio_ms"] = stats([r[0] for r in res[as_turn]])
        rec[name + "_total_ms"] = stats([r[1] for r in res[as_turn]])
        rec[name + "_wire_samples"] = res[as_turn][0][2]
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.reps < 7:
        raise SystemExit("--reps must be at least 7")
    net = make_net(CONFIG)[0]
    lines = []
    for n in (1, 4, 16, 64):
        lines.append(json.dumps(measure_tick(net, n, args.reps)))
        print(lines[-1], flush=True)
    lines.append(json.dumps(measure_reply(net, args.reps)))
    print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
