"""What barge-in costs and saves on the wire path: ljs_mb, 22 050 -> 24 000 Hz.

  pooled_tick   eight concurrent streams of one 3 s utterance (258 z-frames; chunks 32, 64, 128, 34) in a `PcmPool`:
                ms of the second tick (`step()` + device synchronise, host clock), with no fading member and with ONE
                member revoked just before it.  The fade is long (3 s), so the member still wires every output of the
                tick, each through the ramp: the work is the same and the difference is the ramp and its table alone.
                Measured in `--sets` sets of `--reps` rounds, the variants alternating round by round; the spread of
                the unfaded variant's set medians is the run-to-run spread the difference is read against.
                `--parent` (with MBV_LIB naming a build of the parent commit) measures the unfaded tick on that
                library: the same tick before the fade existed.
  revoke        a 10 s request (861 z-frames) through `stream_pcm16`, played to its end, and revoked with the default
                5 ms fade once 1 s of audio (24 000 samples) has been handed out: decoder runs and wall time (host
                clock, ends in a device synchronise) of each.

    python scripts/barge_in_timing.py [--reps 15] [--sets 3] [--out profiles/barge_in_timing.jsonl]
    MBV_LIB=/path/to/parent/libmbistft_vits.so python scripts/barge_in_timing.py --parent

Every run appends its lines to --out.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from gpu_util import make_net          # noqa: E402
from mb_istft_vits_amd import wire     # noqa: E402

CONFIG = "ljs_mb_istft_vits"
MODEL_SR, RATE = 22050, 24000
T_3S, T_10S = 258, 861
CHUNK, CAP = 32, 256
N_STREAMS = 8
LONG_FADE_MS = 3000.0


def make_z(net, lens, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(1, net.cfg.inter_channels, t, generator=g).cuda() for t in lens]


def second_tick_ms(net, zs, fading):
    """ms of the pool's second tick; `fading`: member 0 is revoked (a long fade) just before it"""
    pp = wire.pcm_pool(net, net.stream_pool(), MODEL_SR, RATE)
    fol = [pp.add(net.dec_stream(z, None, CHUNK, CAP)) for z in zs]
    pp.step()
    if fading:
        pp.revoke(fol[0], fade_ms=LONG_FADE_MS)
    torch.cuda.synchronize()
    r0 = wire.wire_runs(net)
    t0 = time.perf_counter()
    out = pp.step()
    torch.cuda.synchronize()
    ms = 1e3 * (time.perf_counter() - t0)
    assert wire.wire_runs(net) - r0 == 1 and len(out) == len(zs)
    assert sum(v.numel() for _, _, v in out) == len(zs) * out[1][2].numel()      # the fading member wires as much
    return ms


def pooled_tick(net, reps, sets, parent):
    zs = make_z(net, [T_3S] * N_STREAMS)
    variants = (False,) if parent else (False, True)
    for fading in variants * 3:                                           # warm-up: shapes, the bank, the pinned paths
        second_tick_ms(net, zs, fading)
    meds = {v: [] for v in variants}
    every = {v: [] for v in variants}
    for _ in range(sets):
        res = {v: [] for v in variants}
        for r in range(reps):
            for fading in (variants if r % 2 == 0 else variants[::-1]):
                res[fading].append(second_tick_ms(net, zs, fading))
        for v in variants:
            meds[v].append(statistics.median(res[v]))
            every[v] += res[v]
    rec = dict(what="pooled_tick", build="parent" if parent else "this", config=CONFIG, model_sr=MODEL_SR, rate=RATE,
               streams=N_STREAMS, tick=1, reps=reps, sets=sets)
    for v, key in ((False, "unfaded"), (True, "one_fading")):
        if v in meds:
            rec[key + "_ms"] = round(statistics.median(every[v]), 4)
            rec[key + "_set_medians_ms"] = [round(m, 4) for m in meds[v]]
            rec[key + "_min_max_ms"] = [round(min(every[v]), 4), round(max(every[v]), 4)]
    rec["unfaded_spread_ms"] = round(max(meds[False]) - min(meds[False]), 4)
    return rec


def play(net, z, revoke_after):
    """-> (ms, decoder runs, samples handed out); `revoke_after`: revoke once that many samples are out (None: never)"""
    f = wire.stream_pcm16(net, net.dec_stream(z, None, CHUNK, CAP), MODEL_SR, RATE)
    torch.cuda.synchronize()
    d0 = net.decoder_runs()
    t0 = time.perf_counter()
    out = 0
    for a, piece in f:
        out = a + piece.shape[1]
        if revoke_after is not None and not f.revoked and out >= revoke_after:
            f.revoke()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), net.decoder_runs() - d0, out


def revoke(net, reps):
    z = make_z(net, [T_10S], seed=1)[0]
    for after in (None, RATE, None, RATE):
        play(net, z, after)
    res = {None: [], RATE: []}
    for r in range(reps):
        for after in ((None, RATE) if r % 2 == 0 else (RATE, None)):
            res[after].append(play(net, z, after))
    rec = dict(what="revoke", build="this", config=CONFIG, model_sr=MODEL_SR, rate=RATE, frames=T_10S,
               revoke_after_samples=RATE, fade_ms=5.0, reps=reps)
    for after, key in ((None, "played_out"), (RATE, "revoked")):
        rec[key + "_ms"] = round(statistics.median(m for m, _, _ in res[after]), 3)
        rec[key + "_min_max_ms"] = [round(min(m for m, _, _ in res[after]), 3), round(max(m for m, _, _ in res[after]), 3)]
        rec[key + "_decoder_runs"] = res[after][0][1]
        rec[key + "_samples"] = res[after][0][2]
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--sets", type=int, default=3)
    ap.add_argument("--parent", action="store_true", help="the unfaded pooled tick only (MBV_LIB: the parent's library)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "barge_in_timing.jsonl"))
    args = ap.parse_args()
    if args.reps < 7 or args.sets < 3:
        raise SystemExit("--reps must be at least 7 and --sets at least 3")
    if not torch.cuda.is_available():
        raise SystemExit("barge_in_timing.py measures on the GPU; there is none here")
    net = make_net(CONFIG)[0]
    lines = [json.dumps(pooled_tick(net, args.reps, args.sets, args.parent))]
    print(lines[-1], flush=True)
    if not args.parent:
        lines.append(json.dumps(revoke(net, args.reps)))
        print(lines[-1], flush=True)
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
