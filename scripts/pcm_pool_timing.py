"""Pooled wire output timing: ljs_mb, 22 050 -> 24 000 Hz, N concurrent streams, default and split-K modes.

Workloads: N in {1, 2, 4, 16, 64} streams of one 3 s utterance each (258 z-frames; chunks 32, 64, 128, 34), and a
mixed set of 16 utterances across all four length classes (the workloads of scripts/pool_timing.py).  Per workload
and mode, every service tick (the next chunk of every stream that has one, as int16 on the host) is obtained two
ways on the same build in the same process:

  per_stream  `pool.step()`, then `next(pcm)` and a copy to the host for each of those streams
              (one `mbv_resample_pcm16_range` launch and one device-to-host copy per stream)
  pooled      one `PcmPool.step(host=True)`
              (one `mbv_resample_pcm16_chunks` launch, one copy into one pinned buffer, one event wait)

Both decode through the same `mbv_decode_chunks` call; only the wire step differs.  The variants alternate round by
round (the order within a round alternates too); each tick ends with its pieces on the host and is timed by the
host clock.  Reported per workload and mode, medians over --reps rounds:

  ticks_ms           ms per tick, tick by tick
  all_ticks_ms       their sum: every stream served to its end
  first_frame_ms     from the start of tick 0 to the first piece of the LAST-served stream on the host
  wire_runs_per_tick resample / int16 launches per tick (`mbv_wire_runs`)

The two variants' bytes are compared before anything is reported; the script refuses to report when they differ.

    python scripts/pcm_pool_timing.py [--reps 9] [--out profiles/pcm_pool_timing.jsonl]

The per-kernel view comes from a profiler run of its own, with no counters in it:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/pcm_pool_timing.py --profile
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
from gpu_util import make_net          # noqa: E402
from mb_istft_vits_amd import wire     # noqa: E402

CONFIG = "ljs_mb_istft_vits"
MODEL_SR, RATE = 22050, 24000
T_3S = 258
MIXED = [9, 16, 40, 64, 100, 200, 258, 300, 12, 30, 120, 400, 60, 17, 257, 150]
CHUNK, CAP = 32, 256


def make_z(net, lens, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(1, net.cfg.inter_channels, t, generator=g).cuda() for t in lens]


def run_round(net, zs, pooled):
    """-> (ms per tick, ms to the first piece of the last-served stream, wire launches per tick, bytes per stream)"""
    sts = [net.dec_stream(z, None, CHUNK, CAP) for z in zs]
    pool = net.stream_pool()
    host = {id(st): [] for st in sts}
    if pooled:
        pp = wire.pcm_pool(net, pool, MODEL_SR, RATE)
        for st in sts:
            pp.add(st)
    else:
        for st in sts:
            pool.add(st)
        pcms = [wire.stream_pcm16(net, st, MODEL_SR, RATE) for st in sts]
    n_ticks = max(len(st) for st in sts)
    ticks, runs, first_frame = [], [], None
    torch.cuda.synchronize()
    for k in range(n_ticks):
        r0 = wire.wire_runs(net)
        t0 = time.perf_counter()
        if pooled:
            for st, _, piece in pp.step(host=True):
                host[id(st)].append(piece.copy())         # (what FrameCutter.push does with it)
        else:
            pool.step()
            for st, p in zip(sts, pcms):
                if k < len(st):
                    host[id(st)].append(next(p)[1][0].cpu().numpy())
        if k == 0:
            first_frame = 1e3 * (time.perf_counter() - t0)
        torch.cuda.synchronize()
        ticks.append(1e3 * (time.perf_counter() - t0))
        runs.append(wire.wire_runs(net) - r0)
    return ticks, first_frame, runs, [np.concatenate(host[id(st)]) for st in sts]


def measure(net, lens, mode, reps):
    zs = make_z(net, lens)
    net.set_option("splitk", int(mode == "splitk"))
    try:
        for pooled in (True, False, True, False):                 # warm-up: both variants' shapes, the arena, the bank
            run_round(net, zs, pooled)
        res = {True: [], False: []}
        for r in range(reps):
            for pooled in ((True, False) if r % 2 == 0 else (False, True)):
                res[pooled].append(run_round(net, zs, pooled))
    finally:
        net.set_option("splitk", 0)
    for a, b in zip(res[True][-1][3], res[False][-1][3]):
        if a.dtype != np.int16 or not np.array_equal(a, b):
            raise SystemExit("pooled and per-stream wire bytes differ (%s, %d streams): nothing is reported" % (mode, len(lens)))

    def med(variant, pick):
        return round(statistics.median(pick(r) for r in res[variant]), 3)

    n_ticks = len(res[True][0][0])
    rec = dict(config=CONFIG, model_sr=MODEL_SR, rate=RATE, mode=mode, streams=len(lens),
               frames=lens if len(set(lens)) > 1 else lens[0], chunk_frames=CHUNK, max_chunk_frames=CAP, ticks=n_ticks,
               reps=reps, bytes_equal=True)
    for variant, name in ((True, "pooled"), (False, "per_stream")):
        rec[name + "_ticks_ms"] = [med(variant, lambda r, k=k: r[0][k]) for k in range(n_ticks)]
        rec[name + "_all_ticks_ms"] = med(variant, lambda r: sum(r[0]))
        rec[name + "_first_frame_ms"] = med(variant, lambda r: r[1])
        rec[name + "_wire_runs_per_tick"] = res[variant][0][2]
    rec["first_tick_ratio"] = round(rec["per_stream_ticks_ms"][0] / rec["pooled_ticks_ms"][0], 3)
    rec["all_ticks_ratio"] = round(rec["per_stream_all_ticks_ms"] / rec["pooled_all_ticks_ms"], 3)
    rec["first_frame_ratio"] = round(rec["per_stream_first_frame_ms"] / rec["pooled_first_frame_ms"], 3)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile", action="store_true", help="N = 16, default mode, a few rounds only (for rocprofv3)")
    args = ap.parse_args()
    if args.reps < 7:
        raise SystemExit("--reps must be at least 7")
    net = make_net(CONFIG)[0]
    if args.profile:
        zs = make_z(net, [T_3S] * 16)
        for _ in range(3):
            run_round(net, zs, True)
            run_round(net, zs, False)
        torch.cuda.synchronize()
        return
    lines = []
    for mode in ("default", "splitk"):
        for lens in [[T_3S] * n for n in (1, 2, 4, 16, 64)] + [MIXED]:
            lines.append(json.dumps(measure(net, lens, mode, args.reps)))
            print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
