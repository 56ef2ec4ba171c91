"""Pooled streaming decode timing: ljs_mb, N concurrent streams, default and split-K modes.

Workloads: N in {1, 2, 4, 16, 64} streams of one 3 s utterance each (258 z-frames, the §7.3 case; chunks 32, 64,
128, 34), and a mixed set of 16 utterances across all four length classes.  Per workload and mode, every step (the
next chunk of every stream that has one) is obtained two ways on the same build in the same process:

  pooled      one `pool.step()`                       (one `mbv_decode_chunks` call)
  sequential  `next(st)` for each of those streams    (one `mbv_decode_range` call each)

The variants alternate round by round (the order within a round alternates too); each step ends in a device
synchronisation and is timed by the host clock.  Reported per workload and mode, medians over --reps rounds:

  steps_ms           ms per step, step by step
  all_steps_ms       their sum: every stream decoded to its end
  first_audio_ms     from the start of step 0 to the first chunk of the LAST-served stream on the host
  runs_per_step      decoder runs per step (`mbv_decoder_runs`)

The two variants' waveforms are compared bitwise (default mode) before anything is reported.

    python scripts/pool_timing.py [--reps 9] [--out profiles/pool_timing.jsonl]

The per-kernel view comes from a profiler run of its own, with no counters in it:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/pool_timing.py --profile
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

CONFIG = "ljs_mb_istft_vits"
T_3S = 258
MIXED = [9, 16, 40, 64, 100, 200, 258, 300, 12, 30, 120, 400, 60, 17, 257, 150]
CHUNK, CAP = 32, 256


def make_z(net, lens, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(1, net.cfg.inter_channels, t, generator=g).cuda() for t in lens]


def run_round(net, zs, pooled):
    """-> (ms per step, ms to the first audio of the last-served stream, runs per step, the waveforms)"""
    sts = [net.dec_stream(z, None, CHUNK, CAP) for z in zs]
    pool = net.stream_pool()
    for st in sts:
        pool.add(st)
    n_steps = max(len(st) for st in sts)
    steps, runs, first_audio = [], [], None
    torch.cuda.synchronize()
    for k in range(n_steps):
        r0 = net.decoder_runs()
        t0 = time.perf_counter()
        if pooled:
            last = pool.step()[-1][2]
        else:
            for st in sts:
                if k < len(st):
                    last = next(st)[1]
        if k == 0:
            last.cpu()
            first_audio = 1e3 * (time.perf_counter() - t0)
        torch.cuda.synchronize()
        steps.append(1e3 * (time.perf_counter() - t0))
        runs.append(net.decoder_runs() - r0)
    return steps, first_audio, runs, [st.o for st in sts]


def measure(net, lens, mode, reps):
    zs = make_z(net, lens)
    net.set_option("splitk", int(mode == "splitk"))
    try:
        for pooled in (True, False, True, False):                 # warm-up: both variants' shapes, the arena
            run_round(net, zs, pooled)
        res = {True: [], False: []}
        for r in range(reps):
            for pooled in ((True, False) if r % 2 == 0 else (False, True)):
                res[pooled].append(run_round(net, zs, pooled))
    finally:
        net.set_option("splitk", 0)
    same = all(torch.equal(a, b) for a, b in zip(res[True][-1][3], res[False][-1][3]))
    if mode == "default" and not same:
        raise SystemExit("pooled and sequential waveforms differ in the default mode")

    def med(variant, pick):
        return round(statistics.median(pick(r) for r in res[variant]), 3)

    n_steps = len(res[True][0][0])
    rec = dict(config=CONFIG, mode=mode, streams=len(lens), frames=lens if len(set(lens)) > 1 else lens[0],
               chunk_frames=CHUNK, max_chunk_frames=CAP, steps=n_steps, reps=reps, bitwise_equal=same)
    for variant, name in ((True, "pooled"), (False, "sequential")):
        rec[name + "_steps_ms"] = [med(variant, lambda r, k=k: r[0][k]) for k in range(n_steps)]
        rec[name + "_all_steps_ms"] = med(variant, lambda r: sum(r[0]))
        rec[name + "_first_audio_ms"] = med(variant, lambda r: r[1])
        rec[name + "_runs_per_step"] = res[variant][0][2]
    rec["first_step_ratio"] = round(rec["sequential_steps_ms"][0] / rec["pooled_steps_ms"][0], 3)
    rec["all_steps_ratio"] = round(rec["sequential_all_steps_ms"] / rec["pooled_all_steps_ms"], 3)
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
