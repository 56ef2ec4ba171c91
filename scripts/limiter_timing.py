"""What the look-ahead limiter of the wire step costs: ljs_mb, 22 050 -> 24 000 Hz, `wire.Limiter()`
(0.9, 5 ms = 120 samples, 20 ms = 480 samples at 24 kHz).

Three measurements, each with and without the limiter on the same build in the same process, alternating round by
round.  The run without the limiter is the unchanged code path (`mbv_resample_pcm16_range` /
`mbv_resample_pcm16_chunks`) and serves as the baseline; no bar is set.

  pooled_tick   16 concurrent streams of one 3 s utterance (258 z-frames; chunks 32, 64, 128, 34) in a `PcmPool`:
                ms per `step(host=True)` tick (decode + ONE wire launch + one copy to the pinned buffer), host clock
                around a tick that ends in a device synchronise
  alone         one such stream through `stream_pcm16`: ms per `next()` + copy to the host, the same way
  wire_step     the wire launch alone, by device events around --launches back-to-back calls of the ranged entry on
                a waveform: us per call for 1, 16 and 512 rows of a 128-frame chunk (about 35 666 outputs per row),
                the largest chunk of the schedule.  With 1 and 16 rows the host's enqueue (about 0.3 ms of Python per
                call) hides the kernel, which is what a service sees; 512 rows keep the device busy and show the
                kernel itself.  This is where the halo recompute shows: at the defaults a workgroup computes
                256 + 2 * 120 + 480 = 976 resampled values for its 256 outputs

The limited and the unlimited bytes are compared where they must agree: the inputs are scaled so that nothing exceeds
the ceiling, where the limiter leaves every int16 as it is.  The script refuses to report when they differ.

    python scripts/limiter_timing.py [--reps 9] [--launches 200] [--out profiles/limiter_timing.jsonl]

The per-kernel view comes from a profiler run of its own, with no counters in it:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/limiter_timing.py --profile
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
CHUNK, CAP = 32, 256
QUIET_PEAK = 1e4                       # a static gain that keeps every sample below the ceiling: the bytes must agree


def make_z(net, lens, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(1, net.cfg.inter_channels, t, generator=g).cuda() for t in lens]


def run_pool(net, zs, limiter):
    """-> (ms per tick, wire launches per tick, bytes per stream)"""
    sts = [net.dec_stream(z, None, CHUNK, CAP) for z in zs]
    pp = wire.pcm_pool(net, net.stream_pool(), MODEL_SR, RATE)
    for st in sts:
        pp.add(st, peak=QUIET_PEAK, limiter=limiter)
    host = {id(st): [] for st in sts}
    ticks, runs = [], []
    torch.cuda.synchronize()
    while len(pp):
        r0 = wire.wire_runs(net)
        t0 = time.perf_counter()
        for st, _, piece in pp.step(host=True):
            host[id(st)].append(piece.copy())
        torch.cuda.synchronize()
        ticks.append(1e3 * (time.perf_counter() - t0))
        runs.append(wire.wire_runs(net) - r0)
    return ticks, runs, [np.concatenate(host[id(st)]) for st in sts]


def run_alone(net, z, limiter):
    st = net.dec_stream(z, None, CHUNK, CAP)
    pcm = wire.stream_pcm16(net, st, MODEL_SR, RATE, peak=QUIET_PEAK, limiter=limiter)
    ticks, host = [], []
    torch.cuda.synchronize()
    for _ in range(len(st)):
        t0 = time.perf_counter()
        host.append(next(pcm)[1][0].cpu().numpy())
        torch.cuda.synchronize()
        ticks.append(1e3 * (time.perf_counter() - t0))
    return ticks, [1] * len(ticks), [np.concatenate(host)]


def wire_step_us(net, rows, limiter, launches):
    """us per launch of the ranged entry over the outputs a 128-frame chunk makes final under the limiter (the same
    range for both variants), `rows` rows; -> (us, the int16 of the range)"""
    n = 256 * T_3S
    wave = (torch.rand(rows, n, generator=torch.Generator().manual_seed(rows)) * 0.2 - 0.1).cuda()
    lim = limiter.resolve(RATE) if limiter else None
    lag = wire.Limiter().resolve(RATE)[1]
    a = wire.limiter_ready(MODEL_SR, RATE, 256 * 96, n, lag)
    b = wire.limiter_ready(MODEL_SR, RATE, 256 * 224, n, lag)
    pcm = torch.zeros(rows, wire.resample_ready(MODEL_SR, RATE, n, n), device="cuda", dtype=torch.int16)
    running = torch.zeros(rows, device="cuda")

    def launch():
        net.resample_pcm16_range(wave, MODEL_SR, RATE, 256 * 224, a, b - a, pcm, running_peak=running, limiter=lim)

    for _ in range(20):
        launch()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        launch()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / launches, pcm[:, a:b].cpu().numpy()


def measure(name, fn, reps):
    lim = wire.Limiter()
    for limiter in (lim, None, lim, None):                            # warm-up: both variants' shapes, the bank
        fn(limiter)
    res = {True: [], False: []}
    for r in range(reps):
        for limited in ((True, False) if r % 2 == 0 else (False, True)):
            res[limited].append(fn(lim if limited else None))
    for a, b in zip(res[True][-1][2], res[False][-1][2]):
        if a.dtype != np.int16 or not np.array_equal(a, b):
            raise SystemExit("%s: limited and unlimited bytes differ on a signal below the ceiling: nothing is reported" % name)

    def med(limited, pick):
        return round(statistics.median(pick(r) for r in res[limited]), 3)

    n_ticks = len(res[True][0][0])
    rec = dict(what=name, config=CONFIG, model_sr=MODEL_SR, rate=RATE, limiter=list(lim.resolve(RATE)), ticks=n_ticks,
               reps=reps, bytes_equal=True)
    for limited, key in ((False, "unlimited"), (True, "limited")):
        rec[key + "_ticks_ms"] = [med(limited, lambda r, k=k: r[0][k]) for k in range(n_ticks)]
        rec[key + "_all_ticks_ms"] = med(limited, lambda r: sum(r[0]))
        rec[key + "_wire_runs_per_tick"] = res[limited][0][1]
    rec["all_ticks_ratio"] = round(rec["limited_all_ticks_ms"] / rec["unlimited_all_ticks_ms"], 3)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile", action="store_true", help="the wire step of 16 rows only, both variants (for rocprofv3)")
    args = ap.parse_args()
    if args.reps < 7:
        raise SystemExit("--reps must be at least 7")
    if not torch.cuda.is_available():
        raise SystemExit("limiter_timing.py measures on the GPU; there is none here")
    net = make_net(CONFIG)[0]
    if args.profile:
        for limiter in (wire.Limiter(), None):
            wire_step_us(net, 16, limiter, 50)
        return
    lines = []
    zs = make_z(net, [T_3S] * 16)
    lines.append(json.dumps(measure("pooled_tick", lambda lim: run_pool(net, zs, lim), args.reps)))
    print(lines[-1], flush=True)
    lines.append(json.dumps(measure("alone", lambda lim: run_alone(net, zs[0], lim), args.reps)))
    print(lines[-1], flush=True)
    lim = wire.Limiter()
    for rows in (1, 16, 512):
        us = {True: [], False: []}
        for r in range(args.reps):
            for limited in ((True, False) if r % 2 == 0 else (False, True)):
                t, got = wire_step_us(net, rows, lim if limited else None, args.launches)
                us[limited].append(t)
                if r == 0 and limited:
                    kept = got
                elif r == 0 and not np.array_equal(got, kept):
                    raise SystemExit("wire_step: limited and unlimited bytes differ: nothing is reported")
        rec = dict(what="wire_step", rows=rows, chunk_frames=128, limiter=list(lim.resolve(RATE)), launches=args.launches,
                   reps=args.reps, unlimited_us=round(statistics.median(us[False]), 2),
                   limited_us=round(statistics.median(us[True]), 2))
        rec["ratio"] = round(rec["limited_us"] / rec["unlimited_us"], 3)
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
