"""What the loudness measurement costs: ljs_mb, 22 050 Hz, 24 000 Hz on the wire.  No bar is set on
the times; the bar is on the launch counts, which the records carry.

  measure       `net.loudness` on a waveform of 3 s and of 30 s, batch 1 and 16: us per call by device events around
                --launches back-to-back calls (at batch 1 the host's enqueue hides part of the kernel: what a service
                sees), and the wall time of ONE call that ends in a synchronise (the latency in front of a one-shot
                `service_pcm16(loudness=)`)
  service       one-shot `service_pcm16` of a 3 s utterance: `auto_normalize=True` (two launches: the peak, then the
                int16) against `loudness=Loudness()` (the measuring launch, then one int16 launch), ms per call that
                ends in a synchronise, alternating round by round.  `--parent` (with MBV_LIB naming a build of the
                parent commit) measures the `auto_normalize=True` call alone on that library, in a process of its own;
                the caller alternates the processes
  pooled_tick   16 concurrent streams of one 3 s utterance (258 z-frames; chunks 32, 64, 128, 34) in a `PcmPool`: ms
                per `step()` tick that ends in a synchronise, with every member measuring and with none, alternating,
                and the wire / loudness launches of every tick

    python scripts/loudness_timing.py [--reps 9] [--launches 200] [--out profiles/loudness_timing.jsonl]
    MBV_LIB=/path/to/parent/libmbistft_vits.so python scripts/loudness_timing.py --parent [--out ...]   (appends)
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
T_3S = 258
CHUNK, CAP = 32, 256


def med(v):
    return round(statistics.median(v), 4)


def speechlike(B, n, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(B, 1, n, generator=g) * 0.2 - 0.1).cuda()


def measure_call(net, B, seconds, launches, reps):
    wave = speechlike(B, int(seconds * MODEL_SR), B + seconds)
    for _ in range(5):
        net.loudness(wave, MODEL_SR)
    torch.cuda.synchronize()
    us, wall = [], []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            net.loudness(wave, MODEL_SR)
        e1.record()
        torch.cuda.synchronize()
        us.append(1e3 * e0.elapsed_time(e1) / launches)
        t0 = time.perf_counter()
        net.loudness(wave, MODEL_SR)
        torch.cuda.synchronize()
        wall.append(1e6 * (time.perf_counter() - t0))
    return dict(what="measure", batch=B, seconds=seconds, samples=wave.shape[-1], launches=launches, reps=reps,
                us_per_call=med(us), us_min=round(min(us), 2), us_max=round(max(us), 2), one_call_wall_us=med(wall))


def service_ms(net, o, reps, variants):
    """ms per one-shot service call that ends in a synchronise, the variants alternating round by round"""
    calls = dict(auto_normalize=lambda: wire.service_pcm16(net, o, None, MODEL_SR, RATE, auto_normalize=True))
    if "loudness" in variants:
        loud = wire.Loudness()
        calls["loudness"] = lambda: wire.service_pcm16(net, o, None, MODEL_SR, RATE, loudness=loud)
    res = {v: [] for v in variants}
    runs = {}
    for v in variants:
        for _ in range(5):
            calls[v]()
    torch.cuda.synchronize()
    for r in range(reps):
        for v in (variants if r % 2 == 0 else variants[::-1]):
            w0 = wire.wire_runs(net)
            m0 = net.loudness_runs() if "loudness" in variants else 0
            t0 = time.perf_counter()
            calls[v]()
            torch.cuda.synchronize()
            res[v].append(1e3 * (time.perf_counter() - t0))
            runs[v] = dict(wire=wire.wire_runs(net) - w0,
                           loudness=(net.loudness_runs() - m0) if "loudness" in variants else 0)
    return res, runs


def run_pool(net, zs, loudness):
    sts = [net.dec_stream(z, None, CHUNK, CAP) for z in zs]
    pp = wire.pcm_pool(net, net.stream_pool(), MODEL_SR, RATE)
    fol = [pp.add(st, loudness=loudness) for st in sts]
    ticks, wires, louds = [], [], []
    torch.cuda.synchronize()
    while len(pp):
        w0, m0 = wire.wire_runs(net), net.loudness_runs()
        t0 = time.perf_counter()
        pp.step()
        torch.cuda.synchronize()
        ticks.append(1e3 * (time.perf_counter() - t0))
        wires.append(wire.wire_runs(net) - w0)
        louds.append(net.loudness_runs() - m0)
    return ticks, wires, louds, fol


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--out", default=None)
    ap.add_argument("--label", default=None, help="a tag for the records of this process")
    ap.add_argument("--parent", action="store_true",
                    help="service_pcm16(auto_normalize=True) only (MBV_LIB: the parent's library); appends to --out")
    ap.add_argument("--service-only", action="store_true", help="the service records only; appends to --out")
    args = ap.parse_args()
    if args.reps < 7:
        raise SystemExit("--reps must be at least 7")
    if not torch.cuda.is_available():
        raise SystemExit("loudness_timing.py measures on the GPU; there is none here")
    net = make_net(CONFIG)[0]
    lines = []

    def emit(rec):
        if args.label:
            rec["label"] = args.label
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    g = torch.Generator().manual_seed(1)
    z = torch.randn(1, net.cfg.inter_channels, T_3S, generator=g).cuda()
    o = net.dec(z)[0]
    variants = ["auto_normalize"] if args.parent else ["auto_normalize", "loudness"]
    res, runs = service_ms(net, o, max(args.reps, 15), variants)
    rec = dict(what="service", library="parent" if args.parent else "this", samples=o.shape[-1], reps=max(args.reps, 15))
    for v in variants:
        rec[v + "_ms"] = med(res[v])
        rec[v + "_min_max_ms"] = [round(min(res[v]), 4), round(max(res[v]), 4)]
        rec[v + "_launches"] = runs[v]
    emit(rec)
    if not (args.parent or args.service_only):
        for seconds in (3, 30):
            for B in (1, 16):
                emit(measure_call(net, B, seconds, args.launches, args.reps))
        zs = [torch.randn(1, net.cfg.inter_channels, T_3S, generator=g).cuda() for _ in range(16)]
        measure = wire.Loudness(target=None)
        for loud in (measure, None, measure, None):
            run_pool(net, zs, loud)
        res = {True: [], False: []}
        for r in range(args.reps):
            for on in ((True, False) if r % 2 == 0 else (False, True)):
                res[on].append(run_pool(net, zs, measure if on else None))
        n_ticks = len(res[True][0][0])
        rec = dict(what="pooled_tick", streams=16, frames=T_3S, ticks=n_ticks, reps=args.reps)
        for on, key in ((False, "plain"), (True, "measuring")):
            rec[key + "_ticks_ms"] = [med([r[0][k] for r in res[on]]) for k in range(n_ticks)]
            rec[key + "_all_ticks_ms"] = med([sum(r[0]) for r in res[on]])
            rec[key + "_wire_runs_per_tick"] = res[on][0][1]
            rec[key + "_loudness_runs_per_tick"] = res[on][0][2]
        rec["all_ticks_ratio"] = round(rec["measuring_all_ticks_ms"] / rec["plain_all_ticks_ms"], 4)
        fol = res[True][-1][3]
        rec["final_lufs"] = [round(float(f.loudness[0]), 3) for f in fol[:2]]
        want = net.loudness(fol[0]._st.o, MODEL_SR)
        if not torch.equal(want.view(torch.int32), fol[0].loudness.view(torch.int32)):
            raise SystemExit("pooled_tick: the running loudness does not end at net.loudness: nothing is reported")
        emit(rec)
    if args.out:
        with open(args.out, "a" if (args.parent or args.service_only) else "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
