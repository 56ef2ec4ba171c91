"""What G.711 on the wire costs: ljs_mb, down to the telephone rate from 22 050 and 16 000 Hz,
kaiser_best, for the three encodings of the wire step ("pcm16", "ulaw", "alaw").

The int16 path is the code of the parent commit (the G.711 epilogue is a template parameter that it does not take) and
serves as the yardstick in the same run; the variants alternate round by round.  No bar is set.

  pooled_tick   16 concurrent streams of one 3 s utterance (258 z-frames; chunks 32, 64, 128, 34) in a `PcmPool`:
                ms per `step(host=True)` tick (decode + ONE wire launch + one copy to the pinned buffer), host clock
                around a tick that ends in a device synchronise
  wire_step     the ranged entry alone, by device events around --launches back-to-back calls: us per call for 1, 16
                and 512 rows of the outputs a 128-frame chunk makes final.  With 1 and 16 rows the host's enqueue hides
                the kernel, which is what a service sees; 512 rows keep the device busy and show the kernel itself
  live_input    the live-input launch (`mbv_resample_ranges`) alone, the same way: 16 and 512 recordings of 3 s at
                8 kHz resampled to 22 050 Hz, int16 rows against mu-law rows

The bytes are compared where they must agree: the G.711 output is `g711_ref.encode` of the int16 output, and the
mu-law input gives bitwise the samples of the int16 recording it decodes to.  The script refuses to report otherwise.

    python scripts/g711_timing.py [--reps 9] [--launches 200] [--out profiles/g711_timing.jsonl]
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
import g711_ref                              # noqa: E402
from gpu_util import make_net                # noqa: E402
from mb_istft_vits_amd import _capi, wire    # noqa: E402

CONFIG = "ljs_mb_istft_vits"
RATE = 8000
PAIRS = [(22050, RATE), (16000, RATE)]
ENCODINGS = ("pcm16", "ulaw", "alaw")
T_3S = 258
CHUNK, CAP = 32, 256


def make_z(net, lens, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(1, net.cfg.inter_channels, t, generator=g).cuda() for t in lens]


def run_pool(net, zs, model_sr, encoding):
    """-> (ms per tick, wire launches per tick, samples per stream)"""
    sts = [net.dec_stream(z, None, CHUNK, CAP) for z in zs]
    pp = wire.pcm_pool(net, net.stream_pool(), model_sr, RATE, encoding=encoding)
    for st in sts:
        pp.add(st, peak=1.0)
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


def wire_step_us(net, rows, model_sr, encoding, launches):
    """us per launch of the ranged entry over the outputs a 128-frame chunk makes final; -> (us, the stored range)"""
    n = 256 * T_3S
    wave = (torch.rand(rows, n, generator=torch.Generator().manual_seed(rows)) * 1.6 - 0.8).cuda()
    a = wire.resample_ready(model_sr, RATE, 256 * 96, n)
    b = wire.resample_ready(model_sr, RATE, 256 * 224, n)
    out = torch.zeros(rows, wire.resample_ready(model_sr, RATE, n, n), device="cuda",
                      dtype=torch.int16 if encoding == "pcm16" else torch.uint8)
    running = torch.zeros(rows, device="cuda")

    def launch():
        net.resample_pcm16_range(wave, model_sr, RATE, 256 * 224, a, b - a, out, running_peak=running, encoding=encoding)

    for _ in range(20):
        launch()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        launch()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / launches, out[:, a:b].cpu().numpy()


def live_input_us(net, rows, ulaw, launches, in_sr=8000, model_sr=22050):
    """us per `mbv_resample_ranges` launch over `rows` closed recordings of 3 s; -> (us, the model-rate samples)"""
    n = 3 * in_sr
    rs = np.random.RandomState(rows)
    data = rs.randint(0, 256, size=(rows, n)).astype(np.uint8)
    raw = torch.from_numpy(data if ulaw else g711_ref.decode(data, "ulaw")).cuda()
    width = wire.resample_ready(in_sr, model_sr, n, n)
    out = torch.zeros(rows, width, device="cuda")
    table = (_capi.MbvResampleRange * rows)()
    for b, r in enumerate(table):
        r.wave, r.wave_dtype = raw[b].data_ptr(), _capi.WAVE_ULAW if ulaw else _capi.WAVE_PCM16
        r.in_avail, r.in_total, r.out_first, r.out_count = n, n, 0, width
        r.out, r.out_capacity = out[b].data_ptr(), width

    def launch():
        net.resample_ranges(table, in_sr, model_sr)

    for _ in range(20):
        launch()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        launch()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / launches, out.cpu().numpy()


def rounds(variants, fn, reps):
    """fn(variant) `reps` times per variant, the order rotating round by round; -> {variant: [results]}"""
    for v in variants + variants:                                     # warm-up: every variant's shapes, the bank
        fn(v)
    res = {v: [] for v in variants}
    for r in range(reps):
        k = r % len(variants)
        for v in variants[k:] + variants[:k]:
            res[v].append(fn(v))
    return res


def check_bytes(what, res):
    """the G.711 results are the encoded int16 results"""
    base = res["pcm16"][-1][-1]
    base = base if isinstance(base, list) else [base]
    for law in ("ulaw", "alaw"):
        got = res[law][-1][-1]
        for a, b in zip(got if isinstance(got, list) else [got], base):
            if a.dtype != np.uint8 or not np.array_equal(a, g711_ref.encode(b, law)):
                raise SystemExit("%s: the %s bytes are not the encoded int16 samples: nothing is reported" % (what, law))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.reps < 7:
        raise SystemExit("--reps must be at least 7")
    if not torch.cuda.is_available():
        raise SystemExit("g711_timing.py measures on the GPU; there is none here")
    net = make_net(CONFIG)[0]
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    variants = list(ENCODINGS)
    zs = make_z(net, [T_3S] * 16)
    for model_sr, rate in PAIRS:
        res = rounds(variants, lambda enc: run_pool(net, zs, model_sr, enc), args.reps)
        check_bytes("pooled_tick", res)
        rec = dict(what="pooled_tick", config=CONFIG, model_sr=model_sr, rate=rate, streams=16, reps=args.reps,
                   ticks=len(res["pcm16"][0][0]), bytes_equal=True)
        for enc in variants:
            all_ms = [sum(r[0]) for r in res[enc]]
            rec[enc + "_all_ticks_ms"] = round(statistics.median(all_ms), 3)
            rec[enc + "_all_ticks_ms_min_max"] = [round(min(all_ms), 3), round(max(all_ms), 3)]
            rec[enc + "_wire_runs_per_tick"] = res[enc][0][1]
        for enc in variants[1:]:
            rec[enc + "_ratio"] = round(rec[enc + "_all_ticks_ms"] / rec["pcm16_all_ticks_ms"], 3)
        emit(rec)
    for model_sr, rate in PAIRS:
        for rows in (1, 16, 512):
            res = rounds(variants, lambda enc: wire_step_us(net, rows, model_sr, enc, args.launches), args.reps)
            check_bytes("wire_step", res)
            rec = dict(what="wire_step", model_sr=model_sr, rate=rate, rows=rows, chunk_frames=128,
                       launches=args.launches, reps=args.reps, bytes_equal=True)
            for enc in variants:
                us = [r[0] for r in res[enc]]
                rec[enc + "_us"] = round(statistics.median(us), 2)
                rec[enc + "_us_min_max"] = [round(min(us), 2), round(max(us), 2)]
            for enc in variants[1:]:
                rec[enc + "_ratio"] = round(rec[enc + "_us"] / rec["pcm16_us"], 3)
            emit(rec)
    for rows in (16, 512):
        res = rounds([False, True], lambda ulaw: live_input_us(net, rows, ulaw, args.launches), args.reps)
        if not np.array_equal(res[False][-1][1].view(np.int32), res[True][-1][1].view(np.int32)):
            raise SystemExit("live_input: the mu-law rows do not give the int16 rows' samples: nothing is reported")
        rec = dict(what="live_input", in_sr=8000, model_sr=22050, rows=rows, seconds=3, launches=args.launches,
                   reps=args.reps, samples_equal=True)
        for ulaw, key in ((False, "int16"), (True, "ulaw")):
            us = [r[0] for r in res[ulaw]]
            rec[key + "_us"] = round(statistics.median(us), 2)
            rec[key + "_us_min_max"] = [round(min(us), 2), round(max(us), 2)]
        rec["ulaw_ratio"] = round(rec["ulaw_us"] / rec["int16_us"], 3)
        emit(rec)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
