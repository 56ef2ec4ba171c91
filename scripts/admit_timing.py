"""Pooled admission timing: ljs_mb, N requests admitted at once, default and split-K modes.

Workloads: N in {1, 2, 4, 16, 64} requests of 100 tokens each, and a ragged mix of 16 text lengths on both sides of
the class cut.  Per workload and mode the streams are obtained two ways on the same build in the same process:

  pooled      one `net.infer_streams(requests)`       (one padded run per class, one host read-back)
  sequential  `net.infer_stream(...)` per request     (one launch chain and one read-back each)

The variants alternate round by round (the order within a round alternates too).  A round is timed by the host clock
to a final device synchronisation — host overhead and the read-backs are what admission costs — and by a pair of HIP
events round the same calls.  Reported per workload and mode, medians over --reps rounds:

  wall_ms            host clock, first call to the end of the last kernel
  event_ms           HIP events round the same span
  runs               text-encoder runs (`mbv_encoder_runs`)
  host_syncs         synchronising calls torch reports (sync debug mode), one counting round: copies from pageable
                     host memory and the read-backs
  pooled_draws_only_ms   the N per-request prior draws of the pooled path timed alone

The two variants' streams are compared bitwise (default mode) before anything is reported.

    python scripts/admit_timing.py [--reps 9] [--out profiles/admit_timing.jsonl]

The per-kernel view and the launch counts come from profiler runs of their own, with no counters in them:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/admit_timing.py --profile pooled
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/admit_timing.py --profile sequential
"""
import argparse
import json
import os
import statistics
import sys
import time
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from gpu_util import make_net          # noqa: E402
from mb_istft_vits_amd.models import Request          # noqa: E402

CONFIG = "ljs_mb_istft_vits"
T_TEXT = 100
MIXED = [9, 16, 40, 64, 100, 200, 256, 300, 12, 30, 120, 400, 60, 17, 257, 150]
PROFILE_ROUNDS = 4


def make_requests(lens, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [Request(torch.randint(1, 59, (t,), generator=g), noise_scale=0.667, noise_scale_w=0.8) for t in lens]


def admit(net, reqs, pooled):
    if pooled:
        return net.infer_streams(reqs)
    return [net.infer_stream(r.x[None].cuda(), torch.tensor([r.x.numel()]).cuda(), None, r.noise_scale, r.length_scale,
                             r.noise_scale_w) for r in reqs]


def run_round(net, reqs, pooled, seed=3):
    """-> (wall ms, event ms, encoder runs, the streams)"""
    torch.manual_seed(seed)
    torch.cuda.manual_seed(seed)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    r0 = net.encoder_runs()
    t0 = time.perf_counter()
    e0.record()
    sts = admit(net, reqs, pooled)
    e1.record()
    torch.cuda.synchronize()
    wall = 1e3 * (time.perf_counter() - t0)
    return wall, e0.elapsed_time(e1), net.encoder_runs() - r0, sts


def draws_only(net, frames, reps):
    """ms (median, host clock to a synchronisation) of the per-request prior draws of one admission alone: N
    normal_() launches into views of one buffer — the only launches of the pooled path that grow with N."""
    I = net.cfg.inter_channels
    flat = torch.empty(I * sum(frames), device="cuda", dtype=torch.float32)
    out = []
    for _ in range(reps + 2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        o = 0
        for t in frames:
            flat[o:o + I * t].view(1, I, t).normal_()
            o += I * t
        torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t0))
    return round(statistics.median(out[2:]), 3)


def count_syncs(fn):
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            fn()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    return sum("synchroniz" in str(v.message).lower() for v in w)


def measure(net, lens, mode, reps):
    reqs = make_requests(lens)
    net.set_option("splitk", int(mode == "splitk"))
    try:
        for pooled in (True, False, True, False):                 # warm-up: both variants' shapes, the arenas
            run_round(net, reqs, pooled)
        res = {True: [], False: []}
        for r in range(reps):
            for pooled in ((True, False) if r % 2 == 0 else (False, True)):
                res[pooled].append(run_round(net, reqs, pooled))
        syncs = {p: count_syncs(lambda p=p: admit(net, reqs, p)) for p in (True, False)}
    finally:
        net.set_option("splitk", 0)
    a, b = res[True][-1][3], res[False][-1][3]
    same = all(x.z.shape == y.z.shape and torch.equal(x.z, y.z) and torch.equal(x.y_lengths, y.y_lengths) for x, y in zip(a, b))
    if mode == "default" and not same:
        raise SystemExit("pooled and sequential streams differ in the default mode")

    def med(variant, k):
        return round(statistics.median(r[k] for r in res[variant]), 3)

    def spread(variant, k):
        v = sorted(r[k] for r in res[variant])
        return round(v[-2] - v[1], 3)                              # without the two extremes

    rec = dict(config=CONFIG, mode=mode, requests=len(lens), tokens=lens if len(set(lens)) > 1 else lens[0],
               frames=[int(s.z.shape[2]) for s in a] if len(lens) <= 16 else int(sum(s.z.shape[2] for s in a)),
               reps=reps, bitwise_equal=same)
    for variant, name in ((True, "pooled"), (False, "sequential")):
        rec[name + "_wall_ms"], rec[name + "_event_ms"] = med(variant, 0), med(variant, 1)
        rec[name + "_wall_spread_ms"] = spread(variant, 0)
        rec[name + "_runs"], rec[name + "_host_syncs"] = res[variant][0][2], syncs[variant]
    rec["pooled_draws_only_ms"] = draws_only(net, [int(x.z.shape[2]) for x in a], reps)
    rec["wall_ratio"] = round(rec["sequential_wall_ms"] / rec["pooled_wall_ms"], 3)
    rec["event_ratio"] = round(rec["sequential_event_ms"] / rec["pooled_event_ms"], 3)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile", choices=("pooled", "sequential"), default=None,
                    help="N = 16, default mode, %d rounds of one variant only (for rocprofv3)" % PROFILE_ROUNDS)
    args = ap.parse_args()
    if args.reps < 7:
        raise SystemExit("--reps must be at least 7")
    net = make_net(CONFIG)[0]
    if args.profile:
        reqs = make_requests([T_TEXT] * 16)
        for _ in range(PROFILE_ROUNDS):
            run_round(net, reqs, args.profile == "pooled")
        torch.cuda.synchronize()
        return
    lines = []
    for mode in ("default", "splitk"):
        for lens in [[T_TEXT] * n for n in (1, 2, 4, 16, 64)] + [MIXED]:
            lines.append(json.dumps(measure(net, lens, mode, args.reps)))
            print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
