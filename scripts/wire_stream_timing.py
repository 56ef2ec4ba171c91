"""Streamed wire output timing: ljs_mb, one utterance of ~3 s and ~20 s, 22 050 -> 24 000 Hz, default
and split-K modes.

Per case (median of --reps runs after a warm-up, both chains measured in the same run, alternating): wall clock from
the call to the first 20 ms frame as base64 text on the host, and to the last, for
  streamed   infer_stream -> wire.stream_pcm16 -> FrameCutter
  one-shot   infer -> wire.service_pcm16 -> wire.frame_pcm16
and whether every streamed piece was on the host before the audio ahead of it had finished playing.  One JSON line
per case.

    python scripts/wire_stream_timing.py [--reps 7] [--out file.jsonl]

The kernel time of the per-chunk launch comes from a profiler run of its own:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/wire_stream_timing.py --profile
    python scripts/wire_stream_timing.py --trace DIR [--out file.csv]      (no GPU needed: reads the trace)
"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SR, RATE = 22050, 24000


def text_for_frames(net, target, seed=1):
    """A synthetic utterance whose T' is closest to `target` frames (text lengths searched by bisection)."""
    import torch
    from mb_istft_vits_amd import synth

    def frames(n):
        x, xl, _ = synth.synthetic_batch(net.cfg, 1, n, seed=seed)
        *_, yl = net._run(torch.from_numpy(x).cuda(), torch.from_numpy(xl).cuda(), None, 0, 1, None, decode=False,
                          outputs=("y_mask",))
        return int(yl[0]), x, xl
    lo, hi = 2, 2000
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if frames(mid)[0] < target:
            lo = mid
        else:
            hi = mid
    t, x, xl = min((frames(lo), frames(hi)), key=lambda r: abs(r[0] - target))
    return t, torch.from_numpy(x).cuda(), torch.from_numpy(xl).cuda()


def run_stream(net, x, xl, chunk, cap, peak):
    """-> (s to the first frame, s to the last, every piece in time, pieces, frames)"""
    from mb_istft_vits_amd import wire
    t0 = time.perf_counter()
    st = net.infer_stream(x, xl, noise_scale=0, chunk_frames=chunk, max_chunk_frames=cap)
    ws = wire.stream_pcm16(net, st, SR, RATE, peak=peak)
    cutter = wire.FrameCutter(RATE)
    first, n_frames, arrived = None, 0, []
    for a, v in ws:
        frames = cutter.push(v[0])                    # device -> host copy of the piece, then base64
        now = time.perf_counter() - t0
        arrived.append((a, now))
        n_frames += len(frames)
        if first is None and frames:
            first = now
    n_frames += len(cutter.close())
    last = time.perf_counter() - t0
    if first is None:
        first = last
    in_time = all(t <= first + a / RATE for a, t in arrived)
    return first, last, in_time, len(arrived), n_frames


def run_one_shot(net, x, xl, auto):
    """-> (s to the first frame = s to the last: the frames exist together, frames)"""
    from mb_istft_vits_amd import wire
    t0 = time.perf_counter()
    (o, *_), yl = net.infer_with_lengths(x, xl, noise_scale=0, outputs=("o",))
    pcm, valid = wire.service_pcm16(net, o, yl, SR, RATE, auto_normalize=auto)
    row = pcm[0].cpu()
    frames = wire.frame_pcm16(row, RATE, valid_samples=int(valid[0]))
    return time.perf_counter() - t0, len(frames)


def measure(args):
    from gpu_util import make_net
    net = make_net("ljs_mb_istft_vits")[0]
    lines = []
    med = lambda v: round(1e3 * statistics.median(v), 2)
    for secs in (3, 20):
        T, x, xl = text_for_frames(net, round(secs * SR / 256))
        for mode in ("default", "splitk"):
            net.set_option("splitk", int(mode == "splitk"))
            for peak in (None, 0.5):                  # 0.5: a calibrated per-speaker constant, the normalising epilogue
                run_stream(net, x, xl, args.chunk, args.cap, peak)
                run_one_shot(net, x, xl, peak is not None)
                rs, os_ = [], []
                for _ in range(args.reps):
                    rs.append(run_stream(net, x, xl, args.chunk, args.cap, peak))
                    os_.append(run_one_shot(net, x, xl, peak is not None))
                assert rs[0][4] == os_[0][1], (rs[0][4], os_[0][1])
                rec = dict(config="ljs_mb_istft_vits", B=1, frames=T, seconds=round(T * 256 / SR, 2), mode=mode,
                           model_sr=SR, rate=RATE, normalise=peak is not None, chunk_frames=args.chunk,
                           max_chunk_frames=args.cap, chunks=rs[0][3], wire_frames=rs[0][4],
                           stream_first_frame_ms=med(r[0] for r in rs), stream_last_frame_ms=med(r[1] for r in rs),
                           one_shot_frames_ms=med(r[0] for r in os_),
                           every_piece_in_time=all(r[2] for r in rs), reps=args.reps)
                lines.append(json.dumps(rec))
                print(lines[-1], flush=True)
        net.set_option("splitk", 0)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def profile(args):
    """The work a profiler run traces: both utterances streamed a few times, and the one-shot chain."""
    import torch
    from gpu_util import make_net
    net = make_net("ljs_mb_istft_vits")[0]
    for secs in (3, 20):
        T, x, xl = text_for_frames(net, round(secs * SR / 256))
        for _ in range(args.reps):
            run_stream(net, x, xl, args.chunk, args.cap, 0.5)
            run_one_shot(net, x, xl, True)
    torch.cuda.synchronize()


def trace_summary(args):
    """Per-dispatch durations of the wire kernels in a rocprofv3 kernel trace, grouped by kernel and grid size."""
    files = sorted(glob.glob(os.path.join(args.trace, "**", "*kernel_trace.csv"), recursive=True))
    if not files:
        sys.exit("no *kernel_trace.csv below " + args.trace)
    groups = {}
    for r in csv.DictReader(open(files[0])):
        name = r["Kernel_Name"]
        if "resample" not in name and "pcm16" not in name and "absmax" not in name:
            continue
        name = name.replace("void ", "").split("(")[0]
        wg = max(int(r.get("Workgroup_Size_X") or 1), 1)
        key = (name, int(r["Grid_Size_X"]) // wg, int(r.get("Grid_Size_Y") or 1))
        groups.setdefault(key, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    rows = [("kernel", "workgroups_x", "rows", "calls", "median_us", "min_us", "max_us")]
    for (name, gx, gy), d in sorted(groups.items()):
        rows.append((name, gx, gy, len(d), round(statistics.median(d), 1), round(min(d), 1), round(max(d), 1)))
    out = open(args.out, "w", newline="") if args.out else sys.stdout
    csv.writer(out).writerows(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--chunk", type=int, default=32)
    ap.add_argument("--cap", type=int, default=256)
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile", action="store_true", help="only run the chains (under rocprofv3)")
    ap.add_argument("--trace", default=None, help="summarise the kernel trace below this directory")
    args = ap.parse_args()
    if args.trace:
        trace_summary(args)
    elif args.profile:
        profile(args)
    else:
        measure(args)


if __name__ == "__main__":
    main()
