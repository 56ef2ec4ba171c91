"""Streaming decode timing: ljs_mb, one utterance of ~3 s and ~20 s, default and split-K modes.

Per case (median of --reps runs after a warm-up): time from the `infer_stream` call to the first chunk's samples on
the host, to the last chunk's, the one-shot `infer(..., outputs=("o",))` time to its samples on the host, and whether
every chunk was on the host before the audio ahead of it had finished playing (playback starting when the first
chunk arrives).  One JSON line per case.

    python scripts/stream_timing.py [--reps 7] [--out file.jsonl]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
from gpu_util import make_net          # noqa: E402
from mb_istft_vits_amd import synth    # noqa: E402

SR = 22050


def text_for_frames(net, target, seed=1):
    """A synthetic utterance whose T' is closest to `target` frames (text lengths searched by bisection)."""
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


def run_stream(net, x, xl, chunk, cap):
    t0 = time.perf_counter()
    st = net.infer_stream(x, xl, noise_scale=0, chunk_frames=chunk, max_chunk_frames=cap)
    ready, starts = [], []
    for a, v in st:
        v.cpu()
        ready.append(time.perf_counter() - t0)
        starts.append(a)
    in_time = all(r <= ready[0] + a / SR for r, a in zip(ready, starts))
    return ready[0], ready[-1], in_time, len(starts)


def run_one_shot(net, x, xl):
    t0 = time.perf_counter()
    o = net.infer(x, xl, noise_scale=0, outputs=("o",))[0]
    o.cpu()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--chunk", type=int, default=32)
    ap.add_argument("--cap", type=int, default=256)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    net = make_net("ljs_mb_istft_vits")[0]
    lines = []
    for secs in (3, 20):
        T, x, xl = text_for_frames(net, round(secs * SR / 256))
        for mode in ("default", "splitk"):
            net.set_option("splitk", int(mode == "splitk"))
            run_stream(net, x, xl, args.chunk, args.cap)
            run_one_shot(net, x, xl)
            rs = [run_stream(net, x, xl, args.chunk, args.cap) for _ in range(args.reps)]
            os_ = [run_one_shot(net, x, xl) for _ in range(args.reps)]
            rec = dict(config="ljs_mb_istft_vits", B=1, frames=T, seconds=round(T * 256 / SR, 2), mode=mode,
                       chunk_frames=args.chunk, max_chunk_frames=args.cap, chunks=rs[0][3],
                       first_chunk_ms=round(1e3 * statistics.median(r[0] for r in rs), 2),
                       last_chunk_ms=round(1e3 * statistics.median(r[1] for r in rs), 2),
                       one_shot_ms=round(1e3 * statistics.median(os_), 2),
                       every_chunk_in_time=all(r[2] for r in rs), reps=args.reps)
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
        net.set_option("splitk", 0)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
