"""Per-token pitch, timing: ljs_mb, 22 050 -> 24 000 Hz.  Every case runs the same decode twice in one
process, in alternating order: with a `WarpMap` on the stream (what `infer_stream(pitch=)` leaves there) and without
one, which is the parent commit's path for the same request (bitwise: tests/test_gpu_pitch.py).

  streamed_10s   one 10 s utterance (861 z-frames; chunks 32, 64, 128, 256, ..), `stream_pcm16` to its end
  pooled_8       eight 3 s utterances (258 z-frames each) in a `PcmPool`, every tick ending with its pieces on the host
  plain_tick     the pooled case with no pitched member: `mbv_warp_runs` must not move (the one condition this script
                 sets; it exits non-zero otherwise)

The rate table is what a text would give: a random pitch in [0.5, 2] per "token" of 5 to 12 frames, with the default
glide.  Reported: the median over --reps repetitions with the fastest and slowest beside it, warp and wire launches.

    python scripts/pitch_timing.py [--reps 7] [--out profiles/pitch_timing.jsonl]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIG = "ljs_mb_istft_vits"
MODEL_SR, RATE = 22050, 24000
T_10S, T_3S, STREAMS = 861, 258, 8
CHUNK, CAP = 32, 256


def stats(values):
    return dict(median=round(statistics.median(values), 4), min=round(min(values), 4), max=round(max(values), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from gpu_util import make_net
    from mb_istft_vits_amd import stream, wire

    net = make_net(CONFIG)[0]
    rs = np.random.RandomState(7)

    def rate_table(frames):
        marks = [0]
        while marks[-1] < frames:
            marks.append(min(frames, marks[-1] + int(rs.randint(5, 13))))
        pitch = rs.uniform(0.5, 2.0, len(marks) - 1).astype(np.float32).tolist()
        return stream.frame_rates(pitch, marks, frames)

    g = torch.Generator().manual_seed(STREAMS)
    z10 = torch.randn(1, net.cfg.inter_channels, T_10S, generator=g).cuda()
    z3 = [torch.randn(1, net.cfg.inter_channels, T_3S, generator=g).cuda() for _ in range(STREAMS)]
    spf = net.cfg.samples_per_frame
    map10 = stream.WarpMap(rate_table(T_10S), spf, "cuda")
    map3 = [stream.WarpMap(rate_table(T_3S), spf, "cuda") for _ in z3]

    def runs():
        return net.warp_runs(), wire.wire_runs(net)

    def streamed(pitched):
        st = net.dec_stream(z10, None, CHUNK, CAP)
        st.warp = map10 if pitched else None
        torch.cuda.synchronize()
        w0, r0 = runs()
        t0 = time.perf_counter()
        wire.stream_pcm16(net, st, MODEL_SR, RATE).run()
        torch.cuda.synchronize()
        ms = 1e3 * (time.perf_counter() - t0)
        w1, r1 = runs()
        return ms, w1 - w0, r1 - r0

    def pooled(pitched):
        sts = [net.dec_stream(z, None, CHUNK, CAP) for z in z3]
        pp = wire.pcm_pool(net, net.stream_pool(), MODEL_SR, RATE)
        for st, m in zip(sts, map3):
            st.warp = m if pitched else None
            pp.add(st)
        torch.cuda.synchronize()
        w0, r0 = runs()
        t0 = time.perf_counter()
        ticks = 0
        while len(pp):
            pp.step(host=True)
            ticks += 1
        torch.cuda.synchronize()
        ms = 1e3 * (time.perf_counter() - t0)
        w1, r1 = runs()
        return ms, w1 - w0, r1 - r0, ticks

    lines = []
    for name, fn in (("streamed_10s", streamed), ("pooled_8", pooled)):
        for v in (False, True) * 2:                       # warm-up: tables, allocator, the filter window
            fn(v)
        res = {False: [], True: []}
        for r in range(args.reps):
            for v in ((False, True) if r % 2 == 0 else (True, False)):
                res[v].append(fn(v))
        plain, pitched = stats([x[0] for x in res[False]]), stats([x[0] for x in res[True]])
        rec = dict(what=name, config=CONFIG, model_sr=MODEL_SR, rate=RATE, reps=args.reps, chunk_frames=CHUNK,
                   max_chunk_frames=CAP, frames=T_10S if name == "streamed_10s" else T_3S,
                   streams=1 if name == "streamed_10s" else STREAMS, plain_ms=plain, pitched_ms=pitched,
                   added_ms=round(pitched["median"] - plain["median"], 4),
                   ratio=round(pitched["median"] / plain["median"], 4),
                   pitched_warp_runs=res[True][0][1], pitched_wire_runs=res[True][0][2],
                   plain_warp_runs=res[False][0][1], plain_wire_runs=res[False][0][2])
        if name == "pooled_8":
            rec["ticks"] = res[True][0][3]
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        if any(x[1] for x in res[False]):
            raise SystemExit("a run without a pitched member launched the warp kernel")
    rec = dict(what="plain_tick", warp_runs_moved=False, note="no pitched member: mbv_warp_runs unchanged over every tick")
    lines.append(json.dumps(rec))
    print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
