"""Blended voices, timing: uudb_ms_istft_vits_ms, the 12-speaker model the service runs.

  define_1, define_64   one `mbv_speakers_define` call for 1 and for 64 three-term blends (the definition table's
                        upload launches and the one blend launch), re-defining the same slots: ms per call, device
                        events around batches of --iters calls
  infer_stream_3s       `infer_stream(...).run()` of one 3 s utterance (47 tokens x 4 frames = 188 z-frames, durations
                        given so that both sides decode the same length) with a plain sid and with a voice sid, the
                        two alternating in one process: ms per call, a host clock around batches that end in a
                        synchronise

The protocol is benchutil's: an untimed warm-up, then 7 bracketed batches (--reps), the median batch reported with the
fastest and slowest beside it.  No figure is expected in advance; what the record states is whether the plain-sid and
voice-sid medians differ by more than the spread of the batches themselves (`within_spread`).

    python scripts/speaker_timing.py [--reps 7] [--iters 20] [--out profiles/speaker_timing.jsonl]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIG = "uudb_ms_istft_vits_ms"
TOKENS, FRAMES_PER_TOKEN = 47, 4
CHUNK, CAP = 32, 256


def stats(values):
    return dict(median=round(statistics.median(values), 4), min=round(min(values), 4), max=round(max(values), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from gpu_util import make_net

    net = make_net(CONFIG)[0]
    h = net._ensure_handle()
    rs = np.random.RandomState(3)
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    # ---- the cost of defining
    for n in (1, 64):
        voices = net.speakers([dict(ids=rs.permutation(net.n_speakers)[:3].tolist(), weights=rs.uniform(0.1, 1, 3).tolist())
                               for _ in range(n)])
        stream = torch.cuda.current_stream()

        def batch():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record(stream)
            for _ in range(args.iters):
                net._define_voices(h, voices)
            e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1) / args.iters, 1e3 * (time.perf_counter() - t0) / args.iters

        runs = net.speaker_runs()
        for _ in range(3):
            batch()                                           # warm-up: code objects, the table's buffers
        res = [batch() for _ in range(args.reps)]
        launches = (net.speaker_runs() - runs) / ((3 + args.reps) * args.iters)
        emit(dict(what="define_%d" % n, config=CONFIG, voices=n, terms=3, reps=args.reps, iters=args.iters,
                  device_ms_per_call=stats([r[0] for r in res]), host_ms_per_call=stats([r[1] for r in res]),
                  blend_launches_per_call=launches))
        if launches != 1:
            raise SystemExit("a define call made %r blend launches" % launches)
        for v in voices:
            v.release()

    # ---- one 3 s utterance, plain sid against voice sid
    voice = net.speaker(ids=[3, 7], weights=[0.7, 0.3])
    x = torch.randint(1, 59, (1, TOKENS), generator=torch.Generator().manual_seed(1)).cuda()
    xl = torch.tensor([TOKENS]).cuda()
    d = torch.full((1, TOKENS), FRAMES_PER_TOKEN, dtype=torch.int32).cuda()
    sids = {"plain": torch.tensor([3]).cuda(), "voice": torch.tensor([voice.sid]).cuda()}

    def utterances(kind):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.iters):
            o = net.infer_stream(x, xl, sids[kind], noise_scale=0.667, durations=d, seed=[5], chunk_frames=CHUNK,
                                 max_chunk_frames=CAP).run()
        torch.cuda.synchronize()
        assert o.shape[-1] == net.cfg.samples_per_frame * TOKENS * FRAMES_PER_TOKEN
        return 1e3 * (time.perf_counter() - t0) / args.iters

    runs = net.speaker_runs()
    for kind in ("plain", "voice") * 2:
        utterances(kind)                                      # warm-up
    res = {"plain": [], "voice": []}
    for r in range(args.reps):
        for kind in (("plain", "voice") if r % 2 == 0 else ("voice", "plain")):
            res[kind].append(utterances(kind))
    plain, voiced = stats(res["plain"]), stats(res["voice"])
    spread = max(plain["max"] - plain["min"], voiced["max"] - voiced["min"])
    diff = voiced["median"] - plain["median"]
    emit(dict(what="infer_stream_3s", config=CONFIG, frames=TOKENS * FRAMES_PER_TOKEN, reps=args.reps, iters=args.iters,
              chunk_frames=CHUNK, max_chunk_frames=CAP, plain_ms=plain, voice_ms=voiced, voice_minus_plain_ms=round(diff, 4),
              spread_ms=round(spread, 4), within_spread=bool(abs(diff) <= spread),
              blend_launches=net.speaker_runs() - runs))
    if net.speaker_runs() != runs:
        raise SystemExit("an utterance launched the blend kernel")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
