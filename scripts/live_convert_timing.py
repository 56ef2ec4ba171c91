"""Live voice conversion timing: a recording pushed in 20 ms pieces, without sleeping, through
`net.convert_live`, against `net.convert_stream(whole).run()` of the same recording on the same build.

Per recording length (10 s, 30 s) and `convert_frames` (16, 32, 64), on uudb_ms_istft_vits_ms:

  live_ms / one_shot_ms     host clock from the first call to a final device synchronisation, medians over --reps rounds,
                            the two alternating; their ratio is the recompute factor (every conversion window carries
                            up to 96 + 31 frames of left and 96 frames of right context that other windows compute too)
  poll_convert_ms           median time of a `poll()` that converts (and may decode), synchronised after each poll
  poll_decode_ms            ... of a `poll()` that only decodes (null when there was none: a chunk becomes decodable when
                            z_hat advances, that is in a poll that converts; only chunks a pool decoded ahead differ)
  poll_idle_us              ... of a `poll()` that finds nothing to do
  first_audio               the samples that must have arrived before the first chunk leaves, in frames and seconds: pure
                            arithmetic of `stream.LivePlan` (also given for a 22.05 kHz model: no GPU involved)
  pool8_ms / alone8_ms      eight live streams of that length fed in step: one `StreamPool.step()` per 20 ms tick against
                            eight `poll()` calls per tick

ljs_ms_istft_vits is a single-speaker model: `convert_live`, like `voice_conversion`, refuses it, so it has no row of its
own; its data config (22.05 kHz) appears in the lag arithmetic only.

Before anything is reported the live result is compared bitwise with the one-shot stream; the script refuses to report
when they differ.

    python scripts/live_convert_timing.py [--reps 5] [--out profiles/live_convert_timing.jsonl]
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
from mb_istft_vits_amd import stream          # noqa: E402

CONFIG = "uudb_ms_istft_vits_ms"
MODEL_SR, HOP, WIN, N_FFT = 16000, 256, 1024, 1024
PIECE_S = 0.02
SCHED = (32, 256)


def audio(seconds, k=0):
    n = int(seconds * MODEL_SR) + (1, 0, 255)[k % 3]
    rs = np.random.RandomState(k)
    t = np.arange(n) / MODEL_SR
    x = 0.3 * np.sin(2 * np.pi * (150 + 20 * k) * t) + 0.2 * np.sin(2 * np.pi * 1234.5 * t + k) + 0.05 * rs.standard_normal(n)
    return torch.from_numpy(x.astype(np.float32)).cuda()


def open_live(net, wave, noise, cf, k=0):
    return net.convert_live(k % 12, (5 * k + 2) % 12, MODEL_SR, HOP, WIN, wave.numel(), noise=noise, chunk_frames=SCHED[0],
                            max_chunk_frames=SCHED[1], convert_frames=cf)


def live_round(net, wave, noise, cf, per_poll=None):
    """The whole recording in 20 ms pieces, a poll after each; -> (ms, stream)."""
    piece = int(PIECE_S * MODEL_SR)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    st = open_live(net, wave, noise, cf)
    for off in range(0, wave.numel(), piece):
        st.push(wave[off:off + piece])
        if per_poll is None:
            st.poll()
        else:
            kind = "convert" if st.pending() is not None else None
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            got = st.poll()
            torch.cuda.synchronize()
            per_poll.setdefault(kind or ("decode" if got else "idle"), []).append(1e3 * (time.perf_counter() - t1))
    st.close()
    st.poll()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), st


def one_shot_round(net, wave, noise, frames):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    st = net.convert_stream(wave, 0, 2, MODEL_SR, HOP, WIN, noise=noise[:, :, :frames], chunk_frames=SCHED[0],
                            max_chunk_frames=SCHED[1])
    st.run()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), st


def eight_round(net, waves, noises, cf, pooled):
    piece = int(PIECE_S * MODEL_SR)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    sts = [open_live(net, w, nz, cf, k) for k, (w, nz) in enumerate(zip(waves, noises))]
    pool = net.stream_pool()
    if pooled:
        for st in sts:
            pool.add(st)
    for off in range(0, max(w.numel() for w in waves), piece):
        for st, w in zip(sts, waves):
            if off < w.numel():
                st.push(w[off:off + piece])
            elif not st.closed:
                st.close()
        if pooled:
            pool.step()
        else:
            for st in sts:
                st.poll()
    for st in sts:
        if not st.closed:
            st.close()
    while pooled and len(pool):
        pool.step()
    for st in sts:
        st.poll()
    torch.cuda.synchronize()
    assert all(st.finished for st in sts)
    return 1e3 * (time.perf_counter() - t0), sts


def first_audio(sr, cf, chunk_frames, r_conv, r_dec):
    """Samples that must have arrived, in 20 ms pieces, before the first chunk is decodable (host arithmetic)."""
    plan = stream.LivePlan(N_FFT, HOP, r_conv, r_dec, chunk_frames, 256, cf)
    piece = int(PIECE_S * sr)
    while True:
        plan.push(piece)
        due = plan.convert_due()
        if due:
            plan.converted(*due)
        if plan.decodable():
            return dict(sr=sr, convert_frames=cf, chunk_frames=chunk_frames, samples=plan.arrived,
                        frames=plan.spec_final, seconds=round(plan.arrived / sr, 3))


def measure(net, seconds, cf, reps):
    wave = audio(seconds)
    frames = int(stream.spectrogram_ready(wave.numel(), True, N_FFT, HOP))
    noise = torch.randn(1, net.cfg.inter_channels, frames, device="cuda")
    _, ref = one_shot_round(net, wave, noise, frames)
    _, st = live_round(net, wave, noise, cf)
    if not (torch.equal(st.z[:, :, :frames], ref.z) and torch.equal(st.result(), ref.o)):
        raise SystemExit("%g s, convert_frames %d: the live result differs from the one-shot stream: nothing to report" % (seconds, cf))
    live, one = [], []
    for r in range(reps):
        for v in ((0, 1) if r % 2 else (1, 0)):
            if v:
                live.append(live_round(net, wave, noise, cf)[0])
            else:
                one.append(one_shot_round(net, wave, noise, frames)[0])
    per_poll = {}
    c0, d0 = net.converter_runs(), net.decoder_runs()
    live_round(net, wave, noise, cf, per_poll)
    counts = dict(converter_runs=net.converter_runs() - c0, decoder_runs=net.decoder_runs() - d0)
    waves = [audio(seconds, k) for k in range(8)]
    noises = [torch.randn(1, net.cfg.inter_channels, int(stream.spectrogram_ready(w.numel(), True, N_FFT, HOP)), device="cuda")
              for w in waves]
    _, a = eight_round(net, waves, noises, cf, True)
    _, b = eight_round(net, waves, noises, cf, False)
    if not all(torch.equal(x.z, y.z) and torch.equal(x.result(), y.result()) for x, y in zip(a, b)):
        raise SystemExit("eight streams: pooled and alone differ: nothing to report")
    pool8, alone8 = [], []
    for r in range(max(3, reps // 2)):
        for v in ((0, 1) if r % 2 else (1, 0)):
            (pool8 if v else alone8).append(eight_round(net, waves, noises, cf, bool(v))[0])
    med = statistics.median
    rec = dict(config=CONFIG, seconds=seconds, frames=frames, convert_frames=cf, piece_ms=1e3 * PIECE_S, reps=reps,
               bitwise_equal=True, live_ms=round(med(live), 3), one_shot_ms=round(med(one), 3),
               live_over_one_shot=round(med(live) / med(one), 3), live_counts=counts,
               polls={k: len(v) for k, v in per_poll.items()},
               poll_convert_ms=round(med(per_poll["convert"]), 3),
               poll_decode_ms=round(med(per_poll["decode"]), 3) if "decode" in per_poll else None,
               poll_idle_us=round(1e3 * med(per_poll["idle"]), 1) if "idle" in per_poll else None,
               pool8_ms=round(med(pool8), 3), alone8_ms=round(med(alone8), 3),
               alone8_over_pool8=round(med(alone8) / med(pool8), 3))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    net = make_net(CONFIG)[0]
    r_conv = net.converter_context()[1]
    r_dec = stream.decoder_context(net._config_struct())[1]
    lines = [json.dumps(dict(first_audio=[first_audio(sr, cf, c, r_conv, r_dec) for sr in (16000, 22050)
                                          for c in (8, 32) for cf in (16, 32, 64)], r_conv=r_conv, r_dec=r_dec))]
    print(lines[-1], flush=True)
    live_round(net, audio(3.0), None, 32)                          # warm-up: the arenas, the spectrogram tables
    for seconds in (10.0, 30.0):
        for cf in (16, 32, 64):
            lines.append(json.dumps(measure(net, seconds, cf, args.reps)))
            print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
