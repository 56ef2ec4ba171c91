"""Live voice conversion with a bounded look-ahead: lag, cost and deviation per `stream.Ahead` setting.

  lag         `LivePlan.lag()` per setting, for a 16 kHz and a 22.05 kHz model: the samples that must have arrived before
              the first chunk leaves, and the steady-state lag in frames.  Pure arithmetic, no GPU involved.
  cost        a 10 s recording pushed in 20 ms pieces, without sleeping, a `poll()` after each: host clock from opening
              the stream to a final device synchronisation.  Every bounded setting runs with convert_frames 4 and chunks
              of 4 frames; it is timed against the unbounded live stream of the same process in its default shape
              (convert_frames 32, chunks 32 .. 256), the two alternating, medians over --reps rounds (as §7.11 measured).
              `unbounded_small` is the unbounded stream on the bounded settings' grid: what the small blocks cost by
              themselves.  Alone, and eight streams fed in step through one `StreamPool.step()` per tick.
  deviation   relative rms of the bounded z_hat and waveform from the full-context stream of the same recording, noise
              and speakers.  This is measured ON THE CHECKPOINT AT HAND.  The repository ships synthetic weights: the
              figures written by a run on them say how far random layers look, and nothing about a trained model.  Run
              the script on the checkpoint you serve.

    python scripts/live_lookahead_timing.py [--reps 3] [--out profiles/live_lookahead.jsonl]
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
from mb_istft_vits_amd.stream import Ahead          # noqa: E402

CONFIG = "uudb_ms_istft_vits_ms"
MODEL_SR, HOP, WIN, N_FFT = 16000, 256, 1024, 1024
PIECE_S, SECONDS = 0.02, 10.0
SETTINGS = [(96, 24), (32, 12), (16, 8), (8, 4), (4, 2)]
GRID = dict(convert_frames=4, chunk_frames=4, max_chunk_frames=4)
DEFAULT = dict(convert_frames=32, chunk_frames=32, max_chunk_frames=256)
NOTE = ("deviation is measured on the checkpoint that was loaded; synthetic weights (the only ones the repository ships) "
        "say nothing about a trained model")


def audio(k=0):
    n = int(SECONDS * MODEL_SR) + (1, 0, 255)[k % 3]
    rs = np.random.RandomState(k)
    t = np.arange(n) / MODEL_SR
    x = 0.3 * np.sin(2 * np.pi * (150 + 20 * k) * t) + 0.2 * np.sin(2 * np.pi * 1234.5 * t + k) + 0.05 * rs.standard_normal(n)
    return torch.from_numpy(x.astype(np.float32)).cuda()


def open_live(net, wave, k, ahead, shape):
    return net.convert_live(k % 12, (5 * k + 2) % 12, MODEL_SR, HOP, WIN, wave.numel(), seed=100 + k, ahead=ahead, **shape)


def alone_round(net, wave, ahead, shape):
    piece = int(PIECE_S * MODEL_SR)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    st = open_live(net, wave, 0, ahead, shape)
    for off in range(0, wave.numel(), piece):
        st.push(wave[off:off + piece])
        st.poll()
    st.close()
    st.poll()
    torch.cuda.synchronize()
    assert st.finished
    return 1e3 * (time.perf_counter() - t0), st


def pool_round(net, waves, ahead, shape):
    piece = int(PIECE_S * MODEL_SR)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    sts = [open_live(net, w, k, ahead, shape) for k, w in enumerate(waves)]
    pool = net.stream_pool()
    for st in sts:
        pool.add(st)
    for off in range(0, max(w.numel() for w in waves), piece):
        for st, w in zip(sts, waves):
            if off < w.numel():
                st.push(w[off:off + piece])
            elif not st.closed:
                st.close()
        pool.step()
    for st in sts:
        if not st.closed:
            st.close()
    while len(pool):
        pool.step()
    for st in sts:
        st.poll()
    torch.cuda.synchronize()
    assert all(st.finished for st in sts)
    return 1e3 * (time.perf_counter() - t0), sts


def rel_rms(a, b):
    b = b.double()
    return float(torch.sqrt(torch.mean((a - b) ** 2)) / torch.sqrt(torch.mean(b ** 2)))


def lag_table(r_conv, r_dec):
    rows = []
    for sr in (16000, 22050):
        for name, ahead, shape in [("unbounded", None, DEFAULT), ("unbounded_small", None, GRID)] + [
                ("ahead_%d_%d" % s, Ahead(*s), GRID) for s in SETTINGS]:
            plan = stream.LivePlan(N_FFT, HOP, r_conv, r_dec, shape["chunk_frames"], shape["max_chunk_frames"],
                                   shape["convert_frames"], ahead=ahead)
            arrived, steady = plan.lag()
            rows.append(dict(sr=sr, setting=name, **shape, first_audio_samples=arrived,
                             first_audio_s=round(arrived / sr, 3), steady_lag_frames=steady,
                             steady_lag_s=round(steady * HOP / sr, 3)))
    return rows


def measure(net, name, ahead, shape, base, waves, reps):
    """One setting against the unbounded default stream, alternating; -> the record."""
    med = statistics.median
    alone, ref_alone, pooled, ref_pooled = [], [], [], []
    for r in range(reps):
        for v in ((0, 1) if r % 2 else (1, 0)):
            (alone if v else ref_alone).append(alone_round(net, waves[0], ahead if v else None, shape if v else DEFAULT)[0])
    for r in range(reps):
        for v in ((0, 1) if r % 2 else (1, 0)):
            (pooled if v else ref_pooled).append(pool_round(net, waves, ahead if v else None, shape if v else DEFAULT)[0])
    c0, d0, s0 = net.converter_runs(), net.decoder_runs(), net.seam_runs()
    _, st = alone_round(net, waves[0], ahead, shape)
    counts = dict(converter_runs=net.converter_runs() - c0, decoder_runs=net.decoder_runs() - d0,
                  seam_runs=net.seam_runs() - s0)
    F = st.frames
    rec = dict(config=CONFIG, setting=name, seconds=SECONDS, frames=F, piece_ms=1e3 * PIECE_S, reps=reps, **shape,
               alone_ms=round(med(alone), 3), unbounded_alone_ms=round(med(ref_alone), 3),
               alone_over_unbounded=round(med(alone) / med(ref_alone), 3),
               pool8_ms=round(med(pooled), 3), unbounded_pool8_ms=round(med(ref_pooled), 3),
               pool8_over_unbounded=round(med(pooled) / med(ref_pooled), 3), counts=counts,
               z_rel_rms=rel_rms(st.z[:, :, :F], base.z[:, :, :F]), o_rel_rms=rel_rms(st.result(), base.result()),
               note=NOTE)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    net = make_net(CONFIG)[0]
    r_conv = net.converter_context()[1]
    r_dec = stream.decoder_context(net._config_struct())[1]
    lines = [json.dumps(dict(lag=lag_table(r_conv, r_dec), r_conv=r_conv, r_dec=r_dec, n_fft=N_FFT, hop=HOP))]
    print(lines[-1], flush=True)
    waves = [audio(k) for k in range(8)]
    alone_round(net, waves[0], None, DEFAULT)                      # warm-up: the arenas, the spectrogram tables
    _, base = alone_round(net, waves[0], None, DEFAULT)           # the full-context stream: same seed, same speakers
    _, full = alone_round(net, waves[0], Ahead(r_conv, r_dec), GRID)
    if not (torch.equal(full.z, base.z) and torch.equal(full.result(), base.result())):
        raise SystemExit("Ahead(R_conv, R_dec) differs from the unbounded stream: nothing to report")
    todo = [("unbounded_small", None, GRID)] + [("ahead_%d_%d" % s, Ahead(*s), GRID) for s in SETTINGS]
    todo.append(("ahead_8_4_seam_5ms", Ahead(8, 4, seam_ms=5.0), GRID))
    for name, ahead, shape in todo:
        lines.append(json.dumps(measure(net, name, ahead, shape, base, waves, args.reps)))
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
