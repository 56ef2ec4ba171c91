"""Live wire timing: a 10 s recording at 48 kHz int16 pushed in 20 ms pieces, without sleeping, through
`wire.convert_live_pcm16` (int16 out at 24 kHz), against two baselines on the same build:

  live_stream_ms   a plain `net.convert_live` stream fed the same audio resampled beforehand (outside the clock) in
                   20 ms pieces at the model's rate: what the two resamplers and the int16 step add
  one_shot_ms      `wire.convert_pcm16` of the whole recording: what arriving piece by piece costs

and eight such wires fed in step: one `PcmPool.step()` per 20 ms tick against eight `poll()` calls per tick.

Host clock from the first call to a final device synchronisation, medians over --reps rounds, the variants alternating
within one visit.  Before anything is reported the live wire is compared bitwise with
`convert_stream(in_sr=) + stream_pcm16`, the plain live stream with the wire's own `LiveStream`, and the pooled wires
with the polled ones; the script refuses to report when any differs.  Whether the one-shot `convert_pcm16` (same seed,
hence the same draw) gives the wire's int16 bitwise is recorded as `one_shot_bitwise_equal`.  `*_runs` are the launches of each stage per 20 ms tick.

`--lag` prints the lag both filters add, in samples and milliseconds, from `mbv_resample_bank`'s (taps, left): pure
arithmetic, no GPU.

    python scripts/live_wire_timing.py [--reps 5] [--out profiles/live_wire_timing.jsonl]
    python scripts/live_wire_timing.py --lag
"""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from mb_istft_vits_amd import _capi, models, wire          # noqa: E402

CONFIG = "uudb_ms_istft_vits_ms"
IN_SR, MODEL_SR, RATE, HOP, WIN, N_FFT = 48000, 22050, 24000, 256, 1024, 1024
PIECE_S = 0.02
SECONDS = 10.0
CF = 32


def lag_table():
    """The samples an output waits for beyond its own position: tap K - 1 of output t reads input floor(t M / L) - left +
    K - 1, so K - left - 1 input samples (rounded up to a whole output on the other side)."""
    rows = []
    for orig, target in ((48000, 22050), (44100, 22050), (16000, 22050), (22050, 24000)):
        for name, filt in sorted(models.RESAMPLE_TYPES.items()):
            taps, left = C.c_int32(), C.c_int32()
            if _capi.lib().mbv_resample_bank(orig, target, filt, None, 0, None, C.byref(taps), C.byref(left)):
                raise SystemExit("mbv_resample_bank refused %d -> %d" % (orig, target))
            lag = taps.value - left.value - 1
            rows.append(dict(orig_sr=orig, target_sr=target, res_type=name, taps=taps.value, left=left.value,
                             lag_input_samples=lag, lag_ms=round(1e3 * lag / orig, 3),
                             lag_output_samples=int(math.ceil(lag * target / orig))))
    return rows


def audio(seconds, k=0):
    n = int(seconds * IN_SR) + (1, 0, 255)[k % 3]
    rs = np.random.RandomState(k)
    t = np.arange(n) / IN_SR
    x = 0.3 * np.sin(2 * np.pi * (150 + 20 * k) * t) + 0.2 * np.sin(2 * np.pi * 1234.5 * t + k) + 0.05 * rs.standard_normal(n)
    return torch.from_numpy((x * 32767).astype(np.int16)).cuda()


def cap_frames(n_raw):
    """Frames of the noise block of a wire opened for n_raw raw samples."""
    cap = int(math.ceil(n_raw * (float(MODEL_SR) / IN_SR)))
    return int(_capi.lib().mbv_spectrogram_frames(cap, N_FFT, HOP))


def open_wire(net, raw, noise, k=0):
    return wire.convert_live_pcm16(net, k % 12, (5 * k + 2) % 12, IN_SR, MODEL_SR, RATE, HOP, WIN, raw.numel(),
                                   dtype=torch.int16, noise=noise, convert_frames=CF)


def counters(net):
    return dict(input_runs=net.input_runs(), converter_runs=net.converter_runs(), decoder_runs=net.decoder_runs(),
                wire_runs=wire.wire_runs(net))


def wire_round(net, raw, noise):
    piece = int(PIECE_S * IN_SR)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    lw = open_wire(net, raw, noise)
    for off in range(0, raw.numel(), piece):
        lw.push(raw[off:off + piece])
        lw.poll()
    lw.close()
    lw.poll()
    torch.cuda.synchronize()
    assert lw.finished
    return 1e3 * (time.perf_counter() - t0), lw


def live_stream_round(net, samples, noise):
    """The plain LiveStream of DESIGN §7.11 on audio that is at the model's rate already."""
    piece = int(PIECE_S * MODEL_SR)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    st = net.convert_live(0, 2, MODEL_SR, HOP, WIN, samples.numel(), noise=noise, convert_frames=CF)
    for off in range(0, samples.numel(), piece):
        st.push(samples[off:off + piece])
        st.poll()
    st.close()
    st.poll()
    torch.cuda.synchronize()
    assert st.finished
    return 1e3 * (time.perf_counter() - t0), st


def one_shot_round(net, raw, seed):
    sid = torch.tensor([0], device="cuda"), torch.tensor([2], device="cuda")
    torch.cuda.manual_seed(seed)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    pcm, valid = wire.convert_pcm16(net, raw[None], None, sid[0], sid[1], IN_SR, MODEL_SR, RATE, HOP, WIN, auto_normalize=False)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), (pcm, valid)


def eight_round(net, raws, noises, pooled):
    piece = int(PIECE_S * IN_SR)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    lws = [open_wire(net, w, nz, k) for k, (w, nz) in enumerate(zip(raws, noises))]
    pp = wire.pcm_pool(net, net.stream_pool(), MODEL_SR, RATE)
    if pooled:
        for lw in lws:
            pp.add_live(lw)
    ticks = 0
    for off in range(0, max(w.numel() for w in raws), piece):
        for lw, w in zip(lws, raws):
            if off < w.numel():
                lw.push(w[off:off + piece])
            elif not lw.closed:
                lw.close()
        ticks += 1
        if pooled:
            pp.step()
        else:
            for lw in lws:
                lw.poll()
    for lw in lws:
        if not lw.closed:
            lw.close()
    while pooled and len(pp):
        pp.step()
        ticks += 1
    for lw in lws:
        lw.poll()
    torch.cuda.synchronize()
    assert all(lw.finished for lw in lws)
    return 1e3 * (time.perf_counter() - t0), lws, ticks


def measure(net, reps):
    from mb_istft_vits_amd import stream
    raw = audio(SECONDS)
    seed = 1234
    samples, n_model = net.resample(raw.float()[None, None] / 32768.0, IN_SR, MODEL_SR)
    samples, n_model = samples[0, 0].contiguous(), int(n_model[0])
    frames = int(stream.spectrogram_ready(n_model, True, N_FFT, HOP))
    torch.cuda.manual_seed(seed)
    noise_t = torch.randn(1, net.cfg.inter_channels, frames, device="cuda")       # the draw convert_pcm16 makes
    noise = torch.zeros(1, net.cfg.inter_channels, cap_frames(raw.numel()), device="cuda")
    noise[:, :, :frames] = noise_t
    # ---- bitwise first
    _, lw = wire_round(net, raw, noise)
    ref = net.convert_stream(raw, 0, 2, MODEL_SR, HOP, WIN, in_sr=IN_SR, noise=noise_t)
    f = wire.stream_pcm16(net, ref, MODEL_SR, RATE)
    pcm_ref, valid_ref = f.run()
    valid = int(valid_ref[0])
    if not (torch.equal(lw.valid_samples, valid_ref) and torch.equal(lw.pcm[:, :valid], pcm_ref[:, :valid])
            and torch.equal(lw.peak, f.peak) and torch.equal(lw.live.samples[:n_model], samples)):
        raise SystemExit("the live wire differs from convert_stream + stream_pcm16: nothing to report")
    _, st = live_stream_round(net, samples, noise)
    if not (torch.equal(st.z, lw.live.z) and torch.equal(st.result(), lw.live.result())):
        raise SystemExit("the plain live stream differs from the wire's: nothing to report")
    _, (pcm1, valid1) = one_shot_round(net, raw, seed)
    one_shot_equal = bool(torch.equal(valid1, valid_ref) and torch.equal(pcm1[:, :valid], lw.pcm[:, :valid]))
    # ---- one stream
    t = dict(wire=[], live_stream=[], one_shot=[])
    order = ["wire", "live_stream", "one_shot"]
    for r in range(reps):
        for name in order[r % 3:] + order[:r % 3]:
            if name == "wire":
                t[name].append(wire_round(net, raw, noise)[0])
            elif name == "live_stream":
                t[name].append(live_stream_round(net, samples, noise)[0])
            else:
                t[name].append(one_shot_round(net, raw, seed)[0])
    c0 = counters(net)
    wire_round(net, raw, noise)
    ticks = -(-raw.numel() // int(PIECE_S * IN_SR)) + 1
    per_tick = {k: round((v - c0[k]) / ticks, 4) for k, v in counters(net).items()}
    totals = {k: v - c0[k] for k, v in counters(net).items()}
    # ---- eight streams
    raws = [audio(SECONDS, k) for k in range(8)]
    noises = [torch.randn(1, net.cfg.inter_channels, cap_frames(w.numel()), device="cuda") for w in raws]
    _, a, _ = eight_round(net, raws, noises, True)
    _, b, _ = eight_round(net, raws, noises, False)
    if not all(torch.equal(x.pcm, y.pcm) and torch.equal(x.valid_samples, y.valid_samples) and torch.equal(x.peak, y.peak)
               and torch.equal(x.live.z, y.live.z) for x, y in zip(a, b)):
        raise SystemExit("eight wires: pooled and polled differ: nothing to report")
    pool8, alone8 = [], []
    for r in range(reps):
        for v in ((0, 1) if r % 2 else (1, 0)):
            (pool8 if v else alone8).append(eight_round(net, raws, noises, bool(v))[0])
    c0 = counters(net)
    _, _, ticks8 = eight_round(net, raws, noises, True)
    pool_tick = {k: round((v - c0[k]) / ticks8, 4) for k, v in counters(net).items()}
    c0 = counters(net)
    _, _, ticks8a = eight_round(net, raws, noises, False)
    alone_tick = {k: round((v - c0[k]) / ticks8a, 4) for k, v in counters(net).items()}
    med = statistics.median
    return dict(config=CONFIG, seconds=SECONDS, in_sr=IN_SR, model_sr=MODEL_SR, rate=RATE, raw_samples=raw.numel(),
                frames=frames, valid_samples=valid, convert_frames=CF, piece_ms=1e3 * PIECE_S, reps=reps, bitwise_equal=True,
                one_shot_bitwise_equal=one_shot_equal,
                wire_ms=round(med(t["wire"]), 3), live_stream_ms=round(med(t["live_stream"]), 3),
                one_shot_ms=round(med(t["one_shot"]), 3),
                wire_over_live_stream=round(med(t["wire"]) / med(t["live_stream"]), 3),
                wire_over_one_shot=round(med(t["wire"]) / med(t["one_shot"]), 3),
                ticks=ticks, runs_total=totals, runs_per_tick=per_tick,
                pool8_ms=round(med(pool8), 3), alone8_ms=round(med(alone8), 3),
                alone8_over_pool8=round(med(alone8) / med(pool8), 3),
                pool8_ticks=ticks8, pool8_runs_per_tick=pool_tick, alone8_runs_per_tick=alone_tick)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--lag", action="store_true", help="print the filters' lag (host arithmetic) and stop")
    args = ap.parse_args()
    lines = [json.dumps(dict(lag=lag_table()))]
    print(lines[-1], flush=True)
    if args.lag:
        return
    from gpu_util import make_net
    net = make_net(CONFIG)[0]
    wire_round(net, audio(3.0), None)                              # warm-up: the arenas, the tables, both banks
    lines.append(json.dumps(measure(net, args.reps)))
    print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
