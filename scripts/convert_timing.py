"""Pooled voice conversion timing: uudb, N audio requests served at once, the WHOLE job from audio on
the device to every int16 sample of every request.

Workloads: N in {1, 2, 4, 16, 64} waves of 3 s at the model's rate (16 kHz -> 24 kHz on the wire), and a mixed set of
16 waves of 0.3 ... 5 s.  Per workload the job is done three ways on the same build in the same process:

  pooled      `PcmPool.admit(ConvertRequest...)` + `step()` until drained   (this change; row-exact, streamed)
  sequential  N `wire.convert_pcm16` calls at B = 1                         (code this change does not touch; row-exact)
  batched     ONE padded `wire.convert_pcm16` call of B = N                 (untouched code; NOT row-exact: every row gets
                                                                             the batch's one-shot decode — the throughput
                                                                             ceiling, not an alternative)

None normalises by a peak (the pool's streams have none before their last chunk).  The variants alternate round by
round (the order within a round rotates).  A round is timed by the host clock from the first call to a final device
synchronisation.  Rounds of their own, alternating the same way, time the way to the FIRST int16 piece of the first
request: admit + one step (pooled), the first call (sequential), the whole call (batched).  Medians over --reps rounds.

Before anything is reported every pooled stream is compared bitwise (z and the int16) with its stand-alone form,
`wire.stream_pcm16(net.convert_stream(...))` from the same RNG state; the script refuses to report when they differ.

    python scripts/convert_timing.py [--reps 9] [--out profiles/convert_timing.jsonl]

The per-kernel view and the launch counts per admission of 16 come from a profiler run of its own, no counters in it:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/convert_timing.py --profile admit
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
from mb_istft_vits_amd import wire          # noqa: E402
from mb_istft_vits_amd.models import ConvertRequest          # noqa: E402

CONFIG = "uudb_ms_istft_vits_ms"
MODEL_SR, RATE, HOP, WIN = 16000, 24000, 256, 1024
SECONDS = 3.0
MIXED = [0.3, 5.0, 1.2, 0.5, 3.3, 2.0, 0.8, 4.1, 1.7, 0.4, 2.6, 3.9, 1.0, 0.6, 4.6, 2.2]
PROFILE_ROUNDS = 4


def make_requests(seconds, seed=0):
    rs = np.random.RandomState(seed)
    reqs = []
    for k, sec in enumerate(seconds):
        n = int(sec * MODEL_SR) + (1, 0, 255)[k % 3]
        t = np.arange(n) / MODEL_SR
        x = 0.3 * np.sin(2 * np.pi * (150 + 20 * k) * t) + 0.2 * np.sin(2 * np.pi * 1234.5 * t + k) + 0.05 * rs.standard_normal(n)
        reqs.append(ConvertRequest(torch.from_numpy(x.astype(np.float32)).cuda(), k % 12, (5 * k + 2) % 12, MODEL_SR, HOP, WIN))
    return reqs


def padded_batch(reqs):
    wave = torch.nn.utils.rnn.pad_sequence([r.wave for r in reqs], batch_first=True)
    valid = torch.tensor([r.wave.numel() for r in reqs]).cuda()
    src = torch.tensor([r.sid_src for r in reqs]).cuda()
    tgt = torch.tensor([r.sid_tgt for r in reqs]).cuda()
    return wave, valid, src, tgt


def job(net, reqs, variant, batch, first_only=False):
    """The whole job one way; -> what it produced (pooled: the followers)."""
    if variant == "pooled":
        pp = wire.pcm_pool(net, net.stream_pool(), MODEL_SR, RATE)
        fol = pp.admit(reqs)
        pp.step()
        while not first_only and len(pp):
            pp.step()
        return fol
    if variant == "sequential":
        out = []
        for r, s, t in zip(reqs[:1] if first_only else reqs, batch[2], batch[3]):
            out.append(wire.convert_pcm16(net, r.wave[None], None, s[None], t[None], MODEL_SR, MODEL_SR, RATE, HOP, WIN,
                                          auto_normalize=False))
        return out
    wave, valid, src, tgt = batch
    return wire.convert_pcm16(net, wave, valid, src, tgt, MODEL_SR, MODEL_SR, RATE, HOP, WIN, auto_normalize=False)


def run_round(net, reqs, variant, batch, first_only=False, seed=3):
    torch.manual_seed(seed)
    torch.cuda.manual_seed(seed)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = job(net, reqs, variant, batch, first_only)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), out


def check_pooled(net, reqs, seed=3):
    """Every pooled stream against its stand-alone form, bitwise; -> the frame counts."""
    _, fol = run_round(net, reqs, "pooled", None, seed=seed)
    torch.manual_seed(seed)
    torch.cuda.manual_seed(seed)
    for k, (f, r) in enumerate(zip(fol, reqs)):
        st = net.convert_stream(r.wave, r.sid_src, r.sid_tgt, MODEL_SR, HOP, WIN)
        same_z = st.z.shape == f._st.z.shape and torch.equal(st.z, f._st.z)
        pcm, valid = wire.stream_pcm16(net, st, MODEL_SR, RATE).run()
        if not (same_z and torch.equal(pcm, f.pcm) and torch.equal(valid, f.valid_samples)):
            raise SystemExit("request %d: the pooled stream differs from its stand-alone form: nothing to report" % k)
    return [int(f._st.z.shape[2]) for f in fol]


VARIANTS = ("pooled", "sequential", "batched")


def measure(net, seconds, reps):
    reqs = make_requests(seconds)
    batch = padded_batch(reqs)
    frames = check_pooled(net, reqs)
    for v in VARIANTS + VARIANTS:                                  # warm-up: every variant's shapes, the arenas
        run_round(net, reqs, v, batch)
    res = {(v, f): [] for v in VARIANTS for f in (False, True)}
    for first_only in (False, True):
        for r in range(reps):
            order = VARIANTS[r % 3:] + VARIANTS[:r % 3]
            for v in order:
                res[(v, first_only)].append(run_round(net, reqs, v, batch, first_only)[0])
    cr, dr, wr = net.converter_runs(), net.decoder_runs(), wire.wire_runs(net)
    run_round(net, reqs, "pooled", batch)
    counts = dict(converter_runs=net.converter_runs() - cr, decoder_runs=net.decoder_runs() - dr, wire_runs=wire.wire_runs(net) - wr)

    def spread(v):
        s = sorted(v)
        return round(s[-2] - s[1], 3)                              # without the two extremes

    rec = dict(config=CONFIG, requests=len(seconds), seconds=seconds if len(set(seconds)) > 1 else seconds[0],
               frames=frames if len(frames) <= 16 else sum(frames), reps=reps, bitwise_equal=True, pooled_counts=counts)
    for v in VARIANTS:
        rec[v + "_wall_ms"] = round(statistics.median(res[(v, False)]), 3)
        rec[v + "_wall_spread_ms"] = spread(res[(v, False)])
        rec[v + "_first_pcm_ms"] = round(statistics.median(res[(v, True)]), 3)
    rec["sequential_over_pooled"] = round(rec["sequential_wall_ms"] / rec["pooled_wall_ms"], 3)
    rec["pooled_over_batched"] = round(rec["pooled_wall_ms"] / rec["batched_wall_ms"], 3)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile", choices=("admit", "sequential"), default=None,
                    help="N = 16: %d rounds of `convert_streams` alone, or of 16 convert_pcm16 calls (for rocprofv3)" % PROFILE_ROUNDS)
    args = ap.parse_args()
    if args.reps < 7:
        raise SystemExit("--reps must be at least 7")
    net = make_net(CONFIG)[0]
    if args.profile:
        reqs = make_requests([SECONDS] * 16)
        batch = padded_batch(reqs)
        for _ in range(PROFILE_ROUNDS):
            if args.profile == "admit":
                net.convert_streams(reqs)
            else:
                job(net, reqs, "sequential", batch)
        torch.cuda.synchronize()
        return
    lines = []
    for seconds in [[SECONDS] * n for n in (1, 2, 4, 16, 64)] + [MIXED]:
        lines.append(json.dumps(measure(net, seconds, args.reps)))
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
