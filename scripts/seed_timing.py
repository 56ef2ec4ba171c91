"""Seeded against unseeded admission: uudb_ms, 16 text requests admitted at once by
`net.infer_streams`, with the StochasticDurationPredictor (`use_sdp` override) and without it.

Both variants run on the same build in the same process, on the same texts:

  unseeded  `Request(...)`          the prior draws are N `normal_()` launches, the SDP draws N `torch.randn` on the CPU,
                                    one `torch.cat` and one host-to-device copy
  seeded    `Request(..., seed=s)`  one `mbv_randn_blocks` launch for the prior blocks, one more for the SDP blocks

The variants alternate round by round (the order within a round alternates too), after a warm-up of both.  A round is
--inner admissions, timed by the host clock to a final device synchronisation and by a pair of HIP events round the
same calls.  Reported per model, medians over --reps rounds, per admission:

  wall_ms, event_ms          as above, divided by --inner
  wall_spread_ms             the rounds' spread without the two extremes
  noise_runs                 `mbv_noise_runs` per admission: exact, and what the tests gate (the time is reported only)
  per_request_draws          the launches / CPU draws the unseeded variant makes for its noise: N, or 2 N with the SDP

Before anything is reported, the seeded streams are checked to be bitwise the same in every round, and bitwise
`infer_stream(..., seed=[s])` of each request alone.

    python scripts/seed_timing.py [--reps 9] [--inner 10] [--out profiles/seed_timing.jsonl]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from gpu_util import make_net          # noqa: E402
from mb_istft_vits_amd.models import Request          # noqa: E402

CONFIG = "uudb_ms_istft_vits_ms"
LENGTHS = [9, 16, 40, 64, 100, 200, 256, 300, 12, 30, 120, 400, 60, 17, 257, 150]     # both classes of admit_plan


def make_requests(net, seeded):
    g = torch.Generator().manual_seed(0)
    return [Request(torch.randint(1, 59, (t,), generator=g), sid=k % net.n_speakers, noise_scale=0.667, noise_scale_w=0.8,
                    seed=100 + k if seeded else None) for k, t in enumerate(LENGTHS)]


def run_round(net, reqs, inner):
    """-> (wall ms, event ms, noise runs) per admission, and the streams of the last one"""
    torch.manual_seed(3)
    torch.cuda.manual_seed(3)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    r0 = net.noise_runs()
    t0 = time.perf_counter()
    e0.record()
    for _ in range(inner):
        sts = net.infer_streams(reqs)
    e1.record()
    torch.cuda.synchronize()
    wall = 1e3 * (time.perf_counter() - t0)
    return wall / inner, e0.elapsed_time(e1) / inner, (net.noise_runs() - r0) / inner, sts


def measure(use_sdp, reps, inner):
    net = make_net(CONFIG, overrides={"use_sdp": True} if use_sdp else None)[0]
    reqs = {True: make_requests(net, True), False: make_requests(net, False)}
    for seeded in (True, False, True, False):                     # warm-up: both variants' shapes, the arenas
        run_round(net, reqs[seeded], 2)
    res = {True: [], False: []}
    for r in range(reps):
        for seeded in ((True, False) if r % 2 == 0 else (False, True)):
            res[seeded].append(run_round(net, reqs[seeded], inner))
    first, last = res[True][0][3], res[True][-1][3]
    repeat = all(torch.equal(a.z, b.z) and torch.equal(a.y_lengths, b.y_lengths) for a, b in zip(first, last))
    alone = True
    for r, st in zip(reqs[True], last):
        solo = net.infer_stream(r.x[None].cuda(), torch.tensor([r.x.numel()]).cuda(), torch.tensor([r.sid]).cuda(),
                                r.noise_scale, r.length_scale, r.noise_scale_w, seed=[r.seed])
        alone = alone and solo.z.shape == st.z.shape and torch.equal(solo.z, st.z)
    if not (repeat and alone):
        raise SystemExit("seeded streams differ between rounds or from the stand-alone seeded calls")

    def med(variant, k):
        return round(statistics.median(r[k] for r in res[variant]), 3)

    def spread(variant, k):
        v = sorted(r[k] for r in res[variant])
        return round(v[-2] - v[1], 3)                              # without the two extremes

    n = len(LENGTHS)
    rec = dict(config=CONFIG, use_sdp=bool(use_sdp), requests=n, tokens=LENGTHS,
               frames=int(sum(s.z.shape[2] for s in last)), reps=reps, inner=inner, seeded_bitwise_repeatable=repeat,
               seeded_bitwise_stand_alone=alone, per_request_draws=2 * n if use_sdp else n)
    for variant, name in ((True, "seeded"), (False, "unseeded")):
        rec[name + "_wall_ms"], rec[name + "_event_ms"] = med(variant, 0), med(variant, 1)
        rec[name + "_wall_spread_ms"] = spread(variant, 0)
        rec[name + "_noise_runs"] = res[variant][0][2]
    rec["wall_ratio"] = round(rec["unseeded_wall_ms"] / rec["seeded_wall_ms"], 3)
    want = 2 if use_sdp else 1
    if rec["seeded_noise_runs"] != want or rec["unseeded_noise_runs"] != 0:
        raise SystemExit("launch counts off: seeded %r (expected %d), unseeded %r (expected 0)"
                         % (rec["seeded_noise_runs"], want, rec["unseeded_noise_runs"]))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.reps < 7 or args.inner < 1:
        raise SystemExit("--reps must be at least 7 and --inner at least 1")
    lines = []
    for use_sdp in (False, True):
        lines.append(json.dumps(measure(use_sdp, args.reps, args.inner)))
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
