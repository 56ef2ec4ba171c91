"""Per-token volume, timing: ljs_mb, 22 050 -> 24 000 Hz, a pooled tick of 8 streams of one 3 s
utterance each (258 z-frames; chunks 32, 64, 128, 34), every tick ending with its pieces on the host.

(a) What the envelope costs a tick that has none.  The unshaped pooled tick (the workload of scripts/pcm_pool_timing.py)
    and the unshaped limited tick (that of scripts/limiter_timing.py) on this build against a build of the parent
    commit (`--parent-lib`).  A process loads one library, so every round starts one worker process per build, in
    alternating order; a worker warms up and reports the median of its own inner repetitions.
(b) What a shaped tick costs: every stream carries an envelope (`PcmPool.add(envelope=)`), against the unshaped tick of
    the same worker.

Reported: medians over --reps rounds with the fastest and slowest round beside them, and for (a) whether the
difference of the medians stays inside the parent's own fastest-to-slowest spread.

    python scripts/gain_timing.py [--reps 9] [--parent-lib /path/to/parent/libmbistft_vits.so] [--out profiles/gain_timing.jsonl]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIG = "ljs_mb_istft_vits"
MODEL_SR, RATE = 22050, 24000
T_3S, STREAMS = 258, 8
CHUNK, CAP = 32, 256
INNER = 5


def stats(values):
    return dict(median=round(statistics.median(values), 4), min=round(min(values), 4), max=round(max(values), 4))


# ---------------------------------------------------------------------------------------------- the worker
def worker(shaped_too):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from gpu_util import make_net
    from mb_istft_vits_amd import wire

    net = make_net(CONFIG)[0]
    g = torch.Generator().manual_seed(STREAMS)
    zs = [torch.randn(1, net.cfg.inter_channels, T_3S, generator=g).cuda() for _ in range(STREAMS)]
    limiter = wire.Limiter()
    tables = None
    if shaped_too:
        rs = np.random.RandomState(5)
        tables = [torch.from_numpy(rs.uniform(0.25, 2.0, (1, T_3S + 1)).astype(np.float32)).cuda() for _ in zs]

    def all_ticks(limited, shaped):
        """-> (ms for every tick of the pool, wire launches)"""
        sts = [net.dec_stream(z, None, CHUNK, CAP) for z in zs]
        pp = wire.pcm_pool(net, net.stream_pool(), MODEL_SR, RATE)
        for st, k in zip(sts, range(STREAMS)):
            kw = dict(envelope=wire.Envelope(tables[k], st.spf)) if shaped else {}
            pp.add(st, peak=0.05 if limited else None, limiter=limiter if limited else None, **kw)
        torch.cuda.synchronize()
        r0 = wire.wire_runs(net)
        t0 = time.perf_counter()
        while len(pp):
            pp.step(host=True)
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0), wire.wire_runs(net) - r0

    variants = [(lim, sh) for sh in ((False, True) if shaped_too else (False,)) for lim in (False, True)]
    for v in variants * 2:
        all_ticks(*v)
    res = {v: [] for v in variants}
    for r in range(INNER):
        for v in (variants if r % 2 == 0 else variants[::-1]):
            res[v].append(all_ticks(*v))
    out = {}
    for (lim, sh), rows in res.items():
        name = ("shaped_" if sh else "unshaped_") + ("limited" if lim else "pooled")
        out[name + "_ms"] = statistics.median(ms for ms, _ in rows)
        out[name + "_wire_runs"] = rows[0][1]
    print("WORKER " + json.dumps(out), flush=True)


def run_worker(lib, shaped_too):
    env = dict(os.environ)
    env.pop("MBV_LIB", None)
    if lib:
        env["MBV_LIB"] = lib
    cmd = [sys.executable, os.path.abspath(__file__), "--worker"] + (["--shaped"] if shaped_too else [])
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    if r.returncode:
        raise SystemExit("worker failed (%d):\n%s" % (r.returncode, r.stderr[-2000:]))
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("WORKER ")][-1]
    return json.loads(line[len("WORKER "):])


# ---------------------------------------------------------------------------------------------- the driver
def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--parent-lib", default=None, help="libmbistft_vits.so built from the parent commit")
    ap.add_argument("--out", default=None)
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--shaped", action="store_true")
    args = ap.parse_args()
    if args.worker:
        worker(args.shaped)
        return
    if args.reps < 7:
        raise SystemExit("--reps must be at least 7")
    here, parent = [], []
    for r in range(args.reps):
        order = ("here", "parent") if r % 2 == 0 else ("parent", "here")
        for which in order:
            if which == "here":
                here.append(run_worker(None, True))
            elif args.parent_lib:
                parent.append(run_worker(os.path.abspath(args.parent_lib), False))
        print("round %d done" % r, flush=True)
    lines = []
    for kind in ("pooled", "limited"):
        name = "unshaped_%s_ms" % kind
        rec = dict(what="unshaped_%s_tick_against_parent" % kind, config=CONFIG, model_sr=MODEL_SR, rate=RATE,
                   streams=STREAMS, frames=T_3S, chunk_frames=CHUNK, max_chunk_frames=CAP, reps=args.reps, inner=INNER,
                   here_all_ticks_ms=stats([w[name] for w in here]),
                   wire_runs=here[0]["unshaped_%s_wire_runs" % kind])
        if parent:
            p = stats([w[name] for w in parent])
            rec["parent_all_ticks_ms"] = p
            rec["difference_ms"] = round(rec["here_all_ticks_ms"]["median"] - p["median"], 4)
            rec["parent_spread_ms"] = round(p["max"] - p["min"], 4)
            rec["inside_parent_spread"] = abs(rec["difference_ms"]) <= rec["parent_spread_ms"]
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        s, u = stats([w["shaped_%s_ms" % kind] for w in here]), rec["here_all_ticks_ms"]
        rec = dict(what="shaped_%s_tick_against_unshaped" % kind, config=CONFIG, streams=STREAMS, frames=T_3S, reps=args.reps,
                   inner=INNER, shaped_all_ticks_ms=s, unshaped_all_ticks_ms=u, ratio=round(s["median"] / u["median"], 4),
                   shaped_wire_runs=here[0]["shaped_%s_wire_runs" % kind],
                   unshaped_wire_runs=here[0]["unshaped_%s_wire_runs" % kind])
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
