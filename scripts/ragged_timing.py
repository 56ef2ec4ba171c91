"""Row-exact ragged decode timing, ljs_mb, one run with the variants alternating.

  batch    the ragged bench batch of DESIGN §7 (B = 64, text lengths 120-200, noise_scale 0): ms per `infer` call
           in the default mode, with trim=True and with ragged=True — and, with --baseline-lib, the default mode of
           another build of the library (the parent commit's), measured by a child process of this run (MBV_LIB is
           read at import, so one process holds one build), alternating with this process round by round.
  service  B = 8 requests of mixed lengths (40 ... 260 frames): one `net.dec(z, lengths=...)` call in the mode
           against the same eight rows as B = 1 `net.dec` calls (the only way to get that audio without the mode),
           in the default and the split-K modes.

    python scripts/ragged_timing.py [--reps 9] [--baseline-lib PATH] [--out file.jsonl]

The per-kernel view comes from a profiler run of its own:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/ragged_timing.py --profile
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CONFIG = "ljs_mb_istft_vits"
SERVICE_LENS = (260, 40, 180, 75, 230, 120, 58, 150)


def bench_batch(net):
    import torch
    from mb_istft_vits_amd import synth
    x, xl, _ = synth.synthetic_batch(net.cfg, 64, 200, seed=0, ragged=True)
    return torch.from_numpy(x).cuda(), torch.from_numpy(xl).cuda()


def classes_hit(net, lens, splitk=False):
    """How many decoder runs (= classes of lengths, at these sizes) the ragged mode makes for a batch."""
    return net.ragged_plan(list(lens), splitk=splitk)[0]


def timed(fn, n):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def child(args):
    """The default-mode infer of the library MBV_LIB names, one round per line read from stdin."""
    from gpu_util import make_net
    net = make_net(CONFIG)[0]
    x, xl = bench_batch(net)
    step = lambda: net.infer(x, xl, noise_scale=0, length_scale=1, outputs=("o",))
    timed(step, 2)
    print("ready", flush=True)
    for _ in sys.stdin:
        print(json.dumps(timed(step, args.inner)), flush=True)


def measure(args):
    import torch
    from gpu_util import make_net
    net = make_net(CONFIG)[0]
    med = lambda v: round(statistics.median(v), 3)
    lines = []

    # ---- the ragged bench batch
    x, xl = bench_batch(net)
    kw = dict(noise_scale=0, length_scale=1, outputs=("o",))
    variants = {"default": lambda: net.infer(x, xl, **kw), "trim": lambda: net.infer(x, xl, trim=True, **kw),
                "ragged": lambda: net.infer(x, xl, ragged=True, **kw)}
    base = None
    if args.baseline_lib:
        env = dict(os.environ, MBV_LIB=os.path.abspath(args.baseline_lib))
        base = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--child", "--inner", str(args.inner)],
                                stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, env=env)
        assert base.stdout.readline().strip() == "ready"
    for fn in variants.values():
        timed(fn, 2)
    (_, *_), yl = net.infer_with_lengths(x, xl, ragged=True, **kw)
    runs = classes_hit(net, [int(v) for v in yl.tolist()])
    ms = {k: [] for k in list(variants) + ["parent_default"]}
    for _ in range(args.reps):
        if base:
            base.stdin.write("go\n")
            base.stdin.flush()
            ms["parent_default"].append(json.loads(base.stdout.readline()))
        for k, fn in variants.items():
            ms[k].append(timed(fn, args.inner))
    if base:
        base.stdin.close()
        base.wait(timeout=60)
    frames = yl.tolist()
    rec = dict(case="bench_batch", config=CONFIG, B=64, t_text="120-200", frames_min=min(frames), frames_max=max(frames),
               padded_fraction=round(1 - sum(frames) / (64 * max(frames)), 4), ragged_decoder_runs=runs,
               reps=args.reps, calls_per_rep=args.inner,
               **{k + "_ms": (med(v) if v else None) for k, v in ms.items()})
    lines.append(json.dumps(rec))
    print(lines[-1], flush=True)

    # ---- the service case
    T = max(SERVICE_LENS)
    z = torch.randn(len(SERVICE_LENS), net.cfg.inter_channels, T, generator=torch.Generator().manual_seed(1)).cuda()
    rows = [z[b:b + 1, :, :n].contiguous() for b, n in enumerate(SERVICE_LENS)]
    for mode in ("default", "splitk"):
        net.set_option("splitk", int(mode == "splitk"))
        outs = [torch.empty(1, 1, 256 * n, device="cuda") for n in SERVICE_LENS]
        one = lambda: net.dec(z, lengths=SERVICE_LENS)
        eight = lambda: [net._decode_into(r, None, (o_, None, None, None)) for r, o_ in zip(rows, outs)]
        timed(one, 2), timed(eight, 2)
        classes = classes_hit(net, SERVICE_LENS, splitk=mode == "splitk")
        a, b = [], []
        for _ in range(args.reps):
            a.append(timed(one, args.inner))
            b.append(timed(eight, args.inner))
        rec = dict(case="service", config=CONFIG, B=len(SERVICE_LENS), frames=list(SERVICE_LENS), mode=mode,
                   ragged_decoder_runs=classes, one_ragged_call_ms=med(a), eight_b1_calls_ms=med(b),
                   reps=args.reps, calls_per_rep=args.inner)
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    net.set_option("splitk", 0)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def profile(args):
    import torch
    from gpu_util import make_net
    net = make_net(CONFIG)[0]
    x, xl = bench_batch(net)
    kw = dict(noise_scale=0, length_scale=1, outputs=("o",))
    z = torch.randn(len(SERVICE_LENS), net.cfg.inter_channels, max(SERVICE_LENS)).cuda()
    for _ in range(args.reps):
        net.infer(x, xl, **kw)
        net.infer(x, xl, ragged=True, **kw)
        net.dec(z, lengths=SERVICE_LENS)
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=5, help="calls per timed round")
    ap.add_argument("--baseline-lib", default=None, help="another build of libmbistft_vits.so (the parent commit's)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile", action="store_true", help="only run the calls (under rocprofv3)")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        child(args)
    elif args.profile:
        profile(args)
    else:
        measure(args)


if __name__ == "__main__":
    main()
