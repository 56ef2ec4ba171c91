"""Per-token prosody timing, ljs_mb, T_text 200, B = 1 and B = 64.

  front      ms per `infer_z_only` call (encode, durations, length regulation, flows; no decoder), seeded:
               scalar   length_scale = 1.2 as a float -- the path of the parent commit, launch for launch
               table    the same 1.2 as a [B, 1, T] tensor: one `mbv_shape_durations` launch more
               extra    the float plus `extra_frames`
               fit      the float plus `fit_frames` (the bisection: up to 32 evaluations of D inside the one launch)
             The difference to `scalar` is what the launch costs inside a call; `table` computes the same durations,
             `extra` and `fit` make the utterance longer or shorter, so their calls also do other work in the flows.
  op         ms per `mbv_op_shape_durations` call on a [B, T] logw (host-timed, each call ends in a stream
             synchronisation: launch + kernel + wake-up), without and with a fit, against `mbv_op_durations` on the
             same logw (the kernel the scalar path runs anyway)
  admit      ms per `infer_streams` call of 16 requests (T_text 40 .. 200), none shaped / all shaped with a table

    python scripts/prosody_timing.py [--reps 9] [--out profiles/prosody_timing.jsonl]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CONFIG = "ljs_mb_istft_vits"
T_TEXT = 200


def timed(fn, n):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def median_of(fn, reps, n):
    fn()
    return statistics.median(timed(fn, n) for _ in range(reps))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prosody_timing.jsonl"))
    args = ap.parse_args()
    import numpy as np
    import torch
    from gpu_util import make_net, ptr
    from mb_istft_vits_amd import _capi, synth
    from mb_istft_vits_amd.models import Request
    net, _ = make_net(CONFIG)
    h, L = net._ensure_handle(), _capi.lib()
    rows = []

    def emit(**kw):
        kw.update(config=CONFIG, device=torch.cuda.get_device_name(0))
        rows.append(kw)
        print(json.dumps(kw))

    for B in (1, 64):
        x, xl, _ = synth.synthetic_batch(net.cfg, B, T_TEXT, seed=0)
        x, xl = torch.from_numpy(x).cuda(), torch.from_numpy(xl).cuda()
        tab = torch.full((B, 1, T_TEXT), 1.2).cuda()
        ex = (torch.arange(T_TEXT) % 10 == 0).to(torch.int32).mul(20).repeat(B, 1).cuda()
        kw = dict(noise_scale=0.667, seed=3)
        base = net.infer_with_lengths(x, xl, length_scale=1.2, outputs=("z",), **kw)[1]
        fit = [int(v * 0.9) for v in base.tolist()]
        n = 20 if B == 1 else 5
        t = {"scalar": median_of(lambda: net.infer_z_only(x, xl, length_scale=1.2, **kw), args.reps, n),
             "table": median_of(lambda: net.infer_z_only(x, xl, length_scale=tab, **kw), args.reps, n),
             "extra": median_of(lambda: net.infer_z_only(x, xl, length_scale=1.2, extra_frames=ex, **kw), args.reps, n),
             "fit": median_of(lambda: net.infer_z_only(x, xl, length_scale=1.2, fit_frames=fit, **kw), args.reps, n)}
        emit(what="front", B=B, T_text=T_TEXT, ms=t, table_minus_scalar_ms=t["table"] - t["scalar"])

        # the kernel by itself on the call's logw
        logw = net.read_stage("logw").view(B, T_TEXT).contiguous()
        lens = xl.to(torch.int32)
        w = torch.empty(B, T_TEXT, device="cuda")
        lw2 = torch.empty(B, T_TEXT, device="cuda")
        cum = torch.empty(B, T_TEXT, dtype=torch.int32, device="cuda")
        y32 = torch.empty(B, dtype=torch.int32, device="cuda")
        y64 = torch.empty(B, dtype=torch.int64, device="cuda")
        fo = torch.empty(B, dtype=torch.int64, device="cuda")
        s2 = tab.view(B, T_TEXT).contiguous()
        fits = (_capi.MbvFit * B)(*[(v, 0.5, 2.0) for v in fit])
        stream = net._stream()

        def op(fit_host):
            _capi.check(h, L.mbv_op_shape_durations(h, ptr(logw), ptr(lens), ptr(s2), ptr(ex), 1.0, fit_host, ptr(w),
                                                    ptr(cum), ptr(y32), ptr(y64), None, ptr(fo), B, T_TEXT, stream), "op")

        def op_plain():
            _capi.check(h, L.mbv_op_durations(h, ptr(logw), None, None, ptr(lens), 1.2, ptr(lw2), ptr(w), ptr(cum), ptr(y32),
                                              ptr(y64), None, B, 1, T_TEXT, stream), "op")

        emit(what="op", B=B, T_text=T_TEXT,
             ms={"durations_kernel": median_of(op_plain, args.reps, 50), "shape": median_of(lambda: op(None), args.reps, 50),
                 "shape_fit": median_of(lambda: op(fits), args.reps, 50)})

    g = torch.Generator().manual_seed(5)
    lens = [40 + 10 * i for i in range(16)] + [200]
    ids = [torch.randint(1, 59, (T,), generator=g) for T in lens[:16]]
    plain = [Request(x, noise_scale=0.667, length_scale=1.2, seed=i) for i, x in enumerate(ids)]
    shaped = [Request(x, noise_scale=0.667, length_scale=torch.full((x.numel(),), 1.2), seed=i) for i, x in enumerate(ids)]
    t = {"plain": median_of(lambda: net.infer_streams(plain), args.reps, 5),
         "table": median_of(lambda: net.infer_streams(shaped), args.reps, 5)}
    emit(what="admit", requests=16, ms=t, table_minus_plain_ms=t["table"] - t["plain"])

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
