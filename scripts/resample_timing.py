#!/usr/bin/env python3
"""Time of the resampler (mbv_resample, 22050 -> 24000, kaiser_best) at the flagship batch shape (64 rows of
256 * 600 samples, ~10.7 M outputs) and for one 3 s utterance, from HIP events around repeated calls.
Prints one JSON line per case (HIP-event time per call, launch gaps included); the kernel time itself comes from a
rocprofv3 --kernel-trace run of this script."""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
from gpu_util import make_net

net, _ = make_net("ljs_mini_mb_istft_vits")
for name, B, n in (("bench_B64", 64, 256 * 600), ("b1_3s", 1, 3 * 22050)):
    x = torch.rand(B, 1, n, device="cuda") * 2 - 1
    for _ in range(5):
        out, ns = net.resample(x, 22050, 24000)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    reps = 50
    e0.record()
    for _ in range(reps):
        out, ns = net.resample(x, 22050, 24000)
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) / reps * 1e3
    outs = B * out.shape[-1]
    flop = 2.0 * outs * 128
    print(json.dumps({"case": name, "B": B, "in_samples": n, "out_samples": outs, "us_per_call": round(us, 2),
                      "gflop": round(flop / 1e9, 3), "tflops": round(flop / us / 1e6, 2)}))
