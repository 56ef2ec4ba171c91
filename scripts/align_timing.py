"""Forced-alignment timing, ljs_mb, T_text 200, T_spec 566, B = 64 and B = 1.

  align      ms per `net.align` call (all outputs, and outputs=("w",))
  kernels    ms per `mbv_op_neg_cent` / `mbv_op_max_path` call on the call's own tensors (host-timed, each call
             ends in a stream synchronisation: launch + kernel + wake-up; the kernel time alone is in the profiler run)
  share      1 - (text encoder + neg_cent + search) / align: what enc_q and the forward flows take.  The text
             encoder's time is the `text_encoder` stage of an `infer` call on the same text.
  reference  the reference's route restated with what exists here: torch.matmul for the four terms on the GPU, a copy
             to the host, and the NumPy fp32 search of tests/align_ref.py (a Python loop, not the Cython one: for
             scale only).  B = 64: the search is run on --ref-rows rows and scaled to the batch.

    python scripts/align_timing.py [--reps 9] [--out file.jsonl]

The per-kernel view comes from a profiler run of its own:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/align_timing.py --profile
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CONFIG = "ljs_mb_istft_vits"
T_TEXT, T_SPEC = 200, 566


def batch(net, B):
    import numpy as np
    import torch
    from mb_istft_vits_amd import synth
    x, xl, _ = synth.synthetic_batch(net.cfg, B, T_TEXT, seed=0)
    rs = np.random.RandomState(1)
    y = np.abs(rs.standard_normal((B, net.cfg.spec_channels, T_SPEC))).astype(np.float32) * 2.0
    yl = np.full((B,), T_SPEC, np.int64)
    return tuple(torch.from_numpy(a).cuda() for a in (x, xl, y, yl))


def timed(fn, n):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def median_of(fn, reps, n):
    return statistics.median(timed(fn, n) for _ in range(reps))


def reference_route(z_p, m_p, logs_p, rows):
    """models.py:670-675 with torch on the GPU, the copy of monotonic_align/__init__.py:13, the NumPy search."""
    import numpy as np
    import torch
    import align_ref
    torch.matmul(z_p.transpose(1, 2), m_p)                   # (the BLAS library's first-call set-up stays outside)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    s = torch.exp(-2 * logs_p)
    n1 = torch.sum(-0.5 * math.log(2 * math.pi) - logs_p, [1], keepdim=True)
    n2 = torch.matmul(-0.5 * (z_p ** 2).transpose(1, 2), s)
    n3 = torch.matmul(z_p.transpose(1, 2), m_p * s)
    n4 = torch.sum(-0.5 * (m_p ** 2) * s, [1], keepdim=True)
    v = (n1 + n2 + n3 + n4).cpu().numpy().astype(np.float32)
    t1 = time.perf_counter()
    for b in range(rows):
        align_ref.maximum_path_each(v[b], T_SPEC, T_TEXT, np.float32)
    t2 = time.perf_counter()
    return (t1 - t0) * 1e3, (t2 - t1) * 1e3 / rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--ref-rows", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile", action="store_true", help="a few align calls only (for rocprofv3)")
    args = ap.parse_args()
    import torch
    from gpu_util import make_net, ptr
    from mb_istft_vits_amd import _capi
    net = make_net(CONFIG)[0]
    L, h = _capi.lib(), net._ensure_handle()
    rows = []
    for B in (64, 1):
        x, xl, y, yl = batch(net, B)
        full = lambda: net.align(x, xl, y, yl, noise_scale=0)
        w_only = lambda: net.align(x, xl, y, yl, noise_scale=0, outputs=("w",))
        for _ in range(3):
            full()
        if args.profile:
            for _ in range(5):
                full()
            continue
        n = 5 if B == 64 else 20
        r = net.align(x, xl, y, yl, noise_scale=0, outputs=("z_p", "neg_cent", "w"))
        z_p, value = r[4][1], r[5]
        c = net.infer(x, xl, noise_scale=0, outputs=("z",))       # (m->stats of this text: read below)
        stats = net.read_stage("stats").reshape(B, 2, net.cfg.inter_channels, T_TEXT)
        m_p, logs_p = stats[:, 0].contiguous(), stats[:, 1].contiguous()
        t_enc = statistics.median(float(dict(net.infer(x, xl, noise_scale=0, outputs=("z",))[7])["text_encoder"]) * 1e3
                                  for _ in range(args.reps))
        ty = torch.full((B,), T_SPEC, dtype=torch.int32, device="cuda")
        tx = torch.full((B,), T_TEXT, dtype=torch.int32, device="cuda")
        v2 = torch.empty_like(value)
        w32 = torch.empty(B, T_TEXT, dtype=torch.int32, device="cuda")
        st = torch.empty(B, dtype=torch.int32, device="cuda")
        I = net.cfg.inter_channels
        k_nc = lambda: L.mbv_op_neg_cent(h, ptr(z_p), ptr(m_p), ptr(logs_p), ptr(ty), ptr(tx), ptr(v2), B, I, T_SPEC, T_TEXT, net._stream())
        k_mp = lambda: L.mbv_op_max_path(h, ptr(value), ptr(ty), ptr(tx), ptr(w32), None, ptr(st), B, T_SPEC, T_TEXT, net._stream())
        k_nc(), k_mp()
        assert torch.equal(w32.float().unsqueeze(1), r[1])
        ms_full, ms_w = median_of(full, args.reps, n), median_of(w_only, args.reps, n)
        ms_nc, ms_mp = median_of(k_nc, args.reps, 20), median_of(k_mp, args.reps, 20)
        ref_rows = min(args.ref_rows, B)
        ref_mat, ref_row = reference_route(z_p, m_p, logs_p, ref_rows)
        row = dict(config=CONFIG, B=B, T_text=T_TEXT, T_spec=T_SPEC, align_ms=round(ms_full, 3), align_w_only_ms=round(ms_w, 3),
                   neg_cent_call_ms=round(ms_nc, 4), max_path_call_ms=round(ms_mp, 4), text_encoder_ms=round(t_enc, 3),
                   enc_q_and_flows_share=round(1 - (t_enc + ms_nc + ms_mp) / ms_full, 3),
                   neg_cent_gflop=round(2 * 2 * I * B * T_SPEC * T_TEXT / 1e9, 2),
                   reference_route=dict(matmul_and_copy_ms=round(ref_mat, 2), numpy_search_ms_per_row=round(ref_row, 1),
                                        numpy_search_rows_timed=ref_rows, total_ms_scaled=round(ref_mat + ref_row * B, 1)))
        del c
        print(json.dumps(row))
        rows.append(row)
    if args.out and rows:
        with open(args.out, "w") as f:
            for row in rows:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
