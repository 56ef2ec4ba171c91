#!/usr/bin/env python3
"""Time of the linear spectrogram (mbv_spectrogram, n_fft 1024, hop 256, win 1024) against torch's GPU path
(F.pad + torch.stft (rocFFT) + abs, as spectrogram_torch computes it) in the same process, for 64 rows of 10 s
at 22 050 Hz (the measurement shape), 256 rows of the same (past the 256 MiB Infinity Cache) and one 3 s
utterance.  Prints one JSON line per case: HIP-event time per call, algorithmic bytes (samples read once,
spectrogram written once) and their fraction of 6.3 TB/s.  The kernel time itself comes from a
`rocprofv3 --kernel-trace` run of this script; `--stats <kernel_trace.csv>` summarises that trace per case."""
import csv, json, os, re, sys

N_FFT, HOP, WIN = 1024, 256, 1024
CASES = (("B64_10s", 64, 220500), ("B256_10s", 256, 220500), ("b1_3s", 1, 3 * 22050))
HBM = 6.3e12


def frames(n):
    return 1 + (n + 2 * ((N_FFT - HOP) // 2) - N_FFT) // HOP


def algo_bytes(B, n):
    return B * n * 4 + B * (N_FFT // 2 + 1) * frames(n) * 4


def stats(trace):
    """per-dispatch durations of mbv's spectrogram kernel, grouped by case (grid y = rows)"""
    rows = {}
    for r in csv.DictReader(open(trace)):
        if "spectrogram_kernel" in r["Kernel_Name"]:
            us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
            rows.setdefault((r["Kernel_Name"], int(r["Grid_Size_X"]), int(r["Grid_Size_Y"]), int(r["VGPR_Count"])),
                            []).append(us)
    w = csv.writer(sys.stdout)
    w.writerow(["kernel", "case", "grid_x", "grid_y", "vgpr", "calls", "median_us", "min_us", "max_us",
                "hbm_fraction"])
    for (name, gx, gy, vgpr), t in sorted(rows.items(), key=lambda kv: kv[0][2]):
        t.sort()
        case = next(c for c in CASES if c[1] == gy)
        med = t[len(t) // 2]
        w.writerow([re.search(r"spectrogram_kernel<[^>]*>", name).group(0), "%s (%d x %d samples)" % case, gx // 256, gy, vgpr, len(t), round(med, 1),
                    round(t[0], 1), round(t[-1], 1), round(algo_bytes(case[1], case[2]) / (med * 1e-6) / HBM, 3)])


def main():
    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    from gpu_util import make_net

    net, _ = make_net("ljs_mini_mb_istft_vits")
    window = torch.hann_window(WIN, device="cuda")
    p = (N_FFT - HOP) // 2

    def torch_path(x):
        y = torch.nn.functional.pad(x.unsqueeze(1), (p, p), mode="constant", value=0).squeeze(1)
        return torch.abs(torch.stft(y, N_FFT, hop_length=HOP, win_length=WIN, window=window, center=False,
                                    pad_mode="reflect", normalized=False, onesided=True, return_complex=True))

    def per_call(fn, reps):
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps * 1e3

    for name, B, n in CASES:
        x = torch.rand(B, n, device="cuda") * 2 - 1
        ours = per_call(lambda: net.spectrogram(x, N_FFT, HOP, WIN), 50)
        theirs = per_call(lambda: torch_path(x), 20)
        got = net.spectrogram(x, N_FFT, HOP, WIN)[0]
        ref = torch_path(x)
        rel = float(((got - ref).double().pow(2).mean().sqrt() / ref.double().pow(2).mean().sqrt()).item())
        nbytes = algo_bytes(B, n)
        print(json.dumps({"case": name, "B": B, "samples": n, "frames": frames(n), "us_per_call": round(ours, 2),
                          "torch_stft_us_per_call": round(theirs, 2), "speedup": round(theirs / ours, 2),
                          "algo_MB": round(nbytes / 1e6, 1), "hbm_fraction": round(nbytes / (ours * 1e-6) / HBM, 3),
                          "rel_rms_vs_torch_fp32": float("%.3g" % rel)}))
        del x, got, ref
        torch.cuda.empty_cache()


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--stats":
        stats(sys.argv[2])
    else:
        main()
