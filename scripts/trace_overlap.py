#!/usr/bin/env python3
"""From a rocprofv3 kernel trace: conv launches that overlap in time with a conv launch on another queue."""
import csv, glob, sys
for d in sys.argv[1:]:
    f = sorted(glob.glob(d + "/**/*kernel_trace.csv", recursive=True))[0]
    rows = [r for r in csv.DictReader(open(f))]
    conv = [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Queue_Id"], r["Kernel_Name"]) for r in rows
            if "conv1d" in r["Kernel_Name"]]
    conv.sort()
    queues = sorted({c[2] for c in conv})
    tot = sum(e - s for s, e, _, _ in conv)
    ov = 0
    pairs = 0
    for i, (s, e, q, _) in enumerate(conv):
        for s2, e2, q2, _ in conv[i + 1:]:
            if s2 >= e:
                break
            if q2 != q:
                ov += min(e, e2) - s2
                pairs += 1
    fill = [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in rows if "tail_fill" in r["Kernel_Name"]]
    tmap = [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in rows if "tail_map" in r["Kernel_Name"]]
    span = max(e for _, e, _, _ in conv) - min(s for s, _, _, _ in conv)
    print("%s: %d conv launches on %d queues, sum of durations %.2f ms, pairwise overlap across queues %.2f ms in %d pairs; "
          "tail_fill %d x, %.3f ms in all; tail_map %d x, %.3f ms" %
          (d, len(conv), len(queues), tot / 1e6, ov / 1e6, pairs, len(fill), sum(fill) / 1e6, len(tmap), sum(tmap) / 1e6))
