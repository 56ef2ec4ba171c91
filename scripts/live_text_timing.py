"""Live text: when the first audio leaves, what the stream costs, and how far a bounded text look-ahead is
from the whole-text stream.

  workload    a 200-token text pushed 4 tokens at a time, without sleeping, a `poll()` after each push; block_tokens 16,
              chunks 32 .. 256, on `uudb_ms_istft_vits_ms` and `ljs_mb_istft_vits`.
  first       tokens pushed and host milliseconds (with a device synchronisation) when the first chunk is handed out,
              for `TextAhead(tokens=4)`; against `infer_stream` on the whole text up to its first chunk, which needs all
              200 tokens before it starts.
  total       host clock from opening the stream to a final device synchronisation, against `infer_stream` decoded to
              the end; the two alternate, medians over --reps rounds (7).  `whole_text` is `TextAhead(tokens=None)`: one
              encoder pass, so the difference to `tokens=4` is what re-encoding every prefix costs.
  launches    the counters over one stream: ticks, and encoder / text / flow / decoder runs.
  pool        eight text streams fed in step through one `StreamPool.step()` per tick, against the same eight polled
              alone one after the other.
  deviation   relative rms of z and of the waveform for `TextAhead(tokens=A)`, A in {0, 4, 16, None}, from the
              whole-text stream (over the frames both have: the durations of a prefix call differ too, so T differs).
              This is measured ON THE CHECKPOINT AT HAND.  The repository ships synthetic weights: the figures say how
              far random layers look, and nothing about a trained model.  No quality claim is made.

    python scripts/live_text_timing.py [--reps 7] [--out profiles/live_text_timing.jsonl]
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
from mb_istft_vits_amd.stream import TextAhead          # noqa: E402

CONFIGS = ["uudb_ms_istft_vits_ms", "ljs_mb_istft_vits"]
TOKENS, PIECE, MAX_FRAMES = 200, 4, 4096
NOTE = ("measured on synthetic weights (the only ones the repository ships): no quality claim; the deviation says how far "
        "random layers look, nothing about a trained model")


def ids_of(k=0):
    return torch.randint(1, 59, (TOKENS,), generator=torch.Generator().manual_seed(500 + k)).tolist()


def sid_of(net, k=0):
    return (3 + k) % 12 if net.n_speakers > 0 else None


def open_text(net, k, tokens):
    return net.infer_live(sid=sid_of(net, k), max_tokens=TOKENS, max_frames=MAX_FRAMES, seed=100 + k,
                          ahead=TextAhead(tokens=tokens))


def live_round(net, ids, tokens, k=0):
    """-> (total ms, stream, tokens pushed at the first chunk, ms at the first chunk, ticks)."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    st = open_text(net, k, tokens)
    first_tokens = first_ms = None
    ticks = 0

    def tick():
        nonlocal first_tokens, first_ms, ticks
        ticks += 1
        if st.poll() and first_ms is None:
            torch.cuda.synchronize()
            first_tokens, first_ms = st.tokens, 1e3 * (time.perf_counter() - t0)

    for off in range(0, len(ids), PIECE):
        st.push(ids[off:off + PIECE])
        tick()
    st.close()
    while not st.finished:
        tick()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), st, first_tokens, first_ms, ticks


def whole_round(net, ids, k=0):
    """`infer_stream` on the whole text -> (total ms, ms at the first chunk, the stream)."""
    sid = sid_of(net, k)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    st = net.infer_stream(torch.tensor([ids]), torch.tensor([len(ids)]), sid=None if sid is None else torch.tensor([sid]),
                          seed=100 + k)
    next(st)
    torch.cuda.synchronize()
    first_ms = 1e3 * (time.perf_counter() - t0)
    st.run()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), first_ms, st


def pool_round(net, texts, tokens, pooled):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    sts = [open_text(net, k, tokens) for k in range(len(texts))]
    pool = net.stream_pool()
    if pooled:
        for st in sts:
            pool.add(st)
    for off in range(0, TOKENS, PIECE):
        for st, ids in zip(sts, texts):
            st.push(ids[off:off + PIECE])
        if pooled:
            pool.step()
        else:
            for st in sts:
                st.poll()
    for st in sts:
        st.close()
    while pooled and len(pool):
        pool.step()
    for st in sts:
        while not st.finished:
            st.poll()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def rel_rms(a, b):
    b = b.double()
    return float(torch.sqrt(torch.mean((a - b) ** 2)) / torch.sqrt(torch.mean(b ** 2)))


def counters(net):
    return dict(encoder_runs=net.encoder_runs(), text_runs=net.text_runs(), flow_runs=net.flow_runs(),
                decoder_runs=net.decoder_runs())


def measure(cfg, reps):
    med = statistics.median
    net = make_net(cfg)[0]
    ids = ids_of()
    live_round(net, ids, 4)                                        # warm-up: the arenas
    whole_round(net, ids)
    live, whole_text, ref, first, ref_first = [], [], [], [], []
    for r in range(reps):
        for v in ((0, 1, 2), (2, 1, 0), (1, 2, 0))[r % 3]:
            if v == 0:
                total, first_ms, _ = whole_round(net, ids)
                ref.append(total)
                ref_first.append(first_ms)
            elif v == 1:
                total, _, first_tokens, first_ms, _ = live_round(net, ids, 4)
                live.append(total)
                first.append(first_ms)
            else:
                whole_text.append(live_round(net, ids, None)[0])
    c0 = counters(net)
    _, st, first_tokens, _, ticks = live_round(net, ids, 4)
    c1 = counters(net)
    texts = [ids_of(k) for k in range(8)]
    pool_round(net, texts, 4, True)
    pooled, alone = [], []
    for r in range(reps):
        for v in ((0, 1) if r % 2 else (1, 0)):
            (pooled if v else alone).append(pool_round(net, texts, 4, bool(v)))
    base = live_round(net, ids, None)[1]
    deviation = []
    for A in (0, 4, 16, None):
        s = live_round(net, ids, A)[1]
        F = min(s.frames, base.frames)
        deviation.append(dict(tokens=A, frames=s.frames, durations_equal=s.durations == base.durations,
                              z_rel_rms=rel_rms(s.z[:, :, :F], base.z[:, :, :F]),
                              o_rel_rms=rel_rms(s.result()[:, :, :s.spf * F], base.result()[:, :, :s.spf * F])))
    return dict(config=cfg, tokens=TOKENS, piece_tokens=PIECE, block_tokens=16, ahead_tokens=4, reps=reps,
                frames=st.frames, audio_s_at_22050=round(st.frames * st.spf / 22050.0, 2),
                first_chunk=dict(tokens_pushed=first_tokens, ms=round(med(first), 3), infer_stream_tokens=TOKENS,
                                 infer_stream_ms=round(med(ref_first), 3)),
                total_ms=round(med(live), 3), whole_text_ms=round(med(whole_text), 3), infer_stream_ms=round(med(ref), 3),
                total_over_infer_stream=round(med(live) / med(ref), 3),
                reencoding_over_whole_text=round(med(live) / med(whole_text), 3),
                launches=dict(ticks=ticks, **{k: c1[k] - c0[k] for k in c0}),
                pool8_ms=round(med(pooled), 3), alone8_ms=round(med(alone), 3),
                pool8_over_alone8=round(med(pooled) / med(alone), 3), deviation=deviation, note=NOTE)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []
    for cfg in CONFIGS:
        lines.append(json.dumps(measure(cfg, args.reps)))
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
