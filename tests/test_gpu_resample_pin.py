"""-m gpu: the resampler kernels (csrc/resample.hip) pinned to float64 at the cases of tests/resample_cases.py, the
rate pairs that reach from below while downsampling included (44100 -> 24000, 22050 -> 12000, 44100 -> 12000: bank
row L read around n_t - 1, which no other test executes where it changes anything).

  a. `net.resample` (resample_kernel): every group through the element and quantile bars, impulses bitwise the fp32
     bank entry, and a row long enough that the from-below output t = 3840 is thread 0 of its tile;
  b. `net.resample_ranges` (resample_ranges_kernel): fp32, int16, mu-law and A-law recordings, open and closed, from
     the from-below output 240 and from 241, against the reference of the DECODED values; sentinel elsewhere;
  c. `net.resample_pcm16_range`, `net.resample_pcm16_chunks`, `net.resample_turns` at those pairs: int16 bitwise
     `net.to_pcm16(net.resample(..))`, cut at frontiers around a from-below output, G.711 and an envelope;
  d. 44100 -> 24000 behind t M = 2^31: three tiles of a 27 M-sample row through (b), one through the ranged int16
     entry, against `resample_at` on the slice they read.

MBV_RESAMPLE_REPORT=<file>: the worst err / (u A) and the largest share of the quantile bars per kernel entry, as JSON
(profiles/resample_bars.json is such a run)."""
import json
import os

import numpy as np
import pytest
import torch

import g711_ref
import gain_ref
import resample_cases as rc
import resample_ref as RR

pytestmark = pytest.mark.gpu
STATS = {k: rc.Stats() for k in ("resample", "resample_ranges", "resample_ranges_long")}
CANARY = 7.5e8
SENTINEL = {"pcm16": -12345, "ulaw": 0x5A}
WIRE_GROUPS = [(44100, 24000, "kaiser_best"), (22050, 12000, "kaiser_fast"), (44100, 12000, "kaiser_best")]


@pytest.fixture(scope="module")
def net():
    from gpu_util import make_net
    n = make_net("ljs_mini_mb_istft_vits")[0]
    yield n
    rows = {k: dict(v, headroom=v["TOL"] / v["err_over_uA"] if v["err_over_uA"] else None)
            for k, s in STATS.items() for v in s.values()}
    print("\nworst err / (u A) per kernel entry: " + ", ".join("%s %.3g (TOL %g)" % (k, v["err_over_uA"], v["TOL"])
                                                                for k, v in rows.items()))
    path = os.environ.get("MBV_RESAMPLE_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump({"entries": rows}, f, indent=1)


# ------------------------------------------------------------------------------------------------ a. whole rows
@pytest.mark.parametrize("c", rc.GROUPS, ids=lambda c: c["name"])
def test_whole_rows_inside_the_bars(net, c):
    x, valid = rc.group_inputs(c["name"])
    out, ns = net.resample(torch.from_numpy(x.copy()).cuda()[:, None, :], c["orig"], c["target"],
                           valid_samples=torch.from_numpy(valid).cuda(), res_type=c["res_type"])
    assert out.dtype == torch.float32 and out.shape == (len(valid), 1, rc.group_out_len(c))
    rc.group_check(c, out[:, 0].cpu().numpy(), ns.cpu().numpy(), stats=STATS["resample"])


@pytest.mark.parametrize("orig,target,res_type", rc.IMPULSE_GROUPS)
def test_impulses_are_the_bank_entries_bitwise(net, orig, target, res_type):
    ps = rc.impulse_positions(orig, target)
    x = np.zeros((len(ps), 1, rc.N_IN), np.float32)
    for b, p in enumerate(ps):
        x[b, 0, p] = 1.0
    out, _ = net.resample(torch.from_numpy(x).cuda(), orig, target, res_type=res_type)
    out = out[:, 0].cpu()
    for b, p in enumerate(ps):
        want = rc.impulse_expected(p, rc.N_IN, orig, target, res_type)
        rc.check_exact("%d_%d_%s impulse at %d" % (orig, target, res_type, p), out[b], torch.from_numpy(want))


# ------------------------------------------------------------------------------------------------ b. live input
_WAVE_DTYPE = {"f32": 0, "pcm16": 1, "ulaw": 8, "alaw": 9}                # MBV_WAVE_*
_UNARRIVED = {"f32": float("nan"), "pcm16": -32768, "ulaw": 0x80, "alaw": 0x2A}   # loud, and a NaN meets no weight unharmed


def _range(buf, dtype, in_avail, in_total, first, count, out):
    from mb_istft_vits_amd import _capi
    r = _capi.MbvResampleRange()
    r.wave, r.wave_dtype = buf.data_ptr(), _WAVE_DTYPE[dtype]
    r.in_avail, r.in_total, r.out_first, r.out_count = in_avail, in_total, first, count
    r.out, r.out_capacity = out.data_ptr(), out.numel()
    return r


@pytest.mark.parametrize("orig,target,res_type", rc.RANGE_GROUPS)
def test_ranges_of_every_input_type_inside_the_bars(net, orig, target, res_type):
    from mb_istft_vits_amd import wire
    rows = rc.range_rows(orig, target, res_type)
    n = rc.N_IN
    total = RR.out_len(n, orig, target)
    nc = rc.n_computed(n, orig, target)
    bufs, outs, table, decoded = [], [], [], {}
    for dt, first, count, closed, avail in rows:
        raw, decoded[dt] = rc.range_raw(orig, target, res_type, dt)
        if not closed:
            assert wire.resample_ready_open(orig, target, avail, res_type) == first + count
            assert wire.resample_ready_open(orig, target, avail - 1, res_type) < first + count
        buf = torch.from_numpy(raw.copy()).cuda()
        buf[avail:] = _UNARRIVED[dt]
        out = torch.full((total + 64,), CANARY, device="cuda")
        bufs.append(buf)
        outs.append(out)
        table.append(_range(buf, dt, avail, n if closed else -1, first, count, out))
    runs = net.input_runs()
    net.resample_ranges(table, orig, target, res_type=res_type)
    assert net.input_runs() - runs == 1
    whole = {dt: net.resample(torch.from_numpy(x.copy()).cuda()[None, None], orig, target, res_type=res_type)[0][0, 0]
             for dt, x in decoded.items()}
    for (dt, first, count, closed, avail), out in zip(rows, outs):
        what = "%d_%d_%s/%s_%d_%s" % (orig, target, res_type, dt, first, "closed" if closed else "open")
        assert bool((out[:first] == CANARY).all()) and bool((out[first + count:] == CANARY).all()), what
        end = min(first + count, nc)
        assert torch.equal(out[first:first + count], whole[dt][first:first + count]), what    # bitwise the one-shot kernel
        got = out[first:first + count].cpu().numpy()
        rc.check_at(what, got[:end - first], decoded[dt], np.arange(first, end), orig, target, res_type, n_in=n,
                    stats=STATS["resample_ranges"])
        if closed:
            assert first + count == total
            rc.check_exact(what + " zeros behind int(n ratio)", torch.from_numpy(got[end - first:].copy()),
                           torch.zeros(total - end))


# ------------------------------------------------------------------------------------------------ c. the wire entries
def _timeline(orig, target, res_type, n=rc.N_IN, cut=1000, pause=37):
    """fp32 [n] up to 1.2 (the clip works) with a pause of zeros inside: one row, and the timeline of two segments."""
    x = (1.2 * rc.signal("wire_%d_%d_%s" % (orig, target, res_type), "unit", n)).astype(np.float32)
    x[cut:cut + pause] = 0
    return x, [(0, cut), (cut + pause, n - cut - pause)]


def _frontiers(orig, target, res_type, n):
    """Frontiers at which a from-below output is the first one NOT ready, and the last one ready; then the whole row."""
    from mb_istft_vits_amd import wire
    hit = int(rc.r0_outputs(orig, target, rc.n_computed(n, orig, target))[0][4])
    fr = []
    for want in (hit, hit + 1):
        f = rc.raw_min(orig, target, res_type, want)
        assert wire.resample_ready(orig, target, f, n, res_type) == want, (f, want)
        fr.append(f)
    assert fr[0] < fr[1] < n
    return fr + [n], hit


def _poisoned(x, f):
    xx = x.clone()
    xx[..., f:] = float("nan")
    return xx


@pytest.mark.parametrize("orig,target,res_type", WIRE_GROUPS)
def test_wire_entries_are_bitwise_the_one_shot_chain(net, orig, target, res_type):
    from mb_istft_vits_amd import _capi, wire
    x_np, seg_spans = _timeline(orig, target, res_type)
    n = len(x_np)
    x = torch.from_numpy(x_np).cuda().view(1, 1, n)
    out, ns = net.resample(x, orig, target, res_type=res_type)
    ref = net.to_pcm16(out, auto_normalize=False, valid_samples=ns)
    width = ref.shape[1]
    assert width == wire.resample_ready(orig, target, n, n, res_type) == int(ns[0])
    frontiers, hit = _frontiers(orig, target, res_type, n)
    ready = [wire.resample_ready(orig, target, f, n, res_type) for f in frontiers]
    assert ready == [hit, hit + 1, width]
    spans = list(zip([0] + ready[:-1], ready))
    assert int((ref.abs() == 32767).sum()) > 0 and ref[0, hit] != 0           # the clip works; the hit is a live sample
    ulaw = torch.from_numpy(g711_ref.encode(ref.cpu().numpy(), "ulaw")).cuda()

    # the ranged entry, int16 and mu-law
    for enc, want in (("pcm16", ref), ("ulaw", ulaw)):
        pcm = torch.full_like(want, SENTINEL[enc])
        for f, (a, b) in zip(frontiers, spans):
            net.resample_pcm16_range(_poisoned(x, f), orig, target, f, a, b - a, pcm, res_type=res_type, encoding=enc)
            assert bool((pcm[:, b:] == SENTINEL[enc]).all())
        assert torch.equal(pcm, want), (enc, int((pcm != want).sum()))

    # the pooled entry: the three steps as three chunks of ONE launch, each from its own poisoned copy
    valid = torch.tensor([n], device="cuda", dtype=torch.int64)
    running = torch.zeros(3, device="cuda")
    pcm = torch.full_like(ref, SENTINEL["pcm16"])
    keep, chunks = [], []
    for i, (f, (a, b)) in enumerate(zip(frontiers, spans)):
        xx = _poisoned(x, f)
        keep.append(xx)
        k = _capi.MbvPcmChunk()
        k.wave, k.in_total, k.valid_samples = xx.data_ptr(), n, valid.data_ptr()
        k.in_avail, k.out_first, k.out_count = f, a, b - a
        k.peak, k.pcm, k.pcm_capacity = None, pcm.data_ptr(), width
        k.running_peak, k.out_samples = running[i:].data_ptr(), None
        chunks.append(k)
    packed = torch.full((width + 8,), SENTINEL["pcm16"], device="cuda", dtype=torch.int16)
    runs = wire.wire_runs(net)
    net.resample_pcm16_chunks(chunks, orig, target, packed=packed, res_type=res_type)
    assert wire.wire_runs(net) - runs == 1
    assert torch.equal(pcm, ref) and torch.equal(packed[:width], ref[0]) and bool((packed[width:] == SENTINEL["pcm16"]).all())
    assert float(running.max()) == float(out.abs().max())

    # a turn: the same row as the timeline of two segments around the pause
    pcm = torch.full_like(ref, SENTINEL["pcm16"])
    turns = []
    for i, (f, (a, b)) in enumerate(zip(frontiers, spans)):
        xx = keep[i]
        k = _capi.MbvTurnChunk()
        c = k.chunk
        c.wave, c.valid_samples, c.in_total, c.in_avail = None, None, n, f
        c.out_first, c.out_count, c.peak = a, b - a, None
        c.pcm, c.pcm_capacity, c.running_peak, c.out_samples = pcm.data_ptr(), width, running[i:].data_ptr(), None
        segs = (_capi.MbvTurnSeg * len(seg_spans))()
        for sg, (s0, ln) in zip(segs, seg_spans):
            w = xx[0, 0, s0:s0 + ln].clone()
            keep.append(w)
            sg.wave, sg.start, sg.length, sg.ramp = w.data_ptr(), s0, ln, 0
        k.segs, k.n_segs = segs, len(seg_spans)
        keep.append(segs)
        turns.append(k)
    net.resample_turns(turns, orig, target, res_type=res_type)
    assert torch.equal(pcm, ref), int((pcm != ref).sum())

    # an envelope: bitwise the entry on the pre-multiplied row, and the one-shot chain of that row
    hop = 256
    G = (0.5 + rc.rng("envelope").uniform(0, 1, -(-n // hop) + 1)).astype(np.float32)
    shaped = torch.from_numpy(gain_ref.shaped(x_np, G, hop)).cuda().view(1, 1, n)
    o2, n2 = net.resample(shaped, orig, target, res_type=res_type)
    want = net.to_pcm16(o2, auto_normalize=False, valid_samples=n2)
    assert not torch.equal(want, ref)
    env = wire.Envelope(torch.from_numpy(G).cuda(), hop)
    got, plain = torch.full_like(ref, SENTINEL["pcm16"]), torch.full_like(ref, SENTINEL["pcm16"])
    for f, (a, b) in zip(frontiers, spans):
        net.resample_pcm16_range(_poisoned(x, f), orig, target, f, a, b - a, got, res_type=res_type, envelope=env)
        net.resample_pcm16_range(_poisoned(shaped, f), orig, target, f, a, b - a, plain, res_type=res_type)
    assert torch.equal(got, plain) and torch.equal(got, want)


# ------------------------------------------------------------------------------------------------ d. t M > 2^31
def test_a_long_row_behind_two_to_the_31(net):
    """44100 -> 24000 at t = 14.6e6: t M no longer fits 32 bits and t / ratio needs float64.  Three tiles through the
    live-input kernel, the first of them through the ranged int16 entry; the reference reads the slice of x they touch."""
    from mb_istft_vits_amd import wire
    o, t, f = rc.LONG["orig"], rc.LONG["target"], rc.LONG["res_type"]
    n, t0, cnt = rc.LONG["n_in"], rc.LONG["t_first"], rc.LONG["tiles"] * rc.TILE
    assert t0 * 147 > 2 ** 31 and wire.resample_ready_open(o, t, n, f) >= t0 + cnt
    g = torch.Generator(device="cuda").manual_seed(31)
    x = torch.empty(n, device="cuda").uniform_(-1, 1, generator=g)
    first, count = rc.long_window()
    xs = x[first:first + count].cpu().numpy()
    out = torch.full((t0 + cnt + 8,), CANARY, device="cuda")
    net.resample_ranges([_range(x, "f32", n, -1, t0, cnt, out)], o, t, res_type=f)
    assert bool((out[t0 - 4096:t0] == CANARY).all()) and bool((out[t0 + cnt:] == CANARY).all())
    got = out[t0:t0 + cnt]
    ts = t0 + np.arange(cnt)
    rc.check_at("long", got.cpu().numpy(), xs, ts, o, t, f, first=first, n_in=n, stats=STATS["resample_ranges_long"])
    pcm = torch.full((1, t0 + rc.TILE + 8), SENTINEL["pcm16"], device="cuda", dtype=torch.int16)
    net.resample_pcm16_range(x.view(1, 1, n), o, t, n, t0, rc.TILE, pcm, res_type=f)
    want = (got[:rc.TILE].clamp(-1, 1) * 32767).to(torch.int32).to(torch.int16)
    assert torch.equal(pcm[0, t0:t0 + rc.TILE], want)
    assert bool((pcm[0, t0 - 4096:t0] == SENTINEL["pcm16"]).all()) and bool((pcm[0, t0 + rc.TILE:] == SENTINEL["pcm16"]).all())
