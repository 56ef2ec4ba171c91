"""Cases, float64 references and bars of the resampler kernels (csrc/resample.hip), importable without a GPU.
test_resample_refs.py (CPU) proves the bars on the fp32 oracle and on mutated restatements and asserts the premises;
test_gpu_resample_pin.py (-m gpu) runs every case through `net.resample` / `net.resample_ranges` into the same checks.

Reference = `resample_ref.resample` (resampy's arithmetic in float64) from the fp32 inputs; `resample_at` evaluates it
at chosen outputs only.  `resample_compute(.., dtype, mut)` is that arithmetic restated dtype-generic: float64 without
`mut` it IS `resample_at`; in fp32 the weights are rounded as the bank's are and the sum runs in four fp32 partial
sums; `mut` names a deliberate mistake (MUTANTS) that the bars must catch.  The fp32 oracle is `apply_bank_at` in
fp32: the polyphase sum of the HOST bank (`mbv_resample_bank`, no GPU), four partial sums, each product and each sum
rounded (no FMA: a kernel that contracts rounds less).

Bars (small_op_cases.check_rounded, reused)
 * per element |y - y64| <= TOL u A + FLOOR, u = 2^-24, A = sum_k |bank[row][k]| |x[n - left + k]| in float64, with
   n = int(t / ratio) as the REFERENCE computes it in float64 and row = t M - n L (= L where the quotient rounds below
   the integer).  Nothing of A comes from the kernel's integer arithmetic;
 * per row: median and 99.9th percentile at most MARGIN = 4 x the oracle's, plus one fp32 ulp of the reference's RMS;
 * outputs in [int(n ratio), out_end) are +0.0 bitwise, out_samples is exact;
 * impulses (x = 1.0f at p, else 0) are bitwise the fp32 bank entry bank[row_t][p - int(t / ratio) + left], +0.0
   where the window does not hold p: one product plus zeros is exact.

TOL["resample"] = 4 x the worst err / (u A) of the fp32 oracle over the committed cases, rounded up to one digit (the
rule of small_op_cases.py).  Measured on the CPU (test_resample_refs.py prints it):

    kernel entry                 oracle worst err / (u A)   TOL    MI355X (profiles/resample_bars.json)
    resample (whole rows)              4.54                 20      5.24
    resample_ranges (live input)       4.93                 20      4.93
    resample_ranges, t M > 2^31        3.07                 20      2.54

(4 x 4.93 = 19.7: TOL 20.  The kernel's worst is above the oracle's on whole rows because its four FMA chains run in
another order than the oracle's rounded products; both are a quarter of the bar.)

Reaching from below.  At r = (t M) mod L = 0 the float64 quotient t / ratio can round below the integer n_t; resampy
then reads around n_t - 1 at fraction ~1 (bank row L).  When upsampling that is the same filter to rounding
(22050 -> 24000: the `never_below` mutant differs by < 1e-12, nothing can see it); when downsampling the truncated
index step makes it another filter.  The pairs of PAIRS with M = 147 that downsample take the branch on about 55 % of
their r = 0 outputs (first hits t = 240, 400, 480, 720 at 44100 -> 24000 and 22050 -> 12000; t = 120, 200, 240 at
44100 -> 12000); `premises` asserts, from the reference alone, that every such group has at least 8 hits and 8 plain
r = 0 outputs in its computed range and that `never_below` is off by more than 100 x the element bar on every hit of
the row `hits_loud` (measured: at least 870 x, 1.4e-3 to 4.8e-3 absolute).  That row exists because on plain noise the
mutant's error at a hit is a random sum: its median is about 400 bars, but one or two hits per row fall below 100 by
chance (measured minima 5 to 80), and on the DC row the two filters agree (below 3 bars).  `loud_signal` gives every
sample near a hit the sign of the difference of the two filters there.

Every mutant of MUTANTS is separated by committed cases; none had to be left out."""
import ctypes as C
import functools
import math
import zlib

import numpy as np
import torch

import resample_ref as RR
import small_op_cases as sc
from small_op_cases import MARGIN, U, Stats, check_exact, check_rounded   # noqa: F401  (re-exported to the tests)

TOL = sc.TOL                                    # check_rounded reads its bar there
TOL["resample"] = 20.0
MUTANTS = {"resample": ["never_below", "below_keeps_row0", "no_eta", "step_rounded", "accumulated_time", "edge_wrap",
                        "ratio_unscaled"]}
FILTERS = {"kaiser_best": 0, "kaiser_fast": 1}
HIT_PAIRS = [(44100, 24000), (22050, 12000), (44100, 12000), (22050, 24000)]     # reach from below (the first three: downsampling)
PAIRS = HIT_PAIRS + [(22050, 8000), (48000, 22050), (16000, 24000)]               # the long filter, live input, L = 3
N_IN = 3001
TILE = 256                                      # outputs per workgroup (kResampleTile)
F32, F64 = np.float32, np.float64


def rng(name):
    return np.random.RandomState(zlib.crc32(name.encode()))


# ---------------------------------------------------------------------------------------------- geometry
def geom(orig, target):
    g = math.gcd(orig, target)
    return target // g, orig // g, float(target) / orig          # L, M, ratio


@functools.lru_cache(maxsize=None)
def host_bank(orig, target, res_type):
    """(bank fp32 [L + 1, K], left) as the library's host code builds them (mbv_resample_bank)."""
    from mb_istft_vits_amd import _capi
    lib = _capi.lib()
    phases, taps, left = C.c_int32(), C.c_int32(), C.c_int32()
    rc = lib.mbv_resample_bank(orig, target, FILTERS[res_type], None, 0, C.byref(phases), C.byref(taps), C.byref(left))
    assert rc == 0, lib.mbv_last_error(None)
    b = np.zeros((phases.value + 1, taps.value), np.float32)
    rc = lib.mbv_resample_bank(orig, target, FILTERS[res_type], b.ctypes.data_as(C.c_void_p), b.size, None, None, None)
    assert rc == 0, lib.mbv_last_error(None)
    b.setflags(write=False)
    return b, left.value


def ref_index(ts, orig, target):
    """The reference's own n = int(t / ratio) in float64, and the bank row it implies: t M - n L (r, or L where the
    quotient rounded below the integer n_t)."""
    L, M, ratio = geom(orig, target)
    ts = np.asarray(ts, np.int64)
    n = (ts / ratio).astype(np.int64)
    row = ts * M - n * L
    assert bool(((row >= 0) & (row <= L)).all())
    return n, row


def r0_outputs(orig, target, t_end, t_first=1):
    """(from-below hits, plain r = 0 outputs) in [t_first, t_end)."""
    L, M, _ = geom(orig, target)
    ts = np.arange(t_first, t_end, dtype=np.int64)
    ts = ts[(ts * M) % L == 0]
    _, row = ref_index(ts, orig, target)
    return ts[row == L], ts[row == 0]


def n_computed(n_in, orig, target):
    return int(n_in * (float(target) / orig))                     # resampy: int(n_in * sample_ratio)


def ready_open(orig, target, res_type, in_avail):
    """Outputs of an open recording that are final with its first in_avail samples (mbv_resample_ready_open)."""
    L, M, _ = geom(orig, target)
    bank, left = host_bank(orig, target, res_type)
    a = in_avail - bank.shape[1] + left + 1
    return 0 if a <= 0 else (a * L + M - 1) // M


def raw_min(orig, target, res_type, out_end):
    """The fewest samples of an open recording that make out_end outputs final."""
    L, M, _ = geom(orig, target)
    r = max(0, out_end * M // L)
    while ready_open(orig, target, res_type, r) < out_end:
        r += 1
    while r > 0 and ready_open(orig, target, res_type, r - 1) >= out_end:
        r -= 1
    return r


# ---------------------------------------------------------------------------------------------- the arithmetic
def _gather(x, idx, first, n_in):
    """x holds the samples [first, first + len(x)) of a row of n_in samples: x[idx], zero outside [0, n_in)."""
    live = (idx >= 0) & (idx < n_in)
    j = np.where(live, idx - first, 0)
    if live.any():
        assert int(j[live].min()) >= 0 and int(j[live].max()) < len(x), "the slice does not hold a sample that is read"
    return np.where(live, x[j] if len(x) else 0, 0).astype(x.dtype)


def fir4(w, xs):
    """sum_k w[:, k] xs[:, k] in the dtype of w: four interleaved partial sums, (a0 + a1) + (a2 + a3)."""
    assert w.shape == xs.shape and w.shape[1] % 4 == 0 and w.dtype == xs.dtype
    acc = np.zeros((w.shape[0], 4), w.dtype)
    for k in range(0, w.shape[1], 4):
        acc += w[:, k:k + 4] * xs[:, k:k + 4]
    return (acc[:, 0] + acc[:, 1]) + (acc[:, 2] + acc[:, 3])


def apply_bank_at(x, ts, orig, target, res_type, dtype=F64, absolute=False, first=0, n_in=None):
    """resample_ref.apply_bank at the outputs ts, with the host bank and the row of `ref_index`; dtype fp32: the fp32
    oracle.  absolute: A = sum |bank| |x| in float64."""
    x = np.asarray(x)
    n_in = len(x) if n_in is None else n_in
    bank, left = host_bank(orig, target, res_type)
    n, row = ref_index(ts, orig, target)
    idx = n[:, None] - left + np.arange(bank.shape[1])[None, :]
    xs = _gather(x, idx, first, n_in).astype(dtype)
    w = bank[row].astype(dtype)
    if absolute:
        return (np.abs(w) * np.abs(xs)).sum(axis=1)
    return fir4(w, xs) if dtype == F32 else (w * xs).sum(axis=1)


def resample_compute(x, ts, orig, target, res_type, dtype=F64, mut=None, first=0, n_in=None):
    """resampy's loop (resample_ref.resample) at the outputs ts, dtype-generic.  x: samples [first, first + len(x)) of
    a row of n_in samples.  float64: the weights times the samples, summed; fp32: the weights rounded to fp32 first (as
    the bank's are), then `fir4`.  mut: one of MUTANTS."""
    x = np.asarray(x)
    n_in = len(x) if n_in is None else n_in
    ts = np.asarray(ts, np.int64)
    L, M, ratio = geom(orig, target)
    win, nb = RR.table(res_type)
    if ratio < 1 and mut != "ratio_unscaled":
        win = win * ratio
    delta = np.zeros_like(win)
    delta[:-1] = np.diff(win)
    scale = min(1.0, ratio)
    step = int(round(scale * nb)) if mut == "step_rounded" else int(scale * nb)
    nwin = len(win)
    if mut == "accumulated_time":                                 # resampy < 0.3: time += 1 / ratio, one add per output
        last = int(ts.max()) if ts.size else 0
        time = np.concatenate([[0.0], np.cumsum(np.full(last, 1.0 / ratio))])[ts]
    else:
        time = ts / ratio
    n = time.astype(np.int64)
    fr = time - n
    if mut == "never_below":                                      # the rational time t M / L
        n, fr = (ts * M) // L, ((ts * M) % L) / L
    elif mut == "below_keeps_row0":                               # around n_t - 1, but with the weights of fraction 0
        fr = np.where(((ts * M) % L == 0) & (n < (ts * M) // L), 0.0, fr)
    frac = scale * fr
    ws, srcs = [], []
    for side in (0, 1):
        f = frac if side == 0 else scale - frac
        idx = f * nb
        off = idx.astype(np.int64)
        eta = np.zeros_like(idx) if mut == "no_eta" else idx - off
        cnt = (nwin - off) // step
        if mut != "edge_wrap":
            cnt = np.minimum(n + 1, cnt) if side == 0 else np.minimum(n_in - n - 1, cnt)
        cnt = np.maximum(cnt, 0)
        taps = np.arange(int(cnt.max()) if cnt.size else 0)
        live = taps[None, :] < cnt[:, None]
        j = np.where(live, off[:, None] + taps[None, :] * step, 0)
        w = np.where(live, win[j] + eta[:, None] * delta[j], 0.0)
        src = n[:, None] - taps[None, :] if side == 0 else n[:, None] + 1 + taps[None, :]
        if mut == "edge_wrap":                                    # x[n - i] with a negative index: Python's wrap-around
            src = src % max(n_in, 1)
        src = np.where(live, src, -1)
        ws.append(w[:, ::-1] if side == 0 else w)
        srcs.append(src[:, ::-1] if side == 0 else src)
    pad = -(ws[0].shape[1] + ws[1].shape[1]) % 4
    w = np.concatenate(ws + [np.zeros((len(ts), pad))], axis=1)
    src = np.concatenate(srcs + [np.full((len(ts), pad), -1, np.int64)], axis=1)
    xs = _gather(x, src, first, n_in).astype(dtype)
    w = w.astype(dtype)
    return fir4(w, xs) if dtype == F32 else (w * xs).sum(axis=1)


def resample_at(x, ts, orig, target, res_type="kaiser_best", first=0, n_in=None):
    """`resample_ref.resample(row)[ts]` for ts below int(n_in ratio), without computing the row."""
    return resample_compute(np.asarray(x, F64), ts, orig, target, res_type, F64, None, first, n_in)


def check_at(what, got, x, ts, orig, target, res_type, first=0, n_in=None, **kw):
    """The bars on the fp32 outputs `got` at ts, from the fp32 samples x."""
    x = np.asarray(x, F32)
    ts = np.asarray(ts, np.int64)
    if not ts.size:
        return
    ref = resample_at(x, ts, orig, target, res_type, first, n_in)
    A = apply_bank_at(x, ts, orig, target, res_type, F64, True, first, n_in)
    orc = apply_bank_at(x, ts, orig, target, res_type, F32, False, first, n_in)
    tt = torch.from_numpy
    check_rounded("resample", what, tt(np.ascontiguousarray(got, F32)), tt(ref), tt(A), tt(orc), **kw)


# ---------------------------------------------------------------------------------------------- whole-row groups
def group(orig, target, res_type, n_in=N_IN, kinds=None):
    return dict(name="%d_%d_%s_n%d" % (orig, target, res_type, n_in), orig=orig, target=target, res_type=res_type,
                n_in=n_in, kinds=kinds)


GROUPS = [group(o, t, f) for o, t in PAIRS for f in FILTERS]
# 44100 -> 24000 with the from-below output t = 3840 as thread 0 of tile 15: the - 1 of resample_window_first is all
# that keeps its read inside the staged window
GROUPS.append(group(44100, 24000, "kaiser_best", n_in=7061, kinds=("unit", "hits_loud")))
GROUP_BY_NAME = {c["name"]: c for c in GROUPS}


def signal(name, kind, n):
    r = rng(name + "/" + kind)
    u = r.uniform(-1, 1, n)
    if kind == "quiet":
        return (1e-4 * u).astype(F32)
    if kind == "quiet_dc":
        return (0.5 + 1e-4 * u).astype(F32)
    return u.astype(F32)


def loud_signal(c, name):
    """Noise in [-1, 1] whose signs around every from-below hit follow the difference between what the hit reads (bank
    row L around n_t - 1) and what `never_below` reads (row 0 around n_t), each sample with its nearest hit: the
    mutant is then far outside the bar on EVERY hit, where plain noise leaves a few of them inside by chance."""
    o, t = c["orig"], c["target"]
    L, M, _ = geom(o, t)
    bank, left = host_bank(o, t, c["res_type"])
    K, n = bank.shape[1], c["n_in"]
    u = rng(name + "/hits_loud").uniform(-1, 1, n)
    nts = r0_outputs(o, t, n_computed(n, o, t))[0] * M // L
    d = np.zeros(K + 1)
    d[:K] += bank[L]
    d[1:] -= bank[0]
    j = np.arange(n)
    k = j - (nts[np.abs(nts[None, :] - j[:, None]).argmin(axis=1)] - 1 - left)
    dk = np.where((k >= 0) & (k <= K), d[np.clip(k, 0, K)], 0.0)
    return np.where(dk != 0, np.sign(dk) * (0.25 + 0.75 * np.abs(u)), u).astype(F32)


def last_hit(c):
    """(t, n_t) of the last from-below output whose row can end a few samples behind n_t inside n_in; None: no hit."""
    L, M, _ = geom(c["orig"], c["target"])
    hits, _ = r0_outputs(c["orig"], c["target"], n_computed(c["n_in"] - 8, c["orig"], c["target"]))
    return (int(hits[-1]), int(hits[-1]) * M // L) if len(hits) else None


@functools.lru_cache(maxsize=None)
def group_rows(name):
    """[(row name, signal kind, valid samples)]: three signals over the whole row (and `loud_signal` where the pair
    reaches from below while downsampling); rows that end one sample behind a
    from-below hit's n_t (the hit is then not computed when downsampling: zeros start at it) and at the first length
    that computes the hit (its right wing is cut by the end of the row); valid 0, 1, left, left + 1, K."""
    c = GROUP_BY_NAME[name]
    n = c["n_in"]
    if c["kinds"] is not None:
        return tuple((k, k, n) for k in c["kinds"])
    rows = [("unit", "unit", n), ("quiet", "quiet", n), ("quiet_dc", "quiet_dc", n)]
    if (c["orig"], c["target"]) in HIT_PAIRS and c["target"] < c["orig"]:
        rows.append(("hits_loud", "hits_loud", n))
    h = last_hit(c)
    if h is not None:
        t, nt = h
        v = nt + 1
        while n_computed(v, c["orig"], c["target"]) <= t:
            v += 1
        for k, vv in enumerate(sorted({nt + 1, v})):
            rows.append(("hit_edge%d" % k, "unit", vv))
    bank, left = host_bank(c["orig"], c["target"], c["res_type"])
    for v in (0, 1, left, left + 1, bank.shape[1]):
        rows.append(("valid%d" % v, "unit", v))
    assert all(0 <= v <= n for _, _, v in rows)
    return tuple(rows)


@functools.lru_cache(maxsize=None)
def group_inputs(name):
    """(x fp32 [B, n_in], valid int64 [B]); the samples behind a row's valid length are noise that must not be read."""
    c = GROUP_BY_NAME[name]
    rows = group_rows(name)
    x = np.stack([loud_signal(c, name) if kind == "hits_loud" else signal(name + "/" + rn, kind, c["n_in"])
                  for rn, kind, _ in rows])
    x.setflags(write=False)
    return x, np.array([v for _, _, v in rows], np.int64)


@functools.lru_cache(maxsize=None)
def group_expected(name):
    """Per row: dict(ref, A float64 [n_comp], orc fp32 [n_comp], n_comp, out_samples), computed once and shared."""
    c = GROUP_BY_NAME[name]
    o, t, f = c["orig"], c["target"], c["res_type"]
    x, valid = group_inputs(name)
    out = []
    for b, v in enumerate(valid):
        v = int(v)
        row = x[b, :v]
        nc = n_computed(v, o, t)
        ts = np.arange(nc, dtype=np.int64)
        ref = RR.resample(row.astype(F64), o, t, f)
        assert len(ref) == RR.out_len(v, o, t) and not ref[nc:].any()
        out.append(dict(ref=ref[:nc], n_comp=nc, out_samples=len(ref),
                        A=apply_bank_at(row, ts, o, t, f, F64, True) if nc else np.zeros(0),
                        orc=apply_bank_at(row, ts, o, t, f, F32) if nc else np.zeros(0, F32)))
    return out


def group_out_len(c):
    return RR.out_len(c["n_in"], c["orig"], c["target"])


def group_check(c, got, out_samples, rows=None, **kw):
    """got fp32 [B, out_len(n_in)], out_samples [B]: every row of the group (or those of `rows`) through the bars."""
    got = np.asarray(got)
    assert got.dtype == F32 and got.shape == (len(group_rows(c["name"])), group_out_len(c)), (got.dtype, got.shape)
    tt = torch.from_numpy
    for b, ((rn, _, v), e) in enumerate(zip(group_rows(c["name"]), group_expected(c["name"]))):
        if rows is not None and rn not in rows:
            continue
        what = "%s/%s" % (c["name"], rn)
        assert int(out_samples[b]) == e["out_samples"], (what, "out_samples", int(out_samples[b]), e["out_samples"])
        nc = e["n_comp"]
        check_exact(what + " zeros behind int(n ratio)", tt(got[b, nc:].copy()), torch.zeros(got.shape[1] - nc))
        if nc:
            check_rounded("resample", what, tt(got[b, :nc].copy()), tt(e["ref"]), tt(e["A"]), tt(e["orc"]), **kw)


def group_run(c, fn):
    """The fp32 rows `fn(row fp32 [v], ts) -> fp32 [len(ts)]` gives, laid out as the kernel's output."""
    x, valid = group_inputs(c["name"])
    out = np.zeros((len(valid), group_out_len(c)), F32)
    for b, v in enumerate(valid):
        nc = n_computed(int(v), c["orig"], c["target"])
        if nc:
            out[b, :nc] = fn(x[b, :int(v)], np.arange(nc, dtype=np.int64))
    return out, [RR.out_len(int(v), c["orig"], c["target"]) for v in valid]


def premises(c):
    """What the reference alone must show for a group of HIT_PAIRS -> (hits, plain r = 0 outputs, the smallest
    |never_below - ref| / (TOL u A) over the hits of the row built for it, the largest |never_below - ref| there)."""
    o, t, f = c["orig"], c["target"], c["res_type"]
    x, valid = group_inputs(c["name"])
    names = [rn for rn, _, _ in group_rows(c["name"])]
    b = names.index("hits_loud") if t < o else names.index("unit")
    e = group_expected(c["name"])[b]
    assert int(valid[b]) == c["n_in"]
    hits, plain = r0_outputs(o, t, e["n_comp"])
    assert len(hits) >= 8, (c["name"], "from-below outputs in the computed range", len(hits))
    assert len(plain) >= 8, (c["name"], "plain r = 0 outputs in the computed range", len(plain))
    mut = resample_compute(x[b].astype(F64), hits, o, t, f, F64, "never_below")
    size = np.abs(mut - e["ref"][hits]) / (TOL["resample"] * U * e["A"][hits])
    if t < o:
        assert float(size.min()) > 100, (c["name"], "never_below against the element bar on every hit", size.tolist())
    return hits, plain, float(size.min()), float(np.abs(mut - e["ref"][hits]).max())


# ---------------------------------------------------------------------------------------------- impulses
IMPULSE_GROUPS = [(44100, 24000, "kaiser_best"), (22050, 12000, "kaiser_fast"), (44100, 12000, "kaiser_best"),
                  (22050, 24000, "kaiser_fast"), (16000, 24000, "kaiser_best")]


def impulse_positions(orig, target, n_in=N_IN):
    """p: n_t of a from-below output (or of a plain r = 0 output where the pair has no hit), n_t of a plain r = 0
    output, the input index under the tile edge t = 255 / 256, 0 and n - 1."""
    L, M, _ = geom(orig, target)
    hits, plain = r0_outputs(orig, target, n_computed(n_in, orig, target))
    a = int(hits[2] if len(hits) > 2 else plain[5]) * M // L
    return [a, int(plain[3]) * M // L, 256 * M // L, 0, n_in - 1]


def impulse_expected(p, n_in, orig, target, res_type):
    """fp32 [out_len(n_in)]: bank[row_t][p - int(t / ratio) + left] for t < int(n_in ratio), +0.0 elsewhere."""
    bank, left = host_bank(orig, target, res_type)
    out = np.zeros(RR.out_len(n_in, orig, target), F32)
    nc = n_computed(n_in, orig, target)
    n, row = ref_index(np.arange(nc), orig, target)
    k = p - n + left
    seen = (k >= 0) & (k < bank.shape[1])
    out[:nc][seen] = bank[row[seen], k[seen]]
    return out + F32(0.0)                                         # (a -0.0 of the bank plus the zeros of the sum is +0.0)


# ---------------------------------------------------------------------------------------------- live input (ranges)
RANGE_GROUPS = [(44100, 24000, "kaiser_best"), (22050, 12000, "kaiser_fast")]
RANGE_DTYPES = ("f32", "pcm16", "ulaw", "alaw")
RANGE_OPEN_COUNT = 300                           # an open row's range: one whole tile and a part of the next


def range_raw(orig, target, res_type, dtype, n_in=N_IN):
    """(raw recording as the caller holds it, the fp32 values it decodes to)."""
    import g711_ref
    x = signal("ranges_%d_%d_%s" % (orig, target, res_type), "unit", n_in)
    if dtype == "f32":
        return x, x
    pcm = (x * 32767).astype(np.int16)
    if dtype == "pcm16":
        return pcm, (pcm.astype(F32) / F32(32768)).astype(F32)
    raw = g711_ref.encode(pcm, dtype)
    return raw, (g711_ref.decode(raw, dtype).astype(F32) / F32(32768)).astype(F32)


def range_rows(orig, target, res_type, n_in=N_IN):
    """[(dtype, out_first, out_count, closed, in_avail)]: every dtype, from the from-below output 240 (thread 0 of its
    tile) and from 241, open at the tightest frontier and closed to the end of the row."""
    hits, _ = r0_outputs(orig, target, 300)
    assert 240 in hits.tolist()
    total = RR.out_len(n_in, orig, target)
    rows = []
    for dt in RANGE_DTYPES:
        for first in (240, 241):
            rows.append((dt, first, RANGE_OPEN_COUNT, False, raw_min(orig, target, res_type, first + RANGE_OPEN_COUNT)))
            rows.append((dt, first, total - first, True, n_in))
    assert all(a < n_in for _, _, _, closed, a in rows if not closed)
    return rows


# ---------------------------------------------------------------------------------------------- a long row: t M > 2^31
LONG = dict(orig=44100, target=24000, res_type="kaiser_best")
LONG["t_first"] = int(r0_outputs(44100, 24000, 2 ** 31 // 147 + 2001, 2 ** 31 // 147 + 1)[0][0])   # from below, t M > 2^31
LONG["tiles"] = 3
LONG["n_in"] = (LONG["t_first"] + LONG["tiles"] * TILE) * 147 // 80 + 2000


def long_window():
    """(first, count) of the input samples the three tiles read, with a margin."""
    bank, left = host_bank(LONG["orig"], LONG["target"], LONG["res_type"])
    lo = LONG["t_first"] * 147 // 80 - left - 8
    hi = (LONG["t_first"] + LONG["tiles"] * TILE) * 147 // 80 + bank.shape[1] + 8
    return lo, hi - lo
