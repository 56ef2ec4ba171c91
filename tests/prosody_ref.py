"""Float64 / NumPy restatement of the per-token prosody kernel (csrc/ops.hip, shape_durations_kernel), its cases and
its tie rule, importable without a GPU.  test_prosody.py (CPU) proves the restatement's own properties and that the
committed cases stay inside the tie budget; test_gpu_prosody.py (-m gpu) runs the kernel against it.

The kernel:   w_t = ceilf(expf(logw_t) * fl32(s_t * f)) + extra_t     for t < len, 0 behind it
              D(f) = sum_t min(ceil part, 2^20) + extra_t              (64-bit)
              f*   = the largest fp32 f in [lo, hi] with D(f) <= N      (f = lo, status 1, if even D(lo) > N)
Here every product and the exponential are float64 on the fp32 inputs; `s_t * f` is rounded to fp32 first, as the
kernel rounds it (that rounding is part of the definition of the table the row is scaled by, not an error of it).

Tie rule (the one of small_op_cases.py for the durations): a token is left out of the exact comparison only if its
float64 duration lies within 8 fp32 ulps of an integer (expf is good to 1-2 ulp and the product rounds once more),
unless it is an exact integer by construction (logw == 0 and an integer scale: every fp32 path gives it exactly).
A case may leave out at most 1 % of its tokens."""
import zlib

import numpy as np

MAX_TOKEN_FRAMES, MAX_TOTAL_FRAMES = 2 ** 20, 2 ** 30
TIE_ULPS = 8
MAX_LEFT_OUT = 0.01
FIT_BAR = 8 * 2.0 ** -24      # |f* - f64*| / f*: expf 1-2 ulp, two roundings and the factor's half ulp, doubled


def gen(name):
    return np.random.RandomState(zlib.crc32(name.encode()))


def f32(x):
    return np.asarray(x, np.float32)


def scaled(scale, f=None):
    """The table a row is scaled by: s_t, or fl32(s_t * f) with a factor -- as float64 values."""
    s = f32(scale)
    if f is not None:
        s = s * np.float32(f)                                   # one fp32 multiplication
    return s.astype(np.float64)


def real_durations(logw, scale, f=None):
    """exp(logw_t) * fl32(s_t * f) in float64 (before the ceil)."""
    with np.errstate(over="ignore", invalid="ignore"):
        d = np.exp(f32(logw).astype(np.float64)) * scaled(scale, f)
    return np.where(d < 2.0 ** -150, 0.0, d)                    # below half the smallest fp32 denormal: 0 in fp32


def total(logw, scale, extra, f=None):
    """D(f) of ONE row (1-D arrays holding the tokens below the row's length): Python int."""
    with np.errstate(invalid="ignore"):
        c = np.ceil(real_durations(logw, scale, f))
    c = np.where(c < MAX_TOKEN_FRAMES, np.maximum(c, 0), MAX_TOKEN_FRAMES)      # (NaN: 2^20, as the kernel counts it)
    e = 0 if extra is None else int(np.maximum(np.asarray(extra, np.int64), 0).sum())
    return int(c.astype(np.int64).sum()) + e


def bits(x):
    return int(np.float32(x).view(np.uint32))


def from_bits(u):
    return np.uint32(u).view(np.float32)


def fit(logw, scale, extra, frames, lo, hi, D=None):
    """(f*, status, evaluations): the bisection on the bit pattern, on D (default: `total` in float64)."""
    if D is None:
        D = lambda f: total(logw, scale, extra, f)
    lo, hi = np.float32(lo), np.float32(hi)
    n = 1
    if D(hi) <= frames:
        return hi, 0, n
    a, z = bits(lo) - 1, bits(hi)                               # a fits (below bits(lo): by decree), z does not
    while z - a > 1:
        mid = a + (z - a) // 2
        n += 1
        if D(from_bits(mid)) <= frames:
            a = mid
        else:
            z = mid
    return (lo, 1, n) if a < bits(lo) else (from_bits(a), 0, n)


def shape(logw, lens, scale, extra=None, f=None, bad=None):
    """The final pass for a batch [B, T] in float64 -> dict: dur (real durations, 0 behind the length), w_ceil (float64
    totals), cum (int64; of flagged rows unspecified), ylen32, ylen64, over (the rows the range rules flag)."""
    logw = f32(logw)
    B, T = logw.shape
    m = np.arange(T)[None, :] < np.asarray(lens)[:, None]
    s = np.broadcast_to(f32(scale), (B, T))
    fb = None if f is None else np.broadcast_to(f32(f).reshape(-1, 1), (B, T))
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.exp(logw.astype(np.float64)) * (s.astype(np.float64) if fb is None else (s * fb).astype(np.float64))
        d = np.where(d < 2.0 ** -150, 0.0, d)
        c = np.ceil(d)
    x = np.zeros((B, T), np.int64) if extra is None else np.asarray(extra, np.int64)
    w = np.where(m, c + x, 0.0)
    with np.errstate(invalid="ignore"):
        ok = (s >= 0) & np.isfinite(s) & (x >= 0) & (c < MAX_TOKEN_FRAMES) & (w < MAX_TOKEN_FRAMES)
    flagged = m & ~ok
    cum = np.cumsum(np.where(m & ok, w, 0.0).astype(np.int64), axis=1)
    over = flagged.any(1) | (cum[:, -1] > MAX_TOTAL_FRAMES)
    tot = np.where(over, 1, np.maximum(cum[:, -1], 1))
    isbad = np.zeros(B, bool) if bad is None else np.asarray(bad) != 0
    return dict(dur=np.where(m, d, 0.0), ceil=np.where(m, c, 0.0), w_ceil=w, cum=cum, ylen32=tot.astype(np.int32),
                ylen64=np.where(isbad | over, -1, tot).astype(np.int64), over=over, mask=m, flagged=flagged)


def near_ties(logw, lens, scale, f=None):
    """Tokens the tie rule leaves out: float64 duration within TIE_ULPS fp32 ulps of an integer, and not an exact
    integer by construction (logw == 0: the duration is the fp32 table entry itself)."""
    r = shape(logw, lens, scale, None, f)
    d = r["dur"]
    with np.errstate(invalid="ignore"):
        band = TIE_ULPS * np.spacing(np.abs(d).astype(np.float32)).astype(np.float64)
        near = r["mask"] & np.isfinite(d) & (d > 0) & (d < MAX_TOKEN_FRAMES) & (np.abs(d - np.round(d)) <= band)
    return near & ~(f32(logw) == 0)


# ------------------------------------------------------------------------------------------------ the op's cases
SCALE_SET = np.asarray([0.0, 0.5, 1.0, 1.75, 3.0], np.float32)


def op_case(name, B, T, lens, plant=(), extras=True, bad=()):
    return dict(name=name, B=B, T=T, lens=lens, plant=plant, extras=extras, bad=bad)


# plant: "ints" (logw = 0 on every third token: the duration is s_t itself), "zero_start" / "zero_mid" / "zero_all"
# (s_t = 0 on row 0 / the last row / row 0), "edge" (row 1: a token of exactly 2^20 frames -- flagged; row 2: one of
# 2^20 - 1 -- in range), "edge_extra" (row 1: 2^20 - 1 frames plus one extra -- flagged)
OP_CASES = [
    op_case("shape_t1", 3, 1, [1, 1, 0], plant=("ints",)),
    op_case("shape_t20", 3, 20, [20, 1, 13], plant=("ints", "zero_start"), bad=(1,)),
    op_case("shape_t256", 3, 256, [256, 1, 200], plant=("ints", "zero_mid")),
    op_case("shape_t257", 3, 257, [257, 1, 256], plant=("ints", "zero_all")),
    op_case("shape_t300", 3, 300, [300, 1, 277], plant=("zero_start", "zero_mid"), extras=False),
    op_case("shape_t257_edge", 3, 257, [257, 257, 257], plant=("ints", "edge")),
    op_case("shape_t300_edge_extra", 3, 300, [300, 300, 1], plant=("edge_extra",)),
    op_case("shape_t2304", 2, 2304, [2304, 2100], plant=("ints", "zero_mid")),       # past the kernel's register tiles
]
OP_BY_NAME = {c["name"]: c for c in OP_CASES}


def op_inputs(c):
    rs = gen(c["name"])
    B, T = c["B"], c["T"]
    logw = np.minimum(1.2 * rs.standard_normal((B, T)), 6.0).astype(np.float32)
    pick = rs.randint(0, len(SCALE_SET), size=(B, T))
    scale = np.where(rs.uniform(size=(B, T)) < 0.5, SCALE_SET[pick], rs.uniform(0.25, 3.0, size=(B, T))).astype(np.float32)
    extra = (rs.randint(0, 40, size=(B, T)) * (rs.uniform(size=(B, T)) < 0.2)).astype(np.int32) if c["extras"] else None
    t = np.arange(T)
    if "ints" in c["plant"]:
        logw[:, t % 3 == 0] = 0.0
    if "zero_start" in c["plant"]:
        scale[0, : max(1, T // 4)] = 0.0
    if "zero_mid" in c["plant"]:
        scale[-1, T // 3: max(T // 3 + 1, 2 * T // 3)] = 0.0
    if "zero_all" in c["plant"]:
        scale[0, :] = 0.0
    if "edge" in c["plant"]:
        logw[1, T // 2], scale[1, T // 2] = 0.0, 2.0 ** 20
        logw[2, T // 2], scale[2, T // 2] = 0.0, 2.0 ** 20 - 1
        if extra is not None:
            extra[1, T // 2] = extra[2, T // 2] = 0
    if "edge_extra" in c["plant"]:
        logw[1, 5], scale[1, 5] = 0.0, 2.0 ** 20 - 1
        extra[1, 5] = 1
    bad = np.asarray([1 if b in c["bad"] else 0 for b in range(B)], np.int32)
    return dict(logw=logw, lens=np.asarray(c["lens"], np.int32), scale=scale, extra=extra, bad=bad)


def op_check(c, inp, got):
    """got: w_ceil [B, T] fp32, cum [B, T] int32, ylen32, ylen64 of the kernel.  Exact but for the tokens of the tie
    rule, which may be either neighbour; the rest of such a row is compared from the sums shifted by what was seen.
    Returns the number of tokens left out."""
    ref = shape(inp["logw"], inp["lens"], inp["scale"], inp["extra"], bad=inp["bad"])
    near = near_ties(inp["logw"], inp["lens"], inp["scale"])
    n_tokens = int(ref["mask"].sum())
    assert int(near.sum()) <= MAX_LEFT_OUT * n_tokens, (c["name"], "tokens left out", int(near.sum()), n_tokens)
    g = np.asarray(got["w_ceil"], np.float64)
    x = np.zeros_like(g) if inp["extra"] is None else inp["extra"].astype(np.float64)
    lo = np.round(ref["dur"]) + x
    assert np.all((g == lo) | (g == lo + 1) | ~near), (c["name"], "a left-out token is neither neighbour")
    huge = ref["flagged"]                                        # a flagged token: w_ceil as it comes, at or past the range
    assert np.all(g[huge] >= MAX_TOKEN_FRAMES), (c["name"], "a token at or beyond 2^20 frames came out below")
    want = np.where(near | huge, g, ref["w_ceil"])
    assert np.array_equal(g, want), (c["name"], "w_ceil", np.argwhere(g != want)[:5])
    cum = np.cumsum(np.where(ref["mask"] & ~huge, want, 0.0).astype(np.int64), axis=1)
    over = huge.any(1) | (cum[:, -1] > MAX_TOTAL_FRAMES)
    assert np.array_equal(over, ref["over"]), (c["name"], "flagged rows")
    keep = ~over
    assert np.array_equal(np.asarray(got["cum"], np.int64)[keep], cum[keep]), (c["name"], "cum")
    tot = np.where(over, 1, np.maximum(cum[:, -1], 1))
    assert np.array_equal(np.asarray(got["ylen32"], np.int64), tot), (c["name"], "ylen32")
    y64 = np.where((inp["bad"] != 0) | over, -1, tot)
    assert np.array_equal(np.asarray(got["ylen64"], np.int64), y64), (c["name"], "ylen64")
    return int(near.sum())
