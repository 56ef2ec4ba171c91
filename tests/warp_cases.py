"""Cases, float64 reference and bars of the time-warp kernel (csrc/warp.hip), importable without a GPU.
test_warp_refs.py (CPU) proves the bars on the fp32 oracle and on mutated restatements and asserts the premises;
test_gpu_warp_pin.py (-m gpu) runs every case through `net.warp` / `net.warp_ranges` into the same checks.

Reference = `warp_ref.warp` (float64) from the fp32 samples, evaluated at chosen outputs through `first` / `end`.
`warp_compute(case, res_type, dtype, mut)` is that arithmetic restated dtype-generic.  float64 without `mut` it IS
`warp_ref.warp` (bitwise; `test_warp_refs.py` asserts it).  In fp32 it restates the kernel: tau in float64, the window
table `float32(win)` and `float32(win[i + 1] - win[i])` of `resample_ref.table` as `warp_window` of capi.hip builds it,
the weight `float32(eta) delta + win`, every product and four partial sums per wing each rounded (no FMA: a kernel that
contracts rounds less), the two wings added, `x float32(scale)` last; and the kernel's window geometry (j0, W, the
count cuts) restated from the tile of the output, so that a mutant can change it.  `mut` names a deliberate mistake
(MUTANTS) that the bars must catch.

Bars (small_op_cases.check_rounded, reused)
 * per element |y - y64| <= TOL u A + FLOOR, u = 2^-24, A = sum_k |w_k| |x[src_k]| in float64 over the taps
   `warp_ref._wings` visits inside [0, min(n, in_avail)), the weights with the `scale` factor as the reference has
   them.  Nothing of A comes from the kernel's arithmetic;
 * per case: median and 99.9th percentile at most MARGIN = 4 x the oracle's, plus one fp32 ulp of the reference's RMS;
 * impulses (x = 1.0f at p, else 0): A = |w|, so every tap's weight is held to about TOL u relative, and an output
   whose wings do not hold p is +0.0 bitwise.  (Not bitwise on the weights: the kernel's `fmaf` weight cannot be
   restated from NumPy without a double rounding.)

TOL["warp"] = 4 x the worst err / (u A) of the fp32 oracle over the committed cases, rounded up to one digit (the
rule of small_op_cases.py).  Measured on the CPU (test_warp_refs.py prints it):

    kernel entry                          oracle worst err / (u A)   TOL    MI355X (profiles/warp_bars.json)
    warp (whole rows, impulses, envelope)       4.42                 20     4.42
    warp_ranges (the open frontier)             3.12                 20     3.12
    warp_ranges, t > 10^6 and t > 2^24          3.18                 20     3.21

What each case is for (the smallest shape at which the thing can still go wrong):
    octave_up     R = 2.0 x 6 frames: three full tiles whose staged window is the 772 floats kWarpWindow was sized for
    octave_down   R = 0.5 x 3 frames
    near_top      a full-width tile that crosses frame boundaries and rates where 512 / R truncates
    alternating   integer U[f] with neighbours of different rates: the only case that sees `frame_lt`
    glided        a two-token table with the default glide
    irrational    fractional U, a hop that is no power of two, frame changes inside tiles
    hop1          700 frames of one sample: one tile spans hundreds of frames, the binary search does real work
    long          1.15 M outputs, the last three tiles: tau in fp32 is off by 0.1 sample there
    past_2_24     20 M outputs: three tiles behind 2^24, where (float)t is no longer exact, and the last two tiles

The widest tile.  255 outputs at 2.0 apart and 128 taps on both sides would be 255 * 2 + 2 * 128 = 766 samples; the
filter gives one fewer.  At R = 2 an output reads 128 taps in one wing only when the table offset of that wing is 0
or 1, and then the other wing starts at offset 255 or 256 and holds 127: 255 taps per output, 255 * 2 + 255 = 765
samples per tile.  `premises` asserts 765 (reached by `octave_up` and `near_top`) and that the staged window of that
tile, 772 floats, fits kWarpWindow.

Every mutant of MUTANTS is separated by committed cases; none had to be left out."""
import functools
import math
import zlib

import numpy as np
import torch

import gain_ref
import resample_ref as RR
import small_op_cases as sc
import warp_ref
from small_op_cases import MARGIN, U, Stats, check_exact, check_rounded   # noqa: F401  (re-exported to the tests)

TOL = sc.TOL                                    # check_rounded reads its bar there
TOL["warp"] = 20.0
MUTANTS = {"warp": ["small_window", "hw_of_one", "step_rounded", "no_eta", "tau_fp32", "frame_lt", "unscaled",
                    "rate_of_tile", "frac_unscaled"]}
FILTERS = ["kaiser_best", "kaiser_fast"]
TILE = 256                                      # outputs per workgroup (kWarpTile, csrc/kernels.h)
WARP_WINDOW = 776                               # floats of the staged window (kWarpWindow, csrc/kernels.h)
NB = 512                                        # table entries per zero crossing (kWarpNb, csrc/warp.hip)
SMALL_WINDOW = 600                              # the cap of the `small_window` mutant
F32, F64 = np.float32, np.float64


def rng(name):
    return np.random.RandomState(zlib.crc32(name.encode()))


# ---------------------------------------------------------------------------------------------- the cases
def _glided():
    """two tokens, 4 and 2 frames, a fifth up and a fourth down, with the default glide (tests/test_gpu_warp.py)"""
    return warp_ref.glide(warp_ref.frame_rates([warp_ref.pitch_of_semitones(7), warp_ref.pitch_of_semitones(-5)],
                                               [0, 4, 6], 6), 2)


def _cycle(F):
    return np.tile(np.asarray([1.37, 0.61, 1.0], F32), -(-F // 3))[:F]


def _case(name, R, hop, ranges=None):
    R = np.ascontiguousarray(R, F32)
    assert bool(((R >= warp_ref.PITCH_MIN) & (R <= warp_ref.PITCH_MAX)).all())
    R.setflags(write=False)
    return dict(name=name, R=R, hop=hop, ranges=ranges)


_TOP = np.nextafter(F32(2.0), F32(0))
CASES = [
    _case("octave_up", np.full(6, 2.0), 256),
    _case("octave_down", np.full(3, 0.5), 256),
    _case("near_top", [2.0, _TOP, 1.9961, 2.0, 2.0, 1.0, 0.5, 2.0, 2.0, 2.0], 256),
    _case("alternating", [0.5, 2.0] * 3, 256),
    _case("glided", _glided(), 256),
    _case("irrational", [1.37, 0.61, 1.9, 0.77, 1.0, 1.21, 0.5, 2.0], 100),
    _case("hop1", rng("hop1/rates").uniform(0.5, 2.0, 700), 1),
    _case("long", _cycle(4000), 256, ranges="tail3"),
    _case("past_2_24", _cycle(70000), 256, ranges="past_2_24"),
]
CASE_BY_NAME = {c["name"]: c for c in CASES}
WHOLE = [c for c in CASES if c["ranges"] is None]
RANGED = [c for c in CASES if c["ranges"] is not None]
IMPULSE_CASES = ["near_top", "irrational"]
FRONTIER_CASES = ["near_top", "irrational"]
ENVELOPE_CASES = ["near_top"]
ENVELOPE_GAINS = [1.0, 4.0, 0.0, 1e-3, 2.5, 1.0, 0.5, 2.0, 0.25, 3.0, 1.0]     # F + 1 of near_top; neighbours differ


@functools.lru_cache(maxsize=None)
def plan(name):
    """(U float64 [F + 1], n_out) of the case, from the reference"""
    c = CASE_BY_NAME[name]
    U_, n_out = warp_ref.plan(c["R"], c["hop"])
    U_.setflags(write=False)
    return U_, n_out


def samples(c):
    return len(c["R"]) * c["hop"]


def case_ranges(c):
    """[(first, end)] of the outputs the case computes: the whole row, or the ranges one `warp_ranges` call takes"""
    n_out = plan(c["name"])[1]
    if c["ranges"] is None:
        return [(0, n_out)]
    if c["ranges"] == "tail3":                                    # the last three tiles of the row
        return [((n_out - 600) // TILE * TILE, n_out)]
    a = 2 ** 24 + TILE                                            # the first multiple of 256 above 2^24
    return [(a, a + 3 * TILE), (((n_out - 1) // TILE - 1) * TILE, n_out)]


@functools.lru_cache(maxsize=None)
def case_x(name):
    """fp32 [F hop], uniform in [-1, 1], seeded from the case's name"""
    x = rng(name).uniform(-1, 1, samples(CASE_BY_NAME[name])).astype(F32)
    x.setflags(write=False)
    return x


def impulse_positions(c):
    """p: inside, 0, n - 1, and the last sample in front of a frame boundary"""
    n = samples(c)
    return [n // 2 + 7, 0, n - 1, 3 * c["hop"] - 1]


def frontier(c):
    return 5 * c["hop"] // 2                                      # in_avail at 2.5 frames


# ---------------------------------------------------------------------------------------------- the arithmetic
def _frames(ts, U_, F, mut):
    """the largest f < F with U[f] <= t  (`frame_lt`: with U[f] < t)"""
    f = np.searchsorted(U_, ts.astype(F64), side="left" if mut == "frame_lt" else "right") - 1
    return np.clip(f, 0, F - 1)


def _tau(ts, c, mut):
    """(tau float64, frame) of the outputs ts; `tau_fp32`: every operation of it in fp32"""
    R, hop = c["R"], c["hop"]
    U_ = plan(c["name"])[0]
    f = _frames(ts, U_, len(R), mut)
    if mut == "tau_fp32":
        return ((f * hop).astype(F32) + (ts.astype(F32) - U_[f].astype(F32)) * R[f]).astype(F64), f
    return (f * hop).astype(F64) + (ts.astype(F64) - U_[f]) * R[f].astype(F64), f


def geometry(c, res_type, ts, first, end, mut=None):
    """Everything the kernel derives from the output index, for the outputs ts of the range [first, end): the staged
    window [j0, j0 + W) of the output's tile, floor(tau), and per wing the table offset, eta and the tap count after
    the window's cuts."""
    ts = np.asarray(ts, np.int64)
    nz = RR.FILTERS[res_type][0]
    nwin = NB * nz + 1
    hw = nz + 2 if mut == "hw_of_one" else warp_ref.half_width(c["R"], res_type)
    cap = SMALL_WINDOW if mut == "small_window" else WARP_WINDOW
    t0 = first + (ts - first) // TILE * TILE
    t_last = np.minimum(t0 + TILE - 1, end - 1)
    tau0, f0 = _tau(t0, c, mut)
    j0 = tau0.astype(np.int64) - hw
    W = np.minimum(_tau(t_last, c, mut)[0].astype(np.int64) + hw + 2 - j0, cap)
    tau, f = _tau(ts, c, mut)
    rate = c["R"][f0 if mut == "rate_of_tile" else f]
    scale = np.where(rate > 1, 1.0 / rate.astype(F64), 1.0)
    step = (np.round(scale * NB) if mut == "step_rounded" else scale * NB).astype(np.int64)
    nt = tau.astype(np.int64)
    cw = nt - j0
    inside = (cw >= 0) & (cw < W)
    cc = np.where(inside, cw, 0)
    frac = tau - nt if mut == "frac_unscaled" else scale * (tau - nt)
    wings = []
    for side in (0, 1):
        fr = frac if side == 0 else scale - frac
        idx = fr * NB
        off = np.clip(idx.astype(np.int64), 0, NB)
        eta = np.zeros_like(idx) if mut == "no_eta" else idx - off
        cnt = np.minimum((nwin - off) // step, cc + 1 if side == 0 else W - cc - 1)
        wings.append((off, eta, np.where(inside, np.maximum(cnt, 0), 0)))
    return dict(nt=nt, scale=scale, step=step, up=rate > 1, wings=wings, W=W, j0=j0)


@functools.lru_cache(maxsize=None)
def _table32(res_type):
    """the device table: fp32 values and fp32 forward differences (fp64, rounded once), the last one zero"""
    win, _ = RR.table(res_type)
    delta = np.zeros_like(win)
    delta[:-1] = np.diff(win)
    return win.astype(F32), delta.astype(F32)


def _wing4(p, cnt):
    """One wing's sum as `warp_wing` keeps it: products p [n, K] fp32 (zero past cnt), taps 4 q + l < 4 (cnt // 4) in
    partial sum l, the remaining taps in partial sum 0, (a0 + a1) + (a2 + a3)."""
    n, K = p.shape
    k = np.arange(K)
    full = cnt // 4 * 4
    main = np.where(k[None, :] < full[:, None], p, F32(0))
    acc = np.zeros((n, 4), F32)
    for q in range(0, K, 4):
        acc += main[:, q:q + 4]
    rows = np.arange(n)
    for r in range(3):
        i = full + r
        acc[:, 0] += np.where(i < cnt, p[rows, np.minimum(i, K - 1)], F32(0))
    assert acc.dtype == F32
    return (acc[:, 0] + acc[:, 1]) + (acc[:, 2] + acc[:, 3])


def warp_compute(c, res_type, x, ts, first, end, dtype=F64, mut=None, in_avail=None):
    """The outputs ts (inside the range [first, end), whose first output starts a tile) of the row x [F hop], in
    `dtype`.  float64: the reference's weights (the window times scale, then interpolated) and its sums; fp32: the
    kernel's.  Taps outside [0, min(n, in_avail)) read a zero."""
    ts = np.asarray(ts, np.int64)
    n = samples(c)
    assert len(x) == n
    limit = n if in_avail is None else min(n, int(in_avail))
    g = geometry(c, res_type, ts, first, end, mut)
    if dtype == F64:
        x = np.asarray(x, F64)
        y = np.zeros(len(ts))
        for i in range(len(ts)):
            scale = 1.0 if mut == "unscaled" else float(g["scale"][i])
            win, delta, _ = warp_ref._window(res_type, scale)
            acc = 0.0
            for side, (off, eta, cnt) in enumerate(g["wings"]):
                k = np.arange(int(cnt[i]))
                j = int(off[i]) + k * int(g["step"][i])
                src = int(g["nt"][i]) - k if side == 0 else int(g["nt"][i]) + 1 + k
                w = win[j] + float(eta[i]) * delta[j]
                ok = (src >= 0) & (src < limit)
                acc += float(np.sum(w[ok] * x[src[ok]]))
            y[i] = acc
        _trim_tables()
        return y
    assert dtype == F32 and np.asarray(x).dtype == F32
    win, delta = _table32(res_type)
    total = np.zeros(len(ts), F32)
    for side, (off, eta, cnt) in enumerate(g["wings"]):
        K = -(-max(int(cnt.max()) if cnt.size else 0, 1) // 4) * 4
        k = np.arange(K)
        live = k[None, :] < cnt[:, None]
        j = np.where(live, off[:, None] + k[None, :] * g["step"][:, None], 0)
        src = g["nt"][:, None] - k[None, :] if side == 0 else g["nt"][:, None] + 1 + k[None, :]
        live &= (src >= 0) & (src < limit)                       # a staged zero: the product adds nothing
        xs = np.where(live, x[np.where(live, src, 0)], F32(0))
        w = eta.astype(F32)[:, None] * delta[j] + win[j]
        p = np.where(live, w * xs, F32(0))
        assert w.dtype == F32 and p.dtype == F32
        total = total + _wing4(p, cnt) if side else _wing4(p, cnt)
    if mut != "unscaled":
        total = np.where(g["up"], total * g["scale"].astype(F32), total)
    assert total.dtype == F32
    return total


def _trim_tables():
    """`warp_ref` keeps one scaled window per rate it has seen: a table of hundreds of rates (hop1) is let go"""
    if len(warp_ref._tables) > 64:
        warp_ref._tables.clear()


def bound(c, res_type, x, ts, in_avail=None):
    """(A float64 [len(ts)], holds bool [len(ts)]): A = sum |w| |x[src]| over the taps `warp_ref._wings` visits inside
    [0, min(n, in_avail)); holds: one of those taps reads a non-zero sample."""
    x = np.abs(np.asarray(x, F64))
    n = samples(c)
    limit = n if in_avail is None else min(n, int(in_avail))
    U_ = plan(c["name"])[0]
    A = np.zeros(len(ts))
    holds = np.zeros(len(ts), bool)
    for i, t in enumerate(ts):
        for src, w in warp_ref._wings(int(t), U_, c["R"], c["hop"], res_type):
            ok = (src >= 0) & (src < limit)
            A[i] += float(np.sum(np.abs(w[ok]) * x[src[ok]]))
            holds[i] |= bool((x[src[ok]] != 0).any())
    _trim_tables()
    return A, holds


def reference(c, res_type, x, first, end, in_avail=None):
    y = warp_ref.warp(np.asarray(x, F64), c["R"], c["hop"], res_type, in_avail=in_avail, first=first, end=end)
    _trim_tables()
    return y


# ---------------------------------------------------------------------------------------------- expectations, shared
def variants(c):
    """[(variant name, x fp32 [F hop] as the kernel's arithmetic sees it, in_avail or None, impulse position or None)]
    of a case: the noise row, and where the case is named for them the impulses, the open frontier and the envelope.
    (The envelope's row is `gain_ref.shaped(x, G, hop)`: the fp32 product the kernel forms where it reads.)"""
    name = c["name"]
    out = [("noise", case_x(name), None, None)]
    if name in IMPULSE_CASES:
        for p in impulse_positions(c):
            x = np.zeros(samples(c), F32)
            x[p] = 1.0
            out.append(("impulse%d" % p, x, None, p))
    if name in FRONTIER_CASES:
        out.append(("frontier", case_x(name), frontier(c), None))
    if name in ENVELOPE_CASES:
        out.append(("envelope", gain_ref.shaped(case_x(name), np.asarray(ENVELOPE_GAINS, F32), c["hop"]), None, None))
    return out


def variant_ranges(c, in_avail, res_type):
    if in_avail is None:
        return case_ranges(c)
    U_ = plan(c["name"])[0]
    return [(0, warp_ref.ready(c["R"], U_, c["hop"], in_avail, res_type))]


@functools.lru_cache(maxsize=None)
def expected(name, res_type):
    """{variant: [dict(first, end, ref, A float64, holds bool, orc fp32)] per range}, computed once and shared"""
    c = CASE_BY_NAME[name]
    out = {}
    for vn, x, in_avail, _ in variants(c):
        rows = []
        for first, end in variant_ranges(c, in_avail, res_type):
            ts = np.arange(first, end, dtype=np.int64)
            A, holds = bound(c, res_type, x, ts, in_avail)
            e = dict(first=first, end=end, ref=reference(c, res_type, x, first, end, in_avail), A=A, holds=holds,
                     orc=warp_compute(c, res_type, x, ts, first, end, F32, None, in_avail))
            for v in e.values():
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)
            rows.append(e)
        out[vn] = rows
    return out


def forget(name):
    """drop what the 70 MB row has cached"""
    if name == "past_2_24":
        case_x.cache_clear()
        expected.cache_clear()


def check(c, res_type, variant, k, got, **kw):
    """The bars on `got` (fp32 [end - first]), the outputs of range k of the case's variant."""
    e = expected(c["name"], res_type)[variant][k]
    what = "%s/%s/%s[%d:%d]" % (c["name"], res_type, variant, e["first"], e["end"])
    got = np.ascontiguousarray(got)
    assert got.dtype == F32 and got.shape == e["ref"].shape, (what, got.dtype, got.shape, e["ref"].shape)
    tt = torch.from_numpy
    check_rounded("warp", what, tt(got), tt(e["ref"].copy()), tt(e["A"].copy()), tt(e["orc"].copy()), **kw)
    if variant.startswith("impulse"):
        away = ~e["holds"]
        assert away.any() and e["holds"].any(), what
        check_exact(what + " +0.0 where no wing holds p", tt(got[away].copy()), torch.zeros(int(away.sum())))


ENTRIES = ("warp", "warp_ranges", "warp_ranges_long")


def entry_of(c, variant):
    """the row of the table above (and of profiles/warp_bars.json) a check is counted under"""
    return "warp_ranges_long" if c["ranges"] is not None else "warp_ranges" if variant == "frontier" else "warp"


def run(c, res_type, fn, stats=None, **kw):
    """Every variant and range of the case, computed by `fn(x, ts, first, end, in_avail) -> fp32`, through the bars.
    stats: {entry: Stats}."""
    for vn, x, in_avail, _ in variants(c):
        for k, (first, end) in enumerate(variant_ranges(c, in_avail, res_type)):
            got = fn(x, np.arange(first, end, dtype=np.int64), first, end, in_avail)
            check(c, res_type, vn, k, got, stats=None if stats is None else stats[entry_of(c, vn)], **kw)


# ---------------------------------------------------------------------------------------------- premises
def tile_extent(c, res_type, t0, t_last):
    """(samples from the lowest to the highest tap of the tile, floats of its staged window as kernels.h defines it),
    from the reference alone"""
    U_ = plan(c["name"])[0]
    ext = [warp_ref.tap_extent(t, U_, c["R"], c["hop"], res_type) for t in range(t0, t_last + 1)]
    hw = warp_ref.half_width(c["R"], res_type)
    j0 = int(warp_ref.tau(t0, U_, c["R"], c["hop"])[0]) - hw
    j_end = int(warp_ref.tau(t_last, U_, c["R"], c["hop"])[0]) + hw + 2
    lo, hi = min(e[0] for e in ext), max(e[1] for e in ext)
    assert j0 <= lo and hi < j_end, (c["name"], "a tap outside the staged window", j0, lo, hi, j_end)
    return hi - lo + 1, j_end - j0


WIDEST_EXTENT = 255 * 2 + 255                   # see "The widest tile" above


def premises():
    """What the reference alone must show about the cases -> dict of the figures"""
    out = {}
    for name in ("octave_up", "near_top"):
        c = CASE_BY_NAME[name]
        n_out = plan(name)[1]
        tiles = [tile_extent(c, "kaiser_best", t0, min(t0 + TILE, n_out) - 1) for t0 in range(0, n_out, TILE)]
        widest = max(e for e, _ in tiles)
        staged = max(w for e, w in tiles if e == widest)
        out[name] = (widest, staged, sum(e == widest for e, _ in tiles))
        assert widest >= WIDEST_EXTENT, (name, "no tile as wide as the window was sized for", widest)
        assert SMALL_WINDOW < staged <= WARP_WINDOW, (name, staged, WARP_WINDOW)
        assert max(w for _, w in tiles) <= WARP_WINDOW, (name, "a staged window past kWarpWindow")
    (a, _), = case_ranges(CASE_BY_NAME["long"])
    assert a >= 10 ** 6 and a % TILE == 0, a
    (b, b_end), (e, n_out) = case_ranges(CASE_BY_NAME["past_2_24"])
    assert b > 2 ** 24 and b % TILE == 0 and b - TILE <= 2 ** 24 and b_end <= e and e % TILE == 0, (b, e)
    assert n_out == plan("past_2_24")[1] and TILE < n_out - e <= 2 * TILE
    assert float(F32(b + 1)) != b + 1                             # (float)t is not exact there
    out["long_first"], out["past_first"] = a, b
    c = CASE_BY_NAME["alternating"]
    U_ = plan("alternating")[0]
    on = [f for f in range(1, len(c["R"])) if U_[f] == math.floor(U_[f]) and c["R"][f] != c["R"][f - 1]]
    assert len(on) >= 4, ("alternating: outputs with t == U[f] at a change of rate", on)
    out["alternating_on_U"] = [int(U_[f]) for f in on]
    return out
