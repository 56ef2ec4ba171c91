"""Cases, float64 reference and bars of `rel_attention_kernel` (csrc/attention.hip), importable without a GPU.
test_attention_refs.py (CPU) proves the bars on the two fp32 oracles and on the mutants; test_gpu_attention.py
(-m gpu) runs every case through `mbv_op_rel_attention` into the same `att_check`.

Reference = `oracle/ref_infer.py: relative_attention` restated dtype-generic (`att_compute`; the test proves the
restatement equal to the original bit for bit), in float64 from the fp32 inputs.  Two fp32 oracles:
 * plain: `att_compute` in fp32 (torch.softmax over the whole row, P normalised before the contraction);
 * tiled: `att_tiled`, the kernel's algorithm: 32-key tiles dealt round-robin to two waves, a running (max, sum) per
   query, O and the nine band weights rescaled by exp(m - m'), wave 1 folded into wave 0, one division by the sum at
   the end, the relative-value term added after the normalisation.
`mut` names a deliberate mistake (MUTANTS, with the restatement that carries it).

Bars, per case, over the valid queries (t < len): median, 99.9th percentile and maximum of |got - ref64| each at most
MARGIN x the larger of the two fp32 oracles' own, plus one fp32 ulp of the reference's RMS.  MARGIN = 4, as in
small_op_cases.py: a kernel may differ from the oracles by operation order, FMA contraction and its libm (each within
a few ulp), not by more.  Padded query columns must be finite (a NaN there survives `* x_mask` and reaches the last
valid column through the FFN's K = 3 conv), nothing may be left at the NaN pre-fill, two launches agree bit for bit.

Input regimes (the `regime` field): flat (randn: a flat softmax, the median row maximum of p is 0.005 at T = 200),
sharp (q, k x 4), shifted (a component shared by q and k along one direction gives every logit of an even query about
+100 and of an odd query about -100: an un-subtracted maximum overflows / underflows in fp32), rising / falling (the
shared component grows / shrinks by key tile so that every valid tile moves the running maximum by more than 20; the
row maximum is in the last / first valid tile, which the lengths put into a wave-1 tile and into a wave-0 tile).
Relative embeddings are 0.3 x randn, and 3 x randn in the `emb3` cases, where the band terms dominate.

Kernels reached: rel_attention_kernel<1> d = 32, <2> d = 40 and 64, <3> d = 96, <4> d = 100 and 128.

The errors |y - y64| over the valid queries, worst case per regime: the larger of the two fp32 oracles (CPU), the
MI355X (profiles/attention_bars.json), and the largest share of a bar (MARGIN x oracle + ulp) the MI355X uses.  The
kernel is inside the oracles' own error everywhere (the fp32 matrix cores accumulate the dot products more exactly
than the CPU's GEMM does); at MARGIN 1 the oracles use their own bar in full by construction.

    regime     oracle median  p99.9     max        MI355X median  p99.9    max       share of the bar
    flat       4.1e-08        6.3e-07   1.3e-06    3.1e-08        3.4e-07  5.2e-07   0.23
    sharp      9.8e-08        8.2e-06   1.7e-05    7.0e-08        4.7e-06  9.7e-06   0.17
    shifted    2.1e-06        3.1e-05   4.8e-05    1.6e-06        1.7e-05  2.3e-05   0.18
    rising     8.1e-07        2.1e-05   4.3e-05    4.8e-07        1.2e-05  1.8e-05   0.22
    falling    2.4e-06        2.3e-05   5.0e-05    1.4e-06        1.2e-05  2.0e-05   0.16
    emb3       1.6e-07        2.3e-05   3.0e-05    1.2e-07        6.9e-06  8.6e-06   0.18

(The errors of the shifted / rising / falling regimes are those of the format: a logit of 100 carries an ulp of 8e-6.)
"""
import functools
import math

import torch

from oracle import ref_infer as R
from small_op_cases import F32, F64, MARGIN, gen, tmask, ulp32

TILE, NW, WINDOW = 32, 2, R.WINDOW
FILL = -1e4

# name -> the restatement that carries the mistake
MUTANTS = {
    "no_max_sub": "tiled",            # P = exp(S), no running maximum at all
    "no_alpha_O": "tiled",            # O is not rescaled when the running maximum moves
    "no_alpha_band": "tiled",         # the nine band weights are not rescaled when the running maximum moves
    "fold_no_rescale": "tiled",       # wave 0 is not rescaled when wave 1 holds the maximum
    "empty_wave_counts": "tiled",     # a wave without key tiles is folded as (m, l) = (0, 1) instead of (-inf, 0)
    "rel_unscaled": "plain",          # relative logits from q instead of q / sqrt(d)
    "band_3": "plain",                # |r| = 4 is dropped (logit and value)
    "window_tile_clipped": "tiled",   # the relative terms are dropped when i and j lie in different 32-tiles
    "val_mirrored": "plain",          # Ev[4 - r] for Ev[4 + r]
    "keys_unmasked": "plain",         # keys behind the length keep their logits
    "pad_fill_inf": "plain",          # -inf for -1e4: a padded query's row is all -inf (caught by finiteness alone)
}


def att_case(name, B, H, heads, T, lens, regime="flat", emb=0.3):
    assert len(lens) == B and H % heads == 0
    return dict(name=name, B=B, H=H, heads=heads, T=T, lens=lens, regime=regime, emb=emb)


# lengths: T, 1 (and 0), the tile boundary 32, inside a tile, a whole wave's tiles padded (T = 64 / 65, len <= 32),
# a trailing tile padded (T = 97, len <= 64)
ATT_CASES = [
    att_case("flat_d32_h4_t1", 2, 128, 4, 1, [1, 0]),
    att_case("flat_d40_h2_t31", 3, 80, 2, 31, [31, 1, 13]),
    att_case("flat_d64_h2_t32", 3, 128, 2, 32, [32, 1, 17]),
    att_case("flat_d96_h2_t33", 3, 192, 2, 33, [33, 32, 1]),
    att_case("flat_d100_h2_t64", 4, 200, 2, 64, [64, 1, 32, 45]),
    att_case("flat_d128_h1_t65", 3, 128, 1, 65, [65, 33, 20]),
    att_case("flat_d128_h2_t97", 4, 256, 2, 97, [97, 64, 0, 70]),
    att_case("sharp_d64_h2_t97", 3, 128, 2, 97, [97, 50, 32], "sharp"),
    att_case("sharp_d100_h1_t33", 2, 100, 1, 33, [33, 9], "sharp"),
    att_case("shifted_d32_h4_t65", 3, 128, 4, 65, [65, 32, 41], "shifted"),
    att_case("shifted_d96_h1_t97", 2, 96, 1, 97, [97, 64], "shifted"),
    att_case("shifted_d128_h1_t64", 2, 128, 1, 64, [64, 30], "shifted"),
    att_case("rising_d64_h2_t64", 4, 128, 2, 64, [64, 45, 32, 20], "rising"),
    att_case("rising_d40_h2_t97", 4, 80, 2, 97, [97, 64, 70, 33], "rising"),
    att_case("rising_d128_h1_t97", 3, 128, 1, 97, [97, 90, 75], "rising"),
    att_case("rising_d100_h2_t65", 3, 200, 2, 65, [65, 64, 1], "rising"),
    att_case("falling_d96_h2_t97", 3, 192, 2, 97, [97, 64, 40], "falling"),
    att_case("falling_d32_h1_t65", 2, 32, 1, 65, [65, 33], "falling"),
    att_case("emb3_d64_h2_t97", 3, 128, 2, 97, [97, 64, 37], emb=3.0),
    att_case("emb3_sharp_d96_h1_t33", 2, 96, 1, 33, [33, 5], "sharp", emb=3.0),
]
STEP = 40.0                   # rising / falling: the shared component's logit step from one key tile to the next
SHIFT = 100.0                 # shifted: the common logit offset of a query


def att_inputs(c):
    g = gen(c["name"])
    B, H, heads, T = c["B"], c["H"], c["heads"], c["T"]
    d = H // heads
    qkv = torch.randn(B, 3, heads, d, T, generator=g)
    u = torch.randn(d, generator=g)
    u = u / u.norm()                                          # the shared direction, one per case
    t = torch.arange(T)
    if c["regime"] == "sharp":
        qkv[:, :2] *= 4
    elif c["regime"] == "shifted":                            # logit offset = (+-a)(a) / sqrt(d)
        a = math.sqrt(SHIFT * math.sqrt(d))
        sign = torch.where(t % 2 == 0, 1.0, -1.0)
        qkv[:, 0] += a * sign[None, None, None, :] * u[None, None, :, None]
        qkv[:, 1] += a * u[None, None, :, None]
    elif c["regime"] in ("rising", "falling"):                # logit offset = a (a tile) / sqrt(d): STEP per key tile
        a = math.sqrt(STEP * math.sqrt(d))
        tile = (t // TILE).float()
        ramp = tile if c["regime"] == "rising" else float((T - 1) // TILE) - tile
        qkv[:, 0] += a * u[None, None, :, None]
        qkv[:, 1] += a * ramp[None, None, None, :] * u[None, None, :, None]
    return {"qkv": qkv.reshape(B, 3 * H, T).contiguous(), "emb_k": c["emb"] * torch.randn(9, d, generator=g),
            "emb_v": c["emb"] * torch.randn(9, d, generator=g), "lens": torch.tensor(c["lens"], dtype=torch.int64)}


# ---------------------------------------------------------------------------------------------- the restatements
def _heads(c, inp, dtype):
    B, H, heads, T = c["B"], c["H"], c["heads"], c["T"]
    d = H // heads
    x = inp["qkv"].to(dtype).view(B, 3, heads, d, T).transpose(3, 4)                  # [B, 3, h, T, d]
    return x[:, 0], x[:, 1], x[:, 2], inp["emb_k"].to(dtype), inp["emb_v"].to(dtype), d


def _band(T, mut=None):
    """(r, i): the queries i whose key i + r exists, for the relative positions r of the window."""
    idx = torch.arange(T)
    w = WINDOW - 1 if mut == "band_3" else WINDOW
    for r in range(-w, w + 1):
        i = idx[(idx + r >= 0) & (idx + r < T)]
        if mut == "window_tile_clipped":
            i = i[i // TILE == (i + r) // TILE]
        yield r, i


def _scores(c, inp, dtype, mut=None):
    """The masked logits [B, h, T, T] (ref_infer.relative_attention up to its softmax), v [B, h, T, d] and Ev."""
    q, k, v, ek, ev, d = _heads(c, inp, dtype)
    T = c["T"]
    qh = q / math.sqrt(d)
    scores = qh @ k.transpose(-1, -2)
    rel = (q if mut == "rel_unscaled" else qh) @ ek.t()
    for r, i in _band(T, mut):
        scores[:, :, i, i + r] += rel[:, :, i, r + WINDOW]
    m = tmask(c["lens"], T, dtype)
    pair = m[:, None, :, None] * (torch.ones_like(m) if mut == "keys_unmasked" else m)[:, None, None, :]
    scores = scores.masked_fill(pair == 0, -float("inf") if mut == "pad_fill_inf" else FILL)
    return scores, v, ev


def _rel_values(c, out, p, ev, mut=None):
    for r, i in _band(c["T"], mut):
        e = ev[WINDOW - r] if mut == "val_mirrored" else ev[r + WINDOW]
        out[:, :, i, :] += p[:, :, i, i + r].unsqueeze(-1) * e[None, None, None, :]
    return out


def att_compute(c, inp, dtype, mut=None):
    """ref_infer.relative_attention, dtype-generic -> [B, H, T]."""
    scores, v, ev = _scores(c, inp, dtype, mut)
    if mut == "no_max_sub":
        e = torch.exp(scores)
        p = e / e.sum(-1, keepdim=True)
    else:
        p = torch.softmax(scores, dim=-1)
    out = _rel_values(c, p @ v, p, ev, mut)
    return out.transpose(2, 3).reshape(c["B"], c["H"], c["T"])


def att_tiled(c, inp, dtype, mut=None):
    """The kernel's algorithm (csrc/attention.hip) -> [B, H, T]."""
    S, v, ev = _scores(c, inp, dtype, mut)
    B, heads, T, d = v.shape
    ntiles = (T + TILE - 1) // TILE
    ninf = torch.full((B, heads, T), -float("inf"), dtype=dtype)
    waves = []
    for w in range(NW):
        m, l = ninf.clone(), torch.zeros(B, heads, T, dtype=dtype)
        O, wb = torch.zeros(B, heads, T, d, dtype=dtype), torch.zeros(B, heads, T, T, dtype=dtype)
        for kt in range(w, ntiles, NW):                          # wb: the band weights, kept at their key's column
            cols = slice(kt * TILE, min(T, (kt + 1) * TILE))
            St = S[..., cols]
            mnew = torch.zeros_like(m) if mut == "no_max_sub" else torch.maximum(m, St.max(-1).values)
            alpha = torch.ones_like(m) if mut == "no_max_sub" else torch.exp(m - mnew)
            P = torch.exp(St - mnew[..., None])
            l = l * alpha + P.sum(-1)
            O = (O if mut == "no_alpha_O" else O * alpha[..., None]) + P @ v[:, :, cols]
            wb = wb if mut == "no_alpha_band" else wb * alpha[..., None]
            wb[..., cols] = P
            m = mnew
        waves.append((m, l, O, wb))
    (m0, l0, O0, wb0), (m1, l1, O1, wb1) = waves
    if mut == "empty_wave_counts" and ntiles < NW:
        m1, l1 = torch.zeros_like(m1), torch.ones_like(l1)
    if mut == "no_max_sub":
        a0, a1 = torch.ones_like(m0), torch.ones_like(m0)
    else:
        mall = torch.maximum(m0, m1)
        a0 = torch.exp(m0 - mall)
        if mut == "fold_no_rescale":
            a0 = torch.where(m1 > m0, torch.ones_like(a0), a0)
        a1 = torch.where(m1 > -float("inf"), torch.exp(m1 - mall), torch.zeros_like(m1))
    rsum = 1 / (l0 * a0 + l1 * a1)
    O = (O0 * a0[..., None] + O1 * a1[..., None]) * rsum[..., None]
    p_band = (wb0 * a0[..., None] + wb1 * a1[..., None]) * rsum[..., None]
    out = _rel_values(c, O, p_band, ev, mut)
    return out.transpose(2, 3).reshape(c["B"], c["H"], c["T"])


ORACLES = {"plain": att_compute, "tiled": att_tiled}


@functools.lru_cache(maxsize=None)
def _shared(name):
    """The inputs, the float64 reference and the two fp32 oracles of a case, computed once and left unchanged."""
    c = next(x for x in ATT_CASES if x["name"] == name)
    inp = att_inputs(c)
    return inp, att_compute(c, inp, F64), {k: f(c, inp, F32) for k, f in ORACLES.items()}


def att_shared(c):
    return _shared(c["name"])


# ---------------------------------------------------------------------------------------------- the bars
class Stats(dict):
    """case -> the errors of the code under test and of the oracles, and the largest share of a bar used."""


def _three(e):
    e = e.flatten()
    return [float(torch.quantile(e, 0.5)), float(torch.quantile(e, 0.999)), float(e.max())]


def att_check(c, got, margin=MARGIN, stats=None):
    """got: fp32 [B, H, T] of the code under test."""
    inp, ref, orcs = att_shared(c)
    got = got.to(F64)
    assert got.shape == ref.shape, (c["name"], got.shape, ref.shape)
    valid = tmask(c["lens"], c["T"]).bool()[:, None, :].expand_as(ref)
    assert not bool(torch.isnan(got).any()), (c["name"], "NaN (pre-fill or computed)", int(torch.isnan(got).sum()))
    assert bool(torch.isfinite(got[~valid]).all()), (c["name"], "non-finite padded query columns")
    assert bool(torch.isfinite(got[valid]).all()), (c["name"], "non-finite output")
    assert bool(torch.isfinite(ref).all())
    ulp = ulp32(float(ref[valid].pow(2).mean().sqrt()))
    e = _three((got - ref)[valid].abs())
    e_o = [max(x) for x in zip(*(_three((o.to(F64) - ref)[valid].abs()) for o in orcs.values()))]
    used = [a / (margin * b + ulp) for a, b in zip(e, e_o)]
    if stats is not None:
        stats[c["name"]] = {"regime": "emb3" if c["emb"] != 0.3 else c["regime"], "median": e[0], "p999": e[1],
                            "max": e[2], "oracle_median": e_o[0], "oracle_p999": e_o[1], "oracle_max": e_o[2],
                            "ulp_rms": ulp, "bar_used": max(used)}
    print("%-24s median %.3g (oracles %.3g)  p99.9 %.3g (%.3g)  max %.3g (%.3g)  ulp(rms) %.3g  bar used %.2f"
          % (c["name"], e[0], e_o[0], e[1], e_o[1], e[2], e_o[2], ulp, max(used)))
    for what, a, b in zip(("median", "p99.9", "max"), e, e_o):
        assert a <= margin * b + ulp, (c["name"], what, a, b, ulp)
