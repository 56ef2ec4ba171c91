"""Cases, float64 references and bars of the small kernels between the convs (csrc/ops.hip, csrc/sdp.hip and the
conv + LayerNorm epilogue of csrc/conv1d_narrow.hip), importable without a GPU.  test_small_op_refs.py (CPU) proves
the bars on the fp32 oracle and on mutated restatements; test_gpu_small_ops.py (-m gpu) runs every case through its
`mbv_op_*` entry point into the same `check_*` functions.

Reference = the operation in float64 from the fp32 inputs: `oracle/ref_infer.py` on `.double()` tensors where it has
a function of that granularity (`channel_layer_norm`, `rq_spline_inverse`, `length_regulate`, the steps of
`dds_conv`), plain float64 torch (CPU) otherwise.  Every `*_compute(case, inputs, dtype, mut)` is dtype-generic:
float64 is the reference, float32 is "the fp32 oracle" (the same formula as torch runs it on the CPU), and `mut` names
a deliberate mistake (MUTANTS) that the bars must catch.

Bars
 * exact outputs (gathers, masks, integer results, one correctly rounded fp32 operation) are compared bitwise;
 * rounded outputs, per element: |y - y64| <= TOL[kernel] * u * A + FLOOR, u = 2^-24, A = first-order propagation of
   one rounding per operation through the formula as the kernel writes it, in float64 (`*_bound`).  FLOOR = 2^-126:
   a result below the smallest normal fp32 may be flushed to zero;
 * rounded outputs, per case: median and 99.9th percentile of |y - y64| at most MARGIN x the fp32 oracle's on the
   same inputs, plus one fp32 ulp of the reference's RMS (the oracle's median can be 0).

TOL[kernel] = 4 x the worst err / (u A) of the fp32 oracle over the committed cases, rounded up to one digit;
MARGIN = 4: a kernel may differ from the oracle by operation order, FMA contraction and its libm (each within a few
ulp), not by more.  The oracle's worst ratios, measured on the CPU (test_small_op_refs.py prints them):

    kernel        oracle worst err / (u A)   TOL    MI355X (profiles/small_op_bars.json)
    layernorm            3.75                 20       3.75    (near-constant columns: the variance's own rounding)
    conv_ln              2.25                 10       1.87    (fused and unfused)
    dds_sep              2.59                 20       1.63
    dds_res              1.35                 6        1.28
    spline               0.358                2        0.325   (KN = 80, `spline_bound`)
    cond_gemv            3.34                 20       3.34    (the same fma chain as the oracle's GEMM on that element)
    dur_logw             0.867                4        0.945
    sdp_pre              1.30                 6        0.913
    sdp_logw             0.561                3        0.561
    expand_zp            0.747                3        0.700
    posterior            0.655                3        0.493

The fp32 oracle's GELU is the erf formula on torch.erf, not F.gelu (see `_gelu`).

Durations: `w_ceil`, `cum`, `y_lengths` are exact.  A token is left out of that only if its float64 duration
exp(logw64) * length_scale lies within 8 fp32 ulps of an integer (plus, where logw is itself a rounded dot product,
what its own bar TOL u A lets through: d/dlogw of the duration is the duration), or in the range [2^-150, 2^-126)
where fp32 has only denormals (ceil is 0 flushed, 1 kept).  Below 2^-150 the duration is 0 in fp32 and the reference
says 0.  At most max(2, 1e-4 x tokens) tokens per case may be left out; such a token may come out as either
neighbour, and the rest of its row is compared from the reference sums shifted by what was observed.

Two spline mutants cannot be separated by any input and are therefore NOT in MUTANTS (do not add them): `<` for `<=`
at |y| = 5, where the spline and the identity agree to rounding, and the 1e-6 nudge of the last knot, which the clamp
of the bin index hides."""
import math
import zlib

import numpy as np
import torch
import torch.nn.functional as F

from oracle import ref_infer as R

U = 2.0 ** -24
FLOOR = 2.0 ** -126
MARGIN = 4.0
F64, F32 = torch.float64, torch.float32
KN = 80.0                    # spline: absolute error, in units of u, granted to every knot, width, height and to t

TOL = {"layernorm": 20.0, "conv_ln": 10.0, "dds_sep": 20.0, "dds_res": 6.0, "spline": 2.0, "cond_gemv": 20.0,
       "dur_logw": 4.0, "sdp_pre": 6.0, "sdp_logw": 3.0, "expand_zp": 3.0, "posterior": 3.0}

MUTANTS = {
    "layernorm": ["eps", "onepass", "nomask"],
    "conv_ln": ["eps", "nomask", "res_after_mask"],
    "dds_sep": ["tanh", "unmasked", "wronghalf", "eps"],
    "dds_res": ["tanh", "nomask", "res_after_mask"],
    "spline": ["notails", "nomind", "nominw", "nothreshold", "edge_softplus0", "heights_unscaled"],
    "durations": ["floor1", "scale_in_exp"],
    "expand": ["ge"],
}


def gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def ragged(B, T, rot=0):
    """Lengths that include T, 0, 1 and a value inside a 32-column tile (as many of them as B allows, rotated)."""
    pool = [T, 0, 1, max(1, min(T - 1, T // 2 // 32 * 32 + 13))]
    out = [pool[(i + rot) % 4] for i in range(min(B, 4))]
    k = 0
    while len(out) < B:
        out.append((k * 7919 + 13) % (T + 1))
        k += 1
    return out


def tmask(lens, T, dtype=F64):
    return (torch.arange(T)[None, :] < torch.as_tensor(lens)[:, None]).to(dtype)      # [B, T]


def _d(inp, dtype):
    return {k: (v.to(dtype) if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in inp.items()}


# ---------------------------------------------------------------------------------------------- the bars
class Stats(dict):
    """kernel -> worst err / (u A) and the largest share of the median / 99.9 % bars used, over the cases seen."""

    def add(self, kernel, ratio, qmed, q999):
        w = self.setdefault(kernel, {"err_over_uA": 0.0, "median_bar_used": 0.0, "p999_bar_used": 0.0, "TOL": TOL[kernel]})
        w["err_over_uA"] = max(w["err_over_uA"], ratio)
        w["median_bar_used"] = max(w["median_bar_used"], qmed)
        w["p999_bar_used"] = max(w["p999_bar_used"], q999)


def ulp32(x):
    return float(np.spacing(np.float32(abs(x)))) if x > 0 else 0.0


def check_rounded(kernel, what, got, ref, A, orc, tol_scale=1.0, margin=MARGIN, stats=None, sel=None):
    """got / orc: fp32 results of the code under test / of the fp32 oracle; ref, A: float64.  sel: the elements the
    bars apply to (default all); elements with A == 0 must be exact."""
    got, orc = got.to(F64), orc.to(F64)
    if sel is not None:
        got, ref, A, orc = got[sel], ref[sel], A[sel], orc[sel]
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert bool(torch.isfinite(ref).all()), (what, "reference not finite")
    assert bool(torch.isfinite(got).all()), (what, "non-finite output", int((~torch.isfinite(got)).sum()))
    if got.numel() == 0:
        return
    err = (got - ref).abs()
    tol = TOL[kernel] * tol_scale
    ratio = float(((err - FLOOR).clamp_min(0) / (U * A).clamp_min(1e-300)).max())
    bad = err > tol * U * A + FLOOR
    e_o = (orc - ref).abs()
    ulp = ulp32(float(ref.pow(2).mean().sqrt()))
    q = lambda e, p: float(torch.quantile(e.flatten()[:: max(1, e.numel() // 4000000)], p))
    med, p999, med_o, p999_o = q(err, 0.5), q(err, 0.999), q(e_o, 0.5), q(e_o, 0.999)
    if stats is not None:
        used = lambda e, o: e / (margin * o + ulp) if margin * o + ulp else 0.0       # share of the quantile bar
        stats.add(kernel, ratio, used(med, med_o), used(p999, p999_o))
    print("%-28s err/(uA) %.3g (tol %.3g)  median %.3g (oracle %.3g)  p99.9 %.3g (oracle %.3g)  ulp(rms) %.3g"
          % (what, ratio, tol, med, med_o, p999, p999_o, ulp))
    assert not bool(bad.any()), (what, "element bar", int(bad.sum()), float(err.max()), ratio, tol)
    assert med <= margin * med_o + ulp, (what, "median", med, med_o, ulp)
    assert p999 <= margin * p999_o + ulp, (what, "p99.9", p999, p999_o, ulp)


def check_exact(what, got, want):
    got, want = torch.as_tensor(got), torch.as_tensor(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if got.is_floating_point():                       # bitwise (-0.0 and +0.0 differ, NaN never matches)
        same = got.contiguous().view(torch.int32) == want.contiguous().view(torch.int32)
    else:
        same = got == want
    assert bool(same.all()), (what, "not bitwise equal", int((~same).sum()), same.numel())


# ---------------------------------------------------------------------------------------------- channel LayerNorm
def _layer_norm(v, gamma, beta, mut=None):
    if mut == "onepass":                              # E[x^2] - mean^2
        mean = v.mean(1, keepdim=True)
        var = (v * v).mean(1, keepdim=True) - mean * mean
        return (v - mean) * torch.rsqrt(var + 1e-5) * gamma[None, :, None] + beta[None, :, None]
    return R.channel_layer_norm(v, gamma, beta, eps=1e-6 if mut == "eps" else 1e-5)


def _ln_A(v, Av, y, gamma):
    """|gamma| rstd (Av + mean_c Av) + |y|: one rounding on every v (Av >= |v|), on the mean, on the difference."""
    v = v.to(F64)
    var = ((v - v.mean(1, keepdim=True)) ** 2).mean(1, keepdim=True)
    rstd = torch.rsqrt(var + 1e-5)
    return gamma.abs()[None, :, None] * rstd * (Av + Av.mean(1, keepdim=True)) + y.abs()


def ln_case(name, B, C, T, cols, res=False, relu=0, lens=None):
    return dict(name=name, B=B, C=C, T=T, cols=cols, res=res, relu=relu, lens=lens)


# column kinds, assigned to t cyclically: randn | const (one value per column) | zero | offset (1e3 + 1e-2 randn) |
# neg (all negative: all zero behind the ReLU) | sparse (randn - 2.5: a few survivors behind the ReLU)
LN_CASES = [
    ln_case("ln_c32_t1_b1", 1, 32, 1, ["randn"]),
    ln_case("ln_c32_t1_const", 1, 32, 1, ["const"], lens=[1]),
    ln_case("ln_c96_t5_b3_res", 3, 96, 5, ["randn", "const", "offset", "zero"], res=True, lens=ragged(3, 5, 1)),
    ln_case("ln_c160_t31_b3_relu", 3, 160, 31, ["sparse", "neg", "randn", "offset"], relu=1),
    ln_case("ln_c192_t32_b3_res_lens", 3, 192, 32, ["randn", "offset", "const"], res=True, lens=ragged(3, 32)),
    ln_case("ln_c256_t33_b3_relu_lens", 3, 256, 33, ["randn", "sparse", "neg", "zero"], relu=1, lens=ragged(3, 33, 2)),
    ln_case("ln_c192_t255_b3_res", 3, 192, 255, ["randn", "randn", "const", "offset"], res=True),
    ln_case("ln_c256_t256_b3_relu", 3, 256, 256, ["randn", "sparse", "neg"], relu=1, lens=ragged(3, 256, 3)),
    ln_case("ln_c192_t257_b3_res_lens", 3, 192, 257, ["randn", "zero", "offset"], res=True, lens=ragged(3, 257, 1)),
    ln_case("ln_c96_t1000_b1", 1, 96, 1000, ["randn", "const", "offset", "sparse"], lens=[777]),
    ln_case("ln_c160_t1000_b1_res_relu", 1, 160, 1000, ["randn", "sparse"], res=True, relu=1),
    ln_case("ln_c192_t33_b64_res_lens", 64, 192, 33, ["randn", "offset", "const", "zero"], res=True, lens=ragged(64, 33)),
    ln_case("ln_c256_t33_b64_relu", 64, 256, 33, ["sparse", "randn", "neg"], relu=1, lens=ragged(64, 33, 2)),
    ln_case("ln_c32_t257_b64", 64, 32, 257, ["randn", "const"], lens=ragged(64, 257, 1)),
]


def _columns(g, B, C, T, cols):
    a = torch.randn(B, C, T, generator=g)
    plain = torch.ones(T, dtype=torch.bool)
    kt = torch.arange(T) % len(cols)
    for i, kind in enumerate(cols):
        sel = kt == i
        n = int(sel.sum())
        if kind == "randn" or n == 0:
            continue
        if kind == "const":
            a[:, :, sel] = (3 * torch.randn(B, 1, n, generator=g)).expand(B, C, n)
            plain[sel] = False
        elif kind == "zero":
            a[:, :, sel] = 0
            plain[sel] = False
        elif kind == "offset":
            a[:, :, sel] = 1e3 + 1e-2 * torch.randn(B, C, n, generator=g)
        elif kind == "neg":
            a[:, :, sel] = -torch.randn(B, C, n, generator=g).abs() - 0.1
        elif kind == "sparse":
            a[:, :, sel] = torch.randn(B, C, n, generator=g) - 2.5
        else:
            raise KeyError(kind)
    return a, plain


def ln_inputs(c):
    g = gen(c["name"])
    a, plain = _columns(g, c["B"], c["C"], c["T"], c["cols"])
    inp = {"a": a, "gamma": 1 + 0.3 * torch.randn(c["C"], generator=g), "beta": 0.3 * torch.randn(c["C"], generator=g)}
    if c["res"]:
        inp["r"] = torch.randn(c["B"], c["C"], c["T"], generator=g) * plain[None, None, :]   # const / zero columns stay so
    return inp


def ln_compute(c, inp, dtype, mut=None):
    i = _d(inp, dtype)
    v = i["a"] + i["r"] if c["res"] else i["a"]
    if c["relu"]:
        v = torch.relu(v)
    y = _layer_norm(v, i["gamma"], i["beta"], mut)
    if c["lens"] is not None and mut != "nomask":
        y = y * tmask(c["lens"], c["T"], dtype)[:, None, :]
    return {"y": y}


def ln_bound(c, inp, ref):
    i = _d(inp, F64)
    v = i["a"] + i["r"] if c["res"] else i["a"]
    Av = i["a"].abs() + i["r"].abs() if c["res"] else v.abs()
    if c["relu"]:
        v = torch.relu(v)
    y = R.channel_layer_norm(v, i["gamma"], i["beta"])
    A = _ln_A(v, Av, y, i["gamma"])
    if c["lens"] is not None:
        A = A * tmask(c["lens"], c["T"])[:, None, :]
    return {"y": A}


def ln_check(c, inp, got, **kw):
    ref, orc = ln_compute(c, inp, F64), ln_compute(c, inp, F32)
    check_rounded("layernorm", c["name"], got["y"], ref["y"], ln_bound(c, inp, ref)["y"], orc["y"], **kw)


# ---------------------------------------------------------------------------------------------- conv + LayerNorm (EPI_LN)
def cln_inputs(c):
    """c: a case of conv_cases.LN_CASES."""
    g = gen(c["name"])
    B, Cin, Cout, T, K = c["B"], c["Cin"], c["Cout"], c["T"], c["K"]
    inp = {"x": torch.randn(B, Cin, T, generator=g), "w": torch.randn(Cout, Cin, K, generator=g) / math.sqrt(Cin * K),
           "bias": 0.5 * torch.randn(Cout, generator=g),
           "gamma": 1 + 0.3 * torch.randn(Cout, generator=g), "beta": 0.3 * torch.randn(Cout, generator=g)}
    if c["chan_add"]:
        inp["chan_add"] = 0.5 * torch.randn(B, Cin, generator=g)
    if c["ln_res"]:
        inp["res"] = torch.randn(B, Cout, T, generator=g)
    return inp


def _cln_conv(c, i, dtype, absolute=False):
    x = i["x"]
    if c["chan_add"]:
        x = x + i["chan_add"][:, :, None]
    if c["in_lens"] is not None:
        x = x * tmask(c["in_lens"], c["T"], dtype)[:, None, :]
    w, b = i["w"], i["bias"]
    if absolute:
        x, w, b = x.abs(), w.abs(), b.abs()
    return F.conv1d(x, w, b, padding=(c["K"] - 1) // 2)


def cln_compute(c, inp, dtype, mut=None):
    i = _d(inp, dtype)
    y = _cln_conv(c, i, dtype)
    if c["relu"]:
        y = torch.relu(y)
    om = tmask(c["out_lens"], c["T"], dtype)[:, None, :] if c["out_lens"] is not None else None
    if mut == "res_after_mask":
        y = y + i["res"] if c["ln_res"] else y
        y = y * om if om is not None else y
    else:
        y = y * om if om is not None else y
        y = y + i["res"] if c["ln_res"] else y
    v = y
    y = _layer_norm(v, i["gamma"], i["beta"], mut)
    if c["ln_out_lens"] is not None and mut != "nomask":
        y = y * tmask(c["ln_out_lens"], c["T"], dtype)[:, None, :]
    return {"y": y, "v": v}


def cln_bound(c, inp, ref):
    i = _d(inp, F64)
    Ac = _cln_conv(c, i, F64, absolute=True)                  # the conv's own A (test_gpu_conv_routes.py)
    if c["out_lens"] is not None:
        Ac = Ac * tmask(c["out_lens"], c["T"])[:, None, :]
    Av = Ac + (i["res"].abs() if c["ln_res"] else 0)
    y = R.channel_layer_norm(ref["v"], i["gamma"], i["beta"])
    A = _ln_A(ref["v"], Av, y, i["gamma"])
    if c["ln_out_lens"] is not None:
        A = A * tmask(c["ln_out_lens"], c["T"])[:, None, :]
    return {"y": A}


def cln_check(c, inp, got, **kw):
    ref, orc = cln_compute(c, inp, F64), cln_compute(c, inp, F32)
    check_rounded("conv_ln", c["name"], got["y"], ref["y"], cln_bound(c, inp, ref)["y"], orc["y"], **kw)


# ---------------------------------------------------------------------------------------------- DDSConv halves
def _gelu_A(x, Ax):
    """gelu as the kernel writes it: 0.5 x (1 + erf(x / sqrt 2)); roundings of the argument, the erf, the sum, the
    products; Ax = the bound on x itself."""
    t = x / math.sqrt(2.0)
    e = torch.erf(t)
    s = 1 + e
    As = 2 / math.sqrt(math.pi) * torch.exp(-t * t) * t.abs() + e.abs() + s.abs()
    gp = 0.5 * s + x * torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)
    return gp.abs() * Ax + 0.5 * x.abs() * As + 2 * (0.5 * x * s).abs()


def _gelu(x, mut=None):
    """float64: F.gelu.  fp32: the erf formula the kernel writes, on torch.erf; NOT F.gelu, whose fused CPU kernel is
    less precise than fp32 arithmetic (measured: 9.8 u A at x = -3.39, absolute 1e-6 on a value of -1.2e-3, against 0.9
    for the formula) and would quadruple TOL for no reason of the format."""
    if mut == "tanh":
        return F.gelu(x, approximate="tanh")
    return F.gelu(x) if x.dtype == F64 else 0.5 * x * (1 + torch.erf(x * 0.70710678118654752440))


def dds_case(name, B, C, T, dil, lens, out_lens=False):
    return dict(name=name, B=B, C=C, T=T, dil=dil, lens=lens, out_lens=out_lens)


DDS_CASES = [
    dds_case("dds_c192_t1_d1", 1, 192, 1, 1, [1]),
    dds_case("dds_c192_t5_d9", 3, 192, 5, 9, ragged(3, 5, 1), out_lens=True),          # T and lengths below the dilation
    dds_case("dds_c96_t31_d3", 3, 96, 31, 3, ragged(3, 31)),
    dds_case("dds_c32_t32_d1", 3, 32, 32, 1, ragged(3, 32, 2), out_lens=True),
    dds_case("dds_c160_t33_d9", 3, 160, 33, 9, [33, 5, 8]),                             # len < dil in the middle of a row
    dds_case("dds_c256_t255_d3", 3, 256, 255, 3, ragged(3, 255, 3), out_lens=True),
    dds_case("dds_c192_t256_d9", 3, 192, 256, 9, ragged(3, 256, 1)),
    dds_case("dds_c192_t257_d1", 3, 192, 257, 1, ragged(3, 257), out_lens=True),
    dds_case("dds_c96_t1000_d9", 1, 96, 1000, 9, [613]),
    dds_case("dds_c192_t33_b64_d3", 64, 192, 33, 3, ragged(64, 33), out_lens=True),
    dds_case("dds_c256_t31_b64_d9", 64, 256, 31, 9, ragged(64, 31, 2)),
]


def dds_inputs(c):
    g = gen(c["name"])
    B, C, T = c["B"], c["C"], c["T"]
    r = lambda *s: torch.randn(*s, generator=g)
    return {"x": r(B, C, T), "w": 0.6 * r(C, 3), "bias": 0.3 * r(C), "g1": 1 + 0.3 * r(C), "b1": 0.3 * r(C),
            "a": 1.5 * r(B, C, T), "xres": r(B, C, T), "g2": 1 + 0.3 * r(C), "b2": 0.3 * r(C)}


def _dw_conv(xm, w, bias, dil, half):
    """y[c, t] = bias[c] + sum_k w[c, k] xm[c, t - half + k dil], zeros outside (half != dil only in a mutant)."""
    T = xm.shape[2]
    xp = F.pad(xm, (32, 32))
    y = bias[None, :, None].expand_as(xm).clone()
    for k in range(3):
        o = 32 - half + k * dil
        y = y + w[None, :, k, None] * xp[:, :, o:o + T]
    return y


def dds_sep_compute(c, inp, dtype, mut=None):
    i = _d(inp, dtype)
    xm = i["x"] if mut == "unmasked" else i["x"] * tmask(c["lens"], c["T"], dtype)[:, None, :]
    dil = c["dil"]
    if mut == "wronghalf":
        v = _dw_conv(xm, i["w"], i["bias"], dil, 1 if dil != 1 else 3)
    else:                                              # the oracle's own step (ref_infer.dds_conv)
        v = F.conv1d(xm, i["w"][:, None, :], i["bias"], padding=(3 * dil - dil) // 2, dilation=dil, groups=c["C"])
    ln = _layer_norm(v, i["g1"], i["b1"], mut)
    return {"y": _gelu(ln, mut), "v": v, "ln": ln}


def dds_sep_bound(c, inp, ref):
    i = _d(inp, F64)
    xm = (i["x"] * tmask(c["lens"], c["T"])[:, None, :]).abs()
    Av = _dw_conv(xm, i["w"].abs(), i["bias"].abs(), c["dil"], c["dil"])
    return {"y": _gelu_A(ref["ln"], _ln_A(ref["v"], Av, ref["ln"], i["g1"]))}


def dds_res_compute(c, inp, dtype, mut=None):
    i = _d(inp, dtype)
    ln = _layer_norm(i["a"], i["g2"], i["b2"])
    y = _gelu(ln, mut)
    m = tmask(c["lens"], c["T"], dtype)[:, None, :] if c["out_lens"] and mut != "nomask" else 1
    y = i["xres"] + y * m if mut == "res_after_mask" else (i["xres"] + y) * m
    return {"y": y, "ln": ln}


def dds_res_bound(c, inp, ref):
    i = _d(inp, F64)
    A = _gelu_A(ref["ln"], _ln_A(i["a"], i["a"].abs(), ref["ln"], i["g2"])) + i["xres"].abs() + ref["y"].abs()
    if c["out_lens"]:
        A = A * tmask(c["lens"], c["T"])[:, None, :]
    return {"y": A}


def dds_sep_check(c, inp, got, **kw):
    ref, orc = dds_sep_compute(c, inp, F64), dds_sep_compute(c, inp, F32)
    check_rounded("dds_sep", c["name"], got["y"], ref["y"], dds_sep_bound(c, inp, ref)["y"], orc["y"], **kw)


def dds_res_check(c, inp, got, **kw):
    ref, orc = dds_res_compute(c, inp, F64), dds_res_compute(c, inp, F32)
    check_rounded("dds_res", c["name"], got["y"], ref["y"], dds_res_bound(c, inp, ref)["y"], orc["y"], **kw)


# ---------------------------------------------------------------------------------------------- inverse spline
EDGE_CONST = float(np.log(np.exp(1 - R.SDP_MIN) - 1))          # transforms.py:74, as the library computes it


def spline_case(name, B, C, T, s_wh, s_d, lens):
    return dict(name=name, B=B, C=C, T=T, s_wh=s_wh, s_d=s_d, lens=lens)


SPLINE_CASES = [
    spline_case("spl_golden_scale_t1000", 1, 192, 1000, 0.1, 0.5, [913]),
    spline_case("spl_s1_t257", 3, 192, 257, 1.0, 1.0, ragged(3, 257)),
    spline_case("spl_s3_t256", 3, 96, 256, 3.0, 3.0, ragged(3, 256, 1)),
    spline_case("spl_s8_t255", 3, 256, 255, 8.0, 8.0, ragged(3, 255, 2)),
    spline_case("spl_s8_d25_t1000", 1, 192, 1000, 8.0, 25.0, [1000]),
    spline_case("spl_s3_d25_b64_t33", 64, 192, 33, 3.0, 25.0, ragged(64, 33)),
    spline_case("spl_s1_d8_b64_t31", 64, 160, 31, 1.0, 8.0, ragged(64, 31, 3)),
    spline_case("spl_s01_t1", 1, 32, 1, 0.1, 0.5, [1]),
    spline_case("spl_s3_t5", 3, 192, 5, 3.0, 3.0, ragged(3, 5, 3)),
    spline_case("spl_s8_t32", 3, 192, 32, 8.0, 3.0, ragged(3, 32)),
]
_F5 = np.float32(5.0)
PLANTED_Y = [5.0, -5.0, float(np.nextafter(_F5, np.float32(6))), float(np.nextafter(_F5, np.float32(0))),
             -float(np.nextafter(_F5, np.float32(6))), -float(np.nextafter(_F5, np.float32(0))), 7.0, -7.0, 0.0, -0.0]


def spline_inputs(c):
    g = gen(c["name"])
    B, C, T = c["B"], c["C"], c["T"]
    h = torch.randn(B, 29, T, generator=g)
    h[:, :20] *= c["s_wh"] * math.sqrt(C)
    h[:, 20:] *= c["s_d"]
    n = B * T
    flat = h.permute(1, 0, 2).reshape(29, n)               # a copy; planted derivative parameters: +100 / -100
    for k, col in enumerate(range(3, n, 11)):
        flat[20 + k % 9, col] = 100.0 if k % 2 == 0 else -100.0
    h = flat.reshape(29, B, T).permute(1, 0, 2).contiguous()
    z = torch.empty(B, 2, T)
    z[:, 0] = 11 * torch.rand(B, T, generator=g) - 5.5
    z[:, 1] = torch.randn(B, T, generator=g)
    z0 = z[:, 0].reshape(n).clone()
    for k, col in enumerate(range(0, n, 7)):
        z0[col] = PLANTED_Y[k % len(PLANTED_Y)]
    z[:, 0] = z0.reshape(B, T)
    return {"h": h, "z": z}


def spline_terms(y, uw, uh, ud, mut=None):
    """ref_infer.rq_spline_inverse restated with its intermediates exposed (for the bound) and with the mutants."""
    nb, MIN, TAIL = uw.shape[-1], R.SDP_MIN, R.SDP_TAIL
    inside = torch.ones_like(y, dtype=torch.bool) if mut == "notails" else (y >= -TAIL) & (y <= TAIL)
    ud = F.pad(ud, (1, 1))
    ud[..., 0] = ud[..., -1] = 0.0 if mut == "edge_softplus0" else EDGE_CONST

    def knots(u):
        p = F.softmax(u, dim=-1)
        if mut != "nominw":
            p = MIN + (1 - MIN * nb) * p
        c = F.pad(torch.cumsum(p, dim=-1), (1, 0))
        c = 2 * TAIL * c - TAIL
        c[..., 0] = -TAIL
        c[..., -1] = TAIL
        return c, c[..., 1:] - c[..., :-1]

    cw, widths = knots(uw)
    ch, heights = knots(uh)
    sp = torch.log1p(torch.exp(ud)) if mut == "nothreshold" else F.softplus(ud)
    deriv = sp if mut == "nomind" else MIN + sp
    yc = torch.where(inside, y, torch.zeros_like(y))
    edges = ch.clone()
    edges[..., -1] += 1e-6
    idx = (torch.sum(yc[..., None] >= edges, dim=-1) - 1).clamp(0, nb - 1)[..., None]
    take = lambda t: t.gather(-1, idx)[..., 0]
    in_cw, in_w, in_ch, in_h = take(cw), take(widths), take(ch), take(heights)
    delta = take(heights / widths)
    d0, d1 = take(deriv), take(deriv[..., 1:])
    t = yc - in_ch
    s2 = d0 + d1 - 2 * delta
    a = t * s2 + in_h * (delta - d0)
    b = in_h * d0 - t * s2
    cc_ = -delta * t
    disc = b * b - 4 * a * cc_
    s = torch.sqrt(disc)
    D = -b - s
    root = (2 * cc_) / D
    out = torch.where(inside, root * in_w + in_cw, y)
    return dict(out=out, inside=inside, w=in_w, h=in_h, cw=in_cw, ch=in_ch, d0=d0, d1=d1, delta=delta, t=t, s2=s2,
                a=a, b=b, c=cc_, disc=disc, s=s, D=D, root=root)


def _spline_params(c, i, mut=None):
    hh = i["h"].permute(0, 2, 1)                                 # [B, T, 29]
    sc = math.sqrt(c["C"])
    uw, uh, ud = hh[..., :10] / sc, hh[..., 10:20] / (1.0 if mut == "heights_unscaled" else sc), hh[..., 20:]
    return uw, uh, ud


def spline_compute(c, inp, dtype, mut=None):
    """z[:, 0] <- z[:, 1] * mask (the Flip), z[:, 1] <- spline^-1(z[:, 0]) * mask."""
    i = _d(inp, dtype)
    uw, uh, ud = _spline_params(c, i, mut)
    y = i["z"][:, 0]
    out = R.rq_spline_inverse(y, uw, uh, ud) if mut is None else spline_terms(y, uw, uh, ud, mut)["out"]
    m = tmask(c["lens"], c["T"], dtype)
    return {"z0": i["z"][:, 1] * m, "z1": out * m}


def spline_bound(c, inp):
    """First-order bound through t, s2, a, b, c, disc, sqrt, -b - sqrt, root, root * w + cw, per element inside
    [-5, 5], with KN u of absolute error on every knot, width, height and on t (a cumsum of ten terms scaled to
    [-5, 5]); also returns the float64 intermediates (the discriminant, `inside`)."""
    i = _d(inp, F64)
    q = spline_terms(i["z"][:, 0], *_spline_params(c, i))
    w, h, d0, d1, delta, t = q["w"], q["h"], q["d0"], q["d1"], q["delta"], q["t"].abs()
    e_delta = KN / w + h * KN / w ** 2 + delta
    S2 = d0 + d1 + 2 * delta + 2 * e_delta
    Aa = t * S2 + KN * q["s2"].abs() + h * (delta + d0 + e_delta) + KN * (delta - d0).abs() + q["a"].abs()
    Ab = h * d0 + KN * d0 + t * S2 + KN * q["s2"].abs() + q["b"].abs()
    Ac = delta * KN + e_delta * t + q["c"].abs()
    Adisc = 2 * q["b"].abs() * Ab + 4 * (Aa * q["c"].abs() + q["a"].abs() * Ac) + q["disc"].abs()
    As = Adisc / (2 * q["s"]) + q["s"]
    AD = Ab + As
    Aroot = 2 * Ac / q["D"].abs() + (2 * q["c"]).abs() * AD / q["D"] ** 2 + q["root"].abs()
    A = Aroot * w + q["root"].abs() * KN + KN + q["out"].abs()
    return A, q


def spline_check(c, inp, got, **kw):
    ref, orc = spline_compute(c, inp, F64), spline_compute(c, inp, F32)
    A, q = spline_bound(c, inp)
    m = tmask(c["lens"], c["T"]).bool()
    check_exact(c["name"] + " z0 (Flip, mask)", got["z0"], orc["z0"])
    z1 = got["z1"]
    pos = q["disc"] > 0
    assert bool(torch.isfinite(z1[pos | ~q["inside"] | ~m]).all()), (c["name"], "non-finite where the float64 discriminant is positive")
    tails = ~q["inside"] & m                                     # the identity: the input's bits
    check_exact(c["name"] + " z1 tails", z1[tails], inp["z"][:, 0][tails])
    assert bool((z1[~m] == 0).all()), (c["name"], "masked columns")
    assert int((q["inside"] & m & ~pos).sum()) == 0, (c["name"], "float64 discriminant not positive")
    check_rounded("spline", c["name"], z1, ref["z1"], A, orc["z1"], sel=q["inside"] & m, **kw)


# ---------------------------------------------------------------------------------------------- durations
def dur_case(name, B, T, mode, ls, lens, C=1, plant=(), bias=0.3, bad=()):
    return dict(name=name, B=B, T=T, mode=mode, ls=ls, lens=lens, C=C, plant=plant, bias=bias, bad=bad)


# plant: "ints" (logw = 0 tokens: duration exactly length_scale), "zero_start" / "zero_mid" / "zero_all" (logw = -200 on
# row 0), "big" (logw = 6), "huge" / "long" (outside the supported range: the row is flagged like an invalid id)
DUR_CASES = [
    dur_case("dur_sdp_t1_ls1", 1, 1, "sdp", 1.0, [1], plant=("ints",)),
    dur_case("dur_sdp_t1_zero", 1, 1, "sdp", 1.0, [1], plant=("zero_all",)),
    dur_case("dur_sdp_t5_ls3", 3, 5, "sdp", 3.0, [5, 3, 0], plant=("ints", "zero_start"), bad=(1,)),
    dur_case("dur_sdp_t31_ls05", 3, 31, "sdp", 0.5, ragged(3, 31), plant=("ints", "zero_mid")),
    dur_case("dur_sdp_t255_ls12", 3, 255, "sdp", 1.2, ragged(3, 255), plant=("zero_start", "big")),
    dur_case("dur_sdp_t256_ls037", 3, 256, "sdp", 0.37, ragged(3, 256, 1), plant=("zero_mid", "big"), bad=(0, 2)),
    dur_case("dur_sdp_t257_ls1", 3, 257, "sdp", 1.0, [257, 257, 256], plant=("ints", "zero_all", "big")),
    dur_case("dur_sdp_t1000_ls12", 1, 1000, "sdp", 1.2, [1000], plant=("zero_start", "zero_mid")),
    dur_case("dur_sdp_t33_b64_ls1", 64, 33, "sdp", 1.0, ragged(64, 33), plant=("ints", "zero_mid"), bad=(5, 63)),
    dur_case("dur_sdp_t257_b64_ls3", 64, 257, "sdp", 3.0, ragged(64, 257, 2), plant=("ints", "zero_start", "big")),
    dur_case("dur_sdp_t257_huge", 4, 257, "sdp", 1.0, [257, 200, 257, 257], plant=("ints", "huge")),
    dur_case("dur_sdp_t1200_long", 3, 1200, "sdp", 1e6, [1200, 1200, 1100], plant=("long",)),
    dur_case("dur_dp_c256_t33_ls1", 3, 33, "dp", 1.0, ragged(3, 33), C=256),
    dur_case("dur_dp_c256_t257_ls12", 3, 257, "dp", 1.2, ragged(3, 257, 1), C=256, bad=(1,)),
    dur_case("dur_dp_c100_t256_ls037", 3, 256, "dp", 0.37, ragged(3, 256), C=100),
    dur_case("dur_dp_c256_t255_ints_ls3", 3, 255, "dp", 3.0, [255, 200, 1], C=256, plant=("ints",), bias=0.0),
    dur_case("dur_dp_c7_t1_ints_ls1", 1, 1, "dp", 1.0, [1], C=7, plant=("ints",), bias=0.0),
    dur_case("dur_dp_c256_t64_zero_all", 3, 64, "dp", 1.0, ragged(3, 64), C=256, bias=-200.0),
    dur_case("dur_dp_c256_t100_b64", 64, 100, "dp", 1.0, ragged(64, 100), C=256),
]
DUR_BY_NAME = {c["name"]: c for c in DUR_CASES}


def dur_inputs(c):
    g = gen(c["name"])
    B, T, C = c["B"], c["T"], c["C"]
    planted = torch.full((B, T), float("nan"))                   # logw values to plant (NaN: none)
    t = torch.arange(T)
    if "ints" in c["plant"]:
        planted[:, t % 3 == 0] = 0.0
    if "big" in c["plant"]:
        planted[:, t % 17 == 5] = 6.0
    if "zero_start" in c["plant"]:
        planted[0, : max(1, T // 4)] = -200.0
    if "zero_mid" in c["plant"]:
        planted[-1, T // 3: max(T // 3 + 1, 2 * T // 3)] = -200.0
    if "zero_all" in c["plant"]:
        planted[0, :] = -200.0
    if "huge" in c["plant"]:                                     # beyond the supported range: 1e13 frames, inf, NaN; row 2 stays
        planted[0, T // 2] = 30.0
        planted[1, 0] = float("inf")
    if "long" in c["plant"]:                 # length_scale 1e6: every token in range and exact, row 0 beyond 2^30 in all
        planted[:, :] = -200.0
        planted[0, :] = 0.0
        planted[1, : T // 2] = 0.0
        planted[2, ::100] = 0.0
    keep = torch.isnan(planted)
    inp = {"bad": torch.tensor([1 if b in c["bad"] else 0 for b in range(B)], dtype=torch.int32)}
    if c["mode"] == "sdp":
        lw = (1.2 * torch.randn(B, T, generator=g)).clamp(max=6.0)
        inp["h"] = torch.where(keep, lw, planted)
        if "huge" in c["plant"]:
            inp["h"][3, T - 1] = float("nan")
    else:                                                        # planted tokens: all-zero columns, logw = the bias
        h = 0.5 * torch.randn(B, C, T, generator=g)
        inp["h"] = h * keep[:, None, :]
        inp["w"] = 2 * torch.randn(C, generator=g) / math.sqrt(C)
        inp["bias"] = torch.tensor([c["bias"]])
    return inp


def dur_logw(c, inp, dtype, absolute=False):
    i = _d(inp, dtype)
    m = tmask(c["lens"], c["T"], dtype)
    if c["mode"] == "sdp":
        return torch.where(m.bool(), i["h"], torch.zeros_like(m))          # the kernel writes +0 behind the length
    h, w, b = (i["h"].abs(), i["w"].abs(), i["bias"].abs()) if absolute else (i["h"], i["w"], i["bias"])
    return ((w[None, :, None] * h).sum(1) + b) * m


def dur_compute(c, inp, dtype, mut=None, logw=None):
    m = tmask(c["lens"], c["T"], dtype)
    logw = dur_logw(c, inp, dtype) if logw is None else logw
    d = torch.exp(logw * c["ls"]) if mut == "scale_in_exp" else torch.exp(logw) * c["ls"]
    if dtype == F64:
        d = torch.where(d < 2.0 ** -150, torch.zeros_like(d), d)          # below half the smallest fp32 denormal: 0
    wc = (torch.floor(d) + 1 if mut == "floor1" else torch.ceil(d)) * m
    return {"logw": logw, "dur": d * m, "w_ceil": wc}


MAX_TOKEN_FRAMES, MAX_TOTAL_FRAMES = 2.0 ** 20, 2 ** 30       # the supported range (ops.hip, durations_kernel)


def dur_tail(c, inp, w_ceil):
    """cum, ylen32, ylen64 from (integer-valued) w_ceil, and `over`: the rows outside the supported range (a token of
    2^20 frames or more, inf and NaN included, counts 0; such a row, or one of more than 2^30 frames, is flagged)."""
    big = ~(w_ceil < MAX_TOKEN_FRAMES)
    cum = torch.cumsum(torch.where(big, torch.zeros_like(w_ceil), w_ceil).to(torch.int64), dim=1)
    over = big.any(1) | (cum[:, -1] > MAX_TOTAL_FRAMES)
    total = torch.where(over, torch.ones_like(cum[:, -1]), cum[:, -1].clamp_min(1))
    y64 = torch.where((inp["bad"] != 0) | over, torch.full_like(total, -1), total)
    return {"cum": cum.clamp_max(2 ** 31 - 1).to(torch.int32), "ylen32": total.to(torch.int32), "ylen64": y64, "over": over}


def dur_check(c, inp, got, tol_scale=1.0, margin=MARGIN, stats=None):
    ref, orc = dur_compute(c, inp, F64), dur_compute(c, inp, F32)
    m = tmask(c["lens"], c["T"]).bool()
    slack = torch.zeros_like(ref["dur"])
    if c["mode"] == "sdp":
        check_exact(c["name"] + " logw", got["logw"], orc["logw"])
        exact_int = inp["h"] == 0
    else:
        A = dur_logw(c, inp, F64, absolute=True) + ref["logw"].abs()
        check_rounded("dur_logw", c["name"] + " logw", got["logw"], ref["logw"], A, orc["logw"], tol_scale=tol_scale,
                      margin=margin, stats=stats)
        slack = ref["dur"] * TOL["dur_logw"] * U * A
        exact_int = A == 0                                       # an all-zero column and a zero bias: logw = 0 in any order
    d = ref["dur"]
    g_wc_raw = got["w_ceil"].to(F64)
    band = 8 * torch.from_numpy(np.spacing(d.numpy().astype(np.float32)).astype(np.float64)) + slack
    near = m & (((d - torch.round(d)).abs() <= band) & (d >= 2.0 ** -126) | (d > 0) & (d < 2.0 ** -126))
    near &= ~exact_int                                           # built to be exact integers: never left out
    huge = m & ~(d < MAX_TOKEN_FRAMES)                           # outside the supported range: flagged, w_ceil as it comes
    assert bool((~(g_wc_raw[huge] < MAX_TOKEN_FRAMES)).all()), (c["name"], "a token beyond 2^20 frames came out below")
    near &= ~huge
    n_tokens = int(m.sum())
    assert int(near.sum()) <= max(2, 1e-4 * n_tokens), (c["name"], "tokens left out", int(near.sum()), n_tokens)
    g_wc = got["w_ceil"].to(F64)
    lo = torch.where(d < 2.0 ** -126, torch.zeros_like(d), torch.round(d))
    ok_near = (g_wc == lo) | (g_wc == lo + 1)
    assert bool(ok_near[near].all()), (c["name"], "a left-out token is neither neighbour")
    want = torch.where(near | huge, g_wc, ref["w_ceil"])
    check_exact(c["name"] + " w_ceil", got["w_ceil"], want.to(F32))
    tail = dur_tail(c, inp, want)
    keep = ~tail.pop("over")                                     # cum of a flagged row is not specified
    check_exact(c["name"] + " cum", got["cum"][keep], tail.pop("cum")[keep])
    for k, v in tail.items():
        check_exact(c["name"] + " " + k, got[k], v)
    return int(near.sum())


# ---------------------------------------------------------------------------------------------- length regulation
def exp_case(name, dur, I, Tp, noise, outs=True):
    """dur: the durations case whose reference cum / y_lengths feed the expansion; Tp: 'max' (the longest row), or an
    offset to it; outs False: every optional output null."""
    return dict(name=name, dur=dur, I=I, Tp=Tp, noise=noise, outs=outs)


EXP_CASES = [
    exp_case("exp_t1_ints", "dur_sdp_t1_ls1", 192, 0, False),
    exp_case("exp_t1_zero_noise", "dur_sdp_t1_zero", 192, 2, True),
    exp_case("exp_t5_lead_zero_above", "dur_sdp_t5_ls3", 32, 7, True),
    exp_case("exp_t31_mid_zero_below", "dur_sdp_t31_ls05", 192, -9, False),
    exp_case("exp_t255_equal_noise", "dur_sdp_t255_ls12", 40, 0, True),
    exp_case("exp_t256_below_noise_no_outs", "dur_sdp_t256_ls037", 48, -33, True, outs=False),
    exp_case("exp_t257_zero_row", "dur_sdp_t257_ls1", 17, 1, False),
    exp_case("exp_t33_b64", "dur_sdp_t33_b64_ls1", 192, 0, True),
    exp_case("exp_dp_zero_all_no_outs", "dur_dp_c256_t64_zero_all", 192, 3, False, outs=False),
    exp_case("exp_t1000_equal", "dur_sdp_t1000_ls12", 16, 0, False),
]


def exp_inputs(c):
    dc = DUR_BY_NAME[c["dur"]]
    tail = dur_tail(dc, dur_inputs(dc), dur_compute(dc, dur_inputs(dc), F64)["w_ceil"])
    g = gen(c["name"])
    B, T, I = dc["B"], dc["T"], c["I"]
    Tp = max(1, int(tail["ylen32"].max()) + c["Tp"])
    inp = {"stats": torch.randn(B, 2 * I, T, generator=g), "cum": tail["cum"], "ylen": tail["ylen32"], "Tp": Tp,
           "noise_scale": 0.667 if c["noise"] else 0.0}
    inp["stats"][:, I:] *= 0.5
    if c["noise"]:
        inp["noise"] = torch.randn(B, I, Tp, generator=g)
    return inp


def exp_compute(c, inp, dtype, mut=None):
    i = _d(inp, dtype)
    B, T, I, Tp = i["cum"].shape[0], i["cum"].shape[1], c["I"], i["Tp"]
    tp = torch.arange(Tp)
    cum = i["cum"].to(torch.int64)
    valid = tp[None, :] < i["ylen"].to(torch.int64)[:, None]                       # [B, Tp]
    hit = (cum[:, None, :] >= tp[None, :, None]) if mut == "ge" else (cum[:, None, :] > tp[None, :, None])
    j = torch.where(hit.any(-1), hit.to(torch.int8).argmax(-1), torch.full((B, Tp), -1))     # first j with cum[j] > tp
    j = torch.where(valid, j, torch.full_like(j, -1))
    jj = j.clamp_min(0)[:, None, :].expand(B, I, Tp)
    live = (j >= 0)[:, None, :].expand(B, I, Tp)
    zero = torch.zeros(B, I, Tp, dtype=dtype)
    m_p = torch.where(live, torch.gather(i["stats"][:, :I], 2, jj), zero)
    logs_p = torch.where(live, torch.gather(i["stats"][:, I:], 2, jj), zero)
    z_p = m_p + i["noise"] * torch.exp(logs_p) * i["noise_scale"] if c["noise"] else m_p
    y_mask = valid.to(dtype)
    prev = F.pad(cum, (1, 0))[:, :-1]
    attn = (valid[:, :, None] & (tp[None, :, None] >= prev[:, None, :]) & (tp[None, :, None] < cum[:, None, :])).to(dtype)
    z = torch.where(valid[:, None, :].expand(B, I, Tp), z_p, zero)
    return {"m_p": m_p, "logs_p": logs_p, "z_p": z_p, "z": z, "y_mask": y_mask, "attn": attn}


def exp_check(c, inp, got, **kw):
    """got: m_p, logs_p, z_p, y_mask, attn only when c['outs']; z always."""
    ref, orc = exp_compute(c, inp, F64), exp_compute(c, inp, F32)
    if c["outs"]:
        for k in ("m_p", "logs_p", "y_mask", "attn"):
            check_exact(c["name"] + " " + k, got[k], orc[k])
        T = inp["cum"].shape[1]
        if inp["Tp"] >= int(inp["ylen"].max()):                  # attn rows sum to the durations
            w = torch.diff(inp["cum"].to(torch.int64), dim=1, prepend=torch.zeros(len(inp["cum"]), 1, dtype=torch.int64))
            assert bool((got["attn"].sum(1).to(torch.int64) == w).all()), c["name"]
    if not c["noise"]:
        if c["outs"]:
            check_exact(c["name"] + " z_p == m_p", got["z_p"], orc["m_p"])
        check_exact(c["name"] + " z == m_p * y_mask", got["z"], orc["z"])
        assert bool((orc["z"] == orc["m_p"] * orc["y_mask"][:, None, :]).all())
        return
    i = _d(inp, F64)
    A = ref["m_p"].abs() + 3 * (i["noise"] * torch.exp(ref["logs_p"]) * i["noise_scale"]).abs() + ref["z_p"].abs()
    if c["outs"]:
        check_rounded("expand_zp", c["name"] + " z_p", got["z_p"], ref["z_p"], A, orc["z_p"], **kw)
    ym = ref["y_mask"][:, None, :]
    check_rounded("expand_zp", c["name"] + " z", got["z"], ref["z"], A * ym, orc["z"], **kw)
    check_exact(c["name"] + " z masked", got["z"][(ym == 0).expand_as(got["z"])], torch.zeros(int((ym == 0).sum()) * c["I"]))


# ---------------------------------------------------------------------------------------------- the linear ones
def lin_case(name, kind, **kw):
    return dict(name=name, kind=kind, **kw)


LIN_CASES = [
    lin_case("gemv_dp_cond", "cond_gemv", B=3, Cin=256, Cout=192, bias=True),
    lin_case("gemv_wn_cond_b64", "cond_gemv", B=64, Cin=256, Cout=1536, bias=True),
    lin_case("gemv_odd_nobias", "cond_gemv", B=1, Cin=100, Cout=5, bias=False),
    lin_case("gemv_cout129", "cond_gemv", B=3, Cin=32, Cout=129, bias=True),
    lin_case("pre_c192_t257", "sdp_pre", B=3, C=192, T=257, zc=1),
    lin_case("pre_c96_t1_zc0", "sdp_pre", B=1, C=96, T=1, zc=0),
    lin_case("pre_c256_t33_b64", "sdp_pre", B=64, C=256, T=33, zc=1),
    lin_case("logw_t257", "sdp_logw", B=3, T=257, lens=ragged(3, 257)),
    lin_case("logw_t1", "sdp_logw", B=1, T=1, lens=[1]),
    lin_case("logw_t33_b64", "sdp_logw", B=64, T=33, lens=ragged(64, 33, 1)),
    lin_case("post_i192_t257", "posterior", B=3, I=192, T=257, lens=ragged(3, 257, 2), noise=True),
    lin_case("post_i32_t1000_nonoise", "posterior", B=1, I=32, T=1000, lens=[400], noise=False),
    lin_case("post_i96_t33_b64", "posterior", B=64, I=96, T=33, lens=ragged(64, 33), noise=True),
]


def lin_inputs(c):
    g = gen(c["name"])
    r = lambda *s: torch.randn(*s, generator=g)
    k = c["kind"]
    if k == "cond_gemv":
        inp = {"g": r(c["B"], c["Cin"]), "W": r(c["Cout"], c["Cin"]) / math.sqrt(c["Cin"])}
        if c["bias"]:
            inp["bias"] = 0.5 * r(c["Cout"])
        return inp
    if k == "sdp_pre":
        return {"z": r(c["B"], 2, c["T"]), "pre_w": r(c["C"]), "pre_b": 0.5 * r(c["C"]), "cond": r(c["B"], c["C"], c["T"])}
    if k == "sdp_logw":
        return {"z": 2 * r(c["B"], 2, c["T"]), "m": 0.7 * r(1), "logs": 0.5 * r(1)}
    inp = {"stats": r(c["B"], 2 * c["I"], c["T"])}
    if c["noise"]:
        inp["noise"] = r(c["B"], c["I"], c["T"])
    return inp


def lin_compute(c, inp, dtype, absolute=False):
    """absolute: the same operation on absolute values, every partial result counted once more (the bound A)."""
    i = _d(inp, dtype)
    if absolute:
        i = {k: (v.abs() if torch.is_tensor(v) else v) for k, v in i.items()}
    k = c["kind"]
    if k == "cond_gemv":
        y = i["g"] @ i["W"].t()
        return y + i["bias"][None, :] if c["bias"] else y
    if k == "sdp_pre":
        return i["pre_w"][None, :, None] * i["z"][:, c["zc"]][:, None, :] + i["pre_b"][None, :, None] + i["cond"]
    raw = _d(inp, dtype)                                         # (the argument of an exp keeps its sign)
    if k == "sdp_logw":                                          # roundings: difference, exp, two products
        m = tmask(c["lens"], c["T"], dtype)
        e = torch.exp(-raw["logs"])
        return 3 * (i["z"][:, 1] + i["m"]) * e * m if absolute else (i["z"][:, 1] - i["m"]) * e * m
    m = tmask(c["lens"], c["T"], dtype)[:, None, :].bool()
    I = c["I"]
    mean = i["stats"][:, :I]
    if c["noise"]:                                               # roundings: exp, product, sum
        n = i["noise"] * torch.exp(raw["stats"][:, I:])
        mean = mean + (3 * n if absolute else n)
    return torch.where(m, mean, torch.zeros_like(mean))


LIN_KERNEL = {"cond_gemv": "cond_gemv", "sdp_pre": "sdp_pre", "sdp_logw": "sdp_logw", "posterior": "posterior"}


def lin_check(c, inp, got, **kw):
    ref, orc = lin_compute(c, inp, F64), lin_compute(c, inp, F32)
    if c["kind"] == "posterior" and not c["noise"]:
        return check_exact(c["name"], got["y"], orc)
    A = lin_compute(c, inp, F64, absolute=True) + ref.abs()
    check_rounded(LIN_KERNEL[c["kind"]], c["name"], got["y"], ref, A, orc, **kw)


# ---------------------------------------------------------------------------------------------- the exact ones
def exact_case(name, kind, **kw):
    return dict(name=name, kind=kind, **kw)


EXACT_CASES = [
    exact_case("embed_h192_t33", "embed", B=3, T=33, H=192, V=59, lens=[33, 0, 13], bad_ids=True),
    exact_case("embed_h96_t257_badlen", "embed", B=3, T=257, H=96, V=59, lens=[300, -2, 257], bad_ids=False),
    exact_case("embed_h32_t1", "embed", B=1, T=1, H=32, V=3, lens=[1], bad_ids=False),
    exact_case("embed_h192_t31_b64", "embed", B=64, T=31, H=192, V=178, lens=ragged(64, 31), bad_ids=True),
    exact_case("gather_c256", "gather", B=5, C=256, rows=7, sid=[0, 6, 3, -1, 7]),
    exact_case("gather_c100_b64", "gather", B=64, C=100, rows=109, sid=[(7 * b) % 109 for b in range(64)]),
    exact_case("lens_t257", "lens", B=6, T=257, lens=[257, 0, 1, 258, -1, 100]),
    exact_case("lens_t1_b64", "lens", B=64, T=1, lens=[b % 3 - 1 for b in range(64)]),
    exact_case("lens_t1000_b70", "lens", B=70, T=1000, lens=[(b * 131) % 1001 for b in range(70)]),
    exact_case("chan_add_c192_t257", "chan_add", B=3, C=192, T=257),
    exact_case("chan_add_c96_t1", "chan_add", B=64, C=96, T=1),
    exact_case("noise_t257", "noise", B=3, T=257, noise=True),
    exact_case("noise_null_t33", "noise", B=64, T=33, noise=False),
]


def exact_inputs(c):
    g = gen(c["name"])
    k = c["kind"]
    if k == "embed":
        ids = torch.randint(0, c["V"], (c["B"], c["T"]), generator=g)
        if c["bad_ids"]:                                          # row 0: an id below 0; the last row: one at n_vocab
            ids[0, c["T"] // 2] = -1
            ids[-1, 0] = c["V"]
        return {"ids": ids, "lens": torch.tensor(c["lens"], dtype=torch.int64), "emb": torch.randn(c["V"], c["H"], generator=g)}
    if k == "gather":
        return {"table": torch.randn(c["rows"], c["C"], generator=g), "sid": torch.tensor(c["sid"], dtype=torch.int64)}
    if k == "lens":
        return {"lens": torch.tensor(c["lens"], dtype=torch.int64)}
    if k == "chan_add":
        return {"x": torch.randn(c["B"], c["C"], c["T"], generator=g), "v": torch.randn(c["B"], c["C"], generator=g)}
    return {"noise": torch.randn(c["B"], 2, c["T"], generator=g), "scale": 0.8}


def exact_expected(c, inp):
    """Bitwise expectations: gathers, masks, integers, or one correctly rounded fp32 operation."""
    k = c["kind"]
    if k == "embed":
        ids, lens, T, V = inp["ids"], inp["lens"], c["T"], c["V"]
        oob = (ids < 0) | (ids >= V)
        x = inp["emb"][torch.where(oob, torch.zeros_like(ids), ids)] * torch.tensor(math.sqrt(c["H"]), dtype=F32)
        x = x.transpose(1, 2) * tmask(lens, T, F32)[:, None, :]
        bad = (oob.any(1) | (lens < 0) | (lens > T)).to(torch.int32)
        return {"x": x.contiguous() + 0.0, "lens32": lens.clamp(0, T).to(torch.int32), "bad": bad}
    if k == "gather":
        sid = inp["sid"]
        oob = (sid < 0) | (sid >= c["rows"])
        return {"out": inp["table"][torch.where(oob, torch.zeros_like(sid), sid)], "bad": oob.to(torch.int32)}
    if k == "lens":
        lens, T = inp["lens"], c["T"]
        l32 = lens.clamp(0, T).to(torch.int32)
        return {"lens32": l32, "bad": ((lens < 0) | (lens > T)).to(torch.int32), "mask": tmask(l32, T, F32)}
    if k == "chan_add":
        return {"x": inp["x"] + inp["v"][:, :, None]}
    return {"z": inp["noise"] * torch.tensor(inp["scale"], dtype=F32) if c["noise"] else torch.zeros(c["B"], 2, c["T"])}


def exact_check(c, inp, got):
    for k, v in exact_expected(c, inp).items():
        check_exact(c["name"] + " " + k, got[k], v)
