"""The small kernels between the convs (csrc/ops.hip, csrc/sdp.hip) and the conv + LayerNorm epilogue (EPI_LN,
csrc/conv1d_narrow.hip), each launched by itself through its `mbv_op_*` entry point and held to the float64 references
and bars of small_op_cases.py (which test_small_op_refs.py proves on the CPU).  Every output is pre-filled with NaN (a
sentinel for integers) so that an unwritten element fails; every launch runs twice and must give equal bits.

Launchers reached, by entry point: launch_embed (mbv_op_embed), launch_layernorm (mbv_op_layernorm), launch_durations
(mbv_op_durations), launch_expand with expand_kernel + attn_path_kernel (mbv_op_expand), launch_cond_gemv
(mbv_op_cond_gemv), launch_gather_rows (mbv_op_gather_rows), launch_posterior_sample (mbv_op_posterior_sample),
launch_lens_to_i32 + launch_sequence_mask (mbv_op_lens), launch_dds_sep (mbv_op_dds_sep), launch_dds_res
(mbv_op_dds_res), launch_sdp_pre (mbv_op_sdp_pre), launch_sdp_spline (mbv_op_sdp_spline), launch_sdp_logw
(mbv_op_sdp_logw), launch_sdp_noise (mbv_op_sdp_noise), launch_chan_add (mbv_op_chan_add), EPI_LN (mbv_op_conv with
MBV_CONV_EPI_LN).

MBV_SMALL_OP_REPORT=<file>: the worst err / (u A) and the largest share of the quantile bars per kernel, as JSON
(profiles/small_op_bars.json is such a run)."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import conv_cases as cc
import small_op_cases as sc

pytestmark = pytest.mark.gpu
STATS = sc.Stats()
LEFT_OUT = {}
SENTINEL = -7777


@pytest.fixture(scope="module")
def net():
    from gpu_util import make_net
    n = make_net("ljs_mini_mb_istft_vits")[0]
    yield n
    rows = {k: dict(v, headroom=v["TOL"] / v["err_over_uA"] if v["err_over_uA"] else None) for k, v in sorted(STATS.items())}
    print("\nworst err / (u A) per kernel: " + ", ".join("%s %.3g (TOL %g)" % (k, v["err_over_uA"], v["TOL"]) for k, v in rows.items()))
    path = os.environ.get("MBV_SMALL_OP_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump({"kernels": rows, "duration_tokens_left_out": LEFT_OUT}, f, indent=1)


def _nan(*shape):
    return torch.full(shape, float("nan"), device="cuda")


def _ints(*shape, dtype=torch.int32):
    return torch.full(shape, SENTINEL, device="cuda", dtype=dtype)


def _i32(v):
    return torch.as_tensor(v, dtype=torch.int32).cuda()


def _op(net, name, *args):
    """mbv_op_<name>(handle, *args, stream); tensors go as device pointers, None as NULL."""
    from mb_istft_vits_amd import _capi
    h = net._ensure_handle()
    a = [C.c_void_p(x.data_ptr()) if torch.is_tensor(x) else x for x in args]
    rc = getattr(_capi.lib(), "mbv_op_" + name)(h, *a, net._stream())
    _capi.check(h, rc, "mbv_op_" + name)


def _twice(run):
    """run() -> dict of CPU tensors, from fresh buffers each time; both runs must agree bit for bit."""
    a, b = run(), run()
    for k in a:
        x, y = a[k], b[k]
        same = torch.equal(x.view(torch.int32), y.view(torch.int32)) if x.is_floating_point() else torch.equal(x, y)
        assert same, ("two launches differ", k)
    return a


KW = dict(stats=STATS)


# ---------------------------------------------------------------------------------------------- LayerNorm, both kernels
@pytest.mark.parametrize("c", sc.LN_CASES, ids=lambda c: c["name"])
def test_layernorm(net, c):
    inp = sc.ln_inputs(c)
    d = {k: v.cuda() for k, v in inp.items()}
    lens = _i32(c["lens"]) if c["lens"] is not None else None

    def run():
        y = _nan(c["B"], c["C"], c["T"])
        _op(net, "layernorm", d["a"], d.get("r"), d["gamma"], d["beta"], y, c["B"], c["C"], c["T"], c["relu"], lens)
        return {"y": y.cpu()}
    sc.ln_check(c, inp, _twice(run), **KW)


def _conv(net, c, d, y, epi, **fields):
    """mbv_op_conv for a case of conv_cases.LN_CASES with the given epilogue and pointer fields."""
    from mb_istft_vits_amd import _capi
    dd = cc.desc(dict(c, epi=epi, ln_res=False, ln_out_lens=None, in_lens=None, out_lens=None, chan_add=False, relu=0), ws=False)
    for k in ("in_lens", "out_lens", "chan_add", "res", "res_chan_add", "accum_in", "ln_gamma", "ln_beta", "ln_out_lens"):
        setattr(dd, k, None)                                     # no placeholder pointers: only what `fields` names
    for k, v in fields.items():
        setattr(dd, k, v.data_ptr() if torch.is_tensor(v) else v)
    w = np.ascontiguousarray(d["w"].numpy(), np.float32)
    b = np.ascontiguousarray(d["bias"].numpy(), np.float32)
    out = (C.c_int32 * 8)()
    h = net._ensure_handle()
    rc = _capi.lib().mbv_op_conv(h, C.byref(dd), C.c_void_p(d["x"].data_ptr()), w.ctypes.data_as(C.c_void_p),
                                 b.ctypes.data_as(C.c_void_p), C.c_void_p(y.data_ptr()), C.byref(out), net._stream())
    _capi.check(h, rc, "mbv_op_conv")
    return _capi.ROUTES[out[0]]


@pytest.mark.parametrize("c", cc.LN_CASES, ids=lambda c: c["name"])
def test_conv_layernorm_fused_and_unfused(net, c):
    """The conv + LayerNorm of mbv_encode in one launch (EPI_LN), and the same inputs as conv (STORE) + layernorm_kernel
    with the arguments mbv_encode's unfused branch uses: both against one float64 reference."""
    inp = sc.cln_inputs(c)
    B, Cout, T = c["B"], c["Cout"], c["T"]
    d = {k: (v if k in ("w", "bias") else v.cuda()) for k, v in inp.items()}
    lens = {k: _i32(c[k]) for k in ("in_lens", "out_lens", "ln_out_lens") if c[k] is not None}
    common = {k: lens[k] for k in ("in_lens",) if k in lens}
    if c["chan_add"]:
        common["chan_add"] = d["chan_add"]

    def fused():
        y = _nan(B, Cout, T)
        f = dict(common, ln_gamma=d["gamma"], ln_beta=d["beta"], relu=c["relu"])
        if "out_lens" in lens:
            f["out_lens"] = lens["out_lens"]
        if "ln_out_lens" in lens:
            f["ln_out_lens"] = lens["ln_out_lens"]
        if c["ln_res"]:
            f["res"] = d["res"]
        assert _conv(net, c, d, y, "LN", **f) == "NARROW_M"
        return {"y": y.cpu()}

    def unfused():
        conv, y = _nan(B, Cout, T), _nan(B, Cout, T)
        f = dict(common)
        if "out_lens" in lens:
            f["out_lens"] = lens["out_lens"]
        _conv(net, c, d, conv, "STORE", **f)                      # (relu stays with the LayerNorm kernel, as in mbv_encode)
        if c["ln_res"]:                                           # launch_layernorm(x, y, ...): the residual is `a`, the conv `r`
            _op(net, "layernorm", d["res"], conv, d["gamma"], d["beta"], y, B, Cout, T, 0, lens.get("ln_out_lens"))
        else:
            _op(net, "layernorm", conv, None, d["gamma"], d["beta"], y, B, Cout, T, c["relu"], None)
        return {"y": y.cpu()}

    sc.cln_check(c, inp, _twice(fused), **KW)
    sc.cln_check(dict(c, name=c["name"] + " (unfused)"), inp, _twice(unfused), **KW)


# ---------------------------------------------------------------------------------------------- DDSConv halves
@pytest.mark.parametrize("c", sc.DDS_CASES, ids=lambda c: c["name"])
def test_dds_halves(net, c):
    inp = sc.dds_inputs(c)
    d = {k: v.cuda() for k, v in inp.items()}
    B, Cn, T = c["B"], c["C"], c["T"]
    lens = _i32(c["lens"])

    def sep():
        y = _nan(B, Cn, T)
        _op(net, "dds_sep", d["x"], lens, d["w"], d["bias"], d["g1"], d["b1"], y, B, Cn, T, 3, c["dil"])
        return {"y": y.cpu()}

    def res():                                                   # in place on the residual, as run_dds calls it
        x = d["xres"].clone()
        _op(net, "dds_res", d["a"], x, d["g2"], d["b2"], x, B, Cn, T, lens if c["out_lens"] else None)
        return {"y": x.cpu()}

    def res_out_of_place():
        y = _nan(B, Cn, T)
        _op(net, "dds_res", d["a"], d["xres"], d["g2"], d["b2"], y, B, Cn, T, lens if c["out_lens"] else None)
        return {"y": y.cpu()}

    sc.dds_sep_check(c, inp, _twice(sep), **KW)
    r = _twice(res)
    sc.dds_res_check(c, inp, r, **KW)
    sc.check_exact(c["name"] + " in place == out of place", r["y"], res_out_of_place()["y"])


# ---------------------------------------------------------------------------------------------- spline
@pytest.mark.parametrize("c", sc.SPLINE_CASES, ids=lambda c: c["name"])
def test_sdp_spline(net, c):
    inp = sc.spline_inputs(c)
    h, lens = inp["h"].cuda(), _i32(c["lens"])

    def run():
        z = inp["z"].cuda()                                      # in place, as mbv_encode runs it
        _op(net, "sdp_spline", h, z, lens, c["B"], c["C"], c["T"], C.c_float(sc.EDGE_CONST))
        z = z.cpu()
        return {"z0": z[:, 0].contiguous(), "z1": z[:, 1].contiguous()}
    sc.spline_check(c, inp, _twice(run), **KW)


# ---------------------------------------------------------------------------------------------- durations, expansion
def _durations(net, c, inp):
    B, T = c["B"], c["T"]
    d = {k: v.cuda() for k, v in inp.items()}
    lens = _i32(c["lens"])

    def run():
        logw, wc = _nan(B, T), _nan(B, T)
        cum, y32, y64 = _ints(B, T), _ints(B), _ints(B, dtype=torch.int64)
        _op(net, "durations", d["h"], d.get("w"), d.get("bias"), lens, C.c_float(c["ls"]), logw, wc, cum, y32, y64,
            d["bad"], B, c["C"], T)
        return {"logw": logw.cpu(), "w_ceil": wc.cpu(), "cum": cum.cpu(), "ylen32": y32.cpu(), "ylen64": y64.cpu()}
    return _twice(run)


@pytest.mark.parametrize("c", sc.DUR_CASES, ids=lambda c: c["name"])
def test_durations(net, c):
    inp = sc.dur_inputs(c)
    LEFT_OUT[c["name"]] = sc.dur_check(c, inp, _durations(net, c, inp), **KW)


def test_durations_without_the_optional_outputs(net):
    """ylen64 and bad null (as a caller that does not want y_lengths): the rest is unchanged."""
    c = sc.DUR_BY_NAME["dur_sdp_t257_ls1"]
    inp = sc.dur_inputs(c)
    full = _durations(net, c, inp)
    B, T = c["B"], c["T"]
    logw, wc, cum, y32 = _nan(B, T), _nan(B, T), _ints(B, T), _ints(B)
    _op(net, "durations", inp["h"].cuda(), None, None, _i32(c["lens"]), C.c_float(c["ls"]), logw, wc, cum, y32, None, None,
        B, 1, T)
    for k, v in (("logw", logw), ("w_ceil", wc), ("cum", cum), ("ylen32", y32)):
        sc.check_exact(k, v.cpu(), full[k])


@pytest.mark.parametrize("c", sc.EXP_CASES, ids=lambda c: c["name"])
def test_expand(net, c):
    inp = sc.exp_inputs(c)
    B, T, I, Tp = inp["cum"].shape[0], inp["cum"].shape[1], c["I"], inp["Tp"]
    stats, cum, ylen = inp["stats"].cuda(), inp["cum"].cuda(), inp["ylen"].cuda()
    noise = inp["noise"].cuda() if c["noise"] else None

    def run():
        o = {"z": _nan(B, I, Tp)}
        if c["outs"]:
            o.update(m_p=_nan(B, I, Tp), logs_p=_nan(B, I, Tp), z_p=_nan(B, I, Tp), attn=_nan(B, Tp, T), y_mask=_nan(B, Tp))
        _op(net, "expand", stats, cum, ylen, noise, C.c_float(inp["noise_scale"]), o.get("m_p"), o.get("logs_p"),
            o.get("z_p"), o["z"], o.get("attn"), o.get("y_mask"), B, I, T, Tp)
        return {k: v.cpu() for k, v in o.items()}
    sc.exp_check(c, inp, _twice(run), **KW)


# ---------------------------------------------------------------------------------------------- GEMV, pre, logw, posterior
@pytest.mark.parametrize("c", sc.LIN_CASES, ids=lambda c: c["name"])
def test_linear_pieces(net, c):
    inp = sc.lin_inputs(c)
    d = {k: v.cuda() for k, v in inp.items()}
    k = c["kind"]

    def run():
        if k == "cond_gemv":
            y = _nan(c["B"], c["Cout"])
            _op(net, "cond_gemv", d["g"], d["W"], d.get("bias"), y, c["B"], c["Cin"], c["Cout"])
        elif k == "sdp_pre":
            y = _nan(c["B"], c["C"], c["T"])
            _op(net, "sdp_pre", d["z"], c["zc"], d["pre_w"], d["pre_b"], d["cond"], y, c["B"], c["C"], c["T"])
        elif k == "sdp_logw":
            y = _nan(c["B"], c["T"])
            _op(net, "sdp_logw", d["z"], d["m"], d["logs"], _i32(c["lens"]), y, c["B"], c["T"])
        else:
            y = _nan(c["B"], c["I"], c["T"])
            _op(net, "posterior_sample", d["stats"], d.get("noise"), _i32(c["lens"]), y, c["B"], c["I"], c["T"])
        return {"y": y.cpu()}
    sc.lin_check(c, inp, _twice(run), **KW)


# ---------------------------------------------------------------------------------------------- the exact ones
@pytest.mark.parametrize("c", sc.EXACT_CASES, ids=lambda c: c["name"])
def test_exact_pieces(net, c):
    inp = sc.exact_inputs(c)
    d = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in inp.items()}
    k, B = c["kind"], c["B"]

    def run():
        if k == "embed":
            x, l32, bad = _nan(B, c["H"], c["T"]), _ints(B), _ints(B)
            _op(net, "embed", d["ids"], d["lens"], d["emb"], x, l32, bad, B, c["T"], c["H"], c["V"])
            return {"x": x.cpu(), "lens32": l32.cpu(), "bad": bad.cpu()}
        if k == "gather":
            out, bad = _nan(B, c["C"]), torch.zeros(B, dtype=torch.int32, device="cuda")     # (set, never cleared)
            _op(net, "gather_rows", d["table"], d["sid"], out, B, c["C"], c["rows"], bad)
            return {"out": out.cpu(), "bad": bad.cpu()}
        if k == "lens":
            l32, bad, mask = _ints(B), _ints(B), _nan(B, c["T"])
            _op(net, "lens", d["lens"], l32, bad, mask, B, c["T"])
            return {"lens32": l32.cpu(), "bad": bad.cpu(), "mask": mask.cpu()}
        if k == "chan_add":
            x = d["x"].clone()
            _op(net, "chan_add", x, d["v"], B, c["C"], c["T"])
            return {"x": x.cpu()}
        z = _nan(B, 2, c["T"])
        _op(net, "sdp_noise", d["noise"] if c["noise"] else None, C.c_float(d["scale"]), z, C.c_int64(B * 2 * c["T"]))
        return {"z": z.cpu()}
    sc.exact_check(c, inp, _twice(run))


def test_gather_rows_without_the_flags(net):
    c = next(x for x in sc.EXACT_CASES if x["name"] == "gather_c256")
    inp = sc.exact_inputs(c)
    out = _nan(c["B"], c["C"])
    _op(net, "gather_rows", inp["table"].cuda(), inp["sid"].cuda(), out, c["B"], c["C"], c["rows"], None)
    sc.check_exact("out", out.cpu(), sc.exact_expected(c, inp)["out"])


# ---------------------------------------------------------------------------------------------- refusals
def test_error_paths_leave_the_handle_usable(net):
    """Arguments an entry refuses before it launches anything: a message, nothing written, and the next call works."""
    from mb_istft_vits_amd import _capi
    L, h, s = _capi.lib(), net._ensure_handle(), net._stream()
    x = _nan(2, 256, 8)
    p = C.c_void_p(x.data_ptr())
    i = C.c_void_p(_ints(64).data_ptr())
    f1 = C.c_float(1.0)
    bad = [
        ("embed", (p, p, p, p, i, i, 2, 8, 0, 59), "> 0"), ("embed", (None, p, p, p, i, i, 2, 8, 96, 59), "NULL"),
        ("layernorm", (p, None, p, p, p, 2, 257, 8, 0, None), r"\[1, 256\]"), ("layernorm", (p, None, p, p, p, 2, 0, 8, 0, None), r"\[1, 256\]"),
        ("layernorm", (p, None, None, p, p, 2, 96, 8, 0, None), "NULL"), ("layernorm", (p, None, p, p, p, 0, 96, 8, 0, None), "B in"),
        ("durations", (p, p, None, i, f1, p, p, i, i, None, None, 2, 256, 8), "together"),
        ("durations", (p, None, None, i, f1, p, p, i, i, None, None, 2, 256, 8), "C must be"),
        ("durations", (p, None, None, i, C.c_float(0.0), p, p, i, i, None, None, 2, 1, 8), "length_scale"),
        ("durations", (p, None, None, i, C.c_float(float("nan")), p, p, i, i, None, None, 2, 1, 8), "length_scale"),
        ("expand", (p, i, i, None, f1, None, None, None, None, None, None, 2, 4, 8, 8), "NULL"),
        ("expand", (p, i, i, None, f1, None, None, None, p, None, None, 2, 4, 8, 70000), "65535"),
        ("cond_gemv", (p, p, None, p, 2, 0, 8), "> 0"), ("gather_rows", (p, i, p, 2, 8, 0, None), "> 0"),
        ("posterior_sample", (p, None, None, p, 2, 4, 8), "NULL"), ("lens", (i, i, None, None, 2, 8), "NULL"),
        ("dds_sep", (p, i, p, p, p, p, x[1:].data_ptr(), 1, 257, 8, 3, 1), r"\[1, 256\]"),
        ("dds_sep", (p, i, p, p, p, p, x[1:].data_ptr(), 1, 96, 8, 5, 1), "K = 3"),
        ("dds_sep", (p, i, p, p, p, p, x[1:].data_ptr(), 1, 96, 8, 3, 2), "dil in"),
        ("dds_sep", (p, i, p, p, p, p, p, 1, 96, 8, 3, 1), "must not be x"),
        ("dds_res", (p, p, p, p, p, 2, 300, 8, None), r"\[1, 256\]"),
        ("sdp_pre", (p, 2, p, p, p, p, 2, 96, 8), "zc"), ("sdp_spline", (p, p, None, 2, 96, 8, f1), "NULL"),
        ("sdp_spline", (p, p, i, 2, 0, 8, f1), "> 0"), ("sdp_logw", (p, p, p, i, None, 2, 8), "NULL"),
        ("sdp_noise", (None, f1, p, C.c_int64(0)), "n must"), ("sdp_noise", (None, f1, None, C.c_int64(8)), "NULL"),
        ("chan_add", (p, p, 2, 70000, 8), "65535"),
    ]
    import re
    for name, args, pat in bad:
        rc = getattr(L, "mbv_op_" + name)(h, *args, s)
        msg = L.mbv_last_error(h).decode()
        assert rc != 0 and msg.startswith("mbv_op_" + name) and re.search(pat, msg), (name, args, rc, msg)
    torch.cuda.synchronize()
    assert bool(torch.isnan(x).all())                            # nothing was launched
    # EPI_LN descriptors that the narrow kernel does not cover are refused by mbv_op_conv as by mbv_conv_plan
    c = cc.LN_BY_NAME["ln_conv_o_h96_t33"]
    inp = sc.cln_inputs(c)
    d = {k: (v if k in ("w", "bias") else v.cuda()) for k, v in inp.items()}
    y = _nan(c["B"], c["Cout"], c["T"])
    with pytest.raises(_capi.MbvError, match="ln_gamma"):
        _conv(net, c, d, y, "LN", res=d["res"])
    with pytest.raises(_capi.MbvError, match="T <= 256"):
        _conv(net, dict(c, T=300, Tin=300), d, y, "LN", res=d["res"], ln_gamma=d["gamma"], ln_beta=d["beta"])
    assert bool(torch.isnan(y).all())
    # the handle still works
    c = sc.LN_CASES[0]
    inp = sc.ln_inputs(c)
    out = _nan(c["B"], c["C"], c["T"])
    _op(net, "layernorm", inp["a"].cuda(), None, inp["gamma"].cuda(), inp["beta"].cuda(), out, c["B"], c["C"], c["T"], 0, None)
    sc.ln_check(c, inp, {"y": out.cpu()})
