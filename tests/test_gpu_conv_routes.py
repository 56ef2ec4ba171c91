"""Every route and epilogue of the conv launcher (`launch_conv1d`, conv1d.hip) against a float64 reference, element
by element, through `mbv_op_conv` (the decoder's own launcher and weight packers).  The case table is conv_cases.py
(its routes are pinned on the CPU by test_conv_plan.py).

Bar: |y - y64| <= tol * A + 1e-7, A = the same operation in float64 on |W|, |act(x)|, |bias|, |res + res_chan_add|,
|accum_in| and |out_scale| (tol 1e-5 exact fp32, 6e-5 split-bf16).  Large launches are checked on a subset of
utterances (first, last, both sides of the batch cut, the virtual-sequence seams) and of output channels (tile and
packing seams); every row of them must equal, bitwise, the same rows launched two at a time on another route."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_cases as cc

pytestmark = pytest.mark.gpu
SPLITK = os.environ.get("MBV_CONV_SPLITK", "0") not in ("", "0")
TOL = {0: 1e-5, 3: 6e-5}
WORST = {}                 # matrix row -> worst err / A seen (printed at the end, MBV_CONV_ROUTE_REPORT: JSON file)


@pytest.fixture(scope="module")
def net():
    from gpu_util import make_net
    n = make_net("ljs_mini_mb_istft_vits")[0]
    yield n
    rows = sorted(WORST.items())
    print("\nworst err / A per route: " + ", ".join("%s %.3g" % kv for kv in rows))
    path = os.environ.get("MBV_CONV_ROUTE_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump(dict(rows), f, indent=1)


def _inputs(c):
    """Seeded fp32 inputs of a case (CPU tensors) and the reference-layout weights."""
    g = torch.Generator().manual_seed(1000 + c["seed"])
    B, Cin, Cout, T, Tin = c["B"], c["Cin"], c["Cout"], c["T"], c["Tin"]
    rs = c["rstride"] or Tin
    t = {"x": torch.randn(B, Cin, rs, generator=g)}
    if c["kind"] == "conv":
        wshape, Tout = (Cout, Cin, c["K"]), T
    else:
        wshape, Tout = (Cin, Cout, 16), c["kind"] * T
    t["w"] = torch.randn(*wshape, generator=g) / float(np.sqrt(Cin * wshape[2] / (1 if c["kind"] == "conv" else c["kind"])))
    t["bias"] = 0.5 * torch.randn(Cout, generator=g)
    if c["chan_add"]:
        t["chan_add"] = 0.5 * torch.randn(B, Cin, generator=g)
    if c["epi"] != "STORE":
        t["res"] = torch.randn(B, Cout, T, generator=g)
    if c["res_chan_add"]:
        t["res_chan_add"] = 0.5 * torch.randn(B, Cout, generator=g)
    if c["accum"]:
        t["accum"] = torch.randn(B, Cout, T, generator=g)
    for k in ("in_lens", "out_lens"):
        if c[k] is not None:
            t[k] = torch.tensor(c[k], dtype=torch.int32)
    t["Tout"] = Tout
    return t


def _launch(net, c, t, rows=None, splitk=None, prec=None, trim=True, stream=None, y_init=None):
    """mbv_op_conv on rows [lo, hi) of the case's inputs; returns (y on the CPU, plan)."""
    from gpu_util import ptr
    from mb_istft_vits_amd import _capi
    lo, hi = rows or (0, c["B"])
    dev = {k: t[k][lo:hi].contiguous().cuda() for k in ("x", "chan_add", "res", "res_chan_add", "in_lens", "out_lens")
           if k in t}
    if y_init is not None:
        y = y_init[lo:hi].contiguous().cuda()
    elif "accum" in t:                                   # the running sum in place, as the decoder runs it
        y = t["accum"][lo:hi].contiguous().cuda()
    else:
        y = torch.full((hi - lo, c["Cout"], t["Tout"]), float("nan"), device="cuda")
    ptrs = {k: dev[k].data_ptr() for k in ("in_lens", "out_lens", "chan_add", "res", "res_chan_add") if k in dev}
    if "accum" in t:
        ptrs["accum_in"] = y.data_ptr()
    cr = dict(c, B=hi - lo)
    if c["trim"]:
        cr["trim"] = (c["trim"][0], c["trim"][1], c["trim"][2][lo:hi])
    d = cc.desc(cr, ptrs=ptrs, splitk=splitk, prec=prec, trim=trim, ws=False)
    w = np.ascontiguousarray(t["w"].numpy(), np.float32)
    b = np.ascontiguousarray(t["bias"].numpy(), np.float32)
    out = (C.c_int32 * 8)()
    h = net._ensure_handle()
    s = C.c_void_p(stream.cuda_stream) if stream is not None else net._stream()
    rc = _capi.lib().mbv_op_conv(h, C.byref(d), ptr(dev["x"]), w.ctypes.data_as(C.c_void_p),
                                 b.ctypes.data_as(C.c_void_p), ptr(y), C.byref(out), s)
    _capi.check(h, rc, "mbv_op_conv")
    p = dict(zip(_capi.PLAN_FIELDS, list(out)))
    p["route"] = _capi.ROUTES[p["route"]]
    return y.cpu(), p


def _channels(c):
    if c["kind"] == "conv":
        sel = [0, 31, 32, 63, 64, 127, c["Cout"] - 1]
    else:                                                # 64-row packing groups: 64 / U channels x two phase halves
        g = 64 // c["kind"]
        sel = [0, g - 1, g, 2 * g - 1, c["Cout"] - g, c["Cout"] - 1]
    return sorted({v for v in sel if 0 <= v < c["Cout"]})


def _utterances(c, plan):
    B = c["B"]
    if B <= 4:
        return list(range(B))
    sel = {0, 1, B - 1}
    if plan["nb_big"]:
        sel |= {plan["nb_big"] - 1, plan["nb_big"]}
    if plan["vs_tv"]:
        tv = plan["vs_tv"]
        cross = [b for b in range(B) if (b * tv) // 384 != (b * tv + c["T"] - 1) // 384]
        sel |= {cross[0], cross[len(cross) // 2]}
        last = (B * tv - 1) // 384 * 384                 # first column of the last (ragged) virtual tile
        sel.add(min(b for b in range(B) if b * tv + c["T"] > last))
    for k in ("in_lens", "out_lens"):
        if c[k] is not None:
            sel |= {b for b, v in enumerate(c[k]) if v in (0, 1)}
    if c["trim"]:
        sel |= {b for b, v in enumerate(c["trim"][2]) if v in (0, 128, 384)}
    return sorted(sel)


def _reference(c, t, utts, chans):
    """float64 result and magnitude bound A on [utts, chans, :]."""
    d = torch.float64
    U = c["kind"] if c["kind"] != "conv" else 1
    x = t["x"][utts, :, :c["Tin"]].to(d)
    if c["chan_add"]:
        x = x + t["chan_add"][utts].to(d)[:, :, None]
    if c["in_lens"] is not None:
        lens = torch.tensor([c["in_lens"][b] for b in utts])
        x = x * (torch.arange(c["Tin"])[None, :] < lens[:, None]).to(d)[:, None, :]
    act = F.leaky_relu(x, c["slope"])
    bias = t["bias"][chans].to(d)
    if c["kind"] == "conv":
        if c["reflect1"]:
            act = torch.cat([act[:, :, 1:2], act], dim=2)
        halo = (c["K"] - 1) * c["dil"]
        pl = halo // 2
        act = F.pad(act, (pl, max(0, c["T"] + halo - pl - act.shape[2])))
        w = t["w"][chans].to(d)
        y = F.conv1d(act, w, dilation=c["dil"])[:, :, :c["T"]]
        A = F.conv1d(act.abs(), w.abs(), dilation=c["dil"])[:, :, :c["T"]]
    else:
        w = t["w"][:, chans].to(d)
        y = F.conv_transpose1d(act, w, stride=U, padding=(16 - U) // 2)
        A = F.conv_transpose1d(act.abs(), w.abs(), stride=U, padding=(16 - U) // 2)
    y = y + bias[None, :, None]
    A = A + bias.abs()[None, :, None]
    if c["epi"] == "STORE":
        if c["relu"]:
            y = y.clamp_min(0)
        if c["out_lens"] is not None:
            lens = torch.tensor([c["out_lens"][b] for b in utts])
            m = (torch.arange(c["T"])[None, :] < lens[:, None]).to(d)[:, None, :]
            y, A = y * m, A * m
    else:
        r = t["res"][utts][:, chans].to(d)
        if c["res_chan_add"]:
            r = r + t["res_chan_add"][utts][:, chans].to(d)[:, :, None]
        y, A = y + r, A + r.abs()
        if c["epi"] == "RESID_ACC":
            if c["accum"]:
                acc = t["accum"][utts][:, chans].to(d)
                y, A = y + acc, A + acc.abs()
            y, A = y * c["out_scale"], A * abs(c["out_scale"])
    return y, A


def _check(c, t, y, plan, prec, key, cols=None):
    utts, chans = _utterances(c, plan), _channels(c)
    y64, A = _reference(c, t, utts, chans)
    got = y[utts][:, chans].to(torch.float64)
    if cols is not None:                                  # trimmed: per utterance, the columns below its limit
        m = torch.zeros_like(got, dtype=torch.bool)
        for i, b in enumerate(utts):
            m[i, :, :cols[b]] = True
        got, y64, A = got[m], y64[m], A[m]
    err = (got - y64).abs()
    bar = TOL[prec] * A + 1e-7
    assert bool(torch.isfinite(got).all()), c["name"]
    ratio = float((err / A.clamp_min(1e-30)).max()) if err.numel() else 0.0
    WORST[key] = max(WORST.get(key, 0.0), ratio)
    bad = err > bar
    assert not bool(bad.any()), (c["name"], key, int(bad.sum()), float(err.max()), ratio)
    if c["out_lens"] is not None:                         # masked positions: exactly 0 on every row
        for b, v in enumerate(c["out_lens"]):
            assert bool((y[b, :, v:] == 0).all()), (c["name"], b, v)


def _same(a, b):
    if not SPLITK or a.numel() == 0:
        return torch.equal(a, b)
    return float((a - b).abs().max()) <= 2e-5 * max(float(b.abs().max()), 1e-3)


@pytest.mark.parametrize("c", cc.CASES, ids=lambda c: c["name"])
def test_conv_route(net, c):
    t = _inputs(c)
    y, plan = _launch(net, c, t, trim=False)
    if not SPLITK or c["splitk"]:                          # (MBV_CONV_SPLITK moves the other cases off their route)
        assert plan["route"] == c["route"], (c["name"], plan)
        if c["S_gt1"]:
            assert plan["S"] > 1, plan
    key = cc.cell_route(dict(c, trim=None)) if not SPLITK else "splitk:" + ("PREC3_" if c["prec"] else "") + plan["route"]
    _check(c, t, y, plan, c["prec"], key)

    if c["trim"]:                                          # the compact tile list: same values below each limit
        num, add, lens = c["trim"]
        y_t, p_t = _launch(net, c, t, trim=True)
        assert p_t["bn"] in (128, 384) and p_t["route"] == c["route"], p_t
        U = c["kind"] if c["kind"] != "conv" else 1
        cols = [U * max(0, min(c["T"], v * num + add)) for v in lens]
        for b, n in enumerate(cols):
            assert _same(y_t[b, :, :n], y[b, :, :n]), (c["name"], b, n)
        _check(c, t, y_t, p_t, c["prec"], cc.cell_route(c), cols=cols)

    if c["pair"]:                                          # every row again, two utterances per launch
        for lo in range(0, c["B"], 2):
            hi = min(lo + 2, c["B"])
            y2, p2 = _launch(net, c, t, rows=(lo, hi))
            if not SPLITK:
                assert p2["route"] == c["pair_route"], (c["name"], p2)
            assert _same(y2, y[lo:hi]), (c["name"], lo, plan["route"], p2["route"])


def test_conv_route_on_a_caller_stream(net):
    """mbv_op_conv enqueues on the stream it is given: a fresh non-default stream gives the default stream's bits."""
    c = cc.BY_NAME["split_resid_cond"]
    t = _inputs(c)
    y0, p0 = _launch(net, c, t)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        y1, p1 = _launch(net, c, t, stream=s)
    assert p1 == p0
    assert torch.equal(y1, y0)
