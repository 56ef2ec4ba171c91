"""The one-shot waveform tails `istft_pqmf_kernel` / `istft_single_kernel` (csrc/istft_pqmf.hip, csrc/istft_tail.inc)
launched by themselves through `mbv_istft_pqmf`, `mbv_istft_finalize` and `mbv_op_istft_single`, and held to the
float64 reference and bars of tail_cases.py (which test_tail_refs.py proves on the CPU; its docstring lists which entry
reaches which template instantiation).  Outputs are pre-filled with NaN, every launch runs twice and must give equal
bits, and a launch without the optional outputs must give the same `o` bit for bit.  The exact-math route
(MBV_ISTFT_EXACT=1 at creation, a net of its own; the "istft_exact" option for mbv_istft_finalize) is held to the
`plain` fp32 oracle, the hardware-transcendental route to the larger of `plain` and `turns`.

MBV_TAIL_REPORT=<file>: worst err / (u A) and share of the quantile bars per output and route, as JSON
(profiles/tail_bars.json is such a run)."""
import json
import os

import pytest
import torch

import tail_cases as tc
from oracle import ref_infer as R
from test_gpu_small_ops import _nan, _twice

pytestmark = pytest.mark.gpu
STATS = {"exact": tc.Stats(), "fast": tc.Stats()}
STYLES = {"exact": ("plain",), "fast": ("plain", "turns")}
MB = [c for c in tc.TAIL_CASES if c["kind"] == "mb"]
SB = [c for c in tc.TAIL_CASES if c["kind"] == "sb"]


@pytest.fixture(scope="module")
def nets():
    from gpu_util import make_net
    out = {"fast": make_net("ljs_mini_mb_istft_vits")[0]}
    before = os.environ.pop("MBV_ISTFT_EXACT", None)
    out["fast"]._ensure_handle()                          # (a handle reads the variable when it is created)
    os.environ["MBV_ISTFT_EXACT"] = "1"
    try:
        out["exact"] = make_net("ljs_mini_mb_istft_vits")[0]
        out["exact"]._ensure_handle()
    finally:
        os.environ.pop("MBV_ISTFT_EXACT")
        if before is not None:
            os.environ["MBV_ISTFT_EXACT"] = before
    yield out
    rows = {r: {k: dict(v, headroom=v["TOL"] / v["err_over_uA"] if v["err_over_uA"] else None) for k, v in sorted(s.items())}
            for r, s in STATS.items()}
    for r, s in rows.items():
        print("\n%s route, worst err / (u A): " % r + ", ".join("%s %.3g (TOL %g)" % (k, v["err_over_uA"], v["TOL"]) for k, v in s.items()))
    path = os.environ.get("MBV_TAIL_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump({"routes": rows}, f, indent=1)


def _lib():
    from mb_istft_vits_amd import _capi
    return _capi


def _pqmf(net, c, inp, extras=True):
    """mbv_istft_pqmf for a run of tail_cases: bank, o_mb layout (bit 0) and prescaled rows (bit 1) as the run says."""
    from gpu_util import ptr
    h, B, Tp, Fr = net._ensure_handle(), c["B"], c["n"], c["F"]
    x = inp["x_pre" if c["variant"] == "pre" else "x"].cuda()
    filt = inp["filt"].cuda() if c["bank"] == "trainable" else None
    bits = (1 if c["layout"] == "ms" else 0) | (2 if c["variant"] == "pre" else 0)

    def run():
        o = {"o": _nan(B, 1, 256 * Tp)}
        if extras:
            o.update(omb=_nan(B, 4, (256 if c["layout"] == "ms" else 64) * Tp), spec=_nan(B, 4, 9, Fr), phase=_nan(B, 4, 9, Fr))
        rc = _lib().lib().mbv_istft_pqmf(h, ptr(x), B, Tp, ptr(filt), bits, ptr(o["o"]), ptr(o.get("omb")), ptr(o.get("spec")),
                                         ptr(o.get("phase")), net._stream())
        _lib().check(h, rc, "mbv_istft_pqmf")
        return {k: v.cpu() for k, v in o.items()}
    return _twice(run)


@pytest.mark.parametrize("route", ["exact", "fast"])
@pytest.mark.parametrize("base", MB, ids=lambda c: c["name"])
def test_istft_pqmf(nets, base, route):
    """FIXED x FAST x PRE of istft_pqmf_kernel, both o_mb layouts with each."""
    for bank in ("fixed", "trainable"):
        for layout in ("mb", "ms"):
            for variant in ("plain", "pre"):
                c = tc.with_variant(base, variant, bank, layout)
                inp = tc.tail_shared(c)[0]
                got = _pqmf(nets[route], c, inp)
                tc.tail_check(c, got, styles=STYLES[route], stats=STATS[route])
                tc.sc.check_exact(c["name"] + " o without the optional outputs", _pqmf(nets[route], c, inp, extras=False)["o"], got["o"])


def _single(net, c, inp, extras=True):
    from gpu_util import ptr
    h, B, Fr = net._ensure_handle(), c["B"], c["F"]
    x = inp["x_pre" if c["variant"] == "pre" else "x"].cuda()

    def run():
        o = {"o": _nan(B, 1, 4 * (Fr - 1))}
        if extras:
            o.update(spec=_nan(B, 9, Fr), phase=_nan(B, 9, Fr))
        rc = _lib().lib().mbv_op_istft_single(h, ptr(x), B, Fr, int(c["variant"] == "pre"), ptr(o["o"]), ptr(o.get("spec")),
                                              ptr(o.get("phase")), net._stream())
        _lib().check(h, rc, "mbv_op_istft_single")
        return {k: v.cpu() for k, v in o.items()}
    return _twice(run)


@pytest.mark.parametrize("route", ["exact", "fast"])
@pytest.mark.parametrize("base", SB, ids=lambda c: c["name"])
def test_istft_single(nets, base, route):
    """FAST x PRE of istft_single_kernel through mbv_op_istft_single."""
    for variant in ("plain", "pre"):
        c = tc.with_variant(base, variant)
        inp = tc.tail_shared(c)[0]
        got = _single(nets[route], c, inp)
        tc.tail_check(c, got, styles=STYLES[route], stats=STATS[route])
        tc.sc.check_exact(c["name"] + " o without the optional outputs", _single(nets[route], c, inp, extras=False)["o"], got["o"])


@pytest.mark.parametrize("cfg_name", ["ljs_mini_mb_istft_vits", "ljs_ms_istft_vits", "ljs_mini_istft_vits"])
def test_istft_finalize(cfg_name):
    """The (spec, phase) input variants through mbv_istft_finalize with the net's own synthesis bank: multi-band
    (fixed bank), multi-stream (the weight-normed trainable bank of the checkpoint) and single-band, on both routes."""
    from gpu_util import make_net, ptr
    net, sd = make_net(cfg_name)
    h = net._ensure_handle()
    sb = cfg_name == "ljs_mini_istft_vits"
    ms = cfg_name == "ljs_ms_istft_vits"
    filt = R.Weights({k: torch.from_numpy(v) for k, v in sd.items()}).w("dec.multistream_conv_post")[0].contiguous() if ms else None
    for route in ("fast", "exact"):
        rc = _lib().lib().mbv_set_option(h, b"istft_exact", int(route == "exact"))
        _lib().check(h, rc, "mbv_set_option")
        for base in (SB if sb else MB):
            c = tc.with_variant(base, "polar") if sb else tc.with_variant(base, "polar", "trainable" if ms else "fixed", "ms" if ms else "mb")
            c = dict(c, filt=filt)
            inp = tc.tail_shared(c)[0]
            spec, phase = inp["spec"].cuda(), inp["phase"].cuda()
            if sb:
                spec, phase = spec[:, 0].contiguous(), phase[:, 0].contiguous()
            B, Fr, n = c["B"], c["F"], c["n"]

            def run(extras=True):
                o = {"o": _nan(B, 1, 4 * (Fr - 1) if sb else 256 * n)}
                if extras and not sb:
                    o["omb"] = _nan(B, 4, (256 if ms else 64) * n)
                rc = _lib().lib().mbv_istft_finalize(h, ptr(spec), ptr(phase), B, Fr, ptr(o["o"]), ptr(o.get("omb")), net._stream())
                _lib().check(h, rc, "mbv_istft_finalize")
                return {k: v.cpu() for k, v in o.items()}
            got = _twice(run)
            tc.tail_check(c, got, styles=STYLES[route], stats=STATS[route])
            tc.sc.check_exact(c["name"] + " o without o_mb", run(extras=False)["o"], got["o"])


def test_op_istft_single_refusals(nets):
    from gpu_util import ptr
    net = nets["fast"]
    h, L = net._ensure_handle(), _lib().lib()
    x, o = torch.zeros(1, 18, 8, device="cuda"), _nan(1, 1, 28)
    for args, pat in (((None, 1, 8, 0, ptr(o), None, None), "NULL"), ((ptr(x), 1, 8, 0, None, None, None), "NULL"),
                      ((ptr(x), 0, 8, 0, ptr(o), None, None), "frames"), ((ptr(x), 1, 1, 0, ptr(o), None, None), "frames"),
                      ((ptr(x), 1 << 15, 1 << 12, 0, ptr(o), None, None), "2 GiB")):
        rc = L.mbv_op_istft_single(h, *args, net._stream())
        msg = L.mbv_last_error(h).decode()
        assert rc != 0 and msg.startswith("mbv_op_istft_single") and pat in msg, (args, rc, msg)
    torch.cuda.synchronize()
    assert bool(torch.isnan(o).all())
