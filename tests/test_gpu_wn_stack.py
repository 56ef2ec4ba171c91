"""The flows and the posterior encoder on every WN route, through the entry points that run them, against the float64
references and bars of wn_stack_ref.py (which test_wn_stack_refs.py proves on the CPU):

  net.align(..., outputs=("z", "z_p"), noise=N)   posterior encoder, then the forward flow; again with noise_scale = 0: m_q
  net.infer_z_only(..., durations=D)              the reverse flow z_p -> z, the row lengths = the row sums of D
  net.voice_conversion                            z -> z_p -> z_hat with two different speakers (one case)

Routes: the fused layer (wn_layer_kernel: prefold, couple with Cs = I / 2, speaker conditioning, skip_accum = 0, the
Flip folded into the packing, both signs — none of which scripts/wn_layer_check.hip reaches), as do_finalize folds it
for each size ("pre+post", "post" only, neither); and the two-launch layer (EPI_GATE, EPI_RES_SKIP split and last,
EPI_COUPLE both signs of csrc/conv1d.hip) with set_option("wn_fused", 0) and as the default route of a hidden size
the fused kernel does not cover.  Every stage is referenced from the GPU's own input to it.  The entry points
allocate their outputs themselves: torch.empty is made to hand out NaN-filled tensors while a call runs, so an
unwritten element fails; every call runs twice and must give equal bits.

MBV_WN_STACK_REPORT=<file>: the share of every bar used, per route, case and stage, as JSON
(profiles/wn_stack_bars.json is such a run)."""
import contextlib
import json
import os

import pytest
import torch

import wn_stack_ref as wr

pytestmark = pytest.mark.gpu
F32, F64 = wr.F32, wr.F64
REPORT = {}
_NETS, _ENC = {}, {}


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    _NETS.clear()
    path = os.environ.get("MBV_WN_STACK_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump({"margin": wr.MARGIN, "stats": list(wr.STAT_NAMES), "routes": REPORT}, f, indent=1, sort_keys=True)


def _net(c):
    if c["name"] not in _NETS:
        from gpu_util import make_net
        net, sd = make_net(c["cfg"], overrides=c["overrides"])
        _NETS[c["name"]] = (net, wr.Weights(sd), wr.inputs(c, spec_channels=net.cfg.spec_channels))
    return _NETS[c["name"]]


@contextlib.contextmanager
def _pinned(randn_as=None):
    """While a call runs: torch.empty hands out NaN-filled float tensors (the entry points allocate their own outputs),
    and torch.randn of the given tensor's shape returns that tensor (the draws `voice_conversion` / `infer` make)."""
    empty, randn = torch.empty, torch.randn

    def nan_empty(*a, **k):
        t = empty(*a, **k)
        return t.fill_(float("nan")) if t.is_floating_point() else t

    def pinned_randn(*a, **k):
        return randn_as if randn_as is not None and tuple(a) == tuple(randn_as.shape) else randn(*a, **k)
    torch.empty, torch.randn = nan_empty, pinned_randn
    try:
        yield
    finally:
        torch.empty, torch.randn = empty, randn


def _twice(run):
    a, b = run(), run()
    for k in a:
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), ("two calls differ", k)
    return a


def _enc_refs(c, W, cfg, inp, g, variants):
    """posterior encoder from (y, noise): float64 and the fp32 oracles, z and m_q — each once per case, for both routes"""
    if c["name"] not in _ENC:
        run = lambda dt, **k: wr.posterior_encoder(W, cfg, inp["y"], c["lens"], g, inp["noise"], dt, **k)
        _ENC[c["name"]] = dict(ref=run(F64), plain=run(F32), run=run)
    e = _ENC[c["name"]]
    for v in variants:
        if v not in e:
            e[v] = e["run"](F32, variant=v)
    return e


def _run_case(c, route):
    net, W, inp = _net(c)
    cfg, lens, fold = net.cfg, c["lens"], c["fold"]
    variants = wr.variants(c, route)
    rep = REPORT.setdefault(route, {})
    what = lambda stage: "%s/%s" % (c["name"], stage)
    cu = lambda t: None if t is None else t.cuda()
    g = W.g(inp["sid"], F64)
    x, xl, y, yl, sid = (cu(inp[k]) for k in ("x", "x_lengths", "y", "y_lengths", "sid"))

    def flows(fn, src, gg):
        """a flow stage from the GPU's own input `src`: (float64 reference, the route's fp32 oracles)"""
        ref = fn(W, cfg, src, lens, gg, F64)
        return ref, [fn(W, cfg, src, lens, gg, F32, variant=v, fold=fold) for v in variants]

    # ---- align: posterior encoder + forward flow, the noise given
    def align(noise_scale, outs):
        with _pinned():
            r = net.align(x, xl, y, yl, sid=sid, noise_scale=noise_scale, outputs=outs, noise=cu(inp["noise"]))
        z, z_p = r[4][0], r[4][1]
        assert r[0] is None and r[1] is None and r[4][2] is None                 # nothing else was asked for
        return {k: v.cpu() for k, v in (("z", z), ("z_p", z_p)) if v is not None}
    got = _twice(lambda: align(1.0, ("z", "z_p")))
    m_q = _twice(lambda: align(0.0, ("z",)))["z"]
    e = _enc_refs(c, W, cfg, inp, g, variants)
    wr.check_stage(what("align m_q"), m_q, e["ref"][1], [e[v][1] for v in variants], lens, rep)
    wr.check_stage(what("align z"), got["z"], e["ref"][0], [e[v][0] for v in variants], lens, rep)
    ref, orc = flows(wr.flow_forward, got["z"], g)
    wr.check_stage(what("align z_p"), got["z_p"], ref, orc, lens, rep)

    # ---- infer_z_only with given durations: the reverse flow
    def z_only():
        with _pinned(cu(inp["prior_noise"])):
            attn, y_mask, (z, z_p, m_p, logs_p), _ = net.infer_z_only(x, xl, sid=sid, noise_scale=0.667, durations=cu(inp["durations"]))
        return {"z": z.cpu(), "z_p": z_p.cpu(), "y_mask": y_mask.cpu(), "m_p": m_p.cpu()}
    got = _twice(z_only)
    assert got["y_mask"][:, 0].sum(1).tolist() == lens                           # the row lengths are the row sums of D
    assert not torch.equal(got["z_p"], got["m_p"])                               # noise_scale > 0: z_p is not just m_p
    ref, orc = flows(wr.flow_reverse, got["z_p"], g)
    wr.check_stage(what("infer_z_only z"), got["z"], ref, orc, lens, rep)

    # ---- voice_conversion: its own z -> z_p -> z_hat chain, source and target speakers differ (default route only:
    # the in_place oracle of the other route costs seconds per stage, and align + infer_z_only reach both signs there)
    if c["vc"] and route == c["route"]:
        def vc():
            with _pinned(cu(inp["noise"])):
                o, o_mb, y_mask, (z, z_p, z_hat) = net.voice_conversion(y, yl, sid, cu(inp["sid_tgt"]))
            assert bool(torch.isfinite(o).all())
            return {"z": z.cpu(), "z_p": z_p.cpu(), "z_hat": z_hat.cpu()}
        got = _twice(vc)
        wr.check_stage(what("vc z"), got["z"], e["ref"][0], [e[v][0] for v in variants], lens, rep)
        ref, orc = flows(wr.flow_forward, got["z"], g)
        wr.check_stage(what("vc z_p"), got["z_p"], ref, orc, lens, rep)
        ref, orc = flows(wr.flow_reverse, got["z_p"], W.g(inp["sid_tgt"], F64))
        wr.check_stage(what("vc z_hat"), got["z_hat"], ref, orc, lens, rep)


@pytest.mark.parametrize("c", wr.CASES, ids=lambda c: c["name"])
def test_default_route(c):
    """The route the library takes by itself: the fused layer wherever wn_fused_supported, else the two-launch layer."""
    _run_case(c, c["route"])


@pytest.mark.parametrize("name", wr.TWO_LAUNCH_AGAIN)
def test_two_launch(name):
    """The same cases with the option "wn_fused" off: gate conv (EPI_GATE) + res/skip conv (EPI_RES_SKIP) per layer and
    the coupling in `post` (EPI_COUPLE), held to the plain and the in_place oracle (wn_stack_ref.py)."""
    c = wr.BY_NAME[name]
    net = _net(c)[0]
    net.set_option("wn_fused", 0)
    try:
        _run_case(c, "two_launch")
    finally:
        net.set_option("wn_fused", 1)
