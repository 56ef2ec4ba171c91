"""Row-exact ragged decode on the MI355X: every row of `net.dec(z, g, lengths=...)` / `infer(..., ragged=True)` is
bitwise its stand-alone decode (`mbv_decode_ragged`, `mbv_synthesize_ragged`)."""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

from mb_istft_vits_amd import _capi, synth, wire
from oracle import ref_infer

from gpu_util import make_net, ptr
from helpers import rms

pytestmark = pytest.mark.gpu

RB2 = {"resblock": "2", "resblock_dilation_sizes": [[1, 3], [1, 3], [1, 3]]}
CASES = [("ljs_mini_mb_istft_vits", None), ("ljs_ms_istft_vits", None), ("uudb_ms_istft_vits_ms", None),
         ("ljs_mini_istft_vits", None), ("ljs_mini_mb_istft_vits", RB2)]
IDS = ["mini_mb", "ms", "uudb", "sb", "rb2"]
T_MAX = 300
_NETS = {}


def _net(name, overrides=None):
    key = (name, repr(overrides))
    if key not in _NETS:
        _NETS[key] = make_net(name, overrides=overrides)
    return _NETS[key]


def _z(net, B, Tp, seed):
    return torch.randn(B, net.cfg.inter_channels, Tp, generator=torch.Generator().manual_seed(seed)).cuda()


def _g(net, B, seed):
    if not net.cfg.gin_channels:
        return None
    return (0.3 * torch.randn(B, net.cfg.gin_channels, 1, generator=torch.Generator().manual_seed(seed))).cuda()


def _lengths(net):
    """Both sides of every class cut, 1, a mid-class value of the first and of a later class, T'."""
    first = net.ragged_classes(T_MAX)
    lens = [T_MAX, 1, 9, 41]
    for f in first[1:]:
        lens += [f, f - 1]
    lens = sorted(set(lens), reverse=True)
    classes = {max(i for i, f in enumerate(first) if f <= n) for n in lens}
    assert len(classes) >= 2 and len(classes) == len(first), (first, lens)
    # not sorted in the batch: the gather and the output placement must not rely on an order
    return lens[1::2] + lens[0::2]


def _alone(net, z, g, lens):
    return [net.dec(z[b:b + 1, :, :n].contiguous(), None if g is None else g[b:b + 1])[0][0, 0].clone()
            for b, n in enumerate(lens)]


def _check_rows(o, alone, lens, spf, tag):
    assert o.shape == (len(lens), 1, spf * T_MAX)
    for b, n in enumerate(lens):
        assert torch.equal(o[b, 0, :spf * n], alone[b]), (tag, b, n, float((o[b, 0, :spf * n] - alone[b]).abs().max()))
        assert not bool(o[b, 0, spf * n:].any()), (tag, b, n)


@pytest.mark.timeout(900)
@pytest.mark.parametrize("name,overrides", CASES, ids=IDS)
def test_rows_are_bitwise_their_standalone_decode(name, overrides):
    net, sd = _net(name, overrides)
    spf = net.cfg.samples_per_frame
    lens = _lengths(net)
    B = len(lens)
    z, g = _z(net, B, T_MAX, 3), _g(net, B, 4)
    for b, n in enumerate(lens):
        z[b, :, n:] = 0
    alone = _alone(net, z, g, lens)
    o, o_mb, spec, phase = net.dec(z, g=g, lengths=lens)
    assert o_mb is None and spec is None and phase is None
    _check_rows(o, alone, lens, spf, "zeros")
    # the default decode of the same batch is NOT that (the unmasked decoder leaks across a row's end)
    d = net.dec(z, g)[0]
    differ = [b for b, n in enumerate(lens) if n < T_MAX and not torch.equal(d[b, 0, :spf * n], alone[b])]
    assert len(differ) == B - 1, (differ, lens)
    # nothing at or behind a row's end is read
    for fill in (float("nan"), 1e30):
        zf = z.clone()
        for b, n in enumerate(lens):
            zf[b, :, n:] = fill
        _check_rows(net.dec(zf, g=g, lengths=torch.tensor(lens))[0], alone, lens, spf, fill)
    # ... nor is stale scratch: a longer, fuller batch through the arena first
    net.dec(_z(net, B + 2, T_MAX + 40, 5), _g(net, B + 2, 6))
    _check_rows(net.dec(z, g=g, lengths=torch.tensor(lens).cuda())[0], alone, lens, spf, "after a longer batch")
    # a batch in one class only (one decoder run): the rows of the last class
    top = [b for b, n in enumerate(lens) if n >= net.ragged_classes(T_MAX)[-1]]
    assert len(top) >= 2
    zt, gt = z[top].contiguous(), None if g is None else g[top].contiguous()
    _check_rows(net.dec(zt, g=gt, lengths=[lens[b] for b in top])[0], [alone[b] for b in top], [lens[b] for b in top], spf,
                "one class")
    # lengths of zero
    l0 = [0 if b % 3 == 0 else n for b, n in enumerate(lens)]
    o0 = net.dec(z, g=g, lengths=l0)[0]
    for b, n in enumerate(l0):
        assert torch.equal(o0[b, 0, :spf * n], alone[b][:spf * n]) if n == lens[b] else not bool(o0[b].any())
        assert not bool(o0[b, 0, spf * n:].any())
    # the project's waveform bar against the oracle's stand-alone decode, row by row
    worst = 0.0
    for b, n in enumerate(lens):
        with torch.no_grad():
            ro = ref_infer.decode(sd, net.cfg, z[b:b + 1, :, :n].cpu(), None if g is None else g[b:b + 1].cpu())[0]
        err = rms(o[b, 0, :spf * n].cpu().numpy() - ro[0, 0].numpy())
        worst = max(worst, err)
        assert err <= 1e-4, (name, n, err)
    print("%s: %d rows in %d classes, worst RMS against the oracle %.2e" % (name, B, len(net.ragged_classes(T_MAX)), worst))


def _batch(net, B, T, seed):
    x, xl, sid = synth.synthetic_batch(net.cfg, B, T, seed=seed, ragged=True)
    xl[0] = max(3, T // 6)
    return (torch.from_numpy(x).cuda(), torch.from_numpy(xl).cuda(),
            torch.from_numpy(sid).cuda() if sid is not None else None)


def _rows_of_infer(net, z, yl, sid):
    out = []
    for b in range(z.shape[0]):
        g = net.emb_g(sid[b:b + 1]).unsqueeze(-1) if sid is not None else None
        out.append(net.dec(z[b:b + 1, :, :int(yl[b])].contiguous(), g)[0])
    return out


@pytest.mark.timeout(900)
@pytest.mark.parametrize("name,kw", [("ljs_mini_mb_istft_vits", dict(noise_scale=0.667)),
                                     ("uudb_ms_istft_vits_ms", dict(noise_scale=0.5, max_len=70)),
                                     ("ljs_mini_istft_vits", dict(noise_scale=0.3, length_scale=1.2))],
                         ids=["mini_mb", "uudb_maxlen", "sb"])
def test_infer_ragged(name, kw):
    net, _ = _net(name)
    spf = net.cfg.samples_per_frame
    x, xl, sid = _batch(net, 6, 40, 12)
    (o, o_mb, spec, phase, _, _, (z, *_), _), yl = net.infer_with_lengths(x, xl, sid, outputs=("o", "z"), ragged=True, **kw)
    assert o_mb is None and spec is None and phase is None
    Td = o.shape[-1] // spf
    yl = yl.clamp(max=Td)
    assert int(yl.min()) < int(yl.max())
    rows = _rows_of_infer(net, z, yl, sid)
    for b, r in enumerate(rows):
        n = spf * int(yl[b])
        assert torch.equal(o[b, 0, :n], r[0, 0]), (name, b)
        assert not bool(o[b, 0, n:].any())
    # the default call differs on the rows that have a longer batch-mate
    torch.manual_seed(1)
    d = net.infer(x, xl, sid, outputs=("o",), **dict(kw, noise_scale=0))[0]
    torch.manual_seed(1)
    (r0, *_), _ = net.infer_with_lengths(x, xl, sid, outputs=("o",), ragged=True, **dict(kw, noise_scale=0))
    short = int(yl.argmin())
    n = spf * int(yl[short])
    assert not torch.equal(d[short, 0, :n], r0[short, 0, :n])
    # infer -> service_pcm16 in the mode = the same chain on per-row B = 1 calls fed that call's z rows
    pcm, valid = wire.service_pcm16(net, o, yl, 22050, 24000)
    for b, r in enumerate(rows):
        p1, v1 = wire.service_pcm16(net, r, yl[b:b + 1], 22050, 24000)
        assert int(v1[0]) == int(valid[b])
        assert torch.equal(pcm[b, :int(valid[b])], p1[0, :int(v1[0])]), (name, b)


def _count_syncs(fn):
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            fn()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    return sum("synchroniz" in str(v.message).lower() for v in w)


def test_infer_ragged_adds_no_host_synchronisation():
    net, _ = _net("ljs_mini_mb_istft_vits")
    x, xl, sid = _batch(net, 5, 30, 2)
    net.infer(x, xl, sid, outputs=("o",), ragged=True)                      # (first-call allocations)
    n_default = _count_syncs(lambda: net.infer(x, xl, sid, outputs=("o",)))
    n_ragged = _count_syncs(lambda: net.infer(x, xl, sid, outputs=("o",), ragged=True))
    print("host synchronisations per infer: default %d, ragged %d" % (n_default, n_ragged))
    assert n_default == 1                                                    # the debug mode sees the one read-back
    assert n_ragged == 1


def test_side_stream_and_interleaved_calls():
    net, _ = _net("ljs_mini_mb_istft_vits")
    spf = net.cfg.samples_per_frame
    lens = _lengths(net)
    z = _z(net, len(lens), T_MAX, 8)
    ref = net.dec(z, lengths=lens)[0].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        out = net.dec(z, lengths=lens)[0]
    side.synchronize()
    assert torch.equal(out, ref)
    a = net.dec(z, lengths=lens)[0]
    x, xl, sid = _batch(net, 3, 25, 3)
    net.infer(x, xl, sid, noise_scale=0)
    b = net.dec(z, lengths=lens)[0]
    assert torch.equal(a, ref) and torch.equal(b, ref)
    assert not bool(ref[lens.index(1), 0, spf:].any())


def test_splitk_mode():
    net, _ = _net("ljs_mb_istft_vits")
    spf = net.cfg.samples_per_frame
    lens = [180, 64, 65, 17, 9, 120]
    z = _z(net, len(lens), 180, 2)
    net.set_option("splitk", 1)
    try:
        alone = _alone(net, z, None, lens)
        a = net.dec(z, lengths=lens)[0].clone()
        b = net.dec(z, lengths=lens)[0].clone()
    finally:
        net.set_option("splitk", 0)
    assert torch.equal(a, b)
    for i, n in enumerate(lens):
        err = float(torch.sqrt(torch.mean((a[i, 0, :spf * n] - alone[i]) ** 2)))
        assert err <= 1e-5, (n, err)
        assert not bool(a[i, 0, spf * n:].any())


def test_error_paths_launch_nothing_and_the_model_serves_on():
    net, _ = _net("ljs_mini_mb_istft_vits")
    L = _capi.lib()
    h = net._ensure_handle()
    z = _z(net, 3, 50, 1)
    good = net.dec(z, lengths=[50, 20, 3])[0].clone()
    for bad in ([50, 51, 3], [50, -1, 3]):
        with pytest.raises(_capi.MbvError, match="outside"):
            net.dec(z, lengths=bad)
    with pytest.raises(ValueError):
        net.dec(z, lengths=[50, 20])
    o = torch.zeros_like(good)
    assert L.mbv_decode_ragged(h, ptr(z), None, 3, 50, None, ptr(o), net._stream()) != 0
    assert L.mbv_decode_ragged(h, ptr(z), None, 3, 50, (C.c_int64 * 3)(50, 60, 3), ptr(o), net._stream()) != 0
    assert L.mbv_last_error(h)
    net.set_option("trim", 1)
    try:
        with pytest.raises(_capi.MbvError, match="trim"):
            net.dec(z, lengths=[50, 20, 3])
    finally:
        net.set_option("trim", 0)
    net.set_option("conv_bf16", 3)
    try:
        with pytest.raises(_capi.MbvError, match="conv_bf16"):
            net.dec(z, lengths=[50, 20, 3])
    finally:
        net.set_option("conv_bf16", 0)
    torch.cuda.synchronize()
    assert not bool(o.any())                                                 # the refusals wrote nothing
    x, xl, sid = _batch(net, 3, 20, 5)
    for outputs in (None, ("o", "spec"), ("o_mb",)):
        with pytest.raises(ValueError):
            net.infer(x, xl, sid, outputs=outputs, ragged=True)
    with pytest.raises(ValueError):
        net.infer(x, xl, sid, outputs=("o",), ragged=True, trim=True)
    # a decoder output through the C entry itself
    net.infer(x, xl, sid, outputs=("o",), noise_scale=0)                     # (a fresh mbv_encode for the raw call below)
    outs = _capi.MbvOutputs()
    spec = torch.zeros(3, 4, 9, 16 * 8 + 1, device="cuda")
    outs.o, outs.spec = o.data_ptr(), spec.data_ptr()
    assert L.mbv_synthesize_ragged(h, 8, None, 0.0, 0, C.byref(outs), (C.c_int64 * 3)(8, 8, 8), net._stream()) != 0
    assert b"spec" in L.mbv_last_error(h)
    torch.cuda.synchronize()
    assert not bool(spec.any())
    assert torch.equal(net.dec(z, lengths=[50, 20, 3])[0], good)              # the handle serves the next call
