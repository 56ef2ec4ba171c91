"""Streaming decode on the MI355X: `dec_stream` / `infer_stream` / `mbv_decode_range` against the one-shot decode."""
import ctypes as C

import numpy as np
import pytest
import torch

from mb_istft_vits_amd import _capi, synth
from mb_istft_vits_amd.stream import chunk_schedule

from gpu_util import make_net, ptr

pytestmark = pytest.mark.gpu

RB2 = {"resblock": "2", "resblock_dilation_sizes": [[1, 3], [1, 3], [1, 3]]}
_NETS = {}


def _net(name, overrides=None):
    key = (name, repr(overrides))
    if key not in _NETS:
        _NETS[key] = make_net(name, overrides=overrides)[0]
    return _NETS[key]


def _z(net, B, Tp, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, net.cfg.inter_channels, Tp, generator=g).cuda()


def _g(net, B, seed):
    if not net.cfg.gin_channels:
        return None
    return (0.3 * torch.randn(B, net.cfg.gin_channels, 1, generator=torch.Generator().manual_seed(seed))).cuda()


def _stream_cat(st):
    parts, nxt = [], 0
    for a, v in st:
        assert a == nxt
        parts.append(v.clone())
        nxt = a + v.shape[2]
    return torch.cat(parts, dim=2)


CASES = [("ljs_mini_mb_istft_vits", None), ("ljs_ms_istft_vits", None), ("uudb_ms_istft_vits_ms", None),
         ("ljs_mini_istft_vits", None), ("ljs_mini_mb_istft_vits", RB2)]


@pytest.mark.parametrize("name,overrides", CASES, ids=["mini_mb", "ms", "uudb", "sb", "rb2"])
@pytest.mark.parametrize("B", [1, 3])
def test_dec_stream_bitwise(name, overrides, B):
    net = _net(name, overrides)
    Lc, Rc = net.decoder_context()
    for Tp in (1, 17, Lc + Rc, 300):
        z, g = _z(net, B, Tp, Tp), _g(net, B, Tp)
        ref = net.dec(z, g)[0]
        for c in (1, 8, 32):
            if c == 1 and Tp == 300:
                c = 2                                 # (150 launches suffice for the smallest chunks)
            st = net.dec_stream(z, g, chunk_frames=c, max_chunk_frames=max(c, 64))
            out = _stream_cat(st)
            assert torch.equal(out, ref), (name, B, Tp, c, float((out - ref).abs().max()))
            assert torch.equal(st.o, ref)


@pytest.mark.parametrize("name,overrides,kw", [
    ("ljs_mini_mb_istft_vits", None, dict(noise_scale=0.667)),
    ("ljs_mini_mb_istft_vits", {"use_sdp": True}, dict(noise_scale=0.5, noise_scale_w=0.8)),
    ("uudb_ms_istft_vits_ms", None, dict(noise_scale=0.667, max_len=40)),
    ("ljs_mini_istft_vits", None, dict(noise_scale=0.3, length_scale=1.2)),
])
def test_infer_stream_bitwise(name, overrides, kw):
    net = _net(name, overrides)
    x, xl, sid = synth.synthetic_batch(net.cfg, 3, 30, seed=11, ragged=True)
    x, xl = torch.from_numpy(x).cuda(), torch.from_numpy(xl).cuda()
    sid = torch.from_numpy(sid).cuda() if sid is not None else None
    torch.manual_seed(5)
    torch.cuda.manual_seed(5)
    (o, *_), yl = net.infer_with_lengths(x, xl, sid=sid, **kw)
    torch.manual_seed(5)
    torch.cuda.manual_seed(5)
    st = net.infer_stream(x, xl, sid=sid, chunk_frames=8, max_chunk_frames=64, **kw)
    assert torch.equal(st.y_lengths, yl)
    assert st.o.shape == o.shape
    assert torch.equal(_stream_cat(st), o)


def test_read_bound_nan_outside_window():
    net = _net("ljs_mini_mb_istft_vits")
    Lc, Rc = net.decoder_context()
    spf = net.cfg.samples_per_frame
    z = _z(net, 2, 200, 1)
    ref = net.dec(z)[0]
    h = net._ensure_handle()
    for first, count in ((0, 8), (60, 32), (190, 10)):
        zn = z.clone()
        lo, hi = max(0, first - Lc), min(200, first + count + Rc)
        zn[:, :, :lo] = float("nan")
        zn[:, :, hi:] = float("nan")
        o = torch.full_like(ref, float("nan"))
        _capi.check(h, _capi.lib().mbv_decode_range(h, ptr(zn), None, 2, 200, first, count, ptr(o), o.stride(0),
                                                    net._stream()), "mbv_decode_range")
        torch.cuda.synchronize()
        a, b = spf * first, spf * (first + count)
        assert torch.equal(o[:, :, a:b], ref[:, :, a:b])
        assert torch.isfinite(o[:, :, a:b]).all()
        assert torch.isnan(o[:, :, :a]).all() and torch.isnan(o[:, :, b:]).all()      # nothing else written


def test_splitk_mode():
    net = _net("ljs_mb_istft_vits")
    z = _z(net, 1, 180, 2)
    net.set_option("splitk", 1)
    try:
        ref = net.dec(z)[0]
        a = net.dec_stream(z, chunk_frames=16, max_chunk_frames=64).run().clone()
        b = net.dec_stream(z, chunk_frames=16, max_chunk_frames=64).run().clone()
    finally:
        net.set_option("splitk", 0)
    assert torch.equal(a, b)
    assert float(torch.sqrt(torch.mean((a - ref) ** 2))) <= 1e-5


def test_side_stream_and_paused_stream():
    net = _net("ljs_mini_mb_istft_vits")
    z = _z(net, 2, 150, 3)
    ref = net.dec(z)[0]
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        out = net.dec_stream(z, chunk_frames=8).run()
    side.synchronize()
    assert torch.equal(out, ref)
    # paused: other calls on the same handle in between
    st = net.dec_stream(z, chunk_frames=8, max_chunk_frames=32)
    first = next(st)
    x, xl, _ = synth.synthetic_batch(net.cfg, 2, 20, seed=4, ragged=True)
    net.infer(torch.from_numpy(x).cuda(), torch.from_numpy(xl).cuda(), noise_scale=0)
    other = net.dec_stream(_z(net, 1, 90, 9), chunk_frames=4)
    next(other)
    net.dec(_z(net, 3, 40, 8))
    for _ in st:
        pass
    assert torch.equal(st.o, ref)
    assert first[0] == 0


def test_raw_ctypes_paths():
    net = _net("ljs_mini_mb_istft_vits")
    L = _capi.lib()
    h = net._ensure_handle()
    s = net._stream()
    z = _z(net, 2, 64, 5)
    ref = net.dec(z)[0]
    big = torch.full((2, 1, 256 * 64 + 128), -7.0, device="cuda")          # row stride larger than a row
    for first, count in chunk_schedule(64, 5, 20):
        assert L.mbv_decode_range(h, ptr(z), None, 2, 64, first, count, ptr(big), big.stride(0), s) == 0
    torch.cuda.synchronize()
    assert torch.equal(big[:, :, :256 * 64], ref)
    assert (big[:, :, 256 * 64:] == -7.0).all()
    o = torch.zeros_like(ref)
    bad = [(2, 64, -1, 4, o.stride(0)), (2, 64, 60, 5, o.stride(0)), (2, 64, 0, 0, o.stride(0)),
           (2, 64, 64, 1, o.stride(0)), (2, 64, 0, 4, o.stride(0) - 4), (0, 64, 0, 4, o.stride(0)),
           (2, 64, 0, 4, o.stride(0) + 2)]
    for B, T, first, count, stride in bad:
        assert L.mbv_decode_range(h, ptr(z), None, B, T, first, count, ptr(o), stride, s) != 0
        assert L.mbv_last_error(h)
    assert L.mbv_decode_range(h, None, None, 2, 64, 0, 4, ptr(o), o.stride(0), s) != 0
    torch.cuda.synchronize()
    assert not o.any()                                                      # errors wrote nothing
    assert torch.equal(net.dec_stream(z, chunk_frames=16).run(), ref)      # the handle serves the next call
    out = (C.c_int32 * 2)()
    assert L.mbv_decoder_context(C.byref(net._config_struct()), C.byref(out)) == 0
    assert (out[0], out[1]) == net.decoder_context()
