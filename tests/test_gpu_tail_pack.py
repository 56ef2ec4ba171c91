"""The packed route of "tail_once" (TAIL_PACK): every row but the donor keeps its columns [0, S_b'), the rows' kept
columns laid end to end share the 128 x 384 tiles, and the rest comes from the donor.  An output element's chain of
operations does not depend on its tile, so every tensor is bitwise the plain launch's."""
import ctypes as C

import numpy as np
import pytest
import torch

import conv_cases as cc
from gpu_util import make_net, ptr
from mb_istft_vits_amd import _capi

pytestmark = pytest.mark.gpu

_NETS = {}


def _net(name):
    if name not in _NETS:
        _NETS[name] = make_net(name)[0]
    return _NETS[name]


def pack_tiles(lens, num, reach, T, halo, bn=384):
    """(column tiles of the packed axis, donor): the layout of DESIGN §9 in the test's own arithmetic."""
    donor = lens.index(min(lens))
    gap = -(-halo // 32) * 32
    blocks = 0
    for b, n in enumerate(lens):
        sp = T if b == donor else min(T, -(-min(T, n * num + reach) // 32) * 32)
        blocks += -(-sp // 32) + gap // 32
    return -(-blocks // (bn // 32)), donor


def _lens(B, T, pad):
    lens = cc.ragged(B, T, 5)                         # T, 0, 1, 32, 128, 384, 383, 129, then a spread
    lens[0] = 384 - pad                               # row 0's region ends exactly on the first tile boundary
    lens[9] = 0                                       # a tie for the donor (row 1 holds the other 0)
    lens[10:16] = [5, 0, 17, 3, 40, 1]                # rows shorter than a block: one tile spans more than three rows
    lens[B - 1] = T                                   # a whole row last
    return lens


OP_CASES = [(epi, K, dil, B, C_, T) for epi in ("STORE", "RESID", "RESID_ACC") for K, dil in ((3, 3), (7, 3), (11, 5))
            for B, C_, T in ((64, 128, 3071),)] + [
    ("STORE", 3, 3, 128, 256, 767), ("RESID", 7, 3, 128, 256, 767), ("RESID_ACC", 11, 5, 128, 256, 767)]


@pytest.mark.parametrize("epi,K,dil,B,Ch,T", OP_CASES)
def test_op_level_packed_launch(epi, K, dil, B, Ch, T):
    """One launch on the big shape per epilogue and channel chunk (K 3: 16 channels, K 7 / 11: 8).  T = 3071: odd (the
    scalar fill), several rows inside one tile; 256 channels x T = 767: two row tiles.  Rows identical to the donor from
    their length on; packed launch + fill against the plain launch."""
    net = _net("ljs_mini_mb_istft_vits")
    acc = epi == "RESID_ACC"
    halo = (K - 1) * dil
    pad = halo // 2
    lens = _lens(B, T, pad)
    donor = 1
    assert lens.index(min(lens)) == donor
    g = torch.Generator(device="cuda").manual_seed(21)
    x = torch.randn(B, Ch, T, device="cuda", generator=g)
    res = torch.randn(B, Ch, T, device="cuda", generator=g)
    accum = torch.randn(B, Ch, T, device="cuda", generator=g)
    for b, n in enumerate(lens):
        for t in (x, res, accum):
            t[b, :, n:] = t[donor, :, n:]
    w = np.ascontiguousarray((torch.randn(Ch, Ch, K, generator=torch.Generator().manual_seed(22)) / (Ch * K) ** 0.5).numpy())
    bias = np.ascontiguousarray(0.5 * torch.randn(Ch, generator=torch.Generator().manual_seed(23)).numpy())

    def launch(tail):
        c = cc.case("pack_" + epi.lower(), "BIG", B, Ch, Ch, T, epi=epi, K=K, dil=dil, accum=acc,
                    out_scale=cc.THIRD if acc else 1.0, trim=(1, pad, lens) if tail else None)
        y = accum.clone() if acc else torch.full((B, Ch, T), float("nan"), device="cuda")
        ptrs = {"res": res.data_ptr()} if epi != "STORE" else {}
        if acc:
            ptrs["accum_in"] = y.data_ptr()
        d = cc.desc(c, ptrs=ptrs, ws=False)
        d.tail_once = tail
        out = (C.c_int32 * 8)()
        h = net._ensure_handle()
        rc = _capi.lib().mbv_op_conv(h, C.byref(d), ptr(x), w.ctypes.data_as(C.c_void_p), bias.ctypes.data_as(C.c_void_p),
                                     ptr(y), C.byref(out), net._stream())
        _capi.check(h, rc, "mbv_op_conv")
        return y, _capi.ROUTES[out[0]], list(out)

    plain, r0, _ = launch(0)
    before = net.tail_dropped()
    packed, r1, p1 = launch(2)
    dropped = net.tail_dropped() - before
    assert (r0, r1) == ("BIG", "TAIL_PACK") and p1[1:5] == [128, 384, 512, 16 if K == 3 else 8]
    tiles, d_ = pack_tiles(lens, 1, pad, T, halo)
    assert d_ == donor
    want = B * -(-T // 384) - tiles
    assert dropped == want and dropped > 0, (dropped, want)
    assert torch.equal(plain, packed)


TAPS = ("dec_conv_pre", "dec_up_0", "dec_res_0", "dec_up_1", "dec_res_1", "x_post")
OUTS = ("o", "o_mb", "spec", "phase")


def _z(net, lens, Tp, seed=5):
    z = torch.randn(len(lens), net.cfg.inter_channels, Tp, generator=torch.Generator().manual_seed(seed)).cuda()
    for b, n in enumerate(lens):
        z[b, :, n:] = 0
    return z


def _decode(net, z, lens):
    """Every tap and output of one decoder run on z * mask(lens), as [B, -1] tensors."""
    B, _, Tp = z.shape
    F = 16 * Tp + 1
    o = torch.empty(B, 1, 256 * Tp, device="cuda")
    o_mb = torch.empty(B, 4, 64 * Tp, device="cuda")
    spec = torch.empty(B, 4, 9, F, device="cuda")
    phase = torch.empty(B, 4, 9, F, device="cuda")
    net._decode_masked_into(z, None, lens, (o, o_mb, spec, phase))
    r = {k: net.read_stage(k).reshape(B, -1).clone() for k in TAPS}
    r.update(o=o.reshape(B, -1), o_mb=o_mb.reshape(B, -1), spec=spec.reshape(B, -1), phase=phase.reshape(B, -1))
    return r


def test_decoder_default_mode_packs_short_stages():
    """ljs_mb, B = 128, T' = 192, the default mode: stage 0 is 768 columns (2 x 2 x 128 = 512 big tiles, two column
    tiles a row) and stage 1 3072 (eight a row), so both take the packed route.  Bitwise the option off, the
    one-stream schedule and — four rows — the B = 1 decode; and more tiles are left out than the maps could drop."""
    name, Tp, B = "ljs_mb_istft_vits", 192, 128
    lens = [Tp, 5, 0, 96] + [1 + (37 * b) % Tp for b in range(4, B)]
    donor = 2
    net = _net(name)
    net.set_option("tail_once", 1)
    try:
        z = _z(net, lens, Tp, seed=13)
        before = net.tail_dropped()
        got = _decode(net, z, lens)
        dropped = net.tail_dropped() - before
        net.set_option("tail_once", 0)
        off = _decode(net, z, lens)
        assert net.tail_dropped() == before + dropped
        alone = {b: _decode(net, z[b:b + 1], lens[b:b + 1]) for b in (0, 1, donor, 77)}
        net.set_option("tail_once", 1)
        net.set_option("dec_streams", 0)
        one = _decode(net, z, lens)
        assert net.tail_dropped() == before + 2 * dropped
    finally:
        net.set_option("dec_streams", 1)
        net.set_option("tail_once", 1)
    for k in TAPS + OUTS:
        assert torch.equal(got[k], off[k]), k
        assert torch.equal(got[k], one[k]), k
        for b, r in alone.items():
            assert torch.equal(got[k][b], r[k][0]), (k, b)
    # the test's own arithmetic, per ResBlock launch (kind 2 / 3 of the tail plan: first / second conv of step q)
    ks, ds = net.cfg.resblock_kernel_sizes, net.cfg.resblock_dilation_sizes
    by_map = by_pack = 0
    for kind, stage, j, q, rate, reach in net.tail_plan():
        if kind not in (2, 3):
            continue
        T = rate * Tp
        halo = (ks[j] - 1) * (ds[j][q] if kind == 2 else 1)
        full = -(-T // 384)
        by_map += sum(full - -(-min(T, rate * n + reach) // 384) for b, n in enumerate(lens) if b != donor)
        tiles, d_ = pack_tiles(lens, rate, reach, T, halo)
        assert d_ == donor
        by_pack += B * full - tiles
    print("tail tiles left out: %d (the maps alone: %d)" % (dropped, by_map))
    assert dropped == by_pack and by_pack > by_map > 0, (dropped, by_pack, by_map)
