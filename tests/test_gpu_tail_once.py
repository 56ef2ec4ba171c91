""""tail_once" on the MI355X: the zero-input tail of a padded batch is computed for the shortest row only and copied to
the others (run_decoder).  Every stage tensor and every output of every row stays bitwise its B = 1 decode
at the same padded T' — a run with one row has no other row, so it never drops a tile.  By default the option works
on launches beyond one round of the grid; the small shapes here force it with `tail_once = 2` (same code), and
`test_default_mode_beyond_one_round` runs the default on a batch large enough."""
import pytest
import torch

from gpu_util import make_net

pytestmark = pytest.mark.gpu

TAPS = ("dec_conv_pre", "dec_up_0", "dec_res_0", "dec_up_1", "dec_res_1", "x_post")
OUTS = ("o", "o_mb", "spec", "phase")
SHAPES = [("ljs_mini_mb_istft_vits", 96, [96, 7, 40, 63, 7]),       # donor tie, a row with nothing to drop, 128-column tiles
          ("ljs_mb_istft_vits", 64, [64, 9, 30])]
IDS = ["mini_mb", "ljs_mb"]
_NETS = {}
_REF = {}


def _net(name, mode=2):
    if name not in _NETS:
        _NETS[name] = make_net(name)[0]
    _NETS[name].set_option("tail_once", mode)
    return _NETS[name]


def _z(net, lens, Tp, seed=5):
    z = torch.randn(len(lens), net.cfg.inter_channels, Tp, generator=torch.Generator().manual_seed(seed)).cuda()
    for b, n in enumerate(lens):
        z[b, :, n:] = 0                      # (the decoder masks at the lengths anyway: z * y_mask)
    return z


def _decode(net, z, lens, g=None):
    """Every tap and output of one default-mode decoder run on z * mask(lens), as [B, -1] tensors."""
    B, _, Tp = z.shape
    F = 16 * Tp + 1
    o = torch.empty(B, 1, 256 * Tp, device="cuda")
    o_mb = torch.empty(B, 4, 64 * Tp, device="cuda")
    spec = torch.empty(B, 4, 9, F, device="cuda")
    phase = torch.empty(B, 4, 9, F, device="cuda")
    net._decode_masked_into(z, g, lens, (o, o_mb, spec, phase))
    r = {k: net.read_stage(k).reshape(B, -1).clone() for k in TAPS}
    r.update(o=o.reshape(B, -1), o_mb=o_mb.reshape(B, -1), spec=spec.reshape(B, -1), phase=phase.reshape(B, -1))
    return r


def _reference(name, Tp, lens):
    """Row b decoded alone at the same padded T' (computed once per shape)."""
    key = (name, Tp, tuple(lens))
    if key not in _REF:
        net = _net(name)
        z = _z(net, lens, Tp)
        before = net.tail_dropped()
        _REF[key] = [_decode(net, z[b:b + 1], lens[b:b + 1]) for b in range(len(lens))]
        assert net.tail_dropped() == before          # one row: the option is inert
    return _REF[key]


@pytest.mark.parametrize("name,Tp,lens", SHAPES, ids=IDS)
def test_every_row_is_bitwise_its_b1_decode(name, Tp, lens):
    net = _net(name)
    alone = _reference(name, Tp, lens)
    before = net.tail_dropped()
    got = _decode(net, _z(net, lens, Tp), lens)
    dropped = net.tail_dropped() - before
    print("tail tiles dropped:", dropped)
    assert dropped > 0                                # not vacuous: tiles were in fact left out and filled
    for k in TAPS + OUTS:
        for b in range(len(lens)):
            assert torch.equal(got[k][b], alone[b][k][0]), (k, b, float((got[k][b] - alone[b][k][0]).abs().max()))
    # the option off: the same tensors, nothing dropped
    net.set_option("tail_once", 0)
    try:
        before = net.tail_dropped()
        off = _decode(net, _z(net, lens, Tp), lens)
        assert net.tail_dropped() == before
    finally:
        net.set_option("tail_once", 2)
    for k in TAPS + OUTS:
        assert torch.equal(got[k], off[k]), k
    # the default: these launches stay below one round of the grid, nothing is dropped
    net.set_option("tail_once", 1)
    try:
        before = net.tail_dropped()
        auto = _decode(net, _z(net, lens, Tp), lens)
        assert net.tail_dropped() == before
    finally:
        net.set_option("tail_once", 2)
    for k in TAPS + OUTS:
        assert torch.equal(got[k], auto[k]), k


def _tap_tail_starts(net, Tp):
    """(columns per row, rate, reach) of every tap: row b's columns at and past rate * len_b + reach are its tail."""
    plan = net.tail_plan()
    by = {(p[0], p[1], p[2], p[3]): p for p in plan}
    last = max(p[3] for p in plan if p[0] == 3)
    pre, up0, up1 = by[(0, -1, 0, 0)], by[(1, 0, 0, 0)], by[(1, 1, 0, 0)]
    res0, res1 = by[(3, 0, 2, last)], by[(3, 1, 2, last)]
    post, wave = by[(4, 2, 0, 0)], by[(5, 2, 0, 0)]
    F = 16 * Tp + 1
    return {"dec_conv_pre": (Tp, pre[4], pre[5]), "dec_up_0": (4 * Tp, up0[4], up0[5]), "dec_res_0": (4 * Tp, res0[4], res0[5]),
            "dec_up_1": (16 * Tp, up1[4], up1[5]), "dec_res_1": (16 * Tp, res1[4], res1[5]),
            "x_post": (F, post[4], post[5]), "spec": (F, post[4], post[5]), "phase": (F, post[4], post[5]),
            # a frame of x_post covers sub-band samples [4 f - 8, 4 f + 8): 4 (16 len - 1 + reach) + 7 - (64 len - 1)
            "o_mb": (64 * Tp, 64, 4 * post[5] + 4), "o": (256 * Tp, wave[4], wave[5])}


@pytest.mark.parametrize("name,Tp,lens", SHAPES, ids=IDS)
def test_reach_is_tight_enough(name, Tp, lens):
    """z of one row changed in its last valid frame only: that row's columns at and past S_b keep their bits in every
    tap (the column just before S_b of the last launch may change), and so does every other row."""
    net = _net(name)
    z = _z(net, lens, Tp)
    base = _decode(net, z, lens)
    starts = _tap_tail_starts(net, Tp)
    donor = lens.index(min(lens))
    for b in sorted({donor, 2}):
        z2 = z.clone()
        z2[b, :, lens[b] - 1] += torch.randn(net.cfg.inter_channels, generator=torch.Generator().manual_seed(9)).cuda()
        got = _decode(net, z2, lens)
        assert not torch.equal(got["o"][b], base["o"][b])
        for k, (cols, rate, reach) in starts.items():
            S = min(rate * lens[b] + reach, cols)
            a = got[k][b].reshape(-1, cols)
            r = base[k][b].reshape(-1, cols)
            assert torch.equal(a[:, S:], r[:, S:]), (k, b, S)
            others = [i for i in range(len(lens)) if i != b]
            assert torch.equal(got[k][others], base[k][others]), (k, b)


def test_three_streams_are_bitwise_one_stream():
    name, Tp = "ljs_mini_mb_istft_vits", 96
    lens = [96, 50, 13, 77, 31, 96, 8, 64]
    net = _net(name)
    z = _z(net, lens, Tp, seed=11)
    before = net.tail_dropped()
    three = _decode(net, z, lens)
    assert net.tail_dropped() > before
    net.set_option("dec_streams", 0)
    try:
        one = _decode(net, z, lens)
    finally:
        net.set_option("dec_streams", 1)
    for k in TAPS + OUTS:
        assert torch.equal(three[k], one[k]), k


def test_default_mode_beyond_one_round():
    """ljs_mb, B = 128, T' = 96: a stage-2 ResBlock conv is 512 tiles of 128 x 384 — two rounds — so the default
    value drops tiles and runs the three ResBlocks as concurrent big-tile launches (above the 192-tile cap of the
    small-launch rule: the schedule only tail maps bring).  Bitwise the option off, and bitwise one stream."""
    name, Tp, B = "ljs_mb_istft_vits", 96, 128
    lens = [Tp, 5] + [1 + (37 * b) % Tp for b in range(2, B)]
    net = _net(name, mode=1)
    try:
        z = _z(net, lens, Tp, seed=13)
        before = net.tail_dropped()
        got = _decode(net, z, lens)
        dropped = net.tail_dropped() - before
        print("tail tiles dropped:", dropped)
        assert dropped > 0
        net.set_option("tail_once", 0)
        off = _decode(net, z, lens)
        assert net.tail_dropped() == before + dropped
        net.set_option("tail_once", 1)
        net.set_option("dec_streams", 0)
        one = _decode(net, z, lens)
        assert net.tail_dropped() == before + 2 * dropped
    finally:
        net.set_option("dec_streams", 1)
        net.set_option("tail_once", 2)
    for k in TAPS + OUTS:
        assert torch.equal(got[k], off[k]), k
        assert torch.equal(got[k], one[k]), k


def test_inert_with_per_row_speaker_conditioning():
    net = _net("uudb_ms_istft_vits_ms")
    lens, Tp = [64, 9, 30], 64
    z = _z(net, lens, Tp)
    g = (0.3 * torch.randn(3, net.cfg.gin_channels, 1, generator=torch.Generator().manual_seed(3))).cuda()
    B, F = 3, 16 * Tp + 1
    o = torch.empty(B, 1, 256 * Tp, device="cuda")
    before = net.tail_dropped()
    net._decode_masked_into(z, g, lens, (o, None, None, None))
    torch.cuda.synchronize()
    assert net.tail_dropped() == before               # the tails differ per row: every tile is computed
    for b in range(B):
        ob = torch.empty(1, 1, 256 * Tp, device="cuda")
        net._decode_masked_into(z[b:b + 1], g[b:b + 1], lens[b:b + 1], (ob, None, None, None))
        assert torch.equal(o[b], ob[0])


@pytest.mark.parametrize("epi,K,dil", [("STORE", 3, 3), ("RESID", 3, 3), ("RESID_ACC", 11, 5)])
def test_op_level_launch_on_big_tiles(epi, K, dil):
    """One launch shaped like `big_resid` of conv_cases.py (64 x 128 x 128 x 3071, 128 x 384 tiles, odd T: the scalar
    fill) per epilogue: rows identical to the donor from their length on; tail map + fill against the plain launch."""
    import ctypes as C
    import numpy as np
    import conv_cases as cc
    from gpu_util import ptr
    from mb_istft_vits_amd import _capi
    net = _net("ljs_mini_mb_istft_vits")
    B, Cin, Cout, T = 64, 128, 128, 3071
    acc = epi == "RESID_ACC"
    lens = cc.ragged(B, T, 5)
    lens[9] = 0                                       # a tie for the donor (row 1 holds the other 0)
    donor, pad = 1, (K - 1) * dil // 2
    assert lens.index(min(lens)) == donor
    g = torch.Generator(device="cuda").manual_seed(21)
    x = torch.randn(B, Cin, T, device="cuda", generator=g)
    res = torch.randn(B, Cout, T, device="cuda", generator=g)
    accum = torch.randn(B, Cout, T, device="cuda", generator=g)
    for b, n in enumerate(lens):
        for t in (x, res, accum):
            t[b, :, n:] = t[donor, :, n:]
    w = np.ascontiguousarray((torch.randn(Cout, Cin, K, generator=torch.Generator().manual_seed(22)) / (Cin * K) ** 0.5).numpy())
    bias = np.ascontiguousarray(0.5 * torch.randn(Cout, generator=torch.Generator().manual_seed(23)).numpy())

    def launch(tail):
        c = cc.case("tail_" + epi.lower(), "BIG", B, Cin, Cout, T, epi=epi, K=K, dil=dil, accum=acc,
                    out_scale=cc.THIRD if acc else 1.0, trim=(1, pad, lens) if tail else None)
        y = accum.clone() if acc else torch.full((B, Cout, T), float("nan"), device="cuda")
        ptrs = {"res": res.data_ptr()} if epi != "STORE" else {}
        if acc:
            ptrs["accum_in"] = y.data_ptr()
        d = cc.desc(c, ptrs=ptrs, ws=False)
        d.tail_once = int(tail)
        out = (C.c_int32 * 8)()
        h = net._ensure_handle()
        rc = _capi.lib().mbv_op_conv(h, C.byref(d), ptr(x), w.ctypes.data_as(C.c_void_p), bias.ctypes.data_as(C.c_void_p),
                                     ptr(y), C.byref(out), net._stream())
        _capi.check(h, rc, "mbv_op_conv")
        return y, _capi.ROUTES[out[0]]

    plain, r0 = launch(False)
    before = net.tail_dropped()
    tailed, r1 = launch(True)
    dropped = net.tail_dropped() - before
    assert (r0, r1) == ("BIG", "BIG")
    want = sum(-(-T // 384) - -(-min(n + pad, T) // 384) for b, n in enumerate(lens) if b != donor)
    assert dropped == want and dropped > 0, (dropped, want)
    assert torch.equal(plain, tailed)
