""""tail_once" on the MI355X beyond the two families of test_gpu_tail_once.py / test_gpu_tail_pack.py: every decoder
family with the option forced, the packed route on another family, rate and reach, and the device builders
(`tail_map_kernel`, both branches; `trim_map_kernel`) past 256 rows, where a thread owns a run of rows.  Every
comparison is bitwise unless it says otherwise; asserted values come from the option off, the B = 1 decode at the same
padded T' (one row has no other row: it never drops a tile) or the arithmetic of tail_once_cases.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import conv_cases as cc
import tail_once_cases as tc
from gpu_util import ptr
from mb_istft_vits_amd import _capi

pytestmark = pytest.mark.gpu

IDS = [tc.ident(c) for c in tc.GPU_FAMILIES]


def _tp(net):
    """Every stage at least three 128-column tiles: 96 frames behind a rate-4 first stage, 48 behind a rate-8 one."""
    return 96 if net.cfg.upsample_rates[0] == 4 else 48


def _has_short_row(net, lens, Tp):
    """Some row but the donor whose S_b at the stage-1 launch that reaches farthest lies a whole 384-column tile (the
    widest there is) or more in front of T: whatever the tile width, a map drops a tile of it."""
    rate, reach = tc.own_reach(net.cfg)[(tc.C2, 1, 2, tc.n_steps(net.cfg) - 1)]
    donor = tc.donor_of(lens)
    return any(rate * n + reach + 384 <= rate * Tp for b, n in enumerate(lens) if b != donor)


@pytest.mark.parametrize("name,overrides", tc.GPU_FAMILIES, ids=IDS)
def test_family_forced_on_fixed_and_seeded_vectors(name, overrides):
    """`tail_once = 2` against the option off on every tap and output, four rows against their B = 1 decode, and the
    counter against the test's own count: five fixed vectors, six seeded ones, and the boundary lengths."""
    net = tc.gpu_net(name, overrides)
    Tp = _tp(net)
    rs = np.random.RandomState(4000 + IDS.index(tc.ident((name, overrides))))
    vectors = [[Tp, 7, 40, min(63, Tp - 1), 7], [Tp, Tp], [0, Tp], [Tp, 0, 0, 1], [Tp] * 5]
    vectors += [tc.seeded_lens(rs, Tp, dup_min=i % 2 == 0) for i in range(6)]
    edges = tc.boundary_lens(net, Tp)                     # S_b - 1 on a tile boundary: where a reach one short drops a tile too many
    assert edges
    vectors += edges
    moved = 0
    try:
        for n_v, lens in enumerate(vectors):
            z = tc.make_z(net, lens, Tp, seed=50 + n_v)
            net.set_option("tail_once", 2)
            before = net.tail_dropped()
            got = tc.decode(net, z, lens)
            dropped = net.tail_dropped() - before
            want, _, how = tc.decoder_left_out(net, lens, Tp, 2)
            print("%s %s: tail tiles dropped %d (own count %d, %s)" % (tc.ident((name, overrides)), lens, dropped, want, how))
            assert dropped == want, (lens, dropped, want)
            if len(set(lens)) == 1:
                assert dropped == 0
            if _has_short_row(net, lens, Tp):
                assert dropped > 0, lens
                moved += 1
            net.set_option("tail_once", 0)
            before = net.tail_dropped()
            off = tc.decode(net, z, lens)
            assert net.tail_dropped() == before
            tc.assert_same(got, off, lens)
            net.set_option("tail_once", 2)
            rows = {0, tc.donor_of(lens), lens.index(max(lens)), int(rs.randint(len(lens)))}
            tc.assert_rows_alone(net, z, lens, got, rows, lens)
    finally:
        net.set_option("tail_once", 1)
    assert moved >= 3                                     # not vacuous: (at least) the fixed vectors with short rows


TIGHT = [("ljs_mini_istft_vits", None), ("ljs_ms_istft_vits", None), ("ljs_mini_mb_istft_vits", tc.RB2)]


@pytest.mark.parametrize("name,overrides", TIGHT, ids=[tc.ident(c) for c in TIGHT])
def test_reach_is_tight_enough(name, overrides):
    """z of one row changed in its last valid frame only: that row's columns at and past S_b keep their bits in every
    tap and output the family has, and so does every other row."""
    net = tc.gpu_net(name, overrides)
    Tp = _tp(net)
    lens = [Tp, 7, 40, min(63, Tp - 1), 7]
    net.set_option("tail_once", 2)
    try:
        z = tc.make_z(net, lens, Tp)
        base = tc.decode(net, z, lens)
        starts = tc.tap_tail_starts(net, Tp)
        assert set(starts) == set(base)
        for b in sorted({tc.donor_of(lens), 2}):
            z2 = z.clone()
            z2[b, :, lens[b] - 1] += torch.randn(net.cfg.inter_channels, generator=torch.Generator().manual_seed(9)).cuda()
            got = tc.decode(net, z2, lens)
            assert not torch.equal(got["o"][b], base["o"][b])
            others = [i for i in range(len(lens)) if i != b]
            for k, (cols, rate, reach) in starts.items():
                S = min(rate * lens[b] + reach, cols)
                a = got[k][b].reshape(-1, cols)
                r = base[k][b].reshape(-1, cols)
                assert not torch.equal(a[:, :S], r[:, :S]), (k, b)
                assert torch.equal(a[:, S:], r[:, S:]), (k, b, S)
                assert torch.equal(got[k][others], base[k][others]), (k, b)
    finally:
        net.set_option("tail_once", 1)


# (family, B, T', tail_once, the two rows of length 0 or None, what stage 0's launches must take)
# ljs_istft, default mode: stage 0 is 256 ch x 384 columns (512 tiles of 128 x 384, one column tile a row), stage 1
# 128 ch x 3072 (eight a row): both pack, behind stride-8 conv-transposes.
# ljs_mini_mb B = 683, default mode: stage 0 is 128 ch x 384 columns, 683 big tiles: the packed branch of
# tail_map_kernel with three rows a thread.  (B = 513 .. 682 plan the untrimmed launch as SPLIT_BATCH — two whole
# rounds of big tiles and the rest on small ones — which a trimmed launch never takes: no map at all.  683 is the first
# B past 512 whose launch stays on the big shape.)  Stage 1 has 64 channels: HALF untrimmed, M64 trimmed — route kept.
# ljs_mini_mb B = 300, tail_once = 2: below 512 big tiles, the plain map branch on 128-column tiles, two rows a thread.
SHAPES = [("ljs_istft_vits", 256, 48, 1, None, "pack"),
          ("ljs_mini_mb_istft_vits", 683, 96, 1, (300, 519), "pack"),
          ("ljs_mini_mb_istft_vits", 300, 96, 2, (270, 297), "map")]


def _shape_lens(B, Tp, zeros, variant):
    if variant == "all_equal":
        return [Tp] * B
    if zeros is None:                                     # (the pattern of test_decoder_default_mode_packs_short_stages)
        return [Tp, 5, 0, Tp // 2] + [1 + (37 * b) % Tp for b in range(4, B - 1)] + [Tp]
    return tc.spread_lens(B, Tp, -(-B // 256), zeros)


@pytest.mark.parametrize("variant", ["ragged", "all_equal"])
@pytest.mark.parametrize("name,B,Tp,mode,zeros,route", SHAPES, ids=["ljs_istft_256", "mini_mb_683", "mini_mb_300"])
def test_builders_past_256_rows_and_the_packed_route(name, B, Tp, mode, zeros, route, variant):
    net = tc.gpu_net(name)
    lens = _shape_lens(B, Tp, zeros, variant)
    donor = tc.donor_of(lens)
    if variant == "ragged":
        assert donor == (2 if zeros is None else zeros[0]) and lens[0] == lens[B - 1] == Tp
    want, by_map, how = tc.decoder_left_out(net, lens, Tp, mode)
    assert how[0] == [route], how                         # the shape reaches the branch it is here for
    if name == "ljs_istft_vits":
        assert how[1] == ["pack"], how
    got = off = one = None
    try:
        z = tc.make_z(net, lens, Tp, seed=13)
        net.set_option("tail_once", mode)
        before = net.tail_dropped()
        got = tc.decode(net, z, lens)
        dropped = net.tail_dropped() - before
        print("%s B = %d %s: tail tiles left out: %d (own count %d; the maps alone: %d; %s)"
              % (name, B, variant, dropped, want, by_map, how))
        assert dropped == want, (dropped, want)
        if variant == "ragged":
            assert dropped > 0 and (route == "map" or want > by_map)
        else:
            assert dropped == 0
            for stage, kind, j, q, rate, reach, c in tc.resblock_launches(net, B, Tp):
                if route == "pack" and stage == 0:        # the gaps cost tiles and no tail saves any: nothing is added
                    halo = (c["K"] - 1) * c["dil"]
                    assert tc.pack_tiles(lens, rate, reach, c["T"], halo) >= B * -(-c["T"] // 384)
        net.set_option("tail_once", 0)
        off = tc.decode(net, z, lens)
        assert net.tail_dropped() == before + dropped
        tc.assert_same(got, off, "option off")
        off = None
        net.set_option("tail_once", mode)
        net.set_option("dec_streams", 0)
        one = tc.decode(net, z, lens)
        assert net.tail_dropped() == before + 2 * dropped
        tc.assert_same(got, one, "one stream")
        one = None
        net.set_option("dec_streams", 1)
        rows = {0, donor, B - 1} | {b for b in (255, 256, 257) if b < B}
        tc.assert_rows_alone(net, z, lens, got, rows, "alone")
    finally:
        net.set_option("dec_streams", 1)
        net.set_option("tail_once", 1)
        got = off = one = z = None
        torch.cuda.empty_cache()


@pytest.mark.parametrize("epi,K,dil", [("STORE", 3, 1), ("RESID", 7, 5), ("RESID_ACC", 11, 3)])
def test_op_level_packed_launch_past_256_rows(epi, K, dil):
    """One packed launch of 260 rows (two rows a thread in the builder), the donor at row 258 with a tie at 259: packed
    launch + fill against the plain launch, a trimmed launch (`trim_map_kernel`, two rows a thread) below its limits,
    and the packed result against the float64 reference of test_gpu_conv_routes.py at that file's bar."""
    from test_gpu_conv_routes import TOL, _reference
    net = tc.gpu_net("ljs_mini_mb_istft_vits")
    B, Ch, T = 260, 128, 767
    acc = epi == "RESID_ACC"
    halo = (K - 1) * dil
    pad = halo // 2
    lens = cc.ragged(B, T, 5)
    lens[1] = 1                                           # the minimum plus one in front of the donor
    lens[9] = 384 - pad                                   # a region that ends exactly on a tile boundary
    lens[258] = lens[259] = 0
    donor = 258
    assert tc.donor_of(lens) == donor
    g = torch.Generator().manual_seed(21)
    t = {"x": torch.randn(B, Ch, T, generator=g), "res": torch.randn(B, Ch, T, generator=g),
         "accum": torch.randn(B, Ch, T, generator=g)}
    for b, n in enumerate(lens):                          # rows identical to the donor from their length on
        for k in t:
            t[k][b, :, n:] = t[k][donor, :, n:]
    t["w"] = torch.randn(Ch, Ch, K, generator=torch.Generator().manual_seed(22)) / (Ch * K) ** 0.5
    t["bias"] = 0.5 * torch.randn(Ch, generator=torch.Generator().manual_seed(23))
    x, res = t["x"].cuda(), t["res"].cuda()
    w = np.ascontiguousarray(t["w"].numpy())
    bias = np.ascontiguousarray(t["bias"].numpy())

    def case(trim):
        return cc.case("pack260_" + epi.lower(), None, B, Ch, Ch, T, epi=epi, K=K, dil=dil, accum=acc,
                       out_scale=cc.THIRD if acc else 1.0, trim=(1, pad, lens) if trim else None)

    def launch(trim, tail):
        y = t["accum"].cuda() if acc else torch.full((B, Ch, T), float("nan"), device="cuda")
        ptrs = {"res": res.data_ptr()} if epi != "STORE" else {}
        if acc:
            ptrs["accum_in"] = y.data_ptr()
        d = cc.desc(case(trim), ptrs=ptrs, ws=False)
        d.tail_once = tail
        out = (C.c_int32 * 8)()
        h = net._ensure_handle()
        rc = _capi.lib().mbv_op_conv(h, C.byref(d), ptr(x), w.ctypes.data_as(C.c_void_p), bias.ctypes.data_as(C.c_void_p),
                                     ptr(y), C.byref(out), net._stream())
        _capi.check(h, rc, "mbv_op_conv")
        return y, _capi.ROUTES[out[0]]

    plain, r0 = launch(False, 0)
    before = net.tail_dropped()
    packed, r1 = launch(True, 2)
    dropped = net.tail_dropped() - before
    assert r1 == "TAIL_PACK" and r0 in ("BIG", "SPLIT_BATCH"), (r0, r1)
    want = B * -(-T // 384) - tc.pack_tiles(lens, 1, pad, T, halo)
    print("plain route %s; packed launch left out %d of %d tiles" % (r0, dropped, B * -(-T // 384)))
    assert dropped == want and dropped > 0, (dropped, want)
    assert torch.equal(plain, packed)
    trimmed, r2 = launch(True, 0)
    assert r2 == "BIG" and net.tail_dropped() == before + dropped
    for b, n in enumerate(lens):
        lim = min(T, n + pad)
        assert torch.equal(trimmed[b, :, :lim], plain[b, :, :lim]), b
    # the packed route in the float64 matrix directly
    utts, chans = [0, 1, 128, 258, 259], [0, 63, 64, 127]
    y64, A = _reference(case(False), t, utts, chans)
    got = packed.cpu()[utts][:, chans].to(torch.float64)
    err = (got - y64).abs()
    assert bool(torch.isfinite(got).all())
    assert not bool((err > TOL[0] * A + 1e-7).any()), (float(err.max()), float((err / A.clamp_min(1e-30)).max()))
