"""The conv launcher's route selection (`conv1d_plan`, conv1d.hip) through the host-only `mbv_conv_plan`: no GPU.

The GPU route tests (test_gpu_conv_routes.py) are written for the routes their cases declare; these tests keep the
declarations true, so that a retune of a threshold cannot silently move a case off the route it was written for."""
import pytest

import conv_cases as cc


@pytest.mark.parametrize("c", cc.CASES, ids=lambda c: c["name"])
def test_case_plans_its_route(c):
    p = cc.plan(cc.desc(c))
    assert p["route"] == c["route"], (c["name"], p)
    if c["S_gt1"]:
        assert p["S"] > 1, p
    if c["route"] == "VS":
        halo = 16 // c["kind"]
        assert p["vs_tv"] == c["T"] + halo, p
    if c["route"] == "SPLIT_BATCH":
        assert 0 < p["nb_big"] < c["B"], p
    if c["pair"]:
        q = cc.plan(cc.desc(c, B=2, trim=False))
        assert q["route"] == c["pair_route"], (c["name"], q)


@pytest.mark.parametrize("c", cc.LN_CASES, ids=lambda c: c["name"])
def test_ln_case_plans_the_narrow_kernel(c):
    """conv + LayerNorm in one launch exists on the narrow kernel only, whatever the mode."""
    for splitk in (0, 1):
        p = cc.plan(cc.desc(c, splitk=splitk))
        assert p["route"] == "NARROW_M" and p["S"] == 1, (c["name"], p)
    assert c["T"] <= 256 and c["Cout"] % 32 == 0 and c["Cout"] <= 768


def test_ln_descriptors_outside_the_narrow_kernel_are_refused():
    base = cc.LN_BY_NAME["ln_ffn2_h192_t200"]
    bad = [dict(base, T=257, Tin=257), dict(base, Cout=800), dict(base, Cout=100), dict(base, reflect1=1),
           dict(base, K=13), dict(base, prec=3), dict(base, res_chan_add=True), dict(base, kind=4),
           dict(base, trim=(1, 0, [1, 2, 3]))]
    for c in bad:
        with pytest.raises(Exception):
            cc.plan(cc.desc(c))
    d = cc.desc(base)
    d.ln_gamma = None
    with pytest.raises(Exception, match="ln_gamma"):
        cc.plan(d)
    d = cc.desc(cc.BY_NAME["narrow_resid"])
    d.ln_out_lens = 1 << 20                 # LayerNorm fields on another epilogue
    with pytest.raises(Exception, match="belong to LN"):
        cc.plan(d)


def test_matrix_is_covered():
    missing = [(r, sorted(f)) for r, f in cc.MATRIX
               if not any(cc.cell_route(c) == r and f <= cc.features(c) for c in cc.CASES)]
    assert not missing, missing
    print("conv route matrix: %d cells, %d cases, every cell covered" % (len(cc.MATRIX), len(cc.CASES)))


@pytest.mark.parametrize("what,c,expected", cc.PRODUCTION, ids=[p[0] for p in cc.PRODUCTION])
def test_production_shapes(what, c, expected):
    p = cc.plan(cc.desc(c))
    assert p["route"] in expected, (what, p)
    if c["splitk"] and p["route"] == "SMALL":
        assert p["S"] > 1, (what, p)


def test_tile_shapes_of_the_routes():
    shapes = {"M64": (64, 128, 256), "HALF": (64, 384, 256), "SMALL": (128, 128, 256), "BIG": (128, 384, 512),
              "SPLIT_BATCH": (128, 384, 512), "VS": (128, 384, 512)}
    for c in cc.CASES:
        p = cc.plan(cc.desc(c))
        if p["route"] in shapes:
            assert (p["bm"], p["bn"], p["threads"]) == shapes[p["route"]], (c["name"], p)
            K, halo = (c["K"], (c["K"] - 1) * c["dil"]) if c["kind"] == "conv" else (16 // c["kind"] + 1, 16 // c["kind"])
            ck = 32 if K == 1 else 16 if K <= 5 and halo <= 24 else 8
            assert p["ck"] == ck, (c["name"], p)
        if p["route"] not in ("SMALL", "M64"):
            assert p["S"] == 1, (c["name"], p)      # split-K exists on the 256-thread 128-column shapes only


def test_trim_width_is_the_plans():
    """A trimmed launch gets the tile width conv1d_trim_bn builds its map for: the untrimmed launch's own width on the
    routes that do not depend on trimming, 128 or 384 otherwise; never split-K, the narrow kernel, HALF or VS."""
    n = 0
    for c in cc.CASES:
        if c["prec"]:
            continue
        lens = [c["T"]] * c["B"]
        cu = dict(c, trim=None)
        untrimmed = cc.plan(cc.desc(cu, splitk=0))
        ct = dict(c, trim=(1, 0, lens), splitk=0)
        if untrimmed["route"] in ("NARROW_M", "NARROW_LAUNCH"):
            with pytest.raises(Exception, match="conv1d_trim_bn"):
                cc.plan(cc.desc(ct))
            continue
        t = cc.plan(cc.desc(ct))
        n += 1
        assert t["route"] in ("SMALL", "BIG", "M64"), (c["name"], t)
        assert t["bn"] in (128, 384) and t["S"] == 1 and t["nb_big"] == 0 and t["vs_tv"] == 0, t
        if untrimmed["route"] in ("SMALL", "BIG", "M64"):
            assert t == untrimmed, (c["name"], t, untrimmed)
    assert n >= 20
    with pytest.raises(Exception, match="split-K"):
        cc.plan(cc.desc(dict(cc.BY_NAME["small_resid"], trim=(1, 0, [1, 2, 3]), splitk=1)))


def test_prec3_never_plans_vs_or_half():
    for c in cc.CASES + [p[1] for p in cc.PRODUCTION]:
        p = cc.plan(cc.desc(c, prec=3))
        assert p["route"] not in ("VS", "HALF"), (c["name"], p)


def test_bad_descriptors_are_refused_not_fatal():
    base = cc.BY_NAME["small_resid"]
    bad = [cc.desc(c) for c in (
        dict(base, K=13), dict(base, Cin=100), dict(base, kind=5), dict(cc.BY_NAME["small_convt4"], T=10),
        dict(base, epi="STORE", res_chan_add=True), dict(base, accum=True), dict(base, prec=2))]
    for c in (base, cc.BY_NAME["small_convt4"], cc.BY_NAME["small_convt8"]):
        d = cc.desc(c)
        d.legacy_convt = 1                   # the slot stays in the ABI; its kernel is gone
        bad.append(d)
    for d in bad:
        with pytest.raises(Exception):
            cc.plan(d)
