"""Route table of the conv launcher tests: every route of `launch_conv1d` (conv1d.hip) under every epilogue the
decoder uses.  test_conv_plan.py (CPU) checks that each case plans the route it declares and that the table covers
MATRIX; test_gpu_conv_routes.py (-m gpu) runs each case through `mbv_op_conv` against a float64 reference.

A case is one launch.  `route` is the route it is written for in the default mode (split-K only where the case asks
for it); `pair` marks a large launch whose rows must equal, bitwise, the same rows launched two at a time (a different
route, `pair_route`); `trim` = (num, add, lengths) makes it a trimmed launch, compared with the untrimmed one."""
import ctypes as C

from mb_istft_vits_amd import _capi

WS_FLOATS = 16 << 20      # the handle's split-K workspace and ticket counters (capi.hip, mbv_create)
N_COUNTERS = 8192

EPI = {"STORE": _capi.CONV_EPI_STORE, "RESID": _capi.CONV_EPI_RESID, "RESID_ACC": _capi.CONV_EPI_RESID_ACC,
       "LN": _capi.CONV_EPI_LN}


def ragged(B, T, seed=0):
    """Per-utterance lengths: T, 0, 1, tile boundaries (32, 128, 384), then a spread of ragged values."""
    head = [T, 0, 1, 32, 128, 384, 383, 129]
    out = [min(v, T) for v in head[:B]]
    k = len(out)
    while len(out) < B:
        out.append(1 + (seed * 7919 + k * 104729) % T)
        k += 1
    return out


def case(name, route, B, Cin, Cout, T, kind="conv", epi="STORE", K=3, dil=1, Tin=None, slope=0.1, **kw):
    c = dict(name=name, route=route, B=B, Cin=Cin, Cout=Cout, T=T, Tin=T if Tin is None else Tin, kind=kind,
             epi=epi, K=K, dil=dil, slope=slope, relu=0, reflect1=0, rstride=0, in_lens=None, out_lens=None,
             chan_add=False, res_chan_add=False, accum=False, out_scale=1.0, trim=None, splitk=0, prec=0,
             pair=False, pair_route=None, S_gt1=False, check=None, seed=len(name), ln_res=False, ln_out_lens=None)
    for k, v in kw.items():
        assert k in c, k
        c[k] = v
    return c


def features(c):
    """What a case exercises, as the labels MATRIX uses."""
    f = {c["epi"] if c["kind"] == "conv" else "CONVT%d" % c["kind"]}
    if c["kind"] != "conv":
        f.add("CONVT")
    for k in ("in_lens", "out_lens", "chan_add", "res_chan_add", "accum", "reflect1"):
        if c[k]:
            f.add(k)
    if c["rstride"]:
        f.add("x_rstride")
    if c["out_scale"] != 1.0:
        f.add("out_scale")
    if c["trim"]:
        lens, T = c["trim"][2], c["T"]
        if 0 in lens:
            f.add("zero_len")
        if any(0 < v < T and v % 128 == 0 for v in lens):
            f.add("tile_len")
    return f


def cell_route(c):
    """The matrix row a case belongs to."""
    r = c["route"]
    if c["trim"]:
        return "TRIM_%d" % (384 if r == "BIG" else 128)
    if c["prec"] == 3:
        return "PREC3_" + r
    if r == "SMALL" and c["S_gt1"]:
        return "SMALL_SPLITK"
    if r == "HALF":
        return "HALF_CK16" if c["K"] <= 5 and (c["K"] - 1) * c["dil"] <= 24 else "HALF_CK8"
    return r


# (matrix row, features a case of that row must have); each cell needs at least one case
MATRIX = [
    ("NARROW_M", {"STORE", "in_lens", "out_lens"}), ("NARROW_M", {"RESID"}),
    ("NARROW_M", {"RESID_ACC", "accum", "out_scale"}),
    ("NARROW_LAUNCH", {"STORE", "chan_add"}), ("NARROW_LAUNCH", {"RESID", "res_chan_add"}),
    ("NARROW_LAUNCH", {"RESID_ACC"}),
    ("SMALL_SPLITK", {"CONVT4"}), ("SMALL_SPLITK", {"STORE", "reflect1"}),
    ("M64", {"RESID"}), ("M64", {"RESID_ACC"}),
    ("HALF_CK16", {"RESID"}), ("HALF_CK16", {"RESID_ACC"}), ("HALF_CK8", {"RESID"}), ("HALF_CK8", {"RESID_ACC"}),
] + [(r, f) for r in ("SMALL", "BIG") for f in (
    {"STORE", "in_lens", "x_rstride"}, {"RESID"}, {"RESID_ACC", "accum"}, {"CONVT4"}, {"CONVT8"}, {"reflect1"})] + [
    ("SPLIT_BATCH", {"RESID", "chan_add", "res_chan_add"}), ("SPLIT_BATCH", {"RESID_ACC", "accum"}),
    ("SPLIT_BATCH", {"CONVT4"}),
    ("VS", {"CONVT4"}),
] + [(r, f) for r in ("TRIM_128", "TRIM_384") for f in (
    {"STORE"}, {"RESID"}, {"RESID_ACC"}, {"CONVT"}, {"zero_len"}, {"tile_len"})] + [
    ("PREC3_" + r, {f}) for r in ("SMALL", "BIG", "SPLIT_BATCH") for f in ("RESID", "RESID_ACC", "CONVT")]

THIRD = 1.0 / 3.0
CASES = [
    # -- narrow kernel, row blocks by M (T <= 256: the text encoder's rule)
    case("narrow_store_lens", "NARROW_M", 5, 64, 96, 200, K=5, in_lens=ragged(5, 200, 1), out_lens=ragged(5, 200, 2),
         relu=1),
    case("narrow_resid", "NARROW_M", 3, 96, 64, 255, epi="RESID", K=3, dil=3, res_chan_add=True),
    case("narrow_resacc", "NARROW_M", 3, 64, 128, 256, epi="RESID_ACC", K=7, accum=True, out_scale=THIRD),
    # -- narrow kernel by launch size (split-K mode, one utterance)
    case("narrowl_store_cadd", "NARROW_LAUNCH", 1, 128, 128, 767, K=3, chan_add=True, splitk=1),
    case("narrowl_resid_rcadd", "NARROW_LAUNCH", 1, 128, 128, 767, epi="RESID", K=3, dil=3, res_chan_add=True,
         splitk=1),
    case("narrowl_resacc", "NARROW_LAUNCH", 1, 128, 128, 767, epi="RESID_ACC", K=7, accum=True, out_scale=THIRD,
         splitk=1),
    # -- 128 x 128 tiles with split-K (S > 1)
    case("splitk_convt4", "SMALL", 1, 256, 128, 383, kind=4, splitk=1, S_gt1=True),
    case("splitk_post", "SMALL", 1, 128, 72, 384, Tin=383, K=7, reflect1=1, slope=0.01, splitk=1, S_gt1=True),
    # -- <= 64 rows: 64 x 384 (HALF, CK 16 / 8) at B = 256, each row again at B = 2 on 64 x 128 (M64)
    case("half16_resid", "HALF", 256, 64, 64, 767, epi="RESID", K=3, dil=5, pair=True, pair_route="M64"),
    case("half16_resacc", "HALF", 256, 64, 64, 767, epi="RESID_ACC", K=3, dil=5, accum=True, out_scale=THIRD,
         pair=True, pair_route="M64"),
    case("half8_resid", "HALF", 256, 64, 64, 767, epi="RESID", K=7, pair=True, pair_route="M64"),
    case("half8_resacc", "HALF", 256, 64, 64, 767, epi="RESID_ACC", K=11, dil=5, accum=True, pair=True,
         pair_route="M64"),
    case("m64_resid", "M64", 3, 64, 64, 767, epi="RESID", K=11, dil=5),
    case("m64_resacc", "M64", 3, 64, 64, 767, epi="RESID_ACC", K=3, dil=5, accum=True, out_scale=THIRD),
    # -- 128 x 128 tiles
    case("small_pre", "SMALL", 3, 192, 512, 566, K=7, rstride=600, in_lens=[566, 0, 383]),
    case("small_resid", "SMALL", 3, 128, 128, 767, epi="RESID", K=7, dil=3),
    case("small_resacc", "SMALL", 3, 128, 128, 767, epi="RESID_ACC", K=11, dil=5, accum=True, out_scale=THIRD),
    case("small_convt4", "SMALL", 2, 256, 128, 566, kind=4),
    case("small_convt8", "SMALL", 2, 128, 64, 385, kind=8),
    case("small_post", "SMALL", 2, 128, 72, 384, Tin=383, K=7, reflect1=1, slope=0.01),
    # -- 128 x 384 tiles, each row again at B = 2 on 128 x 128 tiles
    case("big_pre", "BIG", 64, 192, 512, 767, K=7, rstride=800, in_lens=ragged(64, 767, 3), pair=True,
         pair_route="SMALL"),
    case("big_resid", "BIG", 64, 128, 128, 3071, epi="RESID", K=3, dil=3, pair=True, pair_route="SMALL"),
    case("big_resacc", "BIG", 64, 128, 128, 3071, epi="RESID_ACC", K=11, dil=5, accum=True, out_scale=THIRD,
         pair=True, pair_route="SMALL"),
    case("big_convt4", "BIG", 64, 256, 128, 767, kind=4, pair=True, pair_route="SMALL"),
    case("big_convt8", "BIG", 64, 128, 64, 767, kind=8, pair=True, pair_route="SMALL"),
    case("big_post", "BIG", 64, 128, 72, 3072, Tin=3071, K=7, reflect1=1, slope=0.01, pair=True, pair_route="SMALL"),
    # -- the batch cut (uudb B = 32, stage 0: 256 channels, T' = 566 -> 2264 frames), rows again at B = 2
    case("split_resid_cond", "SPLIT_BATCH", 32, 256, 256, 2264, epi="RESID", K=3, chan_add=True, res_chan_add=True,
         pair=True, pair_route="SMALL"),
    case("split_resacc", "SPLIT_BATCH", 32, 256, 256, 2264, epi="RESID_ACC", K=11, dil=5, accum=True,
         out_scale=THIRD, res_chan_add=True, pair=True, pair_route="SMALL"),
    case("split_convt4", "SPLIT_BATCH", 32, 128, 64, 2264, kind=4, chan_add=True, pair=True, pair_route="SMALL"),
    # -- virtual-sequence tiling of the stride-4 ConvTranspose (ljs_mb B = 64, T' = 566), rows again at B = 2
    case("vs_512", "VS", 64, 512, 256, 566, kind=4, pair=True, pair_route="SMALL"),
    case("vs_256", "VS", 128, 256, 128, 567, kind=4, pair=True, pair_route="SMALL"),       # last virtual tile ragged
    case("vs_ragged", "VS", 61, 512, 256, 385, kind=4, pair=True, pair_route="SMALL"),
    # -- trimmed launches (compact tile lists) against the untrimmed one
    case("trim128_store", "SMALL", 3, 128, 128, 767, K=7, trim=(1, 0, [0, 128, 500])),
    case("trim128_resid", "SMALL", 3, 128, 128, 767, epi="RESID", K=3, dil=5, trim=(1, 0, [256, 0, 767])),
    case("trim128_resacc", "SMALL", 3, 128, 128, 767, epi="RESID_ACC", K=11, accum=True, out_scale=THIRD,
         trim=(1, 3, [100, 125, 0])),
    case("trim128_convt", "SMALL", 3, 256, 128, 566, kind=4, trim=(1, 0, [566, 0, 128])),
    case("trim384_store", "BIG", 64, 192, 512, 767, K=7, trim=(1, 0, ragged(64, 767, 5))),
    case("trim384_resid", "BIG", 64, 128, 128, 3071, epi="RESID", K=3, trim=(1, 0, ragged(64, 3071, 6))),
    case("trim384_resacc", "BIG", 64, 128, 128, 3071, epi="RESID_ACC", K=7, accum=True, out_scale=THIRD,
         trim=(4, 0, ragged(64, 767, 7))),
    case("trim384_convt", "BIG", 64, 256, 128, 767, kind=4, trim=(1, 0, ragged(64, 767, 8))),
    # -- split-bf16 arithmetic (prec 3)
    case("prec3_small_resid", "SMALL", 3, 128, 128, 767, epi="RESID", K=7, prec=3),
    case("prec3_small_resacc", "SMALL", 3, 128, 128, 767, epi="RESID_ACC", K=3, dil=5, accum=True,
         out_scale=THIRD, prec=3),
    case("prec3_small_convt", "SMALL", 2, 256, 128, 566, kind=4, prec=3),
    case("prec3_big_resid", "BIG", 64, 128, 128, 3071, epi="RESID", K=3, prec=3),
    case("prec3_big_resacc", "BIG", 64, 128, 128, 3071, epi="RESID_ACC", K=11, dil=5, accum=True, prec=3),
    case("prec3_big_convt", "BIG", 64, 256, 128, 767, kind=4, prec=3),
    case("prec3_split_resid", "SPLIT_BATCH", 32, 256, 256, 2264, epi="RESID", K=3, chan_add=True,
         res_chan_add=True, prec=3),
    case("prec3_split_resacc", "SPLIT_BATCH", 32, 256, 256, 2264, epi="RESID_ACC", K=7, accum=True,
         out_scale=THIRD, prec=3),
    case("prec3_split_convt", "SPLIT_BATCH", 32, 128, 64, 2264, kind=4, chan_add=True, prec=3),
]
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def _ln_site(site, H, T, B=3, Fc=768, rot=0):
    """The conv + LayerNorm launches of mbv_encode (EPI_LN, conv1d_narrow.hip) as it sets them: `conv_o` (K 1, residual),
    `ffn2` (K 3, in_lens, out_lens, residual, the mask behind the LayerNorm in the last layer only), `dp1` / `dp2` (K 3, relu, in_lens, dp1 with
    the speaker's chan_add).  No activation on the input (slope 1)."""
    pool = [T, 0, 1, max(1, min(T - 1, T // 2 // 32 * 32 + 13))]
    lens = [pool[(i + rot) % 4] for i in range(B)]
    kw = {"conv_o": dict(Cin=H, Cout=H, K=1, ln_res=True),
          "ffn2": dict(Cin=Fc, Cout=H, K=3, in_lens=lens, out_lens=lens, ln_res=True, ln_out_lens=lens),   # the last layer
          "ffn2i": dict(Cin=Fc, Cout=H, K=3, in_lens=lens, out_lens=lens, ln_res=True),                    # the layers before it
          "dp1": dict(Cin=H, Cout=256, K=3, relu=1, chan_add=True, in_lens=lens),
          "dp2": dict(Cin=256, Cout=256, K=3, relu=1, in_lens=lens)}[site]
    return case("ln_%s_h%d_t%d" % (site, H, T), "NARROW_M", B, kw.pop("Cin"), kw.pop("Cout"), T, epi="LN", slope=1.0,
                **kw)


# conv + channel LayerNorm in one launch: not part of CASES / MATRIX (the decoder's matrix); test_conv_plan.py pins their
# route, test_gpu_small_ops.py runs them against the float64 reference of small_op_cases.py
LN_CASES = [
    _ln_site("conv_o", 192, 1), _ln_site("conv_o", 192, 33, rot=1), _ln_site("conv_o", 192, 200), _ln_site("conv_o", 192, 256, rot=2),
    _ln_site("ffn2", 192, 1, rot=2), _ln_site("ffn2", 192, 33), _ln_site("ffn2", 192, 200, rot=1), _ln_site("ffn2", 192, 256, rot=3),
    _ln_site("dp1", 192, 1), _ln_site("dp1", 192, 33, rot=3), _ln_site("dp1", 192, 200, rot=2), _ln_site("dp1", 192, 256),
    _ln_site("dp2", 192, 1, rot=3), _ln_site("dp2", 192, 33, rot=2), _ln_site("dp2", 192, 200), _ln_site("dp2", 192, 256, rot=1),
    # the mini configuration: 96 hidden channels
    _ln_site("conv_o", 96, 33), _ln_site("conv_o", 96, 256, rot=1), _ln_site("ffn2", 96, 1, rot=1), _ln_site("ffn2", 96, 200, rot=2),
    _ln_site("dp1", 96, 33, rot=1), _ln_site("dp1", 96, 256, rot=3),
    _ln_site("ffn2i", 192, 33, rot=1), _ln_site("ffn2i", 192, 200), _ln_site("ffn2i", 96, 256, rot=2),
]
LN_BY_NAME = {c["name"]: c for c in LN_CASES}
assert len(LN_BY_NAME) == len(LN_CASES)

# ljs_mb B = 64, T' = 566 (bench shape) and uudb B = 32 (the per-GPU share of the sharded configuration): DESIGN §3
PRODUCTION = [
    # (what, case, expected routes)
    ("ljs_mb ups[0]", case("p_ups0", "VS", 64, 512, 256, 566, kind=4), {"VS"}),
    ("ljs_mb stage-1 ResBlock conv", case("p_rb1", "BIG", 64, 128, 128, 9056, epi="RESID", K=7), {"BIG"}),
    ("ljs_mb stage-1 running sum", case("p_rb1_acc", "BIG", 64, 128, 128, 9056, epi="RESID_ACC", K=11, dil=5,
                                        accum=True), {"BIG"}),
    ("uudb stage-0 conv (cond)", case("p_uudb_c1", "SPLIT_BATCH", 32, 256, 256, 2264, K=3, chan_add=True),
     {"SPLIT_BATCH"}),
    ("uudb stage-0 residual", case("p_uudb_c2", "SPLIT_BATCH", 32, 256, 256, 2264, epi="RESID", K=3,
                                   res_chan_add=True), {"SPLIT_BATCH"}),
    ("ljs_mini stage-1 ResBlock conv", case("p_mini_rb1", "HALF", 64, 64, 64, 9056, epi="RESID", K=3, dil=5),
     {"HALF", "M64"}),
    ("B = 1 split-K, 128 channels", case("p_b1_rb", "NARROW_LAUNCH", 1, 128, 128, 2264, epi="RESID", K=3,
                                         splitk=1), {"NARROW_LAUNCH", "SMALL"}),
    ("B = 1 split-K, ups[0]", case("p_b1_ups0", "SMALL", 1, 512, 256, 566, kind=4, splitk=1),
     {"NARROW_LAUNCH", "SMALL"}),
]


def desc(c, B=None, ptrs=None, splitk=None, prec=None, trim=True, ws=True):
    """mbv_conv_desc of a case.  ptrs: device pointers by field name; without them every option the case uses gets a
    non-null placeholder (mbv_conv_plan only tests them against null)."""
    d = _capi.MbvConvDesc()
    d.B = c["B"] if B is None else B
    d.Cin, d.Cout, d.Tin, d.T = c["Cin"], c["Cout"], c["Tin"], c["T"]
    d.K, d.dil = (c["K"], c["dil"]) if c["kind"] == "conv" else (0, 1)
    d.x_rstride = c["rstride"]
    d.kind = _capi.CONV_KIND_CONV if c["kind"] == "conv" else c["kind"]
    d.epi = EPI[c["epi"]]
    d.in_slope, d.relu, d.reflect1 = c["slope"], c["relu"], c["reflect1"]
    d.out_scale = c["out_scale"]
    want = {"in_lens": c["in_lens"] is not None, "out_lens": c["out_lens"] is not None, "chan_add": c["chan_add"],
            "res": c["epi"] in ("RESID", "RESID_ACC") or c["ln_res"], "ln_out_lens": c["ln_out_lens"] is not None,
            "ln_gamma": c["epi"] == "LN", "ln_beta": c["epi"] == "LN", "res_chan_add": c["res_chan_add"], "accum_in": c["accum"]}
    for k, on in want.items():
        if on:
            setattr(d, k, (ptrs or {}).get(k, 1 << 20))
    keep = []
    if trim and c["trim"]:
        num, add, lens = c["trim"]
        arr = (C.c_int64 * len(lens))(*lens)
        keep.append(arr)
        d.trim_lens = C.cast(arr, C.c_void_p)
        d.trim_num, d.trim_add = num, add
    d.splitk = c["splitk"] if splitk is None else splitk
    d.prec = c["prec"] if prec is None else prec
    if ws:
        d.ws_floats, d.n_counters = WS_FLOATS, N_COUNTERS
    d._keep = keep                       # the trim lengths live as long as the descriptor
    return d


def plan(d):
    """mbv_conv_plan as a dict (route by name)."""
    L = _capi.lib()
    out = (C.c_int32 * 8)()
    if L.mbv_conv_plan(C.byref(d), C.byref(out)):
        raise _capi.MbvError(L.mbv_last_error(None).decode())
    p = dict(zip(_capi.PLAN_FIELDS, list(out)))
    p["route"] = _capi.ROUTES[p["route"]]
    return p
