"""The bars of wn_stack_ref.py, tested on the CPU before any GPU run: in every case and stage the `folded` fp32 oracle
(what do_finalize packs and gate_fast computes) lies inside bars built from the `plain` oracle alone, so the fold's
rounding fits the margin; every mutant a case lists fails at least one bar of that case (the bars built from the
largest of all the oracle variants any route of the case uses, the in_place one included); the restatement in float32 is ref_infer's own result.  And
the host rule that decides what do_finalize may fold (wn_prefold_fits / wn_postfold_fits of csrc/wn_fused.hip), which
needs no GPU.  A mutant that a case cannot separate means the case is wrong about what it reaches: fix the case."""
import ctypes as C
import functools

import pytest
import torch

import wn_stack_ref as wr
from helpers import config_for
from mb_istft_vits_amd import _capi, synth
from oracle import ref_infer as R

F32, F64 = wr.F32, wr.F64
IN_PLACE = {c["name"] for c in wr.CASES for r in ("fused", "two_launch")
            if "in_place" in wr.variants(c, r) and (r == c["route"] or c["name"] in wr.TWO_LAUNCH_AGAIN)}


@functools.lru_cache(maxsize=None)
def _setup(name):
    """(cfg, weights, inputs, per stage: its fp32 input, float64 reference, plain and folded fp32 oracle)"""
    c = wr.BY_NAME[name]
    _, cfg = config_for(c["cfg"], overrides=c["overrides"])
    W = wr.Weights(synth.make_state_dict(cfg, 1234))
    inp = wr.inputs(c, spec_channels=cfg.spec_channels)
    lens, fold = c["lens"], c["fold"]
    g = W.g(inp["sid"], F64)
    enc = lambda dt, **k: wr.posterior_encoder(W, cfg, inp["y"], lens, g, inp["noise"], dt, **k)[0]
    st = {"enc": dict(ref=enc(F64), plain=enc(F32), folded=enc(F32, variant="folded"))}
    z_in = st["enc"]["plain"]                                    # stands for the GPU's z: an fp32 tensor near the reference
    fwd = lambda dt, **k: wr.flow_forward(W, cfg, z_in, lens, g, dt, fold=fold, **k)
    st["fwd"] = dict(ref=fwd(F64), plain=fwd(F32), folded=fwd(F32, variant="folded"))
    zp_in = st["fwd"]["plain"]
    rev = lambda dt, **k: wr.flow_reverse(W, cfg, zp_in, lens, g, dt, fold=fold, **k)
    st["rev"] = dict(ref=rev(F64), plain=rev(F32), folded=rev(F32, variant="folded"))
    if name in IN_PLACE:                                         # the routes that run convs which accumulate in place
        for stage, run in (("enc", enc), ("fwd", fwd), ("rev", rev)):
            st[stage]["in_place"] = run(F32, variant="in_place")
    return c, cfg, W, inp, st, dict(enc=enc, fwd=fwd, rev=rev)


NAMES = [c["name"] for c in wr.CASES]


@pytest.mark.parametrize("name", sorted(IN_PLACE))
def test_in_place_oracle(name):
    """The in_place oracle (what the two-launch layer and EPI_COUPLE compute) is printed next to the plain one; it is
    correct fp32 code — inside MARGIN x its own error trivially — and its error is the plain oracle's times a factor
    that the sizes explain (about sqrt(H) / 2 roundings at the size of x1): at most 3 x in the median, 8 x above."""
    c, cfg, W, inp, st, _ = _setup(name)
    for stage, s in st.items():
        p, q = wr.err_stats(s["plain"], s["ref"], c["lens"]), wr.err_stats(s["in_place"], s["ref"], c["lens"])
        print("%s %s in_place median %.3g  p99.9 %.3g  max %.3g   = plain x %.2f  %.2f  %.2f" % ((name, stage) + q + tuple(b / a for a, b in zip(p, q))))
        assert q[0] <= 3.5 * p[0] and q[1] <= 8 * p[1] and q[2] <= 10 * p[2], (name, stage, p, q)


@pytest.mark.parametrize("name", NAMES)
def test_folded_oracle_is_inside_the_plain_bars(name):
    c, cfg, W, inp, st, _ = _setup(name)
    for stage, s in st.items():
        for v in ("plain", "folded"):
            print("%s %s %-6s oracle median %.3g  p99.9 %.3g  max %.3g" % ((name, stage, v) + wr.err_stats(s[v], s["ref"], c["lens"])))
        wr.check_stage("%s/%s folded vs plain bars" % (name, stage), s["folded"], s["ref"], [s["plain"]], c["lens"])
        # and the other way round: neither oracle is the loose one
        wr.check_stage("%s/%s plain vs folded bars" % (name, stage), s["plain"], s["ref"], [s["folded"]], c["lens"])


MUT = [(c["name"], m) for c in wr.CASES for m in c["mutants"]]


@pytest.mark.parametrize("name,mut", MUT, ids=["%s-%s" % nm for nm in MUT])
def test_mutant_fails(name, mut):
    c, cfg, W, inp, st, run = _setup(name)
    caught = []
    for stage, s in st.items():
        if mut not in wr.SHOWS_IN[stage]:
            continue
        got = run[stage](F32, mut=mut)
        got = got * wr.fmask(c["lens"], c["T"], F32)             # (only the valid frames are asked: the bars, not the padding test)
        try:
            wr.check_stage("%s/%s %s" % (name, stage, mut), got, s["ref"], [s[v] for v in s if v != "ref"], c["lens"])
        except AssertionError:
            caught.append(stage)
    print("%s / %s: caught in %s" % (name, mut, ", ".join(caught) or "no stage"))
    assert caught, (name, mut, "this case does not separate the mutant")


def test_restatement_is_the_oracle():
    """In float32 and without a mutant, the dtype-generic restatement is ref_infer's own arithmetic (same operations,
    same order): equal to a few ulp of the weight-norm fold, which ref_infer does in float32."""
    c, cfg, W, inp, st, _ = _setup("h192_i192_g")
    sd = synth.make_state_dict(cfg, 1234)
    RW = R.Weights({k: torch.from_numpy(v) for k, v in sd.items()})
    lens = torch.tensor(c["lens"])
    g = RW["emb_g.weight"][inp["sid"]].unsqueeze(-1)
    with torch.no_grad():
        z, _, _, mask = R.posterior_encoder(RW, cfg, inp["y"], lens, g, inp["noise"])
        z_p = R.flow_forward(RW, cfg, st["enc"]["plain"], mask, g)
        z_r = R.flow_reverse(RW, cfg, st["fwd"]["plain"], mask, g)
    for stage, theirs in (("enc", z), ("fwd", z_p), ("rev", z_r)):
        bar, orc, ulp = wr.bars(st[stage]["ref"], [st[stage]["plain"]], c["lens"])
        e = wr.err_stats(theirs, st[stage]["ref"], c["lens"])
        assert all(x <= 2 * o + ulp for x, o in zip(e, orc)), (stage, e, orc)


def test_cases_reach_the_edges():
    for c in wr.CASES:
        assert set(c["lens"]) - {c["T"]} <= wr.EDGE_LENGTHS or c["name"] == "many_tiles", c["name"]
        assert set(c["mutants"]) <= set(wr.MUTANTS)
    by = wr.BY_NAME
    assert wr.half_units(by["h192_i192_g"]["lens"]) == 11                        # odd: the last tile's second half is empty
    assert wr.half_units(by["many_tiles"]["lens"]) == 1250                       # 625 tiles > the 512 workgroups of a launch
    assert any(wr.half_units(c["lens"]) % 2 == 0 for c in wr.CASES)
    seen = set().union(*(c["lens"] for c in wr.CASES))
    assert wr.EDGE_LENGTHS <= seen, wr.EDGE_LENGTHS - seen
    assert set(wr.MUTANTS) == set().union(*(c["mutants"] for c in wr.CASES))
    assert {c["fold"] for c in wr.CASES if c["route"] == "fused"} == {"pre+post", "post", "none"}


def _fits(name, H, I):
    f = getattr(_capi.lib(), name)                               # host functions of namespace mbv (csrc/wn_fused.hip)
    f.argtypes, f.restype = [C.c_int, C.c_int], C.c_bool
    return bool(f(H, I))


def test_fold_capacity_rule():
    """What do_finalize asks before it folds `pre` / `post` into the fused WN layers.  `pre`: the window of layer 0
    holds x0' = [x0 ; mask] in Gi = ceil((I / 2 + 1) / 8) groups, and the kernel stages at most 16 (H <= 128) or 24
    (H = 160, 192) of them; a layer beyond that would leave the mask / bias group out of LDS and read what an earlier
    tile left there.  `post`: H + I / 2 rows of the res/skip GEMM against 256 / 384 row slots."""
    pre = lambda H, I: _fits("_ZN3mbv15wn_prefold_fitsEii", H, I)
    post = lambda H, I: _fits("_ZN3mbv16wn_postfold_fitsEii", H, I)
    assert not pre(64, 256) and not pre(128, 256) and not pre(192, 384)          # Gi = 17 > 16, 17 > 16, 25 > 24
    assert pre(192, 192) and pre(96, 192)                                        # Gi = 13
    assert pre(160, 256) and pre(64, 192) and pre(128, 128) and pre(160, 64)     # 17 <= 24, 13, 9, 5
    assert pre(128, 254) and pre(192, 382)                                       # the last sizes that fit: Gi = 16, 24
    assert not pre(224, 192) and not post(224, 192)                              # not a fused size at all
    assert post(64, 256) and post(128, 256) and post(192, 384) and post(192, 192) and post(96, 192)
    assert not post(128, 384) and not post(96, 384) and post(96, 320) and post(160, 384) and not post(32, 512)
    for c in wr.CASES:                                                            # the cases say what their sizes fold
        want = "none" if not post(c["H"], c["I"]) else "pre+post" if pre(c["H"], c["I"]) else "post"
        assert c["fold"] == want, (c["name"], want)
