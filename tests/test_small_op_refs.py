"""The bars of small_op_cases.py, tested on the CPU: for every case the fp32 oracle passes its check at a quarter of
the element tolerance and margin 1 (the bars are reachable by correct fp32 code), and every mutated fp32 restatement
of MUTANTS fails the check on at least one committed case (the bars see the mistakes they are there for).  A mutant
that no case separates means a case is missing: add the case, not an exemption."""
import pytest
import torch

import conv_cases as cc
import small_op_cases as sc

F32, F64 = sc.F32, sc.F64
STATS = sc.Stats()


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    print("\nfp32 oracle, worst err / (u A) per kernel (TOL = 4 x, rounded up to one digit):")
    for k, v in sorted(STATS.items()):
        print("  %-12s %.3g   TOL %g" % (k, v["err_over_uA"], v["TOL"]))
        assert 4 * v["err_over_uA"] <= v["TOL"], (k, v)


ORACLE = dict(tol_scale=0.25, margin=1.0, stats=STATS)

# family -> (cases, inputs, the fp32 restatement as the `got` of the check, the check)
FAMILIES = {
    "layernorm": (sc.LN_CASES, sc.ln_inputs, lambda c, i, mut=None: sc.ln_compute(c, i, F32, mut), sc.ln_check),
    "conv_ln": (cc.LN_CASES, sc.cln_inputs, lambda c, i, mut=None: sc.cln_compute(c, i, F32, mut), sc.cln_check),
    "dds_sep": (sc.DDS_CASES, sc.dds_inputs, lambda c, i, mut=None: sc.dds_sep_compute(c, i, F32, mut), sc.dds_sep_check),
    "dds_res": (sc.DDS_CASES, sc.dds_inputs, lambda c, i, mut=None: sc.dds_res_compute(c, i, F32, mut), sc.dds_res_check),
    "spline": (sc.SPLINE_CASES, sc.spline_inputs, lambda c, i, mut=None: sc.spline_compute(c, i, F32, mut), sc.spline_check),
}


def _dur_got(c, inp, mut=None):
    o = sc.dur_compute(c, inp, F32, mut)
    return dict(logw=o["logw"], w_ceil=o["w_ceil"], **sc.dur_tail(c, inp, o["w_ceil"]))


def _exp_got(c, inp, mut=None):
    return sc.exp_compute(c, inp, F32, mut)


FAMILIES["durations"] = (sc.DUR_CASES, sc.dur_inputs, _dur_got, sc.dur_check)
FAMILIES["expand"] = (sc.EXP_CASES, sc.exp_inputs, _exp_got, sc.exp_check)
ALL = [(f, c) for f, v in FAMILIES.items() for c in v[0]]


@pytest.mark.parametrize("family,c", ALL, ids=["%s-%s" % (f, c["name"]) for f, c in ALL])
def test_oracle_passes_at_a_quarter_of_the_bar(family, c):
    _, inputs, got, check = FAMILIES[family]
    inp = inputs(c)
    check(c, inp, got(c, inp), **ORACLE)


@pytest.mark.parametrize("c", sc.LIN_CASES, ids=lambda c: c["name"])
def test_linear_oracle_passes_at_a_quarter_of_the_bar(c):
    inp = sc.lin_inputs(c)
    sc.lin_check(c, inp, {"y": sc.lin_compute(c, inp, F32)}, **ORACLE)


MUT = [(f, m) for f, ms in sc.MUTANTS.items() for m in ms]


@pytest.mark.parametrize("family,mut", MUT, ids=["%s-%s" % fm for fm in MUT])
def test_mutant_fails(family, mut):
    cases, inputs, got, check = FAMILIES[family]
    caught = []
    for c in cases:
        inp = inputs(c)
        try:
            check(c, inp, got(c, inp, mut))
        except AssertionError:
            caught.append(c["name"])
    print("%s / %s: caught by %d of %d cases: %s" % (family, mut, len(caught), len(cases), ", ".join(caught[:6])))
    assert caught, (family, mut, "no committed case separates this mutant")


def test_exact_expectations_are_self_consistent():
    """The bitwise expectations against an independent float64 route (exact: products of fp32 fit a double)."""
    for c in sc.EXACT_CASES:
        inp = sc.exact_inputs(c)
        e = sc.exact_expected(c, inp)
        if c["kind"] == "chan_add":
            assert torch.equal(e["x"], (inp["x"].double() + inp["v"].double()[:, :, None]).float())
        if c["kind"] == "embed":
            assert e["bad"].tolist() == [int(bool(c["bad_ids"] and b in (0, c["B"] - 1)) or not 0 <= l <= c["T"])
                                         for b, l in enumerate(c["lens"])]
            assert bool((e["x"][:, :, -1][torch.tensor(c["lens"]) < c["T"]] == 0).all())
        if c["kind"] == "lens":
            assert e["mask"].sum(1).tolist() == [min(max(l, 0), c["T"]) for l in c["lens"]]


def test_spline_restatement_is_the_oracle():
    """spline_terms (the restatement that exposes the intermediates of the bound) equals ref_infer.rq_spline_inverse
    bit for bit, in both precisions."""
    for c in sc.SPLINE_CASES[:4]:
        inp = sc.spline_inputs(c)
        for dt in (F32, F64):
            i = sc._d(inp, dt)
            uw, uh, ud = sc._spline_params(c, i)
            a = sc.R.rq_spline_inverse(i["z"][:, 0], uw, uh, ud)
            b = sc.spline_terms(i["z"][:, 0], uw, uh, ud)["out"]
            assert torch.equal(a, b), c["name"]


def test_expand_restatement_is_the_oracle():
    """exp_compute's gather equals ref_infer.length_regulate (the reference's one-hot path and matmul) in float64."""
    for name in ("exp_t5_lead_zero_above", "exp_t31_mid_zero_below", "exp_t257_zero_row"):
        c = next(x for x in sc.EXP_CASES if x["name"] == name)
        dc = sc.DUR_BY_NAME[c["dur"]]
        di, inp = sc.dur_inputs(dc), sc.exp_inputs(c)
        m = sc.tmask(dc["lens"], dc["T"])[:, None, :]
        I = c["I"]
        st = inp["stats"].double()
        logw = sc.dur_logw(dc, di, F64)
        logw = torch.where(logw < -150, torch.full_like(logw, -float("inf")), logw)     # 0 in fp32 (dur_compute)
        w_ceil, ylen, y_mask, attn, m_e, logs_e = sc.R.length_regulate(
            logw[:, None, :], m, st[:, :I] * m, st[:, I:] * m, dc["ls"], t_frames=inp["Tp"])
        assert torch.equal(ylen.to(torch.int32), inp["ylen"])
        inp_m = dict(inp, stats=(st * m).float())           # (the kernel gathers what it is given; the reference masks)
        ref = sc.exp_compute(c, inp_m, F64)
        assert torch.equal(ref["attn"], attn[:, 0].double()) and torch.equal(ref["y_mask"], y_mask[:, 0].double())
        assert torch.equal(ref["m_p"], m_e) and torch.equal(ref["logs_p"], logs_e), name


def test_cases_cover_the_shapes():
    Ts = {c["T"] for c in sc.LN_CASES} | {c["T"] for c in sc.DDS_CASES}
    assert {1, 5, 31, 32, 33, 255, 256, 257, 1000} <= Ts
    assert {32, 96, 160, 192, 256} <= {c["C"] for c in sc.LN_CASES}
    assert {1, 3, 64} <= {c["B"] for c in sc.LN_CASES} and {1, 3, 64} <= {c["B"] for c in sc.DUR_CASES}
    assert {1, 255, 256, 257} <= {c["T"] for c in sc.DUR_CASES}
    assert {1, 3, 9} == {c["dil"] for c in sc.DDS_CASES}
    for c in sc.LN_CASES + sc.DDS_CASES + sc.SPLINE_CASES + sc.DUR_CASES:
        if c["B"] == 64 and c.get("lens") is not None:
            assert {0, 1, c["T"]} <= set(c["lens"]) and any(0 < v % 32 < 31 and 1 < v < c["T"] for v in c["lens"]), c["name"]
