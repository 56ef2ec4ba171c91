"""The bars of attention_cases.py, tested on the CPU: both fp32 oracles (the plain restatement of the reference and the
kernel's tiled algorithm) pass every case at margin 1, every mutant of MUTANTS fails at least one committed case, the
restatement equals ref_infer.relative_attention bit for bit, and the cases reach the tiles, waves, head dimensions and
regimes they are there for.  A mutant that no case separates means a case is missing: add the case, not an exemption."""
import pytest
import torch

import attention_cases as ac

F32, F64 = ac.F32, ac.F64
STATS = {k: ac.Stats() for k in ac.ORACLES}


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    print("\nfp32 oracles, worst case per regime (median, p99.9, max of |y - y64| over valid queries):")
    for k, st in STATS.items():
        for regime in sorted({v["regime"] for v in st.values()}):
            rows = [v for v in st.values() if v["regime"] == regime]
            print("  %-6s %-8s %.3g  %.3g  %.3g" % (k, regime, max(r["median"] for r in rows),
                                                   max(r["p999"] for r in rows), max(r["max"] for r in rows)))


@pytest.mark.parametrize("oracle", list(ac.ORACLES))
@pytest.mark.parametrize("c", ac.ATT_CASES, ids=lambda c: c["name"])
def test_oracle_passes_at_margin_one(c, oracle):
    ac.att_check(c, ac.att_shared(c)[2][oracle], margin=1.0, stats=STATS[oracle])


@pytest.mark.parametrize("mut", list(ac.MUTANTS))
def test_mutant_fails(mut):
    f = ac.ORACLES[ac.MUTANTS[mut]]
    caught, how = [], set()
    for c in ac.ATT_CASES:
        try:
            ac.att_check(c, f(c, ac.att_shared(c)[0], F32, mut))
        except AssertionError as e:
            caught.append(c["name"])
            how.add(e.args[0][1])
    print("%s: caught by %d of %d cases: %s (%s)" % (mut, len(caught), len(ac.ATT_CASES), ", ".join(caught[:6]), sorted(how)))
    assert caught, (mut, "no committed case separates this mutant")
    if mut == "pad_fill_inf":                  # valid queries do not see it: exp(-1e4 - m) and exp(-inf) are both 0
        assert how <= {"non-finite padded query columns", "NaN (pre-fill or computed)"}, how


def test_no_max_sub_passes_the_flat_regime():
    """Why the regimes exist: with every logit around N(0, 1) a kernel that never subtracts the maximum is as close
    to float64 on the valid queries as the oracles are (only a padded query's row, exp(-1e4) = 0 throughout, shows
    it); the shifted cases see it on the valid ones."""
    for c in ac.ATT_CASES:
        if c["regime"] == "flat" and c["emb"] == 0.3:
            inp, ref, orcs = ac.att_shared(c)
            valid = ac.tmask(c["lens"], c["T"]).bool()[:, None, :].expand_as(ref)
            e = (ac.att_tiled(c, inp, F32, "no_max_sub").double() - ref)[valid].abs().max()
            e_o = max((o.double() - ref)[valid].abs().max() for o in orcs.values())
            assert float(e) <= ac.MARGIN * float(e_o), (c["name"], float(e), float(e_o))
    for c in ac.ATT_CASES:
        if c["regime"] == "shifted":
            with pytest.raises(AssertionError):
                ac.att_check(c, ac.att_tiled(c, ac.att_shared(c)[0], F32, "no_max_sub"))


def test_restatement_is_the_oracle():
    for c in ac.ATT_CASES:
        inp = ac.att_shared(c)[0]
        H = c["H"]
        for dt in (F32, F64):
            x = inp["qkv"].to(dt)
            want = ac.R.relative_attention(x[:, :H], x[:, H:2 * H], x[:, 2 * H:], ac.tmask(c["lens"], c["T"], dt),
                                           inp["emb_k"].to(dt), inp["emb_v"].to(dt), c["heads"])
            assert torch.equal(ac.att_compute(c, inp, dt), want), c["name"]


def test_tiled_agrees_with_plain_in_float64():
    """The tiled algorithm is the same function: in float64 it is within 1e-12 of the reference on every case."""
    for c in ac.ATT_CASES:
        inp, ref, _ = ac.att_shared(c)
        assert float((ac.att_tiled(c, inp, F64) - ref).abs().max()) <= 1e-12 * max(1.0, float(ref.abs().max())), c["name"]


def test_cases_cover_the_shapes_and_regimes():
    C = ac.ATT_CASES
    assert {32, 40, 64, 96, 100, 128} == {c["H"] // c["heads"] for c in C}
    assert {1, 2, 4} == {c["heads"] for c in C}
    assert {1, 31, 32, 33, 64, 65, 97} == {c["T"] for c in C}
    assert all(2 <= c["B"] <= 4 for c in C)
    assert {"flat", "sharp", "shifted", "rising", "falling"} == {c["regime"] for c in C} and any(c["emb"] == 3.0 for c in C)
    for dmin, dmax in ((1, 32), (33, 64), (65, 96), (97, 128)):          # every kernel instance meets a moving maximum
        assert any(dmin <= c["H"] // c["heads"] <= dmax and c["regime"] in ("rising", "falling", "shifted") for c in C)
    lens = [(c["T"], l) for c in C for l in c["lens"]]
    assert any(l == T for T, l in lens) and any(l == 1 for T, l in lens) and any(l == 32 and T > 32 for T, l in lens)
    assert any(0 < l % 32 < 31 and 1 < l < T for T, l in lens)
    assert any(T in (64, 65) and 0 < l <= 32 for T, l in lens)            # all of wave 1's key tiles are padding
    assert any(T == 97 and 0 < l <= 64 for T, l in lens)                  # the trailing tile is padding
    # sharp: the median row maximum of p is about 0.5; flat: below 0.1 at T = 97
    for c in C:
        inp, ref, _ = ac.att_shared(c)
        if c["T"] == 97 and c["emb"] == 0.3 and c["regime"] in ("flat", "sharp"):
            p = torch.softmax(ac._scores(c, inp, F64)[0], -1)[0, :, : c["lens"][0]]
            med = float(p.max(-1).values.median())
            assert (med > 0.4) if c["regime"] == "sharp" else (med < 0.15), (c["name"], med)


def test_moving_maximum_cases_do_what_they_say():
    """shifted: the logits of a valid row sit around +100 or -100.  rising / falling: every valid key tile moves the
    running maximum by at least 20, the row maximum is in the last / first valid tile, and over the cases that tile is
    a wave-1 tile (odd) for some rows and a wave-0 tile behind an earlier wave-0 tile (even, >= 2) for others."""
    last_tiles = set()
    for c in ac.ATT_CASES:
        inp = ac.att_shared(c)[0]
        if c["regime"] not in ("shifted", "rising", "falling"):
            continue
        S = ac._scores(c, inp, F64)[0]
        for b, n in enumerate(c["lens"]):
            if n == 0:
                continue
            s = S[b, :, :n, :n]
            if c["regime"] == "shifted":
                mx = s.max(-1).values
                assert bool((mx[:, 0::2] > 89).all()) and bool((s[:, 1::2] < -60).all()), c["name"]
                continue
            nt = (n + 31) // 32
            tmax = torch.stack([s[..., k * 32:min(n, (k + 1) * 32)].max(-1).values for k in range(nt)], -1)
            step = tmax[..., 1:] - tmax[..., :-1]
            if nt > 1:
                assert bool(((step if c["regime"] == "rising" else -step) >= 20).all()), (c["name"], b, float(step.abs().min()))
            if c["regime"] == "rising":
                last_tiles.add(nt - 1)
    assert {1, 2, 3} <= last_tiles, last_tiles
