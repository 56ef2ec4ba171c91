"""The bars of resample_cases.py, tested on the CPU: the fp32 oracle passes every committed case at a quarter of the
element tolerance and margin 1, every mutated restatement of MUTANTS fails the bars on a named committed case, the
premises about reaching from below hold on the reference alone, and `resample_at` is `resample_ref.resample`."""
import numpy as np
import pytest

import resample_cases as rc
import resample_ref as RR

F32, F64 = rc.F32, rc.F64
STATS = {k: rc.Stats() for k in ("rows", "ranges", "long")}
ORACLE = dict(tol_scale=0.25, margin=1.0)


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    print("\nfp32 oracle, worst err / (u A) (TOL = 4 x, rounded up to one digit):")
    for k, s in STATS.items():
        for v in s.values():
            print("  %-8s %.3g   TOL %g" % (k, v["err_over_uA"], v["TOL"]))
            assert 4 * v["err_over_uA"] <= v["TOL"], (k, v)


def _oracle(c):
    return lambda row, ts: rc.apply_bank_at(row, ts, c["orig"], c["target"], c["res_type"], F32)


@pytest.mark.parametrize("c", rc.GROUPS, ids=lambda c: c["name"])
def test_oracle_passes_at_a_quarter_of_the_bar(c):
    got, ns = rc.group_run(c, _oracle(c))
    rc.group_check(c, got, ns, stats=STATS["rows"], **ORACLE)


@pytest.mark.parametrize("orig,target,res_type", rc.RANGE_GROUPS)
def test_oracle_passes_on_the_decoded_recordings(orig, target, res_type):
    for dt in rc.RANGE_DTYPES:
        raw, x = rc.range_raw(orig, target, res_type, dt)
        assert x.dtype == F32 and (dt == "f32" or np.array_equal(x * 32768, np.round(x * 32768)))
        ts = np.arange(240, rc.n_computed(len(x), orig, target))
        rc.check_at("%d_%d_%s" % (orig, target, dt), rc.apply_bank_at(x, ts, orig, target, res_type, F32), x, ts,
                    orig, target, res_type, stats=STATS["ranges"], **ORACLE)


def test_oracle_passes_on_the_long_row():
    """The three tiles behind t M = 2^31, from a slice of the row (noise of the shape the GPU test fills)."""
    o, t, f = rc.LONG["orig"], rc.LONG["target"], rc.LONG["res_type"]
    first, count = rc.long_window()
    assert rc.LONG["t_first"] * 147 > 2 ** 31 and first + count <= rc.LONG["n_in"]
    assert rc.ref_index([rc.LONG["t_first"]], o, t)[1][0] == 80               # a from-below output
    x = rc.signal("long", "unit", count)
    ts = rc.LONG["t_first"] + np.arange(rc.LONG["tiles"] * rc.TILE)
    got = rc.apply_bank_at(x, ts, o, t, f, F32, first=first, n_in=rc.LONG["n_in"])
    rc.check_at("long", got, x, ts, o, t, f, first=first, n_in=rc.LONG["n_in"], stats=STATS["long"], **ORACLE)
    hits, plain = rc.r0_outputs(o, t, int(ts[-1]) + 1, int(ts[0]))
    assert len(hits) >= 8 and int(hits[0]) == rc.LONG["t_first"]
    mut = rc.resample_compute(x.astype(F64), hits, o, t, f, F64, "never_below", first, rc.LONG["n_in"])
    ref = rc.resample_at(x, hits, o, t, f, first, rc.LONG["n_in"])
    assert np.abs(mut - ref).max() > 1e-4


@pytest.mark.parametrize("c", rc.GROUPS, ids=lambda c: c["name"])
def test_fp32_restatement_without_a_mutation_passes(c):
    """The fp32 form the mutants are made from is itself inside the bars: a mutant fails for its mutation alone."""
    o, t, f = c["orig"], c["target"], c["res_type"]
    got, ns = rc.group_run(c, lambda row, ts: rc.resample_compute(row, ts, o, t, f, F32))
    rc.group_check(c, got, ns)


@pytest.mark.parametrize("mut", rc.MUTANTS["resample"])
def test_mutant_fails(mut):
    caught = []
    for c in rc.GROUPS:
        o, t, f = c["orig"], c["target"], c["res_type"]
        got, ns = rc.group_run(c, lambda row, ts: rc.resample_compute(row, ts, o, t, f, F32, mut))
        for rn, _, _ in rc.group_rows(c["name"]):
            try:
                rc.group_check(c, got, ns, rows=(rn,))
            except AssertionError:
                caught.append("%s/%s" % (c["name"], rn))
    print("%s: caught by %d rows: %s" % (mut, len(caught), ", ".join(caught[:8])))
    assert caught, (mut, "no committed case separates this mutant")
    if mut in ("never_below", "below_keeps_row0"):                # only where the branch changes the filter, or the index
        down = [n for n in caught if n.split("/")[0] in {g["name"] for g in rc.GROUPS if g["target"] < g["orig"]}]
        assert any(n.endswith("/unit") for n in down) and any(n.endswith("/quiet") for n in down), (mut, caught)
        for g in rc.GROUPS:                                       # every downsampling group that reaches from below sees it
            if g["target"] < g["orig"] and (g["orig"], g["target"]) in rc.HIT_PAIRS:
                assert g["name"] + "/hits_loud" in caught, (mut, "not caught by", g["name"] + "/hits_loud")


@pytest.mark.parametrize("c", [g for g in rc.GROUPS if (g["orig"], g["target"]) in rc.HIT_PAIRS], ids=lambda c: c["name"])
def test_premises_of_reaching_from_below(c):
    hits, plain, size, worst = rc.premises(c)
    print("%s: %d hits (first %s), %d plain r = 0; never_below off by >= %.3g element bars, at most %.3g"
          % (c["name"], len(hits), hits[:4].tolist(), len(plain), size, worst))
    if c["target"] > c["orig"]:
        assert worst < 1e-11                                     # upsampling: the same filter, nothing can see the branch
    else:
        assert worst > 1e-4
    if c["n_in"] > 7058 and (c["orig"], c["target"]) == (44100, 24000):
        assert 3840 in hits.tolist() and 3840 % rc.TILE == 0


def test_first_hits_are_where_the_kernel_tests_put_them():
    assert rc.r0_outputs(44100, 24000, 800)[0].tolist() == [240, 400, 480, 720]
    assert rc.r0_outputs(22050, 12000, 800)[0].tolist() == [240, 400, 480, 720]
    assert rc.r0_outputs(44100, 12000, 250)[0].tolist() == [120, 200, 240]
    for o, t in [p for p in rc.PAIRS if p not in rc.HIT_PAIRS]:
        assert not len(rc.r0_outputs(o, t, rc.n_computed(rc.N_IN, o, t))[0]), (o, t)


@pytest.mark.parametrize("c", rc.GROUPS[::3], ids=lambda c: c["name"])
def test_resample_at_is_resample(c):
    o, t, f = c["orig"], c["target"], c["res_type"]
    x, valid = rc.group_inputs(c["name"])
    for b, e in enumerate(rc.group_expected(c["name"])):
        if not e["n_comp"]:
            continue
        row = x[b, :int(valid[b])]
        ts = np.unique(np.concatenate([np.arange(min(40, e["n_comp"])), np.arange(max(0, e["n_comp"] - 40), e["n_comp"]),
                                       rc.r0_outputs(o, t, e["n_comp"])[0]])).astype(np.int64)
        got = rc.resample_at(row, ts, o, t, f)
        assert np.abs(got - e["ref"][ts]).max() <= 64 * 2.0 ** -53 * max(float(e["A"].max()), 1e-300), c["name"]
        if b == 0:                                               # a slice of the row gives the same bits as the row
            lo = int(ts[60] / (float(t) / o)) - 600
            if lo > 0:
                mid = ts[(ts / (float(t) / o) > lo + 500) & (ts / (float(t) / o) < lo + 700)]
                a = rc.resample_at(row[lo:lo + 1200], mid, o, t, f, first=lo, n_in=len(row))
                assert np.array_equal(a, rc.resample_at(row, mid, o, t, f))


def test_impulse_expectation_is_the_bank_applied():
    for o, t, f in rc.IMPULSE_GROUPS:
        bank, left = rc.host_bank(o, t, f)
        for p in rc.impulse_positions(o, t):
            x = np.zeros(rc.N_IN, F32)
            x[p] = 1.0
            want = rc.impulse_expected(p, rc.N_IN, o, t, f)
            got = RR.apply_bank(x, bank, o, t, left).astype(F32)
            assert np.array_equal(got.view(np.int32), want.view(np.int32)), (o, t, f, p)
            assert np.abs(want - RR.resample(x.astype(F64), o, t, f)).max() < 1e-7
            assert np.count_nonzero(want) >= (8 if p in (0, rc.N_IN - 1) else 30)
        hits = rc.r0_outputs(o, t, rc.n_computed(rc.N_IN, o, t))[0]
        if len(hits):                                            # the first impulse is seen by a from-below output
            p, L, M = rc.impulse_positions(o, t)[0], *rc.geom(o, t)[:2]
            assert p * L % M == 0 and p * L // M in hits.tolist()


def test_cases_cover_the_shapes():
    for c in rc.GROUPS:
        if c["kinds"] is not None:
            continue
        bank, left = rc.host_bank(c["orig"], c["target"], c["res_type"])
        valid = [v for _, _, v in rc.group_rows(c["name"])]
        assert {0, 1, left, left + 1, bank.shape[1], c["n_in"]} <= set(valid)
        assert rc.n_computed(c["n_in"], c["orig"], c["target"]) > 2 * rc.TILE + 1
        if (c["orig"], c["target"]) in rc.HIT_PAIRS:
            t, nt = rc.last_hit(c)
            assert nt + 1 in valid and any(rc.n_computed(v, c["orig"], c["target"]) == t + 1 for v in valid)
    for o, t, f in rc.RANGE_GROUPS:
        rows = rc.range_rows(o, t, f)
        assert {r[0] for r in rows} == set(rc.RANGE_DTYPES) and {r[1] for r in rows} == {240, 241}
        assert {r[3] for r in rows} == {True, False}
