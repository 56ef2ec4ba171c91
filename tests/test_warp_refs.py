"""The bars of warp_cases.py, tested on the CPU: the fp32 oracle passes every committed case at a quarter of the element
tolerance and margin 1, every mutated restatement of MUTANTS fails the element bar on a named committed case, the
premises about the widest tile, the far ranges and the integer U[f] hold on the reference alone, and `warp_compute` in
float64 is `warp_ref.warp`."""
import numpy as np
import pytest

import warp_cases as wc
import warp_ref

F32, F64 = wc.F32, wc.F64
STATS = {f: {k: wc.Stats() for k in wc.ENTRIES} for f in wc.FILTERS}
ORACLE = dict(tol_scale=0.25, margin=1.0)
IDS = dict(ids=lambda v: v["name"] if isinstance(v, dict) else v)


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    print("\nfp32 oracle, worst err / (u A) (TOL = 4 x, rounded up to one digit):")
    for f, per in STATS.items():
        for k, s in per.items():
            for v in s.values():
                print("  %-12s %-17s %.3g   TOL %g" % (f, k, v["err_over_uA"], v["TOL"]))
                assert 4 * v["err_over_uA"] <= v["TOL"], (f, k, v)


def _fp32(c, res_type, mut=None):
    return lambda x, ts, first, end, in_avail: wc.warp_compute(c, res_type, x, ts, first, end, F32, mut, in_avail)


@pytest.mark.parametrize("res_type", wc.FILTERS)
@pytest.mark.parametrize("c", wc.CASES, **IDS)
def test_oracle_passes_at_a_quarter_of_the_bar(c, res_type):
    """(the oracle against itself: what this measures is the oracle's worst ratio, the source of TOL)"""
    wc.run(c, res_type, _fp32(c, res_type), stats=STATS[res_type], **ORACLE)


@pytest.mark.parametrize("res_type", wc.FILTERS)
@pytest.mark.parametrize("c", wc.CASES, **IDS)
def test_fp32_restatement_without_a_mutation_passes(c, res_type):
    """The fp32 form the mutants are made from is itself inside the bars: a mutant fails for its mutation alone."""
    wc.run(c, res_type, _fp32(c, res_type))


# what only one kind of table can see: the mutant must be caught THERE, or the case no longer does its work
MUST_CATCH = {"small_window": ["octave_up/kaiser_best/noise", "near_top/kaiser_best/noise"],
              "frame_lt": ["alternating/kaiser_best/noise", "alternating/kaiser_fast/noise"],
              "tau_fp32": ["long/kaiser_best/noise", "past_2_24/kaiser_best/noise"]}


@pytest.mark.parametrize("mut", wc.MUTANTS["warp"])
def test_mutant_fails(mut):
    caught = {}
    for c in wc.CASES:
        for res_type in wc.FILTERS:
            fn = _fp32(c, res_type, mut)
            for vn, x, in_avail, _ in wc.variants(c):
                for k, (first, end) in enumerate(wc.variant_ranges(c, in_avail, res_type)):
                    s = wc.Stats()
                    got = fn(x, np.arange(first, end, dtype=np.int64), first, end, in_avail)
                    try:
                        wc.check(c, res_type, vn, k, got, stats=s)
                    except AssertionError as e:
                        if "element bar" in e.args[0]:
                            key = "%s/%s/%s" % (c["name"], res_type, vn)
                            caught[key] = max(caught.get(key, 0.0), s["warp"]["err_over_uA"] / wc.TOL["warp"])
    print("%s: caught by %d of the case rows: %s" % (mut, len(caught), ", ".join(
        "%s x%.3g" % kv for kv in sorted(caught.items(), key=lambda kv: -kv[1]))))
    assert caught, (mut, "no committed case separates this mutant")
    for key in MUST_CATCH.get(mut, ()):
        assert key in caught, (mut, "not caught by", key)
    if mut == "small_window":                                     # kaiser_fast needs 580 floats: it cannot see a cap of 600
        assert all("kaiser_best" in k for k in caught), caught
    if mut == "frame_lt":
        assert all(k.startswith("alternating/") for k in caught), caught


def test_premises():
    p = wc.premises()
    print("widest tile (taps from .. to, staged floats, tiles): octave_up %s, near_top %s; long from %d, past_2_24 from "
          "%d; alternating has t == U[f] at %s" % (p["octave_up"], p["near_top"], p["long_first"], p["past_first"],
                                                   p["alternating_on_U"]))


def test_the_six_frame_parity_tables_reach_no_wide_window():
    """Why the cases exist: the widest staged window of the tables test_gpu_warp.py runs stays below SMALL_WINDOW, so a
    kWarpWindow of 600 passes all of them."""
    for name, R in (("ones", np.ones(6)), ("up", np.full(6, 1.25)), ("down", np.full(6, 0.8)),
                    ("alternating", [0.5, 2.0] * 3), ("glided", wc.CASE_BY_NAME["glided"]["R"])):
        R = np.asarray(R, F32)
        U_, n_out = warp_ref.plan(R, 256)
        hw = warp_ref.half_width(R)
        w = max(int(warp_ref.tau(min(t0 + wc.TILE, n_out) - 1, U_, R, 256)[0]) + hw + 2
                - (int(warp_ref.tau(t0, U_, R, 256)[0]) - hw) for t0 in range(0, n_out, wc.TILE))
        print("%-12s widest staged window %d" % (name, w))
        assert w < wc.SMALL_WINDOW, (name, w)


@pytest.mark.parametrize("name,res_type", [("near_top", "kaiser_best"), ("irrational", "kaiser_fast"),
                                           ("hop1", "kaiser_best"), ("long", "kaiser_fast")])
def test_float64_warp_compute_is_warp_ref(name, res_type):
    """Bitwise: the restated geometry (tile window, counts, offsets) is the reference's, and with the half width the
    host plans the window cuts nothing."""
    c = wc.CASE_BY_NAME[name]
    for vn, xv, in_avail, _ in wc.variants(c):
        if vn.startswith("impulse"):
            continue
        for k, (first, end) in enumerate(wc.variant_ranges(c, in_avail, res_type)):
            ts = np.arange(first, end, dtype=np.int64)
            got = wc.warp_compute(c, res_type, xv, ts, first, end, F64, None, in_avail)
            ref = wc.expected(name, res_type)[vn][k]["ref"]
            assert got.dtype == F64 and np.array_equal(got, ref), (name, res_type, vn, float(np.abs(got - ref).max()))


def test_the_tile_partition_does_not_change_the_oracle():
    """A range that starts inside a tile of the whole row gives the same fp32 bits: the kernel's range independence
    restated (the window of a tile only has to hold the taps)."""
    c = wc.CASE_BY_NAME["near_top"]
    x, n_out = wc.case_x("near_top"), wc.plan("near_top")[1]
    whole = wc.warp_compute(c, "kaiser_best", x, np.arange(n_out), 0, n_out, F32)
    part = wc.warp_compute(c, "kaiser_best", x, np.arange(301, n_out - 5), 301, n_out - 5, F32)
    assert np.array_equal(whole[301:n_out - 5].view(np.int32), part.view(np.int32))


def test_cases_cover_the_shapes():
    n = {c["name"]: wc.plan(c["name"])[1] for c in wc.CASES}
    assert n["octave_up"] == 3 * wc.TILE and n["octave_down"] == 6 * wc.TILE
    assert 1.1e6 < n["long"] < 1.2e6 and 2 ** 24 + 4 * wc.TILE < n["past_2_24"] < 2.1e7
    assert len(wc.CASE_BY_NAME["hop1"]["R"]) == 700 and n["hop1"] > wc.TILE
    U_ = wc.plan("irrational")[0]
    assert all(u != int(u) for u in U_[1:-1])                     # fractional U
    for name in wc.FRONTIER_CASES:
        c = wc.CASE_BY_NAME[name]
        for f in wc.FILTERS:
            (first, ready), = wc.variant_ranges(c, wc.frontier(c), f)
            assert first == 0 and 0 < ready < n[name], (name, f, ready)
    for name in wc.IMPULSE_CASES:
        c = wc.CASE_BY_NAME[name]
        ps = wc.impulse_positions(c)
        assert 0 in ps and wc.samples(c) - 1 in ps and any((p + 1) % c["hop"] == 0 for p in ps)
    assert len(wc.ENVELOPE_GAINS) == len(wc.CASE_BY_NAME["near_top"]["R"]) + 1
