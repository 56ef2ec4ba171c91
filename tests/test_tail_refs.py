"""The bars of tail_cases.py, tested on the CPU: both fp32 oracles (the reference's formula, and the same written in
turns as the hardware-transcendental path writes it) pass every (case, variant) at a quarter of the element tolerance
and margin 1, TOL is 4 x their worst ratio, every mutant of MUTANTS fails at least one committed run, and the
restatement equals ref_infer.waveform_tail.  A mutant that no run separates means a case is missing."""
import pytest
import torch

import tail_cases as tc
from oracle import ref_infer as R

F32, F64 = tc.F32, tc.F64
STATS = tc.Stats()
RUNS = tc.runs()
OUTS = ("spec", "phase", "omb", "o")


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    print("\nfp32 oracles, worst err / (u A) per output (TOL = 4 x, rounded up to one digit):")
    for k, v in sorted(STATS.items()):
        print("  %-12s %.3g   TOL %g" % (k, v["err_over_uA"], v["TOL"]))
        assert 4 * v["err_over_uA"] <= v["TOL"], (k, v)
        assert v["TOL"] <= 4 * v["err_over_uA"] * 2.0, (k, v, "TOL is more than 4 x the worst ratio rounded up to one digit")


def _got(c, out):
    inp, ref, A, orcs = tc.tail_shared(c)
    return {k: out[k] for k in OUTS if k in A}


@pytest.mark.parametrize("style", ["plain", "turns"])
@pytest.mark.parametrize("c", RUNS, ids=lambda c: c["name"])
def test_oracle_passes_at_a_quarter_of_the_bar(c, style):
    orcs = tc.tail_shared(c)[3]
    tc.tail_check(c, _got(c, orcs[style]), styles=("plain", "turns"), tol_scale=0.25, margin=1.0, stats=STATS)


@pytest.mark.parametrize("mut", tc.MUTANTS)
def test_mutant_fails(mut):
    caught = []
    for c in RUNS:
        inp = tc.tail_shared(c)[0]
        try:
            tc.tail_check(c, _got(c, tc.tail_compute(c, inp, F32, mut)), styles=("plain", "turns"))
        except AssertionError:
            caught.append(c["name"])
            if len(caught) == 3:                 # (enough to name; every further run costs a reference)
                break
    print("%s: first caught by %s" % (mut, ", ".join(caught)))
    assert caught, (mut, "no committed run separates this mutant")


def test_restatement_is_the_oracle():
    """tail_compute in fp32 (plain variant) is ref_infer.waveform_tail: spec and phase bit for bit, the waveform to a
    few ulp (the oracle adds frames in place, the restatement strided); fixed and trainable bank, single band."""
    class Mb:
        subbands, gen_istft_n_fft, gen_istft_hop_size = 4, 16, 4

    class Sb:
        subbands, gen_istft_n_fft, gen_istft_hop_size = 1, 16, 4
    for base in tc.TAIL_CASES:
        for bank in (("fixed", "trainable") if base["kind"] == "mb" else (None,)):
            c = tc.with_variant(base, "plain", bank, "ms" if bank == "trainable" else "mb" if bank else None)
            inp, ref, A, orcs = tc.tail_shared(c)
            sd = {}
            if bank == "trainable":
                h = inp["filt"]
                sd = {"dec.multistream_conv_post.weight_v": h[None], "dec.multistream_conv_post.weight_g": h.norm().reshape(1, 1, 1)}
            o, omb, spec, phase = R.waveform_tail(R.Weights(sd), Mb if base["kind"] == "mb" else Sb, inp["x"])
            mine = orcs["plain"]
            assert torch.equal(spec.reshape(mine["spec"].shape), mine["spec"]) and torch.equal(phase.reshape(mine["phase"].shape), mine["phase"])
            scale = float(o.abs().max())
            assert float((o.reshape(mine["o"].shape) - mine["o"]).abs().max()) <= 1e-5 * scale, c["name"]
            if omb is not None:
                assert float((omb - mine["omb"]).abs().max()) <= 1e-5 * float(omb.abs().max()), c["name"]


def test_packed_transform_is_the_matrix_form():
    """The kernel's packed 16-point inverse transform (irfft16_hann) and its reciprocal envelope, restated operation for
    operation (style `packed`): in float64 the reference itself, in fp32 inside a quarter of the bars like the other
    oracles -- the packed form needs no bars of its own."""
    for c in RUNS:
        if c["variant"] != "polar":
            continue
        inp, ref, A, orcs = tc.tail_shared(c)
        p64 = tc.tail_compute(c, inp, F64, style="packed")
        assert float((p64["o"] - ref["o"]).abs().max()) <= 1e-12 * max(1.0, float(ref["o"].abs().max())), c["name"]
        tc.tail_check(c, _got(c, tc.tail_compute(c, inp, F32, style="packed")), styles=("plain", "turns"), tol_scale=0.25)


def test_cases_cover_the_shapes():
    mb = [c for c in tc.TAIL_CASES if c["kind"] == "mb"]
    sb = [c for c in tc.TAIL_CASES if c["kind"] == "sb"]
    assert {1, 7, 8, 15, 16} == {c["n"] for c in mb} and {1, 3, 251, 252, 253, 505} == {c["n"] for c in sb}
    assert all(c["B"] == 3 for c in tc.TAIL_CASES)
    assert {0.7, 2.0} == {c["std"] for c in mb} == {c["std"] for c in sb}
    for c in tc.TAIL_CASES:
        x = tc.tail_inputs(c)["x"].view(3, c["K"], 18, c["F"])
        assert float(x[:, :, :9].min()) == -100.0 and float(x[:, :, 9:].max()) == 1500.0
        assert abs(float(x[:, :, 14].abs().max()) - 64.0) < 1e-3
