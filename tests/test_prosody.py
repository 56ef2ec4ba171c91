"""Per-token prosody without a GPU: the host checks of `Request` / `infer`, `frames_of_ms`, the float64 restatement's
own properties (prosody_ref.py), the tie budget of the op's cases, and the oracle with a tensor `length_scale` pinned
to vectors from the real reference (tests/golden/make_prosody_golden.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

import prosody_ref as P
from helpers import load_fixture, config_for, rms
from mb_istft_vits_amd import _capi, models, synth
from oracle import ref_infer as R

GOLDEN = {"prosody_mini_b2": "ljs_mini_mb_istft_vits", "prosody_uudb_b2": "uudb_ms_istft_vits_ms"}


# ------------------------------------------------------------------------------------------------ host checks
def test_frames_of_ms_rounds_half_up_in_integers():
    f = models.frames_of_ms
    assert f(0, 22050, 256) == 0
    assert f(300, 22050, 256) == 26                      # 25.84 frames
    assert f(1000, 16000, 256) == 63                     # 62.5: the half goes up
    assert f(8, 16000, 256) == 1                         # 0.5
    assert f(7, 16000, 256) == 0                         # 0.4375
    assert f(10 ** 9, 48000, 1) == 48 * 10 ** 9          # no float anywhere
    for bad in ((-1, 22050, 256), (10, 0, 256), (10, 22050, 0)):
        with pytest.raises(ValueError):
            f(*bad)
    for bad in ((1.5, 22050, 256), (True, 22050, 256), (10, 22050.0, 256)):
        with pytest.raises(TypeError):
            f(*bad)


def test_request_takes_the_three_controls():
    x = list(range(1, 8))
    r = models.Request(x, length_scale=torch.full((7,), 1.5), extra_frames=torch.arange(7), fit_frames=40)
    assert r.length_scale == 1.0 and r.scale.dtype == torch.float32 and tuple(r.scale.shape) == (7,)
    assert r.extra.dtype == torch.int32 and r.extra.tolist() == list(range(7))
    assert r.fit == (40, 0.5, 2.0)
    r = models.Request(x, length_scale=torch.ones(1, 1, 7, dtype=torch.float64), fit_frames=3, fit_bounds=(0.8, 0.8))
    assert r.scale.dtype == torch.float32 and r.fit == (3, float(np.float32(0.8)), float(np.float32(0.8)))
    r = models.Request(x, length_scale=1.25, extra_frames=torch.zeros(7, dtype=torch.int64))
    assert r.length_scale == 1.25 and r.scale is None and r.extra.dtype == torch.int32 and r.fit is None
    r = models.Request(x)                                 # nothing new: nothing set
    assert r.scale is None and r.extra is None and r.fit is None and r.length_scale == 1.0
    # an int64 extra outside int32 keeps its sign and its being out of range
    r = models.Request(x, extra_frames=torch.tensor([0, -(1 << 40), 1 << 40, 5, 0, 0, 0]))
    assert r.extra.tolist() == [0, -1, 1 << 20, 5, 0, 0, 0]


@pytest.mark.parametrize("kw, exc", [
    (dict(length_scale=torch.ones(6)), ValueError),                       # shape
    (dict(length_scale=torch.ones(2, 7)), ValueError),
    (dict(length_scale=torch.ones(7, dtype=torch.int64)), TypeError),     # dtype
    (dict(extra_frames=torch.ones(7)), TypeError),
    (dict(extra_frames=torch.ones(7, dtype=torch.bool)), TypeError),
    (dict(extra_frames=[1] * 7), ValueError),
    (dict(extra_frames=torch.ones(8, dtype=torch.int32)), ValueError),
    (dict(fit_frames=0), ValueError),
    (dict(fit_frames=-3), ValueError),
    (dict(fit_frames=2.5), TypeError),
    (dict(fit_frames=True), TypeError),
    (dict(fit_frames=[10, 10]), ValueError),                              # one utterance: one value
    (dict(fit_frames=10, fit_bounds=(0.0, 2.0)), ValueError),
    (dict(fit_frames=10, fit_bounds=(2.0, 1.0)), ValueError),
    (dict(fit_frames=10, fit_bounds=(1.0, float("inf"))), ValueError),
    (dict(fit_frames=10, fit_bounds=(float("nan"), 1.0)), ValueError),
    (dict(fit_frames=10, fit_bounds=1.0), ValueError),
    # none of the three goes with given durations
    (dict(durations=torch.ones(7, dtype=torch.int32), length_scale=torch.ones(7)), ValueError),
    (dict(durations=torch.ones(7, dtype=torch.int32), extra_frames=torch.ones(7, dtype=torch.int32)), ValueError),
    (dict(durations=torch.ones(7, dtype=torch.int32), fit_frames=10), ValueError),
])
def test_request_refuses(kw, exc):
    with pytest.raises(exc):
        models.Request(list(range(1, 8)), **kw)


def test_batched_entries_check_shapes_and_exclusions():
    chk = lambda **k: models._prosody_args("infer", k.pop("length_scale", 1), k.pop("extra_frames", None),
                                           k.pop("fit_frames", None), k.pop("fit_bounds", models.FIT_BOUNDS),
                                           k.pop("durations", None), 2, 5)
    scalar, scale, extra, fit = chk(length_scale=torch.ones(2, 1, 5), extra_frames=torch.ones(2, 5, dtype=torch.int64),
                                    fit_frames=[30, 40])
    assert scalar == 1.0 and tuple(scale.shape) == (2, 5) and tuple(extra.shape) == (2, 5) and extra.dtype == torch.int32
    assert fit == [(30, 0.5, 2.0), (40, 0.5, 2.0)]
    assert chk(length_scale=1.3) == (1.3, None, None, None)
    assert chk(length_scale=torch.tensor(1.5)) == (1.5, None, None, None)         # a 0-dim tensor stays the scalar
    assert chk(length_scale=2, fit_frames=torch.tensor([7, 9]))[3] == [(7, 0.5, 2.0), (9, 0.5, 2.0)]
    assert chk(fit_frames=np.int64(12))[3] == [(12, 0.5, 2.0)] * 2
    for kw, exc in [(dict(length_scale=torch.ones(2, 4)), ValueError), (dict(length_scale=torch.ones(2, 2, 5)), ValueError),
                    (dict(length_scale=torch.ones(2, 5, dtype=torch.int32)), TypeError),
                    (dict(extra_frames=torch.ones(5, dtype=torch.int32)), ValueError),
                    (dict(fit_frames=[1, 2, 3]), ValueError), (dict(fit_frames=[1, 0]), ValueError),
                    (dict(durations=torch.ones(2, 5), fit_frames=9), ValueError),
                    (dict(durations=torch.ones(2, 5), length_scale=torch.ones(2, 5)), ValueError)]:
        with pytest.raises(exc):
            chk(**kw)


def test_binding_declares_the_new_entries_and_structs():
    for sym in ("mbv_shape_durations", "mbv_shape_durations_rows", "mbv_op_shape_durations", "mbv_shape_runs"):
        assert sym in _capi.SYMBOLS
    assert _capi.ABI_VERSION == 3
    assert C.sizeof(_capi.MbvFit) == 16 and C.sizeof(_capi.MbvShapeRow) == 40
    word = int(np.asarray([(1.25, 1)], dtype=[("scale", "<f4"), ("status", "<i4")]).view(np.int64)[0])
    assert _capi.fit_result(word) == (1.25, 1)


# ------------------------------------------------------------------------------------------------ the restatement
def _row(seed, T=40):
    rs = np.random.RandomState(seed)
    logw = (1.2 * rs.standard_normal(T)).astype(np.float32)
    scale = P.SCALE_SET[rs.randint(0, len(P.SCALE_SET), size=T)]
    extra = (rs.randint(0, 9, size=T) * (rs.uniform(size=T) < 0.3)).astype(np.int32)
    return logw, scale, extra


@pytest.mark.parametrize("seed", range(6))
def test_total_is_monotone_in_the_factor(seed):
    logw, scale, extra = _row(seed)
    grid = np.sort(np.concatenate([np.geomspace(1e-3, 1e3, 4000), [0.5, 1.0, 2.0]]).astype(np.float32))
    # and a run of neighbouring floats: the step the bisection ends on
    grid = np.concatenate([grid, P.from_bits(np.arange(P.bits(1.0) - 300, P.bits(1.0) + 300, dtype=np.uint32))])
    grid = np.unique(grid)
    D = [P.total(logw, scale, extra, f) for f in grid]
    assert all(a <= b for a, b in zip(D, D[1:]))
    assert D[0] >= int(extra.sum()) and D[-1] > D[0]


@pytest.mark.parametrize("seed", range(6))
def test_fit_is_the_largest_factor_that_fits(seed):
    logw, scale, extra = _row(seed)
    lo, hi = np.float32(0.5), np.float32(2.0)
    d_lo, d_hi = P.total(logw, scale, extra, lo), P.total(logw, scale, extra, hi)
    assert d_lo < d_hi
    for frames in (d_lo - 1, d_lo, d_lo + 1, (d_lo + d_hi) // 2, d_hi - 1, d_hi, d_hi + 50):
        f, status, n = P.fit(logw, scale, extra, frames, lo, hi)
        assert n <= 32
        assert lo <= f <= hi and f.dtype == np.float32
        assert status == (1 if d_lo > frames else 0)
        if status:
            assert f == lo
            continue
        assert P.total(logw, scale, extra, f) <= frames
        assert f == hi or P.total(logw, scale, extra, np.nextafter(f, np.float32(np.inf))) > frames
        grid = np.geomspace(float(lo), float(hi), 3000).astype(np.float32)            # maximal on a dense grid
        fits = [g for g in grid if P.total(logw, scale, extra, g) <= frames]
        assert all(g <= f for g in fits)
        assert not fits or max(fits) <= f
    # the search space is the whole positive range: 32 evaluations still do
    f, status, n = P.fit(logw, scale, extra, (d_lo + d_hi) // 2, np.float32(1e-45), np.float32(3e38))
    assert n <= 32 and status == 0 and P.total(logw, scale, extra, f) <= (d_lo + d_hi) // 2


def test_the_final_pass_applies_the_range_rules():
    logw = np.zeros((4, 3), np.float32)
    scale = np.ones((4, 3), np.float32)
    extra = np.zeros((4, 3), np.int32)
    scale[0, 1] = -1.0
    scale[1, 2] = np.nan                     # behind the row's length: not looked at
    extra[2, 0] = -1
    scale[3, 0], extra[3, 1] = 0.0, 7
    r = P.shape(logw, [3, 2, 3, 3], scale, extra, bad=[0, 0, 0, 0])
    assert r["ylen64"].tolist() == [-1, 2, -1, 9] and r["ylen32"].tolist() == [1, 2, 1, 9]
    assert r["w_ceil"][3].tolist() == [0.0, 8.0, 1.0] and r["cum"][3].tolist() == [0, 8, 9]


@pytest.mark.parametrize("name", list(P.OP_BY_NAME))
def test_op_cases_stay_inside_the_tie_budget(name):
    c = P.OP_BY_NAME[name]
    inp = P.op_inputs(c)
    ref = P.shape(inp["logw"], inp["lens"], inp["scale"], inp["extra"], bad=inp["bad"])
    near = P.near_ties(inp["logw"], inp["lens"], inp["scale"])
    assert int(near.sum()) <= P.MAX_LEFT_OUT * int(ref["mask"].sum())
    # the reference run through its own check (the float64 result is an admissible kernel output)
    got = dict(w_ceil=ref["w_ceil"].astype(np.float32), cum=ref["cum"], ylen32=ref["ylen32"], ylen64=ref["ylen64"])
    assert P.op_check(c, inp, got) == int(near.sum())
    if "edge" in c["plant"]:
        assert ref["over"].tolist() == [False, True, False]
    if "edge_extra" in c["plant"]:
        assert ref["over"].tolist() == [False, True, False]


# ------------------------------------------------------------------------------------------------ the reference's golden
@pytest.mark.parametrize("fixture", list(GOLDEN))
def test_oracle_with_a_tensor_length_scale_matches_the_reference(fixture):
    gold = load_fixture(fixture)
    _, cfg = config_for(GOLDEN[fixture], int(gold["n_vocab"]))
    sd = synth.make_state_dict(cfg, int(gold["weight_seed"]))
    torch.set_num_threads(4)
    assert float(gold["ceil_margin"]) >= 1e-3
    out = R.infer(sd, cfg, gold["x"], gold["x_lengths"], gold.get("sid"), noise=gold["noise"],
                  noise_scale=float(gold["noise_scale"]), length_scale=torch.from_numpy(gold["scale"]))
    assert np.array_equal(out["w_ceil"].numpy(), gold["w"])                       # durations exact
    assert np.array_equal(out["y_lengths"].numpy(), gold["y_mask"].sum((1, 2)).astype(np.int64))
    for name in ("y_mask", "m_p", "logs_p", "z_p", "z", "o"):
        got, ref = out[name].numpy(), gold[name]
        assert got.shape == ref.shape, (name, got.shape, ref.shape)
        assert rms(got - ref) <= 2e-5 * max(rms(ref), 1e-3) + 1e-6, name
    assert rms(out["o"].numpy() - gold["o"]) < 1e-4
    # token t of the tensor call has the duration of token t of the scalar call at its own scale
    for s in np.unique(gold["scale"]):
        w_s = R.infer(sd, cfg, gold["x"], gold["x_lengths"], gold.get("sid"), length_scale=float(s))["w_ceil"].numpy()
        sel = (gold["scale"] == s) & (np.arange(gold["x"].shape[1])[None, None, :] < gold["x_lengths"][:, None, None])
        assert np.array_equal(w_s[sel], gold["w"][sel])
