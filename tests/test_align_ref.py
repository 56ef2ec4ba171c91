"""CPU checks of the forced-alignment restatements (tests/align_ref.py) and fixtures: the fp32 search reproduces the
reference's durations, the float64 search is the true optimum, every path is a valid alignment, and the restated
neg_cent matches the reference's within the bound of an fp32 evaluation."""
import numpy as np
import pytest

import align_ref
from helpers import load_fixture

ALIGN_FIXTURES = ("align_mini_b2", "align_uudb_b2")


def neg_cent_bound(z_p, m_p, logs_p, I):
    """Per-cell bound on |fp32 evaluation - float64 value| of models.py:670-675 (first order in u = 2^-24):
      (2 I + 4) u sum|summands|: the value is a sum of 4 I terms.  However an fp32 evaluation groups them (two
        matmuls of depth I plus two column sums, or one contraction of depth 2 I plus a column constant), a
        term passes through at most 2 I + 1 additions, one rounding of its own product or operand, and at most two
        more additions that join the partial results: <= (2 I + 4) u relative to the magnitudes summed.
      eps_in = 2^-23 sum|summands with the factor e^{-2 logs_p}|: the fp32 exponential is correct to 1 ulp
        (<= 2^-23 relative; its argument -2 logs_p is exact), and that error passes linearly into terms 2-4."""
    _, mag = align_ref.neg_cent(z_p, m_p, logs_p)
    return (2 * I + 4) * 2.0 ** -24 * mag + 2.0 ** -23 * align_ref.exp_term_mag(z_p, m_p, logs_p)


@pytest.mark.parametrize("name", ALIGN_FIXTURES)
def test_fp32_search_reproduces_the_reference_durations(name):
    g = load_fixture(name)
    paths, w = align_ref.maximum_path(g["neg_cent"], g["y_lengths"], g["x_lengths"], np.float32)
    assert np.array_equal(w, g["w"])
    # rows as the issue asks: ragged, one with t_x == t_y
    assert w.sum(1).tolist() == g["y_lengths"].tolist()


def test_fixture_rows_cover_the_band_shapes():
    rows = [(int(tx), int(ty)) for n in ALIGN_FIXTURES for tx, ty in zip(load_fixture(n)["x_lengths"], load_fixture(n)["y_lengths"])]
    assert any(tx == ty for tx, ty in rows)
    assert any(ty >= 2 * tx for tx, ty in rows)
    assert len({ty for _, ty in rows}) > 2


@pytest.mark.parametrize("name", ALIGN_FIXTURES)
def test_fixture_paths_are_stable(name):
    """The acceptance condition of make_align_golden.py, re-checked: float64 path == the reference's, also under
    perturbations of 2^-16 sum|summands| per cell."""
    g = load_fixture(name)
    _, mag = align_ref.neg_cent(g["z_p"], g["m_text"], g["logs_text"])
    rs = np.random.RandomState(5)
    for b in range(g["x"].shape[0]):
        ty, tx = int(g["y_lengths"][b]), int(g["x_lengths"][b])
        v = g["neg_cent"][b].astype(np.float64)
        for k in range(21):
            d = 0 if k == 0 else rs.uniform(-1, 1, v.shape) * 2.0 ** -16 * mag[b]
            p = align_ref.maximum_path_each(v + d, ty, tx, np.float64)[0]
            assert np.array_equal(p.sum(0)[:tx], g["w"][b, :tx])


def test_float64_search_is_the_brute_force_maximum():
    rs = np.random.RandomState(0)
    for ty in range(1, 8):
        for tx in range(1, ty + 1):
            for _ in range(3):
                v = rs.standard_normal((ty + 1, tx + 2)) * 3
                path, _ = align_ref.maximum_path_each(v, ty, tx, np.float64)
                best, _ = align_ref.brute_force(v, ty, tx)
                assert abs(align_ref.path_score(v, path) - best) <= 1e-12 * max(1.0, abs(best)), (ty, tx)


def test_every_path_is_a_valid_alignment():
    rs = np.random.RandomState(1)
    for case in range(300):
        ty = int(rs.randint(1, 40))
        tx = int(rs.randint(1, ty + 1))
        v = rs.standard_normal((ty + 2, tx + 3)).astype(np.float32) * (1 + case % 5)
        if case % 7 == 0:
            v = np.round(v)                                  # exact ties: the strict `<` decides
        path, _ = align_ref.maximum_path_each(v, ty, tx, np.float32)
        assert np.array_equal(path[:ty].sum(1), np.ones(ty))            # one token per frame
        assert path[ty:].sum() == 0 and path[:, tx:].sum() == 0
        w = path.sum(0)[:tx]
        assert (w >= 1).all()                                            # at least one frame per token
        assert np.array_equal(align_ref.generate_path(w, ty), path[:ty, :tx])
        tok = path[:ty, :tx].argmax(1)
        assert tok[0] == 0 and tok[-1] == tx - 1 and set(np.diff(tok).tolist()) <= {0, 1}


def test_near_optimality_bound_holds_under_perturbation():
    """The inequality test_gpu_align asserts end to end, on the CPU: the fp32 search on a perturbed matrix is
    near-optimal under the exact one, within the perturbation along both paths plus t_y fp32 additions."""
    rs = np.random.RandomState(2)
    for case in range(300):
        ty = int(rs.randint(2, 60))
        tx = int(rs.randint(1, ty + 1))
        v = rs.standard_normal((ty, tx)) * 50 - 300
        vt = (v * (1 + 2e-5 * rs.uniform(-1, 1, v.shape))).astype(np.float32)
        P = align_ref.maximum_path_each(vt, ty, tx, np.float32)[0]
        Ps = align_ref.maximum_path_each(v, ty, tx, np.float64)[0]
        d = np.abs(vt.astype(np.float64) - v)
        rhs = (d * Ps).sum() + (d * P).sum() + 2 * ty * 2.0 ** -24 * (np.abs(v) * P).sum()
        assert align_ref.path_score(v, Ps) - align_ref.path_score(v, P) <= rhs


@pytest.mark.parametrize("name", ALIGN_FIXTURES)
def test_restated_neg_cent_matches_the_reference(name):
    g = load_fixture(name)
    I = g["z_p"].shape[1]
    v, _ = align_ref.neg_cent(g["z_p"], g["m_text"], g["logs_text"])
    bound = neg_cent_bound(g["z_p"], g["m_text"], g["logs_text"], I)
    worst = 0.0
    for b in range(v.shape[0]):
        ty, tx = int(g["y_lengths"][b]), int(g["x_lengths"][b])
        r = np.abs(v[b, :ty, :tx] - g["neg_cent"][b, :ty, :tx]) / bound[b, :ty, :tx]
        worst = max(worst, float(r.max()))
    print("%s: worst |restated - reference| / bound = %.3f" % (name, worst))
    assert worst <= 1.0


def test_chain_reproduces_the_reference_z_p_and_durations():
    """oracle.ref_infer's stages (float64) against the reference's forward: z_p within fp32 noise, and the float64
    search on the chain's own neg_cent gives the stored durations (the fixtures are stable)."""
    from helpers import config_for
    from mb_istft_vits_amd import synth
    from helpers import rms
    for name, cfg_name in (("align_mini_b2", "ljs_mini_mb_istft_vits"), ("align_uudb_b2", "uudb_ms_istft_vits_ms")):
        g = load_fixture(name)
        _, cfg = config_for(cfg_name, int(g["n_vocab"]))
        sd = synth.make_state_dict(cfg, int(g["weight_seed"]))
        c = align_ref.chain(sd, cfg, g["x"], g["x_lengths"], g["y"], g["y_lengths"], g.get("sid"), g["noise"], 1.0)
        assert rms(c["z_p"] - g["z_p"]) / rms(g["z_p"]) < 5e-5
        _, w = align_ref.maximum_path(c["neg_cent"], g["y_lengths"], g["x_lengths"], np.float64)
        assert np.array_equal(w, g["w"])
