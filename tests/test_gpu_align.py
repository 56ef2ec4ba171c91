"""Forced alignment on the GPU: the two kernels of csrc/align.hip against the restatements of tests/align_ref.py, and
`net.align` / `infer(durations=)` end to end.

Measured on an MI355X (scripts/align_timing.py and this file's printed figures are in DESIGN 7.6)."""
import warnings

import numpy as np
import pytest
import torch

import align_ref
from helpers import load_fixture
from test_align_ref import neg_cent_bound

pytestmark = pytest.mark.gpu

CONFIGS = ("ljs_mini_mb_istft_vits", "ljs_mb_istft_vits", "ljs_ms_istft_vits", "uudb_ms_istft_vits_ms")
GOLD = (("align_mini_b2", "ljs_mini_mb_istft_vits"), ("align_uudb_b2", "uudb_ms_istft_vits_ms"))
_nets = {}


def _net(cfg_name, n_vocab=59, seed=1234):
    from gpu_util import make_net
    key = (cfg_name, n_vocab, seed)
    if key not in _nets:
        _nets[key] = make_net(cfg_name, n_vocab, seed)
    return _nets[key]


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda() if a is not None else None


def op_max_path(net, value, t_y, t_x, want_path=True):
    from mb_istft_vits_amd import _capi
    from gpu_util import ptr
    h = net._ensure_handle()
    v = _cuda(np.asarray(value, np.float32))
    keep = v.clone()
    B, Tt, Ts = v.shape
    ty, tx = _cuda(np.asarray(t_y, np.int32)), _cuda(np.asarray(t_x, np.int32))
    w = torch.full((B, Ts), -7, dtype=torch.int32, device="cuda")
    path = torch.full((B, Tt, Ts), -7, dtype=torch.int32, device="cuda") if want_path else None
    status = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    _capi.check(h, _capi.lib().mbv_op_max_path(h, ptr(v), ptr(ty), ptr(tx), ptr(w), ptr(path), ptr(status), B, Tt, Ts,
                                               net._stream()), "mbv_op_max_path")
    assert torch.equal(v.view(torch.int32), keep.view(torch.int32))          # value is left untouched (bitwise: NaNs too)
    return w.cpu().numpy(), path.cpu().numpy() if want_path else None, status.cpu().numpy()


def op_neg_cent(net, z_p, m_p, logs_p, t_y, t_x, fill=np.nan):
    from mb_istft_vits_amd import _capi
    from gpu_util import ptr
    h = net._ensure_handle()
    z, m, lg = (_cuda(np.asarray(a, np.float32)) for a in (z_p, m_p, logs_p))
    B, I, Tt = z.shape
    Ts = m.shape[2]
    ty, tx = _cuda(np.asarray(t_y, np.int32)), _cuda(np.asarray(t_x, np.int32))
    value = torch.full((B, Tt, Ts), fill, dtype=torch.float32, device="cuda")
    _capi.check(h, _capi.lib().mbv_op_neg_cent(h, ptr(z), ptr(m), ptr(lg), ptr(ty), ptr(tx), ptr(value), B, I, Tt, Ts,
                                               net._stream()), "mbv_op_neg_cent")
    return value.cpu().numpy()


def _check_search(net, value, t_y, t_x, label):
    value = np.asarray(value, np.float32)
    w, path, status = op_max_path(net, value, t_y, t_x)
    assert (status == 0).all(), (label, status)
    clean = np.where(np.isfinite(value) & (np.abs(value) < 1e29), value, 0).astype(np.float32)
    for b in range(value.shape[0]):
        ty, tx = int(t_y[b]), int(t_x[b])
        want = align_ref.maximum_path_each(clean[b], ty, tx, np.float32)[0]
        assert np.array_equal(path[b], want), (label, b, ty, tx)
        assert np.array_equal(w[b], want.sum(0)), (label, b, ty, tx)


def _poison_outside(v, t_y, t_x, what):
    v = v.copy()
    for b in range(v.shape[0]):
        v[b, int(t_y[b]):, :] = what
        v[b, :, int(t_x[b]):] = what
    return v


# --------------------------------------------------------------------------- 1. the search, bitwise
def test_search_is_bitwise_the_fp32_restatement_on_the_goldens():
    net, _ = _net("ljs_mini_mb_istft_vits")
    for name, _cfg in GOLD:
        g = load_fixture(name)
        w, path, status = op_max_path(net, g["neg_cent"], g["y_lengths"], g["x_lengths"])
        want, ww = align_ref.maximum_path(g["neg_cent"], g["y_lengths"], g["x_lengths"], np.float32)
        assert (status == 0).all()
        assert np.array_equal(path, want) and np.array_equal(w, ww) and np.array_equal(w, g["w"])


SHAPES = [(1, 1), (1, 7), (2, 2), (2, 300), (63, 63), (63, 200), (64, 64), (64, 1500), (65, 66), (65, 700), (200, 200),
          (200, 566), (513, 513), (513, 1500)]


@pytest.mark.parametrize("tx,ty", SHAPES)
def test_search_random_matrix(tx, ty):
    """One utterance per shape; NaN in every cell outside [t_y, t_x).  (513, 1500): the decision bits (1500 rows x
    16 words x 8 bytes) leave LDS."""
    net, _ = _net("ljs_mini_mb_istft_vits")
    rs = np.random.RandomState(1000 * tx + ty)
    Tt, Ts = ty + int(rs.randint(0, 4)), tx + int(rs.randint(0, 4))
    v = (rs.standard_normal((1, Tt, Ts)) * 40 - 250).astype(np.float32)
    v = _poison_outside(v, [ty], [tx], np.nan)
    _check_search(net, v, [ty], [tx], "random")


def test_search_ragged_batches_ties_and_poisoned_padding():
    net, _ = _net("ljs_mini_mb_istft_vits")
    rs = np.random.RandomState(3)
    # a ragged batch
    t_x = np.asarray([1, 40, 64, 65, 129, 150, 17])
    t_y = np.asarray([9, 40, 100, 260, 129, 260, 31])
    v = (rs.standard_normal((7, 260, 150)) * 30 - 200).astype(np.float32)
    _check_search(net, _poison_outside(v, t_y, t_x, 1e30), t_y, t_x, "ragged 1e30")
    _check_search(net, _poison_outside(v, t_y, t_x, np.nan), t_y, t_x, "ragged nan")
    # a batch of 64
    t_x = rs.randint(1, 81, size=64)
    t_y = np.asarray([int(rs.randint(a, 201)) for a in t_x])
    t_x[5], t_y[5] = 80, 200
    v = (rs.standard_normal((64, 200, 80)) * 30 - 200).astype(np.float32)
    _check_search(net, _poison_outside(v, t_y, t_x, np.nan), t_y, t_x, "batch of 64")
    # exact ties: the strict `<` of the backtrack decides
    t_x, t_y = np.asarray([70, 5, 33]), np.asarray([150, 5, 90])
    _check_search(net, np.zeros((3, 150, 70), np.float32), t_y, t_x, "zeros")
    _check_search(net, rs.randint(-3, 4, size=(3, 150, 70)).astype(np.float32), t_y, t_x, "small integers")


def test_search_refuses_rows_through_the_status_word():
    net, _ = _net("ljs_mini_mb_istft_vits")
    rs = np.random.RandomState(4)
    v = rs.standard_normal((6, 20, 12)).astype(np.float32)
    t_x = np.asarray([5, 12, 0, 4, 13, 3])
    t_y = np.asarray([9, 11, 6, 0, 20, 21])
    w, path, status = op_max_path(net, v, t_y, t_x)
    assert status.tolist() == [0, 1, 2, 2, 3, 3]
    assert (w[1:] == 0).all() and (path[1:] == 0).all()
    assert np.array_equal(path[0], align_ref.maximum_path_each(v[0], 9, 5, np.float32)[0])


# --------------------------------------------------------------------------- 2. neg_cent, derived bound
def _neg_cent_case(net, z_p, m_p, logs_p, t_y, t_x, label):
    """|GPU - float64| <= (2 I + 4) 2^-24 sum|summands| + eps_in per cell (test_align_ref.neg_cent_bound states the
    derivation: the kernel's grouping is one contraction of depth 2 I + a column constant of four partial sums)."""
    I = np.asarray(z_p).shape[1]
    got = op_neg_cent(net, z_p, m_p, logs_p, t_y, t_x)
    ref, _ = align_ref.neg_cent(z_p, m_p, logs_p)
    bound = neg_cent_bound(z_p, m_p, logs_p, I)
    z, m, lg = (torch.from_numpy(np.asarray(a, np.float32)) for a in (z_p, m_p, logs_p))
    s = torch.exp(-2 * lg)
    zt = z.transpose(1, 2)
    cpu32 = (torch.sum(-0.5 * np.log(2 * np.pi) - lg, [1], keepdim=True) + torch.matmul(-0.5 * zt ** 2, s) +
             torch.matmul(zt, m * s) + torch.sum(-0.5 * m ** 2 * s, [1], keepdim=True)).numpy()
    worst, e_gpu, e_cpu, n = 0.0, 0.0, 0.0, 0
    for b in range(got.shape[0]):
        ty, tx = int(t_y[b]), int(t_x[b])
        assert np.isnan(got[b, ty:, :]).all() and np.isnan(got[b, :, tx:]).all(), label      # nothing written outside
        d = np.abs(got[b, :ty, :tx].astype(np.float64) - ref[b, :ty, :tx])
        worst = max(worst, float((d / bound[b, :ty, :tx]).max()))
        e_gpu += float((d ** 2).sum())
        e_cpu += float(((cpu32[b, :ty, :tx] - ref[b, :ty, :tx]) ** 2).sum())
        n += ty * tx
    print("neg_cent %-22s worst |err| / bound %.4f   rms err: GPU %.3e, torch fp32 CPU %.3e" %
          (label, worst, np.sqrt(e_gpu / n), np.sqrt(e_cpu / n)))
    assert worst <= 1.0, (label, worst)
    return worst


def test_neg_cent_within_the_derived_bound():
    net, _ = _net("ljs_mini_mb_istft_vits")
    for name, _cfg in GOLD:
        g = load_fixture(name)
        _neg_cent_case(net, g["z_p"], g["m_text"], g["logs_text"], g["y_lengths"], g["x_lengths"], name)
    rs = np.random.RandomState(6)
    for (B, I, Tt, Ts) in ((3, 192, 150, 70), (2, 192, 64, 64), (2, 40, 65, 129), (1, 192, 566, 200)):
        z = (rs.standard_normal((B, I, Tt)) * 1.5).astype(np.float32)
        m = rs.standard_normal((B, I, Ts)).astype(np.float32)
        lg = (rs.standard_normal((B, I, Ts)) * 0.4 - 0.3).astype(np.float32)
        t_y = rs.randint(Tt // 2, Tt + 1, size=B)
        t_x = rs.randint(1, Ts + 1, size=B)
        t_y[0], t_x[0] = Tt, Ts
        _neg_cent_case(net, z, m, lg, t_y, t_x, "random %s" % ((B, I, Tt, Ts),))


# --------------------------------------------------------------------------- 3. end to end, goldens
@pytest.mark.parametrize("name,cfg_name", GOLD)
def test_align_matches_reference_golden(name, cfg_name):
    from test_gpu_infer import _rel
    g = load_fixture(name)
    net, sd = _net(cfg_name, int(g["n_vocab"]), int(g["weight_seed"]))
    x, xl, y, yl = (_cuda(g[k]) for k in ("x", "x_lengths", "y", "y_lengths"))
    sid = _cuda(g["sid"]) if "sid" in g else None
    attn, w, x_mask, y_mask, (z, z_p, m_p, logs_p) = net.align(x, xl, y, yl, sid, noise=_cuda(g["noise"]))
    B, T = g["x"].shape
    Tp = g["y"].shape[2]
    assert w.shape == (B, 1, T) and attn.shape == (B, 1, Tp, T) and w.dtype == torch.float32
    assert np.array_equal(w[:, 0].cpu().numpy(), g["w"].astype(np.float32))        # every token
    assert torch.equal(attn.sum(2), w)
    a = attn[:, 0].cpu().numpy()
    for b in range(B):
        ty = int(g["y_lengths"][b])
        assert np.array_equal(a[b, :ty].sum(1), np.ones(ty)) and a[b, ty:].sum() == 0     # one token per frame
    assert np.array_equal(x_mask[:, 0].cpu().numpy(), (np.arange(T)[None] < g["x_lengths"][:, None]).astype(np.float32))
    assert np.array_equal(y_mask[:, 0].cpu().numpy(), (np.arange(Tp)[None] < g["y_lengths"][:, None]).astype(np.float32))
    r = _rel(z_p.cpu().numpy(), g["z_p"])
    print("%s: z_p rel %.2e" % (name, r))
    assert r < 5e-5                                                                # the bar of the voice-conversion test
    # m_p / logs_p: the gather of the text statistics by the path
    neg = net.align(x, xl, y, yl, sid, noise=_cuda(g["noise"]), outputs=("neg_cent", "w"))
    assert neg[0] is None and neg[4] == (None, None, None, None) and torch.equal(neg[1], w)
    c = align_ref.chain(sd, net.cfg, g["x"], g["x_lengths"], g["y"], g["y_lengths"], g.get("sid"), g["noise"], 1.0)
    tok = a.argmax(2)                                                              # [B, Tp]
    for b in range(B):
        ty = int(g["y_lengths"][b])
        want_m = c["m_text"][b][:, tok[b, :ty]]
        want_l = c["logs_text"][b][:, tok[b, :ty]]
        assert _rel(m_p[b, :, :ty].cpu().numpy(), want_m) < 5e-5
        assert _rel(logs_p[b, :, :ty].cpu().numpy(), want_l) < 5e-5
        if ty < Tp:
            assert float(m_p[b, :, ty:].abs().max()) == 0.0
    # and exactly a gather of the GPU's own text statistics: the same row for all frames of a token
    for b in range(B):
        ty = int(g["y_lengths"][b])
        mp = m_p[b, :, :ty].cpu().numpy()
        same = tok[b, 1:ty] == tok[b, :ty - 1]
        assert np.array_equal(mp[:, 1:][:, same], mp[:, :-1][:, same])
    # the GPU's own matrix against the reference's
    v = neg[5].cpu().numpy()
    for b in range(B):
        ty, tx = int(g["y_lengths"][b]), int(g["x_lengths"][b])
        assert _rel(v[b, :ty, :tx], g["neg_cent"][b, :ty, :tx]) < 5e-5


# --------------------------------------------------------------------------- 4. end to end, random inputs
def test_align_random_inputs_are_near_optimal():
    """No stability arranged: the GPU path P must be near-optimal under the float64 chain's matrix v.  With P* the
    float64 optimum and v~ the GPU's own matrix:
        score_v(P*) - score_v(P) <= sum_{P*}|v~ - v| + sum_P|v~ - v| + 2 t_y 2^-24 sum_P|v|
    (exact-arithmetic optimality of P under v~, plus the rounding of t_y fp32 additions)."""
    from mb_istft_vits_amd import synth
    n_cases, n_diff = 0, 0
    for ci, cfg_name in enumerate(CONFIGS):
        net, sd = _net(cfg_name)
        cfg = net.cfg
        for k in range(4):
            rs = np.random.RandomState(50 + 10 * ci + k)
            B, T, Tp = 3, int(rs.randint(6, 30)), int(rs.randint(40, 70))
            x, xl, sid = synth.synthetic_batch(cfg, B, T, seed=60 + 10 * ci + k, ragged=True)
            yl = np.asarray([int(rs.randint(xl[b], Tp + 1)) for b in range(B)], np.int64)
            yl[int(rs.randint(0, B))] = Tp
            y = np.abs(rs.standard_normal((B, cfg.spec_channels, Tp))).astype(np.float32) * 2.0
            for b in range(B):
                y[b, :, yl[b]:] = 0
            noise = rs.standard_normal((B, cfg.inter_channels, Tp)).astype(np.float32)
            r = net.align(_cuda(x), _cuda(xl), _cuda(y), _cuda(yl), _cuda(sid), noise=_cuda(noise), noise_scale=0.7,
                          outputs=("attn", "neg_cent"))
            P_all, vt_all = r[0][:, 0].cpu().numpy(), r[5].cpu().numpy().astype(np.float64)
            c = align_ref.chain(sd, cfg, x, xl, y, yl, sid, noise, 0.7)
            for b in range(B):
                ty, tx = int(yl[b]), int(xl[b])
                v, vt, P = c["neg_cent"][b, :ty, :tx], vt_all[b, :ty, :tx], P_all[b, :ty, :tx]
                assert np.array_equal(P.sum(1), np.ones(ty)) and (P.sum(0) >= 1).all()
                Ps = align_ref.maximum_path_each(v, ty, tx, np.float64)[0]
                d = np.abs(vt - v)
                rhs = (d * Ps).sum() + (d * P).sum() + 2 * ty * 2.0 ** -24 * (np.abs(v) * P).sum()
                gap = align_ref.path_score(v, Ps) - align_ref.path_score(v, P)
                assert gap <= rhs, (cfg_name, k, b, gap, rhs)
                n_cases += 1
                n_diff += int(not np.array_equal(P, Ps))
    print("random inputs: %d cases, %d with P != P*" % (n_cases, n_diff))
    assert n_cases >= 48


# --------------------------------------------------------------------------- 5. round trip
def _golden_inputs(name):
    g = load_fixture(name)
    return g, tuple(_cuda(g[k]) for k in ("x", "x_lengths", "y", "y_lengths")) + (_cuda(g["sid"]) if "sid" in g else None,)


@pytest.mark.parametrize("name,cfg_name", GOLD)
def test_round_trip_durations_reproduce_the_alignment(name, cfg_name):
    g, (x, xl, y, yl, sid) = _golden_inputs(name)
    net, _ = _net(cfg_name, int(g["n_vocab"]), int(g["weight_seed"]))
    attn, w, *_ = net.align(x, xl, y, yl, sid, noise=_cuda(g["noise"]))
    out = net.infer(x, xl, sid, noise_scale=0, durations=w)
    Tp = int(yl.max())
    assert out[4].shape == attn.shape and torch.equal(out[4], attn)
    assert out[0].shape[-1] == net.cfg.samples_per_frame * Tp
    o2 = net.infer(x, xl, sid, noise_scale=0, durations=w[:, 0].to(torch.int64), outputs=("o",))[0]
    assert torch.equal(o2, out[0])                                                  # int64 [B, T] = float [B, 1, T]
    r = net._run(x, xl, sid, 0, 1, None, decode=False, durations=w)
    assert torch.equal(r[8], w.sum(2)[:, 0].to(torch.int64)) and torch.equal(r[8], yl)
    za = net.infer_z_only(x, xl, sid, noise_scale=0, durations=w)
    assert torch.equal(za[0], attn)


def test_default_infer_is_untouched_by_align_and_durations_calls():
    g, (x, xl, y, yl, sid) = _golden_inputs("align_uudb_b2")
    net, _ = _net("uudb_ms_istft_vits_ms", int(g["n_vocab"]), int(g["weight_seed"]))

    def default():
        torch.manual_seed(11)
        return net.infer(x, xl, sid, noise_scale=0.667, length_scale=1.1)

    def same(a, b):
        flat = lambda r: list(r[:6]) + list(r[6])
        return all((p is None and q is None) or torch.equal(p, q) for p, q in zip(flat(a), flat(b)))

    before = default()
    attn, w, *_ = net.align(x, xl, y, yl, sid)
    net.infer(x, xl, sid, durations=w)
    assert same(before, default())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        b2 = default()
        net.align(x, xl, y, yl, sid)
        net.infer(x, xl, sid, durations=w)
        a2 = default()
    side.synchronize()
    assert same(b2, a2) and same(before, a2)


@pytest.mark.parametrize("cfg_name", ("ljs_mini_mb_istft_vits", "uudb_ms_istft_vits_ms"))
def test_own_durations_reproduce_the_default_call_bitwise(cfg_name):
    from mb_istft_vits_amd import synth
    net, _ = _net(cfg_name)
    x, xl, sid = synth.synthetic_batch(net.cfg, 3, 25, seed=8, ragged=True)
    x, xl, sid = _cuda(x), _cuda(xl), _cuda(sid)
    torch.manual_seed(21)
    a = net.infer(x, xl, sid, noise_scale=0.5)
    logw = net.read_stage("logw").reshape(3, 1, 25)
    mask = (torch.arange(25, device="cuda")[None] < xl[:, None]).unsqueeze(1).float()
    wd = torch.ceil(torch.exp(logw) * mask)
    torch.manual_seed(21)
    b = net.infer(x, xl, sid, noise_scale=0.5, durations=wd)
    for p, q in zip(list(a[:6]) + list(a[6]), list(b[:6]) + list(b[6])):
        assert (p is None and q is None) or torch.equal(p, q)


# --------------------------------------------------------------------------- 6. hygiene
def _count_syncs(fn):
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            fn()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    return sum("synchroniz" in str(v.message).lower() for v in w)


def test_align_synchronises_once():
    g, (x, xl, y, yl, sid) = _golden_inputs("align_uudb_b2")
    net, _ = _net("uudb_ms_istft_vits_ms", int(g["n_vocab"]), int(g["weight_seed"]))
    net.align(x, xl, y, yl, sid)                                        # (first-call allocations)
    assert _count_syncs(lambda: net.align(x, xl, y, yl, sid)) == 1     # the status read-back
    assert _count_syncs(lambda: net.align(x, xl, y, yl, sid, outputs=("w",))) == 1


def test_single_speaker_posterior_encoder_runs():
    """enc_q without g (voice_conversion never ran it so): the WN stack takes a null conditioning vector."""
    g, (x, xl, y, yl, sid) = _golden_inputs("align_mini_b2")
    assert sid is None
    net, _ = _net("ljs_mini_mb_istft_vits", int(g["n_vocab"]), int(g["weight_seed"]))
    assert net.n_speakers == 0
    r = net.align(x, xl, y, yl, None, noise_scale=0)
    z = r[4][0]
    assert torch.isfinite(z).all() and float(z.abs().max()) > 0
    with pytest.raises(ValueError):
        net.align(x, xl, y[:, :-1], yl)                                  # a wrong y shape


def test_error_paths_leave_the_handle_usable():
    g, (x, xl, y, yl, sid) = _golden_inputs("align_uudb_b2")
    net, _ = _net("uudb_ms_istft_vits_ms", int(g["n_vocab"]), int(g["weight_seed"]))
    good = net.align(x, xl, y, yl, sid, noise_scale=0)

    def still_fine():
        again = net.align(x, xl, y, yl, sid, noise_scale=0)
        assert torch.equal(again[0], good[0]) and torch.equal(again[4][1], good[4][1])

    with pytest.raises(ValueError):                                      # t_x > t_y
        net.align(x, xl, y, torch.tensor([40, 10]).cuda(), sid)
    still_fine()
    with pytest.raises(ValueError):                                      # zero lengths
        net.align(x, torch.tensor([24, 0]).cuda(), y, yl, sid)
    with pytest.raises(ValueError):
        net.align(x, xl, y, torch.tensor([0, 52]).cuda(), sid)
    still_fine()
    with pytest.raises(ValueError):                                      # a wrong y shape
        net.align(x, xl, y[:, :100], yl, sid)
    with pytest.raises(ValueError):
        net.align(x, xl, y[:1], yl, sid)
    with pytest.raises(IndexError):                                      # lengths outside the tensors, sid out of range
        net.align(x, xl, y, torch.tensor([40, 53]).cuda(), sid)
    with pytest.raises(IndexError):
        net.align(x, xl, y, yl, torch.tensor([0, 10 ** 6]).cuda())
    still_fine()
    w = good[1]
    bad = w.clone()
    bad[0, 0, 2] = -1
    with pytest.raises((ValueError, IndexError)):                        # a negative duration
        net.infer(x, xl, sid, durations=bad)
    frac = w.clone()
    frac[1, 0, 0] = 1.5
    with pytest.raises((ValueError, IndexError)):
        net.infer(x, xl, sid, durations=frac)
    with pytest.raises(ValueError):                                      # a wrong shape
        net.infer(x, xl, sid, durations=w[:, :, :-1])
    with pytest.raises(ValueError):
        net.infer(x, xl, sid, durations=w, length_scale=1.2)
    still_fine()
    out = net.infer(x, xl, sid, noise_scale=0, durations=w)
    assert torch.equal(out[4], good[0])
    with pytest.raises(NotImplementedError, match="align"):
        net.forward(x, xl, y, yl, sid)
