"""-m gpu: per-token prosody -- a tensor `length_scale`, `extra_frames=` and `fit_frames=` on every entry
that takes `length_scale`, through `mbv_shape_durations` / `mbv_shape_durations_rows` / `mbv_op_shape_durations`.
Everything but the reference golden and the fit's distance to float64 is exact: the shaped durations are compared
bitwise with the existing scalar path, the existing `durations=` path and the stand-alone `infer_stream`.

Measured on an MI355X (this file's printed figures are in DESIGN 7.19)."""
import ctypes as C

import numpy as np
import pytest
import torch

import prosody_ref as P
from helpers import load_fixture, rms
from mb_istft_vits_amd import _capi, wire
from mb_istft_vits_amd.models import Request, frames_of_ms

pytestmark = pytest.mark.gpu

NETS = {"mini": ("ljs_mini_mb_istft_vits", None), "uudb": ("uudb_ms_istft_vits_ms", None),
        "sdp": ("ljs_mini_mb_istft_vits", {"use_sdp": True})}
GOLD = (("prosody_mini_b2", "ljs_mini_mb_istft_vits"), ("prosody_uudb_b2", "uudb_ms_istft_vits_ms"))
TEXTS = (1, 20, 257, 300)          # the scan carries across chunks of 256
SCALES = np.asarray([0.0, 0.5, 1.0, 1.75, 3.0], np.float32)
SEED = 7                           # every call is seeded: the SDP's draw, and with it logw, is the same in all of them
_nets, _batches, _plain = {}, {}, {}


def _net(name):
    from gpu_util import make_net
    if name not in _nets:
        cfg_name, overrides = NETS.get(name, (name, None))
        _nets[name] = make_net(cfg_name, overrides=overrides)[0]
    return _nets[name]


def _batch(name, T):
    """B = 3, ragged, one row of length 1: (x, x_lengths, sid) on the device, lens on the host."""
    if (name, T) not in _batches:
        net = _net(name)
        g = torch.Generator().manual_seed(1000 + T)
        lens = [T, 1, max(1, 2 * T // 3)]
        x = torch.randint(1, 59, (3, T), generator=g)
        for b, n in enumerate(lens):
            x[b, n:] = 0
        sid = torch.randint(0, net.cfg.n_speakers, (3,), generator=g).cuda() if net.n_speakers > 0 else None
        _batches[(name, T)] = (x.cuda(), torch.tensor(lens).cuda(), sid, lens)
    return _batches[(name, T)]


def _stream(name, T, **kw):
    """One seeded `infer_stream(marks=True)` -> dict: w [3, T] (the stage w_ceil), y (y_lengths), marks, z, st."""
    net = _net(name)
    x, xl, sid, _ = _batch(name, T)
    kw.setdefault("length_scale", 1.0)
    st = net.infer_stream(x, xl, sid, noise_scale=0.5, noise_scale_w=0.8, seed=SEED, marks=True, **kw)
    return dict(w=net.read_stage("w_ceil").view(3, T).cpu().numpy(), y=st.y_lengths.cpu().numpy(), marks=st.marks,
                z=st.z, st=st, logw=net.read_stage("logw").view(3, T).cpu().numpy())


def _scalar(name, T, s):
    """The existing scalar path at length_scale s, once per (model, T, s)."""
    key = (name, T, float(s))
    if key not in _plain:
        _plain[key] = _stream(name, T, length_scale=float(s))
    return _plain[key]


def _mask(T, lens):
    return np.arange(T)[None, :] < np.asarray(lens)[:, None]


def _table(T, seed):
    rs = np.random.RandomState(seed)
    return SCALES[rs.randint(0, len(SCALES), size=(3, T))]


def _extras(T, seed):
    rs = np.random.RandomState(seed)
    return (rs.randint(1, 30, size=(3, T)) * (rs.uniform(size=(3, T)) < 0.3)).astype(np.int64)


CASES = [(n, T) for n in NETS for T in TEXTS]


# ------------------------------------------------------------------------------------------------ 1, 9
@pytest.mark.parametrize("name, T", CASES)
def test_constant_tensor_is_bitwise_the_scalar(name, T):
    net = _net(name)
    want = _scalar(name, T, 1.75)
    runs = net.shape_runs()
    again = _stream(name, T, length_scale=1.75)                       # 9: a float and nothing else launches nothing new
    assert net.shape_runs() == runs
    shape = (3, T) if T % 2 else (3, 1, T)
    got = _stream(name, T, length_scale=torch.full(shape, 1.75).cuda())
    assert net.shape_runs() == runs + 1
    for r in (again, got):
        assert np.array_equal(r["w"], want["w"]) and np.array_equal(r["y"], want["y"]) and r["marks"] == want["marks"]
        assert torch.equal(r["z"], want["z"])
    assert got["st"].fit_scale is None and got["st"].fit_status is None


def test_constant_tensor_gives_the_scalar_waveform():
    net = _net("mini")
    x, xl, sid, _ = _batch("mini", 20)
    kw = dict(noise_scale=0.5, seed=SEED, outputs=("o", "z", "y_mask"))
    a = net.infer(x, xl, sid, length_scale=0.5, **kw)
    b = net.infer(x, xl, sid, length_scale=torch.full((3, 1, 20), 0.5), **kw)      # (a host tensor is moved over)
    assert torch.equal(a[0], b[0]) and torch.equal(a[6][0], b[6][0]) and torch.equal(a[5], b[5])


# ------------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("name, T", CASES)
def test_every_token_has_the_duration_of_the_scalar_call_at_its_own_scale(name, T):
    _, _, _, lens = _batch(name, T)
    tab = _table(T, 11 + T)
    got = _stream(name, T, length_scale=torch.from_numpy(tab).cuda())
    m = _mask(T, lens)
    assert np.array_equal(got["w"][~m], np.zeros((~m).sum(), np.float32))
    for s in SCALES:
        sel = m & (tab == s)
        if s == 0:
            assert not got["w"][sel].any()                         # a 0 drops the token
        else:
            assert np.array_equal(got["w"][sel], _scalar(name, T, s)["w"][sel])
    assert np.array_equal(got["y"], np.maximum(got["w"].sum(1), 1).astype(np.int64))


# ------------------------------------------------------------------------------------------------ 3
@pytest.mark.parametrize("name, T", CASES)
def test_extra_frames_are_added_to_the_token(name, T):
    _, _, _, lens = _batch(name, T)
    m = _mask(T, lens)
    ex = _extras(T, 21 + T)
    base = _scalar(name, T, 1.75)
    got = _stream(name, T, length_scale=1.75, extra_frames=torch.from_numpy(ex).cuda())       # the scalar is s_t
    assert np.array_equal(got["w"], base["w"] + ex * m)
    tab = _table(T, 31 + T)
    base = _stream(name, T, length_scale=torch.from_numpy(tab).cuda())
    got = _stream(name, T, length_scale=torch.from_numpy(tab).cuda(), extra_frames=torch.from_numpy(ex).int().cuda())
    assert np.array_equal(got["w"], base["w"] + ex * m)
    for b in range(3):                                              # a token's span includes its extras
        assert np.array_equal(np.diff(got["marks"][b]), got["w"][b, :lens[b]].astype(np.int64))
        assert len(got["marks"][b]) == lens[b] + 1 and got["marks"][b][-1] == int(got["w"][b].sum())


# ------------------------------------------------------------------------------------------------ 4
@pytest.mark.parametrize("name", list(NETS))
def test_shaped_call_is_bitwise_the_call_with_those_durations(name):
    net, T = _net(name), 20
    x, xl, sid, _ = _batch(name, T)
    tab, ex = torch.from_numpy(_table(T, 41)).cuda(), torch.from_numpy(_extras(T, 42)).cuda()
    kw = dict(noise_scale=0.667, noise_scale_w=0.8, seed=SEED, outputs=("o", "z", "y_mask", "attn"))
    a = net.infer(x, xl, sid, length_scale=tab, extra_frames=ex, **kw)
    w = a[4].sum(2)                                                  # [3, 1, T]
    assert torch.equal(w.view(3, T), net.read_stage("w_ceil").view(3, T))      # what the rows of attn sum to
    b = net.infer(x, xl, sid, durations=w, **kw)
    for i in (0, 5, 4):
        assert torch.equal(a[i], b[i])
    assert torch.equal(a[6][0], b[6][0])


# ------------------------------------------------------------------------------------------------ 5
def _rel(got, ref):
    return rms(np.asarray(got) - np.asarray(ref)) / max(rms(ref), 1e-3)


@pytest.mark.parametrize("fixture, cfg_name", GOLD)
def test_tensor_length_scale_matches_the_reference_golden(fixture, cfg_name, monkeypatch):
    from gpu_util import make_net
    gold = load_fixture(fixture)
    net, _ = make_net(cfg_name, int(gold["n_vocab"]), int(gold["weight_seed"]))
    x, xl = torch.from_numpy(gold["x"]).cuda(), torch.from_numpy(gold["x_lengths"]).cuda()
    sid = torch.from_numpy(gold["sid"]).cuda() if "sid" in gold else None
    noise, real = gold["noise"], torch.randn

    def pinned(*size, **kw):                                       # the prior draw of the call: the reference's
        shape = tuple(size[0]) if len(size) == 1 and not isinstance(size[0], int) else size
        if shape == noise.shape:
            return torch.from_numpy(noise).to(kw.get("device", "cpu"))
        return real(*size, **kw)

    monkeypatch.setattr(torch, "randn", pinned)
    o, _, _, _, attn, y_mask, (z, z_p, m_p, logs_p), _ = net.infer(
        x, xl, sid, noise_scale=float(gold["noise_scale"]), length_scale=torch.from_numpy(gold["scale"]).cuda())
    monkeypatch.undo()
    assert np.array_equal(attn.sum(2).cpu().numpy(), gold["w"])                  # durations exact
    assert np.array_equal(y_mask.cpu().numpy(), gold["y_mask"])
    for nm, t in (("m_p", m_p), ("logs_p", logs_p), ("z_p", z_p), ("z", z)):
        r = _rel(t.cpu().numpy(), gold[nm])
        print("%s %s: relative rms error %.3e" % (fixture, nm, r))
        assert r < 5e-5, (nm, r)
    e = rms(o.cpu().numpy() - gold["o"])
    print("%s o: rms error %.3e" % (fixture, e))
    assert e < 1e-4


# ------------------------------------------------------------------------------------------------ 6
def _row_total(w, b, lens):
    return int(w[b, :lens[b]].sum())


@pytest.mark.parametrize("with_table", [False, True], ids=["scalar", "table"])
@pytest.mark.parametrize("name, T", [("mini", 20), ("uudb", 257), ("sdp", 300), ("mini", 1)])
def test_fit_is_the_largest_factor_that_fits(name, T, with_table):
    net = _net(name)
    _, _, _, lens = _batch(name, T)
    lo, hi = np.float32(0.5), np.float32(2.0)
    tab = np.maximum(_table(T, 51 + T), np.float32(0.5)) if with_table else np.ones((3, T), np.float32)
    ex = _extras(T, 52 + T) if with_table else np.zeros((3, T), np.int64)
    m = _mask(T, lens)

    def run(f_rows):
        """w through the path of tests 1-2: the scalar f (no table, no extras; one call per distinct f) or the table
        fl32(s_t * f) with the extras."""
        f_rows = np.asarray(f_rows, np.float32)
        if with_table:
            t = (tab * f_rows[:, None]).astype(np.float32)
            return _stream(name, T, length_scale=torch.from_numpy(t).cuda(), extra_frames=torch.from_numpy(ex).cuda())["w"]
        w = np.zeros((3, T), np.float32)
        for f in np.unique(f_rows):
            w[f_rows == f] = _scalar(name, T, f)["w"][f_rows == f]
        return w

    d_lo, d_hi, d_1 = (np.asarray([_row_total(run([f] * 3), b, lens) for b in range(3)]) for f in (lo, hi, 1.0))
    # row 0: fits somewhere inside; row 1 (one token): not even at lo; row 2: at hi with room to spare
    frames = [int(d_1[0]) + 1 if d_1[0] + 1 < d_hi[0] else int(d_hi[0]) - 1, max(1, int(d_lo[1]) - 1), int(d_hi[2]) + 9]
    kw = dict(fit_frames=frames, fit_bounds=(float(lo), float(hi)))
    if with_table:
        kw.update(length_scale=torch.from_numpy(tab).cuda(), extra_frames=torch.from_numpy(ex).cuda())
    got = _stream(name, T, **kw)
    f = np.asarray(got["st"].fit_scale, np.float32)
    status = list(got["st"].fit_status)
    assert np.array_equal(net.read_stage("fit_scale").cpu().numpy(), f)
    assert net.read_stage("fit_status").cpu().tolist() == [float(s) for s in status]
    assert status == [1 if d_lo[b] > frames[b] else 0 for b in range(3)]
    assert status[1] == (1 if d_lo[1] > frames[1] else 0) and f[2] == hi and status[2] == 0
    assert np.array_equal(got["w"], run(f))                         # bitwise the existing path at f*
    up = run(np.nextafter(f, np.float32(np.inf)))
    worst = 0.0
    for b in range(3):
        total = _row_total(got["w"], b, lens)
        if status[b]:
            assert f[b] == lo and total == d_lo[b] > frames[b]
            continue
        assert lo <= f[b] <= hi and total <= frames[b]
        assert f[b] == hi or _row_total(up, b, lens) > frames[b]
        f64, s64, n = P.fit(got["logw"][b, :lens[b]], tab[b, :lens[b]], ex[b, :lens[b]], frames[b], lo, hi)
        assert s64 == 0 and n <= 32
        worst = max(worst, abs(float(f[b]) - float(f64)) / float(f[b]))
    print("fit %s T=%d %s: f = %s status = %s, worst |f - f64| / f = %.3g (%.2f x 2^-24)"
          % (name, T, "table" if with_table else "scalar", f, status, worst, worst * 2 ** 24))
    assert worst <= P.FIT_BAR
    assert np.array_equal(got["y"], np.maximum((got["w"] * m).sum(1), 1).astype(np.int64))


# ------------------------------------------------------------------------------------------------ 7
def _op(net, inp, fit=None, scalar=1.0):
    from gpu_util import ptr
    h = net._ensure_handle()
    B, T = inp["logw"].shape
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    logw, lens, scale, extra, bad = (dev(inp.get(k)) for k in ("logw", "lens", "scale", "extra", "bad"))
    w = torch.full((B, T), -7.0, device="cuda")
    cum = torch.full((B, T), -7, dtype=torch.int32, device="cuda")
    y32 = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    y64 = torch.full((B,), -7, dtype=torch.int64, device="cuda")
    fit_out = torch.zeros(B, dtype=torch.int64, device="cuda")
    fit_host = None if fit is None else (_capi.MbvFit * B)(*fit)
    keep = logw.clone()
    _capi.check(h, _capi.lib().mbv_op_shape_durations(h, ptr(logw), ptr(lens), ptr(scale), ptr(extra), float(scalar),
                                                      fit_host, ptr(w), ptr(cum), ptr(y32), ptr(y64), ptr(bad),
                                                      ptr(fit_out), B, T, net._stream()), "mbv_op_shape_durations")
    assert torch.equal(logw.view(torch.int32), keep.view(torch.int32))
    res = [_capi.fit_result(v) for v in fit_out.tolist()]
    return dict(w_ceil=w.cpu().numpy(), cum=cum.cpu().numpy(), ylen32=y32.cpu().numpy(), ylen64=y64.cpu().numpy(),
                fit_scale=np.asarray([r[0] for r in res], np.float32), fit_status=[r[1] for r in res])


@pytest.mark.parametrize("case", list(P.OP_BY_NAME))
def test_op_against_float64(case):
    c = P.OP_BY_NAME[case]
    inp = P.op_inputs(c)
    got = _op(_net("mini"), inp)
    left = P.op_check(c, inp, got)
    print("%s: %d of %d tokens left out" % (case, left, int(_mask(c["T"], c["lens"]).sum())))
    if "edge" in c["plant"] or "edge_extra" in c["plant"]:
        assert got["ylen64"].tolist()[1] == -1 and got["ylen32"].tolist()[1] == 1 and got["ylen64"][0] > 0
    m = _mask(c["T"], c["lens"])
    assert not got["w_ceil"][~m].any()


def test_op_fit_past_the_register_tiles():
    """T = 2304 > 8 x 256: the tokens the search recomputes from memory count like the others."""
    net = _net("mini")
    c = P.OP_BY_NAME["shape_t2304"]
    inp = P.op_inputs(c)
    lens = c["lens"]
    D = lambda b, f: P.total(inp["logw"][b, :lens[b]], inp["scale"][b, :lens[b]], inp["extra"][b, :lens[b]], f)
    frames = [D(0, 1.3), D(1, 0.7)]                                 # (float64 totals at factors inside the bounds)
    assert all(D(b, 0.5) < frames[b] < D(b, 2.0) for b in range(2))
    got = _op(net, inp, fit=[(n, 0.5, 2.0) for n in frames])
    f = got["fit_scale"]
    assert got["fit_status"] == [0, 0] and np.all((f > 0.5) & (f < 2.0))
    for ff, cmp in ((f, "le"), (np.nextafter(f, np.float32(np.inf)), "gt")):     # D through the op itself, without a fit
        tab = dict(inp, scale=(inp["scale"] * ff[:, None]).astype(np.float32))
        r = _op(net, tab)
        if cmp == "le":
            assert np.array_equal(r["w_ceil"], got["w_ceil"]) and np.array_equal(r["cum"], got["cum"])
        for b in range(2):
            assert (r["ylen32"][b] <= frames[b]) if cmp == "le" else (r["ylen32"][b] > frames[b])
    for b in range(2):
        f64, s64, _ = P.fit(inp["logw"][b, :lens[b]], inp["scale"][b, :lens[b]], inp["extra"][b, :lens[b]], frames[b], 0.5, 2.0)
        assert abs(float(f[b]) - float(f64)) / float(f[b]) <= P.FIT_BAR


def test_entries_refuse_before_any_launch():
    net = _net("mini")
    inp = P.op_inputs(P.OP_BY_NAME["shape_t20"])
    runs = net.shape_runs()
    for fit in ([(5, 0.0, 2.0)] * 3, [(5, 2.0, 1.0)] * 3, [(5, 1.0, float("inf"))] * 3, [(-1, 0.5, 2.0)] * 3,
                [(5, float("nan"), 2.0)] * 3):
        with pytest.raises(_capi.MbvError):
            _op(net, inp, fit=fit)
    with pytest.raises(_capi.MbvError):
        _op(net, dict(inp, scale=None, extra=None))                 # nothing to do
    with pytest.raises(_capi.MbvError):
        _op(net, inp, scalar=1.5)                                    # a table with a scalar other than 1
    assert net.shape_runs() == runs
    # the model entry, after an encode at length_scale 1.5
    x, xl, sid, _ = _batch("mini", 20)
    net.infer_z_only(x, xl, sid, length_scale=1.5, seed=SEED)
    h = net._ensure_handle()
    y = torch.zeros(3, dtype=torch.int64, device="cuda")
    tab = torch.ones(3, 20, device="cuda")
    L = _capi.lib()
    assert L.mbv_shape_durations(h, C.c_void_p(tab.data_ptr()), None, None, 3, 20, None, C.c_void_p(y.data_ptr()), net._stream()) != 0
    assert L.mbv_shape_durations(h, None, None, None, 3, 20, None, C.c_void_p(y.data_ptr()), net._stream()) != 0
    assert L.mbv_shape_durations(h, None, None, (_capi.MbvFit * 3)(*[(0, 0.5, 2.0)] * 3), 3, 20, None,
                                 C.c_void_p(y.data_ptr()), net._stream()) != 0
    assert net.shape_runs() == runs


# ------------------------------------------------------------------------------------------------ 8
def _ids(T, seed):
    return torch.randint(1, 59, (T,), generator=torch.Generator().manual_seed(seed))


def _requests():
    """Shaped and plain requests mixed, in both text classes (T <= 256 and beyond): (T, keyword arguments)."""
    tab = lambda T, s: torch.from_numpy(SCALES[1:][np.random.RandomState(s).randint(0, 4, size=T)])
    ex = lambda T, s: torch.from_numpy(_extras(T, s)[0])
    return [(20, dict(length_scale=tab(20, 1), extra_frames=ex(20, 2), marks=True)),
            (7, dict(length_scale=1.1)),
            (300, dict(fit_frames=700, marks=True)),
            (1, dict(extra_frames=torch.tensor([12]))),
            (257, dict(length_scale=0.9, marks=True)),
            (40, dict(length_scale=tab(40, 3), fit_frames=90, fit_bounds=(0.75, 1.5))),
            (280, dict(length_scale=tab(280, 4))),
            (33, dict())]


def _same_stream(a, b):
    assert torch.equal(a.z, b.z) and torch.equal(a.y_lengths, b.y_lengths)
    assert a.marks == b.marks and a.schedule == b.schedule
    assert a.fit_scale == b.fit_scale and a.fit_status == b.fit_status


@pytest.mark.parametrize("name", ["mini", "uudb", "sdp"])
def test_pooled_admission_is_bitwise_the_stand_alone_stream(name):
    net = _net(name)
    sid = 3 if net.n_speakers > 0 else None
    spec = _requests()
    common = dict(noise_scale=0.5, noise_scale_w=0.8, chunk_frames=16, max_chunk_frames=64)
    reqs = [Request(_ids(T, 60 + i), sid=sid, seed=90 + i, **common, **kw) for i, (T, kw) in enumerate(spec)]
    is_shaped = lambda kw: torch.is_tensor(kw.get("length_scale")) or "extra_frames" in kw or "fit_frames" in kw
    n_runs, run_of = net.admit_plan([T for T, _ in spec])
    shaped_runs = len({run_of[i] for i, (_, kw) in enumerate(spec) if is_shaped(kw)})
    assert n_runs >= 2 and shaped_runs == n_runs                    # both text classes hold a shaped row
    enc, shp = net.encoder_runs(), net.shape_runs()
    sts = net.infer_streams(reqs)
    assert net.encoder_runs() == enc + n_runs and net.shape_runs() == shp + shaped_runs
    assert sts[2].fit_status in (0, 1) and sts[5].fit_status in (0, 1) and sts[0].fit_scale is None
    for i, (T, kw) in enumerate(spec):
        kw = {k: (v.cuda().view(1, -1) if torch.is_tensor(v) else v) for k, v in kw.items()}
        alone = net.infer_stream(_ids(T, 60 + i).view(1, -1).cuda(), torch.tensor([T]).cuda(),
                                 None if sid is None else torch.tensor([sid]).cuda(), seed=[90 + i], **common, **kw)
        _same_stream(sts[i], alone)
    # a call without a shaped row: the encoder runs move as before, the shape runs do not
    plain = [r for r, (_, kw) in zip(reqs, spec) if not is_shaped(kw)]
    enc, shp = net.encoder_runs(), net.shape_runs()
    net.infer_streams(plain)
    assert net.encoder_runs() == enc + net.admit_plan([r.x.numel() for r in plain])[0] and net.shape_runs() == shp
    # one class shaped, the other not: one launch
    enc, shp = net.encoder_runs(), net.shape_runs()
    net.infer_streams([reqs[0], reqs[1], reqs[4]])
    assert net.encoder_runs() == enc + net.admit_plan([20, 7, 257])[0] and net.shape_runs() == shp + 1


def test_turn_with_a_pause_on_a_token_is_bitwise_the_streams_appended():
    net = _net("mini")
    MODEL_SR, RATE = 22050, 24000
    pause = frames_of_ms(300, MODEL_SR, net.cfg.samples_per_frame)
    assert pause == 26
    texts = [(9, 71), (14, 72)]
    extra = [torch.zeros(T, dtype=torch.int32) for T, _ in texts]
    extra[0][4] = pause                                             # a held token inside the first sentence
    extra[1][0] = 3
    common = dict(noise_scale=0.5, length_scale=1.2, chunk_frames=8, max_chunk_frames=16, marks=True)
    runs = net.shape_runs()

    def drive(admit):
        pp = wire.pcm_pool(net, net.stream_pool(), MODEL_SR, RATE)
        turn = pp.add_turn(1 << 18)
        if admit:
            sts = turn.admit([Request(_ids(T, s), seed=s, extra_frames=e, **common) for (T, s), e in zip(texts, extra)],
                             pauses_ms=[0.0, 40.0])
        else:
            sts = [net.infer_stream(_ids(T, s).view(1, -1).cuda(), torch.tensor([T]).cuda(), None, seed=[s],
                                    extra_frames=e.view(1, -1).cuda(), **common) for (T, s), e in zip(texts, extra)]
            for st, p in zip(sts, (0.0, 40.0)):
                turn.append(st, p)
        turn.close()
        n = 0
        while not turn.finished:
            pp.step()
            n += 1
            assert n < 500
        return turn, sts

    a, sa = drive(True)
    assert net.shape_runs() == runs + 1
    b, sb = drive(False)
    for x, y in zip(sa, sb):
        _same_stream(x, y)
        assert torch.equal(x.o, y.o)
    assert sa[0].marks[5] - sa[0].marks[4] > pause                  # the token's own frames and the pause
    assert torch.equal(a.valid_samples, b.valid_samples) and torch.equal(a.pcm, b.pcm)
    assert a.marks == b.marks


# ------------------------------------------------------------------------------------------------ 10
@pytest.mark.parametrize("what", ["negative scale", "nan scale", "inf scale", "negative extra"])
def test_bad_values_flag_the_row_and_the_handle_serves_the_next_call(what):
    name, T = "mini", 20
    net = _net(name)
    x, xl, sid, lens = _batch(name, T)                              # lens [20, 1, 13]
    tab, ex = np.ones((3, T), np.float32), np.zeros((3, T), np.int64)
    bad = {"negative scale": -0.5, "nan scale": np.nan, "inf scale": np.inf}.get(what)

    def call(t_bad):
        s, e = tab.copy(), ex.copy()
        if bad is None:
            e[2, t_bad] = -1
        else:
            s[2, t_bad] = bad
        return net.infer_z_only(x, xl, sid, length_scale=torch.from_numpy(s).cuda(), extra_frames=torch.from_numpy(e).cuda(),
                                seed=SEED)

    with pytest.raises(IndexError):
        call(5)
    with pytest.raises(IndexError):
        call(12)
    call(13)                                                        # behind x_lengths[2]: not looked at
    call(19)
    with pytest.raises(IndexError):                                 # ... and through the pooled entry
        kw = dict(length_scale=torch.from_numpy(tab[0, :13].copy())) if bad is None else \
            dict(length_scale=torch.tensor([1.0] * 12 + [bad]))
        if bad is None:
            kw["extra_frames"] = torch.tensor([0] * 12 + [-1])
        net.infer_streams([Request(_ids(9, 1), seed=1), Request(_ids(13, 2), seed=2, **kw)])
    # the same handle then passes test 1
    want = _scalar(name, T, 1.75)
    got = _stream(name, T, length_scale=torch.full((3, T), 1.75).cuda())
    assert np.array_equal(got["w"], want["w"]) and torch.equal(got["z"], want["z"]) and got["marks"] == want["marks"]
