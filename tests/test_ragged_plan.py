"""Row-exact ragged decode, host side (no GPU): the partition of z-lengths into classes (`mbv_ragged_classes`) against
the conv planner (`mbv_conv_plan`), and the oracle statement of what the mode is for — a row decoded alone equals the
oracle's batched decode of that row only when no batch-mate is longer."""
import ctypes as C

import numpy as np
import pytest
import torch

from mb_istft_vits_amd import _capi, models, synth, utils as mutils
from mb_istft_vits_amd.spec import DEC_SB
from oracle import ref_infer

RB2 = {"resblock": "2", "resblock_dilation_sizes": [[1, 3], [1, 3], [1, 3]]}
CONFIGS = [("ljs_mb_istft_vits", None), ("ljs_mini_mb_istft_vits", None), ("ljs_ms_istft_vits", None),
           ("uudb_ms_istft_vits_ms", None), ("ljs_istft_vits", None), ("ljs_mini_istft_vits", None),
           ("ljs_mini_mb_istft_vits", RB2)]
IDS = [c[0] + ("_rb2" if c[1] else "") for c in CONFIGS]
T_MAX = 300


def _net(name, overrides=None):
    hps = mutils.get_hparams_from_file(mutils.builtin_config(name))
    for k, v in (overrides or {}).items():
        hps.model[k] = v
    return models.SynthesizerTrn(59, hps.data.filter_length // 2 + 1, hps.train.segment_size // hps.data.hop_length,
                                 n_speakers=hps.data.n_speakers, **hps.model)


def _conv(Cin, Cout, K, dil, T, epi, **kw):
    d = _capi.MbvConvDesc()
    d.B, d.Cin, d.Cout, d.Tin, d.T, d.K, d.dil = 1, Cin, Cout, T, T, K, dil
    d.kind, d.epi, d.in_slope, d.out_scale = _capi.CONV_KIND_CONV, epi, 0.1, 1.0
    if epi != _capi.CONV_EPI_STORE:
        d.res = 1                       # "a residual is given": the planner only tests pointers against null
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def decoder_descs(cfg, length):
    """Every conv of the decoder, as `run_decoder` launches it for ONE utterance of `length` z-frames."""
    sb = cfg.decoder == DEC_SB
    us, C0 = (8 if sb else 4), cfg.upsample_initial_channel
    out = [_conv(cfg.inter_channels, C0, 7, 1, length, _capi.CONV_EPI_STORE, in_slope=1.0)]
    L = length
    for i in range(2):
        ch, Lo = C0 >> (i + 1), us * L
        out.append(_conv(C0 >> i, ch, 0, 1, L, _capi.CONV_EPI_STORE,
                         kind=_capi.CONV_KIND_CONVT8 if sb else _capi.CONV_KIND_CONVT4))
        for k, dils in zip(cfg.resblock_kernel_sizes, cfg.resblock_dilation_sizes):
            for q, d in enumerate(dils):
                last = _capi.CONV_EPI_RESID_ACC if q == len(dils) - 1 else _capi.CONV_EPI_RESID
                if cfg.resblock == "2":
                    out.append(_conv(ch, ch, k, d, Lo, last))
                else:
                    out.append(_conv(ch, ch, k, d, Lo, _capi.CONV_EPI_STORE))
                    out.append(_conv(ch, ch, k, 1, Lo, last))
        L = Lo
    out.append(_conv(C0 >> 2, 18 if sb else 72, 7, 1, L + 1, _capi.CONV_EPI_STORE, Tin=L, reflect1=1, in_slope=0.01))
    return out


def routes(cfg, length):
    L = _capi.lib()
    r = []
    for d in decoder_descs(cfg, length):
        out = (C.c_int32 * 8)()
        assert L.mbv_conv_plan(C.byref(d), C.byref(out)) == 0, L.mbv_last_error(None)
        r.append(int(out[0]))
    return tuple(r)


def class_of(first, length):
    return max(i for i, f in enumerate(first) if f <= length)


@pytest.mark.parametrize("name,overrides", CONFIGS, ids=IDS)
def test_classes_are_the_planner_routes(name, overrides):
    """Lengths 1 .. 300: two lengths share a class iff every decoder conv, planned at that length alone, takes the
    same route; the classes are intervals."""
    net = _net(name, overrides)
    first = net.ragged_classes(T_MAX)
    assert first[0] == 1 and first == sorted(set(first)) and first[-1] <= T_MAX
    sig = {t: routes(net.cfg, t) for t in range(1, T_MAX + 1)}
    cls = {t: class_of(first, t) for t in sig}
    by_class, by_sig = {}, {}
    for t in sig:
        by_class.setdefault(cls[t], set()).add(sig[t])
        by_sig.setdefault(sig[t], set()).add(cls[t])
    assert all(len(v) == 1 for v in by_class.values()), by_class        # one route vector per class
    assert all(len(v) == 1 for v in by_sig.values()), by_sig            # and one class per route vector
    # the cuts are where a conv crosses the narrow kernel's 256 columns: never more than a handful of classes
    assert 2 <= len(first) <= 5, first
    narrow = tuple(k for k, v in _capi.ROUTES.items() if v.startswith("NARROW"))
    assert len(narrow) == 2
    for f in first[1:]:
        before, after = sig[f - 1], sig[f]
        assert any((x in narrow) != (y in narrow) for x, y in zip(before, after)), (f, before, after)


def test_class_values():
    """What DESIGN §7.5 quotes: conv_pre at 256 frames, the ResBlock convs at 256 / us and 256 / us^2."""
    assert _net("ljs_mb_istft_vits").ragged_classes(T_MAX) == [1, 17, 65, 257]
    assert _net("uudb_ms_istft_vits_ms").ragged_classes(T_MAX) == [1, 17, 65, 257]
    assert _net("ljs_mini_istft_vits").ragged_classes(T_MAX) == [1, 5, 33, 257]
    assert _net("ljs_mb_istft_vits").ragged_classes(40) == [1, 17]


def test_splitk_mode_is_one_class():
    net = _net("ljs_mini_mb_istft_vits")
    assert net.ragged_classes(T_MAX, splitk=True) == [1]


def test_bad_arguments():
    net = _net("ljs_mini_mb_istft_vits")
    with pytest.raises(ValueError):
        net.ragged_classes(0)


def test_runs_follow_the_classes():
    net = _net("ljs_mb_istft_vits")
    lens = [300, 0, 16, 17, 64, 65, 256, 257, 9, 0, 41]
    n, rows = net.ragged_plan(lens)
    first = net.ragged_classes(300)
    assert n == 4
    for b, v in enumerate(lens):
        assert rows[b] == (-1 if v == 0 else class_of(first, v)), (b, v, rows)
    assert net.ragged_plan([5, 0, 3]) == (1, [0, -1, 0])
    assert net.ragged_plan([0, 0]) == (0, [-1, -1])
    assert net.ragged_plan(lens, splitk=True)[0] == 1
    for bad in ([5, -1], [5, 301]):
        with pytest.raises(ValueError):
            net.ragged_plan(bad, t_frames=300)


def test_runs_are_cut_below_2gib_and_65535_rows():
    """A run's largest tensor (stage 1: C0 / 4 channels x us^2 T columns) stays below 2 GiB, as a stand-alone decode's
    must for `conv1d_narrow_supported` to answer alike; the gather kernel's grid caps a run at 65535 rows."""
    net = _net("ljs_mb_istft_vits")
    cfg = net.cfg
    T, B = 1000, 600
    per_row = 4 * max(cfg.inter_channels * T, (cfg.upsample_initial_channel // 4) * 16 * T, 72 * (16 * T + 1))
    n, rows = net.ragged_plan([T] * B)
    counts = [rows.count(r) for r in range(n)]
    assert sum(counts) == B and n == -(-B * per_row // (2 ** 31 - 1)) and n >= 3, (n, counts)
    assert all(c * per_row < 2 ** 31 for c in counts) and all((c + 1) * per_row >= 2 ** 31 for c in counts[:-1])
    assert rows == sorted(rows)                                   # whole blocks of rows, in order
    n, rows = net.ragged_plan([1] * 70000)
    assert n == 2 and rows.count(0) == 65535 and rows.count(1) == 70000 - 65535


# ---------------------------------------------------------------------------------------------------------------
# The oracle statement of the goal, on the inputs of the issue's table: three rows of 70 / 41 / 9 z-frames.
LENS = (70, 41, 9)


def _decode(sd, cfg, z, g):
    with torch.no_grad():
        return ref_infer.decode(sd, cfg, z, g)[0][:, 0].numpy().astype(np.float64)


@pytest.mark.parametrize("name", ["ljs_mini_mb_istft_vits", "ljs_mini_istft_vits", "uudb_ms_istft_vits_ms"])
def test_oracle_row_alone_against_row_in_batch(name):
    net = _net(name)
    cfg = net.cfg
    sd = synth.make_state_dict(cfg, 1234)
    spf = cfg.samples_per_frame
    rng = np.random.default_rng(11)
    z = torch.from_numpy(rng.standard_normal((3, cfg.inter_channels, LENS[0])).astype(np.float32))
    for b, n in enumerate(LENS):
        z[b, :, n:] = 0
    g = None
    if cfg.gin_channels:
        g = torch.from_numpy(rng.standard_normal((3, cfg.gin_channels, 1)).astype(np.float32))
    Rc = net.decoder_context()[1]
    alone = [_decode(sd, cfg, z[b:b + 1, :, :n].contiguous(), None if g is None else g[b:b + 1])[0]
             for b, n in enumerate(LENS)]
    batch = _decode(sd, cfg, z, g)
    # (a) no batch-mate is longer: the batched row IS the stand-alone row (two conv shapes in torch: rounding only)
    for b, n in enumerate(LENS):
        sub = _decode(sd, cfg, z[b:, :, :n].contiguous(), None if g is None else g[b:])[0]
        err = np.abs(sub[:spf * n] - alone[b]).max() / np.abs(alone[b]).max()
        print("%s row %d alone vs first of its batch: %.3g of the peak" % (name, n, err))
        assert err <= 1e-5, (n, err)
    # (b) a longer batch-mate: the last R frames of the row differ far beyond rounding
    for b, n in list(enumerate(LENS))[1:]:
        w = spf * min(Rc, n)
        d = batch[b, spf * n - w:spf * n] - alone[b][-w:]
        rel = np.sqrt(np.mean(d * d)) / np.sqrt(np.mean(alone[b][-w:] ** 2))
        print("%s row %d in the batch vs alone, last %d frames: relative RMS %.3g" % (name, n, min(Rc, n), rel))
        assert rel > 1e-2, (n, rel)
