"""Pooled streaming decode, host side (no GPU): the decoder runs of one `mbv_decode_chunks` call (`mbv_chunks_plan`)
against the classes of the ragged decode, and what a `StreamPool` refuses before anything is launched."""
import ctypes as C

import pytest
import torch

from mb_istft_vits_amd import _capi, models, stream, utils as mutils

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


def class_of(first, length):
    return max(i for i, f in enumerate(first) if f <= length)


@pytest.mark.parametrize("name,overrides", CONFIGS, ids=IDS)
def test_runs_are_the_classes_of_the_utterance_lengths(name, overrides):
    """t_frames from both sides of every class cut: two chunks share a run iff their utterances share a class, and
    the runs are as many as the classes that hold a chunk — whatever the order, and with lengths repeated."""
    net = _net(name, overrides)
    first = net.ragged_classes(T_MAX)
    assert len(first) >= 2
    t = [T_MAX, 1, 9, 41]
    for f in first[1:]:
        t += [f, f - 1, f]
    t = t[1::2] + t[0::2]                                   # not sorted
    n, runs = net.chunks_plan(t)
    cls = [class_of(first, v) for v in t]
    assert n == len(set(cls)) == len(first)
    for i in range(len(t)):
        for j in range(len(t)):
            assert (runs[i] == runs[j]) == (cls[i] == cls[j]), (t[i], t[j], runs, cls)
    assert sorted(set(runs)) == list(range(n))
    # a subset that leaves classes empty
    sub = [v for v in t if class_of(first, v) in (0, len(first) - 1)]
    n2, runs2 = net.chunks_plan(sub)
    assert n2 == 2 and len(set(runs2)) == 2
    one = [v for v in t if class_of(first, v) == 1]
    assert net.chunks_plan(one) == (1, [0] * len(one))
    # split-K mode: nothing is bitwise across launch sizes anyway, one run
    assert net.chunks_plan(t, splitk=True) == (1, [0] * len(t))


def test_runs_are_cut_below_2gib_and_65535_rows():
    """The cuts of `mbv_ragged_plan` for rows of those lengths (tests/test_ragged_plan.py), reproduced."""
    net = _net("ljs_mb_istft_vits")
    cfg = net.cfg
    T, B = 1000, 600
    per_row = 4 * max(cfg.inter_channels * T, (cfg.upsample_initial_channel // 4) * 16 * T, 72 * (16 * T + 1))
    n, rows = net.chunks_plan([T] * B)
    counts = [rows.count(r) for r in range(n)]
    assert sum(counts) == B and n == -(-B * per_row // (2 ** 31 - 1)) and n >= 3, (n, counts)
    assert all(c * per_row < 2 ** 31 for c in counts) and all((c + 1) * per_row >= 2 ** 31 for c in counts[:-1])
    assert rows == sorted(rows)
    assert (n, rows) == net.ragged_plan([T] * B)
    n, rows = net.chunks_plan([1] * 70000)
    assert n == 2 and rows.count(0) == 65535 and rows.count(1) == 70000 - 65535
    mixed = [300, 16, 17, 64, 65, 256, 257, 9, 41] * 3
    assert net.chunks_plan(mixed) == net.ragged_plan(mixed)


def test_bad_arguments():
    net = _net("ljs_mini_mb_istft_vits")
    L = _capi.lib()
    cfg = net._config_struct()
    t = (C.c_int32 * 3)(20, 30, 40)                        # one class
    out = (C.c_int32 * 3)()
    assert L.mbv_chunks_plan(C.byref(cfg), 0, 3, t, out) == 1
    assert L.mbv_chunks_plan(C.byref(cfg), 0, 3, t, None) == 1            # run_of_chunk is optional
    assert L.mbv_chunks_plan(None, 0, 3, t, out) == -1
    assert L.mbv_chunks_plan(C.byref(cfg), 0, 0, t, out) == -1
    assert L.mbv_chunks_plan(C.byref(cfg), 0, -2, t, out) == -1
    assert L.mbv_chunks_plan(C.byref(cfg), 0, 3, None, out) == -1
    for bad in ((20, 0, 40), (20, -5, 40)):
        assert L.mbv_chunks_plan(C.byref(cfg), 0, 3, (C.c_int32 * 3)(*bad), out) == -1
    cfg.decoder = 77
    assert L.mbv_chunks_plan(C.byref(cfg), 0, 3, t, out) == -1
    for bad in ([], [5, 0]):
        with pytest.raises(ValueError):
            net.chunks_plan(bad)


def test_pool_refuses_a_batch_on_the_host():
    """A stream of B > 1 rows is refused by `add` with the reason, before any launch (this test has no GPU)."""
    net = _net("ljs_mini_mb_istft_vits")
    pool = net.stream_pool()
    assert isinstance(pool, stream.StreamPool) and len(pool) == 0
    st2 = stream.DecodeStream(net, None, torch.zeros(2, net.cfg.inter_channels, 40), None, 32, 256)
    with pytest.raises(ValueError, match="ONE utterance"):
        pool.add(st2)
    with pytest.raises(TypeError):
        pool.add(object())
    other = _net("ljs_mini_mb_istft_vits")
    st1 = stream.DecodeStream(other, None, torch.zeros(1, net.cfg.inter_channels, 40), None, 32, 256)
    with pytest.raises(ValueError, match="another model"):
        pool.add(st1)
    assert len(pool) == 0 and pool.step() == []
