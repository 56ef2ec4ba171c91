"""Pooled admission, host side (no GPU): the classes of text lengths that may share a front-half run
(`mbv_admit_plan`) against the conv planner itself (`mbv_conv_plan`), and the checks of `models.Request`."""
import ctypes as C

import pytest
import torch

from mb_istft_vits_amd import _capi, models, utils as mutils

CONFIGS = ["ljs_mini_mb_istft_vits", "ljs_mb_istft_vits", "uudb_ms_istft_vits_ms"]


def _net(name, overrides=None):
    hps = mutils.get_hparams_from_file(mutils.builtin_config(name))
    for k, v in (overrides or {}).items():
        hps.model[k] = v
    return models.SynthesizerTrn(59, hps.data.filter_length // 2 + 1, hps.train.segment_size // hps.data.hop_length,
                                 n_speakers=hps.data.n_speakers, **hps.model)


def _route(Cin, Cout, K, T, B=1, splitk=0):
    """The planner's route for a plain conv of a text of T tokens."""
    d = _capi.MbvConvDesc()
    d.B, d.Cin, d.Cout, d.Tin, d.T, d.K, d.dil, d.x_rstride = B, Cin, Cout, T, T, K, 1, T
    d.kind, d.epi, d.in_slope, d.out_scale, d.splitk = _capi.CONV_KIND_CONV, _capi.CONV_EPI_STORE, 1.0, 1.0, splitk
    out = (C.c_int32 * 8)()
    if _capi.lib().mbv_conv_plan(C.byref(d), C.byref(out)):
        raise _capi.MbvError(_capi.lib().mbv_last_error(None).decode())
    return _capi.ROUTES[out[0]]


def _text_encoder_convs(cfg):
    H, Fc = cfg.hidden_channels, cfg.filter_channels
    return [(H, 3 * H, 1), (H, H, 1), (H, Fc, cfg.kernel_size), (Fc, H, cfg.kernel_size), (H, 2 * cfg.inter_channels, 1)]


@pytest.mark.parametrize("name", CONFIGS)
def test_two_classes_split_at_256(name):
    net = _net(name)
    lens = [1, 16, 255, 256, 257, 300]
    runs, run_of = net.admit_plan(lens)
    assert runs == 2
    assert run_of == [0, 0, 0, 0, 1, 1]
    # the order of the input decides the numbering, not the length
    runs, run_of = net.admit_plan([300, 16, 257, 1, 256, 255])
    assert runs == 2 and run_of == [0, 1, 0, 1, 1, 1]
    assert net.admit_plan(torch.tensor([5, 256, 100, 1]))[0] == 1
    assert net.admit_plan([5, 256, 100, 1])[1] == [0, 0, 0, 0]
    assert net.admit_plan([257])[0] == 1 and net.admit_plan([1000, 257, 4000]) == (1, [0, 0, 0])
    # the low-latency mode routes on the launch size anyway: one class
    assert net.admit_plan(lens, splitk=True) == (1, [0] * 6)


def test_sdp_model_has_the_same_classes():
    net = _net("ljs_mini_mb_istft_vits", {"use_sdp": True})
    assert net.admit_plan([1, 16, 255, 256, 257, 300]) == (2, [0, 0, 0, 0, 1, 1])


@pytest.mark.parametrize("name", CONFIGS)
def test_a_class_plans_one_route_from_its_shortest_to_its_longest_text(name):
    """The classes come from the planner: a text-encoder conv of the shortest and of the longest text of a class is
    sent to the same kernel family, alone and as a row of the padded run; across the cut it is not."""
    net = _net(name)
    lens = [1, 2, 15, 16, 17, 32, 33, 64, 100, 255, 256, 257, 300, 1000]
    runs, run_of = net.admit_plan(lens)
    narrow = lambda r: r.startswith("NARROW")
    families = []
    for k in range(runs):
        mine = [t for t, r in zip(lens, run_of) if r == k]
        lo, hi = min(mine), max(mine)
        for Cin, Cout, K in _text_encoder_convs(net.cfg):
            alone = {narrow(_route(Cin, Cout, K, t)) for t in (lo, hi)}
            padded = narrow(_route(Cin, Cout, K, hi, B=len(mine)))
            assert alone == {padded}, (name, k, (Cin, Cout, K), lo, hi)
        families.append(narrow(_route(net.cfg.hidden_channels, net.cfg.hidden_channels, 1, hi)))
    assert families == [True, False]


def test_refusals():
    net = _net("ljs_mini_mb_istft_vits")
    with pytest.raises(ValueError, match="empty text"):
        net.admit_plan([5, 0, 7])
    with pytest.raises(ValueError, match="no requests"):
        net.admit_plan([])
    L = _capi.lib()
    cfg = net._config_struct()
    one = (C.c_int32 * 1)(5)
    assert L.mbv_admit_plan(C.byref(cfg), 0, 0, one, None) == -1
    assert L.mbv_admit_plan(C.byref(cfg), 0, 1, None, None) == -1
    assert L.mbv_admit_plan(None, 0, 1, one, None) == -1
    assert L.mbv_admit_plan(C.byref(cfg), 0, 1, (C.c_int32 * 1)(-3), None) == -1
    assert L.mbv_admit_plan(C.byref(cfg), 0, 1, one, None) == 1           # run_of_request is optional


def test_a_run_is_cut_where_the_padded_launch_would_leave_the_narrow_kernel():
    """Rows of one class stay in one run only while B rows padded to the longest text plan as one row does: the
    narrow kernel addresses its tensors with 32-bit byte offsets, so a large enough run is cut in two."""
    net = _net("ljs_mb_istft_vits")
    cfg = net.cfg
    widest = max(3 * cfg.hidden_channels, cfg.filter_channels, 2 * cfg.inter_channels)
    B = -(-(1 << 31) // (4 * widest * 256))            # the first batch whose widest tensor reaches 2 GiB at T = 256
    runs, run_of = net.admit_plan([256] * B)
    assert runs == 2 and run_of[:B - 1] == [0] * (B - 1) and run_of[B - 1] == 1
    assert net.admit_plan([256] * (B - 1))[0] == 1
    assert _route(cfg.hidden_channels, widest, 1, 256, B=B - 1).startswith("NARROW")
    assert not _route(cfg.hidden_channels, widest, 1, 256, B=B).startswith("NARROW")


def test_request_validation():
    R = models.Request
    r = R([3, 4, 5], sid=2, noise_scale=0.5, max_len=40, chunk_frames=8, max_chunk_frames=32)
    assert r.x.dtype == torch.int64 and r.x.tolist() == [3, 4, 5] and r.sid == 2 and r.max_len == 40
    assert r.durations is None and r.durations_dtype is None
    assert R(torch.tensor([1, 2]), sid=torch.tensor([3])).sid == 3
    d = R([1, 2, 3], durations=torch.tensor([[[2., 0., 5.]]]))
    assert d.durations.shape == (3,) and d.durations_dtype == 2
    assert R([1, 2, 3], durations=torch.tensor([2, 0, 5], dtype=torch.int32)).durations_dtype == 0
    assert R([1, 2, 3], durations=torch.tensor([2, 0, 5])).durations_dtype == 1
    assert R([1, 2, 3], durations=torch.tensor([2, 0, 5], dtype=torch.int16)).durations.dtype == torch.int64
    with pytest.raises(ValueError, match="empty text"):
        R([])
    with pytest.raises(ValueError, match="1-D"):
        R(torch.zeros(1, 4, dtype=torch.int64))
    with pytest.raises(TypeError, match="integer token ids"):
        R(torch.zeros(4))
    with pytest.raises(ValueError, match="length_scale must be 1"):
        R([1, 2, 3], length_scale=1.3, durations=torch.tensor([1, 1, 1]))
    with pytest.raises(ValueError, match="durations must be"):
        R([1, 2, 3], durations=torch.tensor([1, 1]))
    with pytest.raises(ValueError, match="durations must be"):
        R([1, 2, 3], durations=[1, 1, 1])
    with pytest.raises(ValueError, match="chunk_frames"):
        R([1], chunk_frames=64, max_chunk_frames=32)
    with pytest.raises(ValueError, match="chunk_frames"):
        R([1], chunk_frames=0)
    with pytest.raises(ValueError, match="max_len"):
        R([1], max_len=0)
    with pytest.raises(ValueError, match="finite"):
        R([1], noise_scale=float("nan"))
    with pytest.raises(TypeError, match="sid"):
        R([1], sid=1.5)
    with pytest.raises(ValueError, match="one speaker id"):
        R([1], sid=torch.tensor([1, 2]))


def test_infer_streams_refuses_before_it_needs_a_device():
    """What does not depend on the handle is refused first: these raise on a machine without a GPU."""
    ms = _net("uudb_ms_istft_vits_ms")
    with pytest.raises(ValueError, match="request 1: sid is required"):
        ms.infer_streams([models.Request([1, 2], sid=0), models.Request([3])])
    with pytest.raises(TypeError, match="models.Request"):
        ms.infer_streams([([1, 2], 0)])
    assert _net("ljs_mini_mb_istft_vits").infer_streams([]) == []
