"""Pooled voice conversion, host side (no GPU): the classes of frame counts that may share a posterior run
(`mbv_convert_plan`) against the conv planner itself (`mbv_conv_plan`), the cuts of a class, the checks of
`models.ConvertRequest`, and what `convert_streams` / `admit` refuse before they need a device."""
import ctypes as C

import numpy as np
import pytest
import torch

from mb_istft_vits_amd import _capi, models, stream, utils as mutils, wire

CONFIGS = ["ljs_mini_mb_istft_vits", "ljs_mb_istft_vits", "uudb_ms_istft_vits_ms"]
CR = models.ConvertRequest


def _net(name):
    hps = mutils.get_hparams_from_file(mutils.builtin_config(name))
    return models.SynthesizerTrn(59, hps.data.filter_length // 2 + 1, hps.train.segment_size // hps.data.hop_length,
                                 n_speakers=hps.data.n_speakers, **hps.model)


def _route(Cin, Cout, T, B=1, lens=(False, True), epi=_capi.CONV_EPI_STORE):
    """The planner's route for a 1x1 conv over T frames (masked on its input / output as the posterior path masks)."""
    some = (C.c_int32 * 1)(1)
    d = _capi.MbvConvDesc()
    d.B, d.Cin, d.Cout, d.Tin, d.T, d.K, d.dil, d.x_rstride = B, Cin, Cout, T, T, 1, 1, T
    d.kind, d.epi, d.in_slope, d.out_scale, d.splitk = _capi.CONV_KIND_CONV, epi, 1.0, 1.0, 0
    if lens[0]:
        d.in_lens = C.cast(some, C.c_void_p)
    if lens[1]:
        d.out_lens = C.cast(some, C.c_void_p)
    out = (C.c_int32 * 8)()
    if _capi.lib().mbv_conv_plan(C.byref(d), C.byref(out)):
        raise _capi.MbvError(_capi.lib().mbv_last_error(None).decode())
    return _capi.ROUTES[out[0]]


def _posterior_convs(cfg):
    """(Cin, Cout, masked input) of enc_q.pre (on the spectrogram padded to a multiple of 32 channels), enc_q.proj,
    and a coupling layer's pre / post."""
    H, I = cfg.hidden_channels, cfg.inter_channels
    cpad = -(-cfg.spec_channels // 32) * 32
    return [(cpad, H, False), (H, 2 * I, True), (I // 2, H, False), (H, I // 2, True)]


@pytest.mark.parametrize("name", CONFIGS)
def test_two_classes_split_at_256_frames(name):
    net = _net(name)
    lens = [1, 16, 255, 256, 257, 300]
    assert net.convert_plan(lens) == (2, [0, 0, 0, 0, 1, 1])
    # the order of the input decides the numbering, not the length
    assert net.convert_plan([300, 16, 257, 1, 256, 255]) == (2, [0, 1, 0, 1, 1, 1])
    assert net.convert_plan(torch.tensor([5, 256, 100, 1])) == (1, [0, 0, 0, 0])
    assert net.convert_plan([1000, 257, 4000]) == (1, [0, 0, 0])
    # the low-latency mode routes on the launch size anyway: one class
    assert net.convert_plan(lens, splitk=True) == (1, [0] * 6)


@pytest.mark.parametrize("name", CONFIGS)
def test_a_class_plans_one_route_from_its_shortest_to_its_longest_request(name):
    """The classes come from the planner: every conv of the posterior path is sent to the same kernel family for the
    shortest and the longest request of a class, alone and as a row of the padded run; across the cut it is not."""
    net = _net(name)
    lens = [1, 2, 15, 16, 17, 32, 33, 64, 100, 255, 256, 257, 300, 1000]
    runs, run_of = net.convert_plan(lens)
    narrow = lambda r: r.startswith("NARROW")
    families = []
    for k in range(runs):
        mine = [t for t, r in zip(lens, run_of) if r == k]
        lo, hi = min(mine), max(mine)
        for Cin, Cout, masked in _posterior_convs(net.cfg):
            alone = {narrow(_route(Cin, Cout, t, lens=(masked, True))) for t in (lo, hi)}
            padded = narrow(_route(Cin, Cout, hi, B=len(mine), lens=(masked, True)))
            assert alone == {padded}, (name, k, (Cin, Cout), lo, hi)
        families.append(narrow(_route(net.cfg.hidden_channels, 2 * net.cfg.inter_channels, hi, lens=(True, True))))
    assert families == [True, False]


def test_plan_refusals():
    net = _net("uudb_ms_istft_vits_ms")
    with pytest.raises(ValueError, match="without frames"):
        net.convert_plan([5, 0, 7])
    with pytest.raises(ValueError, match="no requests"):
        net.convert_plan([])
    L = _capi.lib()
    cfg = net._config_struct()
    one = (C.c_int32 * 1)(5)
    assert L.mbv_convert_plan(C.byref(cfg), 0, 0, one, None) == -1
    assert L.mbv_convert_plan(C.byref(cfg), 0, 1, None, None) == -1
    assert L.mbv_convert_plan(None, 0, 1, one, None) == -1
    assert L.mbv_convert_plan(C.byref(cfg), 0, 1, (C.c_int32 * 1)(-3), None) == -1
    assert L.mbv_convert_plan(C.byref(cfg), 0, 1, one, None) == 1         # run_of_request is optional


def test_a_class_is_cut_at_the_grid_and_at_the_fused_wn_layers():
    net = _net("uudb_ms_istft_vits_ms")
    cfg = net.cfg
    # 65 535 rows a run (the grid's y / z extent)
    runs, run_of = net.convert_plan([5] * 65537)
    assert runs == 2 and run_of[65534] == 0 and run_of[65535] == 1 and run_of[65536] == 1
    assert net.convert_plan([5] * 65535)[0] == 1
    # the fused WN layers address h / skip with 32-bit byte offsets: B * channels * T * 4 bytes < 4 GiB
    ch = max(cfg.hidden_channels, cfg.inter_channels)
    T = 1 << 20
    B = -(-(1 << 32) // (4 * ch * T))                   # the first batch that reaches 4 GiB
    assert B > 2
    runs, run_of = net.convert_plan([T] * B)
    assert runs == 2 and run_of == [0] * (B - 1) + [1]
    assert net.convert_plan([T] * (B - 1), splitk=True)[0] == 1 and net.convert_plan([T] * B, splitk=True)[0] == 2
    # a short request joins the open run only while the padded run fits
    assert net.convert_plan([T] * (B - 1) + [7]) == (2, [0] * (B - 1) + [1])
    # one request beyond the limit has no run at all
    with pytest.raises(ValueError, match="refused"):
        net.convert_plan([-(-(1 << 32) // (4 * ch))])
    assert net.convert_plan([-(-(1 << 32) // (4 * ch)) - 1])[0] == 1


def test_convert_request_validation():
    w = torch.zeros(4000)
    r = CR(w, 2, 5, 16000, 256, 1024, noise_scale=0.5, chunk_frames=8, max_chunk_frames=32)
    assert (r.sid_src, r.sid_tgt, r.in_sr, r.model_sr, r.noise_scale) == (2, 5, 16000, 16000, 0.5)
    assert r.model_samples() == 4000 and r.frames(1024) == 15
    assert CR(w, torch.tensor([3]), torch.tensor(4), 16000, 256, 1024).sid_src == 3
    assert CR(np.zeros(10, np.int16), 0, 1, 16000, 256, 800).wave.dtype == torch.int16
    up = CR(torch.zeros(2401, dtype=torch.int16), 0, 1, 16000, 256, 1024, in_sr=24000)
    assert up.in_sr == 24000 and up.model_samples() == 1601          # ceil(2401 * 16000 / 24000)
    assert not hasattr(r, "n_fft")
    with pytest.raises(ValueError, match="empty wave"):
        CR(torch.zeros(0), 0, 1, 16000, 256, 1024)
    with pytest.raises(ValueError, match="1-D"):
        CR(torch.zeros(1, 400), 0, 1, 16000, 256, 1024)
    with pytest.raises(TypeError, match="int16 or float32"):
        CR(torch.zeros(400, dtype=torch.float64), 0, 1, 16000, 256, 1024)
    with pytest.raises(TypeError, match="int16 or float32"):
        CR(torch.zeros(400, dtype=torch.int32), 0, 1, 16000, 256, 1024)
    with pytest.raises(ValueError, match="win_size"):
        CR(w, 0, 1, 16000, 256, 0)
    with pytest.raises(ValueError, match="win_size"):
        CR(w, 0, 1, 16000, 256, 4097)
    # the constructor's upper bound is the largest transform the library takes: the two must not drift
    L = _capi.lib()
    assert L.mbv_spectrogram_frames(0, CR.MAX_N_FFT, 1) >= 0 and L.mbv_spectrogram_frames(0, 2 * CR.MAX_N_FFT, 1) == -1
    with pytest.raises(ValueError, match="noise_scale"):
        CR(w, 0, 1, 16000, 256, 1024, noise_scale=-0.1)
    with pytest.raises(ValueError, match="noise_scale"):
        CR(w, 0, 1, 16000, 256, 1024, noise_scale=float("nan"))
    with pytest.raises(TypeError, match="sid_tgt"):
        CR(w, 0, 1.5, 16000, 256, 1024)
    with pytest.raises(ValueError, match="one speaker id"):
        CR(w, torch.tensor([1, 2]), 0, 16000, 256, 1024)
    with pytest.raises(ValueError, match="chunk_frames"):
        CR(w, 0, 1, 16000, 256, 1024, chunk_frames=64, max_chunk_frames=32)
    with pytest.raises(ValueError, match="sample rates"):
        CR(w, 0, 1, 16000, 256, 1024, in_sr=0)


def test_convert_streams_refuses_before_it_needs_a_device():
    """What does not depend on the handle is refused first: these raise on a machine without a GPU."""
    ms = _net("uudb_ms_istft_vits_ms")
    w = torch.zeros(4000)
    good = CR(w, 0, 1, 16000, 256, 1024)
    assert ms.convert_streams([]) == []
    with pytest.raises(TypeError, match="models.ConvertRequest"):
        ms.convert_streams([(w, 0, 1)])
    with pytest.raises(TypeError, match="models.ConvertRequest"):
        ms.convert_streams([good, models.Request([1, 2], sid=0)])
    for other in (CR(w, 0, 1, 22050, 256, 1024), CR(w, 0, 1, 16000, 128, 1024), CR(w, 0, 1, 16000, 256, 800)):
        with pytest.raises(ValueError, match="request 1: .*one data config"):
            ms.convert_streams([good, other])
    with pytest.raises(ValueError, match="win_size 2048 must be in \\[1, n_fft"):
        ms.convert_streams([CR(w, 0, 1, 16000, 256, 2048)])
    with pytest.raises(ValueError, match="request 1: 100 samples at 16000 Hz give no spectrogram frame"):
        ms.convert_streams([good, CR(torch.zeros(100), 0, 1, 16000, 256, 1024)])
    with pytest.raises(IndexError, match="request 1: .*sid_tgt 12"):
        ms.convert_streams([good, CR(w, 0, ms.n_speakers, 16000, 256, 1024)])
    with pytest.raises(IndexError, match="request 0: .*sid_src -1"):
        ms.convert_streams([CR(w, -1, 0, 16000, 256, 1024)])
    with pytest.raises(AssertionError, match="n_speakers have to be larger than 0."):
        _net("ljs_mini_mb_istft_vits").convert_streams([good])
    with pytest.raises(AssertionError, match="n_speakers have to be larger than 0."):
        _net("ljs_mini_mb_istft_vits").convert_stream(w, 0, 1, 16000, 256, 1024)


def test_admit_takes_one_kind_of_request():
    ms = _net("uudb_ms_istft_vits_ms")
    sp = stream.StreamPool(ms)
    pp = wire.PcmPool(ms, sp, 16000, 24000)
    audio, text = CR(torch.zeros(4000), 0, 1, 16000, 256, 1024), models.Request([1, 2, 3], sid=0)
    for pool in (sp, pp):
        with pytest.raises(TypeError, match="all models.Request or all models.ConvertRequest"):
            pool.admit([audio, text])
        with pytest.raises(TypeError, match="all models.Request or all models.ConvertRequest"):
            pool.admit([text, audio, text])
        with pytest.raises(TypeError, match="models.Request"):
            pool.admit([([1, 2], 0)])
        assert pool.admit([]) == []
    assert len(sp.streams) == 0 and len(pp.followers) == 0


def test_frame_count_is_the_librarys():
    """The host side's frame count is `mbv_spectrogram_frames`, on both sides of every multiple of the hop."""
    L = _capi.lib()
    n_fft, hop = 1024, 256
    for k in range(0, 4):
        for n in (k * hop - 1, k * hop, k * hop + 1):
            if n < 0:
                continue
            want = L.mbv_spectrogram_frames(n, n_fft, hop)
            assert models.spectrogram_frames(n, n_fft, hop) == want, n
            if n:
                assert CR(torch.zeros(n), 0, 1, 16000, hop, n_fft).frames(n_fft) == want, n
    assert L.mbv_spectrogram_frames(255, n_fft, hop) == 0 and L.mbv_spectrogram_frames(256, n_fft, hop) == 1
    for n_fft, hop, n in ((1024, 255, 1000), (512, 128, 129), (2048, 512, 5000), (1024, 300, 12345)):
        assert models.spectrogram_frames(n, n_fft, hop) == L.mbv_spectrogram_frames(n, n_fft, hop)
