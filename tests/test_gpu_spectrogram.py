"""-m gpu: the linear spectrogram (mbv_spectrogram, mel_processing.py:51-70 with center=False) against the
float64 restatement in tests/spectrogram_ref.py, and voice conversion driven from audio
(`wire.convert_pcm16`).

Error bound, calibrated on torch's own fp32 stft against float64 (worst per frame 6.5e-7 ||w x_f||_2,
relative RMS 1.1e-7): per frame max_k |d| <= 4e-6 ||w x_f||_2 + 1e-9, over a call RMS(d) / RMS(ref) <= 5e-7."""
import numpy as np
import pytest
import torch

import spectrogram_ref as SR
from helpers import rms
from oracle import ref_infer as R

pytestmark = pytest.mark.gpu

PARAMS = [(1024, 256, 1024), (512, 128, 512), (2048, 512, 2048), (1024, 256, 800), (1024, 255, 1024),
          (1024, 300, 1024)]


@pytest.fixture(scope="module")
def net():
    from gpu_util import make_net
    return make_net("ljs_mini_mb_istft_vits")[0]


def _check_bound(got, x, n_fft, hop, win):
    """got: [n_fft // 2 + 1, >= frames] of one row; x: its valid samples."""
    ref = SR.spectrogram(x, n_fft, hop, win)
    nf = ref.shape[1]
    d = np.abs(got[:, :nf].astype(np.float64) - ref)
    if nf:
        norms = SR.frame_norms(x, n_fft, hop, win)
        worst = (d.max(axis=0) / (norms + 1e-30)).max()
        assert np.all(d.max(axis=0) <= 4e-6 * norms + 1e-9), worst
        if rms(ref) > 0:
            assert rms(d) / rms(ref) <= 5e-7, rms(d) / rms(ref)
        return worst
    return 0.0


def _audio(rs, n, sr=22050):
    """random audio, a two-tone row, a row whose peak sits at +-1"""
    t = np.arange(n) / sr
    rows = [rs.uniform(-0.5, 0.5, n),
            0.4 * np.sin(2 * np.pi * 440 * t) + 0.3 * np.cos(2 * np.pi * 3001.7 * t + 0.3),
            rs.standard_normal(n) * 0.2]
    rows[2] /= np.abs(rows[2]).max()
    rows[2][rs.randint(n)] = -1.0
    return np.stack(rows).astype(np.float32)


@pytest.mark.parametrize("n_fft,hop,win", PARAMS)
def test_spectrogram_matches_restatement(net, n_fft, hop, win):
    rs = np.random.RandomState(n_fft * 3 + hop + win)
    n = 20011
    x = _audio(rs, n)
    spec, lens = net.spectrogram(torch.from_numpy(x).cuda(), n_fft, hop, win)
    F = SR.frames(n, n_fft, hop)
    assert spec.shape == (3, n_fft // 2 + 1, F) and spec.dtype == torch.float32
    assert lens.dtype == torch.int64 and [int(v) for v in lens.cpu()] == [F] * 3
    spec = spec.cpu().numpy()
    worst = max(_check_bound(spec[b], x[b], n_fft, hop, win) for b in range(3))
    print("(%d, %d, %d): worst per-frame error %.2e of ||w x_f||" % (n_fft, hop, win, worst))
    # [B, 1, n] takes the same path
    spec3, _ = net.spectrogram(torch.from_numpy(x).cuda().unsqueeze(1), n_fft, hop, win)
    assert np.array_equal(spec3.cpu().numpy(), spec)


def test_spectrogram_known_answers(net):
    n_fft, hop, win = 1024, 256, 1024
    n = 8192
    z, lens = net.spectrogram(torch.zeros(2, n, device="cuda"), n_fft, hop, win)
    assert not z.cpu().numpy().any() and int(lens[0]) == SR.frames(n, n_fft, hop)
    # cos at bin k, amplitude A: |X[k]| = A sum(w) / 2 in every frame that lies inside the signal
    k, A = 37, 0.6
    x = (A * np.cos(2 * np.pi * k * np.arange(n) / n_fft)).astype(np.float32)
    spec, _ = net.spectrogram(torch.from_numpy(x).cuda().view(1, n), n_fft, hop, win)
    spec = spec[0].cpu().numpy().astype(np.float64)
    p = (n_fft - hop) // 2
    inside = [f for f in range(spec.shape[1]) if f * hop - p >= 0 and f * hop - p + n_fft <= n]
    want = A * SR.window(n_fft, win).sum() / 2
    norms = SR.frame_norms(x, n_fft, hop, win)
    for f in inside:
        assert abs(spec[k, f] - want) <= 4e-6 * norms[f] + 1e-9, (f, spec[k, f], want)
    _check_bound(spec, x, n_fft, hop, win)


@pytest.mark.parametrize("n_fft,hop,win", [(1024, 256, 1024), (1024, 255, 1024), (512, 128, 400)])
def test_spectrogram_ragged_batch(net, n_fft, hop, win):
    """Lengths around the 0 / 1-frame edges and a full row: spec_lengths follows the rule, frames past it are
    exact zeros, every row is bitwise its own spectrogram computed alone, and samples past valid_samples are
    never read (NaN / 1e30 there change no bit)."""
    p = (n_fft - hop) // 2
    n = 6000
    e = n_fft - 2 * p                                     # the shortest row with one frame
    valid = np.array([0, 1, hop - 1, e - 1, e, e + hop, n, 3001, -5, n + 100], np.int64)
    B = len(valid)
    rs = np.random.RandomState(11)
    x = rs.uniform(-1, 1, (B, n)).astype(np.float32)
    xt = torch.from_numpy(x).cuda()
    vt = torch.from_numpy(valid).cuda()
    spec, lens = net.spectrogram(xt, n_fft, hop, win, valid_samples=vt)
    F = SR.frames(n, n_fft, hop)
    assert spec.shape == (B, n_fft // 2 + 1, F)
    spec_np, lens = spec.cpu().numpy(), lens.cpu().numpy()
    dirty = x.copy()
    for b in range(B):
        v = int(np.clip(valid[b], 0, n))
        nf = SR.frames(v, n_fft, hop)
        assert lens[b] == nf, b
        assert not spec_np[b, :, nf:].any(), b
        _check_bound(spec_np[b], x[b, :v], n_fft, hop, win)
        if v:
            one, l1 = net.spectrogram(xt[b:b + 1, :v].contiguous(), n_fft, hop, win)
            assert int(l1[0]) == nf and one.shape[-1] == nf
            assert np.array_equal(one[0].cpu().numpy(), spec_np[b, :, :nf]), b
        dirty[b, v:] = np.where(np.arange(n - v) % 2, np.float32(np.nan), np.float32(1e30))
    spec2, lens2 = net.spectrogram(torch.from_numpy(dirty).cuda(), n_fft, hop, win, valid_samples=vt)
    assert np.array_equal(spec2.cpu().numpy().view(np.uint32), spec_np.view(np.uint32))
    assert np.array_equal(lens2.cpu().numpy(), lens)


def test_spectrogram_int16_is_fp32_on_scaled_pcm(net):
    rs = np.random.RandomState(5)
    pcm = rs.randint(-32768, 32768, (3, 9000)).astype(np.int16)
    pcm[0, 100] = -32768
    pcm[1, 200] = 32767
    valid = torch.tensor([9000, 4321, 700], device="cuda")
    p16 = torch.from_numpy(pcm).cuda()
    for n_fft, hop, win in [(1024, 256, 1024), (2048, 300, 1500)]:
        a, la = net.spectrogram(p16, n_fft, hop, win, valid_samples=valid)
        b, lb = net.spectrogram(p16.float() / 32768.0, n_fft, hop, win, valid_samples=valid)
        assert torch.equal(la, lb)
        assert np.array_equal(a.cpu().numpy().view(np.uint32), b.cpu().numpy().view(np.uint32))


def test_spectrogram_on_caller_stream(net):
    x = torch.rand(4, 30000, device="cuda") * 2 - 1
    valid = torch.tensor([30000, 17, 12345, 2999], device="cuda")
    ref, lr = net.spectrogram(x, 1024, 256, 1024, valid_samples=valid)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        got, lg = net.spectrogram(x, 1024, 256, 1024, valid_samples=valid)
    s.synchronize()
    assert torch.equal(ref, got) and torch.equal(lr, lg)


def test_spectrogram_output_past_2gib(net):
    """B = 2 rows of 135 M samples: 2.16 GB of output.  Frames at the end of each row (offsets past 2^31
    elements) against the restatement on those samples only."""
    n_fft, hop, win = 1024, 256, 1024
    n = 135_000_000
    torch.manual_seed(0)
    x = torch.rand(2, n, device="cuda") * 2 - 1
    valid = torch.tensor([n, n - 100_003], device="cuda")
    spec, lens = net.spectrogram(x, n_fft, hop, win, valid_samples=valid)
    F = SR.frames(n, n_fft, hop)
    assert spec.numel() * 4 > 2 ** 31 and spec.shape[-1] == F
    p = (n_fft - hop) // 2
    w = SR.window(n_fft, win)
    for b, v in enumerate([n, n - 100_003]):
        nf = SR.frames(v, n_fft, hop)
        assert int(lens[b]) == nf
        f0 = nf - 24
        s0 = f0 * hop - p
        tail = x[b, s0:v].double().cpu().numpy()
        xp = np.concatenate([tail, np.zeros(n_fft)])
        got = spec[b, :, f0:nf].cpu().numpy().astype(np.float64)
        for i in range(nf - f0):
            seg = xp[i * hop:i * hop + n_fft] * w
            ref = np.abs(np.fft.rfft(seg))
            assert np.abs(got[:, i] - ref).max() <= 4e-6 * np.sqrt((seg ** 2).sum()) + 1e-9, (b, i)
        assert not spec[b, :, nf:].any()
    del spec, x
    torch.cuda.empty_cache()


def _pinned_randn(noise):
    real = torch.randn
    return real, (lambda *a, **k: noise if tuple(a) == tuple(noise.shape) else real(*a, **k))


def _vc_audio(rs, B, n, sr):
    t = np.arange(n) / sr
    x = np.stack([0.3 * np.sin(2 * np.pi * (180 + 60 * b) * t) + 0.2 * np.sin(2 * np.pi * 1234.5 * t + b)
                  + 0.05 * rs.standard_normal(n) for b in range(B)])
    return x.astype(np.float32)


def test_voice_conversion_from_audio_matches_oracle():
    """GPU spectrogram -> voice_conversion against the oracle's voice_conversion on the float64 reference
    spectrogram, posterior noise pinned as in test_voice_conversion_matches_reference_golden."""
    from gpu_util import make_net
    net, sd = make_net("uudb_ms_istft_vits_ms")
    n_fft, hop, win = 1024, 256, 1024
    assert net.cfg.spec_channels == n_fft // 2 + 1
    rs = np.random.RandomState(21)
    n = 12800
    valid = np.array([n, 9001], np.int64)
    x = _vc_audio(rs, 2, n, 16000)
    spec, lens = net.spectrogram(torch.from_numpy(x).cuda(), n_fft, hop, win,
                                 valid_samples=torch.from_numpy(valid).cuda())
    T = spec.shape[-1]
    frames = np.array([SR.frames(int(v), n_fft, hop) for v in valid], np.int64)
    assert np.array_equal(lens.cpu().numpy(), frames)
    ref_spec = np.zeros((2, n_fft // 2 + 1, T))
    for b in range(2):
        ref_spec[b, :, :frames[b]] = SR.spectrogram(x[b, :valid[b]], n_fft, hop, win)
    src, tgt = np.array([3, 7]), np.array([0, 11])
    noise = rs.standard_normal((2, net.cfg.inter_channels, T)).astype(np.float32)
    ref = R.voice_conversion(sd, net.cfg, ref_spec.astype(np.float32), frames, src, tgt, noise=noise)
    real, fake = _pinned_randn(torch.from_numpy(noise).cuda())
    torch.randn = fake
    try:
        o, o_mb, y_mask, (z, z_p, z_hat) = net.voice_conversion(spec, lens, torch.from_numpy(src).cuda(),
                                                                torch.from_numpy(tgt).cuda())
    finally:
        torch.randn = real
    assert np.array_equal(y_mask.cpu().numpy(), ref["y_mask"].numpy())
    zr = ref["z_hat"].numpy()
    zrel = rms(z_hat.cpu().numpy() - zr) / max(rms(zr), 1e-3)
    oerr = rms(o.cpu().numpy() - ref["o"].numpy())
    print("z_hat rel %.2e, o rms %.2e" % (zrel, oerr))
    assert zrel < 5e-5
    assert oerr < 1e-4


@pytest.mark.parametrize("in_sr,pcm", [(16000, True), (22050, False), (22050, True)])
def test_convert_pcm16_is_the_composition(in_sr, pcm):
    from gpu_util import make_net
    from mb_istft_vits_amd import wire
    net, _ = make_net("uudb_ms_istft_vits_ms")
    model_sr, rate, hop, win = 16000, 24000, 256, 1024
    rs = np.random.RandomState(in_sr + pcm)
    n = int(0.9 * in_sr)
    x = _vc_audio(rs, 3, n, in_sr)
    valid = torch.tensor([n, n // 2, n - 777], device="cuda")
    wave = torch.from_numpy((x * 32767).astype(np.int16) if pcm else x).cuda()
    src, tgt = torch.tensor([1, 5, 9], device="cuda"), torch.tensor([2, 2, 0], device="cuda")
    # the composition, step by step
    w = wave.float() / 32768.0 if (pcm and in_sr != model_sr) else wave
    w, v = net.resample(w.unsqueeze(1), in_sr, model_sr, valid_samples=valid)
    spec, lens = net.spectrogram(w, 1024, hop, win, valid_samples=v)
    noise = torch.randn(3, net.cfg.inter_channels, spec.shape[-1], device="cuda")
    real, fake = _pinned_randn(noise)
    torch.randn = fake
    try:
        o = net.voice_conversion(spec, lens, src, tgt)[0]
        want, want_v = wire.service_pcm16(net, o, lens, model_sr, rate)
        got, got_v = wire.convert_pcm16(net, wave, valid, src, tgt, in_sr, model_sr, rate, hop, win)
    finally:
        torch.randn = real
    assert got.dtype == torch.int16 and torch.equal(got, want) and torch.equal(got_v, want_v)
    assert int(got_v.min()) > 0


def test_spectrogram_errors_leave_the_handle_serving(net):
    import ctypes as C
    from mb_istft_vits_amd import _capi, wire
    from gpu_util import make_net
    x = torch.rand(2, 5000, device="cuda")
    ref, _ = net.spectrogram(x, 1024, 256, 1024)
    with pytest.raises(ValueError, match="center"):
        net.spectrogram(x, 1024, 256, 1024, center=True)
    with pytest.raises(ValueError, match="power of two"):
        net.spectrogram(x, 1000, 256, 1000)
    with pytest.raises(ValueError, match="win_size"):
        net.spectrogram(x, 1024, 256, 1025)
    with pytest.raises(ValueError, match="hop_size"):
        net.spectrogram(x, 1024, 0, 1024)
    with pytest.raises(ValueError, match="float32 or int16"):
        net.spectrogram(x.double(), 1024, 256, 1024)
    # the C entry refuses the same arguments itself, with a message, and keeps serving
    h, L = net._ensure_handle(), _capi.lib()
    out = torch.empty_like(ref)
    for n_fft, hop, win, what in [(1000, 256, 1000, b"power of two"), (1024, 0, 1024, b"hop"),
                                  (1024, 256, 2048, b"win"), (8192, 256, 1024, b"power of two")]:
        rc = L.mbv_spectrogram(h, C.c_void_p(x.data_ptr()), 0, None, 2, 5000, n_fft, hop, win,
                               C.c_void_p(out.data_ptr()), ref.shape[-1], None, net._stream())
        assert rc != 0 and what in L.mbv_last_error(h), L.mbv_last_error(h)
    rc = L.mbv_spectrogram(h, C.c_void_p(x.data_ptr()), 0, None, 2, 5000, 1024, 256, 1024,
                           C.c_void_p(out.data_ptr()), ref.shape[-1] + 1, None, net._stream())
    assert rc != 0 and b"frames" in L.mbv_last_error(h)
    # empty inputs: no launch
    e, le = net.spectrogram(torch.zeros(0, 5000, device="cuda"), 1024, 256, 1024)
    assert e.shape == (0, 513, ref.shape[-1]) and le.shape == (0,)
    e, le = net.spectrogram(torch.zeros(2, 0, device="cuda"), 1024, 256, 1024)
    assert e.shape == (2, 513, 0) and not le.any()
    vc, _ = make_net("uudb_ms_istft_vits_ms")
    with pytest.raises(ValueError, match="win_size"):
        wire.convert_pcm16(vc, x, None, torch.tensor([0, 1]).cuda(), torch.tensor([1, 0]).cuda(), 16000, 16000,
                           16000, 256, 1025)
    with pytest.raises(ValueError, match="speakers"):
        wire.convert_pcm16(net, x, None, torch.tensor([0, 1]).cuda(), torch.tensor([1, 0]).cuda(), 16000, 16000,
                           16000, 256, 1024)
    again, _ = net.spectrogram(x, 1024, 256, 1024)
    assert torch.equal(again, ref)
    pcm, v = wire.convert_pcm16(vc, x, None, torch.tensor([0, 1]).cuda(), torch.tensor([1, 0]).cuda(), 16000,
                                16000, 16000, 256, 1024)
    assert pcm.shape[0] == 2 and int(v.min()) > 0
