"""-m gpu: kernel-level parity through the C-ABI.
fp32 tolerances: conv sums of <= 8448 products -> 2e-5 relative to the output RMS;
iSTFT+PQMF -> 2e-5 absolute on O(1) signals (north-star bar on the waveform is 1e-4 RMS)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import load_fixture, rms
from oracle import ref_infer as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def net():
    from gpu_util import make_net
    return make_net("ljs_mini_mb_istft_vits")[0]


CONV_CASES = [
    # B, Cin, Cout, T, K, dil, slope
    (2, 32, 64, 50, 1, 1, 1.0),
    (2, 96, 192, 200, 1, 1, 1.0),
    (3, 192, 576, 131, 1, 1, 1.0),
    (2, 192, 768, 200, 3, 1, 1.0),
    (2, 768, 192, 77, 3, 1, 1.0),
    (2, 192, 384, 300, 5, 1, 1.0),
    (2, 192, 512, 129, 7, 1, 1.0),
    (2, 128, 128, 1000, 3, 5, 0.1),
    (2, 128, 128, 517, 7, 3, 0.1),
    (1, 128, 128, 1300, 11, 5, 0.1),
    (2, 256, 256, 260, 11, 1, 0.1),
    (2, 128, 72, 400, 7, 1, 0.01),
    (2, 192, 96, 90, 1, 1, 1.0),
    (1, 64, 64, 5, 3, 1, 0.1),
]


@pytest.mark.parametrize("B,Cin,Cout,T,K,dil,slope", CONV_CASES)
def test_conv1d_mfma(net, B, Cin, Cout, T, K, dil, slope):
    from gpu_util import op_conv1d
    rs = np.random.RandomState(B * 1000 + Cin + Cout + T + K)
    x = rs.standard_normal((B, Cin, T)).astype(np.float32)
    w = (rs.standard_normal((Cout, Cin, K)) / np.sqrt(Cin * K)).astype(np.float32)
    b = rs.standard_normal(Cout).astype(np.float32)
    y = op_conv1d(net, torch.from_numpy(x).cuda(), w, b, K, dil, slope).cpu()
    xt = torch.from_numpy(x)
    ref = F.conv1d(F.leaky_relu(xt, slope) if slope != 1.0 else xt, torch.from_numpy(w),
                   torch.from_numpy(b), padding=(K - 1) * dil // 2, dilation=dil)
    err = rms((y - ref).numpy())
    assert err <= 2e-5 * rms(ref.numpy()) + 1e-7, err


@pytest.mark.parametrize("B,Cin,Cout,T,K,dil", [(64, 128, 128, 3072, 7, 3), (64, 128, 128, 3100, 11, 5), (64, 256, 256, 1536, 3, 1),
                                               (64, 128, 128, 3072, 3, 5), (64, 128, 72, 3001, 7, 1),
                                               (3, 128, 128, 1001, 7, 5), (2, 256, 256, 517, 11, 1), (5, 192, 512, 300, 7, 1),
                                               (2, 128, 96, 333, 3, 3)])
def test_conv1d_split_bf16_mode(B, Cin, Cout, T, K, dil):
    """Opt-in `conv_bf16 = 3` (hi/mid bf16 planes, three products, fp32 accumulation on the bf16 MFMA) in the
    128-row conv kernels — launches large enough for the 128 x 384 shape (>= 512 tiles) and small ones on the
    128 x 128 shape (incl. a half-height last row tile) — against torch's fp32 conv on the GPU.  Bar for this mode: 3e-5 of the output RMS per conv (measured ~5e-6; the exact path's
    bar is 2e-5 with ~3e-7 measured) — and the mode must actually be taken (the result differs from the
    exact path's) and must leave the default untouched."""
    from gpu_util import make_net, op_conv1d
    net = make_net("ljs_mini_mb_istft_vits")[0]
    g = torch.Generator(device="cuda").manual_seed(Cin + T + K)
    x = torch.randn(B, Cin, T, device="cuda", generator=g)
    rs = np.random.RandomState(K * 100 + dil)
    w = (rs.standard_normal((Cout, Cin, K)) / np.sqrt(Cin * K)).astype(np.float32)
    b = rs.standard_normal(Cout).astype(np.float32)
    ref = F.conv1d(F.leaky_relu(x, 0.1), torch.from_numpy(w).cuda(), torch.from_numpy(b).cuda(),
                   padding=(K - 1) * dil // 2, dilation=dil)
    scale = float(ref.pow(2).mean().sqrt())
    exact = op_conv1d(net, x, w, b, K, dil, 0.1)
    net.set_option("conv_bf16", 3)
    try:
        split = op_conv1d(net, x, w, b, K, dil, 0.1)
        split2 = op_conv1d(net, x, w, b, K, dil, 0.1)
    finally:
        net.set_option("conv_bf16", 0)
    again = op_conv1d(net, x, w, b, K, dil, 0.1)
    e_exact = float((exact - ref).pow(2).mean().sqrt()) / scale
    e_split = float((split - ref).pow(2).mean().sqrt()) / scale
    assert e_exact < 2e-5 and e_split < 3e-5, (e_exact, e_split)
    assert torch.equal(split, split2) and torch.equal(exact, again)
    low_latency = os.environ.get("MBV_CONV_SPLITK", "0") not in ("", "0")
    if B == 64 or not low_latency:         # (the low-latency mode sends small launches to the narrow kernel, which is always exact)
        assert not torch.equal(split, exact)


def test_istft_pqmf_known_answers(net):
    """Stand-alone kernel vs the reference's TorchSTFT.inverse / PQMF.synthesis vectors:
    x_post is built so that exp()/pi*sin() reproduce the stored mag/phase."""
    from gpu_util import op_istft_pqmf
    rs = np.random.RandomState(5)
    B, Tp = 3, 7
    Fr = 16 * Tp + 1
    x_post = (rs.standard_normal((B, 72, Fr)) * 0.7).astype(np.float32)
    xt = torch.from_numpy(x_post)
    W = R.Weights({})

    class Cfg:
        subbands, gen_istft_n_fft, gen_istft_hop_size = 4, 16, 4
    o_ref, omb_ref, spec_ref, phase_ref = R.waveform_tail(W, Cfg, xt)
    o, o_mb, spec, phase = op_istft_pqmf(net, xt.cuda())
    assert np.abs(spec.cpu().numpy() - spec_ref.numpy()).max() < 1e-5 * float(spec_ref.max())
    assert np.abs(phase.cpu().numpy() - phase_ref.numpy()).max() < 5e-6
    assert np.abs(o_mb.cpu().numpy() - omb_ref.numpy()).max() < 2e-5
    assert np.abs(o.cpu().numpy() - o_ref.numpy()).max() < 2e-5
    # waveform-only mode gives the same samples
    o2, _, _, _ = op_istft_pqmf(net, xt.cuda(), extras=False)
    assert torch.equal(o2, o)


@pytest.mark.parametrize("Tp", [1, 2, 29, 30, 31, 61])
def test_istft_pqmf_tile_edges(net, Tp):
    """Tile size is 480 sub-band samples = 7.5 z-frames: lengths around tile boundaries."""
    from gpu_util import op_istft_pqmf
    rs = np.random.RandomState(Tp)
    x_post = (rs.standard_normal((2, 72, 16 * Tp + 1)) * 0.7).astype(np.float32)
    xt = torch.from_numpy(x_post)

    class Cfg:
        subbands, gen_istft_n_fft, gen_istft_hop_size = 4, 16, 4
    o_ref, omb_ref, _, _ = R.waveform_tail(R.Weights({}), Cfg, xt)
    o, o_mb, _, _ = op_istft_pqmf(net, xt.cuda())
    assert np.abs(o_mb.cpu().numpy() - omb_ref.numpy()).max() < 2e-5
    assert np.abs(o.cpu().numpy() - o_ref.numpy()).max() < 2e-5


def test_istft_pqmf_multistream_filter(net):
    from gpu_util import op_istft_pqmf
    rs = np.random.RandomState(11)
    x_post = (rs.standard_normal((2, 72, 16 * 9 + 1)) * 0.7).astype(np.float32)
    h = (rs.standard_normal((4, 63)) * 0.1).astype(np.float32)
    xt = torch.from_numpy(x_post)
    sd = {"dec.multistream_conv_post.weight_v": torch.from_numpy(h)[None],
          "dec.multistream_conv_post.weight_g": torch.from_numpy(h).norm().reshape(1, 1, 1)}

    class Cfg:
        subbands, gen_istft_n_fft, gen_istft_hop_size = 4, 16, 4
    o_ref, up_ref, _, _ = R.waveform_tail(R.Weights(sd), Cfg, xt)
    o, o_mb, _, _ = op_istft_pqmf(net, xt.cuda(), filt=torch.from_numpy(h).cuda(), multistream=True)
    assert np.abs(o_mb.cpu().numpy() - up_ref.numpy()).max() < 5e-5
    assert np.abs(o.cpu().numpy() - o_ref.numpy()).max() < 2e-5


def test_istft_fast_vs_exact_transcendentals():
    """The default kernel uses v_exp/v_sin/v_cos; MBV_ISTFT_EXACT=1 selects libm.  Both must sit
    well inside the 1e-4 RMS bar; this pins how far apart they are on O(1) signals with
    phase pre-activations up to |x| ~ 12 (range reduction)."""
    import os
    from gpu_util import make_net, op_istft_pqmf
    rs = np.random.RandomState(17)
    x_post = (rs.standard_normal((4, 72, 16 * 40 + 1))).astype(np.float32)
    x_post[:, 9::18] *= 4.0                      # large phase arguments on one bin per band
    xt = torch.from_numpy(x_post).cuda()
    os.environ["MBV_ISTFT_EXACT"] = "1"
    try:
        net_exact = make_net("ljs_mini_mb_istft_vits")[0]
        o_exact = op_istft_pqmf(net_exact, xt)[0].cpu().numpy()
    finally:
        os.environ.pop("MBV_ISTFT_EXACT")
    net_fast = make_net("ljs_mini_mb_istft_vits")[0]
    o_fast = op_istft_pqmf(net_fast, xt)[0].cpu().numpy()

    class Cfg:
        subbands, gen_istft_n_fft, gen_istft_hop_size = 4, 16, 4
    o_ref = R.waveform_tail(R.Weights({}), Cfg, torch.from_numpy(x_post))[0].numpy()
    e_exact, e_fast = rms(o_exact - o_ref), rms(o_fast - o_ref)
    print("istft rms err vs oracle: exact %.2e fast %.2e (signal rms %.2f)" % (e_exact, e_fast, rms(o_ref)))
    assert e_exact < 2e-5 * max(1.0, rms(o_ref))
    assert e_fast < 2e-5 * max(1.0, rms(o_ref))


def test_pcm16_epilogue_bit_exact(net):
    """float -> int16 wire format (tts_vits.py:204-217): bit-exact against the NumPy restatement,
    per utterance over its valid samples; quiet utterances (peak <= 0.01) are not normalised."""
    rs = np.random.RandomState(2)
    B, frames = 5, 9
    n = 256 * frames
    wave = (rs.standard_normal((B, 1, n)) * 0.4).astype(np.float32)
    wave[1] *= 5.0                 # clips without normalisation
    wave[2] *= 0.01                # peak below the 0.01 threshold -> left alone
    ylen = np.array([9, 4, 9, 1, 7], np.int64)
    for auto in (True, False):
        pcm = net.to_pcm16(torch.from_numpy(wave).cuda(), torch.from_numpy(ylen).cuda(), auto_normalize=auto).cpu().numpy()
        assert pcm.dtype == np.int16 and pcm.shape == (B, n)
        for b in range(B):
            v = 256 * ylen[b]
            assert np.array_equal(pcm[b, :v], R.to_pcm16(wave[b, 0, :v], auto)), (auto, b)
            assert not pcm[b, v:].any()
    full = net.to_pcm16(torch.from_numpy(wave).cuda()).cpu().numpy()
    assert np.array_equal(full[0], R.to_pcm16(wave[0, 0]))


def test_pcm16_after_max_len_truncation(net):
    """infer(max_len=k) returns rows of 256*k samples while y_lengths keeps the untruncated frame
    counts (models.py:733-734): `to_pcm16(o, y_lengths)` must clamp each utterance to its row — the
    peak of row b must not see row b+1, and the last row must not be read past its end."""
    from mb_istft_vits_amd import synth
    x, xl, _ = synth.synthetic_batch(net.cfg, 3, 20, seed=17, ragged=True)
    (o, *_), ylen = net.infer_with_lengths(torch.from_numpy(x).cuda(), torch.from_numpy(xl).cuda(),
                                           noise_scale=0, length_scale=1, max_len=12)
    assert o.shape[-1] == 256 * 12 and int(ylen.max()) > 12
    # make the rows' peaks very different, so a peak leaking across rows would change the scaling
    scale = torch.tensor([1.0, 0.05, 3.0], device=o.device).view(3, 1, 1)
    wave = (o * scale).contiguous()
    pcm = net.to_pcm16(wave, ylen).cpu().numpy()
    w = wave.cpu().numpy()
    for b in range(3):
        v = min(256 * int(ylen[b]), w.shape[-1])
        assert np.array_equal(pcm[b, :v], R.to_pcm16(w[b, 0, :v], True)), b
        assert not pcm[b, v:].any()
    # negative lengths count as empty
    neg = net.to_pcm16(wave, torch.tensor([-3, 2, 0], device=o.device)).cpu().numpy()
    assert not neg[0].any() and not neg[2].any()
    assert np.array_equal(neg[1, :512], R.to_pcm16(w[1, 0, :512], True))


def test_c_abi_error_paths(net):
    """Misuse of the C ABI returns an error code + message (no crash, no exception across the ABI)."""
    import ctypes as C
    from mb_istft_vits_amd import _capi
    L = _capi.lib()
    c = _capi.MbvConfig()
    c.struct_bytes = C.sizeof(_capi.MbvConfig)
    c.n_vocab, c.inter_channels, c.hidden_channels, c.filter_channels = 59, 192, 96, 768
    c.n_heads, c.n_layers, c.kernel_size, c.upsample_initial_channel = 2, 3, 3, 256
    c.spec_channels = 513
    for j, k in enumerate((3, 7, 11)):
        c.resblock_kernel_sizes[j] = k
        for q, d in enumerate((1, 3, 5)):
            c.resblock_dilations[j][q] = d
    c.resblock_type, c.decoder, c.device = 1, 0, 0
    h = C.c_void_p()
    assert L.mbv_create(C.byref(c), C.byref(h)) == 0
    try:
        # phase B without phase A / without weights
        out = _capi.MbvOutputs()
        assert L.mbv_synthesize(h, 10, None, 0.0, 0, C.byref(out), None) != 0
        assert b"mbv_encode" in L.mbv_last_error(h)
        ids = torch.zeros(1, 4, dtype=torch.int64, device="cuda")
        lens = torch.tensor([4], device="cuda")
        yl = torch.zeros(1, dtype=torch.int64, device="cuda")
        assert L.mbv_encode(h, C.c_void_p(ids.data_ptr()), C.c_void_p(lens.data_ptr()), None, 1, 4,
                            C.c_float(1.0), None, C.c_float(1.0), C.c_void_p(yl.data_ptr()), None) != 0
        assert b"finalize" in L.mbv_last_error(h)
        assert L.mbv_finalize_weights(h, None) != 0 and b"missing weight" in L.mbv_last_error(h)
        n_missing = L.mbv_missing_weights(h, None, 0)
        assert n_missing > 100
        # wrong shape and training-only key
        w = np.zeros((59, 95), np.float32)
        shp = (C.c_int64 * 2)(59, 95)
        assert L.mbv_load_weight(h, b"enc_p.emb.weight", w.ctypes.data_as(C.c_void_p), shp, 2) != 0
        assert b"shape mismatch" in L.mbv_last_error(h)
        assert L.mbv_load_weight(h, b"net_d.conv.weight", w.ctypes.data_as(C.c_void_p), shp, 2) != 0
        assert b"not a weight of the infer path" in L.mbv_last_error(h)
        shp = (C.c_int64 * 2)(59, 96)
        w = np.zeros((59, 96), np.float32)
        assert L.mbv_load_weight(h, b"enc_p.emb.weight", w.ctypes.data_as(C.c_void_p), shp, 2) == 0
        assert L.mbv_missing_weights(h, None, 0) == n_missing - 1
    finally:
        L.mbv_destroy(h)
    with pytest.raises(ValueError):
        net.istft_finalize(torch.zeros(1, 4, 9, 18, device="cuda"), torch.zeros(1, 4, 9, 17, device="cuda"))
    with pytest.raises(_capi.MbvError, match="16 n \\+ 1"):
        net.istft_finalize(torch.zeros(1, 4, 9, 18, device="cuda"), torch.zeros(1, 4, 9, 18, device="cuda"))


def test_c_abi_positive_path_with_raw_ctypes():
    """The path through the C ABI alone — what a maintainer binding `include/mbistft_vits.h` from the
    reference's own `models.py` would write: create, load every state-dict key,
    finalize, encode, read max(y_lengths), synthesize — against the `mini_b1` golden from the
    reference.  No `mb_istft_vits_amd.models` involved; torch only allocates the buffers."""
    import ctypes as C
    from helpers import load_fixture, config_for, rms
    from mb_istft_vits_amd import _capi, synth
    gold = load_fixture("mini_b1")
    _, cfg = config_for("ljs_mini_mb_istft_vits", int(gold["n_vocab"]))
    L = _capi.lib()
    c = _capi.MbvConfig()
    c.struct_bytes = C.sizeof(_capi.MbvConfig)
    c.n_vocab, c.inter_channels, c.hidden_channels = cfg.n_vocab, cfg.inter_channels, cfg.hidden_channels
    c.filter_channels, c.n_heads, c.n_layers = cfg.filter_channels, cfg.n_heads, cfg.n_layers
    c.kernel_size, c.upsample_initial_channel, c.spec_channels = cfg.kernel_size, cfg.upsample_initial_channel, cfg.spec_channels
    for j in range(3):
        c.resblock_kernel_sizes[j] = cfg.resblock_kernel_sizes[j]
        for q, d in enumerate(cfg.resblock_dilation_sizes[j]):
            c.resblock_dilations[j][q] = d
    c.resblock_type, c.n_speakers, c.gin_channels, c.decoder, c.device, c.use_sdp = 1, 0, 0, 0, 0, 0
    h = C.c_void_p()
    assert L.mbv_create(C.byref(c), C.byref(h)) == 0, L.mbv_last_error(None)
    try:
        for k, v in synth.make_state_dict(cfg, int(gold["weight_seed"])).items():
            a = np.ascontiguousarray(v, np.float32)
            assert L.mbv_load_weight(h, k.encode(), a.ctypes.data_as(C.c_void_p),
                                     (C.c_int64 * a.ndim)(*a.shape), a.ndim) == 0, L.mbv_last_error(h)
        assert L.mbv_missing_weights(h, None, 0) == 0
        assert L.mbv_finalize_weights(h, None) == 0, L.mbv_last_error(h)
        x = torch.from_numpy(gold["x"]).cuda()
        xl = torch.from_numpy(gold["x_lengths"]).cuda()
        B, T = x.shape
        ylen = torch.empty(B, dtype=torch.int64, device="cuda")
        p = lambda t: C.c_void_p(t.data_ptr())
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        assert L.mbv_encode(h, p(x), p(xl), None, B, T, C.c_float(1.0), None, C.c_float(1.0), p(ylen), st) == 0
        Tp = int(ylen.max())                                   # the one host sync of the path
        o = torch.empty(B, 1, 256 * Tp, device="cuda")
        z = torch.empty(B, cfg.inter_channels, Tp, device="cuda")
        out = _capi.MbvOutputs()
        out.o, out.z = o.data_ptr(), z.data_ptr()              # every other output skipped (NULL)
        assert L.mbv_synthesize(h, Tp, None, C.c_float(0.0), 0, C.byref(out), st) == 0, L.mbv_last_error(h)
        torch.cuda.synchronize()
        assert np.array_equal(ylen.cpu().numpy(), gold["y_mask"].sum((1, 2)).astype(np.int64))
        assert rms(o.cpu().numpy() - gold["o"]) < 1e-4
        assert rms(z.cpu().numpy() - gold["z"]) <= 5e-5 * rms(gold["z"])
        t5 = (C.c_float * 5)()
        assert L.mbv_stage_times_ms(h, C.byref(t5)) == 0 and all(v >= 0 for v in t5)
    finally:
        L.mbv_destroy(h)


def test_reference_side_binding_runs_against_golden():
    """INTEGRATION.md §B as code: `reference_binding.bind(RefClass)` puts the C ABI under a class that
    has the REFERENCE's constructor attributes and state-dict keys (here a parameter-only stand-in
    built from the key table — the reference's own models.py does not travel to the GPU box) and
    must reproduce the reference's `mini_b1` / `uudb_b2` goldens."""
    from helpers import load_fixture, config_for, rms, FIXTURES, ref_stand_in
    from mb_istft_vits_amd import synth
    from mb_istft_vits_amd.reference_binding import bind

    Bound = bind(ref_stand_in())
    for fx in ("mini_b1", "uudb_b2"):
        gold = load_fixture(fx)
        hps, cfg = config_for(FIXTURES[fx], int(gold["n_vocab"]))
        net = Bound(cfg, dict(hps.model), hps.data.n_speakers)
        sd = synth.make_state_dict(cfg, int(gold["weight_seed"]))
        net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})      # strict: every reference key
        net = net.cuda().eval()
        sid = torch.from_numpy(gold["sid"]).cuda() if "sid" in gold else None
        o, o_mb, spec, phase, attn, y_mask, (z, z_p, m_p, logs_p), timings = net.infer(
            torch.from_numpy(gold["x"]).cuda(), torch.from_numpy(gold["x_lengths"]).cuda(), sid=sid,
            noise_scale=0, length_scale=1)
        assert np.array_equal(attn.sum(2).cpu().numpy(), gold["attn"]), fx
        assert rms(o.cpu().numpy() - gold["o"]) < 1e-4, fx
        assert rms(z.cpu().numpy() - gold["z"]) <= 5e-5 * rms(gold["z"]), fx
        assert set(timings) == {"text_encoder", "duration_predictor", "alignment_and_projection", "flow", "waveform_decoder"}
        g = None if sid is None else torch.from_numpy(sd["emb_g.weight"])[gold["sid"]].cuda()
        do = net.decode(z[:, :, :20].contiguous(), g)[0]
        assert do.shape == (z.shape[0], 1, 256 * 20) and torch.isfinite(do).all()
        # `model.dec(z, g=g)` (synthesis_module.py:158-160) is routed to the same entry
        assert torch.equal(net.dec(z[:, :, :20].contiguous(), g=None if g is None else g.unsqueeze(-1))[0], do)
        # infer_z_only (models.py:742-788): same latents, four timings, no decoder launch
        a2, m2, (z2, zp2, mp2, lp2), t2 = net.infer_z_only(
            torch.from_numpy(gold["x"]).cuda(), torch.from_numpy(gold["x_lengths"]).cuda(), sid=sid, noise_scale=0, length_scale=1)
        assert torch.equal(z2, z) and torch.equal(a2, attn) and torch.equal(m2, y_mask) and torch.equal(mp2, m_p)
        assert set(t2) == {"text_encoder", "duration_predictor", "alignment_and_projection", "flow"}
        # max_len (models.py:734 slices the decoder input): clamps; <= 0 leaves nothing and must not reach the library as "no clamp"
        o5 = net.infer(torch.from_numpy(gold["x"]).cuda(), torch.from_numpy(gold["x_lengths"]).cuda(), sid=sid,
                       noise_scale=0, length_scale=1, max_len=5)[0]
        assert o5.shape[-1] == 256 * 5
        for bad in (0, -3):
            with pytest.raises(ValueError):
                net.infer(torch.from_numpy(gold["x"]).cuda(), torch.from_numpy(gold["x_lengths"]).cuda(), sid=sid,
                          noise_scale=0, length_scale=1, max_len=bad)
    # voice_conversion (models.py:790-798) through the binding, against the reference's golden
    gold = load_fixture("vc_uudb_b2")
    hps, cfg = config_for("uudb_ms_istft_vits_ms", int(gold["n_vocab"]))
    net = Bound(cfg, dict(hps.model), hps.data.n_speakers)
    sd = synth.make_state_dict(cfg, int(gold["weight_seed"]))
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    net = net.cuda().eval()
    y = torch.from_numpy(gold["y"]).cuda()
    noise, real = torch.from_numpy(gold["noise"]).cuda(), torch.randn      # the posterior encoder's draw, pinned to the golden's
    torch.randn = lambda *a, **k: noise if tuple(a) == tuple(noise.shape) else real(*a, **k)
    try:
        o_hat, o_hat_mb, y_mask, (z, z_p, z_hat) = net.voice_conversion(
            y, torch.from_numpy(gold["y_lengths"]).cuda(), torch.from_numpy(gold["sid_src"]).cuda(), torch.from_numpy(gold["sid_tgt"]).cuda())
    finally:
        torch.randn = real
    assert np.array_equal(y_mask.cpu().numpy(), gold["y_mask"])
    assert rms(o_hat.cpu().numpy() - gold["o"]) < 1e-4
    assert rms(z_hat.cpu().numpy() - gold["z_hat"]) <= 5e-5 * rms(gold["z_hat"])
    with pytest.raises(IndexError):
        net.voice_conversion(y, torch.from_numpy(gold["y_lengths"]).cuda(), torch.tensor([3, 12]).cuda(), torch.tensor([0, 1]).cuda())
    # both flags set: the reference's order (models.py:634-644) builds the multiband decoder
    both = Bound(cfg, dict(hps.model, mb_istft_vits=True, ms_istft_vits=True), hps.data.n_speakers)
    assert both.mb_istft_vits and both.ms_istft_vits


@pytest.mark.timeout(600)
def test_fused_wn_layer_kernel_against_cpu_loop(tmp_path):
    """`wn_layer_kernel` (wn_fused.hip) on its own against a plain CPU loop in float64
    (`scripts/wn_layer_check.hip` includes the kernel source and is compiled here with hipcc):
    ragged lengths, tiles that span two utterances, the last layer's 6-tile res/skip GEMM (idle tile
    slots must not store into the next utterance), 64 / 96 / 160 / 192 channels.

    This is ONE plain layer: `gcond` is null, `skip_accum` is 1, `Cs` is H, and `wpre` / `Gi` / `in_cb` (the first
    layer of a coupling reading x0' = [x0 ; mask] through the composed weights), `x1` / `x1_bstride` / `couple_sign`
    (the last layer applying the coupling through the res/skip conv with `post` folded in, Cs = I / 2) are never set.
    Those arguments of `WnLayerArgs`, the Flip folded into the packing, both signs and the two-launch layer are reached
    by test_gpu_wn_stack.py through `align`, `infer_z_only` and `voice_conversion`."""
    import shutil
    import subprocess
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available on this box")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(str(tmp_path), "wn_layer_check")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O2", "-std=c++17", "-I" + os.path.join(root, "mb-istft-vits_amd", "csrc"),
                        os.path.join(root, "scripts", "wn_layer_check.hip"), "-o", exe], capture_output=True, text=True, timeout=400)
    assert r.returncode == 0, r.stderr[-3000:]
    for args in (["3", "96", "45", "0", "45", "41", "15"], ["2", "96", "48", "0", "48", "48"], ["5", "192", "70", "1"],
                 ["5", "192", "70", "0"], ["3", "64", "33", "0"], ["4", "160", "50", "1"], ["2", "96", "74", "0", "61", "74"]):
        r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stdout.strip().endswith("OK"), (args, r.stdout[-1500:], r.stderr[-500:])


def test_rel_attention_kernel_against_the_oracle_op():
    """`rel_attention_kernel` on its own (the attention was only covered through x_enc and the durations):
    random q | k | v and relative embeddings, ragged lengths incl. a 1-token and a full-length utterance, T across the
    32-key tile boundaries, head dimensions 96, 48, 40 and 32 — against the oracle's `relative_attention` (attentions.py:148-243
    restated: -1e4 mask fill, window of +-4, q scaled before both the content and the relative logits)."""
    import ctypes as C
    from gpu_util import make_net, ptr
    from mb_istft_vits_amd import _capi
    from oracle import ref_infer as R
    net = make_net("ljs_mini_mb_istft_vits")[0]
    h = net._ensure_handle()
    g = torch.Generator().manual_seed(7)
    # (r03: + head dimensions 32 and 40 — a head that ends inside a 32-row tile exercises the `kk < d` / `dd < d` guards of the
    # LDS-staged relative-key image and of the relative-value contraction)
    for (B, H, heads, T) in ((3, 192, 2, 200), (2, 96, 2, 33), (4, 192, 2, 64), (1, 192, 2, 1), (2, 192, 2, 257),
                             (2, 64, 2, 70), (3, 80, 2, 45)):
        d = H // heads
        qkv = torch.randn(B, 3 * H, T, generator=g)
        ek, ev = torch.randn(9, d, generator=g) * 0.3, torch.randn(9, d, generator=g) * 0.3
        lens = torch.randint(1, T + 1, (B,), generator=g)
        lens[0] = T
        if B > 1:
            lens[1] = 1
        o = torch.empty(B, H, T, device="cuda")
        dq, dk, dv, dl = qkv.cuda(), ek.cuda(), ev.cuda(), lens.cuda()        # (kept alive across the call)
        rc = _capi.lib().mbv_op_rel_attention(h, ptr(dq), ptr(dk), ptr(dv), ptr(dl), ptr(o), B, H, heads, T, net._stream())
        _capi.check(h, rc, "mbv_op_rel_attention")
        mask = (torch.arange(T)[None, :] < lens[:, None]).float()
        want = R.relative_attention(qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:], mask, ek, ev, heads)
        got = o.cpu()
        for b in range(B):                       # valid queries only (the encoder masks the rest right behind the attention)
            n = int(lens[b])
            err = float((got[b, :, :n] - want[b, :, :n]).abs().max())
            ref = float(want[b, :, :n].abs().max())
            assert err <= 2e-5 * max(ref, 1.0), (B, H, T, b, err, ref)
