"""-m gpu: the whole `SynthesizerTrn.infer` path on the MI355X vs (a) the golden
vectors captured from the real reference and (b) the oracle on fresh inputs.
Bar (north-star): waveform within 1e-4 RMS of the reference CPU path at
noise_scale=0, length_scale=1; durations (ceil) exact."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from helpers import FIXTURES, OVERRIDES, SDP_NOISE_SCALE_W, load_fixture, config_for, thin, rms
from oracle import ref_infer as R

pytestmark = pytest.mark.gpu

# MBV_CONV_SPLITK=1 (opt-in low-latency mode): the summation order of small launches depends on the
# launch size, so "same row, different batch" is equal within rounding instead of bitwise
SPLITK = os.environ.get("MBV_CONV_SPLITK", "0") not in ("", "0")


def _same_rows(a, b):
    if not SPLITK:
        return torch.equal(a, b)
    return float((a - b).abs().max()) <= 2e-5 * max(float(b.abs().max()), 1e-3)

STAGE_SHAPES = {  # read_stage name -> golden key, shape builder
    "x_enc": "x_enc", "m_text": "m_text", "logs_text": "logs_text", "logw": "logw",
    "dec_conv_pre": "dec_conv_pre", "dec_up_0": "dec_up_0", "dec_res_0": "dec_res_0",
    "dec_up_1": "dec_up_1", "dec_res_1": "dec_res_1", "x_post": "x_post",
}


def _rel(got, ref):
    return rms(np.asarray(got) - np.asarray(ref)) / max(rms(ref), 1e-3)


@pytest.mark.parametrize("fixture", list(FIXTURES))
def test_infer_matches_reference_golden(fixture):
    from gpu_util import make_net
    gold = load_fixture(fixture)
    net, sd = make_net(FIXTURES[fixture], int(gold["n_vocab"]), int(gold["weight_seed"]),
                       overrides=OVERRIDES.get(fixture))
    x = torch.from_numpy(gold["x"]).cuda()
    xl = torch.from_numpy(gold["x_lengths"]).cuda()
    sid = torch.from_numpy(gold["sid"]).cuda() if "sid" in gold else None
    if net.use_sdp:
        # like the reference, the shim draws the SDP noise from torch's default CPU generator
        # (models.py:94): the seed the fixture was captured with reproduces it
        torch.manual_seed(4321 + int(gold["weight_seed"]))
    o, o_mb, spec, phase, attn, y_mask, (z, z_p, m_p, logs_p), timings = net.infer(
        x, xl, sid=sid, noise_scale=0, length_scale=1, noise_scale_w=SDP_NOISE_SCALE_W)
    B, T = gold["x"].shape
    Tp = z.shape[-1]
    report = {}
    # durations must be exact (ceil discontinuity)
    assert np.array_equal(attn.sum(2).cpu().numpy(), gold["attn"]), "durations differ"
    assert np.array_equal(y_mask.cpu().numpy(), gold["y_mask"])
    u = net.cfg.upsample_rates[0]                   # 4 (mb / ms) or 8 (single band)
    shapes = {"x_enc": (B, -1, T), "m_text": (B, -1, T), "logs_text": (B, -1, T), "logw": (B, 1, T),
              "dec_conv_pre": (B, -1, Tp), "dec_up_0": (B, -1, u * Tp), "dec_res_0": (B, -1, u * Tp),
              "dec_up_1": (B, -1, u * u * Tp), "dec_res_1": (B, -1, u * u * Tp),
              "x_post": (B, net.cfg.post_channels, u * u * Tp + 1)}
    if net.use_sdp:                                 # z after flows 7, 5, 3 (ConvFlow.reverse outputs)
        shapes["sdp_z"] = (B, 2, T)
    for name, shp in shapes.items():
        got = thin(name, net.read_stage(name).reshape(*shp).cpu()).numpy()
        report[name] = _rel(got, gold["sdp_flow_3" if name == "sdp_z" else name])
    outs = dict(m_p=m_p, logs_p=logs_p, z_p=z_p, z=z, spec=spec, phase=phase, o_mb=o_mb, o=o)
    if "o_mb" not in gold:                          # iSTFT_Generator: (out, None, spec, phase)
        assert o_mb is None
        del outs["o_mb"]
    for name, t in outs.items():
        got = thin(name, t.cpu()).numpy()
        assert got.shape == gold[name].shape, (name, got.shape, gold[name].shape)
        report[name] = _rel(got, gold[name])
    print(fixture, {k: "%.1e" % v for k, v in report.items()})
    for name, r in report.items():
        assert r < 5e-5, "%s: relative rms error %.3e" % (name, r)
    err = rms(o.cpu().numpy() - gold["o"])
    assert err < 1e-4, "waveform rms error %.3e" % err
    t = dict(timings)
    assert sorted(t) == sorted(["text_encoder", "duration_predictor", "alignment_and_projection",
                                "flow", "waveform_decoder"])
    assert all(v >= 0 for v in t.values())


def test_decoder_entry_matches_oracle():
    """`net.dec(z, g)` (models.py:344-377) on its own, multi-speaker config."""
    from gpu_util import make_net
    net, sd = make_net("uudb_ms_istft_vits_ms")
    rs = np.random.RandomState(3)
    z = rs.standard_normal((2, 192, 37)).astype(np.float32)
    sid = torch.tensor([3, 7])
    g = net.emb_g(sid.cuda()).unsqueeze(-1)
    assert g.shape == (2, 256, 1)
    assert torch.equal(g[:, :, 0].cpu(), torch.from_numpy(sd["emb_g.weight"])[sid])
    o, o_mb, spec, phase = net.dec(torch.from_numpy(z).cuda(), g=g)
    _, cfg = config_for("uudb_ms_istft_vits_ms")
    with torch.no_grad():
        ro, romb, rspec, rphase = R.decode(sd, cfg, torch.from_numpy(z), g.cpu())
    assert rms(o.cpu().numpy() - ro.numpy()) < 1e-4
    assert _rel(o_mb.cpu().numpy(), romb.numpy()) < 5e-5
    assert _rel(spec.cpu().numpy(), rspec.numpy()) < 5e-5


def test_infer_vs_oracle_ragged_batch_with_noise_and_maxlen():
    """Fresh inputs (not in the goldens): ragged batch of 6, noise_scale > 0 with the
    noise tensor shared with the oracle, length_scale != 1, max_len truncation."""
    from gpu_util import make_net
    from mb_istft_vits_amd import synth
    net, sd = make_net("ljs_mb_istft_vits", seed=1235)
    x, xl, _ = synth.synthetic_batch(net.cfg, 6, 40, seed=21, ragged=True)
    torch.manual_seed(0)
    (o, o_mb, spec, phase, attn, y_mask, (z, z_p, m_p, logs_p), _), ylen = net.infer_with_lengths(
        torch.from_numpy(x).cuda(), torch.from_numpy(xl).cuda(), noise_scale=0.5, length_scale=1.1,
        max_len=90)
    # recover the noise the shim drew: z_p = m_p + noise * exp(logs_p) * 0.5
    noise = ((z_p - m_p) / (torch.exp(logs_p) * 0.5)).cpu()
    ref = R.infer(sd, net.cfg, x, xl, None, noise=noise, noise_scale=0.5, length_scale=1.1, max_len=90)
    assert np.array_equal(ylen.cpu().numpy(), ref["y_lengths"].numpy())
    assert o.shape == ref["o"].shape
    assert _rel(z.cpu().numpy(), ref["z"].numpy()) < 5e-5
    assert rms(o.cpu().numpy() - ref["o"].numpy()) < 1e-4


def test_sdp_fresh_ragged_batch_vs_oracle():
    """StochasticDurationPredictor (use_sdp) on inputs outside the goldens: ragged batch of 5 x 60
    tokens, full-size config, noise_scale_w 0.667 (the reference's usual inference value) and the
    zero-noise case; durations exact, logw within 5e-5."""
    from gpu_util import make_net
    from mb_istft_vits_amd import synth
    net, sd = make_net("ljs_mb_istft_vits", seed=1236, overrides={"use_sdp": True})
    for nsw, seed in ((0.667, 31), (0.0, 32)):
        for attempt in range(8):                    # redraw if a duration sits on a ceil() edge
            x, xl, _ = synth.synthetic_batch(net.cfg, 5, 60, seed=seed + 100 * attempt, ragged=True)
            torch.manual_seed(7 + attempt)
            noise_w = torch.randn(5, 2, 60)
            ref = R.infer(sd, net.cfg, x, xl, None, noise_w=noise_w, noise_scale_w=nsw, length_scale=1.0)
            w = (torch.exp(ref["logw"]) * ref["x_mask"]).numpy()[ref["x_mask"].numpy() > 0]
            if np.min(np.abs(w - np.round(w))) > 1e-3:
                break
        torch.manual_seed(7 + attempt)              # the shim draws randn(B, 2, T) first (models.py:94)
        (o, _, _, _, attn, _, (z, _, _, _), _), ylen = net.infer_with_lengths(
            torch.from_numpy(x).cuda(), torch.from_numpy(xl).cuda(), noise_scale=0, length_scale=1.0,
            noise_scale_w=nsw)
        logw = net.read_stage("logw").reshape(5, 1, 60).cpu().numpy()
        assert _rel(logw, ref["logw"].numpy()) < 5e-5
        assert np.array_equal(ylen.cpu().numpy(), ref["y_lengths"].numpy())
        assert np.array_equal(attn.sum(2).cpu().numpy(), ref["attn"].sum(2).numpy())
        assert rms(o.cpu().numpy() - ref["o"].numpy()) < 1e-4


def test_infer_z_only_and_errors():
    from gpu_util import make_net
    net, sd = make_net("ljs_mini_mb_istft_vits")
    x = torch.randint(1, 59, (2, 9)).cuda()
    xl = torch.tensor([9, 5]).cuda()
    attn, y_mask, (z, z_p, m_p, logs_p), timings = net.infer_z_only(x, xl, noise_scale=0)
    full = net.infer(x, xl, noise_scale=0)
    assert torch.equal(z, full[6][0]) and torch.equal(attn, full[4])
    with pytest.raises(ValueError):
        net.infer(x[0], xl)
    with pytest.raises(NotImplementedError):
        net(x, xl, None, None)
    bad = x.clone()
    bad[1, 2] = 59                                  # == n_vocab: nn.Embedding raises IndexError
    with pytest.raises(IndexError):
        net.infer(bad, xl, noise_scale=0)
    with pytest.raises(IndexError):
        net.infer(x, torch.tensor([9, 10]).cuda(), noise_scale=0)      # x_lengths > T
    again = net.infer(x, xl, noise_scale=0)          # the handle is still usable afterwards
    assert torch.equal(again[0], full[0])


@pytest.mark.parametrize("cfg_name", ["ljs_mb_istft_vits", "ljs_ms_istft_vits", "ljs_mini_istft_vits"])
def test_chunked_decode_with_istft_finalize(cfg_name):
    """The notebooks' streaming flow (inferz_test.ipynb cells 6-7): infer_z_only -> .dec on
    overlapping z-chunks -> cross-fade (spec, phase) as complex spectrograms -> istft_finalize.
    Checked against the oracle doing the same stitching on the CPU."""
    from gpu_util import make_net
    net, sd = make_net(cfg_name)
    rs = np.random.RandomState(4)
    Tz, chunk, hop = 23, 10, 6
    z = torch.from_numpy(rs.standard_normal((2, 192, Tz)).astype(np.float32))
    sb = cfg_name.endswith("mini_istft_vits")
    fpz = 64 if sb else 16                     # spectrogram frames per z-frame

    def stitch(dec):
        full = None
        for i0 in range(0, Tz, hop):
            zc = z[:, :, i0:min(i0 + chunk, Tz)]
            spec, phase = dec(zc)
            comp = spec * torch.exp(1j * phase)
            if full is None:
                full = comp
            else:
                want = (i0 + zc.shape[-1]) * fpz + 1
                ov = full.shape[-1] + comp.shape[-1] - want          # frames both chunks cover
                alpha = torch.linspace(0.0, 1.0, ov).view(*([1] * (comp.dim() - 1)), ov)
                merged = full[..., -ov:] * (1 - alpha) + comp[..., :ov] * alpha
                full = torch.cat([full[..., :-ov], merged, comp[..., ov:]], dim=-1)
            if i0 + chunk >= Tz:
                break
        return full

    _, cfg = config_for(cfg_name)
    W = R.Weights(sd)
    with torch.no_grad():
        ref_full = stitch(lambda zc: R.decode(W, cfg, zc)[2:4])
        ref_spec, ref_phase = torch.abs(ref_full), torch.angle(ref_full)
        if sb:
            ref_o = R.istft(ref_spec, ref_phase).unsqueeze(1)
        else:
            B = ref_spec.shape[0]
            y = R.istft(ref_spec.reshape(B * 4, 9, -1), ref_phase.reshape(B * 4, 9, -1)).reshape(B, 4, -1)
            h = W.w("dec.multistream_conv_post")[0] if "dec.multistream_conv_post.weight_v" in W \
                else torch.from_numpy(R.pqmf_synthesis_filter())
            ref_o = R.synthesis_filter_apply(R.zero_stuff(y), h)
    gpu_full = stitch(lambda zc: tuple(t.cpu() for t in net.dec(zc.cuda())[2:4]))
    assert gpu_full.shape == ref_full.shape and gpu_full.shape[-1] == Tz * fpz + 1
    o = net.istft_finalize(gpu_full.cuda(), None)                      # complex input, as the notebook
    o2 = net.istft_finalize(torch.abs(gpu_full).cuda(), torch.angle(gpu_full).cuda())
    assert float((o - o2).abs().max()) < 1e-5       # abs/angle taken on the GPU vs on the CPU
    assert o.shape == ref_o.shape
    assert rms(o.cpu().numpy() - ref_o.numpy()) < 1e-4


@pytest.mark.parametrize("B,T,ragged", [(1, 1, False), (17, 37, True), (3, 257, True), (2, 300, False)])
def test_shape_sweep_against_oracle(B, T, ragged):
    """Shapes around the kernels' tile boundaries (attention 32-key tiles, durations scan in
    256-token chunks, conv tiles of 128/192/384 columns, odd batch sizes) on the mini config."""
    from gpu_util import make_net
    from mb_istft_vits_amd import synth
    torch.set_num_threads(8)
    for attempt in range(6):                # re-draw inputs if a duration sits on a ceil() boundary
        net, sd = make_net("ljs_mini_mb_istft_vits", seed=1240 + B)
        x, xl, _ = synth.synthetic_batch(net.cfg, B, T, seed=B * 1000 + T + 7919 * attempt, ragged=ragged)
        ref = R.infer(sd, net.cfg, x, xl)
        w = (torch.exp(ref["logw"]) * ref["x_mask"]).numpy()[ref["x_mask"].numpy() > 0]
        if np.min(np.abs(w - np.round(w))) >= 2e-4:
            break
    else:
        pytest.skip("no input draw away from a ceil() boundary")
    (o, o_mb, spec, phase, attn, y_mask, (z, z_p, m_p, logs_p), _), ylen = net.infer_with_lengths(
        torch.from_numpy(x).cuda(), torch.from_numpy(xl).cuda(), noise_scale=0, length_scale=1)
    assert np.array_equal(ylen.cpu().numpy(), ref["y_lengths"].numpy())
    assert o.shape == ref["o"].shape
    assert _rel(z.cpu().numpy(), ref["z"].numpy()) < 5e-5
    assert rms(o.cpu().numpy() - ref["o"].numpy()) < 1e-4
    assert np.array_equal(attn.cpu().numpy(), ref["attn"].numpy())


def test_zero_length_utterance_in_batch():
    """An empty utterance (x_lengths == 0) next to real ones: the reference clamps its y_length to 1
    (models.py:719) and every mask zeroes it out; its row must not disturb the others."""
    from gpu_util import make_net
    net, sd = make_net("ljs_mini_mb_istft_vits", seed=1251)
    rs = np.random.RandomState(5)
    x = rs.randint(1, 59, size=(3, 9)).astype(np.int64)
    xl = np.asarray([0, 9, 4], np.int64)
    for b in range(3):
        x[b, xl[b]:] = 0
    ref = R.infer(sd, net.cfg, x, xl)
    (o, _, _, _, attn, y_mask, (z, _, _, _), _), ylen = net.infer_with_lengths(
        torch.from_numpy(x).cuda(), torch.from_numpy(xl).cuda(), noise_scale=0, length_scale=1)
    assert int(ylen[0]) == 1 and np.array_equal(ylen.cpu().numpy(), ref["y_lengths"].numpy())
    assert torch.isfinite(o).all()
    assert np.array_equal(attn.cpu().numpy(), ref["attn"].numpy())
    assert _rel(z.cpu().numpy(), ref["z"].numpy()) < 5e-5
    assert rms(o.cpu().numpy() - ref["o"].numpy()) < 1e-4


@pytest.mark.parametrize("cfg_name,B", [("ljs_mb_istft_vits", 64), ("ljs_ms_istft_vits", 64),
                                        ("uudb_ms_istft_vits_ms", 32)])
def test_full_size_properties(cfg_name, B):
    """BASELINE.json configs[1], configs[2] and the per-GPU share of configs[4] at full size
    (ljs_mb / ljs_ms B=64, uudb B=32 with speaker ids; T_text=200): size-independent checks.
      * determinism: two runs are bitwise identical;
      * batch independence: a sub-batch run padded to the same T' reproduces its rows bitwise
        (no cross-utterance arithmetic anywhere on the path);
      * `outputs=("o",)` (waveform-only launch) returns the same waveform bitwise;
      * spot parity: the oracle on two utterances at the same padded T' (the decoder is unmasked,
        so the pad length matters) agrees within the 1e-4 RMS bar."""
    from gpu_util import make_net
    from mb_istft_vits_amd import synth
    net, sd = make_net(cfg_name)
    x, xl, sid = synth.synthetic_batch(net.cfg, B, 200, seed=0)
    xg, xlg = torch.from_numpy(x).cuda(), torch.from_numpy(xl).cuda()
    sg = torch.from_numpy(sid).cuda() if sid is not None else None
    (o, o_mb, spec, phase, attn, y_mask, (z, z_p, m_p, logs_p), _), ylen = net.infer_with_lengths(
        xg, xlg, sg, noise_scale=0, length_scale=1)
    Tp = z.shape[-1]
    assert o.shape == (B, 1, 256 * Tp) and int(ylen.max()) == Tp
    assert torch.isfinite(o).all()
    o2 = net.infer(xg, xlg, sg, noise_scale=0, length_scale=1)[0]
    assert torch.equal(o, o2)
    only = net.infer(xg, xlg, sg, noise_scale=0, length_scale=1, outputs=("o",))
    assert torch.equal(only[0], o) and all(t is None for t in only[1:6]) and all(t is None for t in only[6])
    lo = B - 24
    r = net._run(xg[lo:lo + 8], xlg[lo:lo + 8], sg[lo:lo + 8] if sg is not None else None, 0, 1, None, True,
                 frames_hook=lambda t: Tp)
    assert _same_rows(r[0], o[lo:lo + 8]) and _same_rows(r[6][0], z[lo:lo + 8])
    torch.set_num_threads(8)
    pick = [3, B - 7]
    ref = R.infer(sd, net.cfg, x[pick], xl[pick], sid[pick] if sid is not None else None, t_frames=Tp)
    got = o[pick].cpu().numpy()
    assert np.array_equal(ylen[pick].cpu().numpy(), ref["y_lengths"].numpy())
    assert rms(got - ref["o"].numpy()) < 1e-4


def test_outputs_opt_in_subsets():
    """`infer(outputs=...)`: any subset of the tuple is materialised alone, bitwise equal to the
    full call; unknown names raise."""
    from gpu_util import make_net
    from mb_istft_vits_amd import synth
    for cfg_name in ("ljs_mini_mb_istft_vits", "ljs_mini_istft_vits", "uudb_ms_istft_vits_ms"):
        net, sd = make_net(cfg_name)
        x, xl, sid = synth.synthetic_batch(net.cfg, 3, 21, seed=8, ragged=True)
        xg, xlg = torch.from_numpy(x).cuda(), torch.from_numpy(xl).cuda()
        sg = torch.from_numpy(sid).cuda() if sid is not None else None
        full = net.infer(xg, xlg, sg, noise_scale=0, length_scale=1)
        names = ("o", "o_mb", "spec", "phase", "attn", "y_mask")
        for subset in (("o",), ("spec", "phase"), ("z", "attn"), ("o_mb", "y_mask", "m_p"), ()):
            got = net.infer(xg, xlg, sg, noise_scale=0, length_scale=1, outputs=subset)
            flat_full = dict(zip(names, full[:6]), **dict(zip(("z", "z_p", "m_p", "logs_p"), full[6])))
            flat_got = dict(zip(names, got[:6]), **dict(zip(("z", "z_p", "m_p", "logs_p"), got[6])))
            for k, v in flat_got.items():
                if k in subset and flat_full[k] is not None:
                    assert torch.equal(v, flat_full[k]), (cfg_name, subset, k)
                else:
                    assert v is None, (cfg_name, subset, k)
    with pytest.raises(ValueError):
        net.infer(xg, xlg, sg, noise_scale=0, outputs=("waveform",))


def test_oversized_batch_is_split_not_refused():
    """The fused iSTFT kernels address x_post with 32-bit byte offsets; a batch whose x_post reaches
    2 GiB used to be refused and now runs conv_post + iSTFT in sub-batches with bitwise the unsplit
    result.  (a) the split path forced at a small size through the `xpost_chunk_bytes` option, every
    decoder family, all outputs; (b) a batch that really crosses 2 GiB on the single-band decoder
    (x_post [B, 18, 64 T' + 1]), rows checked against a small batch padded alike."""
    from gpu_util import make_net
    rs = np.random.RandomState(11)
    for cfg_name in ("ljs_mini_mb_istft_vits", "ljs_ms_istft_vits", "ljs_mini_istft_vits"):
        net, sd = make_net(cfg_name)
        z = torch.from_numpy(rs.standard_normal((7, 192, 19)).astype(np.float32)).cuda()
        whole = net.dec(z)
        utt_bytes = (18 * (64 * 19 + 1) if cfg_name == "ljs_mini_istft_vits" else 72 * (16 * 19 + 1)) * 4
        net.set_option("xpost_chunk_bytes", 3 * utt_bytes + 100)      # sub-batches of 3, 3, 1
        split = net.dec(z)
        net.set_option("xpost_chunk_bytes", 0)
        for a, b in zip(whole, split):
            assert (a is None and b is None) or _same_rows(b, a), cfg_name     # bitwise (within rounding in split-K mode)
    net, sd = make_net("ljs_mini_istft_vits")
    B, Tp = 540, 870
    assert B * 18 * (64 * Tp + 1) * 4 >= 2 ** 31
    z = torch.randn(B, 192, Tp, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    o, _, spec, phase = net.dec(z)
    assert o.shape == (B, 1, 256 * Tp) and torch.isfinite(o).all()
    rows = [0, 1, 265, 266, B - 2, B - 1]
    o_s, _, spec_s, _ = net.dec(z[rows].contiguous())
    assert _same_rows(o_s, o[rows]) and _same_rows(spec_s, spec[rows])


def test_split_bf16_mode_meets_the_waveform_bar():
    """Opt-in `conv_bf16 = 3` at BASELINE configs[1] size (the large decoder convs run on the bf16 MFMA with
    split operands): deterministic, waveform within the north-star bar (1e-4 RMS) of the oracle on two
    utterances at the padded T', durations untouched (the text encoder never takes the mode)."""
    from gpu_util import make_net
    from mb_istft_vits_amd import synth
    net, sd = make_net("ljs_mb_istft_vits")
    B = 64
    x, xl, sid = synth.synthetic_batch(net.cfg, B, 200, seed=0)
    xg, xlg = torch.from_numpy(x).cuda(), torch.from_numpy(xl).cuda()
    exact, ylen0 = net.infer_with_lengths(xg, xlg, None, noise_scale=0, length_scale=1)
    net.set_option("conv_bf16", 3)
    try:
        r, ylen = net.infer_with_lengths(xg, xlg, None, noise_scale=0, length_scale=1)
        r2 = net.infer(xg, xlg, None, noise_scale=0, length_scale=1)
    finally:
        net.set_option("conv_bf16", 0)
    o, Tp = r[0], r[6][0].shape[-1]
    assert torch.equal(o, r2[0]) and torch.equal(ylen, ylen0)
    assert not torch.equal(o, exact[0])                                   # the mode was taken
    assert rms((o - exact[0]).cpu().numpy()) < 2e-5
    torch.set_num_threads(8)
    pick = [5, B - 3]
    ref = R.infer(sd, net.cfg, x[pick], xl[pick], None, t_frames=Tp)
    assert rms(o[pick].cpu().numpy() - ref["o"].numpy()) < 1e-4


def test_split_bf16_mode_leaves_long_text_durations_exact():
    """Texts longer than 256 tokens run the text encoder on the conv kernels that have the split-bf16 mode;
    `mbv_encode` must keep them exact all the same: durations and the encoder outputs are bitwise those of
    the exact mode, only the waveform path differs."""
    from gpu_util import make_net
    from mb_istft_vits_amd import synth
    net, sd = make_net("ljs_mb_istft_vits")
    x, xl, _ = synth.synthetic_batch(net.cfg, 8, 300, seed=3)
    xg, xlg = torch.from_numpy(x).cuda(), torch.from_numpy(xl).cuda()
    a, ya = net.infer_with_lengths(xg, xlg, None, noise_scale=0, length_scale=1)
    net.set_option("conv_bf16", 3)
    try:
        b, yb = net.infer_with_lengths(xg, xlg, None, noise_scale=0, length_scale=1)
    finally:
        net.set_option("conv_bf16", 0)
    assert torch.equal(ya, yb) and torch.equal(a[4], b[4])                # durations, attention path
    assert torch.equal(a[6][2], b[6][2]) and torch.equal(a[6][3], b[6][3])  # m_p, logs_p
    assert not torch.equal(a[0], b[0]) and rms((a[0] - b[0]).cpu().numpy()) < 2e-5


def test_split_bf16_mode_follows_weight_refreshes():
    """The mode reads a second, split copy of the packed weights; reloading weights into the same handle must
    rebuild it: after an in-place change of a decoder weight the split-mode result equals that of a fresh
    model built with the changed weights (and differs from the result before the change)."""
    from gpu_util import make_net
    net, sd = make_net("ljs_mini_mb_istft_vits")
    rs = np.random.RandomState(7)
    z = torch.from_numpy(rs.standard_normal((3, 192, 50)).astype(np.float32)).cuda()
    net.set_option("conv_bf16", 3)
    before = net.dec(z)[0].clone()
    key = next(k for k in sd if k.startswith("dec.resblocks.0.convs1.0") and k.endswith("weight_g"))
    sd2 = {k: v.copy() for k, v in sd.items()}
    sd2[key] = (sd2[key] * 1.5).astype(np.float32)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd2.items()})
    after = net.dec(z)[0].clone()
    fresh, _ = make_net("ljs_mini_mb_istft_vits")
    fresh.load_state_dict({k: torch.from_numpy(v) for k, v in sd2.items()})
    fresh = fresh.cuda()
    fresh.set_option("conv_bf16", 3)
    want = fresh.dec(z)[0]
    assert not torch.equal(before, after)
    assert torch.equal(after, want)
    net.set_option("conv_bf16", 0)
    exact = net.dec(z)[0]
    assert not torch.equal(exact, after) and rms((exact - after).cpu().numpy()) < 2e-5


def test_resblock_streams_are_bitwise_the_one_stream_schedule():
    """Small launches run the three ResBlocks of a decoder stage on three streams (capi.hip run_decoder):
    same kernels, the running-sum updates chained in the one-stream order, so every output must be
    bitwise what `dec_streams = 0` gives — in both modes, all decoder families, repeated (a race between
    the streams would show as run-to-run differences)."""
    from gpu_util import make_net
    rs = np.random.RandomState(21)
    for cfg_name in ("ljs_mb_istft_vits", "ljs_ms_istft_vits", "ljs_mini_istft_vits", "uudb_ms_istft_vits_ms"):
        net, sd = make_net(cfg_name)
        _, cfg = config_for(cfg_name)
        for B, Tp in ((1, 265), (3, 41)):
            z = torch.from_numpy(rs.standard_normal((B, cfg.inter_channels, Tp)).astype(np.float32)).cuda()
            g = None
            if cfg.gin_channels:
                g = torch.from_numpy(rs.standard_normal((B, cfg.gin_channels, 1)).astype(np.float32)).cuda()
            for splitk in (0, 1):
                net.set_option("splitk", splitk)
                net.set_option("dec_streams", 0)
                one = net.dec(z, g=g)
                net.set_option("dec_streams", 1)
                for _ in range(3):
                    three = net.dec(z, g=g)
                    for a, b in zip(one, three):
                        assert (a is None and b is None) or torch.equal(a, b), (cfg_name, B, splitk)
            net.set_option("splitk", 0)


def test_infer_on_a_caller_stream_is_bitwise_the_default_stream():
    """Everything is enqueued on the caller's stream: under `torch.cuda.stream(s)` with a fresh non-default stream
    `infer` gives the default stream's bits — at B = 1, where the decoder forks its ResBlocks from the caller's stream
    onto its internal streams (decoder_stage_concurrent), and at B = 8."""
    from gpu_util import make_net
    from mb_istft_vits_amd import synth
    net, _ = make_net("ljs_mb_istft_vits")
    for B in (1, 8):
        x, xl, _ = synth.synthetic_batch(net.cfg, B, 40, seed=11 + B, ragged=True)
        x, xl = torch.from_numpy(x).cuda(), torch.from_numpy(xl).cuda()
        ref = net.infer(x, xl, noise_scale=0, length_scale=1)
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            got = net.infer(x, xl, noise_scale=0, length_scale=1)
        s.synchronize()
        n = 0
        for a, b in zip(list(ref[:6]) + list(ref[6]), list(got[:6]) + list(got[6])):
            if isinstance(a, torch.Tensor):
                assert torch.equal(a, b), (B, n)
                n += 1
        assert n >= 10


def test_voice_conversion_matches_reference_golden():
    """`voice_conversion` (models.py:790-798) against the vector captured from the reference; the
    posterior encoder's noise draw is pinned by seeding torch and recovering it is not possible, so
    the shim's RNG is patched to hand the golden noise to the kernel."""
    from gpu_util import make_net
    gold = load_fixture("vc_uudb_b2")
    net, sd = make_net("uudb_ms_istft_vits_ms", int(gold["n_vocab"]), int(gold["weight_seed"]))
    noise = torch.from_numpy(gold["noise"]).cuda()
    real = torch.randn
    torch.randn = lambda *a, **k: noise if tuple(a) == tuple(noise.shape) else real(*a, **k)
    try:
        o, o_mb, y_mask, (z, z_p, z_hat) = net.voice_conversion(
            torch.from_numpy(gold["y"]).cuda(), torch.from_numpy(gold["y_lengths"]).cuda(),
            torch.from_numpy(gold["sid_src"]).cuda(), torch.from_numpy(gold["sid_tgt"]).cuda())
    finally:
        torch.randn = real
    assert np.array_equal(y_mask.cpu().numpy(), gold["y_mask"])
    for name, t in dict(z=z, z_p=z_p, z_hat=z_hat, o_mb=o_mb, o=o).items():
        assert t.shape == gold[name].shape, name
        assert _rel(t.cpu().numpy(), gold[name]) < 5e-5, (name, _rel(t.cpu().numpy(), gold[name]))
    assert rms(o.cpu().numpy() - gold["o"]) < 1e-4
    with pytest.raises(IndexError):
        net.voice_conversion(torch.from_numpy(gold["y"]).cuda(), torch.from_numpy(gold["y_lengths"]).cuda(),
                             torch.tensor([3, 12]).cuda(), torch.tensor([0, 1]).cuda())


def test_call_parameters_and_decoder_entry_match_reference_golden():
    """`params_mb_b2`: infer(noise_scale=0.667, length_scale=1.2, max_len=30) and `net.dec(z[:, :, 7:29])`
    captured from the real reference.  The shim draws its own noise, so z_p is rebuilt from the
    golden's pinned draw by running the decoder half on the golden z through `net.dec` and the
    encoder half through durations / masks."""
    from gpu_util import make_net
    gold = load_fixture("params_mb_b2")
    net, sd = make_net("ljs_mb_istft_vits", int(gold["n_vocab"]), int(gold["weight_seed"]))
    x, xl = torch.from_numpy(gold["x"]).cuda(), torch.from_numpy(gold["x_lengths"]).cuda()
    ls, ml = float(gold["length_scale"]), int(gold["max_len"])
    o, o_mb, spec, phase, attn, y_mask, (z, z_p, m_p, logs_p), _ = net.infer(
        x, xl, noise_scale=0, length_scale=ls, max_len=ml)
    assert np.array_equal(attn.sum(2).cpu().numpy(), gold["attn"])          # durations at length_scale 1.2
    assert np.array_equal(y_mask.cpu().numpy(), gold["y_mask"])
    assert o.shape == gold["o"].shape                                       # max_len truncation
    # the prior sample with the reference's noise: z_p = m_p + noise * exp(logs_p) * noise_scale
    zp = m_p.cpu() + torch.from_numpy(gold["noise"]) * torch.exp(logs_p.cpu()) * float(gold["noise_scale"])
    assert _rel(zp.numpy(), gold["z_p"]) < 5e-5
    # decoder entry on the reference's own z (masked, truncated as models.py:733 does)
    zin = (torch.from_numpy(gold["z"]) * torch.from_numpy(gold["y_mask"]))[:, :, :ml].cuda()
    do, do_mb, dspec, dphase = net.dec(zin)
    assert rms(do.cpu().numpy() - gold["o"]) < 1e-4
    assert _rel(do_mb.cpu().numpy(), gold["o_mb"]) < 5e-5
    assert _rel(thin("spec", dspec.cpu()).numpy(), gold["spec"]) < 5e-5
    lo, hi = int(gold["dec_chunk_lo"]), int(gold["dec_chunk_hi"])
    co, co_mb, cspec, cphase = net.dec(torch.from_numpy(gold["z"][:, :, lo:hi]).contiguous().cuda())
    assert rms(co.cpu().numpy() - gold["dec_o"]) < 1e-4
    assert _rel(co_mb.cpu().numpy(), gold["dec_o_mb"]) < 5e-5
    assert _rel(thin("phase", cphase.cpu()).numpy(), gold["dec_phase"]) < 5e-5


def test_large_batch_and_long_utterance_index_paths():
    """Sizes well past BASELINE's: (a) batch 520 x 200 tokens on the full config — rows of the big run
    equal, bitwise, the same utterances run as a batch of 8 padded to the same T' (the 128-channel
    decoder activations are > 2^31 bytes each, so 32-bit offset slips would show); (b) two 1 200-token
    utterances (T' ~ 3 500, 0.9 M samples each) on the mini config against the oracle."""
    from gpu_util import make_net
    from mb_istft_vits_amd import synth
    net, sd = make_net("ljs_mb_istft_vits")
    x, xl, _ = synth.synthetic_batch(net.cfg, 520, 200, seed=5, ragged=True)
    xg, xlg = torch.from_numpy(x).cuda(), torch.from_numpy(xl).cuda()
    (o, _, spec, _, _, _, (z, _, _, _), _), ylen = net.infer_with_lengths(xg, xlg, noise_scale=0, length_scale=1)
    Tp = z.shape[-1]
    assert torch.isfinite(o).all() and o.shape == (520, 1, 256 * Tp)
    assert 520 * 128 * 16 * Tp * 4 > 2 ** 31                # bytes of one [B, 128, 16 T'] activation
    r = net._run(xg[510:518], xlg[510:518], None, 0, 1, None, True, frames_hook=lambda t: Tp)
    assert _same_rows(r[0], o[510:518]) and _same_rows(r[2], spec[510:518])
    del o, spec, z, r
    torch.cuda.empty_cache()

    net, sd = make_net("ljs_mini_mb_istft_vits", seed=1260)
    torch.set_num_threads(16)
    for attempt in range(6):
        x, xl, _ = synth.synthetic_batch(net.cfg, 2, 1200, seed=77 + attempt, ragged=True)
        ref = R.infer(sd, net.cfg, x, xl)
        w = (torch.exp(ref["logw"]) * ref["x_mask"]).numpy()[ref["x_mask"].numpy() > 0]
        if np.min(np.abs(w - np.round(w))) >= 2e-4:
            break
    (o, *_), ylen = net.infer_with_lengths(torch.from_numpy(x).cuda(), torch.from_numpy(xl).cuda(),
                                           noise_scale=0, length_scale=1)
    assert np.array_equal(ylen.cpu().numpy(), ref["y_lengths"].numpy())
    assert o.shape == ref["o"].shape and o.shape[-1] > 800000
    assert rms(o.cpu().numpy() - ref["o"].numpy()) < 1e-4


def test_splitk_low_latency_mode_in_subprocess():
    """MBV_CONV_SPLITK=1 (split-K over input channels for launches that leave most of the chip idle —
    the single-utterance service case) is read once per process, so it is exercised in a child:
    three goldens from the real reference + bitwise run-to-run determinism of the ticketed reduce."""
    code = r"""
import sys, numpy as np, torch
sys.path.insert(0, %r); sys.path.insert(0, %r)
from helpers import FIXTURES, OVERRIDES, load_fixture, rms
from gpu_util import make_net
for fx in ("mini_b1", "mb_b3", "uudb_b2", "sb_mini_b2"):
    gold = load_fixture(fx)
    net, sd = make_net(FIXTURES[fx], int(gold["n_vocab"]), int(gold["weight_seed"]), overrides=OVERRIDES.get(fx))
    x, xl = torch.from_numpy(gold["x"]).cuda(), torch.from_numpy(gold["x_lengths"]).cuda()
    sid = torch.from_numpy(gold["sid"]).cuda() if "sid" in gold else None
    out = net.infer(x, xl, sid=sid, noise_scale=0, length_scale=1)
    assert np.array_equal(out[4].sum(2).cpu().numpy(), gold["attn"]), fx
    err = rms(out[0].cpu().numpy() - gold["o"])
    assert err < 1e-4, (fx, err)
    again = net.infer(x, xl, sid=sid, noise_scale=0, length_scale=1)[0]
    assert torch.equal(again, out[0]), fx
    print(fx, "rms err %%.2e" %% err)
print("SPLITK-OK")
""" % (os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MBV_CONV_SPLITK="1")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "SPLITK-OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def test_sharded_infer_single_rank_equals_plain_infer_with_sdp():
    """`dist.sharded_infer` on a one-rank gloo group (the collectives run, on CUDA tensors) returns
    what `infer` returns — including the StochasticDurationPredictor noise, which the sharded path
    draws for the full batch and slices (same CPU seed => same durations)."""
    import socket
    import torch.distributed as dist
    from gpu_util import make_net
    from mb_istft_vits_amd import synth, dist as mdist
    net, sd = make_net("ljs_mini_mb_istft_vits", seed=1271, overrides={"use_sdp": True})
    x, xl, _ = synth.synthetic_batch(net.cfg, 4, 30, seed=3, ragged=True)
    xg, xlg = torch.from_numpy(x).cuda(), torch.from_numpy(xl).cuda()
    torch.manual_seed(99)
    (o_ref, *_), ylen_ref = net.infer_with_lengths(xg, xlg, noise_scale=0, length_scale=1, noise_scale_w=0.5)
    sock = socket.socket(); sock.bind(("127.0.0.1", 0)); port = sock.getsockname()[1]; sock.close()
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=0, world_size=1)
    try:
        torch.manual_seed(99)
        o, ylen = mdist.sharded_infer(net, xg, xlg, None, noise_scale=0, length_scale=1, noise_scale_w=0.5)
    finally:
        dist.destroy_process_group()
    assert torch.equal(ylen, ylen_ref) and torch.equal(o, o_ref)


def test_set_option_splitk_in_process():
    """`net.set_option("splitk", 1)` (mbv_set_option) switches the low-latency mode per model."""
    from gpu_util import make_net
    from mb_istft_vits_amd import _capi
    gold = load_fixture("mb_b3")
    net, sd = make_net("ljs_mb_istft_vits", int(gold["n_vocab"]), int(gold["weight_seed"]))
    x, xl = torch.from_numpy(gold["x"]).cuda(), torch.from_numpy(gold["x_lengths"]).cuda()
    o0 = net.infer(x, xl, noise_scale=0, length_scale=1)[0]
    net.set_option("splitk", 1)
    o1 = net.infer(x, xl, noise_scale=0, length_scale=1)[0]
    net.set_option("splitk", 0)
    o2 = net.infer(x, xl, noise_scale=0, length_scale=1)[0]
    assert rms(o1.cpu().numpy() - gold["o"]) < 1e-4
    assert float((o1 - o0).abs().max()) < 1e-4
    if not SPLITK:
        assert torch.equal(o2, o0)                       # back to the default path, bitwise
        assert not torch.equal(o1, o0)                   # the split path really ran (other summation order)
    with pytest.raises(_capi.MbvError):
        net.set_option("no-such-option", 1)


@pytest.mark.timeout(900)
def test_trimmed_decode_is_bitwise_the_default_on_valid_samples():
    """Opt-in `infer(..., outputs=("o",), trim=True)`: per utterance the decoder computes only what its valid
    256 * y_lengths[b] samples depend on.  Those samples must be BITWISE the default call's, the padded region
    zero — also when the scratch behind an utterance's limit holds the leftovers of a longer batch (run first),
    with speaker conditioning, with max_len, and at the full bench size."""
    from gpu_util import make_net
    from mb_istft_vits_amd import synth
    for cfg_name, B, T, ml in (("ljs_mb_istft_vits", 9, 110, None), ("uudb_ms_istft_vits_ms", 6, 90, None),
                               ("ljs_ms_istft_vits", 5, 140, 300), ("ljs_mb_istft_vits", 64, 200, None)):
        net, _ = make_net(cfg_name)
        # leftovers: one batch of long utterances through the same scratch arena first
        xl_, xll_, sid_ = synth.synthetic_batch(net.cfg, B, T, seed=5)
        net.infer(torch.from_numpy(xl_).cuda(), torch.from_numpy(xll_).cuda(),
                  torch.from_numpy(sid_).cuda() if sid_ is not None else None, noise_scale=0, length_scale=1, outputs=("o",))
        x, xl, sid = synth.synthetic_batch(net.cfg, B, T, seed=6, ragged=True)
        xl[0] = max(3, T // 5)                            # one very short utterance
        xg, xlg = torch.from_numpy(x).cuda(), torch.from_numpy(xl).cuda()
        sg = torch.from_numpy(sid).cuda() if sid is not None else None
        (o_ref, *_), ylen = net.infer_with_lengths(xg, xlg, sg, noise_scale=0, length_scale=1, outputs=("o",), max_len=ml)
        (o_trim, *rest), ylen2 = net.infer_with_lengths(xg, xlg, sg, noise_scale=0, length_scale=1, outputs=("o", "z"),
                                                       max_len=ml, trim=True)
        assert torch.equal(ylen, ylen2) and o_trim.shape == o_ref.shape and rest[5][0] is not None
        spf = net.cfg.samples_per_frame
        for b in range(B):
            n = min(int(ylen[b]) * spf, o_ref.shape[-1])
            assert torch.equal(o_trim[b, 0, :n], o_ref[b, 0, :n]), (cfg_name, b)
            if os.environ.get("MBV_CONV_SPLITK", "0") in ("", "0"):      # (the low-latency mode ignores the option: full decode)
                assert not bool(o_trim[b, 0, n:].any()), (cfg_name, b)
        assert int(ylen.min()) < int(ylen.max())          # the batch really is ragged
        # the default is untouched by the option having been used
        o_again = net.infer(xg, xlg, sg, noise_scale=0, length_scale=1, outputs=("o",), max_len=ml)[0]
        assert torch.equal(o_again, o_ref)
    with pytest.raises(ValueError):
        net.infer(xg, xlg, sg, noise_scale=0, length_scale=1, trim=True)          # all outputs + trim


def test_timings_of_earlier_calls_stay_readable():
    """The reference's `timings` dict is usually read late or never; ours resolves lazily from HIP events.  The
    handle keeps the events of its last 8 calls, so a dict read after newer calls still holds its own call's
    stage times (r02: it turned into NaNs as soon as another infer had started)."""
    from gpu_util import make_net
    from mb_istft_vits_amd import synth
    net, _ = make_net("ljs_mini_mb_istft_vits")
    x, xl, _ = synth.synthetic_batch(net.cfg, 2, 20, seed=1)
    xg, xlg = torch.from_numpy(x).cuda(), torch.from_numpy(xl).cuda()
    ts = [net.infer(xg, xlg, noise_scale=0, length_scale=1)[7] for _ in range(10)]
    late = dict(ts[-6])                                  # five calls later
    assert all(np.isfinite(v) and v >= 0 for v in late.values()) and late["waveform_decoder"] > 0
    assert all(np.isnan(v) for v in dict(ts[0]).values())      # ten calls later: reused, NaN by contract
    assert all(np.isfinite(v) for v in dict(ts[-1]).values())
