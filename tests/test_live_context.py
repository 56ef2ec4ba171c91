"""Live voice conversion, the reach of the posterior path (no GPU): with the CPU oracle, z_hat frame t of
posterior_encoder -> flow_forward -> flow_reverse depends on spectrogram frames within `mbv_converter_context` of t
only, and a window with that context reproduces the whole-recording z_hat on the frames it keeps."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import ref_infer as R

from mb_istft_vits_amd import _capi, models, synth, utils as mutils

T = 300
_CACHE = {}


def _setup(name):
    """(net, W, spectrogram-like input, noise, g_src, g_tgt, whole-run z_hat), computed once per config."""
    if name not in _CACHE:
        hps = mutils.get_hparams_from_file(mutils.builtin_config(name))
        net = models.SynthesizerTrn(59, hps.data.filter_length // 2 + 1, hps.train.segment_size // hps.data.hop_length,
                                    n_speakers=hps.data.n_speakers, **hps.model)
        sd = synth.make_state_dict(net.cfg, 1234)
        W = R.Weights(sd)
        rs = np.random.RandomState(7)
        y = torch.from_numpy(np.abs(rs.standard_normal((1, net.cfg.spec_channels, T))).astype(np.float32))
        noise = torch.from_numpy(rs.standard_normal((1, net.cfg.inter_channels, T)).astype(np.float32))
        g_src = g_tgt = None
        if "emb_g.weight" in sd:
            g_src = W["emb_g.weight"][torch.tensor([3])].unsqueeze(-1)
            g_tgt = W["emb_g.weight"][torch.tensor([7])].unsqueeze(-1)
        _CACHE[name] = (net, W, y, noise, g_src, g_tgt, _z_hat(net.cfg, W, y, noise, g_src, g_tgt))
    return _CACHE[name]


def _z_hat(cfg, W, y, noise, g_src, g_tgt, length=None):
    with torch.no_grad():
        z, _, _, mask = R.posterior_encoder(W, cfg, y, torch.tensor([y.shape[2] if length is None else length]), g_src, noise)
        return R.flow_reverse(W, cfg, R.flow_forward(W, cfg, z, mask, g_src), mask, g_tgt) * mask


@pytest.mark.parametrize("name", ["uudb_ms_istft_vits_ms", "ljs_ms_istft_vits"])
def test_a_perturbed_frame_reaches_no_further_than_the_context(name):
    net, W, y, noise, g_src, g_tgt, whole = _setup(name)
    L, Rr = net.converter_context()
    y2 = y.clone()
    y2[:, :, 150] += 1.0
    moved = (_z_hat(net.cfg, W, y2, noise, g_src, g_tgt) != whole).any(dim=1)[0].nonzero().flatten()
    assert moved.numel() > 0
    lo, hi = 150 - int(moved.min()), int(moved.max()) - 150
    print("%s: perturbing spectrogram frame 150 of %d moves z_hat frames [150 - %d, 150 + %d]; context (%d, %d)"
          % (name, T, lo, hi, L, Rr))
    # z_hat frame t reads spectrogram frames [t - L, t + R]: frame 150 is read by t in [150 - R, 150 + L]
    assert lo <= Rr and hi <= L
    assert lo >= 32 and hi >= 32                        # (the reach is real: enc_q's 16 layers alone give 32)


@pytest.mark.parametrize("name", ["uudb_ms_istft_vits_ms", "ljs_ms_istft_vits"])
def test_a_window_with_the_context_reproduces_the_whole_run(name):
    net, W, y, noise, g_src, g_tgt, whole = _setup(name)
    cfg_s = net._config_struct()
    out = (C.c_int32 * 2)()
    worst = 0.0
    # (first, count, spectrogram frames final): both edges of the recording, the middle, an open recording
    for first, count, final in [(0, 32, T), (120, 32, T), (268, 32, T), (100, 100, 296), (199, 5, T), (97, 1, T)]:
        assert _capi.lib().mbv_convert_window(C.byref(cfg_s), first, count, final, C.byref(out)) == 0
        wa, wb = int(out[0]), int(out[1])
        # the window as the GPU path runs it: one row of a padded run, here padded to the whole run's width (so that
        # the CPU conv library picks one algorithm for both runs and rounding is not what is compared)
        yw, nw = torch.zeros_like(y), torch.zeros_like(noise)
        yw[:, :, :wb - wa], nw[:, :, :wb - wa] = y[:, :, wa:wb], noise[:, :, wa:wb]
        got = _z_hat(net.cfg, W, yw, nw, g_src, g_tgt, length=wb - wa)
        d = float((got[:, :, first - wa:first - wa + count] - whole[:, :, first:first + count]).abs().max())
        print("%s: z_hat[%d, %d) from window [%d, %d): max abs difference %.3g" % (name, first, first + count, wa, wb, d))
        worst = max(worst, d)
    assert worst <= 1e-6
