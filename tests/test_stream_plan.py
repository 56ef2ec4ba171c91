"""Streaming decode, host side (no GPU): the decoder's receptive field (`mbv_decoder_context`) against the oracle's
measured support, the chunk schedule, the oracle decoding each window of the schedule, and the one-shot iSTFT
kernels' code left unchanged by the ranged-output mode."""
import json
import os
import shutil

import numpy as np
import pytest
import torch

from mb_istft_vits_amd import models, synth, utils as mutils
from mb_istft_vits_amd.stream import chunk_schedule
from oracle import ref_infer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RB2 = {"resblock": "2", "resblock_dilation_sizes": [[1, 3], [1, 3], [1, 3]]}
CONFIGS = [("ljs_mb_istft_vits", None), ("ljs_mini_mb_istft_vits", None), ("ljs_ms_istft_vits", None),
           ("uudb_ms_istft_vits_ms", None), ("ljs_istft_vits", None), ("ljs_mini_istft_vits", None),
           ("ljs_mini_mb_istft_vits", RB2)]


def _net(name, overrides=None):
    hps = mutils.get_hparams_from_file(mutils.builtin_config(name))
    for k, v in (overrides or {}).items():
        hps.model[k] = v
    net = models.SynthesizerTrn(59, hps.data.filter_length // 2 + 1, hps.train.segment_size // hps.data.hop_length,
                                n_speakers=hps.data.n_speakers, **hps.model)
    return net, synth.make_state_dict(net.cfg, 1234)


def _decode(sd, cfg, z, g):
    with torch.no_grad():
        return ref_infer.decode(sd, cfg, z, g)[0][:, 0].numpy().astype(np.float64)


def _g(cfg, B, seed):
    if not cfg.gin_channels:
        return None
    return torch.from_numpy(np.random.default_rng(seed).standard_normal((B, cfg.gin_channels, 1)).astype(np.float32))


@pytest.mark.parametrize("name,overrides", CONFIGS, ids=[c[0] + ("_rb2" if c[1] else "") for c in CONFIGS])
def test_context_covers_measured_support(name, overrides):
    net, sd = _net(name, overrides)
    Lc, Rc = net.decoder_context()
    spf = net.cfg.samples_per_frame
    Tp, t = 2 * max(Lc, Rc) + 12, max(Lc, Rc) + 5
    rng = np.random.default_rng(7)
    z = torch.from_numpy(rng.standard_normal((1, net.cfg.inter_channels, Tp)).astype(np.float32))
    g = _g(net.cfg, 1, 8)
    base = _decode(sd, net.cfg, z, g)
    z2 = z.clone()
    z2[:, :, t] += torch.from_numpy(rng.standard_normal(net.cfg.inter_channels).astype(np.float32))
    changed = np.nonzero(_decode(sd, net.cfg, z2, g)[0] != base[0])[0]
    assert changed.size
    lo, hi = int(changed[0]), int(changed[-1])
    # a sample of frame s reads z-frames [s - L, s + R], so z-frame t reaches the samples of frames [t - R, t + L]
    assert lo >= spf * (t - Rc) and hi < spf * (t + 1 + Lc), (lo, hi, Lc, Rc)
    L_meas, R_meas = hi // spf - t, t - lo // spf
    assert L_meas <= Lc <= L_meas + 1 and R_meas <= Rc <= R_meas + 1, ((L_meas, R_meas), (Lc, Rc))


def test_context_values():
    """The per-config values DESIGN §7.3 quotes."""
    assert _net("ljs_mb_istft_vits")[0].decoder_context() == (25, 24)
    assert _net("uudb_ms_istft_vits_ms")[0].decoder_context() == (25, 24)
    assert _net("ljs_mini_istft_vits")[0].decoder_context() == (13, 13)
    assert _net("ljs_mini_mb_istft_vits", RB2)[0].decoder_context() == (12, 12)


@pytest.mark.parametrize("T,c,cap", [(1, 32, 256), (17, 32, 256), (300, 32, 256), (1000, 32, 256), (5, 1, 4),
                                     (777, 8, 64), (64, 64, 64), (2, 1, 1)])
def test_schedule_covers_once(T, c, cap):
    s = chunk_schedule(T, c, cap)
    assert s[0][0] == 0 and sum(n for _, n in s) == T
    for (f0, n0), (f1, _) in zip(s, s[1:]):
        assert f1 == f0 + n0
    counts = [n for _, n in s]
    for i, n in enumerate(counts[:-1]):
        assert n == min(c << i, cap)
    assert 1 <= counts[-1] <= min(c << (len(counts) - 1), cap)


def test_schedule_edges():
    assert chunk_schedule(0) == []
    assert chunk_schedule(1) == [(0, 1)]
    assert chunk_schedule(100, 32, 256) == [(0, 32), (32, 64), (96, 4)]
    assert chunk_schedule(1000, 32, 256) == [(0, 32), (32, 64), (96, 128), (224, 256), (480, 256), (736, 256),
                                             (992, 8)]
    for bad in ((10, 0, 4), (10, 8, 4)):
        with pytest.raises(ValueError):
            chunk_schedule(*bad)


@pytest.mark.parametrize("name,overrides,Tp", [("ljs_mini_mb_istft_vits", None, 100), ("ljs_ms_istft_vits", None, 70),
                                               ("uudb_ms_istft_vits_ms", None, 60), ("ljs_mini_istft_vits", None, 90),
                                               ("ljs_mini_mb_istft_vits", RB2, 75)])
def test_oracle_windows_reproduce_one_shot(name, overrides, Tp):
    net, sd = _net(name, overrides)
    Lc, Rc = net.decoder_context()
    spf = net.cfg.samples_per_frame
    z = torch.from_numpy(np.random.default_rng(3).standard_normal((2, net.cfg.inter_channels, Tp)).astype(np.float32))
    g = _g(net.cfg, 2, 4)
    full = _decode(sd, net.cfg, z, g)
    out = np.full_like(full, np.nan)
    for first, count in chunk_schedule(Tp, 8, 32):
        wa, wb = max(0, first - Lc), min(Tp, first + count + Rc)
        w = _decode(sd, net.cfg, z[:, :, wa:wb].contiguous(), g)
        out[:, spf * first:spf * (first + count)] = w[:, spf * (first - wa):spf * (first - wa + count)]
    err = np.abs(out - full).max() / np.abs(full).max()
    assert err <= 1e-6, err


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_one_shot_istft_kernels_unchanged():
    """The ranged-output mode is a template flag: the instantiations the one-shot decode runs compile to the
    instruction streams recorded before it existed (scripts/istft_disasm.py)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("istft_disasm", os.path.join(ROOT, "scripts", "istft_disasm.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    with open(os.path.join(ROOT, "tests", "golden", "istft_disasm_fingerprints.json")) as f:
        golden = json.load(f)
    now = tool.compile_fingerprints()
    assert len(golden) == 18
    changed = sorted(k for k in golden if now.get(k) != golden[k])
    assert not changed, changed
    assert sum(k.endswith("+ranged") for k in now) == 6
