"""Generate the per-token prosody fixtures (prosody_mini_b2.npz, prosody_uudb_b2.npz) from the REAL reference.

Run in the build container only (the reference is not on the GPU box):

    python tests/golden/make_prosody_golden.py

Like make_golden.py (whose shims and model builder it uses) it imports the reference in-process, loads the synthetic
checkpoint and runs `SynthesizerTrn.infer` -- here with `length_scale` a tensor [B, 1, T_text], which models.py:717
broadcasts, and with the randn_like of models.py:729 handing out a stored draw.  It keeps the inputs, the scale table,
the draw, the durations (attn.sum(2)), the expanded prior, z_p, z and the waveform.  Only data is stored.

A fixture is accepted only if every float64 duration exp(logw) * s_t below x_lengths is at least 1e-3 away from an
integer (so that no fp32 implementation can land on the other side of the ceil); otherwise the next input seed is
taken.  The accepted seed is stored.  B = 2, ragged, T_text = 20, scales drawn from {0.5, 1, 1.75, 3}.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True
from make_golden import import_reference, build_reference_model      # noqa: E402  (also puts the repository on sys.path)

SCALES = (0.5, 1.0, 1.75, 3.0)
NOISE_SCALE = 0.667

CASES = [
    # (fixture, config, n_vocab, T_text, x_lengths, weight seed)
    ("prosody_mini_b2", "ljs_mini_mb_istft_vits", 59, 20, [20, 13], 1234),
    ("prosody_uudb_b2", "uudb_ms_istft_vits_ms", 59, 20, [14, 20], 1234),
]


def main():
    import torch
    from mb_istft_vits_amd import synth, spec as mspec, utils as mutils
    torch.manual_seed(0)
    torch.set_num_threads(4)
    models, utils, _, _ = import_reference()
    for fixture, cfg_name, n_vocab, T, xlens, wseed in CASES:
        hps, net = build_reference_model(models, utils, cfg_name, n_vocab)
        my_hps = mutils.get_hparams_from_file(mutils.builtin_config(cfg_name))
        cfg = mspec.config_from_ctor(n_vocab, my_hps.data.filter_length // 2 + 1,
                                     my_hps.train.segment_size // my_hps.data.hop_length,
                                     n_speakers=my_hps.data.n_speakers, **my_hps.model)
        sd = synth.make_state_dict(cfg, wseed)
        net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        B = len(xlens)
        xl = np.asarray(xlens, np.int64)
        seed = 500
        while True:
            rs = np.random.RandomState(seed)
            x = rs.randint(1, n_vocab, size=(B, T)).astype(np.int64)
            for b in range(B):
                x[b, xl[b]:] = 0
            sid = rs.randint(0, cfg.n_speakers, size=(B,)).astype(np.int64) if cfg.has_speaker else None
            scale = np.asarray(SCALES, np.float32)[rs.randint(0, len(SCALES), size=(B, 1, T))]
            args = (torch.from_numpy(x), torch.from_numpy(xl))
            kw = dict(sid=torch.from_numpy(sid) if sid is not None else None, length_scale=torch.from_numpy(scale))
            taps = {}
            hk = net.dp.register_forward_hook(lambda m, i, o: taps.update(logw=o.detach().clone()))
            with torch.no_grad():
                probe = net.infer(*args, noise_scale=0, **kw)
            hk.remove()
            d = np.exp(taps["logw"].numpy().astype(np.float64)) * scale.astype(np.float64)
            d = np.concatenate([d[b, 0, :xl[b]] for b in range(B)])
            margin = float(np.min(np.abs(d - np.round(d))))
            if margin >= 1e-3:
                break
            print("  %s: input seed %d rejected: ceil margin %.2e" % (fixture, seed, margin))
            seed += 1
        Tp = probe[6][0].shape[-1]
        noise = rs.standard_normal((B, cfg.inter_channels, Tp)).astype(np.float32)
        real = torch.randn_like
        torch.randn_like = lambda t, **k: torch.from_numpy(noise) if tuple(t.shape) == noise.shape else real(t, **k)
        try:
            with torch.no_grad():
                o, o_mb, spec, phase, attn, y_mask, (z, z_p, m_p, logs_p), _ = net.infer(*args, noise_scale=NOISE_SCALE, **kw)
        finally:
            torch.randn_like = real
        w = attn.sum(2).numpy()                                  # [B, 1, T_text]: the durations (models.py:680)
        assert np.array_equal(w[:, 0], np.ceil(np.exp(taps["logw"].numpy().astype(np.float64)) * scale)[:, 0]
                              * (np.arange(T)[None] < xl[:, None]))
        out = dict(x=x, x_lengths=xl, scale=scale, noise=noise, noise_scale=np.float32(NOISE_SCALE), w=w,
                   y_mask=y_mask.numpy(), m_p=m_p.numpy(), logs_p=logs_p.numpy(), z_p=z_p.numpy(), z=z.numpy(),
                   o=o.numpy(), weight_seed=np.int64(wseed), n_vocab=np.int64(n_vocab), input_seed=np.int64(seed),
                   ceil_margin=np.float64(margin))
        if sid is not None:
            out["sid"] = sid
        path = os.path.join(HERE, fixture + ".npz")
        np.savez_compressed(path, **out)
        print("%-16s cfg=%s input seed=%d T'=%d w[0]=%s margin=%.3g  %.0f KB" % (
            fixture, cfg_name, seed, Tp, w[0, 0, :8], margin, os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
