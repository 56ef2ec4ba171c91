"""Generate the forced-alignment fixtures (align_mini_b2.npz, align_uudb_b2.npz) from the REAL reference.

Run in the build container only (the reference is not on the GPU box):

    python tests/golden/make_align_golden.py

Like make_golden.py it imports the reference in-process with the librosa / .cuda() shims, but with a real
`monotonic_align`: core.pyx is compiled with the local Cython into a temporary directory outside the repository
(nothing of it is kept).  It loads the synthetic checkpoint, runs SynthesizerTrn.forward up to models.py:680 under
no_grad (the call is ended right after the search) with the randn_like of models.py:245 handing out a stored draw,
and keeps inputs, noise, neg_cent, w, z_p and the text statistics neg_cent was formed from.  Only data is stored.

A fixture is accepted only if its path is stable: the float64 search on the reference's neg_cent gives the
reference's path, and keeps giving it under 20 random perturbations of neg_cent of size 2^-16 * sum|summands| per
cell.  Otherwise the next input seed is taken; the accepted seed is stored.  Rows: one with t_x == t_y, one with
t_y >= 2 t_x (rows of the band that span every token), the others ragged in between.
"""
import os
import shutil
import subprocess
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("MBV_REFERENCE", "/root/reference")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.dont_write_bytecode = True

SETUP = """
from setuptools import setup, Extension
from Cython.Build import cythonize
setup(name="mas_core", ext_modules=cythonize([Extension("core", ["core.pyx"])], language_level=3))
"""


def build_core(tmp):
    shutil.copy(os.path.join(REF, "monotonic_align", "core.pyx"), os.path.join(tmp, "core.pyx"))
    with open(os.path.join(tmp, "setup.py"), "w") as f:
        f.write(SETUP)
    subprocess.run([sys.executable, "setup.py", "-q", "build_ext", "--inplace"], cwd=tmp, check=True,
                   stdout=subprocess.DEVNULL)
    sys.path.insert(0, tmp)
    import core
    sys.path.remove(tmp)
    return core


def import_reference(core):
    sys.path.insert(0, REF)
    inner = types.ModuleType("monotonic_align.monotonic_align")
    inner.__path__ = []
    inner.core = core
    sys.modules["monotonic_align.monotonic_align"] = inner
    sys.modules["monotonic_align.monotonic_align.core"] = core
    lib = types.ModuleType("librosa")
    libu = types.ModuleType("librosa.util")
    libf = types.ModuleType("librosa.filters")
    for n in ("pad_center", "tiny", "normalize"):
        setattr(libu, n, lambda *a, **k: None)
    lib.util, lib.filters = libu, libf
    sys.modules.update({"librosa": lib, "librosa.util": libu, "librosa.filters": libf})
    import torch
    torch.Tensor.cuda = lambda self, device=None, **k: self.to(device) if device is not None else self
    import monotonic_align    # noqa: the reference's package, on the compiled core
    import models             # noqa: the reference's
    import utils              # noqa
    return models, utils, monotonic_align


class _Done(Exception):
    pass


def run_forward(net, mas, x, xl, y, yl, sid, noise):
    """forward up to models.py:680: neg_cent and the path from the search call, z_p from the flow."""
    import torch
    taps = {}
    real_mp, real_rl = mas.maximum_path, torch.randn_like

    def grab_path(neg_cent, mask):
        taps["neg_cent"] = neg_cent.detach().clone()
        taps["attn"] = real_mp(neg_cent, mask)
        raise _Done()

    hooks = [net.flow.register_forward_hook(lambda m, i, o: taps.update(z_p=o.detach().clone())),
             net.enc_p.register_forward_hook(lambda m, i, o: taps.update(m_text=o[1].clone(), logs_text=o[2].clone()))]
    mas.maximum_path = grab_path
    torch.randn_like = lambda t, **k: torch.from_numpy(noise) if tuple(t.shape) == noise.shape else real_rl(t, **k)
    try:
        with torch.no_grad():
            net(torch.from_numpy(x), torch.from_numpy(xl), torch.from_numpy(y), torch.from_numpy(yl),
                sid=torch.from_numpy(sid) if sid is not None else None)
    except _Done:
        pass
    finally:
        mas.maximum_path, torch.randn_like = real_mp, real_rl
        for h in hooks:
            h.remove()
    return {k: v.numpy() for k, v in taps.items()}


def stable(taps, xl, yl, rs):
    import align_ref
    v32 = taps["neg_cent"].astype(np.float32)
    _, mag = align_ref.neg_cent(taps["z_p"], taps["m_text"], taps["logs_text"])
    for b in range(v32.shape[0]):
        ty, tx = int(yl[b]), int(xl[b])
        want = taps["attn"][b].astype(np.int32)
        if not np.array_equal(align_ref.maximum_path_each(v32[b], ty, tx, np.float32)[0], want):
            raise AssertionError("the fp32 restatement differs from the reference's search")
        v64 = v32[b].astype(np.float64)
        if not np.array_equal(align_ref.maximum_path_each(v64, ty, tx, np.float64)[0], want):
            return False
        for _ in range(20):
            d = rs.uniform(-1, 1, v64.shape) * 2.0 ** -16 * mag[b]
            if not np.array_equal(align_ref.maximum_path_each(v64 + d, ty, tx, np.float64)[0], want):
                return False
    return True


CASES = [
    # (fixture, config, n_vocab, T_text, x_lengths, T_spec, y_lengths, weight seed)
    ("align_mini_b2", "ljs_mini_mb_istft_vits", 59, 20, [20, 11], 48, [48, 11], 1234),
    ("align_uudb_b2", "uudb_ms_istft_vits_ms", 59, 24, [24, 15], 52, [40, 52], 1234),
]


def main():
    import torch
    from mb_istft_vits_amd import synth, spec as mspec, utils as mutils
    torch.set_num_threads(4)
    tmp = tempfile.mkdtemp(prefix="mas_core_")
    try:
        core = build_core(tmp)
        models, utils, mas = import_reference(core)
        for fixture, cfg_name, n_vocab, T, xlens, Tp, ylens, wseed in CASES:
            hps = utils.get_hparams_from_file(os.path.join(REF, "configs", cfg_name + ".json"))
            net = models.SynthesizerTrn(n_vocab, hps.data.filter_length // 2 + 1,
                                        hps.train.segment_size // hps.data.hop_length,
                                        n_speakers=hps.data.n_speakers, **hps.model).eval()
            my_hps = mutils.get_hparams_from_file(mutils.builtin_config(cfg_name))
            cfg = mspec.config_from_ctor(n_vocab, my_hps.data.filter_length // 2 + 1,
                                         my_hps.train.segment_size // my_hps.data.hop_length,
                                         n_speakers=my_hps.data.n_speakers, **my_hps.model)
            sd = synth.make_state_dict(cfg, wseed)
            net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
            B = len(xlens)
            xl, yl = np.asarray(xlens, np.int64), np.asarray(ylens, np.int64)
            seed = 300
            while True:
                rs = np.random.RandomState(seed)
                x = rs.randint(1, n_vocab, size=(B, T)).astype(np.int64)
                for b in range(B):
                    x[b, xl[b]:] = 0
                y = np.abs(rs.standard_normal((B, cfg.spec_channels, Tp))).astype(np.float32) * 2.0
                for b in range(B):
                    y[b, :, yl[b]:] = 0                          # padded as the collate function pads
                sid = rs.randint(0, cfg.n_speakers, size=(B,)).astype(np.int64) if cfg.has_speaker else None
                noise = rs.standard_normal((B, cfg.inter_channels, Tp)).astype(np.float32)
                taps = run_forward(net, mas, x, xl, y, yl, sid, noise)
                if stable(taps, xl, yl, rs):
                    break
                print("  %s: input seed %d rejected (path not stable)" % (fixture, seed))
                seed += 1
            w = taps["attn"].sum(1).astype(np.int32)             # attn.sum(2) of models.py:680, [B, T_text]
            out = dict(x=x, x_lengths=xl, y=y, y_lengths=yl, noise=noise, neg_cent=taps["neg_cent"].astype(np.float32),
                       w=w, z_p=taps["z_p"], m_text=taps["m_text"], logs_text=taps["logs_text"], weight_seed=np.int64(wseed), n_vocab=np.int64(n_vocab),
                       input_seed=np.int64(seed))
            if sid is not None:
                out["sid"] = sid
            path = os.path.join(HERE, fixture + ".npz")
            np.savez_compressed(path, **out)
            print("%-14s cfg=%s input seed=%d w[0]=%s  %.0f KB" % (fixture, cfg_name, seed, w[0][:8], os.path.getsize(path) / 1024))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
