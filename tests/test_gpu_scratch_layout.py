"""The measured scratch layouts of the C API on the MI355X: every entry that measures its layout and then carves it —
`infer`, `voice_conversion`, `align`, `convert_streams`, a `convert_live` poll cycle, `infer_streams` — runs on ONE
handle at shapes that make the scratch arena grow, shrink and grow again, and every output is bitwise the same call
on a fresh handle of a second model instance with the same weights.  A layout whose measuring pass and carving pass
disagree, or a pointer that survives a reallocation, shows here."""
import numpy as np
import pytest
import torch

from mb_istft_vits_amd import _capi
from mb_istft_vits_amd.models import ConvertRequest, Request

from gpu_util import make_net

pytestmark = pytest.mark.gpu

CFG = "uudb_ms_istft_vits_ms"
MODEL_SR, HOP, WIN = 16000, 256, 1024
STEPS = [(2, 40), (3, 300), (1, 33)]           # (rows, frames): grow, grow past 256 frames, shrink
TEXT = [20, 7, 13]                             # tokens per row
CAP_F = 310                                    # max_samples of the live stream, in frames


def _seed(s):
    torch.manual_seed(s)
    torch.cuda.manual_seed(s)


def _fresh(net):
    """Drop the model's handle: the next call creates one, with empty scratch arenas."""
    if net._handle is not None:
        torch.cuda.synchronize()
        _capi.lib().mbv_destroy(net._handle)
        net._handle, net._synced_sig = None, None


def _audio(n, seed):
    rs = np.random.RandomState(seed)
    t = np.arange(n) / MODEL_SR
    x = 0.3 * np.sin(2 * np.pi * (180 + 7 * seed) * t) + 0.2 * np.sin(2 * np.pi * 1234.5 * t + seed)
    return torch.from_numpy((x + 0.05 * rs.standard_normal(n)).astype(np.float32)).cuda()


def _durations(tokens, frames):
    d = torch.full((tokens,), frames // tokens, dtype=torch.int64)
    d[:frames % tokens] += 1
    return d


def _calls(cfg, B, F, k):
    """[(name, fn(net) -> tensors)] of one step; the inputs are made once and shared by both models."""
    g = torch.Generator().manual_seed(10 + k)
    I, SC = cfg.inter_channels, cfg.spec_channels
    xl = torch.tensor(TEXT[:B])
    x = torch.randint(1, 59, (B, int(xl.max())), generator=g)
    yl = torch.tensor([F - 3 * b for b in range(B)])
    dur = torch.zeros(B, x.shape[1], dtype=torch.int64)
    for b in range(B):
        dur[b, :TEXT[b]] = _durations(TEXT[b], int(yl[b]))
    y = torch.rand(B, SC, F, generator=g)
    for b in range(B):
        y[b, :, int(yl[b]):] = 0
    sid, tgt = torch.arange(B) + 1, torch.arange(B) + 5
    x, xl, yl, dur, y, sid, tgt = (t.cuda() for t in (x, xl, yl, dur, y, sid, tgt))
    noise = torch.randn(B, I, F, generator=g).cuda()
    live_noise = torch.randn(1, I, CAP_F, generator=g).cuda()
    waves = [_audio(HOP * F + 1, k), _audio(HOP * (F - 5), 20 + k)]
    audio = [ConvertRequest(w, 1 + i, 4 + i, MODEL_SR, HOP, WIN, noise_scale=0.5 + 0.5 * i) for i, w in enumerate(waves)]
    text = [Request(x[i, :TEXT[i]] if i < B else x[0, :9], sid=2 + i, noise_scale=0.6,
                    durations=_durations(TEXT[i] if i < B else 9, F - 2 * i)) for i in range(2)]

    def infer(net):
        _seed(k)
        out = net.infer(x, xl, sid, noise_scale=0.667, durations=dur)
        assert out[0].shape[-1] == cfg.samples_per_frame * F
        return [out[0], out[5], *out[6]]

    def voice_conversion(net):
        _seed(k)
        o, o_mb, y_mask, zs = net.voice_conversion(y, yl, sid, tgt)
        return [o, o_mb, y_mask, *zs]

    def align(net):
        attn, w, x_mask, y_mask, zs = net.align(x, xl, y, yl, sid, noise_scale=0.5, noise=noise)
        return [attn, w, x_mask, y_mask, *zs]

    def streams(reqs, entry):
        def run(net):
            _seed(k)
            sts = getattr(net, entry)(reqs)
            assert [st.z.shape[2] for st in sts] == ([F, F - 5] if entry == "convert_streams" else [F, F - 2])
            return [t for st in sts for t in (st.z, st.g, st.run())]
        return run

    def convert_live(net):
        st = net.convert_live(3, 7, MODEL_SR, HOP, WIN, HOP * CAP_F, noise=live_noise, convert_frames=32)
        st.push(waves[0])
        got = [v.clone() for _, v in st.poll()]
        st.close()
        got += [v.clone() for _, v in st.poll()]
        assert st.finished and st.z_frames == F
        return got + [st.z[:, :, :F], st.result()]

    return [("infer", infer), ("voice_conversion", voice_conversion), ("align", align),
            ("convert_streams", streams(audio, "convert_streams")), ("convert_live", convert_live),
            ("infer_streams", streams(text, "infer_streams"))]


def test_every_entry_is_bitwise_a_fresh_handle_while_the_arena_grows_shrinks_and_grows():
    one, other = make_net(CFG)[0], make_net(CFG)[0]
    for k, (B, F) in enumerate(STEPS):
        for name, fn in _calls(one.cfg, B, F, k):
            got = [t.clone() if t is not None else None for t in fn(one)]
            _fresh(other)
            want = fn(other)
            assert len(got) == len(want) and len(got) >= 3, (name, B, F)
            for i, (a, b) in enumerate(zip(got, want)):
                assert (a is None) == (b is None), (name, B, F, i)
                if a is not None:
                    assert a.shape == b.shape and torch.equal(a, b), (name, B, F, i)
    _fresh(other)
