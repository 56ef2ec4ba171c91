"""The measured scratch layouts of the C API on the MI355X: every entry that measures its layout and then carves it —
`infer`, `voice_conversion`, `align`, `convert_streams`, a `convert_live` poll cycle, `infer_streams` — runs on ONE
handle at shapes that make the scratch arena grow, shrink and grow again, and every output is bitwise the same call
on a fresh handle of a second model instance with the same weights.  A layout whose measuring pass and carving pass
disagree, or a pointer that survives a reallocation, shows here.  The decoder-only entries (`dec`, the
masked and the ragged decode, `dec_stream`, a `stream_pool` step) run the same way on three decoder types, under
every option that changes what the decoder's layout holds."""
import numpy as np
import pytest
import torch

from mb_istft_vits_amd import _capi
from mb_istft_vits_amd.models import ConvertRequest, Request
from mb_istft_vits_amd import utils as mutils

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


# ---------------------------------------------------------------------------------------------------------------
# The decoder-only entries, whose scratch is measured and carved like the others': `dec`, the masked decode (the
# run `infer` makes: the one that "trim" and "tail_once" act on), the ragged decode, a `dec_stream` drained to the end
# and one `stream_pool` step — under every option that changes what the decoder's layout holds.
RB2 = {"resblock": "2", "resblock_dilation_sizes": [[1, 3], [1, 3], [1, 3]]}
DEC_CONFIGS = [("uudb_ms_istft_vits_ms", None), ("ljs_mini_istft_vits", None), ("ljs_mini_mb_istft_vits", RB2)]
# x_post of one row of 300 frames is 1.38 MB in every decoder type: two rows per sub-batch, so three rows run in two
OPTIONS = [{}, {"trim": 1}, {"tail_once": 2}, {"dec_streams": 0}, {"xpost_chunk_bytes": 2_800_000}]
REFUSAL = b"scratch layout exceeds its buffer"


def _dec_calls(cfg, B, F, k, trim):
    g_ = torch.Generator().manual_seed(40 + k)
    spf = cfg.samples_per_frame
    z = torch.randn(B, cfg.inter_channels, F, generator=g_).cuda()
    g = torch.randn(B, cfg.gin_channels, 1, generator=g_).cuda() if cfg.gin_channels else None
    lens = [F, 9, 41][:B]                          # both sides of a class cut (17 frames at us = 4, 33 at us = 8)
    short = max(9, F - 7)

    def dec(net):
        return list(net.dec(z, g))

    def masked(net):
        o = torch.zeros(B, 1, spf * F, device=z.device)
        net._decode_masked_into(z, g, lens, (o, None, None, None))
        # ("trim" leaves what lies behind a row's length to the caller)
        return [o[b, :, :spf * n] for b, n in enumerate(lens)] if trim else [o]

    def ragged(net):
        return [net.dec(z, g, lengths=lens)[0]]

    def stream(net):
        return [net.dec_stream(z[:1], None if g is None else g[:1]).run()]

    def pool(net):
        p = net.stream_pool()
        p.add(net.dec_stream(z[:1], None if g is None else g[:1]))
        p.add(net.dec_stream(z[-1:, :, :short].contiguous(), None if g is None else g[-1:]))
        got = p.step()
        assert len(got) == 2
        return [v.clone() for _, _, v in got]

    calls = [("dec", dec), ("masked", masked), ("stream", stream)]
    return calls if trim else calls + [("ragged", ragged), ("pool", pool)]     # (the ragged modes refuse "trim")


_DEC_NETS = {}                                     # config id -> (one, other, other's packed weights): one handle for
                                                   # every option of a config, in the order of OPTIONS.  (A case
                                                   # run alone is the same check, bitwise against a fresh handle,
                                                   # on an arena with a shorter history.)


def _dec_nets(name, overrides):
    key = name + ("_rb2" if overrides else "")
    if key not in _DEC_NETS:
        one, other = make_net(name, overrides=overrides)[0], make_net(name, overrides=overrides)[0]
        # (a fresh handle of `other` takes its weights from the exported arena: no fold, no upload)
        _DEC_NETS[key] = (one, other, other.export_arena())
    return _DEC_NETS[key]


# ("trim": multiband / multistream only)
DEC_CASES = [(n, ov, i) for n, ov in DEC_CONFIGS for i, opt in enumerate(OPTIONS)
             if not ("trim" in opt and mutils.get_hparams_from_file(mutils.builtin_config(n)).model["istft_vits"])]


@pytest.mark.parametrize("name, overrides, which", DEC_CASES,
                         ids=["%s%s-%s" % (n, "_rb2" if ov else "", "-".join(OPTIONS[i]) or "default") for n, ov, i in DEC_CASES])
def test_decoder_entries_are_bitwise_a_fresh_handle_under_every_option(name, overrides, which):
    one, other, arena = _dec_nets(name, overrides)
    L, opt = _capi.lib(), OPTIONS[which]
    defaults = {k: L.mbv_get_option(one._ensure_handle(), k.encode()) for k in ("trim", "tail_once", "dec_streams")}
    defaults["xpost_chunk_bytes"] = 0
    for k, v in opt.items():
        one.set_option(k, v)
    try:
        for step, (B, F) in enumerate(STEPS):
            for what, fn in _dec_calls(one.cfg, B, F, step, "trim" in opt):
                got = [t.clone() if t is not None else None for t in fn(one)]
                assert REFUSAL not in L.mbv_last_error(one._handle), (opt, what, B, F)
                _fresh(other)
                other.import_arena(arena)
                for k, v in opt.items():
                    other.set_option(k, v)
                want = fn(other)
                assert REFUSAL not in L.mbv_last_error(other._handle), (opt, what, B, F)
                assert len(got) == len(want) and got[0] is not None, (opt, what, B, F)
                for i, (a, b) in enumerate(zip(got, want)):
                    assert (a is None) == (b is None), (opt, what, B, F, i)
                    if a is not None:
                        assert a.shape == b.shape and torch.equal(a, b), (opt, what, B, F, i)
        if "trim" in opt:                            # why _dec_calls drops the ragged and the pooled call here
            z = torch.zeros(1, one.cfg.inter_channels, 20, device="cuda")
            with pytest.raises(_capi.MbvError, match="trim"):
                one.dec(z, lengths=[20])
            pool = one.stream_pool()
            pool.add(one.dec_stream(z))
            with pytest.raises(_capi.MbvError, match="trim"):
                pool.step()
    finally:
        for k in opt:
            one.set_option(k, defaults[k])
        _fresh(other)


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
