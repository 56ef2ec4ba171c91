"""Seeded device noise on the MI355X: `mbv_randn_blocks` / `net.randn` against the float64 restatement
of tests/rng_ref.py, the table launch against single-block launches, and `seed=` end to end: bitwise today's path on
materialised noise, repeatable, independent of order and company, and neither torch generator touched."""
import ctypes as C

import numpy as np
import pytest
import torch

import rng_ref
from mb_istft_vits_amd import _capi
from mb_istft_vits_amd.models import ConvertRequest, Request

from gpu_util import make_net

pytestmark = pytest.mark.gpu

# |n| <= sqrt(2 * 24 * ln 2) = 5.77; fp32 logf, sqrtf and sincospif are each good to a few ulp: below about 3e-6 of the
# float64 transform.  1e-5 leaves 3x over that and is five orders below what a wrong word or lane produces.
TOL = 1e-5
NETS = {"mini": ("ljs_mini_mb_istft_vits", None), "sdp": ("ljs_mini_mb_istft_vits", {"use_sdp": True}),
        "uudb": ("uudb_ms_istft_vits_ms", None)}
SR, HOP, WIN = 22050, 256, 1024
_NETS = {}


def _net(key):
    if key not in _NETS:
        name, overrides = NETS[key]
        _NETS[key] = make_net(name, overrides=overrides)[0]
    return _NETS[key]


def _ids(T, seed):
    return torch.randint(1, 59, (T,), generator=torch.Generator().manual_seed(seed))


def _batch(lengths, seed):
    x = torch.zeros(len(lengths), max(lengths), dtype=torch.int64)
    for b, T in enumerate(lengths):
        x[b, :T] = _ids(T, seed + b)
    return x.cuda(), torch.tensor(lengths).cuda()


def _audio(seconds, seed):
    n = int(round(seconds * SR))
    rs = np.random.RandomState(seed)
    t = np.arange(n) / SR
    x = 0.3 * np.sin(2 * np.pi * (180 + 7 * seed) * t) + 0.2 * np.sin(2 * np.pi * 1234.5 * t + seed)
    return torch.from_numpy((x + 0.05 * rs.standard_normal(n)).astype(np.float32))


def _rng_states():
    return torch.get_rng_state().clone(), torch.cuda.get_rng_state().clone()


def _states_equal(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    """z, g, y_lengths and schedule of two streams, bitwise."""
    if a.z.shape != b.z.shape or not torch.equal(_bits(a.z), _bits(b.z)):
        return False
    if (a.g is None) != (b.g is None) or (a.g is not None and not torch.equal(_bits(a.g), _bits(b.g))):
        return False
    return torch.equal(a.y_lengths, b.y_lengths) and a.schedule == b.schedule


def _fill(net, blocks):
    """`mbv_randn_blocks` directly: blocks = [(address, stride, channels, first, count, seed, purpose, row)] -> rc."""
    arr = (_capi.MbvRandnBlock * max(len(blocks), 1))()
    for k, (dst, stride, channels, first, count, seed, purpose, row) in zip(arr, blocks):
        k.dst, k.stride, k.channels, k.first, k.count = dst, stride, channels, first, count
        k.seed, k.purpose, k.row = seed, purpose, row
    h = net._ensure_handle()
    with torch.cuda.device(net._device()):
        return _capi.lib().mbv_randn_blocks(h, arr, len(blocks), net._stream())


# ---------------------------------------------------------------------------------------------- 5: the values
def test_device_values_match_the_reference():
    net = _net("mini")
    L = _capi.lib()
    worst = worst_host = 0.0
    cases = [(0, 0, 0, 4, 64, 0), (1234, 0, 0, 5, 9, 8), (1234, 1, 7, 2, 133, 5), (2 ** 64 - 1, 2, 3, 192, 9, 3),
             (2 ** 63 + 5, 2, 2 ** 32 - 1, 3, 70, 1), (77, 0, 1, 1, 1, (1 << 30) - 1)]
    for seed, purpose, row, channels, frames, first in cases:
        got = net.randn(seed, channels, frames, purpose=purpose, row=row, first=first)
        assert got.shape == (channels, frames) and got.dtype == torch.float32 and got.is_cuda
        got = got.cpu().numpy()
        ref = rng_ref.randn(seed, channels, frames, purpose=purpose, row=row, first=first)
        err = float(np.abs(got.astype(np.float64) - ref).max())
        host = np.empty((channels, frames), dtype=np.float32)
        for c in range(channels):
            assert L.mbv_randn_host(seed, purpose, row, c, first, frames, C.c_void_p(host[c].ctypes.data)) == 0
        err_host = float(np.abs(got.astype(np.float64) - host).max())
        worst, worst_host = max(worst, err), max(worst_host, err_host)
        print("randn seed %d purpose %d row %d [%d, %d] first %d: max abs err vs float64 %.3e, vs host entry %.3e"
              % (seed, purpose, row, channels, frames, first, err, err_host))
        assert err < TOL and err_host < TOL, (seed, purpose, row, channels, frames, first, err, err_host)
    print("device generator: max abs err vs float64 reference %.3e, vs mbv_randn_host %.3e" % (worst, worst_host))
    # the worked draw of the specification
    got = net.randn(1234, 4, 4, first=8)[3].cpu().numpy()
    assert np.abs(got - [-0.10601855956, -0.12388860715, 0.29930284658, -0.99568311786]).max() < TOL


# ---------------------------------------------------------------------------------------------- 6: the table launch
def test_table_of_70_blocks_is_every_block_alone():
    net = _net("mini")
    counts, firsts, chans = [0, 1, 3, 4, 5, 9, 133], [0, 1, 2, 3, 5], [1, 2, 192]
    blocks, off = [], 3                                # (offset in floats, ...); the first block starts off alignment
    for i in range(70):
        count, first, channels = counts[i % 7], firsts[i % 5], chans[i % 3]
        stride = count + (0, 1, 6)[(i // 2) % 3]       # stride > count in two cases of three
        blocks.append((off, stride, channels, first, count, 1000 + i, i % 3, i % 4))
        off += channels * stride + (1 if i % 5 == 4 else 0)      # back to back, now and then one float between
    total = off + 5
    assert {(b[4], b[3]) for b in blocks} >= {(133, f) for f in firsts} and any(b[1] > b[4] > 0 for b in blocks)
    assert sum(1 for b in blocks if b[4] >= 4 and b[0] % 4 == 0) >= 3 and sum(1 for b in blocks if b[0] % 4) >= 30
    sentinel = 12345.0
    table = torch.full((total,), sentinel, device="cuda", dtype=torch.float32)
    alone = torch.full((total,), sentinel, device="cuda", dtype=torch.float32)
    torch.cuda.synchronize()
    runs = net.noise_runs()
    assert _fill(net, [(table.data_ptr() + 4 * b[0],) + b[1:] for b in blocks]) == 0
    assert net.noise_runs() == runs + 1
    for b in blocks:
        assert _fill(net, [(alone.data_ptr() + 4 * b[0],) + b[1:]]) == 0
    assert net.noise_runs() == runs + 1 + sum(1 for b in blocks if b[4] > 0)      # an empty block launches nothing
    assert torch.equal(_bits(table), _bits(alone))
    got = table.cpu().numpy()
    written = np.zeros(total, dtype=bool)
    worst = 0.0
    for o, stride, channels, first, count, seed, purpose, row in blocks:
        if count == 0:
            continue
        ref = rng_ref.randn(seed, channels, count, purpose=purpose, row=row, first=first)
        for c in range(channels):
            a = o + c * stride
            worst = max(worst, float(np.abs(got[a:a + count].astype(np.float64) - ref[c]).max()))
            written[a:a + count] = True
    print("table of 70 blocks: max abs err vs float64 reference %.3e" % worst)
    assert worst < TOL
    assert (got[~written] == np.float32(sentinel)).all() and (~written).sum() > 70


def test_block_refusals_launch_nothing():
    net = _net("mini")
    buf = torch.full((64,), 5.0, device="cuda")
    p = buf.data_ptr()
    runs = net.noise_runs()
    good = (p, 8, 2, 0, 8, 1, 0, 0)
    bad = [(None, 8, 2, 0, 8, 1, 0, 0),                # a null dst with count > 0
           (p, 7, 2, 0, 8, 1, 0, 0),                   # stride < count
           (p, 8, 0, 0, 8, 1, 0, 0),                   # channels < 1
           (p, 8, 1, (1 << 30) - 7, 8, 1, 0, 0),       # first + count > 2^30
           (p, 8, 2, 0, 8, 1, 3, 0),                   # purpose > 2
           (p, 8, 2, -1, 8, 1, 0, 0), (p, 8, 2, 0, -1, 1, 0, 0)]
    h = net._ensure_handle()
    for b in bad:
        assert _fill(net, [good, b]) != 0, b
        assert b"block 1" in _capi.lib().mbv_last_error(h)
    assert _fill(net, []) != 0                          # n < 1
    assert _fill(net, [(None, 0, 1, 5, 0, 1, 0, 0)]) == 0      # count 0 is legal and writes nothing
    torch.cuda.synchronize()
    assert net.noise_runs() == runs and bool((buf == 5.0).all())


# ---------------------------------------------------------------------------------------------- 7: the range rule
@pytest.mark.parametrize("a,b", [(1, 2), (3, 9), (6, 8), (5, 70)])
def test_a_range_is_the_slice_of_the_fill_from_zero(a, b):
    net = _net("mini")
    for channels, purpose, row in ((1, 0, 0), (3, 1, 2), (192, 2, 5)):
        whole = net.randn(99, channels, b, purpose=purpose, row=row)
        part = net.randn(99, channels, b - a, purpose=purpose, row=row, first=a)
        assert torch.equal(_bits(part), _bits(whole[:, a:])), (a, b, channels)


# ---------------------------------------------------------------------------------------------- 8: the row rule
def test_row_rule_of_the_batched_entries():
    """B = 3, I = 192, T' = 9 (three tokens of three frames each, given as durations)."""
    net = _net("mini")
    I, B, Tp = net.cfg.inter_channels, 3, 9
    assert I == 192
    x, xl = _batch([3, 3, 3], 40)
    d = torch.full((B, 3), 3, dtype=torch.int64).cuda()
    h = net._ensure_handle()
    for seed, rows in ((21, [(21, 0), (21, 1), (21, 2)]), ([31, 32, 33], [(31, 0), (32, 0), (33, 0)]),
                       (torch.tensor([31, 32, 33]), [(31, 0), (32, 0), (33, 0)])):
        want = torch.stack([net.randn(s, I, Tp, row=r) for s, r in rows])
        with torch.cuda.device(net._device()):
            drawn = net._seeded_rows(h, net_row_seeds(seed, B), I, Tp, _capi.NOISE_PRIOR)     # what `_run` draws
        assert torch.equal(_bits(drawn), _bits(want))
        out = net.infer(x, xl, durations=d, seed=seed, outputs=("z_p", "m_p", "logs_p"))
        z_p, m_p, logs_p = out[6][1], out[6][2], out[6][3]
        assert z_p.shape == (B, I, Tp)
        # z_p = m_p + noise * exp(logs_p) (models.py:729): the noise `infer` used, up to the rounding of that line
        used = (z_p.double() - m_p.double()) * torch.exp(-logs_p.double())
        scale = float((m_p.abs() * torch.exp(-logs_p)).max()) + 6.0
        assert float((used - want.double()).abs().max()) < 16 * 2.0 ** -24 * scale
        # and another row's sub-stream is another draw
        assert float((used[0] - want[1].double()).abs().max()) > 0.1


def net_row_seeds(seed, B):
    from mb_istft_vits_amd.models import _row_seeds
    return _row_seeds(seed, B)


# ---------------------------------------------------------------------------------------------- 9: end to end
def _infer_materialised(net, x, xl, sid, noise_of, noise_w, noise_scale=1.0, length_scale=1.0, noise_scale_w=1.0):
    """`mbv_encode` + `mbv_synthesize` as `_run` calls them, on noise the caller materialised: noise_w [B, 2, T] or
    None, noise_of(T') -> [B, inter, T'].  -> the eight outputs of `infer` (without timings) and y_lengths."""
    h = net._ensure_handle()
    dev = net._device()
    B, T = x.shape
    I = net.cfg.inter_channels
    f32 = dict(device=dev, dtype=torch.float32)
    with torch.cuda.device(dev), torch.no_grad():
        y_lengths = torch.empty(B, dtype=torch.int64, device=dev)
        net._launch(h, "mbv_encode", x, xl, sid, B, T, float(length_scale), noise_w, float(noise_scale_w), y_lengths)
        Tp = int(y_lengths.max())
        noise = noise_of(Tp).contiguous()
        t = dict(attn=torch.empty(B, 1, Tp, T, **f32), y_mask=torch.empty(B, 1, Tp, **f32))
        for k in ("z", "z_p", "m_p", "logs_p"):
            t[k] = torch.empty(B, I, Tp, **f32)
        t["o"], t["o_mb"], t["spec"], t["phase"] = net._alloc_decoder_outputs(B, Tp, dev)
        out = _capi.MbvOutputs()
        for k, v in t.items():
            if v is not None:
                setattr(out, k, v.data_ptr())
        net._launch(h, "mbv_synthesize", Tp, noise, float(noise_scale), 0, C.byref(out))
    return t, y_lengths


_NAMES = ("o", "o_mb", "spec", "phase", "attn", "y_mask")


def _assert_outputs_equal(out, t):
    for k, v in zip(_NAMES, out[:6]):
        assert (v is None) == (t[k] is None), k
        if v is not None:
            assert v.shape == t[k].shape and torch.equal(_bits(v), _bits(t[k])), k
    for k, v in zip(("z", "z_p", "m_p", "logs_p"), out[6]):
        assert torch.equal(_bits(v), _bits(t[k])), k


@pytest.mark.parametrize("key", ["sdp", "uudb"])
def test_seeded_infer_is_todays_path_on_materialised_noise(key):
    net = _net(key)
    I = net.cfg.inter_channels
    lengths = [7, 300]
    x, xl = _batch(lengths, 3)
    B, T = x.shape
    sid = torch.tensor([2, 9]).cuda() if net.n_speakers else None
    for seed, rows in ((5, [(5, 0), (5, 1)]), ([8, 9], [(8, 0), (9, 0)])):
        noise_w = None
        if net.cfg.use_sdp:
            noise_w = torch.stack([net.randn(s, 2, T, purpose=1, row=r) for s, r in rows])
        runs = net.noise_runs()
        out = net.infer(x, xl, sid, noise_scale=0.667, length_scale=1.1, noise_scale_w=0.8, seed=seed)
        assert net.noise_runs() == runs + (2 if net.cfg.use_sdp else 1)      # one launch per noise tensor
        t, y_lengths = _infer_materialised(
            net, x, xl, sid, lambda Tp: torch.stack([net.randn(s, I, Tp, row=r) for s, r in rows]), noise_w,
            noise_scale=0.667, length_scale=1.1, noise_scale_w=0.8)
        _assert_outputs_equal(out, t)
        # repeatable; another seed is another z
        again = net.infer(x, xl, sid, noise_scale=0.667, length_scale=1.1, noise_scale_w=0.8, seed=seed)
        _assert_outputs_equal(again, t)
        other = net.infer_z_only(x, xl, sid, noise_scale=0.667, length_scale=1.1, noise_scale_w=0.8,
                                 seed=6 if isinstance(seed, int) else [8, 10])
        z_other = other[2][0]
        assert z_other.shape != t["z"].shape or not torch.equal(z_other, t["z"])
        lens = net.infer_with_lengths(x, xl, sid, noise_scale=0.667, length_scale=1.1, noise_scale_w=0.8, seed=seed,
                                      outputs=("z_p",))[1]
        assert torch.equal(lens, y_lengths)
    if net.cfg.use_sdp:
        # the SDP draw through `_run`'s existing noise_w=: at noise_scale 0 the prior draw is not read
        noise_w = torch.stack([net.randn(5, 2, T, purpose=1, row=b) for b in range(B)])
        a = net._run(x, xl, sid, 0.0, 1.0, None, decode=True, noise_scale_w=0.8, noise_w=noise_w)
        b = net.infer(x, xl, sid, noise_scale=0.0, length_scale=1.0, noise_scale_w=0.8, seed=5)
        for u, v in zip(a[:6], b[:6]):
            assert (u is None) == (v is None) and (u is None or torch.equal(_bits(u), _bits(v)))
        assert torch.equal(_bits(a[6][0]), _bits(b[6][0]))


def _spec(net, seconds, seed, B=1):
    wave = torch.stack([_audio(seconds, seed + b) for b in range(B)]).cuda()
    return net.spectrogram(wave, 2 * (net.cfg.spec_channels - 1), HOP, WIN)


def test_generators_are_untouched_and_calls_repeat():
    net = _net("uudb")
    sdp = _net("sdp")
    x, xl = _batch([7, 30], 11)
    sid = torch.tensor([1, 4]).cuda()
    y, yl = _spec(net, 0.5, 3, B=2)
    torch.manual_seed(123)
    torch.cuda.manual_seed(123)
    before = _rng_states()
    a = net.infer(x, xl, sid, seed=3, outputs=("o", "z"))
    b = sdp.infer(x, xl, seed=[3, 4], outputs=("o", "z"))
    vc = net.voice_conversion(y, yl, sid, torch.tensor([5, 6]).cuda(), seed=17)
    al = net.align(x[:, :7], torch.tensor([7, 7]).cuda(), y, yl, sid, seed=[17, 18])
    reqs = [Request(_ids(9, 1), sid=2, seed=1), Request(_ids(300, 2), sid=3, seed=2)]
    st = net.infer_streams(reqs)
    st2 = sdp.infer_streams([Request(_ids(9, 1), seed=1), Request(_ids(300, 2), seed=2)])
    cr = [ConvertRequest(_audio(0.3, 1), 1, 2, SR, HOP, WIN, seed=4), ConvertRequest(_audio(3.5, 2), 3, 4, SR, HOP, WIN, seed=5)]
    cs = net.convert_streams(cr)
    torch.cuda.synchronize()
    assert _states_equal(before, _rng_states())
    # the same calls again give the same bits
    assert torch.equal(_bits(a[0]), _bits(net.infer(x, xl, sid, seed=3, outputs=("o", "z"))[0]))
    assert torch.equal(_bits(b[0]), _bits(sdp.infer(x, xl, seed=[3, 4], outputs=("o", "z"))[0]))
    vc2 = net.voice_conversion(y, yl, sid, torch.tensor([5, 6]).cuda(), seed=17)
    assert torch.equal(_bits(vc[0]), _bits(vc2[0])) and torch.equal(_bits(vc[3][0]), _bits(vc2[3][0]))
    assert not torch.equal(vc[3][0], net.voice_conversion(y, yl, sid, torch.tensor([5, 6]).cuda(), seed=18)[3][0])
    al2 = net.align(x[:, :7], torch.tensor([7, 7]).cuda(), y, yl, sid, seed=[17, 18])
    assert torch.equal(_bits(al[4][0]), _bits(al2[4][0])) and torch.equal(al[1], al2[1])
    # voice_conversion's posterior draw is purpose 2 at (seed, row b): align given that noise has the same z
    I, T = net.cfg.inter_channels, y.shape[2]
    noise = torch.stack([net.randn(17, I, T, purpose=2, row=0), net.randn(18, I, T, purpose=2, row=0)])
    al3 = net.align(x[:, :7], torch.tensor([7, 7]).cuda(), y, yl, sid, noise=noise)
    assert torch.equal(_bits(al[4][0]), _bits(al3[4][0]))
    for u, v in zip(st + st2 + cs, net.infer_streams(reqs) + sdp.infer_streams([Request(_ids(9, 1), seed=1),
                                                                                 Request(_ids(300, 2), seed=2)])
                    + net.convert_streams(cr)):
        assert _same(u, v)
    assert _states_equal(before, _rng_states())


@pytest.mark.parametrize("key", ["mini", "sdp", "uudb"])
def test_streams_do_not_depend_on_order_or_company(key):
    net = _net(key)
    lengths = [7, 300, 40, 257]
    assert net.admit_plan(lengths)[0] == 2
    reqs = [Request(_ids(T, 60 + k), sid=(3 * k + 1) % net.n_speakers if net.n_speakers else None,
                    noise_scale=(0.667, 1.0)[k % 2], length_scale=(1.0, 1.2)[k // 2], noise_scale_w=0.8,
                    chunk_frames=(32, 8)[k % 2], max_chunk_frames=(256, 32)[k % 2], seed=11 + k)
            for k, T in enumerate(lengths)]
    runs = net.noise_runs()
    fwd = net.infer_streams(reqs)
    assert net.noise_runs() == runs + (2 if net.cfg.use_sdp else 1)      # across both classes
    rev = net.infer_streams(reqs[::-1])[::-1]
    for k, r in enumerate(reqs):
        alone = net.infer_streams([r])[0]
        sid = torch.tensor([r.sid]).cuda() if r.sid is not None else None
        solo = net.infer_stream(r.x[None].cuda(), torch.tensor([r.x.numel()]).cuda(), sid, r.noise_scale, r.length_scale,
                                r.noise_scale_w, r.max_len, r.chunk_frames, r.max_chunk_frames, seed=[r.seed])
        for other in (rev[k], alone, solo):
            assert _same(fwd[k], other), (key, k)
    assert not torch.equal(fwd[0].z, net.infer_streams([Request(reqs[0].x, sid=reqs[0].sid, noise_scale=0.667,
                                                                noise_scale_w=0.8, seed=12)])[0].z)


def test_converted_streams_do_not_depend_on_order_or_company():
    net = _net("uudb")
    n_fft = 2 * (net.cfg.spec_channels - 1)
    reqs = [ConvertRequest(_audio(0.3, 1), 1, 2, SR, HOP, WIN, seed=21, chunk_frames=8, max_chunk_frames=32),
            ConvertRequest(_audio(3.5, 2).cuda(), 3, 4, SR, HOP, WIN, seed=22)]
    frames = [r.frames(n_fft) for r in reqs]
    assert frames[0] < 256 < frames[1]
    runs = net.noise_runs()
    fwd = net.convert_streams(reqs)
    assert net.noise_runs() == runs + 1
    rev = net.convert_streams(reqs[::-1])[::-1]
    for k, r in enumerate(reqs):
        alone = net.convert_streams([r])[0]
        solo = net.convert_stream(r.wave, r.sid_src, r.sid_tgt, SR, HOP, WIN, chunk_frames=r.chunk_frames,
                                  max_chunk_frames=r.max_chunk_frames, seed=[r.seed])
        for other in (rev[k], alone, solo):
            assert _same(fwd[k], other), k
    # the posterior draw is purpose 2, row 0: the stream on that noise, materialised
    r = reqs[1]
    noise = net.randn(22, net.cfg.inter_channels, frames[1], purpose=2).unsqueeze(0)
    assert _same(fwd[1], net.convert_stream(r.wave, r.sid_src, r.sid_tgt, SR, HOP, WIN, noise=noise))


@pytest.mark.parametrize("key", ["mini", "sdp"])
def test_seeded_and_unseeded_requests_mix(key):
    net = _net(key)
    kw = dict(noise_scale=0.667, noise_scale_w=0.8)
    reqs = [Request(_ids(7, 1), seed=31, **kw), Request(_ids(300, 2), **kw), Request(_ids(40, 3), seed=33, **kw)]

    def solo(r):
        return net.infer_stream(r.x[None].cuda(), torch.tensor([r.x.numel()]).cuda(), None, r.noise_scale, r.length_scale,
                                r.noise_scale_w, seed=None if r.seed is None else [r.seed])

    torch.manual_seed(0)
    torch.cuda.manual_seed(0)
    runs = net.noise_runs()
    got = net.infer_streams(reqs)
    assert net.noise_runs() == runs + (2 if net.cfg.use_sdp else 1)
    after = _rng_states()
    torch.manual_seed(0)
    torch.cuda.manual_seed(0)
    assert _same(got[1], solo(reqs[1]))
    assert _states_equal(after, _rng_states())          # the generators moved as that one unseeded call moves them
    assert _same(got[0], solo(reqs[0])) and _same(got[2], solo(reqs[2]))


def test_live_conversion_is_the_seeded_one_shot():
    net = _net("uudb")
    wave = _audio(3.5, 7).cuda()
    cap = wave.numel() + 5000                            # the capacity block is longer than the recording
    ref = net.convert_stream(wave, 3, 7, SR, HOP, WIN, seed=[41])
    assert ref.z.shape[2] > 256
    want = [(a, v.clone()) for a, v in ref]
    before = _rng_states()
    for piece in (400, wave.numel()):
        runs = net.noise_runs()
        st = net.convert_live(3, 7, SR, HOP, WIN, cap, seed=41)
        assert net.noise_runs() == runs + 1
        got = []
        for off in range(0, wave.numel(), piece):
            st.push(wave[off:off + piece])
            got += [(a, v.clone()) for a, v in st.poll()]
        st.close()
        got += [(a, v.clone()) for a, v in st.poll()]
        assert st.finished and net.noise_runs() == runs + 1
        assert [(a, v.shape[-1]) for a, v in got] == [(a, v.shape[-1]) for a, v in want]
        for (a, v), (_, w) in zip(got, want):
            assert torch.equal(_bits(v), _bits(w)), (piece, a)
    assert _states_equal(before, _rng_states())


def test_seed_refusals():
    net = _net("uudb")
    x, xl = _batch([7, 9], 1)
    sid = torch.tensor([1, 2]).cuda()
    y, yl = _spec(net, 0.3, 1, B=2)
    I = net.cfg.inter_channels
    noise = torch.zeros(2, I, y.shape[2]).cuda()
    torch.cuda.synchronize()
    runs = net.noise_runs()
    with pytest.raises(ValueError):
        net.align(x[:, :7], torch.tensor([7, 7]).cuda(), y, yl, sid, noise=noise, seed=1)
    wave = _audio(0.3, 1)
    with pytest.raises(ValueError):
        net.convert_stream(wave, 1, 2, SR, HOP, WIN, noise=noise[:1], seed=1)
    with pytest.raises(ValueError):
        net.convert_live(1, 2, SR, HOP, WIN, 20000, noise=noise[:1], seed=1)
    for bad in ([1], [1, 2, 3], torch.tensor([1, 2, 3])):
        with pytest.raises(ValueError):
            net.infer(x, xl, sid, seed=bad)
        with pytest.raises(ValueError):
            net.voice_conversion(y, yl, sid, sid, seed=bad)
        with pytest.raises(ValueError):
            net.align(x[:, :7], torch.tensor([7, 7]).cuda(), y, yl, sid, seed=bad)
    for bad in (1.5, True, [1, 2.5]):
        with pytest.raises(TypeError):
            net.infer(x, xl, sid, seed=bad)
    with pytest.raises(ValueError):
        net.infer(x, xl, sid, seed=-1)
    with pytest.raises(ValueError):
        net.convert_stream(wave, 1, 2, SR, HOP, WIN, seed=[1, 2])
    assert net.noise_runs() == runs
