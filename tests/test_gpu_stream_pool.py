"""Pooled streaming decode on the MI355X: `net.stream_pool()` / `mbv_decode_chunks` decode the next chunk of many
streams in shared launches, every stored sample bitwise what the stream yields alone and what the one-shot decode
of its utterance holds there."""
import warnings

import pytest
import torch

from mb_istft_vits_amd import _capi, synth, wire

from gpu_util import make_net

pytestmark = pytest.mark.gpu

RB2 = {"resblock": "2", "resblock_dilation_sizes": [[1, 3], [1, 3], [1, 3]]}
CASES = [("ljs_mini_mb_istft_vits", None), ("ljs_ms_istft_vits", None), ("uudb_ms_istft_vits_ms", None),
         ("ljs_mini_istft_vits", None), ("ljs_mini_mb_istft_vits", RB2)]
IDS = ["mini_mb", "ms", "uudb", "sb", "rb2"]
T_MAX = 300
SENTINEL = -7.5
# (chunk_frames, max_chunk_frames), dealt round the streams
SCHEDULES = [(32, 256), (8, 32), (16, 64), (5, 40), (24, 24), (64, 256), (12, 96)]
_NETS = {}


@pytest.fixture(scope="module", params=CASES, ids=IDS)
def net(request):
    name, overrides = request.param
    return _net(name, overrides)


def _net(name, overrides=None):
    key = (name, repr(overrides))
    if key not in _NETS:
        _NETS[key] = make_net(name, overrides=overrides)[0]
    return _NETS[key]


def _z(net, Tp, seed):
    return torch.randn(1, net.cfg.inter_channels, Tp, generator=torch.Generator().manual_seed(seed)).cuda()


def _g(net, seed):
    if not net.cfg.gin_channels:
        return None
    return (0.3 * torch.randn(1, net.cfg.gin_channels, 1, generator=torch.Generator().manual_seed(seed))).cuda()


def _lengths(net):
    """Both sides of every class cut, 1, 9, 41, T_MAX and one utterance above 600 frames; not sorted."""
    first = net.ragged_classes(T_MAX)
    lens = [T_MAX, 1, 9, 41, 641]
    for f in first[1:]:
        lens += [f, f - 1]
    lens = sorted(set(lens), reverse=True)
    assert len(lens) >= 9 and len({max(i for i, f in enumerate(first) if f <= n) for n in lens}) == len(first)
    return lens[1::2] + lens[0::2]


class Case:
    """One utterance: its z, g, one-shot waveform and the chunks a stream of its own yields alone."""

    def __init__(self, net, Tp, k, seed):
        self.Tp, (self.chunk, self.cap) = Tp, SCHEDULES[k % len(SCHEDULES)]
        self.z, self.g = _z(net, Tp, seed + k), _g(net, seed + 100 + k)
        self.full = net.dec(self.z, self.g)[0].clone()
        self.solo = [(a, v.clone()) for a, v in net.dec_stream(self.z, self.g, self.chunk, self.cap)]

    def stream(self, net, z=None):
        st = net.dec_stream(self.z if z is None else z, self.g, self.chunk, self.cap)
        st.o.fill_(SENTINEL)
        return st


def _cases(net, seed=20):
    return [Case(net, Tp, k, seed) for k, Tp in enumerate(_lengths(net))]


def _step(net, pool, streams=None):
    """One pool.step() whose decoder runs are those `mbv_chunks_plan` names for the streams it advanced."""
    before = net.decoder_runs()
    out = pool.step(streams)
    if out:
        assert net.decoder_runs() - before == net.chunks_plan([st.z.shape[2] for st, _, _ in out])[0]
    else:
        assert net.decoder_runs() == before
    return out


@pytest.mark.timeout(900)
def test_pooled_chunks_are_bitwise_the_streams_alone(net):
    cases = _cases(net)
    assert all(torch.equal(torch.cat([v for _, v in c.solo], dim=2), c.full) for c in cases)     # (§7.3, the yardstick)
    sts = [c.stream(net) for c in cases]
    case_of = {id(st): c for st, c in zip(sts, cases)}
    seen = {id(st): 0 for st in sts}
    pool = net.stream_pool()
    waves = [sts[0::3], sts[1::3], sts[2::3]]                  # added before the first, the second and the fourth step
    steps = 0
    while waves or len(pool):
        if waves and steps in (0, 1, 3):
            for st in waves.pop(0):
                pool.add(st)
        out = _step(net, pool)
        steps += 1
        assert out, "a pool with unfinished streams decoded nothing"
        for st, a, view in out:
            c, k = case_of[id(st)], seen[id(st)]
            a_solo, v_solo = c.solo[k]
            assert a == a_solo and view.shape == v_solo.shape
            assert torch.equal(view, v_solo), (c.Tp, k, float((view - v_solo).abs().max()))
            seen[id(st)] += 1
    assert len(pool) == 0 and pool.step() == []
    for st, c in zip(sts, cases):
        assert seen[id(st)] == len(st) == len(c.solo)
        assert torch.equal(st.o, c.full), c.Tp
        with pytest.raises(StopIteration):                      # the pool's chunks are handed out, then the stream ends
            for _ in range(len(st) + 1):
                next(st)
    # fewer decoder runs than streams, which is the point
    assert steps < sum(len(st) for st in sts)
    print("%d streams, %d chunks in %d pooled steps" % (len(sts), sum(len(st) for st in sts), steps))


@pytest.mark.timeout(900)
def test_one_step_writes_its_chunks_only_and_reads_its_windows_only(net):
    cases = _cases(net, seed=40)
    Lc, Rc = net.decoder_context()
    # a larger pool through the arena first
    big = net.stream_pool()
    for k in range(len(cases) + 3):
        big.add(net.dec_stream(_z(net, 700, 90 + k), _g(net, 95 + k), 128, 256))
    big.step()
    for fill in (float("nan"), 1e30):
        sts = [c.stream(net, c.z.clone()) for c in cases]
        for k, st in enumerate(sts):                           # streams at different places of their schedules
            for _ in range(min(k % 3, len(st) - 1)):
                next(st)
        before = [st.o.clone() for st in sts]
        for st in sts:
            first, count = st.schedule[st._next]
            st.z[:, :, :max(0, first - Lc)] = fill
            st.z[:, :, first + count + Rc:] = fill
        pool = net.stream_pool()
        for st in sts:
            pool.add(st)
        out = _step(net, pool)
        assert [id(st) for st, _, _ in out] == [id(st) for st in sts]
        torch.cuda.synchronize()
        for (st, a, view), c, o0 in zip(out, cases, before):
            b = a + view.shape[2]
            assert torch.equal(view, c.full[:, :, a:b]), (c.Tp, fill, a)
            assert torch.equal(st.o[:, :, :a], o0[:, :, :a]) and torch.equal(st.o[:, :, b:], o0[:, :, b:]), (c.Tp, fill)
            assert bool((st.o[:, :, b:] == SENTINEL).all())     # nothing behind the chunk has been written yet
            assert bool((o0[:, :, a:b] == SENTINEL).all())


@pytest.mark.timeout(900)
def test_mixed_driving_and_wire_follower(net):
    cases = _cases(net, seed=60)
    # one stream through the pool, alone, and the pool again
    c = max(cases, key=lambda c: len(c.solo))
    assert len(c.solo) >= 5
    st = c.stream(net)
    pool = net.stream_pool()
    pool.add(st)
    other = cases[0].stream(net)
    pool.add(other)
    _step(net, pool)
    runs = net.decoder_runs()
    a, v = next(st)                                             # decoded by the pool: handed out, nothing launched
    assert net.decoder_runs() == runs and a == 0 and torch.equal(v, c.solo[0][1])
    a, v = next(st)                                             # not decoded yet: alone
    assert net.decoder_runs() == runs + 1 and torch.equal(v, c.solo[1][1])
    out = _step(net, pool, [st])                                # only the named stream
    assert len(out) == 1 and out[0][0] is st and torch.equal(out[0][2], c.solo[2][1])
    _step(net, pool)
    assert st._decoded == 4 and st._next == 2
    assert torch.equal(st.run(), c.full)
    pool.step()
    assert all(m is not st for m in pool.streams)               # finished alone: dropped at the next step
    with pytest.raises(ValueError):
        pool.step([net.dec_stream(c.z, c.g)])                   # not a member
    # wire followers over pooled streams: pool.step(), then next(pcm) launches the ranged resample only
    sts = [k.stream(net) for k in cases]
    pcms = [wire.stream_pcm16(net, s, 22050, 24000) for s in sts]
    pcm_of = {id(s): p for s, p in zip(sts, pcms)}
    pool = net.stream_pool()
    for s in sts:
        pool.add(s)
    while len(pool):
        out = _step(net, pool)
        runs = net.decoder_runs()
        for s, _, _ in out:
            next(pcm_of[id(s)])
        assert net.decoder_runs() == runs
    for s, p, k in zip(sts, pcms, cases):
        ref, valid = wire.service_pcm16(net, k.full, None, 22050, 24000, auto_normalize=False)
        assert torch.equal(s.o, k.full)
        assert p.pcm.dtype == torch.int16 and torch.equal(p.pcm, ref), k.Tp
        assert torch.equal(p.valid_samples, valid)
        with pytest.raises(StopIteration):
            next(p)


def _count_syncs(fn):
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            fn()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    return sum("synchroniz" in str(v.message).lower() for v in w)


@pytest.mark.timeout(600)
def test_one_call_few_runs_and_no_host_synchronisation():
    net = _net("ljs_mini_mb_istft_vits")
    warm = net.stream_pool()                                    # wider windows first: the arena grows here, not below
    for k in range(16):
        warm.add(net.dec_stream(_z(net, 258, 280 + k), None, 64, 64))
    warm.step()
    pool = net.stream_pool()
    sts = [net.dec_stream(_z(net, 258, 300 + k), None, 32, 32) for k in range(16)]
    for st in sts:
        pool.add(st)
    before = net.decoder_runs()
    assert len(pool.step()) == 16
    assert net.decoder_runs() - before == 1 == net.chunks_plan([258] * 16)[0]
    before = net.decoder_runs()
    out = []
    n = _count_syncs(lambda: out.extend(pool.step()))
    print("host synchronisations in a pooled step of 16 streams: %d" % n)
    assert n == 0
    assert len(out) == 16 and net.decoder_runs() - before == 1
    # 16 streams over all four classes: four runs
    lens = [9, 12, 16, 17, 30, 64, 65, 100, 200, 256, 257, 258, 300, 400, 3, 70]
    pool = net.stream_pool()
    for k, Tp in enumerate(lens):
        pool.add(net.dec_stream(_z(net, Tp, 400 + k), None, 32, 256))
    before = net.decoder_runs()
    assert len(pool.step()) == 16
    assert net.decoder_runs() - before == 4 == net.chunks_plan(lens)[0]


def _batch(net, B, T, seed):
    x, xl, sid = synth.synthetic_batch(net.cfg, B, T, seed=seed, ragged=True)
    return (torch.from_numpy(x).cuda(), torch.from_numpy(xl).cuda(),
            torch.from_numpy(sid).cuda() if sid is not None else None)


@pytest.mark.timeout(600)
def test_side_stream_and_interleaved_calls():
    net = _net("uudb_ms_istft_vits_ms")
    cases = _cases(net, seed=80)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        sts = [c.stream(net) for c in cases]
        pool = net.stream_pool()
        for st in sts:
            pool.add(st)
        while len(pool):
            pool.step()
    side.synchronize()
    for st, c in zip(sts, cases):
        assert torch.equal(st.o, c.full), c.Tp
    # an infer and a ragged decode between two steps
    x, xl, sid = _batch(net, 3, 25, 3)
    ref = net.infer(x, xl, sid, noise_scale=0)[0].clone()
    zr = torch.randn(3, net.cfg.inter_channels, 120, generator=torch.Generator().manual_seed(5)).cuda()
    gr = (0.3 * torch.randn(3, net.cfg.gin_channels, 1, generator=torch.Generator().manual_seed(6))).cuda()
    rag = net.dec(zr, g=gr, lengths=[120, 40, 9])[0].clone()
    sts = [c.stream(net) for c in cases]
    pool = net.stream_pool()
    for st in sts:
        pool.add(st)
    while len(pool):
        pool.step()
        assert torch.equal(net.infer(x, xl, sid, noise_scale=0)[0], ref)
        assert torch.equal(net.dec(zr, g=gr, lengths=[120, 40, 9])[0], rag)
    for st, c in zip(sts, cases):
        assert torch.equal(st.o, c.full), c.Tp


@pytest.mark.timeout(600)
def test_splitk_mode():
    net = _net("ljs_mb_istft_vits")
    lens = [180, 64, 65, 17, 9, 120, 300, 258]
    zs = [_z(net, Tp, 500 + k) for k, Tp in enumerate(lens)]
    net.set_option("splitk", 1)
    try:
        full = [net.dec(z)[0].clone() for z in zs]
        got = []
        for _ in range(2):
            sts = [net.dec_stream(z, None, *SCHEDULES[k % len(SCHEDULES)]) for k, z in enumerate(zs)]
            pool = net.stream_pool()
            for st in sts:
                pool.add(st)
            while len(pool):
                before = net.decoder_runs()
                pool.step()
                assert net.decoder_runs() - before == 1          # one class in this mode
            got.append([st.o.clone() for st in sts])
    finally:
        net.set_option("splitk", 0)
    for a, b, f, Tp in zip(got[0], got[1], full, lens):
        assert torch.equal(a, b), Tp                             # bitwise run to run
        err = float(torch.sqrt(torch.mean((a - f) ** 2)))
        assert err <= 1e-5, (Tp, err)


def _chunk(z, g, o, first, count, t_frames=None, o_off=0):
    k = _capi.MbvChunk()
    k.z, k.z_stride, k.t_frames = z.data_ptr(), z.stride(1), z.shape[2] if t_frames is None else t_frames
    k.g = g.data_ptr() if g is not None else None
    k.first, k.count, k.o = first, count, o.data_ptr() + o_off
    return k


@pytest.mark.timeout(600)
def test_a_table_longer_than_one_upload_launch():
    """65 chunks of 4 frames of one 260-frame z in one call: the run's table goes up in two launches, and an offset
    wrong in the second one shows in table row 64.  Every chunk bitwise the stream's own, the runs as planned."""
    net = _net("ljs_mini_mb_istft_vits")
    z, g = _z(net, 260, 31), _g(net, 32)
    full = net.dec(z, g)[0].clone()
    solo = [(a, v.clone()) for a, v in net.dec_stream(z, g, 4, 4)]
    assert len(solo) == 65
    o = torch.full_like(full, SENTINEL)
    chunks = [_chunk(z, g, o, 4 * k, 4) for k in range(65)]
    runs = net.decoder_runs()
    assert _capi.lib().mbv_decode_chunks(net._ensure_handle(), (_capi.MbvChunk * 65)(*chunks), 65, net._stream()) == 0
    assert net.decoder_runs() - runs == net.chunks_plan([260] * 65)[0] == 1
    torch.cuda.synchronize()
    spf = net.cfg.samples_per_frame
    for k, (a, v) in enumerate(solo):
        assert a == spf * 4 * k and torch.equal(o[:, :, a:a + v.shape[2]], v), k
    assert torch.equal(o, full)


@pytest.mark.timeout(600)
def test_error_paths_launch_nothing_and_the_pool_serves_on():
    net = _net("uudb_ms_istft_vits_ms")
    L = _capi.lib()
    h = net._ensure_handle()
    spf = net.cfg.samples_per_frame
    za, zb = _z(net, 80, 1), _z(net, 50, 2)
    ga, gb = _g(net, 3), _g(net, 4)
    fa, fb = net.dec(za, ga)[0].clone(), net.dec(zb, gb)[0].clone()
    oa, ob = torch.full_like(fa, SENTINEL), torch.full_like(fb, SENTINEL)

    def call(*chunks):
        arr = (_capi.MbvChunk * len(chunks))(*chunks)
        return L.mbv_decode_chunks(h, arr, len(chunks), net._stream())

    good = _chunk(za, ga, oa, 0, 16)
    runs = net.decoder_runs()
    for bad, word in ((_chunk(zb, gb, ob, 40, 11), b"outside"), (_chunk(zb, gb, ob, -1, 4), b"outside"),
                      (_chunk(zb, gb, ob, 50, 1), b"outside"), (_chunk(zb, gb, ob, 0, 0), b"outside"),
                      (_chunk(zb, gb, ob, 0, 8, o_off=4), b"aligned"), (_chunk(zb, None, ob, 0, 8), b"all or none"),
                      (_chunk(zb, gb, ob, 0, 8, t_frames=0), b"t_frames")):
        assert call(good, bad) != 0
        assert word in L.mbv_last_error(h), (word, L.mbv_last_error(h))
    assert L.mbv_decode_chunks(h, None, 2, net._stream()) != 0
    assert L.mbv_decode_chunks(h, (_capi.MbvChunk * 1)(good), 0, net._stream()) != 0
    pool = net.stream_pool()
    sa, sb = net.dec_stream(za, ga, 16, 16), net.dec_stream(zb, gb, 16, 64)
    sa.o.fill_(SENTINEL), sb.o.fill_(SENTINEL)
    pool.add(sa), pool.add(sb)
    for opt, value in (("trim", 1), ("conv_bf16", 3)):
        net.set_option(opt, value)
        try:
            with pytest.raises(_capi.MbvError, match=opt):
                pool.step()
        finally:
            net.set_option(opt, 0)
    torch.cuda.synchronize()
    assert net.decoder_runs() == runs                            # the refusals launched nothing ...
    for o in (oa, ob, sa.o, sb.o):
        assert bool((o == SENTINEL).all())                      # ... and wrote nothing
    assert sa._decoded == 0 and sb._decoded == 0 and len(pool) == 2
    with pytest.raises(ValueError, match="ONE utterance"):
        pool.add(net.dec_stream(torch.cat([za, za]), torch.cat([ga, ga])))
    with pytest.raises(ValueError, match="another model"):
        pool.add(_net("ljs_mini_mb_istft_vits").dec_stream(_z(_net("ljs_mini_mb_istft_vits"), 40, 1)))
    # the handle and the pool serve the next step; all-absent g is a valid call of its own
    while len(pool):
        pool.step()
    assert torch.equal(sa.o, fa) and torch.equal(sb.o, fb)
    # two chunks of ONE utterance in one call, disjoint ranges, plus a chunk of another
    assert call(_chunk(za, ga, oa, 0, 16), _chunk(zb, gb, ob, 10, 40), _chunk(za, ga, oa, 48, 32)) == 0
    torch.cuda.synchronize()
    assert torch.equal(oa[:, :, :spf * 16], fa[:, :, :spf * 16]) and torch.equal(oa[:, :, spf * 48:], fa[:, :, spf * 48:])
    assert bool((oa[:, :, spf * 16:spf * 48] == SENTINEL).all())
    assert torch.equal(ob[:, :, spf * 10:], fb[:, :, spf * 10:]) and bool((ob[:, :, :spf * 10] == SENTINEL).all())
    no_g = net.dec(za, None)[0]
    assert call(_chunk(za, None, oa, 16, 32)) == 0
    torch.cuda.synchronize()
    assert torch.equal(oa[:, :, spf * 16:spf * 48], no_g[:, :, spf * 16:spf * 48])
