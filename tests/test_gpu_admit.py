"""Pooled admission on the MI355X: `net.infer_streams(requests)` runs the front half (text encoder, duration
predictor, length regulation, flows) of many requests as one padded run per class of `admit_plan`, and every stream
it returns is bitwise the stream `net.infer_stream` returns for that request alone."""
import pytest
import torch

from mb_istft_vits_amd import _capi, wire
from mb_istft_vits_amd.models import Request

from gpu_util import make_net

pytestmark = pytest.mark.gpu

NETS = {"mini": ("ljs_mini_mb_istft_vits", None), "sdp": ("ljs_mini_mb_istft_vits", {"use_sdp": True}),
        "uudb": ("uudb_ms_istft_vits_ms", None)}
# both sides of the cuts of the 16-frame half-units and the 32-key tiles, and of the route rule (T <= 256)
SHORT = [1, 2, 15, 16, 17, 32, 33, 64]
LONG = [100, 256, 257, 300]
SCHEDULES = [(32, 256), (8, 32), (16, 64), (5, 40), (24, 24), (64, 256), (12, 96)]
_NETS = {}


def _net(key):
    if key not in _NETS:
        name, overrides = NETS[key]
        _NETS[key] = make_net(name, overrides=overrides)[0]
    return _NETS[key]


@pytest.fixture(scope="module", params=list(NETS), ids=list(NETS))
def net_key(request):
    return request.param


def _lengths(key):
    return SHORT if key == "uudb" else SHORT + LONG          # (texts of at most 64 tokens on the large model)


def _ids(T, seed):
    return torch.randint(1, 59, (T,), generator=torch.Generator().manual_seed(seed))


def _seed(s):
    torch.manual_seed(s)
    torch.cuda.manual_seed(s)


def _rng_states():
    return torch.get_rng_state().clone(), torch.cuda.get_rng_state().clone()


def _solo(net, r, x=None):
    """The stand-alone call the contract names for a request (x: another token row of the same length)."""
    x = r.x if x is None else x
    sid = torch.tensor([r.sid]).cuda() if r.sid is not None else None
    d = r.durations[None] if r.durations is not None else None
    return net.infer_stream(x[None].cuda(), torch.tensor([r.x.numel()]).cuda(), sid, r.noise_scale, r.length_scale,
                            r.noise_scale_w, r.max_len, r.chunk_frames, r.max_chunk_frames, durations=d)


def _same(a, b):
    """z, g, y_lengths and schedule of two streams, bitwise."""
    if a.z.shape != b.z.shape or not torch.equal(a.z, b.z):
        return False
    if (a.g is None) != (b.g is None) or (a.g is not None and not (a.g.shape == b.g.shape and torch.equal(a.g, b.g))):
        return False
    return torch.equal(a.y_lengths, b.y_lengths) and a.schedule == b.schedule and a.o.shape == b.o.shape


def _requests(net, key, seed=0):
    """Mixed lengths, sids, scales, max_len, given durations and chunk schedules; not sorted by length."""
    lens = _lengths(key)
    lens = lens[1::2] + lens[0::2]
    g = torch.Generator().manual_seed(1000 + seed)
    reqs, given = [], 0
    for k, T in enumerate(lens):
        kw = dict(noise_scale=(0.0, 0.5, 1.0)[k % 3], length_scale=(0.8, 1.0, 1.3)[(k // 2) % 3],
                  noise_scale_w=(0.0, 0.8)[k % 2], chunk_frames=SCHEDULES[k % 7][0], max_chunk_frames=SCHEDULES[k % 7][1])
        if net.n_speakers > 0:
            kw["sid"] = (3 * k + 1) % net.n_speakers
        if k % 4 == 1:
            kw["max_len"] = (7, 40, 100000)[(k // 4) % 3]
        if k % 3 == 2 or k == 6:                            # given durations, one dtype each in turn, zeros included
            d = torch.randint(0, 6, (T,), generator=g)
            kw["durations"] = (d.to(torch.int32), d, d.to(torch.float32))[given % 3]
            kw["length_scale"] = 1.0
            given += 1
        reqs.append(Request(_ids(T, 50 * seed + k), **kw))
    assert {r.noise_scale for r in reqs} == {0.0, 0.5, 1.0} and {r.length_scale for r in reqs} == {0.8, 1.0, 1.3}
    assert {r.durations_dtype for r in reqs} == {None, 0, 1, 2} and any(r.max_len for r in reqs)
    return reqs


def _plan_runs(net, reqs, splitk=False):
    return net.admit_plan([r.x.numel() for r in reqs], splitk=splitk)[0]


@pytest.mark.timeout(600)
def test_a_row_does_not_depend_on_its_padding(net_key):
    """The yardstick the contract rests on: `infer_stream` of a text alone equals bitwise `infer_stream` of the same
    row zero-padded to the longest text of its class, same seed.  With the stochastic duration predictor the draw
    randn(1, 2, T) has the padded call's shape there, so its values cannot be the same: through `infer_stream` the
    check runs at noise_scale_w = 0 (the predictor's arithmetic on a zero draw), and once more with noise, the padded
    call being given the row's own draw in its first T columns."""
    net = _net(net_key)
    lens = _lengths(net_key)
    for k, T in enumerate(lens):
        longest = max(t for t in lens if (t <= 256) == (T <= 256))
        if T == longest:
            continue
        r = Request(_ids(T, 300 + k), sid=k % net.n_speakers if net.n_speakers else None, noise_scale=0.667,
                    length_scale=(1.0, 1.1)[k % 2], noise_scale_w=0.0 if net.cfg.use_sdp else 0.8, chunk_frames=16)
        padded = torch.zeros(longest, dtype=torch.int64)
        padded[:T] = r.x
        _seed(7 + k)
        alone = _solo(net, r)
        _seed(7 + k)
        wide = _solo(net, r, x=padded)
        assert _same(alone, wide), (net_key, T, longest)
        if net.cfg.use_sdp:
            nw = torch.randn(1, 2, T, generator=torch.Generator().manual_seed(k))
            nw_wide = torch.zeros(1, 2, longest)
            nw_wide[:, :, :T] = nw
            out = []
            for x, w in ((r.x, nw), (padded, nw_wide)):
                _seed(7 + k)
                res = net._run(x[None].cuda(), torch.tensor([T]).cuda(), None, 0.667, 1.0, None, decode=False,
                               noise_scale_w=0.8, noise_w=w, outputs=("z", "y_mask"))
                out.append((res[6][0] * res[5], res[8]))
            assert torch.equal(out[0][1], out[1][1]) and torch.equal(out[0][0], out[1][0]), (T, longest)


@pytest.mark.timeout(600)
def test_streams_are_bitwise_the_stand_alone_streams(net_key):
    net = _net(net_key)
    reqs = _requests(net, net_key)
    # not vacuous: the scales reach the result
    base = Request(_ids(33, 1), sid=0 if net.n_speakers else None, noise_scale=0.5, length_scale=0.8, noise_scale_w=0.8)
    other_ns = Request(base.x, sid=base.sid, noise_scale=1.0, length_scale=0.8, noise_scale_w=0.8)
    other_ls = Request(base.x, sid=base.sid, noise_scale=0.5, length_scale=1.3, noise_scale_w=0.8)
    got = []
    for r in (base, other_ns, other_ls):
        _seed(5)
        got.append(_solo(net, r))
    assert got[0].z.shape == got[1].z.shape and not torch.equal(got[0].z, got[1].z)
    assert int(got[2].y_lengths) > int(got[0].y_lengths)
    # the N stand-alone calls, in order
    _seed(11)
    solo = [_solo(net, r) for r in reqs]
    states = _rng_states()
    assert len({int(s.y_lengths) for s in solo}) >= 3
    # ... and the one admission
    _seed(11)
    runs = net.encoder_runs()
    sts = net.infer_streams(reqs)
    assert net.encoder_runs() - runs == _plan_runs(net, reqs) == (1 if net_key == "uudb" else 2)
    assert len(sts) == len(reqs)
    for k, (a, b, r) in enumerate(zip(sts, solo, reqs)):
        assert a.z.shape[0] == 1 and a.z.is_contiguous() and a.y_lengths.shape == (1,)
        assert _same(a, b), (net_key, k, r, tuple(a.z.shape), tuple(b.z.shape),
                             float((a.z - b.z).abs().max()) if a.z.shape == b.z.shape else None)
    after = _rng_states()
    assert torch.equal(after[0], states[0]), "the CPU generator ends elsewhere"
    assert torch.equal(after[1], states[1]), "the device generator ends elsewhere"
    # downstream: a pool of the admitted streams decodes what the stand-alone streams decode
    pool = net.stream_pool()
    for st in sts[:4]:
        pool.add(st)
    while len(pool):
        pool.step()
    for a, b in zip(sts[:4], solo[:4]):
        assert torch.equal(a.o, b.run())


@pytest.mark.timeout(600)
def test_admitted_requests_reach_the_wire_bitwise():
    net = _net("mini")
    lens = [33, 100, 257, 16, 300, 64]
    reqs = [Request(_ids(T, 700 + k), noise_scale=(0.5, 1.0)[k % 2], length_scale=(1.0, 1.3, 0.8)[k % 3],
                    chunk_frames=SCHEDULES[k][0], max_chunk_frames=SCHEDULES[k][1], max_len=(None, 90)[k == 4])
            for k, T in enumerate(lens)]
    _seed(21)
    want = []
    for r in reqs:
        p = wire.stream_pcm16(net, _solo(net, r), 22050, 24000)
        pcm, valid = p.run()
        want.append((pcm.clone(), valid.clone(), p.peak.clone()))
    _seed(21)
    sp = net.stream_pool()
    pp = wire.pcm_pool(net, sp, 22050, 24000)
    waves = {0: reqs[:3], 2: reqs[3:]}                        # the second wave arrives after two steps
    fol, steps = [], 0
    while steps in waves or steps < 2 or len(pp):
        if steps in waves:
            runs = net.encoder_runs()
            new = pp.admit(waves[steps])
            assert net.encoder_runs() - runs == _plan_runs(net, waves[steps]) == 2
            assert len(new) == 3 and all(pp.follower(f._st) is f for f in new)
            fol += new
        stepped = [st for st in sp.streams if st._decoded < len(st.schedule)]
        dec, wr = net.decoder_runs(), wire.wire_runs(net)
        out = pp.step()
        steps += 1
        assert net.decoder_runs() - dec == (net.chunks_plan([st.z.shape[2] for st in stepped])[0] if stepped else 0)
        assert wire.wire_runs(net) - wr == (1 if out else 0)
    assert len(fol) == 6 and steps < sum(len(f._st) for f in fol)
    for k, (f, (pcm, valid, peak)) in enumerate(zip(fol, want)):
        assert f.pcm.dtype == torch.int16 and torch.equal(f.pcm, pcm), k
        assert torch.equal(f.valid_samples, valid) and torch.equal(f.peak.view(torch.int32), peak.view(torch.int32)), k


@pytest.mark.timeout(600)
def test_a_flagged_request_fails_the_whole_admission_and_the_pool_serves_on():
    net = _net("uudb")
    lens = [17, 33, 9, 64, 2]
    good = [Request(_ids(T, 800 + k), sid=k, noise_scale=0.5, chunk_frames=8, max_chunk_frames=32) for k, T in enumerate(lens)]
    _seed(31)
    live_req = [Request(_ids(40, 790), sid=1, chunk_frames=4, max_chunk_frames=8),
                Request(_ids(12, 791), sid=2, length_scale=1.3, chunk_frames=2, max_chunk_frames=4)]
    live_want = [_solo(net, r).run().clone() for r in live_req]
    _seed(31)
    pool = net.stream_pool()
    live = pool.admit(live_req)
    pool.step()

    def bad_token(r):
        x = r.x.clone()
        x[x.numel() // 2] = 59                              # one past the table
        return Request(x, sid=r.sid, noise_scale=r.noise_scale, chunk_frames=8, max_chunk_frames=32)

    for make, names in (
            (lambda: [good[0], good[1], bad_token(good[2]), good[3], good[4]], "request 2:"),
            (lambda: [good[0], Request(good[1].x, sid=net.n_speakers), good[2],
                      Request(good[3].x, sid=0, durations=torch.tensor([-1] + [2] * 63)), good[4]], "requests 1, 3:"),
            (lambda: [Request(good[0].x, sid=0, durations=torch.full((17,), 2.5))], "request 0:")):
        reqs = make()
        runs, members = net.encoder_runs(), list(pool.streams)
        with pytest.raises(IndexError, match=names):
            pool.admit(reqs)
        assert net.encoder_runs() - runs <= _plan_runs(net, reqs)
        assert len(pool.streams) == len(members) and all(a is b for a, b in zip(pool.streams, members))
    # refused before any launch
    runs = net.encoder_runs()
    with pytest.raises(ValueError, match="request 1: sid is required"):
        pool.admit([good[0], Request(good[1].x)])
    net.set_option("conv_bf16", 3)
    try:
        with pytest.raises(ValueError, match="conv_bf16"):
            pool.admit(good)
        h, L = net._ensure_handle(), _capi.lib()
        one = (_capi.MbvEncRow * 1)()
        one[0].length_scale, one[0].t_text = 1.0, 4
        ids, n = torch.ones(1, 4, dtype=torch.int64).cuda(), torch.tensor([4]).cuda()
        assert L.mbv_encode_rows(h, 0, ids.data_ptr(), n.data_ptr(), n.data_ptr(), 1, 4, one, n.data_ptr(), None) != 0
        assert b"conv_bf16" in L.mbv_last_error(h)
    finally:
        net.set_option("conv_bf16", 0)
    with pytest.raises(ValueError, match="empty text"):
        Request([])
    with pytest.raises(ValueError, match="length_scale must be 1"):
        Request([1, 2], length_scale=0.8, durations=torch.tensor([1, 1]))
    assert net.encoder_runs() == runs and len(pool.streams) == 2
    # the C entry refuses what the plan would not put into one run, and rows it cannot read
    h, L = net._ensure_handle(), _capi.lib()
    two = (_capi.MbvEncRow * 2)()
    for row, t in zip(two, (300, 20)):
        row.length_scale, row.noise_scale_w, row.t_text = 1.0, 1.0, t
    ids, n2 = torch.ones(2, 300, dtype=torch.int64).cuda(), torch.tensor([300, 20]).cuda()
    sid2, y2 = torch.zeros(2, dtype=torch.int64).cuda(), torch.zeros(2, dtype=torch.int64).cuda()
    assert L.mbv_encode_rows(h, 0, ids.data_ptr(), n2.data_ptr(), sid2.data_ptr(), 2, 300, two, y2.data_ptr(), None) != 0
    assert b"more than one run" in L.mbv_last_error(h)
    two[0].t_text = 301
    assert L.mbv_encode_rows(h, 0, ids.data_ptr(), n2.data_ptr(), sid2.data_ptr(), 2, 300, two, y2.data_ptr(), None) != 0
    assert b"t_text" in L.mbv_last_error(h)
    assert L.mbv_synthesize_rows(h, 5, 10, (_capi.MbvRow * 1)(), 1, None) != 0
    assert b"without a preceding" in L.mbv_last_error(h)
    assert net.encoder_runs() == runs
    # the next valid admission is right, and so are the streams that were live all along
    _seed(41)
    want = [_solo(net, r) for r in good]
    _seed(41)
    sts = pool.admit(good)
    assert len(pool.streams) == 7
    for a, b in zip(sts, want):
        assert _same(a, b)
    while len(pool):
        pool.step()
    for st, o in zip(live, live_want):
        assert torch.equal(st.o, o)
    for a, b in zip(sts, want):
        assert torch.equal(a.o, b.run())


@pytest.mark.timeout(600)
def test_splitk_mode_is_deterministic_and_within_rounding():
    """Low-latency mode: the routes in front of the flows follow the launch size, so admission is not bitwise the
    stand-alone call there.  With given durations both sides have the same T': two admissions are bitwise equal, and
    every z is within 5e-5 relative (rms) of the stand-alone call, the bar of the goldens' z taps."""
    net = _net("mini")
    lens = [17, 300, 64, 1, 256, 100, 33, 257]
    g = torch.Generator().manual_seed(3)
    reqs = [Request(_ids(T, 900 + k), noise_scale=(0.5, 1.0, 0.0)[k % 3], chunk_frames=16,
                    durations=torch.randint(0, 5, (T,), generator=g) + (T == 1)) for k, T in enumerate(lens)]
    net.set_option("splitk", 1)
    try:
        _seed(51)
        solo = [_solo(net, r) for r in reqs]
        got = []
        for _ in range(2):
            _seed(51)
            runs = net.encoder_runs()
            got.append(net.infer_streams(reqs))
            assert net.encoder_runs() - runs == 1 == _plan_runs(net, reqs, splitk=True)
    finally:
        net.set_option("splitk", 0)
    for k, (a, b, s) in enumerate(zip(got[0], got[1], solo)):
        assert _same(a, b), k
        assert a.z.shape == s.z.shape and torch.equal(a.y_lengths, s.y_lengths) and a.schedule == s.schedule
        rel = float(torch.sqrt(torch.mean((a.z - s.z) ** 2)) / torch.sqrt(torch.mean(s.z ** 2)))
        print("splitk: request %d (%d tokens, %d frames): z relative rms %.3e" % (k, lens[k], a.z.shape[2], rel))
        assert rel <= 5e-5, (k, rel)


@pytest.mark.timeout(600)
def test_side_stream_and_interleaved_calls():
    net = _net("uudb")
    reqs = _requests(net, "uudb", seed=2)
    _seed(61)
    want = [_solo(net, r) for r in reqs]
    full = [s.run().clone() for s in want]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _seed(61)
        pool = net.stream_pool()
        sts = pool.admit(reqs)
        while len(pool):
            pool.step()
    side.synchronize()
    for a, b, o in zip(sts, want, full):
        assert _same(a, b) and torch.equal(a.o, o)
    # an infer and a ragged decode between the admission and the pool's steps, and between two admissions
    x = torch.stack([torch.cat([_ids(25, 1), torch.zeros(5, dtype=torch.int64)]), _ids(30, 2), _ids(30, 3)]).cuda()
    xl, sid = torch.tensor([25, 30, 12]).cuda(), torch.tensor([0, 1, 2]).cuda()
    ref = net.infer(x, xl, sid, noise_scale=0)[0].clone()
    zr = torch.randn(3, net.cfg.inter_channels, 120, generator=torch.Generator().manual_seed(5)).cuda()
    gr = (0.3 * torch.randn(3, net.cfg.gin_channels, 1, generator=torch.Generator().manual_seed(6))).cuda()
    rag = net.dec(zr, g=gr, lengths=[120, 40, 9])[0].clone()
    _seed(61)
    pool = net.stream_pool()
    half = len(reqs) // 2
    sts = pool.admit(reqs[:half])
    state = _rng_states()
    assert torch.equal(net.infer(x, xl, sid, noise_scale=0)[0], ref)        # (draws its noise too)
    torch.set_rng_state(state[0])
    torch.cuda.set_rng_state(state[1])
    pool.step()
    sts += pool.admit(reqs[half:])
    while len(pool):
        pool.step()
        assert torch.equal(net.infer(x, xl, sid, noise_scale=0)[0], ref)
        assert torch.equal(net.dec(zr, g=gr, lengths=[120, 40, 9])[0], rag)
    for a, b, o in zip(sts, want, full):
        assert _same(a, b) and torch.equal(a.o, o)


@pytest.mark.timeout(600)
def test_a_table_longer_than_one_upload_launch():
    """65 requests in one run: both admission tables go up in two launches, and an offset wrong in the second one shows
    in table row 64.  Every stream bitwise its stand-alone call, one encoder run, both generators where they end."""
    net = _net("mini")
    reqs = [Request(_ids(4 + k % 6, 700 + k), noise_scale=(0.0, 0.5, 1.0)[k % 3], length_scale=(0.8, 1.0, 1.3)[(k // 2) % 3],
                    noise_scale_w=(0.0, 0.8)[k % 2], chunk_frames=SCHEDULES[k % 7][0], max_chunk_frames=SCHEDULES[k % 7][1])
            for k in range(65)]
    _seed(13)
    solo = [_solo(net, r) for r in reqs]
    states = _rng_states()
    _seed(13)
    runs = net.encoder_runs()
    sts = net.infer_streams(reqs)
    assert net.encoder_runs() - runs == _plan_runs(net, reqs) == 1
    assert len(sts) == 65
    for k, (a, b, r) in enumerate(zip(sts, solo, reqs)):
        assert _same(a, b), (k, r, tuple(a.z.shape), tuple(b.z.shape))
    after = _rng_states()
    assert torch.equal(after[0], states[0]) and torch.equal(after[1], states[1])
