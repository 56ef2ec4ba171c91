"""Live text on the MI355X (`net.infer_live`, `stream.TextStream`): with the whole text ahead the stream is
`infer_stream`; every token block is a prefix call; z_p is the length regulator's; the flows reach R frames; a bounded
stream is a pure function of the tokens whatever the pushes, the polls and the pool; launch counts; refusals."""
import ctypes as C

import pytest
import torch

from mb_istft_vits_amd import _capi, stream
from mb_istft_vits_amd.stream import TextAhead

from gpu_util import make_net

pytestmark = pytest.mark.gpu

NETS = {"mini": ("ljs_mini_mb_istft_vits", None), "sdp": ("ljs_mini_mb_istft_vits", {"use_sdp": True}),
        "uudb": ("uudb_ms_istft_vits_ms", None)}
MODEL_SR, HOP, WIN = 16000, 256, 1024              # the data config of the uudb model (the live recording beside a text)
_CACHE = {}


def _net(name="mini"):
    if name not in _CACHE:
        cfg, over = NETS[name]
        _CACHE[name] = make_net(cfg, overrides=over)[0]
    return _CACHE[name]


def _ids(n, seed=0):
    g = torch.Generator().manual_seed(1000 + seed)
    return torch.randint(1, 59, (n,), generator=g).tolist()


def _drive(st, ids, step, pool=None):
    """Pushes `step` tokens at a time with a tick after each push, closes, ticks to the end -> [(first_sample, clone)]."""
    got = []

    def tick():
        if pool is not None:
            pool.step()
        for a, v in st.poll():
            got.append((a, v.clone()))

    for i in range(0, len(ids), step):
        st.push(ids[i:i + step])
        tick()
    st.close()
    for _ in range(64):
        if st.finished:
            break
        tick()
    assert st.finished and st.poll() == [] and st.y_lengths.tolist() == [st.frames]
    return got


def _counters(net):
    return (net.encoder_runs(), net.text_runs(), net.flow_runs(), net.decoder_runs())


def _same_chunks(a, b):
    assert [x for x, _ in a] == [x for x, _ in b]
    for (_, u), (_, v) in zip(a, b):
        assert torch.equal(u, v)


def _reference(net, ids, length_scale, seed, sid=None):
    key = ("ref", id(net), tuple(ids), length_scale, seed, sid)
    if key not in _CACHE:
        x = torch.tensor([ids])
        ref = net.infer_stream(x, torch.tensor([len(ids)]), sid=None if sid is None else torch.tensor([sid]),
                               seed=seed, length_scale=length_scale, marks=True)
        chunks = [(a, v.clone()) for a, v in ref]
        _CACHE[key] = (ref, chunks)
    return _CACHE[key]


# ------------------------------------------------------------------------------------------------ 1: the anchor
@pytest.mark.parametrize("step", [1, 5, 24])
def test_the_whole_text_ahead_is_bitwise_infer_stream(step):
    net, ids = _net(), _ids(24)
    ref, ref_chunks = _reference(net, ids, 5, 7)
    T = ref.z.shape[2]
    assert T > 256                                  # the class in which a window and the whole utterance agree bitwise
    st = net.infer_live(max_tokens=32, max_frames=T + 40, seed=7, length_scale=5, block_tokens=8,
                        ahead=TextAhead(tokens=None))
    got = _drive(st, ids, step)
    assert st.frames == T and st.tokens == 24 and st.marks == ref.marks
    assert st.durations == [b - a for a, b in zip(ref.marks, ref.marks[1:])]
    assert torch.equal(st.z[:, :, :T], ref.z)
    _same_chunks(got, ref_chunks)
    assert torch.equal(st.result(), ref.o) and st.y_lengths.tolist() == ref.y_lengths.tolist()


def test_a_short_utterance_is_infer_stream_within_rounding():
    """T <= 256: the whole utterance takes the narrow conv kernels, a window the tiled ones, which sum in another order
    (the bars of test_gpu_live_convert.py, for the same cause)."""
    net, ids = _net(), _ids(24)
    ref, _ = _reference(net, ids, 1, 7)
    T = ref.z.shape[2]
    assert T <= 256
    st = net.infer_live(max_tokens=24, max_frames=256, seed=7, block_tokens=8, ahead=TextAhead(tokens=None))
    _drive(st, ids, 5)
    assert st.marks == ref.marks and st.frames == T
    zd = ref.z.double()
    rel = float(torch.sqrt(torch.mean((st.z[:, :, :T] - zd) ** 2)) / torch.sqrt(torch.mean(zd ** 2)))
    o_ref = ref.run()
    err = float(torch.sqrt(torch.mean((st.result() - o_ref).double() ** 2)))
    print("live text against infer_stream, %d frames: z relative rms %.3e, o rms %.3e" % (T, rel, err))
    assert rel <= 5e-5, rel
    assert err <= 1e-4, err


def test_tokens_ahead_of_the_whole_text_is_none():
    net, ids = _net(), _ids(24)
    ref, ref_chunks = _reference(net, ids, 5, 7)
    T = ref.z.shape[2]
    st = net.infer_live(max_tokens=24, max_frames=T, seed=7, length_scale=5, block_tokens=8, ahead=TextAhead(tokens=24))
    got = _drive(st, ids, 5)
    assert torch.equal(st.z[:, :, :T], ref.z) and st.marks == ref.marks
    _same_chunks(got, ref_chunks)
    assert torch.equal(st.result(), ref.o)


# ------------------------------------------------------------------------------------------------ 2: prefix calls
def _assert_blocks_are_prefix_calls(net, st, ids, blocks, bt, sid=None, **kw):
    I = net.cfg.inter_channels
    for k, E in blocks:
        x = torch.tensor([ids[:E]])
        attn = net.infer_z_only(x, torch.tensor([E]), sid=None if sid is None else torch.tensor([sid]), **kw)[0]
        m = net.read_stage("m_text").view(I, E)
        logs = net.read_stage("logs_text").view(I, E)
        d = attn.sum(2).view(E).round().to(torch.int64).tolist()
        a, b = k * bt, min((k + 1) * bt, E)
        assert torch.equal(st.stats[:I, a:b], m[:, a:b]), (k, E)
        assert torch.equal(st.stats[I:, a:b], logs[:, a:b]), (k, E)
        assert st.durations[a:b] == d[a:b] and st.dur[a:b].tolist() == d[a:b], (k, E)


def test_blocks_are_prefix_calls_plain_and_blended_voice():
    net, ids = _net("uudb"), _ids(24, 1)
    voice = net.speaker(ids=[2, 5], weights=[0.25, 0.75])
    try:
        for sid in (3, voice.sid):
            st = net.infer_live(sid=sid, max_tokens=24, max_frames=1024, seed=11, length_scale=1.3, block_tokens=8,
                                ahead=TextAhead(tokens=4))
            _drive(st, ids, 24)
            assert st.tokens == 24 and st.plan.blocks == 3
            _assert_blocks_are_prefix_calls(net, st, ids, [(0, 12), (1, 20), (2, 24)], 8, sid=sid, seed=11,
                                            length_scale=1.3)
    finally:
        voice.release()


def test_blocks_are_prefix_calls_with_the_stochastic_predictor():
    net, ids = _net("sdp"), _ids(24, 2)
    st = net.infer_live(max_tokens=30, max_frames=1024, seed=13, noise_scale_w=0.8, block_tokens=8,
                        ahead=TextAhead(tokens=4))
    _drive(st, ids, 3)
    _assert_blocks_are_prefix_calls(net, st, ids, [(0, 12), (1, 20), (2, 24)], 8, seed=13, noise_scale_w=0.8)


# ------------------------------------------------------------------------------------------------ 3: expand
def _assert_z_p_is_op_expand(net, st, N, noise_scale):
    T, I = st.frames, net.cfg.inter_channels
    dev = st.z.device
    stats = st.stats[:, :N].contiguous().view(1, 2 * I, N)
    cum = torch.cumsum(torch.tensor([st.durations], dtype=torch.int32), 1).to(torch.int32).to(dev)
    assert st.dur[:N].tolist() == st.durations and len(st.durations) == N
    ylen = torch.tensor([T], dtype=torch.int32, device=dev)
    noise = st.noise[:, :, :T].contiguous()
    z_p = torch.full((1, I, T), float("nan"), device=dev)
    z = torch.empty(1, I, T, device=dev)
    h = net._ensure_handle()
    _capi.check(h, _capi.lib().mbv_op_expand(h, stats.data_ptr(), cum.data_ptr(), ylen.data_ptr(), noise.data_ptr(),
                                             noise_scale, None, None, z_p.data_ptr(), z.data_ptr(), None, None, 1, I, N, T,
                                             net._stream()), "mbv_op_expand")
    assert torch.equal(st.z_p[:, :, :T], z_p)
    assert not st.z_p[:, :, T:].any()               # nothing behind T was written


def test_z_p_is_the_length_regulators():
    net, ids = _net(), _ids(40, 3)
    st = net.infer_live(max_tokens=48, max_frames=700, seed=5, length_scale=2, noise_scale=0.667, block_tokens=16,
                        ahead=TextAhead(tokens=4))
    _drive(st, ids, 7)
    _assert_z_p_is_op_expand(net, st, 40, 0.667)


def test_z_p_of_a_block_of_more_than_256_tokens_and_frames():
    """Two rounds of the kernel's scan (288 tokens, the carry between them) and more than one 256-frame block of its grid."""
    net, ids = _net(), _ids(300, 12)
    st = net.infer_live(max_tokens=300, max_frames=4000, seed=6, noise_scale=0.5, block_tokens=288,
                        ahead=TextAhead(tokens=4))
    _drive(st, ids, 150)
    assert st.plan.blocks == 2 and st.marks[288] > 256 and st.marks[288] - st.marks[256] > 0
    _assert_z_p_is_op_expand(net, st, 300, 0.5)


# ------------------------------------------------------------------------------------------------ 4: reach
def test_the_flows_reach_R_frames():
    net, ids = _net(), _ids(24, 4)
    R = net.text_context()[1]
    assert net.text_context() == (32, 32)
    F = 600
    noise = torch.randn(1, net.cfg.inter_channels, F, generator=torch.Generator().manual_seed(3)).cuda()
    runs = []
    for f in (None, 60):
        n = noise.clone()
        if f is not None:
            n[:, :, f] += 1.0
        st = net.infer_live(max_tokens=24, max_frames=F, noise=n, length_scale=3, block_tokens=8,
                            ahead=TextAhead(tokens=4))
        _drive(st, ids, 6)
        runs.append(st)
    a, b = runs
    T = a.frames
    assert T == b.frames and T > 60 + R + 8
    diff = (a.z[0, :, :T] != b.z[0, :, :T]).any(0).nonzero().view(-1).tolist()
    assert diff and min(diff) >= 60 - R and max(diff) <= 60 + R, (min(diff), max(diff))
    assert (a.z_p[0, :, :T] != b.z_p[0, :, :T]).any(0).nonzero().view(-1).tolist() == [60]


# ------------------------------------------------------------------------------------------------ 5: purity
def _bounded(net, ids, sid=None, seed=21):
    return net.infer_live(sid=sid, max_tokens=len(ids), max_frames=800, seed=seed, length_scale=2, block_tokens=8,
                          ahead=TextAhead(tokens=4, dec=4, seam_ms=5), chunk_frames=8, max_chunk_frames=32,
                          model_sr=MODEL_SR)


def test_a_bounded_stream_does_not_depend_on_pushes_polls_or_the_pool():
    """On the multi-speaker model, which a `LiveStream` needs; the single-speaker model below, without one."""
    net, ids = _net("uudb"), _ids(40, 5)
    one = _bounded(net, ids, sid=4)
    got_one = _drive(one, ids, 1)
    assert one.seam == 80 and len(got_one) > 4
    whole = _bounded(net, ids, sid=4)
    got_whole = _drive(whole, ids, 40)
    # ... and in a pool beside a second text stream, a decode stream and a recording that is still arriving
    pool = net.stream_pool()
    other = pool.add(_bounded(net, _ids(33, 6), sid=1, seed=22))
    other.push(_ids(33, 6))
    dec = pool.add(net.infer_stream(torch.tensor([_ids(30, 7)]), torch.tensor([30]), sid=torch.tensor([2]), seed=3,
                                    chunk_frames=8, max_chunk_frames=16))
    live = pool.add(net.convert_live(3, 7, MODEL_SR, HOP, WIN, HOP * 220, seed=9))
    live.push(0.1 * torch.randn(HOP * 200, generator=torch.Generator().manual_seed(1)).cuda())
    pooled = pool.add(_bounded(net, ids, sid=4))
    got_pooled = _drive(pooled, ids, 3, pool=pool)
    T = one.frames
    for st, got in ((whole, got_whole), (pooled, got_pooled)):
        assert st.frames == T and st.marks == one.marks
        assert torch.equal(st.z[:, :, :T], one.z[:, :, :T]) and torch.equal(st.z_p[:, :, :T], one.z_p[:, :, :T])
        _same_chunks(got, got_one)
        assert torch.equal(st.result(), one.result())
    assert live.z_frames > 0 and dec._decoded > 0


def test_a_bounded_stream_on_the_single_speaker_model():
    net, ids = _net(), _ids(40, 5)
    one = _bounded(net, ids)
    got_one = _drive(one, ids, 1)
    pool = net.stream_pool()
    other = pool.add(_bounded(net, _ids(33, 6), seed=22))
    other.push(_ids(33, 6))
    dec = pool.add(net.infer_stream(torch.tensor([_ids(30, 7)]), torch.tensor([30]), seed=3, chunk_frames=8))
    pooled = pool.add(_bounded(net, ids))
    got_pooled = _drive(pooled, ids, 40, pool=pool)
    T = one.frames
    assert pooled.frames == T and torch.equal(pooled.z[:, :, :T], one.z[:, :, :T])
    _same_chunks(got_pooled, got_one)
    assert torch.equal(pooled.result(), one.result()) and dec._decoded > 0


# ------------------------------------------------------------------------------------------------ 6: admission classes
def test_prefixes_on_both_sides_of_256_tokens_make_two_encoder_runs():
    net, ids = _net(), _ids(264, 8)
    st = net.infer_live(max_tokens=264, max_frames=4000, seed=2, block_tokens=128, ahead=TextAhead(tokens=4))
    st.push(ids)
    st.close()
    assert st.plan.due_blocks() == [(0, 132), (1, 260), (2, 264)]
    before = _counters(net)
    st.poll()
    after = _counters(net)
    assert after[0] - before[0] == 2 and after[1] - before[1] == 3          # two take launches, one expand launch
    while not st.finished:
        st.poll()
    _assert_blocks_are_prefix_calls(net, st, ids, [(0, 132)], 128, seed=2)


# ------------------------------------------------------------------------------------------------ 7: launch counts
def test_eight_streams_share_one_encoder_run_two_text_launches_and_the_planned_flow_runs():
    net = _net()
    pool = net.stream_pool()
    sts = [pool.add(net.infer_live(max_tokens=40, max_frames=900, seed=30 + i, length_scale=5, block_tokens=8,
                                   ahead=TextAhead(tokens=4))) for i in range(8)]
    for i, st in enumerate(sts):
        st.push(_ids(12 + i if i < 7 else 20, 40 + i))                      # block 0 of each is due, of the last one two
    assert sum(len(st.plan.due_blocks()) for st in sts) == 9
    before = _counters(net)
    pool.step()
    after = _counters(net)
    assert [st.plan.blocks for st in sts] == [1] * 7 + [2]
    assert after[0] - before[0] == 1 and after[1] - before[1] == 2
    flowed = sum(st.z_frames > 0 for st in sts)
    assert flowed > 0 and after[2] - before[2] == 1                         # the windows of the tick are one planned run
    # nothing due: nothing is launched
    for _ in range(32):
        if not pool.step():
            break
    quiet = _counters(net)
    assert pool.step() == [] and _counters(net) == quiet
    for st in sts:
        st.poll()                                                           # (hands the pooled chunks out)
    assert _counters(net) == quiet
    for st in sts:
        st.close()
    for _ in range(64):
        if not len(pool):
            break
        pool.step()
    assert all(st.plan.all_released for st in sts)


# ------------------------------------------------------------------------------------------------ 8: refusals
def test_python_refusals_launch_nothing():
    net = _net()
    before = _counters(net)
    with pytest.raises(ValueError, match="seed= and noise="):
        net.infer_live(max_tokens=8, max_frames=64, seed=1, noise=torch.zeros(1, net.cfg.inter_channels, 64))
    with pytest.raises(ValueError, match="dec <="):
        net.infer_live(max_tokens=8, max_frames=64, ahead=TextAhead(dec=1000))
    with pytest.raises(ValueError, match="max_tokens"):
        net.infer_live(max_frames=64)
    with pytest.raises(ValueError, match="noise must be"):
        net.infer_live(max_tokens=8, max_frames=64, noise=torch.zeros(1, 3, 64))
    with pytest.raises(TypeError, match="one number"):
        net.infer_live(max_tokens=8, max_frames=64, length_scale=torch.ones(8))
    st = net.infer_live(max_tokens=8, max_frames=64, seed=1)
    with pytest.raises(ValueError, match="empty"):
        st.close()
    with pytest.raises(ValueError, match="max_tokens"):
        st.push(list(range(1, 10)))
    with pytest.raises(TypeError):
        st.push([1.5])
    with pytest.raises(TypeError):
        st.push(torch.zeros(3, dtype=torch.int32))
    st.push(3)
    st.push(torch.tensor([4, 5]))
    assert st.tokens == 3 and st.poll() == []
    st.close()
    with pytest.raises(ValueError, match="after close"):
        st.push([1])
    assert _counters(net) == before
    net.set_option("conv_bf16", 3)
    try:
        with pytest.raises(ValueError, match="conv_bf16"):
            net.infer_live(max_tokens=8, max_frames=64)
    finally:
        net.set_option("conv_bf16", 0)
    with pytest.raises(ValueError, match="sid is required"):
        _net("uudb").infer_live(max_tokens=8, max_frames=64)
    with pytest.raises(IndexError):
        _net("uudb").infer_live(sid=10 ** 6, max_tokens=8, max_frames=64)
    while not st.finished:
        st.poll()
    assert st.frames == sum(st.durations) > 0


def test_c_refusals_launch_nothing_and_leave_the_handle_usable():
    net = _net()
    h, L = net._ensure_handle(), _capi.lib()
    I = net.cfg.inter_channels
    st = net.infer_live(max_tokens=16, max_frames=400, seed=1, length_scale=2, block_tokens=8, ahead=TextAhead(tokens=0))
    st.push(_ids(16, 9))
    st.poll()
    assert st.plan.blocks == 2 and st.plan.frames > 40
    P = st.plan.frames
    s = net._stream()
    keep = []

    def refused(rc, what):
        assert rc == 1 and what in L.mbv_last_error(h).decode(), L.mbv_last_error(h).decode()

    # mbv_take_tokens_rows: an ended run, a range outside the row's text, NULL pointers, a short stride
    x = torch.tensor([_ids(16, 9)], device="cuda")
    xl = torch.tensor([16], device="cuda")
    y = torch.zeros(1, dtype=torch.int64, device="cuda")
    enc = (_capi.MbvEncRow * 1)()
    enc[0].length_scale, enc[0].noise_scale_w, enc[0].t_text = 1.0, 1.0, 16
    assert L.mbv_encode_rows(h, 1, x.data_ptr(), xl.data_ptr(), None, 1, 16, enc, y.data_ptr(), s) == 0
    # ... and a run on slot 0 that a later claim of its scratch ends (`align` lays the same buffer out)
    assert L.mbv_encode_rows(h, 0, x.data_ptr(), xl.data_ptr(), None, 1, 16, enc, y.data_ptr(), s) == 0
    spec = torch.rand(1, net.cfg.spec_channels, 40, generator=torch.Generator().manual_seed(4)).cuda() + 0.1
    net.align(x, xl, spec, torch.tensor([40]).cuda(), noise_scale=0, outputs=("w",))
    before = _counters(net)

    def take(**kw):
        row = _capi.MbvTakeRow()
        row.src, row.a, row.b, row.stride = 0, 0, 8, 16
        row.y_length, row.stats, row.dur = y.data_ptr(), st.stats.data_ptr(), st.dur.data_ptr()
        for k, v in kw.items():
            setattr(row, k, v)
        return (_capi.MbvTakeRow * 1)(row)
    refused(L.mbv_take_tokens_rows(h, 5, take(), 1, s), "without a preceding mbv_encode_rows on slot 5")
    refused(L.mbv_take_tokens_rows(h, 0, take(), 1, s), "without a preceding mbv_encode_rows on slot 0")
    refused(L.mbv_take_tokens_rows(h, 1, take(b=17, stride=32), 1, s), "outside the 16 tokens")
    refused(L.mbv_take_tokens_rows(h, 1, take(a=8, b=8), 1, s), "outside")
    refused(L.mbv_take_tokens_rows(h, 1, take(src=1), 1, s), "outside the run")
    refused(L.mbv_take_tokens_rows(h, 1, take(stats=None), 1, s), "missing")
    refused(L.mbv_take_tokens_rows(h, 1, take(dur=None), 1, s), "missing")
    refused(L.mbv_take_tokens_rows(h, 1, take(y_length=None), 1, s), "missing")
    refused(L.mbv_take_tokens_rows(h, 1, take(stride=7), 1, s), "stride")
    refused(L.mbv_take_tokens_rows(h, 1, None, 1, s), "bad arguments")

    # mbv_expand_ranges: durations that do not fit, negative durations, NULL pointers
    def expand(d, **kw):
        row = _capi.MbvExpandRange()
        dh = (C.c_int32 * len(d))(*d)
        row.stats, row.dur, row.stride, row.dur_host = st.stats.data_ptr(), st.dur.data_ptr(), 16, C.addressof(dh)
        row.a, row.b, row.frame, row.max_frames = 0, len(d), 0, 400
        row.noise, row.noise_stride, row.noise_scale = st.noise.data_ptr(), 400, 1.0
        row.z_p, row.z_stride = st.z_p.data_ptr(), 400
        for k, v in kw.items():
            setattr(row, k, v)
        keep.append(dh)
        return (_capi.MbvExpandRange * 1)(row)
    refused(L.mbv_expand_ranges(h, expand([100] * 8, frame=1), 1, s), "do not fit max_frames")
    refused(L.mbv_expand_ranges(h, expand([1, -1, 1]), 1, s), "negative duration")
    refused(L.mbv_expand_ranges(h, expand([1] * 8, z_p=None), 1, s), "missing")
    refused(L.mbv_expand_ranges(h, expand([1] * 8, noise=None), 1, s), "noise missing")
    refused(L.mbv_expand_ranges(h, expand([1] * 8, noise_stride=399), 1, s), "noise_stride")
    refused(L.mbv_expand_ranges(h, expand([1] * 8, z_stride=399), 1, s), "z_stride")
    refused(L.mbv_expand_ranges(h, expand([1] * 8, stride=7), 1, s), "stride")

    # mbv_flow_ranges: not computable yet, short strides, overlapping rows, conv_bf16.  NOT tested here: rows of more than
    # one run of mbv_flow_ranges_plan (it takes windows of several GiB; tests/test_text_plan.py holds the planner's cut)
    def flow(n=1, **kw):
        arr = (_capi.MbvFlowRange * n)()
        for row in arr:
            row.z_p, row.z_p_stride, row.P, row.complete = st.z_p.data_ptr(), 400, P, 0
            row.first, row.count, row.z, row.z_stride = 0, 8, st.z.data_ptr(), 400
            for k, v in kw.items():
                setattr(row, k, v)
        return arr
    refused(L.mbv_flow_ranges(h, flow(first=P - 32, count=1), 1, s), "row 0: frames [%d, %d + 1) are not computable yet" % (P - 32, P - 32))
    refused(L.mbv_flow_ranges(h, flow(first=P, count=1, complete=1), 1, s), "outside the %d expanded frames" % P)
    refused(L.mbv_flow_ranges(h, flow(z_stride=7), 1, s), "z_stride 7 < first + count")
    refused(L.mbv_flow_ranges(h, flow(z_p_stride=P - 1), 1, s), "z_p_stride")
    refused(L.mbv_flow_ranges(h, flow(z=None), 1, s), "missing")
    refused(L.mbv_flow_ranges(h, flow(n=2), 2, s), "overlapping ranges of one z")
    net.set_option("conv_bf16", 3)
    try:
        refused(L.mbv_flow_ranges(h, flow(), 1, s), "conv_bf16")
    finally:
        net.set_option("conv_bf16", 0)
    assert _counters(net) == before
    # the handle serves the next call: the stream finishes, and is what it is without the refusals in between
    st.close()
    while not st.finished:
        st.poll()
    clean = net.infer_live(max_tokens=16, max_frames=400, seed=1, length_scale=2, block_tokens=8, ahead=TextAhead(tokens=0))
    _drive(clean, _ids(16, 9), 16)
    assert torch.equal(clean.result(), st.result())


def test_a_stream_that_overflows_fails_alone():
    net = _net()
    pool = net.stream_pool()
    ids = _ids(24, 10)
    small = pool.add(net.infer_live(max_tokens=24, max_frames=20, seed=4, length_scale=3, block_tokens=8,
                                    ahead=TextAhead(tokens=0)))
    bad_id = pool.add(net.infer_live(max_tokens=24, max_frames=600, seed=4, block_tokens=8, ahead=TextAhead(tokens=0)))
    fine = pool.add(net.infer_live(max_tokens=24, max_frames=600, seed=4, length_scale=3, block_tokens=8,
                                   ahead=TextAhead(tokens=0)))
    small.push(ids)
    bad_id.push(ids[:8] + [10 ** 6] + ids[9:])
    fine.push(ids)
    for st in (small, bad_id, fine):
        st.close()
    for _ in range(64):
        if not len(pool):
            break
        pool.step()
    assert small.failed and bad_id.failed and small.finished and not len(pool)
    with pytest.raises(ValueError, match="token block [01] .*max_frames = 20"):
        small.poll()
    with pytest.raises(IndexError, match="token block 1 "):
        bad_id.poll()
    with pytest.raises(IndexError):
        bad_id.result()
    assert bad_id.plan.blocks == 1                  # block 0 was fine; nothing behind the failed block is encoded
    alone = net.infer_live(max_tokens=24, max_frames=600, seed=4, length_scale=3, block_tokens=8, ahead=TextAhead(tokens=0))
    _drive(alone, ids, 24)
    fine.poll()
    assert fine.finished and not fine.failed and torch.equal(fine.result(), alone.result())


def test_an_idle_text_stream_leaves_a_pooled_decode_stream_as_it_is():
    net = _net()
    x, xl = torch.tensor([_ids(30, 11)]), torch.tensor([30])
    alone = net.infer_stream(x, xl, seed=6, chunk_frames=16).run().clone()
    pool = net.stream_pool()
    idle = pool.add(net.infer_live(max_tokens=8, max_frames=64, seed=1))
    dec = pool.add(net.infer_stream(x, xl, seed=6, chunk_frames=16))
    before = (net.encoder_runs(), net.text_runs(), net.flow_runs())
    while not dec._drained():
        pool.step()
    assert (net.encoder_runs(), net.text_runs(), net.flow_runs()) == before
    assert torch.equal(dec.o, alone) and not idle.finished and len(pool) == 1
