"""Blended voices on the MI355X: a voice defined with `net.speaker` is the speaker id n_speakers + slot
on every entry that takes one; its row is the fp32 chain of the contract, a one-hot blend is the table row, and the
model cannot tell a voice from a row appended to `emb_g`."""
import numpy as np
import pytest
import torch

from mb_istft_vits_amd import models, utils as mutils
from mb_istft_vits_amd.models import ConvertRequest, Request

import speaker_ref
from gpu_util import make_net

pytestmark = pytest.mark.gpu

NAME = "uudb_ms_istft_vits_ms"
MODEL_SR, HOP, WIN, N_FFT = 16000, 256, 1024, 1024
NS = 12
_STATE = {}


def _net():
    if "net" not in _STATE:
        _STATE["net"] = make_net(NAME)[0]
        assert _STATE["net"].n_speakers == NS and _STATE["net"].cfg.gin_channels == 256
    return _STATE["net"]


def _table(net):
    return net.emb_g.weight.detach().cpu().numpy().astype(np.float64)


def _seed(s):
    torch.manual_seed(s)
    torch.cuda.manual_seed(s)


def _ids(T, seed):
    return torch.randint(1, 59, (T,), generator=torch.Generator().manual_seed(seed))


def _text(B, T, seed):
    x = torch.stack([_ids(T, seed + b) for b in range(B)])
    xl = torch.tensor([T - 3 * b for b in range(B)])
    return x.cuda(), xl.cuda()


def _audio(n, seed):
    rs = np.random.RandomState(seed)
    t = np.arange(n) / MODEL_SR
    x = (0.3 * np.sin(2 * np.pi * (180 + 7 * seed) * t) + 0.2 * np.sin(2 * np.pi * 1234.5 * t + seed)
         + 0.05 * rs.standard_normal(n)).astype(np.float32)
    return torch.from_numpy(x)


def _tensors(out):
    """Every tensor of an entry's result tuple, nested tuples flattened (timings dicts and None dropped)."""
    flat = []
    for v in out:
        if isinstance(v, (tuple, list)):
            flat += _tensors(v)
        elif torch.is_tensor(v):
            flat.append(v)
    return flat


def _equal(a, b):
    a, b = _tensors(a), _tensors(b)
    return len(a) == len(b) > 0 and all(p.shape == q.shape and torch.equal(p, q) for p, q in zip(a, b))


def _same_stream(a, b):
    return (a.z.shape == b.z.shape and torch.equal(a.z, b.z) and torch.equal(a.g, b.g)
            and torch.equal(a.y_lengths, b.y_lengths) and a.schedule == b.schedule)


@pytest.fixture(autouse=True)
def blend_launches():
    """`mbv_speaker_runs` moves by exactly one per `net.speaker` / `net.speakers` call made through `define` and by
    `extra` (the refreshes of the last test) — and by nothing else any test of this file does."""
    net = _net()
    book = {"calls": 0, "extra": 0}

    def define(*specs, **kw):
        before = net.speaker_runs()
        out = net.speaker(**kw) if kw else net.speakers(list(specs))
        assert net.speaker_runs() - before == 1
        book["calls"] += 1
        return out

    book["define"] = define
    start = net.speaker_runs()
    yield book
    assert net.speaker_runs() - start == book["calls"] + book["extra"], book


# ------------------------------------------------------------------ 1. row parity
def _parity_cases():
    rs = np.random.RandomState(5)
    cases = []
    for K in (1, 2, 3, 12, 16):
        ids = rs.permutation(NS)[:K].tolist() if K <= NS else rs.randint(0, NS, K).tolist()
        w = rs.uniform(0.1, 1.0, K)
        cases.append(dict(ids=ids, weights=w.tolist(), normalize=True))
        neg = rs.uniform(0.2, 1.5, K)
        neg[K // 2] = -0.5
        cases.append(dict(ids=ids, weights=neg.tolist(), normalize=False))
        zero = rs.uniform(0.1, 1.0, K)
        zero[-1] = 0.0
        cases.append(dict(ids=ids, weights=zero.tolist(), normalize=False))
    return cases


def test_rows_are_within_the_fma_chain_bound_of_float64(blend_launches):
    net = _net()
    table = _table(net)
    cases = _parity_cases()
    voices = blend_launches["define"](*cases)                     # fifteen voices, one launch
    assert [v.sid for v in voices] == [NS + v.slot for v in voices] and len({v.slot for v in voices}) == 15
    worst = 0.0
    for c, v in zip(cases, voices):
        assert list(v.ids) == c["ids"] and list(v.weights) == models.blend_weights(c["weights"], c["normalize"])
        row = v.row()
        assert row.shape == (256,) and row.dtype == torch.float32 and row.is_cuda
        got = row.cpu().numpy().astype(np.float64)
        want = speaker_ref.blend(table, v.ids, v.weights)
        bound = speaker_ref.bound(table, v.ids, v.weights)
        err = np.abs(got - want)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(bound > 0, err / bound, 0.0)
        worst = max(worst, float(ratio.max()))
        print("K=%2d normalize=%-5s max err %.3e  max err/bound %.3f" % (len(v.ids), c["normalize"], err.max(), ratio.max()))
        assert np.all(err <= bound), (c, float(ratio.max()))
    print("row parity: worst err / bound over the fifteen voices = %.3f" % worst)
    # the same definition alone is the same row, and rows of several voices come back in one gather
    alone = blend_launches["define"](**cases[9])
    assert torch.equal(alone.row(), voices[9].row())
    both = net.emb_g(torch.tensor([voices[3].sid, 4, voices[14].sid]).cuda())
    assert torch.equal(both[0], voices[3].row()) and torch.equal(both[2], voices[14].row())
    assert torch.equal(both[1], net.emb_g.weight[4])
    for v in voices + [alone]:
        v.release()


# ------------------------------------------------------------------ 2. one-hot is the table
def test_a_one_hot_blend_is_the_table_row(blend_launches):
    net = _net()
    a = blend_launches["define"](ids=[5], weights=[1.0])
    b = blend_launches["define"](ids=[2, 5, 9], weights=[0, 1, 0])
    for v in (a, b):
        assert torch.equal(v.row(), net.emb_g.weight[5])
    x, xl = _text(1, 20, 40)
    _seed(3)
    plain = net.infer(x, xl, sid=torch.tensor([5]).cuda(), noise_scale=0.667)
    for v in (a, b):
        _seed(3)
        assert _equal(net.infer(x, xl, sid=torch.tensor([v.sid]).cuda(), noise_scale=0.667), plain)
    _seed(3)
    assert _equal(net.infer(x, xl, sid=a, noise_scale=0.667), plain)          # the Speaker for its one-element tensor
    _seed(3)
    other = net.infer(x, xl, sid=torch.tensor([6]).cuda(), noise_scale=0.667)
    assert not torch.equal(other[0], plain[0])                                # not vacuous: the speaker reaches o
    a.release()
    b.release()


# ------------------------------------------------------------------ 3. a voice is an appended table row
def _net13(net, row):
    hps = mutils.get_hparams_from_file(mutils.builtin_config(NAME))
    big = models.SynthesizerTrn(59, hps.data.filter_length // 2 + 1, hps.train.segment_size // hps.data.hop_length,
                                n_speakers=NS + 1, **hps.model)
    sd = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    sd["emb_g.weight"] = torch.cat([sd["emb_g.weight"], row.detach().cpu()[None]])
    big.load_state_dict(sd)
    return big.cuda().eval()


def test_a_voice_is_an_appended_table_row(blend_launches):
    net = _net()
    v = blend_launches["define"](ids=[3, 7], weights=[0.7, 0.3])
    assert not any(torch.equal(v.row(), net.emb_g.weight[k]) for k in range(NS))
    big = _net13(net, v.row())
    assert torch.equal(big.emb_g.weight[NS], v.row())

    def sids(*ids):
        return torch.tensor(ids).cuda()

    # infer, in a batch that also holds a plain speaker
    x, xl = _text(2, 24, 60)
    _seed(11)
    want = big.infer(x, xl, sid=sids(NS, 4), noise_scale=0.667)
    _seed(11)
    got = net.infer(x, xl, sid=sids(v.sid, 4), noise_scale=0.667)
    assert _equal(got, want)
    # voice conversion: the voice as target, and as source
    wave = torch.stack([_audio(HOP * 40, 1), _audio(HOP * 40, 2)]).cuda()
    y, yl = net.spectrogram(wave, N_FFT, HOP, WIN)
    yl = torch.tensor([int(yl[0]), int(yl[1]) - 7]).cuda()
    _seed(12)
    want = big.voice_conversion(y, yl, sids(3, NS), sids(NS, 5))
    _seed(12)
    got = net.voice_conversion(y, yl, sids(3, v.sid), sids(v.sid, 5))
    assert _equal(got, want)
    # align
    x2, xl2 = _text(2, 20, 70)
    _seed(13)
    want = big.align(x2, xl2, y, yl, sid=sids(NS, 2))
    _seed(13)
    got = net.align(x2, xl2, y, yl, sid=sids(v.sid, 2))
    assert _equal(got, want)
    # the first two chunks of a stream
    x1, xl1 = _text(1, 24, 80)
    _seed(14)
    a = big.infer_stream(x1, xl1, sids(NS), noise_scale=0.5, chunk_frames=8, max_chunk_frames=32)
    _seed(14)
    b = net.infer_stream(x1, xl1, sids(v.sid), noise_scale=0.5, chunk_frames=8, max_chunk_frames=32)
    assert _same_stream(a, b) and len(a.schedule) >= 2
    for _ in range(2):
        (fa, va), (fb, vb) = next(a), next(b)
        assert fa == fb and torch.equal(va, vb)
    v.release()


# ------------------------------------------------------------------ 4. every route takes it
def test_every_route_takes_a_voice(blend_launches):
    net = _net()
    v = blend_launches["define"](ids=[1, 8, 10], weights=[2, 1, 1])
    assert list(v.weights) == [0.5, 0.25, 0.25]
    runs = net.speaker_runs()
    # one admission mixes a plain id, the Speaker and its int
    texts = [_ids(T, 90 + T) for T in (17, 24, 9)]

    def admit(sids):
        before = net.encoder_runs()
        sts = net.infer_streams([Request(x, sid=s, noise_scale=0.667, seed=500 + k, chunk_frames=8, max_chunk_frames=32)
                                 for k, (x, s) in enumerate(zip(texts, sids))])
        return sts, net.encoder_runs() - before

    plain, plain_runs = admit([3, 4, 5])
    mixed, mixed_runs = admit([3, v, v.sid])
    assert mixed_runs == plain_runs >= 1
    assert _same_stream(mixed[0], plain[0]) and not torch.equal(mixed[1].g, plain[1].g)
    for k, (x, s) in enumerate(zip(texts, [3, v.sid, v.sid])):
        alone = net.infer_stream(x[None].cuda(), torch.tensor([x.numel()]).cuda(), torch.tensor([s]).cuda(),
                                 noise_scale=0.667, seed=[500 + k], chunk_frames=8, max_chunk_frames=32)
        assert _same_stream(mixed[k], alone), k
        assert torch.equal(mixed[k].run(), alone.run()), k
    assert torch.equal(mixed[1].g[0], v.row())
    # conversion with a voice target, more than 256 frames: pooled and live against convert_stream
    F = 260
    wave = _audio(HOP * F + 5, 3).cuda()
    noise = torch.randn(1, net.cfg.inter_channels, F + 12, generator=torch.Generator().manual_seed(8)).cuda()
    ref = net.convert_stream(wave, 3, v, MODEL_SR, HOP, WIN, seed=[77], chunk_frames=32, max_chunk_frames=256)
    assert ref.z.shape[2] == F and torch.equal(ref.g[0], v.row())
    pooled = net.convert_streams([ConvertRequest(wave, 3, v, MODEL_SR, HOP, WIN, seed=77, chunk_frames=32,
                                                 max_chunk_frames=256)])[0]
    assert _same_stream(pooled, ref)
    want = ref.run()
    assert torch.equal(pooled.run(), want)
    ref_n = net.convert_stream(wave, 3, v.sid, MODEL_SR, HOP, WIN, noise=noise[:, :, :F], chunk_frames=32,
                               max_chunk_frames=256)
    want = [(a, o.clone()) for a, o in ref_n]
    live = net.convert_live(3, v, MODEL_SR, HOP, WIN, HOP * (F + 12), noise=noise, chunk_frames=32, max_chunk_frames=256)
    got = []
    half = wave.numel() // 2
    for piece in (wave[:half], wave[half:]):
        live.push(piece)
        got += [(a, o.clone()) for a, o in live.poll()]
    live.close()
    got += [(a, o.clone()) for a, o in live.poll()]
    assert live.finished and live.sid_tgt == v.sid
    assert [a for a, _ in got] == [a for a, _ in want]
    assert all(torch.equal(p, q) for (_, p), (_, q) in zip(got, want))
    assert torch.equal(live.z[:, :, :F], ref_n.z) and torch.equal(live.g, ref_n.g)
    assert net.speaker_runs() == runs                                         # nothing above launched a blend
    v.release()


# ------------------------------------------------------------------ 5. refusals and lifetime
def test_refusals_and_lifetime(blend_launches):
    net = _net()
    v = blend_launches["define"](ids=[0, 11], weights=[1, 1])
    free = NS + 200                                                           # a slot nobody defined
    texts = [_ids(12, 1), _ids(12, 2), _ids(12, 3)]
    # in a sid tensor: only its own row is flagged, as for any id outside the table
    for bad in (free, NS + 256, -1, 10 ** 6):
        with pytest.raises(IndexError, match=r"^request 1: index out of range"):
            net.infer_streams([Request(x, sid=s, seed=k) for k, (x, s) in enumerate(zip(texts, [2, bad, v]))])
    x, xl = _text(2, 12, 5)
    with pytest.raises(IndexError):
        net.infer(x, xl, sid=torch.tensor([v.sid, free]).cuda())
    with pytest.raises(IndexError):
        net.emb_g(torch.tensor([v.sid, free]).cuda())
    # as a host value it raises before anything runs
    wave = _audio(HOP * 30, 4)
    for src, tgt in ((3, free), (free, 3)):
        with pytest.raises(IndexError, match="outside"):
            net.convert_stream(wave, src, tgt, MODEL_SR, HOP, WIN)
        with pytest.raises(IndexError, match="outside"):
            net.convert_live(src, tgt, MODEL_SR, HOP, WIN, HOP * 40)
    # release, then the slot is handed out again and gives the new row
    slot, old_sid, old_row = v.slot, v.sid, v.row().clone()
    v.release()
    assert v.released
    with pytest.raises(ValueError, match="released"):
        Request(texts[0], sid=v)
    with pytest.raises(ValueError, match="released"):
        net.convert_live(3, v, MODEL_SR, HOP, WIN, HOP * 40)
    with pytest.raises(IndexError):                                           # the stale id, on the device and on the host
        net.infer(x, xl, sid=torch.tensor([3, old_sid]).cuda())
    with pytest.raises(IndexError):
        net.convert_stream(wave, 3, old_sid, MODEL_SR, HOP, WIN)
    w = blend_launches["define"](ids=[4], weights=[1.0])
    assert w.slot == slot and w.sid == old_sid
    assert torch.equal(w.row(), net.emb_g.weight[4]) and not torch.equal(w.row(), old_row)
    # a voice an open LiveStream passes on every tick cannot be released
    live = net.convert_live(3, w, MODEL_SR, HOP, WIN, HOP * 40, chunk_frames=8, max_chunk_frames=32)
    with pytest.raises(ValueError, match="LiveStream"):
        w.release()
    assert not w.released and torch.equal(w.row(), net.emb_g.weight[4])
    live.push(wave.cuda())
    live.close()
    while not live.finished:
        assert live.poll()
    w.release()                                                               # the stream has finished: free to go
    # a decode stream copied g when it was created and holds nothing
    u = blend_launches["define"](ids=[6, 7], weights=[1, 3])
    st = net.infer_stream(x[:1], xl[:1], torch.tensor([u.sid]).cuda(), seed=[4], chunk_frames=8, max_chunk_frames=32)
    want = net.infer_stream(x[:1], xl[:1], torch.tensor([u.sid]).cuda(), seed=[4], chunk_frames=8, max_chunk_frames=32).run()
    u.release()
    assert torch.equal(st.run(), want)
    # definition errors raise before a launch
    runs = net.speaker_runs()
    taken = len(net._voice_slots)
    gin = net.cfg.gin_channels
    for kw in (dict(ids=[3, NS], weights=[1, 1]), dict(ids=[3, old_sid], weights=[1, 1]), dict(ids=[-1], weights=[1]),
               dict(ids=list(range(12)) + [0, 1, 2, 3, 4], weights=[1.0] * 17),
               dict(ids=[1, 2], weights=[1.0, float("inf")]), dict(ids=[1, 2], weights=[1.0, float("nan")], normalize=False),
               dict(ids=[1, 2], weights=[1.0, -1.0]), dict(ids=[1, 2], weights=[1.0]), dict(ids=[], weights=[]),
               dict(vector=torch.zeros(gin + 1)), dict(vector=torch.zeros(gin - 1)), dict(vector=torch.zeros(2, gin)),
               dict(vector=torch.full((gin,), float("nan"))), dict(vector=torch.zeros(gin), ids=[1]), dict()):
        with pytest.raises(ValueError):
            net.speaker(**kw)
    with pytest.raises(ValueError):                                           # all or nothing
        net.speakers([dict(ids=[1], weights=[1]), dict(ids=[NS], weights=[1])])
    assert net.speaker_runs() == runs and len(net._voice_slots) == taken


# ------------------------------------------------------------------ 6. refresh
def test_a_blend_follows_the_table_and_a_vector_does_not(blend_launches):
    net = _net()
    gin = net.cfg.gin_channels
    given = torch.randn(gin, generator=torch.Generator().manual_seed(21))
    v = blend_launches["define"](ids=[3, 7, 9], weights=[0.5, 0.3, 0.2])
    vec = blend_launches["define"](vector=given)
    assert vec.ids is None and vec.weights is None and torch.equal(vec.row().cpu(), given)
    old_table = net.emb_g.weight.detach().clone()
    old_row = v.row().clone()
    x, xl = _text(1, 16, 33)
    try:
        new_table = torch.randn(NS, gin, generator=torch.Generator().manual_seed(22)).cuda()
        net.emb_g.weight.data.copy_(new_table)
        net.refresh_weights()
        runs = net.speaker_runs()
        blend_launches["extra"] += 1                                          # every blend again, in ONE launch
        row = v.row()
        assert net.speaker_runs() - runs == 0, "the refresh itself blended, before this call's gather"
        table = new_table.cpu().numpy().astype(np.float64)
        err = np.abs(row.cpu().numpy().astype(np.float64) - speaker_ref.blend(table, v.ids, v.weights))
        assert np.all(err <= speaker_ref.bound(table, v.ids, v.weights)) and not torch.equal(row, old_row)
        assert torch.equal(vec.row().cpu(), given)
        out = net.infer(x, xl, sid=torch.tensor([vec.sid]).cuda(), noise_scale=0, outputs=("o",))[0]
        assert bool(torch.isfinite(out).all())
    finally:
        net.emb_g.weight.data.copy_(old_table)
        net.refresh_weights()
        blend_launches["extra"] += 1
        assert torch.equal(v.row(), old_row)
    v.release()
    vec.release()
