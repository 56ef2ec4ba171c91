"""CPU-only checks of the pooled wire output's host side: `mbv_pcm_chunks_plan` against per-chunk
`mbv_resample_ready`, the ctypes mirror of `mbv_pcm_chunk`, and the refusals `wire.PcmPool.add` makes before anything
is launched.  No GPU is touched."""
import ctypes as C
import os
import re
import types

import pytest
import torch

from mb_istft_vits_amd import _capi, stream, wire

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = [(22050, 24000), (22050, 16000), (22050, 22050), (16000, 24000), (24000, 22050), (16000, 8000)]
FILTERS = {"kaiser_best": 0, "kaiser_fast": 1}
N_IN = 6000


def _lag(orig, target, filt):
    """input samples the wire holds back: K - left - 1 of the bank geometry (0 for equal rates: no FIR)"""
    if orig == target:
        return 0
    taps, left = C.c_int32(), C.c_int32()
    assert _capi.lib().mbv_resample_bank(orig, target, filt, None, 0, None, C.byref(taps), C.byref(left)) == 0
    return taps.value - left.value - 1


def _ready(orig, target, filt, in_avail, in_total):
    r = _capi.lib().mbv_resample_ready(orig, target, filt, in_avail, in_total)
    assert r >= 0
    return int(r)


def _chunk(in_total, in_avail, first, count, cap):
    k = _capi.MbvPcmChunk()                       # pointers stay NULL: the plan reads the integer fields only
    k.in_total, k.in_avail, k.out_first, k.out_count, k.pcm_capacity = in_total, in_avail, first, count, cap
    return k


def _plan(orig, target, filt, chunks):
    arr = (_capi.MbvPcmChunk * max(len(chunks), 1))(*chunks)
    first = (C.c_int64 * max(len(chunks), 1))(*([-7] * max(len(chunks), 1)))
    L = _capi.lib()
    total = L.mbv_pcm_chunks_plan(orig, target, filt, arr, len(chunks), first)
    return int(total), list(first)[:len(chunks)], (L.mbv_last_error(None) or b"").decode()


def _frontiers(lag):
    """around the lag in steps of 1 and of 7, the row's end and beyond"""
    f = [lag + d for d in range(-3, 4)] + [lag + 7 * d for d in range(-2, 9)] + [0, 1, 300, 777, N_IN - 1, N_IN, N_IN + 5]
    return sorted(set(v for v in f if v >= 0))


@pytest.mark.parametrize("res_type", sorted(FILTERS))
@pytest.mark.parametrize("orig,target", PAIRS)
def test_plan_is_per_chunk_resample_ready(orig, target, res_type):
    filt = FILTERS[res_type]
    lag = _lag(orig, target, filt)
    cap = _ready(orig, target, filt, N_IN, N_IN)
    fr = _frontiers(lag)
    ready = [_ready(orig, target, filt, f, N_IN) for f in fr]
    assert ready[0] == 0 and ready[-1] == cap and ready == sorted(ready)
    if orig != target:
        assert _ready(orig, target, filt, lag, N_IN) == 0 < _ready(orig, target, filt, lag + 7, N_IN)
    # every range exactly at ready is accepted, in one call; packed_first is the prefix sum
    good = [_chunk(N_IN, f, r // 3, r - r // 3, cap) for f, r in zip(fr, ready)]
    total, first, _ = _plan(orig, target, filt, good)
    counts = [k.out_count for k in good]
    assert total == sum(counts) and 0 in counts          # (empty chunks are allowed)
    assert first == [sum(counts[:i]) for i in range(len(counts))]
    assert (total, first) == wire.pcm_chunks_plan(orig, target, good, res_type)
    # one past ready: refused, and the message names the chunk
    for i, (f, r) in enumerate(zip(fr, ready)):
        if r == cap:
            continue
        bad = list(good)
        bad[i] = _chunk(N_IN, f, r // 3, r - r // 3 + 1, cap)
        total, _, msg = _plan(orig, target, filt, bad)
        assert total == -1 and ("chunk %d:" % i) in msg and "final" in msg, (i, msg)
        bad[i] = _chunk(N_IN, f, r + 1, 0, cap)            # an empty range that starts past ready
        total, _, msg = _plan(orig, target, filt, bad)
        assert total == -1 and ("chunk %d:" % i) in msg, (i, msg)
    with pytest.raises(_capi.MbvError, match="chunk 2:"):
        wire.pcm_chunks_plan(orig, target, good[:2] + [_chunk(N_IN, fr[0], 0, ready[0] + 1, cap)], res_type)
    # the row's capacity bounds the range too
    k = len(good) - 1
    for bad_k in (_chunk(N_IN, N_IN, 0, cap, cap - 1), _chunk(N_IN, N_IN, cap, 1, cap + 10), _chunk(N_IN, N_IN, -1, 1, cap),
                  _chunk(N_IN, N_IN, 0, -1, cap), _chunk(N_IN, -1, 0, 0, cap), _chunk(0, 0, 0, 0, cap),
                  _chunk(N_IN, N_IN, 0, 0, 0)):
        total, _, msg = _plan(orig, target, filt, good[:k] + [bad_k])
        assert total == -1 and ("chunk %d:" % k) in msg, msg
    # a capacity above the row's outputs changes nothing: ready still bounds
    assert _plan(orig, target, filt, [_chunk(N_IN, N_IN, 0, cap, cap + 10)])[0] == cap


def test_plan_edge_cases():
    L = _capi.lib()
    assert _plan(22050, 24000, 0, [])[0] == 0                            # n = 0
    assert L.mbv_pcm_chunks_plan(22050, 24000, 0, None, 0, None) == 0
    assert L.mbv_pcm_chunks_plan(22050, 24000, 0, None, 2, None) == -1
    one = (_capi.MbvPcmChunk * 1)(_chunk(1000, 1000, 0, 10, 2000))
    assert L.mbv_pcm_chunks_plan(22050, 24000, 0, one, 1, None) == 10    # packed_first is optional
    assert L.mbv_pcm_chunks_plan(22050, 24000, 2, one, 1, None) == -1    # unknown filter
    assert b"filter" in L.mbv_last_error(None)
    assert L.mbv_pcm_chunks_plan(22050, 22050, 7, one, 1, None) == -1
    assert L.mbv_pcm_chunks_plan(22050, 22051, 0, one, 1, None) == -1    # a rate pair mbv_resample refuses (22051 phases)
    assert b"phases" in L.mbv_last_error(None)
    assert L.mbv_resample_ready(22050, 22051, 0, 10, 10) == -1
    assert L.mbv_pcm_chunks_plan(0, 24000, 0, one, 1, None) == -1
    assert L.mbv_pcm_chunks_plan(22050, -1, 0, one, 1, None) == -1
    # a row shorter than the filter's half-width is final only once it is complete
    assert _plan(22050, 24000, 0, [_chunk(13, 12, 0, 0, 15)])[0] == 0
    assert _plan(22050, 24000, 0, [_chunk(13, 12, 0, 1, 15)])[0] == -1
    assert _plan(22050, 24000, 0, [_chunk(13, 13, 0, 15, 15)])[0] == 15
    with pytest.raises(ValueError):
        wire.pcm_chunks_plan(22050, 24000, [], "soxr_hq")


def test_pcm_chunk_struct_layout_matches_header():
    hdr = open(os.path.join(ROOT, "include", "mbistft_vits.h")).read()
    body = re.search(r"typedef struct mbv_pcm_chunk \{(.*?)\} mbv_pcm_chunk;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        pointer = "*" in decl
        ctype = C.c_void_p if pointer else {"int64_t": C.c_int64}[decl.split()[0]]
        for name in decl.replace("*", " ").split(",")[0:]:
            fields.append((name.split()[-1], ctype))
    assert [(n, t) for n, t in _capi.MbvPcmChunk._fields_] == fields
    assert C.sizeof(_capi.MbvPcmChunk) == 8 * 11                         # 11 pointers / int64s, no padding
    for i, (name, _) in enumerate(fields):
        assert getattr(_capi.MbvPcmChunk, name).offset == 8 * i


def test_pcm_pool_add_refuses_before_any_launch():
    """The refusals need no device: nothing is allocated or launched before them."""
    net = types.SimpleNamespace(cfg=types.SimpleNamespace(samples_per_frame=256))
    pool = stream.StreamPool(net)
    pp = wire.pcm_pool(net, pool, 22050, 24000)
    assert isinstance(pp, wire.PcmPool) and len(pp) == 0 and pp.step() == []
    two = stream.DecodeStream(net, None, torch.zeros(2, 192, 40), None, 32, 256)
    with pytest.raises(ValueError, match="ONE utterance"):
        pp.add(two)
    with pytest.raises(TypeError):
        pp.add("not a stream")
    other = types.SimpleNamespace(cfg=net.cfg)
    with pytest.raises(ValueError, match="another model"):
        pp.add(stream.DecodeStream(other, None, torch.zeros(1, 192, 40), None, 32, 256))
    assert len(pp) == 0 and len(pool) == 0
    with pytest.raises(ValueError, match="another model"):
        wire.pcm_pool(other, pool, 22050, 24000)
    with pytest.raises(ValueError, match="res_type"):
        wire.pcm_pool(net, pool, 22050, 24000, res_type="soxr_hq")
    with pytest.raises(ValueError, match="not in the pool"):
        pp.step([two])
