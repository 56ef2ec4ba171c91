"""-m gpu: the bytes of the wire kernels, pinned.  Every case of tests/wire_matrix_cases.py runs through
`net.resample_pcm16_range`, `net.resample_pcm16_chunks` or `net.resample_turns` in two calls (a frontier below the row's
end, then a range that starts inside a tile), and the SHA-256 over everything the calls stored (samples, packed
buffers, `out_samples`, the running-peak bits; the untouched sentinels around them included) is compared with
tests/golden/wire_matrix.json, recorded once by tests/golden/make_wire_matrix.py from the commit named there.  The
other wire suites compare one path of these kernels with another; this one holds all of them to recorded bytes.  No
tolerance, no skip."""
import hashlib
import json
import os

import pytest
import torch

from mb_istft_vits_amd import _capi, wire

import wire_matrix_cases as M
from gpu_util import make_net

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wire_matrix.json")
SENTINEL = {"pcm16": -12345, "ulaw": 0x5A, "alaw": 0x5A}
_STATE = {}


def _setup():
    """the model and the device copies of the inputs, once"""
    if not _STATE:
        data = M.inputs()
        _STATE["net"] = make_net("ljs_mini_mb_istft_vits")[0]
        _STATE["x"] = torch.from_numpy(data["x"]).cuda()
        _STATE["gains"] = torch.from_numpy(data["gains"]).cuda()
        _STATE["segs"] = [torch.from_numpy(s).cuda() for s in data["segs"]]
    return _STATE


def _bytes(*tensors):
    return b"".join(t.cpu().numpy().tobytes() for t in tensors)


def _ranges(case, lookahead):
    """(in_avail, out_first, out_count) of the two calls for a row under that lookahead, and the row's width"""
    orig, target = case["orig"], case["target"]
    r1 = wire.limiter_ready(orig, target, M.FIRST_AVAIL, M.N_IN, lookahead)
    total = wire.resample_ready(orig, target, M.N_IN, M.N_IN)
    assert 0 < r1 < total and r1 % 256
    return [(M.FIRST_AVAIL, 0, r1), (M.N_IN, r1, total - r1)], total


def _ranged(net, case, st):
    lim = M.LIMIT if case["lim"] else None
    calls, total = _ranges(case, lim[1] if lim else 0)
    law = case["law"]
    pcm = torch.full((2, total + 3), SENTINEL[law], device="cuda", dtype=torch.int16 if law == "pcm16" else torch.uint8)
    ns = torch.full((2,), -1, device="cuda", dtype=torch.int64)
    running = torch.zeros(2, device="cuda")
    valid = torch.full((2,), M.VALID, device="cuda", dtype=torch.int64)
    peak = torch.full((2,), M.PEAK, device="cuda")
    fade = (calls[0][2] - M.FADE_BACK, M.FADE_COUNT) if case["fade"] else None
    env = wire.Envelope(st["gains"][:2], M.HOP) if case["env"] else None
    for in_avail, first, count in calls:
        net.resample_pcm16_range(st["x"][:2], case["orig"], case["target"], in_avail, first, count, pcm,
                                 valid_samples=valid, peak=peak, running_peak=running, out_samples=ns, limiter=lim,
                                 encoding=law, fade=fade, envelope=env)
    return _bytes(pcm, ns, running)


def _rows_of(case):
    """(input row, limiter, fades, shaped, empty range) of every row of a pooled case"""
    if case["entry"] == "mixed":
        return [(0, M.LIMIT, True, True, False), (1, None, False, True, False), (2, None, True, False, False),
                (0, M.LIMIT, False, False, False), (1, None, False, False, True)]
    lim = M.LIMIT if case["lim"] else None
    return [(0, lim, True, case["env"], False), (1, lim, False, False, False), (2, lim, False, case["env"], True)]


def _pooled(net, case, st):
    law, turns = case["law"], case["entry"] == "turns"
    dtype = torch.int16 if law == "pcm16" else torch.uint8
    rows = _rows_of(case)
    peak = torch.tensor([M.PEAK], device="cuda")
    valid = torch.tensor([M.VALID], device="cuda", dtype=torch.int64)
    state, packs, keep = [], [], []
    for b, lim, _, _, _ in rows:
        calls, total = _ranges(case, lim[1] if lim else 0)
        state.append((calls, torch.full((total + 3,), SENTINEL[law], device="cuda", dtype=dtype),
                      torch.zeros(1, device="cuda"), torch.full((1,), -1, device="cuda", dtype=torch.int64)))
    starts = M.seg_starts()
    for step in range(2):
        chunks, fades, envs = [], [], []
        for (b, lim, fading, shaped, empty), (calls, pcm, running, ns) in zip(rows, state):
            in_avail, first, count = calls[step]
            k = _capi.MbvTurnChunk() if turns else _capi.MbvPcmChunk()
            c = k.chunk if turns else k
            c.wave = None if turns else st["x"][b].data_ptr()
            c.in_total, c.valid_samples, c.in_avail = M.N_IN, valid.data_ptr(), in_avail
            c.out_first, c.out_count = first, 0 if empty else count
            c.peak, c.pcm, c.pcm_capacity = peak.data_ptr(), pcm.data_ptr(), pcm.numel()
            c.running_peak, c.out_samples = running.data_ptr(), ns.data_ptr()
            fades.append((calls[0][2] - M.FADE_BACK, M.FADE_COUNT) if fading else None)
            if turns:
                segs = (_capi.MbvTurnSeg * len(starts))()
                for s, sg in enumerate(segs):
                    sg.wave, sg.start, sg.length = st["segs"][s].data_ptr(), starts[s], M.SEG_LENGTHS[s]
                    sg.ramp = wire.turn_ramp(M.RAMP, M.SEG_LENGTHS[s])
                k.segs, k.n_segs = segs, len(starts)
                keep.append(segs)
                envs.append([wire.Envelope(st["gains"][s], M.HOP) if s in M.SEG_ENVELOPES else None
                             for s in range(len(starts))] if shaped else None)
            else:
                envs.append(wire.Envelope(st["gains"][b], M.HOP) if shaped else None)
            chunks.append(k)
        count = sum((k.chunk if turns else k).out_count for k in chunks)
        packed = torch.full((count + 8,), SENTINEL[law], device="cuda", dtype=dtype)
        call = net.resample_turns if turns else net.resample_pcm16_chunks
        call(chunks, case["orig"], case["target"], packed=packed, limits=[lim for _, lim, _, _, _ in rows], encoding=law,
             fades=fades, envelopes=envs if case["env"] else None)
        packs.append(packed)
    return b"".join(_bytes(pcm, ns, running) for _, pcm, running, ns in state) + _bytes(*packs)


def digest_of(case):
    """SHA-256 (hex) over what the two calls of the case stored"""
    st = _setup()
    run = _ranged if case["entry"] == "range" else _pooled
    return hashlib.sha256(run(st["net"], case, st)).hexdigest()


@pytest.mark.parametrize("case", M.cases(), ids=lambda c: c["id"])
def test_the_stored_bytes_are_those_recorded(case):
    with open(GOLDEN) as f:
        golden = json.load(f)["digests"]
    assert digest_of(case) == golden[case["id"]]
