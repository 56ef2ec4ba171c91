"""`stream.TextPlan` / `stream.TextAhead` and the host-only entries of live text, without a GPU: what is
encoded, flowed and decoded, and from what, does not depend on the pushes, and equals a brute-force restatement that
decides readiness token by token and frame by frame (`live_text_ref.py`)."""
import ctypes as C
import os
import random
import re

import pytest

from mb_istft_vits_amd import _capi, stream
from mb_istft_vits_amd.stream import TextAhead, TextPlan

from live_text_ref import RefText, schedule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SR, SPF = 22050, 256


def _case(rs):
    N = rs.randint(1, 80)
    bt = rs.choice([1, 2, 3, 5, 8, 16, 40])
    A = rs.choice([None, 0, 1, 4, 16, 100])
    R = rs.choice([0, 3, 32])
    r_dec = rs.choice([0, 5, 11])
    dec = rs.choice([None, 0, min(2, r_dec), r_dec])
    chunk = rs.choice([1, 4, 32])
    cap = chunk * rs.choice([1, 2, 8])
    ff = rs.choice([1, 7, 32])
    seam_ms = 5.0 if dec and rs.random() < 0.5 else 0.0           # 110 samples at 22.05 kHz: one frame of overhang
    seed = rs.randrange(1 << 30)
    zero = rs.random() < 0.3                                       # tokens without frames among them

    def dur_of(t, E):
        return random.Random(seed * 1000003 + t * 131 + E).choice([0] if zero and t % 3 == 0 else [1, 2, 5, 9, 30])
    return dict(N=N, bt=bt, A=A, R=R, r_dec=r_dec, dec=dec, chunk=chunk, cap=cap, ff=ff, seam_ms=seam_ms, dur_of=dur_of)


def _events(rs, N, pattern):
    """[("push", n) | ("close",) | ("tick",)]"""
    if pattern == "all":
        return [("push", N), ("tick",), ("close",), ("tick",)]
    if pattern == "all_closed":
        return [("push", N), ("close",), ("tick",)]
    if pattern == "one_poll_each":
        return [e for _ in range(N) for e in (("push", 1), ("tick",))] + [("close",), ("tick",), ("tick",)]
    out, left = [], N
    while left:
        n = min(left, rs.randint(1, 12))
        out.append(("push", n))
        left -= n
        out += [("tick",)] * rs.choice([0, 1, 1, 2])
    return out + [("close",)] + [("tick",)] * rs.choice([1, 3])


def _drive_plan(c, events):
    ahead = TextAhead(c["A"], c["dec"], c["seam_ms"])
    p = TextPlan(c["bt"], c["R"], c["r_dec"], c["chunk"], c["cap"], c["ff"], ahead=ahead, model_sr=SR,
                 samples_per_frame=SPF)
    log = []
    for e in events:
        if e[0] == "push":
            p.push(e[1])
        elif e[0] == "close":
            p.close()
        else:
            for k, E in p.due_blocks():
                a, b = p.block_tokens_of(k, E)
                p.encoded(k, [c["dur_of"](t, E) for t in range(a, b)])
                log.append(("block", k, E))
            fd = p.flow_due()
            if fd:
                p.flowed(*fd)
                log.append(("flow",) + fd)
            for first, n in p.decodable():
                D = p.t_frames(first, n)
                if c["dec"] is None:
                    # what is flowed: at least the chunk's full context
                    assert D >= (p.total if p.complete else first + n + c["r_dec"])
                    D = None
                log.append(("chunk", first, n, D, p.overhang(first, n)))
                p.released(first, n)
    return p, log


def _drive_ref(c, events):
    over = -(-int(round(c["seam_ms"] * SR / 1000.0)) // SPF) if c["seam_ms"] else 0
    r = RefText(c["bt"], c["A"], c["R"], c["r_dec"], c["dec"], c["chunk"], c["cap"], c["ff"], over, c["dur_of"])
    for e in events:
        if e[0] == "push":
            r.push(e[1])
        elif e[0] == "close":
            r.close()
        else:
            r.tick()
    return r


def _canon(log):
    """What must not depend on the pushes: the blocks, the union and order of the flow ranges, the chunks."""
    flows = [e[1:] for e in log if e[0] == "flow"]
    for (a, b), (a2, b2) in zip(flows, flows[1:]):
        assert b == a2 and a < b
    return ([e for e in log if e[0] == "block"], (flows[0][0], flows[-1][1]) if flows else None,
            [e for e in log if e[0] == "chunk"])


@pytest.mark.parametrize("seed", range(60))
def test_the_plan_is_the_restatement_and_does_not_depend_on_the_pushes(seed):
    rs = random.Random(seed)
    c = _case(rs)
    want = None
    for pattern in ("all", "all_closed", "one_poll_each", "random", "random"):
        events = _events(rs, c["N"], pattern)
        p, log = _drive_plan(c, events)
        ref = _drive_ref(c, events)
        assert log == ref.log, (pattern, c)
        T = sum(p.durations)
        assert p.complete and p.total == T == p.marks[-1] and len(p.durations) == c["N"] == len(p.marks) - 1
        assert p.all_released == (T == sum(e[2] for e in log if e[0] == "chunk")) and p.all_released
        got = _canon(log)
        if want is None:
            want = got
        assert got == want, (pattern, c)
    blocks, flows, chunks = want
    N, bt, A = c["N"], c["bt"], c["A"]
    assert blocks == [("block", k, N if A is None else min((k + 1) * bt + A, N)) for k in range(-(-N // bt))]
    assert flows == ((0, T) if T else None)
    assert [e[1:3] for e in chunks] == schedule(T, c["chunk"], c["cap"]) == stream.chunk_schedule(T, c["chunk"], c["cap"])
    if c["dec"] is not None:
        assert [e[3] for e in chunks] == [min(f + n + c["dec"], T) for f, n in schedule(T, c["chunk"], c["cap"])]
        assert chunks == [] or chunks[-1][3] == T                    # the last chunk is cut at T


def test_rules():
    # A = None: nothing is due before close
    p = TextPlan(4, 32, 11, ahead=TextAhead(tokens=None))
    p.push(50)
    assert p.due_blocks() == [] and p.flow_due() is None and p.decodable() == []
    p.close()
    assert p.due_blocks() == [(k, 50) for k in range(13)]
    # a block is due exactly when E_k tokens have arrived
    p = TextPlan(8, 32, 11, ahead=TextAhead(tokens=4))
    p.push(11)
    assert p.due_blocks() == []
    p.push(1)
    assert p.due_blocks() == [(0, 12)]
    p.push(7)
    assert p.due_blocks() == [(0, 12)]
    p.push(1)
    assert p.due_blocks() == [(0, 12), (1, 20)]
    p.encoded(0, [10] * 8)
    assert p.frames == 80 and p.marks == list(range(0, 81, 10)) and p.due_blocks() == [(1, 20)]
    # b = P - R while open
    assert p.flow_due() == (0, 48)
    p.flowed(0, 48)
    assert p.flow_due() is None and p.z_done == 48
    p.encoded(1, [1] * 8)                                        # P = 88: 8 new frames < flow_frames
    assert p.flow_due() is None
    with pytest.raises(ValueError):
        p.encoded(1, [1] * 8)                                    # in order, once
    with pytest.raises(ValueError):
        p.encoded(2, [1] * 5)                                    # more durations than tokens
    # ... and b = P at the end: the last block is cut at N, the last chunk at T
    p.push(2)
    p.close()
    assert p.due_blocks() == [(2, 22)] and p.block_tokens_of(2, 22) == (16, 22) and not p.complete
    p.encoded(2, [3] * 6)
    assert p.complete and p.total == 106 and p.flow_due() == (48, 106)
    p.flowed(48, 106)
    assert p.decodable() == [(0, 32), (32, 64), (96, 10)]
    assert p.t_frames(96, 10) == 106 and p.overhang(96, 10) == 0
    for c in p.decodable():
        p.released(*c)
    assert p.all_released
    # closing after the last block was encoded completes the text
    p = TextPlan(4, 32, 11, ahead=TextAhead(tokens=0))
    p.push(4)
    p.encoded(0, [20] * 4)
    assert not p.complete and p.flow_due() == (0, 48)
    p.close()
    assert p.complete and p.due_blocks() == [] and p.flow_due() == (0, 80)
    # a bounded dec: canonical t_frames, overhang of a seam
    p = TextPlan(4, 32, 11, chunk_frames=8, max_chunk_frames=8, ahead=TextAhead(0, 4, seam_ms=5.0), model_sr=SR,
                 samples_per_frame=SPF)
    assert p.seam == 110
    p.push(4)
    p.encoded(0, [20] * 4)
    p.flowed(*p.flow_due())
    assert p.decodable() == [(f, 8) for f in range(0, 40, 8)] and p.t_frames(8, 8) == 20 and p.overhang(8, 8) == 1


def test_refusals():
    for bad in (dict(tokens=-1), dict(dec=-1), dict(tokens=1.5), dict(dec=True), dict(seam_ms=-1.0),
                dict(seam_ms=float("nan")), dict(seam_ms=5.0), dict(seam_ms="5")):
        with pytest.raises((TypeError, ValueError)):
            TextAhead(**bad)
    assert repr(TextAhead(4, 2, 5.0)) == "TextAhead(tokens=4, dec=2, seam_ms=5)"
    with pytest.raises(ValueError, match="dec <= 11"):
        TextPlan(8, 32, 11, ahead=TextAhead(dec=12))
    with pytest.raises(TypeError):
        TextPlan(8, 32, 11, ahead=stream.Ahead(0, 4))
    with pytest.raises(ValueError, match="block_tokens"):
        TextPlan(0, 32, 11)
    with pytest.raises(ValueError, match="flow_frames"):
        TextPlan(8, 32, 11, flow_frames=0)
    with pytest.raises(ValueError):
        TextPlan(8, 32, 11, chunk_frames=64, max_chunk_frames=32)
    with pytest.raises(ValueError, match="model_sr"):
        TextPlan(8, 32, 11, ahead=TextAhead(dec=4, seam_ms=5.0))
    p = TextPlan(8, 32, 11)
    with pytest.raises(ValueError, match="empty"):
        p.close()
    assert not p.closed
    p.push(3)
    p.close()
    p.close()
    with pytest.raises(ValueError, match="after close"):
        p.push(1)
    with pytest.raises(ValueError):
        p.flowed(0, 5) or p.flowed(0, 5)                         # ranges are flowed in order, once


def _cfg():
    c = _capi.MbvConfig()
    c.struct_bytes = C.sizeof(_capi.MbvConfig)
    c.inter_channels = c.hidden_channels = 192
    return c


def test_host_entries():
    L, cfg, out = _capi.lib(), _cfg(), (C.c_int32 * 2)()
    assert L.mbv_text_context(C.byref(cfg), C.byref(out)) == 0 and list(out) == [32, 32]
    assert stream.text_context(cfg) == (32, 32)
    assert L.mbv_text_context(None, C.byref(out)) == 1 and L.mbv_text_context(C.byref(cfg), None) == 1
    R = 32
    for first, count, P in ((0, 1, 1), (0, 32, 64), (31, 1, 500), (32, 32, 64), (33, 7, 500), (100, 32, 164),
                            (100, 32, 140), (400, 100, 500), (65, 1, 66)):
        assert L.mbv_flow_window(C.byref(cfg), first, count, P, C.byref(out)) == 0
        wa, wb = out
        assert wa % 32 == 0 and wa <= max(0, first - R) < wa + 32          # a start that is a multiple of 32
        assert wb == min(first + count + R, P)                             # clipped to the expanded frames
    for first, count, P in ((-1, 1, 10), (0, 0, 10), (5, 6, 10), (0, 1, 1 << 31)):
        assert L.mbv_flow_window(C.byref(cfg), first, count, P, C.byref(out)) == 1
    assert L.mbv_flow_window(None, 0, 1, 1, C.byref(out)) == 1 and L.mbv_flow_window(C.byref(cfg), 0, 1, 1, None) == 1
    # the plan: one class, cut at the grid's rows and at the fused WN layers' 32-bit offsets
    run_of = (C.c_int32 * 4)()
    assert L.mbv_flow_ranges_plan(C.byref(cfg), 4, (C.c_int32 * 4)(96, 64, 300, 1), run_of) == 1 and list(run_of) == [0] * 4
    assert L.mbv_flow_ranges_plan(C.byref(cfg), 0, (C.c_int32 * 1)(1), None) == -1
    assert L.mbv_flow_ranges_plan(C.byref(cfg), 1, None, None) == -1
    assert L.mbv_flow_ranges_plan(None, 1, (C.c_int32 * 1)(1), None) == -1
    assert L.mbv_flow_ranges_plan(C.byref(cfg), 2, (C.c_int32 * 2)(5, 0), None) == -1
    big = 1 << 22                                                          # 2 x 192 x 2^22 x 4 bytes = 6 GiB > 4 GiB
    two = (C.c_int32 * 2)()
    assert L.mbv_flow_ranges_plan(C.byref(cfg), 2, (C.c_int32 * 2)(big, big), two) == 2 and list(two) == [0, 1]
    assert L.mbv_flow_ranges_plan(C.byref(cfg), 1, (C.c_int32 * 1)(1 << 23), None) == -1
    # a handle-less counter
    assert L.mbv_text_runs(None) == -1 and L.mbv_flow_runs(None) == -1


# ------------------------------------------------------------------------------------------------ the C structs
def _fields(name):
    hdr = open(os.path.join(ROOT, "include", "mbistft_vits.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    types = {"int64_t": C.c_int64, "int32_t": C.c_int32, "float": C.c_float}
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype = C.c_void_p if "*" in decl else types[decl.split()[0]]
        for part in decl.replace("*", " ").split(","):
            fields.append((part.split()[-1], ctype))
    return fields


def test_struct_layouts_match_the_header():
    for cls, name, size in ((_capi.MbvTakeRow, "mbv_take_row", 56), (_capi.MbvExpandRange, "mbv_expand_range", 88),
                            (_capi.MbvFlowRange, "mbv_flow_range", 56)):
        assert [(n, t) for n, t in cls._fields_] == _fields(name)
        assert C.sizeof(cls) == size
    assert [getattr(_capi.MbvTakeRow, n).offset for n, _ in _capi.MbvTakeRow._fields_] == [0, 4, 8, 12, 16, 24, 32, 40, 48]
    assert [getattr(_capi.MbvExpandRange, n).offset for n, _ in _capi.MbvExpandRange._fields_] == [
        0, 8, 16, 24, 32, 36, 40, 44, 48, 56, 64, 68, 72, 80]
    assert [getattr(_capi.MbvFlowRange, n).offset for n, _ in _capi.MbvFlowRange._fields_] == [
        0, 8, 16, 20, 24, 32, 36, 40, 48]
    for s in ("mbv_text_context", "mbv_flow_window", "mbv_flow_ranges_plan", "mbv_take_tokens_rows",
              "mbv_expand_ranges", "mbv_flow_ranges", "mbv_text_runs", "mbv_flow_runs"):
        assert s in _capi.TABLE and hasattr(_capi.lib(), s)
