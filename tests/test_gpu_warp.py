"""-m gpu: the time-warp kernel of per-token pitch (`mbv_warp_ranges`, `net.warp`, `net.warp_ranges`) on
synthetic rows, no model run: parity with the float64 restatement tests/warp_ref.py under the bar the resampler's tests
use for the same kind of filter on unit-scale input (tests/test_gpu_resample.py: max abs <= 5e-6, RMS <= 1e-6), and the
BITWISE relations: a row does not depend on how it is cut into ranges, on the rows that share its launch, on what lies
behind the decoded frontier, and an envelope equals the pre-multiplied waveform.
Parity proper (a per-element bar from the float64 reference, full-width tiles, long rows) is tests/test_gpu_warp_pin.py."""
import functools

import numpy as np
import pytest
import torch

from mb_istft_vits_amd import _capi, stream, wire

import gain_ref
import warp_ref
from test_gpu_turns import _net as _mini      # (ljs_mini_mb_istft_vits: only its handle is used)

pytestmark = pytest.mark.gpu

HOP, F = 256, 6
N = HOP * F
SENTINEL = -7.5
FILTERS = ["kaiser_best", "kaiser_fast"]


def _glided():
    """two tokens, 4 and 2 frames, a fifth up and a fourth down, with the default glide"""
    return stream.frame_rates([warp_ref.pitch_of_semitones(7), warp_ref.pitch_of_semitones(-5)], [0, 4, 6], F)


TABLES = {
    "ones": np.ones(F, np.float32),
    "up": np.full(F, 1.25, np.float32),
    "down": np.full(F, 0.8, np.float32),
    "alternating": np.asarray([0.5, 2.0] * (F // 2), np.float32),
    "glided": _glided(),
}


@functools.lru_cache(maxsize=None)
def _x():
    return np.random.RandomState(41).uniform(-1, 1, N).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _reference(name, res_type):
    """the float64 restatement of the whole row: computed once, shared, never written to"""
    y = warp_ref.warp(_x().astype(np.float64), TABLES[name], HOP, res_type)
    y.setflags(write=False)
    return y


def _map(name):
    return stream.WarpMap(TABLES[name], HOP, "cuda")


def _ranges(net, jobs):
    """ONE `mbv_warp_ranges` call: jobs = [(x device, map, in_avail, first, count, out, envelope, res_type)]"""
    net.warp_ranges([net.warp_row(*j) for j in jobs])


def _fresh(m):
    return torch.full((1, m.n_out), SENTINEL, device="cuda")


def _same(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


# ------------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize("res_type", FILTERS)
@pytest.mark.parametrize("name", list(TABLES))
def test_parity_with_the_restatement(name, res_type):
    net = _mini()
    m = _map(name)
    ref = _reference(name, res_type)
    assert m.n_out == len(ref) == warp_ref.plan(TABLES[name], HOP)[1]
    y = net.warp(torch.from_numpy(_x()).cuda(), m, res_type=res_type)
    assert y.shape == (1, m.n_out) and y.dtype == torch.float32
    d = y[0].cpu().numpy().astype(np.float64) - ref
    print("warp parity %s %s: n_out %d max abs %.3e rms %.3e" % (name, res_type, m.n_out, np.abs(d).max(),
                                                                  np.sqrt(np.mean(d ** 2))))
    assert np.abs(d).max() <= 5e-6
    assert np.sqrt(np.mean(d ** 2)) <= 1e-6


# ------------------------------------------------------------------------------------------------ range independence
@pytest.mark.parametrize("res_type", FILTERS)
def test_a_row_does_not_depend_on_its_ranges(res_type):
    net = _mini()
    x = torch.from_numpy(_x()).cuda()
    for name in ("alternating", "glided"):
        m = _map(name)
        whole = net.warp(x, m, res_type=res_type)
        out = _fresh(m)
        done = 0
        rest = m.n_out - 769
        for count in (1, 255, 256, 257) + ((rest,) if rest % 2 else (3, rest - 3)):      # .. and an odd remainder
            runs = net.warp_runs()
            _ranges(net, [(x, m, N, done, count, out, None, res_type)])
            assert net.warp_runs() - runs == 1
            done += count
            assert (out[:, done:] == SENTINEL).all()             # nothing past the range is written
        assert done == m.n_out
        assert _same(out, whole)


def test_eight_rows_in_one_launch_are_the_rows_alone():
    net = _mini()
    names = list(TABLES)
    rs = np.random.RandomState(43)
    xs = [torch.from_numpy(rs.uniform(-1, 1, N).astype(np.float32)).cuda() for _ in range(8)]
    maps = [_map(names[i % len(names)]) for i in range(8)]
    kinds = [FILTERS[i % 2] for i in range(8)]
    firsts = [0, 3, 255, 256, 700, 1, 0, 511]
    counts = [m.n_out - a if i % 3 == 0 else (1, 300, 257, 0, 513)[i % 5] for i, (m, a) in enumerate(zip(maps, firsts))]
    alone = [net.warp(x, m, res_type=k) for x, m, k in zip(xs, maps, kinds)]
    outs = [_fresh(m) for m in maps]
    runs = net.warp_runs()
    _ranges(net, [(x, m, N, a, c, o, None, k) for x, m, a, c, o, k in zip(xs, maps, firsts, counts, outs, kinds)])
    assert net.warp_runs() - runs == 1                          # ONE launch for all rows (two filters among them)
    for o, w, a, c in zip(outs, alone, firsts, counts):
        assert _same(o[:, a:a + c], w[:, a:a + c])
        assert (o[:, :a] == SENTINEL).all() and (o[:, a + c:] == SENTINEL).all()


# ------------------------------------------------------------------------------------------------ the frontier
@pytest.mark.parametrize("res_type", FILTERS)
@pytest.mark.parametrize("name", ["alternating", "glided", "down"])
def test_nothing_behind_the_frontier_is_read(name, res_type):
    net = _mini()
    m = _map(name)
    x = torch.from_numpy(_x()).cuda()
    closed = net.warp(x, m, res_type=res_type)
    in_avail = 5 * HOP // 2                                      # 2.5 frames
    ready = m.ready(in_avail, res_type)
    assert 0 < ready < m.n_out and ready == warp_ref.ready(TABLES[name], m.U, HOP, in_avail, res_type)
    out = _fresh(m)
    _ranges(net, [(x, m, in_avail, 0, ready, out, None, res_type)])
    assert _same(out[:, :ready], closed[:, :ready]) and (out[:, ready:] == SENTINEL).all()
    poisoned = x.clone()
    poisoned[in_avail:] = float("nan")
    out2 = _fresh(m)
    _ranges(net, [(poisoned, m, in_avail, 0, ready, out2, None, res_type)])
    assert torch.isfinite(out2[:, :ready]).all() and _same(out2[:, :ready], closed[:, :ready])
    # one output past ready is refused with the row named, nothing is launched, and the handle serves the next call
    out3 = _fresh(m)
    runs = net.warp_runs()
    with pytest.raises(_capi.MbvError, match="row 1"):
        _ranges(net, [(x, m, in_avail, 0, ready, out2, None, res_type), (x, m, in_avail, 0, ready + 1, out3, None, res_type)])
    assert net.warp_runs() == runs and (out3 == SENTINEL).all()
    _ranges(net, [(x, m, in_avail, 0, ready, out3, None, res_type)])
    assert _same(out3[:, :ready], closed[:, :ready])


def test_refusals_name_the_row_and_launch_nothing():
    net = _mini()
    m = _map("glided")
    x = torch.from_numpy(_x()).cuda()
    out = _fresh(m)
    good = net.warp_row(x, m, N, 0, 10, out)
    runs = net.warp_runs()

    def refused(row, what):
        with pytest.raises(_capi.MbvError, match=what):
            net.warp_ranges([good, row])
        assert net.warp_runs() == runs

    def edited(**kw):
        row = net.warp_row(x, m, N, 20, 10, out)
        for k, v in kw.items():
            setattr(row, k, v)
        return row

    with pytest.raises(_capi.MbvError):
        net._call("mbv_warp_ranges", (_capi.MbvWarpRow * 1)(good), 0)        # n < 1
    for field in ("wave", "U", "rate", "U_host", "rate_host", "out"):
        refused(edited(**{field: None}), "row 1")
    refused(edited(res_type=2), "row 1: unknown res_type")
    refused(edited(samples=N - 1), "row 1")
    refused(edited(out_capacity=25), "row 1")                                # the destination's capacity
    refused(edited(out_first=m.n_out, out_count=1), "row 1")
    refused(edited(in_avail=-1), "row 1")
    G = torch.ones(F, device="cuda")                                         # F - 1 frames: does not cover the row
    refused(net.warp_row(x, m, N, 20, 10, out, wire.Envelope(G, HOP)), "row 1: the envelope")
    refused(net.warp_row(x, m, N, 5, 10, out), "rows 0 and 1 write overlapping")
    assert (out == SENTINEL).all()
    net.warp_ranges([good])
    assert net.warp_runs() - runs == 1 and _same(out[:, :10], net.warp(x, m)[:, :10])


# ------------------------------------------------------------------------------------------------ the envelope
@pytest.mark.parametrize("res_type", FILTERS)
def test_an_envelope_is_the_premultiplied_waveform(res_type):
    net = _mini()
    G = np.asarray([1.0, 4.0, 0.0, 1e-3, 2.5, 1.0, 0.5], np.float32)          # F + 1 values; neighbours differ
    shaped = gain_ref.shaped(_x(), G, HOP)                                    # x * e in fp32, as the wire kernels form it
    assert shaped.dtype == np.float32
    env = wire.Envelope(torch.from_numpy(G).cuda(), HOP)
    x = torch.from_numpy(_x()).cuda()
    for name in ("alternating", "glided", "ones"):
        m = _map(name)
        assert _same(net.warp(x, m, envelope=env, res_type=res_type),
                     net.warp(torch.from_numpy(shaped).cuda(), m, res_type=res_type))
    ones = wire.Envelope(torch.ones(F + 1, device="cuda"), HOP)               # e = 1.0f exactly: the unshaped bits
    m = _map("glided")
    assert _same(net.warp(x, m, envelope=ones, res_type=res_type), net.warp(x, m, res_type=res_type))
