"""-m gpu: the time-warp kernel (csrc/warp.hip, `warp_ranges_kernel`) pinned to float64 at the cases of
tests/warp_cases.py: tiles whose staged window is as wide as kWarpWindow was sized for (a sustained rate of 2.0), rows
of 1.15 M and 20 M outputs where tau needs its float64 and (float)t is no longer exact, a hop of one sample, integer
and fractional U[f], impulses, the open frontier and an envelope.

  a. `net.warp`: every whole-row case and both filters through the element and quantile bars; impulses under the
     element bar (A = |w|) and +0.0 bitwise where no wing holds them; the envelope against the reference of the
     fp32-shaped row;
  b. `net.warp_ranges` at the open frontier: [0, ready) from a row that is NaN behind in_avail, against
     `warp_ref.warp(.., in_avail=)`; the sentinel behind ready;
  c. `net.warp_ranges` far from t = 0: the last three tiles of the 1.15 M-output row; three tiles behind 2^24 and the
     last two tiles of the 20 M-output row, both ranges in ONE launch; the sentinel everywhere else.

tests/test_gpu_warp.py holds the bitwise relations and the refusals; they are not repeated here.

MBV_WARP_REPORT=<file>: the worst err / (u A) and the largest share of the quantile bars per entry (`warp`,
`warp_ranges`, `warp_ranges_long`), as JSON (profiles/warp_bars.json is such a run)."""
import json
import os

import numpy as np
import pytest
import torch

import warp_cases as wc
from test_gpu_turns import _net as _mini      # (ljs_mini_mb_istft_vits: only its handle is used)

pytestmark = pytest.mark.gpu
STATS = {k: wc.Stats() for k in wc.ENTRIES}
SENTINEL = -7.5
IDS = dict(ids=lambda v: v["name"] if isinstance(v, dict) else v)


@pytest.fixture(scope="module")
def net():
    yield _mini()
    rows = {k: dict(v, headroom=v["TOL"] / v["err_over_uA"] if v["err_over_uA"] else None)
            for k, s in STATS.items() for v in s.values()}
    print("\nworst err / (u A) per kernel entry: " + ", ".join("%s %.3g (TOL %g)" % (k, v["err_over_uA"], v["TOL"])
                                                                for k, v in rows.items()))
    path = os.environ.get("MBV_WARP_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump({"entries": rows}, f, indent=1)


def _map(c):
    from mb_istft_vits_amd import stream
    m = stream.WarpMap(c["R"].copy(), c["hop"], "cuda")
    assert m.n_out == wc.plan(c["name"])[1] and np.array_equal(m.U, wc.plan(c["name"])[0])
    return m


def _ranged(net, c, res_type, variant, x, m, in_avail, ranges):
    """ONE `mbv_warp_ranges` call with a row per range, all into one sentinel-filled destination -> the bars on every
    range, the sentinel everywhere else, one launch."""
    out = torch.full((1, m.n_out), SENTINEL, device="cuda")
    runs = net.warp_runs()
    net.warp_ranges([net.warp_row(x, m, in_avail, a, b - a, out, None, res_type) for a, b in ranges])
    assert net.warp_runs() - runs == 1
    edge = 0
    for k, (a, b) in enumerate(ranges):
        assert bool((out[0, edge:a] == SENTINEL).all()), (c["name"], "written in front of the range", a)
        wc.check(c, res_type, variant, k, out[0, a:b].cpu().numpy(), stats=STATS[wc.entry_of(c, variant)])
        edge = b
    assert bool((out[0, edge:] == SENTINEL).all()), (c["name"], "written behind the range", edge)


# ------------------------------------------------------------------------------------------------ a, b. whole rows
@pytest.mark.parametrize("res_type", wc.FILTERS)
@pytest.mark.parametrize("c", wc.WHOLE, **IDS)
def test_whole_rows_inside_the_bars(net, c, res_type):
    from mb_istft_vits_amd import wire
    m = _map(c)
    for vn, x, in_avail, _ in wc.variants(c):
        ranges = wc.variant_ranges(c, in_avail, res_type)
        if vn == "frontier":
            assert ranges == [(0, m.ready(in_avail, res_type))]
            xd = torch.from_numpy(x.copy()).cuda()
            xd[in_avail:] = float("nan")                         # what has not been decoded yet is never read
            _ranged(net, c, res_type, vn, xd, m, in_avail, ranges)
            continue
        if vn == "envelope":                                     # the kernel shapes the PLAIN row where it reads it
            env = wire.Envelope(torch.tensor(wc.ENVELOPE_GAINS, device="cuda"), c["hop"])
            y = net.warp(torch.from_numpy(wc.case_x(c["name"]).copy()).cuda(), m, envelope=env, res_type=res_type)
        else:
            y = net.warp(torch.from_numpy(x.copy()).cuda(), m, res_type=res_type)
        assert y.shape == (1, m.n_out) and y.dtype == torch.float32 and ranges == [(0, m.n_out)]
        wc.check(c, res_type, vn, 0, y[0].cpu().numpy(), stats=STATS[wc.entry_of(c, vn)])


# ------------------------------------------------------------------------------------------------ c. far from t = 0
@pytest.mark.parametrize("res_type", wc.FILTERS)
@pytest.mark.parametrize("c", wc.RANGED, **IDS)
def test_ranges_far_from_zero_inside_the_bars(net, c, res_type):
    """tau = f hop + (t - U[f]) R[f] at t > 10^6 and t > 2^24: in fp32 it would be off by 0.1 sample and more."""
    m = _map(c)
    ranges = wc.case_ranges(c)
    assert ranges[0][0] >= 10 ** 6 and all(a % wc.TILE == 0 for a, _ in ranges) and ranges[-1][1] == m.n_out
    x = torch.from_numpy(wc.case_x(c["name"]).copy()).cuda()
    try:
        _ranged(net, c, res_type, "noise", x, m, m.samples, ranges)
    finally:
        del x, m
        if res_type == wc.FILTERS[-1]:                           # the 70 MB row and its 80 MB of output: let go
            wc.forget(c["name"])
            torch.cuda.empty_cache()
