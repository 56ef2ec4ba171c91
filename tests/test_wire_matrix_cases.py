"""The case list of the wire byte matrix (tests/wire_matrix_cases.py) against its conditions, without a GPU: it covers
exactly the 96 wire-kernel instantiations, the golden file holds exactly its cases, and no first call ends on a tile
edge."""
import itertools
import json
import os

from mb_istft_vits_amd import wire

import wire_matrix_cases as M


def test_the_cases_launch_exactly_the_96_instantiations():
    flags = (False, True)
    want = {("range", fir, lim, law, fade, env) for fir, lim, law, fade, env in itertools.product(flags, flags, range(3), flags, flags)}
    want |= {("pool", fir, lim, law, turn, env) for fir, lim, law, turn, env in itertools.product(flags, flags, range(3), flags, flags)}
    assert len(want) == 96
    got = set()
    for case in M.cases():
        assert case["kernels"]
        got |= case["kernels"]
    assert got == want
    ids = [case["id"] for case in M.cases()]
    assert len(ids) == len(set(ids)) == 72 + 36 + 36 + 3


def test_the_golden_file_holds_exactly_the_cases(golden_dir):
    with open(os.path.join(golden_dir, "wire_matrix.json")) as f:
        golden = json.load(f)
    assert len(golden["commit"]) == 40
    assert set(golden["digests"]) == {case["id"] for case in M.cases()}
    assert all(len(d) == 64 and int(d, 16) >= 0 for d in golden["digests"].values())


def test_no_first_call_ends_on_a_tile_edge():
    seen = set()
    for case in M.cases():
        for la in M.lookaheads(case):
            key = (case["orig"], case["target"], la)
            if key in seen:
                continue
            seen.add(key)
            r1 = wire.limiter_ready(case["orig"], case["target"], M.FIRST_AVAIL, M.N_IN, la)
            total = wire.resample_ready(case["orig"], case["target"], M.N_IN, M.N_IN)
            assert r1 % 256 != 0 and M.FADE_BACK < r1 < total, key
            assert r1 - M.FADE_BACK + M.FADE_COUNT > r1                  # the ramp straddles the two calls
    assert seen == {(o, t, la) for o, t in M.PAIRS for la in (0, M.LIMIT[1])}
