"""The three greedy run planners (`mbv_admit_plan`, `mbv_convert_plan`, `mbv_convert_ranges_plan`) against answers
recorded from an earlier build of the library (tests/golden/plan_runs.json, written by tests/golden/make_plan_runs.py):
every `run_of_*` array is reproduced exactly, and what was refused is refused.  Host only, no GPU."""
import json
import os

import pytest

from mb_istft_vits_amd import _capi

from golden import make_plan_runs as gen

HERE = os.path.dirname(os.path.abspath(__file__))

with open(os.path.join(HERE, "golden", "plan_runs.json")) as _f:
    CASES = json.load(_f)["cases"]


def test_the_fixture_covers_every_config_planner_and_case():
    want = {(name, planner, splitk, case) for name in gen.configs() for planner, splitk in gen.PLANNERS
            for case in gen.inputs(gen.config_struct(name))}
    assert {(c["config"], c["planner"], c["splitk"], c["case"]) for c in CASES} == want
    for c in CASES:
        assert c["input"] == gen.inputs(gen.config_struct(c["config"]))[c["case"]], c["case"]
        # (pooled admission has no fused-WN rule of its own: a lone long text is one run there)
        refused = c["case"].startswith("refused") and not (
            c["planner"] == "mbv_admit_plan" and c["case"] == "refused_lone_beyond_fused")
        assert (c["run_of"] is None) == refused, (c["config"], c["planner"], c["case"])


@pytest.mark.parametrize("planner, splitk", gen.PLANNERS)
@pytest.mark.parametrize("name", gen.configs())
def test_planner_reproduces_the_recorded_runs(name, planner, splitk):
    L = gen.declare(_capi.lib())
    cfg = gen.config_struct(name)
    mine = [c for c in CASES if (c["config"], c["planner"], c["splitk"]) == (name, planner, splitk)]
    assert mine
    for c in mine:
        r, run_of = gen.ask(L, planner, cfg, splitk, c["input"])
        if c["run_of"] is None:
            assert r == -1, (c["case"], r)
        else:
            want = gen.expand(c["run_of"])
            assert r == max(want) + 1, (c["case"], r)
            assert run_of == want, c["case"]
