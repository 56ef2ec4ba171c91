"""The host entries that describe the decoder (`mbv_tail_plan`, `mbv_decoder_context`, `mbv_ragged_classes`,
`mbv_ragged_plan`, `mbv_chunks_plan`) against answers recorded from an earlier build of the library
(tests/golden/decoder_plan.json, written by tests/golden/make_decoder_plan.py): every integer is reproduced exactly, for
the shipped configs and for variants that move every field of the decoder's description.  Host only, no GPU."""
import json
import os

import pytest

from mb_istft_vits_amd import _capi, utils as mutils

from golden import make_decoder_plan as gen

HERE = os.path.dirname(os.path.abspath(__file__))

with open(os.path.join(HERE, "golden", "decoder_plan.json")) as _f:
    FIXTURE = json.load(_f)
CASES = {c["config"]: c for c in FIXTURE["cases"]}


def test_the_fixture_covers_every_config_and_the_inputs_are_the_recorders():
    assert FIXTURE["t_max"] == gen.T_MAX and FIXTURE["lengths"] == gen.LENGTHS
    assert [[c["config"], c["base"], c["overrides"]] for c in FIXTURE["cases"]] == [list(x) for x in gen.all_configs()]
    lens = set(gen.expand(gen.LENGTHS))
    assert 0 in lens and gen.expand(gen.LENGTHS).count(3) > 65535
    kinds = set()
    for c in FIXTURE["cases"]:
        for f in c["classes"][0][1:]:
            assert f in lens and f - 1 in lens, (c["config"], f)
        assert c["classes"][1] == [1]
        model = mutils.get_hparams_from_file(mutils.builtin_config(c["base"])).model
        kinds.add(((model["istft_vits"], model["mb_istft_vits"], model["ms_istft_vits"]),
                   (c["overrides"] or {}).get("resblock", "1")))
    assert len({k for k, _ in kinds}) == 3                                # each decoder type
    assert {r for _, r in kinds} == {"1", "2"}


@pytest.mark.parametrize("cid", list(CASES))
def test_library_reproduces_the_recorded_answers(cid):
    c = CASES[cid]
    L = gen.declare(_capi.lib())
    got = gen.answers(L, gen.config_struct(c["base"], c["overrides"]))
    for key in got:
        assert got[key] == c[key], (cid, key)
