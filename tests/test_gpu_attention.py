"""`rel_attention_kernel<1..4>` (csrc/attention.hip) launched by itself through `mbv_op_rel_attention` and held to
the float64 reference and bars of attention_cases.py (which test_attention_refs.py proves on the CPU).  The output is
pre-filled with NaN so that an unwritten element, or a padded query column the kernel leaves non-finite, fails; every
launch runs twice and must give equal bits.

MBV_ATTENTION_REPORT=<file>: the per-case statistics as JSON (profiles/attention_bars.json is such a run)."""
import json
import os

import pytest
import torch

import attention_cases as ac
from test_gpu_small_ops import _nan, _twice

pytestmark = pytest.mark.gpu
STATS = ac.Stats()


@pytest.fixture(scope="module")
def net():
    from gpu_util import make_net
    n = make_net("ljs_mini_mb_istft_vits")[0]
    yield n
    path = os.environ.get("MBV_ATTENTION_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump({"margin": ac.MARGIN, "cases": STATS}, f, indent=1)


@pytest.mark.parametrize("c", ac.ATT_CASES, ids=lambda c: c["name"])
def test_rel_attention(net, c):
    from gpu_util import ptr
    from mb_istft_vits_amd import _capi
    inp = ac.att_shared(c)[0]
    d = {k: v.cuda() for k, v in inp.items()}
    h = net._ensure_handle()

    def run():
        o = _nan(c["B"], c["H"], c["T"])
        rc = _capi.lib().mbv_op_rel_attention(h, ptr(d["qkv"]), ptr(d["emb_k"]), ptr(d["emb_v"]), ptr(d["lens"]), ptr(o),
                                              c["B"], c["H"], c["heads"], c["T"], net._stream())
        _capi.check(h, rc, "mbv_op_rel_attention")
        return {"o": o.cpu()}
    ac.att_check(c, _twice(run)["o"], stats=STATS)


def test_head_dimensions_the_entry_refuses(net):
    """Odd, and above the 128 that rel_attention_kernel<4> covers (the limit mbv_create sets): refused, nothing launched."""
    from gpu_util import ptr
    from mb_istft_vits_amd import _capi
    h = net._ensure_handle()
    x, o = torch.zeros(1, 3 * 130, 8, device="cuda"), _nan(1, 130, 8)
    lens = torch.tensor([8], device="cuda")
    for H, heads in ((130, 1), (66, 2), (128, 3)):
        rc = _capi.lib().mbv_op_rel_attention(h, ptr(x), ptr(x), ptr(x), ptr(lens), ptr(o), 1, H, heads, 8, net._stream())
        assert rc != 0 and b"mbv_op_rel_attention" in _capi.lib().mbv_last_error(h), (H, heads)
    torch.cuda.synchronize()
    assert bool(torch.isnan(o).all())
