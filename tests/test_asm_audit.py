"""The compiled kernels must not contain SERIALISED vector-memory loads again: a load that is followed by
`s_waitcnt vmcnt(0)` with no other load in between is one exposed memory round trip, and dozens in a row (what hipcc makes of
`cond ? p[i] : 0` / `if (cond) v += p[i]` in an unrolled loop) were 9 % of the text encoder and 6 % of a single utterance's
latency until r03.  scripts/asm_serial_loads.py counts them per kernel from a device-only compile; this test pins the counts
of the three sources it was found in.  (No GPU needed: hipcc cross-compiles gfx950 here.  conv1d.hip is left out: its
compile alone takes minutes and its remaining counts are the documented per-element edge paths.)"""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "scripts", "asm_serial_loads.py")
CSRC = os.path.join(ROOT, "mb-istft-vits_amd", "csrc")

# source -> (kernel-name regex, most serialised loads any matching kernel may contain)
BUDGET = {
    "attention.hip": ("rel_attention_kernel", 6),          # r03w: 48 + 48 x 9
    "wn_fused.hip": ("wn_layer_kernel", 4),                # r03w: 35 (NRT = 2) / 60 (NRT = 3)
    "conv1d_narrow.hip": ("conv1d_narrow_kernel", 8),      # r03w: 16-32 NRT (start values) + 24 NRT (LayerNorm) + 2 NXI (staging)
}


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
@pytest.mark.parametrize("src", sorted(BUDGET))
def test_no_serialised_loads(src, tmp_path):
    pat, budget = BUDGET[src]
    r = subprocess.run([sys.executable, TOOL, os.path.join(CSRC, src), pat], capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, MBV_ASM_DIR=str(tmp_path)))
    assert r.returncode == 0, r.stderr[-2000:]
    rows = re.findall(r"^(\S+)\s+loads\s+(\d+)\s+single load -> vmcnt\(0\):\s+(\d+)", r.stdout, re.M)
    assert rows, "the audit printed no kernel for %s:\n%s" % (src, r.stdout[-2000:])
    worst = max(rows, key=lambda x: int(x[2]))
    assert int(worst[2]) <= budget, "%s: %s serialised loads in %s (budget %d)" % (src, worst[2], worst[0], budget)
