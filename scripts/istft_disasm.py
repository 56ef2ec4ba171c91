"""Instruction-stream fingerprints of the waveform-tail kernels (istft_pqmf.hip).

Compiles one istft_pqmf.hip for gfx950 (device code only, no GPU needed), cuts the assembly into kernels and
hashes each kernel's instructions with the basic-block labels renumbered.  Kernels are keyed by their template
arguments (the trailing RANGED flag, when present and set, as a "+ranged" suffix):

    istft_pqmf_kernel<TM, NT, FIXED, FAST, PRE, POLAR[, RANGED]>  ->  "pqmf/TM/NT/FIXED,FAST,PRE,POLAR[+ranged]"
    istft_single_kernel<FAST, PRE, POLAR[, RANGED]>                ->  "single/FAST,PRE,POLAR[+ranged]"

tests/test_stream_plan.py compares the one-shot kernels against fingerprints recorded before the streaming
decode's ranged mode was added (tests/golden/istft_disasm_fingerprints.json).

    python scripts/istft_disasm.py [path/to/istft_pqmf.hip] > fingerprints.json
"""
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT_SRC = os.path.join(ROOT, "mb-istft-vits_amd", "csrc", "istft_pqmf.hip")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

_PQMF = re.compile(r"^_ZN3mbv17istft_pqmf_kernelILi(\d+)ELi(\d+)E((?:Lb[01]E)+)EEvNS_9IstftArgsE")
_SINGLE = re.compile(r"^_ZN3mbv19istft_single_kernelI((?:Lb[01]E)+)EEvNS_11IstftSbArgsE")


def kernel_key(sym):
    m = _PQMF.match(sym)
    if m:
        flags = re.findall(r"Lb([01])E", m.group(3))
        return "pqmf/%s/%s/%s" % (m.group(1), m.group(2), ",".join(flags[:4])) + ("+ranged" if flags[4:] == ["1"] else "")
    m = _SINGLE.match(sym)
    if m:
        flags = re.findall(r"Lb([01])E", m.group(1))
        return "single/%s" % ",".join(flags[:3]) + ("+ranged" if flags[3:] == ["1"] else "")
    return None


def fingerprints(asm_text):
    out = {}
    cur, body = None, []
    for line in asm_text.splitlines():
        if cur is None:
            m = re.match(r"^(_Z\w+):", line)
            if m and kernel_key(m.group(1)):
                cur, body = kernel_key(m.group(1)), []
            continue
        if line.startswith(".Lfunc_end"):
            out[cur] = hashlib.sha256("\n".join(body).encode()).hexdigest()
            cur = None
            continue
        s = line.split(";")[0].rstrip()
        if not s.strip():
            continue
        s = re.sub(r"\.LBB\d+_", ".LBB_", s)
        if s.startswith(".LBB_") or re.match(r"^\s+[a-z_][a-z0-9_]*", s) and not s.strip().startswith("."):
            body.append(s.strip())
    return out


def compile_fingerprints(src=DEFAULT_SRC):
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "istft.s")
        inc = os.path.dirname(os.path.abspath(src))
        subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "--offload-device-only", "-S",
                        "-I", inc, src, "-o", out], check=True, capture_output=True, text=True)
        with open(out) as f:
            return fingerprints(f.read())


if __name__ == "__main__":
    fp = compile_fingerprints(sys.argv[1] if len(sys.argv) > 1 else DEFAULT_SRC)
    json.dump(dict(sorted(fp.items())), sys.stdout, indent=1)
    print()
