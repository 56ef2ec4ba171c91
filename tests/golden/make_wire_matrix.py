"""Record the byte matrix of the wire kernels (wire_matrix.json) on an MI355X, from the library BUILT from the commit to
pin (the in-tree one, or the one MBV_LIB names):

    python tests/golden/make_wire_matrix.py <hash of that commit> [output file, default wire_matrix.json beside this script]

One SHA-256 per case of tests/wire_matrix_cases.py over what `tests/test_gpu_wire_matrix.py::digest_of` collects: the
samples, the packed buffers, `out_samples` and the running-peak bits.  Only digests and the commit's hash are stored;
the test reads the digests, a reviewer the hash.  Recorded once, in front of a change that must leave the bytes where
they are, and not again after it.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.dirname(HERE)]
sys.dont_write_bytecode = True

import wire_matrix_cases as M                      # noqa: E402
from test_gpu_wire_matrix import digest_of         # noqa: E402


def main():
    commit = sys.argv[1]
    assert len(commit) == 40 and int(commit, 16) >= 0, "the full hash of the recorded commit"
    digests = {case["id"]: digest_of(case) for case in M.cases()}
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(HERE, "wire_matrix.json")
    with open(out, "w") as f:
        f.write("{\"commit\": \"%s\",\n \"digests\": {\n" % commit
                + ",\n".join("  %s: %s" % (json.dumps(k), json.dumps(v)) for k, v in digests.items()) + "\n}}\n")
    print("wrote", len(digests), "digests of", commit)


if __name__ == "__main__":
    main()
