"""The byte matrix of the wire kernels (tests/test_gpu_wire_matrix.py, tests/golden/make_wire_matrix.py): one case per
combination of entry, rate pair, limiter, codec, fade and envelope, the smallest shapes at which these kernels can
still go wrong, and for every case the kernel instantiations it launches.  CPU only: NumPy inputs from a fixed seed,
no tensor, no library.

An instantiation is a tuple
    ("range", FIR, LIM, LAW, FADE, ENV)      the ranged kernel
    ("pool",  FIR, LIM, LAW, TURN, ENV)      the pooled kernel (FADE always on)
with LAW 0 = int16, 1 = mu-law, 2 = A-law: 48 of each, the 96 wire kernels of resample.hip.
"""
import itertools

import numpy as np

PAIRS = [(22050, 24000), (22050, 8000), (22050, 22050)]   # FIR with the extra bank row; the long filter; FIR = false
LAWS = ["pcm16", "ulaw", "alaw"]
N_IN, VALID = 1500, 1400               # valid < n: the zero tail [n_out, out_end) and floor / ceil of out_samples
FIRST_AVAIL = 900                      # frontier of the first call; the second has the whole row
PEAK = 0.8
LIMIT = (0.5, 32, 64)                  # ceiling below the signal; a halo of 32 + 64 outputs across tile edges
FADE_BACK, FADE_COUNT = 40, 100        # the fade starts 40 outputs in front of the first call's end: it straddles both
HOP, FRAMES = 256, 6                   # 1536 samples: covers the row and every segment
SEG_LENGTHS, SEG_PAUSES, RAMP = [500, 400, 450], [60, 90], 8          # a timeline of N_IN samples
SEG_ENVELOPES = (0, 2)                 # segments that carry an envelope in an ENV case
SEED = 20250


def inputs():
    """-> dict of fp32 arrays: x [3, N_IN] in (-0.9, 0.9), gains [3, FRAMES + 1] in [0.25, 1.5], and segs, one row per
    segment of the turn (5 samples longer than its valid length)"""
    rng = np.random.default_rng(SEED)
    x = rng.uniform(-0.9, 0.9, size=(3, N_IN)).astype(np.float32)
    gains = rng.uniform(0.25, 1.5, size=(3, FRAMES + 1)).astype(np.float32)
    segs = [rng.uniform(-0.9, 0.9, size=n + 5).astype(np.float32) for n in SEG_LENGTHS]
    return {"x": x, "gains": gains, "segs": segs}


def seg_starts():
    starts, at = [], 0
    for s, n in enumerate(SEG_LENGTHS):
        at += SEG_PAUSES[s - 1] if s else 0
        starts.append(at)
        at += n
    assert at == N_IN
    return starts


def _law(law):
    return LAWS.index(law)


def cases():
    """-> list of dicts: id, entry ("range" | "chunks" | "turns" | "mixed"), orig, target, lim, law, fade, env and
    kernels, the set of instantiations the case launches.
      range   B = 2 rows, one fade and one envelope table for both
      chunks  three rows per call: one with the fade (and, under env, the envelope), one with neither, one with an empty
              range that only writes out_samples; all limited or none
      turns   the same three rows, each the timeline of the three segments
      mixed   a chunks call of four rows, limited and unlimited interleaved, rows 0 and 1 shaped: two launches"""
    out = []
    for (orig, target), lim, law, fade, env in itertools.product(PAIRS, (False, True), LAWS, (False, True), (False, True)):
        fir = orig != target
        out.append({"id": "range-%d-%d-%s-%s%s%s" % (orig, target, law, "lim" if lim else "plain", "-fade" if fade else "",
                                                      "-env" if env else ""),
                    "entry": "range", "orig": orig, "target": target, "lim": lim, "law": law, "fade": fade, "env": env,
                    "kernels": {("range", fir, lim, _law(law), fade, env)}})
    for entry in ("chunks", "turns"):
        for (orig, target), lim, law, env in itertools.product(PAIRS, (False, True), LAWS, (False, True)):
            out.append({"id": "%s-%d-%d-%s-%s%s" % (entry, orig, target, law, "lim" if lim else "plain", "-env" if env else ""),
                        "entry": entry, "orig": orig, "target": target, "lim": lim, "law": law, "fade": True, "env": env,
                        "kernels": {("pool", orig != target, lim, _law(law), entry == "turns", env)}})
    for law in LAWS:
        orig, target = PAIRS[0]
        out.append({"id": "mixed-%d-%d-%s" % (orig, target, law), "entry": "mixed", "orig": orig, "target": target,
                    "lim": None, "law": law, "fade": True, "env": True,
                    "kernels": {("pool", True, False, _law(law), False, True), ("pool", True, True, _law(law), False, True)}})
    return out


def lookaheads(case):
    """the limiter lookaheads of the case's rows (0: unlimited)"""
    return {None: (0, LIMIT[1]), False: (0,), True: (LIMIT[1],)}[case["lim"]]
