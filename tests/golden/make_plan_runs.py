"""Record what the three greedy run planners answer (plan_runs.json) from a BUILT library of the commit to pin:

    python tests/golden/make_plan_runs.py /path/to/libmbistft_vits.so

`mbv_admit_plan`, `mbv_convert_plan` (both split-K settings) and `mbv_convert_ranges_plan` for every shipped config:
lengths straddling 256 in mixed order, a class reopened after it was closed, 65 537 requests of 5 (the grid cut), a
batch that the fused WN layers' 32-bit offsets cut, and the refused inputs (0, negative, a lone request beyond the
fused layers).  Only inputs and `run_of_*` arrays are stored, long ones as [value, count] pairs; a refused input
(-1) has `run_of` null.  tests/test_plan_runs_golden.py holds the library of the tree to these answers.
"""
import ctypes as C
import glob
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True

from mb_istft_vits_amd import _capi, models, utils as mutils   # noqa: E402  (config structs only: the library is the given one)


def configs():
    return sorted(os.path.splitext(os.path.basename(p))[0]
                  for p in glob.glob(os.path.join(os.path.dirname(mutils.builtin_config("ljs_mb_istft_vits")), "*.json")))


def config_struct(name):
    hps = mutils.get_hparams_from_file(mutils.builtin_config(name))
    net = models.SynthesizerTrn(59, hps.data.filter_length // 2 + 1, hps.train.segment_size // hps.data.hop_length,
                                n_speakers=hps.data.n_speakers, **hps.model)
    return net._config_struct()


def pairs(values):
    out = []
    for v in values:
        if out and out[-1][0] == v:
            out[-1][1] += 1
        else:
            out.append([int(v), 1])
    return out


def expand(pp):
    return [v for v, n in pp for _ in range(n)]


def inputs(cfg):
    ch = max(cfg.hidden_channels, cfg.inter_channels)
    T = 1 << 20
    B = -(-(1 << 32) // (4 * ch * T))                  # the first batch of T frames that reaches 4 GiB
    return {
        "straddle_256": [[255, 1], [256, 1], [257, 1], [1, 1], [600, 1]],
        "class_reopened": [[5, 65535], [300, 1], [5, 2], [300, 1], [255, 1], [257, 1]],
        "grid_cut": [[5, 65537]],
        "fused_offsets_cut": [[T, B], [7, 1], [T, 1]],
        "refused_zero": [[5, 1], [0, 1], [7, 1]],
        "refused_negative": [[-3, 1]],
        "refused_lone_beyond_fused": [[-(-(1 << 32) // (4 * ch)), 1]],
    }


def ask(L, planner, cfg, splitk, pp):
    t = expand(pp)
    n = len(t)
    arr, run_of = (C.c_int32 * n)(*t), (C.c_int32 * n)()
    if planner == "mbv_convert_ranges_plan":
        r = L.mbv_convert_ranges_plan(C.byref(cfg), n, arr, run_of)
    else:
        r = getattr(L, planner)(C.byref(cfg), splitk, n, arr, run_of)
    return r, list(run_of)


def declare(L):
    i32, p32 = C.c_int32, C.POINTER(C.c_int32)
    for name in ("mbv_admit_plan", "mbv_convert_plan"):
        getattr(L, name).argtypes = [C.POINTER(_capi.MbvConfig), i32, i32, p32, p32]
        getattr(L, name).restype = i32
    L.mbv_convert_ranges_plan.argtypes = [C.POINTER(_capi.MbvConfig), i32, p32, p32]
    L.mbv_convert_ranges_plan.restype = i32
    return L


PLANNERS = [("mbv_admit_plan", 0), ("mbv_admit_plan", 1), ("mbv_convert_plan", 0), ("mbv_convert_plan", 1),
            ("mbv_convert_ranges_plan", 0)]


def main():
    L = declare(C.CDLL(os.path.abspath(sys.argv[1])))
    cases = []
    for name in configs():
        cfg = config_struct(name)
        for planner, splitk in PLANNERS:
            for case, pp in inputs(cfg).items():
                r, run_of = ask(L, planner, cfg, splitk, pp)
                assert r == -1 or r == max(run_of) + 1, (name, planner, case, r)
                cases.append({"config": name, "planner": planner, "splitk": splitk, "case": case, "input": pp,
                              "run_of": None if r < 0 else pairs(run_of)})
    with open(os.path.join(HERE, "plan_runs.json"), "w") as f:
        f.write("{\"cases\": [\n" + ",\n".join(json.dumps(c) for c in cases) + "\n]}\n")
    print("wrote", len(cases), "cases")


if __name__ == "__main__":
    main()
