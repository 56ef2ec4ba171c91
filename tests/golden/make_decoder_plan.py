"""Record what the host entries that describe the decoder answer (decoder_plan.json) from a BUILT library of the
commit to pin:

    python tests/golden/make_decoder_plan.py /path/to/libmbistft_vits.so

For every shipped config, the ResBlock2 override of the plan tests and four variants inside what `mbv_create` accepts
(other kernel sizes, unequal dilations, other `upsample_initial_channel` / `inter_channels`, each decoder type, both
ResBlock types): the whole of `mbv_tail_plan`, `mbv_decoder_context`, `mbv_ragged_classes` up to 1200 frames with
split-K off and on, and `mbv_ragged_plan` / `mbv_chunks_plan` on one mixed list of lengths that straddles every class
cut, holds zeros (which `mbv_chunks_plan` refuses: it is also asked without them) and is cut once by the grid's 65535
rows.  Only inputs and integer answers are stored, long arrays as [value, count] pairs.
tests/test_decoder_plan_golden.py holds the library of the tree to these answers.
"""
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, HERE]
sys.dont_write_bytecode = True

from mb_istft_vits_amd import _capi, models, utils as mutils   # noqa: E402  (config structs only: the library is the given one)

from make_plan_runs import configs as shipped, pairs, expand   # noqa: E402

T_MAX = 1200
RB2 = {"resblock": "2", "resblock_dilation_sizes": [[1, 3], [1, 3], [1, 3]]}
VARIANTS = [
    ("ljs_mini_mb_istft_vits", "rb2", RB2),
    ("ljs_mini_mb_istft_vits", "k579", {"resblock_kernel_sizes": [5, 7, 9], "upsample_initial_channel": 384,
                                        "resblock_dilation_sizes": [[1, 2, 4], [1, 3, 9], [2, 5, 7]],
                                        "inter_channels": 128}),
    ("ljs_mini_istft_vits", "k3511", {"resblock_kernel_sizes": [3, 5, 11], "upsample_initial_channel": 128,
                                      "resblock_dilation_sizes": [[1, 2, 7], [3, 1, 5], [1, 7, 2]],
                                      "inter_channels": 64}),
    ("uudb_ms_istft_vits_ms", "k795_rb2", {"resblock": "2", "resblock_kernel_sizes": [7, 9, 5],
                                           "upsample_initial_channel": 640,
                                           "resblock_dilation_sizes": [[1, 6], [2, 9], [3, 1]],
                                           "inter_channels": 256}),
    ("ljs_ms_istft_vits", "k935", {"resblock_kernel_sizes": [9, 3, 5], "upsample_initial_channel": 1024,
                                   "resblock_dilation_sizes": [[9, 1, 2], [5, 36, 1], [18, 4, 3]],
                                   "inter_channels": 320}),
]
# zeros, both sides of every class cut of every config below (main() checks it), and 65537 rows of one class
LENGTHS = [[300, 1], [0, 1], [16, 1], [17, 1], [64, 1], [65, 1], [256, 1], [257, 1], [4, 1], [5, 1], [32, 1], [33, 1],
           [9, 1], [0, 1], [41, 1], [1200, 1], [1, 1], [3, 65537], [600, 1], [8, 1], [128, 1], [129, 1], [3, 1]]
LENGTHS_NO_ZERO = [p for p in LENGTHS if p[0] > 0]


def all_configs():
    """(id, shipped name, overrides of its model block)"""
    return [(n, n, None) for n in shipped()] + [(n + "_" + tag, n, ov) for n, tag, ov in VARIANTS]


def config_struct(name, overrides=None):
    hps = mutils.get_hparams_from_file(mutils.builtin_config(name))
    for k, v in (overrides or {}).items():
        hps.model[k] = v
    net = models.SynthesizerTrn(59, hps.data.filter_length // 2 + 1, hps.train.segment_size // hps.data.hop_length,
                                n_speakers=hps.data.n_speakers, **hps.model)
    return net._config_struct()


def declare(L):
    i32, p32, cfgp = C.c_int32, C.POINTER(C.c_int32), C.POINTER(_capi.MbvConfig)
    L.mbv_tail_plan.argtypes = [cfgp, p32, i32]
    L.mbv_decoder_context.argtypes = [cfgp, C.POINTER(C.c_int32 * 2)]
    L.mbv_ragged_classes.argtypes = [cfgp, i32, i32, p32, i32]
    L.mbv_ragged_plan.argtypes = [cfgp, i32, i32, i32, C.POINTER(C.c_int64), p32]
    L.mbv_chunks_plan.argtypes = [cfgp, i32, i32, p32, p32]
    for name in ("mbv_tail_plan", "mbv_decoder_context", "mbv_ragged_classes", "mbv_ragged_plan", "mbv_chunks_plan"):
        getattr(L, name).restype = i32
    return L


def tail_plan(L, cfg):
    buf = (C.c_int32 * (6 * 64))()
    n = L.mbv_tail_plan(C.byref(cfg), buf, 64)
    assert 0 < n <= 64, n
    return [list(buf[6 * i:6 * i + 6]) for i in range(n)]


def context(L, cfg):
    out = (C.c_int32 * 2)()
    assert L.mbv_decoder_context(C.byref(cfg), C.byref(out)) == 0
    return list(out)


def classes(L, cfg, splitk):
    n = L.mbv_ragged_classes(C.byref(cfg), splitk, T_MAX, None, 0)
    assert n >= 1, n
    buf = (C.c_int32 * n)()
    assert L.mbv_ragged_classes(C.byref(cfg), splitk, T_MAX, buf, n) == n
    return list(buf)


def ragged_plan(L, cfg, splitk, pp):
    t = expand(pp)
    rows = (C.c_int32 * len(t))()
    n = L.mbv_ragged_plan(C.byref(cfg), splitk, len(t), T_MAX, (C.c_int64 * len(t))(*t), rows)
    return {"runs": n, "run_of": None if n < 0 else pairs(rows)}


def chunks_plan(L, cfg, splitk, pp):
    t = expand(pp)
    rows = (C.c_int32 * len(t))()
    n = L.mbv_chunks_plan(C.byref(cfg), splitk, len(t), (C.c_int32 * len(t))(*t), rows)
    return {"runs": n, "run_of": None if n < 0 else pairs(rows)}


def answers(L, cfg):
    return {
        "tail_plan": tail_plan(L, cfg),
        "context": context(L, cfg),
        "classes": [classes(L, cfg, k) for k in (0, 1)],
        "ragged_plan": [ragged_plan(L, cfg, k, LENGTHS) for k in (0, 1)],
        "chunks_plan_with_zeros": [chunks_plan(L, cfg, k, LENGTHS) for k in (0, 1)],
        "chunks_plan": [chunks_plan(L, cfg, k, LENGTHS_NO_ZERO) for k in (0, 1)],
    }


def main():
    L = declare(C.CDLL(os.path.abspath(sys.argv[1])))
    have = set(expand(LENGTHS))
    cases = []
    for cid, name, ov in all_configs():
        a = answers(L, config_struct(name, ov))
        for f in a["classes"][0][1:]:
            assert f in have and f - 1 in have, (cid, "LENGTHS does not straddle the class cut at", f)
        assert a["chunks_plan_with_zeros"][0]["runs"] == -1 and a["chunks_plan"][0]["runs"] > len(a["classes"][0])
        cases.append(dict({"config": cid, "base": name, "overrides": ov}, **a))
    with open(os.path.join(HERE, "decoder_plan.json"), "w") as f:
        f.write("{\"t_max\": %d, \"lengths\": %s, \"cases\": [\n" % (T_MAX, json.dumps(LENGTHS)) +
                ",\n".join(json.dumps(c) for c in cases) + "\n]}\n")
    print("wrote", len(cases), "configs")


if __name__ == "__main__":
    main()
