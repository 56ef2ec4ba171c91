"""The live wire's C entries (no GPU): declared in the header, exported by the library, bound with the header's struct
layout; the host-only readiness function refuses what `mbv_resample` refuses, with a message."""
import ctypes as C
import os
import re

from mb_istft_vits_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mbv_resample_ready_open", "mbv_resample_ranges", "mbv_input_runs"]


def _header():
    return open(os.path.join(ROOT, "include", "mbistft_vits.h")).read()


def test_the_new_symbols_are_declared_and_exported():
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)                # declarations, not the text about them
    L = _capi.lib()
    for sym in NEW:
        assert re.search(r"\b%s\s*\(" % sym, code), sym
        assert sym in _capi.SYMBOLS and getattr(L, sym) is not None
    assert L.mbv_resample_ready_open.restype is C.c_int64 and L.mbv_input_runs.restype is C.c_int64
    assert L.mbv_input_runs(None) == -1 and L.mbv_resample_ranges(None, None, 0, 48000, 22050, 0, None) != 0


def test_resample_range_struct_layout_matches_header():
    body = re.search(r"typedef struct mbv_resample_range \{(.*?)\} mbv_resample_range;", _header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype = C.c_void_p if "*" in decl else {"int64_t": C.c_int64, "int32_t": C.c_int32}[decl.split()[0]]
        for name in decl.replace("*", " ").split(","):
            fields.append((name.split()[-1], ctype))
    assert [(n, t) for n, t in _capi.MbvResampleRange._fields_] == fields
    # natural alignment: the int32 after the first pointer is padded to 8
    offsets = {n: getattr(_capi.MbvResampleRange, n).offset for n, _ in fields}
    assert offsets == {"wave": 0, "wave_dtype": 8, "in_avail": 16, "in_total": 24, "out_first": 32, "out_count": 40,
                       "out": 48, "out_capacity": 56}
    assert C.sizeof(_capi.MbvResampleRange) == 64


def test_ready_open_refuses_with_a_message():
    L = _capi.lib()

    def refused(*args):
        assert L.mbv_resample_ready_open(*args) < 0, args
        msg = L.mbv_last_error(None)
        assert msg and b"mbv_resample_ready_open" in msg, (args, msg)
        return msg.decode()

    assert "filter" in refused(48000, 22050, 2, 100)
    assert "filter" in refused(48000, 22050, -1, 100)
    assert "positive" in refused(0, 22050, 0, 100)
    assert "positive" in refused(48000, -3, 0, 100)
    assert "4096 polyphase phases" in refused(44100, 48001, 0, 100)
    assert "ratio too small" in refused(48000, 100, 0, 100)
    # and serves on
    taps, left = C.c_int32(), C.c_int32()
    assert L.mbv_resample_bank(48000, 22050, 0, None, 0, None, C.byref(taps), C.byref(left)) == 0
    want = -(-(5000 - taps.value + left.value + 1) * 147 // 320)         # ceil((in_avail - K + left + 1) L / M)
    assert L.mbv_resample_ready_open(48000, 22050, 0, 5000) == want > 0
    assert L.mbv_resample_ready_open(48000, 22050, 1, 5000) > want       # the shorter filter lags less
