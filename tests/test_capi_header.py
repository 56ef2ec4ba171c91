"""`_capi.TABLE`, `_capi.STRUCTS` and the mirrored constants, held to `include/mbistft_vits.h` (CPU only).

Every prototype of the header is compared with the binding's restype and argtypes by kind, every mirrored struct by
field names and by the offsets a C compiler gives them, every `#define` by value; `reference_binding.py` goes through
the same comparisons.  The last test seeds five mistakes and expects each to be reported at its name."""
import ctypes as C
import os
import re
import shutil
import struct
import subprocess
import types

import pytest

from mb_istft_vits_amd import _capi, models, reference_binding, spec, stream

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mbistft_vits.h")
SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64,
           "size_t": C.c_size_t, "float": C.c_float, "double": C.c_double}

# set(SYMBOLS) - set(optional) of the commit before the table, copied from it: what every build must export
CORE = {
    "mbv_abi_version", "mbv_create", "mbv_destroy", "mbv_last_error", "mbv_load_weight", "mbv_finalize_weights",
    "mbv_missing_weights", "mbv_encode", "mbv_synthesize", "mbv_decode", "mbv_speaker_embedding", "mbv_stage_times_ms",
    "mbv_istft_pqmf", "mbv_read_stage", "mbv_op_conv1d", "mbv_kernel_times_ms", "mbv_istft_finalize", "mbv_pcm16",
    "mbv_voice_conversion", "mbv_set_option", "mbv_arena_floats", "mbv_export_arena", "mbv_import_arena", "mbv_ticket",
    "mbv_stage_times_ms_at", "mbv_op_rel_attention", "mbv_pcm16_samples", "mbv_resample", "mbv_resample_bank",
    "mbv_op_conv", "mbv_conv_plan", "mbv_spectrogram", "mbv_spectrogram_frames", "mbv_decoder_context",
    "mbv_decode_range", "mbv_resample_ready", "mbv_resample_pcm16_range", "mbv_op_embed", "mbv_op_layernorm",
    "mbv_op_durations", "mbv_op_expand", "mbv_op_cond_gemv", "mbv_op_gather_rows", "mbv_op_posterior_sample",
    "mbv_op_lens", "mbv_op_dds_sep", "mbv_op_dds_res", "mbv_op_sdp_pre", "mbv_op_sdp_spline", "mbv_op_sdp_logw",
    "mbv_op_sdp_noise", "mbv_op_chan_add", "mbv_op_istft_single", "mbv_align", "mbv_set_durations", "mbv_op_neg_cent",
    "mbv_op_max_path",
}


# ---- the header -------------------------------------------------------------------------------------------------
def parse_header():
    """-> (protos: name -> (return type, [parameter, ..]), structs: name -> [(type text, field), ..], defines)."""
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    defines = dict(re.findall(r"^[ \t]*#[ \t]*define[ \t]+(MBV_\w+)[ \t]+(\S+)[ \t]*$", text, flags=re.M))
    text = re.sub(r"^[ \t]*#[^\n]*$", "", text, flags=re.M)       # else a #define ends up in the next return type
    text = text.replace('extern "C" {', "")
    structs = {}

    def take_struct(m):
        fields = []
        for decl in filter(None, (d.strip() for d in m.group(2).split(";"))):
            first, *more = [p.strip() for p in decl.split(",")]
            head = re.match(r"(.*?)(\w+)\s*((?:\[\w+\])*)$", first, re.S)
            fields.append((" ".join((head.group(1) + head.group(3)).split()), head.group(2)))
            assert not any("*" in name or "[" in name for name in more), decl
            fields += [(fields[-1][0], name) for name in more]                     # `float lo, hi;`
        structs[m.group(1)] = fields
        return ""
    text = re.sub(r"typedef\s+struct\s+(mbv_\w+)\s*\{(.*?)\}\s*\1\s*;", take_struct, text, flags=re.S)
    text = re.sub(r"typedef\s+struct\s+mbv_model\s+mbv_model\s*;", "", text)
    text = re.sub(r"\}\s*$", "", text)                                               # the end of extern "C"
    protos = {}
    for decl in filter(None, (" ".join(d.split()) for d in text.split(";"))):
        m = re.fullmatch(r"([\w\s\*]+?)\s*\b(mbv_\w+)\s*\((.*)\)", decl)
        assert m, "the header has a statement this parser does not read: %r" % decl
        assert m.group(2) not in protos, m.group(2)
        params = [p.strip() for p in m.group(3).split(",")]
        protos[m.group(2)] = (m.group(1).strip(), [] if params == ["void"] else params)
    return protos, structs, defines


PROTOS, HEADER_STRUCTS, DEFINES = parse_header()


def header_kind(text, named):
    """The kind of a return type (named False) or of a parameter: ("scalar", ctype) | ("char*",) | ("void",) |
    ("struct*", c name) | ("array", element ctype, n) | ("ptr",)."""
    text = " ".join(re.sub(r"\bconst\b", " ", text).split())
    array = re.search(r"\[(\w+)\]$", text)
    if array:
        text = text[:array.start()].strip()
    if named:
        text = re.sub(r"\s*\b\w+$", "", text).strip()
    base, stars = text.replace("*", " ").strip(), text.count("*")
    if array:
        return ("array", SCALARS[base], int(array.group(1))) if not stars else ("ptr",)
    if stars:
        if (base, stars) == ("char", 1):
            return ("char*",)
        return ("struct*", base) if (stars == 1 and base in HEADER_STRUCTS) else ("ptr",)
    return ("void",) if base == "void" else ("scalar", SCALARS[base])


def binding_kind(t, structs):
    if t is None:
        return ("void",)
    if t is C.c_char_p:
        return ("char*",)
    if t is C.c_void_p:
        return ("ptr",)
    if issubclass(t, C._Pointer):
        to = t._type_
        if issubclass(to, C.Structure):
            return ("struct*", {cls: name for name, cls in structs.items()}.get(to, to.__name__))
        return ("array", to._type_, to._length_) if issubclass(to, C.Array) else ("ptr",)
    return ("scalar", t)


def agree(h, b):
    """Exact, except that a plain pointer of the binding stands for any pointer or array but `char *`."""
    return h == b or (b == ("ptr",) and h[0] in ("ptr", "struct*", "array"))


# ---- the comparisons ----------------------------------------------------------------------------------------------
def proto_errors(table, structs):
    """[(name, what)] for every entry of `table` (name -> (restype, argtypes)) that differs from its prototype."""
    errors = []
    for name, (restype, argtypes) in table.items():
        if name not in PROTOS:
            errors.append((name, "not declared by the header"))
            continue
        ret, params = PROTOS[name]
        if not agree(header_kind(ret, False), binding_kind(restype, structs)):
            errors.append((name, "returns %s, bound as %r" % (ret, restype)))
        if len(params) != len(argtypes or ()):
            errors.append((name, "takes %d arguments, bound with %d" % (len(params), len(argtypes or ()))))
            continue
        for i, (p, a) in enumerate(zip(params, argtypes or ())):
            if not agree(header_kind(p, True), binding_kind(a, structs)):
                errors.append((name, "argument %d is `%s`, bound as %r" % (i, p, a)))
    return errors


def struct_errors(structs, layout):
    """[(c name, what)] for every class of `structs` whose fields, offsets or size differ from the header's struct."""
    errors = []
    for name, cls in structs.items():
        want, got = [f for _, f in HEADER_STRUCTS[name]], [f[0] for f in cls._fields_]
        if want != got:
            errors.append((name, "fields %s, bound as %s" % (want, got)))
        if layout[name] != (C.sizeof(cls),):
            errors.append((name, "sizeof %d, bound as %d" % (layout[name][0], C.sizeof(cls))))
        for f in got:
            d = getattr(cls, f)
            if layout.get("%s.%s" % (name, f)) != (d.offset, d.size):
                errors.append((name, "%s at %s, bound at %s" % (f, layout.get(name + "." + f), (d.offset, d.size))))
    return errors


@pytest.fixture(scope="module")
def layout(tmp_path_factory):
    """`sizeof` of every struct of the header and (offsetof, size) of every field, as the host C compiler sees them."""
    cc = shutil.which("cc") or shutil.which("clang") or shutil.which("clang", path="/opt/rocm/llvm/bin")
    assert cc, "no C compiler (cc, or ROCm's clang) to lay the header's structs out with"
    lines = ['#include "%s"' % HEADER, "#include <stdio.h>", "int main(void) {"]
    for s, fields in HEADER_STRUCTS.items():
        lines.append('  printf("%s %%zu\\n", sizeof(%s));' % (s, s))
        lines += ['  printf("%s.%s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s *)0)->%s));' % (s, f, s, f, s, f)
                  for _, f in fields]
    lines += ["  return 0;", "}"]
    d = tmp_path_factory.mktemp("layout")
    (d / "layout.c").write_text("\n".join(lines) + "\n")
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", str(d / "layout.c"), "-o", str(d / "layout")], check=True)
    out = subprocess.run([str(d / "layout")], check=True, capture_output=True, text=True).stdout
    return {w[0]: tuple(int(v) for v in w[1:]) for w in (line.split() for line in out.splitlines())}


class StubLibrary:
    """Stands in for a CDLL: one attribute per exported function, with ctypes' defaults."""

    def __init__(self, names):
        for n in names:
            setattr(self, n, types.SimpleNamespace(restype=C.c_int, argtypes=None))

    def declared(self):
        return {n: (f.restype, f.argtypes) for n, f in vars(self).items() if f.argtypes is not None}


# ---- the tests ----------------------------------------------------------------------------------------------------
def test_table_matches_every_prototype():
    assert set(PROTOS) == set(_capi.SYMBOLS) == set(_capi.TABLE)
    assert _capi.SYMBOLS == list(_capi.TABLE) and len(set(_capi.SYMBOLS)) == len(_capi.SYMBOLS)
    assert set(_capi.CORE) == CORE and set(_capi.LATER) == set(PROTOS) - CORE
    assert proto_errors(_capi.TABLE, _capi.STRUCTS) == []
    lib = StubLibrary(_capi.SYMBOLS)
    _capi.declare(lib, allow_missing=False)
    assert lib.declared() == {n: (r, a) for n, (r, a) in _capi.TABLE.items()}


def test_structs_match_the_header(layout):
    assert set(HEADER_STRUCTS) == set(_capi.STRUCTS) | {"mbv_fit_result"}        # the one struct without a class
    assert len(set(_capi.STRUCTS.values())) == len(_capi.STRUCTS)
    mirrored = {v for v in vars(_capi).values() if isinstance(v, type) and issubclass(v, C.Structure)} - {C.Structure}
    assert mirrored == set(_capi.STRUCTS.values())
    assert struct_errors(_capi.STRUCTS, layout) == []


def test_fit_result_unpacks_the_headers_two_fields(layout):
    """`fit_result` reads an int64 of a read-back as the header's {float scale; int32_t status;}."""
    assert HEADER_STRUCTS["mbv_fit_result"] == [("float", "scale"), ("int32_t", "status")]
    assert (layout["mbv_fit_result"], layout["mbv_fit_result.scale"], layout["mbv_fit_result.status"]) \
        == ((8,), (0, 4), (4, 4)) and struct.calcsize("<fi") == 8
    word, = struct.unpack("<q", struct.pack("<fi", 1.5, -7))
    assert _capi.fit_result(word) == (1.5, -7)


def test_constants_equal_the_headers_defines():
    mirrors = {"MBV_ABI_VERSION": _capi.ABI_VERSION, "MBV_TURN_MAX_SEGS": _capi.TURN_MAX_SEGS,
               "MBV_PITCH_MIN": _capi.PITCH_MIN, "MBV_PITCH_MAX": _capi.PITCH_MAX,
               "MBV_SPEAKER_SLOTS": _capi.SPEAKER_SLOTS, "MBV_BLEND_MAX": _capi.BLEND_MAX,
               "MBV_DEC_MULTIBAND": spec.DEC_MB, "MBV_DEC_MULTISTREAM": spec.DEC_MS, "MBV_DEC_SINGLEBAND": spec.DEC_SB}
    for prefix, names in (("MBV_WAVE_", ("F32", "PCM16", "ULAW", "ALAW")),
                          ("MBV_NOISE_", ("PRIOR", "SDP", "POSTERIOR")),
                          ("MBV_CONV_KIND_", ("CONV", "CONVT4", "CONVT8")),
                          ("MBV_CONV_EPI_", ("STORE", "RESID", "RESID_ACC", "LN"))):
        mirrors.update({prefix + n: getattr(_capi, prefix[4:] + n) for n in names})
    mirrors.update({"MBV_G711_" + k.upper(): v for k, v in _capi.G711_LAWS.items()})
    mirrors.update({"MBV_RESAMPLE_" + k.upper(): v for k, v in _capi.RESAMPLE_TYPES.items()})
    mirrors.update({"MBV_ROUTE_" + name: code for code, name in _capi.ROUTES.items()})
    assert set(mirrors) == set(DEFINES), set(mirrors) ^ set(DEFINES)          # every #define MBV_* has its mirror
    for name, value in mirrors.items():
        assert type(value)(DEFINES[name].rstrip("f")) == value, name
    assert len(_capi.ROUTES) == sum(n.startswith("MBV_ROUTE_") for n in DEFINES)
    assert models.RESAMPLE_TYPES is _capi.RESAMPLE_TYPES and stream.RES_TYPES is _capi.RESAMPLE_TYPES
    assert (models.PITCH_MIN, models.PITCH_MAX) == (_capi.PITCH_MIN, _capi.PITCH_MAX)


def test_reference_binding_matches_the_header(layout, monkeypatch):
    """The stand-alone binding declares its own eleven entries and two structs: the same checks, on what it declares."""
    lib = StubLibrary(PROTOS)
    monkeypatch.setattr(reference_binding, "_LIB", None)
    monkeypatch.setattr(C, "CDLL", lambda path: lib)
    assert reference_binding._lib() is lib
    own = {"mbv_config": reference_binding.MbvConfig, "mbv_outputs": reference_binding.MbvOutputs}
    declared = lib.declared()
    called = set(re.findall(r"\.(mbv_\w+)\(", open(reference_binding.__file__).read()))
    assert called and called == set(declared)
    assert proto_errors(declared, own) == []
    assert struct_errors(own, layout) == []


def test_loading_rule():
    """A core entry must resolve in every library, a later one in the in-tree library only."""
    later = [s for s in _capi.SYMBOLS if s not in CORE]
    assert len(later) == len(_capi.SYMBOLS) - len(CORE) > 0
    old = StubLibrary(CORE)
    _capi.declare(old, allow_missing=True)                          # a baseline build from before every later entry
    assert set(old.declared()) == CORE and not hasattr(old, later[0])
    with pytest.raises(AttributeError):
        _capi.declare(StubLibrary(CORE), allow_missing=False)
    for gone in ("mbv_abi_version", "mbv_op_max_path", later[0], later[-1]):
        with pytest.raises(AttributeError, match=gone):
            _capi.declare(StubLibrary(s for s in _capi.SYMBOLS if s != gone), allow_missing=False)
    for gone in ("mbv_abi_version", "mbv_read_stage", "mbv_op_max_path"):
        with pytest.raises(AttributeError, match=gone):
            _capi.declare(StubLibrary(s for s in _capi.SYMBOLS if s != gone), allow_missing=True)
    one = StubLibrary(s for s in _capi.SYMBOLS if s != later[-1])
    _capi.declare(one, allow_missing=True)                            # per entry: its siblings are declared
    assert set(one.declared()) == set(_capi.SYMBOLS) - {later[-1]}


def test_the_checks_report_seeded_mistakes(layout):
    """One c_int -> c_int64, a dropped argument, a forgotten restype, two fields swapped, a trailing field dropped."""
    def seeded(name, restype=None, argtypes=None):
        r, a = _capi.TABLE[name]
        table = dict(_capi.TABLE)
        table[name] = (restype(r) if restype else r, argtypes(list(a)) if argtypes else a)
        return {n for n, _ in proto_errors(table, _capi.STRUCTS)}

    a = _capi.TABLE["mbv_decode_range"][1]
    assert a[3] is C.c_int and a[-1] is C.c_void_p and header_kind(PROTOS["mbv_decode_range"][1][-1], True) == ("ptr",)
    assert seeded("mbv_decode_range", argtypes=lambda a: a[:3] + [C.c_int64] + a[4:]) == {"mbv_decode_range"}
    assert seeded("mbv_decode_range", argtypes=lambda a: a[:-2] + a[-1:]) == {"mbv_decode_range"}  # before stream
    assert _capi.TABLE["mbv_wire_runs"][0] is C.c_int64
    assert seeded("mbv_wire_runs", restype=lambda r: C.c_int) == {"mbv_wire_runs"}     # what ctypes assumes unstated

    fields = list(_capi.MbvPcmChunk._fields_)
    swapped = type("Swapped", (C.Structure,), {"_fields_": fields[:3] + [fields[4], fields[3]] + fields[5:]})
    dropped = type("Dropped", (C.Structure,), {"_fields_": fields[:-1]})
    assert C.sizeof(swapped) == C.sizeof(_capi.MbvPcmChunk)                     # the size alone would not have told
    for bad in (swapped, dropped):
        found = struct_errors(dict(_capi.STRUCTS, mbv_pcm_chunk=bad), layout)
        assert found and {n for n, _ in found} == {"mbv_pcm_chunk"}
