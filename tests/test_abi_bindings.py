"""The ctypes bindings of robustbnns_amd._hip are generated from include/robustbnns_hip.h (robustbnns_amd/_header.py).  CPU only: the
compiler checks that the reader read what it reads (struct layouts, prototypes, scalar kinds), the built library exports exactly the
prototypes, and the reader refuses whatever is outside the header's dialect, with the line."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

from robustbnns_amd import _header, _hip

pytestmark = pytest.mark.usefixtures("built_library")

C_STRUCTS = {**{c: getattr(_hip, py) for py, c in _hip.STRUCTS.items()}, "rbnn_split_images": _hip.SplitImages}


def _unit():
    """One C++ translation unit of static_asserts: the ctypes classes' sizes and offsets, the parsed prototypes, the scalar map."""
    out = ['#include "%s"' % _hip.HEADER_PATH, "#include <cstddef>", "#include <type_traits>"]
    for c, cls in sorted(C_STRUCTS.items()):
        out.append(f'static_assert(sizeof({c}) == {C.sizeof(cls)}, "sizeof {c}");')
        assert [n for n, _ in _hip.HEADER.structs[c]] == [n for n, _ in cls._fields_], c
        for (name, c_type), (_, ctype) in zip(_hip.HEADER.structs[c], cls._fields_):
            out.append(f'static_assert(offsetof({c}, {name}) == {getattr(cls, name).offset}, "offsetof {c}.{name}");')
            out.append(f'static_assert(std::is_same<decltype({c}::{name}), {c_type}>::value, "type of {c}.{name}");')
            assert ctype is (C.c_void_p if c_type.endswith("*") else _header.SCALARS[c_type.replace("const ", "")]), (c, name)
    for name, (ret, args) in sorted(_hip.HEADER.protos.items()):
        out.append(f'static_assert(std::is_same<decltype(&{name}), {ret} (*)({", ".join(args)})>::value, "prototype of {name}");')
    for c_type, ctype in sorted(_header.SCALARS.items()):
        kind = "floating_point" if ctype in (C.c_float, C.c_double) else "signed" if ctype(-1).value == -1 else "unsigned"
        out.append(f'static_assert(sizeof({c_type}) == {C.sizeof(ctype)} && std::is_{kind}<{c_type}>::value, "scalar {c_type}");')
    return out


def _compile(tmp_path, lines):
    import __graft_entry__ as ge
    src = tmp_path / "abi_probe.hip"
    src.write_text("\n".join(lines) + "\n")
    return subprocess.run([ge.HIPCC, "--offload-arch=gfx950", "-std=c++17", "--cuda-host-only", "-c", "-o", str(tmp_path / "abi_probe.o"), str(src)],
                          capture_output=True, text=True)


def test_layouts_and_prototypes_agree_with_the_compiler(tmp_path):
    """sizeof and every offsetof of every struct as ctypes lays it out, every field's and every prototype's C types as the reader parsed them,
    asserted by the compiler on the header itself.  Two controls show that the unit can fail: one offset and one argument width changed."""
    unit = _unit()
    assert _hip.HEADER.protos and set(_hip.HEADER.protos) == set(_hip.SIGNATURES) and set(C_STRUCTS) | {"rbnn_dev_scale"} == set(_hip.HEADER.structs)
    assert sum("offsetof" in ln for ln in unit) == sum(len(f) for c, f in _hip.HEADER.structs.items() if c in C_STRUCTS)
    r = _compile(tmp_path, unit)
    assert r.returncode == 0, r.stderr[-3000:]
    i = next(i for i, ln in enumerate(unit) if "offsetof(rbnn_nn_train_net, member_stride)" in ln)
    r = _compile(tmp_path, unit[:i] + [unit[i].replace("== 56", "== 52")] + unit[i + 1:])
    assert unit[i] != unit[i].replace("== 56", "== 52") and r.returncode != 0 and "offsetof rbnn_nn_train_net.member_stride" in r.stderr
    i = next(i for i, ln in enumerate(unit) if "decltype(&rbnn_pack_rows4)" in ln)
    r = _compile(tmp_path, unit[:i] + [unit[i].replace("int64_t", "int32_t")] + unit[i + 1:])
    assert "int64_t" in unit[i] and r.returncode != 0 and "prototype of rbnn_pack_rows4" in r.stderr


def test_scalar_map():
    assert _header.SCALARS == {"int": C.c_int32, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64,
                               "size_t": C.c_size_t, "float": C.c_float, "double": C.c_double}
    assert [C.sizeof(_header.SCALARS[t]) for t in ("int", "int32_t", "int64_t", "uint32_t", "uint64_t", "float", "double")] == [4, 4, 8, 4, 8, 4, 8]


def test_signatures_follow_the_pointer_rule():
    """A pointer to a struct with a class is typed, a returned const char * is c_char_p, every other pointer is c_void_p — the scalar
    out-parameters and rbnn_dev_scale included, since their callers pass byref(...), c_void_p instances and plain integers."""
    S = _hip.SIGNATURES
    assert S["rbnn_strerror"] == (C.c_char_p, [C.c_int32]) and S["rbnn_lowdim_scratch_bytes"][0] is C.c_size_t
    assert S["rbnn_svi_train_sizes"] == (C.c_int64, [C.POINTER(_hip.SviTrainNet), C.c_void_p])
    assert S["rbnn_fc_forward_split"][1][:2] == [C.POINTER(_hip.Posterior), C.POINTER(_hip.SplitImages)]
    assert _hip.SplitImages is _hip.TripleImages is _hip.PieceImages
    assert S["rbnn_svi_adam_step"][1] == [C.POINTER(_hip.SviTrainNet), C.c_uint64, C.c_uint32, C.c_int64] + [C.c_double] * 4 + [C.c_void_p] * 2
    typed = {t for _, args in S.values() for t in args if hasattr(t, "contents")}
    assert typed == {C.POINTER(cls) for cls in C_STRUCTS.values()}
    assert not any(t is C.c_char_p for _, args in S.values() for t in args)
    for c, (ret, args) in _hip.HEADER.protos.items():                       # rbnn_dev_scale has no class: untyped wherever it appears
        assert all(S[c][1][i] is C.c_void_p for i, t in enumerate(args) if "rbnn_dev_scale" in t)
    n = C.c_int32(0)
    assert C.c_void_p.from_param(C.byref(n)) is not None and C.c_void_p.from_param(None) is None


def test_constants_and_key_tuples_come_from_the_header():
    k = _hip.HEADER.constants
    assert (_hip.ABI_VERSION, _hip.CPAD, _hip.HMC_STATE, _hip.HMC_LOG, _hip.SVI_LOCKSTEP_ACC_SAMPLES) == (10, 16, 16, 8, 10)
    assert _hip.SVI_EPS_MAX == 6.77 and _hip.HMC_UNIF_KEY == 0xE7037ED1A0B428DB and _hip.HMC_SEARCH_KEY == 0xA0761D6478BD642F
    assert all(getattr(_hip, name) == v for name, v in k.items()) and k["ERR_ALIGN"] == -5
    assert _hip.ACTIVATIONS == {"relu": 0, "leaky": 1, "sigm": 2, "tanh": 3} and _hip.ARCHS == {"fc": 0, "fc2": 1}
    assert sorted(_hip.HMC_ST.values()) == list(range(13)) == sorted(v for n, v in k.items() if n.startswith("HMC_ST_"))
    assert (_hip.HipKernels.LOWDIM_FORWARD, _hip.HipKernels.LOWDIM_GRADIENT, _hip.HipKernels.LOWDIM_ATTACK) == (0, 1, 2)
    from robustbnns_amd import svi_train
    assert svi_train.ACC_SAMPLES == k["SVI_MULTI_ACC_SAMPLES"]
    for keys, cls in ((_hip.WS_KEYS, _hip.Workspace), (_hip.CONV_WS_KEYS, _hip.ConvWorkspace), (_hip.SPLIT_WS_KEYS, _hip.SplitWorkspace),
                      (_hip.TRIPLE_WS_KEYS, _hip.TripleWorkspace), (_hip.SVI_TRAIN_WS_KEYS, _hip.SviTrainWs), (_hip.NN_TRAIN_WS_KEYS, _hip.NnTrainWs),
                      (_hip.CONV_TRAIN_WS_KEYS, _hip.ConvTrainWs), (_hip.SVI_LOCKSTEP_ACC_KEYS, _hip.SviLockstepAcc)):
        assert keys == tuple(n for n, _ in _hip.HEADER.structs[_hip.STRUCTS[cls.__name__]]) == cls._pointers_
    assert _hip.WS_KEYS == ("P", "dZ", "mask1", "dact1", "hid1", "mask2", "dact2", "dhid1", "slabs")


def test_library_exports_exactly_the_prototypes():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import kernel_resources as KR
    out = subprocess.run([KR.READELF, "--dyn-syms", "-W", _hip.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if re.search(r"\bFUNC\s+GLOBAL\s+DEFAULT\s+\d+\s+rbnn_\w+$", ln)}
    assert exported == set(_hip.SIGNATURES), exported ^ set(_hip.SIGNATURES)


OK_STRUCT = "typedef struct rbnn_a { int32_t n; float *p; } rbnn_a;\n"
REFUSED = [
    ("unknown scalar", OK_STRUCT + "\ntypedef struct rbnn_b {\n    int32_t n;\n    long double x;\n} rbnn_b;\n", 5, "long"),
    ("unknown scalar in a prototype", OK_STRUCT + "int rbnn_f(int32_t n,\n           short k);\n", 2, "short"),
    ("struct by value", OK_STRUCT + "int rbnn_f(rbnn_a a);\n", 2, "rbnn_a"),
    ("array member", "typedef struct rbnn_b {\n    float *p;\n    int32_t dims[4];\n} rbnn_b;\n", 3, "dims[4]"),
    ("bit-field member", "typedef struct rbnn_b {\n    uint32_t flag : 1;\n} rbnn_b;\n", 2, "flag : 1"),
    ("function-pointer member", "typedef struct rbnn_b {\n    int (*cb)(int);\n} rbnn_b;\n", 2, "cb"),
    ("function-pointer parameter", "\n\nint rbnn_f(int32_t n, void (*cb)(void *), void *stream);\n", 3, "cb"),
    ("pointer to a pointer", "int rbnn_f(float **rows);\n", 1, "rows"),
    ("prototype without the prefix", OK_STRUCT + "\nint other_f(int32_t n);\n", 3, "other_f"),
    ("struct without the prefix", "typedef struct thing { int32_t n; } thing;\n", 1, "thing"),
    ("enumerator without a value", "typedef enum rbnn_e {\n    RBNN_A = 0,\n    RBNN_B } rbnn_e;\n", 1, "RBNN_B"),
    ("macro", "#define RBNN_OK_ONE 1\n#define RBNN_TWICE(x) (2 * (x))\n", 2, "RBNN_TWICE"),
    ("global variable", OK_STRUCT + "extern int rbnn_counter;\n", 2, "rbnn_counter"),
]


@pytest.mark.parametrize("what,text,line,word", REFUSED, ids=[r[0] for r in REFUSED])
def test_reader_refuses_what_it_cannot_read(what, text, line, word):
    with pytest.raises(_hip.HipError, match=rf"line {line}\b.*{re.escape(word)}"):
        _header.parse(text)


def test_reader_reads_the_dialect_comments_included():
    h = _header.parse("/* a header; with (parens) */\n#ifndef H\n#define H\n#ifdef __cplusplus\nextern \"C\" {\n#endif\n#define RBNN_N 3\n"
                      "#define RBNN_KEY 0xFFull\n#define RBNN_EPS 1.5f\n"
                      "typedef struct rbnn_a {   /* stray ; and ( in a comment */\n    const float *x, *y;   /* [n]; see f( */\n"
                      "    // int32_t ghost;\n    size_t n, m;\n    uint8_t *st;\n} rbnn_a;\n"
                      "enum { RBNN_P = 0, RBNN_Q = -2 };\n"
                      "const char *rbnn_name(int status);\nint64_t rbnn_f(const rbnn_a *a, const int32_t *counts, double lr, void *stream);\n"
                      "int rbnn_v(void);\n#ifdef __cplusplus\n}\n#endif\n#endif\n")
    assert h.constants == {"N": 3, "KEY": 255, "EPS": 1.5, "P": 0, "Q": -2}
    assert h.structs == {"rbnn_a": [("x", "const float *"), ("y", "const float *"), ("n", "size_t"), ("m", "size_t"), ("st", "uint8_t *")]}
    assert h.protos == {"rbnn_name": ("const char *", ["int"]), "rbnn_v": ("int", []),
                        "rbnn_f": ("int64_t", ["const rbnn_a *", "const int32_t *", "double", "void *"])}
    classes, sigs = _header.bind(h, {"A": "rbnn_a"})
    assert classes["A"]._fields_ == [("x", C.c_void_p), ("y", C.c_void_p), ("n", C.c_size_t), ("m", C.c_size_t), ("st", C.c_void_p)]
    assert classes["A"]._pointers_ == ("x", "y", "st")
    assert sigs == {"rbnn_name": (C.c_char_p, [C.c_int32]), "rbnn_v": (C.c_int32, []),
                    "rbnn_f": (C.c_int64, [C.POINTER(classes["A"]), C.c_void_p, C.c_double, C.c_void_p])}


def test_struct_mapping_and_header_must_agree(tmp_path):
    h = _header.parse(OK_STRUCT + "typedef struct rbnn_b { int32_t n; float *p; } rbnn_b;\ntypedef struct rbnn_c { int64_t n; } rbnn_c;\n")
    with pytest.raises(_hip.HipError, match="rbnn_zz.*header lacks"):
        _header.bind(h, {"A": "rbnn_a", "B": "rbnn_b", "C": "rbnn_c", "Z": "rbnn_zz"})
    with pytest.raises(_hip.HipError, match="rbnn_c.*mapping lacks"):
        _header.bind(h, {"A": "rbnn_a", "B": "rbnn_b"})
    classes, _ = _header.bind(h, {"A": "rbnn_a", "Also": "rbnn_a"}, same={"rbnn_b": "rbnn_a"}, opaque=("rbnn_c",))
    assert classes["A"] is classes["Also"]
    with pytest.raises(_hip.HipError, match="rbnn_c no longer has the fields of rbnn_a"):
        _header.bind(h, {"A": "rbnn_a", "B": "rbnn_b"}, same={"rbnn_c": "rbnn_a"})
    with pytest.raises(_hip.HipError, match=re.escape(str(tmp_path / "nowhere.h"))):
        _header.read(str(tmp_path / "nowhere.h"))


def test_fill_sets_the_pointer_fields_by_name():
    class T:
        def __init__(self, p):
            self.data_ptr = lambda: p

    ws = _hip.fill(_hip.Workspace, {"P": T(16), "slabs": T(32), "dZ": None, "unrelated": 1})
    assert isinstance(ws, _hip.Workspace) and (ws.P, ws.slabs, ws.dZ, ws.mask1) == (16, 32, None, None)

    class Holder:
        pass

    obj = Holder()
    obj.P, obj.m, obj.v, obj.grad, obj.n_members = T(48), T(64), T(80), T(96), "not a field that is filled"
    net = _hip.NnTrainNet()
    net.n_members, net.member_stride = 3, 7
    assert _hip.fill(net, obj) is net and (net.P, net.m, net.v, net.grad, net.n_members, net.member_stride) == (48, 64, 80, 96, 3, 7)
