"""Reader of include/robustbnns_hip.h: _hip.py's ctypes structures, prototypes and constants come from the header itself.  Not a C parser:
it reads this header's dialect — `#define RBNN_X <number>`, `typedef struct rbnn_x { scalars and pointers } rbnn_x;`, enums with every
value written out, `ret rbnn_x(type name, ...);` — and refuses, with the line, whatever is left over."""
import ctypes as C
import re
from collections import namedtuple


class HipError(RuntimeError):
    pass


SCALARS = {"int": C.c_int32, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64,
           "size_t": C.c_size_t, "float": C.c_float, "double": C.c_double}
# constants: X -> number (RBNN_X);  structs: C name -> [(field, C type)];  protos: C name -> (C return type, [C parameter type]);
# a C type is spelled "[const ]base[ *]"
Header = namedtuple("Header", "constants structs protos")
_NUMBER = re.compile(r"(-?(?:0[xX][0-9a-fA-F]+|[1-9]\d*|0))[uUlL]*|(-?\d+\.\d*|-?\.\d+)[fF]?")


class _At(Exception):
    """(index into the text, what is wrong there): parse() turns it into a HipError that names the line."""


def _number(s, at):
    m = _NUMBER.fullmatch(s.strip())
    if m is None:
        raise _At(at, f"cannot read the number `{s.strip()}`")
    return int(m[1], 0) if m[1] else float(m[2])


def _declarators(at, s):
    """`const float *W1, *b1` -> [("W1", "const float *"), ("b1", "const float *")]; a parameter, or a return type with its name, likewise."""
    s = " ".join(s.split())
    m = re.fullmatch(r"(const )?(\w+) ?(.*)", s)
    out = []
    for d in (m[3].split(",") if m else [""]):
        dm = re.fullmatch(r" ?(\*?) ?(\w+)", d)
        if dm is None:
            raise _At(at, f"cannot read `{s}` (no arrays, bit-fields, function pointers or pointers to pointers in this header)")
        if not dm[1] and m[2] not in SCALARS:
            raise _At(at, f"unknown scalar type `{m[2]}` in `{s}`")
        out.append((dm[2], (m[1] or "") + m[2] + (" *" if dm[1] else "")))
    return out


def parse(text):
    """The Header of the header's text."""
    h = Header({}, {}, {})
    blank = lambda m: "\n" * m.group().count("\n")

    def struct(m):
        pos, h.structs[m[1]] = m.start(2), []
        for stmt in m[2].split(";"):
            if stmt.strip():
                h.structs[m[1]] += _declarators(pos + len(stmt) - len(stmt.lstrip()), stmt)
            pos += len(stmt) + 1

    def enum(m):
        for e in filter(None, (e.strip() for e in m[1].split(","))):
            em = re.fullmatch(r"RBNN_(\w+)\s*=(.+)", e)
            if em is None:
                raise _At(m.start(), f"cannot read the enumerator `{e}`")
            h.constants[em[1]] = _number(em[2], m.start())

    def proto(m):
        (name, ret), = _declarators(m.start(), m[1])
        if not name.startswith("rbnn_"):
            raise _At(m.start(), f"`{name}` lacks the rbnn_ prefix")
        args = [] if m[2].strip() == "void" else m[2].split(",")
        h.protos[name] = (ret, [t for a in args for _, t in _declarators(m.start(), a)])

    patterns = ((r"/\*.*?\*/|//[^\n]*", None), (r"^[ \t]*#ifdef __cplusplus\n.*?^[ \t]*#endif", None),
                (r"^[ \t]*#define RBNN_(\w+)[ \t]+(\S+)[ \t]*$", lambda m: h.constants.__setitem__(m[1], _number(m[2], m.start()))),
                (r"^[ \t]*#(?!define RBNN_)[^\n]*", None),
                (r"typedef\s+struct\s+(rbnn_\w+)\s*\{([^{}]*)\}\s*\1\s*;", struct), (r"(?:typedef\s+)?enum\s*\w*\s*\{([^{}]*)\}\s*\w*\s*;", enum),
                (r"(\w[\w\s*]*?)\(([^;{}]*)\)\s*;", proto))
    try:
        for pattern, take in patterns:
            text = re.sub(pattern, lambda m: (take and take(m)) or blank(m), text, flags=re.S | re.M)
        rest = re.search(r"\S[^\n]*", text)
        if rest:
            raise _At(rest.start(), f"cannot read the declaration `{rest.group()[:80]}`")
    except _At as e:                        # (every pass keeps the line breaks, so an index names the same line in all of them)
        raise HipError("line %d: %s" % (text.count("\n", 0, e.args[0]) + 1, e.args[1])) from None
    return h


def read(path):
    try:
        with open(path) as f:
            return parse(f.read())
    except FileNotFoundError:
        raise HipError(f"{path} is missing: the ctypes bindings are generated from this header") from None


def bind(header, names, same=None, opaque=()):
    """(classes, signatures) of a Header.  names: Python class name -> C struct; classes: the ctypes.Structure of each, pointer fields c_void_p
    and their names in `_pointers_`.  same: C struct -> a struct of `names` with the same field list, which takes that one's class.  opaque:
    structs without a class.  signatures: C name -> (restype, argtypes): a pointer to a struct with a class is POINTER(that class), a returned
    `const char *` c_char_p, every other pointer c_void_p."""
    same = same or {}
    known = set(names.values()) | set(same) | set(opaque)
    odd = sorted(known ^ set(header.structs))
    if odd:
        raise HipError(f"struct {odd[0]}: " + ("the header lacks it" if odd[0] in known else "the header declares it and the name mapping lacks it"))
    base = lambda t: t.replace("const ", "").rstrip(" *")
    by_c = {}
    for py, c in names.items():
        if c not in by_c:
            by_c[c] = type(py, (C.Structure,), {"_fields_": [(n, C.c_void_p if t.endswith("*") else SCALARS[base(t)]) for n, t in header.structs[c]],
                                                "_pointers_": tuple(n for n, t in header.structs[c] if t.endswith("*"))})
    for c, twin in same.items():
        if header.structs[c] != header.structs[twin]:
            raise HipError(f"struct {c} no longer has the fields of {twin}: they share one class")
        by_c[c] = by_c[twin]

    def ctype(t, ret=False):
        if not t.endswith("*"):
            return SCALARS[base(t)]
        if base(t) in by_c:
            return C.POINTER(by_c[base(t)])
        return C.c_char_p if ret and base(t) == "char" else C.c_void_p

    return {py: by_c[c] for py, c in names.items()}, {name: (ctype(ret, True), [ctype(t) for t in args]) for name, (ret, args) in header.protos.items()}
