"""The C ABI as the headers state it: prototypes, integer constants and plain structs read from a header's text, so that the
ctypes bindings (hip.py, host.py) restate none of it.  Whatever the reader cannot map raises, with the header's text quoted:
an ABI change this binding does not understand fails at import, on the CPU, and never binds as `int`."""
import ctypes as C
import os
import re
from typing import Dict, List, Optional, Tuple

SCALARS = {"int": C.c_int, "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t,
           **{f"{u}int{b}_t": getattr(C, f"c_{u}int{b}") for u in ("", "u") for b in (8, 16, 32, 64)}}

_COMMENT = re.compile(r"/\*.*?\*/|//[^\n]*", re.S)
_DEFINE = re.compile(r"#\s*define\s+(\w+)\s+\(?\s*(-?\s*(?:0[xX][0-9a-fA-F]+|\d+))\s*\)?\s*$")
_INCLUDE = re.compile(r'#\s*include\s+"([^"]+)"')
_EXTERN_C = re.compile(r'extern\s+"C"\s*\{')
# one declaration: a struct with its fields, an opaque struct, or anything else up to its semicolon
_DECL = re.compile(r"\s*(?:typedef\s+struct\s+(\w+)\s*\{([^{}]*)\}\s*(\w+)\s*;"
                   r"|typedef\s+struct\s+(\w+)\s+(\w+)\s*;"
                   r"|([^;{}]+);)")
_PROTO = re.compile(r"(.*?)(\w+)\s*\((.*)\)", re.S)
_PARAM = re.compile(r"(?:const\s+)?(\w+)\s*((?:\*\s*(?:const\s*)?)*)(\w+)?\s*(\[\s*\d*\s*\])?")


class HeaderError(ValueError):
    """the header holds something the reader does not map"""


class Header:
    """prototypes {name: (restype, [argtypes], [parameter names])} in declaration order, constants {NAME: int},
    structs {name: ctypes.Structure class}, opaque {names of `typedef struct x x;`}"""

    def __init__(self):
        self.prototypes: Dict[str, Tuple[object, list, List[str]]] = {}
        self.constants: Dict[str, int] = {}
        self.structs: Dict[str, type] = {}
        self.opaque = set()

    def ctype(self, base: str, depth: int, quote: str, ret: bool = False):
        """the ctypes type of `base` behind `depth` pointers"""
        if base == "void" and depth == 0 and ret:
            return None
        if depth == 1 and base in ("char", "void"):
            return C.c_char_p if base == "char" else C.c_void_p
        if base in SCALARS and depth <= 1:
            return C.POINTER(SCALARS[base]) if depth else SCALARS[base]
        if base in self.structs and depth == 1:
            return C.POINTER(self.structs[base])
        if base in self.opaque and 1 <= depth <= 2:
            return C.POINTER(C.c_void_p) if depth == 2 else C.c_void_p
        if base in self.structs or base in self.opaque:
            what = f"the struct `{base}` by value" if depth == 0 else f"`{base}` behind {depth} pointer levels"
        elif base in SCALARS or base in ("char", "void"):
            what = f"`{base}` behind {depth} pointer levels"
        else:
            what = f"the unknown type `{base}`"
        raise HeaderError(f"{what} is not mapped: `{quote}`")

    def _struct(self, name: str, body: str, quote: str):
        fields = []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            m = re.fullmatch(r"(\w+)\s+(\w+(?:\s*,\s*\w+)*)", decl)
            if not m or m.group(1) not in SCALARS:
                raise HeaderError(f"struct {name}: the field `{decl}` is not a scalar: `{quote}`")
            fields += [(n.strip(), SCALARS[m.group(1)]) for n in m.group(2).split(",")]
        self.structs[name] = type(name, (C.Structure,), {"_fields_": fields})

    def _prototype(self, decl: str):
        m = _PROTO.fullmatch(decl)
        if not m:
            raise HeaderError(f"not a prototype, a struct or an opaque type: `{decl}`")
        ret, name, params = m.group(1).strip(), m.group(2), m.group(3).strip()
        if "(" in params or "(" in ret:
            raise HeaderError(f"parentheses beyond the parameter list's (a function pointer, an attribute) are not mapped: `{decl}`")
        r = _PARAM.fullmatch(ret)
        if not r or r.group(3) or r.group(4):
            raise HeaderError(f"the return type is not mapped: `{decl}`")
        restype = self.ctype(r.group(1), r.group(2).count("*"), decl, ret=True)
        argtypes, names = [], []
        for p in ([] if params in ("", "void") else params.split(",")):
            a = _PARAM.fullmatch(p.strip())
            if not a:
                raise HeaderError(f"the parameter `{p.strip()}` is not mapped: `{decl}`")
            argtypes.append(self.ctype(a.group(1), a.group(2).count("*") + bool(a.group(4)), decl))
            names.append(a.group(3) or "")
        self.prototypes[name] = (restype, argtypes, names)


_headers: Dict[str, Header] = {}


def parse(text: str, included: Optional[Header] = None) -> Header:
    """Read a header's text.  included: the header it includes, whose structs and opaque types its prototypes may name (they
    resolve to that header's classes, not to second ones)."""
    h = Header()
    if included is not None:
        h.structs.update(included.structs)
        h.opaque |= included.opaque
    code = []
    for line in _COMMENT.sub(" ", text).split("\n"):
        if line.lstrip().startswith("#"):
            m = _DEFINE.match(line.strip())
            if m:
                h.constants[m.group(1)] = int(m.group(2).replace(" ", ""), 0)
        else:
            code.append(line)
    body = "\n".join(code)
    m = _EXTERN_C.search(body)
    if m:
        body = body[m.end():body.rindex("}")]
    pos = 0
    for m in _DECL.finditer(body):
        if m.start() != pos:
            break
        pos = m.end()
        quote = " ".join(m.group(0).split())
        if m.group(1):
            if m.group(1) != m.group(3):
                raise HeaderError(f"a struct and its typedef of two names are not mapped: `{quote}`")
            h._struct(m.group(1), m.group(2), quote)
        elif m.group(4):
            h.opaque.add(m.group(5))
        else:
            h._prototype(" ".join(m.group(6).split()))
    if body[pos:].strip():
        raise HeaderError(f"not a declaration the reader knows: `{' '.join(body[pos:].split())[:120]}`")
    return h


def read(path: str) -> Header:
    """The header at `path`, read once per process; a header it includes with #include "..." is read first."""
    path = os.path.abspath(path)
    if path not in _headers:
        with open(path) as f:
            text = f.read()
        inc = _INCLUDE.search(_COMMENT.sub(" ", text))
        _headers[path] = parse(text, read(os.path.join(os.path.dirname(path), inc.group(1))) if inc else None)
    return _headers[path]


def _is_typed_pointer(t) -> bool:
    """a POINTER(T), as against c_void_p / c_char_p and the scalars: ctypes gives every POINTER(T) the one metaclass"""
    return isinstance(t, type(C.POINTER(C.c_int)))


def bind(lib: C.CDLL, header_path: str, addresses: Optional[Dict[str, Tuple[str, ...]]] = None) -> List[str]:
    """Set argtypes / restype on every prototype of the header that `lib` exports; returns their names.
    addresses {function: (parameter names)}: pointers the header types by what they point at but that callers hand over as
    bare addresses (c_void_p): memory that may be the device's.  Every entry must name a pointer parameter of the header."""
    h = read(header_path)
    for fn, params in (addresses or {}).items():
        _, argtypes, names = h.prototypes.get(fn, (None, [], []))
        for p in params:
            if p not in names or not _is_typed_pointer(argtypes[names.index(p)]):
                raise HeaderError(f"{fn}({p}) is no pointer parameter of {os.path.basename(header_path)}")
    bound = []
    for name, (restype, argtypes, names) in h.prototypes.items():
        f = getattr(lib, name, None)
        if f is None:
            continue
        f.restype = restype
        f.argtypes = [C.c_void_p if n in (addresses or {}).get(name, ()) else t for t, n in zip(argtypes, names)]
        bound.append(name)
    return bound
