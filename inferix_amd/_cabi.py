"""Reader for the C subset of include/inferix_hip.h: the ctypes structs, the name -> (restype, argtypes) table and the IFX_* constants
of inferix_amd/_hip.py are derived from the header here.  The grammar is what the header uses (comments, include guard, `#include`,
the `extern "C"` wrapper, integer `#define`s, anonymous enums with values, scalar typedefs, `typedef struct`s of scalars / pointers /
fixed arrays, prototypes); anything else raises HeaderError with the line: nothing is skipped.
Type rules (the whole policy): SCALARS and typedefs of them by value; `const char*` -> c_char_p; a pointer to a
struct of the header -> POINTER(ThatStruct); every other pointer -> c_void_p.  Fields follow the same rules except HOST_ARRAY_FIELDS,
which stay POINTER(scalar): C cannot tell a device pointer from a host array that the library reads during the call, and a POINTER
field keeps the Python array it was given alive.  A field named like a Python keyword gets a trailing underscore.
A second header that `#include "..."`s the first (include/inferix_hip_sessions.h) is read over the first one's names (`parse(base=...)`,
`load(path, base=(base_path, base_header))`): its structs may point to the first header's, and the result is its own declarations only."""
import ctypes as C
import keyword
import re
from collections import namedtuple

HOST_ARRAY_FIELDS = frozenset({("ifx_conv3d_desc", "in_slots"), ("ifx_conv3d_desc", "out_slots")})
SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint8_t": C.c_uint8, "uint16_t": C.c_uint16, "float": C.c_float}
POINTEE_ONLY = ("void", "char", "double")      # known names that may stand behind a `*` only
Header = namedtuple("Header", "constants structs functions")      # name -> int, C name -> Structure class, name -> (restype, [argtypes])


class HeaderError(ValueError):
    pass


_INT = r"-?(?:0[xX][0-9a-fA-F]+|\d+)"
_EOL = r"[ \t]*(?=\n|\Z)"
_WS = re.compile(r"\s*")
_GUARD = re.compile(r"#ifndef[ \t]+(\w+)[ \t]*\n\s*#define[ \t]+\1" + _EOL)
_ENDIF = re.compile(r"#endif" + _EOL)
_CPP = re.compile(r'#ifdef[ \t]+__cplusplus[ \t]*\n\s*(extern\s+"C"\s*\{|\})[ \t]*\n\s*#endif' + _EOL)
_INCLUDE = re.compile(r"#include[ \t]*<[\w./]+>" + _EOL)
_INCLUDE_BASE = re.compile(r'#include[ \t]*"[\w./]+"' + _EOL)      # only in a header parsed over a base (parse(base=...))
_DEFINE = re.compile(rf"#define[ \t]+(\w+)[ \t]+(?:({_INT})|\(\s*({_INT})\s*\))" + _EOL)
_ENUM = re.compile(r"enum\s*\{([^{};]*)\}\s*;")
_ENUMERATOR = re.compile(rf"\s*(\w+)\s*=\s*({_INT})\s*")
_STRUCT = re.compile(r"typedef\s+struct(?:\s+\w+)?\s*\{([^{}]*)\}\s*(\w+)\s*;")
_TYPEDEF = re.compile(r"typedef\s+(\w+)\s+(\w+)\s*;")
_PROTO = re.compile(r"(const\s+)?(?!typedef\b)(\w+)(?:\s*(\*+)\s*|\s+)(\w+)\s*\(([^(){};]*)\)\s*;")
_FIELD_TYPE = re.compile(r"\s*(const\s+)?(\w+)\b")
_DECLARATOR = re.compile(r"\s*(\*+)?\s*(\w+)\s*(?:\[\s*(\w+)\s*\])?\s*")
_PARAM = re.compile(r"\s*(const\s+)?(\w+)\s*(\*+)?\s*(\w*)\s*")


def parse(text: str, host_array_fields=HOST_ARRAY_FIELDS, base=None) -> Header:
    """`base`: a (Header, {typedef name: ctype}) pair from `parse_base` — the header this one `#include "..."`s.  Its names are known
    (and cannot be declared again); the result holds only what `text` itself declares."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", lambda m: re.sub(r"[^\n]", " ", m.group()), text, flags=re.S)   # blanked: lines stay
    constants, structs, functions, scalars, seen, host_left = {}, {}, {}, dict(SCALARS), set(), set(host_array_fields)
    if base is not None:
        constants, structs, functions = dict(base[0].constants), dict(base[0].structs), dict(base[0].functions)
        scalars.update(base[1])
        seen.update(base[0].constants, base[0].structs, base[0].functions, base[1])
    known = len(seen)

    def fail(pos, why):
        raise HeaderError(f"line {text.count(chr(10), 0, pos) + 1}: {why}")

    def declare(pos, name):
        if name in seen or name in SCALARS or name in POINTEE_ONLY:
            fail(pos, f"'{name}' is declared twice")
        seen.add(name)

    def ctype(pos, const, base, stars, field=False):
        if base not in scalars and base not in structs and base not in POINTEE_ONLY:
            fail(pos, f"unknown type name '{base}'")
        if not stars:
            if base in scalars or (field and base in structs):
                return scalars.get(base) or structs[base]
            fail(pos, f"no rule for '{base}' by value here")
        if stars == 1 and (base in structs or (const and base == "char")):
            return C.POINTER(structs[base]) if base in structs else C.c_char_p
        return C.c_void_p

    def struct(m):
        body, name = m.groups()
        declare(m.start(), name)
        fields, at = [], m.start(1)
        *decls, tail = body.split(";")
        if tail.strip():
            fail(at + len(body) - len(tail.lstrip()), f"declaration without ';' in {name}: '{tail.strip()}'")
        for decl in decls:
            pos, at = at + len(decl) - len(decl.lstrip()), at + len(decl) + 1
            t = _FIELD_TYPE.match(decl)
            if not t:
                fail(pos, f"not a field of the header's C subset: '{decl.strip()}'")
            for d in decl[t.end():].split(","):
                dm = _DECLARATOR.fullmatch(d)
                if not dm:
                    fail(pos, f"not a declarator of the header's C subset (bit-fields and function pointers are not): '{d.strip()}'")
                stars, field, count = len(dm.group(1) or ""), dm.group(2), dm.group(3)
                ct = ctype(pos, t.group(1), t.group(2), stars, field=True)
                if (name, field) in host_left:
                    host_left.discard((name, field))
                    if stars != 1 or t.group(2) not in scalars or count:
                        fail(pos, f"HOST_ARRAY_FIELDS entry {name}.{field} is not a pointer to a scalar")
                    ct = C.POINTER(scalars[t.group(2)])
                if count is not None:
                    n = int(count) if count.isdigit() else constants.get(count)
                    if not n:
                        fail(pos, f"array length '{count}' of {name}.{field} is not a positive integer or an earlier #define")
                    ct = ct * n
                declare(pos, f"{name}.{field}")
                fields.append((field + "_" * keyword.iskeyword(field), ct))
        cls = "".join(w.capitalize() for w in name.removeprefix("ifx_").split("_"))
        structs[name] = type(cls, (C.Structure,), {"_fields_": fields, "__doc__": name})

    def proto(m):
        const, base, stars, name, params = m.groups()
        declare(m.start(), name)
        res, args = ctype(m.start(), const, base, len(stars or "")), []
        for p in params.split(",") if params.strip() != "void" else ():
            pm = _PARAM.fullmatch(p)
            if not pm:
                fail(m.start(), f"not a parameter of the header's C subset in {name} (variadic lists and function pointers are not): '{p.strip()}'")
            args.append(ctype(m.start(), pm.group(1), pm.group(2), len(pm.group(3) or "")))
        functions[name] = (res, args)

    def define(pos, name, value):
        declare(pos, name)
        constants[name] = int(value, 0)

    pos, guard, closed = 0, None, False
    while (pos := _WS.match(text, pos).end()) < len(text):
        if closed:
            fail(pos, "text behind the #endif of the include guard")
        if (m := _GUARD.match(text, pos)) and not guard and len(seen) == known:
            guard = m.group(1)
        elif (m := _ENDIF.match(text, pos)) and guard:
            closed = True
        elif (m := _CPP.match(text, pos)) or (m := _INCLUDE.match(text, pos)) or (base is not None and (m := _INCLUDE_BASE.match(text, pos))):
            pass                                               # the wrapper's balance is the C++ compiler's business
        elif m := _DEFINE.match(text, pos):
            define(pos, m.group(1), m.group(2) or m.group(3))
        elif m := _ENUM.match(text, pos):
            for e in m.group(1).split(","):
                if not (em := _ENUMERATOR.fullmatch(e)):
                    fail(pos, f"enumerator without an explicit integer value: '{e.strip()}'")
                define(pos, *em.groups())
        elif m := _STRUCT.match(text, pos):
            struct(m)
        elif m := _TYPEDEF.match(text, pos):
            if m.group(1) not in scalars:
                fail(pos, f"unknown type name '{m.group(1)}'")
            declare(pos, m.group(2))
            scalars[m.group(2)] = scalars[m.group(1)]
        elif m := _PROTO.match(text, pos):
            proto(m)
        else:
            fail(pos, f"not part of the header's C subset: '{text[pos:].splitlines()[0].strip()[:80]}'")
        pos = m.end()
    pos = len(text.rstrip())                                   # what is missing at the end is reported at the last line
    if guard and not closed:
        fail(pos, f"include guard {guard} is not closed")
    for s, f in sorted(host_left):
        fail(pos, f"HOST_ARRAY_FIELDS names {s}.{f}, which is no field of the header")
    if base is not None:
        own = lambda d, b: {k: v for k, v in d.items() if k not in b}
        return Header(own(constants, base[0].constants), own(structs, base[0].structs), own(functions, base[0].functions))
    return Header(constants, structs, functions)


def parse_base(text: str, header: Header):
    """What a header that includes `text` (already parsed into `header`) has to know of it: `header` and its scalar typedefs."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    scalars = dict(SCALARS)
    for m in _TYPEDEF.finditer(text):
        if m.group(1) in scalars:
            scalars[m.group(2)] = scalars[m.group(1)]
    return header, {k: v for k, v in scalars.items() if k not in SCALARS}


def load(path: str, base=None, host_array_fields=None) -> Header:
    try:
        with open(path) as f:
            if base is None:
                return parse(f.read())
            with open(base[0]) as b:
                return parse(f.read(), host_array_fields or (), parse_base(b.read(), base[1]))
    except (OSError, HeaderError) as exc:
        raise HeaderError(f"cannot derive the C-ABI bindings from {path}: {exc}") from exc
