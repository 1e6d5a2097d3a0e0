"""CPU tests of the header-derived ctypes bindings (inferix_amd/_cabi.py read by inferix_amd/_hip.py): against the hand-written
table of ABI minor 7 recorded in tests/golden/cabi_table_abi7.json, against the C compiler's sizeof / offsetof, the reader's grammar
and refusals, and the objects the callers pass in the pointer slots that became c_void_p."""
import ctypes as C
import json
import os
import shutil
import subprocess

import pytest

from inferix_amd import _cabi, _hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "inferix_hip.h")
I32, I64, VP = C.c_int32, C.c_int64, C.c_void_p

# the pointer parameters that the hand table typed POINTER(scalar) or c_char_p and the rule types c_void_p
RELAXED_SLOTS = {("ifx_get_option", 1), ("ifx_attn_split_plan", 4), ("ifx_rmsnorm_cl", 4), ("ifx_peer_alloc", 2), ("ifx_peer_export", 1),
                 ("ifx_peer_export", 2), ("ifx_peer_open", 0), ("ifx_peer_open", 1), ("ifx_attn_fwd_partial", 12),
                 ("ifx_attn_fwd_ranges", 8), ("ifx_attn_fwd_ranges", 9)}


def tname(t):
    """The spelling the golden file was recorded with."""
    if t is None:
        return "None"
    if issubclass(t, C.Structure):
        return t.__name__
    if issubclass(t, C.Array):
        return f"{tname(t._type_)}*{t._length_}"
    if issubclass(t, C._Pointer):
        return f"POINTER({tname(t._type_)})"
    return t.__name__


def loose(name, struct_classes):
    """Non-struct pointers (c_void_p, c_char_p, POINTER(scalar)), also as array elements, are one token."""
    elem, star, n = name.partition("*")
    if elem in ("c_void_p", "c_char_p") or (elem.startswith("POINTER(") and elem[8:-1] not in struct_classes):
        elem = "pointer"
    return elem + star + n


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(ROOT, "tests", "golden", "cabi_table_abi7.json")) as f:
        return json.load(f)


def test_derived_table_equals_the_recorded_hand_table(recorded):
    classes = {s["class"] for s in recorded["structs"].values()}
    assert set(_hip.SIGNATURES) == set(recorded["functions"]) and len(_hip.SIGNATURES) == 69
    exact_differences = set()
    for name, want in recorded["functions"].items():
        res, args = _hip.SIGNATURES[name]
        got = [tname(a) for a in args]
        assert tname(res) == want["restype"], name
        assert [loose(a, classes) for a in got] == [loose(a, classes) for a in want["argtypes"]], name
        exact_differences |= {(name, i) for i, (a, b) in enumerate(zip(got, want["argtypes"])) if a != b}
    assert exact_differences == RELAXED_SLOTS                 # the relaxation is used where it was stated and nowhere else
    assert all(tname(_hip.SIGNATURES[n][1][i]) == "c_void_p" for n, i in RELAXED_SLOTS)

    assert set(_hip._ABI.structs) == set(recorded["structs"]) and len(recorded["structs"]) == 11
    n_fields = 0
    for cname, want in recorded["structs"].items():
        cls = _hip._ABI.structs[cname]
        assert cls.__name__ == want["class"] and getattr(_hip, want["class"]) is cls and cls.__doc__ == cname
        assert C.sizeof(cls) == want["sizeof"], cname
        assert len(cls._fields_) == len(want["fields"]), cname
        for (field, ct), (wfield, wtype, woffset) in zip(cls._fields_, want["fields"]):
            assert field == ("in_" if (cname, wfield) == ("ifx_magi_head_prep_desc", "inp") else wfield), (cname, wfield)
            assert getattr(cls, field).offset == woffset, (cname, field)
            assert loose(tname(ct), classes) == loose(wtype, classes), (cname, field)
            if (cname, wfield) not in _cabi.HOST_ARRAY_FIELDS:
                assert tname(ct) == wtype, (cname, field)     # fields had no POINTER(scalar) or c_char_p beside the two host arrays
            n_fields += 1
    assert n_fields == 132

    assert recorded["abi_minor"] == _hip.ABI_MINOR == 7
    assert len(recorded["constants"]) == 18
    for k, v in recorded["constants"].items():
        assert getattr(_hip, k) == v and type(getattr(_hip, k)) is int, k


def test_char_pointers_and_host_arrays_keep_their_exact_types():
    S = _hip.SIGNATURES
    assert S["ifx_set_option"][1][0] is C.c_char_p and S["ifx_get_option"][1][0] is C.c_char_p
    assert S["ifx_last_error"] == (C.c_char_p, []) and S["ifx_arch"] == (C.c_char_p, [])
    fields = dict(_hip.Conv3dDesc._fields_)
    assert fields["in_slots"] is C.POINTER(I32) and fields["out_slots"] is C.POINTER(I32)
    slots = (I32 * 3)(2, 0, 1)
    d = _hip.Conv3dDesc(in_slots=slots)                       # a POINTER field holds on to the array it was given
    del slots
    assert d._objects and list(d.in_slots[:3]) == [2, 0, 1]
    assert _hip.load().ifx_arch() == b"gfx950"                # bytes, not an address


def test_struct_layouts_equal_the_compilers(tmp_path):
    """sizeof and every offsetof of all argument structs, as the C compiler lays the header out."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not present")
    with open(HEADER) as f:
        abi = _cabi.parse(f.read())
    c_name = lambda field: field[:-1] if field.endswith("_") else field
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "inferix_hip.h"', "int main(void) {"]
    for cname, cls in abi.structs.items():
        lines.append(f'  printf("{cname} %zu\\n", sizeof({cname}));')
        lines += [f'  printf("{cname}.{f} %zu\\n", offsetof({cname}, {c_name(f)}));' for f, _ in cls._fields_]
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    b = subprocess.run([hipcc, "-x", "c", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stderr[-3000:]
    compiled = {k: int(v) for k, v in (line.split() for line in p.stdout.splitlines())}
    derived = {}
    for cname, cls in abi.structs.items():
        derived[cname] = C.sizeof(cls)
        derived.update({f"{cname}.{f}": getattr(cls, f).offset for f, _ in cls._fields_})
    assert len(abi.structs) == 11 and len(derived) == 11 + 132
    assert derived == compiled, {k: (derived.get(k), compiled.get(k)) for k in set(derived) | set(compiled) if derived.get(k) != compiled.get(k)}


def test_reader_accepts_every_construct_of_the_header():
    abi = _cabi.parse('''/* a block
comment */
#ifndef T_H
#define T_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define IFX_A 3          // a line comment
#define IFX_NEG (-2)
#define IFX_N 4
enum { IFX_X = 0, IFX_Y = 1,
       IFX_Z = 7 };
typedef uint16_t ifx_bf16;
typedef struct {
  ifx_bf16* p;             /* device */
  const int32_t* table;
  int32_t a, b;
  float f;
  int64_t big;
  uint8_t byte;
  const float *u, *v;
  int in;
} ifx_first;
typedef struct ifx_second {
  int32_t m[9];
  float w[IFX_N];
  ifx_bf16* k[IFX_N];
  ifx_first parts[2];
  const int32_t* slots;
  ifx_bf16 half;
} ifx_second;
int ifx_version(void);
const char* ifx_name(void);
int64_t ifx_bytes(int32_t M, int32_t);
int ifx_call(const ifx_bf16* x, void** out, const ifx_second* desc, const char* key, uint8_t* h,
             const double* freqs,
             float scale, void* stream);
#ifdef __cplusplus
}
#endif
#endif /* T_H */
''', host_array_fields={("ifx_second", "slots")})
    assert abi.constants == {"IFX_A": 3, "IFX_NEG": -2, "IFX_N": 4, "IFX_X": 0, "IFX_Y": 1, "IFX_Z": 7}
    First, Second = abi.structs["ifx_first"], abi.structs["ifx_second"]
    assert (First.__name__, Second.__name__, Second.__doc__) == ("First", "Second", "ifx_second")
    assert First._fields_ == [("p", VP), ("table", VP), ("a", I32), ("b", I32), ("f", C.c_float), ("big", I64), ("byte", C.c_uint8),
                              ("u", VP), ("v", VP), ("in_", C.c_int)]
    assert Second._fields_ == [("m", I32 * 9), ("w", C.c_float * 4), ("k", VP * 4), ("parts", First * 2), ("slots", C.POINTER(I32)),
                               ("half", C.c_uint16)]
    assert abi.functions == {"ifx_version": (C.c_int, []), "ifx_name": (C.c_char_p, []), "ifx_bytes": (I64, [I32, I32]),
                             "ifx_call": (C.c_int, [VP, VP, C.POINTER(Second), C.c_char_p, VP, VP, C.c_float, VP])}
    empty = _cabi.parse("// nothing declared\n", host_array_fields=())
    assert empty == ({}, {}, {})


T = "typedef struct {\n  int32_t a;\n%s\n} ifx_t;\n"


@pytest.mark.parametrize("text, line, word", [
    ("int ifx_f(void);\nint ifx_g(size_t n);\n", 2, "size_t"),                                  # unknown type, parameter
    (T % "  unsigned b;", 3, "unsigned"),                                                       # unknown type, field
    (T % "  struct other s;", 3, "other s"),
    ("typedef long ifx_l;\n", 1, "long"),
    ("\n\ntypedef union { int32_t a; float b; } ifx_u;\n", 3, "union"),
    (T % "  union { int32_t b; float c; } u;", 1, "struct"),                                    # nested anonymous aggregate
    (T % "  int32_t b : 3;", 3, "bit-field"),
    (T % "  void (*callback)(int32_t);", 3, "function pointer"),
    ("int ifx_f(void (*callback)(int32_t));\n", 1, "ifx_f"),
    ("int ifx_f(void);\nint ifx_log(const char* fmt,\n            ...);\n", 2, "variadic"),
    ("int ifx_f(void);\nstray words\nint ifx_g(void);\n", 2, "stray words"),                    # text between declarations
    ("int ifx_f(void) { return 0; }\n", 1, "ifx_f"),
    ("int ifx_f(void);\n#if defined(IFX_EXTRA)\nint ifx_g(void);\n#endif\n", 2, "#if"),
    ("#ifdef IFX_EXTRA\nint ifx_g(void);\n#endif\n", 1, "#ifdef"),
    ("#define IFX_F 1.5\n", 1, "IFX_F"),
    ("#define IFX_SQ(x) ((x) * (x))\n", 1, "IFX_SQ"),
    ("enum { IFX_A, IFX_B };\n", 1, "IFX_A"),
    (T % "  float w[IFX_UNKNOWN];", 3, "IFX_UNKNOWN"),
    ("int ifx_f();\n", 1, "ifx_f"),
    ("void ifx_f(void);\n", 1, "void"),
    ("int ifx_f(void);\n/* open comment\nint ifx_g(void);\n", 2, "/*"),
    ("#ifndef T_H\n#define T_H\nint ifx_f(void);\n#endif\nint ifx_g(void);\n", 5, "#endif"),
    ("#ifndef T_H\n#define T_H\nint ifx_f(void);\n", 3, "guard"),
    ("int ifx_f(void);\nint ifx_f(void);\n", 2, "twice"),
])
def test_reader_refuses_what_it_does_not_understand(text, line, word):
    with pytest.raises(_cabi.HeaderError) as e:
        _cabi.parse(text, host_array_fields=())
    assert str(e.value).startswith(f"line {line}: ") and word in str(e.value), str(e.value)


@pytest.mark.parametrize("entry, line", [(("ifx_t", "missing"), 6),       # no such field: the last line of the header
                                         (("ifx_t", "a"), 3),             # a field, but no pointer
                                         (("ifx_t", "s"), 4),             # a pointer to a struct, not to a scalar
                                         (("ifx_other", "p"), 6)])        # no such struct: the last line of the header
def test_reader_checks_the_host_array_fields(entry, line):
    text = "typedef struct { int32_t x; } ifx_t0;\n" + T % "  const ifx_t0* s;\n  const int32_t* p;"
    assert dict(_cabi.parse(text, host_array_fields={("ifx_t", "p")}).structs["ifx_t"]._fields_)["p"] is C.POINTER(I32)
    with pytest.raises(_cabi.HeaderError) as e:
        _cabi.parse(text, host_array_fields={entry})
    assert str(e.value).startswith(f"line {line}: ") and "HOST_ARRAY_FIELDS" in str(e.value) and ".".join(entry) in str(e.value)


def test_missing_or_broken_header_raises_with_the_path(tmp_path):
    missing = str(tmp_path / "none.h")
    with pytest.raises(_cabi.HeaderError, match="none.h"):
        _cabi.load(missing)
    bad = tmp_path / "bad.h"
    bad.write_text("int ifx_f(void);\nint ifx_g(long n);\n")
    with pytest.raises(_cabi.HeaderError) as e:
        _cabi.load(str(bad))
    assert str(bad) in str(e.value) and "line 2: unknown type name 'long'" in str(e.value)
    assert _hip.HEADER_PATH == HEADER and set(_cabi.load(HEADER).functions) == set(_hip.SIGNATURES)


def test_relaxed_pointer_slots_accept_what_the_callers_pass():
    """Each kind of object that hip_ops and the tests hand to the slots that became c_void_p: converted by the derived argtypes, and
    taken by the library in the calls that need no GPU."""
    S, lib = _hip.SIGNATURES, _hip.load()
    kinds = [C.byref(I32(1)), C.byref(I64(1)), C.byref(VP()), (I32 * 4)(), (I64 * 4)(), C.create_string_buffer(64), b"\0" * 64, None,
             C.addressof(I64(0))]
    for name, i in sorted(RELAXED_SLOTS):
        for obj in kinds:
            S[name][1][i].from_param(obj)                    # what a call runs on the argument; raises ArgumentError / TypeError if refused

    lib.ifx_set_option(b"gemm_variant", 3)
    try:
        v, arr, buf = I32(-1), (I32 * 1)(-1), C.create_string_buffer(4)
        assert lib.ifx_get_option(b"gemm_variant", C.byref(v)) == 0 and v.value == 3
        assert lib.ifx_get_option(b"gemm_variant", arr) == 0 and arr[0] == 3
        assert lib.ifx_get_option(b"gemm_variant", buf) == 0 and int.from_bytes(buf.raw, "little") == 3
        assert lib.ifx_get_option(b"gemm_variant", C.addressof(v)) == 0
        assert lib.ifx_get_option(b"gemm_variant", None) == -1 and b"null argument" in lib.ifx_last_error()
    finally:
        lib.ifx_set_option(b"gemm_variant", 0)

    need, need_arr = I64(-1), (I64 * 1)(-1)
    splits = lib.ifx_attn_split_plan(585, 12, 0, 18720, C.byref(need))
    assert splits >= 1 and need.value >= 0
    assert lib.ifx_attn_split_plan(585, 12, 0, 18720, need_arr) == splits and need_arr[0] == need.value
    assert lib.ifx_attn_split_plan(585, 12, 0, 18720, C.addressof(need_arr)) == splits
    assert lib.ifx_attn_split_plan(585, 12, 0, 18720, None) == splits

    # refusals before any launch or device call, with the relaxed slots filled the way the callers fill them
    slots, used, ranges = (I32 * 2)(0, 1), I32(0), (I32 * 2)(0, 8)
    kv = _hip.KvView(8, 8, None, 1, 100, 12, 128)
    assert lib.ifx_rmsnorm_cl(None, VP(8), VP(8), 64, slots, 2, 4, 8, 0, None) == -1 and b"ifx_rmsnorm_cl: null" in lib.ifx_last_error()
    assert lib.ifx_attn_fwd_partial(None, C.byref(kv), 4, 12, 0, 10, 0.0, 1, VP(8), 1 << 20, 0, 1, C.byref(used), None) == -1
    assert b"ifx_attn_fwd_partial: null" in lib.ifx_last_error()
    assert lib.ifx_attn_fwd_ranges(None, 0, VP(8), 0, C.byref(kv), 8, 12, 1, ranges, ranges, 0.0, None) == -1
    assert b"ifx_attn_fwd_ranges: null" in lib.ifx_last_error()
    assert lib.ifx_peer_alloc(0, 0, C.byref(VP())) == -1 and b"ifx_peer_alloc" in lib.ifx_last_error()
    assert lib.ifx_peer_export(None, C.create_string_buffer(_hip.IFX_PEER_HANDLE_BYTES), C.byref(I64())) == -1
    assert b"ifx_peer_export: null" in lib.ifx_last_error()
    assert lib.ifx_peer_open(b"\0" * _hip.IFX_PEER_HANDLE_BYTES, None) == -1 and b"ifx_peer_open: null" in lib.ifx_last_error()
    assert lib.ifx_peer_open(C.create_string_buffer(_hip.IFX_PEER_HANDLE_BYTES), None) == -1
