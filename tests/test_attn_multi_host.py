"""ifx_attn_fwd_multi without a GPU: the launch plan as a stand-alone program, the argument refusals of the entry point, the second
header's derived bindings against the C compiler — and the main header's table untouched by all of it."""
import ctypes as C
import json
import os
import shutil
import subprocess

import pytest

from inferix_amd import _cabi, _hip

import attn_multi_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SESSIONS_HEADER = os.path.join(ROOT, "include", "inferix_hip_sessions.h")


def _hipcc():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not present")
    return hipcc


def test_plan_program(tmp_path):
    """tools/attn_multi_plan_check.cpp: every item's arguments are its single launch's, longest key range first, one form per launch,
    the refusals — checked inside the program; here: it builds, exits 0 and planned the session shape as documented."""
    exe = str(tmp_path / "attn_multi_plan_check")
    b = subprocess.run([_hipcc(), "--offload-arch=gfx950", "-O1", "-std=c++17", os.path.join(ROOT, "tools", "attn_multi_plan_check.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-1000:]
    lines = p.stdout.splitlines()
    assert lines[-1] == "attn_multi_plan_check: ok"
    assert lines[0].split() == "4 sessions, 480p variant 0 mfma 0: schedule 7 pre 16x16x32 page kind 0, order 2310, 76 tiles x 12 heads".split()
    assert sum("refused" in ln for ln in lines) == 13


def test_argument_refusals():
    """Return code and message of everything the entry point refuses; decided on the host, nothing is launched."""
    from inferix_amd import hip_ops as ops
    before = ops.get_option("attn_variant")
    try:
        U.check_refusals(_hip, lambda v: ops.set_option("attn_variant", v))
    finally:
        ops.set_option("attn_variant", before)


def test_main_header_table_is_untouched():
    """The sessions header adds nothing to the table IFX_ABI_MINOR versions: 69 functions, 11 structs, 18 constants, minor 7."""
    with open(os.path.join(ROOT, "tests", "golden", "cabi_table_abi7.json")) as f:
        recorded = json.load(f)
    assert set(_hip.SIGNATURES) == set(recorded["functions"]) and len(_hip.SIGNATURES) == 69
    assert set(_hip._ABI.structs) == set(recorded["structs"]) and len(_hip._ABI.structs) == 11
    assert sum(len(c._fields_) for c in _hip._ABI.structs.values()) == 132
    assert _hip.ABI_MINOR == recorded["abi_minor"] == 7
    assert all(_hip._ABI.constants[k] == v for k, v in recorded["constants"].items()) and len(recorded["constants"]) == 18
    assert "ifx_attn_fwd_multi" not in _hip.SIGNATURES and "ifx_attn_item" not in _hip._ABI.structs
    assert (_hip.load().ifx_version() >> 8) & 255 == 7


def test_sessions_table_is_derived_from_its_header():
    abi = _hip._SESSIONS_ABI
    assert set(abi.functions) == {"ifx_attn_fwd_multi"} and set(abi.structs) == {"ifx_attn_item"}
    assert abi.constants == {"IFX_ATTN_MULTI_MAX_ITEMS": 8}
    res, args = abi.functions["ifx_attn_fwd_multi"]
    assert res is C.c_int and args == [C.POINTER(_hip.AttnItem), C.c_int32, C.c_int32, C.c_float, C.c_void_p]
    fields = dict(_hip.AttnItem._fields_)
    assert fields["kv"] is C.POINTER(_hip.KvView)               # the main header's struct, not a second class of the same layout
    assert [f for f, _ in _hip.AttnItem._fields_] == ["q", "ldq", "out", "ldo", "kv", "q_rows", "kv_start", "kv_len"]
    # the reader over a base: the base's names are known, cannot be redeclared, and an #include "..." needs a base
    with open(SESSIONS_HEADER) as f:
        text = f.read()
    with pytest.raises(_cabi.HeaderError, match="not part of the header's C subset"):
        _cabi.parse(text, ())
    with open(_hip.HEADER_PATH) as f:
        base = _cabi.parse_base(f.read(), _hip._ABI)
    with pytest.raises(_cabi.HeaderError, match="'ifx_kv_view' is declared twice"):
        _cabi.parse(text.replace("} ifx_attn_item;", "} ifx_kv_view;"), (), base)
    with pytest.raises(_cabi.HeaderError, match="unknown type name 'ifx_kv_vue'"):
        _cabi.parse(text.replace("const ifx_kv_view* kv;", "const ifx_kv_vue* kv;"), (), base)


def test_sessions_struct_layout_equals_the_compilers(tmp_path):
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "inferix_hip_sessions.h"', "int main(void) {",
             '  printf("ifx_attn_item %zu\\n", sizeof(ifx_attn_item));']
    lines += [f'  printf("ifx_attn_item.{f} %zu\\n", offsetof(ifx_attn_item, {f}));' for f, _ in _hip.AttnItem._fields_]
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    b = subprocess.run([_hipcc(), "-x", "c", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    compiled = {k: int(v) for k, v in (line.split() for line in p.stdout.splitlines())}
    derived = {"ifx_attn_item": C.sizeof(_hip.AttnItem)}
    derived.update({f"ifx_attn_item.{f}": getattr(_hip.AttnItem, f).offset for f, _ in _hip.AttnItem._fields_})
    assert len(derived) == 9 and derived == compiled


def test_library_without_the_symbol_names_the_rebuild(monkeypatch):
    """A library built before the sessions entry points existed: HipLibraryMissing with the rebuild, not an AttributeError."""
    class Old:
        def __getattr__(self, name):
            raise AttributeError(name)
    monkeypatch.setattr(_hip, "_sessions_bound", False)
    monkeypatch.setattr(_hip, "load", lambda: Old())
    with pytest.raises(_hip.HipLibraryMissing, match=r"does not export ifx_attn_fwd_multi .*rebuild with __graft_entry__.build\(\)"):
        _hip.load_sessions()
