"""The 8-bit KV cache entry points without a GPU: the launch plan's arithmetic, the third header's derived bindings against the C
compiler, and the argument refusals that are decided on the host."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

from inferix_amd import _hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RING, SLOT = 3, 64 * 128 + 128 * 64 + 32 * 16


@pytest.mark.parametrize("rows", [1, 33, 256, 300, 4680])
@pytest.mark.parametrize("heads", [2, 4, 12])
@pytest.mark.parametrize("k0,k1", [(0, 1), (0, 63), (0, 64), (0, 65), (0, 200), (70, 270), (0, 64 * (RING + 2) + 5), (0, 32760)])
def test_plan(rows, heads, k0, k1):
    from inferix_amd import hip_ops as ops
    p = ops.attention_kv8_plan(rows, heads, k0, k1)
    tiles = -(-rows // 256)
    assert p["row_tiles"] == tiles and p["key_tiles"] == -(-(k1 - k0) // 64) and p["per_xcd"] == -(-tiles * heads // 8) and p["grid"] == 8 * p["per_xcd"]
    assert p["ring"] == RING and p["lds_bytes"] == RING * SLOT <= 160 * 1024
    # workgroup b runs item (b & 7) * per_xcd + (b >> 3): every item exactly once
    items = sorted(i for b in range(p["grid"]) if (i := (b & 7) * p["per_xcd"] + (b >> 3)) < tiles * heads)
    assert items == list(range(tiles * heads))


def test_refusals():
    lib, plan = _hip.load_kv8(), _hip.Kv8Plan()
    for bad in [(0, 2, 0, 8), (8, 0, 0, 8), (8, 2, -1, 8), (8, 2, 8, 8)]:
        assert lib.ifx_attn_kv8_plan(*bad, C.byref(plan)) == _hip.IFX_EINVAL
    # q_rows = 0: the entry point checks everything, then returns IFX_OK WITHOUT a launch, so the made-up addresses are never used
    view = _hip.Kv8View(4096, 8192, 12288, 64, 2, 128)
    call = lambda v, q=4096, ldq=0, out=4096, ldo=0, heads=2, k0=0, k1=64: lib.ifx_attn_fwd_kv8(q, ldq, out, ldo, None, C.byref(v), 0, heads, k0, k1, None)
    assert call(view) == _hip.IFX_OK
    assert call(view, heads=3) == _hip.IFX_EINVAL and b"no multiple of kv_heads" in lib.ifx_last_error()
    assert call(view, k1=65) == _hip.IFX_EINVAL and call(view, k0=64) == _hip.IFX_EINVAL and call(view, ldq=200) == _hip.IFX_EINVAL and call(view, ldq=264) == _hip.IFX_EINVAL and call(view, q=4100) == _hip.IFX_EINVAL
    assert call(view, ldo=260) == _hip.IFX_EINVAL and call(view, out=0) == _hip.IFX_EINVAL
    assert call(_hip.Kv8View(4096, 8192, 12288, 64, 2, 64)) == _hip.IFX_EUNSUP
    assert call(_hip.Kv8View(4096, 8192, 12288, 1 << 23, 2, 128)) == _hip.IFX_EUNSUP and b"2 GiB" in lib.ifx_last_error()


def test_kv8_struct_layout_equals_the_compilers(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not present")
    abi = _hip._KV8_ABI                 # the header as _cabi read it: a table of its own, the versioned one untouched
    assert set(abi.functions) == {"ifx_rmsnorm_rope_kv8_append", "ifx_attn_fwd_kv8", "ifx_attn_kv8_plan"} and not set(abi.functions) & set(_hip.SIGNATURES)
    assert abi.functions["ifx_rmsnorm_rope_kv8_append"][1][5] is C.POINTER(_hip.RopeGrid) and abi.constants == {}
    structs = {"ifx_kv8_view": _hip.Kv8View, "ifx_kv8_plan": _hip.Kv8Plan}
    lines, derived = ['#include <stddef.h>', '#include <stdio.h>', '#include "inferix_hip_kv8.h"', "int main(void) {"], {}
    for name, cls in structs.items():
        lines.append(f'  printf("{name} %zu\\n", sizeof({name}));')
        derived[name] = C.sizeof(cls)
        for f, _ in cls._fields_:
            lines.append(f'  printf("{name}.{f} %zu\\n", offsetof({name}, {f}));')
            derived[f"{name}.{f}"] = getattr(cls, f).offset
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines + ["  return 0;", "}"]) + "\n")
    b = subprocess.run([hipcc, "-x", "c", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    compiled = {k: int(v) for k, v in (line.split() for line in p.stdout.splitlines())}
    assert len(derived) == 14 and derived == compiled
