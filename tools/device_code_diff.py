#!/usr/bin/env python3
"""Is the compiled DEVICE code of a .hip file the same as at another commit?  The check behind a refactor of kernel sources.

usage: tools/device_code_diff.py REV FILE.hip [FILE.hip ...]        (paths relative to the repository root; needs no GPU)

Each file is compiled twice with the flags of inferix_amd/csrc/Makefile plus `--offload-device-only --no-gpu-bundle-output` (a plain code object): as of REV (`git archive` of
inferix_amd/csrc and include into a temporary directory) and as it stands in the working tree.  For every kernel the machine-code
bytes of its function symbol and its 64-byte kernel descriptor (`<kernel>.kd`: LDS and scratch bytes, VGPR / SGPR allocation, kernarg
size, enable bits; the code-entry offset is left out, it only says where the linker put the function) are compared BY SYMBOL, so the
order in which templates get instantiated does not matter.  Prints the kernels added, removed and changed per file and exits 1 if
there are any, 0 when the device code is identical.

What is NOT compared: anything without a kernel descriptor — a device function the compiler did not inline, and constants a kernel
reads from .rodata.  A change there shows only if it moves an instruction of a kernel."""
import concurrent.futures
import os
import re
import struct
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")
CSRC = "inferix_amd/csrc"


def run(*cmd, **kw):
    return subprocess.run(cmd, check=True, stdout=subprocess.PIPE, **kw).stdout


def makefile_flags():
    mk = open(os.path.join(ROOT, CSRC, "Makefile")).read()
    var = lambda name: re.search(rf"^{name}\s*[:?]?=\s*(.*)$", mk, re.M).group(1).strip()
    return var("HIPCC"), var("CXXFLAGS").replace("$(ARCH)", var("ARCH")).split()


def compile_device(hipcc, flags, tree, rel, out):
    cmd = [hipcc, *flags, "--offload-device-only", "--no-gpu-bundle-output", "-c", os.path.join(tree, rel), "-o", out]
    done = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    if done.returncode != 0:
        raise SystemExit(f"{' '.join(cmd)}\nfailed with status {done.returncode}:\n{done.stdout.decode(errors='replace')}")
    return out


def kernels(obj, tmp):
    """kernel symbol -> (machine-code bytes, descriptor bytes without the entry offset)"""
    sections = {}           # name -> (address, bytes)
    for m in re.finditer(r"^\s*\[\s*\d+\]\s+(\.\S+)\s+\S+\s+([0-9a-f]+)\s+[0-9a-f]+\s+([0-9a-f]+)", run(f"{LLVM}/llvm-readelf", "-S", "-W", obj).decode(), re.M):
        if m.group(1) in (".text", ".rodata"):
            dump = os.path.join(tmp, os.path.basename(obj) + m.group(1))
            run(f"{LLVM}/llvm-objcopy", f"--dump-section={m.group(1)}={dump}", obj, os.path.join(tmp, "unused.o"))
            sections[m.group(1)] = (int(m.group(2), 16), open(dump, "rb").read())
    syms = {}               # name -> (value, size)
    for line in run(f"{LLVM}/llvm-readelf", "-s", "-W", obj).decode().splitlines():
        f = line.split()
        if len(f) == 8 and f[3] in ("FUNC", "OBJECT") and f[6] != "UND":
            syms[f[7]] = (int(f[1], 16), int(f[2], 0))

    def body(section, name):
        base, data = sections[section]
        value, size = syms[name]
        assert base <= value and value - base + size <= len(data), (name, section)
        return data[value - base:value - base + size]
    out = {}
    for name in syms:
        if name.endswith(".kd") and name[:-3] in syms:
            kd = body(".rodata", name)
            assert len(kd) == 64, (name, len(kd))
            out[name[:-3]] = (body(".text", name[:-3]), kd[:16] + kd[24:])
    return out


def describe(kd):
    """the descriptor fields a person asks about first (kd: the 56 bytes kept by kernels())"""
    lds, scratch, kernarg = struct.unpack_from("<III", kd, 0)
    rsrc3, rsrc1 = struct.unpack_from("<II", kd, 36)
    return {"lds_bytes": lds, "scratch_bytes": scratch, "kernarg_bytes": kernarg, "vgpr_alloc": ((rsrc1 & 63) + 1) * 8,
            "sgpr_alloc": (((rsrc1 >> 6) & 15) + 1) * 8, "accum_offset": ((rsrc3 & 63) + 1) * 4}


def main():
    if len(sys.argv) < 3:
        raise SystemExit(__doc__)
    rev, files = sys.argv[1], sys.argv[2:]
    hipcc, flags = makefile_flags()
    differences = 0
    with tempfile.TemporaryDirectory() as tmp:
        old_tree = os.path.join(tmp, "rev")
        os.makedirs(old_tree)
        tar = subprocess.Popen(["git", "-C", ROOT, "archive", rev, CSRC, "include"], stdout=subprocess.PIPE)
        subprocess.run(["tar", "-x", "-C", old_tree], stdin=tar.stdout, check=True)
        if tar.wait() != 0:
            raise SystemExit(f"git archive {rev} failed")
        with concurrent.futures.ThreadPoolExecutor(max_workers=min(8, 2 * len(files))) as pool:
            jobs = {(rel, side): pool.submit(compile_device, hipcc, flags, tree, rel, os.path.join(tmp, f"{i}_{side}.co"))
                    for i, rel in enumerate(files) for side, tree in (("old", old_tree), ("new", ROOT))}
            objs = {k: j.result() for k, j in jobs.items()}

        def names(syms):                 # demangled where a demangler is installed
            for tool in (f"{LLVM}/llvm-cxxfilt", "c++filt"):
                try:
                    return run(tool, *syms).decode().splitlines() if syms else []
                except (OSError, subprocess.CalledProcessError):
                    pass
            return list(syms)
        for rel in files:
            old, new = kernels(objs[rel, "old"], tmp), kernels(objs[rel, "new"], tmp)
            added, removed = sorted(set(new) - set(old)), sorted(set(old) - set(new))
            changed = sorted(k for k in set(old) & set(new) if old[k] != new[k])
            print(f"{rel}: {len(old)} kernels at {rev}, {len(new)} in the working tree: {len(added)} added, {len(removed)} removed, {len(changed)} changed")
            for what, syms in (("added", added), ("removed", removed)):
                for sym, name in zip(syms, names(syms)):
                    print(f"  {what}: {name}   [{sym}]")
            for sym, name in zip(changed, names(changed)):
                (code0, kd0), (code1, kd1) = old[sym], new[sym]
                parts = []
                if code0 != code1:
                    first = next((i for i, (a, b) in enumerate(zip(code0, code1)) if a != b), min(len(code0), len(code1)))
                    parts.append(f"code {len(code0)} -> {len(code1)} bytes, first difference at byte {first}")
                if kd0 != kd1:
                    d0, d1 = describe(kd0), describe(kd1)
                    fields = [f"{k} {d0[k]} -> {d1[k]}" for k in d0 if d0[k] != d1[k]] or ["other descriptor bits"]
                    parts.append("descriptor: " + ", ".join(fields))
                print(f"  changed: {name}   [{sym}]: " + "; ".join(parts))
            differences += len(added) + len(removed) + len(changed)
    print("device code identical" if differences == 0 else f"{differences} kernel symbols differ")
    return 1 if differences else 0


if __name__ == "__main__":
    sys.exit(main())
