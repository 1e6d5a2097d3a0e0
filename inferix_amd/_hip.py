"""ctypes binding of libinferix_hip.so (C-ABI declared in include/inferix_hip.h).

The HIP library is the product: there is NO fallback.  Importing this module
without the built library, or calling an op on a non-GPU tensor, raises.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

# torch bundles its own libamdhip64: it MUST be in the process before libinferix_hip.so is dlopen'ed so
# that both share one HIP runtime (loading /opt/rocm's copy first leaves torch without a device).
import torch  # noqa: F401

from . import _cabi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("IFX_HIP_LIB", os.path.join(_HERE, "libinferix_hip.so"))   # override: kernel studies only


class HipLibraryMissing(RuntimeError):
    pass


class HipKernelError(RuntimeError):
    pass


# The header is the one statement of the C-ABI: the argument structs, SIGNATURES and every IFX_* constant below are read from it
# (inferix_amd/_cabi.py holds the reader and the type rules).  A missing or unparsable header raises here, with the path and the reason.
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "inferix_hip.h")
_ABI = _cabi.load(HEADER_PATH)
globals().update(_ABI.constants)                       # IFX_EPI_*, IFX_LN_*, IFX_Q_*, IFX_ACT_*, IFX_YUV420_*, IFX_MAX_PEERS, ...
ABI_MINOR = _ABI.constants["IFX_ABI_MINOR"]            # checked against the loaded library in load(): catches a stale .so
SIGNATURES = _ABI.functions                            # name -> (restype, argtypes); the complete export list of the header

KvView = _ABI.structs["ifx_kv_view"]
RopeGrid = _ABI.structs["ifx_rope_grid"]
Conv3dDesc = _ABI.structs["ifx_conv3d_desc"]
Epilogue = _ABI.structs["ifx_epilogue"]
MagiHeadPrepDesc = _ABI.structs["ifx_magi_head_prep_desc"]
MagiIntegrateSrc = _ABI.structs["ifx_magi_integrate_src"]
MagiIntegrateDesc = _ABI.structs["ifx_magi_integrate_desc"]
CfgUnipcStepDesc = _ABI.structs["ifx_cfg_unipc_step_desc"]
Yuv420Desc = _ABI.structs["ifx_yuv420_desc"]
PeerCaches = _ABI.structs["ifx_peer_caches"]
PeerFlags = _ABI.structs["ifx_peer_flags"]

# The sessions header (ifx_attn_fwd_multi) is a table of its own: it includes the main header, is not versioned by IFX_ABI_MINOR, and
# its symbols are bound on first use (load_sessions), so SIGNATURES / _ABI above stay the statement of inferix_hip.h alone.
SESSIONS_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "inferix_hip_sessions.h")
_SESSIONS_ABI = _cabi.load(SESSIONS_HEADER_PATH, base=(HEADER_PATH, _ABI))
SESSIONS_SIGNATURES = _SESSIONS_ABI.functions
IFX_ATTN_MULTI_MAX_ITEMS = _SESSIONS_ABI.constants["IFX_ATTN_MULTI_MAX_ITEMS"]
AttnItem = _SESSIONS_ABI.structs["ifx_attn_item"]

_lib: Optional[C.CDLL] = None
_sessions_bound = False


def load() -> C.CDLL:
    """dlopen the in-tree library (built by `__graft_entry__.build()` / `make -C inferix_amd/csrc`)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise HipLibraryMissing(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  inferix_amd has no CPU or eager fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)      # AttributeError if the .so does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    got = (lib.ifx_version() >> 8) & 255
    if got != ABI_MINOR:       # a stale .so next to newer bindings (or the reverse): the argument structs would not line up
        raise HipLibraryMissing(f"{LIB_PATH} has ABI minor {got}, these bindings are for {ABI_MINOR} (include/inferix_hip.h "
                                "IFX_ABI_MINOR): rebuild with __graft_entry__.build()")
    _lib = lib
    return lib


def load_sessions() -> C.CDLL:
    """`load()` with the functions of include/inferix_hip_sessions.h bound as well."""
    global _sessions_bound
    lib = load()
    if not _sessions_bound:
        for name, (res, args) in SESSIONS_SIGNATURES.items():
            try:
                fn = getattr(lib, name)
            except AttributeError:
                raise HipLibraryMissing(f"{LIB_PATH} does not export {name} (include/inferix_hip_sessions.h): it was built before "
                                        "the sessions entry points existed; rebuild with __graft_entry__.build()") from None
            fn.restype = res
            fn.argtypes = args
        _sessions_bound = True
    return lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = load().ifx_last_error().decode("utf-8", "replace")
        raise HipKernelError(f"{what} failed (code {rc}): {msg}")


def version() -> str:
    v = load().ifx_version()
    return f"{v >> 16}.{(v >> 8) & 255}.{v & 255}"
