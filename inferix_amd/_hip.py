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

# The 8-bit KV cache header (ifx_rmsnorm_rope_kv8_append, ifx_attn_fwd_kv8, ifx_attn_kv8_plan): a table of its own on the same terms,
# bound on first use (load_kv8).
KV8_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "inferix_hip_kv8.h")
_KV8_ABI = _cabi.load(KV8_HEADER_PATH, base=(HEADER_PATH, _ABI))
KV8_SIGNATURES = _KV8_ABI.functions
Kv8View = _KV8_ABI.structs["ifx_kv8_view"]
Kv8Plan = _KV8_ABI.structs["ifx_kv8_plan"]

# The 8-bit sessions header (ifx_attn_fwd_kv8_multi, ifx_rmsnorm_rope_kv8_append_multi, ifx_attn_kv8_multi_plan): a fourth table on
# the same terms, bound on first use (load_kv8_sessions).  Its item structs carry the cache pointers themselves, so it is read over
# the main header alone.
KV8_SESSIONS_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "inferix_hip_kv8_sessions.h")
_KV8_SESSIONS_ABI = _cabi.load(KV8_SESSIONS_HEADER_PATH, base=(HEADER_PATH, _ABI))
KV8_SESSIONS_SIGNATURES = _KV8_SESSIONS_ABI.functions
IFX_KV8_MULTI_MAX_ITEMS = _KV8_SESSIONS_ABI.constants["IFX_KV8_MULTI_MAX_ITEMS"]
IFX_KV8_MULTI_MAX_STREAMS = _KV8_SESSIONS_ABI.constants["IFX_KV8_MULTI_MAX_STREAMS"]
AttnKv8Item = _KV8_SESSIONS_ABI.structs["ifx_attn_kv8_item"]
Kv8AppendItem = _KV8_SESSIONS_ABI.structs["ifx_kv8_append_item"]
Kv8MultiPlan = _KV8_SESSIONS_ABI.structs["ifx_kv8_multi_plan"]

# The split-key header of the 8-bit cache (ifx_attn_fwd_kv8_split, ifx_attn_kv8_split_plan): a fifth table on the same terms, bound on
# first use (load_kv8_split); the view's fields are plain arguments, so it too is read over the main header alone.
KV8_SPLIT_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "inferix_hip_kv8_split.h")
_KV8_SPLIT_ABI = _cabi.load(KV8_SPLIT_HEADER_PATH, base=(HEADER_PATH, _ABI))
KV8_SPLIT_SIGNATURES = _KV8_SPLIT_ABI.functions
IFX_KV8_SPLIT_MAX = _KV8_SPLIT_ABI.constants["IFX_KV8_SPLIT_MAX"]
IFX_KV8_SPLIT_ROW_WORDS = _KV8_SPLIT_ABI.constants["IFX_KV8_SPLIT_ROW_WORDS"]
Kv8SplitPlan = _KV8_SPLIT_ABI.structs["ifx_kv8_split_plan"]

# The ring / grouped-scale header of the 8-bit cache (ifx_rmsnorm_rope_kv8_append_ring, ifx_attn_fwd_kv8_grouped,
# ifx_attn_kv8_grouped_plan): a sixth table on the same terms, bound on first use (load_kv8_ring); it has a view struct of its own.
KV8_RING_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "inferix_hip_kv8_ring.h")
_KV8_RING_ABI = _cabi.load(KV8_RING_HEADER_PATH, base=(HEADER_PATH, _ABI))
KV8_RING_SIGNATURES = _KV8_RING_ABI.functions
Kv8RingView = _KV8_RING_ABI.structs["ifx_kv8_ring_view"]
Kv8GroupedPlan = _KV8_RING_ABI.structs["ifx_kv8_grouped_plan"]

# The ring cache's sessions header (ifx_rmsnorm_rope_kv8_append_ring_multi, ifx_attn_fwd_kv8_grouped_multi,
# ifx_attn_kv8_grouped_multi_plan): a seventh table on the same terms, bound on first use (load_kv8_ring_sessions).  Its item structs
# carry the ring view's fields themselves, so it is read over the main header alone.
KV8_RING_SESSIONS_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "inferix_hip_kv8_ring_sessions.h")
_KV8_RING_SESSIONS_ABI = _cabi.load(KV8_RING_SESSIONS_HEADER_PATH, base=(HEADER_PATH, _ABI))
KV8_RING_SESSIONS_SIGNATURES = _KV8_RING_SESSIONS_ABI.functions
IFX_KV8_RING_MULTI_MAX_ITEMS = _KV8_RING_SESSIONS_ABI.constants["IFX_KV8_RING_MULTI_MAX_ITEMS"]
IFX_KV8_RING_MULTI_MAX_STREAMS = _KV8_RING_SESSIONS_ABI.constants["IFX_KV8_RING_MULTI_MAX_STREAMS"]
Kv8RingAppendItem = _KV8_RING_SESSIONS_ABI.structs["ifx_kv8_ring_append_item"]
AttnKv8GroupedItem = _KV8_RING_SESSIONS_ABI.structs["ifx_attn_kv8_grouped_item"]
Kv8GroupedMultiPlan = _KV8_RING_SESSIONS_ABI.structs["ifx_kv8_grouped_multi_plan"]

# The ring cache's split-key header (ifx_attn_fwd_kv8_grouped_split, ifx_attn_kv8_grouped_split_plan): an eighth table on the same terms,
# bound on first use (load_kv8_ring_split); the ring view's fields are plain arguments, so it is read over the main header alone.
KV8_RING_SPLIT_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "inferix_hip_kv8_ring_split.h")
_KV8_RING_SPLIT_ABI = _cabi.load(KV8_RING_SPLIT_HEADER_PATH, base=(HEADER_PATH, _ABI))
KV8_RING_SPLIT_SIGNATURES = _KV8_RING_SPLIT_ABI.functions
Kv8GroupedSplitPlan = _KV8_RING_SPLIT_ABI.structs["ifx_kv8_grouped_split_plan"]

# MAGI's 8-bit cache header (ifx_magi_head_prep_kv8, ifx_attn_fwd_kv8_ranges, ifx_attn_kv8_ranges_plan): a ninth table on the same terms,
# bound on first use (load_kv8_magi); the cache's fields are plain arguments, so it is read over the main header alone.
KV8_MAGI_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "inferix_hip_kv8_magi.h")
_KV8_MAGI_ABI = _cabi.load(KV8_MAGI_HEADER_PATH, base=(HEADER_PATH, _ABI))
KV8_MAGI_SIGNATURES = _KV8_MAGI_ABI.functions
IFX_KV8_RANGES_MAX = _KV8_MAGI_ABI.constants["IFX_KV8_RANGES_MAX"]
IFX_KV8_RANGES_MAX_STREAMS = _KV8_MAGI_ABI.constants["IFX_KV8_RANGES_MAX_STREAMS"]
MagiHeadPrepKv8Desc = _KV8_MAGI_ABI.structs["ifx_magi_head_prep_kv8_desc"]
Kv8RangesPlan = _KV8_MAGI_ABI.structs["ifx_kv8_ranges_plan"]

_lib: Optional[C.CDLL] = None
_kv8_magi_bound = False
_kv8_ring_split_bound = False
_kv8_ring_bound = False
_kv8_ring_sessions_bound = False
_sessions_bound = False
_kv8_bound = False
_kv8_sessions_bound = False
_kv8_split_bound = False


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


def load_kv8() -> C.CDLL:
    """`load()` with the functions of include/inferix_hip_kv8.h bound as well."""
    global _kv8_bound
    lib = load()
    if not _kv8_bound:
        for name, (res, args) in KV8_SIGNATURES.items():
            try:
                fn = getattr(lib, name)
            except AttributeError:
                raise HipLibraryMissing(f"{LIB_PATH} does not export {name} (include/inferix_hip_kv8.h): it was built before "
                                        "the 8-bit KV cache entry points existed; rebuild with __graft_entry__.build()") from None
            fn.restype = res
            fn.argtypes = args
        _kv8_bound = True
    return lib


def load_kv8_sessions() -> C.CDLL:
    """`load()` with the functions of include/inferix_hip_kv8_sessions.h bound as well."""
    global _kv8_sessions_bound
    lib = load()
    if not _kv8_sessions_bound:
        for name, (res, args) in KV8_SESSIONS_SIGNATURES.items():
            try:
                fn = getattr(lib, name)
            except AttributeError:
                raise HipLibraryMissing(f"{LIB_PATH} does not export {name} (include/inferix_hip_kv8_sessions.h): it was built before "
                                        "the 8-bit sessions entry points existed; rebuild with __graft_entry__.build()") from None
            fn.restype = res
            fn.argtypes = args
        _kv8_sessions_bound = True
    return lib


def load_kv8_split() -> C.CDLL:
    """`load()` with the functions of include/inferix_hip_kv8_split.h bound as well."""
    global _kv8_split_bound
    lib = load()
    if not _kv8_split_bound:
        for name, (res, args) in KV8_SPLIT_SIGNATURES.items():
            try:
                fn = getattr(lib, name)
            except AttributeError:
                raise HipLibraryMissing(f"{LIB_PATH} does not export {name} (include/inferix_hip_kv8_split.h): it was built before "
                                        "the split-key 8-bit attention existed; rebuild with __graft_entry__.build()") from None
            fn.restype = res
            fn.argtypes = args
        _kv8_split_bound = True
    return lib


def load_kv8_ring() -> C.CDLL:
    """`load()` with the functions of include/inferix_hip_kv8_ring.h bound as well."""
    global _kv8_ring_bound
    lib = load()
    if not _kv8_ring_bound:
        for name, (res, args) in KV8_RING_SIGNATURES.items():
            try:
                fn = getattr(lib, name)
            except AttributeError:
                raise HipLibraryMissing(f"{LIB_PATH} does not export {name} (include/inferix_hip_kv8_ring.h): it was built before "
                                        "the 8-bit ring cache existed; rebuild with __graft_entry__.build()") from None
            fn.restype = res
            fn.argtypes = args
        _kv8_ring_bound = True
    return lib


def load_kv8_ring_sessions() -> C.CDLL:
    """`load()` with the functions of include/inferix_hip_kv8_ring_sessions.h bound as well."""
    global _kv8_ring_sessions_bound
    lib = load()
    if not _kv8_ring_sessions_bound:
        for name, (res, args) in KV8_RING_SESSIONS_SIGNATURES.items():
            try:
                fn = getattr(lib, name)
            except AttributeError:
                raise HipLibraryMissing(f"{LIB_PATH} does not export {name} (include/inferix_hip_kv8_ring_sessions.h): it was built before "
                                        "the ring cache's multi-session launches existed; rebuild with __graft_entry__.build()") from None
            fn.restype = res
            fn.argtypes = args
        _kv8_ring_sessions_bound = True
    return lib


def load_kv8_ring_split() -> C.CDLL:
    """`load()` with the functions of include/inferix_hip_kv8_ring_split.h bound as well."""
    global _kv8_ring_split_bound
    lib = load()
    if not _kv8_ring_split_bound:
        for name, (res, args) in KV8_RING_SPLIT_SIGNATURES.items():
            try:
                fn = getattr(lib, name)
            except AttributeError:
                raise HipLibraryMissing(f"{LIB_PATH} does not export {name} (include/inferix_hip_kv8_ring_split.h): it was built before "
                                        "the ring cache's split-key attention existed; rebuild with __graft_entry__.build()") from None
            fn.restype = res
            fn.argtypes = args
        _kv8_ring_split_bound = True
    return lib


def load_kv8_magi() -> C.CDLL:
    """`load()` with the functions of include/inferix_hip_kv8_magi.h bound as well."""
    global _kv8_magi_bound
    lib = load()
    if not _kv8_magi_bound:
        for name, (res, args) in KV8_MAGI_SIGNATURES.items():
            try:
                fn = getattr(lib, name)
            except AttributeError:
                raise HipLibraryMissing(f"{LIB_PATH} does not export {name} (include/inferix_hip_kv8_magi.h): it was built before "
                                        "MAGI's 8-bit cache existed; rebuild with __graft_entry__.build()") from None
            fn.restype = res
            fn.argtypes = args
        _kv8_magi_bound = True
    return lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = load().ifx_last_error().decode("utf-8", "replace")
        raise HipKernelError(f"{what} failed (code {rc}): {msg}")


def version() -> str:
    v = load().ifx_version()
    return f"{v >> 16}.{(v >> 8) & 255}.{v & 255}"
