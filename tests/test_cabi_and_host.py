"""CPU tests: the C-ABI library loads and exports every declared symbol; host-side mirrors (KV-cache manager,
scheduler, index arithmetic, pipeline control flow) against the reference-generated golden vectors."""
import os
import re
from types import SimpleNamespace

import pytest
import torch

import wan_oracle as O
from fixture_io import golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF = torch.bfloat16


def test_cabi_library_loads_and_exports_all_declared_symbols():
    from inferix_amd import _hip
    lib = _hip.load()                      # raises if the .so is missing: there is no fallback
    hdr = open(os.path.join(ROOT, "include", "inferix_hip.h")).read()
    declared = set(re.findall(r"\b(ifx_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(_hip.SIGNATURES), (declared ^ set(_hip.SIGNATURES))
    for name in declared:
        assert getattr(lib, name) is not None
    assert lib.ifx_arch() == b"gfx950" and lib.ifx_version() > 0
    abi = int(re.search(r"#define\s+IFX_ABI_MINOR\s+(\d+)", hdr).group(1))      # header, bindings and library agree on the ABI generation
    assert abi == _hip.ABI_MINOR == (lib.ifx_version() >> 8) & 255
    assert lib.ifx_last_error() is not None


def test_cabi_gemm_workspace_rules_are_functions_of_n_and_k():
    """`ifx_gemm_workspace_bytes` / `ifx_gemm_q8_workspace_bytes` (pure arithmetic, no GPU): which launches get the two-workgroup K
    split is decided by (N, K) alone — N <= 2048, at least 64 K-steps, an even number of them — at every row count, so that a row's
    summation order does not depend on the batch; the size covers the larger of the 256- and 192-token tilings (4096 bytes of flags +
    one fp32 image per tile); `gemm_small_split` (a sequence-parallel rank) opts launches below 2048 rows out of it."""
    from inferix_amd import _hip
    lib = _hip.load()
    tile = lambda M, t: -(-M // t) * 6 * t * 256 * 4
    for M in (300, 585, 4680, 7020, 9360, 10800):
        want = 4096 + max(tile(M, 256), tile(M, 192))
        assert lib.ifx_gemm_workspace_bytes(M, 1536, 8960) == want, M                   # the block's FFN down-projection
        assert lib.ifx_gemm_q8_workspace_bytes(M, 1536, 8960) == want, M                # 70 K-steps of 128 one-byte elements
        assert lib.ifx_gemm_workspace_bytes(M, 1536, 1536) == 0 and lib.ifx_gemm_workspace_bytes(M, 8960, 1536) == 0
        assert lib.ifx_gemm_workspace_bytes(M, 4608, 8960) == 0                         # N > 2048
        assert lib.ifx_gemm_q8_workspace_bytes(M, 1536, 4096) == 0                      # 32 K-steps
        assert lib.ifx_gemm_q8_workspace_bytes(M, 1536, 8960 + 128) == 0                # an odd number of K-steps
    assert lib.ifx_set_option(b"gemm_small_split", 1) == 0
    try:
        assert lib.ifx_gemm_workspace_bytes(585, 1536, 8960) == 0 and lib.ifx_gemm_q8_workspace_bytes(585, 1536, 8960) == 0
        assert lib.ifx_gemm_workspace_bytes(4680, 1536, 8960) > 0 and lib.ifx_gemm_q8_workspace_bytes(4680, 1536, 8960) > 0
    finally:
        lib.ifx_set_option(b"gemm_small_split", 0)


def test_cabi_argument_validation_without_gpu():
    """Bad arguments are rejected before any launch (no GPU needed): negative code + message, no crash."""
    import ctypes as C
    from inferix_amd import _hip
    lib = _hip.load()
    assert lib.ifx_layernorm(None, None, 4, 128, 1e-6, 0, None, None, None, 0, 0, 0, 1, None) == -1
    assert b"ifx_layernorm" in lib.ifx_last_error()
    assert lib.ifx_gemm_bf16(C.c_void_p(8), 100, C.c_void_p(8), None, C.c_void_p(8), 64, 4, 64, 100, None, None) == -1
    assert b"multiple of 64" in lib.ifx_last_error()
    assert lib.ifx_layernorm_quant(C.c_void_p(8), C.c_void_p(8), 128, C.c_void_p(8), 4, 128, 1e-6, 0, None, None, None, 0, 0, 0, 1,
                                   7, None) == -1
    assert b"unknown format" in lib.ifx_last_error()
    assert lib.ifx_layernorm_quant(C.c_void_p(8), C.c_void_p(8), 64, C.c_void_p(8), 4, 128, 1e-6, 0, None, None, None, 0, 0, 0, 1,
                                   0, None) == -1                      # row stride of the bytes shorter than the row
    assert lib.ifx_layernorm_quant_static(C.c_void_p(8), C.c_void_p(8), 256, C.c_void_p(8), 4, 4, 128, 1e-6, 0, None, None, 1, None) == -1
    assert b"ldq" in lib.ifx_last_error()                               # four outputs of 128 bytes do not fit a 256-byte row
    assert lib.ifx_layernorm_quant_static(C.c_void_p(8), C.c_void_p(8), 512, C.c_void_p(8), 4, 4, 128, 1e-6, 2, None, None, 1, None) == -1
    epi = _hip.Epilogue(_hip.IFX_EPI_BIAS, None, 0, None, 1, 0, 1)
    assert lib.ifx_gemm_q8_quant_out(C.c_void_p(16), 128, C.c_void_p(8), C.c_void_p(16), C.c_void_p(8), None, C.c_void_p(16), 64, 4, 64, 128,
                                     0, C.byref(epi), C.c_void_p(8), 1, None) == -1
    assert b"GELU" in lib.ifx_last_error()
    assert lib.ifx_set_option(b"gemm_variant", 29) == 0 and lib.ifx_set_option(b"gemm_variant", 30) != 0
    assert lib.ifx_set_option(b"gemm_variant", 0) == 0
    assert lib.ifx_set_option(b"gemm_small_split", 1) == 0 and lib.ifx_set_option(b"gemm_small_split", 2) != 0
    assert lib.ifx_set_option(b"gemm_small_split", 0) == 0
    assert lib.ifx_set_option(b"attn_variant", 8) != 0 and lib.ifx_set_option(b"no_such_option", 1) != 0
    kv = _hip.KvView(8, 8, None, 1, 100, 12, 64)
    assert lib.ifx_attn_fwd_paged(C.c_void_p(8), C.c_void_p(8), None, C.byref(kv), 4, 12, 0, 10, 0.0, None) == -1
    assert b"head_dim" in lib.ifx_last_error()


def test_cabi_row_kernel_validation_without_gpu():
    """The row kernels' host checks, each before any launch (dummy non-null pointers, no GPU): row strides shorter than the row, a
    rope shard that leaves the height x width grid, a two-segment cache view handed to a writer by logical token, and the widths
    beyond the last rung of a ladder (IFX_EUNSUP, with the width in the text)."""
    import ctypes as C
    from inferix_amd import _hip
    lib = _hip.load()
    P = C.c_void_p(8)
    EINVAL, EUNSUP = -1, -3

    def refused(rc, code, *parts):
        msg = lib.ifx_last_error()
        assert rc == code and all(p in msg for p in parts), (rc, msg)

    # widths beyond the ladders
    refused(lib.ifx_layernorm(P, P, 4, 5128, 1e-6, 0, None, None, None, 0, 0, 0, 1, None), EUNSUP, b"5128")
    refused(lib.ifx_rmsnorm(P, 5128, P, 5128, P, 4, 5128, 1e-6, None), EUNSUP, b"5128")
    refused(lib.ifx_magi_gate_norm_residual(P, 6152, P, 6152, P, P, 6152, P, P, 1, P, 6152, 4, 6152, 1e-6, None), EUNSUP,
            b"ifx_magi_gate_norm_residual", b"6152")
    # row strides
    refused(lib.ifx_rmsnorm(P, 248, P, 256, P, 4, 256, 1e-6, None), EINVAL, b"ifx_rmsnorm", b"ldx")
    refused(lib.ifx_rmsnorm(P, 256, P, 248, P, 4, 256, 1e-6, None), EINVAL, b"ifx_rmsnorm", b"ldy")
    refused(lib.ifx_quant_per_token(P, 248, P, 256, P, 4, 256, 0, None), EINVAL, b"ifx_quant_per_token", b"ldx")
    refused(lib.ifx_quant_per_token(P, 256, P, 248, P, 4, 256, 1, None), EINVAL, b"ifx_quant_per_token", b"ldq")
    kv = _hip.KvView(8, 8, None, 1, 100, 2, 128)
    app = lambda ld, rope, view: lib.ifx_rmsnorm_rope_kv_append(P, ld, P, P, P, C.byref(rope) if rope else None,
                                                                  C.byref(view) if view else None, 0, 4, 256, 1e-6, None)
    refused(app(248, None, None), EINVAL, b"ifx_rmsnorm_rope_kv_append", b"ld 248")            # q alone: ld >= dim
    refused(app(512, None, kv), EINVAL, b"ifx_rmsnorm_rope_kv_append", b"ld 512")              # q | k | v: ld >= 3 * dim
    in_place = _hip.RopeGrid(8, 1024, 0, 4, 6, 0, 24, 0.0, 1)                                   # flags bit 0: V in place
    refused(app(504, in_place, kv), EINVAL, b"ifx_rmsnorm_rope_kv_append", b"ld 504")          # q | k: ld >= 2 * dim
    # rope shard outside the grid
    refused(app(768, _hip.RopeGrid(8, 1024, 0, 4, 6, -1, 12, 0.0, 0), kv), EINVAL, b"ifx_rmsnorm_rope_kv_append", b"hw_offset")
    refused(app(768, _hip.RopeGrid(8, 1024, 0, 4, 6, 13, 12, 0.0, 0), kv), EINVAL, b"ifx_rmsnorm_rope_kv_append", b"hw_offset 13")
    peers = _hip.PeerCaches()
    peers.count, peers.k[0], peers.v[0] = 1, 8, 8
    refused(lib.ifx_rmsnorm_rope_kv_push(P, 512, P, C.byref(_hip.RopeGrid(8, 1024, 0, 4, 6, 20, 12, 0.0, 0)), C.byref(peers), C.byref(kv),
                                         0, 24, 12, 12, 4, 256, 1e-6, None), EINVAL, b"ifx_rmsnorm_rope_kv_push", b"hw_offset 20")
    # a two-segment map is for readers (and the push kernel): append, roll and scatter refuse it
    seg = _hip.KvView(8, 8, None, 1, 100, 2, 128, 40, 10)
    refused(app(768, None, seg), EINVAL, b"ifx_rmsnorm_rope_kv_append", b"seg_split 40")
    refused(lib.ifx_kv_roll(C.byref(seg), 8, 8, 8, P, None), EINVAL, b"ifx_kv_roll", b"seg_split 40")
    refused(lib.ifx_kv_scatter_shards(P, 2, 1, 4, 8, 0, C.byref(seg), None), EINVAL, b"ifx_kv_scatter_shards", b"seg_split 40")
    paged0 = _hip.KvView(8, 8, 8, 0, 100, 2, 128)
    refused(lib.ifx_kv_roll(C.byref(paged0), 8, 8, 8, P, None), EINVAL, b"ifx_kv_roll", b"page_size")


def test_cabi_gemm_operand_contract_without_gpu():
    """The operand contract of the GEMM entry points (include/inferix_hip.h), each clause refused before any launch: row strides and
    widths that no kernel's vector accesses fit, K that is not whole K-steps, and base pointers below the alignment every kernel of the
    family reads with (16-byte chunks of x / W / w_scale, 8-byte vectors of y / bias / residual / gate rows)."""
    import ctypes as C
    from inferix_amd import _hip
    lib = _hip.load()
    A, A8, A4 = C.c_void_p(4096), C.c_void_p(4104), C.c_void_p(4100)        # 16-, 8- and 4-byte aligned dummies
    EINVAL = -1

    def refused(rc, code, *parts):
        msg = lib.ifx_last_error()
        assert rc == code and all(p in msg for p in parts), (rc, msg)

    bf16 = lambda x=A, ldx=256, w=A, bias=None, y=A, ldy=64, M=4, N=64, K=256, epi=None: \
        lib.ifx_gemm_bf16(x, ldx, w, bias, y, ldy, M, N, K, C.byref(epi) if epi is not None else None, None)
    refused(bf16(ldx=260), EINVAL, b"ifx_gemm_bf16", b"ldx")
    refused(bf16(ldy=66), EINVAL, b"ifx_gemm_bf16", b"ldy")
    refused(bf16(N=66, ldy=68), EINVAL, b"ifx_gemm_bf16", b"N %")
    refused(bf16(K=96, ldx=96), EINVAL, b"ifx_gemm_bf16", b"multiple of 64")
    res = lambda ptr, ld: _hip.Epilogue(_hip.IFX_EPI_RESIDUAL, ptr, ld, None, 1, 0, 1)
    refused(bf16(epi=res(4096, 66)), EINVAL, b"ifx_gemm_bf16", b"ld_res")
    refused(bf16(epi=res(None, 64)), EINVAL, b"ifx_gemm_bf16", b"residual")

    refused(bf16(x=A8), EINVAL, b"ifx_gemm_bf16", b"16-byte")
    refused(bf16(w=A8), EINVAL, b"ifx_gemm_bf16", b"16-byte")
    refused(bf16(y=A4), EINVAL, b"ifx_gemm_bf16", b"8-byte")
    refused(bf16(bias=A4), EINVAL, b"ifx_gemm_bf16", b"8-byte")
    refused(bf16(epi=res(4100, 64)), EINVAL, b"ifx_gemm_bf16", b"8-byte")
    refused(bf16(epi=_hip.Epilogue(_hip.IFX_EPI_GATE_RES, 4096, 64, 4100, 6, 2, 2)), EINVAL, b"ifx_gemm_bf16", b"8-byte")
    ws = lambda x=A, y=A: lib.ifx_gemm_bf16_ws(x, 256, A, None, y, 64, 4, 64, 256, None, A, 1 << 20, None)
    refused(ws(x=A8), EINVAL, b"16-byte")
    refused(ws(y=A4), EINVAL, b"8-byte")
    for v in (22, 23):                 # the forced 256- and 192-token tiles ask for the split-K workspace on the split shapes
        assert lib.ifx_set_option(b"gemm_variant", v) == 0
        try:
            assert lib.ifx_gemm_workspace_bytes(333, 704, 4096) > 4096 and lib.ifx_gemm_workspace_bytes(333, 704, 256) == 0
        finally:
            lib.ifx_set_option(b"gemm_variant", 0)

    q8 = lambda xq=A, ldx=256, sx=A, wq=A, sw=A, bias=None, y=A, ldy=64, M=4, N=64, K=256, fmt=0, epi=None: \
        lib.ifx_gemm_q8(xq, ldx, sx, wq, sw, bias, y, ldy, M, N, K, fmt, C.byref(epi) if epi is not None else None, None)
    refused(q8(ldx=264), EINVAL, b"ifx_gemm_q8", b"ldx")
    refused(q8(ldy=66), EINVAL, b"ifx_gemm_q8", b"ldy")
    refused(q8(N=66, ldy=68), EINVAL, b"ifx_gemm_q8", b"N %")
    refused(q8(K=192, ldx=192), EINVAL, b"ifx_gemm_q8", b"multiple of 128")
    refused(q8(epi=res(4096, 66)), EINVAL, b"ifx_gemm_q8", b"ld_res")
    refused(q8(xq=A8), EINVAL, b"ifx_gemm_q8", b"16-byte")
    refused(q8(wq=A8), EINVAL, b"ifx_gemm_q8", b"16-byte")
    refused(q8(sw=A8), EINVAL, b"ifx_gemm_q8", b"16-byte")
    refused(q8(y=A4), EINVAL, b"ifx_gemm_q8", b"8-byte")
    refused(q8(epi=res(4100, 64)), EINVAL, b"ifx_gemm_q8", b"8-byte")

    refused(lib.ifx_gemm_q8_ws(A8, 256, A, A, A, None, A, 64, 4, 64, 256, 0, None, A, 1 << 20, None), EINVAL, b"16-byte")
    gelu = _hip.Epilogue(_hip.IFX_EPI_GELU_ERF, None, 0, None, 1, 0, 1)
    refused(lib.ifx_gemm_q8_quant_out(A, 256, A, A, A, None, A, 68, 4, 64, 256, 0, C.byref(gelu), A, 1, None), EINVAL,
            b"ifx_gemm_q8_quant_out", b"ldyq")
    refused(lib.ifx_gemm_q8_quant_out(A, 256, A, A, A, None, A4, 64, 4, 64, 256, 0, C.byref(gelu), A, 1, None), EINVAL, b"8-byte")


def test_cabi_round6_additions_without_gpu():
    """ABI minor 7 (round 6), checked without a GPU: the planar-input flag of `ifx_conv3d_desc` and the flags of `ifx_rmsnorm_cl` are
    validated before any launch, the new option keys round-trip through `ifx_set_option` / `ifx_get_option`, and `hip_ops.to_planar`
    is the documented layout `[t, c/32, h, w, 32]`."""
    import ctypes as C
    import torch
    from inferix_amd import _hip, hip_ops
    lib = _hip.load()
    assert (lib.ifx_version() >> 8) & 255 == 7 == _hip.ABI_MINOR
    slots3, slots1 = (C.c_int32 * 3)(0, 1, 2), (C.c_int32 * 1)(0)
    d = _hip.Conv3dDesc(8, 8 * 8 * 64, slots3, 8, 8, 64, 0, 8, None, 3, 3, 8, 8 * 8 * 96, slots1, 96, 1, None, 8, 2)      # in_planar = 2
    assert lib.ifx_conv3d_cl(C.byref(d), None) == -1 and b"in_planar" in lib.ifx_last_error()
    assert lib.ifx_rmsnorm_cl(C.c_void_p(8), C.c_void_p(8), C.c_void_p(8), 64 * 48, slots1, 1, 64, 48, 2, None) == -1      # planar output, 48 channels
    assert b"planar" in lib.ifx_last_error()
    assert lib.ifx_rmsnorm_cl(C.c_void_p(8), C.c_void_p(8), C.c_void_p(8), 64 * 64, slots1, 1, 64, 64, 4, None) == -1      # unknown flag bit
    v = C.c_int32(-1)
    assert lib.ifx_set_option(b"conv_variant", 1) == 0 and lib.ifx_get_option(b"conv_variant", C.byref(v)) == 0 and v.value == 1
    assert lib.ifx_set_option(b"conv_variant", 2) != 0 and lib.ifx_set_option(b"conv_variant", 0) == 0
    assert lib.ifx_get_option(b"attn_debug_counters", C.byref(v)) == 0 and v.value == 0
    assert lib.ifx_get_option(b"attn_rescale_count", C.byref(v)) == 0 and v.value == 0        # never enabled: no device word, reads 0
    x = torch.arange(2 * 3 * 4 * 64, dtype=torch.float32).view(2, 3, 4, 64).to(torch.bfloat16)
    xp = hip_ops.to_planar(x)
    assert xp.shape == (2, 2, 3, 4, 32) and xp.is_contiguous()
    assert torch.equal(xp[1, 1, 2, 3], x[1, 2, 3, 32:]) and torch.equal(xp[0, 0, 1, 2], x[0, 1, 2, :32])


ATTN_PLAN_SHAPES = [(4680, 12, 0, 32760), (585, 12, 0, 32760), (585, 12, 0, 4680), (585, 12, 4680, 9360), (1170, 12, 0, 32760),
                    (10800, 12, 0, 75600), (12150, 3, 0, 48600), (600, 12, 0, 6277), (300, 12, 0, 2048), (130, 12, 0, 1000),
                    (585, 12, 0, 512), (0, 12, 0, 100),
                    (2052, 12, 0, 9360)]         # one more than the twelve first asked for: here auto takes 7 and 6 would plan otherwise
# (splits, workspace bytes) of `ifx_attn_split_plan` per ATTN_PLAN_SHAPES row, recorded from the library as it was before the launch
# plan moved into one function (csrc/ifx_attn.h); the rows depend on the schedule's tile height and workgroup slots only
ATTN_PLAN_256 = [(1, 0), (7, 25356240), (7, 25356240), (7, 25356240), (4, 28978560), (1, 0), (3, 56424600),
                 (7, 26006400), (4, 7430400), (2, 1609920), (1, 0), (1, 0), (2, 25411968)]      # 256-row tiles, 256 workgroup slots: variants 2, 4, 5, 7 (and 1, whose split launches take 7)
ATTN_PLAN_384 = [(3, 86935680), (10, 36223200), (9, 32600880), (9, 32600880), (5, 36223200), (1, 0), (5, 94041000),
                 (10, 37152000), (4, 7430400), (2, 1609920), (1, 0), (1, 0), (3, 38117952)]      # variant 3: 384-row tiles
ATTN_PLAN_128 = [(1, 0), (8, 28978560), (8, 28978560), (8, 28978560), (4, 28978560), (1, 0), (3, 56424600),
                 (8, 29721600), (4, 7430400), (2, 1609920), (1, 0), (1, 0), (5, 63529920)]      # variant 6: 128-row tiles, 512 slots
ATTN_PLAN_AUTO = [(1, 0), (8, 28978560), (8, 28978560), (8, 28978560), (4, 28978560), (1, 0), (3, 56424600),
                  (8, 29721600), (4, 7430400), (2, 1609920), (1, 0), (1, 0), (2, 25411968)]      # auto: 128-row tiles where they fill better (585, 600 rows; 10800 x 12 by rounds), else 256


def test_attention_split_plan_table_for_every_variant():
    """`ifx_attn_split_plan` (pure host arithmetic) under `attn_variant` 0 - 7 at the launch shapes of the clips, a sequence-parallel
    rank, MAGI's ranges and the kernel tests: (splits, workspace bytes) equal the recorded table, which pins the automatic schedule
    choice, each schedule's tile height and workgroup slots, and the split heuristic."""
    import ctypes as C
    from inferix_amd import _hip
    lib = _hip.load()
    assert "IFX_ATTN_SPLIT_PENALTY" not in os.environ, "the table holds for the built-in per-chunk penalty"
    want = {0: ATTN_PLAN_AUTO, 1: ATTN_PLAN_256, 2: ATTN_PLAN_256, 3: ATTN_PLAN_384, 4: ATTN_PLAN_256, 5: ATTN_PLAN_256,
            6: ATTN_PLAN_128, 7: ATTN_PLAN_256}
    need = C.c_int64(-1)
    try:
        for variant in range(8):
            assert lib.ifx_set_option(b"attn_variant", variant) == 0
            got = []
            for rows, heads, k0, k1 in ATTN_PLAN_SHAPES:
                s = lib.ifx_attn_split_plan(rows, heads, k0, k1, C.byref(need))
                got.append((s, need.value))
            assert got == want[variant], (variant, got)
    finally:
        lib.ifx_set_option(b"attn_variant", 0)
    assert lib.ifx_attn_split_plan(585, 12, 0, 32760, None) == 8          # the byte count is optional (auto: 128-row tiles)


def _attention_refusal_cases(lib):
    """name -> call of an attention entry point with one bad argument (dummy non-null pointers: nothing here gets as far as a launch)"""
    import ctypes as C
    from inferix_amd import _hip
    P = C.c_void_p(4096)
    view = lambda **kw: C.byref(_hip.KvView(**{**dict(k=4096, v=4096, page_table=None, page_size=1, num_slots=100, kv_heads=12,
                                                       head_dim=128, seg_split=0, seg_delta=0), **kw}))
    ok, hd64, kvh2, pg0, big = view(), view(head_dim=64), view(kv_heads=2), view(page_table=4096, page_size=0), view(num_slots=4000)
    nok = view(k=None)
    i32s = lambda *v: (C.c_int32 * len(v))(*v)
    q1, k1 = i32s(0, 4), i32s(0, 10)
    q9, k9 = i32s(*([0, 4] * 9)), i32s(*([0, 10] * 9))
    used = C.c_int32(-1)
    paged = lambda q=P, kv=ok, heads=12, kv_len=10: lib.ifx_attn_fwd_paged(q, P, None, kv, 4, heads, 0, kv_len, 0.0, None)
    ld = lambda q=P, ldq=1536, ldo=1536, kv=ok, heads=12, kv_len=10, splits=1, ws=None, wsb=0: \
        lib.ifx_attn_fwd_paged_ld(q, ldq, P, ldo, None, kv, 4, heads, 0, kv_len, 0.0, splits, ws, wsb, None)
    dedup = lambda q=P, kv=ok, heads=12, kv_len=10, mult=3: lib.ifx_attn_fwd_dedup(q, P, kv, 4, heads, kv_len, mult, 0.0, None)
    ranges = lambda q=P, ldq=1536, ldo=1536, kv=ok, heads=12, n=1, qr=q1, kr=k1: \
        lib.ifx_attn_fwd_ranges(q, ldq, P, ldo, kv, 4, heads, n, qr, kr, 0.0, None)
    split = lambda q=P, kv=ok, heads=12, kv_len=10, splits=2, ws=P, wsb=1 << 30: \
        lib.ifx_attn_fwd_paged_split(q, P, None, kv, 4, heads, 0, kv_len, 0.0, splits, ws, wsb, None)
    partial = lambda q=P, kv=ok, rows=4, heads=12, kv_len=10, splits=1, ws=P, wsb=1 << 30, base=0, cap=4: \
        lib.ifx_attn_fwd_partial(q, kv, rows, heads, 0, kv_len, 0.0, splits, ws, wsb, base, cap, C.byref(used), None)
    merge = lambda ws=P, cap=4, n=2, rows=4: lib.ifx_attn_merge_partials(ws, cap, n, P, None, rows, 12, None)
    lse = lambda a=P, heads=12: lib.ifx_lse_merge(a, P, P, P, 4, heads, None)
    cases = {}
    for name, f in (("paged", paged), ("ld", ld), ("dedup", dedup), ("ranges", ranges), ("split", split), ("partial", partial)):
        cases[name + ":null q"] = lambda f=f: f(q=None)
        cases[name + ":null k"] = lambda f=f: f(kv=nok)
        cases[name + ":null view"] = lambda f=f: f(kv=None)
        cases[name + ":head_dim 64"] = lambda f=f: f(kv=hd64)
        cases[name + ":heads 5 on 2"] = lambda f=f: f(kv=kvh2, heads=5)
        cases[name + ":heads 0"] = lambda f=f: f(heads=0)
        cases[name + ":page_size 0"] = lambda f=f: f(kv=pg0)
        if name != "ranges":
            cases[name + ":keys past the slots"] = lambda f=f: f(kv_len=101)
            cases[name + ":no keys"] = lambda f=f: f(kv_len=0)
    for name, f in (("ld", ld), ("split", split)):
        cases[name + ":0 splits"] = lambda f=f: f(splits=0)
        cases[name + ":65 splits"] = lambda f=f: f(splits=65)
        cases[name + ":workspace one byte short"] = lambda f=f: f(splits=2, ws=P, wsb=2 * 4 * 12 * 129 * 4 - 1)
        cases[name + ":split without workspace"] = lambda f=f: f(splits=2, ws=None, wsb=1 << 30)
    cases["ld:no strides"] = lambda: ld(ldq=0)
    cases["ld:short stride"] = lambda: ld(ldo=1528)
    cases["ld:odd stride"] = lambda: ld(ldq=1540)
    cases["ld:null q, no strides, 0 splits"] = lambda: ld(q=None, ldq=0, splits=0)
    cases["dedup:multiplicity 0"] = lambda: dedup(mult=0)
    cases["dedup:2000 keys"] = lambda: dedup(kv=big, kv_len=2000)
    cases["ranges:null k_ranges"] = lambda: ranges(kr=None)
    cases["ranges:9 ranges"] = lambda: ranges(n=9, qr=q9, kr=k9)
    cases["ranges:0 ranges"] = lambda: ranges(n=0)
    cases["ranges:short stride"] = lambda: ranges(ldq=1528)
    cases["ranges:query range past q_rows"] = lambda: ranges(qr=i32s(0, 5))
    cases["ranges:empty query range"] = lambda: ranges(qr=i32s(2, 2))
    cases["ranges:key range past the slots"] = lambda: ranges(kr=i32s(0, 101))
    cases["ranges:second range bad"] = lambda: ranges(n=2, qr=i32s(0, 2, 2, 4), kr=i32s(0, 10, 50, 101))
    cases["partial:null workspace"] = lambda: partial(ws=None)
    cases["partial:0 rows"] = lambda: partial(rows=0)
    cases["partial:0 splits"] = lambda: partial(splits=0)
    cases["partial:cap 129"] = lambda: partial(cap=129)
    cases["partial:negative base"] = lambda: partial(base=-1)
    cases["partial:workspace one byte short"] = lambda: partial(wsb=4 * 4 * 12 * 129 * 4 - 1)
    cases["partial:slots past the cap"] = lambda: partial(kv=big, kv_len=2000, splits=2, base=3, cap=4)
    cases["partial:base at the cap"] = lambda: partial(base=4, cap=4)
    cases["merge:null workspace"] = lambda: merge(ws=None)
    cases["merge:0 slots used"] = lambda: merge(n=0)
    cases["merge:5 of 4 slots"] = lambda: merge(n=5)
    cases["merge:0 rows"] = lambda: merge(rows=0)
    cases["lse_merge:null"] = lambda: lse(a=None)
    cases["lse_merge:0 heads"] = lambda: lse(heads=0)
    return cases


ATTN_REFUSALS = {'paged:null q': (-1, 'ifx_attn_fwd_paged: null argument'),
 'paged:null k': (-1, 'ifx_attn_fwd_paged: null argument'),
 'paged:null view': (-1, 'ifx_attn_fwd_paged: null argument'),
 'paged:head_dim 64': (-1, 'ifx_attn_fwd_paged: head_dim 64 not built (128 only)'),
 'paged:heads 5 on 2': (-1, 'ifx_attn_fwd_paged: heads 5 is not a multiple of kv_heads 2'),
 'paged:heads 0': (-1, 'ifx_attn_fwd_paged: heads 0 is not a multiple of kv_heads 12'),
 'paged:page_size 0': (-1, 'ifx_attn_fwd_paged: page_size must be > 0'),
 'paged:keys past the slots': (-1, 'ifx_attn_fwd_paged: key range [0, 101) out of range (capacity 100)'),
 'paged:no keys': (-1, 'ifx_attn_fwd_paged: key range [0, 0) out of range (capacity 100)'),
 'ld:null q': (-1, 'ifx_attn_fwd_paged: null argument'),
 'ld:null k': (-1, 'ifx_attn_fwd_paged: null argument'),
 'ld:null view': (-1, 'ifx_attn_fwd_paged: null argument'),
 'ld:head_dim 64': (-1, 'ifx_attn_fwd_paged: head_dim 64 not built (128 only)'),
 'ld:heads 5 on 2': (-1, 'ifx_attn_fwd_paged: heads 5 is not a multiple of kv_heads 2'),
 'ld:heads 0': (-1, 'ifx_attn_fwd_paged: heads 0 is not a multiple of kv_heads 12'),
 'ld:page_size 0': (-1, 'ifx_attn_fwd_paged: page_size must be > 0'),
 'ld:keys past the slots': (-1, 'ifx_attn_fwd_paged: key range [0, 101) out of range (capacity 100)'),
 'ld:no keys': (-1, 'ifx_attn_fwd_paged: key range [0, 0) out of range (capacity 100)'),
 'dedup:null q': (-1, 'ifx_attn_fwd_paged: null argument'),
 'dedup:null k': (-1, 'ifx_attn_fwd_paged: null argument'),
 'dedup:null view': (-1, 'ifx_attn_fwd_paged: null argument'),
 'dedup:head_dim 64': (-1, 'ifx_attn_fwd_paged: head_dim 64 not built (128 only)'),
 'dedup:heads 5 on 2': (-1, 'ifx_attn_fwd_paged: heads 5 is not a multiple of kv_heads 2'),
 'dedup:heads 0': (-1, 'ifx_attn_fwd_paged: heads 0 is not a multiple of kv_heads 12'),
 'dedup:page_size 0': (-1, 'ifx_attn_fwd_paged: page_size must be > 0'),
 'dedup:keys past the slots': (-1, 'ifx_attn_fwd_paged: key range [0, 101) out of range (capacity 100)'),
 'dedup:no keys': (-1, 'ifx_attn_fwd_paged: key range [0, 0) out of range (capacity 100)'),
 'ranges:null q': (-1, 'ifx_attn_fwd_ranges: null argument'),
 'ranges:null k': (-1, 'ifx_attn_fwd_ranges: null argument'),
 'ranges:null view': (-1, 'ifx_attn_fwd_ranges: null argument'),
 'ranges:head_dim 64': (-1, 'ifx_attn_fwd_ranges: head_dim 64 not built (128 only)'),
 'ranges:heads 5 on 2': (-1, 'ifx_attn_fwd_ranges: heads 5 / kv_heads 2'),
 'ranges:heads 0': (-1, 'ifx_attn_fwd_ranges: heads 0 / kv_heads 12'),
 'ranges:page_size 0': (-1, 'ifx_attn_fwd_ranges: page_size must be > 0'),
 'split:null q': (-1, 'ifx_attn_fwd_paged: null argument'),
 'split:null k': (-1, 'ifx_attn_fwd_paged: null argument'),
 'split:null view': (-1, 'ifx_attn_fwd_paged: null argument'),
 'split:head_dim 64': (-1, 'ifx_attn_fwd_paged: head_dim 64 not built (128 only)'),
 'split:heads 5 on 2': (-1, 'ifx_attn_fwd_paged: heads 5 is not a multiple of kv_heads 2'),
 'split:heads 0': (-1, 'ifx_attn_fwd_paged: heads 0 is not a multiple of kv_heads 12'),
 'split:page_size 0': (-1, 'ifx_attn_fwd_paged: page_size must be > 0'),
 'split:keys past the slots': (-1, 'ifx_attn_fwd_paged: key range [0, 101) out of range (capacity 100)'),
 'split:no keys': (-1, 'ifx_attn_fwd_paged: key range [0, 0) out of range (capacity 100)'),
 'partial:null q': (-1, 'ifx_attn_fwd_partial: null argument'),
 'partial:null k': (-1, 'ifx_attn_fwd_partial: null argument'),
 'partial:null view': (-1, 'ifx_attn_fwd_partial: null argument'),
 'partial:head_dim 64': (-1, 'ifx_attn_fwd_partial: head_dim 64 not built (128 only)'),
 'partial:heads 5 on 2': (-1, 'ifx_attn_fwd_partial: heads 5 is not a multiple of kv_heads 2'),
 'partial:heads 0': (-1, 'ifx_attn_fwd_partial: heads 0 is not a multiple of kv_heads 12'),
 'partial:page_size 0': (-1, 'ifx_attn_fwd_partial: page_size must be > 0'),
 'partial:keys past the slots': (-1, 'ifx_attn_fwd_partial: key range [0, 101) out of range (capacity 100)'),
 'partial:no keys': (-1, 'ifx_attn_fwd_partial: key range [0, 0) out of range (capacity 100)'),
 'ld:0 splits': (-1, 'ifx_attn_fwd_paged_ld: num_splits 0 outside [1, 64]'),
 'ld:65 splits': (-1, 'ifx_attn_fwd_paged_ld: num_splits 65 outside [1, 64]'),
 'ld:workspace one byte short': (-1, 'ifx_attn_fwd_paged_split: workspace of 49535 B too small for 2 splits (need 49536 B)'),
 'ld:split without workspace': (-1, 'ifx_attn_fwd_paged_split: workspace of 1073741824 B too small for 2 splits (need 49536 B)'),
 'split:0 splits': (-1, 'ifx_attn_fwd_paged_split: num_splits 0 outside [1, 64]'),
 'split:65 splits': (-1, 'ifx_attn_fwd_paged_split: num_splits 65 outside [1, 64]'),
 'split:workspace one byte short': (-1, 'ifx_attn_fwd_paged_split: workspace of 49535 B too small for 2 splits (need 49536 B)'),
 'split:split without workspace': (-1, 'ifx_attn_fwd_paged_split: workspace of 1073741824 B too small for 2 splits (need 49536 B)'),
 'ld:no strides': (-1, 'ifx_attn_fwd_paged_ld: row strides must be given'),
 'ld:short stride': (-1, 'ifx_attn_fwd_paged: row strides (1536, 1528) must be >= heads * 128 and multiples of 8'),
 'ld:odd stride': (-1, 'ifx_attn_fwd_paged: row strides (1540, 1536) must be >= heads * 128 and multiples of 8'),
 'ld:null q, no strides, 0 splits': (-1, 'ifx_attn_fwd_paged_ld: num_splits 0 outside [1, 64]'),
 'dedup:multiplicity 0': (-1, 'ifx_attn_fwd_dedup: multiplicity 0'),
 'dedup:2000 keys': (-1, 'ifx_attn_fwd_dedup: the multiplicity form is built for short key ranges (<= 1024 keys), unsplit, without LSE'),
 'ranges:null k_ranges': (-1, 'ifx_attn_fwd_ranges: null argument'),
 'ranges:9 ranges': (-1, 'ifx_attn_fwd_ranges: 1..8 ranges per launch (got 9)'),
 'ranges:0 ranges': (-1, 'ifx_attn_fwd_ranges: 1..8 ranges per launch (got 0)'),
 'ranges:short stride': (-1, 'ifx_attn_fwd_ranges: row strides (1528, 1536)'),
 'ranges:query range past q_rows': (-1, 'ifx_attn_fwd_ranges: query range 0 = [0, 5) outside [0, 4)'),
 'ranges:empty query range': (-1, 'ifx_attn_fwd_ranges: query range 0 = [2, 2) outside [0, 4)'),
 'ranges:key range past the slots': (-1, 'ifx_attn_fwd_ranges: key range 0 = [0, 101) out of range (capacity 100)'),
 'ranges:second range bad': (-1, 'ifx_attn_fwd_ranges: key range 1 = [50, 101) out of range (capacity 100)'),
 'partial:null workspace': (-1, 'ifx_attn_fwd_partial: null argument'),
 'partial:0 rows': (-1, 'ifx_attn_fwd_partial: key range [0, 10) out of range (capacity 100)'),
 'partial:0 splits': (-1, 'ifx_attn_fwd_partial: bad split / slot arguments (0 splits, base 0, cap 4)'),
 'partial:cap 129': (-1, 'ifx_attn_fwd_partial: bad split / slot arguments (1 splits, base 0, cap 129)'),
 'partial:negative base': (-1, 'ifx_attn_fwd_partial: bad split / slot arguments (1 splits, base -1, cap 4)'),
 'partial:workspace one byte short': (-1, 'ifx_attn_fwd_partial: workspace of 99071 B too small for 4 slots'),
 'partial:slots past the cap': (-1, "ifx_attn_fwd_partial: slots [3, 5) exceed the workspace's 4"),
 'partial:base at the cap': (-1, "ifx_attn_fwd_partial: slots [4, 5) exceed the workspace's 4"),
 'merge:null workspace': (-1, 'ifx_attn_merge_partials: bad arguments (2 of 4 slots)'),
 'merge:0 slots used': (-1, 'ifx_attn_merge_partials: bad arguments (0 of 4 slots)'),
 'merge:5 of 4 slots': (-1, 'ifx_attn_merge_partials: bad arguments (5 of 4 slots)'),
 'merge:0 rows': (-1, 'ifx_attn_merge_partials: bad arguments (2 of 4 slots)'),
 'lse_merge:null': (-1, 'ifx_lse_merge: bad arguments'),
 'lse_merge:0 heads': (-1, 'ifx_lse_merge: bad arguments')}


def test_attention_entry_points_refuse_bad_arguments_with_the_recorded_texts():
    """Every attention entry point (`ifx_attn_fwd_paged`, `_paged_ld`, `_dedup`, `_ranges`, `_paged_split`, `_partial`,
    `ifx_attn_merge_partials`, `ifx_lse_merge`) with null pointers, head_dim 64, 5 heads on 2 kv heads, key and query ranges out of
    range, a page table with page_size 0, 0 / 65 splits, 9 ranges, short workspaces and slots past the cap: return code and
    `ifx_last_error()` are byte for byte what the library answered before its checks were gathered into one function — prefixes that
    name a sibling entry point included.  No call gets as far as a launch."""
    from inferix_amd import _hip
    lib = _hip.load()
    cases = _attention_refusal_cases(lib)
    assert set(cases) == set(ATTN_REFUSALS), set(cases) ^ set(ATTN_REFUSALS)
    for variant in (0, 1, 6):                 # the refusals do not depend on the schedule
        assert lib.ifx_set_option(b"attn_variant", variant) == 0
        try:
            got = {name: (call(), lib.ifx_last_error().decode()) for name, call in cases.items()}
        finally:
            lib.ifx_set_option(b"attn_variant", 0)
        bad = {n: (got[n], ATTN_REFUSALS[n]) for n in cases if got[n] != ATTN_REFUSALS[n]}
        assert not bad, (variant, bad)


def test_ops_refuse_cpu_tensors():
    from inferix_amd import _hip, hip_ops
    with pytest.raises(_hip.HipKernelError):
        hip_ops.layernorm(torch.zeros(4, 128, dtype=BF), 1e-6)
    with pytest.raises(_hip.HipKernelError):
        hip_ops.linear(torch.zeros(4, 64, dtype=BF), torch.zeros(8, 64, dtype=BF), None)


def test_kv_manager_matches_reference_golden():
    from inferix_amd.kvcache_manager import (KVCacheManager, KVCacheRequest, KVCacheRequestSpec, KVCacheSpec)
    from inferix_amd.kvcache_manager.model import SelfForcingKVCacheManagerFactory
    fx = golden("kv_manager.npz")
    kvm = KVCacheManager(device="cpu")
    req = KVCacheRequest("r0")
    ad = SelfForcingKVCacheManagerFactory.create_manager(3, 2, 128, enable_kv_offload=False)
    ad.allocate_kv_cache(kv_cache_manager=kvm, kv_cache_request=req, sequence_length=50, dtype=BF)
    ad.allocate_crossattn_cache(kv_cache_manager=kvm, kv_cache_request=req, crossattn_length=16, dtype=BF)
    assert "|".join(kvm.layers(req)) == str(fx["layers"])
    raw = kvm.get_raw(req, "layer_3")
    raw.zero_()
    assert list(raw.shape) == fx["raw_shape"].tolist()
    assert list(ad.get_kv_cache(kvm, req).shape) == fx["get_kv_shape"].tolist()
    assert list(ad.get_crossattn_cache(kvm, req).shape) == fx["get_cross_shape"].tolist()
    s = kvm.layer_spec(req, "layer_3")
    assert [s.size, s.num_tokens, s.num_blocks, s.block_size] == fx["spec"].tolist()
    ad.set_kv_cache(kvm, req, start_index=0, k_data=fx["set_k"], v_data=fx["set_v"])
    assert torch.equal(kvm.get(req, "layer_3"), fx["after_set"])
    assert torch.equal(kvm.get_range(req, "layer_3", 2, 4), fx["get_range_2_4"])
    assert torch.equal(kvm.select(req, "layer_3", [1, 5]), fx["select_1_5"])
    kvm.allocate_slots(KVCacheRequest("r1"), KVCacheRequestSpec(num_tokens=10, block_size=4, specs={
        "L": KVCacheSpec(num_kv_heads=2, head_size=8, dtype=torch.float32, kv_offload=False, use_mla=False),
        "M": KVCacheSpec(num_kv_heads=1, head_size=8, dtype=torch.float32, kv_offload=False, use_mla=True)}))
    assert list(kvm.get_raw(KVCacheRequest("r1"), "L").shape) == fx["bs4_shape"].tolist()
    assert list(kvm.get_raw(KVCacheRequest("r1"), "M").shape) == fx["mla_shape"].tolist()
    s = kvm.layer_spec(KVCacheRequest("r1"), "L")
    assert [s.size, s.num_tokens, s.num_blocks, s.block_size] == fx["bs4_spec"].tolist()
    errs = []
    try:
        ad.allocate_kv_cache(kv_cache_manager=kvm, kv_cache_request=req, sequence_length=50, dtype=BF)
    except Exception as e:  # noqa: BLE001
        errs.append(type(e).__name__)
    try:
        kvm.free(KVCacheRequest("nope"))
    except Exception as e:  # noqa: BLE001
        errs.append(type(e).__name__)
    assert "|".join(errs) == str(fx["errors"])
    ad.clear_cache(kvm, req)
    assert "|".join(kvm.layers(req)) == str(fx["layers_after_clear"])
    kvm.free(req)
    assert "|".join(kvm.layers(req)) == str(fx["layers_after_free"])


def test_page_table_rotation_equals_physical_roll():
    """rotate_pages gives the same LOGICAL cache as the reference's eviction shift (causal_model.py:287-292)."""
    from inferix_amd.kvcache_manager import KVCacheManager, KVCacheRequest, KVCacheRequestSpec, KVCacheSpec
    kvm, req = KVCacheManager("cpu"), KVCacheRequest("r")
    kvm.allocate_slots(req, KVCacheRequestSpec(num_tokens=144, block_size=1, specs={
        "layer_0": KVCacheSpec(num_kv_heads=1, head_size=2, dtype=torch.float32, kv_offload=False, use_mla=False)}))
    t = kvm.get_raw(req, "layer_0")
    t[0, :, 0, 0, 0] = torch.arange(144.0)
    pt = kvm.enable_paging(req, "layer_0", 24)
    ref = torch.arange(144.0)
    sink, ev, rolled = 24, 72, 48
    ref[sink:sink + rolled] = ref[sink + ev:sink + ev + rolled].clone()
    kvm.rotate_pages(req, "layer_0", sink // 24, ev // 24, rolled // 24)
    tok = torch.arange(144)
    slot = pt.host[tok // 24].long() * 24 + tok % 24
    logical = t[0, slot, 0, 0, 0]
    assert torch.equal(logical[:sink + rolled], ref[:sink + rolled])
    assert sorted(pt.host.tolist()) == list(range(6))           # still a permutation: recycled pages are reused


def test_scheduler_matches_reference_golden():
    from inferix_amd.schedulers import FlowMatchScheduler
    fx = golden("scheduler.npz")
    for shift in (5.0, 8.0):
        tag = str(int(shift))
        s = FlowMatchScheduler(shift=shift, sigma_min=0.0, extra_one_step=True)
        s.set_timesteps(1000, training=True)
        assert torch.equal(s.sigmas, fx[f"sigmas_{tag}"]) and torch.equal(s.timesteps, fx[f"timesteps_{tag}"])
        out = s.add_noise(fx[f"an_x0_{tag}"], fx[f"an_eps_{tag}"], fx[f"an_t_{tag}"])
        assert torch.equal(out, fx[f"an_out_{tag}"])


def test_kv_index_update_matches_oracle_exhaustively():
    from inferix_amd.wan.causal_model import kv_index_update
    for las, sink in ((-1, 0), (6, 24), (4, 0), (9, 48)):
        cap = 504 if las == -1 else las * 24
        ge = le = 0
        for blk in list(range(8)) + [7, 7]:            # includes re-runs of the same block
            for _rep in range(2):
                a = kv_index_update(ge, le, blk * 72, 72, cap, las, sink)
                b = O.kv_index_update(ge, le, blk * 72, 72, cap, las, sink)
                assert (a.local_start, a.local_end, a.global_end, a.evicted, a.rolled) == \
                       (b.local_start, b.local_end, b.global_end, b.evicted, b.rolled)
                ge, le = a.global_end, a.local_end
                if las == -1 and le >= cap:
                    break


class _FakeGen(torch.nn.Module):
    """CPU stand-in generator: records the call schedule of the pipeline (control-flow test only)."""

    def __init__(self, num_layers=2):
        super().__init__()
        from inferix_amd.kvcache_manager.model import SelfForcingKVCacheManagerFactory
        from inferix_amd.schedulers import FlowMatchScheduler
        self.model = SimpleNamespace(num_layers=num_layers, local_attn_size=-1, text_len=16, num_frame_per_block=1,
                                     blocks=[SimpleNamespace(kv_cache_manager=SelfForcingKVCacheManagerFactory.create_manager(i, 2, 128))
                                             for i in range(num_layers)])
        self.parallel_config = None
        self.scheduler = FlowMatchScheduler(shift=5.0, sigma_min=0.0, extra_one_step=True)
        self.scheduler.set_timesteps(1000, training=True)
        self.calls = []

    def get_scheduler(self):
        return self.scheduler

    def forward(self, noisy_image_or_video, conditional_dict, timestep, kv_cache_meta, crossattn_cache_meta,
                current_start, kv_cache_manager, kv_cache_requests):
        self.calls.append((current_start, float(timestep.flatten()[0]), tuple(timestep.shape)))
        return noisy_image_or_video, noisy_image_or_video * 0.5


def test_pipeline_call_schedule_matches_reference_trace():
    """The mirror pipeline issues the same generator calls (current_start, timestep) in the same order as the
    reference's CausalInferencePipeline did when the golden rollouts were generated."""
    from inferix_amd.core import DecodeMode
    from inferix_amd.kvcache_manager import KVCacheManager, KVCacheRequest
    from inferix_amd.pipeline import CausalInferencePipeline
    for name in ("rollout_tiny.npz", "rollout_tiny_prefill.npz"):
        fx = golden(name)
        gen = _FakeGen()
        args = SimpleNamespace(denoising_step_list=fx["steps"].tolist(), warp_denoising_step=True,
                               num_frame_per_block=3, independent_first_frame=False, context_noise=0,
                               frame_seq_length=24, kv_cache_tokens=504)
        gen.scheduler = __import__("inferix_amd.schedulers", fromlist=["x"]).FlowMatchScheduler(
            shift=float(fx["shift"]), sigma_min=0.0, extra_one_step=True)
        gen.scheduler.set_timesteps(1000, training=True)
        pipe = CausalInferencePipeline(args, "cpu", generator=gen, text_encoder=lambda text_prompts: {"prompt_embeds": None},
                                       vae=None)
        seen = []
        out = pipe.inference(noise=fx["noise"], text_prompts=["x"], kv_cache_manager=KVCacheManager("cpu"),
                             kv_cache_requests=[KVCacheRequest("r")], initial_latent=fx.get("initial_latent"),
                             decode_mode=DecodeMode.NO_DECODE, block_callback=lambda lat, i: seen.append((i, tuple(lat.shape))))
        assert [c[0] for c in gen.calls] == fx["trace"][:, 0].tolist()
        ref_t = [float(fx[f"call{i}_t"].flatten()[0]) for i in range(int(fx["num_calls"]))]
        assert [round(c[1], 3) for c in gen.calls] == [round(t, 3) for t in ref_t]
        nb = fx["noise"].shape[1] // 3
        assert [s[0] for s in seen] == list(range(nb)) and all(s[1][1] == 3 for s in seen)
        assert out.shape[1] == fx["out"].shape[1]
        assert pipe.kv_cache_meta is None           # free_cache_before_vae=True cleared the caches


def test_pipeline_pairs_the_rerun_with_the_next_first_step_in_reference_order():
    """With a generator that offers `forward_pair` the pipeline defers each block's clean-context re-run into the next block's first
    denoising step (one `forward_pair(first, second)` call) — except the last block's, which runs alone.  The LOGICAL call sequence
    (first before second inside a pair) must still be the reference's trace, the block callback must see every block once and in
    order BEFORE its re-run, `pair_forwards=False` and `profile=True` must fall back to one call at a time, and the reused timestep
    tensors must carry the reference's values."""
    from inferix_amd.core import DecodeMode
    from inferix_amd.kvcache_manager import KVCacheManager, KVCacheRequest
    from inferix_amd.pipeline import CausalInferencePipeline

    class PairGen(_FakeGen):
        def __init__(self):
            super().__init__()
            self.pairs = 0
            self.events = []

        def forward(self, **kw):
            self.events.append(("call", kw["current_start"]))
            return super().forward(**kw)

        def forward_pair(self, first, second):
            self.pairs += 1
            assert first["kv_cache_manager"] is second["kv_cache_manager"] and first["current_start"] < second["current_start"]
            assert float(first["timestep"].flatten()[0]) == 0.0, "the first of a pair is the clean-context re-run"
            return super().forward(**first), super().forward(**second)

    for name in ("rollout_tiny.npz", "rollout_tiny_prefill.npz"):
        fx = golden(name)
        ref_starts = fx["trace"][:, 0].tolist()
        ref_t = [round(float(fx[f"call{i}_t"].flatten()[0]), 3) for i in range(int(fx["num_calls"]))]
        nb = fx["noise"].shape[1] // 3
        for pair_arg, profile, want_pairs in ((None, False, nb - 1), (False, False, 0), (True, True, 0)):
            gen = PairGen()
            args = SimpleNamespace(denoising_step_list=fx["steps"].tolist(), warp_denoising_step=True, num_frame_per_block=3,
                                   independent_first_frame=False, context_noise=0, frame_seq_length=24, kv_cache_tokens=504,
                                   pair_forwards=pair_arg)
            gen.scheduler = __import__("inferix_amd.schedulers", fromlist=["x"]).FlowMatchScheduler(
                shift=float(fx["shift"]), sigma_min=0.0, extra_one_step=True)
            gen.scheduler.set_timesteps(1000, training=True)
            pipe = CausalInferencePipeline(args, "cpu", generator=gen, text_encoder=lambda text_prompts: {"prompt_embeds": None}, vae=None)
            seen = []

            def cb(lat, i, gen=gen, seen=seen):
                seen.append((i, len(gen.calls)))
            if profile:
                import inferix_amd.pipeline.causal_inference as ci
                real_event, real_sync = torch.cuda.Event, torch.cuda.synchronize

                class _Ev:                       # the block timers of `profile=True` without a GPU
                    def __init__(self, **kw):
                        pass

                    def record(self):
                        pass

                    def elapsed_time(self, other):
                        return 0.0
                torch.cuda.Event, torch.cuda.synchronize = _Ev, (lambda: None)
            try:
                pipe.inference(noise=fx["noise"], text_prompts=["x"], kv_cache_manager=KVCacheManager("cpu"),
                               kv_cache_requests=[KVCacheRequest("r")], initial_latent=fx.get("initial_latent"),
                               decode_mode=DecodeMode.NO_DECODE, block_callback=cb, profile=profile)
            finally:
                if profile:
                    torch.cuda.Event, torch.cuda.synchronize = real_event, real_sync
            assert gen.pairs == want_pairs, (name, pair_arg, profile, gen.pairs)
            assert [c[0] for c in gen.calls] == ref_starts and [round(c[1], 3) for c in gen.calls] == ref_t, (name, pair_arg, profile)
            assert [s_[0] for s_ in seen] == list(range(nb))
            if want_pairs:
                # a block's callback fires with its own steps issued and its re-run still pending (block 0 of the plain rollout: 3 calls)
                per_block = len(fx["steps"])
                n_pref = len(ref_starts) - nb * (per_block + 1)
                assert [s_[1] for s_ in seen[:-1]] == [n_pref + per_block + b * (per_block + 1) for b in range(nb - 1)], seen


def test_parallel_config_and_registry():
    from inferix_amd.attention import collect_supported_attn
    from inferix_amd.wan import ParallelConfig
    assert list(collect_supported_attn()) == ["HipPagedFA"]
    assert ParallelConfig().attn_backend == "HipPagedFA"
    with pytest.raises(ValueError):
        ParallelConfig(attn_backend="FlashAttnV3")


def test_components_match_oracle():
    from inferix_amd.wan import components as C
    t = torch.tensor([0.0, 625.0, 1000.0])
    assert torch.equal(C.sinusoidal_embedding_1d(64, t), O.sinusoidal_embedding_1d(64, t))
    assert torch.equal(C.rope_table(128), torch.view_as_real(O.rope_freqs(128)))
    cfg = O.tiny_config()
    g = torch.Generator().manual_seed(0)
    lat = torch.randn(2, 16, 3, 8, 12, generator=g)
    assert torch.equal(C.patchify(lat, cfg.patch_size), O.patchify(lat, cfg).flatten(0, 1))
    y = torch.randn(2 * 72, 64, generator=g)
    assert torch.equal(C.unpatchify(y, 2, (3, 4, 6), cfg.patch_size, 16), O.unpatchify(y.view(2, 72, 64), (3, 4, 6), cfg))


def test_outer_plugin_refuses_to_run_without_a_gpu(tmp_path):
    """`SelfForcingPipeline` (the reference's plugin class name) exists, parses its yaml, and fails loudly on a host
    without an MI355X instead of falling back to anything."""
    import yaml
    from inferix_amd.pipeline import SelfForcingPipeline
    import torch
    cfg = tmp_path / "c.yaml"
    cfg.write_text(yaml.safe_dump({"denoising_step_list": [1000, 750, 500, 250], "model_kwargs": {}}))
    if torch.cuda.is_available():
        pytest.skip("GPU present: covered by tests/test_hip_plugin_api.py")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        SelfForcingPipeline(str(cfg))
    bidir = tmp_path / "b.yaml"
    bidir.write_text(yaml.safe_dump({"model_kwargs": {}}))
    with pytest.raises(NotImplementedError):
        SelfForcingPipeline(str(bidir))


def test_no_transcendental_to_valu_hazard_in_the_built_kernels():
    """A VALU instruction must not read a v_exp / v_rcp / v_log ... result in the very next slot; the compiler pads its own code but
    not inline asm (found as -inf attention row sums after a recompile).  tools/check_trans_hazard.py disassembles the
    gfx950 code objects of the built library and looks for such pairs."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = os.path.join(root, "inferix_amd", "libinferix_hip.so")
    if not (os.path.exists(lib) and os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump")):
        import pytest
        pytest.skip("library or llvm-objdump not present")
    p = subprocess.run([sys.executable, os.path.join(root, "tools", "check_trans_hazard.py"), lib], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-500:]


# What tools/gemm_plan_check.cpp printed at the commit BEFORE the dispatch moved into inferix_amd/csrc/ifx_gemm_plan.h (there its
# ping-pong stub derived ks by the expression launch_gemm_pp used at that commit): one checksum per (gemm_small_split, gemm_variant,
# entry point) over every launch line, refusal and workspace query of the sweep, then the project's named shapes under the automatic
# choice in full (`path tile tj ks workspace-used y2`, or the kernel of the entry point's own file with grid, block and LDS bytes).
GEMM_DISPATCH_RECORDED = """\
small_split 0 variant  0 bf16:  15580 calls, checksum c3d9ca822d05a8d8
small_split 0 variant  0 q8:    25160 calls, checksum 2527d1c7c50ad047
small_split 0 variant  1 bf16:  15580 calls, checksum eac9862b8532484a
small_split 0 variant  1 q8:    25160 calls, checksum 6461fd4f807d4b37
small_split 0 variant  2 bf16:  15580 calls, checksum 0d51e7193c29daa6
small_split 0 variant  2 q8:    25160 calls, checksum b47988ad7b506e9b
small_split 0 variant  3 bf16:  15580 calls, checksum 7a35a02f75b81e7e
small_split 0 variant  3 q8:    25160 calls, checksum 9b486e7e0ada4b87
small_split 0 variant  4 bf16:  15580 calls, checksum 926cb022b713eed6
small_split 0 variant  4 q8:    25160 calls, checksum 7eee42d7066c5099
small_split 0 variant  5 bf16:  15580 calls, checksum 239c8d3b308bde56
small_split 0 variant  5 q8:    25160 calls, checksum 7eee42d7066c5099
small_split 0 variant  6 bf16:  15580 calls, checksum 899c73bb87aa6cce
small_split 0 variant  6 q8:    25160 calls, checksum 7eee42d7066c5099
small_split 0 variant  7 bf16:  15580 calls, checksum bad234eb5db9bf06
small_split 0 variant  7 q8:    25160 calls, checksum 7eee42d7066c5099
small_split 0 variant  8 bf16:  15580 calls, checksum 634214a07d61e97e
small_split 0 variant  8 q8:    25160 calls, checksum 7eee42d7066c5099
small_split 0 variant  9 bf16:  15580 calls, checksum b9f767abbfa6bace
small_split 0 variant  9 q8:    25160 calls, checksum 7eee42d7066c5099
small_split 0 variant 10 bf16:  15580 calls, checksum 0f500c2ffaaecdc6
small_split 0 variant 10 q8:    25160 calls, checksum 7eee42d7066c5099
small_split 0 variant 11 bf16:  15580 calls, checksum cfd71b1cd23522ae
small_split 0 variant 11 q8:    25160 calls, checksum 7eee42d7066c5099
small_split 0 variant 12 bf16:  15580 calls, checksum f8a6950a42d1932e
small_split 0 variant 12 q8:    25160 calls, checksum 7eee42d7066c5099
small_split 0 variant 13 bf16:  15580 calls, checksum b3cc7aed6b454c0e
small_split 0 variant 13 q8:    25160 calls, checksum 7eee42d7066c5099
small_split 0 variant 14 bf16:  15580 calls, checksum db66fd38359c270e
small_split 0 variant 14 q8:    25160 calls, checksum 7eee42d7066c5099
small_split 0 variant 15 bf16:  15580 calls, checksum 01e3aa15f59c2896
small_split 0 variant 15 q8:    25160 calls, checksum 7eee42d7066c5099
small_split 0 variant 16 bf16:  15580 calls, checksum c272b2185148630e
small_split 0 variant 16 q8:    25160 calls, checksum 7eee42d7066c5099
small_split 0 variant 17 bf16:  15580 calls, checksum 20e0d8c23a17a18e
small_split 0 variant 17 q8:    25160 calls, checksum 7eee42d7066c5099
small_split 0 variant 18 bf16:  15580 calls, checksum 14868364c6dfc37e
small_split 0 variant 18 q8:    25160 calls, checksum 7eee42d7066c5099
small_split 0 variant 19 bf16:  15580 calls, checksum 4d9e843c38a11f66
small_split 0 variant 19 q8:    25160 calls, checksum 7eee42d7066c5099
small_split 0 variant 20 bf16:  15580 calls, checksum 34618adec7f3fdf6
small_split 0 variant 20 q8:    25160 calls, checksum 7eee42d7066c5099
small_split 0 variant 21 bf16:  15580 calls, checksum 211e508709500aae
small_split 0 variant 21 q8:    25160 calls, checksum 7eee42d7066c5099
small_split 0 variant 22 bf16:  15580 calls, checksum 02b6376eeb6acef2
small_split 0 variant 22 q8:    25160 calls, checksum 884358052a46ef97
small_split 0 variant 23 bf16:  15580 calls, checksum 78e189751fefa78e
small_split 0 variant 23 q8:    25160 calls, checksum b7f5460339280217
small_split 0 variant 24 bf16:  15580 calls, checksum 5bb0f38c49e8208e
small_split 0 variant 24 q8:    25160 calls, checksum d18cc73dedda364f
small_split 0 variant 25 bf16:  15580 calls, checksum f5d389557bae4e66
small_split 0 variant 25 q8:    25160 calls, checksum 8625967a129234cf
small_split 0 variant 26 bf16:  15580 calls, checksum 0c460cf6f22179f8
small_split 0 variant 26 q8:    25160 calls, checksum 7eee42d7066c5099
small_split 0 variant 27 bf16:  15580 calls, checksum 54cfbc3397effe94
small_split 0 variant 27 q8:    25160 calls, checksum 7eee42d7066c5099
small_split 0 variant 28 bf16:  15580 calls, checksum a5d67e0b78f01bff
small_split 0 variant 28 q8:    25160 calls, checksum 7eee42d7066c5099
small_split 0 variant 29 bf16:  15580 calls, checksum d3e703cb74842cc1
small_split 0 variant 29 q8:    25160 calls, checksum 7eee42d7066c5099
small_split 1 variant  0 bf16:  15580 calls, checksum dc95d09bc4304fa8
small_split 1 variant  0 q8:    25160 calls, checksum 4ce1e093e3ca796c
small_split 1 variant  1 bf16:  15580 calls, checksum eac9862b8532484a
small_split 1 variant  1 q8:    25160 calls, checksum 6461fd4f807d4b37
small_split 1 variant  2 bf16:  15580 calls, checksum 0d51e7193c29daa6
small_split 1 variant  2 q8:    25160 calls, checksum b47988ad7b506e9b
small_split 1 variant  3 bf16:  15580 calls, checksum 7a35a02f75b81e7e
small_split 1 variant  3 q8:    25160 calls, checksum 9b486e7e0ada4b87
small_split 1 variant  4 bf16:  15580 calls, checksum 926cb022b713eed6
small_split 1 variant  4 q8:    25160 calls, checksum 7eee42d7066c5099
small_split 1 variant  5 bf16:  15580 calls, checksum 239c8d3b308bde56
small_split 1 variant  5 q8:    25160 calls, checksum 7eee42d7066c5099
small_split 1 variant  6 bf16:  15580 calls, checksum 899c73bb87aa6cce
small_split 1 variant  6 q8:    25160 calls, checksum 7eee42d7066c5099
small_split 1 variant  7 bf16:  15580 calls, checksum bad234eb5db9bf06
small_split 1 variant  7 q8:    25160 calls, checksum 7eee42d7066c5099
small_split 1 variant  8 bf16:  15580 calls, checksum 634214a07d61e97e
small_split 1 variant  8 q8:    25160 calls, checksum 7eee42d7066c5099
small_split 1 variant  9 bf16:  15580 calls, checksum b9f767abbfa6bace
small_split 1 variant  9 q8:    25160 calls, checksum 7eee42d7066c5099
small_split 1 variant 10 bf16:  15580 calls, checksum 0f500c2ffaaecdc6
small_split 1 variant 10 q8:    25160 calls, checksum 7eee42d7066c5099
small_split 1 variant 11 bf16:  15580 calls, checksum cfd71b1cd23522ae
small_split 1 variant 11 q8:    25160 calls, checksum 7eee42d7066c5099
small_split 1 variant 12 bf16:  15580 calls, checksum f8a6950a42d1932e
small_split 1 variant 12 q8:    25160 calls, checksum 7eee42d7066c5099
small_split 1 variant 13 bf16:  15580 calls, checksum b3cc7aed6b454c0e
small_split 1 variant 13 q8:    25160 calls, checksum 7eee42d7066c5099
small_split 1 variant 14 bf16:  15580 calls, checksum db66fd38359c270e
small_split 1 variant 14 q8:    25160 calls, checksum 7eee42d7066c5099
small_split 1 variant 15 bf16:  15580 calls, checksum 01e3aa15f59c2896
small_split 1 variant 15 q8:    25160 calls, checksum 7eee42d7066c5099
small_split 1 variant 16 bf16:  15580 calls, checksum c272b2185148630e
small_split 1 variant 16 q8:    25160 calls, checksum 7eee42d7066c5099
small_split 1 variant 17 bf16:  15580 calls, checksum 20e0d8c23a17a18e
small_split 1 variant 17 q8:    25160 calls, checksum 7eee42d7066c5099
small_split 1 variant 18 bf16:  15580 calls, checksum 14868364c6dfc37e
small_split 1 variant 18 q8:    25160 calls, checksum 7eee42d7066c5099
small_split 1 variant 19 bf16:  15580 calls, checksum 4d9e843c38a11f66
small_split 1 variant 19 q8:    25160 calls, checksum 7eee42d7066c5099
small_split 1 variant 20 bf16:  15580 calls, checksum 43998d5cde7669dc
small_split 1 variant 20 q8:    25160 calls, checksum 7eee42d7066c5099
small_split 1 variant 21 bf16:  15580 calls, checksum 211e508709500aae
small_split 1 variant 21 q8:    25160 calls, checksum 7eee42d7066c5099
small_split 1 variant 22 bf16:  15580 calls, checksum 02b6376eeb6acef2
small_split 1 variant 22 q8:    25160 calls, checksum ebf67afa9e169032
small_split 1 variant 23 bf16:  15580 calls, checksum 78e189751fefa78e
small_split 1 variant 23 q8:    25160 calls, checksum b7f5460339280217
small_split 1 variant 24 bf16:  15580 calls, checksum 5bb0f38c49e8208e
small_split 1 variant 24 q8:    25160 calls, checksum d18cc73dedda364f
small_split 1 variant 25 bf16:  15580 calls, checksum f5d389557bae4e66
small_split 1 variant 25 q8:    25160 calls, checksum 8625967a129234cf
small_split 1 variant 26 bf16:  15580 calls, checksum 3e2b73efd661a990
small_split 1 variant 26 q8:    25160 calls, checksum 7eee42d7066c5099
small_split 1 variant 27 bf16:  15580 calls, checksum 54cfbc3397effe94
small_split 1 variant 27 q8:    25160 calls, checksum 7eee42d7066c5099
small_split 1 variant 28 bf16:  15580 calls, checksum a5d67e0b78f01bff
small_split 1 variant 28 q8:    25160 calls, checksum 7eee42d7066c5099
small_split 1 variant 29 bf16:  15580 calls, checksum d3e703cb74842cc1
small_split 1 variant 29 q8:    25160 calls, checksum 7eee42d7066c5099
small_split 0 bf16  4680 x  4608 x  1536 bias      workspace none      : pp - 3 1 0 0
small_split 0 bf16  4680 x  4608 x  1536 bias      workspace 0         : pp - 3 1 0 0
small_split 0 bf16  4680 x  4608 x  1536 gate/1560 workspace none      : pp - 3 1 0 0
small_split 0 bf16  4680 x  4608 x  1536 gate/1560 workspace 0         : pp - 3 1 0 0
small_split 0 fp8   4680 x  4608 x  1536 bias      workspace 0         : pp-f8 - 3 1 0 0
small_split 0 bf16  4680 x  1536 x  1536 bias      workspace none      : pp - 2 1 0 0
small_split 0 bf16  4680 x  1536 x  1536 bias      workspace 0         : pp - 2 1 0 0
small_split 0 bf16  4680 x  1536 x  1536 gate/1560 workspace none      : pp - 2 1 0 0
small_split 0 bf16  4680 x  1536 x  1536 gate/1560 workspace 0         : pp - 2 1 0 0
small_split 0 fp8   4680 x  1536 x  1536 bias      workspace 0         : pp-f8 - 2 1 0 0
small_split 0 bf16  4680 x  8960 x  1536 bias      workspace none      : pp - 4 1 0 0
small_split 0 bf16  4680 x  8960 x  1536 bias      workspace 0         : pp - 4 1 0 0
small_split 0 bf16  4680 x  8960 x  1536 gate/1560 workspace none      : pp - 4 1 0 0
small_split 0 bf16  4680 x  8960 x  1536 gate/1560 workspace 0         : pp - 4 1 0 0
small_split 0 fp8   4680 x  8960 x  1536 bias      workspace 0         : pp-f8 - 4 1 0 0
small_split 0 bf16  4680 x  1536 x  8960 bias      workspace none      : pp - 2 1 0 0
small_split 0 bf16  4680 x  1536 x  8960 bias      workspace 29888512  : pp - 4 2 1 0
small_split 0 bf16  4680 x  1536 x  8960 gate/1560 workspace none      : pp - 2 1 0 0
small_split 0 bf16  4680 x  1536 x  8960 gate/1560 workspace 29888512  : pp - 4 2 1 0
small_split 0 fp8   4680 x  1536 x  8960 bias      workspace 29888512  : pp-f8 - 4 2 1 0
small_split 0 bf16 10800 x  4608 x  1536 bias      workspace none      : pp - 4 1 0 0
small_split 0 bf16 10800 x  4608 x  1536 bias      workspace 0         : pp - 4 1 0 0
small_split 0 bf16 10800 x  4608 x  1536 gate/1560 workspace none      : pp - 4 1 0 0
small_split 0 bf16 10800 x  4608 x  1536 gate/1560 workspace 0         : pp - 4 1 0 0
small_split 0 fp8  10800 x  4608 x  1536 bias      workspace 0         : pp-f8 - 4 1 0 0
small_split 0 bf16 10800 x  1536 x  1536 bias      workspace none      : pp - 2 1 0 0
small_split 0 bf16 10800 x  1536 x  1536 bias      workspace 0         : pp - 2 1 0 0
small_split 0 bf16 10800 x  1536 x  1536 gate/1560 workspace none      : pp - 2 1 0 0
small_split 0 bf16 10800 x  1536 x  1536 gate/1560 workspace 0         : pp - 2 1 0 0
small_split 0 fp8  10800 x  1536 x  1536 bias      workspace 0         : pp-f8 - 2 1 0 0
small_split 0 bf16 10800 x  8960 x  1536 bias      workspace none      : pp - 4 1 0 0
small_split 0 bf16 10800 x  8960 x  1536 bias      workspace 0         : pp - 4 1 0 0
small_split 0 bf16 10800 x  8960 x  1536 gate/1560 workspace none      : pp - 4 1 0 0
small_split 0 bf16 10800 x  8960 x  1536 gate/1560 workspace 0         : pp - 4 1 0 0
small_split 0 fp8  10800 x  8960 x  1536 bias      workspace 0         : pp-f8 - 4 1 0 0
small_split 0 bf16 10800 x  1536 x  8960 bias      workspace none      : pp - 2 1 0 0
small_split 0 bf16 10800 x  1536 x  8960 bias      workspace 67637248  : pp - 3 2 1 0
small_split 0 bf16 10800 x  1536 x  8960 gate/1560 workspace none      : pp - 2 1 0 0
small_split 0 bf16 10800 x  1536 x  8960 gate/1560 workspace 67637248  : pp - 3 2 1 0
small_split 0 fp8  10800 x  1536 x  8960 bias      workspace 67637248  : pp-f8 - 4 2 1 0
small_split 1 bf16   585 x  4608 x  1536 bias      workspace none      : dma 13 - - 0 0
small_split 1 bf16   585 x  4608 x  1536 bias      workspace 0         : dma 13 - - 0 0
small_split 1 bf16   585 x  4608 x  1536 gate/1560 workspace none      : dma 13 - - 0 0
small_split 1 bf16   585 x  4608 x  1536 gate/1560 workspace 0         : dma 13 - - 0 0
small_split 1 fp8    585 x  4608 x  1536 bias      workspace 0         : local void ifx::gemm_q8_kernel<true, 0> 184 256 65536
small_split 1 bf16   585 x  1536 x  1536 bias      workspace none      : dma 10 - - 0 0
small_split 1 bf16   585 x  1536 x  1536 bias      workspace 0         : dma 10 - - 0 0
small_split 1 bf16   585 x  1536 x  1536 gate/1560 workspace none      : dma 10 - - 0 0
small_split 1 bf16   585 x  1536 x  1536 gate/1560 workspace 0         : dma 10 - - 0 0
small_split 1 fp8    585 x  1536 x  1536 bias      workspace 0         : local void ifx::gemm_q8_kernel<true, 0> 64 256 65536
small_split 1 bf16   585 x  8960 x  1536 bias      workspace none      : dma 13 - - 0 0
small_split 1 bf16   585 x  8960 x  1536 bias      workspace 0         : dma 13 - - 0 0
small_split 1 bf16   585 x  8960 x  1536 gate/1560 workspace none      : dma 13 - - 0 0
small_split 1 bf16   585 x  8960 x  1536 gate/1560 workspace 0         : dma 13 - - 0 0
small_split 1 fp8    585 x  8960 x  1536 bias      workspace 0         : local void ifx::gemm_q8_kernel<true, 0> 352 256 65536
small_split 1 bf16   585 x  1536 x  8960 bias      workspace none      : dma 11 - - 0 0
small_split 1 bf16   585 x  1536 x  8960 bias      workspace 0         : dma 11 - - 0 0
small_split 1 bf16   585 x  1536 x  8960 gate/1560 workspace none      : dma 11 - - 0 0
small_split 1 bf16   585 x  1536 x  8960 gate/1560 workspace 0         : dma 11 - - 0 0
small_split 1 fp8    585 x  1536 x  8960 bias      workspace 0         : local void ifx::gemm_q8_kernel<true, 0> 64 256 65536
small_split 1 bf16  1170 x  4608 x  1536 bias      workspace none      : pp - 2 1 0 0
small_split 1 bf16  1170 x  4608 x  1536 bias      workspace 0         : pp - 2 1 0 0
small_split 1 bf16  1170 x  4608 x  1536 gate/1560 workspace none      : pp - 2 1 0 0
small_split 1 bf16  1170 x  4608 x  1536 gate/1560 workspace 0         : pp - 2 1 0 0
small_split 1 fp8   1170 x  4608 x  1536 bias      workspace 0         : pp-f8 - 2 1 0 0
small_split 1 bf16  1170 x  1536 x  1536 bias      workspace none      : dma 2 - - 0 0
small_split 1 bf16  1170 x  1536 x  1536 bias      workspace 0         : dma 2 - - 0 0
small_split 1 bf16  1170 x  1536 x  1536 gate/1560 workspace none      : dma 2 - - 0 0
small_split 1 bf16  1170 x  1536 x  1536 gate/1560 workspace 0         : dma 2 - - 0 0
small_split 1 fp8   1170 x  1536 x  1536 bias      workspace 0         : pp-f8 - 2 1 0 0
small_split 1 bf16  1170 x  8960 x  1536 bias      workspace none      : pp - 3 1 0 0
small_split 1 bf16  1170 x  8960 x  1536 bias      workspace 0         : pp - 3 1 0 0
small_split 1 bf16  1170 x  8960 x  1536 gate/1560 workspace none      : pp - 3 1 0 0
small_split 1 bf16  1170 x  8960 x  1536 gate/1560 workspace 0         : pp - 3 1 0 0
small_split 1 fp8   1170 x  8960 x  1536 bias      workspace 0         : pp-f8 - 3 1 0 0
small_split 1 bf16  1170 x  1536 x  8960 bias      workspace none      : dma 2 - - 0 0
small_split 1 bf16  1170 x  1536 x  8960 bias      workspace 23597056  : pp - 2 4 1 0
small_split 1 bf16  1170 x  1536 x  8960 gate/1560 workspace none      : dma 2 - - 0 0
small_split 1 bf16  1170 x  1536 x  8960 gate/1560 workspace 23597056  : pp - 2 4 1 0
small_split 1 fp8   1170 x  1536 x  8960 bias      workspace 0         : pp-f8 - 2 1 0 0
small_split 1 bf16  2340 x  4608 x  1536 bias      workspace none      : pp - 3 1 0 0
small_split 1 bf16  2340 x  4608 x  1536 bias      workspace 0         : pp - 3 1 0 0
small_split 1 bf16  2340 x  4608 x  1536 gate/1560 workspace none      : pp - 3 1 0 0
small_split 1 bf16  2340 x  4608 x  1536 gate/1560 workspace 0         : pp - 3 1 0 0
small_split 1 fp8   2340 x  4608 x  1536 bias      workspace 0         : pp-f8 - 3 1 0 0
small_split 1 bf16  2340 x  1536 x  1536 bias      workspace none      : dma 12 - - 0 0
small_split 1 bf16  2340 x  1536 x  1536 bias      workspace 0         : dma 12 - - 0 0
small_split 1 bf16  2340 x  1536 x  1536 gate/1560 workspace none      : dma 12 - - 0 0
small_split 1 bf16  2340 x  1536 x  1536 gate/1560 workspace 0         : dma 12 - - 0 0
small_split 1 fp8   2340 x  1536 x  1536 bias      workspace 0         : pp-f8 - 2 1 0 0
small_split 1 bf16  2340 x  8960 x  1536 bias      workspace none      : pp - 3 1 0 0
small_split 1 bf16  2340 x  8960 x  1536 bias      workspace 0         : pp - 3 1 0 0
small_split 1 bf16  2340 x  8960 x  1536 gate/1560 workspace none      : pp - 3 1 0 0
small_split 1 bf16  2340 x  8960 x  1536 gate/1560 workspace 0         : pp - 3 1 0 0
small_split 1 fp8   2340 x  8960 x  1536 bias      workspace 0         : pp-f8 - 3 1 0 0
small_split 1 bf16  2340 x  1536 x  8960 bias      workspace none      : dma 12 - - 0 0
small_split 1 bf16  2340 x  1536 x  8960 bias      workspace 0         : dma 12 - - 0 0
small_split 1 bf16  2340 x  1536 x  8960 gate/1560 workspace none      : dma 12 - - 0 0
small_split 1 bf16  2340 x  1536 x  8960 gate/1560 workspace 0         : dma 12 - - 0 0
small_split 1 fp8   2340 x  1536 x  8960 bias      workspace 15732736  : pp-f8 - 4 2 1 0
small_split 0 bf16  1519 x  8192 x  3072 bias      workspace none      : pp - 3 1 0 0
small_split 0 bf16  1519 x  8192 x  3072 bias      workspace 0         : pp - 3 1 0 0
small_split 0 bf16  1519 x  8192 x  3072 gate/1560 workspace none      : pp - 3 1 0 0
small_split 0 bf16  1519 x  8192 x  3072 gate/1560 workspace 0         : pp - 3 1 0 0
small_split 0 fp8   1519 x  8192 x  3072 bias      workspace 0         : pp-f8 - 3 1 0 0
small_split 0 bf16  1519 x 12288 x  3072 bias      workspace none      : pp - 3 1 0 0
small_split 0 bf16  1519 x 12288 x  3072 bias      workspace 0         : pp - 3 1 0 0
small_split 0 bf16  1519 x 12288 x  3072 gate/1560 workspace none      : pp - 3 1 0 0
small_split 0 bf16  1519 x 12288 x  3072 gate/1560 workspace 0         : pp - 3 1 0 0
small_split 0 fp8   1519 x 12288 x  3072 bias      workspace 0         : pp-f8 - 3 1 0 0
small_split 0 bf16   512 x 20480 x  4096 bias      workspace none      : dma 19 - - 0 0
small_split 0 bf16   512 x 20480 x  4096 bias      workspace 0         : dma 19 - - 0 0
small_split 0 bf16   512 x 20480 x  4096 gate/1560 workspace none      : dma 19 - - 0 0
small_split 0 bf16   512 x 20480 x  4096 gate/1560 workspace 0         : dma 19 - - 0 0
small_split 0 fp8    512 x 20480 x  4096 bias      workspace 0         : local void ifx::gemm_q8_dma_kernel<true, 256, 128, 4, 0, 128, 3> 320 512 147456
"""


def test_gemm_plan_reproduces_the_recorded_dispatch():
    """Which kernel a GEMM call runs — launcher, tile, K split, whether the workspace is touched — for gemm_variant 0 - 29 x
    gemm_small_split 0 / 1 over 20 row counts x 19 (N, K) x six epilogues x operand alignments x workspace offers, both 8-bit formats,
    the y2 launches and the two workspace queries: tools/gemm_plan_check.cpp calls the real entry points with everything behind them
    stubbed (no GPU), and its output has to be the recorded one line for line.  A diff in a checksum line names the variant; the named
    shapes are there in full so that a mismatch at one of them is readable."""
    import shutil
    import subprocess
    import tempfile
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not present")
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "gemm_plan_check")
        b = subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-std=c++17", "-rdynamic", os.path.join(root, "tools", "gemm_plan_check.cpp"),
                            "-ldl", "-o", exe], capture_output=True, text=True, timeout=600)
        assert b.returncode == 0, b.stderr[-3000:]
        p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-1000:] + p.stderr[-1000:]
    got, want = p.stdout.splitlines(), GEMM_DISPATCH_RECORDED.splitlines()
    assert len(want) == 2 * 30 * 2 + 115
    diff = [f"recorded: {w}\n     now: {g}" for w, g in zip(want, got) if w != g]
    assert not diff and len(got) == len(want), f"{len(diff)} of {len(want)} lines differ ({len(got)} printed):\n" + "\n".join(diff[:20])


# What tools/gemm_tile_launch_check.cpp printed at the commit BEFORE the five launchers of the LDS-DMA GEMM tiles became launch_tile
# (inferix_amd/csrc/ifx_gemm_tile.h): per tile id, shape and epilogue the kernel instantiation with grid, block and dynamic LDS bytes,
# or the refusal with its text.  (Tile 17 is the register-staged four-wave tile of another file: `w4 splits`.)
GEMM_TILE_LAUNCHES_RECORDED = """\
tile  0    64 x    64 x   256 epilogue 0: void ifx::gemm_glds_kernel<0> 8 512 147456
tile  0   333 x   712 x  1536 epilogue 0: void ifx::gemm_glds_kernel<0> 16 512 147456
tile  0  2340 x  1536 x  1536 epilogue 0: void ifx::gemm_glds_kernel<0> 120 512 147456
tile  0  4680 x  4608 x  1536 epilogue 0: void ifx::gemm_glds_kernel<0> 688 512 147456
tile  0   585 x  1536 x   384 epilogue 0: void ifx::gemm_glds_kernel<0> 40 512 147456
tile  0   130 x   264 x   192 epilogue 0: void ifx::gemm_glds_kernel<0> 8 512 147456
tile  0   333 x   712 x  1536 epilogue 1: void ifx::gemm_glds_kernel<1> 16 512 147456
tile  0   333 x   712 x  1536 epilogue 2: void ifx::gemm_glds_kernel<2> 16 512 147456
tile  0   333 x   712 x  1536 epilogue 3: void ifx::gemm_glds_kernel<3> 16 512 147456
tile  0   333 x   712 x  1536 epilogue 99: rc -1 ifx_gemm_bf16(glds): unknown epilogue 99
tile  1    64 x    64 x   256 epilogue 0: void ifx::gemm_small_kernel<128, 128, 2, 0, 1> 8 256 65536
tile  1   333 x   712 x  1536 epilogue 0: void ifx::gemm_small_kernel<128, 128, 2, 0, 1> 24 256 65536
tile  1  2340 x  1536 x  1536 epilogue 0: void ifx::gemm_small_kernel<128, 128, 2, 0, 1> 232 256 65536
tile  1  4680 x  4608 x  1536 epilogue 0: void ifx::gemm_small_kernel<128, 128, 2, 0, 1> 1336 256 65536
tile  1   585 x  1536 x   384 epilogue 0: void ifx::gemm_small_kernel<128, 128, 2, 0, 1> 64 256 65536
tile  1   130 x   264 x   192 epilogue 0: void ifx::gemm_small_kernel<128, 128, 2, 0, 1> 8 256 65536
tile  1   333 x   712 x  1536 epilogue 1: void ifx::gemm_small_kernel<128, 128, 2, 1, 1> 24 256 65536
tile  1   333 x   712 x  1536 epilogue 2: void ifx::gemm_small_kernel<128, 128, 2, 2, 1> 24 256 65536
tile  1   333 x   712 x  1536 epilogue 3: void ifx::gemm_small_kernel<128, 128, 2, 3, 1> 24 256 65536
tile  1   333 x   712 x  1536 epilogue 99: rc -1 ifx_gemm_bf16(small): unknown epilogue 99
tile  2    64 x    64 x   256 epilogue 0: void ifx::gemm_small_kernel<64, 64, 4, 0, 1> 8 256 65536
tile  2   333 x   712 x  1536 epilogue 0: void ifx::gemm_small_kernel<64, 64, 4, 0, 1> 72 256 65536
tile  2  2340 x  1536 x  1536 epilogue 0: void ifx::gemm_small_kernel<64, 64, 4, 0, 1> 888 256 65536
tile  2  4680 x  4608 x  1536 epilogue 0: void ifx::gemm_small_kernel<64, 64, 4, 0, 1> 5328 256 65536
tile  2   585 x  1536 x   384 epilogue 0: void ifx::gemm_small_kernel<64, 64, 4, 0, 1> 240 256 65536
tile  2   130 x   264 x   192 epilogue 0: void ifx::gemm_small_kernel<64, 64, 4, 0, 1> 16 256 65536
tile  2   333 x   712 x  1536 epilogue 1: void ifx::gemm_small_kernel<64, 64, 4, 1, 1> 72 256 65536
tile  2   333 x   712 x  1536 epilogue 2: void ifx::gemm_small_kernel<64, 64, 4, 2, 1> 72 256 65536
tile  2   333 x   712 x  1536 epilogue 3: void ifx::gemm_small_kernel<64, 64, 4, 3, 1> 72 256 65536
tile  2   333 x   712 x  1536 epilogue 99: rc -1 ifx_gemm_bf16(small): unknown epilogue 99
tile  3    64 x    64 x   256 epilogue 0: void ifx::gemm_big_kernel<256, 256, 2, 2, 0, 64> 8 512 131072
tile  3   333 x   712 x  1536 epilogue 0: void ifx::gemm_big_kernel<256, 256, 2, 2, 0, 64> 8 512 131072
tile  3  2340 x  1536 x  1536 epilogue 0: void ifx::gemm_big_kernel<256, 256, 2, 2, 0, 64> 64 512 131072
tile  3  4680 x  4608 x  1536 epilogue 0: void ifx::gemm_big_kernel<256, 256, 2, 2, 0, 64> 344 512 131072
tile  3   585 x  1536 x   384 epilogue 0: void ifx::gemm_big_kernel<256, 256, 2, 2, 0, 64> 24 512 131072
tile  3   130 x   264 x   192 epilogue 0: void ifx::gemm_big_kernel<256, 256, 2, 2, 0, 64> 8 512 131072
tile  3   333 x   712 x  1536 epilogue 1: void ifx::gemm_big_kernel<256, 256, 2, 2, 1, 64> 8 512 131072
tile  3   333 x   712 x  1536 epilogue 2: void ifx::gemm_big_kernel<256, 256, 2, 2, 2, 64> 8 512 131072
tile  3   333 x   712 x  1536 epilogue 3: void ifx::gemm_big_kernel<256, 256, 2, 2, 3, 64> 8 512 131072
tile  3   333 x   712 x  1536 epilogue 99: rc -1 ifx_gemm_bf16(k32): unknown epilogue 99
tile  4    64 x    64 x   256 epilogue 0: void ifx::gemm_small_kernel<128, 64, 3, 0, 1> 8 256 73728
tile  4   333 x   712 x  1536 epilogue 0: void ifx::gemm_small_kernel<128, 64, 3, 0, 1> 40 256 73728
tile  4  2340 x  1536 x  1536 epilogue 0: void ifx::gemm_small_kernel<128, 64, 3, 0, 1> 456 256 73728
tile  4  4680 x  4608 x  1536 epilogue 0: void ifx::gemm_small_kernel<128, 64, 3, 0, 1> 2664 256 73728
tile  4   585 x  1536 x   384 epilogue 0: void ifx::gemm_small_kernel<128, 64, 3, 0, 1> 120 256 73728
tile  4   130 x   264 x   192 epilogue 0: void ifx::gemm_small_kernel<128, 64, 3, 0, 1> 16 256 73728
tile  4   333 x   712 x  1536 epilogue 1: void ifx::gemm_small_kernel<128, 64, 3, 1, 1> 40 256 73728
tile  4   333 x   712 x  1536 epilogue 2: void ifx::gemm_small_kernel<128, 64, 3, 2, 1> 40 256 73728
tile  4   333 x   712 x  1536 epilogue 3: void ifx::gemm_small_kernel<128, 64, 3, 3, 1> 40 256 73728
tile  4   333 x   712 x  1536 epilogue 99: rc -1 ifx_gemm_bf16(small): unknown epilogue 99
tile  5    64 x    64 x   256 epilogue 0: void ifx::gemm_big_kernel<256, 128, 2, 2, 0, 32> 8 512 65536
tile  5   333 x   712 x  1536 epilogue 0: void ifx::gemm_big_kernel<256, 128, 2, 2, 0, 32> 16 512 65536
tile  5  2340 x  1536 x  1536 epilogue 0: void ifx::gemm_big_kernel<256, 128, 2, 2, 0, 32> 120 512 65536
tile  5  4680 x  4608 x  1536 epilogue 0: void ifx::gemm_big_kernel<256, 128, 2, 2, 0, 32> 688 512 65536
tile  5   585 x  1536 x   384 epilogue 0: void ifx::gemm_big_kernel<256, 128, 2, 2, 0, 32> 40 512 65536
tile  5   130 x   264 x   192 epilogue 0: void ifx::gemm_big_kernel<256, 128, 2, 2, 0, 32> 8 512 65536
tile  5   333 x   712 x  1536 epilogue 1: void ifx::gemm_big_kernel<256, 128, 2, 2, 1, 32> 16 512 65536
tile  5   333 x   712 x  1536 epilogue 2: void ifx::gemm_big_kernel<256, 128, 2, 2, 2, 32> 16 512 65536
tile  5   333 x   712 x  1536 epilogue 3: void ifx::gemm_big_kernel<256, 128, 2, 2, 3, 32> 16 512 65536
tile  5   333 x   712 x  1536 epilogue 99: rc -1 ifx_gemm_bf16(k32): unknown epilogue 99
tile  6    64 x    64 x   256 epilogue 0: void ifx::gemm_big_kernel<128, 128, 2, 2, 0, 32> 8 512 32768
tile  6   333 x   712 x  1536 epilogue 0: void ifx::gemm_big_kernel<128, 128, 2, 2, 0, 32> 24 512 32768
tile  6  2340 x  1536 x  1536 epilogue 0: void ifx::gemm_big_kernel<128, 128, 2, 2, 0, 32> 232 512 32768
tile  6  4680 x  4608 x  1536 epilogue 0: void ifx::gemm_big_kernel<128, 128, 2, 2, 0, 32> 1336 512 32768
tile  6   585 x  1536 x   384 epilogue 0: void ifx::gemm_big_kernel<128, 128, 2, 2, 0, 32> 64 512 32768
tile  6   130 x   264 x   192 epilogue 0: void ifx::gemm_big_kernel<128, 128, 2, 2, 0, 32> 8 512 32768
tile  6   333 x   712 x  1536 epilogue 1: void ifx::gemm_big_kernel<128, 128, 2, 2, 1, 32> 24 512 32768
tile  6   333 x   712 x  1536 epilogue 2: void ifx::gemm_big_kernel<128, 128, 2, 2, 2, 32> 24 512 32768
tile  6   333 x   712 x  1536 epilogue 3: void ifx::gemm_big_kernel<128, 128, 2, 2, 3, 32> 24 512 32768
tile  6   333 x   712 x  1536 epilogue 99: rc -1 ifx_gemm_bf16(k32): unknown epilogue 99
tile  7    64 x    64 x   256 epilogue 0: void ifx::gemm_ws_kernel<256, 128, 3, 0> 8 512 147456
tile  7   333 x   712 x  1536 epilogue 0: void ifx::gemm_ws_kernel<256, 128, 3, 0> 16 512 147456
tile  7  2340 x  1536 x  1536 epilogue 0: void ifx::gemm_ws_kernel<256, 128, 3, 0> 120 512 147456
tile  7  4680 x  4608 x  1536 epilogue 0: void ifx::gemm_ws_kernel<256, 128, 3, 0> 688 512 147456
tile  7   585 x  1536 x   384 epilogue 0: void ifx::gemm_ws_kernel<256, 128, 3, 0> 40 512 147456
tile  7   130 x   264 x   192 epilogue 0: void ifx::gemm_ws_kernel<256, 128, 3, 0> 8 512 147456
tile  7   333 x   712 x  1536 epilogue 1: void ifx::gemm_ws_kernel<256, 128, 3, 1> 16 512 147456
tile  7   333 x   712 x  1536 epilogue 2: void ifx::gemm_ws_kernel<256, 128, 3, 2> 16 512 147456
tile  7   333 x   712 x  1536 epilogue 3: void ifx::gemm_ws_kernel<256, 128, 3, 3> 16 512 147456
tile  7   333 x   712 x  1536 epilogue 99: rc -1 ifx_gemm_bf16(ws): unknown epilogue 99
tile  8    64 x    64 x   256 epilogue 0: void ifx::gemm_ws_kernel<128, 128, 2, 0> 8 512 65536
tile  8   333 x   712 x  1536 epilogue 0: void ifx::gemm_ws_kernel<128, 128, 2, 0> 24 512 65536
tile  8  2340 x  1536 x  1536 epilogue 0: void ifx::gemm_ws_kernel<128, 128, 2, 0> 232 512 65536
tile  8  4680 x  4608 x  1536 epilogue 0: void ifx::gemm_ws_kernel<128, 128, 2, 0> 1336 512 65536
tile  8   585 x  1536 x   384 epilogue 0: void ifx::gemm_ws_kernel<128, 128, 2, 0> 64 512 65536
tile  8   130 x   264 x   192 epilogue 0: void ifx::gemm_ws_kernel<128, 128, 2, 0> 8 512 65536
tile  8   333 x   712 x  1536 epilogue 1: void ifx::gemm_ws_kernel<128, 128, 2, 1> 24 512 65536
tile  8   333 x   712 x  1536 epilogue 2: void ifx::gemm_ws_kernel<128, 128, 2, 2> 24 512 65536
tile  8   333 x   712 x  1536 epilogue 3: void ifx::gemm_ws_kernel<128, 128, 2, 3> 24 512 65536
tile  8   333 x   712 x  1536 epilogue 99: rc -1 ifx_gemm_bf16(ws): unknown epilogue 99
tile  9    64 x    64 x   256 epilogue 0: void ifx::gemm_big_kernel<256, 256, 2, 4, 0, 32> 8 512 131072
tile  9   333 x   712 x  1536 epilogue 0: void ifx::gemm_big_kernel<256, 256, 2, 4, 0, 32> 8 512 131072
tile  9  2340 x  1536 x  1536 epilogue 0: void ifx::gemm_big_kernel<256, 256, 2, 4, 0, 32> 64 512 131072
tile  9  4680 x  4608 x  1536 epilogue 0: void ifx::gemm_big_kernel<256, 256, 2, 4, 0, 32> 344 512 131072
tile  9   585 x  1536 x   384 epilogue 0: void ifx::gemm_big_kernel<256, 256, 2, 4, 0, 32> 24 512 131072
tile  9   130 x   264 x   192 epilogue 0: void ifx::gemm_big_kernel<256, 256, 2, 4, 0, 32> 8 512 131072
tile  9   333 x   712 x  1536 epilogue 1: void ifx::gemm_big_kernel<256, 256, 2, 4, 1, 32> 8 512 131072
tile  9   333 x   712 x  1536 epilogue 2: void ifx::gemm_big_kernel<256, 256, 2, 4, 2, 32> 8 512 131072
tile  9   333 x   712 x  1536 epilogue 3: void ifx::gemm_big_kernel<256, 256, 2, 4, 3, 32> 8 512 131072
tile  9   333 x   712 x  1536 epilogue 99: rc -1 ifx_gemm_bf16(k32): unknown epilogue 99
tile 10    64 x    64 x   256 epilogue 0: void ifx::gemm_small_kernel<64, 64, 2, 0, 4> 8 1024 131072
tile 10   333 x   712 x  1536 epilogue 0: void ifx::gemm_small_kernel<64, 64, 2, 0, 4> 72 1024 131072
tile 10  2340 x  1536 x  1536 epilogue 0: void ifx::gemm_small_kernel<64, 64, 2, 0, 4> 888 1024 131072
tile 10  4680 x  4608 x  1536 epilogue 0: void ifx::gemm_small_kernel<64, 64, 2, 0, 4> 5328 1024 131072
tile 10   585 x  1536 x   384 epilogue 0: rc -1 ifx_gemm_bf16: K/64 = 6 is not a multiple of the 4 K-groups of this tile
tile 10   130 x   264 x   192 epilogue 0: rc -1 ifx_gemm_bf16: K/64 = 3 is not a multiple of the 4 K-groups of this tile
tile 10   333 x   712 x  1536 epilogue 1: void ifx::gemm_small_kernel<64, 64, 2, 1, 4> 72 1024 131072
tile 10   333 x   712 x  1536 epilogue 2: void ifx::gemm_small_kernel<64, 64, 2, 2, 4> 72 1024 131072
tile 10   333 x   712 x  1536 epilogue 3: void ifx::gemm_small_kernel<64, 64, 2, 3, 4> 72 1024 131072
tile 10   333 x   712 x  1536 epilogue 99: rc -1 ifx_gemm_bf16(small): unknown epilogue 99
tile 11    64 x    64 x   256 epilogue 0: void ifx::gemm_small_kernel<64, 64, 4, 0, 2> 8 512 131072
tile 11   333 x   712 x  1536 epilogue 0: void ifx::gemm_small_kernel<64, 64, 4, 0, 2> 72 512 131072
tile 11  2340 x  1536 x  1536 epilogue 0: void ifx::gemm_small_kernel<64, 64, 4, 0, 2> 888 512 131072
tile 11  4680 x  4608 x  1536 epilogue 0: void ifx::gemm_small_kernel<64, 64, 4, 0, 2> 5328 512 131072
tile 11   585 x  1536 x   384 epilogue 0: void ifx::gemm_small_kernel<64, 64, 4, 0, 2> 240 512 131072
tile 11   130 x   264 x   192 epilogue 0: rc -1 ifx_gemm_bf16: K/64 = 3 is not a multiple of the 2 K-groups of this tile
tile 11   333 x   712 x  1536 epilogue 1: void ifx::gemm_small_kernel<64, 64, 4, 1, 2> 72 512 131072
tile 11   333 x   712 x  1536 epilogue 2: void ifx::gemm_small_kernel<64, 64, 4, 2, 2> 72 512 131072
tile 11   333 x   712 x  1536 epilogue 3: void ifx::gemm_small_kernel<64, 64, 4, 3, 2> 72 512 131072
tile 11   333 x   712 x  1536 epilogue 99: rc -1 ifx_gemm_bf16(small): unknown epilogue 99
tile 12    64 x    64 x   256 epilogue 0: void ifx::gemm_small_kernel<128, 128, 2, 0, 2> 8 512 131072
tile 12   333 x   712 x  1536 epilogue 0: void ifx::gemm_small_kernel<128, 128, 2, 0, 2> 24 512 131072
tile 12  2340 x  1536 x  1536 epilogue 0: void ifx::gemm_small_kernel<128, 128, 2, 0, 2> 232 512 131072
tile 12  4680 x  4608 x  1536 epilogue 0: void ifx::gemm_small_kernel<128, 128, 2, 0, 2> 1336 512 131072
tile 12   585 x  1536 x   384 epilogue 0: void ifx::gemm_small_kernel<128, 128, 2, 0, 2> 64 512 131072
tile 12   130 x   264 x   192 epilogue 0: rc -1 ifx_gemm_bf16: K/64 = 3 is not a multiple of the 2 K-groups of this tile
tile 12   333 x   712 x  1536 epilogue 1: void ifx::gemm_small_kernel<128, 128, 2, 1, 2> 24 512 131072
tile 12   333 x   712 x  1536 epilogue 2: void ifx::gemm_small_kernel<128, 128, 2, 2, 2> 24 512 131072
tile 12   333 x   712 x  1536 epilogue 3: void ifx::gemm_small_kernel<128, 128, 2, 3, 2> 24 512 131072
tile 12   333 x   712 x  1536 epilogue 99: rc -1 ifx_gemm_bf16(small): unknown epilogue 99
tile 13    64 x    64 x   256 epilogue 0: void ifx::gemm_small_kernel<128, 64, 2, 0, 1> 8 256 49152
tile 13   333 x   712 x  1536 epilogue 0: void ifx::gemm_small_kernel<128, 64, 2, 0, 1> 40 256 49152
tile 13  2340 x  1536 x  1536 epilogue 0: void ifx::gemm_small_kernel<128, 64, 2, 0, 1> 456 256 49152
tile 13  4680 x  4608 x  1536 epilogue 0: void ifx::gemm_small_kernel<128, 64, 2, 0, 1> 2664 256 49152
tile 13   585 x  1536 x   384 epilogue 0: void ifx::gemm_small_kernel<128, 64, 2, 0, 1> 120 256 49152
tile 13   130 x   264 x   192 epilogue 0: void ifx::gemm_small_kernel<128, 64, 2, 0, 1> 16 256 49152
tile 13   333 x   712 x  1536 epilogue 1: void ifx::gemm_small_kernel<128, 64, 2, 1, 1> 40 256 49152
tile 13   333 x   712 x  1536 epilogue 2: void ifx::gemm_small_kernel<128, 64, 2, 2, 1> 40 256 49152
tile 13   333 x   712 x  1536 epilogue 3: void ifx::gemm_small_kernel<128, 64, 2, 3, 1> 40 256 49152
tile 13   333 x   712 x  1536 epilogue 99: rc -1 ifx_gemm_bf16(small): unknown epilogue 99
tile 14    64 x    64 x   256 epilogue 0: void ifx::gemm_small_kernel<64, 128, 2, 0, 1> 8 256 49152
tile 14   333 x   712 x  1536 epilogue 0: void ifx::gemm_small_kernel<64, 128, 2, 0, 1> 40 256 49152
tile 14  2340 x  1536 x  1536 epilogue 0: void ifx::gemm_small_kernel<64, 128, 2, 0, 1> 448 256 49152
tile 14  4680 x  4608 x  1536 epilogue 0: void ifx::gemm_small_kernel<64, 128, 2, 0, 1> 2664 256 49152
tile 14   585 x  1536 x   384 epilogue 0: void ifx::gemm_small_kernel<64, 128, 2, 0, 1> 120 256 49152
tile 14   130 x   264 x   192 epilogue 0: void ifx::gemm_small_kernel<64, 128, 2, 0, 1> 16 256 49152
tile 14   333 x   712 x  1536 epilogue 1: void ifx::gemm_small_kernel<64, 128, 2, 1, 1> 40 256 49152
tile 14   333 x   712 x  1536 epilogue 2: void ifx::gemm_small_kernel<64, 128, 2, 2, 1> 40 256 49152
tile 14   333 x   712 x  1536 epilogue 3: void ifx::gemm_small_kernel<64, 128, 2, 3, 1> 40 256 49152
tile 14   333 x   712 x  1536 epilogue 99: rc -1 ifx_gemm_bf16(small): unknown epilogue 99
tile 15    64 x    64 x   256 epilogue 0: void ifx::gemm_small_kernel<64, 128, 3, 0, 1> 8 256 73728
tile 15   333 x   712 x  1536 epilogue 0: void ifx::gemm_small_kernel<64, 128, 3, 0, 1> 40 256 73728
tile 15  2340 x  1536 x  1536 epilogue 0: void ifx::gemm_small_kernel<64, 128, 3, 0, 1> 448 256 73728
tile 15  4680 x  4608 x  1536 epilogue 0: void ifx::gemm_small_kernel<64, 128, 3, 0, 1> 2664 256 73728
tile 15   585 x  1536 x   384 epilogue 0: void ifx::gemm_small_kernel<64, 128, 3, 0, 1> 120 256 73728
tile 15   130 x   264 x   192 epilogue 0: void ifx::gemm_small_kernel<64, 128, 3, 0, 1> 16 256 73728
tile 15   333 x   712 x  1536 epilogue 1: void ifx::gemm_small_kernel<64, 128, 3, 1, 1> 40 256 73728
tile 15   333 x   712 x  1536 epilogue 2: void ifx::gemm_small_kernel<64, 128, 3, 2, 1> 40 256 73728
tile 15   333 x   712 x  1536 epilogue 3: void ifx::gemm_small_kernel<64, 128, 3, 3, 1> 40 256 73728
tile 15   333 x   712 x  1536 epilogue 99: rc -1 ifx_gemm_bf16(small): unknown epilogue 99
tile 16    64 x    64 x   256 epilogue 0: void ifx::gemm_small_kernel<256, 256, 2, 0, 1> 8 256 131072
tile 16   333 x   712 x  1536 epilogue 0: void ifx::gemm_small_kernel<256, 256, 2, 0, 1> 8 256 131072
tile 16  2340 x  1536 x  1536 epilogue 0: void ifx::gemm_small_kernel<256, 256, 2, 0, 1> 64 256 131072
tile 16  4680 x  4608 x  1536 epilogue 0: void ifx::gemm_small_kernel<256, 256, 2, 0, 1> 344 256 131072
tile 16   585 x  1536 x   384 epilogue 0: void ifx::gemm_small_kernel<256, 256, 2, 0, 1> 24 256 131072
tile 16   130 x   264 x   192 epilogue 0: void ifx::gemm_small_kernel<256, 256, 2, 0, 1> 8 256 131072
tile 16   333 x   712 x  1536 epilogue 1: void ifx::gemm_small_kernel<256, 256, 2, 1, 1> 8 256 131072
tile 16   333 x   712 x  1536 epilogue 2: void ifx::gemm_small_kernel<256, 256, 2, 2, 1> 8 256 131072
tile 16   333 x   712 x  1536 epilogue 3: void ifx::gemm_small_kernel<256, 256, 2, 3, 1> 8 256 131072
tile 16   333 x   712 x  1536 epilogue 99: rc -1 ifx_gemm_bf16(small): unknown epilogue 99
tile 17    64 x    64 x   256 epilogue 0: w4 1
tile 17   333 x   712 x  1536 epilogue 0: w4 1
tile 17  2340 x  1536 x  1536 epilogue 0: w4 1
tile 17  4680 x  4608 x  1536 epilogue 0: w4 1
tile 17   585 x  1536 x   384 epilogue 0: w4 1
tile 17   130 x   264 x   192 epilogue 0: w4 1
tile 17   333 x   712 x  1536 epilogue 1: w4 1
tile 17   333 x   712 x  1536 epilogue 2: w4 1
tile 17   333 x   712 x  1536 epilogue 3: w4 1
tile 17   333 x   712 x  1536 epilogue 99: w4 1
tile 18    64 x    64 x   256 epilogue 0: void ifx::gemm_small_kernel<64, 64, 4, 0, 1> 8 256 65536
tile 18   333 x   712 x  1536 epilogue 0: void ifx::gemm_small_kernel<64, 64, 4, 0, 1> 72 256 65536
tile 18  2340 x  1536 x  1536 epilogue 0: void ifx::gemm_small_kernel<64, 64, 4, 0, 1> 888 256 65536
tile 18  4680 x  4608 x  1536 epilogue 0: void ifx::gemm_small_kernel<64, 64, 4, 0, 1> 5328 256 65536
tile 18   585 x  1536 x   384 epilogue 0: void ifx::gemm_small_kernel<64, 64, 4, 0, 1> 240 256 65536
tile 18   130 x   264 x   192 epilogue 0: void ifx::gemm_small_kernel<64, 64, 4, 0, 1> 16 256 65536
tile 18   333 x   712 x  1536 epilogue 1: void ifx::gemm_small_kernel<64, 64, 4, 1, 1> 72 256 65536
tile 18   333 x   712 x  1536 epilogue 2: void ifx::gemm_small_kernel<64, 64, 4, 2, 1> 72 256 65536
tile 18   333 x   712 x  1536 epilogue 3: void ifx::gemm_small_kernel<64, 64, 4, 3, 1> 72 256 65536
tile 18   333 x   712 x  1536 epilogue 99: rc -1 ifx_gemm_bf16(small): unknown epilogue 99
tile 19    64 x    64 x   256 epilogue 0: void ifx::gemm_big_kernel<256, 192, 4, 2, 0, 64> 8 512 114688
tile 19   333 x   712 x  1536 epilogue 0: void ifx::gemm_big_kernel<256, 192, 4, 2, 0, 64> 8 512 114688
tile 19  2340 x  1536 x  1536 epilogue 0: void ifx::gemm_big_kernel<256, 192, 4, 2, 0, 64> 80 512 114688
tile 19  4680 x  4608 x  1536 epilogue 0: void ifx::gemm_big_kernel<256, 192, 4, 2, 0, 64> 456 512 114688
tile 19   585 x  1536 x   384 epilogue 0: void ifx::gemm_big_kernel<256, 192, 4, 2, 0, 64> 24 512 114688
tile 19   130 x   264 x   192 epilogue 0: void ifx::gemm_big_kernel<256, 192, 4, 2, 0, 64> 8 512 114688
tile 19   333 x   712 x  1536 epilogue 1: void ifx::gemm_big_kernel<256, 192, 4, 2, 1, 64> 8 512 114688
tile 19   333 x   712 x  1536 epilogue 2: void ifx::gemm_big_kernel<256, 192, 4, 2, 2, 64> 8 512 114688
tile 19   333 x   712 x  1536 epilogue 3: void ifx::gemm_big_kernel<256, 192, 4, 2, 3, 64> 8 512 114688
tile 19   333 x   712 x  1536 epilogue 99: rc -1 ifx_gemm_bf16(k32): unknown epilogue 99
tile 25    64 x    64 x   256 epilogue 0: void ifx::gemm_small_kernel<64, 64, 4, 0, 1> 8 256 65536
tile 25   333 x   712 x  1536 epilogue 0: void ifx::gemm_small_kernel<64, 64, 4, 0, 1> 72 256 65536
tile 25  2340 x  1536 x  1536 epilogue 0: void ifx::gemm_small_kernel<64, 64, 4, 0, 1> 888 256 65536
tile 25  4680 x  4608 x  1536 epilogue 0: void ifx::gemm_small_kernel<64, 64, 4, 0, 1> 5328 256 65536
tile 25   585 x  1536 x   384 epilogue 0: void ifx::gemm_small_kernel<64, 64, 4, 0, 1> 240 256 65536
tile 25   130 x   264 x   192 epilogue 0: void ifx::gemm_small_kernel<64, 64, 4, 0, 1> 16 256 65536
tile 25   333 x   712 x  1536 epilogue 1: void ifx::gemm_small_kernel<64, 64, 4, 1, 1> 72 256 65536
tile 25   333 x   712 x  1536 epilogue 2: void ifx::gemm_small_kernel<64, 64, 4, 2, 1> 72 256 65536
tile 25   333 x   712 x  1536 epilogue 3: void ifx::gemm_small_kernel<64, 64, 4, 3, 1> 72 256 65536
tile 25   333 x   712 x  1536 epilogue 99: rc -1 ifx_gemm_bf16(small): unknown epilogue 99
"""


def test_lds_dma_gemm_tiles_launch_with_the_recorded_parameters():
    """Every tile id 0 - 19 of launch_gemm_lds_dma and one id without a name, over a one-tile shape, ragged edges, tile counts the
    eight XCDs do not divide and K/64 that the K-groups of a tile do not divide, with the four epilogues and an unknown one:
    tools/gemm_tile_launch_check.cpp calls the real launcher with the runtime stubbed (no GPU), and the kernel instantiation, grid,
    block and LDS bytes of every launch and the text of every refusal have to be the recorded ones line for line."""
    import shutil
    import subprocess
    import tempfile
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not present")
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "gemm_tile_launch_check")
        b = subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-std=c++17", "-rdynamic", os.path.join(root, "tools", "gemm_tile_launch_check.cpp"),
                            "-ldl", "-o", exe], capture_output=True, text=True, timeout=600)
        assert b.returncode == 0, b.stderr[-3000:]
        p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-1000:] + p.stderr[-1000:]
    got, want = p.stdout.splitlines(), GEMM_TILE_LAUNCHES_RECORDED.splitlines()
    assert len(want) == 21 * (6 + 4)
    diff = [f"recorded: {w}\n     now: {g}" for w, g in zip(want, got) if w != g]
    assert not diff and len(got) == len(want), f"{len(diff)} of {len(want)} lines differ ({len(got)} printed):\n" + "\n".join(diff[:20])


# What tools/conv_plan_check.cpp printed at the commit BEFORE the decisions of ifx_conv3d_cl and ifx_rmsnorm_cl moved into
# inferix_amd/csrc/ifx_conv_plan.h: the kernel instantiation with grid, block and dynamic LDS bytes, or the refusal with its text.  A line
# of the first block stands for 18 calls (in_planar 0 / 1 x three t_out x 256 / 304 / 64 CUs) that agreed on kernel, block and LDS: `*` is
# the grid, and the nine grids follow; a norm line for three pixel counts (1, 4095, 3 x 60 x 104).  The ten lines from "in_frame_stride + 4"
# to "cout 20: in_frame_stride + 4" came later, with the alignment contract of ifx_conv3d_desc (no earlier line changed).
CONV_PLAN_RECORDED = """\
conv cout   3 ks 1 ups 0 kt 1 variant 0  8x64 : void ifx::conv::conv_cl_kernel<32, 0, 1> * 512 73728 grids t1 8/8/8 t3 8/8/8 t16 16/16/16
conv cout   3 ks 1 ups 0 kt 1 variant 0 13x70 : void ifx::conv::conv_cl_kernel<32, 0, 1> * 512 73728 grids t1 8/8/8 t3 16/16/16 t16 64/64/64
conv cout   3 ks 1 ups 0 kt 1 variant 0 60x104: void ifx::conv::conv_cl_kernel<32, 0, 1> * 512 73728 grids t1 16/16/16 t3 48/48/48 t16 256/256/256
conv cout   3 ks 1 ups 0 kt 1 variant 1  8x64 : void ifx::conv::conv_cl_kernel<32, 0, 1> * 512 73728 grids t1 8/8/8 t3 8/8/8 t16 16/16/16
conv cout   3 ks 1 ups 0 kt 1 variant 1 13x70 : void ifx::conv::conv_cl_kernel<32, 0, 1> * 512 73728 grids t1 8/8/8 t3 16/16/16 t16 64/64/64
conv cout   3 ks 1 ups 0 kt 1 variant 1 60x104: void ifx::conv::conv_cl_kernel<32, 0, 1> * 512 73728 grids t1 16/16/16 t3 48/48/48 t16 256/256/256
conv cout   3 ks 1 ups 0 kt 3 variant 0  8x64 : void ifx::conv::conv_cl_kernel<32, 0, 1> * 512 73728 grids t1 8/8/8 t3 8/8/8 t14 16/16/16
conv cout   3 ks 1 ups 0 kt 3 variant 0 13x70 : void ifx::conv::conv_cl_kernel<32, 0, 1> * 512 73728 grids t1 8/8/8 t3 16/16/16 t14 56/56/56
conv cout   3 ks 1 ups 0 kt 3 variant 0 60x104: void ifx::conv::conv_cl_kernel<32, 0, 1> * 512 73728 grids t1 16/16/16 t3 48/48/48 t14 224/224/224
conv cout   3 ks 1 ups 0 kt 3 variant 1  8x64 : void ifx::conv::conv_cl_kernel<32, 0, 1> * 512 73728 grids t1 8/8/8 t3 8/8/8 t14 16/16/16
conv cout   3 ks 1 ups 0 kt 3 variant 1 13x70 : void ifx::conv::conv_cl_kernel<32, 0, 1> * 512 73728 grids t1 8/8/8 t3 16/16/16 t14 56/56/56
conv cout   3 ks 1 ups 0 kt 3 variant 1 60x104: void ifx::conv::conv_cl_kernel<32, 0, 1> * 512 73728 grids t1 16/16/16 t3 48/48/48 t14 224/224/224
conv cout   3 ks 3 ups 0 kt 1 variant 0  8x64 : void ifx::conv::conv_cl_kernel<32, 0, 3> * 512 108544 grids t1 8/8/8 t3 8/8/8 t16 16/16/16
conv cout   3 ks 3 ups 0 kt 1 variant 0 13x70 : void ifx::conv::conv_cl_kernel<32, 0, 3> * 512 108544 grids t1 8/8/8 t3 16/16/16 t16 64/64/64
conv cout   3 ks 3 ups 0 kt 1 variant 0 60x104: void ifx::conv::conv_cl_kernel<32, 0, 3> * 512 108544 grids t1 16/16/16 t3 48/48/48 t16 256/256/256
conv cout   3 ks 3 ups 0 kt 1 variant 1  8x64 : void ifx::conv::conv_cl_kernel<32, 0, 3> * 512 108544 grids t1 8/8/8 t3 8/8/8 t16 16/16/16
conv cout   3 ks 3 ups 0 kt 1 variant 1 13x70 : void ifx::conv::conv_cl_kernel<32, 0, 3> * 512 108544 grids t1 8/8/8 t3 16/16/16 t16 64/64/64
conv cout   3 ks 3 ups 0 kt 1 variant 1 60x104: void ifx::conv::conv_cl_kernel<32, 0, 3> * 512 108544 grids t1 16/16/16 t3 48/48/48 t16 256/256/256
conv cout   3 ks 3 ups 0 kt 3 variant 0  8x64 : void ifx::conv::conv_cl_kernel<32, 0, 3> * 512 108544 grids t1 8/8/8 t3 8/8/8 t14 16/16/16
conv cout   3 ks 3 ups 0 kt 3 variant 0 13x70 : void ifx::conv::conv_cl_kernel<32, 0, 3> * 512 108544 grids t1 8/8/8 t3 16/16/16 t14 56/56/56
conv cout   3 ks 3 ups 0 kt 3 variant 0 60x104: void ifx::conv::conv_cl_kernel<32, 0, 3> * 512 108544 grids t1 16/16/16 t3 48/48/48 t14 224/224/224
conv cout   3 ks 3 ups 0 kt 3 variant 1  8x64 : void ifx::conv::conv_cl_kernel<32, 0, 3> * 512 108544 grids t1 8/8/8 t3 8/8/8 t14 16/16/16
conv cout   3 ks 3 ups 0 kt 3 variant 1 13x70 : void ifx::conv::conv_cl_kernel<32, 0, 3> * 512 108544 grids t1 8/8/8 t3 16/16/16 t14 56/56/56
conv cout   3 ks 3 ups 0 kt 3 variant 1 60x104: void ifx::conv::conv_cl_kernel<32, 0, 3> * 512 108544 grids t1 16/16/16 t3 48/48/48 t14 224/224/224
conv cout   3 ks 3 ups 1 kt 1 variant 0  8x64 : void ifx::conv::conv_cl_kernel<32, 1, 3> * 512 49152 grids t1 8/8/8 t3 16/16/16 t16 64/64/64
conv cout   3 ks 3 ups 1 kt 1 variant 0 13x70 : void ifx::conv::conv_cl_kernel<32, 1, 3> * 512 49152 grids t1 16/16/16 t3 40/40/40 t16 192/192/192
conv cout   3 ks 3 ups 1 kt 1 variant 0 60x104: void ifx::conv::conv_cl_kernel<32, 1, 3> * 512 49152 grids t1 64/64/64 t3 184/184/184 t16 960/960/960
conv cout   3 ks 3 ups 1 kt 1 variant 1  8x64 : void ifx::conv::conv_cl_kernel<32, 1, 3> * 512 49152 grids t1 8/8/8 t3 16/16/16 t16 64/64/64
conv cout   3 ks 3 ups 1 kt 1 variant 1 13x70 : void ifx::conv::conv_cl_kernel<32, 1, 3> * 512 49152 grids t1 16/16/16 t3 40/40/40 t16 192/192/192
conv cout   3 ks 3 ups 1 kt 1 variant 1 60x104: void ifx::conv::conv_cl_kernel<32, 1, 3> * 512 49152 grids t1 64/64/64 t3 184/184/184 t16 960/960/960
conv cout   3 ks 3 ups 1 kt 3 variant 0  8x64 : void ifx::conv::conv_cl_kernel<32, 1, 3> * 512 49152 grids t1 8/8/8 t3 16/16/16 t14 56/56/56
conv cout   3 ks 3 ups 1 kt 3 variant 0 13x70 : void ifx::conv::conv_cl_kernel<32, 1, 3> * 512 49152 grids t1 16/16/16 t3 40/40/40 t14 168/168/168
conv cout   3 ks 3 ups 1 kt 3 variant 0 60x104: void ifx::conv::conv_cl_kernel<32, 1, 3> * 512 49152 grids t1 64/64/64 t3 184/184/184 t14 840/840/840
conv cout   3 ks 3 ups 1 kt 3 variant 1  8x64 : void ifx::conv::conv_cl_kernel<32, 1, 3> * 512 49152 grids t1 8/8/8 t3 16/16/16 t14 56/56/56
conv cout   3 ks 3 ups 1 kt 3 variant 1 13x70 : void ifx::conv::conv_cl_kernel<32, 1, 3> * 512 49152 grids t1 16/16/16 t3 40/40/40 t14 168/168/168
conv cout   3 ks 3 ups 1 kt 3 variant 1 60x104: void ifx::conv::conv_cl_kernel<32, 1, 3> * 512 49152 grids t1 64/64/64 t3 184/184/184 t14 840/840/840
conv cout  16 ks 1 ups 0 kt 1 variant 0  8x64 : void ifx::conv::conv_cl_kernel<32, 0, 1> * 512 73728 grids t1 8/8/8 t3 8/8/8 t16 16/16/16
conv cout  16 ks 1 ups 0 kt 1 variant 0 13x70 : void ifx::conv::conv_cl_kernel<32, 0, 1> * 512 73728 grids t1 8/8/8 t3 16/16/16 t16 64/64/64
conv cout  16 ks 1 ups 0 kt 1 variant 0 60x104: void ifx::conv::conv_cl_kernel<32, 0, 1> * 512 73728 grids t1 16/16/16 t3 48/48/48 t16 256/256/256
conv cout  16 ks 1 ups 0 kt 1 variant 1  8x64 : void ifx::conv::conv_cl_kernel<32, 0, 1> * 512 73728 grids t1 8/8/8 t3 8/8/8 t16 16/16/16
conv cout  16 ks 1 ups 0 kt 1 variant 1 13x70 : void ifx::conv::conv_cl_kernel<32, 0, 1> * 512 73728 grids t1 8/8/8 t3 16/16/16 t16 64/64/64
conv cout  16 ks 1 ups 0 kt 1 variant 1 60x104: void ifx::conv::conv_cl_kernel<32, 0, 1> * 512 73728 grids t1 16/16/16 t3 48/48/48 t16 256/256/256
conv cout  16 ks 1 ups 0 kt 3 variant 0  8x64 : void ifx::conv::conv_cl_kernel<32, 0, 1> * 512 73728 grids t1 8/8/8 t3 8/8/8 t14 16/16/16
conv cout  16 ks 1 ups 0 kt 3 variant 0 13x70 : void ifx::conv::conv_cl_kernel<32, 0, 1> * 512 73728 grids t1 8/8/8 t3 16/16/16 t14 56/56/56
conv cout  16 ks 1 ups 0 kt 3 variant 0 60x104: void ifx::conv::conv_cl_kernel<32, 0, 1> * 512 73728 grids t1 16/16/16 t3 48/48/48 t14 224/224/224
conv cout  16 ks 1 ups 0 kt 3 variant 1  8x64 : void ifx::conv::conv_cl_kernel<32, 0, 1> * 512 73728 grids t1 8/8/8 t3 8/8/8 t14 16/16/16
conv cout  16 ks 1 ups 0 kt 3 variant 1 13x70 : void ifx::conv::conv_cl_kernel<32, 0, 1> * 512 73728 grids t1 8/8/8 t3 16/16/16 t14 56/56/56
conv cout  16 ks 1 ups 0 kt 3 variant 1 60x104: void ifx::conv::conv_cl_kernel<32, 0, 1> * 512 73728 grids t1 16/16/16 t3 48/48/48 t14 224/224/224
conv cout  16 ks 3 ups 0 kt 1 variant 0  8x64 : void ifx::conv::conv_cl_kernel<32, 0, 3> * 512 108544 grids t1 8/8/8 t3 8/8/8 t16 16/16/16
conv cout  16 ks 3 ups 0 kt 1 variant 0 13x70 : void ifx::conv::conv_cl_kernel<32, 0, 3> * 512 108544 grids t1 8/8/8 t3 16/16/16 t16 64/64/64
conv cout  16 ks 3 ups 0 kt 1 variant 0 60x104: void ifx::conv::conv_cl_kernel<32, 0, 3> * 512 108544 grids t1 16/16/16 t3 48/48/48 t16 256/256/256
conv cout  16 ks 3 ups 0 kt 1 variant 1  8x64 : void ifx::conv::conv_cl_kernel<32, 0, 3> * 512 108544 grids t1 8/8/8 t3 8/8/8 t16 16/16/16
conv cout  16 ks 3 ups 0 kt 1 variant 1 13x70 : void ifx::conv::conv_cl_kernel<32, 0, 3> * 512 108544 grids t1 8/8/8 t3 16/16/16 t16 64/64/64
conv cout  16 ks 3 ups 0 kt 1 variant 1 60x104: void ifx::conv::conv_cl_kernel<32, 0, 3> * 512 108544 grids t1 16/16/16 t3 48/48/48 t16 256/256/256
conv cout  16 ks 3 ups 0 kt 3 variant 0  8x64 : void ifx::conv::conv_cl_kernel<32, 0, 3> * 512 108544 grids t1 8/8/8 t3 8/8/8 t14 16/16/16
conv cout  16 ks 3 ups 0 kt 3 variant 0 13x70 : void ifx::conv::conv_cl_kernel<32, 0, 3> * 512 108544 grids t1 8/8/8 t3 16/16/16 t14 56/56/56
conv cout  16 ks 3 ups 0 kt 3 variant 0 60x104: void ifx::conv::conv_cl_kernel<32, 0, 3> * 512 108544 grids t1 16/16/16 t3 48/48/48 t14 224/224/224
conv cout  16 ks 3 ups 0 kt 3 variant 1  8x64 : void ifx::conv::conv_cl_kernel<32, 0, 3> * 512 108544 grids t1 8/8/8 t3 8/8/8 t14 16/16/16
conv cout  16 ks 3 ups 0 kt 3 variant 1 13x70 : void ifx::conv::conv_cl_kernel<32, 0, 3> * 512 108544 grids t1 8/8/8 t3 16/16/16 t14 56/56/56
conv cout  16 ks 3 ups 0 kt 3 variant 1 60x104: void ifx::conv::conv_cl_kernel<32, 0, 3> * 512 108544 grids t1 16/16/16 t3 48/48/48 t14 224/224/224
conv cout  16 ks 3 ups 1 kt 1 variant 0  8x64 : void ifx::conv::conv_cl_kernel<32, 1, 3> * 512 49152 grids t1 8/8/8 t3 16/16/16 t16 64/64/64
conv cout  16 ks 3 ups 1 kt 1 variant 0 13x70 : void ifx::conv::conv_cl_kernel<32, 1, 3> * 512 49152 grids t1 16/16/16 t3 40/40/40 t16 192/192/192
conv cout  16 ks 3 ups 1 kt 1 variant 0 60x104: void ifx::conv::conv_cl_kernel<32, 1, 3> * 512 49152 grids t1 64/64/64 t3 184/184/184 t16 960/960/960
conv cout  16 ks 3 ups 1 kt 1 variant 1  8x64 : void ifx::conv::conv_cl_kernel<32, 1, 3> * 512 49152 grids t1 8/8/8 t3 16/16/16 t16 64/64/64
conv cout  16 ks 3 ups 1 kt 1 variant 1 13x70 : void ifx::conv::conv_cl_kernel<32, 1, 3> * 512 49152 grids t1 16/16/16 t3 40/40/40 t16 192/192/192
conv cout  16 ks 3 ups 1 kt 1 variant 1 60x104: void ifx::conv::conv_cl_kernel<32, 1, 3> * 512 49152 grids t1 64/64/64 t3 184/184/184 t16 960/960/960
conv cout  16 ks 3 ups 1 kt 3 variant 0  8x64 : void ifx::conv::conv_cl_kernel<32, 1, 3> * 512 49152 grids t1 8/8/8 t3 16/16/16 t14 56/56/56
conv cout  16 ks 3 ups 1 kt 3 variant 0 13x70 : void ifx::conv::conv_cl_kernel<32, 1, 3> * 512 49152 grids t1 16/16/16 t3 40/40/40 t14 168/168/168
conv cout  16 ks 3 ups 1 kt 3 variant 0 60x104: void ifx::conv::conv_cl_kernel<32, 1, 3> * 512 49152 grids t1 64/64/64 t3 184/184/184 t14 840/840/840
conv cout  16 ks 3 ups 1 kt 3 variant 1  8x64 : void ifx::conv::conv_cl_kernel<32, 1, 3> * 512 49152 grids t1 8/8/8 t3 16/16/16 t14 56/56/56
conv cout  16 ks 3 ups 1 kt 3 variant 1 13x70 : void ifx::conv::conv_cl_kernel<32, 1, 3> * 512 49152 grids t1 16/16/16 t3 40/40/40 t14 168/168/168
conv cout  16 ks 3 ups 1 kt 3 variant 1 60x104: void ifx::conv::conv_cl_kernel<32, 1, 3> * 512 49152 grids t1 64/64/64 t3 184/184/184 t14 840/840/840
conv cout  24 ks 1 ups 0 kt 1 variant 0  8x64 : void ifx::conv::conv_cl_kernel<32, 0, 1> * 512 73728 grids t1 8/8/8 t3 8/8/8 t16 16/16/16
conv cout  24 ks 1 ups 0 kt 1 variant 0 13x70 : void ifx::conv::conv_cl_kernel<32, 0, 1> * 512 73728 grids t1 8/8/8 t3 16/16/16 t16 64/64/64
conv cout  24 ks 1 ups 0 kt 1 variant 0 60x104: void ifx::conv::conv_cl_kernel<32, 0, 1> * 512 73728 grids t1 16/16/16 t3 48/48/48 t16 256/256/256
conv cout  24 ks 1 ups 0 kt 1 variant 1  8x64 : void ifx::conv::conv_cl_kernel<32, 0, 1> * 512 73728 grids t1 8/8/8 t3 8/8/8 t16 16/16/16
conv cout  24 ks 1 ups 0 kt 1 variant 1 13x70 : void ifx::conv::conv_cl_kernel<32, 0, 1> * 512 73728 grids t1 8/8/8 t3 16/16/16 t16 64/64/64
conv cout  24 ks 1 ups 0 kt 1 variant 1 60x104: void ifx::conv::conv_cl_kernel<32, 0, 1> * 512 73728 grids t1 16/16/16 t3 48/48/48 t16 256/256/256
conv cout  24 ks 1 ups 0 kt 3 variant 0  8x64 : void ifx::conv::conv_cl_kernel<32, 0, 1> * 512 73728 grids t1 8/8/8 t3 8/8/8 t14 16/16/16
conv cout  24 ks 1 ups 0 kt 3 variant 0 13x70 : void ifx::conv::conv_cl_kernel<32, 0, 1> * 512 73728 grids t1 8/8/8 t3 16/16/16 t14 56/56/56
conv cout  24 ks 1 ups 0 kt 3 variant 0 60x104: void ifx::conv::conv_cl_kernel<32, 0, 1> * 512 73728 grids t1 16/16/16 t3 48/48/48 t14 224/224/224
conv cout  24 ks 1 ups 0 kt 3 variant 1  8x64 : void ifx::conv::conv_cl_kernel<32, 0, 1> * 512 73728 grids t1 8/8/8 t3 8/8/8 t14 16/16/16
conv cout  24 ks 1 ups 0 kt 3 variant 1 13x70 : void ifx::conv::conv_cl_kernel<32, 0, 1> * 512 73728 grids t1 8/8/8 t3 16/16/16 t14 56/56/56
conv cout  24 ks 1 ups 0 kt 3 variant 1 60x104: void ifx::conv::conv_cl_kernel<32, 0, 1> * 512 73728 grids t1 16/16/16 t3 48/48/48 t14 224/224/224
conv cout  24 ks 3 ups 0 kt 1 variant 0  8x64 : void ifx::conv::conv_cl_kernel<32, 0, 3> * 512 108544 grids t1 8/8/8 t3 8/8/8 t16 16/16/16
conv cout  24 ks 3 ups 0 kt 1 variant 0 13x70 : void ifx::conv::conv_cl_kernel<32, 0, 3> * 512 108544 grids t1 8/8/8 t3 16/16/16 t16 64/64/64
conv cout  24 ks 3 ups 0 kt 1 variant 0 60x104: void ifx::conv::conv_cl_kernel<32, 0, 3> * 512 108544 grids t1 16/16/16 t3 48/48/48 t16 256/256/256
conv cout  24 ks 3 ups 0 kt 1 variant 1  8x64 : void ifx::conv::conv_cl_kernel<32, 0, 3> * 512 108544 grids t1 8/8/8 t3 8/8/8 t16 16/16/16
conv cout  24 ks 3 ups 0 kt 1 variant 1 13x70 : void ifx::conv::conv_cl_kernel<32, 0, 3> * 512 108544 grids t1 8/8/8 t3 16/16/16 t16 64/64/64
conv cout  24 ks 3 ups 0 kt 1 variant 1 60x104: void ifx::conv::conv_cl_kernel<32, 0, 3> * 512 108544 grids t1 16/16/16 t3 48/48/48 t16 256/256/256
conv cout  24 ks 3 ups 0 kt 3 variant 0  8x64 : void ifx::conv::conv_cl_kernel<32, 0, 3> * 512 108544 grids t1 8/8/8 t3 8/8/8 t14 16/16/16
conv cout  24 ks 3 ups 0 kt 3 variant 0 13x70 : void ifx::conv::conv_cl_kernel<32, 0, 3> * 512 108544 grids t1 8/8/8 t3 16/16/16 t14 56/56/56
conv cout  24 ks 3 ups 0 kt 3 variant 0 60x104: void ifx::conv::conv_cl_kernel<32, 0, 3> * 512 108544 grids t1 16/16/16 t3 48/48/48 t14 224/224/224
conv cout  24 ks 3 ups 0 kt 3 variant 1  8x64 : void ifx::conv::conv_cl_kernel<32, 0, 3> * 512 108544 grids t1 8/8/8 t3 8/8/8 t14 16/16/16
conv cout  24 ks 3 ups 0 kt 3 variant 1 13x70 : void ifx::conv::conv_cl_kernel<32, 0, 3> * 512 108544 grids t1 8/8/8 t3 16/16/16 t14 56/56/56
conv cout  24 ks 3 ups 0 kt 3 variant 1 60x104: void ifx::conv::conv_cl_kernel<32, 0, 3> * 512 108544 grids t1 16/16/16 t3 48/48/48 t14 224/224/224
conv cout  24 ks 3 ups 1 kt 1 variant 0  8x64 : void ifx::conv::conv_cl_kernel<32, 1, 3> * 512 49152 grids t1 8/8/8 t3 16/16/16 t16 64/64/64
conv cout  24 ks 3 ups 1 kt 1 variant 0 13x70 : void ifx::conv::conv_cl_kernel<32, 1, 3> * 512 49152 grids t1 16/16/16 t3 40/40/40 t16 192/192/192
conv cout  24 ks 3 ups 1 kt 1 variant 0 60x104: void ifx::conv::conv_cl_kernel<32, 1, 3> * 512 49152 grids t1 64/64/64 t3 184/184/184 t16 960/960/960
conv cout  24 ks 3 ups 1 kt 1 variant 1  8x64 : void ifx::conv::conv_cl_kernel<32, 1, 3> * 512 49152 grids t1 8/8/8 t3 16/16/16 t16 64/64/64
conv cout  24 ks 3 ups 1 kt 1 variant 1 13x70 : void ifx::conv::conv_cl_kernel<32, 1, 3> * 512 49152 grids t1 16/16/16 t3 40/40/40 t16 192/192/192
conv cout  24 ks 3 ups 1 kt 1 variant 1 60x104: void ifx::conv::conv_cl_kernel<32, 1, 3> * 512 49152 grids t1 64/64/64 t3 184/184/184 t16 960/960/960
conv cout  24 ks 3 ups 1 kt 3 variant 0  8x64 : void ifx::conv::conv_cl_kernel<32, 1, 3> * 512 49152 grids t1 8/8/8 t3 16/16/16 t14 56/56/56
conv cout  24 ks 3 ups 1 kt 3 variant 0 13x70 : void ifx::conv::conv_cl_kernel<32, 1, 3> * 512 49152 grids t1 16/16/16 t3 40/40/40 t14 168/168/168
conv cout  24 ks 3 ups 1 kt 3 variant 0 60x104: void ifx::conv::conv_cl_kernel<32, 1, 3> * 512 49152 grids t1 64/64/64 t3 184/184/184 t14 840/840/840
conv cout  24 ks 3 ups 1 kt 3 variant 1  8x64 : void ifx::conv::conv_cl_kernel<32, 1, 3> * 512 49152 grids t1 8/8/8 t3 16/16/16 t14 56/56/56
conv cout  24 ks 3 ups 1 kt 3 variant 1 13x70 : void ifx::conv::conv_cl_kernel<32, 1, 3> * 512 49152 grids t1 16/16/16 t3 40/40/40 t14 168/168/168
conv cout  24 ks 3 ups 1 kt 3 variant 1 60x104: void ifx::conv::conv_cl_kernel<32, 1, 3> * 512 49152 grids t1 64/64/64 t3 184/184/184 t14 840/840/840
conv cout  32 ks 1 ups 0 kt 1 variant 0  8x64 : void ifx::conv::conv_cl_kernel<32, 0, 1> * 512 73728 grids t1 8/8/8 t3 8/8/8 t16 16/16/16
conv cout  32 ks 1 ups 0 kt 1 variant 0 13x70 : void ifx::conv::conv_cl_kernel<32, 0, 1> * 512 73728 grids t1 8/8/8 t3 16/16/16 t16 64/64/64
conv cout  32 ks 1 ups 0 kt 1 variant 0 60x104: void ifx::conv::conv_cl_kernel<32, 0, 1> * 512 73728 grids t1 16/16/16 t3 48/48/48 t16 256/256/256
conv cout  32 ks 1 ups 0 kt 1 variant 1  8x64 : void ifx::conv::conv_cl_kernel<32, 0, 1> * 512 73728 grids t1 8/8/8 t3 8/8/8 t16 16/16/16
conv cout  32 ks 1 ups 0 kt 1 variant 1 13x70 : void ifx::conv::conv_cl_kernel<32, 0, 1> * 512 73728 grids t1 8/8/8 t3 16/16/16 t16 64/64/64
conv cout  32 ks 1 ups 0 kt 1 variant 1 60x104: void ifx::conv::conv_cl_kernel<32, 0, 1> * 512 73728 grids t1 16/16/16 t3 48/48/48 t16 256/256/256
conv cout  32 ks 1 ups 0 kt 3 variant 0  8x64 : void ifx::conv::conv_cl_kernel<32, 0, 1> * 512 73728 grids t1 8/8/8 t3 8/8/8 t14 16/16/16
conv cout  32 ks 1 ups 0 kt 3 variant 0 13x70 : void ifx::conv::conv_cl_kernel<32, 0, 1> * 512 73728 grids t1 8/8/8 t3 16/16/16 t14 56/56/56
conv cout  32 ks 1 ups 0 kt 3 variant 0 60x104: void ifx::conv::conv_cl_kernel<32, 0, 1> * 512 73728 grids t1 16/16/16 t3 48/48/48 t14 224/224/224
conv cout  32 ks 1 ups 0 kt 3 variant 1  8x64 : void ifx::conv::conv_cl_kernel<32, 0, 1> * 512 73728 grids t1 8/8/8 t3 8/8/8 t14 16/16/16
conv cout  32 ks 1 ups 0 kt 3 variant 1 13x70 : void ifx::conv::conv_cl_kernel<32, 0, 1> * 512 73728 grids t1 8/8/8 t3 16/16/16 t14 56/56/56
conv cout  32 ks 1 ups 0 kt 3 variant 1 60x104: void ifx::conv::conv_cl_kernel<32, 0, 1> * 512 73728 grids t1 16/16/16 t3 48/48/48 t14 224/224/224
conv cout  32 ks 3 ups 0 kt 1 variant 0  8x64 : void ifx::conv::conv_cl_kernel<32, 0, 3> * 512 108544 grids t1 8/8/8 t3 8/8/8 t16 16/16/16
conv cout  32 ks 3 ups 0 kt 1 variant 0 13x70 : void ifx::conv::conv_cl_kernel<32, 0, 3> * 512 108544 grids t1 8/8/8 t3 16/16/16 t16 64/64/64
conv cout  32 ks 3 ups 0 kt 1 variant 0 60x104: void ifx::conv::conv_cl_kernel<32, 0, 3> * 512 108544 grids t1 16/16/16 t3 48/48/48 t16 256/256/256
conv cout  32 ks 3 ups 0 kt 1 variant 1  8x64 : void ifx::conv::conv_cl_kernel<32, 0, 3> * 512 108544 grids t1 8/8/8 t3 8/8/8 t16 16/16/16
conv cout  32 ks 3 ups 0 kt 1 variant 1 13x70 : void ifx::conv::conv_cl_kernel<32, 0, 3> * 512 108544 grids t1 8/8/8 t3 16/16/16 t16 64/64/64
conv cout  32 ks 3 ups 0 kt 1 variant 1 60x104: void ifx::conv::conv_cl_kernel<32, 0, 3> * 512 108544 grids t1 16/16/16 t3 48/48/48 t16 256/256/256
conv cout  32 ks 3 ups 0 kt 3 variant 0  8x64 : void ifx::conv::conv_cl_kernel<32, 0, 3> * 512 108544 grids t1 8/8/8 t3 8/8/8 t14 16/16/16
conv cout  32 ks 3 ups 0 kt 3 variant 0 13x70 : void ifx::conv::conv_cl_kernel<32, 0, 3> * 512 108544 grids t1 8/8/8 t3 16/16/16 t14 56/56/56
conv cout  32 ks 3 ups 0 kt 3 variant 0 60x104: void ifx::conv::conv_cl_kernel<32, 0, 3> * 512 108544 grids t1 16/16/16 t3 48/48/48 t14 224/224/224
conv cout  32 ks 3 ups 0 kt 3 variant 1  8x64 : void ifx::conv::conv_cl_kernel<32, 0, 3> * 512 108544 grids t1 8/8/8 t3 8/8/8 t14 16/16/16
conv cout  32 ks 3 ups 0 kt 3 variant 1 13x70 : void ifx::conv::conv_cl_kernel<32, 0, 3> * 512 108544 grids t1 8/8/8 t3 16/16/16 t14 56/56/56
conv cout  32 ks 3 ups 0 kt 3 variant 1 60x104: void ifx::conv::conv_cl_kernel<32, 0, 3> * 512 108544 grids t1 16/16/16 t3 48/48/48 t14 224/224/224
conv cout  32 ks 3 ups 1 kt 1 variant 0  8x64 : void ifx::conv::conv_cl_kernel<32, 1, 3> * 512 49152 grids t1 8/8/8 t3 16/16/16 t16 64/64/64
conv cout  32 ks 3 ups 1 kt 1 variant 0 13x70 : void ifx::conv::conv_cl_kernel<32, 1, 3> * 512 49152 grids t1 16/16/16 t3 40/40/40 t16 192/192/192
conv cout  32 ks 3 ups 1 kt 1 variant 0 60x104: void ifx::conv::conv_cl_kernel<32, 1, 3> * 512 49152 grids t1 64/64/64 t3 184/184/184 t16 960/960/960
conv cout  32 ks 3 ups 1 kt 1 variant 1  8x64 : void ifx::conv::conv_cl_kernel<32, 1, 3> * 512 49152 grids t1 8/8/8 t3 16/16/16 t16 64/64/64
conv cout  32 ks 3 ups 1 kt 1 variant 1 13x70 : void ifx::conv::conv_cl_kernel<32, 1, 3> * 512 49152 grids t1 16/16/16 t3 40/40/40 t16 192/192/192
conv cout  32 ks 3 ups 1 kt 1 variant 1 60x104: void ifx::conv::conv_cl_kernel<32, 1, 3> * 512 49152 grids t1 64/64/64 t3 184/184/184 t16 960/960/960
conv cout  32 ks 3 ups 1 kt 3 variant 0  8x64 : void ifx::conv::conv_cl_kernel<32, 1, 3> * 512 49152 grids t1 8/8/8 t3 16/16/16 t14 56/56/56
conv cout  32 ks 3 ups 1 kt 3 variant 0 13x70 : void ifx::conv::conv_cl_kernel<32, 1, 3> * 512 49152 grids t1 16/16/16 t3 40/40/40 t14 168/168/168
conv cout  32 ks 3 ups 1 kt 3 variant 0 60x104: void ifx::conv::conv_cl_kernel<32, 1, 3> * 512 49152 grids t1 64/64/64 t3 184/184/184 t14 840/840/840
conv cout  32 ks 3 ups 1 kt 3 variant 1  8x64 : void ifx::conv::conv_cl_kernel<32, 1, 3> * 512 49152 grids t1 8/8/8 t3 16/16/16 t14 56/56/56
conv cout  32 ks 3 ups 1 kt 3 variant 1 13x70 : void ifx::conv::conv_cl_kernel<32, 1, 3> * 512 49152 grids t1 16/16/16 t3 40/40/40 t14 168/168/168
conv cout  32 ks 3 ups 1 kt 3 variant 1 60x104: void ifx::conv::conv_cl_kernel<32, 1, 3> * 512 49152 grids t1 64/64/64 t3 184/184/184 t14 840/840/840
conv cout  48 ks 1 ups 0 kt 1 variant 0  8x64 : void ifx::conv::conv_cl_kernel<64, 0, 1> * 512 77824 grids t1 8/8/8 t3 8/8/8 t16 16/16/16
conv cout  48 ks 1 ups 0 kt 1 variant 0 13x70 : void ifx::conv::conv_cl_kernel<64, 0, 1> * 512 77824 grids t1 8/8/8 t3 16/16/16 t16 64/64/64
conv cout  48 ks 1 ups 0 kt 1 variant 0 60x104: void ifx::conv::conv_cl_kernel<64, 0, 1> * 512 77824 grids t1 16/16/16 t3 48/48/48 t16 256/256/256
conv cout  48 ks 1 ups 0 kt 1 variant 1  8x64 : void ifx::conv::conv_cl_kernel<64, 0, 1> * 512 77824 grids t1 8/8/8 t3 8/8/8 t16 16/16/16
conv cout  48 ks 1 ups 0 kt 1 variant 1 13x70 : void ifx::conv::conv_cl_kernel<64, 0, 1> * 512 77824 grids t1 8/8/8 t3 16/16/16 t16 64/64/64
conv cout  48 ks 1 ups 0 kt 1 variant 1 60x104: void ifx::conv::conv_cl_kernel<64, 0, 1> * 512 77824 grids t1 16/16/16 t3 48/48/48 t16 256/256/256
conv cout  48 ks 1 ups 0 kt 3 variant 0  8x64 : void ifx::conv::conv_cl_kernel<64, 0, 1> * 512 77824 grids t1 8/8/8 t3 8/8/8 t14 16/16/16
conv cout  48 ks 1 ups 0 kt 3 variant 0 13x70 : void ifx::conv::conv_cl_kernel<64, 0, 1> * 512 77824 grids t1 8/8/8 t3 16/16/16 t14 56/56/56
conv cout  48 ks 1 ups 0 kt 3 variant 0 60x104: void ifx::conv::conv_cl_kernel<64, 0, 1> * 512 77824 grids t1 16/16/16 t3 48/48/48 t14 224/224/224
conv cout  48 ks 1 ups 0 kt 3 variant 1  8x64 : void ifx::conv::conv_cl_kernel<64, 0, 1> * 512 77824 grids t1 8/8/8 t3 8/8/8 t14 16/16/16
conv cout  48 ks 1 ups 0 kt 3 variant 1 13x70 : void ifx::conv::conv_cl_kernel<64, 0, 1> * 512 77824 grids t1 8/8/8 t3 16/16/16 t14 56/56/56
conv cout  48 ks 1 ups 0 kt 3 variant 1 60x104: void ifx::conv::conv_cl_kernel<64, 0, 1> * 512 77824 grids t1 16/16/16 t3 48/48/48 t14 224/224/224
conv cout  48 ks 3 ups 0 kt 1 variant 0  8x64 : void ifx::conv::conv_cl_kernel<64, 0, 3> * 512 126976 grids t1 8/8/8 t3 8/8/8 t16 16/16/16
conv cout  48 ks 3 ups 0 kt 1 variant 0 13x70 : void ifx::conv::conv_cl_kernel<64, 0, 3> * 512 126976 grids t1 8/8/8 t3 16/16/16 t16 64/64/64
conv cout  48 ks 3 ups 0 kt 1 variant 0 60x104: void ifx::conv::conv_cl_kernel<64, 0, 3> * 512 126976 grids t1 16/16/16 t3 48/48/48 t16 256/256/256
conv cout  48 ks 3 ups 0 kt 1 variant 1  8x64 : void ifx::conv::conv_cl_kernel<64, 0, 3> * 512 126976 grids t1 8/8/8 t3 8/8/8 t16 16/16/16
conv cout  48 ks 3 ups 0 kt 1 variant 1 13x70 : void ifx::conv::conv_cl_kernel<64, 0, 3> * 512 126976 grids t1 8/8/8 t3 16/16/16 t16 64/64/64
conv cout  48 ks 3 ups 0 kt 1 variant 1 60x104: void ifx::conv::conv_cl_kernel<64, 0, 3> * 512 126976 grids t1 16/16/16 t3 48/48/48 t16 256/256/256
conv cout  48 ks 3 ups 0 kt 3 variant 0  8x64 : void ifx::conv::conv_cl_kernel<64, 0, 3> * 512 126976 grids t1 8/8/8 t3 8/8/8 t14 16/16/16
conv cout  48 ks 3 ups 0 kt 3 variant 0 13x70 : void ifx::conv::conv_cl_kernel<64, 0, 3> * 512 126976 grids t1 8/8/8 t3 16/16/16 t14 56/56/56
conv cout  48 ks 3 ups 0 kt 3 variant 0 60x104: void ifx::conv::conv_cl_kernel<64, 0, 3> * 512 126976 grids t1 16/16/16 t3 48/48/48 t14 224/224/224
conv cout  48 ks 3 ups 0 kt 3 variant 1  8x64 : void ifx::conv::conv_cl_kernel<64, 0, 3> * 512 126976 grids t1 8/8/8 t3 8/8/8 t14 16/16/16
conv cout  48 ks 3 ups 0 kt 3 variant 1 13x70 : void ifx::conv::conv_cl_kernel<64, 0, 3> * 512 126976 grids t1 8/8/8 t3 16/16/16 t14 56/56/56
conv cout  48 ks 3 ups 0 kt 3 variant 1 60x104: void ifx::conv::conv_cl_kernel<64, 0, 3> * 512 126976 grids t1 16/16/16 t3 48/48/48 t14 224/224/224
conv cout  48 ks 3 ups 1 kt 1 variant 0  8x64 : void ifx::conv::conv_cl_kernel<64, 1, 3> * 512 73728 grids t1 8/8/8 t3 16/16/16 t16 64/64/64
conv cout  48 ks 3 ups 1 kt 1 variant 0 13x70 : void ifx::conv::conv_cl_kernel<64, 1, 3> * 512 73728 grids t1 16/16/16 t3 40/40/40 t16 192/192/192
conv cout  48 ks 3 ups 1 kt 1 variant 0 60x104: void ifx::conv::conv_cl_kernel<64, 1, 3> * 512 73728 grids t1 64/64/64 t3 184/184/184 t16 960/960/960
conv cout  48 ks 3 ups 1 kt 1 variant 1  8x64 : void ifx::conv::conv_cl_kernel<64, 1, 3> * 512 73728 grids t1 8/8/8 t3 16/16/16 t16 64/64/64
conv cout  48 ks 3 ups 1 kt 1 variant 1 13x70 : void ifx::conv::conv_cl_kernel<64, 1, 3> * 512 73728 grids t1 16/16/16 t3 40/40/40 t16 192/192/192
conv cout  48 ks 3 ups 1 kt 1 variant 1 60x104: void ifx::conv::conv_cl_kernel<64, 1, 3> * 512 73728 grids t1 64/64/64 t3 184/184/184 t16 960/960/960
conv cout  48 ks 3 ups 1 kt 3 variant 0  8x64 : void ifx::conv::conv_cl_kernel<64, 1, 3> * 512 73728 grids t1 8/8/8 t3 16/16/16 t14 56/56/56
conv cout  48 ks 3 ups 1 kt 3 variant 0 13x70 : void ifx::conv::conv_cl_kernel<64, 1, 3> * 512 73728 grids t1 16/16/16 t3 40/40/40 t14 168/168/168
conv cout  48 ks 3 ups 1 kt 3 variant 0 60x104: void ifx::conv::conv_cl_kernel<64, 1, 3> * 512 73728 grids t1 64/64/64 t3 184/184/184 t14 840/840/840
conv cout  48 ks 3 ups 1 kt 3 variant 1  8x64 : void ifx::conv::conv_cl_kernel<64, 1, 3> * 512 73728 grids t1 8/8/8 t3 16/16/16 t14 56/56/56
conv cout  48 ks 3 ups 1 kt 3 variant 1 13x70 : void ifx::conv::conv_cl_kernel<64, 1, 3> * 512 73728 grids t1 16/16/16 t3 40/40/40 t14 168/168/168
conv cout  48 ks 3 ups 1 kt 3 variant 1 60x104: void ifx::conv::conv_cl_kernel<64, 1, 3> * 512 73728 grids t1 64/64/64 t3 184/184/184 t14 840/840/840
conv cout  64 ks 1 ups 0 kt 1 variant 0  8x64 : void ifx::conv::conv_cl_kernel<64, 0, 1> * 512 77824 grids t1 8/8/8 t3 8/8/8 t16 16/16/16
conv cout  64 ks 1 ups 0 kt 1 variant 0 13x70 : void ifx::conv::conv_cl_kernel<64, 0, 1> * 512 77824 grids t1 8/8/8 t3 16/16/16 t16 64/64/64
conv cout  64 ks 1 ups 0 kt 1 variant 0 60x104: void ifx::conv::conv_cl_kernel<64, 0, 1> * 512 77824 grids t1 16/16/16 t3 48/48/48 t16 256/256/256
conv cout  64 ks 1 ups 0 kt 1 variant 1  8x64 : void ifx::conv::conv_cl_kernel<64, 0, 1> * 512 77824 grids t1 8/8/8 t3 8/8/8 t16 16/16/16
conv cout  64 ks 1 ups 0 kt 1 variant 1 13x70 : void ifx::conv::conv_cl_kernel<64, 0, 1> * 512 77824 grids t1 8/8/8 t3 16/16/16 t16 64/64/64
conv cout  64 ks 1 ups 0 kt 1 variant 1 60x104: void ifx::conv::conv_cl_kernel<64, 0, 1> * 512 77824 grids t1 16/16/16 t3 48/48/48 t16 256/256/256
conv cout  64 ks 1 ups 0 kt 3 variant 0  8x64 : void ifx::conv::conv_cl_kernel<64, 0, 1> * 512 77824 grids t1 8/8/8 t3 8/8/8 t14 16/16/16
conv cout  64 ks 1 ups 0 kt 3 variant 0 13x70 : void ifx::conv::conv_cl_kernel<64, 0, 1> * 512 77824 grids t1 8/8/8 t3 16/16/16 t14 56/56/56
conv cout  64 ks 1 ups 0 kt 3 variant 0 60x104: void ifx::conv::conv_cl_kernel<64, 0, 1> * 512 77824 grids t1 16/16/16 t3 48/48/48 t14 224/224/224
conv cout  64 ks 1 ups 0 kt 3 variant 1  8x64 : void ifx::conv::conv_cl_kernel<64, 0, 1> * 512 77824 grids t1 8/8/8 t3 8/8/8 t14 16/16/16
conv cout  64 ks 1 ups 0 kt 3 variant 1 13x70 : void ifx::conv::conv_cl_kernel<64, 0, 1> * 512 77824 grids t1 8/8/8 t3 16/16/16 t14 56/56/56
conv cout  64 ks 1 ups 0 kt 3 variant 1 60x104: void ifx::conv::conv_cl_kernel<64, 0, 1> * 512 77824 grids t1 16/16/16 t3 48/48/48 t14 224/224/224
conv cout  64 ks 3 ups 0 kt 1 variant 0  8x64 : void ifx::conv::conv_cl_kernel<64, 0, 3> * 512 126976 grids t1 8/8/8 t3 8/8/8 t16 16/16/16
conv cout  64 ks 3 ups 0 kt 1 variant 0 13x70 : void ifx::conv::conv_cl_kernel<64, 0, 3> * 512 126976 grids t1 8/8/8 t3 16/16/16 t16 64/64/64
conv cout  64 ks 3 ups 0 kt 1 variant 0 60x104: void ifx::conv::conv_cl_kernel<64, 0, 3> * 512 126976 grids t1 16/16/16 t3 48/48/48 t16 256/256/256
conv cout  64 ks 3 ups 0 kt 1 variant 1  8x64 : void ifx::conv::conv_cl_kernel<64, 0, 3> * 512 126976 grids t1 8/8/8 t3 8/8/8 t16 16/16/16
conv cout  64 ks 3 ups 0 kt 1 variant 1 13x70 : void ifx::conv::conv_cl_kernel<64, 0, 3> * 512 126976 grids t1 8/8/8 t3 16/16/16 t16 64/64/64
conv cout  64 ks 3 ups 0 kt 1 variant 1 60x104: void ifx::conv::conv_cl_kernel<64, 0, 3> * 512 126976 grids t1 16/16/16 t3 48/48/48 t16 256/256/256
conv cout  64 ks 3 ups 0 kt 3 variant 0  8x64 : void ifx::conv::conv_cl_kernel<64, 0, 3> * 512 126976 grids t1 8/8/8 t3 8/8/8 t14 16/16/16
conv cout  64 ks 3 ups 0 kt 3 variant 0 13x70 : void ifx::conv::conv_cl_kernel<64, 0, 3> * 512 126976 grids t1 8/8/8 t3 16/16/16 t14 56/56/56
conv cout  64 ks 3 ups 0 kt 3 variant 0 60x104: void ifx::conv::conv_cl_kernel<64, 0, 3> * 512 126976 grids t1 16/16/16 t3 48/48/48 t14 224/224/224
conv cout  64 ks 3 ups 0 kt 3 variant 1  8x64 : void ifx::conv::conv_cl_kernel<64, 0, 3> * 512 126976 grids t1 8/8/8 t3 8/8/8 t14 16/16/16
conv cout  64 ks 3 ups 0 kt 3 variant 1 13x70 : void ifx::conv::conv_cl_kernel<64, 0, 3> * 512 126976 grids t1 8/8/8 t3 16/16/16 t14 56/56/56
conv cout  64 ks 3 ups 0 kt 3 variant 1 60x104: void ifx::conv::conv_cl_kernel<64, 0, 3> * 512 126976 grids t1 16/16/16 t3 48/48/48 t14 224/224/224
conv cout  64 ks 3 ups 1 kt 1 variant 0  8x64 : void ifx::conv::conv_cl_kernel<64, 1, 3> * 512 73728 grids t1 8/8/8 t3 16/16/16 t16 64/64/64
conv cout  64 ks 3 ups 1 kt 1 variant 0 13x70 : void ifx::conv::conv_cl_kernel<64, 1, 3> * 512 73728 grids t1 16/16/16 t3 40/40/40 t16 192/192/192
conv cout  64 ks 3 ups 1 kt 1 variant 0 60x104: void ifx::conv::conv_cl_kernel<64, 1, 3> * 512 73728 grids t1 64/64/64 t3 184/184/184 t16 960/960/960
conv cout  64 ks 3 ups 1 kt 1 variant 1  8x64 : void ifx::conv::conv_cl_kernel<64, 1, 3> * 512 73728 grids t1 8/8/8 t3 16/16/16 t16 64/64/64
conv cout  64 ks 3 ups 1 kt 1 variant 1 13x70 : void ifx::conv::conv_cl_kernel<64, 1, 3> * 512 73728 grids t1 16/16/16 t3 40/40/40 t16 192/192/192
conv cout  64 ks 3 ups 1 kt 1 variant 1 60x104: void ifx::conv::conv_cl_kernel<64, 1, 3> * 512 73728 grids t1 64/64/64 t3 184/184/184 t16 960/960/960
conv cout  64 ks 3 ups 1 kt 3 variant 0  8x64 : void ifx::conv::conv_cl_kernel<64, 1, 3> * 512 73728 grids t1 8/8/8 t3 16/16/16 t14 56/56/56
conv cout  64 ks 3 ups 1 kt 3 variant 0 13x70 : void ifx::conv::conv_cl_kernel<64, 1, 3> * 512 73728 grids t1 16/16/16 t3 40/40/40 t14 168/168/168
conv cout  64 ks 3 ups 1 kt 3 variant 0 60x104: void ifx::conv::conv_cl_kernel<64, 1, 3> * 512 73728 grids t1 64/64/64 t3 184/184/184 t14 840/840/840
conv cout  64 ks 3 ups 1 kt 3 variant 1  8x64 : void ifx::conv::conv_cl_kernel<64, 1, 3> * 512 73728 grids t1 8/8/8 t3 16/16/16 t14 56/56/56
conv cout  64 ks 3 ups 1 kt 3 variant 1 13x70 : void ifx::conv::conv_cl_kernel<64, 1, 3> * 512 73728 grids t1 16/16/16 t3 40/40/40 t14 168/168/168
conv cout  64 ks 3 ups 1 kt 3 variant 1 60x104: void ifx::conv::conv_cl_kernel<64, 1, 3> * 512 73728 grids t1 64/64/64 t3 184/184/184 t14 840/840/840
conv cout  96 ks 1 ups 0 kt 1 variant 0  8x64 : void ifx::conv::conv_cl_kernel<96, 0, 1> * 512 106496 grids t1 8/8/8 t3 8/8/8 t16 16/16/16
conv cout  96 ks 1 ups 0 kt 1 variant 0 13x70 : void ifx::conv::conv_cl_kernel<96, 0, 1> * 512 106496 grids t1 8/8/8 t3 16/16/16 t16 64/64/64
conv cout  96 ks 1 ups 0 kt 1 variant 0 60x104: void ifx::conv::conv_cl_kernel<96, 0, 1> * 512 106496 grids t1 16/16/16 t3 48/48/48 t16 256/256/256
conv cout  96 ks 1 ups 0 kt 1 variant 1  8x64 : void ifx::conv::conv_cl_kernel<96, 0, 1> * 512 106496 grids t1 8/8/8 t3 8/8/8 t16 16/16/16
conv cout  96 ks 1 ups 0 kt 1 variant 1 13x70 : void ifx::conv::conv_cl_kernel<96, 0, 1> * 512 106496 grids t1 8/8/8 t3 16/16/16 t16 64/64/64
conv cout  96 ks 1 ups 0 kt 1 variant 1 60x104: void ifx::conv::conv_cl_kernel<96, 0, 1> * 512 106496 grids t1 16/16/16 t3 48/48/48 t16 256/256/256
conv cout  96 ks 1 ups 0 kt 3 variant 0  8x64 : void ifx::conv::conv_cl_kernel<96, 0, 1> * 512 106496 grids t1 8/8/8 t3 8/8/8 t14 16/16/16
conv cout  96 ks 1 ups 0 kt 3 variant 0 13x70 : void ifx::conv::conv_cl_kernel<96, 0, 1> * 512 106496 grids t1 8/8/8 t3 16/16/16 t14 56/56/56
conv cout  96 ks 1 ups 0 kt 3 variant 0 60x104: void ifx::conv::conv_cl_kernel<96, 0, 1> * 512 106496 grids t1 16/16/16 t3 48/48/48 t14 224/224/224
conv cout  96 ks 1 ups 0 kt 3 variant 1  8x64 : void ifx::conv::conv_cl_kernel<96, 0, 1> * 512 106496 grids t1 8/8/8 t3 8/8/8 t14 16/16/16
conv cout  96 ks 1 ups 0 kt 3 variant 1 13x70 : void ifx::conv::conv_cl_kernel<96, 0, 1> * 512 106496 grids t1 8/8/8 t3 16/16/16 t14 56/56/56
conv cout  96 ks 1 ups 0 kt 3 variant 1 60x104: void ifx::conv::conv_cl_kernel<96, 0, 1> * 512 106496 grids t1 16/16/16 t3 48/48/48 t14 224/224/224
conv cout  96 ks 3 ups 0 kt 1 variant 0  8x64 : void ifx::conv::pp::conv_pp_kernel<96, 0> * 512 152576 grids t1 8/8/8 t3 8/8/8 t16 16/16/16
conv cout  96 ks 3 ups 0 kt 1 variant 0 13x70 : void ifx::conv::pp::conv_pp_kernel<96, 0> * 512 152576 grids t1 8/8/8 t3 16/16/16 t16 64/64/64
conv cout  96 ks 3 ups 0 kt 1 variant 0 60x104: void ifx::conv::pp::conv_pp_kernel<96, 0> * 512 152576 grids t1 16/16/16 t3 48/48/48 t16 256/256/64
conv cout  96 ks 3 ups 0 kt 1 variant 1  8x64 : void ifx::conv::conv_cl_kernel<96, 0, 3> * 512 145408 grids t1 8/8/8 t3 8/8/8 t16 16/16/16
conv cout  96 ks 3 ups 0 kt 1 variant 1 13x70 : void ifx::conv::conv_cl_kernel<96, 0, 3> * 512 145408 grids t1 8/8/8 t3 16/16/16 t16 64/64/64
conv cout  96 ks 3 ups 0 kt 1 variant 1 60x104: void ifx::conv::conv_cl_kernel<96, 0, 3> * 512 145408 grids t1 16/16/16 t3 48/48/48 t16 256/256/256
conv cout  96 ks 3 ups 0 kt 3 variant 0  8x64 : void ifx::conv::pp::conv_pp_kernel<96, 0> * 512 152576 grids t1 8/8/8 t3 8/8/8 t14 16/16/16
conv cout  96 ks 3 ups 0 kt 3 variant 0 13x70 : void ifx::conv::pp::conv_pp_kernel<96, 0> * 512 152576 grids t1 8/8/8 t3 16/16/16 t14 56/56/56
conv cout  96 ks 3 ups 0 kt 3 variant 0 60x104: void ifx::conv::pp::conv_pp_kernel<96, 0> * 512 152576 grids t1 16/16/16 t3 48/48/48 t14 224/224/64
conv cout  96 ks 3 ups 0 kt 3 variant 1  8x64 : void ifx::conv::conv_cl_kernel<96, 0, 3> * 512 145408 grids t1 8/8/8 t3 8/8/8 t14 16/16/16
conv cout  96 ks 3 ups 0 kt 3 variant 1 13x70 : void ifx::conv::conv_cl_kernel<96, 0, 3> * 512 145408 grids t1 8/8/8 t3 16/16/16 t14 56/56/56
conv cout  96 ks 3 ups 0 kt 3 variant 1 60x104: void ifx::conv::conv_cl_kernel<96, 0, 3> * 512 145408 grids t1 16/16/16 t3 48/48/48 t14 224/224/224
conv cout  96 ks 3 ups 1 kt 1 variant 0  8x64 : void ifx::conv::pp::conv_pp_kernel<96, 1> * 512 93184 grids t1 8/8/8 t3 16/16/16 t16 64/64/64
conv cout  96 ks 3 ups 1 kt 1 variant 0 13x70 : void ifx::conv::pp::conv_pp_kernel<96, 1> * 512 93184 grids t1 16/16/16 t3 40/40/40 t16 192/192/64
conv cout  96 ks 3 ups 1 kt 1 variant 0 60x104: void ifx::conv::pp::conv_pp_kernel<96, 1> * 512 93184 grids t1 64/64/64 t3 184/184/64 t16 256/304/64
conv cout  96 ks 3 ups 1 kt 1 variant 1  8x64 : void ifx::conv::conv_cl_kernel<96, 1, 3> * 512 106496 grids t1 8/8/8 t3 16/16/16 t16 64/64/64
conv cout  96 ks 3 ups 1 kt 1 variant 1 13x70 : void ifx::conv::conv_cl_kernel<96, 1, 3> * 512 106496 grids t1 16/16/16 t3 40/40/40 t16 192/192/192
conv cout  96 ks 3 ups 1 kt 1 variant 1 60x104: void ifx::conv::conv_cl_kernel<96, 1, 3> * 512 106496 grids t1 64/64/64 t3 184/184/184 t16 960/960/960
conv cout  96 ks 3 ups 1 kt 3 variant 0  8x64 : void ifx::conv::pp::conv_pp_kernel<96, 1> * 512 93184 grids t1 8/8/8 t3 16/16/16 t14 56/56/56
conv cout  96 ks 3 ups 1 kt 3 variant 0 13x70 : void ifx::conv::pp::conv_pp_kernel<96, 1> * 512 93184 grids t1 16/16/16 t3 40/40/40 t14 168/168/64
conv cout  96 ks 3 ups 1 kt 3 variant 0 60x104: void ifx::conv::pp::conv_pp_kernel<96, 1> * 512 93184 grids t1 64/64/64 t3 184/184/64 t14 256/304/64
conv cout  96 ks 3 ups 1 kt 3 variant 1  8x64 : void ifx::conv::conv_cl_kernel<96, 1, 3> * 512 106496 grids t1 8/8/8 t3 16/16/16 t14 56/56/56
conv cout  96 ks 3 ups 1 kt 3 variant 1 13x70 : void ifx::conv::conv_cl_kernel<96, 1, 3> * 512 106496 grids t1 16/16/16 t3 40/40/40 t14 168/168/168
conv cout  96 ks 3 ups 1 kt 3 variant 1 60x104: void ifx::conv::conv_cl_kernel<96, 1, 3> * 512 106496 grids t1 64/64/64 t3 184/184/184 t14 840/840/840
conv cout 128 ks 1 ups 0 kt 1 variant 0  8x64 : void ifx::conv::conv_cl_kernel<128, 0, 1> * 512 139264 grids t1 8/8/8 t3 8/8/8 t16 16/16/16
conv cout 128 ks 1 ups 0 kt 1 variant 0 13x70 : void ifx::conv::conv_cl_kernel<128, 0, 1> * 512 139264 grids t1 8/8/8 t3 16/16/16 t16 64/64/64
conv cout 128 ks 1 ups 0 kt 1 variant 0 60x104: void ifx::conv::conv_cl_kernel<128, 0, 1> * 512 139264 grids t1 16/16/16 t3 48/48/48 t16 256/256/256
conv cout 128 ks 1 ups 0 kt 1 variant 1  8x64 : void ifx::conv::conv_cl_kernel<128, 0, 1> * 512 139264 grids t1 8/8/8 t3 8/8/8 t16 16/16/16
conv cout 128 ks 1 ups 0 kt 1 variant 1 13x70 : void ifx::conv::conv_cl_kernel<128, 0, 1> * 512 139264 grids t1 8/8/8 t3 16/16/16 t16 64/64/64
conv cout 128 ks 1 ups 0 kt 1 variant 1 60x104: void ifx::conv::conv_cl_kernel<128, 0, 1> * 512 139264 grids t1 16/16/16 t3 48/48/48 t16 256/256/256
conv cout 128 ks 1 ups 0 kt 3 variant 0  8x64 : void ifx::conv::conv_cl_kernel<128, 0, 1> * 512 139264 grids t1 8/8/8 t3 8/8/8 t14 16/16/16
conv cout 128 ks 1 ups 0 kt 3 variant 0 13x70 : void ifx::conv::conv_cl_kernel<128, 0, 1> * 512 139264 grids t1 8/8/8 t3 16/16/16 t14 56/56/56
conv cout 128 ks 1 ups 0 kt 3 variant 0 60x104: void ifx::conv::conv_cl_kernel<128, 0, 1> * 512 139264 grids t1 16/16/16 t3 48/48/48 t14 224/224/224
conv cout 128 ks 1 ups 0 kt 3 variant 1  8x64 : void ifx::conv::conv_cl_kernel<128, 0, 1> * 512 139264 grids t1 8/8/8 t3 8/8/8 t14 16/16/16
conv cout 128 ks 1 ups 0 kt 3 variant 1 13x70 : void ifx::conv::conv_cl_kernel<128, 0, 1> * 512 139264 grids t1 8/8/8 t3 16/16/16 t14 56/56/56
conv cout 128 ks 1 ups 0 kt 3 variant 1 60x104: void ifx::conv::conv_cl_kernel<128, 0, 1> * 512 139264 grids t1 16/16/16 t3 48/48/48 t14 224/224/224
conv cout 128 ks 3 ups 0 kt 1 variant 0  8x64 : void ifx::conv::conv_cl_kernel<128, 0, 3> * 512 139264 grids t1 8/8/8 t3 8/8/8 t16 16/16/16
conv cout 128 ks 3 ups 0 kt 1 variant 0 13x70 : void ifx::conv::conv_cl_kernel<128, 0, 3> * 512 139264 grids t1 8/8/8 t3 16/16/16 t16 64/64/64
conv cout 128 ks 3 ups 0 kt 1 variant 0 60x104: void ifx::conv::conv_cl_kernel<128, 0, 3> * 512 139264 grids t1 16/16/16 t3 48/48/48 t16 256/256/256
conv cout 128 ks 3 ups 0 kt 1 variant 1  8x64 : void ifx::conv::conv_cl_kernel<128, 0, 3> * 512 139264 grids t1 8/8/8 t3 8/8/8 t16 16/16/16
conv cout 128 ks 3 ups 0 kt 1 variant 1 13x70 : void ifx::conv::conv_cl_kernel<128, 0, 3> * 512 139264 grids t1 8/8/8 t3 16/16/16 t16 64/64/64
conv cout 128 ks 3 ups 0 kt 1 variant 1 60x104: void ifx::conv::conv_cl_kernel<128, 0, 3> * 512 139264 grids t1 16/16/16 t3 48/48/48 t16 256/256/256
conv cout 128 ks 3 ups 0 kt 3 variant 0  8x64 : void ifx::conv::conv_cl_kernel<128, 0, 3> * 512 139264 grids t1 8/8/8 t3 8/8/8 t14 16/16/16
conv cout 128 ks 3 ups 0 kt 3 variant 0 13x70 : void ifx::conv::conv_cl_kernel<128, 0, 3> * 512 139264 grids t1 8/8/8 t3 16/16/16 t14 56/56/56
conv cout 128 ks 3 ups 0 kt 3 variant 0 60x104: void ifx::conv::conv_cl_kernel<128, 0, 3> * 512 139264 grids t1 16/16/16 t3 48/48/48 t14 224/224/224
conv cout 128 ks 3 ups 0 kt 3 variant 1  8x64 : void ifx::conv::conv_cl_kernel<128, 0, 3> * 512 139264 grids t1 8/8/8 t3 8/8/8 t14 16/16/16
conv cout 128 ks 3 ups 0 kt 3 variant 1 13x70 : void ifx::conv::conv_cl_kernel<128, 0, 3> * 512 139264 grids t1 8/8/8 t3 16/16/16 t14 56/56/56
conv cout 128 ks 3 ups 0 kt 3 variant 1 60x104: void ifx::conv::conv_cl_kernel<128, 0, 3> * 512 139264 grids t1 16/16/16 t3 48/48/48 t14 224/224/224
conv cout 128 ks 3 ups 1 kt 1 variant 0  8x64 : void ifx::conv::conv_cl_kernel<128, 1, 3> * 512 139264 grids t1 8/8/8 t3 16/16/16 t16 64/64/64
conv cout 128 ks 3 ups 1 kt 1 variant 0 13x70 : void ifx::conv::conv_cl_kernel<128, 1, 3> * 512 139264 grids t1 16/16/16 t3 40/40/40 t16 192/192/192
conv cout 128 ks 3 ups 1 kt 1 variant 0 60x104: void ifx::conv::conv_cl_kernel<128, 1, 3> * 512 139264 grids t1 64/64/64 t3 184/184/184 t16 960/960/960
conv cout 128 ks 3 ups 1 kt 1 variant 1  8x64 : void ifx::conv::conv_cl_kernel<128, 1, 3> * 512 139264 grids t1 8/8/8 t3 16/16/16 t16 64/64/64
conv cout 128 ks 3 ups 1 kt 1 variant 1 13x70 : void ifx::conv::conv_cl_kernel<128, 1, 3> * 512 139264 grids t1 16/16/16 t3 40/40/40 t16 192/192/192
conv cout 128 ks 3 ups 1 kt 1 variant 1 60x104: void ifx::conv::conv_cl_kernel<128, 1, 3> * 512 139264 grids t1 64/64/64 t3 184/184/184 t16 960/960/960
conv cout 128 ks 3 ups 1 kt 3 variant 0  8x64 : void ifx::conv::conv_cl_kernel<128, 1, 3> * 512 139264 grids t1 8/8/8 t3 16/16/16 t14 56/56/56
conv cout 128 ks 3 ups 1 kt 3 variant 0 13x70 : void ifx::conv::conv_cl_kernel<128, 1, 3> * 512 139264 grids t1 16/16/16 t3 40/40/40 t14 168/168/168
conv cout 128 ks 3 ups 1 kt 3 variant 0 60x104: void ifx::conv::conv_cl_kernel<128, 1, 3> * 512 139264 grids t1 64/64/64 t3 184/184/184 t14 840/840/840
conv cout 128 ks 3 ups 1 kt 3 variant 1  8x64 : void ifx::conv::conv_cl_kernel<128, 1, 3> * 512 139264 grids t1 8/8/8 t3 16/16/16 t14 56/56/56
conv cout 128 ks 3 ups 1 kt 3 variant 1 13x70 : void ifx::conv::conv_cl_kernel<128, 1, 3> * 512 139264 grids t1 16/16/16 t3 40/40/40 t14 168/168/168
conv cout 128 ks 3 ups 1 kt 3 variant 1 60x104: void ifx::conv::conv_cl_kernel<128, 1, 3> * 512 139264 grids t1 64/64/64 t3 184/184/184 t14 840/840/840
conv cout 160 ks 1 ups 0 kt 1 variant 0  8x64 : void ifx::conv::conv_cl_kernel<128, 0, 1> * 512 139264 grids t1 8/8/8 t3 8/8/8 t16 32/32/32
conv cout 160 ks 1 ups 0 kt 1 variant 0 13x70 : void ifx::conv::conv_cl_kernel<128, 0, 1> * 512 139264 grids t1 8/8/8 t3 24/24/24 t16 128/128/128
conv cout 160 ks 1 ups 0 kt 1 variant 0 60x104: void ifx::conv::conv_cl_kernel<128, 0, 1> * 512 139264 grids t1 32/32/32 t3 96/96/96 t16 512/512/512
conv cout 160 ks 1 ups 0 kt 1 variant 1  8x64 : void ifx::conv::conv_cl_kernel<128, 0, 1> * 512 139264 grids t1 8/8/8 t3 8/8/8 t16 32/32/32
conv cout 160 ks 1 ups 0 kt 1 variant 1 13x70 : void ifx::conv::conv_cl_kernel<128, 0, 1> * 512 139264 grids t1 8/8/8 t3 24/24/24 t16 128/128/128
conv cout 160 ks 1 ups 0 kt 1 variant 1 60x104: void ifx::conv::conv_cl_kernel<128, 0, 1> * 512 139264 grids t1 32/32/32 t3 96/96/96 t16 512/512/512
conv cout 160 ks 1 ups 0 kt 3 variant 0  8x64 : void ifx::conv::conv_cl_kernel<128, 0, 1> * 512 139264 grids t1 8/8/8 t3 8/8/8 t14 32/32/32
conv cout 160 ks 1 ups 0 kt 3 variant 0 13x70 : void ifx::conv::conv_cl_kernel<128, 0, 1> * 512 139264 grids t1 8/8/8 t3 24/24/24 t14 112/112/112
conv cout 160 ks 1 ups 0 kt 3 variant 0 60x104: void ifx::conv::conv_cl_kernel<128, 0, 1> * 512 139264 grids t1 32/32/32 t3 96/96/96 t14 448/448/448
conv cout 160 ks 1 ups 0 kt 3 variant 1  8x64 : void ifx::conv::conv_cl_kernel<128, 0, 1> * 512 139264 grids t1 8/8/8 t3 8/8/8 t14 32/32/32
conv cout 160 ks 1 ups 0 kt 3 variant 1 13x70 : void ifx::conv::conv_cl_kernel<128, 0, 1> * 512 139264 grids t1 8/8/8 t3 24/24/24 t14 112/112/112
conv cout 160 ks 1 ups 0 kt 3 variant 1 60x104: void ifx::conv::conv_cl_kernel<128, 0, 1> * 512 139264 grids t1 32/32/32 t3 96/96/96 t14 448/448/448
conv cout 160 ks 3 ups 0 kt 1 variant 0  8x64 : void ifx::conv::conv_cl_kernel<128, 0, 3> * 512 139264 grids t1 8/8/8 t3 8/8/8 t16 32/32/32
conv cout 160 ks 3 ups 0 kt 1 variant 0 13x70 : void ifx::conv::conv_cl_kernel<128, 0, 3> * 512 139264 grids t1 8/8/8 t3 24/24/24 t16 128/128/128
conv cout 160 ks 3 ups 0 kt 1 variant 0 60x104: void ifx::conv::conv_cl_kernel<128, 0, 3> * 512 139264 grids t1 32/32/32 t3 96/96/96 t16 512/512/512
conv cout 160 ks 3 ups 0 kt 1 variant 1  8x64 : void ifx::conv::conv_cl_kernel<128, 0, 3> * 512 139264 grids t1 8/8/8 t3 8/8/8 t16 32/32/32
conv cout 160 ks 3 ups 0 kt 1 variant 1 13x70 : void ifx::conv::conv_cl_kernel<128, 0, 3> * 512 139264 grids t1 8/8/8 t3 24/24/24 t16 128/128/128
conv cout 160 ks 3 ups 0 kt 1 variant 1 60x104: void ifx::conv::conv_cl_kernel<128, 0, 3> * 512 139264 grids t1 32/32/32 t3 96/96/96 t16 512/512/512
conv cout 160 ks 3 ups 0 kt 3 variant 0  8x64 : void ifx::conv::conv_cl_kernel<128, 0, 3> * 512 139264 grids t1 8/8/8 t3 8/8/8 t14 32/32/32
conv cout 160 ks 3 ups 0 kt 3 variant 0 13x70 : void ifx::conv::conv_cl_kernel<128, 0, 3> * 512 139264 grids t1 8/8/8 t3 24/24/24 t14 112/112/112
conv cout 160 ks 3 ups 0 kt 3 variant 0 60x104: void ifx::conv::conv_cl_kernel<128, 0, 3> * 512 139264 grids t1 32/32/32 t3 96/96/96 t14 448/448/448
conv cout 160 ks 3 ups 0 kt 3 variant 1  8x64 : void ifx::conv::conv_cl_kernel<128, 0, 3> * 512 139264 grids t1 8/8/8 t3 8/8/8 t14 32/32/32
conv cout 160 ks 3 ups 0 kt 3 variant 1 13x70 : void ifx::conv::conv_cl_kernel<128, 0, 3> * 512 139264 grids t1 8/8/8 t3 24/24/24 t14 112/112/112
conv cout 160 ks 3 ups 0 kt 3 variant 1 60x104: void ifx::conv::conv_cl_kernel<128, 0, 3> * 512 139264 grids t1 32/32/32 t3 96/96/96 t14 448/448/448
conv cout 160 ks 3 ups 1 kt 1 variant 0  8x64 : void ifx::conv::conv_cl_kernel<128, 1, 3> * 512 139264 grids t1 8/8/8 t3 24/24/24 t16 128/128/128
conv cout 160 ks 3 ups 1 kt 1 variant 0 13x70 : void ifx::conv::conv_cl_kernel<128, 1, 3> * 512 139264 grids t1 24/24/24 t3 72/72/72 t16 384/384/384
conv cout 160 ks 3 ups 1 kt 1 variant 0 60x104: void ifx::conv::conv_cl_kernel<128, 1, 3> * 512 139264 grids t1 120/120/120 t3 360/360/360 t16 1920/1920/1920
conv cout 160 ks 3 ups 1 kt 1 variant 1  8x64 : void ifx::conv::conv_cl_kernel<128, 1, 3> * 512 139264 grids t1 8/8/8 t3 24/24/24 t16 128/128/128
conv cout 160 ks 3 ups 1 kt 1 variant 1 13x70 : void ifx::conv::conv_cl_kernel<128, 1, 3> * 512 139264 grids t1 24/24/24 t3 72/72/72 t16 384/384/384
conv cout 160 ks 3 ups 1 kt 1 variant 1 60x104: void ifx::conv::conv_cl_kernel<128, 1, 3> * 512 139264 grids t1 120/120/120 t3 360/360/360 t16 1920/1920/1920
conv cout 160 ks 3 ups 1 kt 3 variant 0  8x64 : void ifx::conv::conv_cl_kernel<128, 1, 3> * 512 139264 grids t1 8/8/8 t3 24/24/24 t14 112/112/112
conv cout 160 ks 3 ups 1 kt 3 variant 0 13x70 : void ifx::conv::conv_cl_kernel<128, 1, 3> * 512 139264 grids t1 24/24/24 t3 72/72/72 t14 336/336/336
conv cout 160 ks 3 ups 1 kt 3 variant 0 60x104: void ifx::conv::conv_cl_kernel<128, 1, 3> * 512 139264 grids t1 120/120/120 t3 360/360/360 t14 1680/1680/1680
conv cout 160 ks 3 ups 1 kt 3 variant 1  8x64 : void ifx::conv::conv_cl_kernel<128, 1, 3> * 512 139264 grids t1 8/8/8 t3 24/24/24 t14 112/112/112
conv cout 160 ks 3 ups 1 kt 3 variant 1 13x70 : void ifx::conv::conv_cl_kernel<128, 1, 3> * 512 139264 grids t1 24/24/24 t3 72/72/72 t14 336/336/336
conv cout 160 ks 3 ups 1 kt 3 variant 1 60x104: void ifx::conv::conv_cl_kernel<128, 1, 3> * 512 139264 grids t1 120/120/120 t3 360/360/360 t14 1680/1680/1680
conv cout 192 ks 1 ups 0 kt 1 variant 0  8x64 : void ifx::conv::conv_cl_kernel<96, 0, 1> * 512 106496 grids t1 8/8/8 t3 8/8/8 t16 32/32/32
conv cout 192 ks 1 ups 0 kt 1 variant 0 13x70 : void ifx::conv::conv_cl_kernel<96, 0, 1> * 512 106496 grids t1 8/8/8 t3 24/24/24 t16 128/128/128
conv cout 192 ks 1 ups 0 kt 1 variant 0 60x104: void ifx::conv::conv_cl_kernel<96, 0, 1> * 512 106496 grids t1 32/32/32 t3 96/96/96 t16 512/512/512
conv cout 192 ks 1 ups 0 kt 1 variant 1  8x64 : void ifx::conv::conv_cl_kernel<96, 0, 1> * 512 106496 grids t1 8/8/8 t3 8/8/8 t16 32/32/32
conv cout 192 ks 1 ups 0 kt 1 variant 1 13x70 : void ifx::conv::conv_cl_kernel<96, 0, 1> * 512 106496 grids t1 8/8/8 t3 24/24/24 t16 128/128/128
conv cout 192 ks 1 ups 0 kt 1 variant 1 60x104: void ifx::conv::conv_cl_kernel<96, 0, 1> * 512 106496 grids t1 32/32/32 t3 96/96/96 t16 512/512/512
conv cout 192 ks 1 ups 0 kt 3 variant 0  8x64 : void ifx::conv::conv_cl_kernel<96, 0, 1> * 512 106496 grids t1 8/8/8 t3 8/8/8 t14 32/32/32
conv cout 192 ks 1 ups 0 kt 3 variant 0 13x70 : void ifx::conv::conv_cl_kernel<96, 0, 1> * 512 106496 grids t1 8/8/8 t3 24/24/24 t14 112/112/112
conv cout 192 ks 1 ups 0 kt 3 variant 0 60x104: void ifx::conv::conv_cl_kernel<96, 0, 1> * 512 106496 grids t1 32/32/32 t3 96/96/96 t14 448/448/448
conv cout 192 ks 1 ups 0 kt 3 variant 1  8x64 : void ifx::conv::conv_cl_kernel<96, 0, 1> * 512 106496 grids t1 8/8/8 t3 8/8/8 t14 32/32/32
conv cout 192 ks 1 ups 0 kt 3 variant 1 13x70 : void ifx::conv::conv_cl_kernel<96, 0, 1> * 512 106496 grids t1 8/8/8 t3 24/24/24 t14 112/112/112
conv cout 192 ks 1 ups 0 kt 3 variant 1 60x104: void ifx::conv::conv_cl_kernel<96, 0, 1> * 512 106496 grids t1 32/32/32 t3 96/96/96 t14 448/448/448
conv cout 192 ks 3 ups 0 kt 1 variant 0  8x64 : void ifx::conv::pp::conv_pp_kernel<96, 0> * 512 152576 grids t1 8/8/8 t3 8/8/8 t16 32/32/32
conv cout 192 ks 3 ups 0 kt 1 variant 0 13x70 : void ifx::conv::pp::conv_pp_kernel<96, 0> * 512 152576 grids t1 8/8/8 t3 24/24/24 t16 128/128/64
conv cout 192 ks 3 ups 0 kt 1 variant 0 60x104: void ifx::conv::pp::conv_pp_kernel<96, 0> * 512 152576 grids t1 32/32/32 t3 96/96/64 t16 256/304/64
conv cout 192 ks 3 ups 0 kt 1 variant 1  8x64 : void ifx::conv::conv_cl_kernel<96, 0, 3> * 512 145408 grids t1 8/8/8 t3 8/8/8 t16 32/32/32
conv cout 192 ks 3 ups 0 kt 1 variant 1 13x70 : void ifx::conv::conv_cl_kernel<96, 0, 3> * 512 145408 grids t1 8/8/8 t3 24/24/24 t16 128/128/128
conv cout 192 ks 3 ups 0 kt 1 variant 1 60x104: void ifx::conv::conv_cl_kernel<96, 0, 3> * 512 145408 grids t1 32/32/32 t3 96/96/96 t16 512/512/512
conv cout 192 ks 3 ups 0 kt 3 variant 0  8x64 : void ifx::conv::pp::conv_pp_kernel<96, 0> * 512 152576 grids t1 8/8/8 t3 8/8/8 t14 32/32/32
conv cout 192 ks 3 ups 0 kt 3 variant 0 13x70 : void ifx::conv::pp::conv_pp_kernel<96, 0> * 512 152576 grids t1 8/8/8 t3 24/24/24 t14 112/112/64
conv cout 192 ks 3 ups 0 kt 3 variant 0 60x104: void ifx::conv::pp::conv_pp_kernel<96, 0> * 512 152576 grids t1 32/32/32 t3 96/96/64 t14 256/304/64
conv cout 192 ks 3 ups 0 kt 3 variant 1  8x64 : void ifx::conv::conv_cl_kernel<96, 0, 3> * 512 145408 grids t1 8/8/8 t3 8/8/8 t14 32/32/32
conv cout 192 ks 3 ups 0 kt 3 variant 1 13x70 : void ifx::conv::conv_cl_kernel<96, 0, 3> * 512 145408 grids t1 8/8/8 t3 24/24/24 t14 112/112/112
conv cout 192 ks 3 ups 0 kt 3 variant 1 60x104: void ifx::conv::conv_cl_kernel<96, 0, 3> * 512 145408 grids t1 32/32/32 t3 96/96/96 t14 448/448/448
conv cout 192 ks 3 ups 1 kt 1 variant 0  8x64 : void ifx::conv::pp::conv_pp_kernel<96, 1> * 512 93184 grids t1 8/8/8 t3 24/24/24 t16 128/128/64
conv cout 192 ks 3 ups 1 kt 1 variant 0 13x70 : void ifx::conv::pp::conv_pp_kernel<96, 1> * 512 93184 grids t1 24/24/24 t3 72/72/64 t16 256/304/64
conv cout 192 ks 3 ups 1 kt 1 variant 0 60x104: void ifx::conv::pp::conv_pp_kernel<96, 1> * 512 93184 grids t1 120/120/64 t3 256/304/64 t16 256/304/64
conv cout 192 ks 3 ups 1 kt 1 variant 1  8x64 : void ifx::conv::conv_cl_kernel<96, 1, 3> * 512 106496 grids t1 8/8/8 t3 24/24/24 t16 128/128/128
conv cout 192 ks 3 ups 1 kt 1 variant 1 13x70 : void ifx::conv::conv_cl_kernel<96, 1, 3> * 512 106496 grids t1 24/24/24 t3 72/72/72 t16 384/384/384
conv cout 192 ks 3 ups 1 kt 1 variant 1 60x104: void ifx::conv::conv_cl_kernel<96, 1, 3> * 512 106496 grids t1 120/120/120 t3 360/360/360 t16 1920/1920/1920
conv cout 192 ks 3 ups 1 kt 3 variant 0  8x64 : void ifx::conv::pp::conv_pp_kernel<96, 1> * 512 93184 grids t1 8/8/8 t3 24/24/24 t14 112/112/64
conv cout 192 ks 3 ups 1 kt 3 variant 0 13x70 : void ifx::conv::pp::conv_pp_kernel<96, 1> * 512 93184 grids t1 24/24/24 t3 72/72/64 t14 256/304/64
conv cout 192 ks 3 ups 1 kt 3 variant 0 60x104: void ifx::conv::pp::conv_pp_kernel<96, 1> * 512 93184 grids t1 120/120/64 t3 256/304/64 t14 256/304/64
conv cout 192 ks 3 ups 1 kt 3 variant 1  8x64 : void ifx::conv::conv_cl_kernel<96, 1, 3> * 512 106496 grids t1 8/8/8 t3 24/24/24 t14 112/112/112
conv cout 192 ks 3 ups 1 kt 3 variant 1 13x70 : void ifx::conv::conv_cl_kernel<96, 1, 3> * 512 106496 grids t1 24/24/24 t3 72/72/72 t14 336/336/336
conv cout 192 ks 3 ups 1 kt 3 variant 1 60x104: void ifx::conv::conv_cl_kernel<96, 1, 3> * 512 106496 grids t1 120/120/120 t3 360/360/360 t14 1680/1680/1680
conv cout 288 ks 1 ups 0 kt 1 variant 0  8x64 : void ifx::conv::conv_cl_kernel<96, 0, 1> * 512 106496 grids t1 8/8/8 t3 16/16/16 t16 48/48/48
conv cout 288 ks 1 ups 0 kt 1 variant 0 13x70 : void ifx::conv::conv_cl_kernel<96, 0, 1> * 512 106496 grids t1 16/16/16 t3 40/40/40 t16 192/192/192
conv cout 288 ks 1 ups 0 kt 1 variant 0 60x104: void ifx::conv::conv_cl_kernel<96, 0, 1> * 512 106496 grids t1 48/48/48 t3 144/144/144 t16 768/768/768
conv cout 288 ks 1 ups 0 kt 1 variant 1  8x64 : void ifx::conv::conv_cl_kernel<96, 0, 1> * 512 106496 grids t1 8/8/8 t3 16/16/16 t16 48/48/48
conv cout 288 ks 1 ups 0 kt 1 variant 1 13x70 : void ifx::conv::conv_cl_kernel<96, 0, 1> * 512 106496 grids t1 16/16/16 t3 40/40/40 t16 192/192/192
conv cout 288 ks 1 ups 0 kt 1 variant 1 60x104: void ifx::conv::conv_cl_kernel<96, 0, 1> * 512 106496 grids t1 48/48/48 t3 144/144/144 t16 768/768/768
conv cout 288 ks 1 ups 0 kt 3 variant 0  8x64 : void ifx::conv::conv_cl_kernel<96, 0, 1> * 512 106496 grids t1 8/8/8 t3 16/16/16 t14 48/48/48
conv cout 288 ks 1 ups 0 kt 3 variant 0 13x70 : void ifx::conv::conv_cl_kernel<96, 0, 1> * 512 106496 grids t1 16/16/16 t3 40/40/40 t14 168/168/168
conv cout 288 ks 1 ups 0 kt 3 variant 0 60x104: void ifx::conv::conv_cl_kernel<96, 0, 1> * 512 106496 grids t1 48/48/48 t3 144/144/144 t14 672/672/672
conv cout 288 ks 1 ups 0 kt 3 variant 1  8x64 : void ifx::conv::conv_cl_kernel<96, 0, 1> * 512 106496 grids t1 8/8/8 t3 16/16/16 t14 48/48/48
conv cout 288 ks 1 ups 0 kt 3 variant 1 13x70 : void ifx::conv::conv_cl_kernel<96, 0, 1> * 512 106496 grids t1 16/16/16 t3 40/40/40 t14 168/168/168
conv cout 288 ks 1 ups 0 kt 3 variant 1 60x104: void ifx::conv::conv_cl_kernel<96, 0, 1> * 512 106496 grids t1 48/48/48 t3 144/144/144 t14 672/672/672
conv cout 288 ks 3 ups 0 kt 1 variant 0  8x64 : void ifx::conv::pp::conv_pp_kernel<96, 0> * 512 152576 grids t1 8/8/8 t3 16/16/16 t16 48/48/48
conv cout 288 ks 3 ups 0 kt 1 variant 0 13x70 : void ifx::conv::pp::conv_pp_kernel<96, 0> * 512 152576 grids t1 16/16/16 t3 40/40/40 t16 192/192/64
conv cout 288 ks 3 ups 0 kt 1 variant 0 60x104: void ifx::conv::pp::conv_pp_kernel<96, 0> * 512 152576 grids t1 48/48/48 t3 144/144/64 t16 256/304/64
conv cout 288 ks 3 ups 0 kt 1 variant 1  8x64 : void ifx::conv::conv_cl_kernel<96, 0, 3> * 512 145408 grids t1 8/8/8 t3 16/16/16 t16 48/48/48
conv cout 288 ks 3 ups 0 kt 1 variant 1 13x70 : void ifx::conv::conv_cl_kernel<96, 0, 3> * 512 145408 grids t1 16/16/16 t3 40/40/40 t16 192/192/192
conv cout 288 ks 3 ups 0 kt 1 variant 1 60x104: void ifx::conv::conv_cl_kernel<96, 0, 3> * 512 145408 grids t1 48/48/48 t3 144/144/144 t16 768/768/768
conv cout 288 ks 3 ups 0 kt 3 variant 0  8x64 : void ifx::conv::pp::conv_pp_kernel<96, 0> * 512 152576 grids t1 8/8/8 t3 16/16/16 t14 48/48/48
conv cout 288 ks 3 ups 0 kt 3 variant 0 13x70 : void ifx::conv::pp::conv_pp_kernel<96, 0> * 512 152576 grids t1 16/16/16 t3 40/40/40 t14 168/168/64
conv cout 288 ks 3 ups 0 kt 3 variant 0 60x104: void ifx::conv::pp::conv_pp_kernel<96, 0> * 512 152576 grids t1 48/48/48 t3 144/144/64 t14 256/304/64
conv cout 288 ks 3 ups 0 kt 3 variant 1  8x64 : void ifx::conv::conv_cl_kernel<96, 0, 3> * 512 145408 grids t1 8/8/8 t3 16/16/16 t14 48/48/48
conv cout 288 ks 3 ups 0 kt 3 variant 1 13x70 : void ifx::conv::conv_cl_kernel<96, 0, 3> * 512 145408 grids t1 16/16/16 t3 40/40/40 t14 168/168/168
conv cout 288 ks 3 ups 0 kt 3 variant 1 60x104: void ifx::conv::conv_cl_kernel<96, 0, 3> * 512 145408 grids t1 48/48/48 t3 144/144/144 t14 672/672/672
conv cout 288 ks 3 ups 1 kt 1 variant 0  8x64 : void ifx::conv::pp::conv_pp_kernel<96, 1> * 512 93184 grids t1 16/16/16 t3 40/40/40 t16 192/192/64
conv cout 288 ks 3 ups 1 kt 1 variant 0 13x70 : void ifx::conv::pp::conv_pp_kernel<96, 1> * 512 93184 grids t1 40/40/40 t3 112/112/64 t16 256/304/64
conv cout 288 ks 3 ups 1 kt 1 variant 0 60x104: void ifx::conv::pp::conv_pp_kernel<96, 1> * 512 93184 grids t1 184/184/64 t3 256/304/64 t16 256/304/64
conv cout 288 ks 3 ups 1 kt 1 variant 1  8x64 : void ifx::conv::conv_cl_kernel<96, 1, 3> * 512 106496 grids t1 16/16/16 t3 40/40/40 t16 192/192/192
conv cout 288 ks 3 ups 1 kt 1 variant 1 13x70 : void ifx::conv::conv_cl_kernel<96, 1, 3> * 512 106496 grids t1 40/40/40 t3 112/112/112 t16 576/576/576
conv cout 288 ks 3 ups 1 kt 1 variant 1 60x104: void ifx::conv::conv_cl_kernel<96, 1, 3> * 512 106496 grids t1 184/184/184 t3 544/544/544 t16 2880/2880/2880
conv cout 288 ks 3 ups 1 kt 3 variant 0  8x64 : void ifx::conv::pp::conv_pp_kernel<96, 1> * 512 93184 grids t1 16/16/16 t3 40/40/40 t14 168/168/64
conv cout 288 ks 3 ups 1 kt 3 variant 0 13x70 : void ifx::conv::pp::conv_pp_kernel<96, 1> * 512 93184 grids t1 40/40/40 t3 112/112/64 t14 256/304/64
conv cout 288 ks 3 ups 1 kt 3 variant 0 60x104: void ifx::conv::pp::conv_pp_kernel<96, 1> * 512 93184 grids t1 184/184/64 t3 256/304/64 t14 256/304/64
conv cout 288 ks 3 ups 1 kt 3 variant 1  8x64 : void ifx::conv::conv_cl_kernel<96, 1, 3> * 512 106496 grids t1 16/16/16 t3 40/40/40 t14 168/168/168
conv cout 288 ks 3 ups 1 kt 3 variant 1 13x70 : void ifx::conv::conv_cl_kernel<96, 1, 3> * 512 106496 grids t1 40/40/40 t3 112/112/112 t14 504/504/504
conv cout 288 ks 3 ups 1 kt 3 variant 1 60x104: void ifx::conv::conv_cl_kernel<96, 1, 3> * 512 106496 grids t1 184/184/184 t3 544/544/544 t14 2520/2520/2520
conv cout 384 ks 1 ups 0 kt 1 variant 0  8x64 : void ifx::conv::conv_cl_kernel<96, 0, 1> * 512 106496 grids t1 8/8/8 t3 16/16/16 t16 64/64/64
conv cout 384 ks 1 ups 0 kt 1 variant 0 13x70 : void ifx::conv::conv_cl_kernel<96, 0, 1> * 512 106496 grids t1 16/16/16 t3 48/48/48 t16 256/256/256
conv cout 384 ks 1 ups 0 kt 1 variant 0 60x104: void ifx::conv::conv_cl_kernel<96, 0, 1> * 512 106496 grids t1 64/64/64 t3 192/192/192 t16 1024/1024/1024
conv cout 384 ks 1 ups 0 kt 1 variant 1  8x64 : void ifx::conv::conv_cl_kernel<96, 0, 1> * 512 106496 grids t1 8/8/8 t3 16/16/16 t16 64/64/64
conv cout 384 ks 1 ups 0 kt 1 variant 1 13x70 : void ifx::conv::conv_cl_kernel<96, 0, 1> * 512 106496 grids t1 16/16/16 t3 48/48/48 t16 256/256/256
conv cout 384 ks 1 ups 0 kt 1 variant 1 60x104: void ifx::conv::conv_cl_kernel<96, 0, 1> * 512 106496 grids t1 64/64/64 t3 192/192/192 t16 1024/1024/1024
conv cout 384 ks 1 ups 0 kt 3 variant 0  8x64 : void ifx::conv::conv_cl_kernel<96, 0, 1> * 512 106496 grids t1 8/8/8 t3 16/16/16 t14 56/56/56
conv cout 384 ks 1 ups 0 kt 3 variant 0 13x70 : void ifx::conv::conv_cl_kernel<96, 0, 1> * 512 106496 grids t1 16/16/16 t3 48/48/48 t14 224/224/224
conv cout 384 ks 1 ups 0 kt 3 variant 0 60x104: void ifx::conv::conv_cl_kernel<96, 0, 1> * 512 106496 grids t1 64/64/64 t3 192/192/192 t14 896/896/896
conv cout 384 ks 1 ups 0 kt 3 variant 1  8x64 : void ifx::conv::conv_cl_kernel<96, 0, 1> * 512 106496 grids t1 8/8/8 t3 16/16/16 t14 56/56/56
conv cout 384 ks 1 ups 0 kt 3 variant 1 13x70 : void ifx::conv::conv_cl_kernel<96, 0, 1> * 512 106496 grids t1 16/16/16 t3 48/48/48 t14 224/224/224
conv cout 384 ks 1 ups 0 kt 3 variant 1 60x104: void ifx::conv::conv_cl_kernel<96, 0, 1> * 512 106496 grids t1 64/64/64 t3 192/192/192 t14 896/896/896
conv cout 384 ks 3 ups 0 kt 1 variant 0  8x64 : void ifx::conv::pp::conv_pp_kernel<96, 0> * 512 152576 grids t1 8/8/8 t3 16/16/16 t16 64/64/64
conv cout 384 ks 3 ups 0 kt 1 variant 0 13x70 : void ifx::conv::pp::conv_pp_kernel<96, 0> * 512 152576 grids t1 16/16/16 t3 48/48/48 t16 256/256/64
conv cout 384 ks 3 ups 0 kt 1 variant 0 60x104: void ifx::conv::pp::conv_pp_kernel<96, 0> * 512 152576 grids t1 64/64/64 t3 192/192/64 t16 256/304/64
conv cout 384 ks 3 ups 0 kt 1 variant 1  8x64 : void ifx::conv::conv_cl_kernel<96, 0, 3> * 512 145408 grids t1 8/8/8 t3 16/16/16 t16 64/64/64
conv cout 384 ks 3 ups 0 kt 1 variant 1 13x70 : void ifx::conv::conv_cl_kernel<96, 0, 3> * 512 145408 grids t1 16/16/16 t3 48/48/48 t16 256/256/256
conv cout 384 ks 3 ups 0 kt 1 variant 1 60x104: void ifx::conv::conv_cl_kernel<96, 0, 3> * 512 145408 grids t1 64/64/64 t3 192/192/192 t16 1024/1024/1024
conv cout 384 ks 3 ups 0 kt 3 variant 0  8x64 : void ifx::conv::pp::conv_pp_kernel<96, 0> * 512 152576 grids t1 8/8/8 t3 16/16/16 t14 56/56/56
conv cout 384 ks 3 ups 0 kt 3 variant 0 13x70 : void ifx::conv::pp::conv_pp_kernel<96, 0> * 512 152576 grids t1 16/16/16 t3 48/48/48 t14 224/224/64
conv cout 384 ks 3 ups 0 kt 3 variant 0 60x104: void ifx::conv::pp::conv_pp_kernel<96, 0> * 512 152576 grids t1 64/64/64 t3 192/192/64 t14 256/304/64
conv cout 384 ks 3 ups 0 kt 3 variant 1  8x64 : void ifx::conv::conv_cl_kernel<96, 0, 3> * 512 145408 grids t1 8/8/8 t3 16/16/16 t14 56/56/56
conv cout 384 ks 3 ups 0 kt 3 variant 1 13x70 : void ifx::conv::conv_cl_kernel<96, 0, 3> * 512 145408 grids t1 16/16/16 t3 48/48/48 t14 224/224/224
conv cout 384 ks 3 ups 0 kt 3 variant 1 60x104: void ifx::conv::conv_cl_kernel<96, 0, 3> * 512 145408 grids t1 64/64/64 t3 192/192/192 t14 896/896/896
conv cout 384 ks 3 ups 1 kt 1 variant 0  8x64 : void ifx::conv::pp::conv_pp_kernel<96, 1> * 512 93184 grids t1 16/16/16 t3 48/48/48 t16 256/256/64
conv cout 384 ks 3 ups 1 kt 1 variant 0 13x70 : void ifx::conv::pp::conv_pp_kernel<96, 1> * 512 93184 grids t1 48/48/48 t3 144/144/64 t16 256/304/64
conv cout 384 ks 3 ups 1 kt 1 variant 0 60x104: void ifx::conv::pp::conv_pp_kernel<96, 1> * 512 93184 grids t1 240/240/64 t3 256/304/64 t16 256/304/64
conv cout 384 ks 3 ups 1 kt 1 variant 1  8x64 : void ifx::conv::conv_cl_kernel<96, 1, 3> * 512 106496 grids t1 16/16/16 t3 48/48/48 t16 256/256/256
conv cout 384 ks 3 ups 1 kt 1 variant 1 13x70 : void ifx::conv::conv_cl_kernel<96, 1, 3> * 512 106496 grids t1 48/48/48 t3 144/144/144 t16 768/768/768
conv cout 384 ks 3 ups 1 kt 1 variant 1 60x104: void ifx::conv::conv_cl_kernel<96, 1, 3> * 512 106496 grids t1 240/240/240 t3 720/720/720 t16 3840/3840/3840
conv cout 384 ks 3 ups 1 kt 3 variant 0  8x64 : void ifx::conv::pp::conv_pp_kernel<96, 1> * 512 93184 grids t1 16/16/16 t3 48/48/48 t14 224/224/64
conv cout 384 ks 3 ups 1 kt 3 variant 0 13x70 : void ifx::conv::pp::conv_pp_kernel<96, 1> * 512 93184 grids t1 48/48/48 t3 144/144/64 t14 256/304/64
conv cout 384 ks 3 ups 1 kt 3 variant 0 60x104: void ifx::conv::pp::conv_pp_kernel<96, 1> * 512 93184 grids t1 240/240/64 t3 256/304/64 t14 256/304/64
conv cout 384 ks 3 ups 1 kt 3 variant 1  8x64 : void ifx::conv::conv_cl_kernel<96, 1, 3> * 512 106496 grids t1 16/16/16 t3 48/48/48 t14 224/224/224
conv cout 384 ks 3 ups 1 kt 3 variant 1 13x70 : void ifx::conv::conv_cl_kernel<96, 1, 3> * 512 106496 grids t1 48/48/48 t3 144/144/144 t14 672/672/672
conv cout 384 ks 3 ups 1 kt 3 variant 1 60x104: void ifx::conv::conv_cl_kernel<96, 1, 3> * 512 106496 grids t1 240/240/240 t3 720/720/720 t14 3360/3360/3360
conv cout 512 ks 1 ups 0 kt 1 variant 0  8x64 : void ifx::conv::conv_cl_kernel<128, 0, 1> * 512 139264 grids t1 8/8/8 t3 16/16/16 t16 64/64/64
conv cout 512 ks 1 ups 0 kt 1 variant 0 13x70 : void ifx::conv::conv_cl_kernel<128, 0, 1> * 512 139264 grids t1 16/16/16 t3 48/48/48 t16 256/256/256
conv cout 512 ks 1 ups 0 kt 1 variant 0 60x104: void ifx::conv::conv_cl_kernel<128, 0, 1> * 512 139264 grids t1 64/64/64 t3 192/192/192 t16 1024/1024/1024
conv cout 512 ks 1 ups 0 kt 1 variant 1  8x64 : void ifx::conv::conv_cl_kernel<128, 0, 1> * 512 139264 grids t1 8/8/8 t3 16/16/16 t16 64/64/64
conv cout 512 ks 1 ups 0 kt 1 variant 1 13x70 : void ifx::conv::conv_cl_kernel<128, 0, 1> * 512 139264 grids t1 16/16/16 t3 48/48/48 t16 256/256/256
conv cout 512 ks 1 ups 0 kt 1 variant 1 60x104: void ifx::conv::conv_cl_kernel<128, 0, 1> * 512 139264 grids t1 64/64/64 t3 192/192/192 t16 1024/1024/1024
conv cout 512 ks 1 ups 0 kt 3 variant 0  8x64 : void ifx::conv::conv_cl_kernel<128, 0, 1> * 512 139264 grids t1 8/8/8 t3 16/16/16 t14 56/56/56
conv cout 512 ks 1 ups 0 kt 3 variant 0 13x70 : void ifx::conv::conv_cl_kernel<128, 0, 1> * 512 139264 grids t1 16/16/16 t3 48/48/48 t14 224/224/224
conv cout 512 ks 1 ups 0 kt 3 variant 0 60x104: void ifx::conv::conv_cl_kernel<128, 0, 1> * 512 139264 grids t1 64/64/64 t3 192/192/192 t14 896/896/896
conv cout 512 ks 1 ups 0 kt 3 variant 1  8x64 : void ifx::conv::conv_cl_kernel<128, 0, 1> * 512 139264 grids t1 8/8/8 t3 16/16/16 t14 56/56/56
conv cout 512 ks 1 ups 0 kt 3 variant 1 13x70 : void ifx::conv::conv_cl_kernel<128, 0, 1> * 512 139264 grids t1 16/16/16 t3 48/48/48 t14 224/224/224
conv cout 512 ks 1 ups 0 kt 3 variant 1 60x104: void ifx::conv::conv_cl_kernel<128, 0, 1> * 512 139264 grids t1 64/64/64 t3 192/192/192 t14 896/896/896
conv cout 512 ks 3 ups 0 kt 1 variant 0  8x64 : void ifx::conv::conv_cl_kernel<128, 0, 3> * 512 139264 grids t1 8/8/8 t3 16/16/16 t16 64/64/64
conv cout 512 ks 3 ups 0 kt 1 variant 0 13x70 : void ifx::conv::conv_cl_kernel<128, 0, 3> * 512 139264 grids t1 16/16/16 t3 48/48/48 t16 256/256/256
conv cout 512 ks 3 ups 0 kt 1 variant 0 60x104: void ifx::conv::conv_cl_kernel<128, 0, 3> * 512 139264 grids t1 64/64/64 t3 192/192/192 t16 1024/1024/1024
conv cout 512 ks 3 ups 0 kt 1 variant 1  8x64 : void ifx::conv::conv_cl_kernel<128, 0, 3> * 512 139264 grids t1 8/8/8 t3 16/16/16 t16 64/64/64
conv cout 512 ks 3 ups 0 kt 1 variant 1 13x70 : void ifx::conv::conv_cl_kernel<128, 0, 3> * 512 139264 grids t1 16/16/16 t3 48/48/48 t16 256/256/256
conv cout 512 ks 3 ups 0 kt 1 variant 1 60x104: void ifx::conv::conv_cl_kernel<128, 0, 3> * 512 139264 grids t1 64/64/64 t3 192/192/192 t16 1024/1024/1024
conv cout 512 ks 3 ups 0 kt 3 variant 0  8x64 : void ifx::conv::conv_cl_kernel<128, 0, 3> * 512 139264 grids t1 8/8/8 t3 16/16/16 t14 56/56/56
conv cout 512 ks 3 ups 0 kt 3 variant 0 13x70 : void ifx::conv::conv_cl_kernel<128, 0, 3> * 512 139264 grids t1 16/16/16 t3 48/48/48 t14 224/224/224
conv cout 512 ks 3 ups 0 kt 3 variant 0 60x104: void ifx::conv::conv_cl_kernel<128, 0, 3> * 512 139264 grids t1 64/64/64 t3 192/192/192 t14 896/896/896
conv cout 512 ks 3 ups 0 kt 3 variant 1  8x64 : void ifx::conv::conv_cl_kernel<128, 0, 3> * 512 139264 grids t1 8/8/8 t3 16/16/16 t14 56/56/56
conv cout 512 ks 3 ups 0 kt 3 variant 1 13x70 : void ifx::conv::conv_cl_kernel<128, 0, 3> * 512 139264 grids t1 16/16/16 t3 48/48/48 t14 224/224/224
conv cout 512 ks 3 ups 0 kt 3 variant 1 60x104: void ifx::conv::conv_cl_kernel<128, 0, 3> * 512 139264 grids t1 64/64/64 t3 192/192/192 t14 896/896/896
conv cout 512 ks 3 ups 1 kt 1 variant 0  8x64 : void ifx::conv::conv_cl_kernel<128, 1, 3> * 512 139264 grids t1 16/16/16 t3 48/48/48 t16 256/256/256
conv cout 512 ks 3 ups 1 kt 1 variant 0 13x70 : void ifx::conv::conv_cl_kernel<128, 1, 3> * 512 139264 grids t1 48/48/48 t3 144/144/144 t16 768/768/768
conv cout 512 ks 3 ups 1 kt 1 variant 0 60x104: void ifx::conv::conv_cl_kernel<128, 1, 3> * 512 139264 grids t1 240/240/240 t3 720/720/720 t16 3840/3840/3840
conv cout 512 ks 3 ups 1 kt 1 variant 1  8x64 : void ifx::conv::conv_cl_kernel<128, 1, 3> * 512 139264 grids t1 16/16/16 t3 48/48/48 t16 256/256/256
conv cout 512 ks 3 ups 1 kt 1 variant 1 13x70 : void ifx::conv::conv_cl_kernel<128, 1, 3> * 512 139264 grids t1 48/48/48 t3 144/144/144 t16 768/768/768
conv cout 512 ks 3 ups 1 kt 1 variant 1 60x104: void ifx::conv::conv_cl_kernel<128, 1, 3> * 512 139264 grids t1 240/240/240 t3 720/720/720 t16 3840/3840/3840
conv cout 512 ks 3 ups 1 kt 3 variant 0  8x64 : void ifx::conv::conv_cl_kernel<128, 1, 3> * 512 139264 grids t1 16/16/16 t3 48/48/48 t14 224/224/224
conv cout 512 ks 3 ups 1 kt 3 variant 0 13x70 : void ifx::conv::conv_cl_kernel<128, 1, 3> * 512 139264 grids t1 48/48/48 t3 144/144/144 t14 672/672/672
conv cout 512 ks 3 ups 1 kt 3 variant 0 60x104: void ifx::conv::conv_cl_kernel<128, 1, 3> * 512 139264 grids t1 240/240/240 t3 720/720/720 t14 3360/3360/3360
conv cout 512 ks 3 ups 1 kt 3 variant 1  8x64 : void ifx::conv::conv_cl_kernel<128, 1, 3> * 512 139264 grids t1 16/16/16 t3 48/48/48 t14 224/224/224
conv cout 512 ks 3 ups 1 kt 3 variant 1 13x70 : void ifx::conv::conv_cl_kernel<128, 1, 3> * 512 139264 grids t1 48/48/48 t3 144/144/144 t14 672/672/672
conv cout 512 ks 3 ups 1 kt 3 variant 1 60x104: void ifx::conv::conv_cl_kernel<128, 1, 3> * 512 139264 grids t1 240/240/240 t3 720/720/720 t14 3360/3360/3360
conv cout 576 ks 1 ups 0 kt 1 variant 0  8x64 : void ifx::conv::conv_cl_kernel<96, 0, 1> * 512 106496 grids t1 8/8/8 t3 24/24/24 t16 96/96/96
conv cout 576 ks 1 ups 0 kt 1 variant 0 13x70 : void ifx::conv::conv_cl_kernel<96, 0, 1> * 512 106496 grids t1 24/24/24 t3 72/72/72 t16 384/384/384
conv cout 576 ks 1 ups 0 kt 1 variant 0 60x104: void ifx::conv::conv_cl_kernel<96, 0, 1> * 512 106496 grids t1 96/96/96 t3 288/288/288 t16 1536/1536/1536
conv cout 576 ks 1 ups 0 kt 1 variant 1  8x64 : void ifx::conv::conv_cl_kernel<96, 0, 1> * 512 106496 grids t1 8/8/8 t3 24/24/24 t16 96/96/96
conv cout 576 ks 1 ups 0 kt 1 variant 1 13x70 : void ifx::conv::conv_cl_kernel<96, 0, 1> * 512 106496 grids t1 24/24/24 t3 72/72/72 t16 384/384/384
conv cout 576 ks 1 ups 0 kt 1 variant 1 60x104: void ifx::conv::conv_cl_kernel<96, 0, 1> * 512 106496 grids t1 96/96/96 t3 288/288/288 t16 1536/1536/1536
conv cout 576 ks 1 ups 0 kt 3 variant 0  8x64 : void ifx::conv::conv_cl_kernel<96, 0, 1> * 512 106496 grids t1 8/8/8 t3 24/24/24 t14 88/88/88
conv cout 576 ks 1 ups 0 kt 3 variant 0 13x70 : void ifx::conv::conv_cl_kernel<96, 0, 1> * 512 106496 grids t1 24/24/24 t3 72/72/72 t14 336/336/336
conv cout 576 ks 1 ups 0 kt 3 variant 0 60x104: void ifx::conv::conv_cl_kernel<96, 0, 1> * 512 106496 grids t1 96/96/96 t3 288/288/288 t14 1344/1344/1344
conv cout 576 ks 1 ups 0 kt 3 variant 1  8x64 : void ifx::conv::conv_cl_kernel<96, 0, 1> * 512 106496 grids t1 8/8/8 t3 24/24/24 t14 88/88/88
conv cout 576 ks 1 ups 0 kt 3 variant 1 13x70 : void ifx::conv::conv_cl_kernel<96, 0, 1> * 512 106496 grids t1 24/24/24 t3 72/72/72 t14 336/336/336
conv cout 576 ks 1 ups 0 kt 3 variant 1 60x104: void ifx::conv::conv_cl_kernel<96, 0, 1> * 512 106496 grids t1 96/96/96 t3 288/288/288 t14 1344/1344/1344
conv cout 576 ks 3 ups 0 kt 1 variant 0  8x64 : void ifx::conv::conv_cl_kernel<96, 0, 3> * 512 145408 grids t1 8/8/8 t3 24/24/24 t16 96/96/96
conv cout 576 ks 3 ups 0 kt 1 variant 0 13x70 : void ifx::conv::conv_cl_kernel<96, 0, 3> * 512 145408 grids t1 24/24/24 t3 72/72/72 t16 384/384/384
conv cout 576 ks 3 ups 0 kt 1 variant 0 60x104: void ifx::conv::conv_cl_kernel<96, 0, 3> * 512 145408 grids t1 96/96/96 t3 288/288/288 t16 1536/1536/1536
conv cout 576 ks 3 ups 0 kt 1 variant 1  8x64 : void ifx::conv::conv_cl_kernel<96, 0, 3> * 512 145408 grids t1 8/8/8 t3 24/24/24 t16 96/96/96
conv cout 576 ks 3 ups 0 kt 1 variant 1 13x70 : void ifx::conv::conv_cl_kernel<96, 0, 3> * 512 145408 grids t1 24/24/24 t3 72/72/72 t16 384/384/384
conv cout 576 ks 3 ups 0 kt 1 variant 1 60x104: void ifx::conv::conv_cl_kernel<96, 0, 3> * 512 145408 grids t1 96/96/96 t3 288/288/288 t16 1536/1536/1536
conv cout 576 ks 3 ups 0 kt 3 variant 0  8x64 : void ifx::conv::conv_cl_kernel<96, 0, 3> * 512 145408 grids t1 8/8/8 t3 24/24/24 t14 88/88/88
conv cout 576 ks 3 ups 0 kt 3 variant 0 13x70 : void ifx::conv::conv_cl_kernel<96, 0, 3> * 512 145408 grids t1 24/24/24 t3 72/72/72 t14 336/336/336
conv cout 576 ks 3 ups 0 kt 3 variant 0 60x104: void ifx::conv::conv_cl_kernel<96, 0, 3> * 512 145408 grids t1 96/96/96 t3 288/288/288 t14 1344/1344/1344
conv cout 576 ks 3 ups 0 kt 3 variant 1  8x64 : void ifx::conv::conv_cl_kernel<96, 0, 3> * 512 145408 grids t1 8/8/8 t3 24/24/24 t14 88/88/88
conv cout 576 ks 3 ups 0 kt 3 variant 1 13x70 : void ifx::conv::conv_cl_kernel<96, 0, 3> * 512 145408 grids t1 24/24/24 t3 72/72/72 t14 336/336/336
conv cout 576 ks 3 ups 0 kt 3 variant 1 60x104: void ifx::conv::conv_cl_kernel<96, 0, 3> * 512 145408 grids t1 96/96/96 t3 288/288/288 t14 1344/1344/1344
conv cout 576 ks 3 ups 1 kt 1 variant 0  8x64 : void ifx::conv::conv_cl_kernel<96, 1, 3> * 512 106496 grids t1 24/24/24 t3 72/72/72 t16 384/384/384
conv cout 576 ks 3 ups 1 kt 1 variant 0 13x70 : void ifx::conv::conv_cl_kernel<96, 1, 3> * 512 106496 grids t1 72/72/72 t3 216/216/216 t16 1152/1152/1152
conv cout 576 ks 3 ups 1 kt 1 variant 0 60x104: void ifx::conv::conv_cl_kernel<96, 1, 3> * 512 106496 grids t1 360/360/360 t3 1080/1080/1080 t16 5760/5760/5760
conv cout 576 ks 3 ups 1 kt 1 variant 1  8x64 : void ifx::conv::conv_cl_kernel<96, 1, 3> * 512 106496 grids t1 24/24/24 t3 72/72/72 t16 384/384/384
conv cout 576 ks 3 ups 1 kt 1 variant 1 13x70 : void ifx::conv::conv_cl_kernel<96, 1, 3> * 512 106496 grids t1 72/72/72 t3 216/216/216 t16 1152/1152/1152
conv cout 576 ks 3 ups 1 kt 1 variant 1 60x104: void ifx::conv::conv_cl_kernel<96, 1, 3> * 512 106496 grids t1 360/360/360 t3 1080/1080/1080 t16 5760/5760/5760
conv cout 576 ks 3 ups 1 kt 3 variant 0  8x64 : void ifx::conv::conv_cl_kernel<96, 1, 3> * 512 106496 grids t1 24/24/24 t3 72/72/72 t14 336/336/336
conv cout 576 ks 3 ups 1 kt 3 variant 0 13x70 : void ifx::conv::conv_cl_kernel<96, 1, 3> * 512 106496 grids t1 72/72/72 t3 216/216/216 t14 1008/1008/1008
conv cout 576 ks 3 ups 1 kt 3 variant 0 60x104: void ifx::conv::conv_cl_kernel<96, 1, 3> * 512 106496 grids t1 360/360/360 t3 1080/1080/1080 t14 5040/5040/5040
conv cout 576 ks 3 ups 1 kt 3 variant 1  8x64 : void ifx::conv::conv_cl_kernel<96, 1, 3> * 512 106496 grids t1 24/24/24 t3 72/72/72 t14 336/336/336
conv cout 576 ks 3 ups 1 kt 3 variant 1 13x70 : void ifx::conv::conv_cl_kernel<96, 1, 3> * 512 106496 grids t1 72/72/72 t3 216/216/216 t14 1008/1008/1008
conv cout 576 ks 3 ups 1 kt 3 variant 1 60x104: void ifx::conv::conv_cl_kernel<96, 1, 3> * 512 106496 grids t1 360/360/360 t3 1080/1080/1080 t14 5040/5040/5040
conv cout 640 ks 1 ups 0 kt 1 variant 0  8x64 : void ifx::conv::conv_cl_kernel<128, 0, 1> * 512 139264 grids t1 8/8/8 t3 16/16/16 t16 80/80/80
conv cout 640 ks 1 ups 0 kt 1 variant 0 13x70 : void ifx::conv::conv_cl_kernel<128, 0, 1> * 512 139264 grids t1 24/24/24 t3 64/64/64 t16 320/320/320
conv cout 640 ks 1 ups 0 kt 1 variant 0 60x104: void ifx::conv::conv_cl_kernel<128, 0, 1> * 512 139264 grids t1 80/80/80 t3 240/240/240 t16 1280/1280/1280
conv cout 640 ks 1 ups 0 kt 1 variant 1  8x64 : void ifx::conv::conv_cl_kernel<128, 0, 1> * 512 139264 grids t1 8/8/8 t3 16/16/16 t16 80/80/80
conv cout 640 ks 1 ups 0 kt 1 variant 1 13x70 : void ifx::conv::conv_cl_kernel<128, 0, 1> * 512 139264 grids t1 24/24/24 t3 64/64/64 t16 320/320/320
conv cout 640 ks 1 ups 0 kt 1 variant 1 60x104: void ifx::conv::conv_cl_kernel<128, 0, 1> * 512 139264 grids t1 80/80/80 t3 240/240/240 t16 1280/1280/1280
conv cout 640 ks 1 ups 0 kt 3 variant 0  8x64 : void ifx::conv::conv_cl_kernel<128, 0, 1> * 512 139264 grids t1 8/8/8 t3 16/16/16 t14 72/72/72
conv cout 640 ks 1 ups 0 kt 3 variant 0 13x70 : void ifx::conv::conv_cl_kernel<128, 0, 1> * 512 139264 grids t1 24/24/24 t3 64/64/64 t14 280/280/280
conv cout 640 ks 1 ups 0 kt 3 variant 0 60x104: void ifx::conv::conv_cl_kernel<128, 0, 1> * 512 139264 grids t1 80/80/80 t3 240/240/240 t14 1120/1120/1120
conv cout 640 ks 1 ups 0 kt 3 variant 1  8x64 : void ifx::conv::conv_cl_kernel<128, 0, 1> * 512 139264 grids t1 8/8/8 t3 16/16/16 t14 72/72/72
conv cout 640 ks 1 ups 0 kt 3 variant 1 13x70 : void ifx::conv::conv_cl_kernel<128, 0, 1> * 512 139264 grids t1 24/24/24 t3 64/64/64 t14 280/280/280
conv cout 640 ks 1 ups 0 kt 3 variant 1 60x104: void ifx::conv::conv_cl_kernel<128, 0, 1> * 512 139264 grids t1 80/80/80 t3 240/240/240 t14 1120/1120/1120
conv cout 640 ks 3 ups 0 kt 1 variant 0  8x64 : void ifx::conv::conv_cl_kernel<128, 0, 3> * 512 139264 grids t1 8/8/8 t3 16/16/16 t16 80/80/80
conv cout 640 ks 3 ups 0 kt 1 variant 0 13x70 : void ifx::conv::conv_cl_kernel<128, 0, 3> * 512 139264 grids t1 24/24/24 t3 64/64/64 t16 320/320/320
conv cout 640 ks 3 ups 0 kt 1 variant 0 60x104: void ifx::conv::conv_cl_kernel<128, 0, 3> * 512 139264 grids t1 80/80/80 t3 240/240/240 t16 1280/1280/1280
conv cout 640 ks 3 ups 0 kt 1 variant 1  8x64 : void ifx::conv::conv_cl_kernel<128, 0, 3> * 512 139264 grids t1 8/8/8 t3 16/16/16 t16 80/80/80
conv cout 640 ks 3 ups 0 kt 1 variant 1 13x70 : void ifx::conv::conv_cl_kernel<128, 0, 3> * 512 139264 grids t1 24/24/24 t3 64/64/64 t16 320/320/320
conv cout 640 ks 3 ups 0 kt 1 variant 1 60x104: void ifx::conv::conv_cl_kernel<128, 0, 3> * 512 139264 grids t1 80/80/80 t3 240/240/240 t16 1280/1280/1280
conv cout 640 ks 3 ups 0 kt 3 variant 0  8x64 : void ifx::conv::conv_cl_kernel<128, 0, 3> * 512 139264 grids t1 8/8/8 t3 16/16/16 t14 72/72/72
conv cout 640 ks 3 ups 0 kt 3 variant 0 13x70 : void ifx::conv::conv_cl_kernel<128, 0, 3> * 512 139264 grids t1 24/24/24 t3 64/64/64 t14 280/280/280
conv cout 640 ks 3 ups 0 kt 3 variant 0 60x104: void ifx::conv::conv_cl_kernel<128, 0, 3> * 512 139264 grids t1 80/80/80 t3 240/240/240 t14 1120/1120/1120
conv cout 640 ks 3 ups 0 kt 3 variant 1  8x64 : void ifx::conv::conv_cl_kernel<128, 0, 3> * 512 139264 grids t1 8/8/8 t3 16/16/16 t14 72/72/72
conv cout 640 ks 3 ups 0 kt 3 variant 1 13x70 : void ifx::conv::conv_cl_kernel<128, 0, 3> * 512 139264 grids t1 24/24/24 t3 64/64/64 t14 280/280/280
conv cout 640 ks 3 ups 0 kt 3 variant 1 60x104: void ifx::conv::conv_cl_kernel<128, 0, 3> * 512 139264 grids t1 80/80/80 t3 240/240/240 t14 1120/1120/1120
conv cout 640 ks 3 ups 1 kt 1 variant 0  8x64 : void ifx::conv::conv_cl_kernel<128, 1, 3> * 512 139264 grids t1 24/24/24 t3 64/64/64 t16 320/320/320
conv cout 640 ks 3 ups 1 kt 1 variant 0 13x70 : void ifx::conv::conv_cl_kernel<128, 1, 3> * 512 139264 grids t1 64/64/64 t3 184/184/184 t16 960/960/960
conv cout 640 ks 3 ups 1 kt 1 variant 0 60x104: void ifx::conv::conv_cl_kernel<128, 1, 3> * 512 139264 grids t1 304/304/304 t3 904/904/904 t16 4800/4800/4800
conv cout 640 ks 3 ups 1 kt 1 variant 1  8x64 : void ifx::conv::conv_cl_kernel<128, 1, 3> * 512 139264 grids t1 24/24/24 t3 64/64/64 t16 320/320/320
conv cout 640 ks 3 ups 1 kt 1 variant 1 13x70 : void ifx::conv::conv_cl_kernel<128, 1, 3> * 512 139264 grids t1 64/64/64 t3 184/184/184 t16 960/960/960
conv cout 640 ks 3 ups 1 kt 1 variant 1 60x104: void ifx::conv::conv_cl_kernel<128, 1, 3> * 512 139264 grids t1 304/304/304 t3 904/904/904 t16 4800/4800/4800
conv cout 640 ks 3 ups 1 kt 3 variant 0  8x64 : void ifx::conv::conv_cl_kernel<128, 1, 3> * 512 139264 grids t1 24/24/24 t3 64/64/64 t14 280/280/280
conv cout 640 ks 3 ups 1 kt 3 variant 0 13x70 : void ifx::conv::conv_cl_kernel<128, 1, 3> * 512 139264 grids t1 64/64/64 t3 184/184/184 t14 840/840/840
conv cout 640 ks 3 ups 1 kt 3 variant 0 60x104: void ifx::conv::conv_cl_kernel<128, 1, 3> * 512 139264 grids t1 304/304/304 t3 904/904/904 t14 4200/4200/4200
conv cout 640 ks 3 ups 1 kt 3 variant 1  8x64 : void ifx::conv::conv_cl_kernel<128, 1, 3> * 512 139264 grids t1 24/24/24 t3 64/64/64 t14 280/280/280
conv cout 640 ks 3 ups 1 kt 3 variant 1 13x70 : void ifx::conv::conv_cl_kernel<128, 1, 3> * 512 139264 grids t1 64/64/64 t3 184/184/184 t14 840/840/840
conv cout 640 ks 3 ups 1 kt 3 variant 1 60x104: void ifx::conv::conv_cl_kernel<128, 1, 3> * 512 139264 grids t1 304/304/304 t3 904/904/904 t14 4200/4200/4200
conv input 2048x2047 cin 256 cout 96 (under 2 GiB): void ifx::conv::pp::conv_pp_kernel<96, 0> 256 512 152576
conv input 2048x2048 cin 256 cout 96 (2 GiB): void ifx::conv::conv_cl_kernel<96, 0, 3> 8192 512 145408
conv output 2048x1365 cin 32 cout 384 (under 2 GiB): void ifx::conv::pp::conv_pp_kernel<96, 0> 256 512 152576
conv output 2048x1366 cin 32 cout 384 (over 2 GiB): void ifx::conv::conv_cl_kernel<96, 0, 3> 22528 512 145408
conv output 1024x682 upsampled cin 32 cout 384 (under 2 GiB): void ifx::conv::pp::conv_pp_kernel<96, 1> 256 512 93184
conv output 1024x683 upsampled cin 32 cout 384 (over 2 GiB): void ifx::conv::conv_cl_kernel<96, 1, 3> 22528 512 106496
conv weights kt 3 cin 82848 cout 480 (under 2 GiB): void ifx::conv::pp::conv_pp_kernel<96, 0> 8 512 152576
conv weights kt 3 cin 82880 cout 480 (over 2 GiB): void ifx::conv::conv_cl_kernel<96, 0, 3> 8 512 145408
conv weights kt 1 cin 82880 cout 480: void ifx::conv::pp::conv_pp_kernel<96, 0> 8 512 152576
conv null descriptor: rc -1 ifx_conv3d_cl: null argument
conv null x: rc -1 ifx_conv3d_cl: null argument
conv null w: rc -1 ifx_conv3d_cl: null argument
conv null y: rc -1 ifx_conv3d_cl: null argument
conv null zero page: rc -1 ifx_conv3d_cl: null argument
conv no bias: void ifx::conv::pp::conv_pp_kernel<96, 0> 8 512 152576
conv kt 2: rc -1 ifx_conv3d_cl: temporal kernel 2 not built (1 or 3)
conv ks 2: rc -1 ifx_conv3d_cl: spatial kernel 2 not built (1 or 3)
conv upsample with ks 1: rc -1 ifx_conv3d_cl: upsample needs the 3x3 kernel
conv upsample 2: rc -1 ifx_conv3d_cl: upsample needs the 3x3 kernel
conv cin 0: rc -1 ifx_conv3d_cl: cin 0 must be a multiple of 32
conv cin 48: rc -1 ifx_conv3d_cl: cin 48 must be a multiple of 32
conv in_planar 2: rc -1 ifx_conv3d_cl: in_planar 2 (0 or 1)
conv cout 0: rc -1 ifx_conv3d_cl: cout 0 must be a multiple of 4 (or < 4)
conv cout 6: rc -1 ifx_conv3d_cl: cout 6 must be a multiple of 4 (or < 4)
conv cout 2: void ifx::conv::conv_cl_kernel<32, 0, 3> 8 512 108544
conv t_out 0: rc -1 ifx_conv3d_cl: 0 output frames per call (max 16 inputs)
conv t_out 15 with kt 3: rc -1 ifx_conv3d_cl: 15 output frames per call (max 16 inputs)
conv t_out 16 with kt 1: void ifx::conv::pp::conv_pp_kernel<96, 0> 16 512 152576
conv t_out 17 with kt 1: rc -1 ifx_conv3d_cl: 17 output frames per call (max 16 inputs)
conv hs 0: rc -1 ifx_conv3d_cl: empty frame
conv ws 0: rc -1 ifx_conv3d_cl: empty frame
conv input frame 4096x2048 cin 256: rc -1 ifx_conv3d_cl: frame too large for 32-bit pixel offsets
conv output frame 4096x2048 cout 256: rc -1 ifx_conv3d_cl: frame too large for 32-bit pixel offsets
conv upsampled output frame 2048x1024 cout 256: rc -1 ifx_conv3d_cl: frame too large for 32-bit pixel offsets
conv upsampled output frame 2048x1023 cout 256: void ifx::conv::conv_cl_kernel<128, 1, 3> 32768 512 139264
conv in_frame_stride + 4: rc -1 ifx_conv3d_cl: in_frame_stride 16388 must be a multiple of 8 elements (16 bytes)
conv frame strides + 64: void ifx::conv::pp::conv_pp_kernel<96, 0> 8 512 152576
conv x + 8 bytes: rc -1 ifx_conv3d_cl: x and w must be 16-byte aligned
conv w + 2 bytes: rc -1 ifx_conv3d_cl: x and w must be 16-byte aligned
conv out_frame_stride + 4: rc -1 ifx_conv3d_cl: out_frame_stride 49156 must be a multiple of 8 elements (16 bytes) when cout % 8 == 0
conv y + 8 bytes: rc -1 ifx_conv3d_cl: y and residual must be 16-byte aligned when cout % 8 == 0
conv residual: void ifx::conv::pp::conv_pp_kernel<96, 0> 8 512 152576
conv residual + 8 bytes: rc -1 ifx_conv3d_cl: y and residual must be 16-byte aligned when cout % 8 == 0
conv cout 20: out_frame_stride + 4, y and residual + 2 bytes: void ifx::conv::conv_cl_kernel<32, 0, 3> 8 512 108544
conv cout 20: in_frame_stride + 4: rc -1 ifx_conv3d_cl: in_frame_stride 16388 must be a multiple of 8 elements (16 bytes)
norm channels   8: void ifx::conv::rmsnorm_cl_kernel<1, 1> * 256 0 grids 1/4/19
norm channels  16: void ifx::conv::rmsnorm_cl_kernel<2, 1> * 256 0 grids 1/8/37
norm channels  24: void ifx::conv::rmsnorm_cl_kernel<1, 3> * 256 0 grids 1/8/37
norm channels  32: void ifx::conv::rmsnorm_cl_kernel<4, 1> * 256 0 grids 1/16/74
norm channels  40: void ifx::conv::rmsnorm_cl_kernel<8, 1> * 256 0 grids 1/32/147
norm channels  48: void ifx::conv::rmsnorm_cl_kernel<2, 3> * 256 0 grids 1/16/74
norm channels  56: void ifx::conv::rmsnorm_cl_kernel<8, 1> * 256 0 grids 1/32/147
norm channels  64: void ifx::conv::rmsnorm_cl_kernel<8, 1> * 256 0 grids 1/32/147
norm channels  72: void ifx::conv::rmsnorm_cl_kernel<16, 1> * 256 0 grids 1/64/293
norm channels  80: void ifx::conv::rmsnorm_cl_kernel<16, 1> * 256 0 grids 1/64/293
norm channels  88: void ifx::conv::rmsnorm_cl_kernel<16, 1> * 256 0 grids 1/64/293
norm channels  96: void ifx::conv::rmsnorm_cl_kernel<4, 3> * 256 0 grids 1/32/147
norm channels 104: void ifx::conv::rmsnorm_cl_kernel<16, 1> * 256 0 grids 1/64/293
norm channels 112: void ifx::conv::rmsnorm_cl_kernel<16, 1> * 256 0 grids 1/64/293
norm channels 120: void ifx::conv::rmsnorm_cl_kernel<16, 1> * 256 0 grids 1/64/293
norm channels 128: void ifx::conv::rmsnorm_cl_kernel<16, 1> * 256 0 grids 1/64/293
norm channels 136: void ifx::conv::rmsnorm_cl_kernel<32, 1> * 256 0 grids 1/128/585
norm channels 144: void ifx::conv::rmsnorm_cl_kernel<32, 1> * 256 0 grids 1/128/585
norm channels 152: void ifx::conv::rmsnorm_cl_kernel<32, 1> * 256 0 grids 1/128/585
norm channels 160: void ifx::conv::rmsnorm_cl_kernel<32, 1> * 256 0 grids 1/128/585
norm channels 168: void ifx::conv::rmsnorm_cl_kernel<32, 1> * 256 0 grids 1/128/585
norm channels 176: void ifx::conv::rmsnorm_cl_kernel<32, 1> * 256 0 grids 1/128/585
norm channels 184: void ifx::conv::rmsnorm_cl_kernel<32, 1> * 256 0 grids 1/128/585
norm channels 192: void ifx::conv::rmsnorm_cl_kernel<8, 3> * 256 0 grids 1/64/293
norm channels 200: void ifx::conv::rmsnorm_cl_kernel<32, 1> * 256 0 grids 1/128/585
norm channels 208: void ifx::conv::rmsnorm_cl_kernel<32, 1> * 256 0 grids 1/128/585
norm channels 216: void ifx::conv::rmsnorm_cl_kernel<32, 1> * 256 0 grids 1/128/585
norm channels 224: void ifx::conv::rmsnorm_cl_kernel<32, 1> * 256 0 grids 1/128/585
norm channels 232: void ifx::conv::rmsnorm_cl_kernel<32, 1> * 256 0 grids 1/128/585
norm channels 240: void ifx::conv::rmsnorm_cl_kernel<32, 1> * 256 0 grids 1/128/585
norm channels 248: void ifx::conv::rmsnorm_cl_kernel<32, 1> * 256 0 grids 1/128/585
norm channels 256: void ifx::conv::rmsnorm_cl_kernel<32, 1> * 256 0 grids 1/128/585
norm channels 264: void ifx::conv::rmsnorm_cl_kernel<64, 1> * 256 0 grids 1/256/1170
norm channels 272: void ifx::conv::rmsnorm_cl_kernel<64, 1> * 256 0 grids 1/256/1170
norm channels 280: void ifx::conv::rmsnorm_cl_kernel<64, 1> * 256 0 grids 1/256/1170
norm channels 288: void ifx::conv::rmsnorm_cl_kernel<64, 1> * 256 0 grids 1/256/1170
norm channels 296: void ifx::conv::rmsnorm_cl_kernel<64, 1> * 256 0 grids 1/256/1170
norm channels 304: void ifx::conv::rmsnorm_cl_kernel<64, 1> * 256 0 grids 1/256/1170
norm channels 312: void ifx::conv::rmsnorm_cl_kernel<64, 1> * 256 0 grids 1/256/1170
norm channels 320: void ifx::conv::rmsnorm_cl_kernel<64, 1> * 256 0 grids 1/256/1170
norm channels 328: void ifx::conv::rmsnorm_cl_kernel<64, 1> * 256 0 grids 1/256/1170
norm channels 336: void ifx::conv::rmsnorm_cl_kernel<64, 1> * 256 0 grids 1/256/1170
norm channels 344: void ifx::conv::rmsnorm_cl_kernel<64, 1> * 256 0 grids 1/256/1170
norm channels 352: void ifx::conv::rmsnorm_cl_kernel<64, 1> * 256 0 grids 1/256/1170
norm channels 360: void ifx::conv::rmsnorm_cl_kernel<64, 1> * 256 0 grids 1/256/1170
norm channels 368: void ifx::conv::rmsnorm_cl_kernel<64, 1> * 256 0 grids 1/256/1170
norm channels 376: void ifx::conv::rmsnorm_cl_kernel<64, 1> * 256 0 grids 1/256/1170
norm channels 384: void ifx::conv::rmsnorm_cl_kernel<16, 3> * 256 0 grids 1/128/585
norm channels 392: void ifx::conv::rmsnorm_cl_kernel<64, 1> * 256 0 grids 1/256/1170
norm channels 400: void ifx::conv::rmsnorm_cl_kernel<64, 1> * 256 0 grids 1/256/1170
norm channels 408: void ifx::conv::rmsnorm_cl_kernel<64, 1> * 256 0 grids 1/256/1170
norm channels 416: void ifx::conv::rmsnorm_cl_kernel<64, 1> * 256 0 grids 1/256/1170
norm channels 424: void ifx::conv::rmsnorm_cl_kernel<64, 1> * 256 0 grids 1/256/1170
norm channels 432: void ifx::conv::rmsnorm_cl_kernel<64, 1> * 256 0 grids 1/256/1170
norm channels 440: void ifx::conv::rmsnorm_cl_kernel<64, 1> * 256 0 grids 1/256/1170
norm channels 448: void ifx::conv::rmsnorm_cl_kernel<64, 1> * 256 0 grids 1/256/1170
norm channels 456: void ifx::conv::rmsnorm_cl_kernel<64, 1> * 256 0 grids 1/256/1170
norm channels 464: void ifx::conv::rmsnorm_cl_kernel<64, 1> * 256 0 grids 1/256/1170
norm channels 472: void ifx::conv::rmsnorm_cl_kernel<64, 1> * 256 0 grids 1/256/1170
norm channels 480: void ifx::conv::rmsnorm_cl_kernel<64, 1> * 256 0 grids 1/256/1170
norm channels 488: void ifx::conv::rmsnorm_cl_kernel<64, 1> * 256 0 grids 1/256/1170
norm channels 496: void ifx::conv::rmsnorm_cl_kernel<64, 1> * 256 0 grids 1/256/1170
norm channels 504: void ifx::conv::rmsnorm_cl_kernel<64, 1> * 256 0 grids 1/256/1170
norm channels 512: void ifx::conv::rmsnorm_cl_kernel<64, 1> * 256 0 grids 1/256/1170
norm null x: rc -1 ifx_rmsnorm_cl: null argument
norm null gamma: rc -1 ifx_rmsnorm_cl: null argument
norm null y: rc -1 ifx_rmsnorm_cl: null argument
norm null slots: rc -1 ifx_rmsnorm_cl: null argument
norm frames 0: rc -1 ifx_rmsnorm_cl: 0 frames per call (max 16)
norm frames 16: void ifx::conv::rmsnorm_cl_kernel<4, 3> 8 256 0
norm frames 17: rc -1 ifx_rmsnorm_cl: 17 frames per call (max 16)
norm frame_pixels 0: rc -1 ifx_rmsnorm_cl: 1 frames per call (max 16)
norm 16 x 134213632 pixels: rc -1 ifx_rmsnorm_cl: too many pixels per call
norm 16 x 134213631 pixels: void ifx::conv::rmsnorm_cl_kernel<4, 3> 16776704 256 0
norm channels 0: rc -1 ifx_rmsnorm_cl: channels 0 not in [8, 512] step 8
norm channels 12: rc -1 ifx_rmsnorm_cl: channels 12 not in [8, 512] step 8
norm channels 520: rc -1 ifx_rmsnorm_cl: channels 520 not in [8, 512] step 8
norm flags 4: rc -1 ifx_rmsnorm_cl: flags 4 (IFX_NORM_SILU | IFX_NORM_OUT_PLANAR; planar output needs channels % 32 == 0)
norm planar with channels 72: rc -1 ifx_rmsnorm_cl: flags 2 (IFX_NORM_SILU | IFX_NORM_OUT_PLANAR; planar output needs channels % 32 == 0)
softmax 6240 x 6240: ifx::conv::softmax_rows_kernel 1560 256 0
softmax 5 x 70 ld 72: ifx::conv::softmax_rows_kernel 2 256 0
softmax ld 70: rc -1 ifx_softmax_rows: bad arguments
"""


def test_conv_plan_reproduces_the_recorded_launches():
    """Which kernel an ifx_conv3d_cl call runs (lock-step or persistent, channel tile, upsample, spatial kernel), on which grid for
    256, 304 and 64 CUs and with how much LDS, for cout 3 - 640 x kernel shapes x kt x conv_variant x in_planar x one-tile and ragged
    frames x 1, 3 and the most output frames; the three "operand of 2 GiB or more" clauses from both sides; every refusal of the entry
    point, the alignment contract of ifx_conv3d_desc among them (16-byte x and w, frame strides in multiples of 8 elements, y and
    residual only where cout % 8 == 0); the instantiation and block count of ifx_rmsnorm_cl for every channel count 8 - 512 and its refusals; ifx_softmax_rows:
    tools/conv_plan_check.cpp calls the real entry points with the runtime stubbed (no GPU), and its output has to be the recorded one
    line for line."""
    import shutil
    import subprocess
    import tempfile
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not present")
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "conv_plan_check")
        b = subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-std=c++17", "-rdynamic", os.path.join(root, "tools", "conv_plan_check.cpp"),
                            "-ldl", "-o", exe], capture_output=True, text=True, timeout=600)
        assert b.returncode == 0, b.stderr[-3000:]
        p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-1000:] + p.stderr[-1000:]
    got, want = p.stdout.splitlines(), CONV_PLAN_RECORDED.splitlines()
    assert len(want) == 15 * 3 * 2 * 2 * 3 + 9 + 26 + 10 + 64 + 15 + 3      # (+ 10: the alignment contract, added with its refusals)
    diff = [f"recorded: {w}\n     now: {g}" for w, g in zip(want, got) if w != g]
    assert not diff and len(got) == len(want), f"{len(diff)} of {len(want)} lines differ ({len(got)} printed):\n" + "\n".join(diff[:20])


def test_launch_mechanics_hold_on_fake_devices():
    """The dynamic-LDS opt-in is made per kernel and per device before that pair's first launch, from eight host threads at once; a
    refusal is returned (IFX_ELAUNCH, the entry point named) and asked again; a persistent grid is sized by the calling thread's
    device: tools/launch_check.cpp drives the real ifx_conv3d_cl and ifx_t5_attention over a fake runtime (no GPU) and exits 0 only
    when every rule holds (it prints the broken ones)."""
    import shutil
    import subprocess
    import tempfile
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not present")
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "launch_check")
        b = subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-std=c++17", os.path.join(root, "tools", "launch_check.cpp"), "-o", exe],
                           capture_output=True, text=True, timeout=600)
        assert b.returncode == 0, b.stderr[-3000:]
        p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "all rules hold" in p.stdout, p.stdout[-3000:] + p.stderr[-1000:]


def test_parallel_config_maps_ulysses_and_ring_degrees_onto_world_size():
    """reference ParallelConfig (wan_base/utils/parallel_config.py:3-30) takes any degrees; its launcher passes ulysses x ring ==
    world_size (example/self_forcing/self_forcing.sh:12-13 defaults RING_SIZE=2; run_self_forcing.py:58-67).  Here both degrees select
    the one sequence-parallel exchange at degree world_size; only a product that is not the world size is refused."""
    import pytest
    from inferix_amd.wan.causal_model import ParallelConfig
    pc = ParallelConfig()
    assert (pc.ulysses_size, pc.ring_size, pc.attn_backend) == (1, 1, "HipPagedFA")
    assert ParallelConfig(rank=3, world_size=8, local_rank=3).world_size == 8
    for u, r, w in ((1, 2, 2), (2, 1, 2), (2, 4, 8), (1, 8, 8), (4, 1, 4)):
        pc = ParallelConfig(local_rank=1, rank=1, world_size=w, ulysses_size=u, ring_size=r)     # the launcher's keyword order
        assert (pc.ulysses_size, pc.ring_size, pc.world_size, pc.rank) == (u, r, w, 1)
    for kw in (dict(ulysses_size=2), dict(ring_size=4), dict(ulysses_size=2, ring_size=4, world_size=4), dict(ring_size=2, world_size=8),
               dict(ring_size=0)):
        with pytest.raises(ValueError, match="world_size|>= 1"):
            ParallelConfig(**kw)
    with pytest.raises(ValueError, match="not available"):
        ParallelConfig(attn_backend="FA3")


def test_pmc_traffic_stamp_matches_the_kernel_sources():
    """bench.py's `roofline.traffic` / `roofline_gemm.traffic` come from profiles/pmc_traffic.json, which is stamped with the sha256 of
    the kernel sources the PMC passes ran on; a source edited after the last `tools/profile_bench.sh` makes the driver's line say
    `traffic: null` (round-3 verdict: that is how the contract field was lost).  This fails until the passes are re-run —
    the LAST act of a round that touches csrc/."""
    import hashlib
    import json
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "profiles", "pmc_traffic.json")) as f:
        doc = json.load(f)
    assert {"attn_self", "gemm_block"} <= set(doc), sorted(doc)
    for name, sec in doc.items():
        srcs = sec.get("kernel_sources") or [sec["kernel_source"]]
        h = hashlib.sha256()
        for p in srcs:
            h.update(open(os.path.join(root, p), "rb").read())
        assert sec["kernel_source_sha256"] == h.hexdigest(), \
            f"profiles/pmc_traffic.json['{name}'] is stale against {srcs}: re-run tools/profile_bench.sh on the GPU and commit its pmc_traffic.json"
        assert sec["fetch_size_kib"] > 0 and sec["write_size_kib"] > 0 and 0 < sec["mfma_busy"] < 1
    sys_path_bench = os.path.join(root, "bench.py")
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_for_stamp_test", sys_path_bench)
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    t = bench.pmc_traffic(1)
    assert t["traffic"] and t["traffic"] > t["algorithmic_bytes_per_launch"], t
    assert bench._pmc_section("gemm_block")[0] is not None


def test_bench_rejects_arguments_it_cannot_honour():
    """bench.py checks its arguments before it looks for a GPU: at least one timed step, `--kernel-breakdown` only as one of the
    `--full` measurements, and no `--dump-outputs` under `--magi-leg` (which does not run the headline clip)."""
    import subprocess
    import sys
    for args in (["--steps", "0"], ["--kernel-breakdown"], ["--magi-leg", "fp8", "--dump-outputs", "out"]):
        p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True, timeout=300, cwd=ROOT)
        assert p.returncode == 2 and "error:" in p.stderr, (args, p.returncode, p.stderr[-500:])


def test_bench_roofline_gemm_arithmetic_on_synthetic_records():
    """`bench.roofline_gemm` (the `roofline_gemm` object of the bench line) on fabricated timer records: launches are bucketed by
    (FLOPs, bytes) — O + gate and cross-o + residual share a bucket, cross-q and the two FFN launches have their own —, the per-layer
    time is the sum of the six bucket means, achieved = 2 N (6 d^2 + 2 d ffn) / that, and the PMC fields come from the stamped file."""
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("bench_for_gemm_test", os.path.join(root, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)

    class Ev:
        def __init__(self, t):
            self.t = t

        def elapsed_time(self, other):
            return other.t - self.t
    rows, us = 4680, {"qkv": 70.0, "o+gate+res": 40.0, "cross_q": 36.0, "cross_o+res": 38.0, "ffn_up+gelu": 140.0, "ffn_down+gate+res": 120.0}
    recs = []
    for rep in range(3):
        for nm, n_out, n_in, res in bench.BLOCK_GEMMS:
            fl = 2.0 * rows * n_out * n_in
            nb = 2.0 * (rows * n_in + n_out * n_in + rows * n_out * (1 + res))
            recs.append(("gemm", Ev(0.0), Ev(us[nm] * 1e-3), fl, nb))
    recs.append(("gemm", Ev(0.0), Ev(1.0), 2.0 * 3 * 1536 * 256, 123.0))          # a timestep-MLP launch: ignored
    recs.append(("attn_self", Ev(0.0), Ev(1.0), 1.0, 1.0))
    g = bench.roofline_gemm(recs, rows, forwards=35, layers=30, shards=1)
    assert g is not None and g["bound"] == "mfma" and g["peak"] == 2500.0
    assert abs(g["us_per_layer"] - sum(us.values())) < 0.11          # the shared bucket carries the mean of 40 and 38 twice
    assert abs(g["per_launch"]["o+gate+res"]["us"] - 39.0) < 1e-6 and abs(g["per_launch"]["cross_q"]["us"] - 36.0) < 1e-6
    flops = 2.0 * rows * (6 * 1536 ** 2 + 2 * 1536 * 8960)
    assert g["algorithmic_flops_per_layer"] == flops
    assert abs(g["achieved"] - flops / sum(us.values()) / 1e6) < 0.06 and abs(g["frac"] - g["achieved"] / 2500.0) < 1e-4
    assert abs(g["ms_per_clip"] - sum(us.values()) * 35 * 30 / 1e3) < 0.06
    assert g["traffic"] > g["algorithmic_bytes_per_layer"] and 0 < g["mfma_busy"] < 1 and g["traffic_over_algorithmic"] > 1
    assert bench.roofline_gemm(recs[:3], rows, 35, 30, 1) is None      # a launch of the block missing (e.g. the K/V-first split): no object
    sh = bench.roofline_gemm(recs, rows, 35, 30, 8)
    assert sh["traffic"] is None and sh["mfma_busy"] is None            # counters were taken on the unsharded launches


def test_get_option_reads_the_library_and_option_scope_restores_what_it_found():
    """`option_scope` took its 'previous' value from a Python mirror; an option set through the library directly (as several
    tests do) was invisible to it.  `ifx_get_option` reads the library's own value; the scope restores THAT."""
    import ctypes as C
    import pytest
    from inferix_amd import _hip
    from inferix_amd import hip_ops as ops
    lib = _hip.load()
    assert lib.ifx_set_option(b"gemm_small_split", 1) == 0            # behind the mirror's back
    try:
        assert ops.get_option("gemm_small_split") == 1
        with ops.option_scope("gemm_small_split", 0):
            assert ops.get_option("gemm_small_split") == 0
        assert ops.get_option("gemm_small_split") == 1, "the scope must restore the value it found in the library"
        # ... and it is the CALLER's property: a launch another host thread enqueues meanwhile (VAE, text encoder) keeps its own value
        import threading
        seen = []
        th = threading.Thread(target=lambda: seen.append(ops.get_option("gemm_small_split")))
        th.start()
        th.join()
        assert seen == [0], "gemm_small_split must be per host thread"
    finally:
        assert lib.ifx_set_option(b"gemm_small_split", 0) == 0
    assert ops.get_option("gemm_small_split") == 0
    for key, lo in (("gemm_variant", 0), ("attn_variant", 0), ("spin_fault", 0)):
        assert ops.get_option(key) == lo
    assert ops.get_option("spin_timeout_ms") >= 1
    v = C.c_int32(7)
    assert lib.ifx_get_option(b"no_such_option", C.byref(v)) != 0 and b"unknown key" in lib.ifx_last_error()
    assert lib.ifx_set_option(b"spin_timeout_ms", 0) != 0             # out of range
    assert lib.ifx_device_error(1) == 0                               # no kernel has run: the word is clear (and needs no GPU)
    with pytest.raises(_hip.HipKernelError):
        ops.get_option("no_such_option")
    # the tile-12 shortcut of a sequence-parallel rank and the workspace query agree: 2340 x 1536 x 8960 takes the in-workgroup
    # split tile under gemm_small_split and asks for no scratch
    assert lib.ifx_gemm_workspace_bytes(2340, 1536, 8960) > 0
    with ops.option_scope("gemm_small_split", 1):
        assert lib.ifx_gemm_workspace_bytes(2340, 1536, 8960) == 0
        assert lib.ifx_gemm_workspace_bytes(2340, 1536, 1536) == 0
    assert lib.ifx_gemm_workspace_bytes(2340, 1536, 8960) > 0


def test_free_layer_notifies_listeners_with_the_layer():
    """`KVCacheManager.free_layer` told its listeners the request id only, and the peer-store exchange then dropped the
    address book of EVERY layer of the request.  Two-argument listeners now get (request, layer); one-argument ones keep working."""
    import torch
    from inferix_amd.kvcache_manager import KVCacheManager, KVCacheRequest
    from inferix_amd.kvcache_manager.kvcache_manager import KVCacheRequestSpec, KVCacheSpec
    mgr, req = KVCacheManager("cpu"), KVCacheRequest("r")
    spec = KVCacheRequestSpec(num_tokens=8, block_size=1,
                              specs={n: KVCacheSpec(num_kv_heads=1, head_size=4, dtype=torch.float32, kv_offload=False, use_mla=False)
                                     for n in ("layer_0", "layer_1")})
    mgr.allocate_slots(req, spec)
    one, two = [], []
    mgr.add_free_listener(one.append)
    mgr.add_free_listener(lambda r, layer=None: two.append((r, layer)))
    mgr.free_layer(req, "layer_1")
    mgr.free(req)
    assert one == ["r", "r"] and two == [("r", "layer_1"), ("r", None)]

    class Book:                          # the bookkeeping half of PeerStoreExchange.forget, without a device
        def __init__(self):
            self._views = {("r", "layer_0", (1, 1)): 0, ("r", "layer_1", (1, 1)): 1, ("q", "layer_0", (1, 1)): 2}
            self._view_handles, self._handle_refs, self._opened, self.emulated = {}, {}, {}, True

        def _drop(self, key):
            PeerStoreExchange._drop(self, key)
    from inferix_amd.sequence_parallel import PeerStoreExchange
    bk = Book()
    PeerStoreExchange.forget(bk, "r", "layer_1")
    assert sorted(bk._views) == [("q", "layer_0", (1, 1)), ("r", "layer_0", (1, 1))]
    PeerStoreExchange.forget(bk, "r")
    assert sorted(bk._views) == [("q", "layer_0", (1, 1))]


def test_option_scope_restores_and_nests():
    """`hip_ops.option_scope` (how a sequence-parallel model's forward turns `gemm_small_split` on for its own launches only, ADVICE
    r3): sets on entry, restores the previous value on exit — also when nested and when the body raises — and leaves an equal value alone."""
    import pytest
    from inferix_amd import hip_ops as ops
    ops.set_option("gemm_small_split", 0)
    assert ops._OPTIONS["gemm_small_split"] == 0
    with ops.option_scope("gemm_small_split", 1):
        assert ops._OPTIONS["gemm_small_split"] == 1
        with ops.option_scope("gemm_small_split", 1):          # already on: nothing to do, nothing to undo
            assert ops._OPTIONS["gemm_small_split"] == 1
        assert ops._OPTIONS["gemm_small_split"] == 1
        with ops.option_scope("gemm_small_split", 0):
            assert ops._OPTIONS["gemm_small_split"] == 0
        assert ops._OPTIONS["gemm_small_split"] == 1
    assert ops._OPTIONS["gemm_small_split"] == 0
    with pytest.raises(RuntimeError):
        with ops.option_scope("gemm_small_split", 1):
            raise RuntimeError("body failed")
    assert ops._OPTIONS["gemm_small_split"] == 0
    # the workspace a GEMM shape asks for is cached per (shape, small_split): 585 x 1536 x 8960 splits across workgroups only without it
    from inferix_amd import _hip
    lib = _hip.load()
    assert lib.ifx_gemm_workspace_bytes(585, 1536, 8960) > 0
    with ops.option_scope("gemm_small_split", 1):
        assert lib.ifx_gemm_workspace_bytes(585, 1536, 8960) == 0
    assert lib.ifx_gemm_workspace_bytes(585, 1536, 8960) > 0


def test_quantize_dynamic_resolves_names_like_the_quantised_model_oracle():
    """Which linears `inferix_amd.quant.quantize_dynamic` quantises is decided by `_config_for`; which ones the quantised-model oracle
    quantises by `oracle/quant_oracle.py::config_for`.  Both must resolve every nn.Linear name of the reference's transformer the same
    way for any qconfig dict (longest matching module-name prefix, "" = default) — the example's dict and a few adversarial ones."""
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "oracle"))
    import quant_oracle as Q
    from inferix_amd.quant import _BLOCK_LINEARS, _GLOBAL_LINEARS, _config_for
    names = [n for n, _ in _GLOBAL_LINEARS]
    for i in (0, 3, 29, 30):
        for ref_name, key in _BLOCK_LINEARS:
            names += [f"blocks.{i}.self_attn.{c}" for c in "qkv"] if key == "qkv" else [f"blocks.{i}.{ref_name}"]
    dicts = [{"": 1, "text_embedding": None, "proj_out": None, "head": None}, {"": None, "blocks.3": 1}, {"": 1, "blocks.3.ffn": None, "blocks.3": 2},
             {"": 1, "blocks.3.self_attn.q": None}, {"ffn": 1}, {"": 1, "head.head": None, "time_embedding.0": None}]
    for d in dicts[:4] + dicts[5:]:
        for n in names:
            assert _config_for(n, d) == Q.config_for(n, d), (n, d)
    ex = dicts[0]
    assert [n for n in names if Q.config_for(n, ex) is None] == ["text_embedding.0", "text_embedding.2", "head.head"]
    assert Q.config_for("blocks.30.ffn.0", {"": 1, "blocks.3": None}) == 1          # a prefix match stops at a module boundary


def test_tensor_memo_keys_on_host_known_values_only():
    """`schedulers.TensorMemo` (the sigma lookups of `add_noise` / the flow -> x0 conversion, and the same rule in the model's
    modulation-table memo), round 6: a value derived from a timestep tensor is reused only for tensors the pipelines made with
    `const_timestep` — keyed on the scalar the host knows, never on a storage address or a version counter (VERDICT r5 / ADVICE r5:
    `_version` is blind to raw-pointer writes and absent on inference tensors).  Untagged tensors, tensors written in place since
    tagging, another `extra` -> recomputed; equal constants share an entry; inference mode works; the capacity bounds the entries."""
    import torch
    from inferix_amd.schedulers import FlowMatchScheduler, TensorMemo, carry_tag, const_tag, const_timestep
    calls = []

    def make(v):
        def f():
            calls.append(v)
            return v
        return f
    memo = TensorMemo(capacity=2)
    t = const_timestep(757.0, (2, 3), "cpu", torch.float32)
    assert torch.equal(t, torch.ones(2, 3) * 757.0) and const_tag(t) == 757.0
    assert memo.get(t, "a", make(1)) == 1 and memo.get(t, "a", make(2)) == 1 and calls == [1]
    assert memo.get(t.flatten(0, 1), "a", make(3)) == 3, "a view is a new tensor object: untagged, computed directly"
    assert memo.get(carry_tag(t, t.flatten(0, 1)), "a", make(4)) == 4, "carried tag, another shape: another key"
    assert memo.get(carry_tag(t, t.flatten(0, 1)), "a", make(40)) == 4
    u = const_timestep(757.0, (2, 3), "cpu", torch.float32)
    assert memo.get(u, "a", make(5)) == 1, "another tensor holding the same constant is the same values: a hit"
    plain = torch.ones(2, 3) * 757.0
    assert memo.get(plain, "a", make(6)) == 6 and memo.get(plain, "a", make(7)) == 7, "a caller's own tensor is never memoised"
    t.mul_(2)
    assert const_tag(t) is None and memo.get(t, "a", make(8)) == 8, "an in-place write drops the tag"
    assert memo.get(u, "b", make(9)) == 9
    assert len(memo.entries) <= 2
    with torch.inference_mode():                      # inference tensors have no version counter (this used to raise)
        ti = const_timestep(500, (3,), "cpu")
        assert const_tag(ti) == 500.0 and memo.get(ti, "c", make(10)) == 10 and memo.get(ti, "c", make(11)) == 10
        sch_i = FlowMatchScheduler(shift=5.0, sigma_min=0.0, extra_one_step=True)
        xi, ni = torch.randn(3, 2, 2, 2), torch.randn(3, 2, 2, 2)
        assert torch.equal(sch_i.add_noise(xi, ni, ti), sch_i.add_noise(xi, ni, torch.ones(3, dtype=torch.int64) * 500))
    # a new sigma table invalidates the scheduler's memo
    sch2 = FlowMatchScheduler(shift=5.0, sigma_min=0.0, extra_one_step=True)
    tt = const_timestep(750, (3,), "cpu")
    xa, na = torch.randn(3, 2, 2, 2), torch.randn(3, 2, 2, 2)
    a1 = sch2.add_noise(xa, na, tt)
    sch2.shift = 3.0
    sch2.set_timesteps(1000)
    a2 = sch2.add_noise(xa, na, tt)
    sg = sch2.sigmas[sch2._lookup(tt, xa.device)].reshape(-1, 1, 1, 1)
    assert not torch.equal(a1, a2) and torch.equal(a2, ((1 - sg) * xa + sg * na).type_as(na))
    # the scheduler's add_noise through the memo equals the direct formula
    sch = FlowMatchScheduler(shift=5.0, sigma_min=0.0, extra_one_step=True)
    sch.set_timesteps(1000, training=True)
    g = torch.Generator().manual_seed(0)
    x0, eps = torch.randn(3, 4, 5, 6, generator=g).to(torch.bfloat16), torch.randn(3, 4, 5, 6, generator=g).to(torch.bfloat16)
    tn = const_timestep(750, (3,), "cpu", torch.long)
    first = sch.add_noise(x0, eps, tn)
    again = sch.add_noise(x0, eps, tn)
    sigma = sch.sigmas[sch._lookup(tn, x0.device)].reshape(-1, 1, 1, 1)
    assert torch.equal(first, again) and torch.equal(first, ((1 - sigma) * x0 + sigma * eps).type_as(eps))
