"""`ifx_frames_u8` / `hip_ops.frames_u8`: the decoder's bf16 pixels -> the uint8 frames of the streaming callback, bit for bit the fp32
chain `decode_to_pixel(...).float().clamp_(-1, 1)` -> `(v * 0.5 + 0.5).clamp(0, 1)` -> `clamp(v * 255, 0, 255).to(uint8)`."""
import ctypes as C
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF = torch.bfloat16


def chain(x: torch.Tensor) -> torch.Tensor:
    """The chain as the pipeline spells it today (vae.py `decode_to_pixel`, self_forcing.py `_to_frames` and `emit`), op by op in fp32."""
    v = x.float().clamp_(-1, 1)
    v = (v * 0.5 + 0.5).clamp(0, 1)
    return torch.clamp(v * 255.0, 0, 255).to(torch.uint8)


def all_patterns():
    """All 65 536 bf16 bit patterns minus the 254 NaNs (exponent all ones, mantissa non-zero) — the whole allowance."""
    bits = torch.arange(65536, dtype=torch.int32)
    nan = ((bits & 0x7F80) == 0x7F80) & ((bits & 0x007F) != 0)
    assert int(nan.sum()) == 254
    return bits[~nan].to(torch.int16).view(BF)


# ---- no GPU: the symbol through every layer, and the refusals ------------------------------------------------------------
def test_symbol_is_declared_bound_and_exported():
    from inferix_amd import _hip, hip_ops
    hdr = open(os.path.join(ROOT, "include", "inferix_hip.h")).read()
    assert re.search(r"int\s+ifx_frames_u8\(const ifx_bf16\*\s*x,\s*uint8_t\*\s*y,\s*int64_t\s+n,\s*void\*\s*stream\);", hdr)
    assert _hip.SIGNATURES["ifx_frames_u8"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p])
    lib = _hip.load()
    assert lib.ifx_frames_u8 is not None and callable(hip_ops.frames_u8)
    assert "ifx_frames.hip" in open(os.path.join(ROOT, "inferix_amd", "csrc", "Makefile")).read()
    assert int(re.search(r"#define\s+IFX_ABI_MINOR\s+(\d+)", hdr).group(1)) == 7 == _hip.ABI_MINOR      # an additive export


def test_refusals_and_empty_input_without_a_launch():
    """Null pointers and n < 0 are IFX_EINVAL with a message; n == 0 is OK and launches nothing (so it passes without a GPU, on
    pointers that are never dereferenced)."""
    from inferix_amd import _hip
    lib = _hip.load()
    buf = (C.c_uint16 * 16)()
    p = C.addressof(buf)
    err = lambda: lib.ifx_last_error().decode()
    assert lib.ifx_frames_u8(None, p, 8, None) == -1 and "ifx_frames_u8: null argument" in err()
    assert lib.ifx_frames_u8(p, None, 8, None) == -1 and "ifx_frames_u8: null argument" in err()
    assert lib.ifx_frames_u8(p, p, -1, None) == -1 and "ifx_frames_u8: negative element count -1" in err()
    assert lib.ifx_frames_u8(p + 1, p, 8, None) == -1 and "2-byte aligned" in err()
    assert lib.ifx_frames_u8(p, p, 0, None) == 0
    assert lib.ifx_frames_u8(p + 2, p + 3, 0, None) == 0


# ---- GPU -------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_every_bf16_value_equals_the_torch_chain():
    """All 65 282 non-NaN patterns (±0, ±inf, subnormals, every value either side of every k / 255 boundary bf16 can express)."""
    from inferix_amd import hip_ops
    x = all_patterns()
    assert x.numel() == 65536 - 254 and not torch.isnan(x.float()).any()
    want = chain(x)
    got = hip_ops.frames_u8(x.cuda())
    assert got.dtype == torch.uint8 and got.shape == x.shape
    assert torch.equal(got.cpu(), want)
    assert torch.equal(chain(x.cuda()).cpu(), want)                       # the chain itself gives the same bytes on either device
    assert int(want.min()) == 0 and int(want.max()) == 255 and len(torch.unique(want)) == 256
    # a [T, H, W, 3] block goes through as the flat array
    blk = x[:4 * 5 * 7 * 3].reshape(4, 5, 7, 3).cuda()
    assert torch.equal(hip_ops.frames_u8(blk).cpu(), want[:420].reshape(4, 5, 7, 3))


@pytest.mark.gpu
def test_nan_input_does_not_fault():
    """NaN is outside the contract: any byte may come out, the launch completes."""
    from inferix_amd import hip_ops
    bits = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(BF)
    got = hip_ops.frames_u8(bits.cuda())
    torch.cuda.synchronize()
    assert got.shape == bits.shape
    hip_ops.check_device("frames_u8 on NaNs")


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 7, 8, 9, 15, 16, 17, 1027])
def test_ragged_sizes_and_every_alignment(n):
    """Input element offsets 0 .. 7 (every position relative to a 16-byte load) x output byte offsets 0 .. 7 (aligned and unaligned
    stores): the n bytes are right and the guard bytes either side of them are untouched."""
    from inferix_amd import hip_ops
    src = all_patterns()
    src = src[torch.randperm(src.numel(), generator=torch.Generator().manual_seed(n))][:n + 8].contiguous()
    want = chain(src)
    xd = src.cuda()
    GUARD = 16
    for xo in range(8):
        for yo in range(8):
            out = torch.full((GUARD + yo + n + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
            view = out[GUARD + yo:GUARD + yo + n]
            assert view.data_ptr() % 8 == (out.data_ptr() + GUARD + yo) % 8
            hip_ops.frames_u8(xd[xo:xo + n], out=view)
            got = out.cpu()
            assert torch.equal(got[GUARD + yo:GUARD + yo + n], want[xo:xo + n]), (n, xo, yo)
            assert bool((got[:GUARD + yo] == 0xA5).all()) and bool((got[GUARD + yo + n:] == 0xA5).all()), (n, xo, yo)


@pytest.mark.gpu
def test_empty_tensor_and_wrapper_refusals():
    from inferix_amd import _hip, hip_ops
    e = hip_ops.frames_u8(torch.empty(0, 4, 4, 3, dtype=BF, device="cuda"))
    assert e.shape == (0, 4, 4, 3) and e.dtype == torch.uint8
    x = torch.zeros(4, 6, dtype=BF, device="cuda")
    with pytest.raises(ValueError):
        hip_ops.frames_u8(x.t())
    with pytest.raises(ValueError):
        hip_ops.frames_u8(x, out=torch.empty(23, dtype=torch.uint8, device="cuda"))
    with pytest.raises(TypeError):
        hip_ops.frames_u8(x.float())
    with pytest.raises(_hip.HipKernelError):
        hip_ops.frames_u8(x.cpu())


@pytest.mark.gpu
def test_more_than_one_pass_of_the_grid():
    """3 x 2^20 + 5 elements: 1536 workgroups' worth of 16-byte loads on a grid capped at 1024, so the grid-stride loop goes round, plus
    a tail of 5; and the same from an odd element offset (head of 7, unaligned stores)."""
    from inferix_amd import hip_ops
    n = 3 * 2 ** 20 + 5
    pats = all_patterns()
    idx = torch.randint(0, pats.numel(), (n + 1,), generator=torch.Generator().manual_seed(1))
    x = pats[idx].cuda()
    want = chain(x)
    assert torch.equal(hip_ops.frames_u8(x[:n]), want[:n])
    assert torch.equal(hip_ops.frames_u8(x[1:]), want[1:])
