"""The YUV 4:2:0 conversion of include/inferix_hip.h (ifx_frames_yuv420 / ifx_rgb8_yuv420) restated in integer torch on the CPU: the
yardstick of the YUV tests.  Test infrastructure: product code never imports it, and the table below is written out again here instead
of being read from `hip_ops.YUV420_PRESETS`, so that a slip in either shows."""
import torch

# (matrix, full_range) -> (m row-major, a)
PRESETS = {
    ("bt601", False): ((66, 129, 25, -38, -74, 112, 112, -94, -18), (4224, 32896, 32896)),
    ("bt709", False): ((47, 157, 16, -26, -86, 112, 112, -102, -10), (4224, 32896, 32896)),
    ("bt601", True): ((77, 150, 29, -43, -85, 128, 128, -107, -21), (128, 32896, 32896)),
    ("bt709", True): ((54, 183, 19, -29, -99, 128, 128, -116, -12), (128, 32896, 32896)),
}
ALL_PRESETS = sorted(PRESETS)
CORNERS = [(r, g, b) for r in (0, 255) for g in (0, 255) for b in (0, 255)]


def row_sums(rgb: torch.Tensor, matrix: str, full_range: bool, row: int) -> torch.Tensor:
    """`m[row] . rgb + a[row]` before the shift and the clamp; `rgb` integer `[..., 3]` (int32 holds every sum: |.| < 2^17)."""
    m, a = PRESETS[(matrix, bool(full_range))]
    v = rgb.to(torch.int32)
    return m[3 * row] * v[..., 0] + m[3 * row + 1] * v[..., 1] + m[3 * row + 2] * v[..., 2] + a[row]


def mix(rgb: torch.Tensor, matrix: str, full_range: bool, row: int) -> torch.Tensor:
    return (row_sums(rgb, matrix, full_range, row) >> 8).clamp(0, 255)


def quad_mean(rgb: torch.Tensor) -> torch.Tensor:
    """`[..., H, W, 3]` -> `[..., H / 2, W / 2, 3]`: `(p00 + p01 + p10 + p11 + 2) >> 2` per channel."""
    v = rgb.to(torch.int32)
    return (v[..., 0::2, 0::2, :] + v[..., 0::2, 1::2, :] + v[..., 1::2, 0::2, :] + v[..., 1::2, 1::2, :] + 2) >> 2


def planes(rgb: torch.Tensor, matrix: str = "bt601", full_range: bool = False):
    """uint8 `[..., H, W, 3]` -> (Y `[..., H, W]`, U, V `[..., H / 2, W / 2]`), uint8."""
    assert rgb.dtype == torch.uint8 and rgb.shape[-1] == 3 and rgb.shape[-3] % 2 == 0 and rgb.shape[-2] % 2 == 0
    q = quad_mean(rgb)
    return (mix(rgb, matrix, full_range, 0).to(torch.uint8), mix(q, matrix, full_range, 1).to(torch.uint8),
            mix(q, matrix, full_range, 2).to(torch.uint8))


def pack(y: torch.Tensor, u: torch.Tensor, v: torch.Tensor, layout: str) -> torch.Tensor:
    """Planes -> `[..., H * 3 / 2, W]`: `i420` Y, U, V; `nv12` Y, then U and V interleaved."""
    lead, (H, W) = tuple(y.shape[:-2]), y.shape[-2:]
    if layout == "i420":
        chroma = torch.cat([u.reshape(*lead, -1), v.reshape(*lead, -1)], dim=-1)
    else:
        assert layout == "nv12", layout
        chroma = torch.stack([u, v], dim=-1).reshape(*lead, -1)
    return torch.cat([y.reshape(*lead, -1), chroma], dim=-1).reshape(*lead, H * 3 // 2, W)


LAYOUT_OF = {"yuv420p": "i420", "nv12": "nv12", "i420": "i420"}


def rgb_to_yuv420(rgb: torch.Tensor, layout: str = "i420", matrix: str = "bt601", full_range: bool = False) -> torch.Tensor:
    """uint8 `[..., H, W, 3]` -> uint8 `[..., H * 3 / 2, W]`; `layout` also takes a stream's pixel-format name."""
    return pack(*planes(rgb, matrix, full_range), LAYOUT_OF[layout])


def bf16_to_u8(x: torch.Tensor) -> torch.Tensor:
    """The fp32 chain of `ifx_frames_u8` (tests/test_hip_frames.py::chain)."""
    v = x.float().clamp_(-1, 1)
    v = (v * 0.5 + 0.5).clamp(0, 1)
    return torch.clamp(v * 255.0, 0, 255).to(torch.uint8)
