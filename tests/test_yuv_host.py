"""CPU: YUV 4:2:0 frame finishing (`ifx_frames_yuv420`, `ifx_rgb8_yuv420`) below the kernels — the exports through every layer, the
refusals of the C ABI and of the Python wrappers, the properties of the integer definition (tests/yuv_util.py) that make it a sound
yardstick, `yuv420_planes`, and the pixel-format keywords of the segment loops.  Nothing here touches a device."""
import ctypes as C
import os
import re

import pytest
import torch

import yuv_util as Y

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("ifx_frames_yuv420", "ifx_rgb8_yuv420")


def test_symbols_are_declared_bound_and_exported_without_an_abi_bump():
    from inferix_amd import _hip, hip_ops
    hdr = open(os.path.join(ROOT, "include", "inferix_hip.h")).read()
    lib = _hip.load()
    args = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(_hip.Yuv420Desc), C.c_void_p]
    for name, src in zip(SYMBOLS, ("const ifx_bf16", "const uint8_t")):
        decl = re.search(r"\bint %s\(([^;]*)\);" % name, hdr)
        assert decl and decl.group(1).split(",")[0].strip() == src + "* x", name
        assert len([a for a in decl.group(1).split(",") if a.strip()]) == len(args)
        assert _hip.SIGNATURES[name] == (C.c_int, args) and getattr(lib, name) is not None
    assert callable(hip_ops.frames_yuv420) and callable(hip_ops.rgb8_to_yuv420)
    assert re.search(r"typedef struct ifx_yuv420_desc \{\s*int32_t m\[9\];[^}]*int32_t a\[3\];", hdr)
    assert C.sizeof(_hip.Yuv420Desc) == 48
    assert re.search(r"#define IFX_YUV420_I420 0\b", hdr) and re.search(r"#define IFX_YUV420_NV12 1\b", hdr)
    assert (_hip.IFX_YUV420_I420, _hip.IFX_YUV420_NV12) == (0, 1)
    assert (lib.ifx_version() >> 8) & 255 == 7 == _hip.ABI_MINOR and re.search(r"#define IFX_ABI_MINOR 7\b", hdr)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert f"({len(_hip.SIGNATURES)} `extern \"C\"` entry points" in doc, "INTEGRATION.md's export count"
    assert hip_ops.YUV420_PRESETS == Y.PRESETS, "the host's presets are the issue's table"


@pytest.mark.parametrize("name", SYMBOLS)
def test_c_abi_refusals_on_dummy_pointers(name):
    """Every refusal comes before the launch, so pointers that are never dereferenced do; `t == 0` launches nothing."""
    from inferix_amd import _hip
    lib = _hip.load()
    fn = getattr(lib, name)
    buf = (C.c_uint16 * 64)()
    p = C.addressof(buf)
    m, a = Y.PRESETS[("bt601", False)]
    d = C.byref(_hip.Yuv420Desc((C.c_int32 * 9)(*m), (C.c_int32 * 3)(*a)))
    err = lambda: lib.ifx_last_error().decode()
    assert fn(None, p, 1, 2, 2, 0, d, None) == -1 and f"{name}: null argument" in err()
    assert fn(p, None, 1, 2, 2, 0, d, None) == -1 and f"{name}: null argument" in err()
    assert fn(p, p, 1, 2, 2, 0, None, None) == -1 and f"{name}: null argument" in err()
    assert fn(p, p, 1, 3, 2, 0, d, None) == -1 and f"{name}: 4:2:0 needs an even frame size, got h 3, w 2" in err()
    assert fn(p, p, 1, 2, 7, 1, d, None) == -1 and f"{name}: 4:2:0 needs an even frame size, got h 2, w 7" in err()
    assert fn(p, p, -1, 2, 2, 0, d, None) == -1 and f"{name}: negative size (t -1, h 2, w 2)" in err()
    assert fn(p, p, 1, -2, 2, 0, d, None) == -1 and f"{name}: negative size (t 1, h -2, w 2)" in err()
    assert fn(p, p, 1, 2, -2, 0, d, None) == -1 and f"{name}: negative size (t 1, h 2, w -2)" in err()
    assert fn(p, p, 1, 2, 2, 2, d, None) == -1 and f"{name}: unknown layout 2" in err()
    assert fn(p, p, 1, 2, 2, -1, d, None) == -1 and f"{name}: unknown layout -1" in err()
    assert fn(p, p, 0, 2, 2, 0, d, None) == 0
    assert fn(p, p + 3, 0, 480, 832, 1, d, None) == 0


def test_wrapper_refusals_that_need_no_device():
    from inferix_amd import hip_ops
    for fn, dtype in ((hip_ops.frames_yuv420, torch.bfloat16), (hip_ops.rgb8_to_yuv420, torch.uint8)):
        x = torch.zeros(1, 4, 6, 3, dtype=dtype)
        with pytest.raises(ValueError, match="layout is one of"):
            fn(x, layout="yuv444")
        with pytest.raises(ValueError, match="matrix is one of"):
            fn(x, matrix="bt2020")
        with pytest.raises(ValueError, match=r"even frame size, got 3 x 6"):
            fn(torch.zeros(1, 3, 6, 3, dtype=dtype))
        with pytest.raises(ValueError, match=r"even frame size, got 4 x 5"):
            fn(torch.zeros(1, 4, 5, 3, dtype=dtype))
        with pytest.raises(ValueError, match=r"must be \[T, H, W, 3\]"):
            fn(torch.zeros(4, 6, 3, dtype=dtype))
        with pytest.raises(ValueError, match="x must be contiguous"):
            fn(torch.zeros(1, 6, 4, 3, dtype=dtype).transpose(1, 2))
        with pytest.raises(ValueError, match="out must be contiguous with 36 elements"):
            fn(x, out=torch.empty(1, 4, 6, 3, dtype=torch.uint8))
        with pytest.raises(ValueError, match="out must be contiguous with 36 elements"):
            fn(x, out=torch.empty(1, 6, 12, dtype=torch.uint8)[..., ::2])


# ---- the definition -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("matrix,full_range", Y.ALL_PRESETS)
def test_ranges_over_all_triples(matrix, full_range):
    """256^3 triples: every sum is non-negative (so `>> 8` is a plain division), limited range stays inside 16 .. 235 / 16 .. 240 and
    reaches both ends, full range covers 0 .. 255 in luma and 1 .. 255 in chroma (-128 * 255 + 32896 = 256 -> 1 at the low end,
    128 * 255 + 32896 = 65536 -> 256 -> 255 at the high end)."""
    gb = torch.stack(torch.meshgrid(torch.arange(256), torch.arange(256), indexing="ij"), dim=-1)          # [256, 256, 2]
    lo, hi, least = [255] * 3, [0] * 3, 0
    for r0 in range(0, 256, 32):
        r = torch.arange(r0, r0 + 32).view(32, 1, 1, 1).expand(32, 256, 256, 1)
        rgb = torch.cat([r, gb.expand(32, 256, 256, 2)], dim=-1)
        for row in range(3):
            s = Y.row_sums(rgb, matrix, full_range, row)
            least = min(least, int(s.min()))
            v = (s >> 8).clamp(0, 255)
            lo[row], hi[row] = min(lo[row], int(v.min())), max(hi[row], int(v.max()))
    assert least >= 0
    assert (lo, hi) == (([0, 1, 1], [255, 255, 255]) if full_range else ([16, 16, 16], [235, 240, 240]))


@pytest.mark.parametrize("matrix,full_range", Y.ALL_PRESETS)
def test_greys_and_cube_corners(matrix, full_range):
    grey = torch.arange(256, dtype=torch.uint8).view(256, 1, 1, 1).expand(256, 2, 2, 3).contiguous()
    y, u, v = Y.planes(grey, matrix, full_range)
    assert bool((u == 128).all()) and bool((v == 128).all()), "grey carries no chroma"
    assert y[0, 0, 0] == (0 if full_range else 16) and y[255, 0, 0] == (255 if full_range else 235)
    assert bool((y[1:, 0, 0].int() - y[:-1, 0, 0].int() >= 0).all())
    corners = torch.tensor(Y.CORNERS, dtype=torch.uint8).view(8, 1, 1, 3).expand(8, 2, 2, 3).contiguous()
    y, u, v = Y.planes(corners, matrix, full_range)
    lo, lo_c, hi_y, hi_c = (0, 1, 255, 255) if full_range else (16, 16, 235, 240)
    by = {c: (int(y[i, 0, 0]), int(u[i, 0, 0]), int(v[i, 0, 0])) for i, c in enumerate(Y.CORNERS)}
    assert by[(0, 0, 0)] == (lo, 128, 128) and by[(255, 255, 255)] == (hi_y, 128, 128)
    assert by[(0, 0, 255)][1] == hi_c and by[(255, 255, 0)][1] == lo_c          # Cb: blue against yellow
    assert by[(255, 0, 0)][2] == hi_c and by[(0, 255, 255)][2] == lo_c          # Cr: red against cyan
    if full_range:                                                              # 128 * 255 + 32896 = 65536: 256 before the clamp
        blue, red = torch.tensor([0, 0, 255]), torch.tensor([255, 0, 0])
        assert int(Y.row_sums(blue, matrix, True, 1)) >> 8 == 256 and int(Y.row_sums(red, matrix, True, 2)) >> 8 == 256


def test_quad_mean_rounds_half_up_and_packs_both_layouts():
    rgb = torch.tensor([[[1, 0, 255], [2, 0, 255]], [[2, 1, 255], [2, 0, 254]]], dtype=torch.uint8)       # one quad
    assert Y.quad_mean(rgb).flatten().tolist() == [2, 0, 255]                   # (7 + 2) >> 2, (1 + 2) >> 2, (1019 + 2) >> 2
    y = torch.arange(32, dtype=torch.uint8).view(4, 8)
    u, v = 100 + torch.arange(8, dtype=torch.uint8).view(2, 4), 200 + torch.arange(8, dtype=torch.uint8).view(2, 4)
    assert Y.pack(y, u, v, "i420").flatten().tolist() == list(range(32)) + list(range(100, 108)) + list(range(200, 208))
    assert Y.pack(y, u, v, "nv12")[4:].flatten().tolist() == [k for i in range(8) for k in (100 + i, 200 + i)]


@pytest.mark.parametrize("layout", ["i420", "nv12"])
@pytest.mark.parametrize("lead,H,W", [((), 2, 2), ((3,), 6, 24), ((2, 3), 4, 10)])
def test_yuv420_planes_round_trips(layout, lead, H, W):
    """H = 6 is the case whose chroma planes do not end on a row of the `[H * 3 / 2, W]` array."""
    from inferix_amd.streaming import yuv420_planes
    g = torch.Generator().manual_seed(H * W)
    y = torch.randint(0, 256, lead + (H, W), generator=g, dtype=torch.uint8)
    u = torch.randint(0, 256, lead + (H // 2, W // 2), generator=g, dtype=torch.uint8)
    v = torch.randint(0, 256, lead + (H // 2, W // 2), generator=g, dtype=torch.uint8)
    frames = Y.pack(y, u, v, layout)
    assert tuple(frames.shape) == lead + (H * 3 // 2, W)
    got = yuv420_planes(frames, layout)
    assert all(torch.equal(a, b) for a, b in zip(got, (y, u, v)))
    base = frames.untyped_storage().data_ptr()
    assert all(p.untyped_storage().data_ptr() == base for p in got), "the planes are views"
    if layout == "nv12":
        assert got[1].stride(-1) == 2 and got[2].storage_offset() == got[1].storage_offset() + 1
    got[1].fill_(7)
    assert bool((yuv420_planes(frames, layout)[1] == 7).all()) and torch.equal(yuv420_planes(frames, layout)[2], v)
    if layout == "i420":
        assert all(torch.equal(a, b) for a, b in zip(yuv420_planes(frames, "yuv420p"), yuv420_planes(frames, "i420")))


def test_yuv420_planes_refusals():
    from inferix_amd.streaming import yuv420_planes
    with pytest.raises(ValueError, match="layout is one of"):
        yuv420_planes(torch.zeros(6, 4, dtype=torch.uint8), "yv12")
    with pytest.raises(ValueError, match="is not H \\* 3 / 2 rows"):
        yuv420_planes(torch.zeros(4, 4, dtype=torch.uint8))
    with pytest.raises(ValueError, match="is not H \\* 3 / 2 rows"):
        yuv420_planes(torch.zeros(6, 5, dtype=torch.uint8))


# ---- the keywords of the segment loops ----------------------------------------------------------------------------------------
class _Stream:
    frames_pushed = 0

    def flush(self):
        pass

    def video(self):
        return None


def _stub_pipeline():
    from inferix_amd.pipeline import AbstractInferencePipeline

    class Stub(AbstractInferencePipeline):
        made, calls = None, None

        def load_checkpoint(self, checkpoint_path, **kw):
            pass

        def run_text_to_video(self, prompts, **kw):
            pass

        def run_image_to_video(self, prompts, image_path, **kw):
            pass

        def _make_frame_stream(self, stream_callback, keep_video=True, **kw):
            self.made = kw
            return _Stream()

        def _generate_segment_with_streaming(self, prompt, initial_latent, stream_callback, segment_length=21, **kw):
            self.calls = (self.calls or []) + [kw]
            return None, torch.zeros(1, segment_length, 2, 2, 2)
    return Stub({})


def test_pixel_format_keywords_reach_the_stream_and_not_the_segments():
    from inferix_amd.core import InteractiveSession
    p = _stub_pipeline()
    p.run_streaming_generation(["a"], num_segments=2, segment_length=6, continuous=True, pixel_format="nv12", color_matrix="bt709",
                               full_range=True)
    assert p.made == dict(num_samples=1, pixel_format="nv12", matrix="bt709", full_range=True)
    assert all(not {"pixel_format", "color_matrix", "full_range", "matrix"} & set(kw) for kw in p.calls)
    p = _stub_pipeline()
    p.run_interactive_generation(InteractiveSession(), "a", num_segments=1, segment_length=6, continuous=True, pixel_format="yuv420p")
    assert p.made == dict(num_samples=1, pixel_format="yuv420p")
    p = _stub_pipeline()
    p.run_streaming_generation(["a"], num_segments=1, segment_length=6, continuous=True)
    assert p.made == dict(num_samples=1)


def test_keywords_that_disagree_with_a_given_stream_are_refused():
    """A caller's own `frame_stream` keeps its format: a keyword that asks for another one raises instead of being dropped."""
    rgb, nv12 = _Stream(), _Stream()
    nv12.pixel_format, nv12.matrix, nv12.full_range = "nv12", "bt709", False
    run = dict(num_segments=1, segment_length=6, continuous=True)
    p = _stub_pipeline()
    with pytest.raises(ValueError, match="pixel_format='nv12' disagrees with the given frame_stream.*pixel_format='rgb24'"):
        p.run_streaming_generation(["a"], frame_stream=rgb, pixel_format="nv12", **run)
    with pytest.raises(ValueError, match="pixel_format='rgb24' disagrees"):
        p.run_streaming_generation(["a"], frame_stream=nv12, pixel_format="rgb24", **run)
    with pytest.raises(ValueError, match="matrix='bt601' disagrees.*matrix='bt709'"):
        p.run_streaming_generation(["a"], frame_stream=nv12, pixel_format="nv12", color_matrix="bt601", **run)
    with pytest.raises(ValueError, match="full_range=True disagrees"):
        p.run_streaming_generation(["a"], frame_stream=nv12, full_range=True, **run)
    assert p.calls is None and p.made is None
    p.run_streaming_generation(["a"], frame_stream=nv12, pixel_format="nv12", color_matrix="bt709", full_range=False, **run)
    p.run_streaming_generation(["a"], frame_stream=nv12, **run)
    p.run_streaming_generation(["a"], frame_stream=rgb, pixel_format="rgb24", color_matrix="bt709", **run)     # says nothing about rgb24
    assert len(p.calls) == 3 and all(kw["frame_stream"] in (rgb, nv12) for kw in p.calls) and p.made is None


@pytest.mark.parametrize("fmt", ["yuv420p", "nv12"])
def test_a_yuv_pixel_format_needs_continuous(fmt):
    from inferix_amd.core import InteractiveSession
    p = _stub_pipeline()
    with pytest.raises(ValueError, match=f"pixel_format '{fmt}' needs continuous=True"):
        p.run_streaming_generation(["a"], num_segments=1, segment_length=6, pixel_format=fmt)
    with pytest.raises(ValueError, match=f"pixel_format '{fmt}' needs continuous=True"):
        p.run_interactive_generation(InteractiveSession(), "a", num_segments=1, segment_length=6, pixel_format=fmt)
    assert p.calls is None and p.made is None
    p.run_streaming_generation(["a"], num_segments=1, segment_length=6, pixel_format="rgb24")         # the default, spelled out
    assert p.made is None and len(p.calls) == 1 and "pixel_format" not in p.calls[0]
