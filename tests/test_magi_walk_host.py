"""CPU tests of the MAGI per-chunk generator's host half: the hand-out rule against tests/golden/magi_walk.npz (the reference's own
`integrate_velocity`, tools/gen_golden_magi_walk.py), the host-known step scalars against the device-side formulas of `ChunkSchedule.run` /
`_dispatch_3cfg` evaluated with torch, the new export, the reference import paths and `MagiPipeline` on stub parts."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from fixture_io import golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cases():
    fx = golden("magi_walk.npz")
    for c in range(int(fx["n_cases"])):
        yield c, fx, [int(v) for v in fx[f"c{c}_args"]]


def test_hand_out_rule_matches_the_reference_at_every_step():
    from inferix_amd.magi.schedule import ChunkSchedule
    seen_cases = 0
    for c, fx, (num_steps, window, chunk_num, cw, prefix_frames) in _cases():
        sch = ChunkSchedule(num_steps, window, chunk_num, cw, chunk_offset=prefix_frames // cw)
        want = fx[f"c{c}_hand_out"].tolist()
        got = sch.hand_outs(prefix_frames)
        assert len(got) == len(want) == sch.total_forward_step()
        for step, (g, w) in enumerate(zip(got, want)):
            assert (g is None) == (w[0] == 0), (c, step, g, w)
            if g is not None:
                assert list(g) == w[1:], (c, step, g, w)
        seen_cases += 1
    assert seen_cases == 6
    # the branches the cases are there for
    fx = golden("magi_walk.npz")
    assert fx["c3_hand_out"][fx["c3_hand_out"][:, 0] == 1][0].tolist() == [1, 0, 0, 2]          # image: frame 0 is kept
    assert fx["c4_hand_out"][fx["c4_hand_out"][:, 0] == 1][0].tolist() == [1, 0, 3, 4]          # a chunk the prefix reaches into
    assert fx["c5_hand_out"][fx["c5_hand_out"][:, 0] == 1][0].tolist() == [1, 0, 4, 6]          # starts exactly at the prefix's end


@pytest.mark.parametrize("tcfg,shortcut,num_steps,window,chunk_num,off,prefix_frames", [
    ({}, "8,16,16", 64, 4, 4, 0, 0),
    ({"tSchedulerFunc": "square"}, "", 8, 4, 4, 1, 3),
    ({"tSchedulerFunc": "sd3", "shift": 2.0}, "16,16,8", 12, 4, 5, 0, 1),
    ({"tSchedulerFunc": "piecewise"}, "", 16, 4, 6, 2, 4),
])
def test_host_step_scalars_equal_the_device_formulas_bit_for_bit(tcfg, shortcut, num_steps, window, chunk_num, off, prefix_frames):
    """timesteps (with the clean chunk's entry and the prefix's t = 1 rule), dt and the nearly-clean decision of every step: the host
    functions on one host copy of the grid against the tensor expressions `run` evaluates (here on the CPU)."""
    from inferix_amd.magi import schedule as S
    cw, clean_t, threshold = 2, 0.9999, 0.3
    sch = S.ChunkSchedule(num_steps, window, chunk_num, cw, chunk_offset=off)
    t_total = S.init_t(dict(tcfg), num_steps, "cpu", shortcut)
    interval = S.init_interval(num_steps, "cpu", shortcut)
    t_host, i_host = S.host_grid(t_total, interval)
    assert t_host.dtype == np.float32 and np.array_equal(t_host, t_total.numpy()) and np.array_equal(i_host, interval.float().numpy())
    decisions = set()
    for step in range(sch.total_forward_step()):
        p = sch.plan(step)
        t = sch.timestep(t_total, p, clean_t).unsqueeze(0).repeat(2, 1)
        start = p.slice_point * cw
        if prefix_frames > start:
            clean = (prefix_frames - start) // cw
            if clean > 0:
                t[:, :clean] = 1.0
        row = S.step_timesteps(t_host, p, clean_t, S.prefix_clean_chunks(prefix_frames, p.slice_point, cw))
        assert row.dtype == np.float32 and np.array_equal(row.view(np.uint32), t[0].numpy().view(np.uint32)), (step, row, t[0])
        dt = sch.timestep(t_total, p, clean_t, advance=1) - t_total[p.t_index]
        assert np.array_equal(S.step_dt(t_host, p).view(np.uint32), dt.numpy().view(np.uint32)), step
        want = t[0, int(p.fwd_extra_1st_chunk)].item() > threshold
        assert S.nearly_clean(row, p, threshold) == want
        decisions.add(want)
    assert decisions == {True, False}


def test_host_guidance_bins_and_weights_equal_the_device_formulas_bit_for_bit():
    """`searchsorted(t_range - 1e-7, t) - 1` and the three weights as `_dispatch_3cfg` forms them, including timesteps that sit exactly on
    an edge of `cfg_t_range`, one fp32 step below it and one above."""
    from inferix_amd.magi import schedule as S
    t_range, prev, text = [0.0, 0.0217, 0.3, 0.7], [1.5, 1.5, 1.1, 1.0], [7.5, 7.5, 3.3, 0.0]
    tr = torch.tensor(t_range)
    edge = tr[1:].clone()
    ts = torch.cat([edge, torch.nextafter(edge, torch.zeros(())), torch.nextafter(edge, torch.ones(())),
                    edge - 1e-7, torch.tensor([0.0, 1e-8, 0.01, 0.2999, 0.5, 0.9999, 1.0])])
    bins = S.cfg_bins(ts.numpy(), t_range)
    want_bins = [int(torch.searchsorted(tr - 1e-7, t) - 1) for t in ts]
    assert bins == want_bins
    assert set(bins) == {0, 1, 2, 3}
    on_edge = bins[:3]
    assert on_edge == [1, 2, 3], on_edge                     # t == edge k belongs to bin k: the edges are shifted down by 1e-7
    prev_s, text_s = torch.tensor(prev), torch.tensor(text)
    w0, w1, w2 = S.cfg_weights(bins, prev, text)
    for i, b in enumerate(want_bins):
        idx = torch.tensor(b)
        sp, st = prev_s[idx], text_s[idx]
        for got, want in ((w0[i], 1 - sp), (w1[i], sp - st), (w2[i], st)):
            assert np.float32(got).view(np.uint32) == want.numpy().view(np.uint32) and float(np.float32(got)) == got, (i, got, want)
    with pytest.raises(AssertionError):
        S.cfg_bins(np.asarray([-0.5], np.float32), t_range)
    # the nearly-clean blend: `out * scale + out2 * (1 - scale)` with a Python float scale
    a, b = S.nearly_clean_weights(0.7)
    x = torch.tensor([1.2345678, -3.25e-3, 7.0e5])
    assert torch.equal(x * 0.7, x * torch.tensor(a)) and torch.equal(x * (1 - 0.7), x * torch.tensor(b))


def test_magi_integrate_is_exported_bound_and_refuses_a_ninth_chunk():
    from inferix_amd import _hip
    hdr = open(os.path.join(ROOT, "include", "inferix_hip.h")).read()
    assert re.search(r"\bint\s+ifx_magi_integrate\s*\(const ifx_magi_integrate_desc\*", hdr)
    assert int(re.search(r"#define\s+IFX_ABI_MINOR\s+(\d+)", hdr).group(1)) == 7 == _hip.ABI_MINOR
    assert int(re.search(r"#define\s+IFX_MAGI_INTEGRATE_MAX_CHUNKS\s+(\d+)", hdr).group(1)) == _hip.IFX_MAGI_INTEGRATE_MAX_CHUNKS == 8
    assert "ifx_magi_integrate" in _hip.SIGNATURES
    lib = _hip.load()
    assert (lib.ifx_version() >> 8) & 255 == 7
    # the bindings' struct is the header's: 8 + 8 + 8 + 8 x 4 + 8 x 4 bytes in front of three sources of 8 + 8 + 4 x 4 + 8 x 4
    assert C.sizeof(_hip.MagiIntegrateSrc) == 64 and C.sizeof(_hip.MagiIntegrateDesc) == 88 + 3 * 64
    assert _hip.MagiIntegrateDesc.dt.offset == 56 and _hip.MagiIntegrateDesc.src.offset == 88
    d = _hip.MagiIntegrateDesc()
    keep = (C.c_float * 16)()                                  # validation comes before any launch: no GPU is touched
    d.x, d.row_stride, d.chan_stride, d.rows, d.channels, d.frames, d.frame_elems = C.addressof(keep), 0, 16, 1, 1, 16, 1
    d.chunk_width, d.chunk_start, d.n_chunks, d.n_src = 1, 0, 9, 1
    assert lib.ifx_magi_integrate(C.byref(d), None) == -1
    assert b"9 chunks" in lib.ifx_last_error()
    d.n_chunks, d.n_src = 2, 4
    assert lib.ifx_magi_integrate(C.byref(d), None) == -1 and b"sources" in lib.ifx_last_error()
    d.n_src, d.chunk_start = 1, 15
    assert lib.ifx_magi_integrate(C.byref(d), None) == -1 and b"run past the clip" in lib.ifx_last_error()
    d.chunk_start = 0
    s = d.src[0]
    s.v, s.chan_stride, s.frames, s.first_frame, s.first_chunk, s.last_chunk = C.addressof(keep), 16, 2, 1, 0, 1
    assert lib.ifx_magi_integrate(C.byref(d), None) == -1 and b"run past its 2 frames" in lib.ifx_last_error()
    s.first_frame, s.last_chunk = 0, 0
    assert lib.ifx_magi_integrate(C.byref(d), None) == -1 and b"source 0 must cover" in lib.ifx_last_error()


def test_magi_integrate_wrapper_refuses_what_the_kernel_cannot_take():
    from inferix_amd import _hip
    from inferix_amd import hip_ops as ops
    x = torch.zeros(1, 2, 4, 2, 2)
    with pytest.raises(_hip.HipKernelError, match="GPU only"):
        ops.magi_integrate(x, 0, 1, [0.1], [(x[0], 0, 0, 0, [1.0])])
    with pytest.raises(ValueError, match="9 chunks"):
        ops.magi_integrate(x, 0, 1, [0.1] * 9, [(x[0], 0, 0, 8, [1.0] * 9)])


def test_guidance_forwards_build_their_small_tensors_without_a_host_list():
    """`forward_3cfg` and `generate_kv_range_for_uncondition` form the caption-dropout flags and the unconditional key ranges with tensor
    operators on the model's device (a host list would be a blocking upload in every step of `walk`): the values and dtypes are those of
    the literals `[False, True]`, `[True]` and `[[b n, (b + 1) n] for b in range(B)]` int32."""
    from inferix_amd.magi.model import HipVideoDiTModel

    class Fake:
        forward_3cfg = HipVideoDiTModel.forward_3cfg
        generate_kv_range_for_uncondition = HipVideoDiTModel.generate_kv_range_for_uncondition
        device, patch_size, t_patch_size = torch.device("cpu"), 2, 1

        def __init__(self):
            self.calls = []

        def forward(self, x, t, y, caption_dropout_mask=None, xattn_mask=None, kv_range=None, inference_params=None, **kw):
            self.calls.append((caption_dropout_mask, kv_range, inference_params is not None and inference_params.update_kv_cache))
            return torch.zeros_like(x)

    m = Fake()
    for B, shape in ((1, (3, 2, 4, 6)), (3, (3, 2, 4, 6)), (4, (5, 6, 8, 2))):
        got = m.generate_kv_range_for_uncondition(torch.zeros(B, *shape))
        n = shape[1] * (shape[2] // 2) * (shape[3] // 2)
        want = torch.tensor([[b * n, (b + 1) * n] for b in range(B)], dtype=torch.int32)
        assert got.dtype == torch.int32 and got.shape == (B, 2) and torch.equal(got, want)
    dn, cw = 3, 2
    x = torch.zeros(2, 3, (dn + 1) * cw, 4, 6)
    t = torch.zeros(2, dn + 1)
    y, mask = torch.zeros(2 * (dn + 1), 1, 5, 8), torch.ones(2 * (dn + 1), 1, 5)
    kv = torch.zeros(dn + 1, 2, dtype=torch.int32)
    ip = SimpleNamespace(update_kv_cache=False)
    m.forward_3cfg(x, t, y, mask, kv, ip, chunk_width=cw, denoising_range_num=dn + 1, fwd_extra_1st_chunk=True, range_num=dn + 1,
                   slice_point=0)
    (d0, k0, u0), (d1, k1, u1), (d2, k2, u2) = m.calls
    assert [d.dtype for d in (d0, d1, d2)] == [torch.bool] * 3
    assert d0.tolist() == [False] and d1.tolist() == [True] and d2.tolist() == [True]
    assert (u0, u1, u2) == (False, True, False) and k0 is kv and k1 is kv
    per = cw * 2 * 3
    assert k2.dtype == torch.int32 and k2.tolist() == [[b * per, (b + 1) * per] for b in range(dn)]


def test_magi_integrate_wrapper_takes_any_stride_on_a_dimension_of_size_one():
    from inferix_amd import hip_ops as ops
    base = torch.zeros(4000)
    ok = lambda size, stride: ops._thw_contiguous(base.as_strided(size, stride))
    assert ok((2, 4, 3, 5), (60, 15, 5, 1)) and ok((2, 4, 3, 5), (100, 15, 5, 1))          # channel stride is the caller's business
    assert ok((2, 1, 3, 5), (105, 999, 5, 1))                                              # one frame: any frame stride
    assert ok((2, 4, 1, 5), (20, 5, 77, 1)) and ok((2, 4, 3, 1), (12, 3, 1, 9))            # H == 1, W == 1
    assert not ok((2, 4, 3, 5), (120, 30, 10, 2)) and not ok((2, 4, 3, 5), (120, 30, 10, 1))
    assert not ok((2, 4, 3, 5), (80, 20, 5, 1)) and not ok((2, 4, 1, 5), (40, 10, 77, 1))  # T > 1: the frame stride counts


def test_reference_import_paths_resolve_to_the_port():
    import inferix.pipeline.magi.pipeline as P
    import inferix.pipeline.magi.video_generate as G
    import inferix.pipeline.magi.video_process as V
    import inferix_amd.magi.schedule as S
    import inferix_amd.magi.vae as A
    from inferix_amd.pipeline.base_pipeline import AbstractInferencePipeline
    from inferix_amd.pipeline.magi import MagiPipeline
    assert P.MagiPipeline is MagiPipeline and issubclass(MagiPipeline, AbstractInferencePipeline)
    assert G.generate_per_chunk is S.generate_per_chunk
    assert V.post_chunk_process is A.post_chunk_process and V.decode_chunk is A.decode_chunk


class _Embedder:
    model_max_length = 6

    def __init__(self, log):
        self.log = log

    def get_text_embeddings(self, prompts):
        self.log.append(("embed", list(prompts)))
        return torch.ones(1, 6, 4), torch.ones(1, 6)


def _stub_pipeline(monkeypatch, log, writer=True):
    import inferix_amd.magi.vae as A
    import inferix_amd.pipeline.magi as PM
    config = SimpleNamespace(model_config=SimpleNamespace(caption_max_length=6), engine_config=SimpleNamespace(),
                             runtime_config=SimpleNamespace(fps=24, scale_factor=0.5))
    vae, dit = object(), object()

    def encode(pixels, fps, v, scale_factor, parallel_group=None):
        assert v is vae
        log.append(("encode", tuple(pixels.shape), fps, scale_factor))
        return torch.full((1, 2, pixels.shape[0], 1, 1), 9.0)

    def generate(model, prefix_video, caption_embs, emb_masks):
        assert model is dit and tuple(caption_embs.shape) == (1, 1, 6, 4) and tuple(emb_masks.shape) == (1, 6)
        log.append(("generate", None if prefix_video is None else tuple(prefix_video.shape)))
        for i in range(3):
            log.append(("chunk", i))
            yield torch.full((1, 2, 2, 1, 1), float(i + 1))

    def decode(chunk, v, tile_sample_min_height=256, tile_sample_min_width=256, spatial_tile_overlap_factor=0.25,
               temporal_tile_overlap_factor=0, tile_sample_min_length=16, allow_spatial_tiling=True, uint8_output=True,
               parallel_group=None):
        assert v is vae and uint8_output and allow_spatial_tiling and temporal_tile_overlap_factor == 0
        assert (tile_sample_min_height, tile_sample_min_width, spatial_tile_overlap_factor) == (256, 256, 0.25)
        log.append(("decode", float(chunk.flatten()[0]), tile_sample_min_length))
        return chunk.flatten()[0].to(torch.uint8).reshape(1, 1, 1, 1).expand(chunk.shape[2], 3, 2, 2).clone()

    monkeypatch.setattr(PM, "encode_prefix_video", encode)
    monkeypatch.setattr(PM, "generate_per_chunk", generate)
    monkeypatch.setattr(A.VaeHelper, "decode", staticmethod(decode))
    w = (lambda frames, path, fps: log.append(("write", tuple(frames.shape), path, fps))) if writer else None
    return PM.MagiPipeline(config, dit=dit, vae=vae, embedder=_Embedder(log), writer=w)


def test_magi_pipeline_on_stub_parts(monkeypatch):
    log = []
    pipe = _stub_pipeline(monkeypatch, log)
    assert torch.is_grad_enabled(), "constructing the pipeline must not switch autograd off for the process"
    frames = pipe.run_text_to_video("a prompt", "out.mp4")
    assert torch.is_grad_enabled()
    # each chunk is decoded as it arrives, before the generator is asked for the next one; fps // 2 and 1 / scale_factor reach the decode
    assert log == [("embed", ["a prompt"]), ("generate", None), ("chunk", 0), ("decode", 2.0, 12), ("chunk", 1), ("decode", 4.0, 12),
                   ("chunk", 2), ("decode", 6.0, 12), ("write", (6, 3, 2, 2), "out.mp4", 24)]
    assert frames.dtype == torch.uint8 and tuple(frames.shape) == (6, 3, 2, 2)
    assert frames[:, 0, 0, 0].tolist() == [2, 2, 4, 4, 6, 6]                                     # concatenated in arrival order
    log.clear()
    pipe.run_image_to_video("p", image=torch.zeros(1, 4, 4, 3, dtype=torch.uint8))
    assert log[:3] == [("encode", (1, 4, 4, 3), 24, 0.5), ("embed", ["p"]), ("generate", (1, 2, 1, 1, 1))] and log[-1][2] == "./output.mp4"
    log.clear()
    pipe.run_video_to_video("p", prefix_video=torch.zeros(5, 4, 4, 3, dtype=torch.uint8), output_path="v.mp4")
    assert log[0] == ("encode", (5, 4, 4, 3), 24, 0.5) and log[2] == ("generate", (1, 2, 5, 1, 1)) and log[-1][2:] == ("v.mp4", 24)
    with pytest.raises(RuntimeError, match="image="):
        pipe.run_image_to_video("p", "cat.png")
    with pytest.raises(RuntimeError, match="prefix_video="):
        pipe.run_video_to_video("p", "clip.mp4")
    with pytest.raises(NotImplementedError, match="Streaming generation is not yet implemented"):
        pipe._generate_segment_with_streaming("p", None, None)
    log.clear()
    quiet = _stub_pipeline(monkeypatch, log, writer=False)
    assert tuple(quiet.run_text_to_video("p").shape) == (6, 3, 2, 2) and not any(e[0] == "write" for e in log)
