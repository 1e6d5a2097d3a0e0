"""CPU: the host side of MAGI's continuous streaming — the opt-in gate of `MagiPipeline._generate_segment_with_streaming`, the
`[1, T, C, h, w]` <-> `[1, C, T, h, w]` conversion of the overlap latents, the prefix keywords of the first segment, the segment loop of
the base class on top of it, and the new export's declaration.  Stubbed parts in the style of tests/test_magi_walk_host.py: nothing here
touches a device."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Embedder:
    model_max_length = 6

    def __init__(self, log):
        self.log = log

    def get_text_embeddings(self, prompts):
        self.log.append(("embed", list(prompts)))
        return torch.ones(1, 6, 4), torch.ones(1, 6)


class _Stream:
    """What a segment needs of a `MagiFrameStream`: it records the pushes."""

    def __init__(self, log):
        self.log, self.frames_pushed, self.pushed = log, 0, []

    def push(self, chunk):
        self.log.append(("push", tuple(chunk.shape), float(chunk.flatten()[0])))
        self.pushed.append(chunk.clone())
        self.frames_pushed += 4 * chunk.shape[2]

    def flush(self):
        self.log.append(("flush",))

    def video(self):
        self.log.append(("video",))
        return torch.zeros(1, self.frames_pushed, 2, 2, 3, dtype=torch.uint8)


def _stub_pipeline(monkeypatch, log, frames=(2, 2, 1)):
    """Chunks `[1, 2, f, 1, 1]` whose value at (channel c, frame t of the request's new frames) is 100 (segment) + 10 c + t."""
    import inferix_amd.pipeline.magi as PM
    config = SimpleNamespace(model_config=SimpleNamespace(caption_max_length=6), engine_config=SimpleNamespace(),
                             runtime_config=SimpleNamespace(fps=24, scale_factor=0.5))
    vae, dit = object(), object()
    calls = []

    def encode(pixels, fps, v, scale_factor, parallel_group=None):
        assert v is vae
        log.append(("encode", tuple(pixels.shape), fps, scale_factor))
        return torch.full((1, 2, pixels.shape[0], 1, 1), 9.0)

    def generate(model, prefix_video, caption_embs, emb_masks, **kw):
        assert model is dit and tuple(caption_embs.shape) == (1, 1, 6, 4) and tuple(emb_masks.shape) == (1, 6)
        log.append(("generate", None if prefix_video is None else prefix_video.clone(), sorted(kw)))
        calls.append(1)
        at = 0
        for f in frames:
            t = torch.arange(at, at + f, dtype=torch.float32).reshape(1, 1, f, 1, 1)
            c = torch.arange(2, dtype=torch.float32).reshape(1, 2, 1, 1, 1)
            at += f
            yield 100.0 * len(calls) + 10.0 * c + t

    monkeypatch.setattr(PM, "encode_prefix_video", encode)
    monkeypatch.setattr(PM, "generate_per_chunk", generate)
    return PM.MagiPipeline(config, dit=dit, vae=vae, embedder=_Embedder(log))


def test_the_plain_call_still_raises_upstreams_text(monkeypatch):
    pipe = _stub_pipeline(monkeypatch, [])
    text = ("Streaming generation is not yet implemented for MagiPipeline. "
            "Please use the standard run_text_to_video or run_image_to_video methods.")
    for kw in ({}, {"segment_length": 9}, {"continuous": False}, {"image": torch.zeros(1, 4, 4, 3, dtype=torch.uint8)}):
        with pytest.raises(NotImplementedError) as exc:
            pipe._generate_segment_with_streaming("p", None, None, **kw)
        assert str(exc.value) == text
    with pytest.raises(NotImplementedError, match="not yet implemented for MagiPipeline"):
        pipe.run_streaming_generation(["p"], None, num_segments=1)


def test_overlap_latents_become_the_prefix_and_the_chunks_the_final_latents(monkeypatch):
    log = []
    pipe = _stub_pipeline(monkeypatch, log)
    fs = _Stream(log)
    initial = torch.arange(3 * 2, dtype=torch.float32).reshape(1, 3, 2, 1, 1)            # [1, T_o = 3, C = 2, h, w]
    video, final = pipe._generate_segment_with_streaming("p", initial, None, segment_length=5, continuous=True, frame_stream=fs,
                                                         guidance_scale=3.0, num_samples=1)
    assert video is None, "the caller's stream collects the frames"
    kinds = [e[0] for e in log]
    assert kinds == ["embed", "generate", "push", "push", "push"], "no encode, no flush of a stream that is the caller's"
    prefix = log[1][1]
    assert tuple(prefix.shape) == (1, 2, 3, 1, 1) and prefix.is_contiguous() and log[1][2] == []
    assert torch.equal(prefix, initial.transpose(1, 2)) and prefix[0, 1, 2, 0, 0] == initial[0, 2, 1, 0, 0]
    assert [e[1] for e in log[2:]] == [(1, 2, 2, 1, 1), (1, 2, 2, 1, 1), (1, 2, 1, 1, 1)]
    assert tuple(final.shape) == (1, 5, 2, 1, 1)
    assert torch.equal(final, torch.cat(fs.pushed, dim=2).transpose(1, 2))
    assert final[0, :, 0, 0, 0].tolist() == [100, 101, 102, 103, 104] and final[0, :, 1, 0, 0].tolist() == [110, 111, 112, 113, 114]


def test_prefix_keywords_count_on_the_first_segment_only_and_noise_is_passed_on(monkeypatch):
    log = []
    pipe = _stub_pipeline(monkeypatch, log)
    image = torch.zeros(1, 4, 4, 3, dtype=torch.uint8)
    clip = torch.zeros(5, 4, 4, 3, dtype=torch.uint8)
    pipe._generate_segment_with_streaming("p", None, None, continuous=True, frame_stream=_Stream(log), image=image)
    assert log[0] == ("encode", (1, 4, 4, 3), 24, 0.5) and log[1][0] == "embed" and tuple(log[2][1].shape) == (1, 2, 1, 1, 1)
    log.clear()
    pipe._generate_segment_with_streaming("p", None, None, continuous=True, frame_stream=_Stream(log), prefix_video=clip)
    assert log[0] == ("encode", (5, 4, 4, 3), 24, 0.5) and tuple(log[2][1].shape) == (1, 2, 5, 1, 1)
    log.clear()
    initial = torch.ones(1, 3, 2, 1, 1)
    pipe._generate_segment_with_streaming("p", initial, None, continuous=True, frame_stream=_Stream(log), image=image, prefix_video=clip)
    assert not any(e[0] == "encode" for e in log), "a later segment starts from its overlap latents, not from the pixels"
    assert tuple(log[1][1].shape) == (1, 2, 3, 1, 1) and bool((log[1][1] == 1).all())
    log.clear()
    pipe._generate_segment_with_streaming("p", None, None, continuous=True, frame_stream=_Stream(log), noise=torch.zeros(1, 2, 5, 1, 1))
    assert log[1][1] is None and log[1][2] == ["noise"]


def test_a_segment_without_a_stream_opens_flushes_and_returns_its_own(monkeypatch):
    log = []
    pipe = _stub_pipeline(monkeypatch, log)
    made = []

    def make(stream_callback, keep_video=True, **kw):
        made.append((stream_callback, keep_video))
        return _Stream(log)
    monkeypatch.setattr(pipe, "_make_frame_stream", make)
    cb = lambda frames: None
    video, final = pipe._generate_segment_with_streaming("p", None, cb, continuous=True)
    assert made == [(cb, True)] and [e[0] for e in log][-2:] == ["flush", "video"]
    assert video.dtype == torch.uint8 and tuple(video.shape) == (1, 20, 2, 2, 3) and tuple(final.shape) == (1, 5, 2, 1, 1)
    log.clear()
    video, _ = pipe._generate_segment_with_streaming("p", None, cb, continuous=True, keep_video=False)
    assert video is None and made[-1] == (cb, False) and [e[0] for e in log][-1] == "flush"


def test_make_frame_stream_names_the_reason(monkeypatch):
    pipe = _stub_pipeline(monkeypatch, [])
    with pytest.raises(ValueError, match="continuous=True: continuous streaming needs the HIP decoder: vae must be a HipMagiVAEDecoder"):
        pipe._make_frame_stream(None)


def test_the_segment_loop_of_the_base_class_on_the_streamed_segments(monkeypatch):
    """One stream for the call, prompts cycling, the last `overlap_frames` latent frames of a segment as the next one's prefix, a flush
    at the end and on an exception, `stream.video()` as the result."""
    log = []
    pipe = _stub_pipeline(monkeypatch, log)
    streams = []

    def make(stream_callback, keep_video=True, **kw):
        streams.append(_Stream(log))
        return streams[-1]
    monkeypatch.setattr(pipe, "_make_frame_stream", make)
    video = pipe.run_streaming_generation(["a", "b"], None, num_segments=3, overlap_frames=3, continuous=True)
    assert len(streams) == 1 and tuple(video.shape) == (1, 60, 2, 2, 3)
    assert [e[1] for e in log if e[0] == "embed"] == [["a"], ["b"], ["a"]]
    gens = [e[1] for e in log if e[0] == "generate"]
    assert gens[0] is None
    assert gens[1][0, 0, :, 0, 0].tolist() == [102, 103, 104] and gens[1][0, 1, :, 0, 0].tolist() == [112, 113, 114]
    assert gens[2][0, 0, :, 0, 0].tolist() == [202, 203, 204]
    assert [e[0] for e in log].count("push") == 9 and [e[0] for e in log][-2:] == ["flush", "video"]
    # an exception in a segment: the stream is flushed, the exception surfaces
    log.clear()

    def failing(chunk):
        raise RuntimeError("the consumer failed")
    monkeypatch.setattr(_Stream, "push", lambda self, chunk: failing(chunk))
    with pytest.raises(RuntimeError, match="the consumer failed"):
        pipe.run_streaming_generation(["a"], None, num_segments=2, continuous=True)
    assert [e[0] for e in log][-1] == "flush"


def test_hwc_export_is_declared_bound_and_exported_without_an_abi_bump():
    from inferix_amd import _hip
    hdr = open(os.path.join(ROOT, "include", "inferix_hip.h")).read()
    lib = _hip.load()
    _vp, _i32 = C.c_void_p, C.c_int32
    args = [_vp, _vp, _vp] + [_i32] * 14 + [_vp]
    decl = re.search(r"\bint ifx_vit_tile_blend_hwc\(([^;]*)\);", hdr)
    assert decl and len([a for a in decl.group(1).split(",") if a.strip()]) == len(args)
    assert _hip.SIGNATURES["ifx_vit_tile_blend_hwc"] == (C.c_int, args) and lib.ifx_vit_tile_blend_hwc is not None
    assert (lib.ifx_version() >> 8) & 255 == 7 == _hip.ABI_MINOR and re.search(r"#define IFX_ABI_MINOR 7\b", hdr)
    n = len(_hip.SIGNATURES)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert f"({n} `extern \"C\"` entry points" in doc, "INTEGRATION.md's export count"


def test_hwc_argument_checks_answer_without_a_gpu():
    """The three refusals that are the HWC export's own, on dummy pointers (the GPU suite runs the whole list)."""
    from inferix_amd import _hip
    lib = _hip.load()
    P = C.c_void_p(4096)
    call = lambda out=P, T=9, nt=2, batch=1: lib.ifx_vit_tile_blend_hwc(P, P, out, batch, T, 56, 40, nt, 3, 2, 0, 8, 8, 8, 24, 24, 1, None)
    for kw, part in ((dict(out=None), b"null out_hwc"), (dict(out=C.c_void_p(4100)), b"out_hwc 8-byte aligned"),
                     (dict(T=70000, nt=10000), b"70000 frames"), (dict(batch=65536), b"65536 samples")):
        rc = call(**kw)
        msg = lib.ifx_last_error()
        assert rc == -1 and part in msg, (kw, rc, msg)
