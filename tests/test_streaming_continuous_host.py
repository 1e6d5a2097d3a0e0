"""CPU: the segment loops of `AbstractInferencePipeline` with `continuous=True` — one frame stream per call, handed to every segment,
never reset, flushed on the way out (also on STOP and on an exception) — on a stub pipeline and a stub stream: no kernels run."""
import pytest
import torch

from inferix_amd.core import ControlCommand, InteractiveSession, SessionState, calculate_total_frames
from inferix_amd.pipeline import AbstractInferencePipeline


class StubStream:
    def __init__(self, callback, keep):
        self.callback, self.keep, self.blocks, self.log, self.frames_pushed = callback, keep, [], [], 0

    def push(self, block):                     # [B, nf, ...]: 4 nf frames, 3 fewer for the block that opens the stream
        n = 4 * block.shape[1] - (0 if self.blocks else 3)
        self.blocks.append(n)
        self.frames_pushed += n
        self.log.append("push")

    def flush(self):
        self.log.append("flush")
        for n in self.blocks[self.log.count("deliver"):]:
            if self.callback is not None:
                self.callback(n)
            self.log.append("deliver")

    def reset(self):
        self.log.append("reset")

    def video(self):
        return torch.zeros(1, sum(self.blocks), 2, 2, 3, dtype=torch.uint8) if self.keep and self.blocks else None


class StubPipeline(AbstractInferencePipeline):
    def __init__(self, fail_at=None):
        super().__init__({})
        self.calls, self.streams, self.fail_at = [], [], fail_at

    def load_checkpoint(self, checkpoint_path, **kw):
        pass

    def run_text_to_video(self, prompts, **kw):
        pass

    def run_image_to_video(self, prompts, image_path, **kw):
        pass

    def _make_frame_stream(self, stream_callback, keep_video=True, **kw):
        self.streams.append(StubStream(stream_callback, keep_video))
        self.made_with = kw
        return self.streams[-1]

    def _generate_segment_with_streaming(self, prompt, initial_latent, stream_callback, segment_length=21, **kw):
        n_ctx = 0 if initial_latent is None else initial_latent.shape[1]
        self.calls.append(dict(kw, prompt=prompt, n_ctx=n_ctx))
        if self.fail_at == len(self.calls):
            raise RuntimeError("kernel failed")
        lat = torch.zeros(1, segment_length, 2, 2, 2)
        if kw.get("continuous"):
            for b in range(n_ctx, segment_length, 3):          # generated blocks only: the overlap prefill is not pushed
                kw["frame_stream"].push(lat[:, b:b + 3])
            return None, lat
        return torch.zeros(1, segment_length - n_ctx, 2, 2, 3), lat


def test_one_stream_for_the_whole_call():
    p, got = StubPipeline(), []
    out = p.run_streaming_generation(["a", "b"], stream_callback=got.append, num_segments=3, segment_length=6, overlap_frames=3,
                                     continuous=True, num_samples=1)
    assert len(p.streams) == 1 and p.made_with == {"num_samples": 1}
    s = p.streams[0]
    assert all(c["frame_stream"] is s and c["continuous"] is True and c["keep_video"] is True for c in p.calls)
    assert [c["n_ctx"] for c in p.calls] == [0, 3, 3] and [c["prompt"] for c in p.calls] == ["a", "b", "a"]
    assert "reset" not in s.log and s.log[:4] == ["push"] * 4 and s.log[4] == "flush"
    L = calculate_total_frames(3, 6, 3)
    assert got == [9, 12, 12, 12] and out.dtype == torch.uint8 and out.shape[1] == 1 + 4 * (L - 1)
    p2 = StubPipeline()
    assert p2.run_streaming_generation(["a"], num_segments=2, segment_length=6, continuous=True, keep_video=False) is None
    assert p2.streams[0].blocks == [9, 12, 12] and p2.calls[0]["keep_video"] is False


def test_without_the_keyword_nothing_is_added():
    p = StubPipeline()
    out = p.run_streaming_generation(["a"], num_segments=2, segment_length=6, overlap_frames=3, num_samples=1)
    assert not p.streams and all(set(c) == {"num_samples", "prompt", "n_ctx"} for c in p.calls) and out.shape[1] == 9
    p = StubPipeline()
    p.run_streaming_generation(["a"], num_segments=1, segment_length=6, continuous=False)
    assert not p.streams and set(p.calls[0]) == {"continuous", "prompt", "n_ctx"}
    p = StubPipeline()
    out = p.run_interactive_generation(InteractiveSession(), "a", num_segments=2, segment_length=6, overlap_frames=3)
    assert not p.streams and all(set(c) == {"guidance_scale", "prompt", "n_ctx"} for c in p.calls) and out.shape[1] == 9

    class NoStreams(StubPipeline):
        _make_frame_stream = AbstractInferencePipeline._make_frame_stream
    with pytest.raises(NotImplementedError, match="no continuous streaming mode"):
        NoStreams().run_streaming_generation(["a"], continuous=True)


def test_flush_on_exception_and_on_stop():
    p, got = StubPipeline(fail_at=2), []
    with pytest.raises(RuntimeError, match="kernel failed"):
        p.run_streaming_generation(["a"], stream_callback=got.append, num_segments=2, segment_length=6, continuous=True)
    assert got == [9, 12] and p.streams[0].log[-3:] == ["flush", "deliver", "deliver"]

    p, got, session = StubPipeline(), [], InteractiveSession()
    statuses = []
    session.set_status_callback(statuses.append)
    seg = p._generate_segment_with_streaming

    def then_stop(**kw):
        out = seg(**kw)
        session.submit_input(control=ControlCommand.STOP)
        return out
    p._generate_segment_with_streaming = then_stop
    out = p.run_interactive_generation(session, "a", num_segments=3, segment_length=6, overlap_frames=3, stream_callback=got.append,
                                       continuous=True)
    assert len(p.calls) == 1 and got == [9, 12] and out.shape[1] == 21 and len(p.streams) == 1
    assert statuses[-1].frames_generated == 21 and session.state != SessionState.ERROR

    p, session = StubPipeline(fail_at=1), InteractiveSession()
    with pytest.raises(RuntimeError):
        p.run_interactive_generation(session, "a", num_segments=1, segment_length=6, overlap_frames=3, continuous=True)
    assert session.state == SessionState.ERROR and p.streams[0].log == ["flush"]
