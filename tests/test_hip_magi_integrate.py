"""GPU: `ifx_magi_integrate` (guidance mix + Euler step of one MAGI denoising step in one launch) against the torch operator sequence of
`forward_dispatcher` / `_dispatch_3cfg` followed by `integrate`, bit for bit (`torch.equal`)."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu
NAN_BITS = 0x7FC01234


def _rand(*shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).cuda()


def _f32(v):
    return torch.tensor(v, dtype=torch.float32).cuda()


def _reference(x, chunk_start, cw, dt, sources):
    """One separately rounded torch operator per product and per sum, per chunk; both rows of x take row 0's result."""
    x = x.clone()
    for c in range(len(dt)):
        m = None
        for v, first, c0, c1, w in sources:
            if not c0 <= c <= c1:
                continue
            v = v[0] if v.dim() == 5 else v
            first = first + v.shape[1] if first < 0 else first
            f = first + (c - c0) * cw
            term = _f32(w[c]) * v[:, f:f + cw]
            m = term if m is None else m + term
        a = (chunk_start + c) * cw
        x[:, :, a:a + cw] = x[0:1, :, a:a + cw] + m * _f32(dt[c])
    return x


def _f32_list(n, seed, lo=0.01, hi=0.2):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(n, generator=g) * (hi - lo) + lo).tolist()              # fp32 values as Python floats


@pytest.mark.parametrize("first_frame", [1, 0])
def test_one_chunk_odd_span_misaligned_start(first_frame):
    """C = 3, one frame of 5 x 7 per chunk: a 35-float span that starts 12 bytes past a 16-byte boundary.  With the source at the same
    frame the body goes 16 bytes at a time behind a one-element head; with the source one frame off nothing lines up and the span goes
    4 bytes at a time."""
    from inferix_amd import hip_ops as ops
    x = _rand(1, 3, 3, 5, 7, seed=1)
    noise = x.clone()
    v = _rand(3, 2, 5, 7, seed=2)
    dt = _f32_list(1, 3)
    src = [(v, first_frame, 0, 0, [1.0])]
    want = _reference(x, 1, 1, dt, src)
    assert torch.equal(want[:, :, 1], noise[:, :, 1] + v[None, :, first_frame] * _f32(dt[0]))       # a lone source at weight 1: m = v
    ops.magi_integrate(x, 1, 1, dt, src)
    assert torch.equal(x, want) and not torch.equal(x[:, :, 1], noise[:, :, 1])
    assert torch.equal(x[:, :, 0], noise[:, :, 0]) and torch.equal(x[:, :, 2], noise[:, :, 2])


def test_four_chunks_three_sources_with_their_own_first_frames():
    """`cfg_number == 3` as `_dispatch_3cfg` writes it: `(1 - sp) * uncond + (sp - st) * pre[-dw:] + st * text[-dw:]` per chunk with the
    scales looked up per chunk, then `integrate`.  x is a channel window of a wider tensor (its own channel stride), two rows."""
    from inferix_amd import hip_ops as ops
    from inferix_amd.magi import schedule as S
    Cn, cw, H, W, n = 16, 2, 8, 12, 4
    big = _rand(2, Cn + 5, 5 * cw, H, W, seed=10)
    big[1] = big[0]
    x = big[:, 2:2 + Cn]
    dw = n * cw
    uncond, pre, text = _rand(1, Cn, dw, H, W, seed=11), _rand(1, Cn, dw + cw, H, W, seed=12), _rand(1, Cn, dw + 2 * cw, H, W, seed=13)
    prev, txt, t_range = [1.5, 1.1, 1.0], [7.5, 3.3, 0.0], [0.0, 0.3, 0.7]
    bins = [2, 1, 0, 0]
    dt = _f32_list(n, 14)
    # the reference's own expression
    ps, ts = _f32(prev), _f32(txt)
    pieces = []
    for ci in range(n):
        idx = torch.tensor(bins[ci]).cuda()
        sp, st = ps[idx], ts[idx]
        sl = slice(ci * cw, (ci + 1) * cw)
        pieces.append((1 - sp) * uncond[:, :, sl] + (sp - st) * pre[:, :, -dw:][:, :, sl] + st * text[:, :, -dw:][:, :, sl])
    vel = torch.cat(pieces, dim=2)
    vel = torch.cat([vel, vel], 0)
    xc = x[:, :, cw:cw + dw].clone()
    want = x.clone()
    want[:, :, cw:cw + dw] = (xc.reshape(2, Cn, -1, cw, H, W) + vel.reshape(2, Cn, -1, cw, H, W) * _f32(dt).reshape(1, 1, -1, 1, 1, 1)).reshape(2, Cn, dw, H, W)
    untouched = big.clone()
    w = S.cfg_weights(bins, prev, txt)
    ops.magi_integrate(x, 1, cw, dt, [(uncond, 0, 0, n - 1, w[0]), (pre, -dw, 0, n - 1, w[1]), (text, -dw, 0, n - 1, w[2])])
    assert torch.equal(x, want) and torch.equal(x[0], x[1])
    assert torch.equal(big[:, :2], untouched[:, :2]) and torch.equal(big[:, 2 + Cn:], untouched[:, 2 + Cn:])       # channels outside the view
    assert torch.equal(big[:, :, :cw], untouched[:, :, :cw])


def test_five_chunks_two_rows_partial_second_source():
    """C = 4, chunks of 6 x 3 x 3 = 54 floats (every other span 8 bytes off a 16-byte boundary), rows = 2: both rows come back equal and
    hold row 0's result; a second source covers window chunks 1 .. 3 only."""
    from inferix_amd import hip_ops as ops
    Cn, cw, H, W, n = 4, 6, 3, 3, 5
    x = _rand(1, Cn, 6 * cw, H, W, seed=20).repeat(2, 1, 1, 1, 1)
    v0, v1 = _rand(Cn, n * cw, H, W, seed=21), _rand(1, Cn, 4 * cw, H, W, seed=22)
    dt, w0, w1 = _f32_list(n, 23), _f32_list(n, 24, 0.5, 2.0), _f32_list(n, 25, -1.0, 1.0)
    src = [(v0, 0, 0, n - 1, w0), (v1, cw, 1, 3, w1)]
    want = _reference(x, 1, cw, dt, src)
    ops.magi_integrate(x, 1, cw, dt, src)
    assert torch.equal(x, want) and torch.equal(x[0], x[1])


def test_config5_latent_four_chunks():
    """16 x 24 x 90 x 90, a window of four chunks of six frames: the size the kernel runs at in BASELINE config 5, three sources."""
    from inferix_amd import hip_ops as ops
    Cn, cw, H, W, n = 16, 6, 90, 90, 4
    x = _rand(1, Cn, n * cw, H, W, seed=30).repeat(2, 1, 1, 1, 1)
    a, b, c = _rand(1, Cn, n * cw, H, W, seed=31), _rand(1, Cn, (n + 1) * cw, H, W, seed=32), _rand(1, Cn, (n + 1) * cw, H, W, seed=33)
    dt = _f32_list(n, 34)
    src = [(a, 0, 0, n - 1, _f32_list(n, 35, -0.5, 0.0)), (b, -n * cw, 0, n - 1, _f32_list(n, 36, -6.5, -2.0)),
           (c, -n * cw, 0, n - 1, _f32_list(n, 37, 3.0, 7.5))]
    want = _reference(x, 0, cw, dt, src)
    ops.magi_integrate(x, 0, cw, dt, src)
    assert torch.equal(x, want) and torch.equal(x[0], x[1])


@pytest.mark.parametrize("extra", [False, True])
def test_nearly_clean_layout_one_tensor_as_two_sources(extra):
    """The widened forward of `forward_dispatcher`: the first denoising chunk blended with its re-forwarded copy at frame `width`,
    `out * scale + out2 * (1 - scale)` with a Python float scale, the other chunks plain; with and without the clean chunk in front."""
    from inferix_amd import hip_ops as ops
    from inferix_amd.magi import schedule as S
    Cn, cw, H, W, n, scale = 5, 2, 5, 6, 3, 0.7
    s0 = 1 if extra else 0
    width = (n + s0) * cw
    x = _rand(1, Cn, 5 * cw, H, W, seed=40).repeat(2, 1, 1, 1, 1)
    out = _rand(1, Cn, width + cw, H, W, seed=41)
    dt = _f32_list(n, 42)
    o = out.clone()
    o[:, :, s0 * cw:(s0 + 1) * cw] = o[:, :, s0 * cw:(s0 + 1) * cw] * scale + o[:, :, width:] * (1 - scale)
    vel = o[:, :, :width][:, :, -n * cw:]
    want = x.clone()
    xc = x[:, :, 2 * cw:(2 + n) * cw]
    want[:, :, 2 * cw:(2 + n) * cw] = (xc.reshape(2, Cn, -1, cw, H, W) + vel.reshape(1, Cn, -1, cw, H, W) * _f32(dt).reshape(1, 1, -1, 1, 1, 1)).reshape(2, Cn, n * cw, H, W)
    a, b = S.nearly_clean_weights(scale)
    ops.magi_integrate(x, 2, cw, dt, [(out, s0 * cw, 0, n - 1, [a] + [1.0] * (n - 1)), (out, width, 0, 0, [b] + [0.0] * (n - 1))])
    assert torch.equal(x, want)


def test_window_inside_a_longer_clip_leaves_its_neighbours_bitwise_unchanged():
    from inferix_amd import hip_ops as ops
    Cn, cw, H, W, n = 3, 3, 5, 5, 2
    x = _rand(2, Cn, 6 * cw, H, W, seed=50)
    x[1] = x[0]
    bits = x.view(torch.int32)
    bits[:, :, :2 * cw] = NAN_BITS
    bits[:, :, (2 + n) * cw:] = NAN_BITS + 1
    before = bits.clone()
    v = _rand(Cn, n * cw, H, W, seed=51)
    dt = _f32_list(n, 52)
    want = _reference(x, 2, cw, dt, [(v, 0, 0, n - 1, [1.0] * n)])
    ops.magi_integrate(x, 2, cw, dt, [(v, 0, 0, n - 1, [1.0] * n)])
    after = x.view(torch.int32)
    assert torch.equal(after[:, :, :2 * cw], before[:, :, :2 * cw]) and torch.equal(after[:, :, (2 + n) * cw:], before[:, :, (2 + n) * cw:])
    assert torch.equal(x[:, :, 2 * cw:(2 + n) * cw], want[:, :, 2 * cw:(2 + n) * cw])
    assert torch.isfinite(x[:, :, 2 * cw:(2 + n) * cw]).all()


def test_refusals():
    from inferix_amd import _hip
    from inferix_amd import hip_ops as ops
    x = _rand(1, 2, 10, 2, 2, seed=60)
    keep = x.clone()
    v = _rand(2, 10, 2, 2, seed=61)
    # nine chunks: the library's error code, and the wrapper's exception
    d = _hip.MagiIntegrateDesc()
    d.x, d.row_stride, d.chan_stride, d.rows, d.channels, d.frames, d.frame_elems = x.data_ptr(), x.stride(0), x.stride(1), 1, 2, 10, 4
    d.chunk_width, d.chunk_start, d.n_chunks, d.n_src = 1, 0, 9, 1
    d.src[0].v, d.src[0].chan_stride, d.src[0].frames, d.src[0].last_chunk = v.data_ptr(), v.stride(0), 10, 8
    assert _hip.load().ifx_magi_integrate(C.byref(d), None) == -1
    with pytest.raises(ValueError, match="9 chunks"):
        ops.magi_integrate(x, 0, 1, [0.1] * 9, [(v, 0, 0, 8, [1.0] * 9)])
    with pytest.raises(TypeError, match="bfloat16"):
        ops.magi_integrate(x.bfloat16(), 0, 1, [0.1], [(v, 0, 0, 0, [1.0])])
    with pytest.raises(TypeError, match="bfloat16"):
        ops.magi_integrate(x, 0, 1, [0.1], [(v.bfloat16(), 0, 0, 0, [1.0])])
    with pytest.raises(_hip.HipKernelError, match="GPU only"):
        ops.magi_integrate(x, 0, 1, [0.1], [(v.cpu(), 0, 0, 0, [1.0])])
    with pytest.raises(ValueError, match="contiguous"):
        ops.magi_integrate(_rand(1, 2, 10, 2, 4, seed=62)[..., ::2], 0, 1, [0.1], [(v, 0, 0, 0, [1.0])])
    with pytest.raises(_hip.HipKernelError, match="run past"):
        ops.magi_integrate(x, 9, 1, [0.1, 0.1], [(v, 0, 0, 1, [1.0, 1.0])])
    with pytest.raises(_hip.HipKernelError, match="run past its"):
        ops.magi_integrate(x, 0, 1, [0.1, 0.1], [(v, 9, 0, 1, [1.0, 1.0])])
    torch.cuda.synchronize()
    assert torch.equal(x, keep)
