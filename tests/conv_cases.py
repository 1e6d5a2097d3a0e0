"""Cases, references and the launch-plan restatement shared by the tests of inferix_amd/csrc/ifx_conv.hip (test_hip_vae.py,
test_hip_conv_edges.py on the GPU; test_conv_cases_oracle.py on the CPU).  No tests here.

  * `ref_conv`: the fp32 torch reference of one ifx_conv3d_cl call (F.conv3d behind F.interpolate / F.pad).
  * `conv_taps`: the same convolution tap by tap with explicit source indices, in fp64 — an evaluation that shares no code with
    `ref_conv`, and the one place where an error can be PLANTED (`MUTATIONS`): the CPU tests show that the bars of the GPU tests
    reject each of them on these very cases.
  * `plan_row`, `plan_tiles`, `plan_grid`, `norm_row`, `norm_blocks`: a Python restatement of `conv_plan` / `norm_plan`
    (csrc/ifx_conv_plan.h), held against CONV_PLAN_RECORDED by the CPU tests.
  * `CONV_CASES` (+ `INPLACE_PERSISTENT`, `overflow_case`, `STRIDED_CASES`), `NORM_CHANNELS`, `norm_geometries`: the case tables, each
    row the smallest shape that reaches one instantiation, tail or layout of the kernels.
  * `build`, `build_norm`: the host operands and the reference of a case, evaluated once per process (`lru_cache`): treat what they
    return as read-only."""
from collections import namedtuple
from functools import lru_cache
from types import SimpleNamespace

import torch
import torch.nn.functional as F

BF = torch.bfloat16
TH, TW, MAXF = 8, 64, 16          # output tile (pixels) and frames per call: ifx_conv_plan.h
SEED = 1234


def ref_conv(frames_cl, w, b, kt, ks, upsample, residual):
    """fp32 torch reference on the CPU: frames_cl [n_in, h, w, cin] (history first), w torch layout, out [t, ho, wo, cout]."""
    x = frames_cl.float().permute(3, 0, 1, 2).unsqueeze(0)                 # [1, c, t, h, w]
    if upsample:
        t = x.shape[2]
        y = F.interpolate(x[0].permute(1, 0, 2, 3), scale_factor=(2.0, 2.0), mode="nearest-exact")
        x = y.permute(1, 0, 2, 3).unsqueeze(0)
    x = F.pad(x, (ks // 2, ks // 2, ks // 2, ks // 2, 0, 0))
    y = F.conv3d(x, w.float(), b.float() if b is not None else None)       # valid in t: n_in - kt + 1 frames
    y = y[0].permute(1, 2, 3, 0).to(BF)
    if residual is not None:
        y = (y.float() + residual.float()).to(BF)
    return y


# ---- the launch plan, restated (csrc/ifx_conv_plan.h: conv_plan, ConvPlan::grid, norm_plan) ----------------------------------------
def channel_tile(cout):
    return 32 if cout <= 32 else 96 if cout % 96 == 0 else 128 if cout % 128 == 0 else 64 if cout <= 64 else 128


def plan_row(kt, ks, ups, cout, variant):
    """The kernel instantiation an ifx_conv3d_cl call launches, as the kernel is named in the library (operands under 2 GiB each)."""
    bn = channel_tile(cout)
    if ks == 3 and bn == 96 and variant != 1 and cout <= 512:
        return f"pp::conv_pp_kernel<{bn}, {ups}>"
    return f"conv_cl_kernel<{bn}, {ups}, {ks}>"


def plan_tiles(ho, wo, cout, t_out):
    """(tiles_w, tiles_h, tiles_n, total) of an output of t_out frames ho x wo x cout."""
    bn = channel_tile(cout)
    tw, th, tn = -(-wo // TW), -(-ho // TH), -(-cout // bn)
    return tw, th, tn, tw * th * tn * t_out


def plan_grid(row, total, cus):
    """Workgroups: the lock-step kernel one per tile rounded up to a multiple of eight (XCDs); the persistent one at most one per CU."""
    per_xcd = -(-total // 8)
    wgx = per_xcd if (not row.startswith("pp::") or per_xcd < cus // 8) else cus // 8
    return max(wgx, 1) * 8


def norm_row(channels):
    """(G, CPL) of ifx_rmsnorm_cl: G lanes share a pixel and hold CPL 16-byte chunks each."""
    chunks = channels // 8
    thirds = chunks % 3 == 0 and (chunks // 3) & (chunks // 3 - 1) == 0
    g, cpl = 1, 3 if thirds else 1
    while g * cpl < chunks:
        g *= 2
    return g, cpl


def norm_pixels_per_block(channels):
    g, cpl = norm_row(channels)
    return (256 // g) * (4 if cpl == 1 else 2)


def norm_blocks(channels, pixels):
    return -(-pixels // norm_pixels_per_block(channels))


# ---- conv cases ----------------------------------------------------------------------------------------------------------------------
# zero: logical input frames named by a negative slot (all-zero history) in both layouts; zero_planar: in the planar run only.
# variants: the conv_variant settings the case runs under (0 alone where the plan does not look at it).
ConvCase = namedtuple("ConvCase", "name kt ks ups cin cout h w t bias res zero zero_planar variants")


def _case(name, kt, ks, ups, cin, cout, h, w, t, bias=True, res=False, zero=(), zero_planar=(), variants=(0,)):
    return ConvCase(name, kt, ks, ups, cin, cout, h, w, t, bias, res, tuple(zero), tuple(zero_planar), tuple(variants))


CONV_CASES = [
    #      name                  kt ks ups cin cout   h    w   t
    _case("cl32x1-cout1",         1, 1, 0, 32,   1,   9,  65,  2),                       # totalG = 1; scalar bias and stores; cout < 4
    _case("cl32x1-cout20-maxf",   3, 1, 0, 64,  20,   3,   5, 14, res=True, zero=(0, 1)),      # 16 input frames; zero frames with 1 x 1 taps; cout % 8 == 4
    _case("cl64x1-cout36",        1, 1, 0, 96,  36,  17, 130,  1, res=True),             # ragged 64 tile; ragged rows and columns
    _case("cl96x1",               3, 1, 0, 32, 192,   9,  70,  2),                       # <96,0,1>
    _case("cl128x1-cout260",      1, 1, 0, 64, 260,   8,  64,  1, bias=False),           # three channel tiles, 4 channels in the last; one pixel tile
    _case("cl32x3-cout2",         1, 3, 0, 32,   2,   8,  64,  2),                       # totalG = 3; cout = 2
    _case("cl32x3-cout12-maxf",   3, 3, 0, 32,  12,   3,   5, 14, zero=(0,)),            # frame smaller than a tile; MAXF
    _case("cl64x3-cout36",        1, 3, 0, 32,  36,   9,  70,  1, res=True),             # totalG = 3 on the two-ahead ring
    _case("cl128x3-cout200",      3, 3, 0, 64, 200,   9,  66,  1, res=True),             # one-ahead ring; ragged 128 tile
    _case("pp96-1x3-maxf",        1, 3, 0, 32,  96,   1,   3, 16, variants=(0, 1)),      # a tile first and last on both axes; MAXF with kt = 1
    _case("pp96-zero-planar",     3, 3, 0, 64,  96,   9,  70,  2, res=True, zero_planar=(0,), variants=(0, 1)),      # zero frame in the planar layout
    _case("ups32-cout3",          1, 3, 1, 32,   3,   5,  33,  2),                       # upsample; odd source sizes; tile edge at an odd source pixel
    _case("ups64-cout40",         1, 3, 1, 64,  40,   5,  33,  1),                       # <64,1,3>
    _case("ups128-4x32",          1, 3, 1, 32, 128,   4,  32,  1),                       # <128,1,3>: exactly one tile
    _case("ups128-5x33",          1, 3, 1, 32, 128,   5,  33,  1),                       # <128,1,3>: ragged
    _case("ppups96-1x2-maxf",     1, 3, 1, 32,  96,   1,   2, 16, variants=(0, 1)),      # smallest upsampled frame
]
CASE = {c.name: c for c in CONV_CASES}

# in place (y = residual): every case above with a residual, and the persistent kernel over several tiles
INPLACE_PERSISTENT = _case("pp96-17x130", 3, 3, 0, 96, 96, 17, 130, 3, res=True)
INPLACE_CASES = [c for c in CONV_CASES if c.res] + [INPLACE_PERSISTENT]

# frame strides with gaps: one lock-step, one persistent, one upsampling and one cout = 20 case
STRIDED_CASES = [CASE["cl128x3-cout200"], CASE["pp96-zero-planar"], CASE["ups64-cout40"], CASE["cl32x1-cout20-maxf"]]


def overflow_case(cus, ups):
    """32 -> 96 channels, 16 output frames 24 pixels high: the narrowest frame (a multiple of 64 plus 6 columns) whose tile count exceeds
    the persistent kernel's grid on `cus` compute units, 8 * (cus // 8), and is no multiple of it — some workgroups run one tile
    more than others.  With `ups` the source frame that upsamples to that output."""
    grid = 8 * (cus // 8)
    w = 6
    while not (3 * -(-w // TW) * 16 > grid and (3 * -(-w // TW) * 16) % grid != 0):
        w += 64
    return overflow_case_of_width(w, ups)


def overflow_case_of_width(w, ups):
    h, ws = (12, w // 2) if ups else (24, w)
    return _case(f"pp96-overflow-24x{w}-ups{ups}", 1, 3, ups, 32, 96, h, ws, 16)


# 3 x 7 x 16 = 336 tiles: on 256 compute units one step wider than the rule above asks for (24 x 326: 288 tiles), so ten workgroups of an
# XCD instead of four take a second tile
OVERFLOW_NAMED_WIDTH = 390


def zero_frames(case, planar):
    return case.zero + (case.zero_planar if planar else ())


def _repack(w):
    from inferix_amd.vae import _repack_conv
    return _repack_conv(w)


def build(case, seed=SEED, planar=False):
    """See `_build`: one evaluation per (case, seed, set of zero frames), so the two layouts share it wherever they name the same frames."""
    return _build(case, seed, zero_frames(case, planar))


@lru_cache(maxsize=None)
def _build(case, seed, zero):
    """Host operands of `case` (the layout only decides which logical frames are zero frames; the planar copy of `buf` is made on the
    device by hip_ops.to_planar):
      raw [n_in, h, w, cin] what was drawn; frames = raw with the zero frames zeroed (the operand of the reference); slots the physical
      slot of every logical frame (shuffled, -1 for a zero frame); buf [n_in + 2, h, w, cin] the slots, NaN wherever no frame lives;
      wt torch layout, wp repacked; b or None; residual or None; out_slots among t + 1; ref = ref_conv(...) [t, ho, wo, cout]."""
    g = torch.Generator().manual_seed(seed * 7919 + case.kt * 1000 + case.ks * 100 + case.cin + case.cout + case.h + case.w + case.t)
    rnd = lambda *shape, scale=1.0: (torch.randn(*shape, generator=g) * scale).to(BF)
    n_in = case.t + case.kt - 1
    ho, wo = (2 * case.h, 2 * case.w) if case.ups else (case.h, case.w)
    o = SimpleNamespace(case=case, n_in=n_in, ho=ho, wo=wo)
    o.raw = rnd(n_in, case.h, case.w, case.cin)
    o.wt = rnd(case.cout, case.cin, case.kt, case.ks, case.ks, scale=(case.cin * case.kt * case.ks * case.ks) ** -0.5)
    o.wp = _repack(o.wt)
    b = rnd(case.cout, scale=0.1)
    o.b = b if case.bias else None
    o.residual = rnd(case.t, ho, wo, case.cout) if case.res else None
    o.zero = zero
    o.frames = o.raw.clone()
    o.slots = torch.randperm(n_in + 2, generator=g)[:n_in].tolist()
    o.buf = torch.full((n_in + 2, case.h, case.w, case.cin), float("nan"), dtype=BF)
    for f, s in enumerate(o.slots):
        if f in o.zero:
            o.frames[f] = 0
            o.slots[f] = -1
        else:
            o.buf[s] = o.raw[f]
    o.out_slots = torch.randperm(case.t + 1, generator=g)[:case.t].tolist()
    o.ref = ref_conv(o.frames, o.wt, o.b, case.kt, case.ks, case.ups, o.residual)
    return o


# ---- the tap-by-tap evaluation and its planted errors ---------------------------------------------------------------------------------
MUTATIONS = ("tap", "halo", "ups_index", "bias_tail", "swap", "zero_frame")


def mutation_applies(mutation, case, planar=False):
    return {"tap": True,
            "halo": case.ks == 3,                                  # a 1 x 1 kernel reads no halo
            "ups_index": case.ups == 1,
            "bias_tail": case.bias and case.cout % 8 != 0,
            "swap": case.t + case.kt - 1 >= 2,
            "zero_frame": len(zero_frames(case, planar)) > 0}[mutation]


def conv_taps(o, dtype=torch.float64, mutation=None):
    """The call of `build` output `o`, one (dt, dh, dw) tap at a time: output pixel (oh, ow) reads the upsampled pixel (oh + dh - ks // 2,
    ow + dw - ks // 2), zero outside the (upsampled) frame, whose source pixel is that coordinate >> 1 under nearest-2x upsampling (the
    kernel's (o + d - 1) >> 1).  Accumulation in `dtype`, then the kernel's roundings: bf16(conv + bias), bf16(. + residual).
    `mutation` plants ONE error:
      tap         the centre tap of the last input frame loses its last 32 input channels
      halo        the column right of the frame replicates the last column instead of reading zero
      ups_index   upsample source index (o + d) >> 1 instead of (o + d - 1) >> 1
      bias_tail   no bias on the last cout % 8 channels
      swap        the last two input frames change places
      zero_frame  the first zero frame reads a frame of data (a stale history slot) instead of zeros"""
    c = o.case
    kt, ks, ups, pad = c.kt, c.ks, c.ups, c.ks // 2
    x = o.frames.to(dtype).clone()
    w = o.wt.to(dtype).clone()
    b = o.b.to(dtype).clone() if o.b is not None else None
    if mutation == "tap":
        w[:, -32:, kt - 1, pad, pad] = 0
    if mutation == "bias_tail":
        b[c.cout - c.cout % 8:] = 0
    if mutation == "swap":
        x[[-1, -2]] = x[[-2, -1]]
    if mutation == "zero_frame":
        x[o.zero[0]] = o.raw[o.zero[0]].to(dtype)

    def source(n_out, n_src, d, replicate_last):
        up = torch.arange(n_out) + d - pad                          # coordinate in the (upsampled) frame
        if mutation == "ups_index" and ups:
            src = (up + 1) >> 1                                     # (o + d) >> 1 with d counted from 0
            ok = (src >= 0) & (src < n_src)
        else:
            ok = (up >= 0) & (up < n_out)
            if replicate_last:
                ok = ok | (up == n_out)
            src = up >> 1 if ups else up
        return src.clamp(0, n_src - 1), ok.to(dtype)

    acc = torch.zeros(c.t, o.ho, o.wo, c.cout, dtype=dtype)
    for dt in range(kt):
        for dh in range(ks):
            rows, rows_ok = source(o.ho, c.h, dh, False)
            for dw in range(ks):
                cols, cols_ok = source(o.wo, c.w, dw, mutation == "halo")
                xs = x[dt:dt + c.t][:, rows][:, :, cols] * rows_ok.view(1, -1, 1, 1) * cols_ok.view(1, 1, -1, 1)
                acc += xs @ w[:, :, dt, dh, dw].t()
    if b is not None:
        acc += b
    y = acc.to(BF)
    if o.residual is not None:
        y = (y.float() + o.residual.float()).to(BF)
    return y


def parity_figures(got, ref, max_ulp, floor):
    """What util.assert_bf16_parity judges, as numbers: (worst element error / its bound, fraction of elements that differ, rel L2)."""
    g, r = got.detach().cpu().double(), ref.detach().cpu().double()
    rms = float(r.pow(2).mean().sqrt())
    tol = max_ulp * 2.0 ** -7 * torch.maximum(r.abs(), torch.tensor(floor * rms, dtype=torch.float64))
    diff = (g - r).abs()
    return float((diff / tol).max()), float((diff > 0).double().mean()), float(diff.norm() / r.norm().clamp_min(1e-30))


def conv_bars(case):
    """The bars of test_conv3d_cl_against_torch: 1 ulp (2 behind the second rounding of a residual) at max(|ref|, tensor RMS)."""
    return dict(max_ulp=2 if case.res else 1, floor=1.0)


# ---- ifx_rmsnorm_cl -------------------------------------------------------------------------------------------------------------------
NORM_CHANNELS = (8, 16, 24, 40, 48, 64, 72, 200, 256, 264, 512)
# (channels, silu) of test_hip_vae.test_rmsnorm_cl: the decoder's own widths, which reach <4,1> and the three-chunk rows the list above leaves out
NORM_DECODER_CASES = [(32, True), (96, True), (128, False), (192, True), (384, True), (384, False)]
NORM_BARS = dict(max_ulp=2, floor=0.05)


def norm_geometries(channels):
    """(frames, pixels per frame, output slots): one pixel; MAXF frames of 5 pixels (a block of pixels straddles several frames) into 18
    slots; two frames of one pixel more than a block takes."""
    return [(1, 1, 3), (MAXF, 5, 18), (2, norm_pixels_per_block(channels) + 1, 4)]


def build_norm(channels, geometry, seed=SEED, zero_pixel=True):
    return _build_norm(channels, geometry, seed, zero_pixel)


@lru_cache(maxsize=None)
def _build_norm(channels, geometry, seed, zero_pixel):
    """x [frames, 1, pixels, channels] with one all-zero pixel (at `zero_at`; none and `zero_at` None without `zero_pixel`), gamma,
    shuffled out_slots, and the oracle's output without and with SiLU.  In the one-pixel geometry the zero pixel is the whole tensor and
    the reference all zeros: a relative bar has nothing to hold on to there, so that geometry is run both ways — the data pixel against
    the bars, the zero pixel for exact zeros."""
    import vae_oracle as V
    frames, pixels, n_slots = norm_geometries(channels)[geometry]
    g = torch.Generator().manual_seed(seed * 31 + channels * 3 + geometry)
    o = SimpleNamespace(frames=frames, pixels=pixels, n_slots=n_slots)
    o.x = (torch.randn(frames, 1, pixels, channels, generator=g) * 3.0).to(BF)
    o.zero_at = (frames - 1, 0, pixels // 2) if zero_pixel else None
    if zero_pixel:
        o.x[o.zero_at] = 0
    o.gamma = (1 + 0.2 * torch.randn(channels, generator=g)).to(BF)
    o.out_slots = torch.randperm(n_slots, generator=g)[:frames].tolist()
    o.ref = V.rms_norm(o.x, o.gamma, channel_dim=-1)
    o.ref_silu = F.silu(o.ref)
    return o
