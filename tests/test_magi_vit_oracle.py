"""CPU: the MAGI ViT-VAE decoder fixtures and the host side of the three `ifx_vit_*` entry points.  tests/golden/magi_vit_*.npz hold what
the reference's own `ViTDecoder` computed on the CPU in bf16 (tools/gen_golden_magi_vit.py); the first test guards them against the
restatement tests/magi_vit_util.py, the others fail without the kernels, the bindings and the shim package."""
import ctypes as C
import os
import re

import pytest
import torch

import magi_vit_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF = torch.bfloat16


@pytest.mark.parametrize("name", sorted(U.CASES))
def test_restatement_reproduces_the_reference_fixture_bit_for_bit(name):
    cfg, wseed, xseed, batch, latent, stored = U.CASES[name]
    fx = U.load_fixture(name)
    assert int(fx["weight_seed"]) == wseed and int(fx["input_seed"]) == xseed and tuple(fx["latent"].tolist()) == latent
    W = U.make_weights(cfg, wseed)
    x = U.make_input(cfg, xseed, batch, latent)
    assert torch.equal(x, fx["x"])
    taps = {}
    out = U.decoder_forward(W, cfg, x, taps)
    assert out.dtype == BF and torch.equal(out, fx["out"]), name
    if stored:
        keys = ["embed", "patch_rows"] + [f"{t}{i}" for i in range(cfg.depth) for t in ("block", "qkv", "attn")]
        for k in keys:
            assert torch.equal(taps[k], fx[k]), (name, k)
    if name in U.FP32_CASES:
        out32 = U.decoder_forward(U.make_weights(cfg, wseed, dtype=torch.float32), cfg, x.float())
        ref32 = U.load_fixture(name + "_fp32")["out"]
        assert out32.dtype == torch.float32 and torch.equal(out32, ref32), name
        floor = float((out.double() - ref32.double()).norm() / ref32.double().norm())
        assert 1e-3 < floor < 2e-2, floor          # the bf16 evaluation sits a bf16-sized distance from the float32 one, no more


def test_no_vit_fixture_is_above_the_size_limit():
    golden = os.path.join(ROOT, "tests", "golden")
    files = [f for f in os.listdir(golden) if f.startswith("magi_vit_")]
    assert len(files) == len(U.CASES) + len(U.FP32_CASES)
    for f in files:
        assert os.path.getsize(os.path.join(golden, f)) <= 1 << 20, f


def test_vit_exports_are_declared_bound_and_exported_without_an_abi_bump():
    from inferix_amd import _hip
    hdr = open(os.path.join(ROOT, "include", "inferix_hip.h")).read()
    lib = _hip.load()
    _vp, _i32, _f32 = C.c_void_p, C.c_int32, C.c_float
    want = {"ifx_vit_head_prep": [_vp, _i32, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _f32, _vp],
            "ifx_vit_attention": [_vp, _i32, _vp, _i32, _vp, _i32, _vp, _i32, _i32, _i32, _i32, _vp],
            "ifx_vit_unpatch_conv": [_vp, _i32, _i32, _i32, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp]}
    for name, args in want.items():
        decl = re.search(r"\bint " + name + r"\(([^;]*)\);", hdr)
        assert decl, name
        assert len([a for a in decl.group(1).split(",") if a.strip()]) == len(args), name       # the header's parameter count
        assert _hip.SIGNATURES[name] == (C.c_int, args), name
        assert getattr(lib, name) is not None
    assert (lib.ifx_version() >> 8) & 255 == 7 == _hip.ABI_MINOR and re.search(r"#define IFX_ABI_MINOR 7\b", hdr)


def test_vit_argument_validation_without_gpu():
    """Every argument check of the three entry points answers before any launch (dummy aligned pointers, no GPU): code and message."""
    from inferix_amd import _hip
    lib = _hip.load()
    P, P8 = C.c_void_p(4096), C.c_void_p(4104)
    EINVAL = -1

    def refused(rc, *parts):
        msg = lib.ifx_last_error()
        assert rc == EINVAL and all(p in msg for p in parts), (rc, msg)

    # (qkv, ld, sin, cos, batch, tokens, heads, cls_tokens, do_norm, do_rope, eps, stream)
    prep = lambda qkv=P, ld=768, sin=None, cos=None, batch=1, tokens=33, heads=4, cls=1, norm=1, rope=0: \
        lib.ifx_vit_head_prep(qkv, ld, sin, cos, batch, tokens, heads, cls, norm, rope, 1e-5, None)
    refused(prep(qkv=None), b"ifx_vit_head_prep", b"null")
    refused(prep(ld=772), b"ifx_vit_head_prep", b"ld (772)", b"multiple of 8")
    refused(prep(ld=760), b"ifx_vit_head_prep", b"4 heads", b"ld (760)")
    refused(prep(tokens=0), b"ifx_vit_head_prep", b"tokens (0)")
    refused(prep(heads=0), b"ifx_vit_head_prep", b"heads (0)")
    refused(prep(cls=34), b"ifx_vit_head_prep", b"cls_tokens (34)")
    refused(prep(rope=1), b"ifx_vit_head_prep", b"sin and cos")
    refused(prep(rope=1, sin=P, cos=None), b"ifx_vit_head_prep", b"sin and cos")
    refused(prep(qkv=P8), b"ifx_vit_head_prep", b"16-byte")
    assert prep(norm=0, rope=0) == 0                                       # nothing to do: no launch

    # (q, ldq, k, ldk, v, ldv, out, ldo, batch, tokens, heads, stream)
    attn = lambda q=P, ldq=768, k=P, ldk=768, v=P, ldv=768, out=P, ldo=256, batch=1, tokens=33, heads=4: \
        lib.ifx_vit_attention(q, ldq, k, ldk, v, ldv, out, ldo, batch, tokens, heads, None)
    for null in ("q", "k", "v", "out"):
        refused(attn(**{null: None}), b"ifx_vit_attention", b"null")
    for ld in ("ldq", "ldk", "ldv", "ldo"):
        refused(attn(**{ld: 772}), b"ifx_vit_attention", b"772", b"multiples of 8")
        refused(attn(**{ld: 248}), b"ifx_vit_attention", b"4 heads", b"248")
    refused(attn(tokens=0), b"ifx_vit_attention", b"tokens (0)")
    refused(attn(tokens=-5), b"ifx_vit_attention", b"tokens (-5)")
    refused(attn(batch=0), b"ifx_vit_attention", b"batch (0)")
    refused(attn(q=P8), b"ifx_vit_attention", b"16-byte")

    # (x, ldx, tile_rows, cls_tokens, weight, bias, y, batch, t_out, h_out, w_out, patch_t, patch_h, patch_w, channels, stream)
    conv = lambda x=P, ldx=1024, rows=33, cls=1, w=P, b=P, y=P, batch=1, T=8, H=32, W=32, pt=4, ph=8, pw=8, ch=4: \
        lib.ifx_vit_unpatch_conv(x, ldx, rows, cls, w, b, y, batch, T, H, W, pt, ph, pw, ch, None)
    for null in ("x", "w", "b", "y"):
        refused(conv(**{null: None}), b"ifx_vit_unpatch_conv", b"null")
    refused(conv(ch=3), b"ifx_vit_unpatch_conv", b"channels 3", b"4 only")
    refused(conv(ch=16, ldx=4096), b"ifx_vit_unpatch_conv", b"channels 16")
    refused(conv(T=10), b"ifx_vit_unpatch_conv", b"does not divide", b"10 x 32 x 32")
    refused(conv(H=36), b"ifx_vit_unpatch_conv", b"does not divide")
    refused(conv(W=36), b"ifx_vit_unpatch_conv", b"does not divide")
    refused(conv(pt=0), b"ifx_vit_unpatch_conv", b"does not divide")
    refused(conv(ldx=1028), b"ifx_vit_unpatch_conv", b"ldx (1028)", b"multiple of 8")
    refused(conv(ldx=1016), b"ifx_vit_unpatch_conv", b"1024 channels", b"ldx (1016)")
    refused(conv(rows=32), b"ifx_vit_unpatch_conv", b"tile_rows (32)", b"32 patch tokens")
    refused(conv(cls=-1), b"ifx_vit_unpatch_conv", b"cls_tokens (-1)")
    refused(conv(batch=0), b"ifx_vit_unpatch_conv", b"empty output")


def test_decoder_module_shim_paths_and_host_side_refusals():
    """The reference's import paths resolve to the HIP module; construction and its refusals touch no GPU; a CPU tensor raises."""
    from inferix.models.magi.vae import ViTDecoder, ViTVAE
    from inferix.models.magi.vae.vae_model import ViTVAE as V2
    from inferix.models.magi.vae.vae_module import ViTDecoder as D2
    from inferix_amd import _hip
    from inferix_amd import hip_ops as ops
    from inferix_amd.magi.vae import HipMagiVAEDecoder, HipViTDecoder
    assert ViTDecoder is D2 is HipViTDecoder and ViTVAE is V2 is HipMagiVAEDecoder
    cfg = U.TINY
    dec = HipViTDecoder(**cfg.ctor_kwargs(), device="cpu")
    assert set(dec._expected()) == set(U.make_weights(cfg, 1)), "the reference's state-dict keys"
    published = dict(video_size=256, video_length=16, patch_size=8, patch_length=4, embed_dim=1024, depth=24, num_heads=16, ln_in_attn=True,
                     conv_last_layer=True, use_final_proj=True, qkv_bias=True)
    vae = HipMagiVAEDecoder(dict(published, z_chans=16), device="cpu")
    assert vae.spatial_downsample_factor == 8 and vae.temporal_downsample_factor == 4 and len(vae.decoder._expected()) == 24 * 10 + 12
    with pytest.raises(NotImplementedError):
        vae.encode(None)
    with pytest.raises(NotImplementedError, match="use_rope"):
        HipViTDecoder(**dict(published, use_rope=True), device="cpu")
    with pytest.raises(NotImplementedError, match="head size"):
        HipViTDecoder(**dict(published, num_heads=8), device="cpu")
    with pytest.raises(NotImplementedError, match="un-patch"):
        HipViTDecoder(**dict(published, use_final_proj=False, patch_size=4), device="cpu")
    with pytest.raises(AssertionError):
        HipViTDecoder(**dict(published, conv_last_layer=False), device="cpu")
    with pytest.raises(KeyError, match="proj_in.weight"):
        dec.load_state_dict({})
    dec.load_state_dict(U.make_weights(cfg, 1))
    with pytest.raises(_hip.HipKernelError):
        dec(torch.zeros(1, 4, 2, 4, 4, dtype=BF))
    for call in (lambda: ops.vit_head_prep(torch.zeros(33, 768, dtype=BF), batch=1, heads=4, cls_tokens=1, norm=True),
                 lambda: ops.vit_attention(*(torch.zeros(33, 256, dtype=BF),) * 3, batch=1, heads=4),
                 lambda: ops.vit_unpatch_conv(torch.zeros(33, 1024, dtype=BF), torch.zeros(3, 4, 3, 3, 3, dtype=BF), torch.zeros(3, dtype=BF),
                                              batch=1, cls_tokens=1, latent=(2, 4, 4), patch=(4, 8, 8))):
        with pytest.raises(_hip.HipKernelError):
            call()
