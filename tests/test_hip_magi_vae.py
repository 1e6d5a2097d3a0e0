"""GPU: `HipViTDecoder` / `HipMagiVAEDecoder` (inferix_amd/magi/vae.py) against the reference-generated fixtures
tests/golden/magi_vit_*.npz: teacher-forced per stage where the fixture stores the activations, then end to end under the measured-noise
rule of the Wan decoder — the float32 evaluation is the exact answer, the reference's own bf16 result sits `floor` (rel-L2) from it, the
HIP result must be within 1.25 x floor of the exact answer and within 2 x floor of the reference's.  Fixtures and seeds only."""
import functools

import pytest
import torch

import magi_vit_util as U
from util import assert_bf16_parity, rel_l2

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


@functools.lru_cache(maxsize=None)
def _case(name):
    from inferix_amd.magi.vae import HipViTDecoder
    cfg, wseed, xseed, batch, latent, stored = U.CASES[name]
    W = U.make_weights(cfg, wseed)
    dec = HipViTDecoder(**cfg.ctor_kwargs(), device="cuda:0")
    dec.load_state_dict(W)
    return cfg, W, dec, U.load_fixture(name)


@functools.lru_cache(maxsize=None)
def _floor(name):
    """(float32 evaluation, rel-L2 of the reference's bf16 output from it).  Stored for (a) and (d); for the other cases the same
    restatement evaluates it here, once."""
    cfg, wseed, xseed, batch, latent, stored = U.CASES[name]
    fx = U.load_fixture(name)
    if name in U.FP32_CASES:
        exact = U.load_fixture(name + "_fp32")["out"]
    else:
        exact = U.decoder_forward(U.make_weights(cfg, wseed, dtype=torch.float32), cfg, fx["x"].float())
    return exact, rel_l2(fx["out"], exact)


# The bar of a decoder stage fed the reference's own input (the rule tests/test_hip_vae.py applies to the Wan decoder's stages): every element
# within 2 bf16 ULP at max(|ref|, tensor RMS), rel-L2 <= 3e-3, at most 0.2 of the elements differing at all — 0.4 behind an attention,
# whose probabilities are rounded at another point than in the reference's operator.
STAGE = dict(max_ulp=2, floor=1.0, rel=3e-3, max_mismatch_frac=0.2)


@pytest.mark.parametrize("name", ["magi_vit_a", "magi_vit_b"])
def test_decoder_stages_teacher_forced(name):
    """Every stage fed the reference's own input to it: embedding; per block the qkv projection + head prep, the attention, the rest of
    the block; the head."""
    cfg, W, dec, fx = _case(name)
    B, N, D = fx["embed"].shape
    latent = tuple(fx["latent"].tolist())
    rows = lambda t: t.cuda().reshape(B * N, -1)
    assert_bf16_parity(dec.embed(fx["x"].cuda()), fx["embed"], max_ulp=1, floor=1.0, what=f"{name} embed")
    h = fx["embed"]
    for i in range(cfg.depth):
        qkv, attn, out = fx[f"qkv{i}"], fx[f"attn{i}"], fx[f"block{i}"]
        assert_bf16_parity(dec.attn_inputs(i, rows(h), B).view(B, N, 3 * D), qkv, **STAGE, what=f"{name} block {i} qkv + head prep", report=True)
        assert_bf16_parity(dec.attention(rows(qkv), B).view(B, N, D), attn, **dict(STAGE, max_mismatch_frac=0.4),
                           what=f"{name} block {i} attention", report=True)
        assert_bf16_parity(dec.block_tail(i, rows(h), rows(attn)).view(B, N, D), out, **STAGE, what=f"{name} block {i} tail", report=True)
        h = out
    assert_bf16_parity(dec.head(rows(h), B, latent), fx["out"], **STAGE, what=f"{name} head", report=True)


@pytest.mark.parametrize("name", sorted(U.CASES))
def test_decoder_end_to_end_measured_noise(name):
    cfg, W, dec, fx = _case(name)
    exact, floor = _floor(name)
    out = dec(fx["x"].cuda()).cpu()
    assert out.shape == fx["out"].shape and out.dtype == BF and torch.isfinite(out.float()).all()
    err_exact, err_ref = rel_l2(out, exact), rel_l2(out, fx["out"])
    line = f"{name}: bf16 floor {floor:.3e}, HIP vs float32 {err_exact:.3e} (bound {1.25 * floor:.3e}), HIP vs reference {err_ref:.3e} (bound {2 * floor:.3e})"
    print(line)
    assert err_exact <= 1.25 * floor and err_ref <= 2.0 * floor, line


def test_decode_single_frame_state_dict_and_cpu_tensor():
    from inferix_amd import _hip
    from inferix_amd.magi.vae import HipMagiVAEDecoder
    cfg, W, dec, fx = _case("magi_vit_b")                       # latent (1, 5, 3): T == 1
    vae = HipMagiVAEDecoder(cfg.ctor_kwargs(), device="cuda:0")
    vae.load_state_dict({"decoder." + k: v for k, v in W.items()} | {"encoder.proj_in.weight": torch.zeros(1)})
    sd = vae.state_dict()
    assert set(sd) == {"decoder." + k for k in W} and all(torch.equal(sd["decoder." + k].cpu(), W[k]) for k in W), "state-dict round trip"
    x = fx["x"].cuda()
    full = dec(x)
    one = vae.decode(x)
    assert one.shape == (1, 3, 1, 40, 24) and torch.equal(one, full[:, :, :1])
    xa = _case("magi_vit_a")[3]["x"].cuda()
    vae_a = HipMagiVAEDecoder(cfg.ctor_kwargs(), device="cuda:0")
    vae_a.decoder = _case("magi_vit_a")[2]
    assert vae_a.decode(xa).shape == (1, 3, 8, 32, 32)          # T > 1: every frame
    with pytest.raises(_hip.HipKernelError):
        dec(fx["x"])


def test_decoder_is_deterministic_and_batch_invariant():
    cfg, W, dec, fx = _case("magi_vit_a")
    x0 = fx["x"].cuda()
    x1 = U.make_input(cfg, 77, 1, (2, 4, 4)).cuda()
    a, b = dec(x0), dec(x0)
    assert torch.equal(a, b), "two calls differ"
    both = dec(torch.cat((x0, x1)))
    assert torch.equal(both[0:1], a) and torch.equal(both[1:2], dec(x1)), "batch 2 differs from two batch-1 calls"
