#!/usr/bin/env python3
"""TEST INFRASTRUCTURE — generates the MAGI ViT-VAE decoder fixtures tests/golden/magi_vit_*.npz: the REFERENCE's own `ViTDecoder`
(inferix/models/magi/vae/vae_module.py:569-716) runs on the CPU in bf16 through oracle/_refstub.py, the restatement tests/magi_vit_util.py
is asserted equal to it bit for bit on the output and on every block's token rows, and seeds, input and outputs are written (weights are
regenerated from the seed by `magi_vit_util.make_weights`).

Two third-party calls of `Attention.forward` have no implementation on a CPU and get stand-ins here with the published definition of
flash-attn, softmax(q k^T / sqrt(d)) v without a mask:
  * `flash_attn_qkvpacked_func(qkv)`, which `_refstub.install_magi()` does not provide: q, k, v = qkv.unbind(2);
  * `flash_attn_func(q, k, v)`: `Attention.forward` hands it 5-D tensors `[B, N, 1, heads, hd]` — `qkv.chunk(3, dim=2)` keeps the axis it
    splits — so the stand-in squeezes that singleton axis before the product.
Both go through `magi_vit_util.sdpa`, i.e. torch's scaled_dot_product_attention on the CPU.

The rotary path (`use_rope=True`) of the reference raises on every input, for two reasons that do not depend on the stand-ins: the
sin / cos tables are unsqueezed to `[1, N - 1, 1, cols]` and multiplied with the 5-D `[B, N - 1, 1, heads, hd]` slice of q, which
broadcasts to `[B, N - 1, N - 1, heads, hd]` and cannot be assigned back (:289-291); and `cache_rotary_emb` builds 6 * (hd // 6) columns
(:182-201), 60 for heads of 64 channels.  No fixture can therefore come from it: every case here runs with `use_rope=False`, and the
rotation of ifx_vit_head_prep is tested against the restated operator chain alone (tests/test_hip_vit_kernels.py).

The float32 evaluations (`<name>_fp32.npz`, the floor of the measured-noise rule) come from the restatement with dtype float32: the
reference's forward casts qkv to bf16 on the packed path (:295) whatever the module's dtype, so it has no float32 form to run.

usage (build container only; the reference tree must exist):  python tools/gen_golden_magi_vit.py
"""
from __future__ import annotations

import importlib
import os
import sys
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _refstub  # noqa: E402
import magi_vit_util as U  # noqa: E402

FILE_LIMIT = 1 << 20


def import_reference_vae():
    _refstub.install_magi()
    fa = sys.modules["flash_attn"]

    def flash_attn_func(q, k, v, dropout_p=0.0, **kw):
        assert dropout_p == 0.0
        if q.dim() == 5:
            q, k, v = q.squeeze(2), k.squeeze(2), v.squeeze(2)
        return U.sdpa(q, k, v)

    def flash_attn_qkvpacked_func(qkv, dropout_p=0.0, **kw):
        assert dropout_p == 0.0 and qkv.dtype == torch.bfloat16
        q, k, v = qkv.unbind(2)
        return U.sdpa(q, k, v)

    fa.flash_attn_func = flash_attn_func
    fa.flash_attn_qkvpacked_func = flash_attn_qkvpacked_func
    return importlib.import_module("inferix.models.magi.vae.vae_module")


def build(vm, name: str) -> None:
    cfg, wseed, xseed, batch, latent, store_blocks = U.CASES[name]
    W = U.make_weights(cfg, wseed)
    x = U.make_input(cfg, xseed, batch, latent)
    dec = vm.ViTDecoder(**cfg.ctor_kwargs()).bfloat16().eval()
    missing = dec.load_state_dict(W, strict=True)
    assert not missing.missing_keys and not missing.unexpected_keys
    ref_blocks = {}
    hooks = [blk.register_forward_hook(lambda m, a, out, i=i: ref_blocks.__setitem__(i, out.detach().clone()))
             for i, blk in enumerate(dec.blocks)]
    with torch.no_grad():
        ref = dec(x)
    for h in hooks:
        h.remove()
    taps = {}
    got = U.decoder_forward(W, cfg, x, taps)
    assert got.dtype == torch.bfloat16 and torch.equal(got, ref), f"{name}: the restatement differs from the reference's output"
    for i in range(cfg.depth):
        assert torch.equal(taps[f"block{i}"], ref_blocks[i]), f"{name}: block {i}"
    fx = {"weight_seed": torch.tensor(wseed), "input_seed": torch.tensor(xseed), "latent": torch.tensor(latent), "x": x, "out": ref}
    if store_blocks:
        fx["embed"] = taps["embed"]
        for i in range(cfg.depth):
            fx[f"block{i}"] = ref_blocks[i]
            fx[f"qkv{i}"] = taps[f"qkv{i}"]
            fx[f"attn{i}"] = taps[f"attn{i}"]
        fx["patch_rows"] = taps["patch_rows"]
    path = os.path.join(U.GOLDEN_DIR, name + ".npz")
    U.save_fixture(path, fx)
    assert os.path.getsize(path) <= FILE_LIMIT, (path, os.path.getsize(path))
    print(f"wrote {path} ({os.path.getsize(path)} bytes): out {tuple(ref.shape)}")
    if name in U.FP32_CASES:
        W32 = U.make_weights(cfg, wseed, dtype=torch.float32)
        out32 = U.decoder_forward(W32, cfg, x.float())
        path = os.path.join(U.GOLDEN_DIR, name + "_fp32.npz")
        U.save_fixture(path, {"out": out32})
        assert os.path.getsize(path) <= FILE_LIMIT, (path, os.path.getsize(path))
        rel = float((ref.double() - out32.double()).norm() / out32.double().norm())
        print(f"wrote {path} ({os.path.getsize(path)} bytes): bf16 reference vs float32 rel-L2 {rel:.3e}")


def main():
    if not _refstub.available():
        raise SystemExit("reference tree not available: fixtures can only be generated in the build container")
    warnings.filterwarnings("ignore")
    vm = import_reference_vae()
    for name in U.CASES:
        build(vm, name)


if __name__ == "__main__":
    main()
