#!/usr/bin/env python3
"""TEST INFRASTRUCTURE — generates the MAGI ViT-VAE encoder fixtures tests/golden/magi_vitenc_*.npz and the tiled prefix-encode fixtures
tests/golden/magi_enc_tiles_*.npz: the REFERENCE's own `ViTEncoder` (inferix/models/magi/vae/vae_module.py:409-558) and
`ViTVAE.tiled_encode_3d` -> `TileProcessor.tiled_encode` (inferix/distributed/parallelism/tile_parallel.py:254-346) run on the CPU in
bf16 through oracle/_refstub.py, the restatements of tests/magi_vit_encoder_util.py are asserted equal to them bit for bit, and seeds,
inputs and outputs are written (weights are regenerated from the seed by `make_encoder_weights`).

What it takes to run the reference here is what the decoder generators document: the two flash-attn stand-ins of
tools/gen_golden_magi_vit.py, `vae_module.to_2tuple` replaced by a real pair-maker after import (the stub is not subscriptable and
`PatchEmbed` subscripts it) and `torch.distributed.get_rank` patched to return 0 (tools/gen_golden_magi_tiles.py).  `tiled_encode` blends
eagerly (it does not compile its blend functions), three roundings per blend.

The tiles are encoded to the posterior's MODE: the reference's only caller of `tiled_encode_3d` goes through `VaeHelper.get_vae`, which
binds the mode-only `patch_vae_encode` as `vae.encode` (inferix/pipeline/magi/video_process.py:66, 77-110; that module does not import
here, it needs ffmpeg); the same is done here by binding `ViTVAE.encode(..., sample_posterior=False)`.

Every tile fixture also stores the result of the decode-style blend against RAW neighbours, and the generator asserts that it differs from
the reference's: `tiled_encode` blends in place, without the `.clone()` of `tiled_decode`.

The float32 evaluations (`<name>_fp32.npz`, the floor of the measured-noise rule) come from the restatement with dtype float32.

usage (build container only; the reference tree must exist):  python tools/gen_golden_magi_vit_encoder.py
"""
from __future__ import annotations

import os
import sys
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import _refstub  # noqa: E402
import magi_vit_encoder_util as E  # noqa: E402
from gen_golden_magi_tiles import import_reference_vitvae  # noqa: E402

FILE_LIMIT = 1 << 20


def write(name: str, tensors: dict) -> str:
    path = os.path.join(E.GOLDEN_DIR, name + ".npz")
    E.save_fixture(path, tensors)
    assert os.path.getsize(path) <= FILE_LIMIT, (path, os.path.getsize(path))
    return f"wrote {path} ({os.path.getsize(path)} bytes)"


def build_encoder(vmod, name: str) -> None:
    cfg, wseed, inputs, stored = E.CASES[name]
    W = E.make_encoder_weights(cfg, wseed)
    enc = vmod.ViTEncoder(**cfg.ctor_kwargs()).bfloat16().eval()
    res = enc.load_state_dict(W, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    fx = {"weight_seed": torch.tensor(wseed)}
    for n, (xseed, shape) in enumerate(inputs):
        sfx = "" if n == 0 else str(n + 1)
        x = E.make_video(xseed, shape)
        ref_blocks = {}
        hooks = [blk.register_forward_hook(lambda m, a, out, i=i: ref_blocks.__setitem__(i, out.detach().clone()))
                 for i, blk in enumerate(enc.blocks)]
        with torch.no_grad():
            ref = enc(x)
        for h in hooks:
            h.remove()
        taps = {}
        got = E.encoder_forward(W, cfg, x, taps)
        assert got.dtype == torch.bfloat16 and torch.equal(got, ref), f"{name}{sfx}: the restatement differs from the reference's output"
        for i in range(cfg.depth):
            assert torch.equal(taps[f"block{i}"], ref_blocks[i]), f"{name}{sfx}: block {i}"
        assert tuple(ref.shape[2:]) == tuple(s // p for s, p in zip(shape[2:], cfg.patch)), (name, ref.shape)
        fx.update({"input_seed" + sfx: torch.tensor(xseed), "x" + sfx: x, "out" + sfx: ref.contiguous()})
        if stored and n == 0:
            for k in ["patch_rows", "embed", "normed"] + [f"{t}{i}" for i in range(cfg.depth) for t in ("qkv", "attn")]:
                fx[k] = taps[k]
            for i in range(cfg.depth):
                fx[f"block{i}"] = ref_blocks[i]
    print(write(name, fx), "out", tuple(fx["out"].shape))
    if name in E.FP32_CASES:
        W32 = E.make_encoder_weights(cfg, wseed, dtype=torch.float32)
        out32 = E.encoder_forward(W32, cfg, fx["x"].float())
        rel = float((fx["out"].double() - out32.double()).norm() / out32.double().norm())
        print(write(name + "_fp32", {"out": out32}), f"bf16 reference vs float32 rel-L2 {rel:.3e}")


def build_tiles(vm, name: str) -> None:
    shape, tile_px, fs, ft, vseed, grid, out_shape = E.TILE_CASES[name]
    cfg = E.TINY
    W = E.make_encoder_weights(cfg, E.TILE_WEIGHT_SEED)
    vae = vm.ViTVAE(ddconfig=cfg.ctor_kwargs()).bfloat16().eval()
    res = vae.encoder.load_state_dict(W, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    pixels = E.make_pixels(vseed, shape)
    video = E.normalise_pixels(pixels)
    called, raws = [], []
    bound = vae.encode

    def recording_encode(t):
        called.append(tuple(t.shape))
        raws.append(bound(t, sample_posterior=False).detach().clone())      # the clone: the reference blends what it gets back in place
        return raws[-1].clone()

    vae.encode = recording_encode
    with torch.no_grad():
        ref = vae.tiled_encode_3d(video, **E.tile_case_kwargs(name))
    got, raw, axes = E.tiled_encode(E.encode_mode(W, cfg), video, **E.tile_case_kwargs(name), return_tiles=True)
    assert tuple(a.count for a in axes) == grid, (name, [a.count for a in axes])
    assert len(raw) == len(raws) and all(torch.equal(a, b) for a, b in zip(raw.values(), raws)), f"{name}: raw tiles"
    assert ref.dtype == torch.bfloat16 and tuple(ref.shape) == (shape[0], cfg.z_chans) + out_shape, (name, ref.shape)
    assert torch.equal(got, ref), f"{name}: the restatement differs from the reference's output"
    decode_style = E.blend_latent_tiles(raw, axes, in_place=False)
    differ = int((decode_style != ref).sum())
    if axes[0].count * axes[1].count * axes[2].count > 1 and name != "magi_enc_tiles_c":
        assert differ > 0, f"{name}: the in-place chain equals the raw-neighbour blend"
    fx = {"weight_seed": torch.tensor(E.TILE_WEIGHT_SEED), "video_seed": torch.tensor(vseed), "pixels": pixels,
          "tile_sample_min": torch.tensor(tile_px), "overlap_factors": torch.tensor([fs, ft], dtype=torch.float64),
          "encode_shapes": torch.tensor(called), "out": ref.contiguous(), "out_raw_neighbours": decode_style.contiguous()}
    fx.update({f"tile_{k}": t for k, t in enumerate(raws)})
    print(write(name, fx), f"{len(called)} tiles -> out {tuple(ref.shape)}; {differ} elements differ from the raw-neighbour blend")


def main():
    if not _refstub.available():
        raise SystemExit("reference tree not available: fixtures can only be generated in the build container")
    warnings.filterwarnings("ignore")
    vm = import_reference_vitvae()
    vmod = sys.modules["inferix.models.magi.vae.vae_module"]
    for name in E.CASES:
        build_encoder(vmod, name)
    for name in E.TILE_CASES:
        build_tiles(vm, name)


if __name__ == "__main__":
    main()
