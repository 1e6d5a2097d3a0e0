#!/usr/bin/env python3
"""TEST INFRASTRUCTURE — generates the MAGI tiled chunk decode fixtures tests/golden/magi_tiles_{a,b,c,d}.npz: the REFERENCE's own
`ViTVAE(ddconfig=TINY ...).tiled_decode_3d` (inferix/models/magi/vae/vae_model.py:179-219 -> `TileProcessor.tiled_decode`,
inferix/distributed/parallelism/tile_parallel.py:348-448) runs on the CPU in bf16, the restatement
tests/magi_tiles_util.py::tiled_decode_restated is asserted equal to it bit for bit, and the arguments, the seeds, the latent shapes
`decode` was called with (in call order, recorded by wrapping the bound `decode`) and the output are written.  Weights come from the seed
(`magi_vit_util.make_weights`).  The raw tile outputs the wrapped `decode` returned go to `<name>_raw.npz` (`tile_<k>` in call order):
torch's bf16 matrix products on a CPU depend on its instruction set, so a test that feeds the blend kernel cannot recompute them
wherever it runs and still expect the reference's bits.

What it takes to run the reference here, on a CPU and in one process:
  * the flash-attn stand-ins of tools/gen_golden_magi_vit.py::import_reference_vae() are installed BEFORE `vae_model` is imported; the
    stubbed `to_2tuple` of the imported `vae_module` is then replaced by a real pair-maker (`ViTVAE` builds the encoder too, and
    `PatchEmbed` subscripts the result);
  * `TileProcessor` formats `torch.distributed.get_rank(...)` into a progress-bar title outside its `is_initialized()` guards: `get_rank`
    is patched to return 0 in this uninitialised process (initialising gloo instead sends `gather_frames` down a path that allocates on
    "cuda");
  * TORCHDYNAMO_DISABLE=1 (set below, before torch is imported): `tiled_decode` wraps its three blend functions in `torch.compile`;
    disabled, they run eagerly, which is what `tiled_encode` does unconditionally and what a CPU executes: three roundings per blend.
    What a compiled blend rounds to on a GPU is not pinned by these fixtures.

usage (build container only; the reference tree must exist):  python tools/gen_golden_magi_tiles.py
"""
from __future__ import annotations

import os

os.environ["TORCHDYNAMO_DISABLE"] = "1"

import importlib  # noqa: E402
import sys  # noqa: E402
import warnings  # noqa: E402

import torch  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import _refstub  # noqa: E402
import magi_tiles_util as TU  # noqa: E402
import magi_vit_util as U  # noqa: E402
from gen_golden_magi_vit import import_reference_vae  # noqa: E402

FILE_LIMIT = 1 << 20


def import_reference_vitvae():
    vae_module = import_reference_vae()
    vae_module.to_2tuple = lambda v: tuple(v) if isinstance(v, (tuple, list)) else (v, v)
    torch.distributed.get_rank = lambda group=None: 0
    return importlib.import_module("inferix.models.magi.vae.vae_model")


def build(vm, name: str) -> None:
    batch, latent, tile_px, fs, ft, xseed, out_shape = TU.CASES[name]
    cfg = U.TINY
    W = U.make_weights(cfg, TU.WEIGHT_SEED)
    vae = vm.ViTVAE(ddconfig=cfg.ctor_kwargs()).bfloat16().eval()
    res = vae.decoder.load_state_dict(W, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    z = TU.case_input(name)
    called, raws = [], []
    bound = vae.decode

    def recording_decode(t):
        called.append(tuple(t.shape))
        raws.append(bound(t))
        return raws[-1]

    vae.decode = recording_decode
    with torch.no_grad():
        ref = vae.tiled_decode_3d(z, **TU.case_kwargs(name))
    ds = (vae.temporal_downsample_factor, vae.spatial_downsample_factor, vae.spatial_downsample_factor)
    got, raw, axes = TU.tiled_decode_restated(TU.tiny_decode(W), z, **TU.case_kwargs(name), ds=ds, return_tiles=True)
    assert len(raw) == len(raws) and all(torch.equal(a, b) for a, b in zip(raw.values(), raws)), f"{name}: raw tiles"
    assert ref.dtype == torch.bfloat16 and tuple(ref.shape) == (batch, 3) + out_shape, (name, ref.shape)
    assert got.dtype == torch.bfloat16 and torch.equal(got, ref), f"{name}: the restatement differs from the reference's output"
    tl, th, tw = tile_px
    fx = {"weight_seed": torch.tensor(TU.WEIGHT_SEED), "input_seed": torch.tensor(xseed), "latent": torch.tensor(latent),
          "batch": torch.tensor(batch), "tile_sample_min": torch.tensor([tl, th, tw]),
          "overlap_factors": torch.tensor([fs, ft], dtype=torch.float64), "decode_shapes": torch.tensor(called), "out": ref}
    path = os.path.join(U.GOLDEN_DIR, name + ".npz")
    U.save_fixture(path, fx)
    assert os.path.getsize(path) <= FILE_LIMIT, (path, os.path.getsize(path))
    print(f"wrote {path} ({os.path.getsize(path)} bytes): {len(called)} tiles -> out {tuple(ref.shape)}")
    path = os.path.join(U.GOLDEN_DIR, name + "_raw.npz")
    U.save_fixture(path, {f"tile_{k}": t.detach().clone() for k, t in enumerate(raws)})
    assert os.path.getsize(path) <= FILE_LIMIT, (path, os.path.getsize(path))
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


def main():
    if not _refstub.available():
        raise SystemExit("reference tree not available: fixtures can only be generated in the build container")
    warnings.filterwarnings("ignore")
    vm = import_reference_vitvae()
    for name in TU.CASES:
        build(vm, name)


if __name__ == "__main__":
    main()
