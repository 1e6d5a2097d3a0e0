"""Shared by the MAGI ViT-VAE decoder tests and tools/gen_golden_magi_vit.py: the decoder configs of the fixtures, the seeded weight
generator (fixtures hold seeds, inputs and outputs, never weights), and a plain-torch restatement of `ViTDecoder.forward`
(inferix/models/magi/vae/vae_module.py:569-716) that evaluates the reference's op chain on the CPU: bf16 tensors through torch's bf16
operators, so it equals the reference-generated fixtures bit for bit (tests/test_magi_vit_oracle.py); with dtype float32 it is the
exact-arithmetic evaluation the measured-noise rule takes its floor from.  Nothing here imports oracle/ or the reference.

The interleaved rotation is restated (`rotate_interleaved`, for the head-prep kernel's test) as `apply_rot_embed` reads, but the decoder
here refuses `use_rope=True` and no fixture has it: the reference's own rotary path raises on every input (see
tools/gen_golden_magi_vit.py), so there is no result to restate."""
from __future__ import annotations

import dataclasses
import os
from typing import Dict, Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F

BF = torch.bfloat16
GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LN_EPS = 1e-5            # nn.LayerNorm default and ManualLayerNorm's eps


@dataclasses.dataclass(frozen=True)
class VitConfig:
    """The constructor arguments of `ViTDecoder` that reach the forward."""
    video_size: int = 256
    video_length: int = 16
    patch_size: int = 8
    patch_length: int = 4
    z_chans: int = 4
    embed_dim: int = 1024
    depth: int = 24
    num_heads: int = 16
    mlp_ratio: float = 4.0
    qkv_bias: bool = False
    with_cls_token: bool = True
    ln_in_attn: bool = False
    use_rope: bool = False
    use_final_proj: bool = False

    @property
    def latent(self) -> Tuple[int, int, int]:
        return (self.video_length // self.patch_length, self.video_size // self.patch_size, self.video_size // self.patch_size)

    @property
    def head_dim(self) -> int:
        return self.embed_dim // self.num_heads

    @property
    def cls(self) -> int:
        return 1 if self.with_cls_token else 0

    @property
    def patch_volume(self) -> int:
        return self.patch_size * self.patch_size * self.patch_length

    @property
    def unpatch_channels(self) -> int:
        return 4 if self.use_final_proj else self.embed_dim // self.patch_volume

    def ctor_kwargs(self) -> dict:
        return dict(dataclasses.asdict(self), conv_last_layer=True)


# name -> (config, weight seed, input seed, batch, latent shape, stored per-block activations)
TINY = VitConfig(video_size=32, video_length=8, embed_dim=256, depth=2, num_heads=4, ln_in_attn=True, use_final_proj=True)
CASES = {
    # (a) tiny decoder at its trained shape: 2 x 4 x 4 latents + class token = 33 tokens
    "magi_vit_a": (TINY, 4100, 11, 1, (2, 4, 4), True),
    # (b) the same weights at another latent shape: resize_pos_embed, 16 tokens
    "magi_vit_b": (TINY, 4100, 12, 1, (1, 5, 3), True),
    # (c) norm1 path, packed attention call, identity final projection (unpatch_channels = 1024 / 256 = 4), qkv bias
    "magi_vit_c": (VitConfig(video_size=32, video_length=8, embed_dim=1024, depth=1, num_heads=16, qkv_bias=True), 4200, 13, 1, (2, 4, 4),
                   False),
    # (d) one block at the published width: 4 x 8 x 8 latents + class token = 257 tokens
    "magi_vit_d": (VitConfig(video_size=64, video_length=16, embed_dim=1024, depth=1, num_heads=16, ln_in_attn=True, use_final_proj=True,
                             qkv_bias=True), 4300, 14, 1, (4, 8, 8), False),
}
FP32_CASES = ("magi_vit_a", "magi_vit_d")      # (e): the float32 evaluation stored next to the bf16 one


def make_weights(cfg: VitConfig, seed: int, dtype=BF) -> Dict[str, torch.Tensor]:
    """State dict of `ViTDecoder(**cfg.ctor_kwargs())` under the reference's key names, from one seed; values are bf16-representable."""
    g = torch.Generator().manual_seed(seed)
    D, hid = cfg.embed_dim, int(cfg.embed_dim * cfg.mlp_ratio)
    W: Dict[str, torch.Tensor] = {}

    def rnd(*shape, std=1.0, mean=0.0):
        return (torch.randn(*shape, generator=g) * std + mean).to(BF).to(dtype)

    def linear(name, n_out, n_in, bias=True):
        W[name + ".weight"] = rnd(n_out, n_in, std=n_in ** -0.5)
        if bias:
            W[name + ".bias"] = rnd(n_out, std=0.05)

    def norm(name, n):
        W[name + ".weight"] = rnd(n, std=0.1, mean=1.0)
        W[name + ".bias"] = rnd(n, std=0.05)

    linear("proj_in", D, cfg.z_chans)
    if cfg.with_cls_token:
        W["cls_token"] = rnd(1, 1, D, std=0.5)
    lt, lh, lw = cfg.latent
    W["pos_embed"] = rnd(1, lt * lh * lw + cfg.cls, D, std=0.5)
    for i in range(cfg.depth):
        p = f"blocks.{i}."
        if not cfg.ln_in_attn:
            norm(p + "norm1", D)
        linear(p + "attn.qkv", 3 * D, D, bias=cfg.qkv_bias)
        linear(p + "attn.proj", D, D)
        norm(p + "norm2", D)
        linear(p + "mlp.fc1", hid, D)
        linear(p + "mlp.fc2", D, hid)
    norm("norm", D)
    if cfg.use_final_proj:
        linear("final_proj", 4 * cfg.patch_volume, D)
        norm("final_norm", 4 * cfg.patch_volume)
    W["last_layer.weight"] = rnd(3, cfg.unpatch_channels, 3, 3, 3, std=(27 * cfg.unpatch_channels) ** -0.5)
    W["last_layer.bias"] = rnd(3, std=0.05)
    return W


def make_input(cfg: VitConfig, seed: int, batch: int, latent: Tuple[int, int, int], dtype=BF) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    return torch.randn(batch, cfg.z_chans, *latent, generator=g).to(BF).to(dtype)


# ---- host-side tables (once per latent shape) -----------------------------------------------------------------------------------------
def resized_pos_embed(pos_embed: torch.Tensor, cfg: VitConfig, latent: Tuple[int, int, int]) -> torch.Tensor:
    """`pos_embed` `[1, cls + tokens, D]` for `latent`: the trained table, or (:688-696, :400-406) its patch rows as a `[D, lT, lH, lW]`
    volume resampled trilinearly (align_corners off) with the class row kept.  The reference slices row 0 off whatever the class-token
    setting, so a resize without a class token is not a thing it can do."""
    if tuple(latent) == cfg.latent:
        return pos_embed
    assert cfg.with_cls_token, "the reference's resize path drops row 0 of pos_embed: it needs the class token"
    D = pos_embed.shape[-1]
    vol = pos_embed[:, 1:, :].reshape(1, *cfg.latent, D).permute(0, 4, 1, 2, 3)
    vol = F.interpolate(vol, size=tuple(latent), mode="trilinear", align_corners=False)
    rows = vol.permute(0, 2, 3, 4, 1).reshape(1, latent[0] * latent[1] * latent[2], D)
    return torch.cat((pos_embed[:, 0:1, :], rows), dim=1)


# ---- the op chain of Attention.forward :281-292 ---------------------------------------------------------------------------------------
def manual_layernorm(x: torch.Tensor) -> torch.Tensor:
    """`ManualLayerNorm.forward` (:236-242) in x's dtype: every operator's result is a tensor of that dtype."""
    mean = x.mean(dim=-1, keepdim=True)
    std = x.std(dim=-1, keepdim=True, unbiased=False)
    return (x - mean) / (std + LN_EPS)


def rotate_interleaved(x: torch.Tensor, sin: torch.Tensor, cos: torch.Tensor) -> torch.Tensor:
    """`apply_rot_embed` (:142-150): x cos + rot(x) sin, rot(x)[2i] = -x[2i+1], rot(x)[2i+1] = x[2i]; sin / cos broadcast against x."""
    rot = torch.stack((-x[..., 1::2], x[..., ::2]), dim=-1).reshape(x.shape)
    return x * cos + rot * sin


def head_prep_chain(qkv: torch.Tensor, heads: int, cls_tokens: int, norm: bool, sin: Optional[torch.Tensor] = None,
                    cos: Optional[torch.Tensor] = None) -> torch.Tensor:
    """What ifx_vit_head_prep computes, as the reference's operators compute it: qkv `[B, N, 3 * heads * hd]` -> the same shape."""
    B, N, _ = qkv.shape
    t = qkv.reshape(B, N, 3, heads, -1)
    if norm:
        t = manual_layernorm(t)
    t = t.clone()
    if sin is not None:
        s, c = sin[None, :, None, :], cos[None, :, None, :]
        for part in (0, 1):
            t[:, cls_tokens:, part] = rotate_interleaved(t[:, cls_tokens:, part], s, c).to(qkv.dtype)
    return t.reshape(B, N, -1)


def sdpa(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
    """softmax(q k^T / sqrt(hd)) v on `[B, N, heads, hd]` operands: the published definition of flash_attn_func, through torch's CPU
    operator as the fixtures' generator evaluates it."""
    o = F.scaled_dot_product_attention(q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2))
    return o.transpose(1, 2).contiguous()


# ---- the decoder ----------------------------------------------------------------------------------------------------------------------
def embed_tokens(W, cfg: VitConfig, x: torch.Tensor) -> torch.Tensor:
    """:677-699: latents -> token rows + class token + positional embedding."""
    B, C, lt, lh, lw = x.shape
    h = F.linear(x.permute(0, 2, 3, 4, 1).reshape(B, -1, C), W["proj_in.weight"], W["proj_in.bias"])
    if cfg.with_cls_token:
        h = torch.cat((W["cls_token"].expand(B, -1, -1), h), dim=1)
    return h + resized_pos_embed(W["pos_embed"], cfg, (lt, lh, lw))


def block_forward(W, cfg: VitConfig, i: int, h: torch.Tensor, latent: Tuple[int, int, int], taps: Optional[dict] = None) -> torch.Tensor:
    """`Block.forward` (:343-346) with `Attention.forward` (:279-301) and `Mlp.forward` (:217-223)."""
    p = f"blocks.{i}."
    B, N, D = h.shape
    y = h if cfg.ln_in_attn else F.layer_norm(h, (D,), W[p + "norm1.weight"], W[p + "norm1.bias"], LN_EPS)
    qkv = F.linear(y, W[p + "attn.qkv.weight"], W.get(p + "attn.qkv.bias"))
    assert not cfg.use_rope, "the reference's rotary path raises on every input: there is no result to restate"
    qkv = head_prep_chain(qkv, cfg.num_heads, cfg.cls, cfg.ln_in_attn)
    if taps is not None:
        taps[f"qkv{i}"] = qkv
    q, k, v = qkv.reshape(B, N, 3, cfg.num_heads, cfg.head_dim).unbind(2)
    o = sdpa(q, k, v).reshape(B, N, D)
    if taps is not None:
        taps[f"attn{i}"] = o
    h = h + F.linear(o, W[p + "attn.proj.weight"], W[p + "attn.proj.bias"])
    y = F.layer_norm(h, (D,), W[p + "norm2.weight"], W[p + "norm2.bias"], LN_EPS)
    y = F.gelu(F.linear(y, W[p + "mlp.fc1.weight"], W[p + "mlp.fc1.bias"]))
    return h + F.linear(y, W[p + "mlp.fc2.weight"], W[p + "mlp.fc2.bias"])


def unpatch_volume(rows: torch.Tensor, cfg: VitConfig, latent: Tuple[int, int, int]) -> torch.Tensor:
    """:712-713: `[B, lT lH lW, pT pH pW C]` -> `[B, C, lT pT, lH pH, lW pW]`."""
    B = rows.shape[0]
    lt, lh, lw = latent
    pt, ps, c = cfg.patch_length, cfg.patch_size, cfg.unpatch_channels
    t = rows.reshape(B, lt, lh, lw, pt, ps, ps, c).permute(0, 7, 1, 4, 2, 5, 3, 6)
    return t.reshape(B, c, lt * pt, lh * ps, lw * ps)


def head_forward(W, cfg: VitConfig, h: torch.Tensor, latent: Tuple[int, int, int], taps: Optional[dict] = None) -> torch.Tensor:
    """:704-715: final norm, class token dropped, final projection + norm, un-patching, last-layer convolution."""
    h = F.layer_norm(h, (cfg.embed_dim,), W["norm.weight"], W["norm.bias"], LN_EPS)
    if cfg.with_cls_token:
        h = h[:, 1:]
    if cfg.use_final_proj:
        h = F.linear(h, W["final_proj.weight"], W["final_proj.bias"])
        h = F.layer_norm(h, (h.shape[-1],), W["final_norm.weight"], W["final_norm.bias"], LN_EPS)
    if taps is not None:
        taps["patch_rows"] = h
    return F.conv3d(unpatch_volume(h, cfg, latent), W["last_layer.weight"], W["last_layer.bias"], stride=1, padding=1)


def decoder_forward(W, cfg: VitConfig, x: torch.Tensor, taps: Optional[dict] = None) -> torch.Tensor:
    """`ViTDecoder.forward`: x `[B, z_chans, lT, lH, lW]` -> `[B, 3, lT pT, lH pH, lW pW]`; `taps` collects the token rows after the
    embedding (`embed`) and after every block (`block{i}`), the head-prep and attention outputs and the rows the convolution reads."""
    latent = tuple(x.shape[2:])
    h = embed_tokens(W, cfg, x)
    if taps is not None:
        taps["embed"] = h
    for i in range(cfg.depth):
        h = block_forward(W, cfg, i, h, latent, taps)
        if taps is not None:
            taps[f"block{i}"] = h
    return head_forward(W, cfg, h, latent, taps)


# ---- fixture I/O (bf16 as uint16 bit patterns under `<name>::bf16`, the convention of every fixture here) ---------------------------------
def save_fixture(path: str, tensors: Dict[str, torch.Tensor]) -> None:
    out = {}
    for k, v in tensors.items():
        v = v.detach().cpu().contiguous()
        out[k + "::bf16" if v.dtype == BF else k] = v.view(torch.int16).numpy().view(np.uint16) if v.dtype == BF else v.numpy()
    np.savez_compressed(path, **out)


def load_fixture(name: str) -> Dict[str, torch.Tensor]:
    out = {}
    with np.load(os.path.join(GOLDEN_DIR, name + ".npz"), allow_pickle=False) as z:
        for k in z.files:
            a = z[k]
            out[k[:-6] if k.endswith("::bf16") else k] = (torch.from_numpy(a.view(np.int16).copy()).view(BF) if k.endswith("::bf16")
                                                         else torch.from_numpy(a.copy()))
    return out
