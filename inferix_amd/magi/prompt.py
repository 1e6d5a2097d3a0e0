"""MAGI-1 caption packing: from `(caption_embs, emb_masks)` of the T5 embedder to the `y [2, chunk_num, L, C]` / `emb_masks
[2, chunk_num, L]` that `ChunkSchedule.run` takes.  Host tensor work, device-agnostic: it only moves fp32 data.

Mirrors inferix/pipeline/magi/prompt_process.py:31-129, 184-212 (special tokens, the env switches, `pad_special_token`,
`get_txt_embeddings` for one process) and inferix/pipeline/magi/video_generate.py:36-138 (`InferenceInput`, the caption rows of the
denoised chunks, the null caption in front for the clean chunks of a prefix video, the null-caption half with its 50-entry mask, the
all-null branch of an empty prompt, the latent size).  The special-token file is read on first use, not at import; tensors stay on the
device of the embeddings they are joined to.
"""
from __future__ import annotations

import math
import os
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple, Union

import numpy as np
import torch

DEFAULT_SPECIAL_TOKEN_PATH = "example/magi/assets/special_tokens.npz"
CAPTION_ROWS = 800           # rows kept after tokens are prepended (prompt_process.py:101-103; = caption_max_length of every shipped config)
NULL_TOKEN_LENGTH = 50       # mask entries set for the null caption (video_generate.py:77-79)
_TRUE = {"1", "true", "yes", "y", "on", "enabled"}

_OTHER = {"TRANS_TOKEN": 0, "HQ_TOKEN": 1, "STATIC_FIRST_FRAMES_TOKEN": 2, "DYNAMIC_FIRST_FRAMES_TOKEN": 3, "BORDERNESS_TOKEN": 4,
          "THREE_D_MODEL_TOKEN": 15, "TWO_D_ANIME_TOKEN": 16}
_tokens_cache: Dict[str, Dict[str, torch.Tensor]] = {}


def env_is_true(name: str) -> bool:
    return str(os.environ.get(name, "0")).lower() in _TRUE


def load_special_tokens(path: Optional[str] = None) -> Dict[str, torch.Tensor]:
    """The dictionary of prompt_process.py:33-58 from the npz keys `caption_token`, `logo_token`, `other_tokens`: every token `[1, C]`,
    cast through fp16 as upstream does; `DURATION_TOKEN_n` (n chunks remain, n = 1 .. 8) = other_tokens[6 + n].  `path` defaults to
    $SPECIAL_TOKEN_PATH, then to upstream's relative default.  Read once per path."""
    path = path or os.getenv("SPECIAL_TOKEN_PATH", DEFAULT_SPECIAL_TOKEN_PATH)
    key = os.path.abspath(path)
    if key not in _tokens_cache:
        if not os.path.exists(path):
            raise FileNotFoundError(f"special-token file {path} not found: pass its path or set SPECIAL_TOKEN_PATH (INTEGRATION.md)")
        with np.load(path, allow_pickle=False) as z:
            f16 = lambda a: torch.tensor(a.astype(np.float16))
            other = z["other_tokens"]
            d = {"CAPTION_TOKEN": f16(z["caption_token"]), "LOGO_TOKEN": f16(z["logo_token"])}
            for name, i in _OTHER.items():
                d[name] = f16(other[i:i + 1])
            for n in range(1, 9):
                d[f"DURATION_TOKEN_{n}"] = f16(other[6 + n:7 + n])
        _tokens_cache[key] = d
    return _tokens_cache[key]


def get_special_token_keys() -> List[str]:
    keys = [tok for env, tok in (("PAD_STATIC", "STATIC_FIRST_FRAMES_TOKEN"), ("PAD_DYNAMIC", "DYNAMIC_FIRST_FRAMES_TOKEN"),
                                 ("PAD_BORDERNESS", "BORDERNESS_TOKEN"), ("PAD_HQ", "HQ_TOKEN"),
                                 ("PAD_THREE_D_MODEL", "THREE_D_MODEL_TOKEN"), ("PAD_TWO_D_ANIME", "TWO_D_ANIME_TOKEN")) if env_is_true(env)]
    if env_is_true("PAD_DURATION"):
        keys.append("DURATION_TOKEN")
    return keys


def get_negative_special_token_keys() -> Optional[List[str]]:
    return ["CAPTION_TOKEN", "LOGO_TOKEN", "TRANS_TOKEN", "BORDERNESS_TOKEN"] if env_is_true("NEG_PROMPT") else None


def _prepend(token: torch.Tensor, embs: torch.Tensor, masks: Optional[torch.Tensor]):
    """One token row in front of every (sample, chunk), truncated to CAPTION_ROWS; the mask gains a leading one."""
    N, C, _, D = embs.shape
    embs = torch.cat([token.to(device=embs.device, dtype=embs.dtype).expand(N, C, 1, D), embs], dim=2)[:, :, :CAPTION_ROWS]
    if masks is not None:
        masks = torch.cat([torch.ones(N, C, 1, dtype=embs.dtype, device=embs.device), masks], dim=-1)[:, :, :CAPTION_ROWS]
    return embs, masks


def pad_special_token(keys: Optional[List[str]], caption_embs: torch.Tensor, emb_masks: Optional[torch.Tensor],
                      tokens: Optional[Dict[str, torch.Tensor]] = None):
    """caption_embs `[N, chunks, L, C]`, emb_masks `[N, chunks, L]` or None.  Every key prepends its token, in order, so the LAST key
    ends up first.  `DURATION_TOKEN` is per chunk: chunk i of n gets DURATION_TOKEN_{min(n - i - 1, 7) + 1}.  Unknown keys are skipped
    as upstream skips them.  The mask takes the embeddings' dtype once a token is prepended (upstream's `torch.ones(dtype=_dtype)`)."""
    if not keys:
        return caption_embs, emb_masks
    tokens = load_special_tokens() if tokens is None else tokens
    for key in keys:
        if key == "DURATION_TOKEN":
            n = caption_embs.size(1)
            parts = [_prepend(tokens[f"DURATION_TOKEN_{min(n - i - 1, 7) + 1}"], caption_embs[:, i:i + 1],
                              None if emb_masks is None else emb_masks[:, i:i + 1]) for i in range(n)]
            caption_embs = torch.cat([p[0] for p in parts], dim=1)
            emb_masks = None if emb_masks is None else torch.cat([p[1] for p in parts], dim=1)
        elif key in tokens:
            caption_embs, emb_masks = _prepend(tokens[key], caption_embs, emb_masks)
    return caption_embs, emb_masks


@dataclass(frozen=True)
class InferenceInput:
    """video_generate.py:35-47"""
    caption_embs: torch.Tensor
    emb_masks: torch.Tensor
    y: torch.Tensor
    prefix_video: Union[torch.Tensor, None]
    latent_size: Tuple[int]
    t_schedule_config: Dict = field(default_factory=dict)
    num_steps: int = None
    vae_ckpt: str = None
    task_idx_list: List[int] = None
    report_chunk_num_list: List[int] = None
    chunk_num: int = None


def process_txt_embeddings(caption_embs: torch.Tensor, emb_masks: torch.Tensor, null_emb: torch.Tensor, infer_chunk_num: int,
                           clean_chunk_num: int, tokens: Optional[Dict[str, torch.Tensor]] = None):
    """The conditional half: the caption on every denoised chunk with the switched-on special tokens in front, the null caption with a
    zero mask on the clean chunks of a prefix video (video_generate.py:50-66)."""
    n = infer_chunk_num - clean_chunk_num
    caption_embs = caption_embs.repeat(1, n, 1, 1)
    emb_masks = emb_masks.unsqueeze(1).repeat(1, n, 1)
    caption_embs, emb_masks = pad_special_token(get_special_token_keys(), caption_embs, emb_masks, tokens)
    caption_embs = torch.cat([null_emb.repeat(1, clean_chunk_num, 1, 1), caption_embs], dim=1)
    emb_masks = torch.cat([torch.zeros(1, clean_chunk_num, emb_masks.size(2), dtype=emb_masks.dtype, device=emb_masks.device), emb_masks], dim=1)
    return caption_embs, emb_masks


def process_null_embeddings(null_caption_embedding: torch.Tensor, null_emb_masks: torch.Tensor, infer_chunk_num: int,
                            tokens: Optional[Dict[str, torch.Tensor]] = None):
    """The unconditional half: the null caption on every chunk (negative-prompt tokens in front under NEG_PROMPT), its mask set on the
    first 50 entries — `null_emb_masks` is written in place, as upstream writes it (video_generate.py:69-81)."""
    null_embs = null_caption_embedding.repeat(1, infer_chunk_num, 1, 1)
    neg = get_negative_special_token_keys()
    if neg:
        null_embs, _ = pad_special_token(neg, null_embs, None, tokens)
    null_emb_masks[:, :, :NULL_TOKEN_LENGTH] = 1
    null_emb_masks[:, :, NULL_TOKEN_LENGTH:] = 0
    return null_embs, null_emb_masks


def _null_caption(model) -> torch.Tensor:
    y = getattr(model, "y_embedder", None)
    if y is not None and hasattr(y, "null_caption_embedding"):
        return y.null_caption_embedding
    return model.w["y_embedder.null_caption_embedding"]          # HipVideoDiTModel keeps its fp32 modules' weights by name


@torch.no_grad()
def extract_feature_for_inference(model, prefix_video: Optional[torch.Tensor], caption_embs: torch.Tensor, emb_masks: torch.Tensor,
                                  tokens: Optional[Dict[str, torch.Tensor]] = None) -> InferenceInput:
    """video_generate.py:84-138.  caption_embs `[1, 1, L, C]`, emb_masks `[1, L]` (what `get_txt_embeddings` returns), prefix_video
    `[N, C, Tp, H, W]` latents or None."""
    mc, rc = model.model_config, model.runtime_config
    clean_chunk_num, prefix_frames = 0, 0
    if prefix_video is not None:
        prefix_frames = prefix_video.size(2)
        clean_chunk_num = prefix_frames // rc.chunk_width
    infer_chunk_num = math.ceil((rc.num_frames // rc.temporal_downsample_factor * 1.0 + prefix_frames) / rc.chunk_width)

    null = _null_caption(model).unsqueeze(0)                     # [1, L, C]
    cap, cap_masks = process_txt_embeddings(caption_embs, emb_masks, null, infer_chunk_num, clean_chunk_num, tokens)
    null_embs, null_masks = process_null_embeddings(null, torch.zeros_like(cap_masks), infer_chunk_num, tokens)
    if emb_masks.sum() == 0:                                      # the empty prompt: both halves are the null caption
        out_masks, y = torch.cat([null_masks, null_masks], dim=0), torch.cat([null_embs, null_embs])
    else:
        out_masks, y = torch.cat([cap_masks, null_masks], dim=0), torch.cat([cap, null_embs])

    in_channels = 16 if getattr(mc, "half_channel_vae", False) else mc.in_channels
    latent_t = infer_chunk_num * rc.chunk_width
    return InferenceInput(caption_embs=cap, emb_masks=out_masks, y=y, prefix_video=prefix_video,
                          latent_size=(1, in_channels, latent_t, rc.video_size_h // 8, rc.video_size_w // 8), t_schedule_config={},
                          num_steps=rc.num_steps, task_idx_list=[0], report_chunk_num_list=[infer_chunk_num - clean_chunk_num],
                          chunk_num=latent_t // rc.chunk_width)


def get_txt_embeddings(prompt: str, config, embedder) -> Tuple[torch.Tensor, torch.Tensor]:
    """prompt_process.py:184-212 for one process: `(caption_embs [1, 1, L, C] fp32, emb_masks [1, L])` on the embedder's device.
    `embedder` is a `HipT5Embedder` (upstream builds its own from `config.runtime_config.t5_pretrained`; here it is handed in, its
    `model_max_length` must be `config.model_config.caption_max_length`).  The tensor-parallel broadcast is not done here."""
    want = getattr(getattr(config, "model_config", None), "caption_max_length", None)
    if want is not None and getattr(embedder, "model_max_length", want) != want:
        raise ValueError(f"the embedder pads to {embedder.model_max_length}, the model's caption_max_length is {want}")
    caption_embs, emb_masks = embedder.get_text_embeddings([prompt])
    return caption_embs.float()[:, None], emb_masks
