"""Argument bundles of the MAGI attention path — field-for-field mirrors of the reference's dataclasses
(inferix/core/types/inference.py:51-101) so call sites read the same."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from ..kvcache_manager import KVCacheManager, KVCacheRequest


@dataclass(frozen=True, eq=False)
class RangePlan:
    """What the host already knows of one forward's ranges, carried beside the device tensors (`forward(..., range_plan=plan)`) so that
    the model does not read it back from the device: the rows of `kv_range` and, per caption row of `xattn_mask` (in the row order of
    the `y` / `xattn_mask` handed to the same call), the number of valid caption tokens — `xattn_mask.sum` of that row.  The valid
    tokens of a caption are its FIRST ones (tokenizer padding: what `extract_feature_for_inference` and `get_txt_embeddings` produce);
    a mask with holes has no plan and takes the path that reads the mask."""
    kv_range: np.ndarray                     # int32 [rows, 2], host
    caption_lens: Tuple[int, ...]

    @staticmethod
    def make(kv_range, caption_lens: Sequence[int]) -> "RangePlan":
        kv = np.ascontiguousarray(np.asarray(kv_range, dtype=np.int32).reshape(-1, 2))
        return RangePlan(kv, tuple(int(v) for v in caption_lens))

    @property
    def max_seqlen_k(self) -> int:
        """`flat = torch.unique(kv_range, sorted=True); flat[-1] - flat[0]` (dit_model.py:300-301), an int32 subtraction."""
        return int(np.int32(self.kv_range.max()) - np.int32(self.kv_range.min()))

    def captions(self, start: Optional[int] = None, stop: Optional[int] = None) -> "RangePlan":
        """The same key ranges with the caption rows `[start:stop]` (the halves of a guidance batch)."""
        return RangePlan(self.kv_range, self.caption_lens[slice(start, stop)])

    def extended(self, tokens: int, caption_row: int, half: int) -> "RangePlan":
        """The nearly-clean widening of `forward_dispatcher` (dit_model.py:548-561): the conditional caption rows `[0:half]`, one more range
        `[0, tokens) + kv_range.max()` that sees only itself, and caption row `caption_row` once more behind them."""
        top = np.int32(self.kv_range.max())
        new = np.asarray([[0, tokens]], np.int32) + top
        return RangePlan(np.concatenate([self.kv_range, new], axis=0), self.caption_lens[:half] + (self.caption_lens[caption_row],))

    @staticmethod
    def uncondition(batch: int, tokens: int, caption_lens: Sequence[int]) -> "RangePlan":
        """`generate_kv_range_for_uncondition` (dit_model.py:91-100): one self-contained range `[b n, (b + 1) n]` per batch row."""
        b = np.arange(batch, dtype=np.int32)
        return RangePlan(np.stack([b * np.int32(tokens), (b + 1) * np.int32(tokens)], axis=1), tuple(int(v) for v in caption_lens))

    def batch_row(self, b: int, batch: int, denoising_range_num: int) -> "RangePlan":
        """Row `b` of a batched forward: its share of the key ranges rebased to the row (`kv - kv.min()`) and its captions."""
        rows = self.kv_range.shape[0] // batch
        kv = self.kv_range[b * rows:(b + 1) * rows]
        dn = denoising_range_num
        return RangePlan(kv - kv.min(), self.caption_lens[b * dn:(b + 1) * dn])


def cu_seqlens(lengths: Sequence[int]) -> np.ndarray:
    """`cat([0, lengths]).to(int64).cumsum(-1).to(int32)`: the packed offsets of `PackedCrossAttnParams`, on the host."""
    return np.concatenate([np.zeros(1, np.int64), np.asarray(lengths, np.int64).reshape(-1)]).cumsum().astype(np.int32)


@dataclass(frozen=True)
class PackedCoreAttnParams:
    q_range: torch.Tensor
    k_range: torch.Tensor
    np_q_range: np.ndarray
    np_k_range: np.ndarray
    max_seqlen_q: int
    max_seqlen_k: int


@dataclass(frozen=True)
class PackedCrossAttnParams:
    q_ranges: Optional[torch.Tensor] = None
    kv_ranges: Optional[torch.Tensor] = None
    cu_seqlens_q: Optional[torch.Tensor] = None
    cu_seqlens_kv: Optional[torch.Tensor] = None
    max_seqlen_q: Optional[int] = None
    max_seqlen_kv: Optional[int] = None
    # host copies of the two range tables ([[start, end], ...] per segment), present when the forward came with a RangePlan: the layers
    # read them instead of `.tolist()` on the device tensors.  None: read the tensors.
    host_q_ranges: Optional[List[List[int]]] = None
    host_kv_ranges: Optional[List[List[int]]] = None


@dataclass(frozen=True)
class ModelMetaArgs:
    H: int
    W: int
    cp_pad_size: int
    cp_split_sizes: Optional[List[int]]
    slice_point: int
    denoising_range_num: int
    range_num: int
    extract_prefix_video_feature: bool
    fwd_extra_1st_chunk: bool
    distill_nearly_clean_chunk: bool
    clip_token_nums: int
    enable_cuda_graph: bool
    core_attn_params: Optional[PackedCoreAttnParams]
    cross_attn_params: Optional[PackedCrossAttnParams]


class InferenceParams:
    """inference.py:90-101: per-request cache handle.  The manager lives on the given device (the reference takes
    torch.cuda.current_device())."""

    def __init__(self, max_batch_size: int, max_sequence_length: int, device=None):
        self.max_sequence_length = max_sequence_length
        self.max_batch_size = max_batch_size
        self.sequence_len_offset = 0
        self.kv_cache_request = KVCacheRequest(request_id="magi")
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.kv_cache_manager = KVCacheManager(device=device)
        self.key_value_memory_dict = {}
        self.update_kv_cache = False
