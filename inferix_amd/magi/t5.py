"""MAGI-1's caption encoder on MI355X: T5 v1.1 XXL in fp32, what stands between a prompt and the first chunk.

Drop-in for `T5Embedder` (inferix/models/magi/t5/t5_model.py:27-150) and the HuggingFace `T5EncoderModel` it runs with
`torch_dtype=torch.float` (inferix/pipeline/magi/prompt_process.py:135-144): HF's state-dict keys, `get_text_embeddings(texts) ->
(last_hidden_state [B, L, 4096] fp32, attention_mask [B, L])`.  The tokenizer (sentencepiece files) and the caption cleaning
(`T5Embedder.text_preprocessing`, regexes over ftfy / bs4) are host-side string work and are injected.

How it runs here, all in fp32: per layer 4 GEMM launches (fused q|k|v, o + residual in place, fused wi_0|wi_1, wo + residual in place:
`ifx_gemm_f32`, exact-fp32 MFMA with one k-ordered chain per element), 2 `ifx_rmsnorm_f32`, one `ifx_t5_attention_f32` (one bias table
for all layers: only block 0 owns `relative_attention_bias`) and one `ifx_t5_gated_gelu_f32`; then the final norm.  The embedding gather
is a torch index.  `rows="valid"` runs the GEMMs and row kernels on the valid rows of every prompt packed into one matrix (a caption of
120 tokens padded to 800 is 15 % of the rows) and returns zeros in the padded rows; the valid rows are bit-identical to `rows="all"`.
"""
from __future__ import annotations

from typing import Callable, Dict, List, Optional, Sequence, Tuple

import torch

from .. import _hip
from .. import hip_ops as ops
from ..t5 import relative_position_table

F32 = torch.float32


def _key(state_dict, *names):
    for n in names:
        if n in state_dict:
            return state_dict[n]
    raise KeyError(f"HipT5v11Encoder: none of {names} in the state dict")


class HipT5v11Encoder:
    """HF `T5EncoderModel` (t5-v1_1: gated tanh-GELU FFN, shared relative-position bias) on the fp32 HIP kernels.
    `forward(ids, mask, rows="all" | "valid") -> [B, L, d_model]` fp32.  `mask` marks a PREFIX of every row valid (the tokenizer pads on
    the right)."""

    def __init__(self, state_dict: Optional[Dict[str, torch.Tensor]], *, d_model: int = 4096, num_heads: int = 64, d_ff: int = 10240,
                 num_layers: int = 24, num_buckets: int = 32, max_distance: int = 128, eps: float = 1e-6, device="cuda"):
        _hip.load()                                         # fail loudly without the HIP library
        self.device = torch.device(device)
        self.d_model, self.heads, self.d_ff, self.layers = d_model, num_heads, d_ff, num_layers
        self.buckets, self.max_distance, self.eps = num_buckets, max_distance, eps
        self.inner = num_heads * 64
        self.blocks: List[Dict[str, torch.Tensor]] = []
        self._tables: Dict[int, torch.Tensor] = {}
        if state_dict is not None:
            self.load_state_dict(state_dict)

    def load_state_dict(self, sd: Dict[str, torch.Tensor]) -> None:
        q0 = sd["encoder.block.0.layer.0.SelfAttention.q.weight"]
        if q0.shape[0] != self.heads * 64:
            raise NotImplementedError(f"ifx_t5_attention_f32 is built for head size 64, got {q0.shape[0] // self.heads}")
        g = lambda k: sd[k].to(device=self.device, dtype=F32)
        self.emb = _key(sd, "shared.weight", "encoder.embed_tokens.weight").to(device=self.device, dtype=F32).contiguous()
        self.final_norm = g("encoder.final_layer_norm.weight").contiguous()
        self.rel_bias = g("encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight").contiguous()     # [buckets, heads]
        self.blocks = []
        for i in range(self.layers):
            a, f = f"encoder.block.{i}.layer.0.", f"encoder.block.{i}.layer.1."
            self.blocks.append(dict(
                norm1=g(a + "layer_norm.weight").contiguous(), norm2=g(f + "layer_norm.weight").contiguous(),
                wqkv=torch.cat([g(a + f"SelfAttention.{n}.weight") for n in "qkv"], 0).contiguous(),
                wo=g(a + "SelfAttention.o.weight").contiguous(),
                wi=torch.cat([g(f + "DenseReluDense.wi_0.weight"), g(f + "DenseReluDense.wi_1.weight")], 0).contiguous(),
                wo_ff=g(f + "DenseReluDense.wo.weight").contiguous()))
        self._tables.clear()

    def load_synthetic(self, seed: int = 0, vocab_size: int = 32128) -> None:
        """Full-size random weights generated on the device block by block (no checkpoint exists offline): benchmarks.  Scales keep
        activations of order one and the attention scores a few units wide."""
        gen = torch.Generator(device=self.device).manual_seed(seed)
        r = lambda *s: torch.randn(*s, generator=gen, device=self.device, dtype=F32)
        d, inner, ff = self.d_model, self.inner, self.d_ff
        self.emb = r(vocab_size, d)
        self.final_norm = 1 + 0.1 * r(d)
        self.rel_bias = 2.0 * r(self.buckets, self.heads)
        self.blocks = []
        for _ in range(self.layers):
            self.blocks.append(dict(
                norm1=1 + 0.1 * r(d), norm2=1 + 0.1 * r(d),
                wqkv=torch.cat([r(inner, d) * (0.5 * d ** -0.5), r(inner, d) * d ** -0.5, r(inner, d) * d ** -0.5], 0),      # q.k: std 4
                wo=r(d, inner) * inner ** -0.5, wi=r(2 * ff, d) * d ** -0.5, wo_ff=r(d, ff) * ff ** -0.5))
        self._tables.clear()

    def _bias_table(self, L: int) -> torch.Tensor:
        t = self._tables.get(L)
        if t is None:
            t = self._tables[L] = relative_position_table(self.rel_bias, L, self.buckets, self.max_distance)      # [heads, 2L-1]
        return t

    @torch.no_grad()
    def forward(self, ids: torch.Tensor, mask: Optional[torch.Tensor] = None, rows: str = "all",
                taps: Optional[List[torch.Tensor]] = None) -> torch.Tensor:
        """`taps`, when given, receives the hidden state [B, L, d_model] after every block (tests name a failing layer with it)."""
        if rows not in ("all", "valid"):
            raise ValueError(f"rows must be 'all' or 'valid', got {rows!r}")
        if not self.blocks:
            raise RuntimeError("HipT5v11Encoder: no weights loaded (pass a state dict, or call load_synthetic)")
        B, L = ids.shape
        if L % 8 or not 8 <= L <= 1024:
            raise ValueError(f"sequence length {L}: ifx_t5_attention_f32 needs a multiple of 8 in [8, 1024] (MAGI pads to 800)")
        dev, d, inner = self.device, self.d_model, self.inner
        lens = torch.full((B,), L, dtype=torch.int64) if mask is None else mask.gt(0).sum(dim=1).to(torch.int64).cpu()
        seq = lens.to(device=dev, dtype=torch.int32)
        ids = ids.to(dev).reshape(-1)
        valid = rows == "valid"
        if valid:       # the rows of every prompt's valid prefix, in order
            keep = (torch.arange(L).unsqueeze(0) < lens.unsqueeze(1)).reshape(-1)
            pick = torch.nonzero(keep).squeeze(1).to(dev)
            ids = ids[pick]
            if pick.numel() == 0:       # outside the tokenizer's contract (it always emits EOS)
                return torch.zeros(B, L, d, dtype=F32, device=dev)
        x = self.emb[ids].contiguous()                                  # [rows, d]
        table = self._bias_table(L)
        qkv_full = torch.empty(B * L, 3 * inner, dtype=F32, device=dev) if valid else None
        for blk in self.blocks:
            h = ops.rmsnorm_f32(x, blk["norm1"], self.eps)
            if valid:       # attention addresses rows as prompt * L + token: scatter the packed rows (the others are never read)
                qkv_full[pick] = ops.gemm_f32(h, blk["wqkv"])
                qkv = qkv_full
            else:
                qkv = ops.gemm_f32(h, blk["wqkv"])
            o = ops.t5_attention_f32(qkv[:, :inner], qkv[:, inner:2 * inner], qkv[:, 2 * inner:], table, seq, B, self.heads,
                                     valid_rows_only=valid)
            if valid:
                o = o[pick]
            ops.gemm_f32(o, blk["wo"], residual=x, out=x)                # hidden + attention(...)
            h = ops.rmsnorm_f32(x, blk["norm2"], self.eps)
            hh = ops.t5_gated_gelu_f32(ops.gemm_f32(h, blk["wi"]))
            ops.gemm_f32(hh, blk["wo_ff"], residual=x, out=x)            # hidden + ff(...)
            if taps is not None:
                taps.append(self._unpack(x, pick, B, L) if valid else x.view(B, L, d).clone())      # x is updated in place
        y = ops.rmsnorm_f32(x, self.final_norm, self.eps)
        return self._unpack(y, pick if valid else None, B, L)

    def _unpack(self, x: torch.Tensor, pick: Optional[torch.Tensor], B: int, L: int) -> torch.Tensor:
        if pick is None:
            return x.view(B, L, self.d_model)
        out = torch.zeros(B * L, self.d_model, dtype=F32, device=self.device)
        out[pick] = x
        return out.view(B, L, self.d_model)

    __call__ = forward


class HipT5Embedder:
    """`T5Embedder` (t5_model.py:27-150) around a `HipT5v11Encoder`.  `tokenizer` is called as upstream calls HF's (`max_length`,
    `padding="max_length"`, `truncation=True`, `return_attention_mask=True`, `add_special_tokens=True`, `return_tensors="pt"`) and returns
    a mapping with `input_ids` and `attention_mask`.  `preprocess` is the caption cleaning (`T5Embedder.text_preprocessing` of the
    reference); None is upstream's `use_text_preprocessing=False` branch, `text.lower().strip()`."""

    def __init__(self, encoder: HipT5v11Encoder, tokenizer: Callable, *, model_max_length: int = 800,
                 preprocess: Optional[Callable[[str], str]] = None, rows: str = "all"):
        if not isinstance(encoder, HipT5v11Encoder):
            raise TypeError("HipT5Embedder: encoder must be a HipT5v11Encoder (there is no other text-encoder path)")
        if tokenizer is None:
            raise RuntimeError("HipT5Embedder: no tokenizer was given (pass AutoTokenizer.from_pretrained(<t5-v1_1-xxl files>))")
        self.model, self.tokenizer, self.model_max_length, self.preprocess, self.rows = encoder, tokenizer, model_max_length, preprocess, rows
        self.device = encoder.device
        self.torch_dtype = F32

    def text_preprocessing(self, text: str) -> str:
        return self.preprocess(text) if self.preprocess is not None else text.lower().strip()

    @torch.no_grad()
    def get_text_embeddings(self, texts: Sequence[str]) -> Tuple[torch.Tensor, torch.Tensor]:
        texts = [self.text_preprocessing(t) for t in texts]
        tok = self.tokenizer(texts, max_length=self.model_max_length, padding="max_length", truncation=True,
                             return_attention_mask=True, add_special_tokens=True, return_tensors="pt")
        ids, mask = tok["input_ids"], tok["attention_mask"]
        embs = self.model(ids, mask, rows=self.rows)
        return embs, mask.to(self.device)
