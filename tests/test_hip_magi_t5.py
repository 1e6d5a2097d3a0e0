"""GPU tests of the fp32 T5 caption encoder (inferix_amd/csrc/ifx_t5f.hip, inferix_amd/magi/t5.py) and of the prompt-to-caption path.

Parity rule for everything but the GEMM's derived bound: both sides are fp32 evaluations of one formula, so
    rel_l2(HIP, exact64) <= 2 x rel_l2(reference fp32, exact64)          (and the same factor on the max-abs error of the per-op tests)
with the reference fp32 distance measured in the test by torch on the CPU (per-op) or stored by the generator (`hf32`, HuggingFace's
`T5EncoderModel` in fp32).  One bf16 rounding anywhere in the chain would be ~4e-3, three orders of magnitude past the bound.
Neither `transformers` nor the reference is imported here.  Measured values: profiles/r17_magi_t5.md.
"""
import dataclasses
from types import SimpleNamespace

import pytest
import torch

import magi_t5_util as U

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
FACTOR = U.PARITY_FACTOR


def _parity(name, got, ref32, exact64, max_abs=True):
    """Prints both distances, then asserts the rule."""
    d_hip, d_ref = U.rel_l2(got, exact64), U.rel_l2(ref32, exact64)
    m_hip, m_ref = U.max_abs(got, exact64), U.max_abs(ref32, exact64)
    print(f"{name}: rel_l2 HIP {d_hip:.3e} reference fp32 {d_ref:.3e} ({d_hip / max(d_ref, 1e-300):.2f}x); "
          f"max-abs HIP {m_hip:.3e} reference fp32 {m_ref:.3e}")
    assert torch.isfinite(got).all(), name
    assert d_hip <= FACTOR * d_ref, f"{name}: rel_l2 {d_hip:.3e} > {FACTOR} x {d_ref:.3e}"
    if max_abs:
        assert m_hip <= FACTOR * m_ref, f"{name}: max-abs {m_hip:.3e} > {FACTOR} x {m_ref:.3e}"


# ---- ifx_gemm_f32 --------------------------------------------------------------------------------------------------------------------
GEMM_SHAPES = [(1, 64, 64), (33, 192, 64), (129, 320, 192), (150, 64, 2048), (800, 128, 64)]


def _gemm_data(M, N, K, seed=0):
    g = torch.Generator().manual_seed(1000 + seed + M + N + K)
    wide = torch.randn(M, K + 64, generator=g)              # x is the column block [32, 32 + K) of this
    w = torch.randn(N, K, generator=g) * K ** -0.5
    res = torch.randn(M, N, generator=g)
    return wide, w, res


def _gemm_bound(x, w, res, K):
    return (K + 2) * 2.0 ** -24 * (x.double().abs() @ w.double().abs().t() + (0 if res is None else res.double().abs()))


@pytest.mark.parametrize("M,N,K", GEMM_SHAPES)
def test_gemm_f32_accuracy_strides_and_aliasing(M, N, K):
    """|y - y64| <= (K + 2) 2^-24 (|x| |w|^T + |res|), the standard bound of a length-K fp32 chain plus the residual add: derived."""
    from inferix_amd import hip_ops as ops
    wide, w, res = _gemm_data(M, N, K)
    x = wide[:, 32:32 + K]
    xd, wd, rd = wide.cuda()[:, 32:32 + K], w.cuda(), res.cuda()
    assert xd.stride(0) == K + 64
    y64 = x.double() @ w.double().t()
    plain = ops.gemm_f32(xd.contiguous(), wd)
    variants = {
        "plain": (plain, None),
        "x column block": (ops.gemm_f32(xd, wd), None),
        "residual": (ops.gemm_f32(xd, wd, residual=rd), res),
        "ldy > N": (ops.gemm_f32(xd, wd, out=torch.full((M, N + 64), 7.0, device="cuda")[:, 32:32 + N]), None),
    }
    inplace = rd.clone()
    assert ops.gemm_f32(xd, wd, residual=inplace, out=inplace) is inplace
    variants["y == res"] = (inplace, res)
    for name, (got, r) in variants.items():
        want = y64 + (0 if r is None else r.double())
        err = (got.cpu().double() - want).abs()
        bound = _gemm_bound(x, w, r, K)
        worst = float((err / bound).max())
        print(f"gemm {M}x{N}x{K} {name}: worst error / bound {worst:.3f}")
        assert torch.isfinite(got).all() and worst <= 1.0, (name, worst)
    assert torch.equal(variants["x column block"][0], plain) and torch.equal(variants["ldy > N"][0], plain)
    assert torch.equal(variants["y == res"][0], variants["residual"][0])
    pad = torch.full((M, N + 64), 7.0, device="cuda")
    ops.gemm_f32(xd, wd, out=pad[:, 32:32 + N])
    assert bool((pad[:, :32] == 7.0).all()) and bool((pad[:, 32 + N:] == 7.0).all()), "the launch wrote outside its columns"
    assert torch.equal(ops.gemm_f32(xd, wd, residual=rd), variants["residual"][0]), "two runs differ"


def test_gemm_f32_rows_do_not_depend_on_m_or_on_the_tile():
    """One k-ordered chain per element: rows 0..32 of an M = 150 launch are the M = 33 launch's, through either tile and through both."""
    from inferix_amd import hip_ops as ops
    wide, w, res = _gemm_data(150, 64, 2048, seed=5)
    xd, wd, rd = wide.cuda()[:, 32:32 + 2048], w.cuda(), res.cuda()
    outs = {(m, t): ops.gemm_f32(xd[:m], wd, residual=rd[:m], tile=t) for m in (150, 33) for t in (0, 1, 2)}
    for (m, t), y in outs.items():
        assert torch.equal(y, outs[(150, 1)][:m]), f"M {m} tile {t} differs from the 128-row tile at M 150"
    assert not torch.equal(outs[(150, 1)][:33], torch.zeros_like(outs[(33, 2)]))
    # a second shape whose N is not a multiple of the tall tile's 128 columns, and K long enough for many staging rounds
    wide, w, res = _gemm_data(129, 320, 192, seed=6)
    xd, wd = wide.cuda()[:, 32:32 + 192], w.cuda()
    assert torch.equal(ops.gemm_f32(xd, wd, tile=1), ops.gemm_f32(xd, wd, tile=2))


def test_gemm_f32_refuses_shapes_outside_its_contract():
    from inferix_amd import _hip
    lib = _hip.load()
    a = torch.zeros(4, 128, device="cuda")
    for M, N, K in ((4, 64, 40), (4, 72, 64)):
        rc = lib.ifx_gemm_f32(a.data_ptr(), 128, a.data_ptr(), None, 0, a.data_ptr(), 128, M, N, K, 0, None)
        assert rc == -3 and b"ifx_gemm_f32" in lib.ifx_last_error() and b"% 64" in lib.ifx_last_error()       # IFX_EUNSUP, with a message
    torch.cuda.synchronize()
    assert float(a.abs().sum()) == 0.0      # nothing was launched


# ---- ifx_t5_attention_f32 ------------------------------------------------------------------------------------------------------------
ATTN_CASES = [(1, 64, 2, [64]), (3, 96, 1, [1, 96, 50]), (2, 200, 2, [150, 37]), (1, 800, 1, [517])]


@pytest.mark.parametrize("B,L,heads,lens", ATTN_CASES)
def test_t5_attention_f32(B, L, heads, lens):
    from inferix_amd import hip_ops as ops
    g = torch.Generator().manual_seed(2000 + L)
    inner = heads * 64
    qkv = torch.randn(B * L, 3 * inner, generator=g)
    qkv[:, :inner] *= 0.5                                       # q.k over 64 channels: std 4
    table = 2.0 * torch.randn(heads, 2 * L - 1, generator=g)
    pad = torch.cat([torch.arange(L) >= n for n in lens])       # rows past each prompt's length
    exact = U.attention_ref(qkv[:, :inner].double(), qkv[:, inner:2 * inner].double(), qkv[:, 2 * inner:].double(), table.double(), lens, B, heads)
    ref32 = U.attention_ref(qkv[:, :inner], qkv[:, inner:2 * inner], qkv[:, 2 * inner:], table, lens, B, heads)
    seq = torch.tensor(lens, dtype=torch.int32, device="cuda")
    # mode 0: every padded query row, K / V rows past the length poisoned
    d0 = qkv.clone()
    d0[pad, inner:] = float("nan")
    d0 = d0.cuda()
    out0 = ops.t5_attention_f32(d0[:, :inner], d0[:, inner:2 * inner], d0[:, 2 * inner:], table.cuda(), seq, B, heads)
    _parity(f"attention B{B} L{L} h{heads} all rows", out0.cpu(), ref32, exact)
    # mode 1: the q rows past the length poisoned too
    d1 = qkv.clone()
    d1[pad] = float("nan")
    d1 = d1.cuda()
    out1 = torch.full((B * L, inner), float("nan"), device="cuda")
    ops.t5_attention_f32(d1[:, :inner], d1[:, inner:2 * inner], d1[:, 2 * inner:], table.cuda(), seq, B, heads, valid_rows_only=True, out=out1)
    assert torch.isfinite(out1).all()
    assert torch.equal(out1[~pad.cuda()], out0[~pad.cuda()]), "valid rows differ between the two row modes"
    assert float(out1[pad.cuda()].abs().sum()) == 0.0 if pad.any() else True
    again = ops.t5_attention_f32(d0[:, :inner], d0[:, inner:2 * inner], d0[:, 2 * inner:], table.cuda(), seq, B, heads)
    assert torch.equal(again, out0), "two runs differ"


def test_t5_attention_f32_zero_length_prompt_writes_zeros():
    """Outside the contract (the tokenizer always emits EOS): in bounds, zeros."""
    from inferix_amd import hip_ops as ops
    L = 40
    qkv = torch.full((2 * L, 192), float("nan"), device="cuda")
    qkv[L:L + 8] = torch.randn(8, 192, device="cuda")
    seq = torch.tensor([0, 8], dtype=torch.int32, device="cuda")
    for mode in (False, True):
        out = ops.t5_attention_f32(qkv[:, :64], qkv[:, 64:128], qkv[:, 128:], torch.zeros(1, 2 * L - 1, device="cuda"), seq, 2, 1,
                                   valid_rows_only=mode, out=torch.full((2 * L, 64), float("nan"), device="cuda"))
        assert float(out[:L].abs().sum()) == 0.0 and torch.isfinite(out[L:L + 8]).all()


# ---- row kernels ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [128, 4096])
def test_rmsnorm_f32(dim):
    from inferix_amd import hip_ops as ops
    g = torch.Generator().manual_seed(dim)
    x = torch.randn(70, dim, generator=g) * torch.rand(70, 1, generator=g) * 4
    w = 1 + 0.1 * torch.randn(dim, generator=g)
    got = ops.rmsnorm_f32(x.cuda(), w.cuda(), 1e-6).cpu()
    _parity(f"rmsnorm 70x{dim}", got, U.rmsnorm_ref(x, w, 1e-6), U.rmsnorm_ref(x.double(), w.double(), 1e-6))
    wide = torch.zeros(70, dim + 64, device="cuda")
    wide[:, 32:32 + dim] = x.cuda()
    assert torch.equal(ops.rmsnorm_f32(wide[:, 32:32 + dim], w.cuda(), 1e-6).cpu(), got), "row stride"


def test_gated_gelu_f32():
    """Gate pre-activations of scale 2: the 1 + tanh cancellation tail is hit."""
    from inferix_amd import hip_ops as ops
    g = torch.Generator().manual_seed(9)
    gu = torch.randn(70, 2 * 256, generator=g)
    gu[:, :256] *= 2.0
    gu[0, :8] = torch.tensor([-9.0, -6.0, -4.5, -3.0, 0.0, 3.0, 6.0, 9.0])
    got = ops.t5_gated_gelu_f32(gu.cuda()).cpu()
    assert float((gu[:, :256] < -3).float().mean()) > 0.02
    _parity("gated gelu 70x2x256", got, U.gated_gelu_ref(gu), U.gated_gelu_ref(gu.double()))


# ---- the encoder end to end ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=list(U.CASES))
def encoder_case(request):
    from inferix_amd.magi.t5 import HipT5v11Encoder
    name = request.param
    c = U.CASES[name]
    fx = U.load_parts(name)
    enc = HipT5v11Encoder(U.make_weights(c), device="cuda", **c.hip_kwargs())
    ids, mask = U.make_inputs(c)
    taps_all, taps_valid = [], []
    out_all = enc(ids, mask, rows="all", taps=taps_all)
    out_valid = enc(ids, mask, rows="valid", taps=taps_valid)
    return SimpleNamespace(name=name, c=c, fx=fx, enc=enc, ids=ids, mask=mask, out_all=out_all, out_valid=out_valid, taps_all=taps_all,
                           taps_valid=taps_valid, keep=U.valid_rows(mask))


def test_encoder_all_rows_vs_exact(encoder_case):
    e = encoder_case
    assert e.out_all.dtype == F32 and e.out_all.shape == (len(e.c.lens), e.c.L, e.c.d_model)
    for i, t in enumerate(e.taps_all):       # a failure names its layer
        _parity(f"{e.name} block {i} (all rows)", t.cpu(), e.fx[f"block{i}_ref32"], e.fx[f"block{i}_exact64"], max_abs=False)
    _parity(f"{e.name} last_hidden_state (all rows)", e.out_all.cpu(), e.fx["hf32"], e.fx["exact64"], max_abs=False)


def test_encoder_valid_rows_vs_exact(encoder_case):
    e = encoder_case
    k = e.keep
    for i, t in enumerate(e.taps_valid):
        _parity(f"{e.name} block {i} (valid rows)", t.cpu()[k], e.fx[f"block{i}_ref32"][k], e.fx[f"block{i}_exact64"][k], max_abs=False)
    _parity(f"{e.name} last_hidden_state (valid rows)", e.out_valid.cpu()[k], e.fx["hf32"][k], e.fx["exact64"][k], max_abs=False)


def test_encoder_valid_rows_are_bitwise_those_of_all_rows(encoder_case):
    e = encoder_case
    k = e.keep.cuda()
    assert torch.equal(e.out_valid[k], e.out_all[k])
    assert float(e.out_valid[~k].abs().sum()) == 0.0 if bool((~k).any()) else True
    for a, v in zip(e.taps_all, e.taps_valid):
        assert torch.equal(v[k], a[k])


def test_encoder_rows_do_not_depend_on_the_batch_and_runs_repeat(encoder_case):
    e = encoder_case
    for rows in ("all", "valid"):
        want = e.out_all if rows == "all" else e.out_valid
        assert torch.equal(e.enc(e.ids, e.mask, rows=rows), want), f"two runs differ ({rows})"
        for b in range(len(e.c.lens)):
            alone = e.enc(e.ids[b:b + 1], e.mask[b:b + 1], rows=rows)
            assert torch.equal(alone[0], want[b]), f"prompt {b} alone differs from the batch ({rows})"


# ---- embedder and packing ------------------------------------------------------------------------------------------------------------
class FakeTokenizer:
    """Stands in for HF's tokenizer: one id per character, EOS = 1, right padding.  Records how it was called."""

    def __init__(self, vocab):
        self.vocab, self.calls = vocab, []

    def __call__(self, texts, **kw):
        self.calls.append((list(texts), kw))
        L = kw["max_length"]
        ids = torch.zeros(len(texts), L, dtype=torch.int64)
        mask = torch.zeros(len(texts), L, dtype=torch.int64)
        for b, t in enumerate(texts):
            toks = [2 + ord(ch) % (self.vocab - 2) for ch in t][:L - 1] + [1]
            ids[b, :len(toks)] = torch.tensor(toks)
            mask[b, :len(toks)] = 1
        return {"input_ids": ids, "attention_mask": mask}


def _small_embedder(L, rows="all", preprocess=None):
    from inferix_amd.magi.t5 import HipT5Embedder, HipT5v11Encoder
    c = dataclasses.replace(U.CASES["magi_t5_long"], L=L)       # d_model 64: the caption width of the tiny MAGI model
    enc = HipT5v11Encoder(U.make_weights(c), device="cuda", **c.hip_kwargs())
    tok = FakeTokenizer(c.vocab)
    return HipT5Embedder(enc, tok, model_max_length=L, preprocess=preprocess, rows=rows), tok


def test_embedder_calls_the_tokenizer_like_upstream_and_returns_fp32_with_the_mask_on_the_device():
    emb, tok = _small_embedder(24)
    embs, mask = emb.get_text_embeddings(["  A Cat on a Mat ", "dog"])
    texts, kw = tok.calls[0]
    assert texts == ["a cat on a mat", "dog"]                                   # preprocess=None: lower().strip()
    assert kw == dict(max_length=24, padding="max_length", truncation=True, return_attention_mask=True, add_special_tokens=True,
                      return_tensors="pt")
    assert embs.dtype == F32 and embs.shape == (2, 24, 64) and embs.is_cuda and torch.isfinite(embs).all()
    assert mask.is_cuda and mask.shape == (2, 24) and mask.sum(1).tolist() == [15, 4]
    emb2, tok2 = _small_embedder(24, rows="valid", preprocess=lambda s: s.upper())
    embs2, _ = emb2.get_text_embeddings(["  A Cat on a Mat "])
    assert tok2.calls[0][0] == ["  A CAT ON A MAT "] and float(embs2[0, 19:].abs().sum()) == 0.0


def test_prompt_to_one_schedule_step_smoke(monkeypatch):
    """A prompt through the embedder, `get_txt_embeddings`, `extract_feature_for_inference` and one step of `ChunkSchedule.run` on the
    tiny model of tests/test_hip_magi_model.py (its caption width; the caption length raised from 12 to 16, a multiple of 8)."""
    import magi_model_oracle as MM
    from test_hip_magi_model import _config
    from inferix.pipeline.magi.prompt_process import get_txt_embeddings
    from inferix.pipeline.magi.video_generate import extract_feature_for_inference
    from inferix_amd.magi.model import HipVideoDiTModel
    from inferix_amd.magi.schedule import ChunkSchedule
    from inferix_amd.magi.types import InferenceParams
    for k in U.ENV_SWITCHES:
        monkeypatch.delenv(k, raising=False)
    cfg = dataclasses.replace(MM.tiny_model_config(), caption_max_length=16)
    config = _config(cfg)
    chunk_num, cw, Hl, Wl = 3, 2, 8, 12
    config.runtime_config = SimpleNamespace(cfg_number=1, noise2clean_kvrange=[4, 3, 2, 2], clean_chunk_kvrange=1, clean_t=0.9999,
                                            chunk_width=cw, num_frames=chunk_num * cw * 4, temporal_downsample_factor=4,
                                            video_size_h=Hl * 8, video_size_w=Wl * 8, num_steps=8)
    config.engine_config.shortcut_mode = "8,16,16"
    config.engine_config.distill_nearly_clean_chunk_threshold = 0.3
    model = HipVideoDiTModel(config, "cuda")
    model.load_synthetic(3)
    emb, _ = _small_embedder(cfg.caption_max_length)
    assert emb.model.d_model == cfg.caption_channels
    caption_embs, emb_masks = get_txt_embeddings("a red fox", config, emb)
    assert caption_embs.shape == (1, 1, 16, cfg.caption_channels) and caption_embs.is_cuda and emb_masks.is_cuda
    ii = extract_feature_for_inference(model, None, caption_embs, emb_masks)
    assert ii.y.shape == (2, chunk_num, 16, cfg.caption_channels) and ii.emb_masks.shape == (2, chunk_num, 16) and ii.y.is_cuda
    assert ii.latent_size == (1, cfg.in_channels, chunk_num * cw, Hl, Wl) and ii.chunk_num == chunk_num
    assert ii.emb_masks[0].sum(-1).eq(10).all()
    g = torch.Generator().manual_seed(1)
    x0 = torch.randn(*ii.latent_size, generator=g)
    x = torch.cat([x0, x0], 0).cuda()
    tokens = cw * (Hl // 2) * (Wl // 2)
    out = ChunkSchedule(ii.num_steps, 4, ii.chunk_num, cw).run(model, x.clone(), ii.y, ii.emb_masks.float(), InferenceParams(1, chunk_num * tokens),
                                                               steps=[0])
    assert torch.isfinite(out).all() and not torch.equal(out, x)
