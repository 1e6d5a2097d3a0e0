"""CPU tests of the MAGI prompt-to-caption path: the caption packing of inferix_amd/magi/prompt.py against fixtures the REFERENCE's own
functions produced (tools/gen_golden_magi_t5.py), bit for bit — the packing only moves fp32 data; the env switches; the fields of
`InferenceInput`; the float32 restatement of the T5 encoder (tests/magi_t5_util.py) against HuggingFace's fp32 output; the new exports
in header, bindings and library; the three import paths of the reference."""
import os
import re

import pytest
import torch

import magi_t5_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOKEN_PATH = os.path.join(U.GOLDEN_DIR, "magi_special_tokens.npz")


@pytest.fixture(scope="module")
def pack():
    return U.load_parts("magi_prompt_pack")


@pytest.fixture(scope="module")
def tokens():
    from inferix_amd.magi import prompt as P
    return P.load_special_tokens(TOKEN_PATH)


def test_special_tokens_are_cast_through_fp16_and_named_like_upstream(tokens):
    raw = U.make_special_tokens()
    assert set(tokens) == {"CAPTION_TOKEN", "LOGO_TOKEN", "TRANS_TOKEN", "HQ_TOKEN", "STATIC_FIRST_FRAMES_TOKEN", "DYNAMIC_FIRST_FRAMES_TOKEN",
                           "BORDERNESS_TOKEN", "THREE_D_MODEL_TOKEN", "TWO_D_ANIME_TOKEN"} | {f"DURATION_TOKEN_{n}" for n in range(1, 9)}
    f16 = lambda a: torch.tensor(a).to(torch.float16)
    assert tokens["HQ_TOKEN"].dtype == torch.float16 and torch.equal(tokens["HQ_TOKEN"], f16(raw["other_tokens"][1:2]))
    assert torch.equal(tokens["CAPTION_TOKEN"], f16(raw["caption_token"]))
    assert torch.equal(tokens["DURATION_TOKEN_1"], f16(raw["other_tokens"][7:8]))
    assert torch.equal(tokens["DURATION_TOKEN_8"], f16(raw["other_tokens"][14:15]))
    assert torch.equal(tokens["TWO_D_ANIME_TOKEN"], f16(raw["other_tokens"][16:17]))


def test_special_token_file_is_read_lazily_from_the_argument_or_the_environment(monkeypatch, tmp_path):
    from inferix_amd.magi import prompt as P           # importing did not need the file
    monkeypatch.setenv("SPECIAL_TOKEN_PATH", str(tmp_path / "absent.npz"))
    with pytest.raises(FileNotFoundError, match="SPECIAL_TOKEN_PATH"):
        P.load_special_tokens()
    monkeypatch.setenv("SPECIAL_TOKEN_PATH", TOKEN_PATH)
    assert torch.equal(P.load_special_tokens()["LOGO_TOKEN"], P.load_special_tokens(TOKEN_PATH)["LOGO_TOKEN"])


def test_env_switches_select_the_token_keys_in_upstream_order(monkeypatch):
    from inferix_amd.magi import prompt as P
    for k in U.ENV_SWITCHES:
        monkeypatch.delenv(k, raising=False)
    assert P.get_special_token_keys() == [] and P.get_negative_special_token_keys() is None
    for k in U.ENV_SWITCHES:
        monkeypatch.setenv(k, "true")
    assert P.get_special_token_keys() == ["STATIC_FIRST_FRAMES_TOKEN", "DYNAMIC_FIRST_FRAMES_TOKEN", "BORDERNESS_TOKEN", "HQ_TOKEN",
                                          "THREE_D_MODEL_TOKEN", "TWO_D_ANIME_TOKEN", "DURATION_TOKEN"]
    assert P.get_negative_special_token_keys() == ["CAPTION_TOKEN", "LOGO_TOKEN", "TRANS_TOKEN", "BORDERNESS_TOKEN"]
    for v, want in (("1", True), ("Yes", True), ("on", True), ("enabled", True), ("0", False), ("false", False), ("", False)):
        monkeypatch.setenv("PAD_HQ", v)
        assert ("HQ_TOKEN" in P.get_special_token_keys()) is want, v


@pytest.mark.parametrize("name", list(U.PACK_CASES))
def test_packing_matches_the_reference_bit_for_bit(name, pack, tokens):
    from inferix_amd.magi import prompt as P
    assert int(pack["from_reference"]) == 1, "the fixture was not produced by the reference's functions"
    c = U.PACK_CASES[name]
    model = U.pack_model(c)
    prefix, embs, mask = U.pack_inputs(c)
    with U.pack_env(c):
        e2, m2 = P.pad_special_token(P.get_special_token_keys(), embs.repeat(1, 2, 1, 1), mask.unsqueeze(1).repeat(1, 2, 1), tokens)
        ii = P.extract_feature_for_inference(model, prefix, embs.clone(), mask.clone(), tokens)
    for got, key in ((e2, "pad2.embs"), (m2, "pad2.masks")) + tuple((getattr(ii, k), k) for k in U.PACK_FIELDS):
        want = pack[f"{name}.{key}"]
        assert got.dtype == want.dtype and got.shape == want.shape, (key, got.dtype, want.dtype, got.shape, want.shape)
        assert torch.equal(got, want), f"{name}.{key}"
    assert isinstance(ii, P.InferenceInput)
    assert tuple(ii.latent_size) == tuple(pack[f"{name}.latent_size"].tolist())
    assert [ii.num_steps, ii.chunk_num, ii.report_chunk_num_list[0], ii.task_idx_list[0]] == pack[f"{name}.scalars"].tolist()
    assert ii.t_schedule_config == {} and ii.vae_ckpt is None and ii.prefix_video is prefix
    # the shapes ChunkSchedule.run takes
    assert ii.y.shape == (2, ii.chunk_num, c.L, U.TOKEN_WIDTH) and ii.emb_masks.shape == (2, ii.chunk_num, c.L)


def test_packing_cases_cover_what_they_claim(pack):
    raw = U.make_special_tokens()
    tok = lambda i: torch.tensor(raw["other_tokens"][i]).to(torch.float16).float()
    # DURATION per chunk: chunk i of n carries other_tokens[7 + min(n - i - 1, 7)] in row 0 (prepended last), HQ in row 1
    for name, n in (("hq_duration_3", 3), ("hq_duration_10", 10)):
        y = pack[f"{name}.y"]
        for i in range(n):
            assert torch.equal(y[0, i, 0], tok(7 + min(n - i - 1, 7))), (name, i)
            assert torch.equal(y[0, i, 1], tok(1))
    assert torch.equal(pack["hq_duration_10.y"][0, 0, 0], pack["hq_duration_10.y"][0, 2, 0])            # saturated at index 7
    assert not torch.equal(pack["hq_duration_10.y"][0, 2, 0], pack["hq_duration_10.y"][0, 3, 0])
    # a prefix video of two clean chunks: null caption with zero masks in front, on the conditional half
    c = U.PACK_CASES["prefix_2_clean"]
    null = U.pack_model(c).y_embedder.null_caption_embedding
    y, m = pack["prefix_2_clean.y"], pack["prefix_2_clean.emb_masks"]
    assert torch.equal(y[0, 0], null) and torch.equal(y[0, 1], null) and m[0, :2].sum() == 0 and m[0, 2].sum() == c.caption_len + 1
    assert tuple(pack["prefix_2_clean.latent_size"].tolist())[1] == 16                                   # half_channel_vae
    # the null half: 50 mask entries; the empty prompt: both halves null
    assert all(pack[f"{k}.emb_masks"][1].sum(-1).eq(50).all() for k in U.PACK_CASES)
    assert torch.equal(pack["empty_prompt.y"][0], pack["empty_prompt.y"][1])
    assert torch.equal(pack["empty_prompt.emb_masks"][0], pack["empty_prompt.emb_masks"][1])
    # NEG_PROMPT: four tokens in front of the null caption, last key first
    assert torch.equal(pack["neg_prompt.y"][1, 0, 0], tok(4))
    assert torch.equal(pack["neg_prompt.y"][1, 0, 3], torch.tensor(raw["caption_token"][0]).to(torch.float16).float())
    # truncation: 800 rows stay 800 and the caption's last three rows fall off
    _, embs, _ = U.pack_inputs(U.PACK_CASES["truncate_800"])
    assert pack["truncate_800.y"].shape[2] == 800 and torch.equal(pack["truncate_800.y"][0, 0, 3:], embs[0, 0, :797])


def test_get_txt_embeddings_returns_what_the_packing_takes():
    from inferix_amd.magi import prompt as P

    class Embedder:
        model_max_length = 16

        def get_text_embeddings(self, texts):
            assert texts == ["a prompt"]
            return torch.ones(1, 16, 4, dtype=torch.float32), torch.ones(1, 16, dtype=torch.int64)

    cfg = type("C", (), {"model_config": type("M", (), {"caption_max_length": 16})()})()
    embs, masks = P.get_txt_embeddings("a prompt", cfg, Embedder())
    assert embs.shape == (1, 1, 16, 4) and embs.dtype == torch.float32 and masks.shape == (1, 16)
    cfg.model_config.caption_max_length = 800
    with pytest.raises(ValueError, match="caption_max_length"):
        P.get_txt_embeddings("a prompt", cfg, Embedder())


@pytest.mark.parametrize("name", list(U.CASES))
def test_fp32_restatement_sits_inside_the_generators_assertion(name):
    """Two fp32 evaluations of one formula: the restatement is no further from HF's fp32 output than HF is from the exact answer, and the
    stored exact answer is the restatement's float64 evaluation."""
    c, fx = U.CASES[name], U.load_parts(name)
    ids, mask = U.make_inputs(c)
    assert torch.equal(ids, fx["ids"]) and torch.equal(mask, fx["mask"])
    d_hf = U.rel_l2(fx["hf32"], fx["exact64"])
    mine = U.encoder_forward(U.make_weights(c, torch.float32), c, ids, mask)
    d_mine = U.rel_l2(mine, fx["hf32"])
    print(f"{name}: hf32 vs exact64 {d_hf:.3e}, restatement32 vs hf32 {d_mine:.3e}")
    assert 1e-8 < d_hf < 1e-5 and d_mine <= float(fx["restatement_fraction"]) * d_hf
    taps = []
    exact = U.encoder_forward(U.make_weights(c, torch.float64), c, ids, mask, taps)
    assert U.rel_l2(exact, fx["exact64"]) < 1e-13
    for i, t in enumerate(taps):
        assert U.rel_l2(t, fx[f"block{i}_exact64"]) < 1e-13, i
        assert U.rel_l2(fx[f"block{i}_ref32"], fx[f"block{i}_exact64"]) < 1e-5, i


def test_new_exports_are_in_header_bindings_and_library_and_the_abi_minor_stays_7():
    from inferix_amd import _hip
    names = {"ifx_gemm_f32", "ifx_t5_attention_f32", "ifx_rmsnorm_f32", "ifx_t5_gated_gelu_f32"}
    hdr = open(os.path.join(ROOT, "include", "inferix_hip.h")).read()
    assert names <= set(re.findall(r"\b(ifx_[a-z0-9_]+)\s*\(", hdr)) and names <= set(_hip.SIGNATURES)
    lib = _hip.load()
    for n in names:
        assert getattr(lib, n) is not None
    assert int(re.search(r"#define\s+IFX_ABI_MINOR\s+(\d+)", hdr).group(1)) == 7 == _hip.ABI_MINOR == (lib.ifx_version() >> 8) & 255
    from inferix_amd import hip_ops
    for n in ("gemm_f32", "t5_attention_f32", "rmsnorm_f32", "t5_gated_gelu_f32"):
        assert callable(getattr(hip_ops, n))


def test_fp32_entry_points_refuse_what_they_are_not_built_for_without_a_gpu():
    """Validation happens before any launch: the refusals of the shape contract need no device."""
    from inferix_amd import _hip
    lib = _hip.load()
    p = 1 << 20      # never dereferenced
    for M, N, K in ((4, 64, 40), (4, 72, 64)):
        assert lib.ifx_gemm_f32(p, K, p, None, 0, p, N, M, N, K, 0, None) == -3
        assert b"K % 64" in lib.ifx_last_error()
    assert lib.ifx_gemm_f32(p, 64, p, None, 0, p, 64, 4, 64, 64, 3, None) == -1
    assert lib.ifx_rmsnorm_f32(p, 96, p, p, 96, 2, 96, 1e-6, None) == -3 and b"multiples of 64" in lib.ifx_last_error()
    assert lib.ifx_t5_attention_f32(p, 64, p, 64, p, 64, p, 64, p, p, 1, 1032, 1, 0, None) == -1
    assert lib.ifx_t5_attention_f32(p, 64, p, 64, p, 64, p, 64, p, p, 1, 20, 1, 0, None) == -1
    assert lib.ifx_t5_attention_f32(p, 64, p, 64, p, 64, p, 64, p, p, 1, 64, 1, 2, None) == -1
    assert lib.ifx_t5_gated_gelu_f32(p, p, 2, 6, None) == -1


def test_encoder_and_embedder_fail_loudly_off_the_gpu():
    from inferix_amd import _hip
    from inferix_amd.magi.t5 import HipT5Embedder, HipT5v11Encoder
    c = U.CASES["magi_t5_tiny"]
    W = U.make_weights(c)
    bad = dict(W)
    bad["encoder.block.0.layer.0.SelfAttention.q.weight"] = torch.zeros(2 * 32, c.d_model)
    with pytest.raises(NotImplementedError, match="head size 64"):
        HipT5v11Encoder(bad, device="cpu", **c.hip_kwargs())
    enc = HipT5v11Encoder(W, device="cpu", **c.hip_kwargs())
    ids, mask = U.make_inputs(c)
    with pytest.raises(_hip.HipKernelError, match="GPU only"):
        enc(ids, mask)
    with pytest.raises(ValueError, match="multiple of 8"):
        enc(ids[:, :50], mask[:, :50])
    with pytest.raises(RuntimeError, match="tokenizer"):
        HipT5Embedder(enc, None)
    with pytest.raises(TypeError):
        HipT5Embedder(object(), lambda *a, **k: None)


def test_reference_import_paths_resolve():
    from inferix.models.magi.t5 import T5Embedder
    from inferix.pipeline.magi.prompt_process import get_special_token_keys, get_txt_embeddings, pad_special_token
    from inferix.pipeline.magi.video_generate import InferenceInput, extract_feature_for_inference
    from inferix_amd.magi import prompt as P
    from inferix_amd.magi.t5 import HipT5Embedder
    assert T5Embedder is HipT5Embedder and InferenceInput is P.InferenceInput
    assert extract_feature_for_inference is P.extract_feature_for_inference and pad_special_token is P.pad_special_token
    assert callable(get_special_token_keys) and callable(get_txt_embeddings)
