#!/usr/bin/env python3
"""TEST INFRASTRUCTURE — generates the fixtures of the fp32 T5 caption encoder and of the MAGI caption packing:
tests/golden/magi_t5_tiny*.npz, magi_t5_long*.npz, magi_prompt_pack*.npz and magi_special_tokens.npz.

Encoder.  The class the reference instantiates (inferix/models/magi/t5/t5_model.py:126), HuggingFace's `T5EncoderModel`, is built from a
`T5Config` (nothing is fetched: HF_HUB_OFFLINE=1), loaded with the seeded weights of tests/magi_t5_util.py and run on the CPU in fp32:
`hf32` and the hidden state after every block.  The exact answer, `exact64`, is the float64 evaluation of the restatement
`magi_t5_util.encoder_forward` — NOT `model.double()`, whose `T5LayerNorm` keeps fp32 statistics (printed here: how far that sits from
the true fp64 evaluation).  The restatement in fp32 is asserted against HF's fp32 output: two fp32 evaluations of one formula, so it must
sit no further from HF's output than HF's output sits from the exact answer (RESTATEMENT_FRACTION).

Packing.  The reference's own `pad_special_token` / `_pad_special_token` (inferix/pipeline/magi/prompt_process.py) and
`_process_txt_embeddings` / `_process_null_embeddings` / `extract_feature_for_inference` (inferix/pipeline/magi/video_generate.py) run on
the CPU through oracle/_refstub.py, with SPECIAL_TOKEN_PATH pointed at the synthetic token file and the `cuda:N` device string they
build mapped to the CPU for the duration of the call.  A function that cannot be imported here is reported and the case is pinned to
the port's restatement only (DESIGN §3f names which).

usage (build container only; the reference tree must exist):  python tools/gen_golden_magi_t5.py
"""
from __future__ import annotations

import os
import sys
import warnings

os.environ["HF_HUB_OFFLINE"] = "1"

import torch  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _refstub  # noqa: E402
import magi_t5_util as U  # noqa: E402

RESTATEMENT_FRACTION = 1.0     # rel_l2(restatement fp32, hf32) <= this x rel_l2(hf32, exact64): two fp32 evaluations of one formula


def build_encoder(name: str) -> None:
    from transformers import T5Config, T5EncoderModel
    c = U.CASES[name]
    cfg = T5Config(vocab_size=c.vocab, d_model=c.d_model, d_kv=c.d_kv, d_ff=c.d_ff, num_layers=c.num_layers, num_heads=c.num_heads,
                   relative_attention_num_buckets=c.num_buckets, relative_attention_max_distance=c.max_distance,
                   feed_forward_proj="gated-gelu", layer_norm_epsilon=c.eps, is_encoder_decoder=False, use_cache=False,
                   tie_word_embeddings=False)
    model = T5EncoderModel(cfg).float().eval()
    W32 = U.make_weights(c, torch.float32)
    res = model.load_state_dict(W32, strict=False)
    tied = {"encoder.embed_tokens.weight", "shared.weight"}
    assert set(res.missing_keys) <= tied and set(res.unexpected_keys) <= tied, res
    assert torch.equal(model.get_input_embeddings().weight, W32["shared.weight"])
    ids, mask = U.make_inputs(c)
    with torch.no_grad():
        out = model(input_ids=ids, attention_mask=mask, output_hidden_states=True)
        hf32 = out.last_hidden_state
        # hidden_states: the embedding, then the state after every block; HF applies the final norm to the last entry it returns
        hf_blocks = [h for h in out.hidden_states[1:]]
    taps32, taps64 = [], []
    mine32 = U.encoder_forward(W32, c, ids, mask, taps32)
    W64 = U.make_weights(c, torch.float64)
    exact64 = U.encoder_forward(W64, c, ids, mask, taps64)
    with torch.no_grad():
        hf_double = model.double()(input_ids=ids, attention_mask=mask).last_hidden_state
    model.float()
    d_hf, d_mine = U.rel_l2(hf32, exact64), U.rel_l2(mine32, hf32)
    assert d_mine <= RESTATEMENT_FRACTION * d_hf, f"{name}: the fp32 restatement sits {d_mine:.3e} from HF's output, HF {d_hf:.3e} from exact"
    fx = {"ids": ids, "mask": mask, "hf32": hf32.contiguous(), "exact64": exact64.contiguous(),
          "restatement_fraction": torch.tensor(RESTATEMENT_FRACTION, dtype=torch.float64)}
    # per block: HF's fp32 state where HF exposes the un-normed one (all but the last), else the fp32 restatement's
    for i in range(c.num_layers):
        last = i == c.num_layers - 1
        b32 = taps32[i] if last else hf_blocks[i]
        if not last:
            assert U.rel_l2(taps32[i], hf_blocks[i]) <= RESTATEMENT_FRACTION * max(U.rel_l2(hf_blocks[i], taps64[i]), 1e-9), (name, i)
        fx[f"block{i}_ref32"] = b32.contiguous()
        fx[f"block{i}_exact64"] = taps64[i].contiguous()
    paths = U.save_parts(name, fx)
    print(f"{name}: wrote {len(paths)} file(s), {sum(os.path.getsize(p) for p in paths)} bytes; hf32 vs exact64 {d_hf:.3e}, "
          f"restatement32 vs hf32 {d_mine:.3e}, model.double() vs exact64 {U.rel_l2(hf_double, exact64):.3e}")


class cuda_strings_to_cpu:
    """The reference builds f"cuda:{torch.cuda.current_device()}" and moves tokens there: send such strings to the CPU meanwhile."""

    def __enter__(self):
        self.orig = torch.Tensor.to
        orig = self.orig

        def to(t, *a, **k):
            a = tuple("cpu" if isinstance(x, str) and x.startswith("cuda") else x for x in a)
            if isinstance(k.get("device"), str) and k["device"].startswith("cuda"):
                k["device"] = "cpu"
            return orig(t, *a, **k)

        torch.Tensor.to = to
        return self

    def __exit__(self, *exc):
        torch.Tensor.to = self.orig
        return False


def import_reference_packing(token_path: str):
    """(prompt_process, video_generate) of the reference, or (module, None) when video_generate cannot be imported here."""
    import importlib
    os.environ["SPECIAL_TOKEN_PATH"] = token_path
    _refstub.install_magi()
    # the two functions' modules only: the packages' own __init__ import the whole pipeline (VAE, ffmpeg, flash-attn entry points the
    # stand-ins do not have), so the packages are entered as bare path holders
    import types
    for pkg in ("inferix.pipeline", "inferix.pipeline.magi"):
        m = types.ModuleType(pkg)
        m.__path__ = [os.path.join(_refstub.REFERENCE_ROOT, *pkg.split("."))]
        sys.modules[pkg] = m
    pp = importlib.import_module("inferix.pipeline.magi.prompt_process")
    assert pp.__file__.startswith(_refstub.REFERENCE_ROOT), pp.__file__
    try:
        vg = importlib.import_module("inferix.pipeline.magi.video_generate")
        vg.print_rank_0 = lambda *a, **k: None
    except Exception as e:      # noqa: BLE001
        print(f"NOTE: the reference's video_generate does not import here ({type(e).__name__}: {e}); its three functions are pinned to "
              "the restatement of inferix_amd/magi/prompt.py only")
        vg = None
    return pp, vg


def build_packing() -> None:
    token_path = U.write_special_tokens(os.path.join(U.GOLDEN_DIR, "magi_special_tokens.npz"))
    assert os.path.getsize(token_path) <= U.FILE_LIMIT
    pp, vg = import_reference_packing(token_path)
    fx = {"from_reference": torch.tensor(1 if vg is not None else 0)}
    for name, c in U.PACK_CASES.items():
        model = U.pack_model(c)
        prefix, embs, mask = U.pack_inputs(c)
        with U.pack_env(c, token_path), cuda_strings_to_cpu(), torch.no_grad():
            keys = pp.get_special_token_keys()
            neg = pp.get_negative_special_token_keys()
            # pad_special_token on its own, on two chunks of the raw embeddings
            e2, m2 = pp.pad_special_token(keys, embs.repeat(1, 2, 1, 1), mask.unsqueeze(1).repeat(1, 2, 1))
            if vg is not None:
                ii = vg.extract_feature_for_inference(model, prefix, embs.clone(), mask.clone())
            else:
                sys.path.insert(0, ROOT)
                from inferix_amd.magi import prompt as P
                ii = P.extract_feature_for_inference(model, prefix, embs.clone(), mask.clone(), P.load_special_tokens(token_path))
        fx[f"{name}.pad2.embs"], fx[f"{name}.pad2.masks"] = e2.contiguous(), m2.contiguous()
        for k in U.PACK_FIELDS:
            fx[f"{name}.{k}"] = getattr(ii, k).clone().contiguous()
        fx[f"{name}.latent_size"] = torch.tensor(ii.latent_size)
        fx[f"{name}.scalars"] = torch.tensor([ii.num_steps, ii.chunk_num, ii.report_chunk_num_list[0], ii.task_idx_list[0]])
        print(f"pack {name}: keys {keys} neg {neg} y {tuple(ii.y.shape)} masks {tuple(ii.emb_masks.shape)} {ii.emb_masks.dtype} "
              f"latent {ii.latent_size} chunks {ii.chunk_num}")
    paths = U.save_parts("magi_prompt_pack", fx)
    print(f"packing: wrote {len(paths)} file(s), {sum(os.path.getsize(p) for p in paths)} bytes")


def main():
    if not _refstub.available():
        raise SystemExit("reference tree not available: fixtures can only be generated in the build container")
    warnings.filterwarnings("ignore")
    torch.set_num_threads(1)          # one summation order for every regeneration
    for name in U.CASES:
        build_encoder(name)
    build_packing()


if __name__ == "__main__":
    main()
