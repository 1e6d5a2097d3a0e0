"""CPU: the gated-MLP (SwiGLU, `gated_linear_unit`: the MAGI-24B configs) fixtures and the host side of `ifx_silu_and_mul`.
The fixtures tests/golden/magi_block_{gated_tiny,gated_fp8_tiny,24b}* hold what the reference's own gated `TransformerLayer` computed
on the CPU (tools/gen_golden_magi_gated.py); the first test guards them, the second fails without the kernel."""
import ctypes as C
import os
import re

import pytest
import torch

import magi_block_oracle as MB
from magi_gated_util import GATED_FIXTURES, gated_geometry, gated_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF = torch.bfloat16


@pytest.mark.parametrize("name", GATED_FIXTURES)
def test_gated_oracle_reproduces_the_reference_fixture_bit_for_bit(name):
    """oracle/magi_block_oracle.py with `gated_linear_unit=True` against every stored output, intermediate tensor and cache row."""
    fx = gated_golden(name)
    cfg, n_layers, clip, n_calls, wseed, max_tokens = gated_geometry(fx)
    fp8 = bool(int(fx["fp8_quant"]))
    Ws = [MB.init_layer_weights(cfg, wseed + li, fp8=fp8 and MB.layer_is_fp8(li, max(n_layers, 3))) for li in range(n_layers)]
    assert Ws[0]["mlp.linear_fc1.weight"].shape[-2] == 2 * cfg.ffn_hidden_size
    caches = [MB.MagiLayerCache(max_tokens, cfg.num_query_groups, cfg.kv_channels) for _ in range(n_layers)]
    n_taps = 0
    for ci in range(n_calls):
        inp, m = MB.fixture_call(fx, ci)
        x = inp["x"]
        for li in range(n_layers):
            taps = {} if li == 0 else None
            x = MB.layer_forward(Ws[li], cfg, x, inp["condition"], inp["condition_map"], inp["y"], inp["rope"], m, caches[li], taps)
            assert torch.equal(x, fx[f"c{ci}_out_l{li}"]), (name, ci, li)
            if li == 0:
                for t, v in taps.items():
                    if f"c{ci}_tap_{t}" in fx:
                        assert torch.equal(v, fx[f"c{ci}_tap_{t}"]), (name, ci, t)
                        n_taps += 1
    assert n_taps > 0
    written = int(fx["cache_written"])
    assert written > 0
    for li in range(n_layers):
        c = fx[f"cache_l{li}"]
        assert torch.equal(c[0, :written, 0], caches[li].k[:written]) and torch.equal(c[1, :written, 0], caches[li].v[:written]), (name, li)


def test_no_fixture_file_is_above_the_size_limit():
    golden = os.path.join(ROOT, "tests", "golden")
    for f in os.listdir(golden):
        if f.startswith(GATED_FIXTURES):
            assert os.path.getsize(os.path.join(golden, f)) <= 1 << 20, f


def test_silu_and_mul_export_and_argument_checks_without_gpu():
    """`ifx_silu_and_mul` is declared, bound and exported without an ABI bump, and every argument check answers before any launch
    (dummy aligned pointers, no GPU); the widths of the LayerNorm ladder's new rung are named by its refusal."""
    from inferix_amd import _hip
    from inferix_amd import hip_ops as ops
    hdr = open(os.path.join(ROOT, "include", "inferix_hip.h")).read()
    assert re.search(r"\bint ifx_silu_and_mul\(", hdr) and "ifx_silu_and_mul" in _hip.SIGNATURES
    lib = _hip.load()
    assert lib.ifx_silu_and_mul is not None
    assert (lib.ifx_version() >> 8) & 255 == 7 and re.search(r"#define IFX_ABI_MINOR 7\b", hdr)
    P = C.c_void_p(16)
    EINVAL, EUNSUP = -1, -3

    def refused(rc, code, *parts):
        msg = lib.ifx_last_error()
        assert rc == code and all(p in msg for p in parts), (rc, msg)

    f = lib.ifx_silu_and_mul            # (x, ldx, y, ldy, q, ldq, divisor, divisor_len, rows, f, stream)
    refused(f(P, 200, P, 104, None, 0, None, 0, 4, 100, None), EINVAL, b"ifx_silu_and_mul", b"f (100)")
    refused(f(P, 256, P, 128, None, 0, None, 0, 4, 0, None), EINVAL, b"f (0)")
    refused(f(P, 248, P, 128, None, 0, None, 0, 4, 128, None), EINVAL, b"ifx_silu_and_mul", b"ldx (248)")      # ldx < 2f
    refused(f(P, 260, P, 128, None, 0, None, 0, 4, 128, None), EINVAL, b"ldx (260)")                          # not a multiple of 8
    refused(f(P, 256, P, 120, None, 0, None, 0, 4, 128, None), EINVAL, b"ldy (120)")
    refused(f(P, 256, None, 0, P, 120, P, 128, 4, 128, None), EINVAL, b"ldq (120)")
    refused(f(P, 256, None, 0, P, 128, None, 0, 4, 128, None), EINVAL, b"ifx_silu_and_mul", b"divisor")      # q without divisor
    refused(f(P, 256, P, 128, None, 0, P, 128, 4, 128, None), EINVAL, b"divisor")                             # divisor without q
    refused(f(P, 256, None, 0, P, 128, P, 64, 4, 128, None), EINVAL, b"divisor_len 64")
    refused(f(P, 256, None, 0, None, 0, None, 0, 4, 128, None), EINVAL, b"ifx_silu_and_mul", b"neither y nor q")
    refused(f(None, 256, P, 128, None, 0, None, 0, 4, 128, None), EINVAL, b"ifx_silu_and_mul")
    refused(f(C.c_void_p(8), 256, P, 128, None, 0, None, 0, 4, 128, None), EINVAL, b"aligned")
    assert f(P, 256, P, 128, P, 128, P, 1, 0, 128, None) == 0                                                 # rows == 0: nothing to launch
    with pytest.raises(_hip.HipKernelError):
        ops.silu_and_mul(torch.zeros(2, 16, dtype=BF))
    # the LayerNorm ladder: the refusal names the new limit; beyond it, and between the rungs above 5120, IFX_EUNSUP as before
    for dim in (6152, 6656, 5128):
        refused(lib.ifx_layernorm(P, P, 4, dim, 1e-6, 0, None, None, None, 0, 0, 0, 1, None), EUNSUP, b"6144", str(dim).encode())
    refused(lib.ifx_layernorm_quant_static(P, P, 6152, P, 1, 4, 6152, 1e-6, 0, None, None, 1, None), EUNSUP, b"6144", b"6152")
    refused(lib.ifx_rmsnorm(P, 6144, P, 6144, P, 4, 6144, 1e-6, None), EUNSUP, b"5120", b"6144")              # LayerNorm-only rung


def test_gated_layer_and_24b_settings_construct():
    """The layer no longer refuses `gated_linear_unit`, and the reference's 24B model settings (example/magi/configs/24B: hidden 6144,
    ffn 16384, 48 heads on 8 groups, in / out channels 32 with half_channel_vae, x_rescale_factor 0.1, gated MLP) construct the model
    and its layer stack; no GPU is touched before weights are loaded."""
    from types import SimpleNamespace
    from inferix_amd.magi.dit import HipMagiTransformerLayer
    from inferix_amd.magi.model import HipVideoDiTModel
    mc = SimpleNamespace(num_layers=48, hidden_size=6144, ffn_hidden_size=16384, num_attention_heads=48, num_query_groups=8, kv_channels=128,
                         layernorm_epsilon=1e-6, apply_layernorm_1p=True, gated_linear_unit=True, params_dtype=BF, patch_size=2,
                         t_patch_size=1, in_channels=32, out_channels=32, caption_channels=4096, caption_max_length=800,
                         cond_hidden_ratio=0.25, xattn_cond_hidden_ratio=1.0, cond_gating_ratio=1.0, x_rescale_factor=0.1,
                         half_channel_vae=True)
    for fp8 in (False, True):
        ec = SimpleNamespace(cp_size=1, cp_strategy="none", fp8_quant=fp8, kv_offload=False, ulysses_overlap_degree=1, distill=False)
        layer = HipMagiTransformerLayer(mc, ec, 1, "cpu")
        assert layer.gated and layer.self_attention.adapt_linear_quant == fp8
        model = HipVideoDiTModel(SimpleNamespace(model_config=mc, engine_config=ec, runtime_config=None), "cpu")
        assert model.half_channel_vae and model.in_channels == 32
