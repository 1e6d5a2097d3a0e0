"""The harness of the MAGI row-kernel tests, judged on the CPU: the head-prep rule of magi_rows_util (`judge_head_prep`, the bars of
test_head_prep_vs_oracle) must accept an fp32 restatement of magi_head_prep_kernel's arithmetic at every rotary width, and must
reject every single-step departure from it — a second rounding of q, `w + 1` in the wrong dtype, a lost `+ 1`, the neighbouring
token's rotary row, a lost q scale, a ten times larger eps.  That is what proves the GPU tests of test_hip_magi_row_kernels.py can
fail.  Plus the facts about the quantiser references that make the every-bf16-value test able to tell `via_bf16` apart."""
import pytest
import torch

import magi_rows_util as U
from magi_rows_util import BF

ROWS = 37


@pytest.mark.parametrize("half", U.ROPE_HALVES)
def test_rule_accepts_the_restated_kernel_arithmetic(half):
    """(3, 1) and (2, 1) heads, q_scale 1 and the attention prescale, plain heads and heads at 40 +- 0.4 / low variance / constant."""
    worst = [0.0, 0.0, 0.0]
    for hq, hk in ((3, 1), (2, 1)):
        for plant in (None,) + U.PLANTS:
            inp = U.head_prep_inputs(ROWS, hq, hk, half, plant=plant)
            for q_scale in (1.0, U.Q_PRESCALE):
                ref = U.head_prep_reference(inp, q_scale)
                got = U.head_prep_restatement(inp, q_scale)
                U.judge_head_prep("cpu restatement", got, ref, what=f"{hq}/{hk} half {half} plant {plant} scale {q_scale:.4f}")
                assert all(torch.isfinite(got[n].float()).all() for n in ("q", "k", "qx"))
    U.report("cpu restatement")


def test_q_scale_zero_means_one_and_a_power_of_two_commutes_with_the_rounding():
    inp = U.head_prep_inputs(ROWS, 3, 1, 48)
    one = U.head_prep_reference(inp, 1.0)
    assert torch.equal(U.head_prep_reference(inp, 0.0)["q"], one["q"])
    assert torch.equal(U.head_prep_reference(inp, 0.5)["q"], (one["q"].float() * 0.5).to(BF))


@pytest.mark.parametrize("mutation", U.MUTATIONS)
def test_rule_rejects_every_single_step_departure(mutation):
    """Each mutation is judged on the output it touches, on the inputs the GPU tests use (37 rows, (3, 1) heads, half 48, the
    prescale); `eps_1e-5` on the input with the planted low-variance heads, where alone eps is visible."""
    plant = "low_variance" if mutation == "eps_1e-5" else None
    inp = U.head_prep_inputs(ROWS, 3, 1, 48, plant=plant)
    ref = U.head_prep_reference(inp, U.Q_PRESCALE)
    U.judge_head_prep(None, U.head_prep_restatement(inp, U.Q_PRESCALE), ref, what="unmutated")
    bad = U.head_prep_restatement(inp, U.Q_PRESCALE, mutation=mutation)
    touched = {"round_before_scale": ("q",), "w1p_bf16_qk": ("q", "k"), "w1p_fp32_qx": ("qx",), "drop_1p": ("q", "k", "qx"),
               "rope_row_off": ("q", "k"), "omit_scale": ("q",), "eps_1e-5": ("q", "k", "qx")}[mutation]
    for name in ("q", "k", "qx"):
        f = U.parity_figures(bad[name], ref[name], max_ulp=1, floor=1.0 if name in ("q", "k") else 0.05)
        print(f"{mutation} {name}: element error {f[0]:.2f} of the bound, {f[1]:.4f} of the elements differ, rel L2 {f[2]:.3f} of the bound")
        if name in touched:
            with pytest.raises(AssertionError):
                U.judge_head_prep(None, bad, ref, what=mutation, only=(name,))
        else:
            U.judge_head_prep(None, bad, ref, what=mutation, only=(name,))
    assert torch.equal(bad["v"], ref["v"])
    if mutation == "eps_1e-5":          # ordinary heads do not see eps at all: the same mutation passes without the planted heads
        plain = U.head_prep_inputs(ROWS, 3, 1, 48)
        U.judge_head_prep(None, U.head_prep_restatement(plain, U.Q_PRESCALE, mutation=mutation), U.head_prep_reference(plain, U.Q_PRESCALE))
    if mutation == "round_before_scale":
        assert U.parity_figures(bad["q"], ref["q"], max_ulp=1, floor=1.0)[1] > 0.1          # a second rounding: a large share differs


def test_rule_rejects_a_non_finite_result():
    inp = U.head_prep_inputs(ROWS, 3, 1, 48)
    ref = U.head_prep_reference(inp, U.Q_PRESCALE)
    bad = {n: t.clone() for n, t in U.head_prep_restatement(inp, U.Q_PRESCALE).items()}
    bad["k"][5, 0, 100] = float("nan")
    with pytest.raises(AssertionError):
        U.judge_head_prep(None, bad, ref)


def test_planted_heads_are_what_they_claim():
    g = torch.Generator().manual_seed(0)
    low = U.plant_head("low_variance", g).float()
    assert 1.2e-5 < float(low.var(unbiased=False)) < 1.6e-5 and set(low.tolist()) == {1.0, 1.0078125}
    assert float(U.plant_head("constant", g).float().var()) == 0.0
    off = U.plant_head("offset", g).float()
    assert abs(float(off.mean()) - 40.0) < 0.2 and 0.2 < float(off.std()) < 0.6
    for plant in U.PLANTS:          # planted into one q, one qx and one k slot of three rows; every other head unchanged
        a, b = U.head_prep_inputs(ROWS, 3, 1, 48), U.head_prep_inputs(ROWS, 3, 1, 48, plant=plant)
        changed = (a["mixed"].view(ROWS, 8, 128) != b["mixed"].view(ROWS, 8, 128)).any(-1)
        assert sorted(changed.nonzero().tolist()) == [[r, s] for r in (0, 18, 36) for s in (2, 5, 6)]


def test_quantiser_references_over_every_bf16_value():
    """The three facts behind the every-value test: the references yield no NaN byte (e4m3fn: 0x7f / 0xff) for any finite input and
    any of the divisors; the bf16 intermediate changes e4m3 bytes at divisors 0.03 and 1000 and int8 bytes at divisor 3.0 — a kernel
    that ignored `via_bf16` would fail there."""
    x = U.all_finite_bf16()
    assert x.shape == (120, 544) and bool(torch.isfinite(x.float()).all())
    assert x.view(torch.int16).unique().numel() == 65280
    divs = [torch.tensor([d]) for d in U.DIVISORS] + [U.cycling_divisor(544)]
    for d in divs:
        for via in (True, False):
            q = U.quant_reference(x, d, "e4m3", via)
            assert not bool(((q & 0x7F) == 0x7F).any()), (d[:5], via)
            assert int(q.max()) >= 0xFE and int((q == 0x7E).sum()) > 0                      # both +-448 are reached
    sep = {(fmt, d): int((U.quant_reference(x, torch.tensor([d]), fmt, True) != U.quant_reference(x, torch.tensor([d]), fmt, False)).sum())
           for fmt in ("e4m3", "int8") for d in U.DIVISORS}
    print(sep)
    assert sep[("e4m3", 0.03)] == 128 and sep[("e4m3", 1000.0)] == 120 and sep[("int8", 3.0)] == 126
    assert sep[("e4m3", 1.0)] == 0 and sep[("int8", 1.0)] == 0 and sep[("e4m3", 2.0 ** -10)] == 0       # exact quotients: one rounding
    cyc = U.cycling_divisor(544)
    assert cyc[:6].tolist() == [1.0, 0.029999999329447746, 3.0, 2.0 ** -10, 1000.0, 1.0]
    for fmt in ("e4m3", "int8"):
        assert int((U.quant_reference(x, cyc, fmt, True) != U.quant_reference(x, cyc, fmt, False)).sum()) > 0


def test_per_tensor_reference_and_window_helpers():
    z = torch.zeros(4, 16, dtype=BF)
    q, s = U.per_tensor_reference(z, "int8")
    assert float(s) == 1.0 and int(q.sum()) == 0
    x, _ = U.quant_rows(9, 520)
    for fmt in ("e4m3", "int8"):
        q, s = U.per_tensor_reference(x, fmt)
        assert float(s) == float(torch.tensor(40.0) / U.QMAX[fmt])
        assert int(q[0, 0]) == (0x7E if fmt == "e4m3" else 127) and int(q[-1, -1]) == (0xFE if fmt == "e4m3" else 0x81)
    buf, view = U.window(x, 16, U.NAN, device="cpu")
    assert buf.shape == (9, 576) and torch.equal(view, x) and bool(buf[:, :16].isnan().all()) and bool(buf[:, 536:].isnan().all())
    qb, qv = U.window(torch.zeros(9, 520, dtype=torch.uint8), 16, 0x5A, device="cpu")
    assert U.margins_intact(qb, 16, 520, 0x5A)
    qb[3, 536] = 0
    assert not U.margins_intact(qb, 16, 520, 0x5A)


def test_quantisers_refuse_row_strides_below_k_without_gpu():
    """ifx_quant_static / ifx_quant_per_tensor answer ldx < K and ldq < K before any launch (dummy aligned pointers, no GPU), as
    ifx_silu_and_mul and ifx_magi_gate_norm_residual do: with ldq < K rows would overwrite each other."""
    import ctypes as C
    from inferix_amd import _hip
    lib = _hip.load()
    P, EINVAL = C.c_void_p(16), -1

    def refused(rc, *parts):
        msg = lib.ifx_last_error()
        assert rc == EINVAL and all(p in msg for p in parts), (rc, msg)

    for fmt in (_hip.IFX_Q_FP8_E4M3, _hip.IFX_Q_INT8):
        # (x, ldx, q, ldq, divisor, divisor_len, row_scale, rows, K, format, via_bf16, stream)
        refused(lib.ifx_quant_static(P, 512, P, 520, P, 1, None, 4, 520, fmt, 1, None), b"ifx_quant_static", b"ldx (512)", b"K (520)")
        refused(lib.ifx_quant_static(P, 520, P, 512, P, 520, None, 4, 520, fmt, 0, None), b"ifx_quant_static", b"ldq (512)")
        refused(lib.ifx_quant_static(P, 0, P, 520, P, 1, None, 4, 520, fmt, 1, None), b"ldx (0)")
        # (x, ldx, q, ldq, row_scale, amax_workspace, rows, K, format, stream)
        refused(lib.ifx_quant_per_tensor(P, 512, P, 520, P, P, 4, 520, fmt, None), b"ifx_quant_per_tensor", b"ldx (512)", b"K (520)")
        refused(lib.ifx_quant_per_tensor(P, 520, P, 512, P, P, 4, 520, fmt, None), b"ifx_quant_per_tensor", b"ldq (512)")
        assert lib.ifx_quant_static(P, 520, P, 520, P, 1, None, 0, 520, fmt, 1, None) == 0          # rows == 0: nothing to launch
        assert lib.ifx_quant_per_tensor(P, 520, P, 520, P, P, 0, 520, fmt, None) == 0


def test_activation_bands_cover_every_value_once():
    x = U.all_finite_bf16().flatten()
    total = torch.zeros(x.numel(), dtype=torch.int32)
    for _, m in U.act_bands(x):
        total += m.int()
    assert bool((total == 1).all())
