"""The harness of the attention window tests, judged on the CPU: `attn_window_util.check` must reject a result that is exact except
for ONE key too many or too few at a window edge, or for the kv-head mapping h % hk, and must accept the reference's own bf16
path.  This is what proves that the GPU tests of test_hip_attention_windows.py can fail."""
import pytest
import torch

import wan_oracle as O
from attn_window_util import BF, build_case, check, exact, figures

# (rows, hq, hk, cap, k0, k1): a window inside a tile and a page, a short cache, a window of one tile and a bit, a single key
SHAPES = [(129, 6, 2, 900, 137, 811), (33, 3, 1, 300, 5, 263), (257, 24, 8, 200, 1, 66), (4, 4, 4, 70, 3, 4)]


def _attend(q, k, v, keys, head_of):
    """fp64 attention of q over the logical keys `keys`, query head h reading kv head head_of(h); bf16 output, fp64 LSE."""
    hq = q.shape[1]
    idx = torch.tensor([head_of(h) for h in range(hq)])
    if len(keys) == 0:                    # every key masked: no weight anywhere
        return torch.zeros_like(q), torch.full((hq, q.shape[0]), float("-inf"), dtype=torch.float64)
    kw, vw = k[keys][:, idx], v[keys][:, idx]
    out, lse = O.attention_with_lse(q[None], kw[None], vw[None])
    return out[0].to(BF), lse[0]


@pytest.mark.parametrize("rows,hq,hk,cap,k0,k1", SHAPES)
def test_check_rejects_every_window_and_head_mutation(rows, hq, hk, cap, k0, k1):
    q, k, v = build_case(rows, hq, hk, cap, k0, k1, seed=11)
    assert torch.isfinite(k.float()).all() and torch.isfinite(v.float()).all()
    out64, lse64, ref_bf = exact(q, k, v, k0, k1)
    g = hq // hk
    right = lambda h: h // g
    # the unmutated fp64 result rounded to bf16, and the reference's own bf16 path, pass
    good, good_lse = _attend(q, k, v, list(range(k0, k1)), right)
    check(good, good_lse, out64, lse64, ref_bf)
    f = check(ref_bf, None, out64, lse64, ref_bf)
    assert f["err"] <= 0.5 * f["err_bound"] and f["rel"] <= f["rel_bound"] / 1.5 + 1e-12
    mutations = {
        "include k0 - 1": (list(range(k0 - 1, k1)), right),
        "include k1": (list(range(k0, k1 + 1)), right),
        "drop k0": (list(range(k0 + 1, k1)), right),
        "drop k1 - 1": (list(range(k0, k1 - 1)), right),
    }
    if any(h % hk != h // g for h in range(hq)):
        mutations["head h % hk"] = (list(range(k0, k1)), lambda h: h % hk)
    else:
        # one kv head, or as many as query heads: h % hk IS h // g, there is no wrong mapping of that form to tell apart
        assert hk == 1 or hk == hq
    for name, (keys, head_of) in mutations.items():
        bad, bad_lse = _attend(q, k, v, keys, head_of)
        f = figures(bad, bad_lse, out64, lse64, ref_bf)
        print(f"{name}: max|err| {f['err']:.3g} (bound {f['err_bound']:.3g}), rel-L2 {f['rel']:.3g} (bound {f['rel_bound']:.3g}), "
              f"lse {f['lse']:.3g}")
        # rejected by the output alone (strided and multi-range launches return no LSE), by each of its two clauses, and by the LSE
        assert f["err"] > f["err_bound"] and f["rel"] > f["rel_bound"] and not f["lse"] < 2e-3, (name, f)
        with pytest.raises(AssertionError):
            check(bad, None, out64, lse64, ref_bf, name)
        with pytest.raises(AssertionError):
            check(bad, bad_lse, out64, lse64, ref_bf, name)


def test_check_rejects_non_finite_results():
    q, k, v = build_case(5, 3, 1, 40, 3, 30, seed=2)
    out64, lse64, ref_bf = exact(q, k, v, 3, 30)
    bad = ref_bf.clone()
    bad[2, 1, 7] = float("nan")
    with pytest.raises(AssertionError):
        check(bad, None, out64, lse64, ref_bf)
    with pytest.raises(AssertionError):
        check(ref_bf, torch.full_like(lse64, float("nan")), out64, lse64, ref_bf)


def test_head_mutation_is_covered_by_the_grouped_shapes():
    """The mapping h % hk differs from h // g on the 6 / 2 and 24 / 8 shapes (the GPU tests use both head pairs throughout)."""
    assert sum(any(h % hk != h // (hq // hk) for h in range(hq)) for _, hq, hk, *_ in SHAPES) == 2
