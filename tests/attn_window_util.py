"""Case builder, exact reference and acceptance rule of the attention window tests (test_attn_window_oracle.py proves on the CPU
that the rule rejects every window-edge and kv-head error; test_hip_attention_windows.py applies it to the HIP launches).

A window is the logical keys [k0, k1) of a cache of `cap` keys; `hq` query heads share `hk` kv heads in groups of g = hq // hk
(query head h reads kv head h // g).  On random data one key too many or too few moves a row by O(1 / keys), inside every
rounding bound; `build_case` plants four rows per kv head that make each such error O(1):

  * in-window edges   k[k0] = 4 q[0, h],  k[k1 - 1] = 4 q[rows - 1, h]   (v random): rows 0 / rows - 1 of head h put nearly all
                      their weight on that key (score 4 |q|^2 / sqrt(128) ~ 45), so dropping it moves the row by ~|v| ~ 3;
  * decoys outside    k[k0 - 1] = 4 q[1, h],  k[k1] = 4 q[rows - 2, h], both with v = 64: including one moves the row by ~64;

with h = c g + g - 1, the LAST query head of kv head c's group, so that the mapping h % hk fails as well wherever it differs from
h // g.  Every other key of [0, cap) keeps finite random data (a MAGI cache holds stale rows there); the view builders put NaN
into every physical slot that no logical key maps to."""
import math

import torch

import wan_oracle as O
from util import rel_l2

BF = torch.bfloat16
HD = 128
NAN = float("nan")


def edge_head(c, hq, hk):
    g = hq // hk
    return c * g + g - 1


def plant(q, k, v, k0, k1):
    """The four edge rows per kv head, in place (`k`, `v` hold logical keys [0, cap))."""
    rows, hq, _ = q.shape
    cap, hk, _ = k.shape
    assert 0 <= k0 < k1 <= cap and hq % hk == 0
    for c in range(hk):
        h = edge_head(c, hq, hk)
        if rows >= 4:
            if k0 - 1 >= 0:
                k[k0 - 1, c], v[k0 - 1, c] = (4 * q[1, h].float()).to(BF), 64.0
            if k1 < cap:
                k[k1, c], v[k1, c] = (4 * q[rows - 2, h].float()).to(BF), 64.0
        k[k0, c] = (4 * q[0, h].float()).to(BF)
        k[k1 - 1, c] = (4 * q[rows - 1, h].float()).to(BF)
    return q, k, v


def build_case(rows, hq, hk, cap, k0, k1, seed):
    """CPU bf16 q [rows, hq, 128], k / v [cap, hk, 128]: random, with the edge rows of window [k0, k1) planted."""
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(rows, hq, HD, generator=g).to(BF)
    k = torch.randn(cap, hk, HD, generator=g).to(BF)
    v = torch.randn(cap, hk, HD, generator=g).to(BF)
    return plant(q, k, v, k0, k1)


def exact(q, k, v, k0, k1, q_call=None, scale=0.0):
    """(out64 [rows, hq, 128], lse64 [hq, rows], ref_bf): fp64 attention with LSE over keys [k0, k1), kv heads expanded to the query
    heads, and the yardstick — the reference's bf16 SDPA path on the same inputs.  A prescaled call (`q_call` = bf16(q * q_scale),
    attention scale `scale`) is judged on the bf16-rounded scaled q it was given; the yardstick stays the unscaled call."""
    g = q.shape[1] // k.shape[1]
    kw = k[k0:k1].repeat_interleave(g, dim=1)
    vw = v[k0:k1].repeat_interleave(g, dim=1)
    q64 = q if q_call is None else q_call.double() * (scale * math.sqrt(HD))
    out64, lse64 = O.attention_with_lse(q64[None], kw[None], vw[None])
    ref_bf = O.attention(q[None], kw[None], vw[None])
    return out64[0], lse64[0], ref_bf[0]


def figures(out, lse, out64, lse64, ref_bf):
    """The numbers `check` judges: errors of `out` and of the yardstick against fp64, the two bounds, and the LSE error (or None)."""
    out = out.detach().cpu()
    err = (out.double() - out64).abs().max().item()
    err_ref = (ref_bf.double() - out64).abs().max().item()
    f = {"err": err, "err_bound": 2 * err_ref + 4e-3,
         "rel": rel_l2(out, out64), "rel_bound": max(1.5 * rel_l2(ref_bf, out64), 3e-3),
         "lse": None if lse is None else (lse.detach().cpu().double() - lse64).abs().max().item()}
    if not math.isfinite(err):           # NaN compares false with everything: a non-finite result must not pass
        f["err"] = f["rel"] = math.inf
    if f["lse"] is not None and not math.isfinite(f["lse"]):
        f["lse"] = math.inf
    return f


def check(out, lse, out64, lse64, ref_bf, what=""):
    """The rule of `_attn_case` (test_hip_kernels.py) over all rows, the edge rows included: as close to exact attention as the
    reference's own bf16 path is (x2 + one bf16 ulp of the output scale), rel-L2 within 1.5x of it (at least 3e-3), LSE within 2e-3."""
    f = figures(out, lse, out64, lse64, ref_bf)
    assert f["err"] <= f["err_bound"], (what, "max|err|", f)
    assert f["rel"] <= f["rel_bound"], (what, "rel-L2", f)
    if lse is not None:
        assert f["lse"] < 2e-3, (what, "lse", f)
    return f


# ---- physical views of logical keys [0, cap): slots no logical key maps to hold NaN --------------------------------------------------
def contiguous_slots(k, v, pad=3):
    """(kc, vc): the logical keys followed by `pad` slots of capacity that no key of the window may touch."""
    fill = torch.full((pad,) + tuple(k.shape[1:]), NAN, dtype=BF)
    return torch.cat([k, fill]), torch.cat([v, fill])


def paged_slots(k, v, ps, seed=0, spare=2):
    """(kc, vc, table): pages of `ps` rows in a random order, `spare` pages unused; unused pages and the tail of the last page are NaN."""
    cap = k.shape[0]
    npg = (cap + ps - 1) // ps + spare
    perm = torch.randperm(npg, generator=torch.Generator().manual_seed(1000 + seed + ps))
    kc = torch.full((npg * ps,) + tuple(k.shape[1:]), NAN, dtype=BF)
    vc = torch.full_like(kc, NAN)
    t = torch.arange(cap)
    slot = perm[t // ps] * ps + t % ps
    kc[slot], vc[slot] = k, v
    return kc, vc, perm.to(torch.int32)


def segment_slots(k, v, split, delta):
    """(kc, vc): logical keys >= split live `delta` slots further on; the gap is NaN."""
    cap = k.shape[0]
    assert 0 < split < cap
    kc = torch.full((cap + delta,) + tuple(k.shape[1:]), NAN, dtype=BF)
    vc = torch.full_like(kc, NAN)
    kc[:split], vc[:split] = k[:split], v[:split]
    kc[split + delta:], vc[split + delta:] = k[split:], v[split:]
    return kc, vc
