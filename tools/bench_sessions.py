"""Concurrent sessions, measured: 1 / 2 / 4 / 8 live sessions of the full-size synthetic model (Wan 1.3B, 480p, blocks of 3 latent frames
= 4680 rows) at DIFFERENT positions of their videos, one block each per leg, three ways that alternate in one process:

    round_robin   every session's forwards at B = 1, one session after the other (what existed before SessionBatch)
    ragged        SessionBatch.step(): ragged forwards over all sessions, the self-attention launched per sample
    multi         the same with the samples' self-attention in one launch (ifx_attn_fwd_multi)
    ragged_again  `ragged` once more: the A/A pair that gives the run-to-run spread

    python tools/bench_sessions.py [--rounds 3] [--layers 30] [--sessions 1,2,4,8] [--out sessions.json]

A session's position is host integers (its block counter and the cache index state); after every leg they are put back, so all legs of a
session count run the SAME blocks at the SAME key counts (the caches' contents do not matter for the time).  Positions per session:
POSITIONS below (block index; key count after the block = (block + 1) * 4680), so a row of the table is comparable across modes,
not across session counts.  No frame streams: this measures the generator.  Per leg: wall time of one step (host clock, device
synchronised at both ends); reported: the median over the rounds as ms per session-block and aggregate latent frames / s.

The `attention` section times the launch alone at mixed key counts — 4 x 4680 rows x 12 heads over 4680, 14040, 23400 and 32760 keys,
q prescaled as the model makes it — as one multi launch against the four single launches, alternating, between a pair of events
(medians of `--attn-reps` repetitions, with the single launches measured twice for the spread)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WAN_1_3B = dict(patch_size=[1, 2, 2], text_len=512, in_dim=16, dim=1536, ffn_dim=8960, freq_dim=256, text_dim=4096, out_dim=16,
                num_heads=12, num_layers=30, eps=1e-6)
LATENT = [16, 60, 104]
BLOCK, FSL = 3, 1560
POSITIONS = [3, 0, 5, 1, 4, 2, 3, 0]          # the block session i is at (at most 6: the cache holds 7 blocks)


def build(layers):
    from inferix_amd.pipeline import SelfForcingPipeline
    from inferix_amd.wan import HipCausalWanModel, HipWanDiffusionWrapper
    from inferix_amd.wan.synthetic import synthetic_state_dict
    mk = dict(WAN_1_3B, num_layers=layers)
    model = HipCausalWanModel(**{**mk, "patch_size": tuple(mk["patch_size"])}, device="cuda:0")
    model.load_state_dict(synthetic_state_dict(model, seed=0))
    gen = HipWanDiffusionWrapper(model=model, timestep_shift=5.0)
    pe = torch.zeros(1, 512, 4096)
    pe[:, :40] = torch.randn(1, 40, 4096, generator=torch.Generator().manual_seed(1))
    pe = pe.to(torch.bfloat16).cuda()
    conf = dict(denoising_step_list=[1000, 750, 500, 250], warp_denoising_step=True, num_frame_per_block=BLOCK,
                independent_first_frame=False, context_noise=0, frame_seq_length=FSL, kv_cache_tokens=32760, latent_shape=LATENT)
    return SelfForcingPipeline(conf, text_encoder=lambda text_prompts: {"prompt_embeds": pe.expand(len(text_prompts), -1, -1)},
                               vae=None, generator=gen)


def place(session, block):
    """Put a session at `block` without generating what is in front of it: the host integers only."""
    session.block, session.frames_done = block, block * BLOCK
    for m in session.kv_meta:
        m["global_end_index"].fill_(block * BLOCK * FSL)
        m["local_end_index"].fill_(block * BLOCK * FSL)


def bench_sessions(pipe, counts, rounds):
    from inferix_amd.serving import SessionBatch
    model = pipe.pipeline.generator.model
    out = []
    for n in counts:
        sb = SessionBatch(pipe, max_sessions=n)
        sessions = [sb.open(f"session {i}", seed=i) for i in range(n)]
        where = POSITIONS[:n]

        def reset():
            for s, p in zip(sessions, where):
                place(s, p)

        def leg(mode):
            reset()
            model.attn_multi = mode == "multi"
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if mode == "round_robin":
                for s in sessions:
                    sb.sessions = [s]
                    sb.step()
                sb.sessions = list(sessions)
            else:
                sb.step()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3
        modes = ("round_robin", "ragged", "multi", "ragged_again")
        for mode in modes[:3]:                       # warm-up: the text K / V of every session, every launch shape once
            leg(mode)
        times = {m: [] for m in modes}
        for _ in range(rounds):
            for mode in modes:
                times[mode].append(leg(mode))
        rec = dict(sessions=n, positions=where, keys_after_block=[(p + 1) * BLOCK * FSL for p in where])
        for mode in modes:
            med = statistics.median(times[mode])
            rec[mode] = dict(step_ms=times[mode], median_step_ms=med, ms_per_session_block=med / n,
                             latent_frames_per_s=n * BLOCK / (med * 1e-3))
        rec["aa_spread"] = abs(rec["ragged_again"]["median_step_ms"] / rec["ragged"]["median_step_ms"] - 1.0)
        rec["ragged_vs_round_robin"] = rec["ragged"]["median_step_ms"] / rec["round_robin"]["median_step_ms"]
        rec["multi_vs_ragged"] = rec["multi"]["median_step_ms"] / rec["ragged"]["median_step_ms"]
        print(f"{n} sessions at blocks {where}: " + ", ".join(f"{m} {rec[m]['median_step_ms']:.1f} ms" for m in modes) +
              f"; A/A spread {100 * rec['aa_spread']:.2f} %", file=sys.stderr, flush=True)
        out.append(rec)
        model.attn_multi = True
        sb.close_all()
    return out


def bench_attention(reps):
    from inferix_amd import hip_ops as ops
    heads, rows, keys = 12, 4680, [4680, 14040, 23400, 32760]
    g = torch.Generator().manual_seed(0)
    q_scale, scale = ops.attn_q_prescale(128)
    items = []
    for nk in keys:
        q = (torch.randn(rows, heads * 128, generator=g) * q_scale).to(torch.bfloat16).cuda()
        k = torch.randn(32760, heads, 128, generator=g).to(torch.bfloat16).cuda()
        v = torch.randn(32760, heads, 128, generator=g).to(torch.bfloat16).cuda()
        items.append((q, ops.KvCacheView(k, v), nk, torch.empty_like(q)))

    def singles():
        for q, view, nk, o in items:
            ops.attention(q.view(rows, heads, 128), view, nk, scale=scale, out=o.view(rows, heads, 128))

    def multi():
        ops.attention_multi(items, heads, scale=scale)
    legs = dict(singles=singles, multi=multi, singles_again=singles)
    for fn in legs.values():
        fn()
    times = {k: [] for k in legs}
    for _ in range(reps):
        for name, fn in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3)
    flops = sum(4.0 * rows * nk * heads * 128 for nk in keys)
    rec = dict(rows=rows, heads=heads, keys=keys, reps=reps)
    for name, t in times.items():
        med = statistics.median(t)
        rec[name] = dict(median_us=med, min_us=min(t), tflops=flops / (med * 1e-6) / 1e12)
    rec["aa_spread"] = abs(rec["singles_again"]["median_us"] / rec["singles"]["median_us"] - 1.0)
    rec["multi_vs_singles"] = rec["multi"]["median_us"] / rec["singles"]["median_us"]
    print("attention alone: " + ", ".join(f"{k} {rec[k]['median_us']:.0f} us" for k in legs) + f"; A/A spread {100 * rec['aa_spread']:.2f} %",
          file=sys.stderr, flush=True)
    return rec


def place_interactive(session, block):
    """`place` for a session of an InteractiveSessionBatch: between two blocks, nothing queued, no prompt change pending."""
    place(session, block)
    session.position = session.frames_done
    session._queue, session._x, session._x0, session._pending = [], None, None, None


def bench_interactive(pipe, counts, rounds):
    """`--interactive`: what InteractiveSessionBatch adds, per count n of live sessions (the arriving one included), legs alternating:

    join      open() -> the new session's first finished block, its n - 1 neighbours at POSITIONS.  `step`: SessionBatch, the session
              joins at the next step (arrival exactly at a block boundary: the best case; `neighbour_step_ms` is the step of the n - 1
              neighbours it waits for when it arrives just after one began, the worst case).  `advance`: InteractiveSessionBatch, the
              neighbours two forwards into their block, the session in the next forward.  `step_again`: the A/A leg.
    prompt    set_prompt() on session 0 at a block boundary -> its first block under the new prompt (the prefill of 3 overlap frames
              and a block, beside neighbours that carry on).
    step      InteractiveSessionBatch.step() against SessionBatch.step() on the SAME sessions (`base`, `interactive`, `base_again`)."""
    from inferix_amd.serving import InteractiveSessionBatch, SessionBatch
    out = []
    for n in counts:
        ib = InteractiveSessionBatch(pipe, max_sessions=n)
        base = SessionBatch(pipe, max_sessions=n)
        base.kvm, base.sessions = ib.kvm, ib.sessions        # one set of sessions behind both classes; sessions are opened through `ib`
        where = POSITIONS[:n]
        sessions = [ib.open(f"session {i}", seed=i) for i in range(n)]

        def reset():
            for s, p in zip(sessions, where):
                place_interactive(s, p)

        def timed(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3

        # ---- step against step ------------------------------------------------------------------------------------------------
        def step_leg(mode):
            reset()
            return timed(ib.step if mode == "interactive" else base.step)
        modes = ("base", "interactive", "base_again")
        for mode in modes[:2]:
            step_leg(mode)
        step_ms = {m: [] for m in modes}
        for _ in range(rounds):
            for mode in modes:
                step_ms[mode].append(step_leg(mode))
        rec = dict(sessions=n, positions=where)
        rec["step"] = {m: dict(step_ms=t, median_step_ms=statistics.median(t)) for m, t in step_ms.items()}
        rec["step"]["aa_spread"] = abs(rec["step"]["base_again"]["median_step_ms"] / rec["step"]["base"]["median_step_ms"] - 1.0)
        rec["step"]["interactive_vs_base"] = rec["step"]["interactive"]["median_step_ms"] / rec["step"]["base"]["median_step_ms"]

        # ---- prompt change ----------------------------------------------------------------------------------------------------
        def prompt_leg():
            reset()                                          # session 0 retains its last block's latents from the legs above

            def run():
                ib.set_prompt(sessions[0], "another prompt")
                while sessions[0] not in ib.advance():
                    pass
            return timed(run)
        prompt_leg()
        t = [prompt_leg() for _ in range(rounds)]
        rec["prompt"] = dict(ms=t, median_ms=statistics.median(t), forwards=1 + len(pipe.pipeline.denoising_step_list) + 1)

        # ---- join -------------------------------------------------------------------------------------------------------------
        ib.close(sessions.pop())                             # n - 1 neighbours; the n-th session arrives in every leg
        where = where[:n - 1]

        def join_leg(mode):
            reset()
            if mode == "advance":
                ib.advance(), ib.advance()                   # the neighbours are two forwards into their block
            new = []

            def run():
                new.append(ib.open("a new viewer", seed=99))
                if mode == "advance":
                    while new[0] not in ib.advance():
                        pass
                else:
                    base.step()
            ms = timed(run)
            ib.close(new[0])
            return ms
        modes = ("step", "advance", "step_again")
        for mode in modes[:2]:
            join_leg(mode)
        join_ms = {m: [] for m in modes}
        wait_ms = []
        for _ in range(rounds):
            for mode in modes:
                join_ms[mode].append(join_leg(mode))
            if n > 1:
                reset()
                wait_ms.append(timed(base.step))
        rec["join"] = {m: dict(ms=t, median_ms=statistics.median(t)) for m, t in join_ms.items()}
        rec["join"]["aa_spread"] = abs(rec["join"]["step_again"]["median_ms"] / rec["join"]["step"]["median_ms"] - 1.0)
        rec["join"]["neighbour_step_ms"] = statistics.median(wait_ms) if wait_ms else 0.0
        rec["join"]["step_worst_case_ms"] = rec["join"]["step"]["median_ms"] + rec["join"]["neighbour_step_ms"]
        print(f"{n} sessions: step base {rec['step']['base']['median_step_ms']:.1f} / interactive "
              f"{rec['step']['interactive']['median_step_ms']:.1f} ms (A/A {100 * rec['step']['aa_spread']:.2f} %); set_prompt -> block "
              f"{rec['prompt']['median_ms']:.1f} ms; open -> block: step {rec['join']['step']['median_ms']:.1f} .. "
              f"{rec['join']['step_worst_case_ms']:.1f} ms, advance {rec['join']['advance']['median_ms']:.1f} ms "
              f"(A/A {100 * rec['join']['aa_spread']:.2f} %)", file=sys.stderr, flush=True)
        out.append(rec)
        ib.close_all()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--layers", type=int, default=30)
    ap.add_argument("--sessions", default="1,2,4,8")
    ap.add_argument("--attn-reps", type=int, default=20)
    ap.add_argument("--interactive", default=None, metavar="COUNTS",
                    help="the InteractiveSessionBatch legs at these session counts (e.g. 1,4,8) INSTEAD of the sections above")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.manual_seed(0)
    if a.interactive:
        pipe = build(a.layers)
        result = dict(device=torch.cuda.get_device_name(0), layers=a.layers,
                      interactive=bench_interactive(pipe, [int(x) for x in a.interactive.split(",")], a.rounds))
    else:
        result = dict(device=torch.cuda.get_device_name(0), layers=a.layers, attention=bench_attention(a.attn_reps))
        pipe = build(a.layers)
        result["sessions"] = bench_sessions(pipe, [int(x) for x in a.sessions.split(",")], a.rounds)
    text = json.dumps(result)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
