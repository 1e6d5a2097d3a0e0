"""GPU: the first use of a big-LDS kernel from two host threads at once, and on a second device.

Every kernel that needs more dynamic LDS than the default opts in on its first launch, per kernel and per device
(inferix_amd/csrc/ifx_launch.h).  In a fresh process every kernel below is on its first use: two host threads, each on its own stream
and with its own output, meet at a barrier and issue the same call; the main thread issues it a third time afterwards.  The three
outputs have to be bit-identical and written (a thread that launched before the opt-in had returned would be refused, and leave its
output untouched).  The shapes are the smallest that still reach each family's big-LDS kernel.  tools/launch_check.cpp covers the same
rules on fake devices without a GPU; the second test here runs on real ones where the box has two.
Run on the MI355X box: pytest -m gpu."""
import hashlib
import threading
import traceback

import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
SENTINEL = 0x7FA5          # a bf16 NaN no kernel here writes


def _cases(ops, dev):
    """[(name, option, value, out_shape, call(out))] with the inputs on `dev` (seeded on the CPU: the same on every device)."""
    from inferix_amd import _hip
    from inferix_amd.t5 import relative_position_table
    from inferix_amd.vae import _repack_conv
    g = torch.Generator().manual_seed(16)

    def rnd(*shape, scale=1.0):
        return (torch.randn(*shape, generator=g) * scale).to(BF).to(dev)
    cases = []
    # 130 x 192 x 256: one full 128-row tile and a ragged one; N and K multiples of 64 (the ping-pong tile)
    x, w, b = rnd(130, 256), rnd(192, 256, scale=256 ** -0.5), rnd(192, scale=0.1)
    for v in (1, 3, 19, 24):
        cases.append((f"linear gemm_variant {v}", "gemm_variant", v, (130, 192), lambda out: ops.linear(x, w, b, out=out)))
    xq, sx = ops.quant_per_token(x, _hip.IFX_Q_FP8_E4M3)
    wq, sw = ops.quant_per_token(w, _hip.IFX_Q_FP8_E4M3)
    for v in (0, 22):
        cases.append((f"linear_q8 gemm_variant {v}", "gemm_variant", v, (130, 192),
                      lambda out: ops.linear_q8(xq, sx, wq, sw, b, _hip.IFX_Q_FP8_E4M3, out=out)))
    # 257 rows (one past the 256-row tile), 3 query heads on 1 kv head, 261 keys
    q, kv = rnd(257, 3, 128), ops.KvCacheView(rnd(261, 1, 128), rnd(261, 1, 128))
    for v in (2, 7):
        cases.append((f"attention attn_variant {v}", "attn_variant", v, (257, 3, 128), lambda out: ops.attention(q, kv, 261, out=out, splits=1)))
    # 3 x 3 x 3, 32 -> 96 channels, one frame of 8 x 64 pixels: the persistent kernel (0) and the lock-step one (1)
    frames, cw, cb = rnd(3, 8, 64, 32), _repack_conv(rnd(96, 32, 3, 3, 3, scale=864 ** -0.5)).to(dev), rnd(96, scale=0.1)
    for v in (0, 1):
        cases.append((f"conv3d_cl conv_variant {v}", "conv_variant", v, (1, 8, 64, 96),
                      lambda out: ops.conv3d_cl(frames, [0, 1, 2], cw, cb, kt=3, ks=3, y=out, out_slots=[0])))
    qkv, bias = rnd(128, 3 * 64, scale=0.6), relative_position_table(rnd(32, 1, scale=0.5).cpu(), 128, 32).to(dev)
    lens = torch.tensor([100], dtype=torch.int32, device=dev)
    cases.append(("t5_attention", None, 0, (128, 64), lambda out: ops.t5_attention(qkv[:, :64], qkv[:, 64:128], qkv[:, 128:], bias, lens, 1, 1, out=out)))
    return cases


def _run_cases(dev):
    """{case: sha256 of the output}; asserts, per case, that the two racing first calls and a third one wrote the same bits."""
    from inferix_amd import _hip, hip_ops as ops
    torch.cuda.set_device(dev)
    _hip.load()
    ops._zero_page(torch.device(dev))          # the Python side's own lazy page is not what is raced here
    digests = {}
    for name, option, value, shape, call in _cases(ops, dev):
        outs = [torch.full(shape, SENTINEL, dtype=torch.int16, device=dev).view(BF) for _ in range(3)]
        streams = [torch.cuda.Stream(dev) for _ in range(2)]
        torch.cuda.synchronize(dev)
        barrier, errors = threading.Barrier(2), []

        def first_use(i):
            try:
                torch.cuda.set_device(dev)
                with torch.cuda.stream(streams[i]):
                    barrier.wait()
                    call(outs[i])
            except BaseException:           # noqa: BLE001 - reported by the main thread
                errors.append(f"thread {i}: {traceback.format_exc()}")
                barrier.abort()
        previous = ops.get_option(option) if option else 0
        if option:
            ops.set_option(option, value)
        try:
            threads = [threading.Thread(target=first_use, args=(i,)) for i in range(2)]
            for t in threads:
                t.start()
            for t in threads:
                t.join()
            torch.cuda.synchronize(dev)
            assert not errors, f"{name} on {dev}: " + "\n".join(errors)
            call(outs[2])
            torch.cuda.synchronize(dev)
        finally:
            if option:
                ops.set_option(option, previous)
        ops.check_device(name)
        bits = [o.view(torch.int16).cpu() for o in outs]
        for i, o in enumerate(bits):
            assert not bool((o == SENTINEL).any()), f"{name} on {dev}: call {i} left {int((o == SENTINEL).sum())} of {o.numel()} elements unwritten"
        assert torch.equal(bits[0], bits[1]) and torch.equal(bits[0], bits[2]), f"{name} on {dev}: the three calls differ"
        digests[name] = hashlib.sha256(bits[0].numpy().tobytes()).hexdigest()
    return digests


def _child(devices, ret):
    try:
        ret.put(("ok", [_run_cases(dev) for dev in devices]))
    except BaseException:                   # noqa: BLE001 - the parent fails with the text
        ret.put(("failed", traceback.format_exc()))


def _in_fresh_process(devices):
    ctx = mp.get_context("spawn")
    ret = ctx.SimpleQueue()
    p = ctx.Process(target=_child, args=(devices, ret))
    p.start()
    p.join()
    assert p.exitcode == 0 and not ret.empty(), f"the child process ended with status {p.exitcode}"
    status, result = ret.get()
    assert status == "ok", result
    return result


def test_first_use_from_two_host_threads_at_once():
    (digests,) = _in_fresh_process(["cuda:0"])
    assert len(digests) == 11, sorted(digests)


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs a second device: the per-device opt-in on real devices (tools/launch_check.cpp covers it on fake ones)")
def test_first_use_on_a_second_device_of_one_process():
    first, second = _in_fresh_process(["cuda:0", "cuda:1"])
    assert len(first) == 11 and first == second, [k for k in first if first[k] != second.get(k)]
