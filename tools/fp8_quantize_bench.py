"""MX-FP8 operand quantisation: the torch chain against the fused HIP kernel.

Both paths run in one process, in alternation, selected per call by
RING_ATTN_NO_FUSED_QUANT.  One JSON line per shape:

  b 1, h 8, d 64 at 8k and 32k tokens; d 128 at 8k; 32 q / 4 kv heads at 8k
  (quantize_fp8 and end-to-end flash_attn_fp8, causal), and quantize_kv_cache
  at 128k keys (b 1, 8 kv heads, d 128).

    python tools/fp8_quantize_bench.py [--rounds 7] [--out FILE]

A time is the device-synchronised host time of --iters back-to-back calls
after a warm-up of the shape, per call; each record holds the median and the
min-max of --rounds such windows per path.  GB/s is the fused kernel's own
traffic (every input element read once, every output byte written once,
computed from the shapes) over its median time.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from ring_attention_amd.ops import fp8  # noqa: E402

ENV = "RING_ATTN_NO_FUSED_QUANT"


def window_us(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6


def ab(fn, rounds, iters):
    """{path: (median, min, max)} us of fn under the torch chain and the kernel."""
    times = {"torch": [], "fused": []}
    for path in times:                       # warm up both paths at this shape
        os.environ[ENV] = "1" if path == "torch" else ""
        for _ in range(3):
            fn()
    for _ in range(rounds):
        for path in times:
            os.environ[ENV] = "1" if path == "torch" else ""
            times[path].append(window_us(fn, iters))
    os.environ.pop(ENV, None)
    return {p: (statistics.median(t), min(t), max(t)) for p, t in times.items()}


def fmt(rec, key, stats):
    for path, (med, lo, hi) in stats.items():
        rec[f"{key}_{path}_us"] = round(med, 1)
        rec[f"{key}_{path}_minmax_us"] = [round(lo, 1), round(hi, 1)]


def quantize_bytes(nq, nk, h, hk, d):
    """bytes the fused quantize_fp8 moves at b = 1: bf16 in, e4m3 + e8m0 out"""
    nq_pad, nk_pad, kd = -(-nq // 256) * 256, -(-nk // 128) * 128, 64 if d <= 64 else 128
    read = 2 * d * (nq * h + 2 * nk * hk)
    data = kd * (nq_pad * h + 2 * nk_pad * hk)
    return read + data + data // 64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.rounds >= 7, "at least 7 rounds"
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    sink = open(args.out, "w") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    for n, h, hk, d in ((8192, 8, 8, 64), (32768, 8, 8, 64), (8192, 8, 8, 128),
                        (8192, 32, 4, 64)):
        torch.manual_seed(0)
        q = torch.randn(1, n, h, d, device="cuda", dtype=torch.bfloat16)
        k = torch.randn(1, n, hk, d, device="cuda", dtype=torch.bfloat16)
        v = torch.randn_like(k)
        rec = dict(op="quantize_fp8", n=n, h=h, hk=hk, d=d, rounds=args.rounds,
                   iters=args.iters)
        stats = ab(lambda: fp8.quantize_fp8(q, k, v), args.rounds, args.iters)
        fmt(rec, "quant", stats)
        nbytes = quantize_bytes(n, n, h, hk, d)
        rec["fused_bytes"] = nbytes
        rec["fused_GBps"] = round(nbytes / stats["fused"][0] / 1e3, 1)
        fmt(rec, "e2e", ab(lambda: fp8.flash_attn_fp8(q, k, v, causal=True),
                           args.rounds, args.iters))
        emit(rec)

    n, hk, d = 131072, 8, 128
    torch.manual_seed(0)
    k = torch.randn(1, hk, n, d, device="cuda", dtype=torch.bfloat16)
    v = torch.randn_like(k)
    rec = dict(op="quantize_kv_cache", n=n, hk=hk, d=d, rounds=args.rounds, iters=args.iters)
    stats = ab(lambda: fp8.quantize_kv_cache(k, v), args.rounds, args.iters)
    fmt(rec, "quant", stats)
    nbytes = 2 * hk * n * (2 * d + d + 1)
    rec["fused_bytes"] = nbytes
    rec["fused_GBps"] = round(nbytes / stats["fused"][0] / 1e3, 1)
    emit(rec)
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
