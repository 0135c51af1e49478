"""Paged decode step vs the dense decode step (bench.py --config 5 shape).

Times the LOCAL step (partial kernel + fused chunk merge) of
  dense : _local_decode_partial / decode_partial_fp8 on a (b, hk, n, d) cache
  paged : _local_paged_decode_partial on a PagedKVCache holding the same tokens
for page_size in {16, 64, 256} with identity and shuffled block tables, bf16
and fp8, plus one ragged batch (b = 8, lengths 1k .. 128k) that the dense path
can only serve padded to the longest sequence.  Every paged configuration
is timed with the binding's own workgroup order and with the other one forced
(RING_ATTN_PAGED_ORDER).

Dense and paged measurements ALTERNATE inside every round (the box is shared)
and the median over the rounds is reported; each measurement is `--iters`
steps between two device events after a warm-up.

`--window W [W ...]` adds the sliding-window groups: one sequence with
`--kv-len` keys cached, decoded with `window=W`, against an UNWINDOWED step
over a cache that holds exactly W + 1 keys (the same keys: the windowed row
attends W + 1 of them), bf16 and fp8, every page size, alternating in the same
rounds.  `vs_short` is windowed / short.  `--only-window` skips the dense
groups.

    python tools/paged_decode_bench.py [--kv-len 131072] [--rounds 7] [--out F]
        [--window 1024 4096 32768] [--only-window]
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ring_attention_amd import PagedKVCache                       # noqa: E402
from ring_attention_amd.ops import hip_ext                        # noqa: E402
from ring_attention_amd.ops.fp8 import quantize_kv_cache          # noqa: E402
from ring_attention_amd.tree_decode import (                      # noqa: E402
    _local_decode_partial,
    _local_paged_decode_partial,
)


def time_us(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    start = torch.cuda.Event(enable_timing=True)
    end = torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / iters


def dense_step(q, k, v, fp8):
    if not fp8:
        return lambda: _local_decode_partial(q, k, v)
    ext = hip_ext.require()
    c = quantize_kv_cache(k, v)
    scale = q.shape[-1] ** -0.5

    def step():
        return ext.decode_merge(*ext.decode_partial_fp8(q, *c, scale))
    return step


def ordered(fn, order):
    """Same step with the workgroup order forced: "row" = the dense kernels'
    (row block fast, kv chunk slow), "chunk" = kv chunk fast.  Unforced, the
    binding picks row for b == 1 and chunk for b > 1."""
    def step():
        os.environ["RING_ATTN_PAGED_ORDER"] = order
        try:
            return fn()
        finally:
            del os.environ["RING_ATTN_PAGED_ORDER"]
    return step


def run_group(name, steps, args, results, note="", base_of=None, ratio="vs_dense"):
    """steps: {label: fn}; alternates all of them for `rounds` rounds.
    `base_of(label)` names the step a label is compared with (default
    "dense"); the ratio of the medians is recorded under `ratio`."""
    samples = {label: [] for label in steps}
    for _ in range(args.rounds):
        for label, fn in steps.items():
            samples[label].append(time_us(fn, args.iters, args.warmup))
    for label, xs in samples.items():
        med = statistics.median(xs)
        base = statistics.median(samples[base_of(label) if base_of else "dense"])
        rec = {"group": name, "config": label, "median_us": round(med, 2),
               "min_us": round(min(xs), 2), "max_us": round(max(xs), 2),
               ratio: round(med / base, 3), "rounds": len(xs), "note": note}
        results.append(rec)
        print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kv-len", type=int, default=131072)
    ap.add_argument("--heads", type=int, default=8)
    ap.add_argument("--kv-heads", type=int, default=None)
    ap.add_argument("--d-head", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--page-sizes", type=int, nargs="+", default=[16, 64, 256])
    ap.add_argument("--window", type=int, nargs="*", default=[],
                    help="also time a windowed step over --kv-len cached keys "
                         "against an unwindowed step over window + 1 keys")
    ap.add_argument("--only-window", action="store_true",
                    help="skip the dense-vs-paged groups")
    ap.add_argument("--out", default=None, help="also write the records here (JSON)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "paged_decode_bench needs a GPU"
    hip_ext.require()
    dev, bf = "cuda", torch.bfloat16
    n, h, d = args.kv_len, args.heads, args.d_head
    hk = args.kv_heads or h
    results = []

    def paged_steps(q, k, v, lens, fp8, tables, forced):
        """{label: step} for every page size x table kind, each with the
        binding's own order and once more with the `forced` order."""
        steps = {}
        for ps in args.page_sizes:
            for kind in tables:
                cache = PagedKVCache.from_dense(
                    k, v, lens, ps, fp8=fp8,
                    shuffle_seed=7 if kind == "shuffled" else None)
                fn = (lambda c=cache: _local_paged_decode_partial(q, c))
                steps[f"paged ps={ps} {kind}"] = fn
                steps[f"paged ps={ps} {kind} order={forced}"] = ordered(fn, forced)
        return steps

    def check(steps):
        # paged == dense on the same tokens before anything is timed
        ref = steps["dense"]()[0]
        for label, fn in steps.items():
            err = (fn()[0] - ref).abs().max().item()
            assert err < 5e-3, (label, err)

    # ---- one sequence: the config-5 shape ---------------------------------
    torch.manual_seed(1234)
    q = torch.randn(1, h, 1, d, device=dev, dtype=bf)
    k = torch.randn(1, hk, n, d, device=dev, dtype=bf)
    v = torch.randn(1, hk, n, d, device=dev, dtype=bf)

    # ---- sliding window: kv-len cached, window w, vs w + 1 keys cached -----
    for w in args.window:
        assert 0 <= w < n
        for fp8 in (False, True):
            steps = {}
            for ps in args.page_sizes:
                full = PagedKVCache.from_dense(k, v, [n], ps, fp8=fp8, shuffle_seed=7)
                short = PagedKVCache.from_dense(
                    k[:, :, n - w - 1:].contiguous(), v[:, :, n - w - 1:].contiguous(),
                    [w + 1], ps, fp8=fp8, shuffle_seed=7)
                steps[f"short ps={ps}"] = (
                    lambda c=short: _local_paged_decode_partial(q, c))
                steps[f"window ps={ps}"] = (
                    lambda c=full: _local_paged_decode_partial(q, c, window=w))
                err = (steps[f"window ps={ps}"]()[0]
                       - steps[f"short ps={ps}"]()[0]).abs().max().item()
                assert err < 5e-3, (w, ps, err)
            run_group(f"{'fp8' if fp8 else 'bf16'} b=1 kv={n} window={w}", steps, args,
                      results, base_of=lambda label: label.replace("window", "short"),
                      ratio="vs_short",
                      note=f"short = unwindowed step over a cache of {w + 1} keys")
            del steps
    for fp8 in (False, True) if not args.only_window else ():
        steps = {"dense": dense_step(q, k, v, fp8)}
        steps.update(paged_steps(q, k, v, [n], fp8, ("identity", "shuffled"), "chunk"))
        check(steps)
        run_group(f"{'fp8' if fp8 else 'bf16'} b=1 kv={n}", steps, args, results)
        del steps

    if args.only_window:
        return write(args, results)

    # ---- uniform batch: b = 8 at kv / 4 (same bytes as dense, no padding) -
    b, nb = 8, n // 4
    torch.manual_seed(4321)
    q = torch.randn(b, h, 1, d, device=dev, dtype=bf)
    k = torch.randn(b, hk, nb, d, device=dev, dtype=bf)
    v = torch.randn(b, hk, nb, d, device=dev, dtype=bf)
    steps = {"dense": dense_step(q, k, v, False)}
    steps.update(paged_steps(q, k, v, [nb] * b, False, ("identity", "shuffled"), "row"))
    check(steps)
    run_group(f"bf16 b={b} kv={nb}", steps, args, results)
    del steps

    # ---- ragged batch: b = 8, lengths 1k .. 128k --------------------------
    lens = [max(1, n >> (b - 1 - i)) for i in range(b)]
    torch.manual_seed(99)
    k = torch.randn(b, hk, n, d, device=dev, dtype=bf)
    v = torch.randn(b, hk, n, d, device=dev, dtype=bf)
    steps = {"dense": dense_step(q, k, v, False)}
    steps.update(paged_steps(q, k, v, lens, False, ("shuffled",), "row"))
    frac = sum(lens) / (b * n)
    run_group(f"bf16 ragged b={b} lens={lens[0]}..{lens[-1]}", steps, args, results,
              note=f"dense is PADDED to {n} per sequence; the ragged batch "
                   f"holds {frac:.3f} of those bytes")

    write(args, results)


def write(args, results):
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
