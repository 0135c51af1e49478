"""Paged prefill vs the dense forward on a gathered copy of the same K/V.

Times, forward only,
  dense          : flash_attn_offset on a dense (b, n, hk, d) copy of the K/V
  dense split=S  : the same dense kernel launched with the grid.z split the
                   paged path picks, + attn_fwd_merge (kernel against kernel)
  dense+gather   : the gather copy out of the pages (what the paged path
                   removes; with dequantisation for an fp8 pool) + dense
  paged ...      : paged_prefill_attn on the PagedKVCache holding the tokens,
                   for page_size in {16, 64, 256} x identity / shuffled tables,
                   with the automatic split (and split=1 where that differs)
on: a full causal prefill of one prompt, a chunk over a long cached context,
and a ragged b = 8 batch of chunks over contexts 1k .. 128k (the dense path
serves that one sequence at a time).

All steps of a group ALTERNATE inside every round (the box is shared); the
median over the rounds is reported with min / max; each measurement is
`--iters` calls between two device events after a warm-up.

    python tools/paged_prefill_bench.py [--rounds 5] [--out F]
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ring_attention_amd import PagedKVCache, paged_prefill_attn     # noqa: E402
from ring_attention_amd.ops import hip_ext                          # noqa: E402
from ring_attention_amd.ops.ring_flash_hip import flash_attn_offset  # noqa: E402
from ring_attention_amd.paged_prefill import auto_kv_split          # noqa: E402


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


def gather_dense(cache, seq):
    """Dense bf16 (1, n, hk, D) k, v of one sequence, on the device, with no
    host read: the copy a dense-kernel server makes before every call."""
    n = cache.host_lens[seq]
    ids = cache.block_table[seq, :-(-n // cache.page_size)].long()

    def dense(pool, scales):
        x = pool.index_select(0, ids)                         # (np, hk, ps, D)
        if cache.fp8:
            x = (x.view(torch.float8_e4m3fn).float()
                 * torch.exp2(scales.index_select(0, ids).float() - 127.0).unsqueeze(-1))
        x = x.permute(0, 2, 1, 3).reshape(1, -1, cache.kv_heads, cache.kernel_dim)
        return x[:, :n].to(torch.bfloat16).contiguous()

    return dense(cache.k_pages, cache.k_scales), dense(cache.v_pages, cache.v_scales)


def dense_split_step(q, k, v, q_offset, split):
    """The dense kernel with a forced grid.z split + merge (one sequence)."""
    ext = hip_ext.require()
    b, n, h, d = q.shape
    out = torch.empty_like(q)
    lse = torch.empty(b, h, n, device=q.device, dtype=torch.float32)
    o_part = torch.empty(split, b, h, d, n, device=q.device, dtype=torch.float32)
    m_part = torch.empty(split, b, h, n, device=q.device, dtype=torch.float32)
    l_part = torch.empty(split, b, h, n, device=q.device, dtype=torch.float32)

    def step():
        ext.attn_fwd(q, k, v, None, o_part, m_part, l_part, None, None,
                     d ** -0.5, True, q_offset, 1, 0, False, False, 50.0,
                     True, True, split, 0, None)
        ext.attn_fwd_merge(o_part, m_part, l_part, None, None, None, out, lse,
                           split, b, h, d, n, True, True)
        return out
    return step


def run_group(name, steps, args, results, note=""):
    samples = {label: [] for label in steps}
    for _ in range(args.rounds):
        for label, fn in steps.items():
            samples[label].append(time_us(fn, args.iters, args.warmup))
    base = statistics.median(samples["dense"])
    for label, xs in samples.items():
        med = statistics.median(xs)
        rec = {"group": name, "config": label, "median_us": round(med, 1),
               "min_us": round(min(xs), 1), "max_us": round(max(xs), 1),
               "vs_dense": round(med / base, 3), "rounds": len(xs), "note": note}
        results.append(rec)
        print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--heads", type=int, default=8)
    ap.add_argument("--kv-heads", type=int, default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--page-sizes", type=int, nargs="+", default=[16, 64, 256])
    ap.add_argument("--out", default=None, help="also write the records here (JSON)")
    args = ap.parse_args()
    assert args.rounds >= 5, "report a median of at least 5 rounds"
    assert torch.cuda.is_available(), "paged_prefill_bench needs a GPU"
    hip_ext.require()
    dev, bf = "cuda", torch.bfloat16
    h = args.heads
    hk = args.kv_heads or h
    results = []

    def one_sequence(t, n, d, fp8):
        """A chunk of t queries at the tail of one sequence of n tokens."""
        torch.manual_seed(1000 + t + d)
        q = torch.randn(1, t, h, d, device=dev, dtype=bf)
        k = torch.randn(1, hk, n, d, device=dev, dtype=bf)
        v = torch.randn(1, hk, n, d, device=dev, dtype=bf)
        split = auto_kv_split(t, 1, h, n, d)
        steps, ref = {}, None
        for ps in args.page_sizes:
            for kind in ("identity", "shuffled"):
                cache = PagedKVCache.from_dense(
                    k, v, [n], ps, fp8=fp8,
                    shuffle_seed=7 if kind == "shuffled" else None)
                if ref is None:
                    # every cache holds the same (de)quantised rows
                    kd, vd = gather_dense(cache, 0)
                    steps["dense"] = lambda: flash_attn_offset(q, kd, vd, n - t, True)
                    if split > 1:
                        steps[f"dense split={split}"] = dense_split_step(q, kd, vd, n - t, split)
                    steps["dense+gather"] = (
                        lambda c=cache: flash_attn_offset(q, *gather_dense(c, 0), n - t, True))
                    ref = steps["dense"]().float()
                steps[f"paged ps={ps} {kind}"] = (
                    lambda c=cache: paged_prefill_attn(q, c, [t], causal=True))
                if split > 1 and kind == "shuffled":
                    steps[f"paged ps={ps} {kind} split=1"] = (
                        lambda c=cache: paged_prefill_attn(q, c, [t], causal=True, kv_split=1))
        for label, fn in steps.items():       # same result before anything is timed
            err = (fn().float() - ref).abs().max().item()
            assert err < 2e-2, (label, err)
        tag = f"{'fp8' if fp8 else 'bf16'} d={d} T={t} over kv={n}"
        run_group(tag, steps, args, results, note=f"auto kv_split={split}")

    for d, fp8 in ((64, False), (128, False), (64, True)):
        one_sequence(8192, 8192, d, fp8)        # full causal prefill of one prompt
        one_sequence(2048, 32768, d, fp8)       # a chunk over a cached context

    # ---- ragged batch: b = 8 chunks of 512 over contexts 1k .. 128k
    b, t, d, n = 8, 512, 64, 131072
    lens = [max(t, n >> (b - 1 - i)) for i in range(b)]
    torch.manual_seed(99)
    q = torch.randn(b, t, h, d, device=dev, dtype=bf)
    k = torch.randn(b, hk, n, d, device=dev, dtype=bf)
    v = torch.randn(b, hk, n, d, device=dev, dtype=bf)
    steps, dense_kv = {}, None
    for ps in args.page_sizes:
        cache = PagedKVCache.from_dense(k, v, lens, ps, shuffle_seed=7)
        if dense_kv is None:
            dense_kv = [gather_dense(cache, i) for i in range(b)]

            def dense_loop():
                return [flash_attn_offset(q[i:i + 1], *dense_kv[i], lens[i] - t, True)
                        for i in range(b)]

            def dense_gather_loop(c=cache):
                return [flash_attn_offset(q[i:i + 1], *gather_dense(c, i), lens[i] - t, True)
                        for i in range(b)]
            steps["dense"] = dense_loop
            steps["dense+gather"] = dense_gather_loop
            ref = torch.cat(dense_loop()).float()
        steps[f"paged ps={ps} shuffled"] = (
            lambda c=cache: paged_prefill_attn(q, c, [t] * b, causal=True))
        err = (steps[f"paged ps={ps} shuffled"]().float() - ref).abs().max().item()
        assert err < 2e-2, (ps, err)
    del k, v
    run_group(f"bf16 d={d} ragged b={b} T={t} over kv={lens[0]}..{lens[-1]}",
              steps, args, results,
              note="dense runs one sequence per launch (8 launches); "
                   f"paged auto kv_split={auto_kv_split(t, b, h, n, d)}")

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
