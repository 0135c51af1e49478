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

`--grouped NQ [NQ ...]` times the grouped MFMA kernel (`grouped=True`) against
the row kernel of the same build on one sequence with NQ query tokens per
head, bf16 and fp8, page size 64, shuffled table, alternating in the same
rounds, and returns; `vs_row` is grouped / row.  With `--window` both kernels
take `window=W` over the `--kv-len` cached keys, one group per W.

`--dense-grouped NQ [NQ ...]` does the same on the DENSE cache: the row kernel
(decode_partial / decode_partial_fp8) against csrc/decode_grouped.hip with at
most 1, 2 and 4 row tiles per workgroup (RING_ATTN_GROUPED_TILES, as far as the
shape has that many) and as the launcher picks them; `vs_row` is grouped / row.

`--shared-prefix P --batch B [B ...] --suffix N` builds one forked cache per
batch size (page size 64, shuffled pages: B sequences behind P shared tokens,
N of their own each), and times `shared_prefix=True`
(csrc/decode_paged_shared.hip) against `grouped=True` on that same cache, one
query token per head, bf16 and fp8, alternating in the same rounds, and
returns; `vs_grouped` is shared / grouped.  The cache does not change between
steps, so the unit plan is built and uploaded once.

`--latent` times the MLA latent-cache step (csrc/decode_paged_latent.hip plus
the D = 512 chunk merge) against `gather` + fp32 torch einsums on a
PagedLatentCache: h = 16 and h = 128 on one sequence of `--kv-len` keys, and
h = 16 on a batch of 32 x `--kv-len` / 16, alternating in the same rounds, and
returns; `vs_torch` is hip / torch and `tb_s` the unique cache bytes per
second of the median.

    python tools/paged_decode_bench.py [--kv-len 131072] [--rounds 7] [--out F]
        [--latent]
        [--window 1024 4096 32768] [--only-window] [--grouped 1 4 16]
        [--dense-grouped 1 4 16] [--softclamp 50]
        [--shared-prefix 8192 --batch 8 32 --suffix 256]
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


def dense_grouped_step(q, k, v, fp8):
    """The grouped MFMA kernel on the dense cache (partial + merge)."""
    ext = hip_ext.require()
    c = quantize_kv_cache(k, v) if fp8 else (k, v, None, None)
    scale = q.shape[-1] ** -0.5
    return lambda: ext.decode_merge(*ext.decode_partial_grouped(q, *c, scale))


def with_env(fn, name, value):
    """Same step with one of the bindings' A/B environment switches set."""
    def step():
        os.environ[name] = value
        try:
            return fn()
        finally:
            del os.environ[name]
    return step


def ordered(fn, order):
    """Same step with the workgroup order forced: "row" = the dense kernels'
    (row block fast, kv chunk slow), "chunk" = kv chunk fast.  Unforced, the
    binding picks row for b == 1 and chunk for b > 1."""
    return with_env(fn, "RING_ATTN_PAGED_ORDER", order)


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
    ap.add_argument("--grouped", type=int, nargs="*", default=[],
                    help="query tokens per head: time grouped=True against the "
                         "row kernel (ps 64, shuffled) and nothing else")
    ap.add_argument("--dense-grouped", type=int, nargs="*", default=[],
                    help="query tokens per head: time the grouped kernel on the DENSE "
                         "cache (at most 1, 2, 4 tiles per workgroup and its own pick) "
                         "against the dense row kernel and nothing else")
    ap.add_argument("--shared-prefix", type=int, default=0, metavar="P",
                    help="tokens every sequence of the batch shares (share_prefix): time "
                         "shared_prefix=True against grouped=True on one forked cache "
                         "and nothing else")
    ap.add_argument("--batch", type=int, nargs="+", default=[8],
                    help="with --shared-prefix: sequences behind the prefix")
    ap.add_argument("--suffix", type=int, default=256,
                    help="with --shared-prefix: tokens each sequence holds of its own")
    ap.add_argument("--softclamp", type=float, default=None, metavar="VALUE",
                    help="with --grouped: also time both kernels with "
                         "softclamp_qk_sim=True at this softclamp_value, in the same rounds")
    ap.add_argument("--latent", action="store_true",
                    help="time the MLA latent-cache step (tree_attn_decode_mla's local "
                         "partial) against gather + torch einsums and nothing else")
    ap.add_argument("--out", default=None, help="also write the records here (JSON)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "paged_decode_bench needs a GPU"
    hip_ext.require()
    dev, bf = "cuda", torch.bfloat16
    if args.latent:
        return latent_groups(args, dev, bf)
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

    # ---- grouped MFMA kernel vs the row kernel ------------------------------
    for nq in args.grouped:
        qn = torch.randn(1, h, nq, d, device=dev, dtype=bf)
        for fp8 in (False, True):
            cache = PagedKVCache.from_dense(k, v, [n], 64, fp8=fp8, shuffle_seed=7)
            for w in args.window or [None]:
                steps = {"row": lambda c=cache, w=w: _local_paged_decode_partial(
                             qn, c, window=w),
                         "grouped": lambda c=cache, w=w: _local_paged_decode_partial(
                             qn, c, window=w, grouped=True)}
                err = (steps["grouped"]()[0] - steps["row"]()[0]).abs().max().item()
                assert err < 5e-3, (nq, fp8, w, err)
                if args.softclamp is not None:
                    clamp = dict(softclamp_qk_sim=True, softclamp_value=args.softclamp)
                    steps["row softclamp"] = lambda c=cache, w=w: _local_paged_decode_partial(
                        qn, c, window=w, **clamp)
                    steps["grouped softclamp"] = lambda c=cache, w=w: _local_paged_decode_partial(
                        qn, c, window=w, grouped=True, **clamp)
                    err = (steps["grouped softclamp"]()[0]
                           - steps["row softclamp"]()[0]).abs().max().item()
                    assert err < 5e-3, (nq, fp8, w, "softclamp", err)
                run_group(f"{'fp8' if fp8 else 'bf16'} b=1 kv={n} {h}q/{hk}kv nq={nq}"
                          + ("" if w is None else f" window={w}"),
                          steps, args, results, base_of=lambda label: "row", ratio="vs_row")
    if args.grouped:
        return write(args, results)

    # ---- forked cache: shared-prefix units vs the grouped kernel ------------
    for b in args.batch if args.shared_prefix else ():
        ps, prefix, sfx = 64, args.shared_prefix, args.suffix
        assert prefix % ps == 0 and prefix > 0 and sfx >= 0
        qb = torch.randn(b, h, 1, d, device=dev, dtype=bf)
        for fp8 in (False, True):
            cache = PagedKVCache(prefix // ps + b * (-(-sfx // ps) + 1), ps, hk, d, b,
                                 -(-(prefix + sfx) // ps) + 1, fp8=fp8, device=dev)
            cache._free = torch.randperm(cache.num_pages,
                                         generator=torch.Generator().manual_seed(7)).tolist()
            kp = torch.randn(b, hk, max(prefix, sfx), d, device=dev, dtype=bf)
            vp = torch.randn(b, hk, max(prefix, sfx), d, device=dev, dtype=bf)
            cache.append(kp, vp, [prefix] + [0] * (b - 1))
            for dst in range(1, b):
                cache.share_prefix(0, dst, prefix)
            cache.append(kp, vp, [sfx] * b)
            steps = {"grouped": lambda c=cache: _local_paged_decode_partial(
                         qb, c, grouped=True),
                     "shared": lambda c=cache: _local_paged_decode_partial(
                         qb, c, shared_prefix=True)}
            err = (steps["shared"]()[0] - steps["grouped"]()[0]).abs().max().item()
            assert err < 5e-3, (b, fp8, err)
            run_group(f"{'fp8' if fp8 else 'bf16'} b={b} prefix={prefix} suffix={sfx} "
                      f"{h}q/{hk}kv ps={ps}", steps, args, results,
                      base_of=lambda label: "grouped", ratio="vs_grouped",
                      note=f"one forked cache, {cache.pages_held()} distinct pages; the "
                           "unit plan is reused while the cache is unchanged")
            del cache, steps
    if args.shared_prefix:
        return write(args, results)

    # ---- dense cache: grouped MFMA kernel vs the dense row kernel -----------
    for nq in args.dense_grouped:
        qn = torch.randn(1, h, nq, d, device=dev, dtype=bf)
        tiles = -(-(h // hk) * nq // 32)
        caps = [c for c in (1, 2, 4) if c == 1 or c // 2 < min(tiles, 4 if d == 64 else 2)]
        for fp8 in (False, True):
            steps = {"row": dense_step(qn, k, v, fp8)}
            fn = dense_grouped_step(qn, k, v, fp8)
            for cap in caps + [None]:
                steps["grouped" if cap is None else f"grouped tiles<={cap}"] = (
                    fn if cap is None else with_env(fn, "RING_ATTN_GROUPED_TILES", str(cap)))
            ref = steps["row"]()[0]
            for label, fn in steps.items():
                err = (fn()[0] - ref).abs().max().item()
                assert err < 5e-3, (nq, fp8, label, err)
            run_group(f"dense {'fp8' if fp8 else 'bf16'} b=1 kv={n} {h}q/{hk}kv nq={nq}",
                      steps, args, results, base_of=lambda label: "row", ratio="vs_row",
                      note=f"{tiles} row tile(s) per kv head")
    if args.dense_grouped:
        return write(args, results)

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


def latent_groups(args, dev, bf):
    """csrc/decode_paged_latent.hip + decode_merge<512> against the only other
    way to serve a PagedLatentCache: gather + fp32 torch einsums on the same
    GPU.  page_size 64, shuffled pages, one query token per head.  `tb_s` is
    the unique cache bytes (tokens x 1152) over the median step time."""
    from ring_attention_amd import PagedLatentCache
    from ring_attention_amd.tree_decode import _local_mla_decode_partial
    results = []
    n = args.kv_len
    for h, b, kv in ((16, 1, n), (128, 1, n), (16, 32, n // 16)):
        torch.manual_seed(1234 + h + b)
        ckv = torch.randn(b, 1, kv, 576, device=dev, dtype=bf)
        q = torch.randn(b, h, 1, 576, device=dev, dtype=bf)
        cache = PagedLatentCache.from_dense(ckv, [kv] * b, 64, shuffle_seed=7)
        del ckv
        steps = {"torch": lambda c=cache, q=q: _local_mla_decode_partial(
                     q, c, use_hip_kernel=False),
                 "hip": lambda c=cache, q=q: _local_mla_decode_partial(q, c)}
        err = (steps["hip"]()[0] - steps["torch"]()[0]).abs().max().item()
        assert err < 5e-3, (h, b, err)
        first = len(results)
        run_group(f"latent bf16 b={b} kv={kv} h={h} nq=1 ps=64 shuffled", steps, args,
                  results, base_of=lambda label: "torch", ratio="vs_torch")
        for rec in results[first:]:
            rec["tb_s"] = round(b * kv * 1152 / rec["median_us"] * 1e-6, 3)
        print(json.dumps({"tb_s": {r["config"]: r["tb_s"] for r in results[first:]}}),
              flush=True)
        del cache, steps
    write(args, results)


def write(args, results):
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
