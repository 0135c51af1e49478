"""Token-by-token decoding over cluster-sharded KV with tree attention.

Demonstrates the serving path: each rank holds a shard of the KV cache;
every decode step is one local kv-chunked kernel partial plus TWO RCCL
all-reduce rounds (MAX lse + one packed [den|num] SUM — the reference's
scheme used three).  Run distributed:

    torchrun --standalone --local-addr 127.0.0.1 --nproc-per-node N \
        examples/serve_tree_decode.py

or single-process (no collectives, same math).  On GPU the local partial
is the HIP decode kernel (2.6 TB/s at 128k KV — 101 us/step; `--fp8`
halves the stream to 50 us); on CPU it
falls back to the eager partial so this example runs anywhere.

`--paged` serves a RAGGED batch from a block-table paged KV cache instead
(`PagedKVCache` + `tree_attn_decode_paged`): every sequence has its own
length, and each step appends the new token's K/V to the tail rank's pages
before decoding — the cache grows page by page, nothing is reallocated.
Works with and without `--fp8` (fused quantising append), on GPU and CPU.
In a single process the ragged prompts first go through `paged_prefill_attn`
right after the prompt append: causal attention straight off the pages, one
length and one diagonal per sequence.

`--paged --window W` serves a sliding-window (lookback) model: the prefill and
every decode step attend only the W keys behind each query, ranks that do not
hold the tail tell the kernel how many keys the later ranks hold
(`kv_after`), and after every step `release_prefix` hands the pages that fell
out of the window back to the pool — the cache holds about W / page_size + 2
pages per sequence however long the sequence grows.
"""

from __future__ import annotations

import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ring_attention_amd import tree_attn_decode
from ring_attention_amd.parallel import get_rank, get_world_size, is_distributed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kv-len", type=int, default=8192, help="total KV cache length")
    ap.add_argument("--heads", type=int, default=8)
    ap.add_argument("--d-head", type=int, default=64)
    ap.add_argument("--batch", type=int, default=None,
                    help="sequences (default 1; 4 with --paged)")
    ap.add_argument("--steps", type=int, default=16, help="tokens to decode")
    ap.add_argument("--fp8", action="store_true",
                    help="serve from an e4m3-quantized KV cache (GPU only; "
                         "half the HBM stream per step)")
    ap.add_argument("--paged", action="store_true",
                    help="ragged batch over a paged KV cache that grows by "
                         "one token per step")
    ap.add_argument("--page-size", type=int, default=64,
                    help="tokens per page with --paged (power of two, 16..256)")
    ap.add_argument("--window", type=int, default=None,
                    help="with --paged: token-exact lookback window; pages "
                         "that fall out of it are released after every step")
    args = ap.parse_args()
    if args.window is not None and not args.paged:
        ap.error("--window needs --paged")
    if args.batch is None:
        args.batch = 4 if args.paged else 1

    if "RANK" in os.environ and not is_distributed():
        torch.distributed.init_process_group(
            "nccl" if torch.cuda.is_available() else "gloo")
    rank, world = get_rank(), get_world_size()
    device = "cuda" if torch.cuda.is_available() else "cpu"
    if device == "cuda":
        torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", 0)))
    dtype = torch.bfloat16 if device == "cuda" else torch.float32

    if args.paged:
        return serve_paged(args, rank, world, device, dtype)

    b, h, d = args.batch, args.heads, args.d_head
    n_local = args.kv_len // world

    # this rank's shard of a COMMON synthetic KV cache (in service: filled
    # by prefill) — outputs are identical for any world size
    torch.manual_seed(1234)
    k_full = torch.randn(b, h, args.kv_len, d, device=device, dtype=dtype)
    v_full = torch.randn(b, h, args.kv_len, d, device=device, dtype=dtype)
    k_cache = k_full[:, :, rank * n_local:(rank + 1) * n_local].contiguous()
    v_cache = v_full[:, :, rank * n_local:(rank + 1) * n_local].contiguous()
    del k_full, v_full

    torch.manual_seed(7)
    q = torch.randn(b, h, 1, d, device=device, dtype=dtype)

    if args.fp8 and device == "cuda":
        # quantize once at cache-write time; every decode step then streams
        # 8-bit rows (scales fold into the softmax weights)
        from ring_attention_amd.ops.fp8 import quantize_kv_cache
        from ring_attention_amd.tree_decode import tree_attn_decode_fp8
        cache8 = quantize_kv_cache(k_cache, v_cache)

        def decode_step(q):
            return tree_attn_decode_fp8(q, *cache8)
    else:
        def decode_step(q):
            return tree_attn_decode(q, k_cache, v_cache, shard_kv_seq=False)

    outs = []
    t0 = time.perf_counter()
    for step in range(args.steps):
        # one decode step over the sharded cache (each rank contributes its
        # local partial; the cache is ALREADY sharded)
        out = decode_step(q)
        outs.append(out)
        # in a real server: out -> lm head -> next token -> append its K/V
        # to ONE rank's shard; here we just feed the output back as q
        q = out
    if device == "cuda":
        torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / args.steps

    if rank == 0:
        print(f"world {world}  kv {args.kv_len} ({n_local}/rank)  "
              f"{args.steps} steps  {dt*1e6:.0f} us/token  "
              f"out[0,0,0,:4] = {outs[-1][0,0,0,:4].float().tolist()}")


def serve_paged(args, rank, world, device, dtype):
    from ring_attention_amd import PagedKVCache, tree_attn_decode_paged

    b, h, d, ps = args.batch, args.heads, args.d_head, args.page_size
    # ragged batch: sequence i holds kv_len, ..., down to about kv_len / 2
    lens = [args.kv_len - i * (args.kv_len // (2 * b)) for i in range(b)]
    # this rank's shard [lo, hi) of every sequence of a COMMON synthetic
    # cache (in service: filled by prefill); the LAST rank holds the tails
    # and takes the new tokens
    lo = [n * rank // world for n in lens]
    hi = [n * (rank + 1) // world for n in lens]
    local = [e - s for s, e in zip(lo, hi)]
    tail = rank == world - 1

    torch.manual_seed(1234)
    k_full = torch.randn(b, h, args.kv_len, d, device=device, dtype=dtype)
    v_full = torch.randn(b, h, args.kv_len, d, device=device, dtype=dtype)
    t = max(max(local), 1)
    k_loc = torch.zeros(b, h, t, d, device=device, dtype=dtype)
    v_loc = torch.zeros(b, h, t, d, device=device, dtype=dtype)
    for i in range(b):
        k_loc[i, :, :local[i]] = k_full[i, :, lo[i]:hi[i]]
        v_loc[i, :, :local[i]] = v_full[i, :, lo[i]:hi[i]]
    del k_full, v_full

    grow = args.steps if tail else 0
    per_seq = [-(-(n + grow) // ps) for n in local]
    cache = PagedKVCache(sum(per_seq), ps, h, d, b, max(max(per_seq), 1),
                         fp8=args.fp8, device=device)
    cache.append(k_loc, v_loc, local)          # ragged prompt prefill
    del k_loc, v_loc

    if world == 1:
        # the prompt's own attention, straight off the pages it was just
        # appended to (append first, then attend): ragged, causal, no dense
        # K/V copy.  Stand-in queries; in a real server they come from the
        # model, layer by layer.
        from ring_attention_amd import paged_prefill_attn
        torch.manual_seed(11)
        q_prompt = torch.randn(b, t, h, d, device=device, dtype=dtype)
        t0 = time.perf_counter()
        o_prompt = paged_prefill_attn(q_prompt, cache, local, causal=True,
                                      window=args.window)
        if device == "cuda":
            torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        print(f"paged prefill  prompts {local[0]}..{local[-1]}  {dt*1e3:.2f} ms  "
              f"out[0,-1,0,:4] = {o_prompt[0, local[0] - 1, 0, :4].float().tolist()}")
        del q_prompt, o_prompt

    torch.manual_seed(7)
    q = torch.randn(b, h, 1, d, device=device, dtype=dtype)

    outs = []
    t0 = time.perf_counter()
    for step in range(args.steps):
        # the new token's K/V go to the tail rank's pages first (stand-ins
        # derived from q; in a real server they come from the model), then
        # every rank decodes over its shard: 2 collective rounds per token
        if tail:
            cache.append(q, q.flip(-1))
        if args.window is None:
            out = tree_attn_decode_paged(q, cache)
        else:
            # the query is the sequence's last token, step + 1 tokens past the
            # prompt on the tail rank: every other rank passes what the later
            # ranks hold, and every rank gives back the pages that the NEXT
            # query (one position on) can no longer reach
            total = [n + step + 1 for n in lens]
            after = None if tail else [n - e for n, e in zip(total, hi)]
            out = tree_attn_decode_paged(q, cache, window=args.window, kv_after=after)
            cache.release_prefix([max(0, n - args.window - s)
                                  for n, s in zip(total, lo)])
        outs.append(out)
        q = out
    if device == "cuda":
        torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / args.steps

    if rank == 0:
        win = "" if args.window is None else f"  window {args.window}"
        print(f"world {world}  paged{' fp8' if args.fp8 else ''}  page {ps}{win}  "
              f"pages held {cache.pages_held()}{' on rank 0' if world > 1 else ''}  "
              f"batch {b}  kv {lens[0]}..{lens[-1]} (+{args.steps})  "
              f"{args.steps} steps  {dt*1e6:.0f} us/token  "
              f"out[0,0,0,:4] = {outs[-1][0,0,0,:4].float().tolist()}")


if __name__ == "__main__":
    main()
