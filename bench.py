"""Flagship benchmark: ring flash attention fwd+bwd on MI355X.

Measures BASELINE.json's headline metric — attention TFLOP/s, d_head=64,
fwd+bwd — on BASELINE config #2 (non-causal ring flash attention, 8 heads,
d_head 64, 8k tokens per GPU => 64k total at ring_size 8).  Weak scaling:
per-GPU sequence shard is fixed as N grows.

Single process:   python bench.py --gpus 1 --steps 20 --warmup 5
  --dump-outputs DIR  also writes the last timed step's out/dq/dk/dv as .npy
  --full              reserved for measurements beyond the headline figure
Multi-GPU (driver): torchrun --nproc-per-node N bench.py --gpus N ...
  (one rank per GPU over RCCL; reads RANK/LOCAL_RANK/WORLD_SIZE/MASTER_*)

FLOP convention: fwd = 4 * n_shard * n_total * d * h * b per
GPU (halved for causal); fwd+bwd = 2.5 x fwd.  Values reported are the
WHOLE-JOB aggregate over all N GPUs.
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch


# --dump-outputs writes at most this many bytes over all arrays; an array
# over its share is cut to a fixed, seeded sample of its flattened elements
DUMP_BUDGET_BYTES = 32 * 1000 * 1000


def dump_outputs(path, outputs):
    """Write {name: tensor} as path/<name>.npy (float32).  The inputs are
    seeded, so two builds given the same arguments can be compared array by
    array.  Sampled arrays keep their element order (sorted flat indices)."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    share = DUMP_BUDGET_BYTES // 4 // max(len(outputs), 1)   # fp32 elements
    for i, (name, t) in enumerate(sorted(outputs.items())):
        flat = t.detach().reshape(-1)
        if flat.numel() > share:
            rng = np.random.default_rng(20240 + i)
            idx = np.sort(rng.integers(0, flat.numel(), size=share))
            flat = flat[torch.from_numpy(idx).to(flat.device)]
            arr = flat.float().cpu().numpy()
        else:
            arr = flat.float().cpu().numpy().reshape(tuple(t.shape))
        np.save(os.path.join(path, name + ".npy"), arr)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--seq-per-gpu", type=int, default=8192)
    ap.add_argument("--heads", type=int, default=8)
    ap.add_argument("--kv-heads", type=int, default=None,
                    help="GQA: kv heads (default = heads)")
    ap.add_argument("--d-head", type=int, default=64)
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--causal", action="store_true")
    ap.add_argument("--striped", action="store_true")
    ap.add_argument("--fp8", action="store_true",
                    help="MX-FP8 serving forward (e4m3 block-scaled MFMA; "
                         "implies --fwd-only, 1 GPU; combine with --causal)")
    ap.add_argument("--softclamp", action="store_true",
                    help="gemma-style tanh score cap (dedicated kernel instantiations)")
    ap.add_argument("--fwd-only", action="store_true",
                    help="measure forward only (diagnostics; not the headline metric)")
    ap.add_argument("--config", type=int, default=None, choices=[2, 3, 4, 5],
                    help="BASELINE.json config preset: 2=non-causal ring 64k-class, "
                         "3=causal striped 256k-class, 4=GQA 32q/4kv zig-zag "
                         "causal 1M-class, 5=tree-decode step 128k KV")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed "
                         "step returned (out, and dq/dk/dv unless forward-"
                         "only) as DIR/<name>.npy in float32")
    ap.add_argument("--full", action="store_true",
                    help="also run the measurements beyond the headline "
                         "figure (there are none yet: a plain run already "
                         "does only set-up, warm-up and the timed steps)")
    args = ap.parse_args()

    # BASELINE.json config presets (per-GPU shards of the 8-GPU configs, so
    # the same command measures any world size the driver launches)
    if args.config == 2:
        pass                                    # = the defaults
    elif args.config == 3:
        args.causal = True; args.striped = True; args.seq_per_gpu = 32768
    elif args.config == 4:
        args.causal = True
        args.heads, args.kv_heads, args.seq_per_gpu = 32, 4, 131072
    elif args.config == 5:
        args.seq_per_gpu = 131072

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    distributed = world > 1

    on_gpu = torch.cuda.is_available()
    if on_gpu:
        torch.cuda.set_device(local_rank)   # before init_process_group (RCCL)
    if distributed:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        torch.distributed.init_process_group("nccl" if on_gpu else "gloo")
    if on_gpu:
        device = torch.device("cuda", local_rank)
        dtype = torch.bfloat16
        from ring_attention_amd.ops.ring_flash_hip import ring_flash_attn_hip_ as attn
    else:
        # no-GPU fallback so the contract is testable anywhere: tiny oracle run
        device = torch.device("cpu")
        dtype = torch.float32
        args.seq_per_gpu = min(args.seq_per_gpu, 512)
        from ring_attention_amd.ops.ring_flash import ring_flash_attn_ as attn

    b, n, h, d = args.batch, args.seq_per_gpu, args.heads, args.d_head
    hk = args.kv_heads if args.kv_heads is not None else h
    if not on_gpu and args.config in (4, 5):
        n = args.seq_per_gpu = min(args.seq_per_gpu, 512)
    torch.manual_seed(1234 + rank)

    if args.config == 5:
        # tree-attention decode: single-query step over world-sharded KV.
        # --fp8 streams the e4m3-quantized cache (half the HBM bytes)
        from ring_attention_amd.tree_decode import tree_attn_decode
        q5 = torch.randn(b, h, 1, d, device=device, dtype=dtype)
        k5 = torch.randn(b, h, n, d, device=device, dtype=dtype)
        v5 = torch.randn(b, h, n, d, device=device, dtype=dtype)

        if getattr(args, "fp8", False) and on_gpu:
            from ring_attention_amd.ops.fp8 import quantize_kv_cache
            from ring_attention_amd.tree_decode import tree_attn_decode_fp8
            c5 = quantize_kv_cache(k5, v5)

            def step():
                return {"out": tree_attn_decode_fp8(q5, *c5)}
        else:
            def step():
                return {"out": tree_attn_decode(q5, k5, v5, shard_kv_seq=False)}
    elif args.config == 4:
        # zig-zag causal GQA + fused rotary (per-GPU slice of the 1M config)
        from ring_attention_amd.zigzag import zig_zag_attn
        from ring_attention_amd.models.rotary import apply_rotary_pos_emb
        q = torch.randn(b, n, h, d, device=device, dtype=dtype, requires_grad=True)
        k = torch.randn(b, n, hk, d, device=device, dtype=dtype, requires_grad=True)
        v = torch.randn(b, n, hk, d, device=device, dtype=dtype, requires_grad=True)
        half = n // 2
        starts = (rank * half, (2 * world - 1 - rank) * half)
        pos = torch.cat([starts[0] + torch.arange(half, device=device),
                         starts[1] + torch.arange(n - half, device=device)])
        inv_freq = 1.0 / (10000.0 ** (torch.arange(0, d, 2, device=device).float() / d))
        f_ = torch.einsum("i,j->ij", pos.float(), inv_freq)
        freqs = torch.cat((f_, f_), dim=-1)

        def step():
            qr = apply_rotary_pos_emb(freqs, q)
            kr = apply_rotary_pos_emb(freqs, k)
            out = zig_zag_attn(qr.permute(0, 2, 1, 3), kr.permute(0, 2, 1, 3),
                               v.permute(0, 2, 1, 3), causal=True,
                               q_chunk_starts=starts)
            res = {"out": out}
            if not args.fwd_only:
                out.backward(out.detach())
                res.update(dq=q.grad, dk=k.grad, dv=v.grad)
                q.grad = None; k.grad = None; v.grad = None
            return res
    elif getattr(args, "fp8", False) and on_gpu:
        # MX-FP8 serving forward: quantization is per-prefill (outside the
        # step, like a KV-cache write); the step is the fused e4m3 forward
        from ring_attention_amd.ops.fp8 import quantize_fp8, flash_attn_fp8_quantized
        args.fwd_only = True
        q = torch.randn(b, n, h, d, device=device, dtype=dtype)
        k = torch.randn(b, n, h, d, device=device, dtype=dtype)
        v = torch.randn(b, n, h, d, device=device, dtype=dtype)
        fp8_args = quantize_fp8(q, k, v)
        fp8_scale = d ** -0.5

        def step():
            out, lse = flash_attn_fp8_quantized(*fp8_args, fp8_scale,
                                                causal=args.causal)
            return {"out": out, "lse": lse}
    else:
        q = torch.randn(b, n, h, d, device=device, dtype=dtype, requires_grad=True)
        k = torch.randn(b, n, hk, d, device=device, dtype=dtype, requires_grad=True)
        v = torch.randn(b, n, hk, d, device=device, dtype=dtype, requires_grad=True)

        def step():
            out, _ = attn(q, k, v, causal=args.causal, ring_reduce_col=True,
                          striped_ring_attn=args.striped, ring_size=world,
                          bucket_size=min(n, 1024),
                          softclamp_qk_sim=args.softclamp)
            res = {"out": out}
            if not args.fwd_only:
                out.backward(out.detach())  # fwd + full bwd (dq, dk, dv incl. ring)
                res.update(dq=q.grad, dk=k.grad, dv=v.grad)
                q.grad = None; k.grad = None; v.grad = None
            return res

    for _ in range(args.warmup):
        step()

    # single-GPU: replay the whole fwd+bwd step as ONE hipGraph (cuts every
    # per-launch host round-trip; the same kernels run the same work).
    # Collectives make capture unsafe at world>1, so only when local.
    graph = None
    if on_gpu and world == 1 and not os.environ.get("RING_ATTN_BENCH_NO_GRAPH"):
        try:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):     # allocator warmup for capture
                step()
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            g_ = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g_):
                graph_outputs = step()   # static tensors every replay refills
            g_.replay()
            torch.cuda.synchronize()
            graph = g_
        except Exception:
            graph = None

    if distributed:
        torch.distributed.barrier()
    if on_gpu:
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    last = None
    for _ in range(args.steps):
        if graph is not None:
            graph.replay()
        else:
            last = step()
    if distributed:
        torch.distributed.barrier()
    if on_gpu:
        torch.cuda.synchronize()
    t1 = time.perf_counter()

    elapsed = torch.tensor([t1 - t0], dtype=torch.float64)
    if distributed:
        # max over ranks
        elapsed_d = elapsed.to(device if on_gpu else "cpu")
        torch.distributed.all_reduce(elapsed_d, torch.distributed.ReduceOp.MAX)
        elapsed = elapsed_d.cpu()
    secs = float(elapsed.item())
    ms_per_step = secs / args.steps * 1e3

    if args.dump_outputs is not None and rank == 0:
        dump_outputs(args.dump_outputs,
                     (graph_outputs if graph is not None else last) or {})

    n_total = n * world
    fwd_flops_per_gpu = 4.0 * b * n * n_total * d * h
    if args.causal:
        fwd_flops_per_gpu /= 2
    total_flops = (1.0 if args.fwd_only else 2.5) * fwd_flops_per_gpu * world * args.steps
    tflops_aggregate = total_flops / secs / 1e12
    if args.config == 4:
        # zig-zag attends the GLOBAL gathered kv per GPU: n * n_total * ... is
        # already that; convention unchanged
        pass

    if rank == 0 and args.config == 5:
        print(json.dumps({
            "metric": "tree_decode_step_latency",
            "value": round(ms_per_step * 1e3, 1),
            "unit": "us/step",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 4),
            "higher_is_better": False,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "bf16" if on_gpu else "fp32-cpu-fallback",
            "data": "synthetic",
            "config": {
                "model": "tree_attn_decode (single-query, sharded KV)",
                "global_batch": b,
                "seq_len": n * world, "seq_per_gpu": n,
                "heads": h, "d_head": d,
                "parallelism": f"tree{world}",
                "hipgraph": graph is not None,
                "kv_stream_TBps": round(b * h * n * d * 2 * 2 / (ms_per_step * 1e-3) / 1e12, 2),
            },
        }))
    elif rank == 0:
        print(json.dumps({
            "metric": "attn_tflops",
            "value": round(tflops_aggregate, 2),
            "unit": "TFLOP/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 3),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": ("fp8_e4m3" if getattr(args, "fp8", False) and on_gpu
                      else "bf16" if on_gpu else "fp32-cpu-fallback"),
            "data": "synthetic",
            "config": {
                "model": ("flash_attn_fp8 (MX-FP8 serving forward)"
                          if getattr(args, "fp8", False) and on_gpu
                          else "zig_zag_attn (causal GQA + rotary)" if args.config == 4
                          else "ring_flash_attn (non-causal, d_head 64)" if not args.causal
                          else "ring_flash_attn (causal%s)" % (" striped" if args.striped else "")),
                "global_batch": b,
                "seq_len": n_total,
                "seq_per_gpu": n,
                "heads": h,
                "kv_heads": hk,
                "d_head": d,
                "parallelism": f"ring{world}",
                "hipgraph": graph is not None,
                "flop_convention": "fwd=4*b*n_shard*n_total*d*h (/2 causal); fwd+bwd=2.5x",
            },
        }))

    if distributed:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
