"""Tree attention decoding — single-token decode over cluster-sharded KV.

Capability parity with the reference's tree_attn_decode
(/root/reference/ring_attention_pytorch/tree_attn_decoding.py:23-103),
Shyam et al. Algorithm 3 (arXiv:2408.04093), re-designed for RCCL over xGMI:
the reference issues THREE all-reduces (MAX lse, SUM den, SUM num); latency
dominates at decode-time payload sizes, so here the two SUM reductions are
packed into ONE RCCL all-reduce on a fused [den | num] buffer — 2 collective
rounds per decoded token instead of 3.

Layout parity with the reference: q (b, h, 1, d); k, v (b, h, n, dv).
Generalized beyond the reference (tree_attn_decoding.py:54-79 handles one
query per head, no GQA): q may carry NQ query tokens per head (speculative /
tree-decode heads) as (b, h, nq, d), and k/v may have fewer heads
(b, hk, n, dv) with the tile GQA pairing qh % hk — the HIP kernel shares the
kv stream across the extra queries through L2/L3.
"""

from __future__ import annotations

import torch
import torch.distributed as dist
from torch import Tensor

from .parallel import get_rank, get_world_size, is_distributed


def _local_decode_partial(q: Tensor, k: Tensor, v: Tensor,
                          use_hip_kernel: bool | None = None) -> tuple[Tensor, Tensor]:
    """Local flash-decode partial: (out fp32 (b,h,nq,dv), lse fp32 (b,h,nq,1))."""
    if q.is_cuda and use_hip_kernel is not False:
        from .ops import hip_ext
        if hip_ext.available():
            d = q.shape[-1]
            dv = v.shape[-1]
            kd = 64 if max(d, dv) <= 64 else 128
            import torch.nn.functional as _F
            qb = _F.pad(q, (0, kd - d)) if d != kd else q
            kb = _F.pad(k, (0, kd - d)) if d != kd else k
            vb = _F.pad(v, (0, kd - dv)) if dv != kd else v
            outs, lses = hip_ext.decode_partial(
                qb.to(torch.bfloat16).contiguous(),
                kb.to(torch.bfloat16).contiguous(),
                vb.to(torch.bfloat16).contiguous(),
                sm_scale=d ** -0.5)
            # fused S-chunk merge (the torch reduce expression costs more
            # dispatches than the decode kernel itself at S = 256)
            out, lse = hip_ext.require().decode_merge(outs, lses)
            if dv != kd:
                out = out[..., :dv]
            return out, lse
    scale = q.shape[-1] ** -0.5
    kf, vf = k.float(), v.float()
    groups = q.shape[1] // k.shape[1]
    if groups > 1:                      # tile GQA pairing (qh % hk)
        kf = kf.repeat(1, groups, 1, 1)
        vf = vf.repeat(1, groups, 1, 1)
    sim = torch.einsum("bhid,bhjd->bhij", q.float(), kf) * scale
    lse = sim.logsumexp(dim=-1, keepdim=True)
    attn = torch.softmax(sim, dim=-1)
    out = torch.einsum("bhij,bhjd->bhid", attn, vf)
    return out, lse


@torch.no_grad()
def tree_attn_decode(
    q: Tensor,
    k: Tensor | None = None,
    v: Tensor | None = None,
    eps: float = 1e-8,
    shard_kv_seq: bool = True,
    use_hip_kernel: bool | None = None,
) -> Tensor:
    assert (k is None) == (v is None)
    dtype = q.dtype
    b, h, nq, d = q.shape

    # capture the value dim from the FULL v before chunking: a rank whose
    # shard is empty must still pack a (b,h,1,1+dv)-shaped all-reduce buffer,
    # and dv may differ from q's head dim d
    dim_v = v.shape[-1] if v is not None else d

    if shard_kv_seq:
        assert k is not None
        rank, world = get_rank(), get_world_size()
        ks = k.chunk(world, dim=-2)
        vs = v.chunk(world, dim=-2)
        k, v = (ks[rank], vs[rank]) if rank < len(ks) else (None, None)

    if v is not None:
        local_out, lse = _local_decode_partial(q, k, v, use_hip_kernel)
    else:
        # seq shorter than world: this rank holds nothing
        local_out = q.new_zeros((b, h, nq, dim_v), dtype=torch.float32)
        lse = torch.full((b, h, nq, 1), -torch.finfo(torch.float32).max,
                         device=q.device, dtype=torch.float32)

    return _merge_across_ranks(local_out, lse, dtype, eps)


def _merge_across_ranks(local_out: Tensor, lse: Tensor, dtype, eps: float) -> Tensor:
    if not is_distributed():
        return local_out.to(dtype)

    # round 1: global max(lse)
    max_lse = lse.clone()
    dist.all_reduce(max_lse, dist.ReduceOp.MAX)

    # round 2: ONE summed all-reduce over the packed [den | num] buffer
    den = (lse - max_lse).exp()                         # (b,h,nq,1)
    packed = torch.cat((den, local_out * den), dim=-1)  # (b,h,nq,1+dv)
    dist.all_reduce(packed)
    den_sum, num_sum = packed[..., :1], packed[..., 1:]

    out = num_sum / den_sum.clamp(min=eps)
    return out.to(dtype)


@torch.no_grad()
def tree_attn_decode_fp8(
    q: Tensor,
    k8: Tensor, v8: Tensor, ks: Tensor, vs: Tensor,
    eps: float = 1e-8,
) -> Tensor:
    """Tree-attention decode over an FP8-quantized LOCAL KV-cache shard.

    The cache (from ops.fp8.quantize_kv_cache, layouts (b, hk, n, d) e4m3 +
    (b, hk, n) e8m0 row scales) streams at HALF the bf16 bytes — decode is
    bandwidth-bound, so the step time roughly halves.  Cross-rank merge is
    identical to tree_attn_decode (2 collective rounds).  Each rank passes
    its own pre-quantized shard (there is no in-function sharding: a serving
    cache lives pre-sharded next to its rank).
    """
    dtype = q.dtype
    d = q.shape[-1]
    if q.is_cuda:
        from .ops import hip_ext
        outs, lses = hip_ext.require().decode_partial_fp8(
            q.to(torch.bfloat16).contiguous(), k8, v8, ks, vs, d ** -0.5)
        local_out, lse = hip_ext.require().decode_merge(outs, lses)
    else:
        # CPU fallback: dequantize the cache and run the eager partial (the
        # fp8 serving paths test and run anywhere, like the rest of the
        # framework's CPU fallbacks)
        kd = (k8.view(torch.float8_e4m3fn).float()
              * torch.exp2(ks.float() - 127.0).unsqueeze(-1))
        vd = (v8.view(torch.float8_e4m3fn).float()
              * torch.exp2(vs.float() - 127.0).unsqueeze(-1))
        local_out, lse = _local_decode_partial(q, kd, vd)
    return _merge_across_ranks(local_out, lse, dtype, eps)


def _window_spans(lens: list[int], after: list[int], nq: int, causal: bool,
                 window: int) -> list[list[tuple[int, int]]]:
    """Per sequence, the [lo, limit) key span of every query row (the
    definition shared with paged_prefill_attn, in local key coordinates)."""
    spans = []
    for n, a in zip(lens, after):
        rows = []
        for iq in range(nq):
            limit = max(0, n - (nq - 1 - iq)) if causal else n
            rows.append((min(max(n + a - nq + iq - window, 0), limit), limit))
        spans.append(rows)
    return spans


def _local_paged_decode_partial(q: Tensor, cache, causal: bool = False,
                                use_hip_kernel: bool | None = None,
                                chunks: int = 0, window: int | None = None,
                                kv_after=None) -> tuple[Tensor, Tensor]:
    """Local flash-decode partial over a PagedKVCache:
    (out fp32 (b,h,nq,d), lse fp32 (b,h,nq,1)).

    q (b, h, nq, d) with b == cache.max_seqs and d == cache.dim_head (the
    paged path requires dv == d).  Row (b, iq) attends keys [lo, limit) of
    sequence b, limit = seq_lens[b], or with `causal`
    max(0, seq_lens[b] - (nq - 1 - iq)): the last nq cached positions are
    the queries' own tokens.  lo is 0 without a window; with `window=w` the
    query sits at position seq_lens[b] + kv_after[b] - nq + iq in local key
    coordinates (kv_after: tokens of the sequence held by LATER ranks, a host
    list or int tensor read on the host, default 0) and
    lo = clamp(position - w, 0, limit) — paged_prefill_attn's token-exact
    lookback, with or without `causal`.  A row with lo == limit returns
    out == 0 with a finite lse <= -1e30, so it drops out of any later merge.

    A cache that has released pages (`release_prefix`) is only served with a
    window whose rows all start at or beyond `cache.host_starts`; anything
    else raises ValueError before a kernel is launched.
    """
    b, h, nq, d = q.shape
    assert b == cache.max_seqs and d == cache.dim_head
    assert h % cache.kv_heads == 0
    if window is not None and window < 0:
        raise ValueError("tree_attn_decode_paged: window must be >= 0")
    after = None
    if kv_after is not None:
        after = [int(x) for x in (kv_after.tolist() if isinstance(kv_after, Tensor)
                                  else kv_after)]
        if len(after) != b or any(x < 0 for x in after):
            raise ValueError(f"tree_attn_decode_paged: kv_after needs {b} "
                             f"entries >= 0")
    spans = None
    if window is not None and (any(cache.host_starts) or not
                               (q.is_cuda and use_hip_kernel is not False)):
        spans = _window_spans(cache.host_lens, after or [0] * b, nq, causal,
                             int(window))
    if any(cache.host_starts):
        cache.check_released(
            "tree_attn_decode_paged",
            None if spans is None else
            [min((lo for lo, hi in rows if lo < hi), default=None) for rows in spans])
    if q.is_cuda and use_hip_kernel is not False:
        from .ops import hip_ext
        ext = hip_ext.require()       # no eager fallback on GPU
        kd = cache.kernel_dim
        import torch.nn.functional as _F
        qb = _F.pad(q, (0, kd - d)) if d != kd else q
        outs, lses = ext.decode_partial_paged(
            qb.to(torch.bfloat16).contiguous(),
            cache.k_pages, cache.v_pages, cache.k_scales, cache.v_scales,
            cache.block_table, cache.seq_lens, cache.max_seq_len,
            d ** -0.5, causal, chunks, window is not None,
            0 if window is None else int(window),
            None if window is None or after is None else
            torch.tensor(after, dtype=torch.int32).to(q.device))
        out, lse = ext.decode_merge(outs, lses)
        if d != kd:
            out = out[..., :d]
        return out, lse

    # eager fallback (CPU): gather each sequence, mask by length, tail and
    # window (released rows gather as zeros and are always masked)
    scale = d ** -0.5
    hk = cache.kv_heads
    groups = h // hk
    neg = -torch.finfo(torch.float32).max
    out = q.new_zeros((b, h, nq, d), dtype=torch.float32)
    lse = torch.full((b, h, nq, 1), neg, device=q.device, dtype=torch.float32)
    lens = cache.host_lens
    for i in range(b):
        n = lens[i]
        if n == 0:
            continue
        kf, vf = cache.gather(i)
        kf = kf.float().repeat(groups, 1, 1)            # tile pairing qh % hk
        vf = vf.float().repeat(groups, 1, 1)
        sim = torch.einsum("hid,hjd->hij", q[i].float(), kf) * scale
        if causal:
            limit = n - (nq - 1 - torch.arange(nq, device=q.device))
            masked = torch.arange(n, device=q.device)[None, :] >= limit[:, None]
            sim = sim.masked_fill(masked[None], float("-inf"))
        if spans is not None:
            lo = torch.tensor([r[0] for r in spans[i]], device=q.device)
            masked = torch.arange(n, device=q.device)[None, :] < lo[:, None]
            sim = sim.masked_fill(masked[None], float("-inf"))
        row_lse = sim.logsumexp(dim=-1, keepdim=True)   # -inf where limit <= 0
        live = torch.isfinite(row_lse)
        attn = torch.softmax(sim, dim=-1)
        o = torch.einsum("hij,hjd->hid", torch.nan_to_num(attn), vf)
        out[i] = torch.where(live, o, torch.zeros_like(o))
        lse[i] = torch.where(live, row_lse, torch.full_like(row_lse, neg))
    return out, lse


@torch.no_grad()
def tree_attn_decode_paged(
    q: Tensor,
    cache,
    causal: bool = False,
    eps: float = 1e-8,
    use_hip_kernel: bool | None = None,
    window: int | None = None,
    kv_after=None,
) -> Tensor:
    """Tree-attention decode over a paged KV cache with per-sequence lengths.

    q (b, h, nq, d); `cache` is this rank's PagedKVCache holding its LOCAL
    shard of every sequence (ragged, 0 tokens is legal; dv == d).  The local
    partial is the HIP paged-decode kernel plus the fused chunk merge; ranks
    merge exactly like tree_attn_decode (2 collective rounds).  Pass
    `causal=True` only on the rank that holds the tail of the sequences: its
    last nq cached positions are then the queries' own tokens and query iq
    attends up to and including its own.

    `window=w` is the token-exact lookback of RingAttention and
    paged_prefill_attn: a query attends only the keys at most w positions
    behind it.  The queries are the last nq tokens of each sequence, so a
    rank that does not hold the tail passes `kv_after` (host list or int
    tensor, one entry per sequence): the tokens of the sequence held by LATER
    ranks.  A rank whose whole shard lies outside the window merges with
    weight 0.  A cache that has released pages (`PagedKVCache.release_prefix`)
    must be served with a window that stays at or beyond its released prefix;
    otherwise ValueError is raised before anything runs.
    """
    local_out, lse = _local_paged_decode_partial(q, cache, causal, use_hip_kernel,
                                                 window=window, kv_after=kv_after)
    return _merge_across_ranks(local_out, lse, q.dtype, eps)
