"""Paged prefill attention: a chunk of queries over the block-table KV cache.

The serving-side forward next to `tree_attn_decode_paged`: chunked prefill
(new tokens attending thousands already cached), prefix reuse (no dense
regather of the history) and ragged prompt batches (one length and one
diagonal per sequence).  The hot path is the HIP kernel
`attn_fwd_paged_kernel` (csrc/attn_fwd_paged.hip): the dense forward's tile
loop reading K/V through the block table, bf16 or fp8 pools.

Positions: the chunk's own tokens are ALREADY in the cache — append first,
then attend, the convention of `tree_attn_decode_paged(causal=True)`.  Query
t < q_lens[i] of sequence i sits at position seq_len[i] - q_lens[i] + t and
attends keys [0, seq_len[i]); with `causal` only j <= position, with
`window=w` only position - j <= w (the project's token-exact lookback, with
or without `causal`).  A cache whose pages below the window were released
(`PagedKVCache.release_prefix`) is served only with a window that stays at
or beyond the released prefix; anything else raises ValueError up front.
"""

from __future__ import annotations

import torch
import torch.nn.functional as F
from torch import Tensor

_ROWS_WG = 256          # q rows per workgroup (csrc/attn_mask.h ROWS_WG)
_TARGET_WGS = 256       # one workgroup per CU
_MAX_SPLIT = 16         # attn_fwd_merge holds at most 16 shares


def _kvblk(kernel_dim: int) -> int:
    return 128 if kernel_dim == 64 else 64      # csrc/attn_mask.h kvblk()


def auto_kv_split(t: int, b: int, h: int, max_seq_len: int, kernel_dim: int) -> int:
    """Host-side grid.z choice: the smallest split, capped at 16, that brings
    ceil(t / 256) * b * h * split to at least 256 workgroups, and never more
    than the longest sequence's kv tile count."""
    base = max(1, -(-t // _ROWS_WG) * b * h)
    tiles = max(1, -(-max_seq_len // _kvblk(kernel_dim)))
    return max(1, min(-(-_TARGET_WGS // base), _MAX_SPLIT, tiles))


def _host_q_lens(q_lens, b: int, t: int, seq_lens: list[int]) -> list[int]:
    if q_lens is None:
        q_lens = [t] * b
    elif isinstance(q_lens, Tensor):
        q_lens = q_lens.tolist()
    q_lens = [int(x) for x in q_lens]
    if len(q_lens) != b:
        raise ValueError(f"paged_prefill_attn: q_lens has {len(q_lens)} entries, "
                         f"the cache holds {b} sequences")
    for i, (ql, n) in enumerate(zip(q_lens, seq_lens)):
        if not 0 <= ql <= min(t, n):
            raise ValueError(
                f"paged_prefill_attn: q_lens[{i}] = {ql} must lie in "
                f"[0, min(T = {t}, seq_len = {n})] — append the chunk to the "
                f"cache before attending")
    return q_lens


def _eager(q: Tensor, cache, q_lens: list[int], causal: bool, window):
    """Same result from cache.gather, in fp32 (CPU / use_hip_kernel=False)."""
    b, t, h, d = q.shape
    groups = h // cache.kv_heads
    neg = -torch.finfo(torch.float32).max
    out = torch.zeros(b, t, h, d, dtype=torch.float32, device=q.device)
    lse = torch.full((b, h, t), neg, dtype=torch.float32, device=q.device)
    lens = cache.host_lens
    for i in range(b):
        n, ql = lens[i], q_lens[i]
        if ql == 0:
            continue
        kf, vf = cache.gather(i)
        kf = kf.float().repeat(groups, 1, 1)            # tile pairing qh % hk
        vf = vf.float().repeat(groups, 1, 1)
        sim = torch.einsum("thd,hjd->htj", q[i, :ql].float(), kf) * d ** -0.5
        pos = (n - ql + torch.arange(ql, device=q.device))[:, None]
        j = torch.arange(n, device=q.device)[None, :]
        ok = torch.ones(ql, n, dtype=torch.bool, device=q.device)
        if causal:
            ok &= j <= pos
        if window is not None:
            ok &= pos - j <= window
        sim = sim.masked_fill(~ok[None], float("-inf"))
        row_lse = sim.logsumexp(dim=-1)                 # (h, ql); -inf = no key
        live = torch.isfinite(row_lse)
        o = torch.einsum("htj,hjd->thd", torch.nan_to_num(torch.softmax(sim, dim=-1)), vf)
        out[i, :ql] = torch.where(live.t()[..., None], o, torch.zeros_like(o))
        lse[i, :, :ql] = torch.where(live, row_lse, torch.full_like(row_lse, neg))
    return out.to(torch.bfloat16), lse


@torch.no_grad()
def paged_prefill_attn(
    q: Tensor,
    cache,
    q_lens=None,
    causal: bool = True,
    window: int | None = None,
    return_lse: bool = False,
    use_hip_kernel: bool | None = None,
    kv_split: int = 0,
):
    """Attention of a query chunk over a PagedKVCache (serving path, no autograd).

    q (b, T, h, d) with b == cache.max_seqs, d == cache.dim_head and
    h % cache.kv_heads == 0 (q head qh reads kv head qh % hk).  `q_lens` is a
    host list (or int tensor, read on the host like `append`'s) with
    0 <= q_lens[i] <= min(T, seq_len[i]); default T for every sequence.  The
    lengths and the cache's host mirror size the grid and the split — nothing
    is read back from the device.

    Returns out bf16 (b, T, h, d); with `return_lse` also lse fp32 (b, h, T),
    natural log.  A row with t >= q_lens[i], or with no attendable key,
    returns out == 0 and a finite lse <= -1e30.

    On CUDA the HIP kernel is the only path (`hip_ext.require()`, no silent
    fallback); on CPU, or with use_hip_kernel=False, an eager fp32 fallback
    computes the same from `cache.gather`.  `kv_split=0` picks the grid.z
    split automatically (`auto_kv_split`); a positive value forces it (tests,
    A/B runs).
    """
    if q.requires_grad:
        raise RuntimeError(
            "paged_prefill_attn is a serving path without a backward pass: "
            "q must not require grad (detach it)")
    if q.dim() != 4:
        raise ValueError("paged_prefill_attn: q must be (b, T, h, d)")
    b, t, h, d = q.shape
    if b != cache.max_seqs:
        raise ValueError(f"paged_prefill_attn: q batch {b} != cache.max_seqs "
                         f"{cache.max_seqs}")
    if d != cache.dim_head:
        raise ValueError(f"paged_prefill_attn: q head dim {d} != cache.dim_head "
                         f"{cache.dim_head}")
    if h % cache.kv_heads != 0:
        raise ValueError(f"paged_prefill_attn: {h} q heads are not a multiple of "
                         f"{cache.kv_heads} kv heads")
    if window is not None and window < 0:
        raise ValueError("paged_prefill_attn: window must be >= 0")
    if not 0 <= kv_split <= _MAX_SPLIT:
        raise ValueError(f"paged_prefill_attn: kv_split must lie in [0, {_MAX_SPLIT}]")
    lens = _host_q_lens(q_lens, b, t, cache.host_lens)
    if any(cache.host_starts):
        # released pages (PagedKVCache.release_prefix): the first live row of
        # sequence i sits at seq_len - q_len and starts `window` keys back
        cache.check_released(
            "paged_prefill_attn",
            None if window is None else
            [max(0, n - ql - int(window)) if ql > 0 else None
             for n, ql in zip(cache.host_lens, lens)])

    if not (q.is_cuda and use_hip_kernel is not False):
        out, lse = _eager(q, cache, lens, causal, window)
        return (out, lse) if return_lse else out

    from .ops import hip_ext
    ext = hip_ext.require()           # no eager fallback on GPU
    kd = cache.kernel_dim
    qb = (F.pad(q, (0, kd - d)) if d != kd else q).to(torch.bfloat16).contiguous()
    out = torch.empty_like(qb)
    lse = torch.empty(b, h, t, device=q.device, dtype=torch.float32)
    if b * t * h == 0:
        return (out[..., :d], lse) if return_lse else out[..., :d]
    q_lens_dev = torch.tensor(lens, dtype=torch.int32).to(q.device)
    split = kv_split if kv_split > 0 else auto_kv_split(t, b, h, cache.max_seq_len, kd)
    win = 0 if window is None else int(window)
    pool = (cache.k_pages, cache.v_pages, cache.k_scales, cache.v_scales,
            cache.block_table, cache.seq_lens, q_lens_dev)
    if split > 1:
        o_part = torch.empty(split, b, h, kd, t, device=q.device, dtype=torch.float32)
        m_part = torch.empty(split, b, h, t, device=q.device, dtype=torch.float32)
        l_part = torch.empty(split, b, h, t, device=q.device, dtype=torch.float32)
        ext.attn_fwd_paged(qb, *pool, None, None, o_part, m_part, l_part,
                           d ** -0.5, causal, win, window is not None, split)
        ext.attn_fwd_merge(o_part, m_part, l_part, None, None, None,
                           out, lse, split, b, h, kd, t, True, True)
    else:
        ext.attn_fwd_paged(qb, *pool, out, lse, None, None, None,
                           d ** -0.5, causal, win, window is not None, 1)
    if d != kd:
        out = out[..., :d]
    return (out, lse) if return_lse else out
