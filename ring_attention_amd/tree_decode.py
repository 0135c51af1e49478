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


def _check_softclamp(name: str, softclamp_qk_sim: bool, softclamp_value: float) -> None:
    if softclamp_qk_sim and not softclamp_value > 0:
        raise ValueError(f"{name}: softclamp_value must be > 0 (got {softclamp_value})")


def _softclamp(sim: Tensor, softclamp_qk_sim: bool, softclamp_value: float) -> Tensor:
    """Logit capping of the scaled scores, before any mask (the training
    kernels' definition): c * tanh(sim / c)."""
    if not softclamp_qk_sim:
        return sim
    return softclamp_value * torch.tanh(sim / softclamp_value)


def _local_decode_partial(q: Tensor, k: Tensor, v: Tensor,
                          use_hip_kernel: bool | None = None,
                          vis: Tensor | None = None,
                          grouped: bool = False,
                          softclamp_qk_sim: bool = False,
                          softclamp_value: float = 50.0) -> tuple[Tensor, Tensor]:
    """Local flash-decode partial: (out fp32 (b,h,nq,dv), lse fp32 (b,h,nq,1)).

    `vis` ((b, nq, nq) bool, from _draft_visibility) makes the last nq keys
    the drafts' own tokens: row i attends key n - nq + t iff vis[:, i, t], and
    every key below n - nq.  `grouped` (implied by `vis`) takes the grouped
    MFMA kernel (csrc/decode_grouped.hip) instead of the row kernel.
    `softclamp_qk_sim` caps the scaled scores at `softclamp_value` (see
    tree_attn_decode) in either kernel and in the eager path."""
    clamp = (bool(softclamp_qk_sim), float(softclamp_value))
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
            if grouped or vis is not None:
                outs, lses = hip_ext.require().decode_partial_grouped(
                    qb.to(torch.bfloat16).contiguous(),
                    kb.to(torch.bfloat16).contiguous(),
                    vb.to(torch.bfloat16).contiguous(),
                    None, None, d ** -0.5, 0,
                    None if vis is None else _tree_bits(vis), *clamp)
            else:
                outs, lses = hip_ext.decode_partial(
                    qb.to(torch.bfloat16).contiguous(),
                    kb.to(torch.bfloat16).contiguous(),
                    vb.to(torch.bfloat16).contiguous(),
                    d ** -0.5, *clamp)
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
    sim = _softclamp(torch.einsum("bhid,bhjd->bhij", q.float(), kf) * scale, *clamp)
    if vis is not None:                 # prefix open, drafts by mask (diagonal set)
        nq, n = q.shape[2], k.shape[2]
        masked = torch.zeros(q.shape[0], nq, n, dtype=torch.bool, device=q.device)
        masked[:, :, n - nq:] = ~vis
        sim = sim.masked_fill(masked[:, None], float("-inf"))
    lse = sim.logsumexp(dim=-1, keepdim=True)
    attn = torch.softmax(sim, dim=-1)
    out = torch.einsum("bhij,bhjd->bhid", attn, vf)
    return out, lse


def _dense_visibility(name: str, tree_mask, grouped, causal: bool, b: int, nq: int,
                      n: int | None, device, here: bool = True
                      ) -> tuple[bool, Tensor | None]:
    """The dense entry points' routing: (the call takes the grouped kernel,
    its (b, nq, nq) draft visibility or None).  `n`: keys this rank holds
    (None: none).  `here=False`: the arguments are checked but the mask
    belongs to another rank, and this one runs the grouped kernel unmasked."""
    _check_mask_args(name, tree_mask, grouped, causal)
    if causal and grouped is False:
        raise ValueError(f"{name}: causal needs the grouped kernel (grouped=False given): "
                         "the row kernel has no key limit per row")
    if tree_mask is None and not causal:
        return bool(grouped), None
    if here and (n is None or n < nq):
        raise ValueError(f"{name}: a masked call needs at least nq = {nq} keys on the "
                         f"rank that holds the tail")
    vis = _draft_visibility(name, tree_mask, [], b, nq, device)
    return True, vis if here else None


def _tail_shard(n: int, world: int, nq: int, name: str) -> int:
    """Rank that holds the last chunk of `k.chunk(world, dim=-2)` over n keys
    (the drafts' own tokens).  That chunk must hold all nq of them: ValueError
    otherwise, from shapes alone, so on every rank."""
    size = -(-n // world) if n else 0
    tail = -(-n // size) - 1 if size else 0
    last = n - tail * size
    if last < nq:
        raise ValueError(f"{name}: the last kv shard holds {last} keys, fewer than "
                         f"nq = {nq}: the drafts' tokens must lie on one rank")
    return tail


@torch.no_grad()
def tree_attn_decode(
    q: Tensor,
    k: Tensor | None = None,
    v: Tensor | None = None,
    eps: float = 1e-8,
    shard_kv_seq: bool = True,
    use_hip_kernel: bool | None = None,
    causal: bool = False,
    tree_mask: Tensor | None = None,
    grouped: bool | None = None,
    softclamp_qk_sim: bool = False,
    softclamp_value: float = 50.0,
) -> Tensor:
    """Tree-attention decode of q (b, h, nq, d) over k, v (b, hk, n, dv).

    `softclamp_qk_sim` / `softclamp_value` are ring_flash_attn's (Gemma-2
    style logit capping): sim = c * tanh(q.k * d**-0.5 / c), c =
    softclamp_value > 0 (ValueError otherwise), applied before any mask, so a
    model trained with the clamp decodes with the function it was trained on.
    Every serving entry point of this module and of paged_prefill takes the
    pair with this meaning.

    `tree_mask` / `causal` verify drafts on the dense cache with
    tree_attn_decode_paged's meaning (minus the window): the last nq keys of
    the sequence are the drafts' own tokens, tree_mask[i, t] (bool (b, nq, nq)
    or (nq, nq), diagonal set, nq <= 64, n >= nq) lets draft i attend key
    n - nq + t, every draft attends the whole prefix, and `causal=True` is the
    lower-triangular mask; the two exclude each other.  Either runs the grouped
    MFMA kernel (csrc/decode_grouped.hip), which streams K/V once for all
    (group-mate, draft) rows of a kv head; `grouped=True` takes it for a plain
    call, `grouped=False` with a mask is a ValueError (the row kernel has no
    key limit per row), and a call with none of the three runs the row kernel
    as before.

    With `shard_kv_seq=True` the mask goes to the rank that holds the last
    chunk of `k.chunk(world)`, which must hold at least nq keys (ValueError on
    every rank otherwise); the other ranks run unmasked.  With
    `shard_kv_seq=False` the caller passes the mask only on the rank that
    holds the tail.
    """
    assert (k is None) == (v is None)
    dtype = q.dtype
    b, h, nq, d = q.shape
    name = "tree_attn_decode"
    _check_softclamp(name, softclamp_qk_sim, softclamp_value)

    # capture the value dim from the FULL v before chunking: a rank whose
    # shard is empty must still pack a (b,h,1,1+dv)-shaped all-reduce buffer,
    # and dv may differ from q's head dim d
    dim_v = v.shape[-1] if v is not None else d

    masked_here = tree_mask is not None or causal
    if shard_kv_seq:
        assert k is not None
        rank, world = get_rank(), get_world_size()
        if masked_here:
            masked_here = rank == _tail_shard(k.shape[-2], world, nq, name)
        ks = k.chunk(world, dim=-2)
        vs = v.chunk(world, dim=-2)
        k, v = (ks[rank], vs[rank]) if rank < len(ks) else (None, None)

    use_grouped, vis = _dense_visibility(
        name, tree_mask, grouped, causal, b, nq,
        None if k is None else k.shape[-2], q.device, masked_here)

    if v is not None:
        local_out, lse = _local_decode_partial(q, k, v, use_hip_kernel, vis, use_grouped,
                                               softclamp_qk_sim, softclamp_value)
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
    causal: bool = False,
    tree_mask: Tensor | None = None,
    grouped: bool | None = None,
    softclamp_qk_sim: bool = False,
    softclamp_value: float = 50.0,
) -> Tensor:
    """Tree-attention decode over an FP8-quantized LOCAL KV-cache shard.

    The cache (from ops.fp8.quantize_kv_cache, layouts (b, hk, n, d) e4m3 +
    (b, hk, n) e8m0 row scales) streams at HALF the bf16 bytes — decode is
    bandwidth-bound, so the step time roughly halves.  Cross-rank merge is
    identical to tree_attn_decode (2 collective rounds).  Each rank passes
    its own pre-quantized shard (there is no in-function sharding: a serving
    cache lives pre-sharded next to its rank).

    `causal`, `tree_mask` and `grouped` are tree_attn_decode's: the last nq
    keys of the shard are the drafts' own tokens, so only the rank that holds
    the tail of the sequence passes a mask.  `softclamp_qk_sim` /
    `softclamp_value` are tree_attn_decode's; the clamp applies to the true
    score, after the e8m0 key scale.
    """
    dtype = q.dtype
    b, _, nq, d = q.shape
    _check_softclamp("tree_attn_decode_fp8", softclamp_qk_sim, softclamp_value)
    clamp = (bool(softclamp_qk_sim), float(softclamp_value))
    use_grouped, vis = _dense_visibility("tree_attn_decode_fp8", tree_mask, grouped,
                                         causal, b, nq, k8.shape[-2], q.device)
    if q.is_cuda:
        from .ops import hip_ext
        if use_grouped:
            outs, lses = hip_ext.require().decode_partial_grouped(
                q.to(torch.bfloat16).contiguous(), k8, v8, ks, vs, d ** -0.5, 0,
                None if vis is None else _tree_bits(vis), *clamp)
        else:
            outs, lses = hip_ext.require().decode_partial_fp8(
                q.to(torch.bfloat16).contiguous(), k8, v8, ks, vs, d ** -0.5, 0, *clamp)
        local_out, lse = hip_ext.require().decode_merge(outs, lses)
    else:
        # CPU fallback: dequantize the cache and run the eager partial (the
        # fp8 serving paths test and run anywhere, like the rest of the
        # framework's CPU fallbacks)
        kd = (k8.view(torch.float8_e4m3fn).float()
              * torch.exp2(ks.float() - 127.0).unsqueeze(-1))
        vd = (v8.view(torch.float8_e4m3fn).float()
              * torch.exp2(vs.float() - 127.0).unsqueeze(-1))
        local_out, lse = _local_decode_partial(q, kd, vd, vis=vis,
                                               softclamp_qk_sim=clamp[0],
                                               softclamp_value=clamp[1])
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


def _tree_visibility(tree_mask, grouped, causal: bool, window, cache, b: int,
                     nq: int, device) -> tuple[bool, Tensor | None]:
    """Checks the tree_mask / grouped arguments on the host (no device read)
    and returns (the call takes the grouped kernel, its (b, nq, nq) bool
    draft visibility or None for no mask).  `grouped=True, causal=True` is
    the chain: the lower-triangular mask."""
    name = "tree_attn_decode_paged"
    if tree_mask is None and not grouped:
        return False, None
    _check_mask_args(name, tree_mask, grouped, causal)
    if tree_mask is not None and (window is not None or any(cache.host_starts)):
        raise ValueError(f"{name}: a tree mask serves neither a window nor a cache "
                         "with released pages (a draft's position is its depth)")
    if tree_mask is None and not causal:
        return True, None
    return True, _draft_visibility(name, tree_mask, cache.host_lens, b, nq, device)


def _check_mask_args(name: str, tree_mask, grouped, causal: bool) -> None:
    """What a tree_mask excludes, for the paged and the dense entry points."""
    if tree_mask is not None and grouped is False:
        raise ValueError(f"{name}: tree_mask needs the grouped kernel (grouped=False given)")
    if tree_mask is not None and causal:
        raise ValueError(f"{name}: tree_mask and causal=True exclude each other "
                         "(a chain is the lower-triangular mask)")


def _draft_visibility(name: str, tree_mask, lens, b: int, nq: int, device) -> Tensor:
    """Host checks of a masked grouped call (no device read beyond the
    mask's diagonal) -> (b, nq, nq) bool; tree_mask None is the chain.
    `lens`: the sequences' cached lengths."""
    if nq > 64:
        raise ValueError(f"{name}: a tree mask covers at most 64 drafts (nq = {nq})")
    if any(0 < n < nq for n in lens):
        raise ValueError(f"{name}: a masked sequence holds 0 or at least nq = {nq} tokens")
    if tree_mask is None:
        vis = torch.ones(nq, nq, dtype=torch.bool, device=device).tril()
    else:
        vis = tree_mask.to(device=device, dtype=torch.bool)
    if vis.dim() == 2:
        vis = vis[None].expand(b, nq, nq)
    if tuple(vis.shape) != (b, nq, nq):
        raise ValueError(f"{name}: tree_mask must be (nq, nq) or (b, nq, nq)")
    if not bool(vis.diagonal(dim1=-2, dim2=-1).all()):
        raise ValueError(f"{name}: every draft attends itself (tree_mask diagonal)")
    return vis


def _tree_bits(vis: Tensor) -> Tensor:
    """(b, nq, nq) bool -> int32 (b, nq, 2): bit t of the 64-bit row word
    (low word first) = draft t visible."""
    b, nq, _ = vis.shape
    w = torch.zeros(b, nq, 64, dtype=torch.int64, device=vis.device)
    w[..., :nq] = vis
    pw = torch.tensor([1 << t for t in range(32)], dtype=torch.int64, device=vis.device)
    words = (w.view(b, nq, 2, 32) * pw).sum(-1)             # unsigned 32-bit values
    return torch.where(words >= 1 << 31, words - (1 << 32), words).to(torch.int32).contiguous()


_PSU_INTS = 12                  # csrc/attn_common.h PSU_INTS
_PSU_PREFIX, _PSU_SUFFIX = 0, 1
_SHARED_TARGET_UNITS = 2 * 256  # planner: workgroups aimed at (two per CU)
_SHARED_PASS = 128              # keys a workgroup consumes per pass


def plan_shared_units(lens, groups, hk: int, rows: int, nq: int, masked: bool,
                      chunks: int = 0, unit_tiles: int = 2,
                      target_units: int | None = None):
    """Work units of one shared-prefix decode call, on the host (nothing is
    read back): `lens` and `groups` are the cache's `host_lens` and
    `prefix_groups()`, `rows` = G * nq rows per (sequence, kv head).

    A group's members join its PREFIX span [0, P) when no draft of theirs lies
    inside it: always without a mask, with one only if P <= len - nq (the
    others are served whole by their suffix span, as is every sequence outside
    a group).  Groups left with fewer than two members are dropped.  Every
    sequence with keys beyond its prefix gets a SUFFIX span [P_s, len), cut
    from P_s & ~127.  A span's stacked rows make ceil(members * rows / 32)
    tiles, `unit_tiles` of them per unit; its keys are cut into shares of
    `per` keys, a multiple of 128: one figure for the whole call, sized so
    that about `target_units` units result, or with `chunks` > 0
    ceil(keys / chunks) per span.  Share z of a prefix span writes partial
    slot z, share z of a suffix span slot S_prefix + z.

    Returns (units, members, n_slots): int rows [kind, kv head, first tile,
    tiles, j_lo, j_hi, slot, member offset, member count, lo, len, 0],
    heaviest first; the flat member lists; the number of partial slots.
    """
    target = _SHARED_TARGET_UNITS if target_units is None else int(target_units)
    prefix_of = [0] * len(lens)
    spans = []                                  # (kind, members, lo, hi)
    for seqs, shared in groups:
        joined = [s for s in seqs if not masked or shared <= lens[s] - nq]
        if len(joined) >= 2 and shared > 0:
            for s in joined:
                prefix_of[s] = shared
            spans.append((_PSU_PREFIX, joined, 0, shared))
    n_prefix = len(spans)
    spans += [(_PSU_SUFFIX, [s], prefix_of[s], n) for s, n in enumerate(lens)
              if n > prefix_of[s]]

    def up(x):                                  # next multiple of a pass
        return -(-x // _SHARED_PASS) * _SHARED_PASS

    geom = []                                   # (base, keys, tiles) per span
    for _, mem, lo, hi in spans:
        base = lo // _SHARED_PASS * _SHARED_PASS
        geom.append((base, hi - base, -(-len(mem) * rows // 32)))
    work = sum(keys * -(-tiles // unit_tiles) * hk for _, keys, tiles in geom)
    per_all = max(_SHARED_PASS, up(-(-work // max(1, target))))
    counts = []
    for _, keys, _ in geom:
        per = up(-(-keys // chunks)) if chunks > 0 else per_all
        counts.append((per, -(-keys // per)))
    s_prefix = max((c for _, c in counts[:n_prefix]), default=0)
    n_slots = max(1, s_prefix + max((c for _, c in counts[n_prefix:]), default=0))

    keyed, members = [], []
    for (kind, mem, lo, hi), (base, _, tiles), (per, count) in zip(spans, geom, counts):
        mem0 = len(members)
        members.extend(mem)
        for z in range(count):
            j_lo, j_hi = base + z * per, min(hi, base + (z + 1) * per)
            slot = z if kind == _PSU_PREFIX else s_prefix + z
            for tile0 in range(0, tiles, unit_tiles):
                ntile = min(unit_tiles, tiles - tile0)
                for head in range(hk):
                    keyed.append(((j_hi - max(j_lo, lo)) * ntile,
                                  [kind, head, tile0, ntile, j_lo, j_hi, slot, mem0,
                                   len(mem), lo, hi, 0]))
    keyed.sort(key=lambda u: -u[0])             # stable: heaviest first
    return [u for _, u in keyed], members, n_slots


def _shared_plan(ext, cache, h: int, nq: int, masked: bool, chunks: int, device):
    """The device copy of `plan_shared_units` for this cache state and call
    shape: (plan tensor, units, slots, most tiles in a unit).  Kept on the
    cache until it changes (every mutation bumps its version), so repeated
    steps over an unchanged cache neither plan nor upload again."""
    plans = cache.__dict__.setdefault("_shared_plans", {})
    key = (h, nq, masked, chunks, str(device))
    hit = plans.get(key)
    if hit is not None and hit[0] == cache._version:
        return hit[1]
    hk, kd = cache.kv_heads, cache.kernel_dim
    units, members, n_slots = plan_shared_units(
        cache.host_lens, cache.prefix_groups(), hk, h // hk * nq, nq, masked,
        chunks, ext.paged_shared_unit_tiles(kd))
    flat = torch.tensor([x for u in units for x in u] + members, dtype=torch.int32)
    dev = ext.paged_shared_upload(flat, len(units), n_slots, cache.max_seqs, h, hk, nq,
                                  cache.page_size, cache.max_pages_per_seq, masked, kd,
                                  device)
    plan = (dev, len(units), n_slots, max((u[3] for u in units), default=1))
    plans[key] = (cache._version, plan)
    return plan


def _local_paged_decode_partial(q: Tensor, cache, causal: bool = False,
                                use_hip_kernel: bool | None = None,
                                chunks: int = 0, window: int | None = None,
                                kv_after=None, tree_mask: Tensor | None = None,
                                grouped: bool | None = None,
                                softclamp_qk_sim: bool = False,
                                softclamp_value: float = 50.0,
                                shared_prefix: bool | None = None) -> tuple[Tensor, Tensor]:
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

    `tree_mask` (bool (b, nq, nq) or (nq, nq)) replaces the chain-shaped tail:
    the last nq cached tokens are the drafts, tree_mask[i, t] lets draft i
    attend draft t (key seq_len - nq + t), and every draft attends the whole
    prefix below seq_len - nq.  It runs the grouped MFMA kernel
    (csrc/decode_paged_grouped.hip), as does `grouped=True` with `causal`
    either way; see tree_attn_decode_paged for the rules.  `grouped=True`
    takes `window` / `kv_after` and a released cache with the meaning above
    (the kernel's windowed variant); `tree_mask` takes neither.
    `softclamp_qk_sim` / `softclamp_value` (tree_attn_decode's) cap the scores
    before any of these masks, in the row kernel, the grouped kernel and the
    eager path alike.

    `shared_prefix=True` takes the work-unit kernel
    (csrc/decode_paged_shared.hip): the sequences of a `cache.prefix_groups()`
    group stream the pages they share once per kv head, for the rows of all
    of them (`plan_shared_units`); `chunks` > 0 then fixes the shares per
    span.  It implies `grouped`, takes `causal` or `tree_mask` and the
    softclamp, and refuses `window`, `kv_after`, a cache with released pages
    and `grouped=False` with ValueError before any launch.  The result is the
    same attention: on CPU the eager path runs unchanged.
    """
    b, h, nq, d = q.shape
    _check_softclamp("tree_attn_decode_paged", softclamp_qk_sim, softclamp_value)
    clamp = (bool(softclamp_qk_sim), float(softclamp_value))
    assert b == cache.max_seqs and d == cache.dim_head
    assert h % cache.kv_heads == 0
    if shared_prefix:
        for given, what in ((window is not None, "a window"),
                            (kv_after is not None, "kv_after"),
                            (any(cache.host_starts), "a cache with released pages"),
                            (grouped is False, "grouped=False")):
            if given:
                raise ValueError(f"tree_attn_decode_paged: shared_prefix=True does "
                                 f"not serve {what}")
        grouped = True
    use_grouped, vis = _tree_visibility(tree_mask, grouped, causal, window, cache,
                                        b, nq, q.device)
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
        win_args = (window is not None, 0 if window is None else int(window),
                    None if window is None or after is None else
                    torch.tensor(after, dtype=torch.int32).to(q.device))
        if shared_prefix:
            plan, n_units, n_slots, unit_tiles = _shared_plan(
                ext, cache, h, nq, vis is not None, int(chunks), q.device)
            outs, lses = ext.decode_partial_paged_shared(
                qb.to(torch.bfloat16).contiguous(),
                cache.k_pages, cache.v_pages, cache.k_scales, cache.v_scales,
                cache.block_table, cache.seq_lens, plan, n_units, n_slots, unit_tiles,
                d ** -0.5, None if vis is None else _tree_bits(vis), *clamp)
            out, lse = ext.decode_merge(outs, lses)
            return (out[..., :d] if d != kd else out), lse
        if use_grouped:
            outs, lses = ext.decode_partial_paged_grouped(
                qb.to(torch.bfloat16).contiguous(),
                cache.k_pages, cache.v_pages, cache.k_scales, cache.v_scales,
                cache.block_table, cache.seq_lens, cache.max_seq_len,
                d ** -0.5, chunks, None if vis is None else _tree_bits(vis),
                *win_args, *clamp)
            out, lse = ext.decode_merge(outs, lses)
            return (out[..., :d] if d != kd else out), lse
        outs, lses = ext.decode_partial_paged(
            qb.to(torch.bfloat16).contiguous(),
            cache.k_pages, cache.v_pages, cache.k_scales, cache.v_scales,
            cache.block_table, cache.seq_lens, cache.max_seq_len,
            d ** -0.5, causal, chunks, *win_args, *clamp)
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
        sim = _softclamp(torch.einsum("hid,hjd->hij", q[i].float(), kf) * scale, *clamp)
        if vis is not None:                             # prefix open, drafts by mask
            masked = torch.zeros(nq, n, dtype=torch.bool, device=q.device)
            masked[:, n - nq:] = ~vis[i]
            sim = sim.masked_fill(masked[None], float("-inf"))
        elif causal:
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
    tree_mask: Tensor | None = None,
    grouped: bool | None = None,
    softclamp_qk_sim: bool = False,
    softclamp_value: float = 50.0,
    shared_prefix: bool | None = None,
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

    `tree_mask` verifies a TREE of drafts in one step (Medusa / EAGLE /
    SpecInfer style): a bool tensor (b, nq, nq), or (nq, nq) shared by the
    batch, where tree_mask[i, t] lets draft i attend draft t, the token cached
    at seq_len - nq + t.  Every draft attends the whole prefix below
    seq_len - nq; the diagonal must be True; nq <= 64; every sequence holds
    at least nq tokens or none (an empty slot returns dead rows).  It runs the
    grouped MFMA kernel, which stacks the (group-mate, draft) rows of a kv
    head into 32-row tiles and streams K/V once per tile.  Only the rank
    that holds the tail passes it.  `grouped=True` takes that kernel without
    a mask too (`causal=True` is then the chain, the lower-triangular mask);
    `grouped=None` takes it exactly when tree_mask is given.  `grouped=True`
    without a tree_mask serves `window` / `kv_after` and a cache with released
    pages exactly as the row kernel does.  tree_mask with causal=True, with
    grouped=False, with `window` or with a cache that has released pages
    raises ValueError before anything runs, as does a violated rule above
    (lengths come from the host mirrors).

    `softclamp_qk_sim` / `softclamp_value` are tree_attn_decode's and combine
    with every legal combination of the arguments above.

    `shared_prefix=True` serves a cache whose sequences were forked with
    `PagedKVCache.share_prefix` (one system prompt behind a batch, n samples
    of a prompt, beams, each with its draft tree): the pages a
    `cache.prefix_groups()` group shares are streamed once per kv head for
    the rows of all its members, by the work-unit kernel, instead of once per
    sequence.  The result is that of the call without it.  It implies
    `grouped` and combines with plain, `causal=True`, `tree_mask` and the
    softclamp; with `window`, `kv_after`, a cache that has released pages or
    `grouped=False` it raises ValueError before anything runs.  With no group
    in the cache the same kernel runs one span per sequence.  The default
    (None) runs what runs without the argument.
    """
    local_out, lse = _local_paged_decode_partial(q, cache, causal, use_hip_kernel,
                                                 window=window, kv_after=kv_after,
                                                 tree_mask=tree_mask, grouped=grouped,
                                                 softclamp_qk_sim=softclamp_qk_sim,
                                                 softclamp_value=softclamp_value,
                                                 shared_prefix=shared_prefix)
    return _merge_across_ranks(local_out, lse, q.dtype, eps)


def _local_mla_decode_partial(q: Tensor, cache, causal: bool = False,
                              scale: float | None = None,
                              use_hip_kernel: bool | None = None,
                              chunks: int = 0) -> tuple[Tensor, Tensor]:
    """Local flash-decode partial over a PagedLatentCache:
    (out fp32 (b,h,nq,512), lse fp32 (b,h,nq,1)).

    q (b, h, nq, 576) with b == cache.max_seqs; every head attends the
    sequence's 576-wide rows as keys and their first 512 columns as values.
    Row (b, iq) attends keys [0, limit), limit = seq_lens[b], or with `causal`
    max(0, seq_lens[b] - (nq - 1 - iq)).  A row with limit == 0 returns
    out == 0 with a finite lse <= -1e30 (`_local_paged_decode_partial`'s
    convention).  On GPU this is csrc/decode_paged_latent.hip plus the fused
    chunk merge, with no eager fallback; `chunks` > 0 fixes the kv-split.  A
    cache with released pages raises ValueError before any launch (there is
    no window on this path).
    """
    b, h, nq, d = q.shape
    assert b == cache.max_seqs and d == cache.dim_head == 576
    if any(cache.host_starts):
        raise ValueError("tree_attn_decode_mla: the cache has released pages "
                         "(release_prefix), and this path has no window")
    scale = d ** -0.5 if scale is None else float(scale)
    if q.is_cuda and use_hip_kernel is not False:
        from .ops import hip_ext
        ext = hip_ext.require()       # no eager fallback on GPU
        outs, lses = ext.decode_partial_latent(
            q.to(torch.bfloat16).contiguous(), cache.k_pages, cache.block_table,
            cache.seq_lens, cache.max_seq_len, scale, causal, chunks)
        return tuple(ext.decode_merge(outs, lses))

    # eager path (CPU): gather each sequence, mask by length and tail
    neg = -torch.finfo(torch.float32).max
    out = q.new_zeros((b, h, nq, cache.latent_dim), dtype=torch.float32)
    lse = torch.full((b, h, nq, 1), neg, device=q.device, dtype=torch.float32)
    for i, n in enumerate(cache.host_lens):
        if n == 0:
            continue
        kf, vf = cache.gather(i)
        sim = torch.einsum("hid,jd->hij", q[i].float(), kf[0].float()) * scale
        if causal:
            limit = n - (nq - 1 - torch.arange(nq, device=q.device))
            masked = torch.arange(n, device=q.device)[None, :] >= limit[:, None]
            sim = sim.masked_fill(masked[None], float("-inf"))
        row_lse = sim.logsumexp(dim=-1, keepdim=True)   # -inf where limit <= 0
        live = torch.isfinite(row_lse)
        attn = torch.nan_to_num(torch.softmax(sim, dim=-1))
        o = torch.einsum("hij,jd->hid", attn, vf[0].float())
        out[i] = torch.where(live, o, torch.zeros_like(o))
        lse[i] = torch.where(live, row_lse, torch.full_like(row_lse, neg))
    return out, lse


@torch.no_grad()
def tree_attn_decode_mla(
    q: Tensor,
    cache,
    causal: bool = False,
    scale: float | None = None,
    eps: float = 1e-8,
    use_hip_kernel: bool | None = None,
) -> Tensor:
    """Tree-attention decode over an MLA latent cache (DeepSeek-V2/V3 style,
    up-projections absorbed): q (b, h, nq, 576) -> (b, h, nq, 512) in q.dtype.

    `cache` is this rank's PagedLatentCache holding its LOCAL shard of every
    sequence (ragged, 0 tokens is legal).  `scale` defaults to 576 ** -0.5;
    MLA models pass the scale of their unabsorbed head dim, with a YaRN
    factor where they use one.  `causal=True` has tree_attn_decode_paged's
    meaning: only the rank that holds the tail passes it, the last nq cached
    tokens are the queries' own, and row iq attends [0, len - (nq - 1 - iq)).
    Ranks merge exactly like tree_attn_decode_paged.
    """
    local_out, lse = _local_mla_decode_partial(q, cache, causal, scale, use_hip_kernel)
    return _merge_across_ranks(local_out, lse, q.dtype, eps)
