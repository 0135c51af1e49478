"""Sliding-window decode on the paged KV cache, with page release.

One definition, shared with `paged_prefill_attn`: the queries are the last nq
tokens of each sequence; with L local keys and A keys held by later ranks,
row (b, iq) sits at qpos = L + A - nq + iq (local key coordinates) and attends
local keys [lo, limit), limit = causal ? max(0, L - (nq-1-iq)) : L and
lo = clamp(qpos - window, 0, limit).

Every oracle is computed here in fp32 on the CPU from keys gathered by hand
BEFORE anything is released (`_pool_rows` of tests/test_paged_decode.py) or
from a dense history kept outside the cache.  The GPU cases then release the
pages below the call's smallest lo and overwrite every page the cache no
longer holds with NaN, so a dereferenced released page or a read below lo
shows as a non-finite output.

Bounds: the paged-decode ones (out max-abs 3e-3 bf16 / 5e-3 fp8 against the
oracle on the dequantised pool, lse max-abs 2e-3).  A dead row (lo == limit)
is exactly 0 with a finite lse <= -1e30; with window >= 0 and no later rank a
row is dead only where limit == 0.
"""

import os
import re
import subprocess
import sys

import pytest
import torch

from ring_attention_amd import PagedKVCache, paged_prefill_attn, tree_attn_decode_paged
from ring_attention_amd.tree_decode import _local_paged_decode_partial

from .loopback_dist import loopback_world
from .test_paged_decode import (LSE_TOL, OUT_BF16, OUT_FP8, _check, _hand_built,
                                _pool_rows, _rand_q, _same_state, _sharded_caches,
                                _state)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LENS = [1, 63, 130, 517]
# descending: lo only grows as the window shrinks, so one cache serves every
# window of a case with release_prefix called before each
WINDOWS = [10000, 200, 65, 64, 63, 16, 15, 1, 0]


# --------------------------------------------------------------------------
# in-test oracle
# --------------------------------------------------------------------------
def _spans(lens, nq, causal, window, after=None):
    """[[(lo, limit)] * nq] per sequence, straight from the definition."""
    after = after or [0] * len(lens)
    out = []
    for n, a in zip(lens, after):
        rows = []
        for iq in range(nq):
            limit = max(0, n - (nq - 1 - iq)) if causal else n
            lo = 0 if window is None else min(max(n + a - nq + iq - window, 0), limit)
            rows.append((lo, limit))
        out.append(rows)
    return out


def _oracle(q, ks, vs, spans):
    """fp32 attention of q (b, h, nq, d) over per-sequence k/v [(hk, L, d)]
    (qh % hk pairing), row (i, iq) over keys spans[i][iq].  Returns (out, lse,
    live (b, nq)); dead rows have out = 0, lse = -inf."""
    q = q.detach().float().cpu()
    b, h, nq, d = q.shape
    out = torch.zeros(b, h, nq, d)
    lse = torch.full((b, h, nq, 1), float("-inf"))
    live = torch.zeros(b, nq, dtype=torch.bool)
    for i in range(b):
        heads = torch.arange(h) % ks[i].shape[0]
        for iq, (lo, hi) in enumerate(spans[i]):
            if lo >= hi:
                continue
            live[i, iq] = True
            kk = ks[i][heads, lo:hi].float()                 # (h, n, d)
            vv = vs[i][heads, lo:hi].float()
            s = torch.einsum("hjd,hd->hj", kk, q[i, :, iq]) * d ** -0.5
            lse[i, :, iq, 0] = torch.logsumexp(s, dim=-1)
            out[i, :, iq] = torch.einsum("hj,hjd->hd", torch.softmax(s, dim=-1), vv)
    return out, lse, live


def _check_dead(live, spans, lens, nq):
    """With window >= 0 and no later rank, dead <=> limit == 0, and a
    sequence holding at least nq keys has no dead row."""
    for i, rows in enumerate(spans):
        for iq, (lo, hi) in enumerate(rows):
            assert bool(live[i, iq]) == (hi > 0), (i, iq, lo, hi)
        if lens[i] >= nq:
            assert live[i].all(), (i, rows)


def _keep_from(spans):
    """Smallest lo over each sequence's live rows (0 if it has none)."""
    return [min((lo for lo, hi in rows if lo < hi), default=0) for rows in spans]


def _poison_unheld(cache):
    """NaN (0x7f = e4m3 NaN for an fp8 pool) in every page the cache does not
    hold: the spare ones and the released ones."""
    held = {pg for s in range(cache.max_seqs) for pg in cache.pages_of(s) if pg >= 0}
    free = [pg for pg in range(cache.num_pages) if pg not in held]
    assert len(free) == cache.free_pages
    if free:
        idx = torch.tensor(free, device=cache.k_pages.device)
        fill = 0x7f if cache.fp8 else float("nan")
        cache.k_pages[idx] = fill
        cache.v_pages[idx] = fill


def _run_windows(cache, q, ks, vs, lens, causal, chunks, tol, tag):
    nq = q.shape[2]
    starts = cache.host_starts
    for w in WINDOWS:
        spans = _spans(lens, nq, causal, w)
        cache.release_prefix(_keep_from(spans))
        assert all(a <= b for a, b in zip(starts, cache.host_starts))
        starts = cache.host_starts
        _poison_unheld(cache)
        out, lse = _local_paged_decode_partial(q, cache, causal=causal, chunks=chunks,
                                               window=w)
        ref = _oracle(q, ks, vs, spans)
        _check_dead(ref[2], spans, lens, nq)
        _check(out, lse, *ref, tol, f"{tag} w={w}")
    # the smallest windows did release pages of the long sequences
    assert cache.host_starts[-1] >= (lens[-1] - nq) // cache.page_size * cache.page_size


# --------------------------------------------------------------------------
# GPU
# --------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("chunks", [0, 7])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("heads", [(4, 4, 1), (6, 2, 3)])
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("page_size", [16, 64, 128])
def test_window_ragged(page_size, d, heads, causal, chunks):
    """Ragged batch, every window from 'everything' down to 0, pages below
    each call's smallest lo released and NaN-poisoned first."""
    h, hk, nq = heads
    torch.manual_seed(200 + page_size + d + h)
    cache = _hand_built(LENS, page_size, hk, d, "cuda", seed=page_size + d + 1)
    ks, vs = _pool_rows(cache.k_pages, cache.v_pages, cache.block_table, LENS, d)
    q = _rand_q(len(LENS), h, nq, d, "cuda")
    _run_windows(cache, q, ks, vs, LENS, causal, chunks, OUT_BF16, "ragged")


@pytest.mark.gpu
@pytest.mark.parametrize("chunks", [1, 7])
@pytest.mark.parametrize("page_size", [16, 64, 128])
def test_window_first_pass_hazard(page_size, chunks):
    """len 517, nq 1, window 216: lo = 300, base = 256.  At page 16 the pages
    of [0, 288) are released, so the row's first pass holds lanes whose table
    entry is -1 (256..287), lanes of a live page below lo (288..299) and
    attended lanes.  At page 64 / 128 the pass's page is live and its first
    lane is below lo: the scalar page id must not come from a lo-predicated
    read."""
    torch.manual_seed(300 + page_size)
    lens, w, d = [517], 216, 64
    cache = _hand_built(lens, page_size, 2, d, "cuda", seed=page_size + 3)
    ks, vs = _pool_rows(cache.k_pages, cache.v_pages, cache.block_table, lens, d)
    q = _rand_q(1, 4, 1, d, "cuda")
    spans = _spans(lens, 1, True, w)
    assert spans == [[(300, 517)]]
    cache.release_prefix([300])
    assert cache.host_starts == [300 // page_size * page_size]
    if page_size == 16:
        assert cache.host_starts == [288]
        assert cache.block_table[0, :19].cpu().tolist()[15:] == [-1, -1, -1] + \
            cache.pages_of(0)[18:19]
    _poison_unheld(cache)
    out, lse = _local_paged_decode_partial(q, cache, causal=True, chunks=chunks, window=w)
    _check(out, lse, *_oracle(q, ks, vs, spans), OUT_BF16, f"hazard ps{page_size}")


@pytest.mark.gpu
@pytest.mark.parametrize("nq", [1, 3])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("page_size", [16, 64])
def test_window_counting_probe(page_size, causal, nq):
    """q = 0 makes every attended key weigh the same: exp(lse) counts the keys
    (limit - lo) and, with v[j] = (j % 128, j // 128) — both exact in bf16 —
    128 * out[1] + out[0] is their mean position (lo + limit - 1) / 2.  An
    off-by-one at either end moves the count by 1, a shifted span moves the
    mean by 1; fp32 error at these sizes is below 1e-2, the bound is 0.25."""
    hk, h, d = 2, 2, 64
    n = max(LENS)
    j = torch.arange(n)
    k = torch.randn(len(LENS), hk, n, d).to(torch.bfloat16)
    v = torch.zeros(len(LENS), hk, n, d)
    v[..., 0] = (j % 128).float()
    v[..., 1] = (j // 128).float()
    cache = PagedKVCache.from_dense(k.cuda(), v.to(torch.bfloat16).cuda(), LENS,
                                    page_size, shuffle_seed=page_size)
    q = torch.zeros(len(LENS), h, nq, d, dtype=torch.bfloat16, device="cuda")
    for w in WINDOWS:
        spans = _spans(LENS, nq, causal, w)
        out, lse = _local_paged_decode_partial(q, cache, causal=causal, window=w)
        out, lse = out.cpu(), lse.cpu()
        assert torch.isfinite(out).all() and torch.isfinite(lse).all()
        for i, rows in enumerate(spans):
            for iq, (lo, hi) in enumerate(rows):
                if lo >= hi:
                    assert hi == 0
                    assert (out[i, :, iq] == 0).all() and (lse[i, :, iq] <= -1e30).all()
                    continue
                count = lse[i, :, iq, 0].exp()
                mean = 128 * out[i, :, iq, 1] + out[i, :, iq, 0]
                assert (count - (hi - lo)).abs().max() < 0.25, (w, i, iq, lo, hi, count)
                assert (mean - (lo + hi - 1) / 2).abs().max() < 0.25, (w, i, iq, lo, hi, mean)


@pytest.mark.gpu
@pytest.mark.parametrize("page_size", [16, 64])
def test_window_same_definition_as_prefill(page_size):
    """Decode rows == paged_prefill_attn(q_lens = 4, causal, window) on the
    same cache.  Prefill returns bf16: v is drawn at 0.1 * randn so |out| <
    0.5 and the bf16 rounding of the prefill output (<= 2^-9 * 0.5 = 1e-3)
    stays inside OUT_BF16."""
    torch.manual_seed(400 + page_size)
    lens, hk, h, nq, d = [5, 63, 130, 517], 2, 4, 4, 64
    k = torch.randn(len(lens), hk, max(lens), d).to(torch.bfloat16).cuda()
    v = (0.1 * torch.randn(len(lens), hk, max(lens), d)).to(torch.bfloat16).cuda()
    assert v.float().abs().max() < 0.5
    cache = PagedKVCache.from_dense(k, v, lens, page_size, shuffle_seed=6)
    q = _rand_q(len(lens), h, nq, d, "cuda")
    for w in [0, 5, 64, 300]:
        out, lse = _local_paged_decode_partial(q, cache, causal=True, window=w)
        p_out, p_lse = paged_prefill_attn(q.transpose(1, 2).contiguous(), cache,
                                          [nq] * len(lens), causal=True, window=w,
                                          return_lse=True)
        e_out = (out - p_out.float().transpose(1, 2)).abs().max().item()
        e_lse = (lse[..., 0] - p_lse).abs().max().item()
        print(f"prefill w={w} out err {e_out:.3e} lse err {e_lse:.3e}")
        assert e_out < OUT_BF16 and e_lse < LSE_TOL, (w, e_out, e_lse)


@pytest.mark.gpu
@pytest.mark.parametrize("chunks", [0, 7])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("heads", [(4, 4, 1), (6, 2, 3)])
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("page_size", [16, 64])
def test_window_ragged_fp8(page_size, d, heads, causal, chunks):
    """test_window_ragged on an fp8 pool built through the quantising append,
    against the oracle on the dequantised pool."""
    h, hk, nq = heads
    torch.manual_seed(500 + page_size + d + h)
    k = torch.randn(len(LENS), hk, max(LENS), d).to(torch.bfloat16).cuda()
    v = torch.randn(len(LENS), hk, max(LENS), d).to(torch.bfloat16).cuda()
    cache = PagedKVCache.from_dense(k, v, LENS, page_size, fp8=True, shuffle_seed=5,
                                    spare_pages=4)
    ks, vs = _pool_rows(cache.k_pages, cache.v_pages, cache.block_table, LENS, d,
                        cache.k_scales, cache.v_scales)
    for s, n in enumerate(LENS):                # rows past each length: NaN
        if n % page_size:
            last = cache.pages_of(s)[-1]
            cache.k_pages[last, :, n % page_size:] = 0x7f
            cache.v_pages[last, :, n % page_size:] = 0x7f
    q = _rand_q(len(LENS), h, nq, d, "cuda")
    _run_windows(cache, q, ks, vs, LENS, causal, chunks, OUT_FP8, "fp8")


@pytest.mark.gpu
def test_window_grow_decode_release():
    """60 steps of append one token, decode with window 20, release: two
    sequences from [14, 30] at page 16 reach [74, 90], 11 pages without
    release, in a pool of 8.  Each sequence holds at most
    ceil((window + nq) / page) + 1 = 3 pages."""
    torch.manual_seed(600)
    hk, h, d, ps, w = 2, 4, 64, 16, 20
    start = [14, 30]
    k0 = torch.randn(2, hk, 30, d).to(torch.bfloat16).cuda()
    v0 = torch.randn(2, hk, 30, d).to(torch.bfloat16).cuda()
    cache = PagedKVCache(8, ps, hk, d, 2, 6, device="cuda")
    cache.append(k0, v0, start)
    hist_k = [k0[i, :, :n].float().cpu() for i, n in enumerate(start)]
    hist_v = [v0[i, :, :n].float().cpu() for i, n in enumerate(start)]
    starts = cache.host_starts
    for step in range(60):
        kn = torch.randn(2, hk, 1, d).to(torch.bfloat16).cuda()
        vn = torch.randn(2, hk, 1, d).to(torch.bfloat16).cuda()
        cache.append(kn, vn)
        assert cache.free_pages >= 8 - 2 * 3, (step, cache.free_pages)
        for i in range(2):
            hist_k[i] = torch.cat((hist_k[i], kn[i].float().cpu()), dim=1)
            hist_v[i] = torch.cat((hist_v[i], vn[i].float().cpu()), dim=1)
        lens = cache.host_lens
        q = _rand_q(2, h, 1, d, "cuda")
        out, lse = _local_paged_decode_partial(q, cache, causal=True, window=w)
        _check(out, lse, *_oracle(q, hist_k, hist_v, _spans(lens, 1, True, w)),
               OUT_BF16, f"step {step}")
        # the next query sits at position len: nothing below len - w is
        # attended again
        cache.release_prefix([max(0, n - w) for n in lens])
        assert all(a <= b for a, b in zip(starts, cache.host_starts))
        starts = cache.host_starts
    assert cache.host_lens == [74, 90] and cache.seq_lens.cpu().tolist() == [74, 90]
    assert cache.host_starts == [48, 64]
    assert cache.pages_held() == 4 and cache.free_pages == 4


def _loopback_case(world, w, device, dtype, hk, h, d):
    lens, nq, ps = [37, 300], 2, 16
    k = torch.randn(2, hk, max(lens), d).to(torch.bfloat16).to(device)
    v = torch.randn(2, hk, max(lens), d).to(torch.bfloat16).to(device)
    q = torch.randn(2, h, nq, d).to(dtype).to(device)
    single = PagedKVCache.from_dense(k, v, lens, ps, shuffle_seed=9)
    ref = tree_attn_decode_paged(q, single, causal=True, window=w)
    caches = _sharded_caches(k, v, lens, world, ps, device)
    after = [[sum(c.host_lens[i] for c in caches[r + 1:]) for i in range(2)]
             for r in range(world)]
    assert after[-1] == [0, 0]

    def run(rank):
        return tree_attn_decode_paged(q, caches[rank], causal=rank == world - 1,
                                      window=w, kv_after=after[rank])

    outs = loopback_world(world, run)
    # rank 0 holds keys (of every sequence at world 4), but with the small
    # window all of them lie outside it: its partial is dead (weight 0 in the
    # merge) for every row
    if w == 10:
        assert caches[0].host_lens[1] > 0 and (world == 2 or caches[0].host_lens[0] > 0)
        o0, l0 = _local_paged_decode_partial(q, caches[0], window=w, kv_after=after[0])
        assert (o0 == 0).all() and torch.isfinite(l0).all() and (l0 <= -1e30).all()
    return ref, outs, (q, k, v, lens, nq)


@pytest.mark.gpu
@pytest.mark.parametrize("w", [10, 100])
@pytest.mark.parametrize("world", [2, 4])
def test_window_loopback_multirank(world, w):
    torch.manual_seed(700 + world + w)
    ref, outs, _ = _loopback_case(world, w, "cuda", torch.bfloat16, 2, 4, 64)
    for rank, out in enumerate(outs):
        e = (out.float() - ref.float()).abs().max().item()
        s = ref.float().abs().max().item() + 1e-6
        assert e / s < 2e-2, f"rank {rank} rel err {e/s}"


# --------------------------------------------------------------------------
# CPU
# --------------------------------------------------------------------------
def _state_full(cache):
    return _state(cache), cache.host_starts, [cache.pages_of(s)
                                              for s in range(cache.max_seqs)]


def _same_state_full(cache, saved):
    base, starts, pages = saved
    return (_same_state(cache, base) and cache.host_starts == starts
            and [cache.pages_of(s) for s in range(cache.max_seqs)] == pages)


def test_window_allocator_cpu():
    torch.manual_seed(800)
    ps = 16
    cache = PagedKVCache(8, ps, 1, 16, 2, 6)
    k = torch.randn(2, 1, 70, 16).to(torch.bfloat16)
    cache.append(k, k, [70, 20])                       # 5 + 2 pages
    p0 = cache.pages_of(0)
    assert cache.free_pages == 1 and cache.host_starts == [0, 0]
    gk_full, _ = cache.gather(0)

    # pages wholly below 40 -> slots 0, 1; sequence 1: nothing below 10
    assert cache.release_prefix([40, 10]) == 2
    assert cache.host_starts == [32, 0] and cache.free_pages == 3
    assert cache.block_table[0].tolist() == [-1, -1] + p0[2:] + [-1]
    assert cache.pages_of(0) == [-1, -1] + p0[2:] and cache.pages_held(0) == 3
    assert cache.host_lens == [70, 20] and cache.seq_lens.tolist() == [70, 20]

    # the same prefix again, and a smaller one: no-ops
    saved = _state_full(cache)
    assert cache.release_prefix([40, 10]) == 0 and _same_state_full(cache, saved)
    assert cache.release_prefix([5, 0]) == 0 and _same_state_full(cache, saved)

    # gather keeps its shape; released rows are zeros, the rest unchanged
    gk, gv = cache.gather(0)
    assert gk.shape == (1, 70, 16)
    assert (gk[:, :32] == 0).all() and (gv[:, :32] == 0).all()
    assert torch.equal(gk[:, 32:], gk_full[:, 32:])

    # append continues at the absolute position: slot 70 >> 4 = 4 is full at
    # 80, then slot 5; the table row (6 slots) still bounds the length
    cache.append(k[:, :, :12], k[:, :, :12], [12, 0])
    assert cache.host_lens == [82, 20] and len(cache.pages_of(0)) == 6
    assert cache.block_table[0, :2].tolist() == [-1, -1]
    assert (cache.block_table[0, 2:] >= 0).all()
    gk, _ = cache.gather(0)
    assert torch.equal(gk[:, 70:82], k[0, :, :12]) and (gk[:, :32] == 0).all()
    saved = _state_full(cache)
    with pytest.raises(RuntimeError):                  # 82 + 20 > 6 * 16
        cache.append(k[:, :, :20], k[:, :, :20], [20, 0])
    assert _same_state_full(cache, saved)

    # keep_from beyond seq_len: only whole pages below seq_len go
    assert cache.release_prefix([1000, 1000]) == 3 + 1
    assert cache.host_starts == [80, 16]
    assert cache.pages_held(0) == 1 and cache.pages_held(1) == 1
    assert cache.free_pages == 8 - 2

    # free after a release returns only what is still held
    cache.free(0)
    assert cache.free_pages == 7 and cache.host_starts == [0, 16]
    assert cache.host_lens == [0, 20] and cache.block_table[0].tolist() == [-1] * 6
    cache.append(k[:, :, :33], k[:, :, :33], [33, 0])
    held = [pg for s in range(2) for pg in cache.pages_of(s) if pg >= 0]
    assert len(held) == 4 and len(set(held)) == 4 and cache.free_pages == 4
    with pytest.raises(ValueError):
        cache.release_prefix([1])
    with pytest.raises(ValueError):
        cache.release_prefix([-1, 0])


def test_window_guard_cpu():
    """A call that would attend below the released prefix raises ValueError
    from the host mirrors and leaves every tensor and mirror unchanged."""
    torch.manual_seed(810)
    lens, hk, h, nq, d, ps = [70, 40], 1, 2, 2, 16, 16
    k = torch.randn(2, hk, 70, d).to(torch.bfloat16)
    cache = PagedKVCache.from_dense(k, k, lens, ps, spare_pages=1)
    q = torch.randn(2, h, nq, d)
    qp = q.transpose(1, 2).contiguous()
    cache.release_prefix([40, 0])                      # starts [32, 0]
    assert cache.host_starts == [32, 0]
    saved = _state_full(cache)
    for causal in (False, True):
        # rows of sequence 0 sit at 68, 69: window 36 reaches key 32, 37 key 31
        tree_attn_decode_paged(q, cache, causal=causal, window=36)
        paged_prefill_attn(qp, cache, [nq, nq], causal=causal, window=36)
        for bad in (None, 37, 10000):
            with pytest.raises(ValueError):
                tree_attn_decode_paged(q, cache, causal=causal, window=bad)
            with pytest.raises(ValueError):
                _local_paged_decode_partial(q, cache, causal=causal, window=bad)
            with pytest.raises(ValueError):
                paged_prefill_attn(qp, cache, [nq, nq], causal=causal, window=bad)
        assert _same_state_full(cache, saved)
    # a later rank's keys move the queries forward: the same window is fine
    _local_paged_decode_partial(q, cache, window=37, kv_after=[1, 0])
    # a sequence that attends nothing in this call is not held to the guard
    paged_prefill_attn(qp, cache, [0, nq], window=0)
    with pytest.raises(ValueError):
        tree_attn_decode_paged(q, cache, window=-1)
    with pytest.raises(ValueError):
        _local_paged_decode_partial(q, cache, window=5, kv_after=[0])
    assert _same_state_full(cache, saved)


@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("causal", [False, True])
def test_window_fallback_cpu(fp8, causal):
    """Eager windowed decode vs the oracle: ragged lengths, a zero-length
    row, GQA, nq = 3, head dim 16 stored padded, pages released first."""
    torch.manual_seed(820)
    lens, hk, h, nq, d, ps = [0, 5, 33, 70], 2, 4, 3, 16, 16
    k = torch.randn(4, hk, max(lens), d).to(torch.bfloat16)
    v = torch.randn(4, hk, max(lens), d).to(torch.bfloat16)
    cache = PagedKVCache.from_dense(k, v, lens, ps, fp8=fp8, shuffle_seed=3,
                                    spare_pages=2)
    ks, vs = _pool_rows(cache.k_pages, cache.v_pages, cache.block_table, lens, d,
                        cache.k_scales, cache.v_scales)
    q = _rand_q(4, h, nq, d, "cpu")
    for w in [10000, 40, 16, 3, 0]:
        spans = _spans(lens, nq, causal, w)
        cache.release_prefix(_keep_from(spans))
        _poison_unheld(cache)
        out, lse = _local_paged_decode_partial(q, cache, causal=causal, window=w)
        ref_out, ref_lse, live = _oracle(q, ks, vs, spans)
        _check_dead(live, spans, lens, nq)
        m = live[:, None, :, None].expand_as(lse)
        assert (out - ref_out).abs().max().item() < 1e-5, w
        assert (lse[m] - ref_lse[m]).abs().max().item() < 1e-5, w
        assert (out[~m.expand_as(out)] == 0).all()
        assert torch.isfinite(lse).all() and (lse[~m] <= -1e30).all()
    assert cache.host_starts == [0, 0, 16, 64]


@pytest.mark.parametrize("w", [10, 100])
@pytest.mark.parametrize("world", [2, 4])
def test_window_loopback_cpu(world, w):
    torch.manual_seed(830 + world + w)
    ref, outs, (q, k, v, lens, nq) = _loopback_case(world, w, "cpu", torch.float32,
                                                    1, 3, 16)
    ks = [k[i, :, :n].float() for i, n in enumerate(lens)]
    vs = [v[i, :, :n].float() for i, n in enumerate(lens)]
    want = _oracle(q, ks, vs, _spans(lens, nq, True, w))[0]
    assert (ref - want).abs().max().item() < 1e-5
    for rank, out in enumerate(outs):
        e = (out - ref).abs().max().item()
        assert e < 1e-5, f"rank {rank} err {e}"


def test_window_example_runs():
    def run(*extra):
        r = subprocess.run(
            [sys.executable, os.path.join(ROOT, "examples", "serve_tree_decode.py"),
             "--paged", "--kv-len", "256", "--steps", "4", *extra],
            capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        held = re.search(r"pages held (\d+)", r.stdout)
        assert held, r.stdout
        return int(held.group(1)), r.stdout

    full, _ = run()
    windowed, out = run("--window", "64")
    assert "window 64" in out and "us/token" in out
    assert 0 < windowed < full, (windowed, full)
