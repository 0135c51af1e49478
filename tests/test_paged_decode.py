"""Paged KV-cache decode: block-table pages + per-sequence lengths.

Every oracle here is computed in the test, in fp32 on the CPU, and never
goes through the library's own gather or eager fallback: keys are gathered
from the raw pools by table and length (or kept as a dense history), masked
by length and causal tail, and softmaxed.  The fp32 partials of
`_local_paged_decode_partial` are compared, not the bf16-cast public output.

Bounds (the project's own, tests/test_gpu_kernels.py): out max-abs 3e-3 for
a bf16 cache, 5e-3 for an fp8 cache against the oracle on the DEQUANTISED
cache, lse max-abs 2e-3.
"""

import os
import subprocess
import sys

import pytest
import torch

from ring_attention_amd import PagedKVCache, tree_attn_decode_paged
from ring_attention_amd.ops.fp8 import quantize_kv_cache
from ring_attention_amd.tree_decode import _local_paged_decode_partial

from .loopback_dist import loopback_world

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

OUT_BF16, OUT_FP8, LSE_TOL = 3e-3, 5e-3, 2e-3


# --------------------------------------------------------------------------
# in-test oracle
# --------------------------------------------------------------------------
def _pool_rows(k_pages, v_pages, table, lens, d, k_scales=None, v_scales=None):
    """Per-sequence dense fp32 [(hk, L, d)] k and v lists, gathered by hand
    from the raw pools (dequantised when scales are given)."""
    ps = k_pages.shape[2]
    table = table.cpu().tolist()
    ks, vs = [], []
    for b, n in enumerate(lens):
        ids = table[b][:(n + ps - 1) // ps]
        assert all(i >= 0 for i in ids)
        out = []
        for pool, sc in ((k_pages, k_scales), (v_pages, v_scales)):
            x = pool.cpu()[ids]                               # (np, hk, ps, D)
            if sc is not None:
                x = (x.view(torch.float8_e4m3fn).float()
                     * torch.exp2(sc.cpu()[ids].float() - 127.0)[..., None])
            x = x.float().permute(1, 0, 2, 3).reshape(pool.shape[1], -1, pool.shape[3])
            out.append(x[:, :n, :d])
        ks.append(out[0])
        vs.append(out[1])
    return ks, vs


def _oracle(q, ks, vs, causal):
    """fp32 attention of q (b, h, nq, d) over per-sequence k/v [(hk, L, d)]
    with the qh % hk pairing.  Returns (out (b,h,nq,d), lse (b,h,nq,1),
    live (b,nq) bool); rows with no visible key have out = 0, lse = -inf."""
    q = q.detach().float().cpu()
    b, h, nq, d = q.shape
    out = torch.zeros(b, h, nq, d)
    lse = torch.full((b, h, nq, 1), float("-inf"))
    live = torch.zeros(b, nq, dtype=torch.bool)
    for i in range(b):
        n = ks[i].shape[1]
        hk = ks[i].shape[0]
        for iq in range(nq):
            limit = max(0, n - (nq - 1 - iq)) if causal else n
            if limit == 0:
                continue
            live[i, iq] = True
            for qh in range(h):
                kk = ks[i][qh % hk, :limit].float()
                vv = vs[i][qh % hk, :limit].float()
                s = (kk @ q[i, qh, iq]) * d ** -0.5
                lse[i, qh, iq, 0] = torch.logsumexp(s, dim=0)
                out[i, qh, iq] = torch.softmax(s, dim=0) @ vv
    return out, lse, live


def _check(out, lse, ref_out, ref_lse, live, out_tol, tag=""):
    out, lse = out.float().cpu(), lse.float().cpu()
    assert torch.isfinite(out).all() and torch.isfinite(lse).all(), f"{tag} non-finite"
    m = live[:, None, :, None].expand_as(lse)
    e_out = (out - ref_out).abs().max().item()
    e_lse = (lse[m] - ref_lse[m]).abs().max().item() if m.any() else 0.0
    print(f"{tag} out err {e_out:.3e} lse err {e_lse:.3e}")
    assert e_out < out_tol, f"{tag} out err {e_out}"
    assert e_lse < LSE_TOL, f"{tag} lse err {e_lse}"
    dead = ~m
    if dead.any():                      # limit-0 rows: exact zero, finite lse
        assert (out[dead.expand_as(out)] == 0).all(), f"{tag} dead row out != 0"
        assert (lse[dead] <= -1e30).all(), f"{tag} dead row lse"


def _hand_built(lens, page_size, hk, kd, device, seed, spare=5):
    """Shuffled bf16 pool with spare pages; spare pages and the rows at or
    beyond seq_len inside each last page are NaN, unused table entries -1."""
    gen = torch.Generator().manual_seed(seed)
    per_seq = [(n + page_size - 1) // page_size for n in lens]
    num_pages = sum(per_seq) + spare
    perm = torch.randperm(num_pages, generator=gen).tolist()
    k_pages = torch.full((num_pages, hk, page_size, kd), float("nan"), dtype=torch.bfloat16)
    v_pages = torch.full_like(k_pages, float("nan"))
    table = torch.full((len(lens), max(max(per_seq), 1) + 1), -1, dtype=torch.int32)
    for b, n in enumerate(lens):
        k = torch.randn(hk, n, kd, generator=gen).to(torch.bfloat16)
        v = torch.randn(hk, n, kd, generator=gen).to(torch.bfloat16)
        for s in range(per_seq[b]):
            pg = perm.pop()
            table[b, s] = pg
            rows = min(page_size, n - s * page_size)
            k_pages[pg, :, :rows] = k[:, s * page_size:s * page_size + rows]
            v_pages[pg, :, :rows] = v[:, s * page_size:s * page_size + rows]
    lens_t = torch.tensor(lens, dtype=torch.int32)
    return PagedKVCache.from_pages(k_pages.to(device), v_pages.to(device),
                                   table.to(device), lens_t.to(device))


def _rand_q(b, h, nq, d, device, dtype=torch.bfloat16):
    return torch.randn(b, h, nq, d).to(dtype).to(device)


# --------------------------------------------------------------------------
# GPU
# --------------------------------------------------------------------------
RAGGED = [
    (16, (4, 4, 1), 64), (16, (6, 2, 3), 128), (16, (6, 2, 3), 64),
    (64, (4, 4, 1), 128), (64, (6, 2, 3), 64),
    (128, (4, 4, 1), 64), (128, (6, 2, 3), 128), (128, (4, 4, 1), 128),
]


@pytest.mark.gpu
@pytest.mark.parametrize("chunks", [0, 7])
@pytest.mark.parametrize("page_size,heads,d", RAGGED)
def test_paged_ragged(page_size, heads, d, chunks):
    """Ragged batch over a shuffled, NaN-poisoned pool: catches a
    dereferenced invalid table entry, a read past the length, an unwritten
    empty-chunk partial and a wrong page / row split."""
    h, hk, nq = heads
    lens = [1, 63, 130, 517]
    torch.manual_seed(100 + page_size + d + h)
    cache = _hand_built(lens, page_size, hk, d, "cuda", seed=page_size + d)
    q = _rand_q(len(lens), h, nq, d, "cuda")
    out, lse = _local_paged_decode_partial(q, cache, chunks=chunks)
    torch.cuda.synchronize()
    ks, vs = _pool_rows(cache.k_pages, cache.v_pages, cache.block_table, lens, d)
    _check(out, lse, *_oracle(q, ks, vs, False), OUT_BF16, "ragged")


@pytest.mark.gpu
def test_paged_empty_sequence():
    torch.manual_seed(7)
    lens = [0, 40]
    cache = _hand_built(lens, 16, 2, 64, "cuda", seed=1)
    q = _rand_q(2, 4, 2, 64, "cuda")
    out, lse = _local_paged_decode_partial(q, cache)
    assert (out[0] == 0).all()
    assert torch.isfinite(lse[0]).all() and (lse[0] <= -1e30).all()
    ks, vs = _pool_rows(cache.k_pages, cache.v_pages, cache.block_table, lens, 64)
    _check(out, lse, *_oracle(q, ks, vs, False), OUT_BF16, "empty")


@pytest.mark.gpu
@pytest.mark.parametrize("page_size", [16, 64])
def test_paged_causal_tail(page_size):
    """nq = 4 with the draft tokens already cached; the first sequence is
    shorter than nq, so its query 0 sees nothing."""
    torch.manual_seed(11)
    lens = [3, 200]
    cache = _hand_built(lens, page_size, 2, 64, "cuda", seed=2)
    q = _rand_q(2, 4, 4, 64, "cuda")
    out, lse = _local_paged_decode_partial(q, cache, causal=True)
    ks, vs = _pool_rows(cache.k_pages, cache.v_pages, cache.block_table, lens, 64)
    ref = _oracle(q, ks, vs, True)
    assert not ref[2][0, 0] and ref[2][0, 1]
    _check(out, lse, *ref, OUT_BF16, "causal")


APPEND_START, APPEND_T, APPEND_LENS = [13, 0, 16], 8, [8, 0, 5]


def _append_setup(d, fp8, device="cuda"):
    """Cache at lengths [13, 0, 16] (page 16) with the whole pool then
    overwritten by a sentinel; returns (cache, k_new, v_new)."""
    hk, ps = 2, 16
    cache = PagedKVCache(8, ps, hk, d, 3, 3, fp8=fp8, device=device)
    z = torch.zeros(3, hk, 16, d, dtype=torch.bfloat16, device=device)
    cache.append(z, z, APPEND_START)
    if fp8:
        cache.k_pages.fill_(0x25)
        cache.v_pages.fill_(0x25)
        cache.k_scales.fill_(0x5a)
        cache.v_scales.fill_(0x5a)
    else:
        cache.k_pages.view(torch.int16).fill_(0x4d4e)
        cache.v_pages.view(torch.int16).fill_(0x4d4e)
    k_new = torch.randn(3, hk, APPEND_T, d).to(torch.bfloat16).to(device)
    v_new = torch.randn(3, hk, APPEND_T, d).to(torch.bfloat16).to(device)
    return cache, k_new, v_new


def _append_targets(cache):
    """[(seq, t, page, row)] of every appended token, from the device table."""
    table = cache.block_table.cpu().tolist()
    ps = cache.page_size
    return [(s, t, table[s][(APPEND_START[s] + t) // ps], (APPEND_START[s] + t) % ps)
            for s in range(3) for t in range(APPEND_LENS[s])]


@pytest.mark.gpu
@pytest.mark.parametrize("d", [64, 128])
def test_paged_append_bf16(d):
    """Crosses a page boundary (13 + 8), does nothing for one sequence and
    starts exactly on a boundary (16) for another."""
    torch.manual_seed(21)
    cache, k_new, v_new = _append_setup(d, fp8=False)
    before_k = cache.k_pages.clone()
    before_v = cache.v_pages.clone()
    cache.append(k_new, v_new, APPEND_LENS)
    torch.cuda.synchronize()
    for s, t, pg, row in _append_targets(cache):
        assert pg >= 0
        before_k[pg, :, row] = k_new[s, :, t]
        before_v[pg, :, row] = v_new[s, :, t]
    # written rows bit-equal to their source, every other row untouched
    assert torch.equal(cache.k_pages.view(torch.int16), before_k.view(torch.int16))
    assert torch.equal(cache.v_pages.view(torch.int16), before_v.view(torch.int16))
    want = [a + b for a, b in zip(APPEND_START, APPEND_LENS)]
    assert cache.seq_lens.cpu().tolist() == want and cache.host_lens == want


def _check_append_fp8(cache, k_new, v_new):
    """Appended rows bit-equal to quantize_kv_cache (scale bytes identical,
    dequantised values torch.equal), every other row untouched."""
    k8, v8, ks, vs = quantize_kv_cache(k_new.cpu(), v_new.cpu())
    written = torch.zeros(cache.k_scales.shape, dtype=torch.bool)
    for pool, scales, ref8, refs, src in (
            (cache.k_pages, cache.k_scales, k8, ks, k_new.cpu()),
            (cache.v_pages, cache.v_scales, v8, vs, v_new.cpu())):
        pool, scales = pool.cpu(), scales.cpu()
        for s, t, pg, row in _append_targets(cache):
            written[pg, :, row] = True
            assert torch.equal(scales[pg, :, row], refs[s, :, t]), (s, t)
            got = pool[pg, :, row].view(torch.float8_e4m3fn).float()
            ref = ref8[s, :, t].view(torch.float8_e4m3fn).float()
            if not torch.equal(got, ref):
                bad = (got != ref).nonzero()
                raise AssertionError(
                    f"seq {s} tok {t}: {bad.shape[0]} values differ, first "
                    f"input {src[s, :, t][tuple(bad[0])].item()!r} "
                    f"got {got[tuple(bad[0])].item()} want {ref[tuple(bad[0])].item()}")
        assert (pool[~written] == 0x25).all()
        assert (scales[~written] == 0x5a).all()
    want = [a + b for a, b in zip(APPEND_START, APPEND_LENS)]
    assert cache.seq_lens.cpu().tolist() == want and cache.host_lens == want


@pytest.mark.gpu
@pytest.mark.parametrize("d", [64, 128])
def test_paged_append_fp8(d):
    """Fused quantising append == quantize_kv_cache on the same rows: scale
    bytes identical, dequantised values torch.equal (+-0 compare equal)."""
    torch.manual_seed(22)
    cache, k_new, v_new = _append_setup(d, fp8=True)
    cache.append(k_new, v_new, APPEND_LENS)
    torch.cuda.synchronize()
    _check_append_fp8(cache, k_new, v_new)


@pytest.mark.gpu
@pytest.mark.parametrize("d", [64, 128])
def test_paged_append_fp8_gains(d):
    """The same append (13 + 8 crosses a page) with every appended row at its
    own gain 2^[-4, 4]: neighbouring rows carry different scale bytes, so a
    scale written to the wrong row or page breaks the bit-equality."""
    torch.manual_seed(23)
    cache, k_new, v_new = _append_setup(d, fp8=True)
    gains = lambda: torch.exp2(torch.randint(-4, 5, k_new.shape[:3] + (1,)).float()).cuda()
    k_new = (k_new.float() * gains()).to(torch.bfloat16)
    v_new = (v_new.float() * gains()).to(torch.bfloat16)
    _, _, ks, vs = quantize_kv_cache(k_new.cpu(), v_new.cpu())
    assert ks.unique().numel() >= 5 and vs.unique().numel() >= 5
    cache.append(k_new, v_new, APPEND_LENS)
    torch.cuda.synchronize()
    _check_append_fp8(cache, k_new, v_new)


@pytest.mark.gpu
@pytest.mark.parametrize("d", [64, 128])
def test_paged_fp8_decode(d):
    """Cache built through the fp8 append; spare pages and the rows past
    each length hold 0x7f (e4m3 NaN)."""
    torch.manual_seed(31)
    lens, ps, (h, hk, nq) = [70, 517], 64, (8, 2, 2)
    k = torch.randn(2, hk, max(lens), d).to(torch.bfloat16).cuda()
    v = torch.randn(2, hk, max(lens), d).to(torch.bfloat16).cuda()
    cache = PagedKVCache.from_dense(k, v, lens, ps, fp8=True, shuffle_seed=5,
                                    spare_pages=4)
    used = {pg for s in range(2) for pg in cache.pages_of(s)}
    spare = [pg for pg in range(cache.num_pages) if pg not in used]
    assert len(spare) == 4
    cache.k_pages[spare] = 0x7f
    cache.v_pages[spare] = 0x7f
    for s, n in enumerate(lens):
        last = cache.pages_of(s)[-1]
        cache.k_pages[last, :, n % ps:] = 0x7f
        cache.v_pages[last, :, n % ps:] = 0x7f
    q = _rand_q(2, h, nq, d, "cuda")
    out, lse = _local_paged_decode_partial(q, cache)
    ks, vs = _pool_rows(cache.k_pages, cache.v_pages, cache.block_table, lens, d,
                        cache.k_scales, cache.v_scales)
    _check(out, lse, *_oracle(q, ks, vs, False), OUT_FP8, "fp8")


@pytest.mark.gpu
@pytest.mark.parametrize("ps", [16, 64])
def test_paged_fp8_decode_gains(ps):
    """Rows at their own gains 2^[-4, 4] through the fp8 append, queries
    leaning on the rows around page and 64-key boundaries (15|16, 63|64,
    127|128, 511|512).  Judged relative to mag = softmax |v| against the fp64
    oracle on the dequantised pool: bound B_FP32 (tests/fp8_emulation.py:
    fp32 eager floor 1.0e-6, neighbour-scale ceiling 0.205)."""
    from .fp8_emulation import (B_FP32, CACHE_GAINS_CASES, build_gains_cache,
                                relative_failures, rows_oracle)
    lens, hk, h, nq, d, edges = CACHE_GAINS_CASES["paged_decode"]
    q, k, v = build_gains_cache(lens, hk, h, nq, d, edges)
    cache = PagedKVCache.from_dense(k.cuda(), v.cuda(), lens, ps, fp8=True,
                                    shuffle_seed=5, spare_pages=2)
    out, lse = _local_paged_decode_partial(q.cuda(), cache)
    ks, vs = _pool_rows(cache.k_pages, cache.v_pages, cache.block_table, lens, d,
                        cache.k_scales, cache.v_scales)
    heads = torch.arange(h) % hk
    for i in range(len(lens)):
        ref, mag, ref_lse = rows_oracle(q[i], ks[i][heads], vs[i][heads], d ** -0.5)
        relative_failures(out[i], ref, mag, B_FP32, f"paged fp8 gains ps{ps} seq {i}")
        e_lse = (lse[i, ..., 0].double().cpu() - ref_lse).abs().max().item()
        assert e_lse < LSE_TOL, f"lse err {e_lse}"


@pytest.mark.gpu
def test_paged_grow_while_decoding():
    """20 steps of append-one-token-then-decode from lengths [14, 30] at
    page 16: crosses page boundaries mid-run and exercises the allocator.
    The oracle runs on a dense history kept outside the cache."""
    torch.manual_seed(41)
    hk, h, d, ps = 2, 4, 64, 16
    start = [14, 30]
    k0 = torch.randn(2, hk, 30, d).to(torch.bfloat16).cuda()
    v0 = torch.randn(2, hk, 30, d).to(torch.bfloat16).cuda()
    cache = PagedKVCache(8, ps, hk, d, 2, 4, device="cuda")
    cache.append(k0, v0, start)
    hist_k = [k0[i, :, :n].float().cpu() for i, n in enumerate(start)]
    hist_v = [v0[i, :, :n].float().cpu() for i, n in enumerate(start)]
    for step in range(20):
        kn = torch.randn(2, hk, 1, d).to(torch.bfloat16).cuda()
        vn = torch.randn(2, hk, 1, d).to(torch.bfloat16).cuda()
        cache.append(kn, vn)
        for i in range(2):
            hist_k[i] = torch.cat((hist_k[i], kn[i].float().cpu()), dim=1)
            hist_v[i] = torch.cat((hist_v[i], vn[i].float().cpu()), dim=1)
        q = _rand_q(2, h, 1, d, "cuda")
        out, lse = _local_paged_decode_partial(q, cache)
        _check(out, lse, *_oracle(q, hist_k, hist_v, False), OUT_BF16, f"step {step}")
    assert cache.host_lens == [34, 50] and cache.seq_lens.cpu().tolist() == [34, 50]


def _sharded_caches(k, v, lens, world, ps, device):
    """Uneven per-sequence shards; at least one (rank, sequence) pair holds
    0 tokens, and the tail rank holds >= nq - 1 tokens of every sequence."""
    b, hk, _, d = k.shape
    frac = {2: [[0.0, 1.0], [0.7, 0.3]],
            4: [[0.3, 0.0, 0.5, 0.2], [0.4, 0.1, 0.0, 0.5]]}[world]
    caches, held = [], []
    for r in range(world):
        lo = [int(n * sum(frac[i % 2][:r])) for i, n in enumerate(lens)]
        hi = [n if r == world - 1 else int(n * sum(frac[i % 2][:r + 1]))
              for i, n in enumerate(lens)]
        local = [e - s for s, e in zip(lo, hi)]
        held.append(local)
        t = max(max(local), 1)
        kr = torch.zeros(b, hk, t, d, dtype=k.dtype, device=device)
        vr = torch.zeros(b, hk, t, d, dtype=k.dtype, device=device)
        for i in range(b):
            kr[i, :, :local[i]] = k[i, :, lo[i]:hi[i]]
            vr[i, :, :local[i]] = v[i, :, lo[i]:hi[i]]
        caches.append(PagedKVCache.from_dense(kr, vr, local, ps, shuffle_seed=r))
    assert any(n == 0 for row in held for n in row)
    assert [sum(c) for c in zip(*held)] == lens
    return caches


@pytest.mark.gpu
@pytest.mark.parametrize("world", [2, 4])
def test_paged_loopback_multirank(world):
    torch.manual_seed(51 + world)
    lens, hk, h, nq, d, ps = [37, 300], 2, 4, 2, 64, 16
    k = torch.randn(2, hk, max(lens), d).to(torch.bfloat16).cuda()
    v = torch.randn(2, hk, max(lens), d).to(torch.bfloat16).cuda()
    q = _rand_q(2, h, nq, d, "cuda")
    single = PagedKVCache.from_dense(k, v, lens, ps, shuffle_seed=9)
    ref = tree_attn_decode_paged(q, single, causal=True)
    caches = _sharded_caches(k, v, lens, world, ps, "cuda")

    def run(rank):
        return tree_attn_decode_paged(q, caches[rank], causal=rank == world - 1)

    for rank, out in enumerate(loopback_world(world, run)):
        e = (out.float() - ref.float()).abs().max().item()
        s = ref.float().abs().max().item() + 1e-6
        assert e / s < 2e-2, f"rank {rank} rel err {e/s}"


# --------------------------------------------------------------------------
# CPU
# --------------------------------------------------------------------------
def _state(cache):
    t = [cache.k_pages, cache.v_pages, cache.block_table, cache.seq_lens]
    return [x.clone() for x in t], cache.host_lens, cache.free_pages


def _same_state(cache, saved):
    tensors, lens, free = saved
    now = [cache.k_pages, cache.v_pages, cache.block_table, cache.seq_lens]
    return (all(torch.equal(a.view(torch.int16) if a.dtype == torch.bfloat16 else a,
                            b.view(torch.int16) if b.dtype == torch.bfloat16 else b)
                for a, b in zip(now, tensors))
            and cache.host_lens == lens and cache.free_pages == free)


def test_paged_allocator_cpu():
    torch.manual_seed(61)
    cache = PagedKVCache(6, 16, 1, 16, 2, 4)
    k = torch.randn(2, 1, 64, 16)
    cache.append(k[:, :, :20], k[:, :, :20], [20, 5])
    p0, p1 = cache.pages_of(0), cache.pages_of(1)
    assert len(p0) == 2 and len(p1) == 1 and not set(p0) & set(p1)
    assert cache.free_pages == 3
    table = cache.block_table.tolist()
    assert table[0] == p0 + [-1, -1] and table[1] == p1 + [-1, -1, -1]

    saved = _state(cache)
    with pytest.raises(RuntimeError):       # pool: 2 + 3 pages wanted, 3 free
        cache.append(k[:, :, :48], k[:, :, :48], [40, 48])
    assert _same_state(cache, saved)
    with pytest.raises(RuntimeError):       # table row: 70 tokens = 5 pages > 4
        cache.append(k[:, :, :50], k[:, :, :50], [50, 0])
    assert _same_state(cache, saved)

    cache.free(0)
    assert cache.free_pages == 5 and cache.host_lens == [0, 5]
    assert cache.seq_lens.tolist() == [0, 5]
    assert cache.block_table[0].tolist() == [-1] * 4
    cache.append(k[:, :, :40], k[:, :, :40], [40, 30])
    pages = cache.pages_of(0) + cache.pages_of(1)
    assert len(pages) == 6 and len(set(pages)) == 6 and cache.free_pages == 0
    assert cache.host_lens == [40, 35]


@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("causal", [False, True])
def test_paged_fallback_cpu(fp8, causal):
    """Eager fallback vs the in-test oracle: ragged lengths, a zero-length
    row, GQA, nq = 3, and a head dim (16) stored zero-padded to 64."""
    torch.manual_seed(71)
    lens, hk, h, nq, d, ps = [0, 5, 33, 70], 2, 4, 3, 16, 16
    k = torch.randn(4, hk, max(lens), d).to(torch.bfloat16)
    v = torch.randn(4, hk, max(lens), d).to(torch.bfloat16)
    cache = PagedKVCache.from_dense(k, v, lens, ps, fp8=fp8, shuffle_seed=3,
                                    spare_pages=2)
    assert cache.k_pages.shape[-1] == 64
    q = _rand_q(4, h, nq, d, "cpu")
    out, lse = _local_paged_decode_partial(q, cache, causal=causal)
    ks, vs = _pool_rows(cache.k_pages, cache.v_pages, cache.block_table, lens, d,
                        cache.k_scales, cache.v_scales)
    ref_out, ref_lse, live = _oracle(q, ks, vs, causal)
    assert not live[0].any()
    m = live[:, None, :, None].expand_as(lse)
    assert (out - ref_out).abs().max().item() < 1e-5
    assert (lse[m] - ref_lse[m]).abs().max().item() < 1e-5
    assert (out[~m.expand_as(out)] == 0).all()
    assert torch.isfinite(lse).all() and (lse[~m] <= -1e30).all()


@pytest.mark.parametrize("fp8", [False, True])
def test_paged_from_dense_gather_cpu(fp8):
    torch.manual_seed(81)
    lens, hk, d = [17, 0, 64], 2, 64
    k = torch.randn(3, hk, 64, d).to(torch.bfloat16)
    v = torch.randn(3, hk, 64, d).to(torch.bfloat16)
    cache = PagedKVCache.from_dense(k, v, lens, 16, fp8=fp8, shuffle_seed=4)
    order = [pg for s in range(3) for pg in cache.pages_of(s)]
    assert sorted(order) == list(range(cache.num_pages)) and order != sorted(order)
    if fp8:
        k8, v8, ks, vs = quantize_kv_cache(k, v)
        k_ref = k8.view(torch.float8_e4m3fn).float() * torch.exp2(ks.float() - 127)[..., None]
        v_ref = v8.view(torch.float8_e4m3fn).float() * torch.exp2(vs.float() - 127)[..., None]
    else:
        k_ref, v_ref = k, v
    for i, n in enumerate(lens):
        gk, gv = cache.gather(i)
        assert gk.shape == (hk, n, d)
        assert torch.equal(gk, k_ref[i, :, :n]) and torch.equal(gv, v_ref[i, :, :n])


def test_paged_loopback_cpu():
    """Two-round cross-rank merge over ragged, unevenly sharded paged
    caches (one (rank, sequence) pair empty), causal tail on the last rank."""
    torch.manual_seed(91)
    world, lens, hk, h, nq, d, ps = 4, [37, 120], 1, 3, 2, 16, 16
    k = torch.randn(2, hk, max(lens), d).to(torch.bfloat16)
    v = torch.randn(2, hk, max(lens), d).to(torch.bfloat16)
    q = torch.randn(2, h, nq, d)
    single = PagedKVCache.from_dense(k, v, lens, ps, shuffle_seed=9)
    ref = tree_attn_decode_paged(q, single, causal=True)
    ks, vs = _pool_rows(single.k_pages, single.v_pages, single.block_table, lens, d)
    assert (ref - _oracle(q, ks, vs, True)[0]).abs().max().item() < 1e-5
    caches = _sharded_caches(k, v, lens, world, ps, "cpu")

    def run(rank):
        return tree_attn_decode_paged(q, caches[rank], causal=rank == world - 1)

    for rank, out in enumerate(loopback_world(world, run)):
        e = (out - ref).abs().max().item()
        assert e < 1e-5, f"rank {rank} err {e}"


def test_paged_example_runs():
    r = subprocess.run(
        [sys.executable, os.path.join(ROOT, "examples", "serve_tree_decode.py"),
         "--paged", "--kv-len", "256", "--steps", "4"],
        capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "paged" in r.stdout and "us/token" in r.stdout
