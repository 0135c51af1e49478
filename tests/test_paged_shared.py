"""Shared-prefix paged decode: `PagedKVCache.share_prefix` and the work-unit
kernel behind `tree_attn_decode_paged(..., shared_prefix=True)`.

Oracle, judge and bounds are tests/test_paged_grouped.py's (its docstring
derives them): fp64 `rows_oracle` over the raw pool rows gathered by table,
|out - ref| <= 2^-8 * mag, |lse - ref| <= 1e-3, dead rows exactly 0 with
lse <= -1e30.  The out bound survives the fp32 merge of prefix and suffix
partials: the merge weights the partials' errors and their mags alike.
"""

import pytest
import torch

from ring_attention_amd import PagedKVCache
from ring_attention_amd.tree_decode import _local_paged_decode_partial

from .test_paged_grouped import BOUND, _judge, _tree_mask

GROUP_A, GROUP_B, SINGLE, SLOTS = [0, 1, 2, 3, 4], [5, 6], 7, 9


def _forked_cache(ps, hk, d, fp8, nq, masked, device, seed=0):
    """Group A: five sequences behind 3 pages; group B: two behind one page;
    one unshared sequence of 129 tokens; one empty slot.  Pages are handed out
    in a seeded random order.  Returns the cache and the dense (k, v) every
    sequence was built from."""
    gen = torch.Generator().manual_seed(seed + ps + d)
    cache = PagedKVCache(80, ps, hk, d, SLOTS, 16, fp8=fp8, device=device)
    cache._free = torch.randperm(cache.num_pages, generator=gen).tolist()
    first = [0] * SLOTS
    first[GROUP_A[0]], first[GROUP_B[0]], first[SINGLE] = 3 * ps, ps, 129
    sfx_a = [1 if masked else 0, nq + 1, nq + 31, nq + 33, nq + 130]
    second = sfx_a + [nq, nq + 2, 0, 0]
    dense = []
    for lens in (first, second):
        k = torch.randn(SLOTS, hk, max(lens), d, generator=gen).to(torch.bfloat16)
        v = torch.randn(SLOTS, hk, max(lens), d, generator=gen).to(torch.bfloat16)
        cache.append(k.to(device), v.to(device), lens)
        dense.append((k, v, lens))
        if lens is first:
            for dst in GROUP_A[1:]:
                cache.share_prefix(GROUP_A[0], dst, 3 * ps)
            cache.share_prefix(GROUP_B[0], GROUP_B[1], ps)
    return cache, dense


def _expected_dense(dense, seq):
    (k1, v1, l1), (k2, v2, l2) = dense
    src = GROUP_A[0] if seq in GROUP_A else GROUP_B[0] if seq in GROUP_B else seq
    return (torch.cat([k1[src, :, :l1[src]], k2[seq, :, :l2[seq]]], dim=1),
            torch.cat([v1[src, :, :l1[src]], v2[seq, :, :l2[seq]]], dim=1))


def _mode_args(mode, nq, device):
    """(call kwargs, per-sequence masks for _judge)."""
    if mode == "plain":
        return {}, [None] * SLOTS
    if mode == "causal":
        return dict(causal=True), [torch.ones(nq, nq, dtype=torch.bool).tril()] * SLOTS
    masks = torch.stack([_tree_mask(nq, 70 + i) for i in range(SLOTS)])
    return dict(tree_mask=masks.to(device)), list(masks)


@pytest.mark.parametrize("fp8", [False, True])
def test_share_prefix_allocator(fp8):
    ps, hk, d, nq = 16, 2, 16, 2
    cache = PagedKVCache(12, ps, hk, d, 4, 4, fp8=fp8)
    gen = torch.Generator().manual_seed(1)
    k0 = torch.randn(4, hk, 40, d, generator=gen).to(torch.bfloat16)
    v0 = torch.randn(4, hk, 40, d, generator=gen).to(torch.bfloat16)
    cache.append(k0, v0, [40, 0, 0, 5])

    def state():
        return cache.free_pages, cache.block_table.clone(), cache.host_lens

    before = state()
    for src, dst, tokens in ((0, 3, 32), (0, 1, 24), (0, 1, 48)):
        with pytest.raises(ValueError):
            cache.share_prefix(src, dst, tokens)
    after = state()
    assert before[0] == after[0] and before[2] == after[2] and (before[1] == after[1]).all()

    src_k, src_v = cache.gather(0)
    cache.share_prefix(0, 1, 32)
    cache.share_prefix(0, 2, 32)
    assert cache.free_pages == 12 - 4 and cache.host_lens[:3] == [40, 32, 32]
    assert sorted(cache.prefix_groups()) == [([0, 1, 2], 32)]
    k1 = torch.randn(4, hk, 20, d, generator=gen).to(torch.bfloat16)
    v1 = torch.randn(4, hk, 20, d, generator=gen).to(torch.bfloat16)
    cache.append(k1, v1, [0, 3, 20, 0])
    assert cache.pages_held(1) == 3 and cache.pages_held() == 3 + 1 + 2 + 1
    assert all(torch.equal(a, b) for a, b in zip(cache.gather(0), (src_k, src_v)))
    # every sequence reads as the dense tokens it was built from: bf16 as
    # given, fp8 as an unshared cache stores the same rows
    lens = [40, 35, 52, 5]
    full = [torch.zeros(4, hk, 52, d, dtype=torch.bfloat16) for _ in range(2)]
    for x, x0, x1 in zip(full, (k0, v0), (k1, v1)):
        x[0, :, :40], x[3, :, :5] = x0[0], x0[3, :, :5]
        for seq, n_new in ((1, 3), (2, 20)):
            x[seq, :, :32], x[seq, :, 32:32 + n_new] = x0[0, :, :32], x1[seq, :, :n_new]
    plain = PagedKVCache.from_dense(*full, lens, ps, fp8=fp8)
    ref = cache.gather(0)
    for seq, n in enumerate(lens):
        for got, exp, x in zip(cache.gather(seq), plain.gather(seq), full):
            assert torch.equal(got, exp) and (fp8 or torch.equal(got, x[seq, :, :n]))

    q = torch.randn(4, 4, nq, d, generator=gen).to(torch.bfloat16)
    base = _local_paged_decode_partial(q, cache, causal=True)
    shared = _local_paged_decode_partial(q, cache, causal=True, shared_prefix=True)
    assert all((a - b).abs().max() <= 1e-5 for a, b in zip(base, shared))

    cache.free(0)                       # the shared pages stay with 1 and 2
    assert cache.free_pages == 12 - cache.pages_held() == 12 - 6
    assert torch.equal(cache.gather(1)[0][:, :32], ref[0][:, :32])
    released = PagedKVCache(4, ps, hk, d, 2, 4, fp8=fp8)
    released.append(k0[:2], v0[:2], [40, 0])
    released.release_prefix([16, 0])
    table = released.block_table.clone()
    with pytest.raises(ValueError):
        released.share_prefix(0, 1, 32)
    assert released.free_pages == 2 and torch.equal(released.block_table, table)
    for seq in (1, 2, 3):
        cache.free(seq)
    assert cache.free_pages == cache.num_pages and cache.prefix_groups() == []


def test_shared_prefix_argument_errors():
    cache, _ = _forked_cache(16, 2, 16, False, 2, False, "cpu")
    q = torch.randn(SLOTS, 4, 2, 16).to(torch.bfloat16)
    gone = PagedKVCache(8, 16, 2, 16, SLOTS, 4)
    gone.append(torch.zeros(SLOTS, 2, 40, 16), torch.zeros(SLOTS, 2, 40, 16), [40] + [0] * 8)
    gone.release_prefix([16] + [0] * 8)
    for c, kw in ((cache, dict(window=8)), (cache, dict(kv_after=[0] * SLOTS)),
                  (cache, dict(grouped=False)), (gone, dict())):
        with pytest.raises(ValueError):
            _local_paged_decode_partial(q, c, shared_prefix=True, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("chunks", [0, 3])
@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("page_size", [16, 64])
@pytest.mark.parametrize("G,nq,mode", [(1, 1, "plain"), (4, 3, "causal"), (8, 5, "tree")])
def test_shared_prefix_kernel(G, nq, mode, page_size, d, fp8, chunks):
    """Group A stacks 5, 60 and 200 rows per kv head: a partial tile, tiles
    across sequences, two-tile units with an odd tile left over.  P = 48 at
    page size 16 splits a 32-key block between prefix and suffix; in the
    masked modes the member with a 1-token suffix falls out of the prefix."""
    hk = 2
    cache, dense = _forked_cache(page_size, hk, d, fp8, nq, mode != "plain", "cuda")
    assert sorted(cache.prefix_groups()) == [(GROUP_A, 3 * page_size), (GROUP_B, page_size)]
    if not fp8:
        for seq in (GROUP_A[-1], GROUP_B[1]):
            assert all(torch.equal(g.cpu(), e)
                       for g, e in zip(cache.gather(seq), _expected_dense(dense, seq)))
    torch.manual_seed(G * 100 + nq)
    q = torch.randn(SLOTS, G * hk, nq, d).to(torch.bfloat16).cuda()
    kw, masks = _mode_args(mode, nq, "cuda")
    out, lse = _local_paged_decode_partial(q, cache, chunks=chunks, shared_prefix=True, **kw)
    _judge(out, lse, q, cache, cache.host_lens, masks, BOUND, f"shared {mode}")


@pytest.mark.gpu
def test_shared_prefix_matches_grouped():
    G, hk, nq, d = 8, 2, 5, 64
    cache, _ = _forked_cache(16, hk, d, False, nq, True, "cuda")
    torch.manual_seed(9)
    q = torch.randn(SLOTS, G * hk, nq, d).to(torch.bfloat16).cuda()
    kw, masks = _mode_args("tree", nq, "cuda")
    out, lse = _local_paged_decode_partial(q, cache, shared_prefix=True, **kw)
    mags = _judge(out, lse, q, cache, cache.host_lens, masks, BOUND, "shared")
    ref, _ = _local_paged_decode_partial(q, cache, grouped=True, **kw)
    for i, mag in enumerate(mags):
        if mag is not None:
            diff = (out[i] - ref[i]).abs().double().cpu()
            print(f"shared vs grouped seq {i}: {float((diff / mag).max()):.3g}")
            assert (diff <= 2 * BOUND * mag).all()
