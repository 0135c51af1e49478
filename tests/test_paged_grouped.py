"""Grouped MFMA paged decode with token-tree draft masks.

The oracle is fp64 `rows_oracle` over K/V taken from the raw pools by table
and length (dequantised for fp8) with an explicit (nq, n) visibility matrix;
the fp32 partial of `_local_paged_decode_partial` is judged with
`relative_failures`.

Bound: |out - ref| <= 2^-8 * mag (mag = the reference with |v|).  P is
rounded to bf16 and l is summed unrounded, so the PV error is one bf16
rounding per weight, relative to mag; the rest is fp32 at the level of the
row kernel (about 1e-6).  A bf16 rounding is off by up to 2^-8 relative
(half an ulp of 2^-7 at the bottom of a binade), so the bound is tight:
measured worst ratio 0.00377 (bound 0.00391), on the sequences of 1 + nq
keys, where one weight carries a row.  |lse - ref| <= 1e-3 on live rows; dead
rows are exactly 0 with lse <= -1e30.
"""

import pytest
import torch

from ring_attention_amd import PagedKVCache
from ring_attention_amd.tree_decode import _local_paged_decode_partial

from .fp8_emulation import (CACHE_GAINS_CASES, build_gains_cache, relative_failures,
                            rows_oracle)
from .test_paged_decode import _pool_rows

BOUND, LSE_TOL = 2.0 ** -8, 1e-3
PREFIXES = [0, 1, 31, 32, 33, 127, 128, 129, 300]


def _tree_mask(nq, seed):
    """Random parent list (draft t's parent < t, or none) -> (nq, nq) bool:
    a draft attends itself and its ancestors."""
    gen = torch.Generator().manual_seed(seed)
    mask = torch.eye(nq, dtype=torch.bool)
    for t in range(1, nq):
        parent = int(torch.randint(-1, t, (1,), generator=gen))
        if parent >= 0:
            mask[t] |= mask[parent]
    return mask


def _cache(lens, hk, d, ps, fp8, device, seed):
    gen = torch.Generator().manual_seed(seed)
    n = max(max(lens), 1)
    k = torch.randn(len(lens), hk, n, d, generator=gen).to(torch.bfloat16).to(device)
    v = torch.randn(len(lens), hk, n, d, generator=gen).to(torch.bfloat16).to(device)
    return PagedKVCache.from_dense(k, v, lens, ps, fp8=fp8, shuffle_seed=seed,
                                   spare_pages=2)


def _judge(out, lse, q, cache, lens, masks, bound, tag):
    """masks[i]: (nq, nq) bool draft visibility of sequence i, or None for
    every key visible.  Returns the per-sequence mag (None for an empty one)."""
    b, h, nq, d = q.shape
    ks, vs = _pool_rows(cache.k_pages, cache.v_pages, cache.block_table, lens, d,
                        cache.k_scales, cache.v_scales)
    heads = torch.arange(h) % cache.kv_heads
    mags = []
    for i, n in enumerate(lens):
        if n == 0:
            assert (out[i] == 0).all() and (lse[i] <= -1e30).all(), f"{tag} dead rows"
            mags.append(None)
            continue
        vis = torch.ones(nq, n, dtype=torch.bool)
        if masks[i] is not None:
            vis[:, n - nq:] = masks[i]
        ref, mag, ref_lse = rows_oracle(q[i].cpu(), ks[i][heads], vs[i][heads],
                                        d ** -0.5, vis)
        relative_failures(out[i], ref, mag, bound, f"{tag} seq {i}")
        e_lse = (lse[i, ..., 0].double().cpu() - ref_lse).abs().max().item()
        assert e_lse <= LSE_TOL, f"{tag} seq {i} lse err {e_lse}"
        mags.append(mag)
    return mags


@pytest.mark.gpu
@pytest.mark.parametrize("chunks", [0, 3])
@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("page_size", [16, 64])
@pytest.mark.parametrize("G,nq", [(2, 3), (8, 4), (8, 5)])
def test_grouped_tree_mask(G, nq, page_size, d, fp8, chunks):
    """R = 6, 32, 40 rows per kv head over a ragged batch with one empty
    slot, shuffled table, a different random tree per sequence."""
    hk = 2
    lens = [p + nq for p in PREFIXES[:4]] + [0] + [p + nq for p in PREFIXES[4:]]
    torch.manual_seed(G * 100 + nq)
    cache = _cache(lens, hk, d, page_size, fp8, "cuda", seed=7 + page_size + d)
    q = torch.randn(len(lens), G * hk, nq, d).to(torch.bfloat16).cuda()
    masks = torch.stack([_tree_mask(nq, 50 + i) for i in range(len(lens))])
    out, lse = _local_paged_decode_partial(q, cache, chunks=chunks, tree_mask=masks.cuda())
    _judge(out, lse, q, cache, lens, list(masks), BOUND, "tree")


@pytest.mark.gpu
def test_grouped_star_and_chain():
    G, hk, nq, d, lens = 8, 2, 5, 64, [129, 300]
    torch.manual_seed(3)
    cache = _cache(lens, hk, d, 64, False, "cuda", seed=11)
    q = torch.randn(2, G * hk, nq, d).to(torch.bfloat16).cuda()
    star = torch.eye(nq, dtype=torch.bool)
    chain = torch.ones(nq, nq, dtype=torch.bool).tril()
    out, lse = _local_paged_decode_partial(q, cache, tree_mask=star.cuda())
    _judge(out, lse, q, cache, lens, [star] * 2, BOUND, "star")
    row_out, _ = _local_paged_decode_partial(q, cache, causal=True)
    for kw in (dict(tree_mask=chain.cuda()), dict(grouped=True, causal=True)):
        out, lse = _local_paged_decode_partial(q, cache, **kw)
        mags = _judge(out, lse, q, cache, lens, [chain] * 2, BOUND, "chain")
        for i, mag in enumerate(mags):
            diff = (out[i] - row_out[i]).abs().double().cpu()
            print(f"chain vs row kernel seq {i}: {float((diff / mag).max()):.3g}")
            assert (diff <= 2 * BOUND * mag).all()


@pytest.mark.gpu
@pytest.mark.parametrize("ps", [16, 64])
def test_grouped_no_mask_gains(ps):
    """Rows at their own gains around page and block boundaries: a block
    boundary reading a neighbour's scale or page moves the output by far
    more than the bound."""
    lens, hk, h, nq, d, edges = CACHE_GAINS_CASES["paged_decode"]
    q, k, v = build_gains_cache(lens, hk, h, nq, d, edges)
    cache = PagedKVCache.from_dense(k.cuda(), v.cuda(), lens, ps, fp8=True,
                                    shuffle_seed=5, spare_pages=2)
    out, lse = _local_paged_decode_partial(q.cuda(), cache, grouped=True, causal=False)
    _judge(out, lse, q, cache, lens, [None] * len(lens), BOUND, f"gains ps{ps}")


def test_tree_mask_cpu_and_errors():
    lens, hk, h, nq, d = [0, 7, 40], 2, 4, 4, 16
    torch.manual_seed(5)
    cache = _cache(lens, hk, d, 16, True, "cpu", seed=13)
    q = torch.randn(3, h, nq, d).to(torch.bfloat16)
    masks = torch.stack([_tree_mask(nq, 60 + i) for i in range(3)])
    out, lse = _local_paged_decode_partial(q, cache, tree_mask=masks)
    _judge(out, lse, q, cache, lens, list(masks), 1e-5, "cpu tree")

    bad_diag = masks.clone()
    bad_diag[1, 2, 2] = False
    short = _cache([0, 3, 40], hk, d, 16, False, "cpu", seed=14)
    wide = torch.eye(65, dtype=torch.bool)
    for kw, c, qq in ((dict(tree_mask=bad_diag), cache, q),
                      (dict(tree_mask=wide), cache, q[:, :, :1].expand(3, h, 65, d)),
                      (dict(tree_mask=masks), short, q),
                      (dict(tree_mask=masks, causal=True), cache, q),
                      (dict(tree_mask=masks, window=8), cache, q),
                      (dict(tree_mask=masks, grouped=False), cache, q)):
        with pytest.raises(ValueError):
            _local_paged_decode_partial(qq, c, **kw)
