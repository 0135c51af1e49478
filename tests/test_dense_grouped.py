"""Grouped MFMA decode over the dense KV cache (csrc/decode_grouped.hip).

The oracle is fp64 `rows_oracle` on the (dequantised) operands with an
explicit (nq, n) visibility matrix.  Bounds are test_paged_grouped.py's:
|out - ref| <= 2^-8 * mag (one bf16 rounding of P per weight), |lse - ref| <=
1e-3, and an empty kv chunk's partial is exactly 0 with lse <= -1e30.  Two
results that each carry one such rounding differ by at most 2 * 2^-8 * mag; so
does a bf16 output (the cast is one more rounding of at most 2^-8 relative)
from an fp32 reference.
"""

import pytest
import torch

from ring_attention_amd.tree_decode import (_local_decode_partial, _tail_shard, _tree_bits,
                                            tree_attn_decode, tree_attn_decode_fp8)

from .fp8_emulation import (CACHE_GAINS_CASES, build_gains_cache, dequant_rows,
                            relative_failures, rows_oracle)
from .test_paged_grouped import _tree_mask

BOUND, LSE_TOL = 2.0 ** -8, 1e-3
PREFIXES = [0, 1, 31, 32, 33, 127, 128, 129, 300]


def _ext():
    from ring_attention_amd.ops import hip_ext
    return hip_ext.require()


def _judge(out, lse, q, kd, vd, masks, bound, tag):
    """q (b, h, nq, d), kd / vd (b, hk, n, d) as the kernel sees them, masks
    (b, nq, nq) bool or None.  Returns the per-sequence mag."""
    b, h, nq, d = q.shape
    n = kd.shape[2]
    heads = torch.arange(h) % kd.shape[1]
    mags = []
    for i in range(b):
        vis = torch.ones(nq, n, dtype=torch.bool)
        if masks is not None:
            vis[:, n - nq:] = masks[i]
        ref, mag, ref_lse = rows_oracle(q[i].cpu(), kd[i].cpu()[heads], vd[i].cpu()[heads],
                                        d ** -0.5, vis)
        relative_failures(out[i], ref, mag, bound, f"{tag} seq {i}")
        e_lse = (lse[i, ..., 0].double().cpu() - ref_lse).abs().max().item()
        assert e_lse <= LSE_TOL, f"{tag} seq {i} lse err {e_lse}"
        mags.append(mag)
    return mags


def _operands(b, hk, n, d, fp8, seed):
    """(k, v, kscale, vscale) for the binding and the (kd, vd) they stand for."""
    from ring_attention_amd.ops.fp8 import quantize_kv_cache
    gen = torch.Generator().manual_seed(seed)
    k = torch.randn(b, hk, n, d, generator=gen).to(torch.bfloat16).cuda()
    v = torch.randn(b, hk, n, d, generator=gen).to(torch.bfloat16).cuda()
    if not fp8:
        return (k, v, None, None), (k, v)
    k8, v8, ks, vs = quantize_kv_cache(k, v)
    return (k8, v8, ks, vs), (dequant_rows(k8.cpu(), ks.cpu()), dequant_rows(v8.cpu(), vs.cpu()))


@pytest.mark.gpu
@pytest.mark.parametrize("chunks", [0, 3])
@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("G,nq", [(2, 3), (8, 4), (8, 5), (8, 16), (8, 17)])
def test_dense_grouped_tree_mask(G, nq, d, fp8, chunks, monkeypatch):
    """R = 6, 32, 40, 128, 136 rows per kv head: one tile, an exact tile, two
    tiles, a full 4-tile workgroup, one tile more; a batch of 3 with its own
    random tree per sequence; every prefix length around a block and a pass.
    The launcher's limit of 2 tiles per workgroup is lifted to 4, so that
    every built variant runs (the other tests keep the default)."""
    monkeypatch.setenv("RING_ATTN_GROUPED_TILES", "4")
    hk, b, ext = 2, 3, _ext()
    torch.manual_seed(G * 100 + nq)
    q = torch.randn(b, G * hk, nq, d).to(torch.bfloat16).cuda()
    masks = torch.stack([_tree_mask(nq, 50 + i) for i in range(b)])
    bits = _tree_bits(masks.cuda())
    for p in PREFIXES:
        n = nq + p
        ops, (kd, vd) = _operands(b, hk, n, d, fp8, seed=7 + d + p)
        outs, lses = ext.decode_partial_grouped(q, *ops, d ** -0.5, chunks, bits)
        if chunks:      # [0, n) in `chunks` 128-key-aligned spans: the rest is empty
            per = (n + chunks - 1) // chunks
            per = (per + 127) // 128 * 128
            for s in range(chunks):
                if s * per >= n:
                    assert (outs[s] == 0).all() and (lses[s] <= -1e30).all(), f"p {p} chunk {s}"
        out, lse = ext.decode_merge(outs, lses)
        _judge(out, lse, q, kd, vd, masks, BOUND, f"tree p={p}")


@pytest.mark.gpu
def test_dense_grouped_tile_sharing_invisible(monkeypatch):
    G, hk, nq, d, n = 8, 2, 16, 64, 316
    torch.manual_seed(9)
    q = torch.randn(1, G * hk, nq, d).to(torch.bfloat16).cuda()
    ops, (kd, vd) = _operands(1, hk, n, d, False, seed=21)
    masks = _tree_mask(nq, 77)[None]
    got = {}
    for cap in ("1", None):
        if cap:
            monkeypatch.setenv("RING_ATTN_GROUPED_TILES", cap)
        else:
            monkeypatch.delenv("RING_ATTN_GROUPED_TILES", raising=False)
        out, lse = _local_decode_partial(q, ops[0], ops[1], vis=masks.cuda())
        mag, = _judge(out, lse, q, kd, vd, masks, BOUND, f"tiles cap {cap}")
        got[cap] = out
    diff = (got["1"][0] - got[None][0]).abs().double().cpu()
    print(f"one tile vs shared: {float((diff / mag).max()):.3g}, "
          f"equal {torch.equal(got['1'], got[None])}")
    assert (diff <= 2 * BOUND * mag).all()


@pytest.mark.gpu
def test_dense_grouped_gains_against_row_kernel():
    """fp8 rows at their own gains around block boundaries, no mask."""
    from ring_attention_amd.ops.fp8 import quantize_kv_cache
    lens, hk, h, nq, d, edges = CACHE_GAINS_CASES["decode"]
    q, k, v = build_gains_cache(lens, hk, h, nq, d, edges)
    q = q.cuda()
    k8, v8, ks, vs = quantize_kv_cache(k.cuda(), v.cuda())
    ext = _ext()
    out, lse = ext.decode_merge(*ext.decode_partial_grouped(q, k8, v8, ks, vs, d ** -0.5))
    row, _ = ext.decode_merge(*ext.decode_partial_fp8(q, k8, v8, ks, vs, d ** -0.5))
    mags = _judge(out, lse, q, dequant_rows(k8.cpu(), ks.cpu()),
                  dequant_rows(v8.cpu(), vs.cpu()), None, BOUND, "gains")
    for i, mag in enumerate(mags):
        diff = (out[i] - row[i]).abs().double().cpu()
        print(f"grouped vs row kernel seq {i}: {float((diff / mag).max()):.3g}")
        assert (diff <= 2 * BOUND * mag).all()


@pytest.mark.gpu
def test_dense_grouped_public_wrappers():
    """bf16 results of the GPU entry points against their own eager fallback
    on CPU copies in fp32; mag is that fallback over |v|."""
    from ring_attention_amd.ops.fp8 import quantize_kv_cache
    b, hk, h, nq, d, n = 2, 2, 8, 5, 64, 200
    torch.manual_seed(4)
    q = torch.randn(b, h, nq, d).to(torch.bfloat16)
    k = torch.randn(b, hk, n, d).to(torch.bfloat16)
    v = torch.randn(b, hk, n, d).to(torch.bfloat16)
    masks = torch.stack([_tree_mask(nq, 90 + i) for i in range(b)])
    kw = dict(tree_mask=masks, shard_kv_seq=False)
    out = tree_attn_decode(q.cuda(), k.cuda(), v.cuda(), tree_mask=masks.cuda(),
                           shard_kv_seq=False)
    assert out.dtype == torch.bfloat16
    relative_failures(out, tree_attn_decode(q.float(), k, v, **kw).double(),
                      tree_attn_decode(q.float(), k, v.abs(), **kw).double(), 2 * BOUND, "bf16")
    c8 = [t.cpu() for t in quantize_kv_cache(k.cuda(), v.cuda())]
    c8_abs = [c8[0], c8[1] & 0x7F, c8[2], c8[3]]        # e4m3 sign bit cleared
    out = tree_attn_decode_fp8(q.cuda(), *[t.cuda() for t in c8], causal=True)
    relative_failures(out, tree_attn_decode_fp8(q.float(), *c8, causal=True).double(),
                      tree_attn_decode_fp8(q.float(), *c8_abs, causal=True).double(),
                      2 * BOUND, "fp8 chain")


def test_dense_mask_cpu_and_errors():
    b, hk, h, nq, d, n = 3, 2, 4, 4, 16, 40
    torch.manual_seed(5)
    q, k, v = torch.randn(b, h, nq, d), torch.randn(b, hk, n, d), torch.randn(b, hk, n, d)
    masks = torch.stack([_tree_mask(nq, 60 + i) for i in range(b)])
    chain = torch.ones(nq, nq, dtype=torch.bool).tril()[None].expand(b, nq, nq)
    from ring_attention_amd.ops.fp8 import quantize_kv_cache
    c8 = quantize_kv_cache(k, v)
    kd8, vd8 = dequant_rows(c8[0], c8[2]), dequant_rows(c8[1], c8[3])
    heads = torch.arange(h) % hk
    for out, kd, vd, vis in (
            (tree_attn_decode(q, k, v, tree_mask=masks), k, v, masks),
            (tree_attn_decode(q, k, v, causal=True, shard_kv_seq=False), k, v, chain),
            (tree_attn_decode_fp8(q, *c8, tree_mask=masks), kd8, vd8, masks),
            (tree_attn_decode_fp8(q, *c8, causal=True), kd8, vd8, chain)):
        for i in range(b):
            full = torch.ones(nq, n, dtype=torch.bool)
            full[:, n - nq:] = vis[i]
            ref, mag, _ = rows_oracle(q[i], kd[i][heads], vd[i][heads], d ** -0.5, full)
            relative_failures(out[i], ref, mag, 1e-5, f"cpu seq {i}")

    bad_diag = masks.clone()
    bad_diag[1, 2, 2] = False
    q65 = q[:, :, :1].expand(b, h, 65, d)
    for kw, qq, kk in ((dict(tree_mask=bad_diag), q, k),
                       (dict(tree_mask=torch.eye(65, dtype=torch.bool)), q65, k.repeat(1, 1, 2, 1)),
                       (dict(tree_mask=masks), q, k[:, :, :3]),
                       (dict(tree_mask=masks, causal=True), q, k),
                       (dict(tree_mask=masks, grouped=False), q, k),
                       (dict(causal=True, grouped=False), q, k)):
        with pytest.raises(ValueError):
            tree_attn_decode(qq, kk, kk, **kw)
        with pytest.raises(ValueError):
            tree_attn_decode_fp8(qq, *quantize_kv_cache(kk, kk), **kw)
    # k.chunk(world): 40 keys over 8 ranks end on rank 7 with 5 keys, 41 keys
    # over 8 ranks (chunks of 6) on rank 6 with 5; 4 drafts fit, 6 do not
    assert _tail_shard(40, 8, 4, "t") == 7 and _tail_shard(41, 8, 4, "t") == 6
    assert _tail_shard(40, 1, 40, "t") == 0
    for n_, world, nq_ in ((40, 8, 6), (41, 8, 6), (3, 8, 2)):
        with pytest.raises(ValueError):
            _tail_shard(n_, world, nq_, "t")
