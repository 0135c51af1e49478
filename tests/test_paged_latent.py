"""MLA latent-cache paged decode (d_qk 576, d_v 512): PagedLatentCache and
tree_attn_decode_mla.

The oracle is fp64 `rows_oracle` over the dense rows the cache was built
from: every head reads the 576-wide row as its key and the first 512 columns
as its value.

Bound: |out - ref| <= (2^-8 + 1e-5) * mag (mag = the reference with |v|).
2^-8 is the one bf16 rounding of P (derived in tests/test_paged_grouped.py),
1e-5 the project's fp32 eager bound.  |lse - ref| <= 1e-3 on live rows; dead
rows are exactly 0 with lse <= -1e30.
"""

import pytest
import torch

from ring_attention_amd import PagedLatentCache, tree_attn_decode_mla
from ring_attention_amd.tree_decode import _local_mla_decode_partial

from .fp8_emulation import relative_failures, rows_oracle

BOUND, EAGER_BOUND, LSE_TOL = 2.0 ** -8 + 1e-5, 1e-5, 1e-3
LENS = [0, 1, 31, 32, 33, 127, 128, 129, 300]
DK, DV = 576, 512


def _rows(lens, seed):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(len(lens), 1, max(max(lens), 1), DK, generator=gen).to(torch.bfloat16)


def _judge(out, lse, q, ckv, lens, causal, scale, bound, tag):
    b, h, nq, _ = q.shape
    assert out.shape == (b, h, nq, DV) and lse.shape == (b, h, nq, 1)
    for i, n in enumerate(lens):
        limit = (n - (nq - 1 - torch.arange(nq))).clamp(min=0) if causal \
            else torch.full((nq,), n)
        vis = torch.arange(max(n, 1))[None, :] < limit[:, None]
        live = limit > 0
        o, l = out[i].cpu(), lse[i, ..., 0].cpu()
        assert (o[:, ~live] == 0).all() and (l[:, ~live] <= -1e30).all(), f"{tag} dead rows"
        if not live.any():
            continue
        kd = ckv[i, :, :max(n, 1)].cpu().expand(h, -1, -1)
        ref, mag, ref_lse = rows_oracle(q[i].cpu(), kd, kd[..., :DV], scale, vis)
        relative_failures(o[:, live], ref[:, live], mag[:, live], bound, f"{tag} seq {i}")
        e_lse = (l[:, live].double() - ref_lse[:, live]).abs().max().item()
        assert e_lse <= LSE_TOL, f"{tag} seq {i} lse err {e_lse}"


@pytest.mark.gpu
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("chunks", [0, 3])
@pytest.mark.parametrize("page_size", [16, 64, 256])
@pytest.mark.parametrize("h,nq", [(16, 1), (16, 3), (128, 2)])
def test_latent_ragged(h, nq, page_size, chunks, causal):
    """Half a tile, 1.5 tiles across head boundaries and 8 tiles over a ragged
    batch with an empty slot, shuffled tables, empty chunks at chunks = 3."""
    lens = [n for n in LENS if not causal or n >= nq or n == 0]
    ckv = _rows(lens, 7 + page_size).cuda()
    cache = PagedLatentCache.from_dense(ckv, lens, page_size, shuffle_seed=page_size + nq,
                                        spare_pages=2)
    torch.manual_seed(h + nq)
    q = torch.randn(len(lens), h, nq, DK).to(torch.bfloat16).cuda()
    out, lse = _local_mla_decode_partial(q, cache, causal, chunks=chunks)
    _judge(out, lse, q, ckv, lens, causal, DK ** -0.5, BOUND, "latent")


@pytest.mark.gpu
@pytest.mark.parametrize("rising", [True, False])
def test_latent_rescale_paths(rising):
    """All heads' q point the same way (gain 6), and the keys are sorted by
    their score: rising, every block rescales; falling, the skip arm is taken
    after block 0."""
    torch.manual_seed(11)
    u = torch.randn(DK)
    q = (6.0 * u * torch.linspace(0.5, 1.5, 16)[:, None]).to(torch.bfloat16)
    ckv = _rows([300], 13)
    order = (ckv[0, 0].float() @ u).argsort(descending=not rising)
    ckv = ckv[:, :, order].contiguous().cuda()
    cache = PagedLatentCache.from_dense(ckv, [300], 64, shuffle_seed=3)
    q = q.view(1, 16, 1, DK).cuda()
    out, lse = _local_mla_decode_partial(q, cache, chunks=1)
    _judge(out, lse, q, ckv, [300], False, DK ** -0.5, BOUND, f"rising={rising}")


@pytest.mark.gpu
def test_latent_append_and_merge512():
    lens1, lens2 = [5, 0, 40, 17], [20, 3, 0, 47]
    new = _rows([48] * 4, 17)
    caches = [PagedLatentCache(12, 16, 4, 6, device=dev) for dev in ("cpu", "cuda")]
    for c in caches:
        c.append(new[:, :, :40].to(c.device), lens1)
        c.append(new.to(c.device), lens2)
    assert torch.equal(caches[1].k_pages.cpu(), caches[0].k_pages)
    assert torch.equal(caches[1].block_table.cpu(), caches[0].block_table)
    assert caches[1].seq_lens.tolist() == [25, 3, 40, 64]

    from ring_attention_amd.ops import hip_ext
    torch.manual_seed(19)
    outs = torch.randn(5, 2, 3, 2, DV, device="cuda")
    lses = torch.randn(5, 2, 3, 2, 1, device="cuda") * 3
    out, lse = hip_ext.require().decode_merge(outs, lses)
    w = torch.softmax(lses.double(), dim=0)
    relative_failures(out, (w * outs.double()).sum(0).cpu(),
                      (w * outs.double().abs()).sum(0).cpu(), EAGER_BOUND, "merge 512")
    assert ((lse - lses.double().logsumexp(0)).abs() <= EAGER_BOUND).all()


def test_latent_cpu():
    lens, h, nq = [0, 2, 40, 33], 4, 3
    ckv = _rows(lens, 23)
    cache = PagedLatentCache.from_dense(ckv, lens, 16, shuffle_seed=5, spare_pages=3)
    assert cache.v_pages.data_ptr() == cache.k_pages.data_ptr()
    k, v = cache.gather(2)
    assert k.shape == (1, 40, DK) and v.shape == (1, 40, DV)
    assert torch.equal(k, ckv[2, :, :40]) and torch.equal(v, k[..., :DV])
    torch.manual_seed(29)
    q = torch.randn(4, h, nq, DK).to(torch.bfloat16)
    for causal, scale in ((False, None), (True, 0.1)):
        out, lse = _local_mla_decode_partial(q, cache, causal, scale)
        _judge(out, lse, q, ckv, lens, causal, scale or DK ** -0.5, EAGER_BOUND, "cpu")
    assert tree_attn_decode_mla(q, cache).dtype == q.dtype

    # bookkeeping on the subclass: fork, overflow, free, release
    cache.share_prefix(2, 0, 32)
    assert cache.prefix_groups() == [([0, 2], 32)] and cache.host_lens[0] == 32
    assert torch.equal(cache.gather(0)[0], ckv[2, :, :32])
    free, pool = cache.free_pages, cache.k_pages.clone()
    with pytest.raises(RuntimeError):
        cache.append(ckv[:, :, :40], [40, 0, 0, 0])
    assert cache.free_pages == free and torch.equal(cache.k_pages, pool)
    cache.free(2)
    assert cache.free_pages == free + 1 and cache.pages_held(0) == 2
    cache.release_prefix([16, 0, 0, 0])
    with pytest.raises(ValueError):
        tree_attn_decode_mla(q, cache)
    for dims in ((256, 64), (512, 128)):
        with pytest.raises(ValueError):
            PagedLatentCache(4, 16, 1, 4, *dims)
