"""Varlen paged prefill: packed queries, one workgroup per work unit.

`paged_prefill_attn_varlen` against the fp32 oracle of tests/test_paged_prefill.py
(attention over rows gathered by hand from the raw pools) on the packed rows,
with that file's bounds for the bf16 forward: out max-abs < 2e-2, lse max-abs
< 2e-3, dead rows exactly out == 0 with lse <= -1e30, everything finite.
"""

import pytest
import torch

from ring_attention_amd import PagedKVCache, paged_prefill_attn, paged_prefill_attn_varlen
from ring_attention_amd.paged_prefill import plan_units

from .test_paged_decode import _hand_built, _pool_rows
from .test_paged_prefill import LSE_TOL, OUT_TOL, _oracle

# q_lens 0 and 1, a second q tile of 44 rows, a one-row chunk over 9 kv tiles
# (d 64) or 18 (d 128)
SEQ_LENS = [1, 63, 130, 517, 0, 1100]
Q_LENS = [1, 40, 130, 300, 0, 1]

_memo = {}


def _pack(x, q_lens, dim):
    """(b, T, ..) or (b, h, T) padded -> packed along the row axis."""
    return torch.cat([x[i].narrow(dim, 0, ql) for i, ql in enumerate(q_lens)], dim=dim)


def _queries(h, d, q_lens, seed):
    """bf16 randn queries: padded (NaN beyond q_lens) for the oracle, packed."""
    gen = torch.Generator().manual_seed(seed)
    q = torch.randn(len(q_lens), max(q_lens), h, d, generator=gen).to(torch.bfloat16)
    for i, ql in enumerate(q_lens):
        q[i, ql:] = float("nan")
    return q, _pack(q, q_lens, 0)


def _packed_ref(q_pad, ks, vs, q_lens, causal, window=None):
    out, lse, live = _oracle(q_pad, ks, vs, q_lens, causal, window)
    return _pack(out, q_lens, 0), _pack(lse, q_lens, 1), _pack(live, q_lens, 1)


def _check(out, lse, ref, tag):
    ref_out, ref_lse, live = ref
    out, lse = out.float().cpu(), lse.float().cpu()
    assert out.shape == ref_out.shape and lse.shape == ref_lse.shape
    assert torch.isfinite(out).all() and torch.isfinite(lse).all(), f"{tag} non-finite"
    e_out = (out - ref_out).abs().max().item()
    e_lse = (lse[live] - ref_lse[live]).abs().max().item() if live.any() else 0.0
    print(f"{tag} out err {e_out:.3e} lse err {e_lse:.3e}")
    assert e_out < OUT_TOL and e_lse < LSE_TOL, f"{tag} out {e_out} lse {e_lse}"
    dead = ~live
    assert (out[dead.t()] == 0).all() and (lse[dead] <= -1e30).all(), f"{tag} dead rows"


def _case(page_size, hk, d, fp8, device="cuda"):
    """Poisoned shuffled cache + its hand-gathered rows, built once."""
    key = (page_size, hk, d, fp8, device)
    if key not in _memo:
        if fp8:
            gen = torch.Generator().manual_seed(31 + page_size + d)
            n = max(SEQ_LENS)
            k = torch.randn(len(SEQ_LENS), hk, n, d, generator=gen).to(torch.bfloat16)
            v = torch.randn(len(SEQ_LENS), hk, n, d, generator=gen).to(torch.bfloat16)
            cache = PagedKVCache.from_dense(k.to(device), v.to(device), SEQ_LENS, page_size,
                                            fp8=True, shuffle_seed=5, spare_pages=3)
        else:
            cache = _hand_built(SEQ_LENS, page_size, hk, d, device, seed=page_size + d + hk)
        _memo[key] = (cache, _pool_rows(cache.k_pages, cache.v_pages, cache.block_table,
                                        SEQ_LENS, d, cache.k_scales, cache.v_scales))
    return _memo[key]


@pytest.mark.gpu
@pytest.mark.parametrize("unit_tiles", [2, 10**6, 0])
@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("h,hk,d", [(4, 4, 64), (6, 2, 64), (6, 2, 128)])
@pytest.mark.parametrize("page_size", [16, 256])
def test_varlen_ragged_poisoned(page_size, h, hk, d, causal, fp8, unit_tiles):
    """Ragged packed batch over a shuffled pool whose spare pages and rows
    beyond each length are NaN and whose unused table entries are -1.
    unit_tiles = 2 cuts the long sequences into 3 and 5 (d 64) shares and
    leaves shares empty; 10**6 is one unit per q tile; 0 is the planner."""
    cache, (ks, vs) = _case(page_size, hk, d, fp8)
    key = ("ref", page_size, h, hk, d, causal, fp8)
    if key not in _memo:
        q_pad, q = _queries(h, d, Q_LENS, 11 + h + d)
        _memo[key] = (q.cuda(), _packed_ref(q_pad, ks, vs, Q_LENS, causal))
    q, ref = _memo[key]
    out, lse = paged_prefill_attn_varlen(q, cache, Q_LENS, causal=causal,
                                         return_lse=True, unit_tiles=unit_tiles)
    torch.cuda.synchronize()
    assert out.dtype == torch.bfloat16 and lse.dtype == torch.float32
    _check(out, lse, ref, f"ps{page_size} h{h}/{hk} d{d} c{causal} fp8{fp8} u{unit_tiles}")


@pytest.mark.gpu
@pytest.mark.parametrize("page_size,d", [(16, 64), (256, 128)])
def test_varlen_single_share_equals_grid_kernel(page_size, d):
    """One unit per q tile walks the tiles and does the arithmetic of the
    grid launch with kv_split = 1: the rows < q_lens are bitwise equal."""
    h, hk = 6, 2
    cache, _ = _case(page_size, hk, d, False)
    q_pad, q = _queries(h, d, Q_LENS, 3 + d)
    out, lse = paged_prefill_attn_varlen(q.cuda(), cache, Q_LENS, return_lse=True,
                                         unit_tiles=10**6)
    ref_out, ref_lse = paged_prefill_attn(torch.nan_to_num(q_pad).cuda(), cache, Q_LENS,
                                          return_lse=True, kv_split=1)
    torch.cuda.synchronize()
    assert torch.equal(out, _pack(ref_out, Q_LENS, 0))
    assert torch.equal(lse, _pack(ref_lse, Q_LENS, 1))


@pytest.mark.gpu
@pytest.mark.parametrize("d", [64, 128])
def test_varlen_window_released_pages(d):
    """window = 20 in shares of 2 kv tiles on a cache whose pages below the
    window were released; a wider window is refused before any launch."""
    h, hk, ps, w = 4, 2, 16, 20
    gen = torch.Generator().manual_seed(17 + d)
    n = max(SEQ_LENS)
    k = torch.randn(len(SEQ_LENS), hk, n, d, generator=gen).to(torch.bfloat16).cuda()
    v = torch.randn(len(SEQ_LENS), hk, n, d, generator=gen).to(torch.bfloat16).cuda()
    cache = PagedKVCache.from_dense(k, v, SEQ_LENS, ps, shuffle_seed=4, spare_pages=2)
    ks, vs = _pool_rows(cache.k_pages, cache.v_pages, cache.block_table, SEQ_LENS, d)
    freed = cache.release_prefix([max(0, n - ql - w) for n, ql in zip(SEQ_LENS, Q_LENS)])
    assert freed > 0
    q_pad, q = _queries(h, d, Q_LENS, 23)
    out, lse = paged_prefill_attn_varlen(q.cuda(), cache, Q_LENS, causal=True, window=w,
                                         return_lse=True, unit_tiles=2)
    torch.cuda.synchronize()
    _check(out, lse, _packed_ref(q_pad, ks, vs, Q_LENS, True, w), f"window d{d}")
    with pytest.raises(ValueError):
        paged_prefill_attn_varlen(q.cuda(), cache, Q_LENS, causal=True, window=w + 100)


# --------------------------------------------------------------------------
# CPU
# --------------------------------------------------------------------------
@pytest.mark.parametrize("window", [None, 20])
@pytest.mark.parametrize("causal", [True, False])
def test_varlen_eager_fallback(causal, window):
    lens, q_lens, h, hk, d, ps = [1, 63, 130, 0], [1, 40, 70, 0], 4, 2, 64, 16
    cache = _hand_built(lens, ps, hk, d, "cpu", seed=2)
    ks, vs = _pool_rows(cache.k_pages, cache.v_pages, cache.block_table, lens, d)
    q_pad, q = _queries(h, d, q_lens, 6)
    out, lse = paged_prefill_attn_varlen(q, cache, torch.tensor(q_lens), causal=causal,
                                         window=window, return_lse=True)
    assert out.dtype == torch.bfloat16
    _check(out, lse, _packed_ref(q_pad, ks, vs, q_lens, causal, window), "eager")


def test_varlen_argument_checks():
    k = torch.randn(2, 2, 40, 64).to(torch.bfloat16)
    cache = PagedKVCache.from_dense(k, k.clone(), [5, 40], 16)
    q = torch.randn(13, 4, 64).to(torch.bfloat16)
    assert paged_prefill_attn_varlen(q, cache, [5, 8]).shape == q.shape
    for bad_q, bad_lens, kw in ((q, [5, 7], {}),              # total != sum(q_lens)
                                (q, [13], {}),                # q_lens length != b
                                (q, [6, 7], {}),              # q_len > seq_len
                                (q, [5, 8], {"window": -1}),
                                (q[..., :32], [5, 8], {}),
                                (q[:, :3], [5, 8], {})):
        with pytest.raises(ValueError):
            paged_prefill_attn_varlen(bad_q, cache, bad_lens, **kw)
    with pytest.raises(RuntimeError, match="require grad"):
        paged_prefill_attn_varlen(q.float().requires_grad_(), cache, [5, 8])


@pytest.mark.parametrize("unit_tiles", [0, 2])
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("h,d", [(4, 64), (6, 128), (64, 64)])
def test_varlen_planner(h, d, causal, unit_tiles):
    """Every live q tile's units are shares 0 .. count - 1 exactly once, the
    tiles' slot ranges tile [0, slots) without overlap, the merge table names
    the split tiles, and the planner's own unit count stays within
    live q tiles + target_workgroups / h."""
    target = 512
    units, merges, slots = plan_units(SEQ_LENS, Q_LENS, h, d, causal, None, unit_tiles,
                                      target_workgroups=target)
    live = {(i, x): sum(Q_LENS[:i]) + 256 * x
            for i, ql in enumerate(Q_LENS) for x in range(-(-ql // 256))}
    shares, spans = {}, []
    for seq, x, row0, z, count, slot0, *_ in units:
        assert row0 == live[(seq, x)]
        shares.setdefault((seq, x), []).append((z, count, slot0))
    assert shares.keys() == live.keys()
    for got in shares.values():
        count, slot0 = got[0][1], got[0][2]
        assert sorted(got) == [(z, count, slot0) for z in range(count)]
        if count > 1:
            spans.append((slot0, slot0 + count))
    spans.sort()
    assert [a for a, _ in spans] == [0] + [b for _, b in spans[:-1]]
    assert slots == (spans[-1][1] if spans else 0)
    assert sorted(m[0] for m in merges) == [a for a, _ in spans]
    if unit_tiles == 0:
        assert len(units) <= len(live) + target // h
    else:
        assert max(c for _, c, _ in sum(shares.values(), [])) == (5 if d == 64 else 9)
