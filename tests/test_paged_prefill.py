"""Paged prefill attention over the block-table KV cache.

The oracle is fp32 attention on the CPU over rows gathered BY HAND from the
raw pools (`_pool_rows`, dequantised for fp8) with the position rule of
`paged_prefill_attn`: query t < q_lens[i] sits at seq_len[i] - q_lens[i] + t
and attends keys [0, seq_len[i]), `j <= pos` under causal, `pos - j <= w`
under a window.  It never goes through the library's gather or fallback.

Bounds are the project's own for the bf16 forward against an fp32 oracle on
randn inputs (tests/test_gpu_kernels.py): out max-abs < 2e-2, lse max-abs
< 2e-3 on live rows; dead rows exactly out == 0 with lse <= -1e30; everything
finite.  An fp8 pool keeps them: dequantisation to bf16 is exact.
"""

import pytest
import torch

from ring_attention_amd import PagedKVCache, paged_prefill_attn
from ring_attention_amd.paged_prefill import auto_kv_split
from ring_attention_amd.tree_decode import _local_paged_decode_partial

from .test_paged_decode import _hand_built, _pool_rows

OUT_TOL, LSE_TOL = 2e-2, 2e-3

SEQ_LENS = [1, 63, 130, 517, 0]
Q_LENS = [1, 40, 130, 300, 0]
T = 300


# --------------------------------------------------------------------------
# in-test oracle
# --------------------------------------------------------------------------
def _oracle(q, ks, vs, q_lens, causal, window=None):
    """q (b, T, h, d) over per-sequence fp32 k/v [(hk, L, d)] with the
    qh % hk pairing.  Returns out (b,T,h,d), lse (b,h,T) (-inf where dead),
    live (b,h,T) bool."""
    q = q.detach().float().cpu()
    b, t, h, d = q.shape
    out = torch.zeros(b, t, h, d)
    lse = torch.full((b, h, t), float("-inf"))
    for i in range(b):
        n, ql = ks[i].shape[1], q_lens[i]
        if ql == 0:
            continue
        heads = torch.arange(h) % ks[i].shape[0]
        kk, vv = ks[i][heads].float(), vs[i][heads].float()       # (h, n, d)
        sim = torch.einsum("thd,hjd->htj", q[i, :ql], kk) * d ** -0.5
        pos = (n - ql + torch.arange(ql))[:, None]
        j = torch.arange(n)[None, :]
        ok = torch.ones(ql, n, dtype=torch.bool)
        if causal:
            ok &= j <= pos
        if window is not None:
            ok &= pos - j <= window
        sim = sim.masked_fill(~ok[None], float("-inf"))
        row = sim.logsumexp(dim=-1)                               # (h, ql)
        p = torch.nan_to_num(torch.softmax(sim, dim=-1))
        out[i, :ql] = torch.einsum("htj,hjd->thd", p, vv)
        lse[i, :, :ql] = row
    return out, lse, torch.isfinite(lse)


def _check(out, lse, ref, tag=""):
    ref_out, ref_lse, live = ref
    out, lse = out.float().cpu(), lse.float().cpu()
    assert out.shape == ref_out.shape and lse.shape == ref_lse.shape
    assert torch.isfinite(out).all() and torch.isfinite(lse).all(), f"{tag} non-finite"
    e_out = (out - ref_out).abs().max().item()
    e_lse = (lse[live] - ref_lse[live]).abs().max().item() if live.any() else 0.0
    print(f"{tag} out err {e_out:.3e} lse err {e_lse:.3e}")
    assert e_out < OUT_TOL, f"{tag} out err {e_out}"
    assert e_lse < LSE_TOL, f"{tag} lse err {e_lse}"
    dead = ~live
    if dead.any():
        dead_o = dead.permute(0, 2, 1)[..., None].expand_as(out)
        assert (out[dead_o] == 0).all(), f"{tag} dead row out != 0"
        assert (lse[dead] <= -1e30).all(), f"{tag} dead row lse"


def _rand_q(b, t, h, d, q_lens, seed, device):
    """randn bf16 q whose rows at t >= q_lens[i] are NaN."""
    gen = torch.Generator().manual_seed(seed)
    q = torch.randn(b, t, h, d, generator=gen).to(torch.bfloat16)
    for i, ql in enumerate(q_lens):
        q[i, ql:] = float("nan")
    return q.to(device)


_memo = {}


def _ragged_case(page_size, hk, d, device):
    """Poisoned hand-built cache + its hand-gathered rows, built once."""
    key = (page_size, hk, d, device)
    if key not in _memo:
        cache = _hand_built(SEQ_LENS, page_size, hk, d, device, seed=page_size + d + hk)
        _memo[key] = (cache, _pool_rows(cache.k_pages, cache.v_pages,
                                        cache.block_table, SEQ_LENS, d))
    return _memo[key]


def _ragged_ref(page_size, h, hk, d, causal, device):
    key = ("ref", page_size, h, hk, d, causal, device)
    if key not in _memo:
        _, (ks, vs) = _ragged_case(page_size, hk, d, device)
        q = _rand_q(len(SEQ_LENS), T, h, d, Q_LENS, 11 + h + d, device)
        _memo[key] = (q, _oracle(q, ks, vs, Q_LENS, causal))
    return _memo[key]


# --------------------------------------------------------------------------
# GPU
# --------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kv_split", [1, 3])
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("h,hk,d", [(4, 4, 64), (6, 2, 64), (4, 4, 128), (6, 2, 128)])
@pytest.mark.parametrize("page_size", [16, 64, 256])
def test_prefill_ragged_poisoned(page_size, h, hk, d, causal, kv_split):
    """Ragged batch over a shuffled pool whose spare pages, rows beyond each
    length and dead q rows are NaN and whose unused table entries are -1:
    catches a dereferenced invalid entry, a read past the length, a wrong
    page / row split, an unwritten partial (the 3-way split leaves whole
    shares empty for the short sequences) and a NaN leaking across rows."""
    cache, _ = _ragged_case(page_size, hk, d, "cuda")
    q, ref = _ragged_ref(page_size, h, hk, d, causal, "cuda")
    out, lse = paged_prefill_attn(q, cache, Q_LENS, causal=causal,
                                  return_lse=True, kv_split=kv_split)
    torch.cuda.synchronize()
    assert out.dtype == torch.bfloat16 and lse.dtype == torch.float32
    _check(out, lse, ref, f"ragged ps{page_size} h{h}/{hk} d{d} c{causal} s{kv_split}")


@pytest.mark.gpu
@pytest.mark.parametrize("kv_split", [1, 2])
@pytest.mark.parametrize("page_size", [16, 256])
@pytest.mark.parametrize("d,dw", [(64, -1), (64, 0), (64, 1), (64, None),
                                  (128, -1), (128, 0), (128, 1), (128, None)])
def test_prefill_exact_mask_counts(d, dw, page_size, kv_split):
    """q = 0: every score is exactly 0, so round(exp(lse)) is the number of
    attended keys: min(pos, w) + 1 under causal + window w, pos + 1 without a
    window — w one below, at and one above the kv tile width."""
    kvblk = 128 if d == 64 else 64
    w = None if dw is None else kvblk + dw
    cache, _ = _ragged_case(page_size, 2, d, "cuda")
    q = torch.zeros(len(SEQ_LENS), T, 4, d, dtype=torch.bfloat16, device="cuda")
    out, lse = paged_prefill_attn(q, cache, Q_LENS, causal=True, window=w,
                                  return_lse=True, kv_split=kv_split)
    torch.cuda.synchronize()
    lse = lse.float().cpu()
    assert torch.isfinite(lse).all() and torch.isfinite(out.float()).all()
    for i, (n, ql) in enumerate(zip(SEQ_LENS, Q_LENS)):
        pos = n - ql + torch.arange(ql)
        want = (pos if w is None else pos.clamp(max=w)) + 1
        got = lse[i, :, :ql].exp().round().long()
        assert (got == want[None]).all(), \
            f"seq {i} w {w}: first mismatch at row {(got != want[None]).nonzero()[0].tolist()}"
        assert (lse[i, :, ql:] <= -1e30).all()


@pytest.mark.gpu
@pytest.mark.parametrize("kv_split", [1, 3])
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("page_size", [16, 128])
def test_prefill_fp8_pool(page_size, d, causal, kv_split):
    """The ragged case over an fp8 pool (e4m3 rows + e8m0 row scales) built
    by the append kernel; the oracle runs over the dequantised rows."""
    h, hk = 6, 2
    key = ("fp8", page_size, d)
    if key not in _memo:
        gen = torch.Generator().manual_seed(31 + page_size + d)
        n = max(SEQ_LENS)
        k = torch.randn(len(SEQ_LENS), hk, n, d, generator=gen).to(torch.bfloat16).cuda()
        v = torch.randn(len(SEQ_LENS), hk, n, d, generator=gen).to(torch.bfloat16).cuda()
        cache = PagedKVCache.from_dense(k, v, SEQ_LENS, page_size, fp8=True,
                                        shuffle_seed=5, spare_pages=3)
        _memo[key] = (cache, _pool_rows(cache.k_pages, cache.v_pages, cache.block_table,
                                        SEQ_LENS, d, cache.k_scales, cache.v_scales))
    cache, (ks, vs) = _memo[key]
    q = _rand_q(len(SEQ_LENS), T, h, d, Q_LENS, 77 + d, "cuda")
    out, lse = paged_prefill_attn(q, cache, Q_LENS, causal=causal,
                                  return_lse=True, kv_split=kv_split)
    torch.cuda.synchronize()
    _check(out, lse, _oracle(q, ks, vs, Q_LENS, causal),
           f"fp8 ps{page_size} d{d} c{causal} s{kv_split}")


@pytest.mark.gpu
@pytest.mark.parametrize("kv_split", [1, 3])
@pytest.mark.parametrize("page_size", [16, 128])
def test_prefill_fp8_pool_gains(page_size, kv_split):
    """fp8 pool whose rows carry their own gains 2^[-4, 4], 40 tail queries
    per sequence leaning on the rows around page and kv-tile boundaries
    (15|16, 63|64, 127|128, 255|256), causal.  Judged relative to
    mag = softmax |v| against the fp64 oracle on the dequantised pool; the
    output is bf16, so the bound is B_BF16 = 2**-6 (tests/fp8_emulation.py:
    fp32 eager floor 1.6e-6, neighbour-scale ceiling 0.52)."""
    from .fp8_emulation import (B_BF16, CACHE_GAINS_CASES, build_gains_cache,
                                relative_failures, rows_oracle)
    lens, hk, h, nq, d, edges = CACHE_GAINS_CASES["prefill"]
    key = ("gains", page_size)
    if key not in _memo:
        q, k, v = build_gains_cache(lens, hk, h, nq, d, edges)
        cache = PagedKVCache.from_dense(k.cuda(), v.cuda(), lens, page_size, fp8=True,
                                        shuffle_seed=5, spare_pages=3)
        ks, vs = _pool_rows(cache.k_pages, cache.v_pages, cache.block_table, lens, d,
                            cache.k_scales, cache.v_scales)
        heads = torch.arange(h) % hk
        refs = []
        for i, n in enumerate(lens):
            vis = torch.arange(n)[None, :] <= (n - nq + torch.arange(nq))[:, None]
            refs.append(rows_oracle(q[i], ks[i][heads], vs[i][heads], d ** -0.5, vis))
        _memo[key] = (q.transpose(1, 2).contiguous().cuda(), cache, refs)
    qt, cache, refs = _memo[key]
    out, lse = paged_prefill_attn(qt, cache, [nq] * len(lens), causal=True,
                                  return_lse=True, kv_split=kv_split)
    torch.cuda.synchronize()
    for i, (ref, mag, ref_lse) in enumerate(refs):
        relative_failures(out[i].transpose(0, 1), ref, mag, B_BF16,
                          f"prefill fp8 gains ps{page_size} s{kv_split} seq {i}")
        e_lse = (lse[i].double().cpu() - ref_lse).abs().max().item()
        assert e_lse < LSE_TOL, f"lse err {e_lse}"


@pytest.mark.gpu
def test_prefill_agrees_with_decode():
    """T = 4 tail queries, causal: the prefill kernel against the paged
    decode kernel (same convention: the queries' tokens are already cached)."""
    lens = [4, 200]
    cache = _hand_built(lens, 16, 2, 64, "cuda", seed=3)
    q = _rand_q(2, 4, 4, 64, [4, 4], 5, "cuda")
    out, lse = paged_prefill_attn(q, cache, [4, 4], causal=True, return_lse=True)
    ref_out, ref_lse = _local_paged_decode_partial(q.transpose(1, 2).contiguous(),
                                                   cache, causal=True)
    torch.cuda.synchronize()
    e_out = (out.float().transpose(1, 2) - ref_out).abs().max().item()
    e_lse = (lse - ref_lse[..., 0]).abs().max().item()
    print(f"vs decode: out err {e_out:.3e} lse err {e_lse:.3e}")
    assert e_out < OUT_TOL and e_lse < LSE_TOL


@pytest.mark.gpu
def test_prefill_chunked_end_to_end():
    """Prompts of 300 and 77 tokens appended in chunks of 128 with a prefill
    call after each append: the concatenated outputs are full causal
    attention over each whole prompt."""
    prompts, chunk, ps, h, hk, d = [300, 77], 128, 16, 4, 2, 64
    n = max(prompts)
    gen = torch.Generator().manual_seed(9)
    q = torch.randn(2, n, h, d, generator=gen).to(torch.bfloat16).cuda()
    k = torch.randn(2, hk, n, d, generator=gen).to(torch.bfloat16).cuda()
    v = torch.randn(2, hk, n, d, generator=gen).to(torch.bfloat16).cuda()
    cache = PagedKVCache(sum(-(-x // ps) for x in prompts) + 2, ps, hk, d, 2,
                         -(-n // ps), device="cuda")
    out = torch.zeros(2, n, h, d, dtype=torch.bfloat16, device="cuda")
    lse = torch.full((2, h, n), float("-inf"), device="cuda")
    for c0 in range(0, n, chunk):
        lens = [max(0, min(chunk, x - c0)) for x in prompts]
        pad = chunk - (min(n, c0 + chunk) - c0)
        sl = slice(c0, c0 + chunk)
        padded = [torch.nn.functional.pad(x[:, :, sl], (0, 0, 0, pad)) for x in (k, v)]
        cache.append(*padded, lens)
        qc = torch.nn.functional.pad(q[:, sl], (0, 0, 0, 0, 0, pad))
        o, l = paged_prefill_attn(qc, cache, lens, causal=True, return_lse=True)
        for i, ln in enumerate(lens):
            out[i, c0:c0 + ln] = o[i, :ln]
            lse[i, :, c0:c0 + ln] = l[i, :, :ln]
    torch.cuda.synchronize()
    assert cache.host_lens == prompts
    ks, vs = _pool_rows(cache.k_pages, cache.v_pages, cache.block_table, prompts, d)
    ref_out, ref_lse, live = _oracle(q, ks, vs, prompts, True)
    out, lse = out.float().cpu(), lse.cpu()
    e_out = (out - ref_out).abs().max().item()
    e_lse = (lse[live] - ref_lse[live]).abs().max().item()
    print(f"chunked: out err {e_out:.3e} lse err {e_lse:.3e}")
    assert torch.isfinite(out).all()
    assert e_out < OUT_TOL and e_lse < LSE_TOL


@pytest.mark.gpu
@pytest.mark.parametrize("causal", [True, False])
def test_prefill_small_head_dim(causal):
    """dim_head = 48 is stored zero-padded to 64; the scale stays 48 ** -0.5."""
    d, h, hk, ps = 48, 4, 2, 16
    gen = torch.Generator().manual_seed(21)
    n = max(SEQ_LENS)
    k = torch.randn(len(SEQ_LENS), hk, n, d, generator=gen).to(torch.bfloat16).cuda()
    v = torch.randn(len(SEQ_LENS), hk, n, d, generator=gen).to(torch.bfloat16).cuda()
    cache = PagedKVCache.from_dense(k, v, SEQ_LENS, ps, shuffle_seed=2, spare_pages=2)
    ks, vs = _pool_rows(cache.k_pages, cache.v_pages, cache.block_table, SEQ_LENS, d)
    q = _rand_q(len(SEQ_LENS), T, h, d, Q_LENS, 8, "cuda")
    out, lse = paged_prefill_attn(q, cache, Q_LENS, causal=causal, return_lse=True)
    torch.cuda.synchronize()
    assert out.shape == q.shape
    _check(out, lse, _oracle(q, ks, vs, Q_LENS, causal), f"d48 c{causal}")


# --------------------------------------------------------------------------
# CPU
# --------------------------------------------------------------------------
@pytest.mark.parametrize("window", [None, 20])
@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("causal", [True, False])
def test_prefill_eager_fallback(causal, fp8, window):
    lens, q_lens, t, h, hk, d, ps = [1, 63, 130, 0], [1, 40, 70, 0], 70, 4, 2, 64, 16
    gen = torch.Generator().manual_seed(4)
    n = max(lens)
    k = torch.randn(len(lens), hk, n, d, generator=gen).to(torch.bfloat16)
    v = torch.randn(len(lens), hk, n, d, generator=gen).to(torch.bfloat16)
    cache = PagedKVCache.from_dense(k, v, lens, ps, fp8=fp8, shuffle_seed=1, spare_pages=2)
    ks, vs = _pool_rows(cache.k_pages, cache.v_pages, cache.block_table, lens, d,
                        cache.k_scales, cache.v_scales)
    q = _rand_q(len(lens), t, h, d, q_lens, 6, "cpu")
    out, lse = paged_prefill_attn(q, cache, q_lens, causal=causal, window=window,
                                  return_lse=True)
    assert out.dtype == torch.bfloat16 and out.shape == q.shape
    _check(out, lse, _oracle(q, ks, vs, q_lens, causal, window), "eager")
    only = paged_prefill_attn(q, cache, torch.tensor(q_lens), causal=causal, window=window)
    assert torch.equal(only, out)


def test_prefill_argument_checks():
    lens, hk, d, ps = [5, 40], 2, 64, 16
    k = torch.randn(2, hk, 40, d).to(torch.bfloat16)
    cache = PagedKVCache.from_dense(k, k.clone(), lens, ps)
    q = torch.randn(2, 8, 4, d).to(torch.bfloat16)
    paged_prefill_attn(q, cache, [5, 8])
    with pytest.raises(ValueError, match="q_lens"):
        paged_prefill_attn(q, cache, [6, 8])            # q_len > seq_len
    with pytest.raises(ValueError, match="q_lens"):
        paged_prefill_attn(q, cache)                    # default T = 8 > 5
    with pytest.raises(ValueError, match="q_lens"):
        paged_prefill_attn(q, cache, [5, 9])            # q_len > T
    with pytest.raises(ValueError, match="max_seqs"):
        paged_prefill_attn(q[:1], cache, [5])
    with pytest.raises(ValueError, match="head dim"):
        paged_prefill_attn(q[..., :32], cache, [5, 8])
    with pytest.raises(ValueError, match="kv heads"):
        paged_prefill_attn(q[:, :, :3], cache, [5, 8])
    with pytest.raises(RuntimeError, match="require grad"):
        paged_prefill_attn(q.float().requires_grad_(), cache, [5, 8])


def test_prefill_auto_kv_split():
    # the grid already holds 256 workgroups: no split
    assert auto_kv_split(8192, 1, 8, 8192, 64) == 1
    assert auto_kv_split(256, 8, 32, 1 << 17, 64) == 1
    # T = 512, 8 heads: 16 workgroups -> the cap
    assert auto_kv_split(512, 1, 8, 32768, 64) == 16
    # smallest split reaching 256 workgroups
    assert auto_kv_split(2048, 1, 8, 32768, 64) == 4
    assert auto_kv_split(300, 5, 6, 4096, 64) == 5          # 60 * 5 >= 256 > 60 * 4
    # never more than the longest sequence's tile count (128 / 64 wide)
    assert auto_kv_split(4, 2, 4, 200, 64) == 2
    assert auto_kv_split(4, 2, 4, 200, 128) == 4
    assert auto_kv_split(4, 2, 4, 0, 64) == 1
    for t in (1, 300, 5000):
        for bh in (1, 7, 64, 512):
            for n in (0, 1, 129, 100000):
                for kd in (64, 128):
                    s = auto_kv_split(t, 1, bh, n, kd)
                    tiles = max(1, -(-n // (128 if kd == 64 else 64)))
                    base = -(-t // 256) * bh
                    assert 1 <= s <= min(16, tiles)
                    assert s == 1 or base * (s - 1) < 256
                    assert base * s >= 256 or s == min(16, tiles)
