"""Softclamp (logit capping) in the serving kernels: row decode, grouped paged
and dense decode, paged prefill (grid and varlen).

Reference: fp64 softmax over c * tanh(q.k * d**-0.5 / c) on the bf16-rounded
(fp8: dequantised) operands with an explicit visibility matrix.  q carries a
gain so that the unclamped scores have standard deviation 1.5 c (c = 4, gain 6)
or 3 c (c = 50, gain 150), and every reference asserts that clamped and
unclamped results differ by at least 20x the bound of its family: a kernel that
ignored the flag would fail.  The bounds are the families' own for unclamped
calls (the clamp adds fp32 error only): grouped 2^-8 * mag and lse 1e-3; row
decode 3e-3 (fp8 5e-3) and lse 2e-3; prefill 2e-2 and lse 2e-3.
"""

import pytest
import torch

from ring_attention_amd import (PagedKVCache, paged_prefill_attn, paged_prefill_attn_varlen,
                                tree_attn_decode, tree_attn_decode_fp8, tree_attn_decode_paged)
from ring_attention_amd.ops.fp8 import quantize_kv_cache
from ring_attention_amd.tree_decode import _local_paged_decode_partial, _tree_bits

from .fp8_emulation import dequant_rows, relative_failures
from .test_paged_decode import OUT_BF16, OUT_FP8, _check as check_rows, _pool_rows
from .test_paged_grouped import BOUND, LSE_TOL, _cache, _tree_mask
from .test_paged_prefill import OUT_TOL, _check as check_prefill

C, GAIN = 4.0, 6.0


def _ext():
    from ring_attention_amd.ops import hip_ext
    return hip_ext.require()


def _ref(q, kd, vd, vis, c):
    """q (h, nq, d), kd / vd (hk, n, d), vis (nq, n) bool, c None = no clamp
    -> fp64 out, mag (= out with |v|), lse (h, nq); dead rows 0 / -inf."""
    heads = torch.arange(q.shape[0]) % kd.shape[0]
    q, kd, vd = q.double().cpu(), kd.double().cpu()[heads], vd.double().cpu()[heads]
    s = torch.einsum("hid,hjd->hij", q, kd) * q.shape[-1] ** -0.5
    if c is not None:
        s = c * torch.tanh(s / c)
    s = s.masked_fill(~vis[None], float("-inf"))
    p = torch.nan_to_num(torch.softmax(s, dim=-1))
    return (torch.einsum("hij,hjd->hid", p, vd), torch.einsum("hij,hjd->hid", p, vd.abs()),
            s.logsumexp(-1))


def _refs(q, ks, vs, vis, c, bound, relative):
    """Per-sequence clamped references, after the clamp-matters check."""
    refs, gap = [], 0.0
    for i in range(len(ks)):
        out, mag, lse = _ref(q[i], ks[i], vs[i], vis[i], c)
        diff = (out - _ref(q[i], ks[i], vs[i], vis[i], None)[0]).abs()
        if diff.numel():
            gap = max(gap, float((diff / mag.clamp(min=1e-30)).max() if relative else diff.max()))
        refs.append((out, mag, lse))
    assert gap >= 20 * bound, f"the clamp moves the result by {gap}, under 20 x {bound}"
    return refs


def _judge_grouped(out, lse, refs, tag):
    for i, (ref, mag, ref_lse) in enumerate(refs):
        relative_failures(out[i], ref, mag, BOUND, f"{tag} seq {i}")
        live = torch.isfinite(ref_lse)
        got = lse[i, ..., 0].double().cpu()
        assert (got[~live] <= -1e30).all(), f"{tag} seq {i} dead lse"
        if live.any():
            assert (got[live] - ref_lse[live]).abs().max() <= LSE_TOL, f"{tag} seq {i} lse"


def _judge_rows(out, lse, refs, tol, tag):
    ref_out = torch.stack([r[0] for r in refs]).float()
    ref_lse = torch.stack([r[2] for r in refs]).float()[..., None]
    check_rows(out, lse, ref_out, ref_lse, torch.isfinite(ref_lse[:, 0, :, 0]), tol, tag)


def _spans(lens, nq, causal, window):
    """(nq, n) visibility per sequence: keys [lo, limit) of tree_decode._window_spans."""
    vis = []
    for n in lens:
        j = torch.arange(n)[None, :]
        iq = torch.arange(nq)[:, None]
        ok = j < (n - (nq - 1 - iq) if causal else n)
        if window is not None:
            ok = ok & (j >= n - nq + iq - window)
        vis.append(ok.expand(nq, n))
    return vis


# --------------------------------------------------------------------------
# GPU
# --------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("chunks", [0, 3])
@pytest.mark.parametrize("nq", [1, 2])
@pytest.mark.parametrize("d,fp8,c,gain", [(64, False, C, GAIN), (128, False, C, GAIN),
                                          (64, True, C, GAIN), (128, True, 50.0, 150.0)])
def test_row_decode_dense(d, fp8, c, gain, nq, chunks):
    b, h, hk, n = 2, 4, 2, 333
    gen = torch.Generator().manual_seed(d + nq)
    q = (gain * torch.randn(b, h, nq, d, generator=gen)).to(torch.bfloat16).cuda()
    k = torch.randn(b, hk, n, d, generator=gen).to(torch.bfloat16).cuda()
    v = torch.randn(b, hk, n, d, generator=gen).to(torch.bfloat16).cuda()
    if fp8:
        k8, v8, ks, vs = quantize_kv_cache(k, v)
        outs, lses = _ext().decode_partial_fp8(q, k8, v8, ks, vs, d ** -0.5, chunks, True, c)
        k, v = dequant_rows(k8.cpu(), ks.cpu()), dequant_rows(v8.cpu(), vs.cpu())
    else:
        outs, lses = _ext().decode_partial(q, k, v, d ** -0.5, chunks, True, c)
    out, lse = _ext().decode_merge(outs, lses)
    tol = OUT_FP8 if fp8 else OUT_BF16
    refs = _refs(q, k, v, _spans([n] * b, nq, False, None), c, tol, False)
    _judge_rows(out, lse, refs, tol, "dense rows")


@pytest.mark.gpu
@pytest.mark.parametrize("causal,window", [(False, None), (True, None), (True, 40)])
@pytest.mark.parametrize("ps,d,fp8", [(16, 64, False), (64, 128, True)])
def test_row_decode_paged(ps, d, fp8, causal, window):
    lens, h, hk, nq = [0, 1, 65, 333], 4, 2, 2
    cache = _cache(lens, hk, d, ps, fp8, "cuda", seed=3 + ps)
    torch.manual_seed(ps + d)
    q = (GAIN * torch.randn(len(lens), h, nq, d)).to(torch.bfloat16).cuda()
    out, lse = _local_paged_decode_partial(q, cache, causal, window=window,
                                           softclamp_qk_sim=True, softclamp_value=C)
    ks, vs = _pool_rows(cache.k_pages, cache.v_pages, cache.block_table, lens, d,
                        cache.k_scales, cache.v_scales)
    tol = OUT_FP8 if fp8 else OUT_BF16
    refs = _refs(q, ks, vs, _spans(lens, nq, causal, window), C, tol, False)
    _judge_rows(out, lse, refs, tol, "paged rows")


@pytest.mark.gpu
@pytest.mark.parametrize("chunks", [0, 3])
@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("ps", [16, 64])
@pytest.mark.parametrize("G,nq", [(2, 3), (8, 5)])
def test_grouped_paged(G, nq, ps, d, fp8, chunks):
    """R = 6 (one partial tile) and 40 (two tiles); prefixes around a block
    and a pass, one empty slot, a random tree per sequence."""
    hk = 2
    lens = [p + nq for p in (0, 31, 33)] + [0, 129 + nq]
    cache = _cache(lens, hk, d, ps, fp8, "cuda", seed=7 + ps + d)
    torch.manual_seed(G * 100 + nq)
    q = (GAIN * torch.randn(len(lens), G * hk, nq, d)).to(torch.bfloat16).cuda()
    masks = torch.stack([_tree_mask(nq, 50 + i) for i in range(len(lens))])
    out, lse = _local_paged_decode_partial(q, cache, chunks=chunks, tree_mask=masks.cuda(),
                                           softclamp_qk_sim=True, softclamp_value=C)
    ks, vs = _pool_rows(cache.k_pages, cache.v_pages, cache.block_table, lens, d,
                        cache.k_scales, cache.v_scales)
    vis = [torch.cat([torch.ones(nq, max(n - nq, 0), dtype=torch.bool), masks[i][:, :n]], 1)
           for i, n in enumerate(lens)]
    _judge_grouped(out, lse, _refs(q, ks, vs, vis, C, BOUND, True), "grouped paged")


@pytest.mark.gpu
def test_grouped_paged_window_and_default_cap():
    """grouped=True, causal=True under a window of 50, with c = 50 (the model
    default) and the gain that goes with it."""
    lens, hk, G, nq, d, c = [55, 0, 200], 2, 4, 3, 64, 50.0
    cache = _cache(lens, hk, d, 16, False, "cuda", seed=11)
    torch.manual_seed(5)
    q = (3 * c * torch.randn(len(lens), G * hk, nq, d)).to(torch.bfloat16).cuda()
    out, lse = _local_paged_decode_partial(q, cache, True, window=50, grouped=True,
                                           softclamp_qk_sim=True, softclamp_value=c)
    ks, vs = _pool_rows(cache.k_pages, cache.v_pages, cache.block_table, lens, d)
    refs = _refs(q, ks, vs, _spans(lens, nq, True, 50), c, BOUND, True)
    _judge_grouped(out, lse, refs, "grouped window")


@pytest.mark.gpu
@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("prefix", [1, 129])
@pytest.mark.parametrize("nq", [2, 8, 16])
def test_grouped_dense(nq, prefix, d, fp8, monkeypatch):
    """G = 8: R = 16, 64, 128 rows, i.e. TILES 1, 2 and (limit lifted) 4; causal."""
    monkeypatch.setenv("RING_ATTN_GROUPED_TILES", "4")
    b, hk, G, n = 2, 2, 8, prefix + nq
    gen = torch.Generator().manual_seed(nq + d + prefix)
    q = (GAIN * torch.randn(b, G * hk, nq, d, generator=gen)).to(torch.bfloat16).cuda()
    k = torch.randn(b, hk, n, d, generator=gen).to(torch.bfloat16).cuda()
    v = torch.randn(b, hk, n, d, generator=gen).to(torch.bfloat16).cuda()
    ops = (k, v, None, None)
    if fp8:
        ops = quantize_kv_cache(k, v)
        k, v = dequant_rows(ops[0].cpu(), ops[2].cpu()), dequant_rows(ops[1].cpu(), ops[3].cpu())
    chain = torch.ones(b, nq, nq, dtype=torch.bool).tril()
    outs, lses = _ext().decode_partial_grouped(q, *ops, d ** -0.5, 0, _tree_bits(chain.cuda()),
                                               True, C)
    out, lse = _ext().decode_merge(outs, lses)
    refs = _refs(q, k, v, _spans([n] * b, nq, True, None), C, BOUND, True)
    _judge_grouped(out, lse, refs, "grouped dense")


def _prefill_case(ps, d, fp8, window, device):
    """Two sequences, T = 300: a full and a ragged q tile, a 77-row chunk."""
    seq_lens, q_lens, h, hk, t = [377, 77], [300, 77], 4, 2, 300
    cache = _cache(seq_lens, hk, d, ps, fp8, device, seed=ps + d)
    gen = torch.Generator().manual_seed(9 + d)
    q = (GAIN * torch.randn(2, t, h, d, generator=gen)).to(torch.bfloat16)
    ks, vs = _pool_rows(cache.k_pages, cache.v_pages, cache.block_table, seq_lens, d,
                        cache.k_scales, cache.v_scales)
    vis = []
    for n, ql in zip(seq_lens, q_lens):
        pos, j = (n - ql + torch.arange(ql))[:, None], torch.arange(n)[None, :]
        vis.append((j <= pos) & (pos - j <= (n if window is None else window)))
    refs = _refs([q[i, :ql].transpose(0, 1) for i, ql in enumerate(q_lens)], ks, vs, vis, C,
                 OUT_TOL, False)
    out = torch.zeros(2, t, h, d)
    lse = torch.full((2, h, t), float("-inf"))
    for i, ql in enumerate(q_lens):
        out[i, :ql], lse[i, :, :ql] = refs[i][0].transpose(0, 1).float(), refs[i][2].float()
    return cache, q.to(device), q_lens, (out, lse, torch.isfinite(lse))


_prefill_memo = {}


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["split1", "split2", "varlen"])
@pytest.mark.parametrize("ps,d,fp8,window", [
    (ps, d, fp8, None) for ps in (16, 128) for d in (64, 128) for fp8 in (False, True)
] + [(16, 64, False, 100)])
def test_prefill(ps, d, fp8, window, form):
    key = (ps, d, fp8, window)
    if key not in _prefill_memo:
        _prefill_memo[key] = _prefill_case(ps, d, fp8, window, "cuda")
    cache, q, q_lens, ref = _prefill_memo[key]
    kw = dict(causal=True, window=window, return_lse=True, softclamp_qk_sim=True,
              softclamp_value=C)
    if form == "varlen":
        packed = torch.cat([q[i, :ql] for i, ql in enumerate(q_lens)])
        po, pl = paged_prefill_attn_varlen(packed, cache, q_lens, **kw)
        out, lse = torch.zeros_like(q), torch.full_like(ref[1], -1e38, device="cuda")
        row0 = 0
        for i, ql in enumerate(q_lens):
            out[i, :ql], lse[i, :, :ql] = po[row0:row0 + ql], pl[:, row0:row0 + ql]
            row0 += ql
    else:
        out, lse = paged_prefill_attn(q, cache, q_lens, kv_split=int(form[-1]), **kw)
    check_prefill(out, lse, ref, f"prefill {form}")


# --------------------------------------------------------------------------
# CPU: the eager fallbacks of the five entry points, and the argument check
# --------------------------------------------------------------------------
def test_eager_fallbacks_cpu():
    b, h, hk, nq, d, n = 2, 4, 2, 2, 64, 70
    gen = torch.Generator().manual_seed(1)
    q = (GAIN * torch.randn(b, h, nq, d, generator=gen)).to(torch.bfloat16)
    k = torch.randn(b, hk, n, d, generator=gen).to(torch.bfloat16)
    v = torch.randn(b, hk, n, d, generator=gen).to(torch.bfloat16)
    kw = dict(softclamp_qk_sim=True, softclamp_value=C)
    full = _spans([n] * b, nq, False, None)

    def close(got, refs, tag):
        ref = torch.stack([r[0] for r in refs])
        err = (got.double() - ref).abs().max().item()
        assert err < OUT_TOL, f"{tag} err {err}"      # bf16 output rounding

    refs = _refs(q, k, v, full, C, OUT_TOL, False)
    close(tree_attn_decode(q, k, v, shard_kv_seq=False, **kw), refs, "dense")
    k8, v8, ks, vs = quantize_kv_cache(k, v)
    refs8 = _refs(q, dequant_rows(k8, ks), dequant_rows(v8, vs), full, C, OUT_TOL, False)
    close(tree_attn_decode_fp8(q, k8, v8, ks, vs, **kw), refs8, "fp8")

    cache = PagedKVCache.from_dense(k, v, [n, n], 16)
    chain = _refs(q, k, v, _spans([n] * b, nq, True, None), C, OUT_TOL, False)
    close(tree_attn_decode_paged(q, cache, causal=True, **kw), chain, "paged")
    close(tree_attn_decode_paged(q, cache, causal=True, grouped=True, **kw), chain, "grouped")
    qp = q.transpose(1, 2).contiguous()                 # (b, T = nq, h, d)
    ref_p = torch.stack([r[0] for r in chain]).transpose(1, 2)
    got = paged_prefill_attn(qp, cache, [nq, nq], **kw)
    assert (got.double() - ref_p).abs().max() < OUT_TOL
    got = paged_prefill_attn_varlen(qp.reshape(b * nq, h, d), cache, [nq, nq], **kw)
    assert (got.double().view(b, nq, h, d) - ref_p).abs().max() < OUT_TOL


@pytest.mark.parametrize("value", [0.0, -1.0])
def test_softclamp_value_must_be_positive(value):
    q = torch.zeros(1, 2, 1, 64, dtype=torch.bfloat16)
    k = torch.zeros(1, 2, 4, 64, dtype=torch.bfloat16)
    cache = PagedKVCache.from_dense(k, k, [4], 16)
    kw = dict(softclamp_qk_sim=True, softclamp_value=value)
    calls = [lambda: tree_attn_decode(q, k, k, shard_kv_seq=False, **kw),
             lambda: tree_attn_decode_fp8(q, *quantize_kv_cache(k, k), **kw),
             lambda: tree_attn_decode_paged(q, cache, **kw),
             lambda: paged_prefill_attn(q.transpose(1, 2), cache, [1], **kw),
             lambda: paged_prefill_attn_varlen(q[0].transpose(0, 1), cache, [1], **kw)]
    for call in calls:
        with pytest.raises(ValueError, match="softclamp_value"):
            call()
