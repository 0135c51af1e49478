"""Sliding window and released pages in the grouped MFMA paged decode.

One definition (`_window_spans` of tree_decode.py, restated by `_spans` of
test_paged_window.py): row (b, iq) sits at qpos = len + kv_after - nq + iq and
attends keys [lo, limit), limit = len or, with `causal`,
max(0, len - (nq-1-iq)), lo = clamp(qpos - w, 0, limit).

The oracle is fp64 `rows_oracle` over K/V gathered from the pools BEFORE
anything is released, with the explicit (nq, n) visibility of the spans.  The
bound is the grouped kernel's own (test_paged_grouped.py):
|out - ref| <= 2^-8 * mag and |lse - ref| <= 1e-3 on live rows; dead rows are
exactly out == 0, lse <= -1e30.  Released and spare pages are NaN before every
call, so a read of one shows as a non-finite result.
"""

import pytest
import torch

from ring_attention_amd.tree_decode import _local_paged_decode_partial

from .fp8_emulation import relative_failures, rows_oracle
from .test_paged_decode import _pool_rows
from .test_paged_grouped import BOUND, LSE_TOL, _cache
from .test_paged_window import _keep_from, _poison_unheld, _spans

LONG = 517


def _windows(nq):
    """Descending windows; for the longest sequence lo_min = LONG - nq - w:
    0 (a window larger than every length); 255, 256, 257 (around the 128-key
    pass edge 256); 287, 288, 289 (around the 32-key block edge 288, no pass
    edge); 440 (upper 16-key half of block [416, 448): at page 16 the lower
    half's page is released); LONG - nq (w = 0)."""
    return [10000] + [LONG - nq - lo for lo in (255, 256, 257, 287, 288, 289, 440)] + [0]


def _judge(out, lse, q, ks, vs, hk, spans, bound, tag):
    """Returns the per-sequence (live rows, mag) for a later comparison."""
    b, h, nq, d = q.shape
    heads = torch.arange(h) % hk
    mags = []
    for i, rows in enumerate(spans):
        live = [iq for iq, (lo, hi) in enumerate(rows) if lo < hi]
        dead = [iq for iq in range(nq) if iq not in live]
        assert (out[i][:, dead] == 0).all() and (lse[i][:, dead] <= -1e30).all(), \
            f"{tag} seq {i} dead rows"
        mags.append((live, None))
        if not live:
            continue
        vis = torch.zeros(nq, ks[i].shape[1], dtype=torch.bool)
        for iq, (lo, hi) in enumerate(rows):
            vis[iq, lo:hi] = True
        ref, mag, ref_lse = rows_oracle(q[i][:, live].cpu(), ks[i][heads], vs[i][heads],
                                        d ** -0.5, vis[live])
        relative_failures(out[i][:, live], ref, mag, bound, f"{tag} seq {i}")
        e_lse = (lse[i][:, live, 0].double().cpu() - ref_lse).abs().max().item()
        assert e_lse <= LSE_TOL, f"{tag} seq {i} lse err {e_lse}"
        mags[-1] = (live, mag)
    return mags


def _run_windows(cache, q, lens, causal, chunks, windows, bound, tag):
    nq = q.shape[2]
    ks, vs = _pool_rows(cache.k_pages, cache.v_pages, cache.block_table, lens,
                        q.shape[3], cache.k_scales, cache.v_scales)
    for w in windows:
        spans = _spans(lens, nq, causal, w)
        cache.release_prefix(_keep_from(spans))
        _poison_unheld(cache)
        out, lse = _local_paged_decode_partial(q, cache, causal=causal, chunks=chunks,
                                               window=w, grouped=True)
        _judge(out, lse, q, ks, vs, cache.kv_heads, spans, bound, f"{tag} w={w}")


@pytest.mark.gpu
@pytest.mark.parametrize("chunks", [0, 3])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("page_size", [16, 64])
@pytest.mark.parametrize("G,nq", [(8, 4), (8, 5)])
def test_grouped_window_ragged_release(G, nq, page_size, d, fp8, causal, chunks):
    """R = 32 and 40 rows per kv head, ragged batch with an empty slot, every
    window of `_windows`, the pages below each call's smallest lo released
    and NaN-poisoned first."""
    hk = 2
    lens = [nq, 33 + nq, 0, 130 + nq, LONG]
    torch.manual_seed(G * 100 + nq)
    cache = _cache(lens, hk, d, page_size, fp8, "cuda", seed=17 + page_size + d)
    q = torch.randn(len(lens), G * hk, nq, d).to(torch.bfloat16).cuda()
    _run_windows(cache, q, lens, causal, chunks, _windows(nq), BOUND, "ragged")
    assert cache.host_starts[-1] == (LONG - nq) // page_size * page_size > 0


@pytest.mark.gpu
@pytest.mark.parametrize("after_kind", ["none", "partly", "wholly"])
@pytest.mark.parametrize("nq", [1, 3])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("page_size", [16, 64])
def test_grouped_window_counting_probe(page_size, causal, nq, after_kind):
    """q = 0: every attended key weighs the same and exp(lse) is their count,
    limit - lo.  An off-by-one at lo or at the chain limit moves it by 1; the
    fp32 lse is good to 1e-6 relative.  kv_after moves the window partly
    (w / 2 keys) or wholly (w + nq keys) past the end of the shard; wholly
    outside, every row is dead."""
    lens, hk, h, d = [3, 63, 130, LONG], 2, 4, 64
    cache = _cache(lens, hk, d, page_size, False, "cuda", seed=page_size)
    q = torch.zeros(len(lens), h, nq, d, dtype=torch.bfloat16, device="cuda")
    for w in [300, 100, 33, 32, 1, 0]:
        after = {"none": None, "partly": [w // 2] * len(lens),
                 "wholly": [w + nq] * len(lens)}[after_kind]
        spans = _spans(lens, nq, causal, w, after)
        out, lse = _local_paged_decode_partial(q, cache, causal=causal, window=w,
                                               kv_after=after, grouped=True)
        lse = lse.cpu()
        assert torch.isfinite(out).all() and torch.isfinite(lse).all()
        for i, rows in enumerate(spans):
            for iq, (lo, hi) in enumerate(rows):
                assert after_kind != "wholly" or lo == hi
                if lo == hi:
                    assert (out[i, :, iq] == 0).all() and (lse[i, :, iq] <= -1e30).all()
                    continue
                count = lse[i, :, iq, 0].double().exp()
                assert ((count - (hi - lo)).abs() <= 1e-3 * (hi - lo)).all(), \
                    (w, i, iq, lo, hi, count)


@pytest.mark.gpu
@pytest.mark.parametrize("fp8", [False, True])
def test_grouped_window_same_definition_as_row_kernel(fp8):
    G, hk, nq, d, lens, w = 8, 2, 5, 64, [135, 300], 100
    torch.manual_seed(4)
    cache = _cache(lens, hk, d, 16, fp8, "cuda", seed=21)
    ks, vs = _pool_rows(cache.k_pages, cache.v_pages, cache.block_table, lens, d,
                        cache.k_scales, cache.v_scales)
    q = torch.randn(2, G * hk, nq, d).to(torch.bfloat16).cuda()
    kw = dict(causal=True, window=w, kv_after=[7, 0])
    row_out, _ = _local_paged_decode_partial(q, cache, **kw)
    out, lse = _local_paged_decode_partial(q, cache, grouped=True, **kw)
    mags = _judge(out, lse, q, ks, vs, hk, _spans(lens, nq, True, w, [7, 0]), BOUND, "row")
    for i, (live, mag) in enumerate(mags):
        diff = (out[i][:, live] - row_out[i][:, live]).abs().double().cpu()
        print(f"window vs row kernel seq {i}: {float((diff / mag).max()):.3g}")
        assert (diff <= 2 * BOUND * mag).all()


@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("causal", [False, True])
def test_grouped_window_fallback_cpu(fp8, causal):
    lens, hk, h, nq, d = [0, 5, 33, 70], 2, 4, 3, 16
    torch.manual_seed(6)
    cache = _cache(lens, hk, d, 16, fp8, "cpu", seed=23)
    q = torch.randn(len(lens), h, nq, d).to(torch.bfloat16)
    _run_windows(cache, q, lens, causal, 0, [10000, 40, 16, 3, 0], 1e-5, "cpu")
    assert cache.host_starts == [0, 0, 16, 64]


def test_grouped_window_guards_cpu():
    lens, hk, h, nq, d = [70, 40], 1, 2, 2, 16
    cache = _cache(lens, hk, d, 16, False, "cpu", seed=25)
    q = torch.randn(2, h, nq, d).to(torch.bfloat16)
    mask = torch.eye(nq, dtype=torch.bool)
    cache.release_prefix([40, 0])                      # starts [32, 0]
    # rows of sequence 0 sit at 68, 69: window 36 reaches key 32, 37 key 31
    _local_paged_decode_partial(q, cache, grouped=True, window=36)
    for kw in (dict(grouped=True), dict(grouped=True, window=37),
               dict(tree_mask=mask, window=36), dict(tree_mask=mask)):
        with pytest.raises(ValueError):
            _local_paged_decode_partial(q, cache, **kw)
