"""The fused HIP quantiser (csrc/quantize_fp8.hip) against the format's
definition: the retained torch chain on CPU copies of the same inputs.  bf16 /
fp16 amax mantissas have at most 10 bits, so amax / 448 never sits within float
error of a power of two and the comparison is exact: scale bytes identical,
data equal as e4m3 values (+-0 compare equal).  Outputs are handed in through
`out=` pre-filled with 0xFF, the e4m3 NaN byte, so an unwritten padding byte
fails the comparison."""

import pytest
import torch
import torch.nn.functional as F

from ring_attention_amd.ops import fp8

pytestmark = pytest.mark.gpu

LOW, HIGH = 1.75, 225.0 / 128.0   # last amax mantissa of one exponent, first of the next


def _rows(gen, b, n, h, d):
    """randn times per-row gains 2^[-4, 4] (fp32, quantised by the caller)."""
    gain = torch.exp2(torch.randint(-4, 5, (b, n, h, 1), generator=gen).float())
    return torch.randn(b, n, h, d, generator=gen) * gain


def _plant_rows(x):
    """(b, n, h, d): chunk amax exactly LOW * 2^3 / HIGH * 2^-5, a zero row."""
    n = x.shape[1]
    x[0, 0, 0, :64] *= 2.0 ** -12
    x[0, 0, 0, 0] = LOW * 8.0
    x[-1, n - 1, -1, :64] *= 2.0 ** -12
    x[-1, n - 1, -1, 1] = -HIGH / 32.0
    if n >= 3:
        x[:, n // 2] = 0.0
    return x


def _plant_v(v):
    """(b, n, hk, d): the same amax plants down the first 64-key chunk of
    columns 1 and 2, an all-zero chunk in column 3, a zero key row."""
    n = v.shape[1]
    v[0, :64, 0, 1:3] *= 2.0 ** -12
    v[0, 0, 0, 1] = LOW / 32.0
    v[0, min(n, 64) - 1, 0, 2] = -HIGH * 8.0
    v[-1, :64, 0, 3] = 0.0
    if n >= 3:
        v[:, n // 2] = 0.0
    return v


def _assert_same(got, ref, n_scales):
    """the last `n_scales` tensors are scale bytes, the others e4m3 data"""
    assert len(got) == len(ref)
    for i, (g, r) in enumerate(zip(got, ref)):
        assert g.shape == r.shape and g.dtype == r.dtype == torch.uint8, i
        if i >= len(ref) - n_scales:
            assert torch.equal(g.cpu(), r), f"scale tensor {i}"
        else:
            assert torch.equal(g.cpu().view(torch.float8_e4m3fn).float(),
                               r.view(torch.float8_e4m3fn).float()), f"data tensor {i}"


@pytest.mark.parametrize("nq,nk,h,hk,d,dtype,fused", [
    (1, 1, 2, 2, 64, torch.bfloat16, False),
    (63, 65, 4, 2, 128, torch.bfloat16, False),
    (257, 129, 2, 2, 32, torch.bfloat16, False),
    (300, 200, 4, 2, 96, torch.bfloat16, False),
    (300, 200, 2, 2, 64, torch.bfloat16, True),
    (63, 65, 2, 2, 64, torch.float16, False),
])
def test_quantize_fp8_matches_torch(nq, nk, h, hk, d, dtype, fused):
    b = 2
    gen = torch.Generator().manual_seed(nq * 1000 + nk + d)
    q = _plant_rows(_rows(gen, b, nq, h, d)).to(dtype)
    k = _plant_rows(_rows(gen, b, nk, hk, d)).to(dtype)
    v = _plant_v(_rows(gen, b, nk, hk, d)).to(dtype)
    kd = 64 if d <= 64 else 128
    ref = fp8._quantize_fp8_torch(*(F.pad(t, (0, kd - d)) for t in (q, k, v)))
    if fused:
        # q, k, v as slices of one projection output: strided, never copied
        n = max(nq, nk)
        proj = torch.zeros(b, n, h + 2 * hk, d, dtype=dtype)
        proj[:, :nq, :h], proj[:, :nk, h:h + hk], proj[:, :nk, h + hk:] = q, k, v
        proj = proj.cuda()
        qg, kg, vg = proj[:, :nq, :h], proj[:, :nk, h:h + hk], proj[:, :nk, h + hk:]
        assert not kg.is_contiguous()
    else:
        qg, kg, vg = q.cuda(), k.cuda(), v.cuda()
    out = [torch.full(r.shape, 0xFF, dtype=torch.uint8, device="cuda") for r in ref]
    got = fp8.quantize_fp8(qg, kg, vg, out=out)
    assert all(g.data_ptr() == o.data_ptr() for g, o in zip(got, out))
    _assert_same(got, ref, n_scales=3)


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("n", [5, 70])
def test_quantize_kv_cache_matches_torch(n, d):
    gen = torch.Generator().manual_seed(n + d)
    # (b, hk, n, d) caches; the plants are written on the (b, n, hk, d) view
    k = _rows(gen, 2, 2, n, d)
    v = _rows(gen, 2, 2, n, d)
    for x in (k, v):
        xt = x.permute(0, 2, 1, 3)
        xt[0, 0, 0] *= 2.0 ** -12
        xt[-1, n - 1, -1] *= 2.0 ** -12
        _plant_rows(xt)
    k, v = k.bfloat16(), v.bfloat16()
    ref = fp8._quantize_kv_cache_torch(k, v)
    _assert_same(fp8.quantize_kv_cache(k.cuda(), v.cuda()), ref, n_scales=2)


@pytest.mark.parametrize("d", [64, 96])
def test_flash_attn_fp8_unchanged(d, monkeypatch):
    """the forward computes the same bits from either quantiser"""
    gen = torch.Generator().manual_seed(d)
    q, k, v = (_rows(gen, 1, 300, 2, d).bfloat16().cuda() for _ in range(3))
    monkeypatch.delenv("RING_ATTN_NO_FUSED_QUANT", raising=False)
    out, lse = fp8.flash_attn_fp8(q, k, v, causal=True)
    monkeypatch.setenv("RING_ATTN_NO_FUSED_QUANT", "1")
    out_t, lse_t = fp8.flash_attn_fp8(q, k, v, causal=True)
    assert torch.equal(out, out_t) and torch.equal(lse, lse_t)
