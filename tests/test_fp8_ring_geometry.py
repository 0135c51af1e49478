"""`ring_flash_attn_fp8` with the bf16 ring's hop geometry: striped shards and
`max_lookback_seq_len`, and `RingAttention(fp8_inference=True)` reaching it.

The ring cases run the counting probe of tests/test_mask_exactness.py over the
GLOBAL sequence: rank r of R holds positions r + R*i (striped) or r*n + i, q is
0 and v one-hot in the global position, so exp(lse) of a row is the number of
global keys it attends and out counts them per residue class.  The reference
is a boolean mask over global positions built here; it does not go through
`_hop_geometry`, so a wrong use of that helper (which a per-hop model would
share) shows.  On the CPU the hops run `_eager_fp8` over gloo, on the GPU the
kernel under `loopback_world`.

The `gains` case (GPU, world 2, striped) judges the merged result against the
per-hop masked model merged in fp64, at fp8_emulation's BOUND: each hop's
bf16 out costs 2**-9 of its share of mag (test_gpu_two_hop_merge).

Measured on MI355X: probe, worst over worlds 2 and 4 and the five layouts,
err / mag 0.0074 and |exp(lse) - count| 0.00082; gains err / mag 0.0075, lse
difference 3.8e-6.
"""

import pytest
import torch

from ring_attention_amd.ops.fp8 import quantize_fp8, ring_flash_attn_fp8

from .distributed_utils import run_distributed
from .fp8_emulation import build_inputs, fp8_failures, fp8_kvblk, merge_two_hops_fp64
from .fp8_geometry_emulation import emulate_fp8_forward_masked
from .test_mask_exactness import _probe_failures, _probe_slice, _reference

N_SHARD = 256
# (striped, max_lookback_seq_len)
RING_CASES = [(True, None), (True, 100), (True, 300), (False, 100), (False, 300)]


def _positions(rank, world, n, striped):
    i = torch.arange(n)
    return rank + world * i if striped else rank * n + i


def _ring_probe(rank, world, striped, lookback, device="cpu"):
    """One rank of the probe; returns the checker's failure strings."""
    n, d, h = N_SHARD, 64, 2
    total = world * n
    pos = _positions(rank, world, n, striped)
    _, _, v_glob, _ = _probe_slice(total, total, d)
    g = torch.Generator().manual_seed(100 + rank)
    q = torch.zeros(1, n, h, d, dtype=torch.bfloat16, device=device)
    k = torch.randn(1, n, h, d, generator=g).to(torch.bfloat16).to(device)
    v = v_glob[pos][None, :, None, :].expand(1, n, h, d).to(torch.bfloat16).contiguous().to(device)
    before = [t.clone() for t in (q, k, v)]
    out, lse = ring_flash_attn_fp8(q, k, v, causal=True, striped=striped,
                                   max_lookback_seq_len=lookback)
    if device != "cpu":
        torch.cuda.synchronize()
    # the ring must leave the caller's shards alone (FUTURE_WORK.md section 5)
    assert all(torch.equal(a, b_) for a, b_ in zip(before, (q, k, v)))
    gi, gj = pos[:, None], torch.arange(total)[None, :]
    attend = gj <= gi
    if lookback is not None:
        attend &= (gi - gj) <= lookback
    ref = _reference(attend, d)
    return _probe_failures(dict(lse=lse.cpu(), out=out.cpu().permute(0, 2, 1, 3)), ref,
                           tag=f"rank {rank}/{world} striped={striped} lookback={lookback}",
                           family="fp8 ring")


def _assert_all_ranks(results):
    fails = [f for r in results for f in r]
    assert not fails, "\n".join(fails[:12])


@pytest.mark.parametrize("striped,lookback", RING_CASES)
@pytest.mark.parametrize("world", [2, 4])
def test_ring_probe_gloo(world, striped, lookback):
    _assert_all_ranks(run_distributed(world, _ring_probe, striped, lookback))


def test_striped_requires_causal():
    q = torch.zeros(1, 256, 2, 64, dtype=torch.bfloat16)
    with pytest.raises(AssertionError, match="striped"):
        ring_flash_attn_fp8(q, q, q, causal=False, striped=True)


@pytest.mark.gpu
@pytest.mark.parametrize("striped,lookback", RING_CASES)
@pytest.mark.parametrize("world", [2, 4])
def test_ring_probe_loopback_gpu(world, striped, lookback):
    from .loopback_dist import loopback_world
    _assert_all_ranks(loopback_world(
        world, lambda r: _ring_probe(r, world, striped, lookback, "cuda")))


@pytest.mark.gpu
@pytest.mark.parametrize("d", [64, 128])
def test_ring_gains_striped_loopback_gpu(d):
    from .loopback_dist import loopback_world
    world, n, h = 2, N_SHARD, 2
    q, k, v = (t.cuda() for t in build_inputs("gains", 1, world * n, world * n, h, h, d,
                                              seed=31, kvblk=fp8_kvblk()))
    shard = lambda t, r: t[:, r::world].contiguous()
    before = [t.clone() for t in (q, k, v)]

    def run(rank):
        return ring_flash_attn_fp8(shard(q, rank), shard(k, rank), shard(v, rank),
                                   causal=True, striped=True)

    results = loopback_world(world, run)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b_) for a, b_ in zip(before, (q, k, v)))
    sm = d ** -0.5
    for rank, (out, lse) in enumerate(results):
        ref = None
        for src in range(world):
            ops = quantize_fp8(shard(q, rank), shard(k, src), shard(v, src))
            # positions rank + R*i against src + R*j: j <= i, strictly below
            # for a later source
            mo = emulate_fp8_forward_masked(*ops, sm, True, n,
                                            diag=0 if src <= rank else -1)
            ref = mo if ref is None else merge_two_hops_fp64(ref, mo)
        bad, f = fp8_failures(out, lse, ref)
        print(f"striped ring gains d{d} rank {rank}: err/mag {f['ratio']:.4g}  "
              f"lse diff {f['lse']:.3g}")
        assert not bad, bad


# ---------------------------------------------------------------------------
# the module: fp8_inference with striped_ring_attn / max_lookback_seq_len
# ---------------------------------------------------------------------------
def _spy(monkeypatch_setattr):
    """Counts calls of the two fp8 entry points the module may take."""
    import ring_attention_amd.ops.fp8 as fp8
    calls = {"flash_attn_fp8": 0, "ring_flash_attn_fp8": 0}
    for name in calls:
        real = getattr(fp8, name)

        def wrapped(*a, _real=real, _name=name, **kw):
            calls[_name] += 1
            return _real(*a, **kw)

        monkeypatch_setattr(fp8, name, wrapped)
    return calls


def _module_case(striped, lookback, ring, setattr_):
    from ring_attention_amd.models.attention import RingAttention
    torch.manual_seed(47)
    kw = dict(dim=128, dim_head=64, heads=2, causal=True, striped_ring_attn=striped,
              max_lookback_seq_len=lookback, bucket_size=256, ring_seq_size=256,
              ring_attn=ring)
    attn = RingAttention(**kw, fp8_inference=True).to(torch.bfloat16)
    x = torch.randn(1, 512, 128, dtype=torch.bfloat16)
    calls = _spy(setattr_)
    taken = "ring_flash_attn_fp8" if ring else "flash_attn_fp8"
    with torch.no_grad():
        out_fp8 = attn(x)
    assert calls[taken] == 1 and sum(calls.values()) == 1, calls
    attn.fp8_inference = False
    with torch.no_grad():
        ref = attn(x)
    assert sum(calls.values()) == 1, calls
    rel = ((out_fp8.float() - ref.float()).abs().mean()
           / (ref.float().abs().mean() + 1e-9)).item()
    assert out_fp8.shape == ref.shape
    # the tolerance of test_fp8_cpu.py::test_ring_attention_module_fp8_inference
    assert rel < 0.2, f"fp8 module path rel {rel}"
    # with grad enabled the fp8 path must not engage (it has no backward)
    attn.fp8_inference = True
    x2 = x.clone().requires_grad_(True)
    attn(x2).sum().backward()
    assert x2.grad is not None and sum(calls.values()) == 1, calls
    return rel


@pytest.mark.parametrize("striped,lookback", [(True, None), (True, 100), (False, 100)])
def test_module_fp8_inference_takes_the_fp8_path(monkeypatch, striped, lookback):
    _module_case(striped, lookback, False, monkeypatch.setattr)


def _module_rank(rank, world, striped, lookback):
    return _module_case(striped, lookback, True, setattr)


@pytest.mark.parametrize("striped,lookback", [(True, None), (True, 300)])
def test_module_fp8_inference_striped_ring_gloo(striped, lookback):
    run_distributed(2, _module_rank, striped, lookback)
