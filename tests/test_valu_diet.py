"""Hot-loop VALU diet of the fwd / dq / dkv attention kernels.

The kernels feed the packed bf16 P / dS pairs to the second GEMM as they come
out of the score tile, with the other operand (the V^T, Q^T and dO^T LDS
images, the K^T transpose reads) staged in the same k order; the softmax scale
is applied once to dq / dk in the epilogue instead of per ds element; and the
dkv kernel stages lse already in the exp2 domain.  A wrong k permutation gives
O(1) errors on random normal inputs, a scale applied twice (or never) on an
accumulating path gives a factor of d**-0.5, so every case is held to the
fp32 oracle (ops/reference.py) at the bounds tests/test_gpu_kernels.py uses
for the same comparison: out 2e-2 abs, lse 2e-3 abs, gradients 4e-2 of the
reference's max (5e-2 with softclamp, as test_softclamp_parity).

n = 320 is one full 256-row tile plus a 64-row ragged one (and, for the dq
kernel's 128/64-row kv tiles, full tiles followed by a ragged one), so the
full-tile and the masked hot loops both run; d = 32 and d = 128 have softmax
scales that are not powers of two.
"""

import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

OUT_TOL = 2e-2          # test_fwd_bwd_parity: out, absolute
LSE_TOL = 2e-3          # test_fwd_bwd_parity: lse, absolute
GRAD_TOL = 4e-2         # test_fwd_bwd_parity: gradients, of the reference's max
GRAD_TOL_SOFTCLAMP = 5e-2   # test_softclamp_parity
SOFTCLAMP_VALUE = 5.0       # test_softclamp_parity

SINGLE_PASS_ENV = {"RING_ATTN_SPLIT_DQ": "1", "RING_ATTN_SPLIT_DKV": "1",
                   "RING_ATTN_NO_DESC": "1"}


def _ext():
    from ring_attention_amd.ops import hip_ext
    return hip_ext.require()


@functools.lru_cache(maxsize=None)
def _case(b, nq, nk, h, hk, d, causal, softclamp=False, q_offset=0, seed=0):
    """bf16 inputs and the fp32 oracle's out / lse / dq / dk / dv for one
    case; computed once and shared (callers must not modify it)."""
    from ring_attention_amd.ops.reference import (
        MASK_VALUE, default_attention, softclamp as softclamp_fn)
    g = torch.Generator(device="cuda").manual_seed(seed)
    mk = lambda *s: torch.randn(*s, device="cuda", dtype=torch.bfloat16, generator=g)
    q, k, v, do = mk(b, nq, h, d), mk(b, nk, hk, d), mk(b, nk, hk, d), mk(b, nq, h, d)
    qf, kf, vf = (t.float().requires_grad_(True) for t in (q, k, v))
    qpos = torch.arange(nq, device="cuda") + q_offset
    out = default_attention(qf, kf, vf, causal=causal, softclamp_qk_sim=softclamp,
                            softclamp_value=SOFTCLAMP_VALUE, q_positions=qpos)
    out.backward(do.float())
    with torch.no_grad():       # lse of the same scores (the oracle returns out only)
        sim = torch.einsum("bihd,bjhd->bhij", qf, kf.repeat(1, 1, h // hk, 1)) * d ** -0.5
        if softclamp:
            sim = softclamp_fn(sim, SOFTCLAMP_VALUE)
        if causal:
            cut = torch.arange(nk, device="cuda")[None, :] > qpos[:, None]
            sim = sim.masked_fill(cut[None, None], MASK_VALUE)
        lse = sim.logsumexp(dim=-1)
    ref = dict(out=out.detach(), lse=lse, dq=qf.grad, dk=kf.grad, dv=vf.grad)
    return (q, k, v, do), ref


def _check(name, got, ref, tol, relative):
    e = (got.float() - ref).abs().max().item()
    bound = tol * (ref.abs().max().item() + 1e-6 if relative else 1.0)
    print(f"{name}: max abs err {e:.4g} (bound {bound:.4g})")
    assert torch.isfinite(got.float()).all(), name
    assert e < bound, f"{name} err {e} >= {bound}"


def _check_grads(grads, ref, tol=GRAD_TOL):
    for name, g_ in zip(("dq", "dk", "dv"), grads):
        _check(name, g_, ref[name], tol, relative=True)


def _run(fn, q, k, v, do):
    """fn(q, k, v) -> (out, lse or None); returns out, lse, (dq, dk, dv)."""
    qg, kg, vg = (t.clone().requires_grad_(True) for t in (q, k, v))
    out, lse = fn(qg, kg, vg)
    out.backward(do)
    torch.cuda.synchronize()
    return out, lse, (qg.grad, kg.grad, vg.grad)


def _ring(causal, **kw):
    from ring_attention_amd.ops.ring_flash_hip import ring_flash_attn_hip_
    return lambda q, k, v: ring_flash_attn_hip_(q, k, v, causal=causal, **kw)


def _setenv(monkeypatch, env):
    for key, val in env.items():
        monkeypatch.setenv(key, val)


# ---------------------------------------------------------------------------
# single-pass launches (fused bf16 epilogue): plain, GQA, softclamp, offset
# diagonal, PAIRED
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("d", [32, 64, 128])
def test_plain(monkeypatch, d, causal):
    _setenv(monkeypatch, SINGLE_PASS_ENV)
    (q, k, v, do), ref = _case(1, 320, 320, 2, 2, d, causal)
    out, lse, grads = _run(_ring(causal), q, k, v, do)
    _check("out", out, ref["out"], OUT_TOL, relative=False)
    _check("lse", lse, ref["lse"], LSE_TOL, relative=False)
    _check_grads(grads, ref)


def test_gqa_group_loop(monkeypatch):
    _setenv(monkeypatch, SINGLE_PASS_ENV)
    (q, k, v, do), ref = _case(1, 320, 320, 4, 2, 64, True, seed=1)
    out, lse, grads = _run(_ring(True), q, k, v, do)
    _check("out", out, ref["out"], OUT_TOL, relative=False)
    _check("lse", lse, ref["lse"], LSE_TOL, relative=False)
    _check_grads(grads, ref)


@pytest.mark.parametrize("causal", [False, True])
def test_softclamp(monkeypatch, causal):
    _setenv(monkeypatch, SINGLE_PASS_ENV)
    (q, k, v, do), ref = _case(1, 320, 320, 2, 2, 64, causal, softclamp=True, seed=2)
    fn = _ring(causal, softclamp_qk_sim=True, softclamp_value=SOFTCLAMP_VALUE)
    out, lse, grads = _run(fn, q, k, v, do)
    _check("out", out, ref["out"], OUT_TOL, relative=False)
    _check("lse", lse, ref["lse"], LSE_TOL, relative=False)
    _check_grads(grads, ref, GRAD_TOL_SOFTCLAMP)


def test_cross_length_offset(monkeypatch):
    # test_bwd_epilogue.py::test_cross_length_offset's shape: nq != nk, the
    # diagonal offset by 512; once single-pass, once with dkv on descriptor
    # units (fp32 atomics, each unit's partial scaled in its own epilogue)
    from ring_attention_amd.ops.ring_flash_hip import flash_attn_offset
    (q, k, v, do), ref = _case(1, 256, 768, 4, 2, 64, True, q_offset=512, seed=4)
    fn = lambda q_, k_, v_: (flash_attn_offset(q_, k_, v_, q_offset=512, causal=True), None)
    monkeypatch.setenv("RING_ATTN_NO_DESC", "1")
    out, _, grads = _run(fn, q, k, v, do)
    _check("out", out, ref["out"], OUT_TOL, relative=False)
    _check_grads(grads, ref)
    monkeypatch.delenv("RING_ATTN_NO_DESC")
    _, _, grads = _run(fn, q, k, v, do)
    _check_grads(grads, ref)


@pytest.mark.parametrize("d", [64, 128])
def test_paired(monkeypatch, d):
    # test_bwd_epilogue.py::test_direct_paired's shape: the binding engages
    # the PAIRED instantiations of fwd, dq and dkv
    _setenv(monkeypatch, SINGLE_PASS_ENV)
    (q, k, v, do), ref = _case(4, 2048, 2048, 16, 16, d, True, seed=3)
    out, lse, grads = _run(_ring(True), q, k, v, do)
    _check("out", out, ref["out"], OUT_TOL, relative=False)
    _check("lse", lse, ref["lse"], LSE_TOL, relative=False)
    _check_grads(grads, ref)


# ---------------------------------------------------------------------------
# fp32-accumulating epilogues: the scale is applied exactly once per partial
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("d", [64, 128])
def test_split_atomic(monkeypatch, d, causal):
    _setenv(monkeypatch, {"RING_ATTN_SPLIT_DQ": "2", "RING_ATTN_SPLIT_DKV": "2",
                          "RING_ATTN_NO_DESC": "1"})
    (q, k, v, do), ref = _case(1, 320, 320, 2, 2, d, causal)
    _, _, grads = _run(_ring(causal), q, k, v, do)
    _check_grads(grads, ref)


@pytest.mark.parametrize("d", [64, 128])
def test_two_hop_accumulate(d):
    # non-causal, through the binding: dq summed over two kv halves, dk/dv
    # over two q halves, the second call of each with accumulate=True
    ext = _ext()
    (q, k, v, do), ref = _case(1, 320, 320, 2, 2, d, False)
    b, n, h, _ = q.shape
    scale, half = d ** -0.5, n // 2
    out = torch.empty_like(q)
    lse = torch.empty(b, h, n, device="cuda", dtype=torch.float32)
    ext.attn_fwd(q, k, v, None, None, None, None, out, lse, scale, False, 0,
                 1, 0, False, False, 50.0, True, True, 1, 0, None)
    delta = ext.attn_delta(do, out)
    tail = lambda acc, which: (scale, False, 0, 1, 0, False, False, 50.0, acc,
                               1, which, None, None)

    dq = torch.empty(b, n, h, d, device="cuda", dtype=torch.float32)
    for hop, sl in enumerate((slice(0, half), slice(half, n))):
        ext.attn_bwd(q, k[:, sl].contiguous(), v[:, sl].contiguous(), do, None,
                     lse, delta, dq, None, None, *tail(hop > 0, 1))

    dk = torch.empty(b, h, n, d, device="cuda", dtype=torch.float32)
    dv = torch.empty(b, h, d, n, device="cuda", dtype=torch.float32)
    for hop, sl in enumerate((slice(0, half), slice(half, n))):
        ext.attn_bwd(q[:, sl].contiguous(), k, v, do[:, sl].contiguous(), None,
                     lse[:, :, sl].contiguous(), delta[:, :, sl].contiguous(),
                     None, dk, dv, *tail(hop > 0, 2))
    torch.cuda.synchronize()
    _check_grads((dq, dk.permute(0, 2, 1, 3), dv.permute(0, 3, 1, 2)), ref)
