"""dkv kernel: transposed operands read from the row-major Q / dO images.

At d 32 and d 64 the dk/dv kernel stages each q tile once, row-major, and
builds the dO^T / Q^T fragments of the dv/dk MFMAs from those images with
ds_read_b64_tr_b16: per fragment two reads of 4 consecutive q rows, each
16-lane group addressing 4 rows x 16 d columns behind the row's XOR chunk
swizzle.  The softmax/ds blocks of dq and dkv use single-issue f32 ops.  What
can go wrong, and the smallest shapes that show it:

  * a wrong row / column pairing in a fragment (row term, lane group, swizzle
    key, element order): random data exposes it at any shape; nq = 1 .. 160
    ends the walk inside each 4-row read, 8-row pair, 16-row k-step and the
    second 32-row q block, then in a second and third tile;
  * rows past a ragged last tile: they are zeroed only in the row-major
    staging now, and the transposed reads must see those zeros (nq = 1, 3, 37,
    63, 69, 127, 160 leave 63 .. 32 dead rows);
  * a partly valid last kv wave (nk = 288) beside a ragged q tile;
  * the GQA group loop restaging the images behind the group barrier;
  * PAIRED (three kv tiles, the middle one self-paired), grid.z shares with
    the fp32 atomic epilogue, d 32 (4-chunk swizzle), d 128 (keeps the two
    image form), softclamp (its dtanh product is a single-issue op now);
  * a transposed read ahead of the barrier publishing its image: repeated
    launches must agree bitwise.

Every case is held to the fp32 oracle (ops/reference.py) at the bounds of
tests/test_dkv_prefetch.py: out 2e-2 abs, lse 2e-3 abs, gradients 4e-2 of the
reference's max (5e-2 with softclamp).  The q rows carry gains of 0.25 .. 3, so
lse differs from row to row by more than its random spread.
"""

import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

OUT_TOL = 2e-2
LSE_TOL = 2e-3
GRAD_TOL = 4e-2
GRAD_TOL_SOFTCLAMP = 5e-2
SOFTCLAMP_VALUE = 5.0

SINGLE_PASS_ENV = {"RING_ATTN_SPLIT_DQ": "1", "RING_ATTN_SPLIT_DKV": "1",
                   "RING_ATTN_NO_DESC": "1"}

NQ_EDGES = [1, 3, 37, 63, 64, 69, 127, 160]


def _ext():
    from ring_attention_amd.ops import hip_ext
    return hip_ext.require()


def _setenv(monkeypatch, env):
    for key, val in env.items():
        monkeypatch.setenv(key, val)


@functools.lru_cache(maxsize=None)
def _case(b, nq, nk, h, hk, d, causal, softclamp=False, seed=0):
    """bf16 inputs and the fp32 oracle's out / lse / dq / dk / dv; computed
    once and shared (callers must not modify it)."""
    from ring_attention_amd.ops.reference import (
        MASK_VALUE, default_attention, softclamp as softclamp_fn)
    g = torch.Generator(device="cuda").manual_seed(seed)
    mk = lambda *s: torch.randn(*s, device="cuda", dtype=torch.bfloat16, generator=g)
    q, k, v, do = mk(b, nq, h, d), mk(b, nk, hk, d), mk(b, nk, hk, d), mk(b, nq, h, d)
    # per-row gain: sharp and flat softmax rows side by side (lse spread)
    gain = 0.25 + 2.75 * torch.rand(b, nq, h, 1, device="cuda", generator=g)
    q = (q.float() * gain).to(torch.bfloat16)
    qf, kf, vf = (t.float().requires_grad_(True) for t in (q, k, v))
    out = default_attention(qf, kf, vf, mask=None, causal=causal,
                            softclamp_qk_sim=softclamp, softclamp_value=SOFTCLAMP_VALUE)
    out.backward(do.float())
    with torch.no_grad():       # lse of the same scores (the oracle returns out only)
        sim = torch.einsum("bihd,bjhd->bhij", qf, kf.repeat(1, 1, h // hk, 1)) * d ** -0.5
        if softclamp:
            sim = softclamp_fn(sim, SOFTCLAMP_VALUE)
        if causal:
            cut = torch.arange(nk, device="cuda")[None, :] > torch.arange(nq, device="cuda")[:, None]
            sim = sim.masked_fill(cut[None, None], MASK_VALUE)
        lse = sim.logsumexp(dim=-1)
    ref = dict(out=out.detach(), lse=lse, dq=qf.grad, dk=kf.grad, dv=vf.grad)
    return (q, k, v, do), ref


# Causal with nq = 1 attends a single key: p = 1, ds = p * (dp - delta) is
# analytically ZERO and with it dq = ds k and dk = ds^T q (dv = p^T do is
# not), so no multiple of the reference's max can bound them.  Oracle and
# kernel both return what is left of dp - delta, two fp32 dot products over
# d of terms up to |do * v| ~ 10 that cancel: rounding noise of order
# d * 2^-24 * 10 ~ 4e-5 before the O(1) factors k, q and scale.  Those two
# gradients of that one case are held to this absolute bound (a tenth of a
# bf16 ulp of the other cases' gradients); every other check is
# tests/test_dkv_prefetch.py's _check unchanged.
ZERO_DS_ABS = 4e-5


def _check(name, got, ref, tol, relative):
    e = (got.float() - ref).abs().max().item()
    bound = tol * (ref.abs().max().item() + 1e-6 if relative else 1.0)
    print(f"{name}: max abs err {e:.4g} (bound {bound:.4g})")
    assert torch.isfinite(got.float()).all(), name
    assert e < bound, f"{name} err {e} >= {bound}"


def _check_zero(name, got, ref, bound):
    assert ref.abs().max().item() < bound, f"{name}: reference is not zero"
    e = got.float().abs().max().item()
    print(f"{name}: max abs {e:.4g} (reference zero, bound {bound:.4g})")
    assert torch.isfinite(got.float()).all(), name
    assert e < bound, f"{name} abs {e} >= {bound}"


def _check_grads(grads, ref, tol=GRAD_TOL, names=("dq", "dk", "dv"), zero_ds=False):
    for name, g_ in zip(names, grads):
        if zero_ds and name in ("dq", "dk"):
            _check_zero(name, g_, ref[name], ZERO_DS_ABS)
        else:
            _check(name, g_, ref[name], tol, relative=True)


def _run(fn, q, k, v, do):
    """fn(q, k, v) -> out or (out, lse); returns out, lse or None, (dq, dk, dv)."""
    qg, kg, vg = (t.clone().requires_grad_(True) for t in (q, k, v))
    res = fn(qg, kg, vg)
    out, lse = res if isinstance(res, tuple) else (res, None)
    out.backward(do)
    torch.cuda.synchronize()
    return out.detach(), lse, (qg.grad, kg.grad, vg.grad)


def _ring(causal, **kw):
    from ring_attention_amd.ops.ring_flash_hip import ring_flash_attn_hip_
    return lambda q, k, v: ring_flash_attn_hip_(q, k, v, causal=causal, **kw)


def _flash(causal, **kw):
    # single launch per kernel, nq != nk allowed; bf16 epilogue
    from ring_attention_amd.ops.ring_flash_hip import flash_attn
    return lambda q, k, v: flash_attn(q, k, v, causal=causal, **kw)


def _check_all(fn, inputs, ref, grad_tol=GRAD_TOL, zero_ds=False):
    out, lse, grads = _run(fn, *inputs)
    _check("out", out, ref["out"], OUT_TOL, relative=False)
    if lse is not None:
        _check("lse", lse.detach(), ref["lse"], LSE_TOL, relative=False)
    _check_grads(grads, ref, grad_tol, zero_ds=zero_ds)


def _dkv_split(q, k, v, do, causal, split):
    """dk, dv (b, nk, hk, d) from one dkv launch through the binding with
    `split` grid.z shares: fp32 atomics into zeroed scratch buffers."""
    ext = _ext()
    b, nq, h, d = q.shape
    nk, hk = k.shape[1], k.shape[2]
    out = torch.empty_like(q)
    lse = torch.empty(b, h, nq, device="cuda", dtype=torch.float32)
    ext.attn_fwd(q, k, v, None, None, None, None, out, lse, d ** -0.5, causal, 0,
                 1, 0, False, False, 50.0, True, True, 1, 0, None)
    delta = ext.attn_delta(do, out)
    dk = torch.zeros(b, hk, nk, d, device="cuda", dtype=torch.float32)
    dv = torch.zeros(b, hk, d, nk, device="cuda", dtype=torch.float32)
    ext.attn_bwd(q, k, v, do, None, lse, delta, None, dk, dv, d ** -0.5, causal,
                 0, 1, 0, False, False, 50.0, False, split, 2, None, None)
    torch.cuda.synchronize()
    return dk.permute(0, 2, 1, 3), dv.permute(0, 3, 1, 2)


# ---------------------------------------------------------------------------
# every address class of the transposed reads, and the ragged zeroing
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("nq", NQ_EDGES)
def test_q_tile_edges(nq, causal):
    inputs, ref = _case(2, nq, 256, 2, 2, 64, causal, seed=nq)
    _check_all(_flash(causal), inputs, ref, zero_ds=(causal and nq == 1))


@pytest.mark.parametrize("causal", [False, True])
def test_partly_valid_wave_ragged_tile(causal):
    # nk = 288: the second kv tile's first wave is its only valid one
    inputs, ref = _case(1, 69, 288, 2, 2, 64, causal, seed=11)
    _check_all(_flash(causal), inputs, ref)


@pytest.mark.parametrize("causal", [False, True])
def test_gqa_group_loop(causal):
    inputs, ref = _case(2, 69, 256, 4, 2, 64, causal, seed=12)
    _check_all(_flash(causal), inputs, ref)


def test_paired_three_kv_tiles(monkeypatch):
    # three kv tiles at b * hk = 128 pass the binding's PAIRED gate (as
    # tests/test_dkv_prefetch.py::test_paired_odd_tile_count); the middle
    # tile is self-paired
    n, b, h = 768, 2, 64
    assert -(-n // 256) == 3 and -(-3 // 2) * b * h == 256
    _setenv(monkeypatch, dict(SINGLE_PASS_ENV, RING_ATTN_KV_SPLIT="1"))
    inputs, ref = _case(b, n, n, h, h, 64, True, seed=13)
    _check_all(_ring(True), inputs, ref)


@pytest.mark.parametrize("nq", [69, 192])
def test_grid_z_shares_atomic_epilogue(nq):
    # two grid.z shares: nq 69 gives one tile each (the second ragged), nq
    # 192 two tiles and one
    inputs, ref = _case(1, nq, 256, 2, 2, 64, False, seed=14)
    dk, dv = _dkv_split(*inputs, False, split=2)
    _check_grads((dk, dv), ref, names=("dk", "dv"))


@pytest.mark.parametrize("d", [32, 128])
def test_other_head_dims(d):
    # d 32: same reads under the 4-chunk swizzle; d 128: two-image form
    inputs, ref = _case(2, 69, 256, 2, 2, d, False, seed=15)
    _check_all(_flash(False), inputs, ref)


def test_softclamp():
    inputs, ref = _case(2, 69, 256, 2, 2, 64, True, softclamp=True, seed=16)
    fn = _flash(True, softclamp_qk_sim=True, softclamp_value=SOFTCLAMP_VALUE)
    _check_all(fn, inputs, ref, GRAD_TOL_SOFTCLAMP)


# ---------------------------------------------------------------------------
# race guard
# ---------------------------------------------------------------------------
def test_repeated_launches_agree_bitwise():
    # single pass: one writer and a fixed summation order per element
    inputs, ref = _case(2, 160, 256, 2, 2, 64, False, seed=160)
    _, _, first = _run(_flash(False), *inputs)
    _, _, second = _run(_flash(False), *inputs)
    for name, a, b_ in zip(("dq", "dk", "dv"), first, second):
        same = torch.equal(a, b_)
        print(f"{name}: bitwise equal {same}")
        assert same, f"{name} differs between two launches"
