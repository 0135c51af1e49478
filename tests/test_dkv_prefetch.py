"""dkv kernel: scalar uniform state and explicit LDS operand prefetch.

The d64 dk/dv body keeps its wave-uniform state (parameters, tile bounds,
loop counters) in SGPRs, reads its MFMA operands from LDS one block of work
ahead of the MFMAs, loads q tiles unconditionally (rows past a ragged end are
clamped on load and zeroed when staged) and rebuilds the masked-path row
positions from one per-lane base.  What can go wrong, and the smallest shapes
that show it:

  * a value that is uniform per workgroup taken as uniform per grid: two
    batches, two kv heads, a GQA group loop of 2, three kv tiles;
  * a per-lane value made scalar: Nk % 32 != 0 (last wave partly valid) and
    key-pad masks that differ inside a batch;
  * the prefetch across q-walk lengths: one q tile, a tile whose second
    32-row block is all invalid, two and three tiles; empty and one-tile
    grid.z shares; PAIRED with an odd tile count; descriptor units;
  * a read hoisted over the barrier that publishes its buffer: repeated
    launches must agree bitwise.

Every case is held to the fp32 oracle (ops/reference.py) at the bounds of
tests/test_gpu_kernels.py, as tests/test_valu_diet.py: out 2e-2 abs, lse 2e-3
abs, gradients 4e-2 of the reference's max (5e-2 with softclamp).
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


def _ext():
    from ring_attention_amd.ops import hip_ext
    return hip_ext.require()


def _setenv(monkeypatch, env):
    for key, val in env.items():
        monkeypatch.setenv(key, val)


@functools.lru_cache(maxsize=None)
def _case(b, nq, nk, h, hk, d, causal, softclamp=False, pads=None, seed=0):
    """bf16 inputs, the key-pad mask (b, nk) bool or None (batch i keeps its
    first nk - pads[i] keys) and the fp32 oracle's out / lse / dq / dk / dv;
    computed once and shared (callers must not modify it)."""
    from ring_attention_amd.ops.reference import (
        MASK_VALUE, default_attention, softclamp as softclamp_fn)
    g = torch.Generator(device="cuda").manual_seed(seed)
    mk = lambda *s: torch.randn(*s, device="cuda", dtype=torch.bfloat16, generator=g)
    q, k, v, do = mk(b, nq, h, d), mk(b, nk, hk, d), mk(b, nk, hk, d), mk(b, nq, h, d)
    mask = None
    if pads is not None:
        keep = torch.tensor([nk - p for p in pads], device="cuda")
        mask = torch.arange(nk, device="cuda")[None, :] < keep[:, None]
    qf, kf, vf = (t.float().requires_grad_(True) for t in (q, k, v))
    out = default_attention(qf, kf, vf, mask=mask, causal=causal,
                            softclamp_qk_sim=softclamp, softclamp_value=SOFTCLAMP_VALUE)
    out.backward(do.float())
    with torch.no_grad():       # lse of the same scores (the oracle returns out only)
        sim = torch.einsum("bihd,bjhd->bhij", qf, kf.repeat(1, 1, h // hk, 1)) * d ** -0.5
        if softclamp:
            sim = softclamp_fn(sim, SOFTCLAMP_VALUE)
        if mask is not None:
            sim = sim.masked_fill(~mask[:, None, None, :], MASK_VALUE)
        if causal:
            cut = torch.arange(nk, device="cuda")[None, :] > torch.arange(nq, device="cuda")[:, None]
            sim = sim.masked_fill(cut[None, None], MASK_VALUE)
        lse = sim.logsumexp(dim=-1)
    ref = dict(out=out.detach(), lse=lse, dq=qf.grad, dk=kf.grad, dv=vf.grad)
    return (q, k, v, do), mask, ref


def _check(name, got, ref, tol, relative):
    e = (got.float() - ref).abs().max().item()
    bound = tol * (ref.abs().max().item() + 1e-6 if relative else 1.0)
    print(f"{name}: max abs err {e:.4g} (bound {bound:.4g})")
    assert torch.isfinite(got.float()).all(), name
    assert e < bound, f"{name} err {e} >= {bound}"


def _check_grads(grads, ref, tol=GRAD_TOL, names=("dq", "dk", "dv")):
    for name, g_ in zip(names, grads):
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


def _flash(causal, mask=None):
    # single launch per kernel, nq != nk allowed, optional key-pad mask
    from ring_attention_amd.ops.ring_flash_hip import flash_attn
    return lambda q, k, v: flash_attn(q, k, v, key_pad_mask=mask, causal=causal)


def _check_all(fn, inputs, ref, grad_tol=GRAD_TOL):
    out, lse, grads = _run(fn, *inputs)
    _check("out", out, ref["out"], OUT_TOL, relative=False)
    if lse is not None:
        _check("lse", lse.detach(), ref["lse"], LSE_TOL, relative=False)
    _check_grads(grads, ref, grad_tol)


def _fwd_direct(q, k, v, causal):
    """out, lse, delta-ready forward through the binding (single pass)."""
    ext = _ext()
    b, nq, h, d = q.shape
    out = torch.empty_like(q)
    lse = torch.empty(b, h, nq, device="cuda", dtype=torch.float32)
    ext.attn_fwd(q, k, v, None, None, None, None, out, lse, d ** -0.5, causal, 0,
                 1, 0, False, False, 50.0, True, True, 1, 0, None)
    return out, lse


def _dkv_direct(q, k, v, do, out, lse, causal, split=1, desc=None):
    """dk, dv (b, nk, hk, d) from one dkv launch through the binding; grid.z
    shares and descriptor units accumulate with atomics into zeroed buffers,
    a plain launch stores into NaN-filled ones."""
    ext = _ext()
    b, nq, h, d = q.shape
    nk, hk = k.shape[1], k.shape[2]
    delta = ext.attn_delta(do, out)
    atomic = split > 1 or desc is not None
    fill = 0.0 if atomic else float("nan")
    dk = torch.full((b, hk, nk, d), fill, device="cuda", dtype=torch.float32)
    dv = torch.full((b, hk, d, nk), fill, device="cuda", dtype=torch.float32)
    ext.attn_bwd(q, k, v, do, None, lse, delta, None, dk, dv, d ** -0.5, causal,
                 0, 1, 0, False, False, 50.0, False, split, 2, None, desc)
    torch.cuda.synchronize()
    return dk.permute(0, 2, 1, 3), dv.permute(0, 3, 1, 2)


# ---------------------------------------------------------------------------
# uniform per workgroup, not per grid
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("causal", [False, True])
def test_uniform_per_workgroup(monkeypatch, causal):
    # three kv tiles (the last one 64 rows), two batches, two kv heads, a GQA
    # group loop of 2
    _setenv(monkeypatch, SINGLE_PASS_ENV)
    inputs, _, ref = _case(2, 576, 576, 4, 2, 64, causal)
    _check_all(_ring(causal), inputs, ref)


# ---------------------------------------------------------------------------
# per-lane values stay per-lane
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("causal", [False, True])
def test_partly_valid_wave(causal):
    # Nk % 32 != 0: kv rows 288..299 are the valid lanes of the last wave;
    # nq = 200 ends in a ragged q tile whose second 32-row block is empty
    inputs, _, ref = _case(1, 200, 300, 2, 2, 64, causal, seed=1)
    _check_all(_flash(causal), inputs, ref)


@pytest.mark.parametrize("causal", [False, True])
def test_key_pad_differs_in_batch(causal):
    inputs, mask, ref = _case(2, 200, 300, 2, 2, 64, causal, pads=(7, 150), seed=2)
    _check_all(_flash(causal, mask), inputs, ref)


# ---------------------------------------------------------------------------
# q-walk lengths around the prefetch
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("nq", [64, 96, 128, 192])
def test_q_walk_lengths(nq, causal):
    # one tile / a tile with an all-invalid second q block / two / three tiles
    inputs, _, ref = _case(1, nq, 256, 2, 2, 64, causal, seed=3)
    _check_all(_flash(causal), inputs, ref)


@pytest.mark.parametrize("d", [32, 128])
def test_q_walk_other_head_dims(d):
    inputs, _, ref = _case(1, 96, 256, 2, 2, d, False, seed=3)
    _check_all(_flash(False), inputs, ref)


@pytest.mark.parametrize("nq", [64, 192])
def test_grid_z_shares(nq):
    # two grid.z shares of the q walk: nq 64 leaves one share empty, nq 192
    # gives shares of two tiles and one
    inputs, _, ref = _case(1, nq, 256, 2, 2, 64, False, seed=3)
    q, k, v, do = inputs
    out, lse = _fwd_direct(q, k, v, False)
    dk, dv = _dkv_direct(q, k, v, do, out, lse, False, split=2)
    _check_grads((dk, dv), ref, names=("dk", "dv"))


def test_paired_odd_tile_count(monkeypatch):
    # tests/test_mask_exactness.py::test_paired_odd_tile_count's shape: three
    # kv tiles at b * h = 128 pass the binding's PAIRED gate; the middle tile
    # is self-paired (one pass of the pair loop)
    n, b, h = 640, 8, 16
    assert -(-n // 256) == 3 and -(-3 // 2) * b * h == 256
    _setenv(monkeypatch, dict(SINGLE_PASS_ENV, RING_ATTN_KV_SPLIT="1"))
    inputs, _, ref = _case(b, n, n, h, h, 64, True, seed=4)
    _check_all(_ring(True), inputs, ref)


def test_descriptor_units():
    # descriptor units of the dkv walk, as tests/test_mask_exactness.py
    # engages them: built by _walk_descriptors, passed to the binding
    from ring_attention_amd.ops.ring_flash_hip import _walk_descriptors
    b, n, h, hk, d = 1, 576, 4, 2, 64
    inputs, _, ref = _case(b, n, n, h, hk, d, True, seed=5)
    q, k, v, do = inputs
    out, lse = _fwd_direct(q, k, v, True)
    desc = _walk_descriptors("dkv", d, n, n, 0, 1, b * hk, q.device)
    assert desc is not None and desc.shape[0] > -(-n // 256)   # tiles are cut into units
    dk, dv = _dkv_direct(q, k, v, do, out, lse, True, desc=desc)
    _check_grads((dk, dv), ref, names=("dk", "dv"))


def test_softclamp(monkeypatch):
    _setenv(monkeypatch, SINGLE_PASS_ENV)
    inputs, _, ref = _case(1, 576, 576, 4, 2, 64, True, softclamp=True, seed=6)
    fn = _ring(True, softclamp_qk_sim=True, softclamp_value=SOFTCLAMP_VALUE)
    _check_all(fn, inputs, ref, GRAD_TOL_SOFTCLAMP)


def test_two_hop_accumulate():
    # dk / dv summed over two q halves, the second launch with accumulate
    ext = _ext()
    d = 64
    inputs, _, ref = _case(1, 320, 320, 4, 2, d, False, seed=7)
    q, k, v, do = inputs
    b, n, h, _ = q.shape
    hk = k.shape[2]
    out, lse = _fwd_direct(q, k, v, False)
    delta = ext.attn_delta(do, out)
    dk = torch.full((b, hk, n, d), float("nan"), device="cuda", dtype=torch.float32)
    dv = torch.full((b, hk, d, n), float("nan"), device="cuda", dtype=torch.float32)
    half = n // 2
    for hop, sl in enumerate((slice(0, half), slice(half, n))):
        ext.attn_bwd(q[:, sl].contiguous(), k, v, do[:, sl].contiguous(), None,
                     lse[:, :, sl].contiguous(), delta[:, :, sl].contiguous(),
                     None, dk, dv, d ** -0.5, False, 0, 1, 0, False, False, 50.0,
                     hop > 0, 1, 2, None, None)
    torch.cuda.synchronize()
    _check_grads((dk.permute(0, 2, 1, 3), dv.permute(0, 3, 1, 2)), ref,
                 names=("dk", "dv"))


# ---------------------------------------------------------------------------
# race guard
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("causal", [False, True])
def test_repeated_launches_agree_bitwise(monkeypatch, causal):
    # single pass: every output element has one writer and a fixed summation
    # order, so five launches on the same inputs must agree bit for bit; a
    # read that runs ahead of the barrier publishing its LDS buffer does not
    _setenv(monkeypatch, SINGLE_PASS_ENV)
    inputs, _, ref = _case(1, 1024, 1024, 4, 2, 64, causal, seed=8)
    first = None
    for launch in range(5):
        _, _, grads = _run(_ring(causal), *inputs)
        if first is None:
            first = grads
            _check_grads(grads, ref)
            continue
        for name, a, b_ in zip(("dq", "dk", "dv"), first, grads):
            same = torch.equal(a, b_)
            print(f"launch {launch} {name}: bitwise equal {same}")
            assert same, f"{name} differs between launch 0 and launch {launch}"
