"""Backward gradient epilogue: final-layout bf16 gradients straight from the
dq/dkv kernels (single-pass launches) or from ONE attn_bwd_finalize launch
(fp32-accumulating launches), against the torch permute/contiguous/cast chain
that RING_ATTN_NO_FUSED_EPILOGUE=1 still selects.

Both sides round the same fp32 value with round-to-nearest-even and the build
has no fast-math, so wherever the fp32 value itself is deterministic (single
writer per element) the comparison is BITWISE (torch.equal).  Launches that
accumulate with fp32 atomics (grid.z splits, descriptor units) have a
run-to-run summation order, so those are held to the fp32 oracle at the
tolerance test_gpu_kernels.test_fwd_bwd_parity uses (4e-2 of the reference's
max), and the finalize kernel itself is checked bitwise on fixed fp32 buffers.

The ring Function fills the chip with grid.z splits at test-sized shapes, so
the direct-epilogue cases pin RING_ATTN_SPLIT_DQ/DKV=1 and RING_ATTN_NO_DESC=1
for BOTH runs: that is the single-pass launch the headline shape takes.
"""

import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

SINGLE_PASS_ENV = {"RING_ATTN_SPLIT_DQ": "1", "RING_ATTN_SPLIT_DKV": "1",
                   "RING_ATTN_NO_DESC": "1"}
REL_TOL = 4e-2          # test_fwd_bwd_parity's gradient bound


def _ext():
    from ring_attention_amd.ops import hip_ext
    return hip_ext.require()


def _mk(b, nq, nk, h, hk, d, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    q = torch.randn(b, nq, h, d, device="cuda", dtype=torch.bfloat16, generator=g)
    k = torch.randn(b, nk, hk, d, device="cuda", dtype=torch.bfloat16, generator=g)
    v = torch.randn(b, nk, hk, d, device="cuda", dtype=torch.bfloat16, generator=g)
    do = torch.randn(b, nq, h, d, device="cuda", dtype=torch.bfloat16, generator=g)
    return q, k, v, do


def _grads(fn, q, k, v, do):
    qg, kg, vg = (t.clone().requires_grad_(True) for t in (q, k, v))
    out = fn(qg, kg, vg)
    out.backward(do.to(out.dtype))
    torch.cuda.synchronize()
    return qg.grad, kg.grad, vg.grad


def _ab(monkeypatch, fn, q, k, v, do, env=()):
    """(fused grads, unfused grads) of the same call within one process."""
    for key, val in dict(env).items():
        monkeypatch.setenv(key, val)
    monkeypatch.delenv("RING_ATTN_NO_FUSED_EPILOGUE", raising=False)
    fused = _grads(fn, q, k, v, do)
    monkeypatch.setenv("RING_ATTN_NO_FUSED_EPILOGUE", "1")
    plain = _grads(fn, q, k, v, do)
    monkeypatch.delenv("RING_ATTN_NO_FUSED_EPILOGUE")
    return fused, plain


def _assert_bitwise(fused, plain):
    for a, r, name in zip(fused, plain, ("dq", "dk", "dv")):
        assert a.dtype == r.dtype and a.shape == r.shape, name
        assert a.is_contiguous(), name
        assert torch.isfinite(r.float()).all(), name
        assert torch.equal(a, r), (
            f"{name}: {(a != r).sum().item()} of {a.numel()} elements differ, "
            f"max abs {(a.float() - r.float()).abs().max().item()}")


def _ring(causal):
    from ring_attention_amd.ops.ring_flash_hip import ring_flash_attn_hip
    return lambda q, k, v: ring_flash_attn_hip(q, k, v, causal=causal)


# ---------------------------------------------------------------------------
# direct epilogue
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("d", [32, 64, 128])
def test_direct_plain(monkeypatch, d, causal):
    q, k, v, do = _mk(2, 512, 512, 4, 4, d)
    _assert_bitwise(*_ab(monkeypatch, _ring(causal), q, k, v, do, SINGLE_PASS_ENV))


@pytest.mark.parametrize("causal", [False, True])
def test_direct_flash_attn_function(monkeypatch, causal):
    # FlashAttnFunction is single-pass at every shape (no env pinning)
    from ring_attention_amd.ops.ring_flash_hip import flash_attn
    q, k, v, do = _mk(2, 512, 512, 4, 4, 64, seed=1)
    fn = lambda q_, k_, v_: flash_attn(q_, k_, v_, causal=causal)
    _assert_bitwise(*_ab(monkeypatch, fn, q, k, v, do))


@pytest.mark.parametrize("h,hk,d,causal", [(8, 2, 64, True), (4, 2, 128, False)])
def test_direct_gqa_group_loop(monkeypatch, h, hk, d, causal):
    q, k, v, do = _mk(2, 512, 512, h, hk, d, seed=2)
    _assert_bitwise(*_ab(monkeypatch, _ring(causal), q, k, v, do, SINGLE_PASS_ENV))


@pytest.mark.parametrize("d", [64, 128])
def test_direct_paired(monkeypatch, d):
    # causal, 8 q/kv tiles x (b*h = 64): the paired grid is ceil(8/2)*64 = 256
    # workgroups, so the binding engages PAIRED for dq and dkv
    q, k, v, do = _mk(4, 2048, 2048, 16, 16, d, seed=3)
    _assert_bitwise(*_ab(monkeypatch, _ring(True), q, k, v, do, SINGLE_PASS_ENV))


def test_cross_length_offset(monkeypatch):
    from ring_attention_amd.ops.ring_flash_hip import flash_attn_offset
    q, k, v, do = _mk(1, 256, 768, 4, 2, 64, seed=4)
    fn = lambda q_, k_, v_: flash_attn_offset(q_, k_, v_, q_offset=512, causal=True)
    # single-pass dkv (descriptor units off): everything bitwise
    _assert_bitwise(*_ab(monkeypatch, fn, q, k, v, do, {"RING_ATTN_NO_DESC": "1"}))
    # default heuristics put dkv on descriptor units (fp32 atomics, then the
    # finalize kernel): dq is still single-writer, dk/dv differ only by the
    # atomics' summation order
    monkeypatch.delenv("RING_ATTN_NO_DESC")
    fused, plain = _ab(monkeypatch, fn, q, k, v, do)
    assert torch.equal(fused[0], plain[0])
    for a, r, name in zip(fused[1:], plain[1:], ("dk", "dv")):
        e = (a.float() - r.float()).abs().max().item()
        assert e <= REL_TOL * r.float().abs().max().item(), f"{name} {e}"


# ---------------------------------------------------------------------------
# ragged tiles, through the binding, outputs fenced by canaries
# ---------------------------------------------------------------------------
PAD = 4096          # canary elements on either side (keeps 16-byte alignment)
SENTINEL = 777.0


def _fenced(shape):
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + 2 * PAD,), SENTINEL, device="cuda", dtype=torch.bfloat16)
    return buf, buf[PAD:PAD + n].view(shape)


def _binding_bwd(q, k, v, do, causal, diag, fused):
    ext = _ext()
    b, nq, h, d = q.shape
    nk, hk = k.shape[1], k.shape[2]
    scale = d ** -0.5
    out = torch.empty_like(q)
    lse = torch.empty(b, h, nq, device="cuda", dtype=torch.float32)
    ext.attn_fwd(q, k, v, None, None, None, None, out, lse, scale, causal, diag,
                 1, 0, False, False, 50.0, True, True, 1, 0, None)
    delta = ext.attn_delta(do, out)
    tail = (scale, causal, diag, 1, 0, False, False, 50.0, False, 1, 0, None, None)
    if not fused:
        dq = torch.empty(b, nq, h, d, device="cuda", dtype=torch.float32)
        dk = torch.empty(b, hk, nk, d, device="cuda", dtype=torch.float32)
        dv = torch.empty(b, hk, d, nk, device="cuda", dtype=torch.float32)
        ext.attn_bwd(q, k, v, do, None, lse, delta, dq, dk, dv, *tail)
        return (dq.to(torch.bfloat16),
                dk.permute(0, 2, 1, 3).contiguous().to(torch.bfloat16),
                dv.permute(0, 3, 1, 2).contiguous().to(torch.bfloat16))
    fences = [_fenced(t.shape) for t in (q, k, v)]
    ext.attn_bwd(q, k, v, do, None, lse, delta, None, None, None, *tail,
                 dq_bf=fences[0][1], dk_bf=fences[1][1], dv_bf=fences[2][1])
    torch.cuda.synchronize()
    for (buf, _), name in zip(fences, ("dq", "dk", "dv")):
        assert (buf[:PAD] == SENTINEL).all(), f"{name}: store below the tensor"
        assert (buf[-PAD:] == SENTINEL).all(), f"{name}: store past the tensor"
    return tuple(view for _, view in fences)


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("n,d", [(320, 64),      # last tile of 64 rows
                                 (200, 128)])    # a single partial tile
def test_ragged_tiles_with_canaries(n, d, causal):
    q, k, v, do = _mk(1, n, n, 2, 2, d, seed=5)
    plain = _binding_bwd(q, k, v, do, causal, 0, fused=False)
    fused = _binding_bwd(q, k, v, do, causal, 0, fused=True)
    _assert_bitwise(fused, plain)
    # and both are right: a partially valid wave (n % 32 != 0) must still
    # write every d column of its valid kv rows
    qf, kf, vf = (t.float().requires_grad_(True) for t in (q, k, v))
    s = torch.einsum("bihd,bjhd->bhij", qf, kf) * d ** -0.5
    if causal:
        s = s.masked_fill(torch.ones(n, n, device="cuda").triu(1).bool(), float("-inf"))
    torch.einsum("bhij,bjhd->bihd", s.softmax(-1), vf).backward(do.float())
    _assert_close_to_oracle(fused, tuple(t.grad.cpu() for t in (qf, kf, vf)))


# ---------------------------------------------------------------------------
# finalize kernel
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("d", [32, 64, 128])
@pytest.mark.parametrize("n", [64, 200, 513])
def test_finalize_binding(n, d):
    b, hk, h = 2, 3, 6
    g = torch.Generator(device="cuda").manual_seed(n * 1000 + d)
    dk = torch.randn(b, hk, n, d, device="cuda", generator=g)
    dv = torch.randn(b, hk, d, n, device="cuda", generator=g)
    dq = torch.randn(b, n, h, d, device="cuda", generator=g)
    dq_bf, dk_bf, dv_bf = _ext().attn_bwd_finalize(dk, dv, dq)
    assert torch.equal(dk_bf, dk.permute(0, 2, 1, 3).contiguous().to(torch.bfloat16))
    assert torch.equal(dv_bf, dv.permute(0, 3, 1, 2).contiguous().to(torch.bfloat16))
    assert torch.equal(dq_bf, dq.to(torch.bfloat16))
    # each part alone
    _, dk2, dv2 = _ext().attn_bwd_finalize(dk, dv)
    assert torch.equal(dk2, dk_bf) and torch.equal(dv2, dv_bf)
    dq2, none_k, none_v = _ext().attn_bwd_finalize(None, None, dq)
    assert torch.equal(dq2, dq_bf) and none_k is None and none_v is None


REF_SHAPE = dict(b=2, n=512, h=4, d=64)


@functools.lru_cache(maxsize=None)
def _reference():
    """bf16 inputs and the fp32 CPU oracle's gradients for REF_SHAPE, causal;
    computed once and shared (callers must not modify it)."""
    from ring_attention_amd.ops.ring_flash import ring_flash_attn_
    s = REF_SHAPE
    q, k, v, do = _mk(s["b"], s["n"], s["n"], s["h"], s["h"], s["d"], seed=6)
    qc, kc, vc = (t.float().cpu().requires_grad_(True) for t in (q, k, v))
    out, lse = ring_flash_attn_(qc, kc, vc, causal=True, bucket_size=64)
    out.backward(do.float().cpu())
    return (q, k, v, do), (qc.grad, kc.grad, vc.grad)


def _assert_close_to_oracle(grads, ref):
    for a, r, name in zip(grads, ref, ("dq", "dk", "dv")):
        e = (a.float().cpu() - r).abs().max().item()
        bound = REL_TOL * r.abs().max().item()
        print(f"{name}: max abs err {e:.4g} (bound {bound:.4g})")
        assert e <= bound, f"{name} err {e} > {bound}"


def test_finalize_end_to_end_split(monkeypatch):
    (q, k, v, do), ref = _reference()
    env = {"RING_ATTN_SPLIT_DQ": "2", "RING_ATTN_SPLIT_DKV": "2"}
    fused, plain = _ab(monkeypatch, _ring(True), q, k, v, do, env)
    _assert_close_to_oracle(fused, ref)
    _assert_close_to_oracle(plain, ref)

    # the same split launch through the binding: finalize is bitwise the
    # torch chain on the SAME fp32 buffers
    ext = _ext()
    b, n, h, d = q.shape
    out = torch.empty_like(q)
    lse = torch.empty(b, h, n, device="cuda", dtype=torch.float32)
    ext.attn_fwd(q, k, v, None, None, None, None, out, lse, d ** -0.5, True, 0,
                 1, 0, False, False, 50.0, True, True, 1, 0, None)
    delta = ext.attn_delta(do, out)
    dq = torch.zeros(b, n, h, d, device="cuda", dtype=torch.float32)
    dk = torch.zeros(b, h, n, d, device="cuda", dtype=torch.float32)
    dv = torch.zeros(b, h, d, n, device="cuda", dtype=torch.float32)
    ext.attn_bwd(q, k, v, do, None, lse, delta, dq, dk, dv, d ** -0.5, True, 0,
                 1, 0, False, False, 50.0, False, 2, 0, None, None)
    dq_bf, dk_bf, dv_bf = ext.attn_bwd_finalize(dk, dv, dq)
    assert torch.equal(dq_bf, dq.to(torch.bfloat16))
    assert torch.equal(dk_bf, dk.permute(0, 2, 1, 3).contiguous().to(torch.bfloat16))
    assert torch.equal(dv_bf, dv.permute(0, 3, 1, 2).contiguous().to(torch.bfloat16))
    _assert_close_to_oracle((dq_bf, dk_bf, dv_bf), ref)


# ---------------------------------------------------------------------------
# multi-rank wiring (all-gather reduce-scatter, ring accumulator) on one GPU
# through the in-process loopback layer
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("pin_single_pass", [True, False])
@pytest.mark.parametrize("strategy,causal,striped,hk", [
    ("allgather", False, False, 4),
    ("allgather", True, True, 2),
    ("ring", False, False, 4),
    ("ring", True, False, 2),
])
def test_multirank_fused_vs_unfused(monkeypatch, strategy, causal, striped, hk,
                                    pin_single_pass):
    """Two ranks.  With the splits pinned to 1 every fp32 value has one
    writer per rank and the two-rank sum is commutative, so fused and unfused
    are bitwise equal: all-gather takes dq straight from the kernel and dk/dv
    through finalize after the reduce-scatter; ring takes all three through
    finalize after the accumulator comes home.  With the default heuristics
    (grid.z splits, fp32 atomics) both are held to the unsharded run."""
    from ring_attention_amd.ops.ring_flash_hip import ring_flash_attn_hip_
    from .loopback_dist import loopback_world
    world, b, n_total, h, d = 2, 2, 1024, 4, 64
    q, k, v, do = _mk(b, n_total, n_total, h, hk, d, seed=8)

    def shard(rank):
        n = n_total // world
        if striped:
            return torch.arange(n, device="cuda") * world + rank
        return torch.arange(n, device="cuda") + rank * n

    monkeypatch.setenv("RING_ATTN_FORCE_STRATEGY", strategy)
    if pin_single_pass:
        for key, val in SINGLE_PASS_ENV.items():
            monkeypatch.setenv(key, val)

    def run(rank):
        idx = shard(rank)
        fn = lambda q_, k_, v_: ring_flash_attn_hip_(
            q_, k_, v_, causal=causal, ring_reduce_col=True,
            striped_ring_attn=striped, ring_size=world)[0]
        return _grads(fn, q[:, idx], k[:, idx], v[:, idx], do[:, idx])

    fused = loopback_world(world, run)
    monkeypatch.setenv("RING_ATTN_NO_FUSED_EPILOGUE", "1")
    plain = loopback_world(world, run)
    monkeypatch.delenv("RING_ATTN_NO_FUSED_EPILOGUE")
    monkeypatch.delenv("RING_ATTN_FORCE_STRATEGY")

    ref = _grads(_ring(causal), q, k, v, do)          # unsharded, one rank
    for rank in range(world):
        idx = shard(rank)
        if pin_single_pass:
            _assert_bitwise(fused[rank], plain[rank])
        for grads in (fused[rank], plain[rank]):
            for a, r, name in zip(grads, ref, ("dq", "dk", "dv")):
                r = r[:, idx].float()
                e = (a.float() - r).abs().max().item()
                assert e <= REL_TOL * r.abs().max().item(), f"rank {rank} {name} {e}"


# ---------------------------------------------------------------------------
# binding guards, other dtypes, lse gradient
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["split", "desc_dq", "desc_dkv", "accumulate"])
def test_binding_rejects_bf16_outputs_when_accumulating(mode):
    ext = _ext()
    q, k, v, do = _mk(1, 256, 256, 2, 2, 64, seed=7)
    b, n, h, d = q.shape
    lse = torch.zeros(b, h, n, device="cuda", dtype=torch.float32)
    delta = torch.zeros(b, h, n, device="cuda", dtype=torch.float32)
    desc = torch.tensor([[0, 0, 1]], dtype=torch.int32, device="cuda")
    accumulate = mode == "accumulate"
    split = 2 if mode == "split" else 1
    ddq = desc if mode == "desc_dq" else None
    ddkv = desc if mode == "desc_dkv" else None
    dq32 = torch.zeros(b, n, h, d, device="cuda", dtype=torch.float32)
    dk32 = torch.zeros(b, h, n, d, device="cuda", dtype=torch.float32)
    dv32 = torch.zeros(b, h, d, n, device="cuda", dtype=torch.float32)
    with pytest.raises(RuntimeError, match="single-pass"):
        ext.attn_bwd(q, k, v, do, None, lse, delta, dq32, dk32, dv32, d ** -0.5,
                     False, 0, 1, 0, False, False, 50.0, accumulate, split, 0,
                     ddq, ddkv, dq_bf=torch.empty_like(q),
                     dk_bf=torch.empty_like(k), dv_bf=torch.empty_like(v))


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_other_input_dtypes_keep_old_path(dtype):
    # bf16 values are exact in fp16 (normal range) and fp32, so the kernels
    # see the oracle's inputs
    (q, k, v, do), ref = _reference()
    grads = _grads(_ring(True), q.to(dtype), k.to(dtype), v.to(dtype), do)
    for g_ in grads:
        assert g_.dtype == dtype
    _assert_close_to_oracle(grads, ref)


def test_lse_gradient_not_materialised(monkeypatch):
    from ring_attention_amd.ops.ring_flash_hip import ring_flash_attn_hip_
    (q, k, v, do), ref = _reference()

    def run(use_lse):
        qg, kg, vg = (t.clone().requires_grad_(True) for t in (q, k, v))
        out, lse = ring_flash_attn_hip_(qg, kg, vg, causal=True)
        if use_lse == "only":
            lse.sum().backward()
        elif use_lse:
            torch.autograd.backward([out, lse], [do, torch.ones_like(lse)])
        else:
            out.backward(do)
        torch.cuda.synchronize()
        return qg.grad, kg.grad, vg.grad

    for key, val in SINGLE_PASS_ENV.items():     # deterministic fp32 values
        monkeypatch.setenv(key, val)
    base = run(False)
    _assert_close_to_oracle(base, ref)
    # lse's gradient is not propagated (unchanged behaviour): consuming lse
    # as well must neither crash nor change the gradients
    _assert_bitwise(run(True), base)
    for g_ in run("only"):
        assert g_ is not None and not g_.any()
