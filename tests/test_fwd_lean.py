"""The lean forward instantiations (no ticks / ablate / key-pad mask / bias in
the body) against the fp32 reference, and against the full-featured kernel.

ext.attn_fwd is called directly: the launcher picks the lean kernel whenever
none of the four cold features is passed.  Shapes are the smallest that run
the 3-deep staging pipeline (>= 3 kv tiles at every head dim), a ragged last
kv tile and a partial q tile: nq = nk = 300 (kv tile 128 at d64, 64 else; q
tile 256).  Every feature runs at d 32, 64 and 128: at d32 the workgroup has
more threads than a tile has staging chunks, so the staging guards matter.  Tolerances are those of tests/test_gpu_kernels.py for the same
feature: out 2e-2, lse 2e-3.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

OUT_TOL, LSE_TOL = 2e-2, 2e-3
N = 300


def _mk(b, n, h, hk, d, seed):
    torch.manual_seed(seed)
    q = torch.randn(b, n, h, d, device="cuda", dtype=torch.bfloat16)
    k = torch.randn(b, n, hk, d, device="cuda", dtype=torch.bfloat16)
    v = torch.randn(b, n, hk, d, device="cuda", dtype=torch.bfloat16)
    return q, k, v


def _reference(q, k, v, causal, softclamp=None):
    """fp32 attention on the bf16 inputs -> out (B,N,H,D), lse (B,H,N).
    GQA pairs q head qh with kv head qh % hk."""
    q, k, v = q.float(), k.float(), v.float()
    b, n, h, d = q.shape
    g = h // k.shape[2]
    k, v = k.repeat(1, 1, g, 1), v.repeat(1, 1, g, 1)
    outs, lses = [], []
    for bi in range(b):                       # per batch: bounds the score tensor
        sim = torch.einsum("ihd,jhd->hij", q[bi], k[bi]) * d ** -0.5
        if softclamp is not None:
            sim = (sim / softclamp).tanh() * softclamp
        if causal:
            pos = torch.arange(n, device=q.device)
            sim = sim.masked_fill(pos[None, :] > pos[:, None], torch.finfo(torch.float32).min)
        lses.append(sim.logsumexp(-1))
        outs.append(torch.einsum("hij,jhd->ihd", sim.softmax(-1), v[bi]))
    return torch.stack(outs), torch.stack(lses)


def _ext():
    from ring_attention_amd.ops import hip_ext
    return hip_ext.require()


def _fwd(q, k, v, causal, *, softclamp=None, ticks=None, diag=0):
    """One single-pass launch -> (out, lse)."""
    b, n, h, d = q.shape
    out = torch.empty_like(q)
    lse = torch.empty(b, h, n, device="cuda", dtype=torch.float32)
    _ext().attn_fwd(q, k, v, None, None, None, None, out, lse, d ** -0.5,
                    causal, diag, 1, 0, False, softclamp is not None,
                    softclamp if softclamp is not None else 50.0,
                    True, True, 1, 0, ticks)
    return out, lse


def _check(out, lse, ref, ref_lse, what):
    err = (out.float() - ref).abs().max().item()
    lse_err = (lse - ref_lse).abs().max().item()
    print(f"{what}: out err {err:.3e} lse err {lse_err:.3e}")
    assert err < OUT_TOL, f"{what}: out err {err}"
    assert lse_err < LSE_TOL, f"{what}: lse err {lse_err}"


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("d", [32, 64, 128])
def test_lean_base(d, causal):
    q, k, v = _mk(1, N, 2, 2, d, seed=d)
    out, lse = _fwd(q, k, v, causal)
    _check(out, lse, *_reference(q, k, v, causal), f"d{d} causal={causal}")


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("d", [32, 64, 128])
def test_lean_gqa(d, causal):
    q, k, v = _mk(1, N, 4, 2, d, seed=100 + d)
    out, lse = _fwd(q, k, v, causal)
    _check(out, lse, *_reference(q, k, v, causal), f"gqa d{d} causal={causal}")


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("d", [32, 64, 128])
def test_lean_softclamp(d, causal):
    q, k, v = _mk(1, N, 2, 2, d, seed=200 + d)
    out, lse = _fwd(q, k, v, causal, softclamp=5.0)
    _check(out, lse, *_reference(q, k, v, causal, softclamp=5.0),
           f"softclamp d{d} causal={causal}")


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("d", [32, 64, 128])
def test_lean_resume_two_hops(d, causal):
    """is_first over the first half of the keys, is_last over the second."""
    ext = _ext()
    b, h = 1, 2
    q, k, v = _mk(b, N, h, h, d, seed=300 + d)
    half = N // 2
    out = torch.empty_like(q)
    lse = torch.empty(b, h, N, device="cuda", dtype=torch.float32)
    o_acc = torch.empty(b, h, d, N, device="cuda", dtype=torch.float32)
    m = torch.empty(b, h, N, device="cuda", dtype=torch.float32)
    l = torch.empty(b, h, N, device="cuda", dtype=torch.float32)
    for hop, sl in enumerate((slice(0, half), slice(half, N))):
        # causal in kv-local coordinates: j_local <= i - start
        ext.attn_fwd(q, k[:, sl].contiguous(), v[:, sl].contiguous(), None, o_acc, m, l,
                     out, lse, d ** -0.5, causal, -sl.start, 1, 0, False, False, 50.0,
                     hop == 0, hop == 1, 1, 0, None)
    _check(out, lse, *_reference(q, k, v, causal), f"resume d{d} causal={causal}")


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("d", [32, 64, 128])
def test_lean_kv_split_merge(d, causal):
    ext = _ext()
    b, h, S = 1, 2, 2
    q, k, v = _mk(b, N, h, h, d, seed=400 + d)
    out = torch.empty_like(q)
    lse = torch.empty(b, h, N, device="cuda", dtype=torch.float32)
    o_p = torch.empty(S, b, h, d, N, device="cuda", dtype=torch.float32)
    m_p = torch.empty(S, b, h, N, device="cuda", dtype=torch.float32)
    l_p = torch.empty(S, b, h, N, device="cuda", dtype=torch.float32)
    ext.attn_fwd(q, k, v, None, o_p, m_p, l_p, None, None, d ** -0.5,
                 causal, 0, 1, 0, False, False, 50.0, True, True, S, 0, None)
    ext.attn_fwd_merge(o_p, m_p, l_p, None, None, None, out, lse, S, b, h, d, N, True, True)
    _check(out, lse, *_reference(q, k, v, causal), f"kv_split d{d} causal={causal}")


def test_lean_paired_odd_tile_count():
    """T = 3 q tiles and ((T+1)/2) * b * h = 256 workgroups: the binding
    engages causal pairing, and the middle tile is its own partner."""
    q, k, v = _mk(2, 768, 64, 64, 64, seed=500)
    out, lse = _fwd(q, k, v, True)
    _check(out, lse, *_reference(q, k, v, True), "paired T=3")


@pytest.mark.parametrize("softclamp", [None, 5.0])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("d", [32, 64, 128])
def test_lean_equals_full_featured(d, causal, softclamp):
    """A ticks tensor selects the full-featured kernel (and rules pairing
    out); its arithmetic is the lean kernel's, so the results are the same
    bits.  (An all-ones key mask or a zero bias would NOT do: those take the
    masked-tile arithmetic, mul then sub instead of one fma.)"""
    q, k, v = _mk(1, N, 2, 2, d, seed=600 + d)
    out, lse = _fwd(q, k, v, causal, softclamp=softclamp)
    ticks = torch.zeros(64 * 6, device="cuda", dtype=torch.int64)
    out_f, lse_f = _fwd(q, k, v, causal, softclamp=softclamp, ticks=ticks)
    assert torch.equal(out, out_f)
    assert torch.equal(lse, lse_f)
    # workgroup (0, 0, 0) stamped its tiles: causal rows 0..255 reach keys
    # 0..255, otherwise all 300
    tiles = -(-(256 if causal else N) // (128 if d == 64 else 64))
    t = ticks[: tiles * 6].cpu()
    assert (t > 0).all(), "missing stamps"
    assert (t[1:] >= t[:-1]).all(), "stamps decrease"
    assert (ticks[tiles * 6:] == 0).all()
