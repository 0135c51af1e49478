"""MX-FP8 serving forward — an MI355X-only capability beyond the reference.

The reference's kernels are bf16/fp16 Triton
(/root/reference/ring_attention_pytorch/triton_flash_attn.py); gfx950 adds
block-scaled e4m3 MFMA at ~2x the bf16 matrix rate, which this module
exposes as a quantize + fused-forward pair for inference/prefill:

    out, lse = flash_attn_fp8(q, k, v)          # (b, n, h, d) bf16 in/out

Numerics: Q/K use one e8m0 scale per row (2^ceil(log2(amax/448))), V one
per (d row, 64-kv chunk), and the softmax matrix P needs no scale at all
(exp2(x - m) <= 1).  Softmax and the output accumulator stay fp32 inside
the kernel; only the MFMA operands are 8-bit.  Measured error vs an fp32
reference: ~5% mean-relative on out, lse within 0.03 on long rows; P's
e4m3 rounding alone moves out by 2.4% mean-relative (CPU model of the
kernel vs `_eager_fp8` on the same bytes, 1 x 512 x 2 x 64 randn); use the
bf16 path when training.  Against that model (tests/fp8_emulation.py: the
kernel's tile order, P rounding and the scaled MFMA's product alignment) the
kernel agrees on every element to 0.0041 of sum(P |V|) — bf16 rounding —
and to 7.6e-6 in lse (MI355X, tests/test_fp8_emulation.py).

Causal (``causal=True``) uses the bf16 kernels' mirrored paired-tile
load balance; GQA follows the framework-wide ``qh % hk`` pairing.

Mask: the bf16 kernels' geometry (docs/KERNELS.md section 1),

    attend(i, j) <=> j < nk_true and (not causal or j <= qpos(i))
                     and (window is None or qpos(i) - j <= window),
    qpos(i) = i * q_stride + diag,

so a ring hop of any layout (rank-ordered, striped, with lookback) is one
launch.  A row that attends no key returns out == 0 and lse == LSE_FLOOR,
a finite stand-in for log(0) that `merge_fp8_partials` combines without NaN.

Scope: forward only (use the bf16 path for training); no bias/key-pad
mask/softclamp; any head dim <= 128 (native 64/128 + exact zero-pad).
Ragged lengths are handled by padding the quantized buffers (zero bytes —
a valid e4m3, never NaN) while the kernel masks at the true kv length.
"""

from __future__ import annotations

import math

import torch
from torch import Tensor

from . import hip_ext

# lse of a row that attends no key, as the kernel's epilogue forms it:
# log(max(l, 1e-38)) + m * ln 2 with l = 0 and m = MASK_VALUE_F (-FLT_MAX)
LSE_FLOOR = math.log(1e-38) + -3.4028234663852886e38 * 0.6931471805599453


def _e8m0(amax: Tensor) -> tuple[Tensor, Tensor]:
    """amax (positive fp32) -> (e8m0 byte = exp+127, scale = 2^exp)."""
    e = torch.ceil(torch.log2(amax.clamp(min=2.0 ** -126) / 448.0))
    e = e.clamp(-127.0, 127.0)
    return (e + 127.0).to(torch.uint8), torch.exp2(e)


def _pad_dim(x: Tensor, dim: int, mult: int) -> Tensor:
    n = x.shape[dim]
    pad = (-n) % mult
    if pad == 0:
        return x.contiguous()
    shape = list(x.shape)
    shape[dim] = pad
    return torch.cat((x, x.new_zeros(shape)), dim=dim).contiguous()


def quantize_fp8(q: Tensor, k: Tensor, v: Tensor):
    """Quantize (b, n, h, d) q/k/v for attn_fwd_fp8.

    Returns (q8, k8, v8t, qs, ks, vs) uint8 views, PADDED to the kernel's
    tile alignment (q rows to 256, kv rows to 128) with zero bytes and
    scale 2^-127 — zero is a valid e4m3 (never NaN), and the kernel masks
    scores at the true kv length (nk_true):
      q8/k8 (b, nq_pad, h, d) e4m3; v8t (b, hk, d, nk_pad) e4m3;
      qs/ks (b, n_pad, h, d // 64) e8m0; vs (b, hk, d, nk_pad // 64) e8m0.
    """
    qf, kf = q.float(), k.float()
    d = q.shape[-1]
    assert d % 64 == 0
    nd = d // 64
    # per (row, 64-d chunk) scales: shape (..., nd)
    qs_b, qs_s = _e8m0(qf.view(*qf.shape[:-1], nd, 64).abs().amax(dim=-1))
    ks_b, ks_s = _e8m0(kf.view(*kf.shape[:-1], nd, 64).abs().amax(dim=-1))
    q8 = (qf / qs_s.repeat_interleave(64, dim=-1)).to(torch.float8_e4m3fn)
    k8 = (kf / ks_s.repeat_interleave(64, dim=-1)).to(torch.float8_e4m3fn)

    vt = v.permute(0, 2, 3, 1).float().contiguous()      # (b, hk, d, n)
    b, hk, dv, n = vt.shape
    n64 = n + ((-n) % 64)
    vt = _pad_dim(vt, 3, 128)
    vs_b, vs_s = _e8m0(vt[..., :n64].view(b, hk, dv, n64 // 64, 64)
                       .abs().amax(dim=-1))
    vs_b = _pad_dim(vs_b, 3, 2)          # to nk_pad // 64
    vs_s = _pad_dim(vs_s, 3, 2).clamp(min=2.0 ** -127)
    v8t = (vt / vs_s.repeat_interleave(64, dim=-1)).to(torch.float8_e4m3fn)
    return (_pad_dim(q8.view(torch.uint8), 1, 256),
            _pad_dim(k8.view(torch.uint8), 1, 128),
            v8t.view(torch.uint8).contiguous(),
            _pad_dim(qs_b, 1, 256), _pad_dim(ks_b, 1, 128),
            vs_b.contiguous())


@torch.no_grad()
def flash_attn_fp8(
    q: Tensor, k: Tensor, v: Tensor,
    sm_scale: float | None = None,
    causal: bool = False,
    window: int | None = None,
    causal_mask_diagonal: bool = False,
) -> tuple[Tensor, Tensor]:
    """MX-FP8 attention forward on (b, n, h, d) tensors.

    Returns (out bf16 (b, n, h, d), lse fp32 (b, h, n)).  Quantizes
    internally; pass pre-quantized operands via flash_attn_fp8_quantized
    to amortize quantization across decode steps.  `window` keeps keys with
    i - j <= window; `causal_mask_diagonal` masks the diagonal too (j < i),
    both as in `flash_attn`.
    """
    d = q.shape[-1]
    sm = sm_scale if sm_scale is not None else d ** -0.5
    if d % 64 != 0:
        # exact zero-pad to the next kernel dim ({64, 128}, like the bf16
        # path's _pad_head_dim): padded q/k dims contribute 0 to scores,
        # padded v dims are sliced off below
        kd = 64 if d < 64 else 128
        assert d <= 128, "fp8 path: head dim <= 128"
        import torch.nn.functional as F
        q = F.pad(q, (0, kd - d))
        k = F.pad(k, (0, kd - d))
        v = F.pad(v, (0, kd - d))
    q8, k8, v8t, qs, ks, vs = quantize_fp8(q, k, v)
    out, lse = flash_attn_fp8_quantized(
        q8, k8, v8t, qs, ks, vs, sm,
        causal=causal, nk_true=k.shape[1],
        diag=-1 if (causal and causal_mask_diagonal) else 0, window=window)
    nq = q.shape[1]
    return out[:, :nq, :, :d], lse[..., :nq]


def flash_attn_fp8_quantized(q8, k8, v8t, qs, ks, vs, sm_scale: float,
                             causal: bool = False, nk_true: int = 0,
                             diag: int = 0, q_stride: int = 1,
                             window: int | None = None):
    """The fused forward on quantize_fp8's operands, masked by the module
    docstring's geometry (the defaults are the standard mask)."""
    if q8.is_cuda:
        out, lse = hip_ext.require().attn_fwd_fp8(
            q8, k8, v8t, qs, ks, vs, sm_scale, causal, nk_true,
            diag=diag, q_stride=q_stride, has_win=window is not None,
            win=window if window is not None else 0)
        return out, lse
    return _eager_fp8(q8, k8, v8t, qs, ks, vs, sm_scale, causal, nk_true,
                      diag, q_stride, window)


def _dequant(x8: Tensor, scales: Tensor) -> Tensor:
    return (x8.view(torch.float8_e4m3fn).float()
            * torch.exp2(scales.float() - 127.0).repeat_interleave(64, dim=-1))


def _eager_fp8(q8, k8, v8t, qs, ks, vs, sm_scale, causal, nk_true,
               diag=0, q_stride=1, window=None):
    """CPU fallback: dequantized eager attention with the kernel's masking
    semantics (true length, causal at qpos(i) = i * q_stride + diag, window;
    rows with no key: out 0, lse LSE_FLOOR).  Approximates the GPU path to within
    its P-quantization error (the fallback keeps P in fp32) — it exists so
    the fp8 wrapper/ring logic runs and tests anywhere, like the rest of
    the framework's CPU fallbacks."""
    b, nq, h, d = q8.shape
    hk, nk = k8.shape[2], k8.shape[1]
    if nk_true <= 0:
        nk_true = nk
    qd = _dequant(q8, qs)                                  # (b, nq, h, d)
    kd = _dequant(k8, ks)                                  # (b, nk, hk, d)
    # v8t (b, hk, d, nk), vs (b, hk, d, nk//64): dequant along the last dim
    vd = (v8t.view(torch.float8_e4m3fn).float()
          * torch.exp2(vs.float() - 127.0).repeat_interleave(64, dim=-1))
    vd = vd.permute(0, 3, 1, 2)                            # (b, nk, hk, d)
    groups = h // hk
    if groups > 1:
        kd = kd.repeat(1, 1, groups, 1)                    # qh pairs qh % hk
        vd = vd.repeat(1, 1, groups, 1)
    sim = torch.einsum("bihd,bjhd->bhij", qd, kd) * sm_scale
    jpos = torch.arange(nk, device=sim.device)
    sim = sim.masked_fill((jpos >= nk_true)[None, None, None, :], float("-inf"))
    qpos = torch.arange(nq, device=sim.device) * q_stride + diag
    if causal:
        sim = sim.masked_fill((jpos[None, :] > qpos[:, None])[None, None],
                              float("-inf"))
    if window is not None:
        sim = sim.masked_fill(((qpos[:, None] - jpos[None, :]) > window)[None, None],
                              float("-inf"))
    lse = sim.logsumexp(dim=-1).clamp(min=LSE_FLOOR)       # (b, h, nq)
    out = torch.einsum("bhij,bjhd->bihd", torch.softmax(sim, dim=-1), vd)
    out = torch.nan_to_num(out)                            # all-masked rows
    return out.to(torch.bfloat16), lse.float()


def merge_fp8_partials(out: Tensor, lse: Tensor, o_h: Tensor, l_h: Tensor):
    """Fold one hop's partial (o_h (b, n, h, d), l_h (b, h, n)) into the
    running (out fp32, lse fp32): the exact online-softmax combine of two
    attentions over disjoint key sets, in fp32."""
    m = torch.maximum(lse, l_h)
    wa = (lse - m).exp()                              # (b, h, n)
    wb = (l_h - m).exp()
    den = wa + wb
    wa4 = (wa / den).permute(0, 2, 1).unsqueeze(-1)   # (b, n, h, 1)
    wb4 = (wb / den).permute(0, 2, 1).unsqueeze(-1)
    return out.float() * wa4 + o_h.float() * wb4, m + den.log()


@torch.no_grad()
def ring_flash_attn_fp8(
    q: Tensor, k: Tensor, v: Tensor,
    sm_scale: float | None = None,
    ring_size: int | None = None,
    causal: bool = False,
    striped: bool = False,
    max_lookback_seq_len: int | None = None,
) -> tuple[Tensor, Tensor]:
    """RING attention forward in MX-FP8 over sharded KV.

    Each rank quantizes its LOCAL (b, n_shard, hk, d) k/v once; the 8-bit
    shards then rotate the ring — half the bf16 wire bytes per hop (xGMI
    ring hops are single-link bound, so the fp8 wire format directly halves
    the transport time too) — and every hop's fused-fp8 partial merges by
    logsumexp (exact online-softmax combine in fp32).

    Causal: every hop takes its mask from `_hop_geometry`, the bf16 ring's
    own (q rank, kv rank) -> (skip, diag, win) rule, with n_shard the TRUE
    shard length.  Rank-ordered shards (rank r owns global rows
    [r*n_shard, (r+1)*n_shard)) skip hops from later ranks, cut the own hop
    at the diagonal and run earlier ones full.  `striped=True` (rank r owns
    rows r, r + R, ...; requires causal) makes every hop a triangle with
    diag 0 (source <= self) or -1, so every rank does the same work.
    `max_lookback_seq_len` adds the sliding window in global positions and
    skips hops beyond it.  A skipped hop launches nothing; rows a hop masks
    whole merge as out 0 / lse LSE_FLOOR.  Zig-zag stays on the bf16 path.

    Returns (out bf16 (b, n, h, d), lse fp32 (b, h, n)).
    """
    from ..parallel import RingTopology, all_ring_pass, is_distributed
    from ..parallel.ring_pass import null_ring_pass
    from .ring_flash_hip import _hop_geometry

    assert causal or not striped, "striped ring attention requires causal"
    lookback = max_lookback_seq_len
    assert causal or lookback is None, "lookback (sliding window) requires causal"
    sm = sm_scale if sm_scale is not None else q.shape[-1] ** -0.5
    n_shard = k.shape[1]
    q8, k8, v8t, qs, ks, vs = quantize_fp8(q, k, v)

    my_rank, ring = 0, 1
    if is_distributed():
        topo = RingTopology(ring_size)
        my_rank, ring = topo.ring_rank, topo.ring_size
        hops = all_ring_pass(topo, k8, v8t, ks, vs)
    else:
        hops = null_ring_pass(k8, v8t, ks, vs)

    out = lse = None
    for info, (k8h, v8th, ksh, vsh) in hops:
        skip, diag, win = _hop_geometry(my_rank, info.source_ring_rank, n_shard,
                                        ring, striped, causal, lookback)
        if skip:
            continue                   # future rows, or beyond the window
        o_h, l_h = flash_attn_fp8_quantized(
            q8, k8h, v8th, qs, ksh, vsh, sm, causal=causal, nk_true=n_shard,
            diag=diag, window=win if lookback is not None else None)
        if out is None:
            out, lse = o_h.float(), l_h
        else:
            out, lse = merge_fp8_partials(out, lse, o_h, l_h)
    assert out is not None, "every hop masked: degenerate configuration"
    nq = q.shape[1]
    return out[:, :nq].to(q.dtype), lse[..., :nq]


def quantize_kv_cache(k: Tensor, v: Tensor):
    """Quantize a decode KV cache (b, hk, n, d) to e4m3 + per-row e8m0.

    Returns (k8, v8, ks, vs) uint8: k8/v8 (b, hk, n, d), ks/vs (b, hk, n).
    Halves the decode kernel's HBM stream (decode is bandwidth-bound); the
    scales fold into the score / softmax weight, so the decode math is the
    same fp32 online softmax.  Quantize once at cache-write time.
    """
    kf, vf = k.float(), v.float()
    ks_b, ks_s = _e8m0(kf.abs().amax(dim=-1))
    vs_b, vs_s = _e8m0(vf.abs().amax(dim=-1))
    k8 = (kf / ks_s.unsqueeze(-1)).to(torch.float8_e4m3fn)
    v8 = (vf / vs_s.unsqueeze(-1)).to(torch.float8_e4m3fn)
    return (k8.view(torch.uint8), v8.view(torch.uint8),
            ks_b.contiguous(), vs_b.contiguous())
