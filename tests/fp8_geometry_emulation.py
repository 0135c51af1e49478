"""CPU model of csrc/attn_fwd_fp8.hip under the mask geometry, and its checker.

`emulate_fp8_forward_masked` is tests/fp8_emulation.py's `emulate_fp8_forward`
with the mask of docs/KERNELS.md section 1 in place of the standard one:

    attend(i, j) <=> j < nk_true and (not causal or j <= qpos(i))
                     and (window is None or qpos(i) - j <= window)
    qpos(i) = i * q_stride + diag

It is built on the same `mfma_scores` and walks the keys in the same tiles of
FP8_KVBLK with the same arithmetic per tile.  The kernel visits only the tiles
of its workgroup's kv_tile_range; a tile outside it is masked whole for every
row of the workgroup, and a masked-whole tile changes nothing (max unchanged,
every exponential 0, rescale factor 2^0), so walking all tiles gives the same
numbers.  With diag 0, q_stride 1 and no window the result is `torch.equal`
to `emulate_fp8_forward` (test_fp8_geometry.py pins that).

Rows that attend no key are reported as `dead_rows` (b, h, nq).  The model
gives them out 0 and the kernel's finite lse floor; `masked_failures` demands
of the kernel: out exactly 0 there, lse finite and below -1e30, and every
other row within fp8_emulation's BOUND and LSE_TOL of the model.
"""

import torch

from ring_attention_amd.ops.fp8 import LSE_FLOOR

from .fp8_emulation import (LN2, LOG2E, M_FLOOR, P_SHIFT, _bf16r, _e4m3_rne,
                            _scale, fp8_failures, fp8_kvblk, mfma_scores)

DEAD_LSE_BELOW = -1e30      # a dead row's lse: finite and below this


def attend_matrix(nq, nk, nk_true, causal, diag=0, q_stride=1, window=None):
    """(nq, nk) bool, straight from the definition."""
    qpos = (torch.arange(nq) * q_stride + diag)[:, None]
    j = torch.arange(nk)[None, :]
    a = (j < nk_true).expand(nq, nk).clone()
    if causal:
        a &= j <= qpos
    if window is not None:
        a &= (qpos - j) <= window
    return a


def emulate_fp8_forward_masked(q8, k8, v8t, qs, ks, vs, sm_scale, causal=False,
                               nk_true=0, *, diag=0, q_stride=1, window=None,
                               kvblk=None, hw_dot=True):
    """Model of attn_fwd_fp8 with geometry on CPU uint8 operands (shapes as
    `emulate_fp8_forward`).  Returns out, out_bf16, lse, mag as that function
    does, plus dead_rows (b, h, nq) bool."""
    q8, k8, v8t, qs, ks, vs = (t.cpu() for t in (q8, k8, v8t, qs, ks, vs))
    b, nq, h, d = q8.shape
    nk, hk = k8.shape[1], k8.shape[2]
    nd = d // 64
    if nk_true <= 0:
        nk_true = nk
    if kvblk is None:
        kvblk = fp8_kvblk()
    assert nk % kvblk == 0 and kvblk % 64 == 0
    qs, ks = qs.reshape(b, nq, h, nd), ks.reshape(b, nk, hk, nd)

    acc = torch.float64
    f8 = lambda x: x.view(torch.float8_e4m3fn).double()
    vd = f8(v8t) * _scale(vs).repeat_interleave(64, dim=-1)      # (b, hk, d, nk)
    heads = torch.arange(h) % hk
    vd = vd[:, heads].to(acc)

    s = mfma_scores(q8, k8[:, :, heads], qs, ks[:, :, heads], hw_dot)
    s = s.to(acc) * (sm_scale * LOG2E)
    attend = attend_matrix(nq, nk, nk_true, causal, diag, q_stride, window)
    s = s.masked_fill(~attend[None, None], float("-inf"))
    dead_rows = (~attend.any(-1))[None, None].expand(b, h, nq)

    m = torch.full((b, h, nq), float("-inf"), dtype=acc)
    l = torch.zeros(b, h, nq, dtype=acc)
    o = torch.zeros(b, h, nq, d, dtype=acc)
    omag = torch.zeros_like(o)
    for t in range(nk // kvblk):
        st = s[..., t * kvblk:(t + 1) * kvblk]
        vt = vd[..., t * kvblk:(t + 1) * kvblk]                   # (b, h, d, kvblk)
        m_new = torch.maximum(m, st.amax(dim=-1))
        e = torch.exp2((st - m_new.clamp(min=M_FLOOR)[..., None]).float())
        p = _e4m3_rne(e * P_SHIFT) / P_SHIFT
        alpha = torch.exp2(m.clamp(min=M_FLOOR) - m_new.clamp(min=M_FLOOR))
        l = l * alpha + e.to(acc).sum(-1)
        pa = p.to(acc)
        o = o * alpha[..., None] + torch.einsum("bhij,bhdj->bhid", pa, vt)
        omag = omag * alpha[..., None] + torch.einsum("bhij,bhdj->bhid", pa, vt.abs())
        m = m_new

    l_safe = l.clamp(min=1e-38)
    out = (o / l_safe[..., None]).permute(0, 2, 1, 3).contiguous().float()
    mag = (omag / l_safe[..., None]).permute(0, 2, 1, 3).contiguous().float()
    lse = (l_safe.log() + m * LN2).float()
    lse = torch.where(dead_rows, torch.full_like(lse, LSE_FLOOR), lse)
    return dict(out=out, out_bf16=_bf16r(out), lse=lse, mag=mag,
                dead_rows=dead_rows.clone())


def masked_failures(out, lse, model):
    """Failure strings (empty = accepted) and figures for a result judged
    against the masked model: dead rows exact, live rows by `fp8_failures`
    at the project's BOUND / LSE_TOL."""
    out, lse = out.detach().float().cpu(), lse.detach().float().cpu()
    dead = model["dead_rows"]                                   # (b, h, nq)
    assert out.shape == model["out"].shape and lse.shape == dead.shape
    bad = []
    o_rows = out.permute(0, 2, 1, 3)                            # (b, h, nq, d)
    n_dead = int(dead.sum())
    if n_dead:
        if not (o_rows[dead] == 0).all():
            bad.append(f"dead rows: {int((o_rows[dead] != 0).sum())} non-zero outputs")
        dl = lse[dead]
        if not (torch.isfinite(dl).all() and (dl < DEAD_LSE_BELOW).all()):
            bad.append(f"dead rows: lse not finite and below {DEAD_LSE_BELOW:g} "
                       f"(max {dl.max().item():g}, min {dl.min().item():g})")
    live = ~dead
    sub = dict(out=model["out"].permute(0, 2, 1, 3)[live],
               mag=model["mag"].permute(0, 2, 1, 3)[live], lse=model["lse"][live])
    if not (torch.isfinite(o_rows[live]).all() and torch.isfinite(lse[live]).all()):
        return bad + ["live rows: non-finite value"], dict(
            ratio=float("inf"), lse=float("inf"), nonzero_at_zero_mag=0, dead=n_dead)
    more, f = fp8_failures(o_rows[live], lse[live], sub)
    f["dead"] = n_dead
    return bad + more, f
