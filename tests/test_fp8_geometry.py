"""The MX-FP8 forward under the mask geometry (diag, q_stride, window).

Two oracles, as for the standard mask:

  * the COUNTING PROBE of tests/test_mask_exactness.py (q = 0, v one-hot:
    every value exact in e4m3, exp(lse) is the number of attended keys) sees
    a single key too many or too few.  It judges `_eager_fp8`, the masked CPU
    model and the kernel, and the CPU tests show it rejecting the model with
    diag +- 1, win +- 1 and q_stride ignored: the defects a geometry change
    can introduce;
  * the masked model of tests/fp8_geometry_emulation.py on `gains` inputs
    judges the kernel's arithmetic under the mask (tile walk starting at
    lo > 0, masked tiles, rows without keys) at fp8_emulation's BOUND and
    LSE_TOL; rows without a key must be exactly 0 with a finite lse floor.

GPU figures (MI355X, worst over the GPU cases of this file; each case prints
its own):
  counting probe   err / mag 0.0039 (bf16 rounding), |exp(lse) - count| 0.00073
                   (768 x 768 at diag -1; 0.00038 over the GEOMS cases)
  masked model     err / mag 0.00394 (256 x 256 diag 0, d 128; every case lies
                   between 0.0038 and 0.0040), lse difference 7.6e-6 (256 x
                   1024 diag 700 window 300, d 128; 3.8e-6 elsewhere); the
                   100 rows per head without a key of the diag -100 case are
                   exactly 0 with lse at the floor
"""

import functools

import pytest
import torch

from ring_attention_amd.ops.fp8 import (LSE_FLOOR, _eager_fp8,
                                        flash_attn_fp8_quantized,
                                        merge_fp8_partials, quantize_fp8)

from .fp8_emulation import build_inputs, emulate_fp8_forward, fp8_kvblk
from .fp8_geometry_emulation import (attend_matrix, emulate_fp8_forward_masked,
                                     masked_failures)
from .test_mask_exactness import (GEOMS, WINS, _assert_probe, _attend, _ext,
                                  _print_worst, _probe_failures, _probe_slice,
                                  _ref_cached)

FP8_WINS = [None, 0, 1, 127, 128, 129]
assert set(FP8_WINS) <= set(WINS)

_worst = {"gpu_out": 0.0, "gpu_lse": 0.0}


def _geo_id(g):
    return "x".join(map(str, g))


def _probe_operands(nq, nk, d, h, hk, device="cpu"):
    """quantize_fp8 of the probe: q = 0 (every score exactly 0 whatever k
    holds), k randn, v one-hot; (1, n, heads, d)."""
    _, _, v, _ = _probe_slice(nq, nk, d)
    g = torch.Generator().manual_seed(11)
    q = torch.zeros(1, nq, h, d, dtype=torch.bfloat16, device=device)
    k = torch.randn(1, nk, hk, d, generator=g).to(torch.bfloat16).to(device)
    v = v[None, :, None, :].expand(1, nk, hk, d).to(torch.bfloat16).contiguous().to(device)
    return quantize_fp8(q, k, v)


@functools.lru_cache(maxsize=None)
def _cpu_probe_operands(nq, nk, d, h, hk):
    return _probe_operands(nq, nk, d, h, hk)


def _got(out, lse, nq):
    """(b, h, n, d) / (b, h, n) views of a padded result, cut to nq rows."""
    return dict(lse=lse[..., :nq], out=out[:, :nq].permute(0, 2, 1, 3))


# ---------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("d", [64, 128])
def test_masked_model_is_the_model_at_the_standard_mask(d, causal):
    q, k, v = build_inputs("gains", 1, 256, 256, 4, 2, d, kvblk=fp8_kvblk())
    ops = quantize_fp8(q, k, v)
    ref = emulate_fp8_forward(*ops, d ** -0.5, causal, 256)
    got = emulate_fp8_forward_masked(*ops, d ** -0.5, causal, 256,
                                     diag=0, q_stride=1, window=None)
    for name in ("out", "lse", "mag"):
        assert torch.equal(got[name], ref[name]), name
    assert not got["dead_rows"].any()


@pytest.mark.parametrize("geo", GEOMS, ids=_geo_id)
def test_probe_accepts_masked_model_rejects_shifted_geometry(geo):
    """The counting probe accepts the masked model at the true geometry and
    rejects it with diag +- 1, win +- 1 and q_stride ignored."""
    nq, nk, diag, qs = geo
    d = 64
    ops = _cpu_probe_operands(nq, nk, d, 1, 1)
    n_rejected = 0
    for win in (None, 1, 128):
        ref = _ref_cached(nq, nk, diag, qs, True, win, d)
        true = _attend(nq, nk, diag, qs, True, win)

        def model(diag_, qs_, win_):
            m = emulate_fp8_forward_masked(*ops, d ** -0.5, True, nk, diag=diag_,
                                           q_stride=qs_, window=win_)
            return _got(m["out_bf16"], m["lse"], nq)

        fails = _probe_failures(model(diag, qs, win), ref, tag=f"{geo} win{win}",
                                family="fp8 model")
        assert not fails, "\n".join(fails[:8])
        shifted = [("diag+1", diag + 1, qs, win), ("diag-1", diag - 1, qs, win)]
        if win is not None:
            shifted += [("win+1", diag, qs, win + 1), ("win-1", diag, qs, win - 1)]
        if qs != 1:
            shifted.append(("q_stride ignored", diag, 1, win))
        for lab, diag_, qs_, win_ in shifted:
            assert not torch.equal(_attend(nq, nk, diag_, qs_, True, win_), true), lab
            assert _probe_failures(model(diag_, qs_, win_), ref, track=False,
                                   quiet=True), f"{geo} win{win}: '{lab}' accepted"
            n_rejected += 1
    assert n_rejected >= 10


@pytest.mark.parametrize("geo", GEOMS, ids=_geo_id)
def test_eager_fallback_geometry_on_the_probe(geo):
    nq, nk, diag, qs = geo
    d, h, hk = 64, 2, 1
    ops = _cpu_probe_operands(nq, nk, d, h, hk)
    for win in FP8_WINS:
        ref = _ref_cached(nq, nk, diag, qs, True, win, d)
        out, lse = _eager_fp8(*ops, d ** -0.5, True, nk, diag, qs, win)
        assert torch.isfinite(lse).all()
        dead = ref["count"] == 0
        assert (lse[0, :, :nq][:, dead] == LSE_FLOOR).all()
        _assert_probe(_got(out, lse, nq), ref, tag=f"eager {geo} win{win}",
                      family="fp8 eager")


@pytest.mark.parametrize("geo", GEOMS, ids=_geo_id)
def test_row_cut_against_brute_force(geo):
    """Mask::row_cut (csrc/attn_mask.h), the kernel's per-row offset range of
    a tile, is the definition's row restricted to the tile."""
    nq, nk, diag, qs = geo
    W = fp8_kvblk()
    for causal, win in [(True, w) for w in FP8_WINS + [200]] + [(False, None), (False, 64)]:
        m = _ext().Mask(causal, diag, qs, win is not None, 0 if win is None else win)
        att = attend_matrix(nq, -(-nk // W) * W, nk, causal, diag, qs, win)
        for t in range(att.shape[1] // W):
            cuts = [m.row_cut(m.qpos(i), t * W, W, nk) for i in range(nq)]
            assert all(0 <= lo <= W and -1 <= hi <= W - 1 for lo, hi in cuts)
            lo, hi = torch.tensor(cuts).T[:, :, None]
            o = torch.arange(W)[None, :]
            assert torch.equal(att[:, t * W:(t + 1) * W], (lo <= o) & (o <= hi)), \
                (causal, win, t)


def test_merge_of_two_floor_rows_stays_at_the_floor():
    out = torch.zeros(1, 4, 2, 8)
    lse = torch.full((1, 2, 4), LSE_FLOOR)
    lse[0, 0, 1] = 0.5                                  # one live row
    o2, l2 = merge_fp8_partials(out, lse, torch.zeros(1, 4, 2, 8).bfloat16(),
                                torch.full((1, 2, 4), LSE_FLOOR))
    assert torch.isfinite(o2).all() and torch.isfinite(l2).all()
    assert (o2 == 0).all()
    floor = lse != 0.5
    assert (l2[floor] < -1e30).all() and l2[0, 0, 1] == 0.5


@pytest.mark.parametrize("world", [2, 4, 8])
def test_hop_geometry_is_the_old_fp8_ring_rule(world):
    """striped=False, no lookback: a hop from a later rank is skipped, the own
    hop is the causal triangle, a hop from an earlier rank is full."""
    from ring_attention_amd.ops.ring_flash_hip import _hop_geometry
    n = 256
    tril = torch.ones(n, n, dtype=torch.bool).tril()
    for rq in range(world):
        for rk in range(world):
            skip, diag, win = _hop_geometry(rq, rk, n, world, False, True, None)
            assert skip == (rk > rq), (rq, rk)
            if skip:
                continue
            att = attend_matrix(n, n, n, True, diag, 1, None)
            assert torch.equal(att, tril) if rk == rq else att.all(), (rq, rk)
            assert (diag >= n - 1) == (rk < rq)         # the launcher's full-hop rule
            skip, _, _ = _hop_geometry(rq, rk, n, world, False, False, None)
            assert not skip


# ---------------------------------------------------------------------------
# GPU: counting probe
# ---------------------------------------------------------------------------
def _gpu_probe(ops, nq, nk, d, diag, qs, win, tag):
    ref = _ref_cached(nq, nk, diag, qs, True, win, d)
    out, lse = flash_attn_fp8_quantized(*ops, d ** -0.5, causal=True, nk_true=nk,
                                        diag=diag, q_stride=qs, window=win)
    torch.cuda.synchronize()
    _assert_probe(_got(out, lse, nq), ref, tag=tag, family="fwd_fp8")


@pytest.mark.gpu
@pytest.mark.parametrize("h,hk", [(2, 2), (4, 2)])
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("geo", GEOMS, ids=_geo_id)
def test_gpu_probe_geometries(geo, d, h, hk):
    nq, nk, diag, qs = geo
    ops = _probe_operands(nq, nk, d, h, hk, "cuda")
    for win in FP8_WINS + [200]:
        _gpu_probe(ops, nq, nk, d, diag, qs, win, f"{_geo_id(geo)} win{win}")
    _print_worst()


@pytest.mark.gpu
@pytest.mark.parametrize("h,hk", [(2, 2), (4, 2)])
@pytest.mark.parametrize("d", [64, 128])
def test_gpu_probe_walk_starts_past_tile_zero(d, h, hk):
    """diag 700, window 300 over 1024 keys: the only workgroup walks kv tiles
    [3, 8) (the header's own range, asserted here)."""
    nq, nk, diag, win = 256, 1024, 700, 300
    m = _ext().Mask(True, diag, 1, True, win)
    assert tuple(m.kv_tile_range(0, nq - 1, nk, fp8_kvblk())) == (3, 8)
    ops = _probe_operands(nq, nk, d, h, hk, "cuda")
    _gpu_probe(ops, nq, nk, d, diag, 1, win, "lo>0")
    _print_worst()


@pytest.mark.gpu
@pytest.mark.parametrize("h,hk", [(2, 2), (4, 2)])
@pytest.mark.parametrize("d", [64, 128])
def test_gpu_probe_paired_three_tiles_strict_diagonal(d, h, hk):
    """diag -1 at three q tiles: the PAIRED grid with the general mask runs
    tiles (0, 2) in one workgroup and the middle one alone."""
    n = 768
    ops = _probe_operands(n, n, d, h, hk, "cuda")
    _gpu_probe(ops, n, n, d, -1, 1, None, "paired diag-1")
    _print_worst()


# ---------------------------------------------------------------------------
# GPU: the masked model on gains
# ---------------------------------------------------------------------------
# (nq, nk, diag, q_stride, window)
EMU_CASES = [(256, 256, 0, 1, None), (256, 256, -1, 1, None),
             (256, 512, 256, 1, 100), (256, 1024, 700, 1, 300),
             (64, 256, 3, 4, None), (256, 256, -100, 1, None)]


@pytest.mark.gpu
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("case", EMU_CASES, ids=_geo_id)
def test_gpu_gains_against_the_masked_model(case, d):
    nq, nk, diag, qs, win = case
    h, hk = (4, 2) if nk <= 256 else (2, 2)
    q, k, v = (t.cuda() for t in build_inputs("gains", 1, nq, nk, h, hk, d,
                                              seed=nq + nk, kvblk=fp8_kvblk()))
    ops = quantize_fp8(q, k, v)
    sm = d ** -0.5
    out, lse = flash_attn_fp8_quantized(*ops, sm, causal=True, nk_true=nk, diag=diag,
                                        q_stride=qs, window=win)
    torch.cuda.synchronize()
    model = emulate_fp8_forward_masked(*ops, sm, True, nk, diag=diag, q_stride=qs,
                                       window=win)
    if diag == -100:
        assert model["dead_rows"][0, 0, :100].all() and not model["dead_rows"][0, 0, 100:nq].any()
    bad, f = masked_failures(out, lse, model)
    print(f"gains {_geo_id(case)} d{d}: err/mag {f['ratio']:.4g}  lse diff "
          f"{f['lse']:.3g}  dead rows {f['dead']}")
    _worst["gpu_out"] = max(_worst["gpu_out"], f["ratio"])
    _worst["gpu_lse"] = max(_worst["gpu_lse"], f["lse"])
    print("running worst: " + "  ".join(f"{k_} {v_:.4g}" for k_, v_ in _worst.items()))
    assert not bad, bad
