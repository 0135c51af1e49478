"""Exact mask-boundary tests for the attention kernels.

Every kernel reduces masking to a few integers (diag, q_stride, win, nk) plus
a key-pad byte mask and turns them into a per-workgroup tile range, a
`full_tile` predicate and a per-element `ok`; the forward, dq, dkv and fp8
forward kernels take that arithmetic from csrc/attn_mask.h (checked here on
the CPU against a brute-force mask) and apply it under the grid.z splits,
PAIRED and the descriptor units.  The oracle comparisons on
randn data are too loose to see one key too many among a hundred, so this
file uses a COUNTING PROBE whose expected value depends only on which (i, j)
pairs attend:

    q[i] = e[i % half]            (columns [0, half), half = D // 2)
    k[j] = e[half + j % half]     (columns [half, D))   =>  q.k = 0 always
    v[j] = e[j % D]
    do[i][c] = w[c] * (1 + [c == i % D]),  w = +1 / -1 on even / odd c

Every unmasked score is exactly 0 (softclamp included), every value is one of
{0, +-1, +-2} (exact in bf16; 1 is exact in e4m3), so with A(i) the attended
set of row i (docs/KERNELS.md section 1: j < nk; causal j <= qpos(i); window
qpos(i) - j <= win; kmask[j]; qpos(i) = i * q_stride + diag), count = |A(i)|
and P = [j in A(i)] / count:

    lse = log(count), out = P v, dv = P^T do, dp = do v^T,
    delta = rowsum(P * dp), ds = P * (dp - delta),
    dq = scale * ds k, dk = scale * ds^T q

exp(lse) is the count, out * count the number of attended keys per residue
class mod D, dq / dk live in columns [half, D) / [0, half) sorted by residue
class, and within a class every term has the same sign.  The fp64 reference
is built here from a boolean mask, independent of ops/reference.py.

Checker (elementwise):  |exp(lse) - count| < 0.25 (one key off is 1.0; every
case keeps count <= 1024) and |got - ref| <= BOUND * mag for out, dq, dk, dv,
where mag is the same formula with absolute values (mag_out = out,
mag_dv = P^T |do|, mag_dq = scale * (P * (|dp| + |delta|)) |k|, dk alike);
where mag == 0 the result must be exactly 0.  Rows with count == 0 must give
out == 0, dq == 0, finite everything (lse finite with exp(lse) == 0) and no
contribution to dk / dv.

Bound in force: BOUND = 2**-6.
  * CPU emulation of the kernels' rounding points (out rounded to bf16 before
    delta, P and ds rounded to bf16 before the second GEMM, scale applied in
    fp32 afterwards, result rounded to bf16): worst err / mag 0.0073 over
    ~440 geometries, just under 2**-7; 2**-6 is twice that.
    test_probe_accepts_emulation_rejects_mutations re-measures it and shows
    that the checker rejects win +- 1, diag +- 1, a dropped last key, a single
    flipped (i, j) and a dropped 32x32 block at this bound.
    The sampled geometries of that test give 0.0066.
  * Measured on MI355X, worst over every GPU case of this file (each test
    prints its own figures and the running worst):
      forward (out)            err / mag 0.0039   |exp(lse) - count| 0.00062
      dq kernel (dq)           err / mag 0.0073
      dkv kernel (dk, dv)      err / mag 0.0071
      fp8 forward (out)        err / mag 0.0039   |exp(lse) - count| 0.00073
    All below 2**-7, so v_exp_f32 / __logf need no extra room and the bound
    stays at 2**-6.  No case failed: no mask copy is off by one.
"""

import functools

import pytest
import torch

BOUND = 2.0 ** -6           # err <= BOUND * mag (see module docstring)
COUNT_TOL = 0.25            # |exp(lse) - count|
MAX_COUNT = 1024            # fp32 log error stays far below COUNT_TOL
SOFTCLAMP_VALUE = 5.0

# (nq, nk, diag, q_stride): one full 256-row q tile plus a ragged one; 3.5 kv
# tiles of 128 keys / 7 of 64; a ragged last 256-key dkv workgroup;
# nk % 32 != 0; rows with no attendable key; the strided layout
GEOMS = [(448, 448, 0, 1), (448, 448, -1, 1), (192, 448, 256, 1),
         (320, 200, -130, 1), (112, 448, 3, 4)]
WINS = [None, 0, 1, 31, 32, 63, 64, 65, 127, 128, 129, 200]
NONCAUSAL = (320, 448, 0, 1)
# (nq, nk, diag, q_stride, causal): the probe cases of every GPU path
CASES = [g + (True,) for g in GEOMS] + [NONCAUSAL + (False,)]
DIMS = [32, 64, 128]


def _case_id(c):
    return "nq{}_nk{}_diag{}_qs{}_{}".format(*c[:4], "causal" if c[4] else "full")


def _wins_of(case, wins=WINS):
    """Windows run for a case: the causal ones take the list, the one
    non-causal case runs without a window."""
    return list(wins) if case[4] else [None]


# ---------------------------------------------------------------------------
# 1. the counting probe: inputs, fp64 reference, checker
# ---------------------------------------------------------------------------
def _attend(nq, nk, diag, q_stride, causal, win, kmask=None):
    """Boolean (nq, nk) attend matrix from the mask algebra."""
    qpos = (torch.arange(nq) * q_stride + diag)[:, None]
    j = torch.arange(nk)[None, :]
    a = torch.ones(nq, nk, dtype=torch.bool)
    if causal:
        a &= j <= qpos
    if win is not None:
        a &= (qpos - j) <= win
    if kmask is not None:
        a &= kmask[None, :].bool()
    return a


def _probe_slice(nq, nk, d):
    """fp64 q (nq, d), k, v (nk, d), do (nq, d) of one (b, h) slice."""
    half = d // 2
    i, j, c = torch.arange(nq), torch.arange(nk), torch.arange(d)
    q = torch.zeros(nq, d, dtype=torch.float64)
    k = torch.zeros(nk, d, dtype=torch.float64)
    v = torch.zeros(nk, d, dtype=torch.float64)
    q[i, i % half] = 1.0
    k[j, half + j % half] = 1.0
    v[j, j % d] = 1.0
    w = torch.where(c % 2 == 0, 1.0, -1.0).double()
    do = w[None, :] * (1.0 + (c[None, :] == (i % d)[:, None]).double())
    return q, k, v, do


def _reference(attend, d):
    """fp64 reference and magnitudes of one slice for an attend matrix."""
    nq, nk = attend.shape
    q, k, v, do = _probe_slice(nq, nk, d)
    scale = d ** -0.5
    a = attend.double()
    count = a.sum(-1)
    assert count.max().item() <= MAX_COUNT
    p = a / count.clamp(min=1.0)[:, None]
    dp = do @ v.T
    delta = (p * dp).sum(-1)
    ds = p * (dp - delta[:, None])
    pm = p * (dp.abs() + delta.abs()[:, None])
    out = p @ v
    return dict(count=count, out=out, mag_out=out,
                dv=p.T @ do, mag_dv=p.T @ do.abs(),
                dq=scale * (ds @ k), mag_dq=scale * (pm @ k.abs()),
                dk=scale * (ds.T @ q), mag_dk=scale * (pm.T @ q.abs()))


@functools.lru_cache(maxsize=16)
def _ref_cached(nq, nk, diag, q_stride, causal, win, d, mask_key=None):
    return _reference(_attend(nq, nk, diag, q_stride, causal, win,
                              _key_mask(nk, mask_key)), d)


def _key_mask(nk, key):
    """Fixed-seed key-pad masks: ~20% of the keys dropped; "mid" also blanks
    keys [128, 256) (a whole tile in the middle of a walk), "head" blanks
    [0, 128) (the first tile a row visits)."""
    if key is None:
        return None
    g = torch.Generator().manual_seed(20240607)
    m = torch.rand(nk, generator=g) >= 0.2
    if key == "mid":
        m[128:256] = False
    elif key == "head":
        m[0:128] = False
    else:
        assert key == "rand"
    return m


_WORST = {}          # kernel family -> worst err / mag seen in this process
_FAMILY = {"lse": "fwd", "out": "fwd", "dq": "dq", "dk": "dkv", "dv": "dkv"}


def _probe_failures(got, ref, group=1, bound=BOUND, tag="", family=None,
                    quiet=False, track=True):
    """Checks whichever of lse / out / dq / dk / dv `got` holds against the
    reference of one slice.  Tensors are (..., n) for lse and (..., n, d)
    otherwise and broadcast against the reference.  Returns the list of
    violations (empty = accepted)."""
    fails, ratios = [], {}
    dev = next(iter(got.values())).device
    count = ref["count"].to(dev)
    if "lse" in got:
        lse = got["lse"].double()
        if not torch.isfinite(lse).all():
            fails.append(f"{tag} lse: non-finite value")
        # rows with count == 0 included: their lse must be finite and act
        # as log(0), exp(lse) == 0 (docs/KERNELS.md section 1, "Mask edges")
        e = torch.nan_to_num((lse.exp() - count).abs(), nan=float("inf"))
        ratios["lse"] = e.max().item()
        bad = e >= COUNT_TOL
        for ix in bad.nonzero()[:4].tolist():
            fails.append(f"{tag} lse{ix}: exp(lse) = {lse[tuple(ix)].exp().item():.4f}, "
                         f"count = {count[ix[-1]].item():.0f}")
    for name in ("out", "dq", "dk", "dv"):
        if name not in got:
            continue
        gs = group if name in ("dk", "dv") else 1
        g = got[name].double()
        r = (ref[name].to(dev) * gs).expand_as(g)
        mag = (ref["mag_" + name].to(dev) * gs).expand_as(g)
        err = (g - r).abs()
        zero = mag == 0
        ratio = torch.where(zero, torch.zeros_like(err), err / mag.clamp(min=1e-300))
        ratio = torch.nan_to_num(ratio, nan=float("inf"))
        ratios[name] = ratio.max().item()
        bad = torch.where(zero, g != 0, ratio > bound) | ~torch.isfinite(g)
        for ix in bad.nonzero()[:4].tolist():
            t = tuple(ix)
            # class counts: out * count is the number of attended keys of the
            # residue class; the row is ix[-2] for out / dq
            cnt = count[ix[-2]].item() if name in ("out", "dq") else float("nan")
            fails.append(
                f"{tag} {name}{ix}: got {g[t].item():.6g}, ref {r[t].item():.6g}, "
                f"mag {mag[t].item():.6g}, row count {cnt:.0f} "
                f"(got * count {g[t].item() * cnt:.3f}, ref * count {r[t].item() * cnt:.3f})")
    for name, val in ratios.items() if track else ():
        fam = family or _FAMILY[name]
        if name == "lse":
            fam += " |exp(lse)-count|"
        _WORST[fam] = max(_WORST.get(fam, 0.0), val)
    if not quiet:
        print(f"{tag}: " + ", ".join(
            f"{n} {'|exp(lse)-count|' if n == 'lse' else 'err/mag'} {x:.4g}"
            for n, x in ratios.items()))
    return fails


def _assert_probe(got, ref, **kw):
    fails = _probe_failures(got, ref, **kw)
    assert not fails, "\n".join(fails[:12])


def _print_worst():
    print("worst err/mag so far: " + ", ".join(
        f"{fam} {val:.4g}" for fam, val in sorted(_WORST.items())))


# ---------------------------------------------------------------------------
# 2. CPU tests
# ---------------------------------------------------------------------------
def _bf16r(x):
    return x.to(torch.bfloat16).float()


def _emulate(att_fwd, att_bwd, d):
    """fp32 torch emulation of the kernels' rounding points for one slice;
    the forward masks with att_fwd, the backward kernels with att_bwd."""
    nq, nk = att_fwd.shape
    q, k, v, do = (t.float() for t in _probe_slice(nq, nk, d))
    scale = d ** -0.5
    cnt = att_fwd.float().sum(-1)
    l_safe = cnt.clamp(min=1e-38)
    out = _bf16r((att_fwd.float() @ v) / l_safe[:, None])   # p = exp2(0) = 1
    lse = l_safe.log()
    delta = (do * out).sum(-1)                              # out already bf16
    p = torch.where(att_bwd, (-lse).exp()[:, None].expand(nq, nk),
                    torch.zeros(nq, nk))
    dv = _bf16r(_bf16r(p).T @ do)
    ds = _bf16r(p * (do @ v.T - delta[:, None]))
    dq = _bf16r((ds @ k) * scale)
    dk = _bf16r((ds.T @ q) * scale)
    return dict(lse=lse, out=out, dq=dq, dk=dk, dv=dv)


def _mutations(geo, win, kmask, rng):
    """(label, attend) for every mutation class that changes the mask."""
    nq, nk, diag, qs, causal = geo
    true = _attend(nq, nk, diag, qs, causal, win, kmask)
    cand = []
    if win is not None:
        cand += [("win+1", _attend(nq, nk, diag, qs, causal, win + 1, kmask)),
                 ("win-1", _attend(nq, nk, diag, qs, causal, win - 1, kmask))]
    if causal or win is not None:
        cand += [("diag+1", _attend(nq, nk, diag + 1, qs, causal, win, kmask)),
                 ("diag-1", _attend(nq, nk, diag - 1, qs, causal, win, kmask))]
    last = true.clone()
    last[:, nk - 1] = False
    cand.append(("last key dropped", last))
    i = int(torch.randint(nq, (1,), generator=rng))
    j = int(torch.randint(nk, (1,), generator=rng))
    flip = true.clone()
    flip[i, j] = ~flip[i, j]
    cand.append((f"flip ({i}, {j})", flip))
    hit = true.nonzero()
    if len(hit):
        i, j = hit[int(torch.randint(len(hit), (1,), generator=rng))].tolist()
        i0, j0 = i // 32 * 32, j // 32 * 32
        block = true.clone()
        block[i0:i0 + 32, j0:j0 + 32] = False
        cand.append((f"block ({i0}, {j0}) dropped", block))
    return true, [(lab, a) for lab, a in cand if not torch.equal(a, true)]


def _dq_blind(true, att, d, ref):
    """True where a backward-only mask change leaves dq unchanged in exact
    arithmetic (a row with a single key has ds = 0: dropping that key, as
    win 0 -> -1 does, cannot show in dq; it shows in dv)."""
    nq, nk = true.shape
    _, k, v, do = _probe_slice(nq, nk, d)
    p = att.double() / ref["count"].clamp(min=1.0)[:, None]
    delta = (do * ref["out"]).sum(-1)
    dq = d ** -0.5 * ((p * (do @ v.T - delta[:, None])) @ k)
    return torch.allclose(dq, ref["dq"], rtol=0, atol=1e-12)


def test_probe_accepts_emulation_rejects_mutations():
    """The checker accepts the rounding emulation of a correct kernel and
    rejects every mutation class, so the GPU tests below can fail.  Each
    mutation is applied to the whole pipeline (forward and backward mask
    alike); the structured ones (win, diag, last key, block) are also applied
    to the backward alone, with the true forward's lse / out, and must then
    be rejected by dq alone and by dk / dv alone, because the dq and the dkv
    kernel each carry their own copy of the mask."""
    rng = torch.Generator().manual_seed(7)
    n_geo = n_mut = n_bwd = n_blind = 0
    for ci, case in enumerate(CASES):
        for di, d in enumerate(DIMS):
            wins = _wins_of(case)
            if len(wins) > 1:      # sample: every window appears for every
                wins = wins[(ci + di) % 3::3]      # geometry at some d
            for mask_key in (None, "rand"):
                if mask_key and (ci + di) % 2:
                    continue
                kmask = _key_mask(case[1], mask_key)
                for win in wins:
                    true, muts = _mutations(case, win, kmask, rng)
                    ref = _reference(true, d)
                    tag = f"{_case_id(case)} d{d} win{win} mask{mask_key}"
                    got = _emulate(true, true, d)
                    fails = _probe_failures(got, ref, tag=tag, family="emulation",
                                            quiet=True)
                    assert not fails, "\n".join(fails[:8])
                    n_geo += 1
                    for lab, att in muts:
                        bad = _emulate(att, att, d)
                        assert _probe_failures(bad, ref, track=False, quiet=True), \
                            f"{tag}: mutation '{lab}' accepted"
                        n_mut += 1
                        if lab.startswith("flip"):
                            continue
                        # the dq and the dkv kernel each carry their own
                        # copy of the mask: either alone must be caught
                        bwd = _emulate(true, att, d)
                        for names in (("dq",), ("dk", "dv")):
                            if names == ("dq",) and _dq_blind(true, att, d, ref):
                                n_blind += 1
                                continue
                            assert _probe_failures({n: bwd[n] for n in names}, ref,
                                                   track=False, quiet=True), \
                                f"{tag}: backward-only mutation '{lab}' accepted by {names}"
                        n_bwd += 1
    worst = _WORST.pop("emulation")
    _WORST.pop("emulation |exp(lse)-count|")
    print(f"{n_geo} geometries accepted, worst emulated err/mag {worst:.4g} "
          f"(bound {BOUND:.4g}); {n_mut} mutated pipelines and {n_bwd} "
          f"backward-only mutations rejected ({n_blind} of them invisible to dq)")
    assert worst <= BOUND / 2          # the bound is twice the emulated worst case
    assert n_mut >= 500 and n_bwd >= 400 and n_blind <= n_bwd // 10


DESC_GEOMS = GEOMS + [(640, 640, 0, 1)]


@pytest.mark.parametrize("kind", ["dq", "dkv"])
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("geo", DESC_GEOMS, ids=lambda g: "x".join(map(str, g)))
def test_walk_descriptors_cover_the_walk(geo, d, kind):
    """The descriptor units cover every (owner tile, walked tile) pair that
    holds an attended (i, j) of the causal mask, none twice, and name no tile
    outside the tensors."""
    from ring_attention_amd.ops.ring_flash_hip import _walk_descriptors
    nq, nk, diag, qs = geo
    att = _attend(nq, nk, diag, qs, True, None)
    if kind == "dq":
        own, walk = 256, (128 if d == 64 else 64)       # DQ_KVBLK
    else:
        att = att.T
        own, walk = 256, 64                             # dkv QT
    n_own = -(-att.shape[0] // own)
    n_walk = -(-att.shape[1] // walk)
    needed = {(x, t) for x in range(n_own) for t in range(n_walk)
              if att[x * own:(x + 1) * own, t * walk:(t + 1) * walk].any()}
    for bh in (1, 2, 64, 4096):
        desc = _walk_descriptors(kind, d, nq, nk, diag, qs, bh, "cpu")
        covered = []
        if desc is not None:
            assert desc.dtype == torch.int32 and desc.dim() == 2 and desc.shape[1] == 3
            for x, lo, hi in desc.tolist():
                assert 0 <= x < n_own and 0 <= lo < hi <= n_walk, (x, lo, hi)
                covered += [(x, t) for t in range(lo, hi)]
        assert len(covered) == len(set(covered)), "a pair is covered twice"
        assert needed <= set(covered), sorted(needed - set(covered))[:8]


HEADER_CASES = [c + (w,) for c in CASES for w in _wins_of(c)]


@pytest.mark.parametrize("walk", ["dq64", "dq128", "dkv64"])
@pytest.mark.parametrize("case", HEADER_CASES,
                         ids=lambda c: _case_id(c) + "_win{}".format(c[5]))
def test_mask_header_against_brute_force(case, walk):
    """csrc/attn_mask.h, reached through the extension's host functions,
    against the brute-force mask: per owner tile (256 rows) of both walks
    (dq: q rows walk kv tiles of 64 / 128; dkv: kv rows walk q tiles of 64)
    the range covers every walked tile holding an attended pair, stays inside
    [0, n_tiles] with lo <= hi, "uncut" holds only for tiles whose every
    in-bounds pair attends, attends is the mask element for element, and the
    grid.z shares are contiguous, ordered, disjoint and union to the range."""
    ext = _ext()
    nq, nk, diag, qs, causal, win = case
    m = ext.Mask(causal, diag, qs, win is not None, 0 if win is None else win)
    att = _attend(nq, nk, diag, qs, causal, win)
    assert torch.equal(m.attends_matrix(nq, nk), att)
    assert m.attends(m.qpos(nq - 1), nk - 1) == bool(att[-1, -1])
    assert not m.attends(m.qpos(0), 0, False)      # the caller's own terms

    own, W = 256, int(walk.lstrip("dqkv"))
    shapes = ext.mask_tile_shapes(64 if W == 128 else 128)
    assert shapes["rows_wg"] == own and W in (shapes["kvblk"], shapes["dkv_qt"])
    if walk.startswith("dq"):
        tile_range = m.kv_tile_range
        uncut = lambda i0, i1, j0, j1: m.uncut(m.qpos(i0), m.qpos(i1), j0, j1)
    else:
        att = att.T
        tile_range = m.q_tile_range
        uncut = lambda j0, j1, i0, i1: m.uncut(m.qpos(i0), m.qpos(i1), j0, j1)
    n_own, n_walk = att.shape
    n_tiles = -(-n_walk // W)
    for x in range(-(-n_own // own)):
        o0, o1 = x * own, min((x + 1) * own, n_own) - 1
        lo, hi = tile_range(o0, o1, n_walk, W)
        assert 0 <= lo <= hi <= n_tiles, (x, lo, hi)
        for t in range(n_tiles):
            w0, w1 = t * W, min((t + 1) * W, n_walk) - 1
            blk = att[o0:o1 + 1, w0:w1 + 1]
            if blk.any():
                assert lo <= t < hi, (x, t, lo, hi)
            if uncut(o0, o1, w0, w1):
                assert blk.all(), (x, t)
        for splits in (1, 2, 3, 5):
            shares = [ext.mask_split_share(lo, hi, splits, z) for z in range(splits)]
            assert shares[0][0] == lo and shares[-1][1] == hi, (x, shares)
            for (a0, a1), (b0, b1) in zip(shares, shares[1:]):
                assert a0 <= a1 == b0 <= b1, (x, shares)


# ---------------------------------------------------------------------------
# 3. GPU probe cases
# ---------------------------------------------------------------------------
def _ext():
    from ring_attention_amd.ops import hip_ext
    return hip_ext.require()


def _gpu_inputs(nq, nk, d, b=1, h=2, hk=2):
    """bf16 probe tensors (b, n, h, d) on the GPU, every (b, h) alike."""
    q, k, v, do = _probe_slice(nq, nk, d)
    up = lambda t, heads: (t[None, :, None, :].expand(b, t.shape[0], heads, d)
                           .to(torch.bfloat16).contiguous().cuda())
    return up(q, h), up(k, hk), up(v, hk), up(do, h)


def _nan(*shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), device="cuda", dtype=dtype)


def _mask_args(geo, win, softclamp):
    nq, nk, diag, qs, causal = geo
    return (causal, diag, qs, win if win is not None else 0, win is not None,
            softclamp, SOFTCLAMP_VALUE)


def _fwd(q, k, v, geo, win, kmask=None, softclamp=False, kv_split=1):
    """One forward launch (kv_split > 1: partials + merge); out (b, h, n, d)
    view and lse (b, h, n)."""
    ext = _ext()
    b, nq, h, d = q.shape
    out = _nan(*q.shape, dtype=torch.bfloat16)
    lse = _nan(b, h, nq)
    args = (d ** -0.5,) + _mask_args(geo, win, softclamp) + (True, True)
    if kv_split == 1:
        ext.attn_fwd(q, k, v, kmask, None, None, None, out, lse, *args, 1, 0, None)
    else:
        o_part = _nan(kv_split, b, h, d, nq)
        m_part, l_part = _nan(kv_split, b, h, nq), _nan(kv_split, b, h, nq)
        ext.attn_fwd(q, k, v, kmask, o_part, m_part, l_part, None, None, *args,
                     kv_split, 0, None)
        ext.attn_fwd_merge(o_part, m_part, l_part, None, None, None, out, lse,
                           kv_split, b, h, d, nq, True, True)
    return out, lse


def _bwd(q, k, v, do, out, lse, geo, win, kmask=None, softclamp=False, split=1,
         fused=False, desc_dq=None, desc_dkv=None, which=0):
    """Backward through the binding; dq / dk / dv as (b, h, n, d) views.
    Plain stores land on NaN-filled buffers (an element the kernel skips is
    caught), atomic modes on zeroed ones."""
    ext = _ext()
    b, nq, h, d = q.shape
    nk, hk = k.shape[1], k.shape[2]
    delta = ext.attn_delta(do, out)
    tail = (d ** -0.5,) + _mask_args(geo, win, softclamp) + (False, split)
    res = {}
    if fused:
        dq, dk, dv = (_nan(*t.shape, dtype=torch.bfloat16) for t in (q, k, v))
        ext.attn_bwd(q, k, v, do, kmask, lse, delta, None, None, None, *tail,
                     0, None, None, dq_bf=dq, dk_bf=dk, dv_bf=dv)
        return dict(dq=dq.permute(0, 2, 1, 3), dk=dk.permute(0, 2, 1, 3),
                    dv=dv.permute(0, 2, 1, 3))
    mk = lambda atomic, *s: (torch.zeros(*s, device="cuda") if atomic else _nan(*s))
    dq = mk(split > 1 or desc_dq is not None, b, nq, h, d)
    dk = mk(split > 1 or desc_dkv is not None, b, hk, nk, d)
    dv = mk(split > 1 or desc_dkv is not None, b, hk, d, nk)
    if which in (0, 1):
        ext.attn_bwd(q, k, v, do, kmask, lse, delta, dq, dk, dv, *tail, 1,
                     desc_dq, None)
        res["dq"] = dq.permute(0, 2, 1, 3)
    if which in (0, 2):
        ext.attn_bwd(q, k, v, do, kmask, lse, delta, dq, dk, dv, *tail, 2,
                     None, desc_dkv)
        res["dk"], res["dv"] = dk, dv.permute(0, 1, 3, 2)
    return res


def _o4(out):
    return out.permute(0, 2, 1, 3)


def _kmask_gpu(nk, key, b=1):
    m = _key_mask(nk, key)
    return None if m is None else m.to(torch.uint8)[None].expand(b, nk).contiguous().cuda()


def _single_pass(case, d, win, mask_key=None, tag="", h=2, hk=2, softclamp=False):
    """fwd kv_split = 1; bwd split = 1 with fp32 outputs and again with the
    fused bf16 outputs."""
    nq, nk = case[0], case[1]
    ref = _ref_cached(*case, win, d, mask_key)
    q, k, v, do = _gpu_inputs(nq, nk, d, h=h, hk=hk)
    kmask = _kmask_gpu(nk, mask_key)
    out, lse = _fwd(q, k, v, case, win, kmask, softclamp)
    _assert_probe(dict(lse=lse, out=_o4(out)), ref, tag=f"{tag} fwd")
    for fused in (False, True):
        grads = _bwd(q, k, v, do, out, lse, case, win, kmask, softclamp, fused=fused)
        _assert_probe(grads, ref, group=h // hk,
                      tag=f"{tag} bwd {'bf16' if fused else 'fp32'}")


@pytest.mark.gpu
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_single_pass(case, d):
    for win in _wins_of(case):
        _single_pass(case, d, win, tag=f"win{win}")
    _print_worst()


@pytest.mark.gpu
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("geo", [GEOMS[0], GEOMS[2]], ids=lambda g: "x".join(map(str, g)))
def test_key_pad_mask(geo, causal, d):
    case = geo + (causal,)
    for mask_key in ("rand", "mid", "head"):
        for win in (None, 1, 64, 129):
            _single_pass(case, d, win, mask_key, tag=f"mask-{mask_key} win{win}")
    _print_worst()


@pytest.mark.gpu
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_splits(case, d):
    """grid.z splits: fwd kv_split + merge, bwd split with fp32 atomics; the
    narrow windows leave some z with an empty share."""
    nq, nk = case[0], case[1]
    q, k, v, do = _gpu_inputs(nq, nk, d)
    for win in _wins_of(case, (None, 0, 64, 200)):
        ref = _ref_cached(*case, win, d)
        for z in (2, 4):
            out, lse = _fwd(q, k, v, case, win, kv_split=z)
            _assert_probe(dict(lse=lse, out=_o4(out)), ref, tag=f"win{win} kv_split{z}")
            grads = _bwd(q, k, v, do, out, lse, case, win, split=z)
            _assert_probe(grads, ref, tag=f"win{win} split{z}")
    _print_worst()


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_gqa(case):
    d, h, hk = 64, 4, 2
    nq, nk = case[0], case[1]
    q, k, v, do = _gpu_inputs(nq, nk, d, h=h, hk=hk)
    for win in _wins_of(case, (None, 63, 128)):
        _single_pass(case, d, win, tag=f"gqa win{win}", h=h, hk=hk)
        ref = _ref_cached(*case, win, d)
        out, lse = _fwd(q, k, v, case, win, kv_split=2)
        _assert_probe(dict(lse=lse, out=_o4(out)), ref, tag=f"gqa win{win} kv_split2")
        grads = _bwd(q, k, v, do, out, lse, case, win, split=2)
        _assert_probe(grads, ref, group=h // hk, tag=f"gqa win{win} split2")
    _print_worst()


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_softclamp(case):
    # scores are 0: tanh(0) = 0, dtanh = 1, the reference is unchanged
    for win in _wins_of(case, (None, 64)):
        _single_pass(case, 64, win, tag=f"softclamp win{win}", softclamp=True)
    _print_worst()


@pytest.mark.gpu
@pytest.mark.parametrize("kv_split", [1, 2])
@pytest.mark.parametrize("d", [64, 128])
def test_resume_across_hops(d, kv_split):
    """Three key shards visited as [256, 448), [0, 128), [128, 256): each hop
    uses diag - start and the same win; the first hop leaves rows < 256 with
    nothing attended.  dq accumulates over the hops, dk / dv run per shard."""
    ext = _ext()
    case = GEOMS[0] + (True,)
    nq, nk, diag, qs, causal = case
    b, h = 1, 2
    q, k, v, do = _gpu_inputs(nq, nk, d)
    shards = [(256, 448), (0, 128), (128, 256)]
    scale = d ** -0.5
    for win in (None, 129):
        ref = _ref_cached(*case, win, d)
        out = _nan(*q.shape, dtype=torch.bfloat16)
        lse = _nan(b, h, nq)
        o_acc, m, l = _nan(b, h, d, nq), _nan(b, h, nq), _nan(b, h, nq)
        for hop, (s, e) in enumerate(shards):
            ks, vs = k[:, s:e].contiguous(), v[:, s:e].contiguous()
            geo = (nq, e - s, diag - s, qs, causal)
            first, last = hop == 0, hop == len(shards) - 1
            args = (scale,) + _mask_args(geo, win, False) + (first, last)
            if kv_split == 1:
                ext.attn_fwd(q, ks, vs, None, o_acc, m, l, out, lse, *args, 1, 0, None)
            else:
                o_part = _nan(kv_split, b, h, d, nq)
                m_part, l_part = _nan(kv_split, b, h, nq), _nan(kv_split, b, h, nq)
                ext.attn_fwd(q, ks, vs, None, o_part, m_part, l_part, None, None,
                             *args, kv_split, 0, None)
                ext.attn_fwd_merge(o_part, m_part, l_part, o_acc, m, l,
                                   out if last else None, lse if last else None,
                                   kv_split, b, h, d, nq, first, last)
        tag = f"hops win{win} kv_split{kv_split}"
        _assert_probe(dict(lse=lse, out=_o4(out)), ref, tag=tag + " fwd")
        if kv_split > 1:
            continue            # the backward does not depend on kv_split
        delta = ext.attn_delta(do, out)
        dq = _nan(b, nq, h, d)
        dk, dv = _nan(b, h, nk, d), _nan(b, h, nk, d)
        for hop, (s, e) in enumerate(shards):
            ks, vs = k[:, s:e].contiguous(), v[:, s:e].contiguous()
            geo = (nq, e - s, diag - s, qs, causal)
            dk_s, dv_s = _nan(b, h, e - s, d), _nan(b, h, d, e - s)
            tail = (scale,) + _mask_args(geo, win, False)
            ext.attn_bwd(q, ks, vs, do, None, lse, delta, dq, None, None, *tail,
                         hop > 0, 1, 1, None, None)
            ext.attn_bwd(q, ks, vs, do, None, lse, delta, None, dk_s, dv_s, *tail,
                         False, 1, 2, None, None)
            dk[:, :, s:e] = dk_s
            dv[:, :, s:e] = dv_s.permute(0, 1, 3, 2)
        _assert_probe(dict(dq=dq.permute(0, 2, 1, 3), dk=dk, dv=dv), ref,
                      tag=tag + " bwd")
    _print_worst()


def _autograd(fn, q, k, v, do):
    qg, kg, vg = (t.clone().requires_grad_(True) for t in (q, k, v))
    res = fn(qg, kg, vg)
    out, lse = res if isinstance(res, tuple) else (res, None)
    out.backward(do)
    torch.cuda.synchronize()
    got = dict(out=_o4(out.detach()), dq=_o4(qg.grad), dk=_o4(kg.grad), dv=_o4(vg.grad))
    if lse is not None:
        got["lse"] = lse.detach()
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("d", [64, 128])
def test_paired_odd_tile_count(monkeypatch, d):
    """Three q / kv tiles: the middle one is self-paired (n_pit == 1)."""
    from ring_attention_amd.ops.ring_flash_hip import ring_flash_attn_hip_
    n, b, h = 640, 8, 16
    tiles = -(-n // 256)
    assert tiles == 3 and -(-tiles // 2) * b * h == 256   # the binding's PAIRED gate
    for key, val in {"RING_ATTN_SPLIT_DQ": "1", "RING_ATTN_SPLIT_DKV": "1",
                     "RING_ATTN_NO_DESC": "1", "RING_ATTN_KV_SPLIT": "1"}.items():
        monkeypatch.setenv(key, val)
    case = (n, n, 0, 1, True)
    q, k, v, do = _gpu_inputs(n, n, d, b=b, h=h, hk=h)
    for mask_key, no_pair in ((None, False), ("rand", False), (None, True)):
        if no_pair:
            monkeypatch.setenv("RING_ATTN_NO_PAIR", "1")
        ref = _ref_cached(*case, None, d, mask_key)
        mask = None if mask_key is None else _kmask_gpu(n, mask_key, b).bool()
        fn = lambda q_, k_, v_: ring_flash_attn_hip_(q_, k_, v_, mask=mask, causal=True)
        _assert_probe(_autograd(fn, q, k, v, do), ref,
                      tag=f"paired mask-{mask_key} no_pair={no_pair}")
    _print_worst()


@pytest.mark.gpu
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("geo", GEOMS, ids=lambda g: "x".join(map(str, g)))
def test_descriptor_units(geo, d):
    """desc_dq / desc_dkv of the binding on the causal no-window walks."""
    from ring_attention_amd.ops.ring_flash_hip import _walk_descriptors
    case = geo + (True,)
    nq, nk, diag, qs, _ = case
    assert diag < nk
    ref = _ref_cached(*case, None, d)
    q, k, v, do = _gpu_inputs(nq, nk, d)
    out, lse = _fwd(q, k, v, case, None)
    for bh in (2, 64):
        ddq = _walk_descriptors("dq", d, nq, nk, diag, qs, bh, q.device)
        ddkv = _walk_descriptors("dkv", d, nq, nk, diag, qs, bh, q.device)
        assert ddq is not None and ddkv is not None
        grads = _bwd(q, k, v, do, out, lse, case, None, desc_dq=ddq, desc_dkv=ddkv)
        _assert_probe(grads, ref, tag=f"desc bh{bh}")
    _print_worst()


@pytest.mark.gpu
@pytest.mark.parametrize("d", DIMS)
def test_probe_rejects_shifted_launch(d):
    """The GPU harness can fail on the real kernels: a launch whose window or
    diagonal is one off is rejected against the unshifted reference, by the
    forward outputs, and (true forward, shifted backward) by dq alone and by
    dk / dv alone."""
    case = GEOMS[0] + (True,)
    nq, nk, diag, qs, causal = case
    q, k, v, do = _gpu_inputs(nq, nk, d)
    for win in (None, 64, 200):
        ref = _ref_cached(*case, win, d)
        out, lse = _fwd(q, k, v, case, win)
        shifted = [((nq, nk, diag + s, qs, causal), win) for s in (1, -1)]
        if win is not None:
            shifted += [(case, win + s) for s in (1, -1)]
        for bad_case, bad_win in shifted:
            tag = f"diag{bad_case[2]} win{bad_win} for diag{diag} win{win}"
            o2, l2 = _fwd(q, k, v, bad_case, bad_win)
            for got in (dict(lse=l2), dict(out=_o4(o2))):
                assert _probe_failures(got, ref, track=False, quiet=True), tag
            grads = _bwd(q, k, v, do, out, lse, bad_case, bad_win)
            for names in (("dq",), ("dk", "dv")):
                assert _probe_failures({n: grads[n] for n in names}, ref,
                                       track=False, quiet=True), f"{tag}: {names}"


@pytest.mark.gpu
def test_public_wrappers():
    from ring_attention_amd.ops.ring_flash_hip import (
        flash_attn, flash_attn_offset, ring_flash_attn_hip_)
    d = 64
    nq, nk = 448, 448
    q, k, v, do = _gpu_inputs(nq, nk, d)
    kpm = _kmask_gpu(nk, "rand").bool()
    for w in (0, 1, 64, 129):
        ref = _ref_cached(nq, nk, 0, 1, True, w, d, "rand")
        fn = lambda q_, k_, v_: flash_attn(q_, k_, v_, key_pad_mask=kpm,
                                           causal=True, window=w)
        _assert_probe(_autograd(fn, q, k, v, do), ref, tag=f"flash_attn window{w}")
        ref = _ref_cached(nq, nk, 0, 1, True, w, d)
        fn = lambda q_, k_, v_: ring_flash_attn_hip_(q_, k_, v_, causal=True,
                                                     max_lookback_seq_len=w)
        _assert_probe(_autograd(fn, q, k, v, do), ref, tag=f"ring lookback{w}")
    ref = _ref_cached(nq, nk, -1, 1, True, 64, d)
    fn = lambda q_, k_, v_: flash_attn(q_, k_, v_, causal=True,
                                       causal_mask_diagonal=True, window=64)
    _assert_probe(_autograd(fn, q, k, v, do), ref, tag="flash_attn strict diagonal")
    q, k, v, do = _gpu_inputs(192, 448, d)
    ref = _ref_cached(192, 448, 256, 1, True, None, d)
    fn = lambda q_, k_, v_: flash_attn_offset(q_, k_, v_, q_offset=256)
    _assert_probe(_autograd(fn, q, k, v, do), ref, tag="flash_attn_offset")
    _print_worst()


@pytest.mark.gpu
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("h,hk", [(2, 2), (4, 2)])
@pytest.mark.parametrize("nq,nk,causal", [
    (300, 300, True), (300, 300, False), (448, 448, True), (448, 448, False),
    (777, 777, True), (777, 777, False), (256, 1000, False)])
def test_fp8_forward(nq, nk, causal, h, hk, d):
    """q = 0 makes every score 0 whatever k holds; P = 1 and V = 1 are exact
    in e4m3, so quantisation adds nothing and the counts are exact."""
    from ring_attention_amd.ops.fp8 import flash_attn_fp8
    _, _, v, _ = _gpu_inputs(nq, nk, d, h=h, hk=hk)
    g = torch.Generator(device="cuda").manual_seed(11)
    q = torch.zeros(1, nq, h, d, device="cuda", dtype=torch.bfloat16)
    k = torch.randn(1, nk, hk, d, device="cuda", dtype=torch.bfloat16, generator=g)
    ref = _ref_cached(nq, nk, 0, 1, causal, None, d)
    out, lse = flash_attn_fp8(q, k, v, causal=causal)
    _assert_probe(dict(lse=lse, out=_o4(out)), ref, tag="fp8", family="fwd_fp8")
    _print_worst()


# ---------------------------------------------------------------------------
# 4. window backward on random data (online-softmax rescale, real ds values)
# ---------------------------------------------------------------------------
OUT_TOL = 2e-2          # tests/test_valu_diet.py: out, absolute
LSE_TOL = 2e-3          # lse, absolute
GRAD_TOL = 4e-2         # gradients, of the reference's max


def _check_abs(name, got, ref, tol, relative):
    e = (got.float() - ref).abs().max().item()
    bound = tol * (ref.abs().max().item() + 1e-6 if relative else 1.0)
    print(f"{name}: max abs err {e:.4g} (bound {bound:.4g})")
    assert torch.isfinite(got.float()).all(), name
    assert e < bound, f"{name} err {e} >= {bound}"


@pytest.mark.gpu
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("geo", [GEOMS[0], GEOMS[4]], ids=lambda g: "x".join(map(str, g)))
def test_window_backward_random(geo, d):
    from ring_attention_amd.ops.reference import MASK_VALUE, default_attention
    nq, nk, diag, qs = geo
    h, hk = 4, 2
    case = geo + (True,)
    g = torch.Generator(device="cuda").manual_seed(nq + d)
    mk = lambda *s: torch.randn(*s, device="cuda", dtype=torch.bfloat16, generator=g)
    q, k, v, do = mk(1, nq, h, d), mk(1, nk, hk, d), mk(1, nk, hk, d), mk(1, nq, h, d)
    qpos = torch.arange(nq, device="cuda") * qs + diag
    jpos = torch.arange(nk, device="cuda")
    for win in (1, 31, 64, 129):
        qf, kf, vf = (t.float().requires_grad_(True) for t in (q, k, v))
        ref_out = default_attention(qf, kf, vf, causal=True, q_positions=qpos,
                                    max_lookback_seq_len=win)
        ref_out.backward(do.float())
        with torch.no_grad():       # lse of the same masked scores
            sim = torch.einsum("bihd,bjhd->bhij", qf, kf.repeat(1, 1, h // hk, 1)) * d ** -0.5
            cut = (jpos[None, :] > qpos[:, None]) | ((qpos[:, None] - jpos[None, :]) > win)
            ref_lse = sim.masked_fill(cut[None, None], MASK_VALUE).logsumexp(dim=-1)
        for z in (1, 2):
            tag = f"win{win} split{z} "
            out, lse = _fwd(q, k, v, case, win, kv_split=z)
            _check_abs(tag + "out", out, ref_out.detach(), OUT_TOL, relative=False)
            _check_abs(tag + "lse", lse, ref_lse, LSE_TOL, relative=False)
            gr = _bwd(q, k, v, do, out, lse, case, win, split=z)
            _check_abs(tag + "dq", gr["dq"], qf.grad.permute(0, 2, 1, 3), GRAD_TOL, True)
            _check_abs(tag + "dk", gr["dk"], kf.grad.permute(0, 2, 1, 3), GRAD_TOL, True)
            _check_abs(tag + "dv", gr["dv"], vf.grad.permute(0, 2, 1, 3), GRAD_TOL, True)
