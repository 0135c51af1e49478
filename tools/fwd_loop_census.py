#!/usr/bin/env python3
"""Instruction census of a function's tile loop in gfx950 assembly.

    hipcc -O3 -std=c++17 --offload-arch=gfx950 --cuda-device-only -S \
        -I ring_attention_amd/csrc ring_attention_amd/csrc/attn_fwd.hip -o attn_fwd.s
    python tools/fwd_loop_census.py attn_fwd.s attn_fwd_kernelILi64ELb0ELb0ELb1E
    python tools/fwd_loop_census.py attn_fwd.s --resources attn_fwd_kernel

The tile loop is the smallest span [label .. backward branch to that label]
that holds the most MFMAs of the function.  For every basic block of the span
(cut at labels and after branches) that holds an instruction, one line:

    MFMA, v_exp, other VALU, v_mov_b64, v_pk_* f32, vector scratch ops,
    v_readlane/v_writelane, ds_*, s_waitcnt, global/flat loads, all

followed by the totals over the span.  Blocks off the hot path (the masked
tile, the ragged load) are part of the span and are listed too: the hot path
is the blocks with MFMAs or v_exp plus the unpredicated staging block.
--hot lists only the blocks with an MFMA, a v_exp or at least 30 VALU ops
(the totals stay those of the whole span).

--resources prints, for every kernel whose name contains the substring, the
code-object metadata: VGPRs, SGPR and VGPR spill counts, scratch bytes per
lane and LDS bytes.

Pure text processing: needs no GPU and no ROCm install.
"""

import argparse
import collections
import re
import sys

from mfma_wait_hist import LABEL, functions

COLS = ("mfma", "v_exp", "valu", "v_mov_b64", "v_pk_f32", "scratch", "lane", "ds", "waitcnt",
        "vmem_ld", "all")
PK_F32 = ("v_pk_add_f32", "v_pk_mul_f32", "v_pk_fma_f32")


def classify(inst):
    o = inst.split()[0]
    if o.startswith("v_mfma"):
        return "mfma"
    if o.startswith("v_exp"):
        return "v_exp"
    if o.startswith("v_mov_b64"):
        return "v_mov_b64"
    if o in PK_F32:
        return "v_pk_f32"
    if o.startswith("scratch_") or (o.startswith("buffer_") and "s[0:3]" in inst):
        return "scratch"
    if o.startswith("v_readlane") or o.startswith("v_writelane"):
        return "lane"
    if o.startswith("ds_"):
        return "ds"
    if o == "s_waitcnt":
        return "waitcnt"
    if o.startswith("global_load") or o.startswith("flat_load"):
        return "vmem_ld"
    if o.startswith("v_"):
        return "valu"
    return None


def tile_loop(body):
    """(start, end) indices into body of the tile loop, or None."""
    where = {}
    best = None
    for k, i in enumerate(body):
        m = LABEL.match(i)
        if m:
            where[m.group(1)] = k
            continue
        parts = i.split()
        if parts and parts[0].startswith(("s_cbranch", "s_branch")) and parts[-1] in where:
            lo = where[parts[-1]]
            n = sum(1 for j in body[lo:k] if j.startswith("v_mfma"))
            if n and (best is None or (n, -(k - lo)) > (best[0], -(best[2] - best[1]))):
                best = (n, lo, k)
    return None if best is None else (best[1], best[2] + 1)


def census(body):
    span = tile_loop(body)
    if span is None:
        return []
    blocks, cur, name = [], collections.Counter(), "(entry)"
    for i in body[span[0]:span[1]]:
        m = LABEL.match(i)
        if m:
            if cur["all"]:
                blocks.append((name, cur))
            cur, name = collections.Counter(), m.group(1)
            continue
        cur["all"] += 1
        c = classify(i)
        if c:
            cur[c] += 1
        if i.split()[0].startswith(("s_cbranch", "s_branch")):
            blocks.append((name, cur))
            cur, name = collections.Counter(), name + "+"
    if cur["all"]:
        blocks.append((name, cur))
    return blocks


def resources(lines, sub):
    """Rows of (.name, {field: value}) from the .amdgpu_metadata kernels list."""
    rows, cur = [], None
    for ln in lines:
        if re.match(r"  - \.", ln):          # a new entry of amdhsa.kernels
            cur = {}
            rows.append(cur)
            ln = "    " + ln[4:]
        m = re.match(r"    \.(\w+):\s*(\S+)$", ln)
        if m and cur is not None:
            cur[m.group(1)] = m.group(2)
        elif not ln.startswith(" "):
            cur = None
    return [r for r in rows if "symbol" in r and sub in r.get("name", "")]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("asm")
    ap.add_argument("name", help="substring of the function label (or kernel name)")
    ap.add_argument("--hot", action="store_true",
                    help="list only blocks with an MFMA, a v_exp or >= 30 VALU ops")
    ap.add_argument("--resources", action="store_true",
                    help="print code-object metadata instead of the census")
    args = ap.parse_args()
    with open(args.asm) as f:
        lines = f.read().splitlines()
    if args.resources:
        for r in resources(lines, args.name):
            print(f"{r['name']}\tVGPRs: {r.get('vgpr_count')}"
                  f"\tSGPR spills: {r.get('sgpr_spill_count')}"
                  f"\tVGPR spills: {r.get('vgpr_spill_count')}"
                  f"\tScratch [bytes/lane]: {r.get('private_segment_fixed_size')}"
                  f"\tLDS [bytes/block]: {r.get('group_segment_fixed_size')}")
        return
    funcs = functions(lines)
    hits = [k for k in funcs if args.name in k and not k.endswith("$local")]
    if not hits:
        sys.exit(f"no function label contains {args.name!r}")
    for name in hits:
        blocks = census(funcs[name])
        print(f"== {name}")
        if not blocks:
            print("no loop with an MFMA\n")
            continue
        print(f"{'block':<14}" + "".join(f"{c:>10}" for c in COLS))
        tot = collections.Counter()
        for label, c in blocks:
            tot.update(c)
            if args.hot and not (c["mfma"] or c["v_exp"] or c["valu"] >= 30):
                continue
            print(f"{label[-13:]:<14}" + "".join(f"{c[k]:>10}" for k in COLS))
        print(f"{'loop total':<14}" + "".join(f"{tot[k]:>10}" for k in COLS))
        print()


if __name__ == "__main__":
    main()
