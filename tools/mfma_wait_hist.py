#!/usr/bin/env python3
"""Static MFMA / LDS-wait histogram of one function in gfx950 assembly.

    hipcc -O3 -std=c++17 --offload-arch=gfx950 --cuda-device-only -S \
        ring_attention_amd/csrc/attn_bwd.hip -o attn_bwd.s
    python tools/mfma_wait_hist.py attn_bwd.s dkv_kernelILi64ELi64ELb0ELb0ELb0

Given a .s file and a substring of a function label (mangled name), prints for
every matching function:

  * the MFMA count;
  * how many MFMAs sit directly behind an `s_waitcnt lgkmcnt(N)` (no other
    instruction in between), by N;
  * for every MFMA, how many instructions back the nearest ds_read is;
  * counts of scalar loads, v_readfirstlane, scratch ops, 64-bit v_cmp and
    saveexec, and whether the loop back-edges are scalar or exec-masked.

Pure text processing: needs no GPU and no ROCm install.
"""

import argparse
import collections
import re
import sys

LABEL = re.compile(r"^([A-Za-z_.$][\w.$]*):")
LGKM = re.compile(r"lgkmcnt\((\d+)\)")


def functions(lines):
    """{label: [instruction lines]} for every .type @function symbol."""
    funcs, name, body = {}, None, []
    is_func = set()
    for ln in lines:
        m = re.match(r"\s*\.type\s+([\w.$]+),@function", ln)
        if m:
            is_func.add(m.group(1))
    for ln in lines:
        m = LABEL.match(ln)
        if m and m.group(1) in is_func:
            name, body = m.group(1), []
            funcs[name] = body
            continue
        s = ln.strip()
        if name is None or not s:
            continue
        if s.startswith(".Lfunc_end") or s.startswith(".size"):
            name = None
            continue
        if s.startswith((".", ";")) and not LABEL.match(s):
            continue
        body.append(s.split(";")[0].strip())
    return funcs


def bucket(n):
    for hi in (0, 1, 2, 4, 8, 16, 32):
        if n <= hi:
            return f"<={hi}"
    return ">32"


def analyse(body):
    insts = [i for i in body if i and not LABEL.match(i)]
    op = lambda i: i.split()[0]
    n = collections.Counter()
    behind = collections.Counter()
    dist = collections.Counter()
    last_ds = None
    for k, i in enumerate(insts):
        o = op(i)
        if o.startswith("ds_read") or o.startswith("ds_load"):
            last_ds = k
            n["ds_read"] += 1
        elif o.startswith("v_mfma"):
            n["mfma"] += 1
            prev = insts[k - 1] if k else ""
            m = LGKM.search(prev) if op(prev or "x") == "s_waitcnt" else None
            behind[f"lgkmcnt({m.group(1)})" if m else "no wait"] += 1
            dist["none before" if last_ds is None else bucket(k - last_ds)] += 1
        elif o.startswith("s_load") or o.startswith("s_buffer_load"):
            n["s_load"] += 1
        elif o.startswith("v_readfirstlane"):
            n["v_readfirstlane"] += 1
        elif o.startswith("scratch_") or (o.startswith("buffer_") and " offen" in i and "s[0:3]" in i):
            n["scratch ops"] += 1
        elif o.startswith("v_cmp") and re.search(r"_[iuf]64", o):
            n["v_cmp 64-bit"] += 1
        elif "saveexec" in o:
            n["saveexec"] += 1
        elif o.startswith("flat_load"):
            n["flat_load"] += 1
        elif o == "s_barrier":
            n["s_barrier"] += 1
        elif o in ("v_pk_add_f32", "v_pk_mul_f32", "v_pk_fma_f32"):
            n["v_pk f32"] += 1
    # back-edges: a branch to a label defined earlier in the function
    seen, edges = set(), collections.Counter()
    for i in body:
        m = LABEL.match(i)
        if m:
            seen.add(m.group(1))
            continue
        parts = i.split()
        if parts and parts[0].startswith("s_cbranch") and parts[-1] in seen:
            edges[parts[0]] += 1
        elif parts and parts[0] == "s_branch" and parts[-1] in seen:
            edges["s_branch"] += 1
    return len(insts), n, behind, dist, edges


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("asm")
    ap.add_argument("name", help="substring of the function label")
    args = ap.parse_args()
    with open(args.asm) as f:
        funcs = functions(f.read().splitlines())
    hits = [k for k in funcs if args.name in k]
    if not hits:
        sys.exit(f"no function label contains {args.name!r}")
    for name in hits:
        total, n, behind, dist, edges = analyse(funcs[name])
        print(f"== {name}")
        print(f"instructions        {total}")
        print(f"MFMAs               {n['mfma']}")
        print("MFMA directly behind an s_waitcnt, by lgkmcnt:")
        for k in sorted(behind, key=lambda s: (s == "no wait", s)):
            print(f"    {k:<14}{behind[k]}")
        print("instructions from an MFMA back to the nearest ds_read:")
        for k in ("<=0", "<=1", "<=2", "<=4", "<=8", "<=16", "<=32", ">32", "none before"):
            if dist[k]:
                print(f"    {k:<14}{dist[k]}")
        for k in ("ds_read", "s_barrier", "s_load", "flat_load", "v_readfirstlane",
                  "scratch ops", "v_cmp 64-bit", "saveexec", "v_pk f32"):
            print(f"{k:<20}{n[k]}")
        print("loop back-edges     " +
              (", ".join(f"{k} x{v}" for k, v in sorted(edges.items())) or "none"))
        print()


if __name__ == "__main__":
    main()
