"""MX-FP8 forward under the mask geometry: timings on one GPU.

b 1, h 8, d 64 and 128, 8k and 32k tokens; one JSON line per case:

  a  the standard calls: non-causal, causal (diag 0)
  b  a striped ring hop: causal with diag 0 (the launch of a's causal call)
     and diag -1 (the PAIRED grid with the general mask, one key less per row)
  c  a windowed hop: diag = n, window = n / 2

    python tools/fp8_geometry_bench.py [--cases a,b,c] [--ext FILE]

--ext loads the extension from FILE instead of the in-tree build, to time
another build of the same interface in alternation (only case a's positional
call is understood by builds without the geometry arguments).  Times are
device-event times of a window of at least --window seconds after a warm-up;
TF counts 4 * d flops per attended (row, key) pair.
"""
import argparse
import importlib.util
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def load_ext(path):
    if path is None:
        from ring_attention_amd.ops import hip_ext
        return hip_ext.require()
    spec = importlib.util.spec_from_file_location(
        "ring_attention_amd._ring_attn_hip", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def attended_pairs(nq, nk, causal, diag=0, window=None):
    qpos = torch.arange(nq, dtype=torch.int64) + diag
    hi = torch.clamp(qpos, max=nk - 1) if causal else torch.full_like(qpos, nk - 1)
    lo = torch.zeros_like(qpos) if window is None else torch.clamp(qpos - window, min=0)
    return int(torch.clamp(hi - lo + 1, min=0).sum())


def time_call(fn, window_s):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(5):
        fn()
    end.record()
    torch.cuda.synchronize()
    per = start.elapsed_time(end) / 5 * 1e-3
    iters = max(20, int(window_s / max(per, 1e-6)))
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / iters * 1e3, iters       # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="a,b,c")
    ap.add_argument("--ext", default=None)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--label", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    ext = load_ext(args.ext)
    from ring_attention_amd.ops.fp8 import quantize_fp8
    cases = set(args.cases.split(","))
    b, h = 1, 8
    for d in (64, 128):
        for n in (8192, 32768):
            torch.manual_seed(0)
            q = torch.randn(b, n, h, d, device="cuda", dtype=torch.bfloat16)
            k, v = torch.randn_like(q), torch.randn_like(q)
            ops = quantize_fp8(q, k, v)
            sm = d ** -0.5
            runs = []
            if "a" in cases:
                runs += [("a_noncausal", lambda: ext.attn_fwd_fp8(*ops, sm, False, n),
                          attended_pairs(n, n, False)),
                         ("a_causal", lambda: ext.attn_fwd_fp8(*ops, sm, True, n),
                          attended_pairs(n, n, True))]
            if "b" in cases:
                runs += [("b_striped_diag0", lambda: ext.attn_fwd_fp8(
                              *ops, sm, True, n, diag=0),
                          attended_pairs(n, n, True)),
                         ("b_striped_diag-1", lambda: ext.attn_fwd_fp8(
                              *ops, sm, True, n, diag=-1),
                          attended_pairs(n, n, True, -1))]
            if "c" in cases:
                runs += [("c_window_hop", lambda: ext.attn_fwd_fp8(
                              *ops, sm, True, n, diag=n, has_win=True, win=n // 2),
                          attended_pairs(n, n, True, n, n // 2))]
            for name, fn, pairs in runs:
                us, iters = time_call(fn, args.window)
                rec = dict(case=name, d=d, n=n, b=b, h=h, us=round(us, 2),
                           tflops=round(4 * d * pairs * b * h / us / 1e6, 1),
                           iters=iters)
                if args.label:
                    rec["build"] = args.label
                print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
