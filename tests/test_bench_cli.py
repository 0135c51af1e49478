"""bench.py command-line contract: the JSON result line carries ms_per_step,
--full is accepted, and --dump-outputs writes the last timed step's arrays as
float32 .npy files that are identical from run to run (seeded inputs)."""

import importlib.util
import json
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load_bench():
    spec = importlib.util.spec_from_file_location("bench", os.path.join(REPO, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _run(bench, monkeypatch, capsys, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    bench.main()
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


def test_dump_outputs_cpu_deterministic(tmp_path, monkeypatch, capsys):
    if torch.cuda.is_available():
        monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    bench = _load_bench()
    common = ("--gpus", "1", "--steps", "2", "--warmup", "1", "--seq-per-gpu", "128")
    a, b = tmp_path / "a", tmp_path / "b"
    rec = _run(bench, monkeypatch, capsys, *common, "--dump-outputs", str(a))
    _run(bench, monkeypatch, capsys, *common, "--full", "--dump-outputs", str(b))

    assert rec["metric"] == "attn_tflops" and rec["unit"] == "TFLOP/s"
    assert rec["higher_is_better"] is True
    assert rec["steps"] == 2 and rec["ms_per_step"] > 0

    assert sorted(os.listdir(a)) == ["dk.npy", "dq.npy", "dv.npy", "out.npy"]
    for name in os.listdir(a):
        x, y = np.load(a / name), np.load(b / name)
        assert x.dtype == np.float32 and x.shape == (1, 128, 8, 64)
        assert np.isfinite(x).all() and np.abs(x).max() > 0
        assert np.array_equal(x, y), name


def test_dump_outputs_samples_within_budget(tmp_path, monkeypatch):
    bench = _load_bench()
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 4000)   # 500 fp32 per array
    big = torch.arange(10000, dtype=torch.float32).reshape(100, 100)
    small = torch.ones(3, 5, dtype=torch.bfloat16)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"big": big, "small": small})
    xa, xb = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "b" / "big.npy")
    assert xa.shape == (500,) and xa.dtype == np.float32
    assert np.array_equal(xa, xb)                 # same seeded sample every run
    assert (np.diff(xa) >= 0).all() and len(np.unique(xa)) > 400   # spread, in order
    s = np.load(tmp_path / "a" / "small.npy")
    assert s.shape == (3, 5) and s.dtype == np.float32 and (s == 1).all()
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= 4000 + 2 * 128                # payload + two .npy headers


@pytest.mark.gpu
def test_dump_outputs_gpu_matches_oracle(tmp_path, monkeypatch, capsys):
    """The arrays dumped after hipGraph replays are the step's real results:
    compare with the fp32 oracle on the same seeded inputs (bounds as in
    test_gpu_kernels.test_fwd_bwd_parity)."""
    from ring_attention_amd.ops.ring_flash import ring_flash_attn_
    bench = _load_bench()
    n = 1024
    rec = _run(bench, monkeypatch, capsys, "--gpus", "1", "--steps", "3",
               "--warmup", "1", "--seq-per-gpu", str(n),
               "--dump-outputs", str(tmp_path))
    assert rec["dtype"] == "bf16" and rec["ms_per_step"] > 0
    assert rec["config"]["hipgraph"] is True

    torch.manual_seed(1234)                       # bench.py's rank-0 inputs
    q, k, v = (torch.randn(1, n, 8, 64, device="cuda", dtype=torch.bfloat16)
               for _ in range(3))
    qc, kc, vc = (t.float().cpu().requires_grad_(True) for t in (q, k, v))
    ref, _ = ring_flash_attn_(qc, kc, vc, causal=False, bucket_size=64)
    out = np.load(tmp_path / "out.npy")
    assert out.dtype == np.float32 and out.shape == (1, n, 8, 64)
    err = np.abs(out - ref.detach().numpy()).max()
    assert err < 2e-2, f"out err {err}"
    # bench.py feeds the (bf16) output back as the upstream gradient
    ref.backward(torch.from_numpy(out))
    for name, rt in (("dq", qc.grad), ("dk", kc.grad), ("dv", vc.grad)):
        g = np.load(tmp_path / f"{name}.npy")
        e = np.abs(g - rt.numpy()).max() / (rt.abs().max().item() + 1e-6)
        assert e < 4e-2, f"{name} rel err {e}"
