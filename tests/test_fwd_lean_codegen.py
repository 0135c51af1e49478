"""Code-object metadata of the lean d64 plain forward kernels: no scratch and
no spilled VGPR.  Compiles attn_fwd.hip for gfx950 device-only into a
temporary directory; needs hipcc but no GPU."""

import os
import re
import shutil
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    "ring_attention_amd", "csrc")


def _hipcc():
    return shutil.which("hipcc") or (
        "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """{kernel name: {metadata field: value}} of attn_fwd.hip."""
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("hipcc not found")
    asm = tmp_path_factory.mktemp("fwd_lean") / "attn_fwd.s"
    subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950",
                    "--cuda-device-only", "-S", "-I", CSRC,
                    os.path.join(CSRC, "attn_fwd.hip"), "-o", str(asm)],
                   check=True, capture_output=True)
    out, cur = {}, None
    for ln in asm.read_text().splitlines():
        if re.match(r"  - \.", ln):              # next entry of amdhsa.kernels
            cur = {}
            ln = "    " + ln[4:]
        m = re.match(r"    \.(\w+):\s*(\S+)$", ln)
        if m and cur is not None:
            cur[m.group(1)] = m.group(2)
            if m.group(1) == "name":
                out[m.group(2)] = cur
    return out


@pytest.mark.parametrize("softclamp", [False, True])
def test_lean_d64_plain_has_no_scratch(kernels, softclamp):
    # attn_fwd_kernel<64, SOFTCLAMP, PAIRED = false, LEAN = true>
    tag = f"attn_fwd_kernelILi64ELb{int(softclamp)}ELb0ELb1E"
    hits = [v for k, v in kernels.items() if tag in k]
    assert len(hits) == 1, f"{len(hits)} kernels match {tag}"
    assert int(hits[0]["private_segment_fixed_size"]) == 0
    assert int(hits[0]["vgpr_spill_count"]) == 0
