"""CPU: the ragged encoder self-attention kernels (csrc/encoder_attn_span.hip) compile for gfx950, in both builds and both block
heights, without scratch memory or register spills (tests/test_kernel_resources.py says why that is a test), with the parent kernel's
32 KB of LDS and registers for two workgroups per CU (DESIGN.md "Encoder spans")."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "whisper.axera_amd", "csrc")


@pytest.mark.parametrize("f16", [0, 1], ids=["bf16", "fp16"])
def test_no_scratch_no_spills(f16, tmp_path):
    out = tmp_path / "encoder_attn_span.s"
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                        f"-DAXW_F16={f16}", "--cuda-device-only", "-S", "-o", str(out), os.path.join(CSRC, "encoder_attn_span.hip")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    text = out.read_text()
    field = lambda k: [int(x) for x in re.findall(r"^\s+\." + k + r":\s+(\d+)", text, re.M)]
    names = re.findall(r"^\s+\.name:\s+(\S+)", text, re.M)
    assert sorted("ILi64E" in x for x in names) == [False, True] and all("encoder_attention_span_kernel" in x for x in names), names
    assert field("private_segment_fixed_size") == [0, 0] and field("vgpr_spill_count") == [0, 0] and field("sgpr_spill_count") == [0, 0]
    assert field("group_segment_fixed_size") == [32768, 32768]
    assert max(field("vgpr_count")) <= 256  # 4 waves per workgroup, one per SIMD: two workgroups per CU fit 512 registers per lane
