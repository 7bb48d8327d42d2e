"""CPU: the prompt-prefill kernels (csrc/decode_prefill.hip) compile for gfx950, in both builds, without scratch memory or register
spills (tests/test_kernel_resources.py says why that is a test), and the attention kernel stays within the registers and the LDS
DESIGN.md states for it."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "whisper.axera_amd", "csrc")


@pytest.mark.parametrize("f16", [0, 1], ids=["bf16", "fp16"])
def test_no_scratch_no_spills(f16, tmp_path):
    out = tmp_path / "decode_prefill.s"
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                        f"-DAXW_F16={f16}", "--cuda-device-only", "-S", "-o", str(out), os.path.join(CSRC, "decode_prefill.hip")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    text = out.read_text()
    field = lambda k: [int(x) for x in re.findall(r"^\s+\." + k + r":\s+(\d+)", text, re.M)]
    names = re.findall(r"^\s+\.name:\s+(\S+)", text, re.M)
    assert len(names) == 5 and sorted(n.split("prefill_")[1].split("_kernel")[0] for n in names) == ["attention", "cache_store", "embed", "gather_rows", "handover"]
    assert field("private_segment_fixed_size") == [0] * 5 and field("vgpr_spill_count") == [0] * 5 and field("sgpr_spill_count") == [0] * 5
    i = next(i for i, n in enumerate(names) if "attention" in n)
    assert field("vgpr_count")[i] <= 128 and field("group_segment_fixed_size")[i] == 9216  # 100 VGPRs, 9 KiB
    assert "v_mfma_f32_16x16x32" in text
