"""CPU: the fused vocabulary log-probability kernels (csrc/vocab_logprob.hip) compile for gfx950, in both builds, without scratch
memory or register spills (tests/test_kernel_resources.py says why that is a test), and each stays within the registers and the LDS
of its build (DESIGN.md "Fused vocabulary log-probabilities": the main kernel at 64 / 32 / 16 rows per tile takes 208 / 144 / 100
registers, 53 / 55 / 43 SGPRs and 3072 / 1536 / 768 bytes of static LDS beside the row tile's dynamic image; the merge 14 / 28 / 0)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "whisper.axera_amd", "csrc")

#            VGPRs, SGPRs, static LDS bytes: ceilings a step (8 registers) above what the build takes; the LDS is exact
CEILINGS = {"vocab_logprob_kernelILi4E": (216, 64, 3072), "vocab_logprob_kernelILi2E": (152, 64, 1536), "vocab_logprob_kernelILi1E": (108, 56, 768),
            "vocab_logprob_merge_kernel": (24, 32, 0)}


@pytest.mark.parametrize("f16", [0, 1], ids=["bf16", "fp16"])
def test_no_scratch_no_spills_and_ceilings(f16, tmp_path):
    out = tmp_path / "vocab_logprob.s"
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                        f"-DAXW_F16={f16}", "--cuda-device-only", "-S", "-o", str(out), os.path.join(CSRC, "vocab_logprob.hip")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    text = out.read_text()
    field = lambda k: [int(x) for x in re.findall(r"^\s+\." + k + r":\s+(\d+)", text, re.M)]
    names = re.findall(r"^\s+\.name:\s+(\S+)", text, re.M)
    short = [next(k for k in CEILINGS if k in n) for n in names]
    assert sorted(short) == sorted(CEILINGS)
    assert field("private_segment_fixed_size") == [0] * 4 and field("vgpr_spill_count") == [0] * 4 and field("sgpr_spill_count") == [0] * 4
    for i, k in enumerate(short):
        vg, sg, lds = CEILINGS[k]
        got = (field("vgpr_count")[i], field("sgpr_count")[i], field("group_segment_fixed_size")[i])
        assert got[0] <= vg and got[1] <= sg and got[2] == lds, (k, got)
    assert "v_mfma_f32_16x16x32" in text
